"""Training step of the acoustic model on MI355X (reference: model.py:167-226 loss + training_step,
:279-283 AdamW, train.py:66-76; the train=True data flow of layers/networks.py:336-434).

Every arithmetic operation of the step is a HIP kernel behind the C-ABI (`esmi_train_*`, csrc/train_ops.h and the train_*.h it includes): forward operators
that keep what their backward reads, data- and weight-gradient kernels, the fused masked loss, AdamW.  torch.autograd is used
as the TAPE only (which operator's backward runs when, and the accumulation of gradients that fan in); torch.distributed
(RCCL) carries the one gradient all-reduce.  Parameters and gradients of the model live in ONE flat fp32 buffer each
(`FlatParams`): the data-parallel exchange is a single all-reduce of 1.07 MB (tiny ES) and the optimizer a single launch.

The operators take the model's own `nn.Parameter`s in checkpoint layout, so `Phoneme2Mel.state_dict()` after N steps is a
reference-compatible checkpoint and the inference path (`networks.py`) picks the updated weights up through its pack cache.
"""
import contextlib
import ctypes as C
import dataclasses
import numbers

import torch

from . import _lib, networks
from .networks import _ptr, _mask_u8

ACT_RELU, ACT_GELU, ACT_TANH = 1, 2, 3
USE_MATRIX_PIPE = True    # dense convolutions (forward and data gradient) through the implicit-GEMM kernels; False: plain fp32 kernels


def _rt(t):
    return networks._runtime(t)


def _new(shape, like, dtype=torch.float32):
    return torch.empty(shape, dtype=dtype, device=like.device)


@dataclasses.dataclass
class _Step:
    """What a running `TrainStep` tells the operators; `TrainStep` turns the last three on as the step gets there (`_operators_in_step`, `_fwd_bwd`)."""
    precision: object               # 16: the reference's `--precision 16` -- the dense GEMMs (forward, data gradient) round their operands to
    #                                 binary16 (one MFMA product instead of three); "bf16": `--precision bf16-mixed`, the same in bfloat16
    loss_seed: object               # what the backward is seeded with: False = 1, else the device scalar (the loss scale) -- the loss kernel
    #                                 writes its gradients already multiplied by it and `_Loss.backward` passes them on as they are
    packed_valid: bool = False      # once the step's pack launch has been enqueued: `param._esmi_packed` holds this step's GEMM copies
    direct_grads: bool = False      # only around the backward: ONE backward per zeroed buffer, so overwriting == accumulating
    reduce_queue: object = None     # only around the backward: (esmi_reduce_queue, [workspaces kept alive]) -- the second stages of the chunked
    #                                 parameter-gradient reductions are queued and run as ONE launch before the optimizer (62 launches otherwise)


_STEP = None              # the `_Step` of the `TrainStep` whose step is running; None outside one: precision 32, fresh gradient tensors, nothing
#                           deferred, no packed copies, `_Loss.backward` scaling by the incoming seed.  A plain module variable on purpose, not a
#                           thread-local: on the GPU `total.backward()` runs the operators' `backward` on autograd's device thread


@contextlib.contextmanager
def _step_context(precision, loss_seed):
    global _STEP
    outer, _STEP = _STEP, _Step(precision, loss_seed)
    try:
        yield _STEP
    finally:
        _STEP = outer


def _defer(ws, *direct):
    """The queue to hand to an operator's backward, or None: only gradients that go straight into the flat buffer may be late
    (autograd would read a returned tensor at once); the partial sums in `ws` must outlive the flush."""
    q = _STEP.reduce_queue if _STEP is not None else None
    if q is None or not all(direct):
        return None
    q[1].append(ws)
    return C.byref(q[0])


def _grad_buffer(param):
    """Where an operator's backward writes a PARAMETER's gradient: straight into the flat gradient buffer when `FlatParams` owns
    the parameter AND a `TrainStep` is driving the step (then autograd gets None for it: no temporary, no accumulation launch),
    else a fresh tensor for autograd to accumulate -- so `training_step(...).backward()` called twice before an optimizer step
    (gradient accumulation through the wrapper's public route) adds up as torch semantics require.  The direct write is valid
    inside `TrainStep` because the buffer is zeroed per step and every parameter of this model feeds exactly one operator."""
    view = getattr(param, "_esmi_grad_view", None)
    direct = _STEP is not None and _STEP.direct_grads
    if direct and view is not None and param.grad is not None and param.grad.data_ptr() == view.data_ptr():   # still the buffer autograd would add to
        return view, True
    return torch.empty_like(param), False


# --------------------------------------------------------------------------- what _Conv, _LayerNorm and _ConvLN are made of
_DESC_PRECISION = {16: 16, "bf16": _lib.PRECISION_BF16}     # `_Step.precision` -> esmi_conv_desc.precision (everything else: fp32-accurate)


normalize_precision = _lib.normalize_precision     # (shared with inference: its home is _lib)


def _conv_desc(lib, x, w0, w, n_out, stride, pad, groups, transposed, act):
    """-> (d, ws, nws): the `ConvDesc` of a convolution of x (B, n_in, Cin) by the Parameter `w0` (`w`: contiguous) and what its forward
    GEMM copies the weight into -- this step's packed copies (made by TrainStep's one pack launch) in `d`, else the workspace `ws`."""
    B, n_in, c_in = x.shape
    w3 = w if w.dim() == 3 else w.unsqueeze(-1)
    c_out, k = (w3.shape[1] if transposed else w3.shape[0]), w3.shape[2]
    precision = _DESC_PRECISION.get(_STEP.precision, 0) if _STEP is not None else 0
    d = _lib.ConvDesc(B, n_in, c_in, n_out, c_out, k, stride, pad, groups, 1 if transposed else 0, precision, act)
    packed = getattr(w0, "_esmi_packed", None) if (USE_MATRIX_PIPE and _STEP is not None and _STEP.packed_valid) else None
    if packed is not None:
        d.packed_fwd, d.packed_grad = _ptr(packed[0]), _ptr(packed[1])
    nws = lib.esmi_train_conv_workspace_bytes(C.byref(d)) if (USE_MATRIX_PIPE and packed is None) else 0
    return d, (_new((nws,), x, torch.uint8) if nws else None), nws


def _conv_backward(lib, st, d, x, w, dy, w0, b0):
    """The convolution's two gradients -> (dx, dw, db); dw / db are None where the gradient went straight into the flat buffer of the
    Parameter (`w0`, `b0`: the Parameter objects themselves)."""
    dx = torch.empty_like(x)
    dw, w_direct = _grad_buffer(w0)
    db, b_direct = _grad_buffer(b0) if b0 is not None else (None, True)
    if USE_MATRIX_PIPE:
        # one call for both gradients: the weight-gradient pass leaves max|dy| behind for the data-gradient GEMM's operand scale
        nws = lib.esmi_train_conv_bwd_workspace_bytes(C.byref(d))
        ws = _new((nws,), w, torch.uint8)
        lib.esmi_train_conv_bwd_f32(C.byref(d), _ptr(x), _ptr(dy), _ptr(w), _ptr(dx), _ptr(dw), _ptr(db), _ptr(ws), nws,
                                    _defer(ws, w_direct, b_direct), st)
    else:
        lib.esmi_train_conv_dgrad_f32(C.byref(d), _ptr(dy), _ptr(w), _ptr(dx), None, 0, st)
        nws = lib.esmi_train_conv_wgrad_workspace_bytes(C.byref(d))
        ws = _new((nws,), w, torch.uint8)
        lib.esmi_train_conv_wgrad_f32(C.byref(d), _ptr(x), _ptr(dy), _ptr(dw), _ptr(db), _ptr(ws), nws, st)
    return dx, (None if w_direct else dw), (None if b_direct else db)


def _layer_norm_backward(lib, st, x, g, mean, rstd, mask, y_relu, dy, in_act, g0, b0):
    """The norm's backward (with the row mask, the norm's ReLU and the activation `in_act` in front of it) -> (dx, dg, db); dg / db are
    None where the gradient went straight into the flat buffer of the Parameter (`g0`, `b0`)."""
    rows, Cc = x.numel() // x.shape[-1], x.shape[-1]
    dx = torch.empty_like(x)
    (dg, g_direct), (db, b_direct) = _grad_buffer(g0), _grad_buffer(b0)
    nws = lib.esmi_train_layernorm_bwd_workspace_bytes(rows, Cc)
    ws = _new((nws,), x, torch.uint8)
    lib.esmi_train_layernorm_bwd_f32(_ptr(x), _ptr(g), _ptr(mean), _ptr(rstd), _ptr(dy), rows, Cc, _ptr(dx), _ptr(dg), _ptr(db),
                                     _ptr(ws), nws, _defer(ws, g_direct, b_direct), _ptr(mask), in_act, _ptr(y_relu), st)
    return dx, (None if g_direct else dg), (None if b_direct else db)


# --------------------------------------------------------------------------- operators (autograd = the tape)
class _Conv(torch.autograd.Function):
    """Conv1d / ConvTranspose1d / Linear on channels-last (B, n, C); `w` in checkpoint layout (Linear: (Cout, Cin))."""

    @staticmethod
    def forward(ctx, x, w, b, stride, pad, groups, transposed, n_out, act=0, act_grad_downstream=False):
        """act: ReLU / tanh applied to the result inside the convolution's launch (`esmi_conv_desc.act`); their derivatives come
        from the saved output, so the backward is act' then the convolution's -- unless the one consumer of the result takes care of
        act' in its own backward (`act_grad_downstream`: the LayerNorm that follows, `in_act`)."""
        assert act in (0, ACT_RELU, ACT_TANH)
        ctx.act_here = bool(act) and not act_grad_downstream
        w0 = w
        x, w = x.contiguous(), w.contiguous()
        lib, st = _rt(x)
        d, ws, nws = _conv_desc(lib, x, w0, w, n_out, stride, pad, groups, transposed, act)
        y = _new((d.B, n_out, d.c_out), x)
        lib.esmi_train_conv_fwd_f32(C.byref(d), _ptr(x), _ptr(w), _ptr(b), _ptr(y), _ptr(ws), nws, st)
        ctx.save_for_backward(x, w, *((y,) if ctx.act_here else ()))
        ctx.d, ctx.params = d, (w0, b)          # the Parameter objects themselves: their flat gradient views are the outputs
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors[:2]
        dy = dy.contiguous()
        lib, st = _rt(dy)
        if ctx.act_here:
            da = torch.empty_like(dy)
            lib.esmi_train_act_bwd_f32(_ptr(ctx.saved_tensors[2]), _ptr(dy), dy.numel(), ctx.d.act, _ptr(da), st)
            dy = da
        return _conv_backward(lib, st, ctx.d, x, w, dy, *ctx.params) + (None,) * 7


class _LayerNorm(torch.autograd.Function):
    """LayerNorm over the last dim -- optionally of x + res (both summands get the backward's dx) and with padded rows zeroed
    afterwards (`mask` (rows) uint8; those rows pass no gradient): the add and the masked_fill ride in the norm's launches.
    in_act: x is the output of that ReLU / tanh and has no other consumer -- the backward returns the gradient of the activation's
    INPUT, so the producer (`conv(..., act=kind, act_grad_downstream=True)`) must not apply the activation's backward again."""

    @staticmethod
    def forward(ctx, x, g, b, res=None, mask=None, in_act=0, relu_out=False):
        """relu_out: y = relu(LN(.)) in the same launch (networks.py:153-154); the backward gates dy with the saved output."""
        assert in_act in (0, ACT_RELU, ACT_TANH) and not (in_act and res is not None)
        x = x.contiguous()
        lib, st = _rt(x)
        rows, Cc = x.numel() // x.shape[-1], x.shape[-1]
        y, mean, rstd = torch.empty_like(x), _new((rows,), x), _new((rows,), x)
        xs = x
        if res is not None:
            res, xs = res.contiguous(), torch.empty_like(x)
        lib.esmi_train_layernorm_fwd_f32(_ptr(x), _ptr(g), _ptr(b), rows, Cc, _ptr(y), _ptr(mean), _ptr(rstd), _ptr(res),
                                         _ptr(xs) if res is not None else None, _ptr(mask), 1 if relu_out else 0, st)
        ctx.save_for_backward(xs, g, mean, rstd, mask, y if relu_out else None)
        ctx.params, ctx.has_res, ctx.in_act = (g, b), res is not None, in_act
        return y

    @staticmethod
    def backward(ctx, dy):
        dy = dy.contiguous()
        lib, st = _rt(dy)
        dx, dg, db = _layer_norm_backward(lib, st, *ctx.saved_tensors, dy, ctx.in_act, *ctx.params)
        return dx, dg, db, (dx if ctx.has_res else None), None, None, None


class _ConvLN(torch.autograd.Function):
    """conv (stride 1) / Linear, its activation, an optional residual add, LayerNorm, the norm's ReLU and row mask in ONE forward
    launch (`esmi_train_conv_ln_fwd_f32`: the norm in the GEMM's epilogue) -- the chain `layer_norm(conv(x, m, act, True), norm, res,
    mask, in_act=act, relu_out)` of two launches otherwise.  The backward is that chain's: the fused LayerNorm backward (which also
    runs the activation's), then the convolution's two gradients.  Shapes the fused launch does not take run the two forward launches
    here, so the saved tensors and the backward are the same either way."""

    @staticmethod
    def forward(ctx, x, w, b, pad, groups, act, g, beta, res, mask, relu_out):
        assert act in (0, ACT_RELU, ACT_TANH) and not (act and res is not None)
        w0 = w
        x, w = x.contiguous(), w.contiguous()
        lib, st = _rt(x)
        d, ws, nws = _conv_desc(lib, x, w0, w, x.shape[1], 1, pad, groups, False, act)
        rows, c_out = d.B * d.n_out, d.c_out
        y_pre, y, mean, rstd = _new((d.B, d.n_out, c_out), x), _new((d.B, d.n_out, c_out), x), _new((rows,), x), _new((rows,), x)
        if res is not None:
            res = res.contiguous()
        fused = False
        if USE_MATRIX_PIPE and groups == 1:
            try:
                lib.esmi_train_conv_ln_fwd_f32(C.byref(d), _ptr(x), _ptr(w), _ptr(b), _ptr(res), _ptr(g), _ptr(beta), _ptr(mask),
                                               1 if relu_out else 0, _ptr(y_pre), _ptr(y), _ptr(mean), _ptr(rstd), _ptr(ws), nws, st)
                fused = True
            except _lib.Unsupported:
                pass
        if not fused:                       # the two launches (conv into y, then the norm in place: it reads a row before it writes it)
            tmp = y if res is not None else y_pre
            lib.esmi_train_conv_fwd_f32(C.byref(d), _ptr(x), _ptr(w), _ptr(b), _ptr(tmp), _ptr(ws), nws, st)
            lib.esmi_train_layernorm_fwd_f32(_ptr(tmp), _ptr(g), _ptr(beta), rows, c_out, _ptr(y), _ptr(mean), _ptr(rstd),
                                             _ptr(res), _ptr(y_pre) if res is not None else None, _ptr(mask), 1 if relu_out else 0, st)
        ctx.save_for_backward(x, w, y_pre, g, mean, rstd, mask, y if relu_out else None)
        ctx.d, ctx.params, ctx.has_res = d, (w0, b, g, beta), res is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w, *norm_saved = ctx.saved_tensors
        dy = dy.contiguous()
        lib, st = _rt(dy)
        w0, b0, g0, beta0 = ctx.params
        dpre, dg, dbeta = _layer_norm_backward(lib, st, *norm_saved, dy, ctx.d.act, g0, beta0)
        dx, dw, db = _conv_backward(lib, st, ctx.d, x, w, dpre, w0, b0)
        return dx, dw, db, None, None, None, dg, dbeta, (dpre if ctx.has_res else None), None, None


class _Act(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, kind):
        x = x.contiguous()
        lib, st = _rt(x)
        y = torch.empty_like(x)
        lib.esmi_train_act_fwd_f32(_ptr(x), x.numel(), kind, _ptr(y), st)
        ctx.save_for_backward(x if kind == ACT_GELU else y)
        ctx.kind = kind
        return y

    @staticmethod
    def backward(ctx, dy):
        (saved,) = ctx.saved_tensors
        dy = dy.contiguous()
        lib, st = _rt(dy)
        dx = torch.empty_like(dy)
        lib.esmi_train_act_bwd_f32(_ptr(saved), _ptr(dy), dy.numel(), ctx.kind, _ptr(dx), st)
        return dx, None


class _AttnCore(torch.autograd.Function):
    """qkv (B, N, 3*h*C) as the qkv Linear leaves it -> softmax(q k^T / sqrt(C/h)) v, heads concatenated (B, N, h*C)."""

    @staticmethod
    def forward(ctx, qkv, h):
        qkv = qkv.contiguous()
        lib, st = _rt(qkv)
        B, N, w = qkv.shape
        Cc = w // (3 * h)
        P, out = _new((B, h, N, N), qkv), _new((B, N, h * Cc), qkv)
        lib.esmi_train_attention_fwd_f32(_ptr(qkv), B, N, Cc, h, _ptr(P), _ptr(out), st)
        ctx.save_for_backward(qkv, P)
        ctx.dims = (B, N, Cc, h)
        return out

    @staticmethod
    def backward(ctx, dctx):
        qkv, P = ctx.saved_tensors
        dctx = dctx.contiguous()
        lib, st = _rt(dctx)
        B, N, Cc, h = ctx.dims
        dS, dqkv = torch.empty_like(P), torch.empty_like(qkv)
        lib.esmi_train_attention_bwd_f32(_ptr(qkv), _ptr(P), _ptr(dctx), B, N, Cc, h, _ptr(dS), _ptr(dqkv), st)
        return dqkv, None


class _Embedding(torch.autograd.Function):
    @staticmethod
    def forward(ctx, ids, table, padding_idx):
        ids = ids.contiguous().to(torch.int32)
        lib, st = _rt(table)
        V, Cc = table.shape
        out = _new(tuple(ids.shape) + (Cc,), table)
        lib.esmi_train_embedding_fwd_f32(_ptr(ids), _ptr(table), ids.numel(), V, Cc, _ptr(out), st)
        ctx.save_for_backward(ids)
        ctx.dims, ctx.param = (V, Cc, padding_idx), table
        return out

    @staticmethod
    def backward(ctx, dy):
        (ids,) = ctx.saved_tensors
        dy = dy.contiguous()
        lib, st = _rt(dy)
        V, Cc, pad = ctx.dims
        dt, direct = _grad_buffer(ctx.param)
        nws = lib.esmi_train_embedding_bwd_workspace_bytes(ids.numel(), V, Cc)
        ws = _new((nws,), dy, torch.uint8)
        lib.esmi_train_embedding_bwd_f32(_ptr(ids), _ptr(dy), ids.numel(), V, Cc, pad, _ptr(dt), _ptr(ws), nws, _defer(ws, direct), st)
        return None, (None if direct else dt), None


class _MaskRows(torch.autograd.Function):
    """x.masked_fill(mask[..., None], 0) for a (B, n) uint8 mask."""

    @staticmethod
    def forward(ctx, x, mask_u8):
        x = x.contiguous()
        lib, st = _rt(x)
        y = torch.empty_like(x)
        lib.esmi_train_mask_rows_f32(_ptr(x), _ptr(mask_u8), x.numel() // x.shape[-1], x.shape[-1], _ptr(y), st)
        ctx.save_for_backward(mask_u8)
        return y

    @staticmethod
    def backward(ctx, dy):
        (mask_u8,) = ctx.saved_tensors
        dy = dy.contiguous()
        lib, st = _rt(dy)
        dx = torch.empty_like(dy)
        lib.esmi_train_mask_rows_f32(_ptr(dy), _ptr(mask_u8), dy.numel() // dy.shape[-1], dy.shape[-1], _ptr(dx), st)
        return dx, None


class _Add(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b):
        a, b = a.contiguous(), b.contiguous()
        lib, st = _rt(a)
        y = torch.empty_like(a)
        lib.esmi_train_add_f32(_ptr(a), _ptr(b), a.numel(), _ptr(y), st)
        return y

    @staticmethod
    def backward(ctx, dy):
        return dy, dy


class _Cat(torch.autograd.Function):
    """torch.cat(parts, dim=-1) in one launch; parts whose bit is set in `masked` are first zeroed on the rows of the (rows) uint8
    `mask` (x.masked_fill(mask[..., None], 0) in front of the cat), gradients likewise."""

    @staticmethod
    def _run(lib, st, parts, widths, rows, cat, mask, masked, backward):
        ptrs = (C.c_void_p * len(parts))(*[_ptr(p) for p in parts])
        lib.esmi_train_cat_f32(ptrs, (C.c_int * len(parts))(*widths), len(parts), rows, _ptr(cat), _ptr(mask), masked, backward, st)

    @staticmethod
    def forward(ctx, mask, masked, *parts):
        parts = [p.contiguous() for p in parts]
        lib, st = _rt(parts[0])
        widths = [p.shape[-1] for p in parts]
        rows, tot = parts[0].numel() // widths[0], sum(widths)
        y = _new(tuple(parts[0].shape[:-1]) + (tot,), parts[0])
        masked = masked if mask is not None else 0
        _Cat._run(lib, st, parts, widths, rows, y, mask, masked, 0)
        ctx.widths, ctx.masked = widths, masked
        ctx.save_for_backward(*((mask,) if masked else ()))
        return y

    @staticmethod
    def backward(ctx, dy):
        dy = dy.contiguous()
        lib, st = _rt(dy)
        rows = dy.numel() // dy.shape[-1]
        outs = [_new(tuple(dy.shape[:-1]) + (w,), dy) for w in ctx.widths]
        _Cat._run(lib, st, outs, ctx.widths, rows, dy, ctx.saved_tensors[0] if ctx.masked else None, ctx.masked, 1)
        return (None, None) + tuple(outs)


class _Repeat(torch.autograd.Function):
    """FeatureUpsampler: (B, T, C) -> (B, L, C) by the inclusive duration cumsum `cum` (B, T) int32."""

    @staticmethod
    def forward(ctx, feat, cum, L):
        feat = feat.contiguous()
        lib, st = _rt(feat)
        B, T, Cc = feat.shape
        out = _new((B, L, Cc), feat)
        lib.esmi_train_repeat_fwd_f32(_ptr(feat), _ptr(cum), B, T, Cc, L, _ptr(out), st)
        ctx.save_for_backward(cum)
        ctx.dims = (B, T, Cc, L)
        return out

    @staticmethod
    def backward(ctx, dout):
        (cum,) = ctx.saved_tensors
        dout = dout.contiguous()
        lib, st = _rt(dout)
        B, T, Cc, L = ctx.dims
        df = _new((B, T, Cc), dout)
        lib.esmi_train_repeat_bwd_f32(_ptr(dout), _ptr(cum), B, T, Cc, L, _ptr(df), st)
        return df, None, None


class _Loss(torch.autograd.Function):
    """model.py:167-216.  Returns (parts, total): the four means (mel L1, pitch MSE, energy MSE, log-duration MSE; reported, not
    differentiable -- the reference's `loss()` values are only ever logged) and the weighted total, whose backward hands the
    kernel's gradient seeds d total / d prediction to the four predictions, scaled by the incoming seed."""

    @staticmethod
    def forward(ctx, mel_pred, pitch_pred, energy_pred, dur_pred, mel, pitch, energy, dur, mel_mask, ph_mask):
        mel_pred, pitch_pred, energy_pred, dur_pred = (t.contiguous() for t in (mel_pred, pitch_pred, energy_pred, dur_pred))
        lib, st = _rt(mel_pred)
        B, L, nm = mel_pred.shape
        T = pitch_pred.shape[1]
        out = _new((5,), mel_pred)
        grads = [torch.empty_like(t) for t in (mel_pred, pitch_pred, energy_pred, dur_pred)]
        scratch = _new((_lib.TRAIN_LOSS_SCRATCH_FLOATS,), mel_pred)      # held until the call has been enqueued
        seed = _STEP.loss_seed if _STEP is not None else None      # None: unknown here (scaled in backward); False: 1; else the device scalar
        a = _lib.TrainLossArgs(_ptr(mel_pred), _ptr(mel), _ptr(pitch_pred), _ptr(pitch), _ptr(energy_pred), _ptr(energy),
                               _ptr(dur_pred), _ptr(dur), _ptr(mel_mask), _ptr(ph_mask), B, T, L, nm, _ptr(out),
                               *[_ptr(g) for g in grads], _ptr(scratch), _ptr(seed) if torch.is_tensor(seed) else None)
        lib.esmi_train_loss_f32(C.byref(a), st)
        ctx.save_for_backward(*grads)
        ctx.prescaled = seed is not None
        parts, total = out[:4], out[4]
        ctx.mark_non_differentiable(parts)
        return parts, total

    @staticmethod
    def backward(ctx, _dparts, dtotal):
        if ctx.prescaled:                          # TrainStep told the forward what this backward is seeded with
            return tuple(ctx.saved_tensors) + (None,) * 6
        return tuple(g * dtotal for g in ctx.saved_tensors) + (None,) * 6     # (seed 1 from `.backward()`: four scalings, exact)


def loss_vector(parts, total):
    """The 5-vector (mel, pitch, energy, duration, total) for reporting."""
    return torch.cat([parts.detach(), total.detach().reshape(1)])


def conv(x, m, n_out=None, act=0, act_grad_downstream=False):
    """Apply an nn.Conv1d / nn.ConvTranspose1d / nn.Linear parameter container to channels-last x (+ ReLU / tanh in the same launch)."""
    if isinstance(m, torch.nn.Linear):
        return _Conv.apply(x, m.weight, m.bias, 1, 0, 1, False, x.shape[1], act, act_grad_downstream)
    tr = isinstance(m, torch.nn.ConvTranspose1d)
    k, s, p = m.kernel_size[0], m.stride[0], m.padding[0]
    full = (x.shape[1] - 1) * s - 2 * p + k if tr else (x.shape[1] + 2 * p - k) // s + 1
    return _Conv.apply(x, m.weight, m.bias, s, p, m.groups, tr, full if n_out is None else min(full, n_out), act, act_grad_downstream)


def layer_norm(x, m, res=None, mask=None, in_act=0, relu_out=False):
    return _LayerNorm.apply(x, m.weight, m.bias, res, mask, in_act, relu_out)


FUSE_CONV_LN = False      # True: a convolution and the LayerNorm behind it are ONE forward launch (`_ConvLN`, esmi_train_conv_ln_fwd_f32).
#                           Measured on tiny ES at B = 128 (profiles/r05_probes/train_conv_ln_fusion.md): 194 -> 182 launches, but 3.14 -> 3.19 ms of
#                           kernels per step -- the norm in the GEMM's epilogue (two row reductions per row in the MFMA C layout, a second
#                           full-size store for the pre-norm tensor) costs more than the 15 us stand-alone norm it replaces: off by default


def conv_ln(x, m, norm, act=0, res=None, mask=None, relu_out=False):
    """layer_norm(conv(x, m, act, act_grad_downstream=True), norm, res, mask, in_act=act, relu_out); with FUSE_CONV_LN the norm rides in
    the convolution's launch (`_ConvLN`).  m: a Linear or a stride-1 Conv1d."""
    if not FUSE_CONV_LN:
        return layer_norm(conv(x, m, act=act, act_grad_downstream=bool(act)), norm, res=res, mask=mask, in_act=act, relu_out=relu_out)
    if isinstance(m, torch.nn.Linear):
        return _ConvLN.apply(x, m.weight, m.bias, 0, 1, act, norm.weight, norm.bias, res, mask, relu_out)
    assert not isinstance(m, torch.nn.ConvTranspose1d) and m.stride[0] == 1 and x.shape[1] + 2 * m.padding[0] - (m.kernel_size[0] - 1) == x.shape[1]
    return _ConvLN.apply(x, m.weight, m.bias, m.padding[0], m.groups, act, norm.weight, norm.bias, res, mask, relu_out)


def act(x, kind):
    return _Act.apply(x, kind)


# --------------------------------------------------------------------------- the train=True forward, operator by operator
def _pooled_mask(mask_u8, n, T, n_out):
    """blocks.py:51-57 for the pool factor the encoder derives (networks.py:71-72)."""
    pool = int(torch.round(torch.tensor([n / n_out])).item())
    if pool <= 1:
        return mask_u8
    lib, st = _rt(mask_u8)
    out = _new((mask_u8.shape[0], n_out), mask_u8, torch.uint8)
    lib.esmi_pool_mask_u8(_ptr(mask_u8), mask_u8.shape[0], T, pool, _ptr(out), n_out, st)
    return out


def encoder_forward(enc, phoneme, mask_u8):
    """Encoder.forward, networks.py:52-87."""
    x = _Embedding.apply(phoneme, enc.embed.weight, 0)
    T = x.shape[1]
    feats = []
    for merge3, merge1, attn, ffn, norm1, norm2 in enc.attn_blocks:
        x = conv(conv(x, merge3), merge1)
        m = _pooled_mask(mask_u8, T, T, x.shape[1]) if mask_u8 is not None else None
        # LN(attn(x) + x) and LN(ffn(x) + x), padded positions zeroed: the add, the norm and the mask ride in the last Linear's launch
        x = conv_ln(_AttnCore.apply(conv(x, attn.qkv), attn.num_heads), attn.proj, norm1, res=x, mask=m)
        x = conv_ln(act(conv(conv(x, ffn.mlp1), ffn.conv), ACT_GELU), ffn.mlp2, norm2, res=x, mask=m)
        feats.append(x)
    return feats


def fuse_forward(fuse, feats, mask_u8):
    """Fuse.forward, networks.py:196-219."""
    T = feats[0].shape[1]
    parts = []
    for f, (mlp, up) in zip(feats, fuse.mlps):
        x = conv(f, mlp)
        if isinstance(up, torch.nn.ConvTranspose1d):
            x = conv(x, up, n_out=T)
        parts.append(x)
    x = conv(_Cat.apply(None, 0, *parts), fuse.fuse)
    return _MaskRows.apply(x, mask_u8) if mask_u8 is not None else x


def predictor_forward(dec, fused):
    """AcousticDecoder.forward, networks.py:151-165 -> (pred (B, T, 1), features (B, T, dim))."""
    y = conv_ln(fused, dec.conv1[0], dec.norm1, act=ACT_RELU, relu_out=True)
    y = conv(y, dec.conv2[0], act=ACT_RELU)
    if dec.duration:
        return conv(y, dec.linear, act=ACT_RELU), layer_norm(y, dec.norm2)
    pred = conv(y, dec.linear)
    return pred, None


def _bucket_embedding(dec, target):
    """get_embedding with a target (networks.py:128-149): the table row of torch.bucketize(target, bins)."""
    bins = dec.pitch_bins if dec.pitch_bins is not None else dec.energy_bins
    emb = dec.pitch_embedding if dec.pitch_embedding is not None else dec.energy_embedding
    lib, st = _rt(target)
    t = target.contiguous().float()
    idx = _new(tuple(t.shape), t, torch.int32)
    scratch = _new(tuple(t.shape) + (emb.weight.shape[1],), t)
    lib.esmi_bucket_embedding_f32(_ptr(t), _ptr(bins), _ptr(emb.weight.detach()), t.numel(), emb.weight.shape[1], _ptr(scratch), _ptr(idx), st)
    return _Embedding.apply(idx, emb.weight, -1)


def decoder_forward(dec, features):
    """MelDecoder.forward, networks.py:291-304."""
    skip = conv_ln(features, dec.proj[0], dec.proj[2], act=ACT_TANH)
    for convs, skip_norm in dec.blocks:
        x = skip
        for seq, norm in convs:
            x = conv_ln(conv(x, seq[0]), seq[1], norm, act=ACT_TANH)
        skip = layer_norm(x, skip_norm, res=skip)
    return conv(skip, dec.mel_linear)


def train_forward(net, x, mask_mel=True):
    """Phoneme2Mel.forward(x, train=True), networks.py:336-434 -> dict(mel, pitch, energy, duration, mel_len)."""
    pe = net.encoder
    phoneme = x["phoneme"]
    B, T = phoneme.shape
    ph_mask = _mask_u8(x["phoneme_mask"]) if B > 1 else None
    feats = encoder_forward(pe.encoder, phoneme, ph_mask)
    fused = fuse_forward(pe.fuse, feats, ph_mask)
    pitch_pred, _ = predictor_forward(pe.pitch_decoder, fused)
    energy_pred, _ = predictor_forward(pe.energy_decoder, fused)
    dur_pred, dur_feat = predictor_forward(pe.duration_decoder, fused)
    pf, ef = _bucket_embedding(pe.pitch_decoder, x["pitch"]), _bucket_embedding(pe.energy_decoder, x["energy"])
    feat4 = _Cat.apply(ph_mask, 0b1110, fused, pf, ef, dur_feat)     # the three masked_fills (networks.py:366-368) inside the cat's launch
    # length regulator on the TARGET durations (masked, clamped at 0), padded to the batch's longest target mel
    lib, st = _rt(feat4)
    dur = x["duration"].to(torch.int32).contiguous()
    if ph_mask is not None:
        dur = dur.masked_fill(x["phoneme_mask"], 0)
    cum, mel_len, lmax = _new((B, T), feat4, torch.int32), _new((B,), feat4, torch.int32), _new((1,), feat4, torch.int32)
    lib.esmi_length_regulate_i32(_ptr(dur), B, T, _ptr(cum), _ptr(mel_len), _ptr(lmax), st)
    L = int(x["mel"].shape[1]) if "mel" in x else int(torch.max(x["mel_len"]).item())
    features = _Repeat.apply(feat4, cum, L)
    mel = decoder_forward(net.decoder, features)
    if ph_mask is not None and mask_mel:
        frames = torch.arange(L, device=mel.device)[None, :] >= mel_len[:, None]        # FeatureUpsampler's masks, one bit per frame
        mel = _MaskRows.apply(mel, _mask_u8(frames))
    return {"mel": mel, "pitch": pitch_pred, "energy": energy_pred, "duration": dur_pred, "mel_len": mel_len}


def training_loss(net, x, y):
    """training_step's forward + loss (model.py:212-216): returns (parts, total) -- the four reported means and the differentiable
    weighted total 10 mel + 2 pitch + 2 energy + duration."""
    xx = dict(x)
    xx.setdefault("mel", y["mel"])
    # (the masked_fill of the padded mel frames, networks.py:423-424, is skipped here: the loss leaves those frames out and
    #  gives them a zero gradient either way)
    out = train_forward(net, xx, mask_mel=False)
    B, T = x["phoneme"].shape
    ph_mask = _mask_u8(x["phoneme_mask"]) if x.get("phoneme_mask") is not None else None
    mel_mask = _mask_u8(x["mel_mask"]) if x.get("mel_mask") is not None else None
    f = lambda t: t.contiguous().float()      # noqa: E731
    return _Loss.apply(out["mel"], out["pitch"].reshape(B, T), out["energy"].reshape(B, T), out["duration"].reshape(B, T),
                       f(y["mel"]), f(x["pitch"]), f(x["energy"]), x["duration"].to(torch.int32).contiguous(), mel_mask, ph_mask)


# --------------------------------------------------------------------------- flat parameters, AdamW, data-parallel step
# parameters the train=True graph never reaches (their .grad stays None in the reference, so AdamW skips them): the pitch /
# energy predictors' norm2 feeds only `features`, which only the duration predictor returns (networks.py:160-165, 347-365)
_UNREACHED = ("encoder.pitch_decoder.norm2.", "encoder.energy_decoder.norm2.")


class FlatParams:
    """All trainable parameters of a module as views into one flat fp32 buffer, their gradients into another.  accumulate=True adds
    `acc`, the running sum of a window of micro-batch gradients (`TrainStep(accumulate_grad_batches=N)`); without it there is no such
    attribute.  ema=True adds `ema`, the exponential moving average of the weights (`TrainStep(ema_decay=d)`): a copy of `data` at
    construction, pad elements 0 like `data`'s (the update launch averages 0 with 0); without it there is no such attribute either."""

    def __init__(self, net, accumulate=False, ema=False):
        named = [(k, p) for k, p in net.named_parameters() if p.requires_grad and not k.startswith(_UNREACHED)]
        self.names = [k for k, _ in named]
        self.params = [p for _, p in named]
        self.slices, n = [], 0                      # each parameter's elements in the flat buffers
        for p in self.params:
            self.slices.append(slice(n, n + p.numel()))
            n = (n + p.numel() + 3) & ~3            # every tensor starts 16-byte aligned
        dev = named[0][1].device
        self.data = torch.zeros(n, dtype=torch.float32, device=dev)          # (pad elements stay 0 under AdamW: g = 0, p = 0)
        self.grad = torch.zeros(n, dtype=torch.float32, device=dev)
        self.m, self.v = torch.zeros_like(self.data), torch.zeros_like(self.data)
        if accumulate:
            self.acc = torch.zeros_like(self.grad)  # (pad elements stay 0 here too: the accumulate launch adds weight * 0)
        for p, sl in zip(self.params, self.slices):
            self.data[sl].copy_(p.detach().reshape(-1))
            p.data = self.data[sl].view(p.shape)
            p.grad = self.grad[sl].view(p.shape)
            p._esmi_grad_view = p.grad              # operators' backward passes write here directly (see _grad_buffer)
        if ema:
            self.ema = self.data.clone()            # ema_0: the weights at construction

    def zero_grad(self):
        self.grad.zero_()


# torch.amp.GradScaler.state_dict()'s keys (Lightning stores it next to the optimizer) and the slots of the scaler block that hold them
_SCALER_KEYS = (("scale", _lib.SCALER_SCALE), ("growth_factor", _lib.SCALER_GROWTH_FACTOR), ("backoff_factor", _lib.SCALER_BACKOFF_FACTOR),
                ("growth_interval", _lib.SCALER_GROWTH_INTERVAL), ("_growth_tracker", _lib.SCALER_CLEAN_STEPS))


class AdamWState:
    """What AdamW and the loss scaler keep besides the moments (`FlatParams.m`, `.v`), and the optimizer launch that reads it.

    Where the scalars live is decided here, once: `on_device` (graph replay, precision 16, gradient clipping) keeps the step counter as one int32 and
    the hyper block (`_lib.HYPER_*`: the caller's slot is the learning rate, the rest is the launch's own) in device memory, so that
    the step never waits for the host; otherwise the counter is a Python int and the scalars travel as arguments.  Either way there
    is ONE counter, and `t` reads and writes it: on the device a read is one device -> host copy and a write one `fill_`.

    Precision 16 adds torch.amp.GradScaler on the device: the scaler block (`_lib.SCALER_*`) and the slot that max|g| is reduced
    into.  Without them (`scaler is None`) the backward is seeded with the constant 1 and no step is skipped.

    `gradient_clip_val` (Lightning's Trainer knob, algorithm "norm") = torch.nn.utils.clip_grad_norm_(params, value, norm_type=2)
    between the scaler's unscale and the update, on the device: one more launch reduces the sum of squares of the flat gradient buffer
    and the optimizer launch's bookkeeping kernel turns it into the coefficient every gradient is multiplied by.  None or 0: off (not
    one launch, buffer or attribute differs from a state built without the keyword); inf: the norm is measured, nothing is clipped.
    `grad_norm` / `clip_coef` read the last launch's norm of the unscaled gradients and its coefficient.  At precision 16 an overflow
    still skips the step (the norm recorded is then not finite); at precision 32 / bf16 a non-finite norm makes the coefficient nan and
    poisons the update exactly as torch's clip + step would: no skip is invented there."""

    def __init__(self, dev, precision=32, graph=False, lr=1e-3, init_scale=65536.0, growth_factor=2.0, backoff_factor=0.5,
                 growth_interval=2000, gradient_clip_val=None):
        clip = float(gradient_clip_val or 0.0)
        if not clip >= 0.0:
            raise ValueError(f"gradient_clip_val must be None or >= 0, not {gradient_clip_val!r}")
        self.on_device = bool(graph) or precision == 16 or clip > 0.0
        self.scaler = self.absmax = self.hyper = None
        self.lr = lr                                # what `set_lr` recorded last: the host-scalar launch's argument
        self._count = 0                             # the step counter: this int, or (on_device) one int32 in device memory
        if self.on_device:
            self._count = torch.zeros(1, dtype=torch.int32, device=dev)
            self.hyper = torch.full((_lib.TRAIN_ADAMW_HYPER_FLOATS,), lr, dtype=torch.float32, device=dev)
            self._lr = self.hyper[_lib.HYPER_LR:_lib.HYPER_LR + 1]
        self.max_norm = clip if clip > 0.0 else None      # None: no clipping -- no reduction launch, no partial sums, the plain optimizer launch
        if self.max_norm is not None:
            self._sumsq = torch.zeros(_lib.TRAIN_GRAD_NORM_PARTIALS, dtype=torch.float64, device=dev)
            self.hyper[_lib.HYPER_GRAD_NORM], self.hyper[_lib.HYPER_CLIP_COEF] = 0.0, 1.0     # what a read-out before the first step gives
        if precision == 16:
            block = [0.0] * _lib.TRAIN_SCALER_FLOATS              # (clean steps in a row and skipped steps start at 0)
            block[_lib.SCALER_SCALE], block[_lib.SCALER_GROWTH_FACTOR] = init_scale, growth_factor
            block[_lib.SCALER_BACKOFF_FACTOR], block[_lib.SCALER_GROWTH_INTERVAL] = backoff_factor, growth_interval
            self.scaler = torch.tensor(block, dtype=torch.float32, device=dev)
            self.absmax = torch.zeros(1, dtype=torch.float32, device=dev)
        # what the backward is seeded with (GradScaler.scale(loss).backward()): the device-side scale, else the constant one
        self.loss_seed = (torch.ones(1, dtype=torch.float32, device=dev) if self.scaler is None
                          else self.scaler[_lib.SCALER_SCALE:_lib.SCALER_SCALE + 1])

    @property
    def t(self):
        return int(self._count.item()) if self.on_device else self._count

    @t.setter
    def t(self, v):
        if self.on_device:
            self._count.fill_(int(v))
        else:
            self._count = int(v)

    # read-outs of the scaler block (each is one small device -> host copy; the step itself never reads them)
    @property
    def scale(self):
        return 1.0 if self.scaler is None else float(self.scaler[_lib.SCALER_SCALE].item())

    @property
    def skipped(self):
        return 0 if self.scaler is None else int(self.scaler[_lib.SCALER_SKIPPED].item())

    def _need_scaler(self, what):
        if self.scaler is None:
            raise AttributeError(f"no {what}: this step has no loss scaler (only precision 16 has one)")
        return self.scaler

    @property
    def growth_interval(self):
        return int(self._need_scaler("growth_interval")[_lib.SCALER_GROWTH_INTERVAL].item())

    @growth_interval.setter
    def growth_interval(self, n):
        self._need_scaler("growth_interval")[_lib.SCALER_GROWTH_INTERVAL] = float(n)

    # read-outs of the last clipped launch (one small device -> host copy each, like `scale`)
    def _need_clip(self, what):
        if self.max_norm is None:
            raise AttributeError(f"no {what}: this step does not clip (gradient_clip_val is None or 0)")
        return self.hyper

    @property
    def grad_norm(self):
        """The 2-norm of the last launch's unscaled gradients, before clipping."""
        return float(self._need_clip("grad_norm")[_lib.HYPER_GRAD_NORM].item())

    @property
    def clip_coef(self):
        """min(1, gradient_clip_val / (grad_norm + 1e-6)) of the last launch: what its gradients were multiplied by."""
        return float(self._need_clip("clip_coef")[_lib.HYPER_CLIP_COEF].item())

    def scaler_state_dict(self):
        """torch.amp.GradScaler.state_dict() of the scaler block; None without one."""
        if self.scaler is None:
            return None
        block = self.scaler.cpu().tolist()
        sd = {key: block[slot] for key, slot in _SCALER_KEYS}
        sd.update(growth_interval=int(sd["growth_interval"]), _growth_tracker=int(sd["_growth_tracker"]))
        return sd

    def load_scaler_state_dict(self, sd):
        """... and back; without a scaler block a checkpoint's entry is ignored."""
        if self.scaler is not None and sd is not None:
            for key, slot in _SCALER_KEYS:
                self.scaler[slot] = float(sd[key])

    def set_lr(self, lr):
        """The learning rate of the launches that follow: kept here for the launch that takes it as an argument, and written to the hyper
        block for the one that reads it from device memory (outside a captured graph: before the replay)."""
        self.lr = lr
        if self.on_device:
            self._lr.fill_(lr)

    def launch(self, flat, betas, eps, weight_decay, grad=None):
        """One AdamW update of `flat` by its (already exchanged) gradients: `grad`, the buffer all three launches read -- None: `flat.grad`;
        a `TrainStep` that accumulates passes `flat.acc` on a window's boundary.  Which buffer is the only thing it selects."""
        f = flat
        g = f.grad if grad is None else grad
        lib, st = _rt(f.data)
        if self.scaler is not None:
            # GradScaler.step + .update on the device: max|g| of the (still scaled) gradients -- absmax's integer max orders inf and
            # nan above every finite magnitude -- decides inside the optimizer launch whether the update runs (on g / scale) or is
            # skipped with the scale backed off; nothing is read back.
            lib.esmi_absmax_f32(_ptr(g), g.numel(), _ptr(self.absmax), st)
        if self.max_norm is not None:
            # clip_grad_norm_ on the device: the buffer's sum of squares as per-workgroup partial sums; the optimizer launch adds them up,
            # divides the norm by the loss scale and folds the coefficient into the scale that every gradient is multiplied by
            lib.esmi_train_grad_sumsq_f32(_ptr(g), g.numel(), _ptr(self._sumsq), st)
        if self.on_device:                          # (the launch counts: a skipped step does not advance the counter)
            absmax, scaler = (None, None) if self.scaler is None else (_ptr(self.absmax), _ptr(self.scaler))
            args = (_ptr(f.data), _ptr(g), _ptr(f.m), _ptr(f.v), f.data.numel(), _ptr(self.hyper), betas[0], betas[1], eps,
                    weight_decay, _ptr(self._count), absmax, scaler)
            if self.max_norm is not None:
                lib.esmi_train_adamw_clip_f32(*args, _ptr(self._sumsq), self.max_norm, st)
            else:
                lib.esmi_train_adamw_graph_f32(*args, st)
        else:
            self._count += 1
            lib.esmi_train_adamw_f32(_ptr(f.data), _ptr(g), _ptr(f.m), _ptr(f.v), f.data.numel(), self.lr, betas[0], betas[1], eps,
                                     weight_decay, self._count, 1.0, st)


class WeightAverage:
    """The exponential moving average of the weights that `TrainStep(ema_decay=d)` keeps in `FlatParams.ema`: its decay, its two launches
    and its entry in a checkpoint.  `open` is set while `TrainStep.ema_weights()` has the weights and the average exchanged."""

    def __init__(self, flat, decay):
        self.flat, self.decay, self.open = flat, float(decay), False
        self.weight = 1.0 - self.decay              # 1 - d in double, rounded to fp32 once by the call

    def update(self, opt):
        """ema = lerp(ema, p, 1 - d), one launch directly behind the optimizer's (capturable).  Where the optimizer keeps its scalars on
        the device the launch reads the skip flag there: a skipped precision-16 step does not advance the average."""
        f = self.flat
        lib, st = _rt(f.data)
        lib.esmi_train_ema_update_f32(_ptr(f.ema), _ptr(f.data), f.data.numel(), self.weight, _ptr(opt.hyper) if opt.on_device else None, st)

    def exchange(self, packed):
        """The contents of `flat.data` and `flat.ema` change places, in one launch and in place; `packed` (the inference path's copies of
        the weights that just left) is invalidated."""
        f = self.flat
        lib, st = _rt(f.data)
        lib.esmi_train_swap_f32(_ptr(f.data), _ptr(f.ema), f.data.numel(), st)
        packed.invalidate()

    def weights(self, net):
        """The averaged weights as {'phoneme2mel.<key>': tensor}, cloned; what the flat buffer does not own is `net`'s."""
        f = self.flat
        avg = f.data if self.open else f.ema        # (inside ema_weights() the two are exchanged)
        sd = {"phoneme2mel." + k: v.detach().clone() for k, v in net.state_dict().items()}
        for k, p, sl in zip(f.names, f.params, f.slices):
            sd["phoneme2mel." + k] = avg[sl].view(p.shape).clone()
        return sd

    def entry(self, net):
        """The checkpoint's "ema" entry."""
        return {"decay": self.decay, "state_dict": self.weights(net)}

    def accept(self, entry):
        """-> `entry` (a checkpoint's "ema" entry, or None) once it is known to load: one kept with another decay is refused."""
        if entry is not None and float(entry["decay"]) != self.decay:
            raise RuntimeError(f"the checkpoint's average was kept with ema_decay {entry['decay']!r}, this step's is {self.decay!r}")
        return entry

    def load(self, entry):
        """Restart the average from the weights as they are, then take the entry's where there is one."""
        f = self.flat
        f.ema.copy_(f.data)
        if entry is not None:
            for k, sl in zip(f.names, f.slices):
                f.ema[sl].copy_(entry["state_dict"]["phoneme2mel." + k].reshape(-1))


_EAGER, _SHAPE_GRAPH, _SHARED_GRAPH = "eager", "in the per-shape graph", "in the shared boundary graph"     # `TrainStep._boundary_in`


class TrainStep:
    """One optimizer step of the reference's training loop (model.py:212-226 + :279-283) on one GPU of a data-parallel job.

    step(x, y): forward + loss + backward on this rank's batch, ONE all-reduce (mean) of the flat gradient buffer over `group`
    (RCCL when the process group is `nccl`), one AdamW launch.  lr follows torch.optim.AdamW's defaults as model.py sets them.

    graph=True captures the step into one hipGraph the first time a batch SHAPE is seen and replays it for every later batch of
    that shape (inputs are copied into the graph's static buffers; step count, learning rate and the loss scaler live in device
    memory): the whole step on one GPU, everything up to the gradient all-reduce when data-parallel (the collective and the
    optimizer launch then follow eagerly).  The eager step is bound by the host's dispatch of its ~180-220 launches (pinned row by row in
    tests/test_train_dispatch.py); the replay runs at the kernels' own pace (both are `bench.py`'s `train_step` leg).

    gradient_clip_val=c (Lightning's Trainer knob; None / 0: off) clips the gradients' 2-norm to c before the update, on the device and
    inside a captured graph; `grad_norm` and `clip_coef` read the last step's norm and coefficient (inf: measure only).

    accumulate_grad_batches=N (Lightning's Trainer knob; None / 1: off -- not one launch, buffer or attribute differs) makes `step` one
    MICRO-batch: forward, loss and backward as ever, then one launch adds its gradients / N to `flat.acc`.  Every N-th call is the
    window's boundary: the all-reduce (data-parallel: only there, Lightning's `no_sync` in between), the unscale, the clipping and the
    AdamW launch run once on the sum, which is then zeroed.  At precision 16 the loss scale holds for the whole window and an inf / nan
    of any micro-batch skips all of it.  `micro` counts the open window's micro-batches, `flush()` closes a short one (the last batches
    of an epoch; not renormalised), `t` counts optimizer steps.  graph=True: the per-shape graph ends with the accumulate launch, and one
    more graph, shared by all shapes, replays the boundary (one GPU; data-parallel it stays eager, as the optimizer launch does).  Without
    the knob the schedule is the same with a window of one: the table in `__init__` says where the boundary runs in every case.

    ema_decay=d (a float, 0 < d < 1; None: off -- not one launch, buffer or attribute differs) keeps an exponential moving average of the
    weights in `flat.ema`: ema_0 is the weights at construction and one launch directly after every optimizer launch makes
    ema_k = lerp(ema_{k-1}, p_k, 1 - d) -- torch.optim.swa_utils.AveragedModel with get_ema_multi_avg_fn(d) whose first update_parameters
    saw the initial weights, so there is no update counter, and there is NO decay warm-up.  The launch lies inside whatever is captured,
    runs only on a window's boundary (and `flush()`) when accumulating, does not run for a skipped precision-16 step (it reads the
    optimizer's skip flag on the device) and adds no collective: replicas hold identical weights, hence identical averages.
    `ema_weights()` is a context manager inside which `net` holds the averaged weights (one in-place exchange of the two buffers each
    way: parameters, packed copies and captured graphs keep their addresses); while it is open `step`, `flush`, `state_dict`,
    `load_state_dict` and a nested `ema_weights()` raise RuntimeError.  `ema_state_dict()` exports the average as 'phoneme2mel.<key>'
    weights; `state_dict()` stores it under "ema" and `load_state_dict` restores it (a checkpoint without one restarts the average from
    the loaded weights).

    evaluate(x, y, ema=None) is the teacher-forced forward and the loss under no_grad, eagerly: a validation loss that touches neither
    the optimizer nor any buffer of the step (ema=None: on the averaged weights where the step has them)."""

    def __init__(self, net, lr=1e-3, weight_decay=1e-6, betas=(0.9, 0.999), eps=1e-8, group=None, world_size=1, graph=False,
                 precision=32, init_scale=65536.0, growth_factor=2.0, backoff_factor=0.5, growth_interval=2000, gradient_clip_val=None,
                 accumulate_grad_batches=None, ema_decay=None):
        if ema_decay is not None and (isinstance(ema_decay, bool) or not isinstance(ema_decay, float) or not 0.0 < ema_decay < 1.0):
            raise ValueError(f"ema_decay must be None or a float with 0 < ema_decay < 1, not {ema_decay!r}")
        n_acc = 1 if accumulate_grad_batches is None else accumulate_grad_batches
        if isinstance(n_acc, bool) or not isinstance(n_acc, numbers.Integral) or n_acc < 1:
            raise ValueError(f"accumulate_grad_batches must be None or an int >= 1, not {accumulate_grad_batches!r}")
        self.net, self.flat = net, FlatParams(net, accumulate=n_acc > 1, ema=ema_decay is not None)
        self.lr, self.wd, self.betas, self.eps = lr, weight_decay, betas, eps
        self.group, self.world = group, world_size
        # The schedule: a call of `step` is one micro-batch, and a boundary when it fills the window of N (None / 1: a window of one).
        self._window, self._micro = int(n_acc), 0   # N, and the micro-batches in the open window
        self._avg = WeightAverage(self.flat, ema_decay) if ema_decay is not None else None
        # Where the boundary runs:
        #   graph   world   N     the per-shape graph holds        the boundary
        #   off     any     any   --                               eager
        #   on      1       1     micro-batch + boundary           inside that graph
        #   on      1       > 1   micro-batch (accumulate last)    the one shared graph `_boundary_graph` (the first boundary runs eagerly,
        #                                                          then is captured: a capture does not execute)
        #   on      > 1     any   micro-batch                      eager, behind the all-reduce: a collective stays outside a graph
        #                                                          (N = 1: as the tail of the shape's replay, see `_replayed`)
        self._boundary_in = _EAGER if not graph or world_size > 1 else (_SHAPE_GRAPH if n_acc == 1 else _SHARED_GRAPH)
        self._boundary_graph = None                 # (stays None unless the third row applies)
        self.epoch = 0                              # what `state_dict()` records; `fit` and `load_state_dict` set it
        # precision 16 = what Lightning's `precision=16` does around the reference's step (train.py:66-70): autocast-class GEMMs
        # (binary16 operands, fp32 accumulate, fp32 master weights) + torch.amp.GradScaler's dynamic loss scaling: the backward
        # is seeded with `scale`, a step whose gradients hold inf / nan is skipped and halves the scale, `growth_interval` clean
        # steps in a row double it.  `skipped` counts the skipped steps (they do not advance the optimizer's step count).
        # precision "bf16" ("bf16-mixed") = autocast-class GEMMs with bfloat16 operands.  bfloat16 has fp32's exponent range, so there
        # is no scaler: the backward is seeded with 1, no step is skipped, and everything else runs as at precision 32.
        precision = normalize_precision(precision)
        self.precision = precision
        self.graph = bool(graph)
        # gradient_clip_val = Lightning's Trainer knob (algorithm "norm"): clip_grad_norm_ over the flat gradient buffer -- after the
        # all-reduce and the division by the world size, so every rank clips by the same coefficient -- on the device (`AdamWState`)
        self._opt = AdamWState(self.flat.data.device, precision, self.graph, lr, init_scale, growth_factor, backoff_factor, growth_interval,
                               gradient_clip_val)
        self._graphs = {}
        self._build_pack_list()
        self._packed = networks.PackedCopies(net)   # what the inference path keeps of the weights this step's optimizer overwrites

    # the optimizer's step count and the loss scaler's read-outs: `AdamWState`'s (under graph replay and at precision 16 each read is
    # one small device -> host copy; the step itself never reads them)
    t = property(lambda self: self._opt.t, lambda self, v: setattr(self._opt, "t", v))
    scale = property(lambda self: self._opt.scale)
    skipped = property(lambda self: self._opt.skipped)
    growth_interval = property(lambda self: self._opt.growth_interval, lambda self, n: setattr(self._opt, "growth_interval", n))
    grad_norm = property(lambda self: self._opt.grad_norm)      # (both: AttributeError unless gradient_clip_val is set)
    clip_coef = property(lambda self: self._opt.clip_coef)
    micro = property(lambda self: self._micro)     # micro-batches in the open accumulation window: a Python int, no device read (0 when off)

    # ---- checkpoint / resume (what Lightning's ModelCheckpoint keeps: weights, hyper-parameters, the optimizer's state_dict)
    def hyper_parameters(self):
        """The constructor arguments of the reference's LightningModule (model.py:104-121) that describe this network: what
        `load_from_checkpoint` needs next to the weights."""
        pe, dec = self.net.encoder, self.net.decoder
        e = pe.encoder
        return {"depth": e.depth, "reduction": e.embed_dim // pe.dim, "head": e.heads[0], "embed_dim": e.embed_dim,
                "kernel_size": e.kernels[0], "expansion": e.expansion, "n_blocks": dec.n_blocks, "block_depth": dec.block_depth,
                "decoder_kernel_size": dec.kernel_size, "lr": self.lr, "weight_decay": self.wd}

    def optimizer_state_dict(self):
        """`torch.optim.AdamW(net.parameters()).state_dict()` as the reference's optimizer would hold it after `self.t` steps:
        per-parameter `step` / `exp_avg` / `exp_avg_sq` (views of the flat moment buffers, cloned), indexed by the parameter's
        position in `net.parameters()`; parameters that never received a gradient (the bins, the two unreached LayerNorms) have
        no state, as in torch."""
        f = self.flat
        index = {id(p): j for j, p in enumerate(self.net.parameters())}
        state = {}
        t_now = self.t                          # (possibly a device read -- once, not per parameter)
        for p, sl in zip(f.params, f.slices):
            if t_now > 0:
                state[index[id(p)]] = {"step": torch.tensor(float(t_now)), "exp_avg": f.m[sl].view(p.shape).clone(),
                                       "exp_avg_sq": f.v[sl].view(p.shape).clone()}
        group = {"lr": self.lr, "initial_lr": self.lr, "betas": tuple(self.betas), "eps": self.eps, "weight_decay": self.wd, "amsgrad": False,
                 "maximize": False, "foreach": None, "capturable": False, "differentiable": False, "fused": None,
                 "decoupled_weight_decay": True, "params": list(range(len(index)))}
        return {"state": state, "param_groups": [group]}

    def state_dict(self):
        """A Lightning-shaped checkpoint dict: `state_dict` ('phoneme2mel.<key>' weights), `hyper_parameters` (what
        `EfficientSpeech.load_from_checkpoint` / the reference's constructor need), `optimizer_states` = [a torch AdamW
        state_dict] (loads into `torch.optim.AdamW(net.parameters())`), `global_step`.  The reference's own
        `load_from_checkpoint` additionally expects `hifigan.*` weights (its module owns the vocoder, model.py:148) and a
        `preprocess_config` argument: pass `strict=False, preprocess_config=...` there, or attach the vocoder's weights under
        `hifigan.` before saving.  Inside an accumulation window (`micro != 0`) there is no consistent state to write: RuntimeError."""
        self._refuse_inside_ema_weights("state_dict()")
        if self._micro:
            raise RuntimeError(f"{self._micro} micro-batch(es) of an accumulation window are pending: call flush() before state_dict()")
        ck = {"state_dict": {"phoneme2mel." + k: v.detach().clone() for k, v in self.net.state_dict().items()},
              "hyper_parameters": self.hyper_parameters(), "optimizer_states": [self.optimizer_state_dict()],
              "global_step": self.t, "epoch": int(self.epoch)}
        scaler = self._opt.scaler_state_dict()
        if scaler is not None:
            ck["scaler"] = scaler
        if self._avg is not None:
            ck["ema"] = self._avg.entry(self.net)
        return ck

    def load_state_dict(self, ckpt):
        """Resume: weights into the flat buffer's views (in place), the AdamW moments and step count from the optimizer state
        (torch's AdamW state_dict layout, as `state_dict()` writes it).  Only optimizer states written by `TrainStep.state_dict()` --
        i.e. over `net.parameters()` of the acoustic model alone -- load: the reference's own optimizer also owns the vocoder's
        parameters (model.py:148, 279-283), so its state has a different parameter list and is refused below.  `ckpt['epoch']`
        (when present) is returned so that the caller can pass it to `fit(first_epoch=...)`.  An open accumulation window is dropped
        (the accumulator zeroed, `micro` = 0): a checkpoint is never taken inside one, and `accumulate_grad_batches` is not part of it.
        With `ema_decay`: the checkpoint's "ema" entry restores the average (a stored decay other than this step's: RuntimeError); without
        an entry the average starts again from the loaded weights.  A step without `ema_decay` ignores the entry."""
        self._refuse_inside_ema_weights("load_state_dict()")
        ema = self._avg.accept(ckpt.get("ema")) if self._avg is not None else None      # (refused before anything is overwritten)
        sd = {k[len("phoneme2mel."):]: v for k, v in ckpt["state_dict"].items() if k.startswith("phoneme2mel.")}
        own = dict(self.net.state_dict())
        missing = [k for k in own if k not in sd]
        if missing:
            raise RuntimeError(f"checkpoint lacks {missing[:3]} ...")
        with torch.no_grad():
            for k, t in own.items():
                t.copy_(sd[k])                      # in place: parameters stay views of the flat buffer
        o = ckpt["optimizer_states"][0]
        f = self.flat
        index = {id(p): j for j, p in enumerate(self.net.parameters())}
        if len(o["param_groups"][0]["params"]) != len(index):
            raise RuntimeError("optimizer state was saved for a different parameter list")
        f.m.zero_()
        f.v.zero_()
        steps = set()
        for p, sl in zip(f.params, f.slices):
            st = o["state"].get(index[id(p)])
            if st is not None:
                f.m[sl].copy_(st["exp_avg"].reshape(-1))
                f.v[sl].copy_(st["exp_avg_sq"].reshape(-1))
                steps.add(int(st["step"]))
        if len(steps) > 1:
            raise RuntimeError(f"per-parameter step counts differ: {sorted(steps)}")
        self.t = steps.pop() if steps else 0
        g = o["param_groups"][0]
        # the BASE learning rate: under a scheduler torch stores it as `initial_lr` and keeps the scheduled value in `lr` (0 at the
        # first step of the reference's LambdaLR warm-up) -- `fit` derives every step's rate from the base one
        self.lr, self.wd, self.betas, self.eps = g.get("initial_lr", g["lr"]), g["weight_decay"], tuple(g["betas"]), g["eps"]
        self._opt.load_scaler_state_dict(ckpt.get("scaler"))
        self._packed.invalidate()
        if self._window > 1:
            f.acc.zero_()
            self._micro = 0
        if self._avg is not None:
            self._avg.load(ema)
        self.epoch = int(ckpt.get("epoch", 0))
        return self.epoch

    def _build_pack_list(self):
        """Persistent GEMM copies (forward layout, data-gradient layout) of every dense convolution / Linear weight, re-made by ONE
        launch per step (esmi_train_pack_weights_f32) instead of one pack launch per operator call (40 per step)."""
        mods = [m for m in self.net.modules() if isinstance(m, (torch.nn.Conv1d, torch.nn.ConvTranspose1d, torch.nn.Linear))
                and getattr(m, "groups", 1) == 1 and getattr(m.weight, "_esmi_grad_view", None) is not None]
        self._pack_n = len(mods)
        self._pack_descs = (_lib.ConvDesc * max(1, len(mods)))()
        self._pack_w = (C.c_void_p * max(1, len(mods)))()
        lib = _lib.load()
        for j, m in enumerate(mods):
            w = m.weight
            tr = isinstance(m, torch.nn.ConvTranspose1d)
            w3 = w if w.dim() == 3 else w.unsqueeze(-1)
            c_in, c_out, k = (w3.shape[0], w3.shape[1], w3.shape[2]) if tr else (w3.shape[1], w3.shape[0], w3.shape[2])
            stride, pad = (m.stride[0], m.padding[0]) if w.dim() == 3 else (1, 0)
            d = _lib.ConvDesc(1, 1, c_in, 1, c_out, k, stride, pad, 1, 1 if tr else 0, 0)
            nb = lib.esmi_train_conv_workspace_bytes(C.byref(d))
            w._esmi_packed = (torch.zeros(nb, dtype=torch.uint8, device=w.device), torch.zeros(nb, dtype=torch.uint8, device=w.device))
            d.packed_fwd, d.packed_grad = _ptr(w._esmi_packed[0]), _ptr(w._esmi_packed[1])
            self._pack_descs[j] = d
            self._pack_w[j] = w.data_ptr()

    @contextlib.contextmanager
    def _operators_in_step(self, loss_seed):
        """The operators run inside a step: its context (precision, what the backward is seeded with) and, first of all, the ONE pack
        launch whose copies of the current weights every dense operator then reads."""
        with _step_context(self.precision, loss_seed) as now:
            if USE_MATRIX_PIPE and self._pack_n:
                lib, st = _rt(self.flat.data)
                lib.esmi_train_pack_weights_f32(self._pack_descs, self._pack_w, self._pack_n, st)
                now.packed_valid = True
            yield now

    def _fwd_bwd(self, x, y):
        """Forward, loss, backward, and the one launch that finishes every parameter gradient: everything up to the exchange.
        Capturable as a hipGraph (no host reads, no collectives)."""
        f = self.flat
        f.zero_grad()
        rq = (_lib.ReduceQueue(), [])
        lib0, st0 = _rt(f.data)
        seed = self._opt.loss_seed                 # one device float: the loss scale, or the constant 1 where there is no scaler
        with self._operators_in_step(seed if self._opt.scaler is not None else False) as now:
            parts, total = training_loss(self.net, x, y)
            # one backward on a zeroed buffer: operators write parameter gradients in place and queue their reductions' second stages
            now.direct_grads, now.reduce_queue = True, rq
            total.backward(gradient=seed.reshape(total.shape))
        lib0.esmi_train_reduce_flush_f32(C.byref(rq[0]), st0)      # every queued parameter-gradient reduction in one launch
        rq[1].clear()
        return loss_vector(parts, total)

    # ---- the schedule: micro-batch, boundary, and where each runs (the table in __init__)
    def _micro_batch(self, x, y):
        """One micro-batch: everything up to the exchange and, in a window of N > 1, the one launch that adds its gradients / N to the
        accumulator (the backward overwrites `flat.grad`, so the sum cannot live there).  Capturable."""
        losses = self._fwd_bwd(x, y)
        if self._window > 1:
            f = self.flat
            lib, st = _rt(f.data)
            lib.esmi_train_grad_accumulate_f32(_ptr(f.acc), _ptr(f.grad), f.grad.numel(), 1.0 / self._window, st)   # (1 / N rounds to fp32 once)
        return losses

    def _boundary(self):
        """A window's boundary on its gradients -- `flat.acc` where the step accumulates, else `flat.grad`: the exchange (one all-reduce of
        that buffer when data-parallel), the optimizer launch (step count, learning rate and the loss scaler's state are `AdamWState`'s),
        the average's update.  Capturable on one GPU."""
        f = self.flat
        g = f.acc if self._window > 1 else f.grad
        if self.world > 1:
            import torch.distributed as dist
            dist.all_reduce(g, op=dist.ReduceOp.SUM, group=self.group)
            g.div_(self.world)                     # DDP averages (train.py:66-70 runs Lightning's default DDP strategy)
        self._opt.launch(f, self.betas, self.eps, self.wd, grad=g)
        if self._avg is not None:
            self._avg.update(self._opt)
        if g is not f.grad:
            g.zero_()                              # (also after a skipped window: its inf / nan must not reach the next one)

    def _captured(self, x, y):
        """What the hipGraph of a batch shape holds."""
        losses = self._micro_batch(x, y)
        if self._boundary_in == _SHAPE_GRAPH:
            self._boundary()
        return losses

    def _replayed(self, x, y, tail):
        """graph=True: `_captured(x, y)` -> losses through the hipGraph of this batch SHAPE (inputs are copied into its static buffers), then
        `tail()` eagerly where there is one (what cannot be captured: a collective and what follows it).  The first batch of a shape runs
        both eagerly on a side stream, which warms the allocator, and then captures `_captured`: the capture itself does not execute."""
        key = tuple((k, tuple(v.shape)) for k, v in sorted({**x, **{"y." + k: v for k, v in y.items()}}.items()) if torch.is_tensor(v))
        ent = self._graphs.get(key)
        if ent is None:
            sx = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in x.items()}
            sy = {k: v.clone() for k, v in y.items()}
            side = torch.cuda.Stream(device=self.flat.data.device)
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                out = self._captured(sx, sy)
                if tail is not None:
                    tail()
            torch.cuda.current_stream().wait_stream(side)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                static_out = self._captured(sx, sy)
            self._graphs[key] = (g, sx, sy, static_out)
            return out.clone()
        g, sx, sy, static_out = ent
        for k, v in x.items():
            if torch.is_tensor(v):
                sx[k].copy_(v)
        for k, v in y.items():
            sy[k].copy_(v)
        g.replay()
        if tail is not None:
            tail()
        return static_out.clone()

    def _close_window(self, boundary_ran=False):
        """The boundary, unless the call's graph or its tail has run it, and the one place where a window ends."""
        if not boundary_ran:
            if self._boundary_in != _SHARED_GRAPH:
                self._boundary()
            elif self._boundary_graph is not None:
                self._boundary_graph.replay()
            else:                                  # one graph for every window, whatever shapes its micro-batches had
                self._boundary()                   # (this window's boundary runs eagerly: the capture itself does not execute)
                self._boundary_graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(self._boundary_graph):
                    self._boundary()
        self._micro = 0
        self._packed.invalidate()

    def step(self, x, y, lr=None):
        """One training step.  graph=True: a hipGraph per batch SHAPE replays the step (inputs are copied into its static buffers) --
        the whole step on one GPU; data-parallel, everything up to the gradient all-reduce (the collective and the optimizer launch
        follow eagerly).  With accumulate_grad_batches=N this is one micro-batch, and every N-th call ends with the window's boundary;
        the losses returned are this micro-batch's own, undivided."""
        self._refuse_inside_ema_weights("step()")
        self._opt.set_lr(self.lr if lr is None else lr)
        # a captured window of one runs its boundary within this call's replay: inside the shape's graph, or eagerly as its tail
        within = self.graph and self._window == 1
        if not self.graph:
            out = self._micro_batch(x, y)
        else:
            out = self._replayed(x, y, self._boundary if within and self._boundary_in == _EAGER else None)
        self._micro += 1                           # (only now: a forward that raised has left the window as it was)
        if self._micro == self._window:
            self._close_window(boundary_ran=within)
        return out

    def flush(self, lr=None):
        """Close the open accumulation window now (Lightning's last-batch-of-the-epoch rule): the boundary on whatever has
        accumulated, the 1 / N weights kept (a short window is not renormalised).  -> False, and nothing runs, when `micro == 0`."""
        self._refuse_inside_ema_weights("flush()")
        if not self._micro:
            return False
        self._opt.set_lr(self.lr if lr is None else lr)
        self._close_window()
        return True

    # ---- the weights' exponential moving average (ema_decay=d: `WeightAverage`) and the validation loss
    _ema_open = property(lambda self: self._avg is not None and self._avg.open)

    def _need_ema(self, what):
        if self._avg is None:
            raise AttributeError(f"no {what}: this step keeps no average of the weights (ema_decay is None)")
        return self._avg

    def _refuse_inside_ema_weights(self, what):
        if self._ema_open:
            raise RuntimeError(f"{what} inside ema_weights(): the weights and their average are exchanged; leave the context first")

    @contextlib.contextmanager
    def ema_weights(self):
        """Inside the context `net` (its inference path, `evaluate`) runs on the averaged weights: one launch exchanges the contents of
        `flat.data` and `flat.ema` on entry and one exchanges them back on exit, after which both are bitwise what they were."""
        avg = self._need_ema("ema_weights()")
        self._refuse_inside_ema_weights("ema_weights()")
        avg.exchange(self._packed)
        avg.open = True
        try:
            yield self
        finally:
            avg.open = False
            avg.exchange(self._packed)

    def ema_state_dict(self):
        """The averaged weights as {'phoneme2mel.<key>': tensor}, cloned: with `hyper_parameters()` what `EfficientSpeech.load_from_checkpoint`
        needs to synthesize from the average.  Parameters outside the flat buffer (the bins, the two unreached LayerNorms) and buffers
        are `net`'s own."""
        return self._need_ema("ema_state_dict()").weights(self.net)

    def evaluate(self, x, y, ema=None):
        """The loss 5-vector (`step`'s layout) of the teacher-forced forward under no_grad: a validation loss.  ema=None: on the averaged
        weights if this step keeps them; True: on them (AttributeError without `ema_decay`); False: on the weights as they are.  Runs
        eagerly (also when graph=True), in a step context of its own -- the step's precision, no loss seed, the pack launch first, so it
        reads the weights as they are now -- and changes nothing: weights, average, gradients, moments, accumulator, counters, scaler
        and hyper block stay bitwise what they were, also inside an open accumulation window."""
        if ema is None:
            ema = self._avg is not None
        if ema:
            self._need_ema("evaluate(ema=True)")
        on_average = self.ema_weights() if ema and not self._ema_open else contextlib.nullcontext()     # (inside ema_weights() they already are)
        with on_average, torch.no_grad(), self._operators_in_step(False):
            parts, total = training_loss(self.net, x, y)
        return loss_vector(parts, total)


def lr_at_epoch(epoch, base_lr=1e-3, warmup=50, total=5000, min_lr=0.0):
    """model.py:77-101 + :281: LambdaLR(linear warm-up over `warmup` epochs, then cosine decay to `total`), stepped once per epoch
    by Lightning's default scheduler interval -- epoch 0 therefore trains at lr 0, as in the reference."""
    import math
    if epoch < warmup:
        lam = float(epoch) / float(max(1, warmup))
    else:
        lam = max(min_lr, 0.5 * (1.0 + math.cos(math.pi * float(epoch - warmup) / float(max(1, total - warmup)))))
    return base_lr * lam


def to_device(batch, device):
    """Move the tensors of a datamodule batch (x or y dict; x also carries the raw `text` list) to `device`."""
    return {k: (v.to(device) if torch.is_tensor(v) else v) for k, v in batch.items()}


def _epoch_mean(step, acc, n):
    """The mean of `n` summed loss vectors, averaged over the data-parallel ranks (one 5-float all-reduce on `step.group`)."""
    mean = acc / max(n, 1) if acc is not None else None
    if mean is not None and step.world > 1:
        import torch.distributed as dist
        dist.all_reduce(mean, op=dist.ReduceOp.SUM, group=step.group)
        mean = mean / step.world
    return mean


def fit(step, loader, epochs, device, base_lr=None, warmup=50, total=5000, first_epoch=0, log=None, val_loader=None,
        check_val_every_n_epoch=10):
    """The reference's training loop (train.py:66-76 -> Lightning `trainer.fit`) reduced to what it computes: for every epoch,
    the scheduled learning rate; for every batch of the datamodule, one `TrainStep.step`; at the end of the epoch the means of the
    five losses over the epoch's steps, averaged over the data-parallel ranks (model.py:227-242: `on_train_epoch_end` logs them
    with `sync_dist=True`) -- one 5-float all-reduce per epoch on `step.group`.  Returns the per-epoch records.  A step that
    accumulates (`accumulate_grad_batches=N`) is flushed after the last batch of every epoch, so no window stays open, and the means
    are over its micro-batches: the reference logs per `training_step`.  With a `val_loader`, validation runs after every epoch e with
    (e + 1) % check_val_every_n_epoch == 0 (Lightning's rule; the reference's Trainer sets 10, train.py:66-70), after the epoch's flush:
    the mean of `step.evaluate` over its batches (on the averaged weights where the step keeps them), averaged over the ranks as the
    training means are, is that epoch's record["val_losses"].  Every other record has no such key."""
    if val_loader is not None and (isinstance(check_val_every_n_epoch, bool) or not isinstance(check_val_every_n_epoch, numbers.Integral)
                                   or check_val_every_n_epoch < 1):
        raise ValueError(f"check_val_every_n_epoch must be an int >= 1, not {check_val_every_n_epoch!r}")
    base_lr = step.lr if base_lr is None else base_lr
    history = []
    for epoch in range(first_epoch, first_epoch + epochs):
        lr = lr_at_epoch(epoch, base_lr, warmup, total)
        acc, n = None, 0
        for x, y in loader:
            losses = step.step(to_device(x, device), to_device(y, device), lr=lr)
            acc = losses.clone() if acc is None else acc + losses        # five scalars per step: bookkeeping, like self.log()
            n += 1
        if step.micro:                  # an epoch never leaves an accumulation window open
            step.flush(lr)
        mean = _epoch_mean(step, acc, n)
        history.append({"epoch": epoch, "lr": lr, "losses": mean.cpu().tolist() if mean is not None else None})
        if val_loader is not None and (epoch + 1) % check_val_every_n_epoch == 0:
            acc, n = None, 0
            for x, y in val_loader:
                losses = step.evaluate(to_device(x, device), to_device(y, device))
                acc = losses.clone() if acc is None else acc + losses
                n += 1
            mean = _epoch_mean(step, acc, n)
            history[-1]["val_losses"] = mean.cpu().tolist() if mean is not None else None
        step.epoch = epoch + 1          # what `state_dict()` records: the epoch a resumed `fit(first_epoch=...)` starts with
        if log:
            log(history[-1])
    return history


def synthetic_batch(B, T, dur, device, seed=5):
    """A seeded teacher-forced batch of the shapes datamodule.collate_fn produces (datamodule.py:29-76): no padding, D-const."""
    import numpy as np
    from .synth import synth_phonemes
    g = np.random.default_rng(seed)
    ids, mask = synth_phonemes(B, T, seed)
    L = T * dur
    x = {"phoneme": torch.from_numpy(ids), "phoneme_mask": torch.from_numpy(mask),
         "pitch": torch.from_numpy(g.uniform(-3, 10, (B, T)).astype(np.float32)),
         "energy": torch.from_numpy(g.uniform(-2, 8, (B, T)).astype(np.float32)),
         "duration": torch.full((B, T), dur, dtype=torch.int32), "mel_len": torch.full((B,), L, dtype=torch.int32),
         "mel_mask": torch.zeros((B, L), dtype=torch.bool)}
    y = {"mel": torch.from_numpy(g.normal(-5, 2, (B, L, 80)).astype(np.float32))}
    return {k: v.to(device) for k, v in x.items()}, {k: v.to(device) for k, v in y.items()}
