"""Every kernel variant of the training step (csrc/train_ops.h) at the edge shapes where csrc/tu_train.hip's host code switches between
them, against the same operation in plain PyTorch on float64 CPU copies of the inputs (forward and torch.autograd.grad).  Shared by the
wave-simulator tier and the GPU tier of tests/test_train_variants.py: `run_row` takes the device ("cuda", or "cpu" inside `use_sim()`).

`ROWS` is the table.  A row names the operator (`train._Conv`, `_LayerNorm`, `_AttnCore`, `_Repeat`, or a C entry point called through
`_lib`), the shape, `train.USE_MATRIX_PIPE` where the dispatch reads it, the kernels the row must launch and the alternatives it must
not (the LDS-staged attention pair in a global-memory row, the 16-byte kernels in a misaligned one).  The names are checked on the
simulator tier only (`tests.simlib.launched_kernels()` records the simulator's launches).  The dispatch -- every `if` of tu_train.hip
on a shape, an alignment or an LDS budget -- is host code that both builds compile from the same lines, so the simulator's name check
speaks for the device as well.  The one known difference between the builds that a row depends on: `kReduceGroups` (the waves of a
reduction workgroup, csrc/wavesim_shim.h) is 4 on the simulator and 16 on the device; the reduction row takes its chunk counts from
`_lib.REDUCE_GROUPS` of the build under test, so it sits on the unrolled loop's edges in both.

Yardstick and bounds are the project's, no new numbers: max |got - ref64| / max(1e-6, max |ref64|) per tensor (`_err`, as in
tests/test_train_gemm_at_size.py), 2e-5 forward, 5e-5 gradients, 1e-4 for gradients that pass through an activation + LayerNorm chain
(tests/test_train_gemm_at_size.py); 1e-5 LayerNorm forward, 1e-5 attention forward (tests/test_train_ops.py); exact operators assert
torch.equal.  One exception to the yardstick: a single-number output -- the bias gradient of a one-channel Linear -- is measured
relative to sum |dy|, the scale of its summands: with zero-mean dy the reference is a cancelled sum, and a correct kernel's 1e-7
rounding of the summands shows as 2.8e-6 of it (lin1_c48).  Every figure is printed before it is asserted (pytest -s), with the error
of torch's own fp32 operator on the same inputs against the same float64 reference beside it (profiles/r20_train_variants.md).

The output ReLU of a LayerNorm row (`relu_out`) is a discrete decision: its gate is taken from the kernel's own output, and must agree
with float64 wherever |LN| > 1e-5 (as tests/test_train_gemm_at_size.py's check_conv_ln has it).  "offset" rows pass every float tensor
as a contiguous view one float into its buffer (4 bytes past a 16-byte boundary), which the flat parameter and gradient buffers make
ordinary; the 16-byte kernels must then give way to the generic ones."""
import ctypes as C
import dataclasses

import torch
import torch.nn.functional as F

from efficientspeech_amd import _lib, train
from efficientspeech_amd.networks import _ptr

FWD, GRAD, CHAIN = 2e-5, 5e-5, 1e-4         # tests/test_train_gemm_at_size.py
LN_FWD = ATTN_FWD = 1e-5                    # tests/test_train_ops.py
GATE_MARGIN = 1e-5                          # |LN| above which the output ReLU's gate must be float64's (check_conv_ln)


@dataclasses.dataclass(frozen=True)
class Row:
    id: str
    op: str                     # "attn" | "lin1" | "ln" | "conv" | "repeat" | "copy_cols" | "reduce"
    shape: tuple
    must: tuple                 # kernels the row must launch
    absent: tuple = ()          # the alternatives it must not
    matrix_pipe: object = None  # train.USE_MATRIX_PIPE for the row; None: the dispatch does not read it
    opt: tuple = ()             # "offset", "nobias", "res_mask_relu", "tanh_mask_relu"


def _rand(*shape, seed, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def _offset(t, dev):
    """`t` on `dev` as a contiguous view one float into a buffer: 4 bytes past a 16-byte boundary."""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=dev)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v.detach()


def _put(t, dev, offset=False):
    """The kernel's copy of a CPU tensor: fp32 on the device, a leaf that takes a gradient."""
    if t is None:
        return None
    t = t.float()
    return (_offset(t, dev) if offset else t.to(dev).clone()).requires_grad_()


def _err(got, ref, scale=None):
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    return float((got - ref).abs().max()) / (max(1e-6, float(ref.abs().max())) if scale is None else scale)


class _Judge:
    """One row's reference: `fn(*inputs)` -> y and its gradients for the incoming `dy`, once on float64 CPU copies (the reference) and
    once in torch's own fp32 on the device (the figure printed beside the kernel's).  inputs: CPU tensors, None for an absent one.
    perturb(what, tensor) -> tensor is applied to every tensor of the kernel's before it is measured (the self-check)."""

    def __init__(self, row, dev, fn, inputs, dy, perturb=None, figures=None):
        self.row, self.perturb, self.figures = row, perturb, figures
        self.y64, self.g64 = self._run(fn, inputs, dy, torch.float64, "cpu")
        self.y32, self.g32 = self._run(fn, inputs, dy, torch.float32, dev)

    @staticmethod
    def _run(fn, inputs, dy, dtype, dev):
        leaves = [None if t is None else t.detach().to(device=dev, dtype=dtype).clone().requires_grad_() for t in inputs]
        y = fn(*leaves)
        grads = iter(torch.autograd.grad(y, [t for t in leaves if t is not None], dy.detach().to(device=dev, dtype=dtype)))
        return y.detach(), [None if t is None else next(grads) for t in leaves]

    def check(self, what, got, index, bound, scale=None, exact=False):
        """index: None the forward, else the input whose gradient `got` is.  scale: the yardstick's denominator, where it is not max |ref|."""
        ref, t32 = (self.y64, self.y32) if index is None else (self.g64[index], self.g32[index])
        if self.perturb is not None:
            got = self.perturb(what, got.detach().clone())
        e, e32 = _err(got, ref, scale), _err(t32, ref, scale)
        print(f"    {self.row.id} {what}: {e:.3e} (bound {bound:.1e}; torch fp32 {e32:.3e})")
        if self.figures is not None:
            self.figures.append((self.row.id, what, e, bound, e32))
        assert bool(torch.isfinite(got).all()), (self.row.id, what, "not finite")
        assert got.shape == ref.shape, (self.row.id, what, got.shape, ref.shape)
        if exact:
            assert torch.equal(got.detach().cpu().double(), ref), (self.row.id, what, "not exact")
        assert e < bound, (self.row.id, what, e, bound)


# ------------------------------------------------------------------------------------------------------------------- attention
def _attn_ref(Cc, h):
    def fn(qkv):                                               # blocks.py:43-64, as tests/test_train_ops.py::test_attention_core
        B, N, _ = qkv.shape
        q, k, v = qkv.reshape(B, N, 3, h, Cc).permute(2, 0, 3, 1, 4).unbind(0)
        attn = ((q @ k.transpose(-2, -1)) * (Cc // h) ** -0.5).softmax(dim=-1)
        return (attn @ v).transpose(1, 2).reshape(B, N, -1)
    return fn


def _run_attn(dev, row, kw):
    B, N, Cc, h = row.shape
    qkv, dy = _rand(B, N, 3 * h * Cc, seed=7, scale=0.5), _rand(B, N, h * Cc, seed=8)
    x = _put(qkv, dev)
    got = train._AttnCore.apply(x, h)
    (gx,) = torch.autograd.grad(got, x, dy.to(dev))
    J = _Judge(row, dev, _attn_ref(Cc, h), (qkv,), dy, **kw)
    J.check("forward", got, None, ATTN_FWD)
    J.check("dqkv", gx, 0, GRAD)


# ---------------------------------------------------------------------------------------------------------- one-channel Linear
def _run_lin1(dev, row, kw):
    """x (B, n, c_in) -> 1 channel through `train._Conv` (forward `conv_to1_kernel`; backward the three gradients in one launch).  The
    "offset" row: the forward GEMM path refuses a misaligned input (ESMI_ERR_ARG), so the forward runs on the aligned copy and the
    backward is `esmi_train_conv_bwd_f32` itself, called on the view one float into its buffer."""
    cin, B, n = row.shape
    bias, off = "nobias" not in row.opt, "offset" in row.opt
    x0, w0, dy = _rand(B, n, cin, seed=1), _rand(1, cin, seed=2) * cin ** -0.5, _rand(B, n, 1, seed=4)
    b0 = _rand(1, seed=3) if bias else None
    x, w, b = _put(x0, dev), _put(w0, dev), _put(b0, dev)
    got = train._Conv.apply(x, w, b, 1, 0, 1, False, n)
    if off:
        lib, st = train._rt(x)
        xo, dyd = _offset(x0, dev), dy.to(dev).contiguous()
        d = _lib.ConvDesc(B, n, cin, n, 1, 1, 1, 0, 1, 0, 0, 0)
        nws = lib.esmi_train_conv_bwd_workspace_bytes(C.byref(d))
        ws = torch.empty(nws, dtype=torch.uint8, device=dev)
        gx, gw, gb = torch.full_like(x0, float("nan"), device=dev), torch.full_like(w0, float("nan"), device=dev), torch.full((1,), float("nan"), device=dev)
        lib.esmi_train_conv_bwd_f32(C.byref(d), _ptr(xo), _ptr(dyd), _ptr(w.detach()), _ptr(gx), _ptr(gw), _ptr(gb), _ptr(ws), nws, None, st)
        grads = [gx, gw, gb]
    else:
        grads = list(torch.autograd.grad(got, (x, w, b) if bias else (x, w), dy.to(dev)))
    J = _Judge(row, dev, lambda x_, w_, b_=None: x_ @ w_.T + (0 if b_ is None else b_), (x0, w0, b0), dy, **kw)
    J.check("forward", got, None, FWD)
    J.check("dgrad", grads[0], 0, GRAD)
    J.check("wgrad", grads[1], 1, GRAD)
    if bias:
        J.check("bias grad", grads[2], 2, GRAD, scale=float(dy.double().abs().sum()))      # (one number: relative to its summands)


# ------------------------------------------------------------------------------------------------------------------- LayerNorm
def _run_ln(dev, row, kw):
    rows, Cc = row.shape
    off = "offset" in row.opt
    res_v, tanh_v = "res_mask_relu" in row.opt, "tanh_mask_relu" in row.opt
    z0 = _rand(rows, Cc, seed=11, scale=1.0 if tanh_v else 3.0)
    x0 = torch.tanh(z0) if tanh_v else z0          # (fp32: what the kernel is given; the reference's leaf is atanh of it, in float64)
    g0, b0, dy = _rand(Cc, seed=13) + 1.0, _rand(Cc, seed=14), _rand(rows, Cc, seed=15)
    res0 = _rand(rows, Cc, seed=12, scale=2.0) if res_v else None
    masked = res_v or tanh_v
    r = torch.arange(rows)
    mask = ((r % 7 == 3) | (r >= rows - 5)) if masked else None
    x, g, b, res = (_put(t, dev, off) for t in (x0, g0, b0, res0))
    m8 = mask.to(torch.uint8).to(dev).contiguous() if masked else None
    got = train._LayerNorm.apply(x, g, b, res, m8, train.ACT_TANH if tanh_v else 0, masked)
    grads = torch.autograd.grad(got, (x, g, b) + ((res,) if res_v else ()), dy.to(dev))
    gate = (got.detach().cpu() > 0) if masked else None          # the output ReLU's decision, as the kernel took it

    def fn(x_, g_, b_, res_=None):
        a = torch.tanh(x_) if tanh_v else x_
        y = F.layer_norm(a if res_ is None else a + res_, (Cc,), g_, b_)
        if masked:
            if y.dtype == torch.float64:
                wrong = (gate != (y.detach() > 0)) & (y.detach().abs() > GATE_MARGIN) & ~mask[:, None]
                assert not bool(wrong.any()), (row.id, "the output ReLU's gate differs from float64 beyond the margin", int(wrong.sum()))
            y = (y * gate.to(y.device)).masked_fill(mask.to(y.device)[:, None], 0.0)
        return y
    leaf = torch.atanh(x0.double()) if tanh_v else x0
    J = _Judge(row, dev, fn, (leaf, g0, b0, res0), dy, **kw)
    gbound = CHAIN if tanh_v else GRAD                           # (the tanh variant's gradients pass through activation + LayerNorm)
    J.check("forward", got, None, LN_FWD)
    for what, gr, i in zip(("dx", "dgamma", "dbeta", "dres"), grads, range(4)):
        J.check(what, gr, i, gbound)


# ---------------------------------------------------------------------------------------------------------------- convolutions
def _run_conv(dev, row, kw):
    cin, cout, k, s, p, groups, B, n = row.shape
    n_out = (n + 2 * p - k) // s + 1
    x0, w0, b0 = _rand(B, n, cin, seed=1), _rand(cout, cin // groups, k, seed=2) * (cin * k / groups) ** -0.5, _rand(cout, seed=3)
    dy = _rand(B, n_out, cout, seed=4)
    x, w, b = _put(x0, dev), _put(w0, dev), _put(b0, dev)
    got = train._Conv.apply(x, w, b, s, p, groups, False, n_out)
    gx, gw, gb = torch.autograd.grad(got, (x, w, b), dy.to(dev))
    J = _Judge(row, dev, lambda x_, w_, b_: F.conv1d(x_.transpose(1, 2), w_, b_, stride=s, padding=p, groups=groups).transpose(1, 2),
               (x0, w0, b0), dy, **kw)
    J.check("forward", got, None, FWD)
    J.check("dgrad", gx, 0, GRAD)
    J.check("wgrad", gw, 1, GRAD)
    J.check("bias grad", gb, 2, GRAD)


# ------------------------------------------------------------------------------------------------------------ length regulator
def _run_repeat(dev, row, kw):
    """(B, T, C): durations 0 .. 6 with zeros among them, one utterance of zeros only, L five frames beyond the longest utterance."""
    B, T, Cc = row.shape
    feat0 = _rand(B, T, Cc, seed=11)
    dur = torch.randint(0, 7, (B, T), generator=torch.Generator().manual_seed(2))
    dur[:, ::5] = 0
    dur[B - 1] = 0
    L = int(dur.sum(1).max()) + 5
    dy = _rand(B, L, Cc, seed=12)
    feat = _put(feat0, dev, "offset" in row.opt)
    cum = torch.cumsum(dur, 1).to(torch.int32).to(dev).contiguous()
    got = train._Repeat.apply(feat, cum, L)
    (gf,) = torch.autograd.grad(got, feat, dy.to(dev))
    J = _Judge(row, dev, lambda f_: torch.stack([F.pad(f.repeat_interleave(d.to(f.device), dim=0), (0, 0, 0, L - int(d.sum()))) for f, d in zip(f_, dur)]),
               (feat0,), dy, **kw)
    J.check("forward", got, None, FWD, exact=True)
    J.check("dfeat", gf, 0, GRAD)


# ------------------------------------------------------------------------------------------------------- esmi_train_copy_cols_f32
def _run_copy_cols(dev, row, kw):
    import pytest
    ld_src, col_src, ld_dst, col_dst, Cc, rows = row.shape
    src = _rand(rows, ld_src, seed=21).to(dev)
    dst0 = _rand(rows, ld_dst, seed=22).to(dev)
    dst = dst0.clone()
    lib, st = train._rt(src)
    lib.esmi_train_copy_cols_f32(_ptr(src), ld_src, col_src, _ptr(dst), ld_dst, col_dst, rows, Cc, st)
    want = dst0.clone()
    want[:, col_dst: col_dst + Cc] = src[:, col_src: col_src + Cc]
    assert torch.equal(dst.cpu(), want.cpu()), row.id            # the columns copied, every other element untouched
    for bad in ((ld_src, ld_src - Cc + 1, ld_dst, col_dst), (ld_src, col_src, ld_dst, ld_dst - Cc + 1), (ld_src, -1, ld_dst, col_dst)):
        with pytest.raises(RuntimeError, match="ESMI_ERR_ARG"):      # a range that overruns either leading dimension
            lib.esmi_train_copy_cols_f32(_ptr(src), bad[0], bad[1], _ptr(dst), bad[2], bad[3], rows, Cc, st)
    assert torch.equal(dst.cpu(), want.cpu())


# --------------------------------------------------------------------------------- esmi_reduce_queue + esmi_train_reduce_flush_f32
REDUCE_N = (1, 63, 64, 65, 1000)


def reduce_chunk_counts(groups):
    """The edges of train_reduce_batch_kernel's loop, which covers four chunk groups per trip: one chunk; one short of a full trip (the
    tail clamp `cc < it.chunks ? cc : c` in its last slot); exactly one trip; one chunk into the second."""
    return (1, 4 * groups - 1, 4 * groups, 4 * groups + 1)


def _run_reduce(dev, row, kw):
    """A FULL queue (`first[]` of every slot is used) of independent reductions in one launch: item i sums `chunks` partial rows of n
    floats, `stride` floats apart; every third item splits its row at n0 between two outputs.  The outputs start out poisoned, so every
    element must be written; the reference is the float64 sum of the partial rows."""
    probe = torch.zeros(1, device=dev)
    lib, st = train._rt(probe)
    groups = _lib.REDUCE_GROUPS[lib.esmi_backend().decode()]
    counts = reduce_chunk_counts(groups)
    q = _lib.ReduceQueue()
    keep, want, pairs = [], [], set()
    for i in range(_lib.REDUCE_QUEUE_ITEMS):
        n, chunks = REDUCE_N[i % len(REDUCE_N)], counts[(i // len(REDUCE_N)) % len(counts)]
        pairs.add((n, chunks))
        stride = n + 3 * (i % 2)
        part = _rand(chunks, stride, seed=100 + i)
        split = i % 3 == 0
        n0 = n // 2 if split else -1
        out = torch.full((n,), float("nan"), device=dev)
        out1 = torch.full((n,), float("nan"), device=dev) if split else None
        pd = part.to(dev).contiguous()
        keep.append((pd, out, out1))
        q.items[i] = _lib.ReduceItem(_ptr(pd), n, stride, chunks, _ptr(out), n0, _ptr(out1))
        want.append((part.double()[:, :n].sum(0), n0, chunks))
    q.count = _lib.REDUCE_QUEUE_ITEMS
    assert len(pairs) == len(REDUCE_N) * len(counts)             # every n at every chunk count
    lib.esmi_train_reduce_flush_f32(C.byref(q), st)
    assert q.count == 0
    perturb, figures = kw.get("perturb"), kw.get("figures")
    worst = 0.0
    for i, ((pd, out, out1), (ref, n0, chunks)) in enumerate(zip(keep, want)):
        got = out.cpu() if n0 < 0 else torch.cat([out.cpu()[:n0], out1.cpu()[: ref.numel() - n0]])
        if n0 >= 0:                                              # ... and nothing is written outside either segment
            assert bool(torch.isnan(out.cpu()[n0:]).all()) and bool(torch.isnan(out1.cpu()[ref.numel() - n0:]).all()), (row.id, i)
        if perturb is not None:
            got = perturb(f"item {i}", got.clone())
        assert bool(torch.isfinite(got).all()), (row.id, i, "an element was not written")
        e = _err(got, ref)
        worst = max(worst, e)
        assert e < GRAD, (row.id, i, ref.numel(), chunks, e)
    e32 = max(_err(pd.float()[:, : ref.numel()].sum(0), ref) for (pd, _, _), (ref, _, _) in zip(keep, want))
    print(f"    {row.id} sums ({groups} groups, chunk counts {counts}): worst {worst:.3e} (bound {GRAD:.1e}; torch fp32 {e32:.3e})")
    if figures is not None:
        figures.append((row.id, "sums", worst, GRAD, e32))


_RUN = {"attn": _run_attn, "lin1": _run_lin1, "ln": _run_ln, "conv": _run_conv, "repeat": _run_repeat, "copy_cols": _run_copy_cols,
        "reduce": _run_reduce}


def run_row(dev, row, perturb=None, figures=None):
    """Run one row on `dev` and assert its bounds.  figures: a list that receives (row id, tensor, error, bound, torch fp32's error)."""
    old = train.USE_MATRIX_PIPE
    try:
        if row.matrix_pipe is not None:
            train.USE_MATRIX_PIPE = row.matrix_pipe
        print(f"  {row.id}: {row.op} {row.shape} {' '.join(row.opt)}")
        _RUN[row.op](dev, row, dict(perturb=perturb, figures=figures))
    finally:
        train.USE_MATRIX_PIPE = old


# ------------------------------------------------------------------------------------------------------------------- the table
_ATTN_GLOBAL = ("train_attn_fwd_kernel", "train_attn_bwd_rows_kernel", "train_attn_bwd_cols_kernel")
_ATTN_LDS = ("train_attn_fwd_lds_kernel", "train_attn_bwd_rows_lds_kernel", "train_attn_bwd_cols_kernel")
_LN_FWD4 = tuple(f"train_ln_fwd4_kernel<{l}>" for l in (8, 16, 32, 64))
_LN_BWD4 = tuple(f"train_ln_bwd4_kernel<{l}>" for l in (8, 16, 32))
_LIN1_4 = tuple(f"train_lin1_bwd4_kernel<{l}>" for l in (4, 8, 16, 32, 64))


def _attn(B, N, Cc, h, lds):
    return Row(f"attn_B{B}_N{N}_C{Cc}_h{h}", "attn", (B, N, Cc, h), _ATTN_LDS if lds else _ATTN_GLOBAL, (_ATTN_GLOBAL if lds else _ATTN_LDS)[:2])


def _lin1(cin, B, n, lpr, *opt):
    must = (f"train_lin1_bwd4_kernel<{lpr}>",) if lpr else ("train_lin1_bwd_kernel",)
    absent = tuple(k for k in _LIN1_4 + ("train_lin1_bwd_kernel",) if k not in must)
    return Row("_".join((f"lin1_c{cin}",) + opt), "lin1", (cin, B, n), must + ("conv_to1_kernel", "train_reduce_chunks_kernel"), absent, True, opt)


def _ln(rows, Cc, fwd, bwd, *opt):
    must = (fwd,) + ((bwd,) if isinstance(bwd, str) else bwd) + ("train_reduce_chunks_kernel",)
    every = _LN_FWD4 + _LN_BWD4 + ("train_ln_fwd_kernel", "train_ln_bwd_fused_kernel", "train_ln_bwd_dx_kernel", "train_ln_bwd_params_kernel")
    return Row("_".join((f"ln_{rows}x{Cc}",) + opt), "ln", (rows, Cc), must, tuple(k for k in every if k not in must), None, opt)


_GENERIC, _FUSED, _TWO_PASS = "train_ln_fwd_kernel", "train_ln_bwd_fused_kernel", ("train_ln_bwd_dx_kernel", "train_ln_bwd_params_kernel")
_LN_ROWS = [_ln(70, 256, "train_ln_fwd4_kernel<64>", _FUSED),           # base's C = 256 norms
            _ln(70, 48, _GENERIC, _FUSED), _ln(70, 50, _GENERIC, _FUSED),
            _ln(300, 320, _GENERIC, _TWO_PASS),                         # two row chunks of the dx / params pair
            _ln(70, 128, _GENERIC, _FUSED, "offset"),                   # the generic kernels at a width the 16-byte ones own
            _ln(1, 32, "train_ln_fwd4_kernel<8>", "train_ln_bwd4_kernel<8>"),
            _ln(63, 64, "train_ln_fwd4_kernel<16>", "train_ln_bwd4_kernel<16>"),
            _ln(65, 64, "train_ln_fwd4_kernel<16>", "train_ln_bwd4_kernel<16>"),
            _ln(129, 128, "train_ln_fwd4_kernel<32>", "train_ln_bwd4_kernel<32>")]
for _v in ("res_mask_relu", "tanh_mask_relu"):      # the arguments that take other code in the generic kernels
    _LN_ROWS += [_ln(70, 256, "train_ln_fwd4_kernel<64>", _FUSED, _v), _ln(70, 50, _GENERIC, _FUSED, _v), _ln(70, 128, _GENERIC, _FUSED, "offset", _v)]

_PLAIN = ("train_conv_fwd_kernel", "train_conv_dgrad_kernel")
_DW = ("train_conv_dw_kernel",)
_WG, _WG_DW, _WG_DW4, _WG_MFMA = "train_conv_wgrad_kernel", "train_conv_wgrad_dw_kernel", "train_conv_wgrad_dw4_kernel", "train_conv_wgrad_mfma_kernel<false>"
_CONVS = [  # (c_in, c_out, k, stride, pad, groups, B, n), the kernels at either setting of USE_MATRIX_PIPE, the alternatives
    ((32, 64, 3, 1, 1, 4, 2, 21), _PLAIN + (_WG, "train_colsum_kernel"), _DW + (_WG_DW, _WG_DW4, _WG_MFMA)),      # grouped, not depthwise
    ((32, 32, 3, 2, 1, 32, 2, 21), _PLAIN + (_WG_DW,), _DW + (_WG, _WG_DW4, _WG_MFMA)),                          # depthwise, stride 2
    ((30, 30, 3, 1, 1, 30, 2, 21), _PLAIN + (_WG_DW,), _DW + (_WG, _WG_DW4, _WG_MFMA)),                          # depthwise, C % 4 != 0
    ((32, 32, 7, 1, 3, 32, 2, 21), _DW + (_WG_DW4,), _PLAIN + (_WG, _WG_DW, _WG_MFMA)),                          # the widest wgrad_dw4 takes
    ((32, 32, 8, 1, 3, 32, 2, 21), _DW + (_WG_DW,), _PLAIN + (_WG, _WG_DW4, _WG_MFMA)),                          # k <= 8, n_out != n_in
    ((32, 32, 9, 1, 4, 32, 2, 21), _PLAIN + (_WG, "train_colsum_kernel"), _DW + (_WG_DW, _WG_DW4, _WG_MFMA)),     # depthwise k = 9: the grouped path
    ((8, 8, 3, 1, 1, 1, 5, 16), (_WG_MFMA,), (_WG, _WG_DW, _WG_DW4)),                                            # the matrix-pipe weight gradient's floor
    ((8, 12, 3, 1, 1, 1, 5, 17), (_WG_MFMA,), (_WG, _WG_DW, _WG_DW4)),                                           # an utterance boundary inside nearly every 16-row trip
    ((128, 128, 5, 1, 2, 1, 1, 16), (_WG_MFMA,), (_WG, _WG_DW, _WG_DW4)),
]


def _conv_rows():
    out = []
    for shape, must, absent in _CONVS:
        for pipe in (True, False):
            dense = shape[5] == 1
            # a dense shape runs the plain forward / data gradient without the GEMMs -- and the plain data gradient with them where
            # c_out, the data-gradient GEMM's contraction length, is no multiple of 8 (c_out = 12)
            gemm = tuple(pipe and dense and c % 8 == 0 for c in shape[:2])
            more = tuple(k for k, on in zip(_PLAIN, gemm) if not on) if dense else ()
            less = tuple(k for k, on in zip(_PLAIN, gemm) if on)
            cid = "conv_cin{0}_cout{1}_k{2}_s{3}_g{5}_n{7}_".format(*shape) + ("pipe" if pipe else "plain")
            out.append(Row(cid, "conv", shape, must + more + ("train_reduce_chunks_kernel",), absent + less, pipe))
    return out


ROWS = [
    _attn(1, 147, 128, 2, False),       # base stage 0 at its threshold: N (2C + 6) = 38514 > 38400
    _attn(1, 75, 256, 4, False),        # base stage 1 at its threshold
    _attn(1, 30, 640, 1, False),        # global pair with N < 64: lanes 30 .. 63 own no key (the -3.0e38f start of the max reduction)
    _attn(1, 146, 128, 2, True),        # the last shape of the LDS pair: 149.7 KiB, the limit raised
    _attn(1, 130, 64, 2, True),         # LDS pair at 68 KiB
    _attn(1, 1, 8, 1, True), _attn(2, 17, 32, 2, True),     # one row; two row segments
    _attn(260, 4, 8, 4, True),          # B h > 1024: one row segment per (utterance, head)
    _lin1(16, 1, 5, 4), _lin1(32, 2, 33, 8), _lin1(64, 2, 32, 16), _lin1(128, 1, 31, 32), _lin1(256, 1, 33, 64),
    _lin1(48, 3, 21, 0),
    _lin1(32, 2, 33, 0, "offset"),      # the misaligned fall-back at a width the 16-byte kernel owns
    _lin1(64, 2, 32, 16, "nobias"),
    *_LN_ROWS,
    *_conv_rows(),
    Row("repeat_C6", "repeat", (3, 50, 6), ("train_repeat_fwd_kernel", "train_repeat_bwd_kernel"), ("train_repeat_fwd4_kernel",)),
    Row("repeat_C8_offset", "repeat", (3, 50, 8), ("train_repeat_fwd_kernel", "train_repeat_bwd_kernel"), ("train_repeat_fwd4_kernel",), None, ("offset",)),
    Row("copy_cols", "copy_cols", (7, 2, 5, 1, 3, 300), ("train_copy_cols_kernel",)),
    Row("reduce_batch", "reduce", (), ("train_reduce_batch_kernel",), ("train_reduce_chunks_kernel",)),
]
BY_ID = {r.id: r for r in ROWS}
assert len(BY_ID) == len(ROWS)

# The template instantiations tu_train.hip launches: the completeness test adds them to the `__global__` names of train_ops.h.
INSTANTIATIONS = {"train_ln_fwd4_kernel": (8, 16, 32, 64), "train_ln_bwd4_kernel": (8, 16, 32), "train_lin1_bwd4_kernel": (4, 8, 16, 32, 64),
                  "train_conv_wgrad_mfma_kernel": ("true", "false")}

# Kernels of train_ops.h whose test lives elsewhere: kernel -> an existing test that launches it (checked with launched_kernels() when
# the entry was written; the completeness test only checks that the test id exists).  Where the table reaches a kernel, the table counts.
_OPS = "tests/test_train_ops.py::test_simulated_layernorm_attention_loss"
COVERED_ELSEWHERE = {
    "train_conv_wgrad_mfma_kernel<true>": "tests/test_train_ops.py::test_simulated_conv_forward_and_gradients[cin64_cout32_k3_s2_g1_T]",
    "train_act_fwd_kernel": _OPS, "train_act_bwd_kernel": _OPS,
    "train_embed_fwd_kernel": _OPS, "train_embed_bwd_kernel": _OPS,
    "train_mask_rows_kernel": _OPS, "train_add_kernel": _OPS, "train_cat_kernel": _OPS, "train_repeat_fwd4_kernel": _OPS,
    "train_loss_partial_kernel": _OPS, "train_loss_final_kernel": _OPS, "train_loss_grad_kernel": _OPS,
    "train_adamw_kernel": _OPS,
    "train_pack_batch_kernel": "tests/test_grad_clip.py::test_clipped_step_adds_exactly_the_reduction_launch[32]",
    "train_bump_step_kernel": "tests/test_grad_clip.py::test_clipped_step_adds_exactly_the_reduction_launch[32]",
    "train_adamw_dev_kernel": "tests/test_grad_clip.py::test_simulated_clipped_optimizer_launch_matches_torch",
    "train_grad_sumsq_kernel": "tests/test_grad_clip.py::test_simulated_clipped_optimizer_launch_matches_torch",
    "train_bump_clip_kernel": "tests/test_grad_clip.py::test_simulated_clipped_optimizer_launch_matches_torch",
}
