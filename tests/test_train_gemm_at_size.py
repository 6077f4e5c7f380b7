"""The training step's implicit-GEMM kernels at the sizes the benchmark launches them, against an fp64 contraction.

`launch_convgemm` (csrc/tu_convgemm.hip) picks a kernel family by row count: `pwgemm_kernel` from 32,768 rows, `convgemm_dma_kernel` from
2,048 rows (MT = 2 from ~131,000), `convgemm_kernel` below -- on the device; on the wave simulator both thresholds are 1.  The cases of
tests/test_train_ops.py stop at 3,500 rows, so this module runs every `pwgemm_kernel` instantiation at 32,768 .. 76,800 rows (the
benchmark's B = 128 x 600 frames), the other two families under `precision = 16`, the data gradient's power-of-two operand scale away
from O(1), and one whole step at the benchmark's shape against the fp64 mirror.  Small twins of the operator checks run on the simulator.

Reference models (which one applies is said per case):
  * fp32 kernels (split-f16 products, fp32-accurate): the fp64 contraction of the operands as given.
  * `precision = 16` GEMMs (`pwgemm_kernel<.,.,true>`, `convgemm_dma_kernel<.,.,.,true,.>`, `convgemm_kernel<.,true>`): the ROUNDED-OPERAND
    model -- activations `x.half()`, weights `(256 w).half() / 256`, the data gradient's input `(s dy).half() / s` with
    s = 2^(9 - floor(log2 max|dy|)); a product of two binary16 values is exact in fp32, so only the fp32 accumulation error is left and
    the fp32 bounds apply.  Every such case also shows that the model matters: the error against the UNROUNDED reference is at
    least 10 x the error against the rounded one -- otherwise the AMP kernel was not the one launched.
  * what does not round under `precision = 16` (the weight and bias gradients -- always split-bf16 --, `conv_to1_kernel`, depthwise, the
    plain kernels): the unrounded reference.
Bounds are the project's: 2e-5 forward, 5e-5 gradients, 1e-4 through an activation + LayerNorm chain (tests/test_train_ops.py)."""
import contextlib
import ctypes as C
import math
import time

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from efficientspeech_amd import train
from efficientspeech_amd.networks import _ptr

gpu = pytest.mark.gpu
DEV = "cuda"
FWD, GRAD, CHAIN = 2e-5, 5e-5, 1e-4
# GRAD also holds for the sums over all rows (weight, bias, LayerNorm parameter gradients) at benchmark size -- measured on the device at
# 32,768 .. 131,072 rows: the kernels' weight gradient 4e-7 .. 7e-7, bias gradient <= 2e-7, dgamma / dbeta <= 4e-7 against fp64; torch's
# own fp32 operator (matmul) on the same inputs 4.1e-6 .. 7.1e-6 (weight), <= 3.1e-7 (bias), so 4 x its error stays below 5e-5 too.
# The worst figures are the 131,072-row cases of OTHER_FAMILIES: the kernels' 6.8e-7 at `dma_k5_mt2`, torch's 7.1e-6 at `dma_k3_mt2`
# (pytest -s prints every figure before it asserts).
MATTERS = 10.0            # error vs the unrounded reference / error vs the rounded-operand model, at least


def _rand(*shape, seed=0, scale=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(DEV)


def _err(a, b):
    a, b = a.detach().double(), b.detach().double()
    return float((a - b).abs().max()) / max(1e-6, float(b.abs().max()))


def _check(got, ref, bound, what):
    """The project's `_close` (max error relative to the reference's largest magnitude), printing the figure before it asserts."""
    e = _err(got, ref)
    print(f"    {what}: {e:.3e} (bound {bound:.1e})")
    assert bool(torch.isfinite(got).all()), (what, "not finite")
    assert e < bound, (what, e, bound)
    return e


def _matters(got, rounded, unrounded, what):
    e_r, e_u = _err(got, rounded), _err(got, unrounded)
    print(f"    {what}: vs unrounded {e_u:.3e} = {e_u / max(e_r, 1e-30):.0f} x the rounded-operand model's {e_r:.3e}")
    assert e_u >= MATTERS * e_r, (what, "the rounded-operand model does not matter: was the AMP kernel launched?", e_u, e_r)


def _precision(amp):
    return train._step_context(16, False) if amp else contextlib.nullcontext()


# ----------------------------------------------------------------------------------------------------------- the fp64 reference
def _r16(t, mult=1.0):
    """binary16 round-to-nearest-even of mult * t (mult a power of two: exact in fp32), divided back, as float64."""
    return (t.float() * mult).half().double() / mult


def _dy_scale(dy):
    """convgemm.h conv_pow2_scales: the power of two that puts max|dy| into [2^9, 2^10); 1 for an all-zero tensor."""
    m = float(dy.abs().max())
    return 1.0 if m == 0.0 else 2.0 ** (9 - (math.frexp(m)[1] - 1))


def _conv_ref(x, w, b, k, stride, pad, transposed, n_out):
    """Conv1d / ConvTranspose1d (cropped to n_out) / Linear on channels-last x as a sum of shifted matmuls, in x's dtype; w in
    checkpoint layout ((c_out, c_in, k), Linear (c_out, c_in), transposed (c_in, c_out, k))."""
    w = w if w.dim() == 3 else w.unsqueeze(-1)
    B, n, _ = x.shape
    if not transposed:
        xp = F.pad(x, (0, 0, pad, pad))
        y = sum(xp[:, j: j + stride * (n_out - 1) + 1: stride] @ w[:, :, j].T for j in range(k))
    else:
        taps = [F.pad((x @ w[:, :, j]).unsqueeze(2), (0, 0, 0, stride - 1)).reshape(B, n * stride, -1) for j in range(k)]   # row i -> i * stride
        y = sum(F.pad(t, (0, 0, j, k - j)) for j, t in enumerate(taps))[:, pad: pad + n_out]
    return y if b is None else y + b


def _conv_refs(x, w, b, dy, geom, amp):
    """Forward and the three gradients of one convolution in fp64 -> dict(y, dx, dw, db); under `amp` y and dx follow the
    rounded-operand model and y0 / dx0 keep the unrounded ones."""
    x64, w64, b64, dy64 = (t.detach().double() for t in (x, w, b, dy))
    fwd = lambda xx, ww, bb: _conv_ref(xx, ww, bb, *geom)      # noqa: E731

    def dgrad(ww, dd):
        xl = torch.zeros_like(x64).requires_grad_()
        return torch.autograd.grad(fwd(xl, ww, None), xl, dd)[0]
    wl, bl = w64.clone().requires_grad_(), b64.clone().requires_grad_()
    dw, db = torch.autograd.grad(fwd(x64, wl, bl), (wl, bl), dy64)
    out = {"y": fwd(x64, w64, b64), "dx": dgrad(w64, dy64), "dw": dw, "db": db}
    if amp:
        rw = _r16(w64, 256.0)
        out["y0"], out["dx0"] = out["y"], out["dx"]
        out["y"], out["dx"] = fwd(_r16(x64), rw, b64), dgrad(rw, _r16(dy64, _dy_scale(dy64)))
    return out


def _geom(cfg):
    cin, cout, k, s, p, tr, B, n = cfg
    n_out = min((n - 1) * s - 2 * p + k, 2 * n) if tr else (n + 2 * p - k) // s + 1
    return (k, s, p, tr, n_out)


def _conv_inputs(cfg, seed=0):
    cin, cout, k, s, p, tr, B, n = cfg
    x = _rand(B, n, cin, seed=seed + 1).requires_grad_()
    w = (_rand(cin, cout, k, seed=seed + 2) if tr else (_rand(cout, cin, k, seed=seed + 2) if k > 1 else _rand(cout, cin, seed=seed + 2))) * (1.0 / np.sqrt(cin * k))
    return x, w.detach().requires_grad_(), _rand(cout, seed=seed + 3).requires_grad_()


def check_conv(cfg, amp, dy_of=None):
    """One dense convolution through `train._Conv`: forward, data gradient, weight gradient, bias gradient against the fp64 reference
    (`amp`: the rounded-operand model for forward and data gradient, the unrounded one for the two parameter gradients).
    cfg = (c_in, c_out, k, stride, pad, transposed, B, n); dy_of(shape) -> the incoming gradient (default N(0, 1))."""
    geom = _geom(cfg)
    x, w, b = _conv_inputs(cfg)
    print(f"  conv {cfg} amp={amp}")
    with _precision(amp):
        got = train._Conv.apply(x, w, b, cfg[3], cfg[4], 1, cfg[5], geom[4])
        dy = _rand(*got.shape, seed=4) if dy_of is None else dy_of(got.shape)
        gx, gw, gb = torch.autograd.grad(got, (x, w, b), dy)
    r = _conv_refs(x, w, b, dy, geom, amp)
    _check(got, r["y"], FWD, "forward")
    _check(gx, r["dx"], GRAD, "dgrad")
    _check(gw, r["dw"], GRAD, "wgrad")
    _check(gb, r["db"], GRAD, "bias grad")
    if amp:
        _matters(got, r["y"], r["y0"], "forward")
        _matters(gx, r["dx"], r["dx0"], "dgrad")
    return got, gx, gw, gb


# ------------------------------------------------------------------------------------------ conv + LayerNorm in one launch (_ConvLN)
LN_VARIANTS = {   # name -> (act, residual, row mask, ReLU output)
    "tanh": (train.ACT_TANH, False, False, False),          # the mel decoder's LN(tanh(Linear(x)))
    "res_mask": (0, True, True, False),                     # the encoder's LN(Linear(x) + x), padded rows zeroed
    "relu_out_mask": (0, False, True, True),                # relu(LN(.)) with the row mask: the predictor's epilogue
    "relu_relu_out": (train.ACT_RELU, False, True, True),   # the predictor's relu(LN(relu(.))): small (simulator) sizes only -- at 10^7
    #                                                         elements some pre-activation sits within rounding of the first ReLU's kink
}


def check_conv_ln(cin, B, n, variant, amp):
    """A Linear c_in -> 128 with the LayerNorm epilogue (`esmi_train_conv_ln_fwd_f32`; `pwgemm_kernel<8|5, 4, amp>` from 32,768 rows) and
    its backward (LayerNorm backward kernel, then the convolution's two gradients: `<8, 2>` / a 128 -> c_in data gradient).
    Model: pre = act(Linear(x)) + res with the Linear's operands rounded under `amp`; LayerNorm, ReLU, row mask in fp64.  The gate of
    the output ReLU is taken from the kernel's own output (a LayerNorm output within rounding of zero may legitimately fall on either
    side; it must agree with fp64 wherever |LN| > 1e-5).  The LayerNorm backward's dx is checked against fp64 on its own; the
    convolution's gradients are then referred to the gradient that actually ENTERED the convolution's backward -- the LayerNorm
    backward kernel's output, re-run here on the tensors the forward saved (with a residual it is also the residual's gradient:
    asserted bitwise equal) -- so the rounded-operand model stays exact.  (Referred to the fp64 dx instead, a binary16 rounding that
    flips on the fp32 kernel's last bit costs one binary16 ulp of that element: 1.1e-4 .. 2.6e-4 of max|dx| was measured on the
    device at 32,768 .. 76,800 rows for a data gradient whose error against its true input is 2e-7.)"""
    act, use_res, use_mask, relu_out = LN_VARIANTS[variant]
    cout, rows = 128, B * n
    print(f"  conv_ln {cin}->{cout} rows={rows} {variant} amp={amp}")
    x = _rand(B, n, cin, seed=11).requires_grad_()
    w = (_rand(cout, cin, seed=12) * (1.0 / np.sqrt(cin))).requires_grad_()
    b = _rand(cout, seed=13).requires_grad_()
    g, beta = (_rand(cout, seed=14) + 1.0).requires_grad_(), _rand(cout, seed=15).requires_grad_()
    res = _rand(B, n, cout, seed=16).requires_grad_() if use_res else None
    r_idx = torch.arange(rows, device=DEV)
    mask = ((r_idx % 7 == 3) | (r_idx >= rows - 5)).view(B, n) if use_mask else None
    m8 = mask.to(torch.uint8).contiguous() if use_mask else None
    dy = _rand(B, n, cout, seed=17)
    ins = (x, w, b, g, beta) + ((res,) if use_res else ())
    with _precision(amp):
        got = train._ConvLN.apply(x, w, b, 0, 1, act, g, beta, res, m8, relu_out)
        saved = got.grad_fn.saved_tensors                   # (x, w, pre-norm tensor, gamma, mean, rstd, row mask, ReLU output)
        grads = torch.autograd.grad(got, ins, dy)
    gx, gw, gb, gg, gbeta = grads[:5]
    # ---- fp64 model of the forward, and of the LayerNorm's backward
    geom = (1, 1, 0, False, n)
    x64, w64, b64 = x.detach().double(), w.detach().double(), b.detach().double()
    lin = lambda xx, ww: _conv_ref(xx, ww, b64, *geom)      # noqa: E731
    c = (lin(_r16(x64), _r16(w64, 256.0)) if amp else lin(x64, w64)).requires_grad_()
    g64, beta64 = g.detach().double().requires_grad_(), beta.detach().double().requires_grad_()

    def epilogue(c_, check_gate=True):
        a = torch.tanh(c_) if act == train.ACT_TANH else (F.relu(c_) if act == train.ACT_RELU else c_)
        ln = F.layer_norm(a + res.detach().double() if use_res else a, (cout,), g64, beta64)
        y_ = ln
        if relu_out:
            gate = (got.detach() > 0).double()
            clear = ln.detach().abs() > 1e-5
            if use_mask:
                clear = clear & ~mask[..., None]
            assert not check_gate or bool(((ln.detach() > 0).double() == gate)[clear].all()), "the output ReLU's gate differs from fp64 away from the kink"
            y_ = ln * gate
        return y_.masked_fill(mask[..., None], 0.0) if use_mask else y_
    y = epilogue(c)
    dc, dg, dbeta = torch.autograd.grad(y, (c, g64, beta64), dy.double())
    chain = bool(act) or relu_out
    _check(got, y, CHAIN if chain else FWD, "forward")
    if amp:
        y0 = epilogue(lin(x64, w64), check_gate=False)
        _matters(got, y, y0, "forward")
    bound = CHAIN if chain else GRAD
    _check(gg, dg, bound, "dgamma")
    _check(gbeta, dbeta, bound, "dbeta")
    with _precision(amp):
        dc_in, dc_again = (train._layer_norm_backward(*train._rt(dy), *saved[2:], dy.contiguous(), act, g, beta)[0].detach() for _ in range(2))
    assert torch.equal(dc_in, dc_again), "the LayerNorm backward's dx does not repeat bitwise: its re-run is no stand-in for the step's"
    if use_res:
        assert torch.equal(dc_in, grads[5])
    _check(dc_in, dc, bound, "the LayerNorm backward's dx")
    r = _conv_refs(x, w, b, dc_in, geom, amp)
    _check(gx, r["dx"], GRAD, "dgrad")
    _check(gw, r["dw"], GRAD, "wgrad")
    _check(gb, r["db"], GRAD, "bias grad")
    if amp:
        _matters(gx, r["dx"], r["dx0"], "dgrad")


# ------------------------------------------------------------------------------------- 2. pwgemm on the device, every instantiation
# rows as (B, n): the threshold exactly; threshold + 33 as ONE utterance (ragged last tile); the benchmark's 128 x 600; 65,631 =
# 32 x 2,050 + 31 rows (2,051 row tiles on 2,048 waves: waves walk unequal numbers of items, and the last tile is ragged)
PW_ROWS = [(4, 8192), (1, 32768 + 33), (128, 600), (3, 21877)]
_ids_rows = [f"rows{B * n}" for B, n in PW_ROWS]


@gpu
@pytest.mark.parametrize("amp", [False, True], ids=["fp32", "amp"])
@pytest.mark.parametrize("rows", PW_ROWS, ids=_ids_rows)
@pytest.mark.parametrize("cout", [128, 80])
def test_pwgemm_linear_at_size(cout, rows, amp):
    """`train._Conv` Linear 128 -> 128: forward and data gradient both `pwgemm_kernel<8, 2, amp>`.  128 -> 80 (mel_linear): forward
    `<8, 2, amp>` with a half-empty last column tile, data gradient `<5, 2, amp>` (80 -> 128).  amp: rounded-operand model."""
    check_conv((128, cout, 1, 1, 0, False) + rows, amp)


@gpu
@pytest.mark.parametrize("amp", [False, True], ids=["fp32", "amp"])
@pytest.mark.parametrize("rows", PW_ROWS, ids=_ids_rows)
@pytest.mark.parametrize("variant", ["tanh", "res_mask", "relu_out_mask"])
def test_pwgemm_layernorm_epilogue_at_size(variant, rows, amp):
    """`train._ConvLN` 128 -> 128: `pwgemm_kernel<8, 4, amp>` with the LayerNorm epilogue, with and without residual, row mask and ReLU
    output.  amp: rounded-operand model for the Linear, fp64 for everything behind it."""
    check_conv_ln(128, *rows, variant, amp)


@gpu
@pytest.mark.parametrize("amp", [False, True], ids=["fp32", "amp"])
@pytest.mark.parametrize("rows", PW_ROWS, ids=_ids_rows)
@pytest.mark.parametrize("variant", ["tanh", "res_mask"])
def test_pwgemm_80_to_128_layernorm_epilogue_at_size(variant, rows, amp):
    """80 -> 128 with the LayerNorm epilogue: `pwgemm_kernel<5, 4, amp>` -- the model never launches it, but it is compiled and reachable
    through the ABI.  (Its data gradient is a 128 -> 80 problem: `<8, 2, amp>`.)"""
    check_conv_ln(80, *rows, variant, amp)


POISON = -12345.678


def _guarded(*shape):
    """A tensor inside a larger poisoned buffer -> (tensor, intact()): 4,096 floats on either side, more than a whole 32-row tile."""
    n, pad = int(np.prod(shape)), 4096
    big = torch.full((n + 2 * pad,), POISON, device=DEV)
    return big[pad:pad + n].view(*shape), lambda: bool((big[:pad] == POISON).all()) and bool((big[pad + n:] == POISON).all())


def check_ragged_tile_stays_in_bounds(cin, cout, B, n, amp, ln):
    """The ragged last tile through the C ABI with every output inside a poisoned buffer: nothing is written before the first or past
    the last row, and what is written is right (the same models as above)."""
    from efficientspeech_amd import _lib
    print(f"  guarded {cin}->{cout} rows={B * n} amp={amp} ln={ln}")
    x, w, b = (t.detach() for t in _conv_inputs((cin, cout, 1, 1, 0, False, B, n)))
    geom = (1, 1, 0, False, n)
    lib, st = train._rt(x)
    checks = []

    def out(*shape):
        t, ok = _guarded(*shape)
        checks.append(ok)
        return t
    with _precision(amp):
        d, ws, nws = train._conv_desc(lib, x, w, w, n, 1, 0, 1, False, 0)
    y = out(B, n, cout)
    if ln:
        g, beta, res = _rand(cout, seed=14) + 1.0, _rand(cout, seed=15), _rand(B, n, cout, seed=16)
        y_pre, mean, rstd = out(B, n, cout), out(B * n), out(B * n)
        lib.esmi_train_conv_ln_fwd_f32(C.byref(d), _ptr(x), _ptr(w), _ptr(b), _ptr(res), _ptr(g), _ptr(beta), None, 0, _ptr(y_pre), _ptr(y),
                                       _ptr(mean), _ptr(rstd), _ptr(ws), nws, st)
    else:
        lib.esmi_train_conv_fwd_f32(C.byref(d), _ptr(x), _ptr(w), _ptr(b), _ptr(y), _ptr(ws), nws, st)
    dy = _rand(B, n, cout, seed=4)
    dx, dw, db = out(B, n, cin), out(*w.shape), out(cout)
    nbw = lib.esmi_train_conv_bwd_workspace_bytes(C.byref(d))
    wsb = torch.empty((nbw,), dtype=torch.uint8, device=DEV)
    lib.esmi_train_conv_bwd_f32(C.byref(d), _ptr(x), _ptr(dy), _ptr(w), _ptr(dx), _ptr(dw), _ptr(db), _ptr(wsb), nbw, None, st)
    assert all(ok() for ok in checks), "a kernel wrote outside its output tensor"
    r = _conv_refs(x, w, b, dy, geom, amp)
    if ln:
        pre = r["y"] + res.double()
        _check(y_pre, pre, FWD, "pre-norm tensor")
        _check(y, F.layer_norm(pre, (cout,), g.double(), beta.double()), FWD, "forward")
        _check(mean, pre.mean(-1).reshape(-1), FWD, "mean")
        _check(rstd, (pre.var(-1, unbiased=False) + 1e-5).rsqrt().reshape(-1), FWD, "rstd")
    else:
        _check(y, r["y"], FWD, "forward")
        if amp:
            _matters(y, r["y"], r["y0"], "forward")
    _check(dx, r["dx"], GRAD, "dgrad")
    _check(dw, r["dw"], GRAD, "wgrad")
    _check(db, r["db"], GRAD, "bias grad")
    if amp:
        _matters(dx, r["dx"], r["dx0"], "dgrad")


@gpu
@pytest.mark.parametrize("amp", [False, True], ids=["fp32", "amp"])
@pytest.mark.parametrize("cin,cout,ln", [(128, 128, False), (128, 80, False), (128, 128, True), (80, 128, True)],
                         ids=["128to128", "128to80", "128to128_ln", "80to128_ln"])
def test_pwgemm_ragged_last_tile_writes_nothing_past_the_end(cin, cout, ln, amp):
    """32,768 + 33 rows as one utterance: the last 32-row tile holds one row; the rows behind it are buffer loads that read zero and
    stores that must not happen.  All four (KS, NT) shapes of `pwgemm_kernel`, both precisions."""
    check_ragged_tile_stays_in_bounds(cin, cout, 1, 32768 + 33, amp, ln)


# ------------------------------------------------------------------------------------------- 3. the other two families under AMP
# (c_in, c_out, k, stride, pad, transposed, B, n) -> the kernel the data flow takes on the device.  All GEMM kernels: rounded-operand
# model under amp.  The fp32 twins run too: test_train_ops.CONVS has no k > 1 shape above 2,048 rows, and none that keeps
# `convgemm_kernel` at 2 or 4 column tiles (below 1,024 row tiles the dispatch narrows them to 1).
OTHER_FAMILIES = [
    ((128, 128, 3, 1, 1, False, 4, 600), "dma_k3_mt1"),         # 2,400 rows: convgemm_dma_kernel<4, 1, ...>
    ((128, 128, 5, 1, 2, False, 4, 600), "dma_k5_mt1"),
    ((128, 128, 3, 1, 1, False, 256, 512), "dma_k3_mt2"),       # 131,072 rows: convgemm_dma_kernel<4, 2, ...>
    ((128, 128, 5, 1, 2, False, 256, 512), "dma_k5_mt2"),
    ((128, 128, 3, 2, 1, False, 4, 131), "stride2_odd_nt1"),    # convgemm_kernel<1>: strided conv, odd length; its data gradient MODE_CONVT
    ((128, 128, 3, 2, 0, True, 4, 64), "convT_crop_nt1"),       # ConvTranspose1d cropped to 2n
    ((40, 24, 3, 1, 1, False, 2, 50), "cin40_nt1"),             # c_in = 40: one full 32-channel step and a quarter one
    ((128, 128, 3, 2, 1, False, 8, 4099), "stride2_odd_nt2"),   # 520 row tiles: convgemm_kernel<2>
    ((128, 128, 3, 2, 1, False, 16, 4099), "stride2_odd_nt4"),  # 1,040 row tiles: convgemm_kernel<4>
    ((128, 128, 3, 2, 0, True, 8, 2048), "convT_crop_nt4"),     # 1,024 row tiles over the two phases: convgemm_kernel<4>, MODE_CONVT
]


@gpu
@pytest.mark.parametrize("amp", [False, True], ids=["fp32", "amp"])
@pytest.mark.parametrize("cfg", [c for c, _ in OTHER_FAMILIES], ids=[i for _, i in OTHER_FAMILIES])
def test_dma_and_streaming_gemm_families(cfg, amp):
    check_conv(cfg, amp)


# ----------------------------------------------------------------------------- 4. the data gradient's operand scale, both precisions
def _wgrad_chunk(rows, cin, cout, k):
    """Rows per wave of train_conv_wgrad_mfma_kernel (tu_train.hip wgrad_plan): the kernel that leaves max|dy| behind as a side effect."""
    tiles = ((cout + 127) // 128) * ((cin + 31) // 32) * k
    want = (rows * tiles + 2048 * 16 - 1) // (2048 * 16)
    return 16 * min(max(want, 1), 64)


def check_scale_equivariance(cfg, amp):
    """(a) dy scaled by 2^-40, 2^-20, 2^20: the operand scale adapts by the same power of two, so dx is the unscaled dx times that
    power BITWISE.  (c) all-zero dy: exactly zero dx and dw."""
    geom = _geom(cfg)
    x, w, b = _conv_inputs(cfg)
    with _precision(amp):
        got = train._Conv.apply(x, w, b, cfg[3], cfg[4], 1, cfg[5], geom[4])
        dy = _rand(*got.shape, seed=4)
        base = torch.autograd.grad(got, x, dy, retain_graph=True)[0]
        assert float(base.abs().max()) > 0
        for e in (-40, -20, 20):
            gx = torch.autograd.grad(got, x, dy * 2.0 ** e, retain_graph=True)[0]
            assert torch.equal(gx, base * 2.0 ** e), (cfg, amp, e, _err(gx, base * 2.0 ** e))
        gx, gw = torch.autograd.grad(got, (x, w), torch.zeros_like(dy))
        assert float(gx.abs().max()) == 0.0 and float(gw.abs().max()) == 0.0


def check_spike_positions(cfg, amp):
    """(b) a spike of 2^10 x the rest of dy wherever the maximum could be missed: dx stays finite and inside the bound.  A scale
    formed without the spike is 2^10 too large: the spike leaves binary16's range."""
    cin, cout, k, s, p, tr, B, n = cfg
    geom = _geom(cfg)
    rows, chunk = B * geom[4], _wgrad_chunk(B * geom[4], cin, cout, k)
    spots = {"first row": (0, 1), "last row": (rows - 1, 2), "last row of a weight-gradient chunk": (chunk - 1, 3), "first row after it": (chunk, 5),
             "last row of a workgroup's four chunks": (4 * chunk - 1, 7), "a column >= 64": (rows // 2, min(cout - 1, 77))}
    if cout > 96:
        spots["a column >= 96"] = (rows // 3, 101)
    for what, (r_, c_) in spots.items():
        assert 0 <= r_ < rows

        def dy_of(shape, r_=r_, c_=c_):
            dy = _rand(*shape, seed=4)
            dy.view(-1, cout)[r_, c_] = 1024.0 * float(dy.abs().max())
            return dy
        print(f"  spike at {what}")
        check_conv(cfg, amp, dy_of=dy_of)


def check_padded_tile_ignores_what_lies_outside(cfg, amp):
    """The 80-wide dy is read in 128-column tiles: columns 80 .. 127 of the last row would lie past the tensor.  dy sits in a larger
    buffer whose tail holds 2^30: picked up, it would push every real value out of binary16's range (the result collapses)."""
    geom = _geom(cfg)

    def dy_of(shape):
        dy = _rand(*shape, seed=4)
        big = torch.cat([dy.flatten(), torch.full((4096,), 2.0 ** 30, device=DEV)])
        return big[:dy.numel()].view(shape)
    assert cfg[1] == 80
    check_conv(cfg, amp, dy_of=dy_of)


SCALE_SHAPES = [((128, 80, 1, 1, 0, False, 1, 32768 + 33), "pwgemm_128to80"), ((128, 128, 3, 1, 1, False, 4, 600), "dma_k3")]


@gpu
@pytest.mark.parametrize("amp", [False, True], ids=["fp32", "amp"])
@pytest.mark.parametrize("cfg", [c for c, _ in SCALE_SHAPES], ids=[i for _, i in SCALE_SHAPES])
def test_dgrad_operand_scale(cfg, amp):
    check_scale_equivariance(cfg, amp)
    check_spike_positions(cfg, amp)
    if cfg[1] == 80:
        check_padded_tile_ignores_what_lies_outside(cfg, amp)


# ------------------------------------------------------------------------- 5. one step at the benchmark's shape against the fp64 mirror
BENCH_B, BENCH_T, BENCH_D = 128, 100, 6       # tools/bench_train.py, `bench.py --full`'s train_step leg: 76,800 decoder rows
# (fallback, if the fp64 mirror ever needs more than ~5 minutes on 16 CPUs: B = 64, 38,400 rows, still above the 32,768 threshold.
#  Measured: 10 s at B = 128 -- no need.)
NUDGE_NEAR, NUDGE_TO, NUDGE_CAP = 1e-3, 2e-3, 1e-3
# parameters outside the decoder whose gradient reaches them through no ReLU (embedding rows gathered into the decoder's input; the
# duration predictor's second norm, whose output is a decoder feature): held to the decoder's bounds
NO_RELU_PARAMS = ("encoder.pitch_decoder.pitch_embedding.weight", "encoder.energy_decoder.energy_embedding.weight",
                  "encoder.duration_decoder.norm2.weight", "encoder.duration_decoder.norm2.bias")


def benchmark_shape_reference(B=BENCH_B):
    """The fp64 mirror (tests/torch_mirror.py, CPU) on `train.synthetic_batch(B, 100, 6)`, tiny ES.  The L1 loss's |.| has 6.1 M inputs
    here, so no seed keeps them all off the kink: the forward (which does not depend on the target) runs first, and every target
    element within 1e-3 of the prediction is moved to prediction +- 2e-3.  -> (cfg, sd, x, y (nudged, fp32), losses [4 parts, total],
    {name: grad}, share of targets moved, seconds)."""
    from efficientspeech_amd import CONFIGS, build_phoneme2mel
    from efficientspeech_amd.synth import synth_state_dict
    from tests import torch_mirror as M
    t0 = time.time()
    cfg = CONFIGS["tiny"]
    sd = synth_state_dict(cfg, 1234)
    x, y = train.synthetic_batch(B, BENCH_T, BENCH_D, "cpu")
    net = build_phoneme2mel(cfg)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    net = net.double().train()
    for k, p in net.named_parameters():
        p.requires_grad_(not k.endswith("_bins"))
    x64 = {k: (v.double() if v.is_floating_point() else v) for k, v in x.items()}
    out = M.train_forward(net, dict(x64, mel=y["mel"].double()))
    pred = out["mel"].detach()
    diff = y["mel"].double() - pred
    near = diff.abs() < NUDGE_NEAR
    mel = torch.where(near, pred + torch.where(diff >= 0, NUDGE_TO, -NUDGE_TO), y["mel"].double()).float()
    assert float((mel.double() - pred).abs().min()) > 0.9 * NUDGE_NEAR
    y = {"mel": mel}
    parts, total = M.loss(out, x64, {"mel": mel.double()})
    total.backward()
    grads = {k: (None if p.grad is None else p.grad.clone()) for k, p in net.named_parameters()}
    return cfg, sd, x, y, [float(p.detach()) for p in parts] + [float(total.detach())], grads, float(near.double().mean()), time.time() - t0


@gpu
def test_step_at_benchmark_shape_matches_fp64_mirror():
    """One forward + backward of tiny ES at B = 128 x 100 phonemes x D = 6 (the `train_step` leg of `bench.py --full`, 76,800 decoder
    rows: ten decoder GEMMs per step in `pwgemm_kernel`) against the fp64 mirror, with `USE_MATRIX_PIPE` on and off: the four loss
    parts and the total within 2e-5 relative; every `decoder.*` gradient, and NO_RELU_PARAMS, within SPLIT_BOUND / FP32_BOUND (the
    bounds of test_train_step.check_gradients_at_size).  Then one `TrainStep(precision=16, init_scale=2048)` step on the same batch:
    not skipped, losses within the AMP fixture test's rtol = 1e-3 of the fp64 losses.

    Encoder and predictor parameters are deliberately left out: their gradients pass ten ReLUs over 1.6 M inputs (some input is
    within rounding of a kink whatever the seed), their kernels run at 12,800 rows, which the operator cases cover, and
    check_gradients_at_size checks their composition on margin-checked seeds.

    Measured (16 CPU threads): the mirror's forward + backward takes 10 s; share of nudged targets 2.6e-5 (the cap 1e-3 is no measurement)."""
    from efficientspeech_amd import build_phoneme2mel
    from tests.test_train_step import FP32_BOUND, SPLIT_BOUND
    cfg, sd, x, y, ref_losses, ref, share, secs = benchmark_shape_reference()
    print(f"  fp64 mirror: {secs:.1f} s; share of targets nudged {share:.2e}; losses {ref_losses}")
    assert share <= NUDGE_CAP, share
    assert all(ref[k] is not None for k in NO_RELU_PARAMS)

    def fresh():
        net = build_phoneme2mel(cfg)
        net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
        return net.to(DEV).train()
    xd, yd = ({k: v.to(DEV) for k, v in d.items()} for d in (x, y))
    net = fresh()
    old = train.USE_MATRIX_PIPE
    try:
        for matrix_pipe, bound in ((False, FP32_BOUND), (True, SPLIT_BOUND)):
            train.USE_MATRIX_PIPE = matrix_pipe
            for p in net.parameters():
                p.grad = None
            parts, total = train.training_loss(net, xd, yd)
            total.backward()
            losses = train.loss_vector(parts, total).double().cpu().tolist()
            print(f"  matrix_pipe={matrix_pipe}: losses {losses}")
            for a, r in zip(losses, ref_losses):
                assert abs(a - r) < 2e-5 * abs(r), (matrix_pipe, losses, ref_losses)
            errs = []
            for k, p in net.named_parameters():
                if k.startswith("decoder.") or k in NO_RELU_PARAMS:
                    errs.append((_err(p.grad.cpu(), ref[k]), k))
            assert len(errs) >= 20 + len(NO_RELU_PARAMS), len(errs)
            print(f"  matrix_pipe={matrix_pipe}: worst gradients {sorted(errs)[-3:]} (bound {bound:.0e})")
            assert max(errs)[0] < bound, (matrix_pipe, sorted(errs)[-5:])
    finally:
        train.USE_MATRIX_PIPE = old
    step = train.TrainStep(fresh(), lr=1e-3, weight_decay=1e-6, precision=16, init_scale=2048.0)
    losses = step.step(xd, yd).double().cpu().numpy()
    print(f"  precision 16: losses {losses.tolist()}")
    assert step.skipped == 0
    assert np.allclose(losses[:4], ref_losses[:4], rtol=1e-3, atol=1e-5), (losses, ref_losses)
    assert abs(losses[4] - ref_losses[4]) < 1e-3 * ref_losses[4]


# ------------------------------------------------------------------------------------------ 6. the same checks on the wave simulator
# (thresholds 1: every k = 1 shape with 128 / 80 input channels and 65 .. 128 output channels takes pwgemm_kernel, every other stride-1
# shape with c_in % 32 == 0 and c_out > 64 convgemm_dma_kernel.)  The CPU tier's first operator-level check of `precision = 16`.
def _on_sim(fn, expect=()):
    """Run a check body on host tensors through the simulator build; `expect`: kernels that must be among those it launched."""
    import tests.test_train_gemm_at_size as me
    from tests.simlib import launched_kernels, use_sim
    old = me.DEV
    me.DEV = "cpu"
    try:
        with use_sim(), launched_kernels() as names:
            fn()
    finally:
        me.DEV = old
    for k in expect:
        assert k in names, (k, sorted(set(names)))


_nowarn = pytest.mark.filterwarnings("ignore")
SIM_AMP_CONVS = [   # (cfg, id, kernels the simulator must have launched)
    ((128, 128, 1, 1, 0, False, 1, 70), "128to128", ("pwgemm_kernel<8,2,true>",)),
    ((128, 80, 1, 1, 0, False, 2, 45), "128to80", ("pwgemm_kernel<8,2,true>", "pwgemm_kernel<5,2,true>")),
    ((128, 128, 3, 1, 1, False, 2, 37), "dma_k3", ("convgemm_dma_kernel<4,1,NWV,true,false>",)),
    ((32, 32, 3, 1, 1, False, 2, 37), "cin32_k3", ("convgemm_kernel<1,true>",)),
    ((32, 64, 3, 2, 1, False, 2, 19), "stride2_odd", ("convgemm_kernel<1,true>",)),
    ((64, 32, 3, 2, 0, True, 2, 9), "convT_crop", ("convgemm_kernel<1,true>",)),
    ((40, 24, 3, 1, 1, False, 1, 11), "cin40", ("convgemm_kernel<1,true>",)),
]


@_nowarn
@pytest.mark.parametrize("cfg,expect", [(c, e) for c, _, e in SIM_AMP_CONVS], ids=[i for _, i, _ in SIM_AMP_CONVS])
def test_simulated_amp_conv_matches_rounded_operand_model(cfg, expect):
    _on_sim(lambda: check_conv(cfg, True), expect)


@_nowarn
@pytest.mark.parametrize("cin,variant,amp,expect", [
    (128, "tanh", True, "pwgemm_kernel<8,4,true>"), (128, "res_mask", True, "pwgemm_kernel<8,4,true>"),
    (128, "relu_out_mask", True, "pwgemm_kernel<8,4,true>"), (128, "relu_relu_out", True, "pwgemm_kernel<8,4,true>"),
    (128, "res_mask", False, "pwgemm_kernel<8,4,false>"),
    (80, "res_mask", True, "pwgemm_kernel<5,4,true>"), (80, "tanh", False, "pwgemm_kernel<5,4,false>")])
def test_simulated_layernorm_epilogue_variants(cin, variant, amp, expect):
    _on_sim(lambda: check_conv_ln(cin, 2, 35, variant, amp), (expect,))


@_nowarn
@pytest.mark.parametrize("amp", [False, True], ids=["fp32", "amp"])
def test_simulated_ragged_last_tile_writes_nothing_past_the_end(amp):
    _on_sim(lambda: (check_ragged_tile_stays_in_bounds(128, 80, 1, 33, amp, False), check_ragged_tile_stays_in_bounds(80, 128, 1, 33, amp, True)),
            ("pwgemm_kernel<8,2,%s>" % str(amp).lower(), "pwgemm_kernel<5,4,%s>" % str(amp).lower()))


SIM_SCALE_SHAPES = [((128, 80, 1, 1, 0, False, 1, 70), "pwgemm_128to80"), ((128, 128, 3, 1, 1, False, 2, 37), "dma_k3")]


@_nowarn
@pytest.mark.parametrize("amp", [False, True], ids=["fp32", "amp"])
@pytest.mark.parametrize("cfg", [c for c, _ in SIM_SCALE_SHAPES], ids=[i for _, i in SIM_SCALE_SHAPES])
def test_simulated_dgrad_operand_scale(cfg, amp):
    _on_sim(lambda: test_dgrad_operand_scale(cfg, amp), ("train_conv_wgrad_mfma_kernel<false>",))


def test_conv_reference_matches_torch_operators():
    """The shifted-matmul reference itself against torch's conv1d / conv_transpose1d in float64 on the CPU, every geometry used above."""
    for cfg in [c for c, _ in OTHER_FAMILIES[4:7]] + [(8, 8, 5, 1, 2, False, 2, 9), (8, 16, 1, 1, 0, False, 2, 5)]:
        cin, cout, k, s, p, tr, B, n = cfg
        g = torch.Generator().manual_seed(3)
        x = torch.randn(B, min(n, 21), cin, generator=g, dtype=torch.float64)
        w = torch.randn((cin, cout, k) if tr else (cout, cin, k), generator=g, dtype=torch.float64)
        b = torch.randn(cout, generator=g, dtype=torch.float64)
        geom = _geom((cin, cout, k, s, p, tr, B, x.shape[1]))
        if tr:
            ref = F.conv_transpose1d(x.transpose(1, 2), w, b, stride=s, padding=p)[:, :, :geom[4]].transpose(1, 2)
        else:
            ref = F.conv1d(x.transpose(1, 2), w, b, stride=s, padding=p).transpose(1, 2)
        assert _err(_conv_ref(x, w if k > 1 else w[:, :, 0], b, *geom), ref) < 1e-13, cfg
