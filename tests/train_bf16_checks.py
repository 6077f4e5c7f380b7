"""Check bodies of tests/test_train_bf16.py: the training step's bf16-mixed precision (`TrainStep(precision="bf16")`,
ESMI_PRECISION_BF16).  Every body takes the device ("cuda", or "cpu" inside `on_sim`) and is run by a simulator test and a `gpu` test.

The model of the arithmetic is tests/test_train_gemm_at_size.py's rounded-operand model with bfloat16 in place of binary16 and
nothing scaled: forward and data-gradient GEMMs contract `x.bfloat16()`, `w.bfloat16()`, `dy.bfloat16()` (round to nearest even) with
fp32 accumulation.  A product of two bfloat16 values is exact in fp32, so against the fp64 contraction of the rounded operands only
the accumulation error is left and the project's fp32 bounds apply (FWD 2e-5, GRAD 5e-5, CHAIN 1e-4 behind an activation +
LayerNorm); the weight and bias gradients do not round and go against the unrounded reference.  MATTERS: the error against the
unrounded reference is at least 10 x the error against the model -- otherwise the bf16 kernel was not the one launched."""
import contextlib
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import tests.test_train_gemm_at_size as G
from efficientspeech_amd import train
from efficientspeech_amd.networks import _ptr
from tests.test_train_gemm_at_size import CHAIN, FWD, GRAD, LN_VARIANTS, MATTERS, _check, _conv_inputs, _conv_ref, _err, _geom, _guarded, _rand

GOLD_BF16 = os.path.join(os.path.dirname(__file__), "golden", "tiny_train_step_bf16.npz")      # tools/gen_golden_train.py --bf16


def bf16_context():
    return train._step_context("bf16", False)


@contextlib.contextmanager
def on_sim(expect=()):
    """Run a body on host tensors through the simulator build; `expect`: kernels that must be among those it launched."""
    from tests.simlib import launched_kernels, use_sim
    old, G.DEV = G.DEV, "cpu"
    try:
        with use_sim(), launched_kernels() as names:
            yield names
    finally:
        G.DEV = old
    for k in expect:
        assert k in names, (k, sorted(set(names)))


def _rb(t):
    """bfloat16 round-to-nearest-even, as float64"""
    return t.detach().float().bfloat16().double()


def _matters(got, rounded, unrounded, what):
    e_r, e_u = _err(got, rounded), _err(got, unrounded)
    print(f"    {what}: vs unrounded {e_u:.3e} = {e_u / max(e_r, 1e-30):.0f} x the rounded-operand model's {e_r:.3e}")
    assert e_u >= MATTERS * e_r, (what, "the rounded-operand model does not matter: was the bf16 kernel launched?", e_u, e_r)


def conv_refs(x, w, b, dy, geom):
    """fp64: y / dx by the bf16 rounded-operand model, y0 / dx0 unrounded, dw / db unrounded."""
    x64, w64, b64, dy64 = (t.detach().double() for t in (x, w, b, dy))
    fwd = lambda xx, ww, bb: _conv_ref(xx, ww, bb, *geom)      # noqa: E731

    def dgrad(ww, dd):
        xl = torch.zeros_like(x64).requires_grad_()
        return torch.autograd.grad(fwd(xl, ww, None), xl, dd)[0]
    wl, bl = w64.clone().requires_grad_(), b64.clone().requires_grad_()
    dw, db = torch.autograd.grad(fwd(x64, wl, bl), (wl, bl), dy64)
    return {"y": fwd(_rb(x), _rb(w), b64), "dx": dgrad(_rb(w), _rb(dy)), "y0": fwd(x64, w64, b64), "dx0": dgrad(w64, dy64), "dw": dw, "db": db}


# ------------------------------------------------------------------------------------------------------ 1. operator level
def check_conv(cfg):
    """One dense convolution through `train._Conv` under bf16: forward and data gradient against the rounded-operand model, weight and
    bias gradient against the unrounded reference.  cfg = (c_in, c_out, k, stride, pad, transposed, B, n)."""
    geom = _geom(cfg)
    x, w, b = _conv_inputs(cfg)
    print(f"  conv {cfg} bf16")
    with bf16_context():
        got = train._Conv.apply(x, w, b, cfg[3], cfg[4], 1, cfg[5], geom[4])
        dy = _rand(*got.shape, seed=4)
        gx, gw, gb = torch.autograd.grad(got, (x, w, b), dy)
    r = conv_refs(x, w, b, dy, geom)
    _check(got, r["y"], FWD, "forward")
    _check(gx, r["dx"], GRAD, "dgrad")
    _check(gw, r["dw"], GRAD, "wgrad")
    _check(gb, r["db"], GRAD, "bias grad")
    _matters(got, r["y"], r["y0"], "forward")
    _matters(gx, r["dx"], r["dx0"], "dgrad")


def check_conv_ln(cin, cout, B, n, variant):
    """A Linear c_in -> c_out with the LayerNorm behind it (`train._ConvLN`: one launch up to 128 output channels, conv + norm launches
    at 256) and its backward, as tests/test_train_gemm_at_size.check_conv_ln has it: the Linear's operands rounded to bfloat16,
    everything behind it in fp64; the convolution's gradients are referred to the gradient that ENTERED its backward (the LayerNorm
    backward's own output, re-run on the saved tensors), so the rounded-operand model stays exact."""
    act, use_res, use_mask, relu_out = LN_VARIANTS[variant]
    rows = B * n
    dev = G.DEV
    print(f"  conv_ln {cin}->{cout} rows={rows} {variant} bf16")
    x = _rand(B, n, cin, seed=11).requires_grad_()
    w = (_rand(cout, cin, seed=12) * (1.0 / np.sqrt(cin))).requires_grad_()
    b = _rand(cout, seed=13).requires_grad_()
    g, beta = (_rand(cout, seed=14) + 1.0).requires_grad_(), _rand(cout, seed=15).requires_grad_()
    res = _rand(B, n, cout, seed=16).requires_grad_() if use_res else None
    r_idx = torch.arange(rows, device=dev)
    mask = ((r_idx % 7 == 3) | (r_idx >= rows - 5)).view(B, n) if use_mask else None
    m8 = mask.to(torch.uint8).contiguous() if use_mask else None
    dy = _rand(B, n, cout, seed=17)
    ins = (x, w, b, g, beta) + ((res,) if use_res else ())
    with bf16_context():
        got = train._ConvLN.apply(x, w, b, 0, 1, act, g, beta, res, m8, relu_out)
        saved = got.grad_fn.saved_tensors
        grads = torch.autograd.grad(got, ins, dy)
    gx, gw, gb, gg, gbeta = grads[:5]
    geom = (1, 1, 0, False, n)
    x64, w64, b64 = x.detach().double(), w.detach().double(), b.detach().double()
    lin = lambda xx, ww: _conv_ref(xx, ww, b64, *geom)      # noqa: E731
    c = lin(_rb(x), _rb(w)).requires_grad_()
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
    _matters(got, y, epilogue(lin(x64, w64), check_gate=False), "forward")
    bound = CHAIN if chain else GRAD
    _check(gg, dg, bound, "dgamma")
    _check(gbeta, dbeta, bound, "dbeta")
    with bf16_context():
        dc_in = train._layer_norm_backward(*train._rt(dy), *saved[2:], dy.contiguous(), act, g, beta)[0].detach()
    if use_res:
        assert torch.equal(dc_in, grads[5])
    _check(dc_in, dc, bound, "the LayerNorm backward's dx")
    r = conv_refs(x, w, b, dc_in, geom)
    _check(gx, r["dx"], GRAD, "dgrad")
    _check(gw, r["dw"], GRAD, "wgrad")
    _check(gb, r["db"], GRAD, "bias grad")
    _matters(gx, r["dx"], r["dx0"], "dgrad")


def check_ragged_tile_stays_in_bounds(cin, cout, B, n, ln):
    """The ragged last tile through the C ABI with every output inside a poisoned buffer: nothing is written outside the tensors, and
    what is written follows the bf16 model."""
    print(f"  guarded {cin}->{cout} rows={B * n} bf16 ln={ln}")
    x, w, b = (t.detach() for t in _conv_inputs((cin, cout, 1, 1, 0, False, B, n)))
    geom = (1, 1, 0, False, n)
    lib, st = train._rt(x)
    checks = []

    def out(*shape):
        t, ok = _guarded(*shape)
        checks.append(ok)
        return t
    with bf16_context():
        d, ws, nws = train._conv_desc(lib, x, w, w, n, 1, 0, 1, False, 0)
    from efficientspeech_amd import _lib
    assert d.precision == _lib.PRECISION_BF16
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
    wsb = torch.empty((nbw,), dtype=torch.uint8, device=G.DEV)
    lib.esmi_train_conv_bwd_f32(C.byref(d), _ptr(x), _ptr(dy), _ptr(w), _ptr(dx), _ptr(dw), _ptr(db), _ptr(wsb), nbw, None, st)
    assert all(ok() for ok in checks), "a kernel wrote outside its output tensor"
    r = conv_refs(x, w, b, dy, geom)
    if ln:
        pre = r["y"] + res.double()
        _check(y_pre, pre, FWD, "pre-norm tensor")
        _check(y, F.layer_norm(pre, (cout,), g.double(), beta.double()), FWD, "forward")
        _check(mean, pre.mean(-1).reshape(-1), FWD, "mean")
        _check(rstd, (pre.var(-1, unbiased=False) + 1e-5).rsqrt().reshape(-1), FWD, "rstd")
    else:
        _check(y, r["y"], FWD, "forward")
        _matters(y, r["y"], r["y0"], "forward")
    _check(dx, r["dx"], GRAD, "dgrad")
    _check(dw, r["dw"], GRAD, "wgrad")
    _check(db, r["db"], GRAD, "bias grad")
    _matters(dx, r["dx"], r["dx0"], "dgrad")


# ------------------------------------------------------------------------------------------------------ 2. the rounding is RNE
def _with_ties(t, seed):
    """t with a quarter of its elements moved onto exact bfloat16 ties: low 16 bits 0x8000, half of them above an even bfloat16
    neighbour (bit 16 clear: the tie rounds down), half above an odd one (bit 16 set: it rounds up)."""
    bits = t.detach().cpu().contiguous().view(torch.int32).clone().flatten()
    g = torch.Generator().manual_seed(seed)
    pick = torch.randperm(bits.numel(), generator=g)[: bits.numel() // 4]
    odd = torch.arange(pick.numel()) % 2 == 1
    tie = (bits[pick] & ~0xFFFF) | 0x8000
    tie = torch.where(odd, tie | 0x10000, tie & ~0x10000)
    bits[pick] = tie
    out = bits.view(torch.float32).view(t.shape)
    assert int(((out.view(torch.int32) & 0xFFFF) == 0x8000).sum()) >= pick.numel()
    return out.to(t.device)


def check_rounding_is_rne(cfg):
    """Arbitrary fp32 operands (with exact ties, both directions) and the same operands pre-rounded by torch's `.bfloat16().float()`
    give bit-identical y and dx: the kernels round to nearest even, and round nothing else."""
    geom = _geom(cfg)
    x, w, b = _conv_inputs(cfg)
    x, w = _with_ties(x, 21), _with_ties(w, 22)
    b = b.detach()
    n_odd = int((((x.cpu().view(torch.int32) >> 16) & 1) == 1).logical_and((x.cpu().view(torch.int32) & 0xFFFF) == 0x8000).sum())
    n_even = int((((x.cpu().view(torch.int32) >> 16) & 1) == 0).logical_and((x.cpu().view(torch.int32) & 0xFFFF) == 0x8000).sum())
    assert n_odd > 0 and n_even > 0

    def run(xx, ww, dy):
        xx, ww = xx.clone().requires_grad_(), ww.clone().requires_grad_()
        with bf16_context():
            y = train._Conv.apply(xx, ww, b, cfg[3], cfg[4], 1, cfg[5], geom[4])
            d = dy(y.shape)
            return y.detach(), torch.autograd.grad(y, xx, d)[0]
    dy_raw = lambda shape: _with_ties(_rand(*shape, seed=4), 23)      # noqa: E731
    rb = lambda t: t.bfloat16().float()                                # noqa: E731
    y0, dx0 = run(x, w, dy_raw)
    y1, dx1 = run(rb(x), rb(w), lambda shape: rb(dy_raw(shape)))
    assert not torch.equal(rb(x), x)
    assert torch.equal(y0, y1), (cfg, "forward", _err(y0, y1))
    assert torch.equal(dx0, dx1), (cfg, "dgrad", _err(dx0, dx1))


# ------------------------------------------------------------------------------ 3. one step against the reference's bf16 run
def check_step_against_reference(dev):
    """`TrainStep(precision="bf16")` against the reference's own step under torch.autocast(bfloat16) (tiny_train_step_bf16.npz), in
    the form of tests/test_train_step.check_precision16_step.  Every bar comes from the fixtures: the reference's bf16 run against
    its fp32 run (tiny_train_step.npz), and the ratio r of that distance to the binary16 run's (tiny_train_step_amp16.npz)."""
    from tests.test_train_step import GOLD, GOLD_AMP, _setup
    tr, g, net, x, y = _setup(dev, GOLD_BF16)
    f32, f16 = np.load(GOLD), np.load(GOLD_AMP)
    step = tr.TrainStep(net, lr=1e-3, weight_decay=1e-6, precision="bf16")
    losses = step.step(x, y).cpu().numpy().astype(np.float64)
    assert step.skipped == 0 and step.scale == 1.0 and step.t == 1
    # losses: 2.5 x the reference's own bf16-vs-fp32 distance (the precision-16 test's 1e-3 stands in that ratio to its 4e-4)
    ref_l = np.append(g["losses"], float(g["total"]))
    ref_l32 = np.append(f32["losses"], float(f32["total"]))
    bar_l = 2.5 * float((np.abs(g["losses"] - f32["losses"]) / np.abs(f32["losses"])).max())
    rel = np.abs(losses - ref_l) / np.abs(ref_l)
    print(f"  losses {losses.tolist()}\n  vs the bf16 fixture: {rel.tolist()} (bar {bar_l:.3e}; the fixture vs fp32 {(np.abs(ref_l - ref_l32) / np.abs(ref_l32)).tolist()})")
    named = dict(net.named_parameters())

    def d_ref_of(fix):
        out = {}
        for k in fix.files:
            if k.startswith("grad.") and k in f32.files:
                a, b32 = fix[k].astype(np.float64).ravel(), f32[k].astype(np.float64).ravel()
                out[k] = np.abs(a - b32).max() / max(1e-9, np.abs(a).max())
        return out
    d_bf, d_f16 = d_ref_of(g), d_ref_of(f16)
    r = float(np.median(list(d_bf.values())) / np.median(list(d_f16.values())))
    n, rows, ref_cos = 0, [], []
    for k in g.files:
        if not k.startswith("grad."):
            continue
        ref = g[k].astype(np.float64).ravel()
        mine = named[k[5:]].grad.detach().cpu().numpy().astype(np.float64).ravel()        # (seeded with 1: nothing to unscale)
        scale = max(1e-9, np.abs(ref).max())
        cos = None
        if ref.size >= 32 and np.linalg.norm(ref) > 1e-6 * ref.size ** 0.5:
            cos = float(mine @ ref / (np.linalg.norm(mine) * np.linalg.norm(ref) + 1e-30))
            if k in f32.files:
                r32 = f32[k].astype(np.float64).ravel()
                ref_cos.append(float(ref @ r32 / (np.linalg.norm(ref) * np.linalg.norm(r32) + 1e-30)))
        excess = None
        if k in f32.files:
            excess = np.abs(mine - ref).max() / scale - max(d_bf[k], 2e-3 * r)
        rows.append((k, cos, excess))
        n += 1
    bar_cos = 2.0 * (1.0 - min(ref_cos))
    worst_cos = min(c for _, c, _ in rows if c is not None)
    worst_excess = max((e, k) for k, _, e in rows if e is not None)
    print(f"  {n} tensors; r = {r:.3f} (median d_ref bf16 {np.median(list(d_bf.values())):.4f}, f16 {np.median(list(d_f16.values())):.4f})")
    print(f"  worst cosine {worst_cos:.4f} (the reference's bf16 vs fp32: {min(ref_cos):.4f}; bar 1 - cos <= {bar_cos:.4f})")
    print(f"  worst d_mine - max(d_ref, 2e-3 r) = {worst_excess[0]:.4f} at {worst_excess[1]} (bar {0.05 * r:.4f})")
    assert float(rel.max()) <= bar_l, (losses, ref_l, bar_l)
    assert n >= 60
    for k, cos, _ in rows:
        assert cos is None or 1.0 - cos <= bar_cos, (k, cos, bar_cos)
    assert worst_excess[0] < 0.05 * r, (worst_excess, r)


# ------------------------------------------------------------------------------------------------------------ 4. mechanics
def check_mechanics(dev):
    """No scaler state; the update is AdamW on our own gradients; two fresh steps are bitwise equal; checkpoint -> resume continues
    bitwise; "bf16-mixed" is the same precision; anything else is refused."""
    from tests.test_train_step import _setup
    tr, g, net, x, y = _setup(dev, GOLD_BF16)
    step = tr.TrainStep(net, lr=1e-3, weight_decay=1e-6, precision="bf16-mixed")
    assert step.precision == "bf16"
    opt = step._opt                                   # no scaler block, no absmax slot, and (eager) nothing else in device memory either
    assert isinstance(opt, tr.AdamWState) and opt.scaler is None and opt.absmax is None and not opt.on_device and opt.hyper is None
    with pytest.raises(AttributeError, match="no loss scaler"):
        step.growth_interval
    before = {k: p.detach().clone() for k, p in net.named_parameters()}
    first = step.step(x, y).clone()
    assert step.scale == 1.0 and step.skipped == 0 and step.t == 1 and "scaler" not in step.state_dict()
    # the update: torch's AdamW on a copy of the weights with OUR gradients (the flat buffer still holds them), the project's 2e-6
    names = step.flat.names
    named = dict(net.named_parameters())
    copies = {k: before[k].cpu().clone().requires_grad_() for k in names}
    opt = torch.optim.AdamW([copies[k] for k in names], lr=1e-3, weight_decay=1e-6)
    for k in names:
        copies[k].grad = named[k].grad.detach().cpu().clone()
    opt.step()
    for k in names:
        d = float((named[k].detach().cpu() - copies[k].detach()).abs().max())
        assert d < 2e-6, (k, d)
    assert any(float((named[k].detach() - before[k]).abs().max()) > 5e-4 for k in names)
    # reproducible, and resume continues bitwise
    second = step.step(x, y).clone()
    ckpt = step.state_dict()
    third = step.step(x, y).clone()
    t2, _, net2, x2, y2 = _setup(dev, GOLD_BF16)
    other = t2.TrainStep(net2, lr=1e-3, weight_decay=1e-6, precision="bf16")
    assert torch.equal(other.step(x2, y2), first) and torch.equal(other.step(x2, y2), second)
    t3, _, net3, x3, y3 = _setup(dev, GOLD_BF16)
    resumed = t3.TrainStep(net3, lr=1e-3, weight_decay=1e-6, precision="bf16")
    resumed.load_state_dict(dict(ckpt, scaler={"scale": 4.0, "growth_factor": 2.0, "backoff_factor": 0.5, "growth_interval": 7, "_growth_tracker": 1}))
    assert resumed.t == 2 and resumed.scale == 1.0                     # (a checkpoint's scaler entry is ignored, as at precision 32)
    assert torch.equal(resumed.step(x3, y3), third) and torch.equal(resumed.flat.data, step.flat.data) and resumed.t == 3
    for bad in (8, "fp8", "bf16-true", True):
        try:
            tr.TrainStep(net3, precision=bad)
        except ValueError:
            continue
        raise AssertionError(f"precision {bad!r} was accepted")


def check_inference_sees_the_update(dev, steps):
    """Packed copies: an eval forward after bf16 training equals a fresh net loaded from state_dict().  -> (first, last) loss."""
    from efficientspeech_amd import CONFIGS, build_phoneme2mel
    from tests.test_train_step import _setup
    tr, g, net, x, y = _setup(dev, GOLD_BF16)
    xe = {"phoneme": x["phoneme"], "phoneme_mask": x["phoneme_mask"], "duration_forced": x["duration"]}
    net.eval()
    with torch.no_grad():
        before = net(xe)[0].clone()
    net.train()
    step = tr.TrainStep(net, lr=1e-3, precision="bf16")
    first = last = float(step.step(x, y)[4])
    for _ in range(steps - 1):
        last = float(step.step(x, y)[4])
    assert step.skipped == 0 and step.t == steps
    net.eval()
    with torch.no_grad():
        after = net(xe)[0].clone()
    fresh = build_phoneme2mel(CONFIGS["tiny"])
    fresh.load_state_dict({k: v.detach().cpu().clone() for k, v in net.state_dict().items()}, strict=True)
    fresh = fresh.to(dev).eval()
    with torch.no_grad():
        want = fresh(xe)[0]
    assert float((after - before).abs().max()) > 1e-3
    assert torch.equal(after, want), float((after - want).abs().max())
    return first, last


def check_abi_refuses_other_precisions(dev):
    """Any esmi_conv_desc.precision but 0 / 32 / 16 / ESMI_PRECISION_BF16 is ESMI_ERR_ARG with nothing written."""
    from efficientspeech_amd import _lib
    x, w, b = (t.detach() for t in _conv_inputs((32, 32, 1, 1, 0, False, 1, 8)))
    lib, st = train._rt(x)
    y = torch.full((1, 8, 32), -7.0, device=G.DEV)
    for prec in (8, 0xB15, 0xB17, -16):
        d = _lib.ConvDesc(1, 8, 32, 8, 32, 1, 1, 0, 1, 0, prec, 0)
        assert lib.esmi_train_conv_workspace_bytes(C.byref(d)) == 0
        try:
            lib.esmi_train_conv_fwd_f32(C.byref(d), _ptr(x), _ptr(w), _ptr(b), _ptr(y), None, 0, st)
        except RuntimeError as e:   # (the binding raises on a non-zero status; not the Unsupported subclass: ESMI_ERR_ARG)
            assert not isinstance(e, _lib.Unsupported), e
        else:
            raise AssertionError(f"precision {prec} was accepted")
    assert bool((y == -7.0).all())
