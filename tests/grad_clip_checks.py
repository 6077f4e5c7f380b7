"""Checks of the training step's opt-in gradient-norm clipping (`TrainStep(gradient_clip_val=)`, esmi_train_grad_sumsq_f32,
esmi_train_adamw_clip_f32), shared by the GPU tier and the wave-simulator tier of tests/test_grad_clip.py.  Every check takes the device
("cuda", or "cpu" inside `use_sim()`).  The reference throughout is torch's own pair: torch.nn.utils.clip_grad_norm_(params, c, 2)
followed by torch.optim.AdamW, on float64 CPU copies (`torch_clip_adamw`).

Tolerances (each relative to the tensor's largest magnitude), from the arithmetic:
  norm     1e-6   the squares are exact in double and so is the sum to 1e-16; sqrt, the division by the loss scale and the rounding to
                  fp32 leave 6e-8.  (An fp32 square would cost 2^-24 per term, 1.2e-7 on the norm: the bound is 8x that.)
  m        1e-5   the coefficient carries the norm's error plus two fp32 roundings (the quotient, and coef / scale rounded once), the
                  moment one product and one fused update more: a few 2^-24 = 6e-8 each
  v        2e-5   the gradient enters squared: twice m's
  weights  rtol 1e-4, atol 1e-6: the project's device-versus-host pair (tests/test_train_step.py)
"""
import functools
import types

import numpy as np
import torch

from tests.test_train_step import _setup

LR, BETAS, EPS, WD = 1e-3, (0.9, 0.999), 1e-8, 1e-6
NORM_RTOL, M_TOL, V_TOL = 1e-6, 1e-5, 2e-5
PARTIALS = 1024                 # ESMI_TRAIN_GRAD_NORM_PARTIALS (tests/test_grad_clip.py compares it with _lib's mirror)
SIZES = (1, 3, 4, 5, 1003, 4 * 256 * 2 + 3)                    # both tiers; the last: two workgroups and a three-element tail
SIZE_SECOND_TRIP = 1024 * 256 * 4 + 1028 + 3                   # GPU: the grid-stride loop's second trip, a tail that is no multiple of 4


def _rt(t):
    from efficientspeech_amd import train
    return train._rt(t)


def _ptr(t):
    from efficientspeech_amd.networks import _ptr as p
    return p(t)


# ------------------------------------------------------------------------------------------------ 1. the reduction alone
def check_sumsq(dev, n):
    """sqrt of the partial sums (added in float64 on the host) against g.double().norm(); two runs give the same bits; every one of
    the ESMI_TRAIN_GRAD_NORM_PARTIALS slots is written (the buffer starts out poisoned)."""
    gen = torch.Generator().manual_seed(1000 + n % 997)
    g = (torch.randn(n, generator=gen) * 10.0 ** (-4.0 * torch.rand(n, generator=gen))).to(dev)     # magnitudes over four decades
    runs = []
    for _ in range(2):
        part = torch.full((PARTIALS,), float("nan"), dtype=torch.float64, device=dev)
        lib, st = _rt(g)
        lib.esmi_train_grad_sumsq_f32(_ptr(g), n, _ptr(part), st)
        runs.append(part.cpu())
    got, ref = float(runs[0].sum().sqrt()), float(g.double().norm())
    err = abs(got - ref) / ref
    print(f"sumsq n={n}: norm {got!r} vs {ref!r}, relative error {err:.3e}")
    assert err <= NORM_RTOL, (n, got, ref, err)
    assert torch.equal(runs[0], runs[1])
    work = n // 4 or n                                             # 16-byte loads, or (n < 4) the scalar tail alone
    blocks = min(PARTIALS, (work + 255) // 256)
    assert int((runs[0] != 0).sum()) <= blocks and bool((runs[0][blocks:] == 0).all())       # one partial per workgroup, zeros behind
    return got


# ------------------------------------------------------------------------------------------------ the reference: torch's pair
def torch_clip_adamw(data, m, v, t_prev, grad, c):
    """clip_grad_norm_(c) + one torch.optim.AdamW step on float64 CPU copies, from the given pre-step state -> (data, m, v, norm, coef).
    float64 copies keep the reference's own round-off out of the comparison: torch's fp32 CPU norm of the tiny fixture's flat gradient
    buffer (266236 elements, one of them 24.4) comes out as 328.2500 against 328.2574 in float64, 2.3e-5 off -- more than the bounds
    above allow the code under test."""
    cp = lambda t: t.detach().cpu().double().clone()     # noqa: E731
    p = torch.nn.Parameter(cp(data))
    p.grad = cp(grad)
    opt = torch.optim.AdamW([p], lr=LR, betas=BETAS, eps=EPS, weight_decay=WD)
    if t_prev > 0:
        opt.state[p] = {"step": torch.tensor(float(t_prev)), "exp_avg": cp(m), "exp_avg_sq": cp(v)}
    norm = float("nan")
    coef = 1.0
    if c is not None:
        norm = float(torch.nn.utils.clip_grad_norm_([p], c, norm_type=2))
        coef = min(1.0, c / (norm + 1e-6))
    opt.step()
    return p.detach(), opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"], norm, coef


def _close(name, got, ref, tol):
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    err = float((got - ref).abs().max()) / max(1e-30, float(ref.abs().max()))
    print(f"  {name}: relative error {err:.3e} (allowed {tol:.0e})")
    assert err <= tol, (name, err, tol)


# ------------------------------------------------------------------------------------------------ 2. the optimizer launch alone
def _fresh(n, seed):
    gen = torch.Generator().manual_seed(seed)
    return 1e-2 * torch.randn(n, generator=gen)


def check_optimizer_launch(dev, launches=None):
    """`AdamWState(gradient_clip_val=c).launch` on a flat buffer of n = 1003, three consecutive launches with fresh gradients, against
    torch's pair.  From zero moments AdamW's first update is ~ lr sign(g) whatever the gradient's scale, so the MOMENTS are compared at
    every step (they carry the coefficient linearly and squared) and the parameters after the third.  `launches` (simulator): a
    context manager collecting the launched kernels' names."""
    from efficientspeech_amd import train
    n = 1003
    p0 = torch.randn(n, generator=torch.Generator().manual_seed(7))
    grads = [_fresh(n, 11 + j) for j in range(3)]
    c = 0.5 * float(grads[0].double().norm())
    flat = types.SimpleNamespace(data=p0.clone().to(dev), grad=torch.zeros(n, device=dev), m=torch.zeros(n, device=dev), v=torch.zeros(n, device=dev))
    opt = train.AdamWState(dev, precision=32, graph=False, lr=LR, gradient_clip_val=c)
    assert opt.on_device and opt.hyper is not None and opt.scaler is None and opt.absmax is None
    opt.set_lr(LR)
    ref = (p0.clone(), torch.zeros(n), torch.zeros(n))
    for j, g in enumerate(grads):
        flat.grad.copy_(g)
        if launches is not None and j == 0:
            with launches() as names:
                opt.launch(flat, BETAS, EPS, WD)
            assert names == ["train_grad_sumsq_kernel", "train_bump_clip_kernel", "train_adamw_dev_kernel"]
        else:
            opt.launch(flat, BETAS, EPS, WD)
        ref = torch_clip_adamw(*ref[:3], j, g, c)
        print(f"launch {j + 1}: grad_norm {opt.grad_norm!r} (torch {ref[3]!r}), clip_coef {opt.clip_coef!r} (torch {ref[4]!r})")
        assert opt.t == j + 1 and opt.clip_coef < 1.0
        assert abs(opt.grad_norm - ref[3]) <= NORM_RTOL * ref[3] and abs(opt.clip_coef - ref[4]) <= 2 * NORM_RTOL * ref[4]
        assert torch.equal(flat.grad.cpu(), g)                     # the optimizer does not modify the gradient buffer
        _close("m", flat.m, ref[1], M_TOL)
        _close("v", flat.v, ref[2], V_TOL)
    assert torch.allclose(flat.data.cpu().double(), ref[0], rtol=1e-4, atol=1e-6)


def check_inactive_clip_is_bitwise_the_unclipped_launch(dev):
    """gradient_clip_val = inf and = 1e9: the coefficient is exactly 1 and three launches leave data, m and v bit for bit where the
    unclipped on-device launch leaves them; the norm is still measured."""
    from efficientspeech_amd import train
    n = 1003
    p0 = torch.randn(n, generator=torch.Generator().manual_seed(7))
    grads = [_fresh(n, 11 + j) for j in range(3)]
    out = {}
    for c in (None, float("inf"), 1e9):
        flat = types.SimpleNamespace(data=p0.clone().to(dev), grad=torch.zeros(n, device=dev), m=torch.zeros(n, device=dev), v=torch.zeros(n, device=dev))
        opt = train.AdamWState(dev, precision=32, graph=True, lr=LR, gradient_clip_val=c)
        opt.set_lr(LR)
        for g in grads:
            flat.grad.copy_(g)
            opt.launch(flat, BETAS, EPS, WD)
            if c is not None:
                assert opt.clip_coef == 1.0
                assert abs(opt.grad_norm - float(g.double().norm())) <= NORM_RTOL * float(g.double().norm())
        out[c] = flat
    for c in (float("inf"), 1e9):
        for k in ("data", "m", "v"):
            assert torch.equal(getattr(out[c], k), getattr(out[None], k)), (c, k)


# ------------------------------------------------------------------------------------------------ 3. the whole step
P16_SCALE = 2048.0          # the scale `tests.test_train_step.check_precision16_step` shows the fixture batch does not overflow at


def _step_kw(precision):
    return dict(lr=LR, weight_decay=WD, precision=precision, **({"init_scale": P16_SCALE} if precision == 16 else {}))


@functools.lru_cache(maxsize=None)
def clipped_steps(dev, precision):
    """Three steps on the tiny fixture (B = 2) with gradient_clip_val = half of an unclipped run's first norm, run ONCE per (device,
    precision) and shared: -> (c, records); a record holds the state before the step, the gradient buffer the step left (divided by
    the loss scale in force during the step), the state after it and the step's read-outs, all on the CPU."""
    train, g, net, x, y = _setup(dev)
    probe = train.TrainStep(net, gradient_clip_val=float("inf"), **_step_kw(precision))
    probe.step(x, y)
    assert probe.clip_coef == 1.0
    c = 0.5 * probe.grad_norm
    train, g, net, x, y = _setup(dev)
    step = train.TrainStep(net, gradient_clip_val=c, **_step_kw(precision))
    f, records = step.flat, []
    cpu = lambda t: t.detach().cpu().clone()     # noqa: E731
    for j in range(3):
        before, scale = (cpu(f.data), cpu(f.m), cpu(f.v)), step.scale
        losses = step.step(x, y)
        assert bool(torch.isfinite(losses).all()) and step.t == j + 1 and step.skipped == 0
        records.append(dict(before=before, grad=cpu(f.grad).double().div(scale), after=(cpu(f.data), cpu(f.m), cpu(f.v)),
                            grad_norm=step.grad_norm, clip_coef=step.clip_coef, t_prev=j))
    return c, records


def check_whole_step(dev, precision, c_factor=1.0):
    """After each of the three steps: `grad_norm` is the float64 norm of `flat.grad` (unscaled), and m, v (and the weights) are what
    torch's clip + AdamW make of that same gradient buffer and the pre-step state.  c_factor != 1: the reference clips by
    c_factor * c instead -- the comparison must then fail (the sensitivity check)."""
    c, records = clipped_steps(dev, precision)
    for r in records:
        ref_norm = float(r["grad"].norm())
        err = abs(r["grad_norm"] - ref_norm) / ref_norm
        print(f"precision {precision} step {r['t_prev'] + 1}: grad_norm {r['grad_norm']!r} vs {ref_norm!r} ({err:.3e}), clip_coef {r['clip_coef']!r}")
        assert err <= NORM_RTOL, (precision, r["grad_norm"], ref_norm)
        want = min(1.0, c / (ref_norm + 1e-6))      # (active at the first step by construction; the norm falls as the batch is learnt)
        assert abs(r["clip_coef"] - want) <= 2 * NORM_RTOL * want and (r["t_prev"] > 0 or r["clip_coef"] < 0.51)
        ref =torch_clip_adamw(*r["before"], r["t_prev"], r["grad"].float(), c_factor * c)
        _close("m", r["after"][1], ref[1], M_TOL)
        _close("v", r["after"][2], ref[2], V_TOL)
        assert torch.allclose(r["after"][0].double(), ref[0], rtol=1e-4, atol=1e-6)


# ------------------------------------------------------------------------------------------------ 4. GPU only
def check_captured_clipped_step_equals_eager(dev="cuda"):
    """graph=True with clipping: four steps (one captures and runs eagerly, three replay) give the eager clipped step's losses and
    parameters at test_gpu_captured_step_equals_eager_step's tolerances, and its gradient norm after each step."""
    c = clipped_steps(dev, 32)[0]
    res = {}
    for graph in (False, True):
        train, g, net, x, y = _setup(dev)
        step = train.TrainStep(net, lr=LR, graph=graph, gradient_clip_val=c)
        rows = []
        for _ in range(4):
            losses = step.step(x, y).clone()
            rows.append((losses, step.grad_norm, step.clip_coef))
        res[graph] = (rows, step.flat.data.clone(), step.t)
    for (la, na, ca), (lb, nb, cb) in zip(res[False][0], res[True][0]):
        print(f"eager norm {na!r} coef {ca!r} | captured norm {nb!r} coef {cb!r}")
        assert torch.allclose(la, lb, rtol=1e-5, atol=0), (la, lb)
        assert abs(na - nb) <= NORM_RTOL * na and abs(ca - cb) <= 2 * NORM_RTOL * ca
    assert res[False][2] == res[True][2] == 4 and res[True][0][0][2] < 0.51 and res[True][0][1][2] < 1.0     # (clipping was active)
    assert torch.allclose(res[False][1], res[True][1], rtol=1e-4, atol=1e-6)


def check_precision16_overflow_still_skips(dev, how):
    """One precision-16 step whose scaled gradients are not finite, with clipping on: the step is skipped (skipped == 1, the counter
    stays, the scale backs off), the parameters and moments are bitwise unchanged, and the recorded norm is not finite.
    how = "scale": an init_scale that overflows the fixture batch on its own (2^126: the loss seeds are ~1e35, the first GEMM of the
    backward leaves fp32); how = "target": the overflow `check_precision16_step` provokes, an inf target at its scale of 2048."""
    train, g, net, x, y = _setup(dev)
    scale = 2.0 ** 126 if how == "scale" else P16_SCALE
    step = train.TrainStep(net, lr=LR, precision=16, init_scale=scale, gradient_clip_val=1.0)
    if how == "target":
        x = dict(x, pitch=x["pitch"].clone())
        x["pitch"][0, 0] = float("inf")
    snap = [t.clone() for t in (step.flat.data, step.flat.m, step.flat.v)]
    step.step(x, y)
    assert step.skipped == 1 and step.t == 0 and step.scale == 0.5 * scale
    for a, b in zip(snap, (step.flat.data, step.flat.m, step.flat.v)):
        assert torch.equal(a, b)
    assert not np.isfinite(step.grad_norm)


# ------------------------------------------------------------------------------------------------ 7. arguments
def check_arguments():
    from efficientspeech_amd import train
    import pytest
    for bad in (-1.0, -1e-9, float("nan")):
        with pytest.raises(ValueError):
            train.AdamWState("cpu", gradient_clip_val=bad)
    same = lambda a, b: (a is None and b is None) or (a is not None and b is not None and torch.equal(a, b))     # noqa: E731
    for graph in (False, True):
        for precision in (32, 16, "bf16"):
            today = train.AdamWState("cpu", precision, graph, LR)
            for off in (None, 0, 0.0):
                st = train.AdamWState("cpu", precision, graph, LR, gradient_clip_val=off)
                assert st.on_device == today.on_device and same(st.hyper, today.hyper) and same(st.scaler, today.scaler)
                assert same(st.absmax, today.absmax) and st.max_norm is None and not hasattr(st, "_sumsq")
                for name in ("grad_norm", "clip_coef"):
                    with pytest.raises(AttributeError):
                        getattr(st, name)
            on = train.AdamWState("cpu", precision, graph, LR, gradient_clip_val=float("inf"))
            assert on.on_device and on.hyper is not None and same(on.scaler, today.scaler) and (on.grad_norm, on.clip_coef) == (0.0, 1.0)
