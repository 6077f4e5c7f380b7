"""Checks of the training step's opt-in gradient accumulation (`TrainStep(accumulate_grad_batches=N)`, esmi_train_grad_accumulate_f32), shared
by the GPU tier and the wave-simulator tier of tests/test_grad_accum.py.  Every check takes the device ("cuda", or "cpu" inside `use_sim()`).

What is checked is what HAPPENS to the micro-batch gradients: they are read from `flat.grad` after each micro-batch (the existing tests hold
them to the reference) and torch's own pair, clip_grad_norm_ + AdamW on float64 copies (`grad_clip_checks.torch_clip_adamw`), is fed their
weighted sum.  Only check 4 goes back to autograd (the fp64 mirror), to show that the sum in `flat.acc` is a sum of the right things.

Tolerances are the project's: NORM_RTOL, M_TOL, V_TOL and the weights' rtol 1e-4 / atol 1e-6 (tests/grad_clip_checks.py), FP32_BOUND /
SPLIT_BOUND and KINK_MARGIN (tests/test_train_step.py).  The accumulator adds N roundings of 2^-24 relative each to a sum of N terms and
1 / N is rounded to fp32 once (3e-8 for 1 / 3): a few 1e-7 on the moments, far inside M_TOL = 1e-5.
"""
import functools

import numpy as np
import torch

from efficientspeech_amd import CONFIGS, build_phoneme2mel
from efficientspeech_amd.synth import synth_state_dict
from tests.grad_clip_checks import LR, M_TOL, NORM_RTOL, P16_SCALE, V_TOL, WD, _close, _ptr, _rt, torch_clip_adamw
from tests.test_train_step import FP32_BOUND, KINK_MARGIN, SPLIT_BOUND, _setup, at_size_case, fp64_reference

N_WINDOW = 3
SIZES = (1, 3, 4, 5, 1003, 4 * 256 * 2 + 3)                    # both tiers; the last: two workgroups and a three-element tail
SIZE_SECOND_TRIP = 1024 * 256 * 4 + 1028 + 3                   # GPU: the grid-stride loop's second trip, a tail that is no multiple of 4
WEIGHTS = (1.0 / 3.0, 0.25)
OFFSETS = ((0, 0), (1, 1), (0, 1))                             # (acc, g) in elements: 16-byte loads; both misaligned; only g misaligned
GRID_CAP = 1024                                                # workgroups of 256 (tu_train.hip esmi_train_grad_accumulate_f32)


def _to(d, dev):
    return {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in d.items()}


# ------------------------------------------------------------------------------------------------ the micro-batches
def _assert_margins(taps, what):
    assert len(taps) == 11 and min(taps.values()) > KINK_MARGIN, (
        f"{what}: a kink input of the fp64 reference lies within the margin", min(taps.values()), taps)


@functools.lru_cache(maxsize=None)
def fixture_micro():
    """The fixture window (N = 3): utterance 0 twice, utterance 1 twice, the whole batch of tests/golden/tiny_train_step.npz, on the CPU.
    -> (micro-batches, c): the kink margins of every micro-batch are asserted from the fp64 mirror alone, and c is HALF the 2-norm of
    the mirror's mean gradient over the window: a clip value that makes the window's coefficient about 0.5."""
    _, _, _, x, y = _setup("cpu")
    cut = lambda d, r: {k: (torch.cat([v[r:r + 1], v[r:r + 1]]) if torch.is_tensor(v) and v.dim() > 0 and v.shape[0] == 2 else v)   # noqa: E731
                        for k, v in d.items()}
    micro = [(cut(x, 0), cut(y, 0)), (cut(x, 1), cut(y, 1)), (x, y)]
    cfg = CONFIGS["tiny"]
    sd = synth_state_dict(cfg, 1234)
    grads = []
    for j, (xi, yi) in enumerate(micro):
        _, g, taps = fp64_reference(cfg, sd, xi, yi)
        _assert_margins(taps, f"fixture micro-batch {j}")
        print(f"fixture micro-batch {j}: smallest kink margin {min(taps.values()):.2e}")
        grads.append(g)
    sq = sum(float((sum(g[k] for g in grads) / len(grads)).pow(2).sum()) for k in grads[0] if grads[0][k] is not None)
    return micro, 0.5 * sq ** 0.5


@functools.lru_cache(maxsize=None)
def at_size_micro():
    """`at_size_case("tiny")` rows 0:2, 2:4 and 4:6, each trimmed to its own longest phoneme and mel length: three batch shapes.
    -> (cfg, sd, micro-batches, fp64 gradients of the first two), margins asserted from the reference alone."""
    cfg, sd, x, y = at_size_case("tiny")
    micro, grads = [], []
    for j in range(3):
        rows = slice(2 * j, 2 * j + 2)
        T = int((~x["phoneme_mask"][rows]).sum(1).max())
        L = int(x["mel_len"][rows].max())
        xi = {k: (v[rows, :L] if k == "mel_mask" else v[rows] if k == "mel_len" else v[rows, :T]).contiguous() for k, v in x.items()}
        yi = {"mel": y["mel"][rows, :L].contiguous()}
        _, g, taps = fp64_reference(cfg, sd, xi, yi, backward=j < 2)
        _assert_margins(taps, f"at-size rows {2 * j}:{2 * j + 2}")
        print(f"at-size rows {2 * j}:{2 * j + 2}: T {T}, L {L}, smallest kink margin {min(taps.values()):.2e}")
        micro.append((xi, yi))
        grads.append(g)
    assert len({(m[0]["phoneme"].shape, m[1]["mel"].shape) for m in micro}) == 3
    return cfg, sd, micro, grads[:2]


def _at_size_net(dev):
    cfg, sd, micro, _ = at_size_micro()
    net = build_phoneme2mel(cfg)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    return net.to(dev).train(), [(_to(a, dev), _to(b, dev)) for a, b in micro]


# ------------------------------------------------------------------------------------------------ 1. the kernel alone
CANARY = 12345.0


def _operands(n, pad, seed):
    gen = torch.Generator().manual_seed(seed)
    val = lambda: torch.randn(n, generator=gen) * 10.0 ** (-4.0 * torch.rand(n, generator=gen))     # noqa: E731 -- over four decades
    buf = lambda off, v: torch.cat([torch.full((off,), CANARY), v, torch.full((pad,), CANARY)])   # noqa: E731
    return val(), val(), buf


def _accumulate(acc, g, n, w):
    lib, st = _rt(acc)
    lib.esmi_train_grad_accumulate_f32(_ptr(acc), _ptr(g), n, w, st)


def check_kernel(dev, n):
    """acc[q] = fmaf(g[q], w, acc[q]) for q < n against float64, |got - ref| <= 2^-23 |ref| elementwise (one rounding, with a factor of
    two to spare; a result below the smallest normal number may be off by one subnormal step instead); for both weights, on the 16-byte
    path, with both pointers offset by one element and with only g offset; the canaries around acc and all of g stay as they were; two
    runs give the same bits."""
    pad = 8
    for w in WEIGHTS:
        w32 = float(np.float32(w))
        for a_off, g_off in OFFSETS:
            a0, g0, buf = _operands(n, pad, 1000 + n % 997)
            runs = []
            for _ in range(2):
                abuf, gbuf = buf(a_off, a0).to(dev), buf(g_off, g0).to(dev)
                acc, g = abuf[a_off:a_off + n], gbuf[g_off:g_off + n]
                assert (acc.data_ptr() % 16 == 0) == (a_off == 0) and (g.data_ptr() % 16 == 0) == (g_off == 0)
                _accumulate(acc, g, n, w)
                runs.append(abuf.cpu())
                assert torch.equal(gbuf.cpu(), buf(g_off, g0))
            got = runs[0][a_off:a_off + n].double()
            ref = a0.double() + g0.double() * w32
            slack = torch.where(ref.abs() < 2.0 ** -126, 2.0 ** -149, 0.0).double()
            excess = float(((got - ref).abs() - 2.0 ** -23 * ref.abs() - slack).max())
            worst = float(((got - ref).abs() / ref.abs().clamp_min(1e-300)).max())
            print(f"accumulate n={n} w={w32!r} offsets {(a_off, g_off)}: worst relative error {worst:.3e} (allowed {2.0 ** -23:.3e})")
            assert excess <= 0.0, (n, w, a_off, g_off, worst)
            assert bool((runs[0][:a_off] == CANARY).all()) and bool((runs[0][a_off + n:] == CANARY).all())
            assert torch.equal(runs[0], runs[1])


def check_kernel_nonfinite_and_empty(dev, launches=None):
    """inf and nan in g arrive in acc on the 16-byte path, in its tail and on the scalar path, and touch nothing else; n == 0 succeeds
    without a launch (`launches`, simulator: a context manager collecting the launched kernels' names); overlapping buffers are refused."""
    import pytest
    n = 1003
    at = {0: float("inf"), 5: float("nan"), 6: float("-inf"), n - 1: float("nan")}      # (n - 1: the three-element tail)
    for off in (0, 1):
        a0, g0, buf = _operands(n, 4, 77)
        for q, v in at.items():
            g0[q] = v
        abuf, gbuf = buf(off, a0).to(dev), buf(off, g0).to(dev)
        acc, g = abuf[off:off + n], gbuf[off:off + n]
        _accumulate(acc, g, n, 0.25)
        got = acc.cpu()
        assert got[0] == float("inf") and got[6] == float("-inf") and bool(got[5].isnan()) and bool(got[n - 1].isnan())
        clean = torch.ones(n, dtype=torch.bool)
        clean[list(at)] = False
        assert bool(torch.isfinite(got[clean]).all()) and int((~torch.isfinite(abuf.cpu())).sum()) == len(at)
        _accumulate(acc, g, n, 0.25)                              # inf + -inf... whatever follows, a poisoned element stays poisoned
        assert int((~torch.isfinite(acc.cpu())).sum()) == len(at)
    acc, g = torch.full((8,), CANARY).to(dev), torch.ones(8).to(dev)
    if launches is not None:
        with launches() as names:
            _accumulate(acc, g, 0, 0.5)
        assert names == []
    else:
        _accumulate(acc, g, 0, 0.5)
    assert bool((acc.cpu() == CANARY).all())
    with pytest.raises(RuntimeError, match="ESMI_ERR_ARG"):
        _accumulate(acc, acc[4:], 8, 0.5)                         # (refused before any launch)


# ------------------------------------------------------------------------------------------------ 2. one window against torch
def _step_kw(precision, clip):
    kw = dict(lr=LR, weight_decay=WD, precision=precision, accumulate_grad_batches=N_WINDOW)
    if precision == 16:
        kw["init_scale"] = P16_SCALE
    if clip:
        kw["gradient_clip_val"] = fixture_micro()[1]
    return kw


@functools.lru_cache(maxsize=None)
def window_records(dev, precision, clip):
    """Two windows of N = 3 on the fixture micro-batches, run ONCE per (device, precision, clip) and shared.  Inside a window nothing of
    the optimizer moves; a record holds the state before the window, sum g_i / N in float64 (g_i = `flat.grad` after micro-batch i,
    divided by the loss scale), the state after the boundary and its read-outs, all on the CPU."""
    micro = [(_to(a, dev), _to(b, dev)) for a, b in fixture_micro()[0]]
    train, _, net, _, _ = _setup(dev)
    step = train.TrainStep(net, **_step_kw(precision, clip))
    f, records = step.flat, []
    cpu = lambda t: t.detach().cpu().clone()     # noqa: E731
    assert f.acc.shape == f.grad.shape and step.micro == 0 and step.t == 0
    for w in range(2):
        before, scale = (cpu(f.data), cpu(f.m), cpu(f.v)), step.scale
        total = torch.zeros(f.grad.numel(), dtype=torch.float64)
        for j, (x, y) in enumerate(micro):
            losses = step.step(x, y)
            assert bool(torch.isfinite(losses).all())
            total += cpu(f.grad).double() / scale / N_WINDOW
            if j < N_WINDOW - 1:
                assert step.micro == j + 1 and step.t == w and step.scale == scale
                for a, b in zip(before, (f.data, f.m, f.v)):
                    assert torch.equal(a, b.cpu()), "the optimizer's state moved inside a window"
        assert step.t == w + 1 and step.micro == 0 and step.skipped == 0
        assert not bool(f.acc.any()), "the accumulator is not zero after the boundary"
        records.append(dict(before=before, grad=total, after=(cpu(f.data), cpu(f.m), cpu(f.v)), t_prev=w,
                            grad_norm=step.grad_norm if clip else None, clip_coef=step.clip_coef if clip else None))
    return records


def check_window(dev, precision, clip, wrong_n=None):
    """After each of two windows in a row (the second starts from a zeroed accumulator and non-zero moments): m, v and the weights are
    what torch's clip + AdamW make of sum g_i / N and the state before the window; `grad_norm` is the float64 norm of that sum and
    `clip_coef` follows from it, below 1 in the first window.  wrong_n: the reference divides by it instead of N -- the comparison
    must then fail (the sensitivity check)."""
    c = fixture_micro()[1] if clip else None
    for r in window_records(dev, precision, clip):
        grad = r["grad"] * (N_WINDOW / wrong_n) if wrong_n else r["grad"]
        if clip:
            ref_norm = float(grad.norm())
            want = min(1.0, c / (ref_norm + 1e-6))
            err = abs(r["grad_norm"] - ref_norm) / ref_norm
            print(f"precision {precision} window {r['t_prev'] + 1}: grad_norm {r['grad_norm']!r} vs {ref_norm!r} ({err:.3e}), clip_coef {r['clip_coef']!r}")
            assert err <= NORM_RTOL, (precision, r["grad_norm"], ref_norm)
            assert abs(r["clip_coef"] - want) <= 2 * NORM_RTOL * want and (r["t_prev"] > 0 or r["clip_coef"] < 0.75)
        ref = torch_clip_adamw(*r["before"], r["t_prev"], grad, c)
        _close("m", r["after"][1], ref[1], M_TOL)
        _close("v", r["after"][2], ref[2], V_TOL)
        assert torch.allclose(r["after"][0].double(), ref[0], rtol=1e-4, atol=1e-6)


# ------------------------------------------------------------------------------------------------ 4. the accumulated gradient against autograd
def check_accumulated_gradient_at_size(dev):
    """`flat.acc` after two of three at-size micro-batches against (g1 + g2) / 3 from the fp64 mirror, per parameter and relative to the
    target's largest element, on both operator paths.  Each g_i is held to bound * max|g_i| by check_gradients_at_size, so the sum is
    off by at most bound * sum_i max|g_i| / 3 = bound * rho_k * max|target| with rho_k = mean_i max|g_i| / max|mean_i g_i| >= 1, taken
    from the reference alone (the accumulator's own roundings, 2^-24 each, disappear in that)."""
    from efficientspeech_amd import train
    _, _, _, (g1, g2) = at_size_micro()
    worst, old = {}, train.USE_MATRIX_PIPE
    try:
        for matrix_pipe, bound in ((False, FP32_BOUND), (True, SPLIT_BOUND)):
            train.USE_MATRIX_PIPE = matrix_pipe
            net, micro = _at_size_net(dev)
            step = train.TrainStep(net, accumulate_grad_batches=N_WINDOW)
            for x, y in micro[:2]:
                step.step(x, y)
            assert step.micro == 2 and step.t == 0
            acc = step.flat.acc.detach().cpu().double()
            rows = []
            for k, sl in zip(step.flat.names, step.flat.slices):
                target = (g1[k] + g2[k]).reshape(-1) / N_WINDOW
                rho = 0.5 * (float(g1[k].abs().max()) + float(g2[k].abs().max())) / max(1e-6, float((0.5 * (g1[k] + g2[k])).abs().max()))
                err = float((acc[sl] - target).abs().max()) / max(1e-6, float(target.abs().max()))
                rows.append((err / (bound * rho), err, rho, k))
            assert len(rows) >= 100
            worst[matrix_pipe] = max(rows)
            print(f"matrix pipe {matrix_pipe}: worst error / allowed {max(rows)[0]:.3f} (error {max(rows)[1]:.2e}, rho {max(rows)[2]:.2f}, {max(rows)[3]}); "
                  f"largest rho {max(r[2] for r in rows):.2f}")
            assert max(rows)[0] < 1.0, (matrix_pipe, sorted(rows)[-5:])
    finally:
        train.USE_MATRIX_PIPE = old
    return worst


# ------------------------------------------------------------------------------------------------ 5. off is off
def check_off_is_off(dev, records=None):
    """accumulate_grad_batches absent, None and 1: no accumulator, the same attributes on the step, its flat buffers and its optimizer state,
    bitwise the same weights after one step -- and (`records`, simulator: tests.simlib.launch_records) the same launches, record for record."""
    out = []
    for kw in ({}, {"accumulate_grad_batches": None}, {"accumulate_grad_batches": 1}):
        train, _, net, x, y = _setup(dev)
        step = train.TrainStep(net, lr=LR, **kw)
        assert not hasattr(step.flat, "acc") and step.micro == 0
        got = None
        if records is not None:
            with records() as got:
                step.step(x, y)
        else:
            step.step(x, y)
        assert step.micro == 0 and step.t == 1 and step.flush() is False
        out.append((sorted(vars(step)), sorted(vars(step.flat)), sorted(vars(step._opt)), step.flat.data.cpu().clone(), got))
    for other in out[1:]:
        assert other[:3] == out[0][:3] and torch.equal(other[3], out[0][3])
        assert other[4] == out[0][4] and (records is None or len(other[4]) > 100)


# ------------------------------------------------------------------------------------------------ 7. GPU only
def check_captured_window_equals_eager(dev="cuda"):
    """graph=True, N = 2, two windows over two at-size shapes mixed within each window (A B | B A): the first window captures (each
    capture runs its micro-batch eagerly once, the boundary likewise), the second replays both shape graphs and the shared boundary
    graph.  Losses and parameters against the eager run at test_gpu_captured_step_equals_eager_step's tolerances.  Between the windows
    `t` is set to 7 on both: the REPLAYED boundary graph must read it (with t = 1 -> 2 instead of 7 -> 8 the bias corrections move the
    update by far more than the tolerance)."""
    from efficientspeech_amd import train
    res = {}
    for graph in (False, True):
        net, micro = _at_size_net(dev)
        step = train.TrainStep(net, lr=LR, graph=graph, accumulate_grad_batches=2)
        losses = []
        for w, order in enumerate(((0, 1), (1, 0))):
            for j, i in enumerate(order):
                losses.append(step.step(*micro[i]).clone())
                assert step.micro == (j + 1) % 2
            assert not bool(step.flat.acc.any())
            if w == 0:
                assert step.t == 1
                step.t = 7
        res[graph] = (losses, step.flat.data.clone(), step.t)
        if graph:
            assert len(step._graphs) == 2 and step._boundary_graph is not None
    for a, b in zip(res[False][0], res[True][0]):
        assert torch.allclose(a, b, rtol=1e-5, atol=0), (a, b)
    assert res[False][2] == res[True][2] == 8
    assert torch.allclose(res[False][1], res[True][1], rtol=1e-4, atol=1e-6)


def check_checkpoint_between_windows_resumes_into_a_captured_step(dev="cuda"):
    """A checkpoint taken between two windows of a captured accumulating step resumes into a fresh captured step; the next window gives
    the uninterrupted run's losses and parameters, and both count 2."""
    micro = [(_to(a, dev), _to(b, dev)) for a, b in fixture_micro()[0][:2]]
    kw = dict(lr=LR, graph=True, accumulate_grad_batches=2)
    train, _, net, _, _ = _setup(dev)
    a = train.TrainStep(net, **kw)
    for x, y in micro:
        a.step(x, y)
    ckpt = a.state_dict()
    assert ckpt["global_step"] == 1
    last_a = [a.step(x, y).clone() for x, y in micro]
    t2, _, net2, _, _ = _setup(dev)
    b = t2.TrainStep(net2, **kw)
    b.load_state_dict(ckpt)
    last_b = [b.step(x, y).clone() for x, y in micro]
    assert a.t == b.t == 2 and a.micro == b.micro == 0
    for la, lb in zip(last_a, last_b):
        assert torch.allclose(la, lb, rtol=1e-4, atol=1e-6), (la, lb)
    assert torch.allclose(a.flat.data, b.flat.data, rtol=1e-4, atol=1e-6)


# ------------------------------------------------------------------------------------------------ 8. precision-16 overflow
def check_precision16_overflow_skips_the_window(dev):
    """An inf target in the MIDDLE micro-batch only (check_precision16_overflow_still_skips's "target"), clipping on: the non-finite
    gradients reach the boundary through the accumulator and the whole window is skipped -- skipped == 1, t == 0, the scale halved (and
    untouched inside the window), weights and moments bitwise unchanged, the accumulator zero again.  The next window, clean, updates."""
    micro = [(_to(a, dev), _to(b, dev)) for a, b in fixture_micro()[0]]
    train, _, net, _, _ = _setup(dev)
    step = train.TrainStep(net, lr=LR, precision=16, init_scale=P16_SCALE, gradient_clip_val=1.0, accumulate_grad_batches=N_WINDOW)
    f = step.flat
    snap = [t.clone() for t in (f.data, f.m, f.v)]
    for j, (x, y) in enumerate(micro):
        if j == 1:
            x = dict(x, pitch=x["pitch"].clone())
            x["pitch"][0, 0] = float("inf")
        step.step(x, y)
        if j < N_WINDOW - 1:
            assert step.scale == P16_SCALE and step.skipped == 0
            assert bool(torch.isfinite(f.acc).all()) == (j == 0)
    assert step.skipped == 1 and step.t == 0 and step.micro == 0 and step.scale == 0.5 * P16_SCALE
    for a, b in zip(snap, (f.data, f.m, f.v)):
        assert torch.equal(a, b)
    assert not np.isfinite(step.grad_norm) and not bool(f.acc.any())
    for x, y in micro:
        step.step(x, y)
    assert step.skipped == 1 and step.t == 1 and step.scale == 0.5 * P16_SCALE and np.isfinite(step.grad_norm)
    assert not torch.equal(snap[0], f.data) and bool(torch.isfinite(f.data).all())


# ------------------------------------------------------------------------------------------------ 10. fit
def check_fit(dev):
    """Three batches per epoch, N = 2, two epochs: every epoch is one full window and one flushed short one, so t == 4 and no window
    stays open; a record's losses are the mean of the undivided losses `step` returned for that epoch's three micro-batches."""
    micro = [(_to(a, dev), _to(b, dev)) for a, b in fixture_micro()[0]]
    train, _, net, _, _ = _setup(dev)
    step = train.TrainStep(net, lr=LR, accumulate_grad_batches=2)
    seen, open_windows, inner = [], [], step.step

    def recording(x, y, lr=None):
        seen.append(inner(x, y, lr=lr).clone())
        return seen[-1]
    step.step = recording
    before = step.flat.data.clone()
    hist = train.fit(step, micro, epochs=2, device=dev, first_epoch=60, log=lambda rec: open_windows.append(step.micro))
    assert step.t == 4 and open_windows == [0, 0] and step.micro == 0 and len(seen) == 6
    for e, rec in enumerate(hist):
        want = torch.stack(seen[3 * e:3 * e + 3]).mean(0).cpu()
        assert torch.allclose(torch.tensor(rec["losses"]), want, rtol=1e-6, atol=0), (rec, want)
    assert not torch.equal(step.flat.data, before) and not bool(step.flat.acc.any())


# ------------------------------------------------------------------------------------------------ 11. state_dict() and arguments
def check_state_dict_and_flush(dev):
    import pytest
    micro = [(_to(a, dev), _to(b, dev)) for a, b in fixture_micro()[0]]
    train, _, net, _, _ = _setup(dev)
    a = train.TrainStep(net, lr=LR, accumulate_grad_batches=2)
    assert a.flush() is False
    a.step(*micro[0])
    with pytest.raises(RuntimeError, match=r"flush\(\)"):
        a.state_dict()
    before = a.flat.data.clone()
    assert a.flush() is True and a.micro == 0 and a.t == 1 and not bool(a.flat.acc.any()) and not torch.equal(a.flat.data, before)
    ckpt = a.state_dict()
    assert ckpt["global_step"] == 1 and "accumulate_grad_batches" not in ckpt and "accumulate_grad_batches" not in ckpt["hyper_parameters"]
    t2, _, net2, _, _ = _setup(dev)
    b = t2.TrainStep(net2, lr=LR, accumulate_grad_batches=2)
    b.step(*micro[1])
    assert b.micro == 1 and bool(b.flat.acc.any())
    b.load_state_dict(ckpt)                                       # clears the open window
    assert b.micro == 0 and not bool(b.flat.acc.any()) and b.t == 1
    for k in ("data", "m", "v"):
        assert torch.equal(getattr(a.flat, k), getattr(b.flat, k)), k
    for s in (a, b):                                              # ... and the next window is the same on both
        for x, y in micro[:2]:
            s.step(x, y)
    assert a.t == b.t == 2 and torch.equal(a.flat.data, b.flat.data)


def check_arguments():
    import pytest
    from efficientspeech_amd import EfficientSpeech
    train, _, net, _, _ = _setup("cpu")
    before = [p.data_ptr() for p in net.parameters()]
    for bad in (0, -1, -3, 2.5, 2.0, True, False, "2"):
        with pytest.raises(ValueError, match="accumulate_grad_batches"):
            train.TrainStep(net, accumulate_grad_batches=bad)
    assert before == [p.data_ptr() for p in net.parameters()]      # (refused before the parameters were re-homed)
    step = train.TrainStep(net, accumulate_grad_batches=np.int64(4))
    assert step.flat.acc.shape == step.flat.grad.shape and step.flat.acc.data_ptr() % 16 == 0 and step.micro == 0
    assert step._opt.on_device is False                            # accumulation alone does not move the optimizer's scalars to the device
    model = EfficientSpeech.from_config("tiny")
    via = model.make_train_step(accumulate_grad_batches=2)         # the wrapper passes the keyword through
    assert via.micro == 0 and via.flat.acc.shape == via.flat.grad.shape
