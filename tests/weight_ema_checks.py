"""Checks of the training step's opt-in weight average (`TrainStep(ema_decay=d)`, esmi_train_ema_update_f32, esmi_train_swap_f32), of
`TrainStep.evaluate` and of `fit`'s validation pass, shared by the GPU tier and the wave-simulator tier of tests/test_weight_ema.py.  Every
check takes the device ("cuda", or "cpu" inside `use_sim()`).

Bounds.  The update is ema' = fl(fl(p - ema) * w + ema) (one subtraction, one fused multiply-add): two roundings of 2^-24 relative each,
|err| <= 2^-24 (|ref| + w |p - ema|); the kernel check allows twice that, plus one subnormal step where the result is subnormal.  Over
steps the error of step j is carried on with the factor (1 - w) <= 1, so after k steps it is at most the k per-step bounds summed:
k 2^-23 max_j(|ema_j|, |p_j|) elementwise.  The float64 references use w as the kernel gets it: 1 - d formed in double, rounded to fp32 once.
The exchange moves bits and is compared as int32.
"""
import functools

import numpy as np
import torch

from efficientspeech_amd import _lib
from tests.grad_accum_checks import CANARY, GRID_CAP, OFFSETS, SIZE_SECOND_TRIP, SIZES, _operands, _to, fixture_micro   # noqa: F401
from tests.grad_clip_checks import LR, P16_SCALE, WD, _ptr, _rt
from tests.test_train_step import _setup

DECAY = 0.9
DECAYS = (0.9, 0.999)
STEPS = 4
EPS = 2.0 ** -23


def w32(decay):
    return float(np.float32(1.0 - decay))


def _update(ema, p, n, w, hyper=None):
    lib, st = _rt(ema)
    lib.esmi_train_ema_update_f32(_ptr(ema), _ptr(p), n, w, _ptr(hyper) if hyper is not None else None, st)


def _swap(a, b, n):
    lib, st = _rt(a)
    lib.esmi_train_swap_f32(_ptr(a), _ptr(b), n, st)


def _hyper(dev, skip):
    h = torch.full((_lib.TRAIN_ADAMW_HYPER_FLOATS,), 0.5)           # (every other slot non-zero: only the skip slot may decide)
    h[_lib.HYPER_SKIP] = skip
    return h.to(dev)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


# ------------------------------------------------------------------------------------------------ 2. the update kernel alone
def check_update_kernel(dev, n):
    """ema[q] = fmaf(w, p[q] - ema[q], ema[q]) for q < n against float64 within 2^-23 (|ref| + w |p - ema|) elementwise (+ one subnormal
    step for a subnormal result), for both decays and the three offset pairs; the canaries around ema and all of p stay; two runs give
    the same bits."""
    pad = 8
    for decay in DECAYS:
        w = w32(decay)
        for e_off, p_off in OFFSETS:
            e0, p0, buf = _operands(n, pad, 2000 + n % 997)
            runs = []
            for _ in range(2):
                ebuf, pbuf = buf(e_off, e0).to(dev), buf(p_off, p0).to(dev)
                ema, p = ebuf[e_off:e_off + n], pbuf[p_off:p_off + n]
                assert (ema.data_ptr() % 16 == 0) == (e_off == 0) and (p.data_ptr() % 16 == 0) == (p_off == 0)
                _update(ema, p, n, 1.0 - decay)
                runs.append(ebuf.cpu())
                assert torch.equal(pbuf.cpu(), buf(p_off, p0))
            got = runs[0][e_off:e_off + n].double()
            delta = p0.double() - e0.double()
            ref = e0.double() + w * delta
            allowed = EPS * (ref.abs() + w * delta.abs()) + torch.where(ref.abs() < 2.0 ** -126, 2.0 ** -149, 0.0).double()
            ratio = float(((got - ref).abs() / allowed.clamp_min(1e-300)).max())
            print(f"ema update n={n} decay={decay} offsets {(e_off, p_off)}: worst error / allowed {ratio:.3f}")
            assert ratio <= 1.0, (n, decay, e_off, p_off, ratio)
            assert bool((runs[0][:e_off] == CANARY).all()) and bool((runs[0][e_off + n:] == CANARY).all())
            assert torch.equal(runs[0], runs[1])


# ------------------------------------------------------------------------------------------------ 3. the skip flag
def check_skip_flag(dev):
    """hyper[ESMI_HYPER_SKIP] == 1: ema bitwise unchanged; == 0: the NULL call's bits.  n = 1003, 16-byte path and scalar path."""
    n = 1003
    for off in (0, 1):
        e0, p0, buf = _operands(n, 4, 31)
        results = {}
        for name, hyper in (("null", None), ("skip", _hyper(dev, 1.0)), ("run", _hyper(dev, 0.0))):
            ebuf, pbuf = buf(off, e0).to(dev), buf(off, p0).to(dev)
            _update(ebuf[off:off + n], pbuf[off:off + n], n, 0.1, hyper)
            results[name] = ebuf.cpu()
            if hyper is not None:
                assert hyper[_lib.HYPER_SKIP].item() == (1.0 if name == "skip" else 0.0) and float(hyper[0]) == 0.5   # (read only)
        assert same_bits(results["skip"], buf(off, e0)), off
        assert same_bits(results["run"], results["null"]) and not same_bits(results["null"], buf(off, e0)), off


# ------------------------------------------------------------------------------------------------ 4. non-finite values, empty input, overlap
def check_update_nonfinite_and_empty(dev, launches=None):
    import pytest
    n = 1003
    at = {0: float("inf"), 5: float("nan"), 6: float("-inf"), n - 1: float("nan")}      # (n - 1: the three-element tail)
    for off in (0, 1):
        e0, p0, buf = _operands(n, 4, 78)
        for q, v in at.items():
            p0[q] = v
        ebuf, pbuf = buf(off, e0).to(dev), buf(off, p0).to(dev)
        _update(ebuf[off:off + n], pbuf[off:off + n], n, 0.1)
        got = ebuf[off:off + n].cpu()
        assert got[0] == float("inf") and got[6] == float("-inf") and bool(got[5].isnan()) and bool(got[n - 1].isnan())
        assert int((~torch.isfinite(ebuf.cpu())).sum()) == len(at)
    ema, p = torch.full((8,), CANARY).to(dev), torch.ones(8).to(dev)
    if launches is not None:
        with launches() as names:
            _update(ema, p, 0, 0.5)
        assert names == []
    else:
        _update(ema, p, 0, 0.5)
    assert bool((ema.cpu() == CANARY).all())
    with pytest.raises(RuntimeError, match="ESMI_ERR_ARG"):
        _update(ema, ema[4:], 8, 0.5)                             # (refused before any launch)
    assert bool((ema.cpu() == CANARY).all())


# ------------------------------------------------------------------------------------------------ 5. the exchange
_SPECIAL = (0x7FC00001, 0x7FA00001, -0x00800000, 0x7F800000, -0x80000000, 0x7FFFFFFF)   # quiet / signalling nan with payloads, -inf, +inf, -0.0, nan


def _swap_operand(n, seed):
    gen = torch.Generator().manual_seed(seed)
    t = torch.randn(n, generator=gen).view(torch.int32).clone()
    for k, bits in enumerate(_SPECIAL):
        t[(seed + k * 7919) % n] = bits
    return t


def check_swap_kernel(dev, n):
    """After one exchange each buffer holds the other's bytes, after two both hold their own; nan payloads, infinities and -0.0
    included; canaries intact.  Compared as int32."""
    pad, canary = 8, torch.full((1,), CANARY).view(torch.int32).item()
    for a_off, b_off in OFFSETS:
        a0, b0 = _swap_operand(n, 11), _swap_operand(n, 12)
        buf = lambda off, v: torch.cat([torch.full((off,), canary, dtype=torch.int32), v, torch.full((pad,), canary, dtype=torch.int32)])   # noqa: E731
        abuf, bbuf = buf(a_off, a0).view(torch.float32).to(dev), buf(b_off, b0).view(torch.float32).to(dev)
        a, b = abuf[a_off:a_off + n], bbuf[b_off:b_off + n]
        assert (a.data_ptr() % 16 == 0) == (a_off == 0) and (b.data_ptr() % 16 == 0) == (b_off == 0)
        _swap(a, b, n)
        assert torch.equal(_bits(abuf), buf(a_off, b0)) and torch.equal(_bits(bbuf), buf(b_off, a0)), (n, a_off, b_off)
        _swap(a, b, n)
        assert torch.equal(_bits(abuf), buf(a_off, a0)) and torch.equal(_bits(bbuf), buf(b_off, b0)), (n, a_off, b_off)


def check_swap_empty_and_overlap(dev, launches=None):
    import pytest
    a, b = torch.full((8,), CANARY).to(dev), torch.ones(8).to(dev)
    if launches is not None:
        with launches() as names:
            _swap(a, b, 0)
        assert names == []
    else:
        _swap(a, b, 0)
    with pytest.raises(RuntimeError, match="ESMI_ERR_ARG"):
        _swap(a, a[4:], 8)
    assert bool((a.cpu() == CANARY).all()) and bool((b.cpu() == 1).all())


# ------------------------------------------------------------------------------------------------ 7. the average follows the steps
def step_kw(precision, **kw):
    kw = dict(lr=LR, weight_decay=WD, precision=precision, ema_decay=DECAY, **kw)
    if precision == 16:
        kw["init_scale"] = P16_SCALE
    return kw


@functools.lru_cache(maxsize=None)
def step_records(dev, precision, graph):
    """Four steps on the fixture batch with ema_decay = 0.9, run ONCE per (device, precision, graph) and shared:
    -> (the initial weights, [(weights, average) after step k]), on the CPU."""
    train, _, net, x, y = _setup(dev)
    step = train.TrainStep(net, **step_kw(precision, graph=graph))
    f = step.flat
    assert f.ema.shape == f.data.shape and f.ema.data_ptr() != f.data.data_ptr() and same_bits(f.ema, f.data)
    p0, out = f.data.cpu().clone(), []
    for _ in range(STEPS):
        assert bool(torch.isfinite(step.step(x, y)).all())
        out.append((f.data.cpu().clone(), f.ema.cpu().clone()))
    assert step.t == STEPS and step.skipped == 0
    pad = torch.ones(f.data.numel(), dtype=torch.bool)
    for sl in f.slices:
        pad[sl] = False
    assert not bool(f.ema.cpu()[pad].any()), "a pad element of the average moved"
    return p0, out


def check_average_follows_the_steps(dev, precision, graph=False, decay=DECAY):
    """ema_k against the float64 recurrence e_k = e_{k-1} + w (p_k - e_{k-1}), e_0 = p_0, over the weights the step itself produced,
    within k 2^-23 max_j(|e_j|, |p_j|) elementwise.  decay: the reference's -- another one than the step's must fail."""
    p0, records = step_records(dev, precision, graph)
    w = w32(decay)
    ref = p0.double()
    scale = ref.abs()
    for k, (p, ema) in enumerate(records, 1):
        ref = ref + w * (p.double() - ref)
        scale = torch.maximum(scale, torch.maximum(ref.abs(), p.double().abs()))
        err = (ema.double() - ref).abs()
        ratio = float((err / (k * EPS * scale).clamp_min(1e-300)).max())
        print(f"precision {precision} graph {graph} step {k}: worst error / allowed {ratio:.3f} (largest error {float(err.max()):.3e})")
        assert ratio <= 1.0, (precision, graph, k, ratio)
    assert not torch.equal(records[-1][1], p0) and not torch.equal(records[-1][1], records[-1][0])


# ------------------------------------------------------------------------------------------------ 8. accumulation
def check_accumulation(dev):
    """N = 2: the average stays bitwise through a non-boundary micro-batch, moves on the boundary and moves on flush()."""
    micro = [(_to(a, dev), _to(b, dev)) for a, b in fixture_micro()[0]]
    train, _, net, _, _ = _setup(dev)
    step = train.TrainStep(net, lr=LR, accumulate_grad_batches=2, ema_decay=DECAY)
    f = step.flat
    e0 = f.ema.clone()
    step.step(*micro[0])
    assert step.micro == 1 and same_bits(f.ema, e0)
    step.step(*micro[1])
    assert step.micro == 0 and step.t == 1 and not torch.equal(f.ema, e0)
    e1 = f.ema.clone()
    step.step(*micro[2])
    assert step.micro == 1 and same_bits(f.ema, e1)
    assert step.flush() is True and step.t == 2 and not torch.equal(f.ema, e1)
    want = e1.double() + w32(DECAY) * (f.data.double() - e1.double())
    assert float(((f.ema.double() - want).abs() - EPS * torch.maximum(want.abs(), f.data.double().abs())).max()) <= 0.0


# ------------------------------------------------------------------------------------------------ 9. precision-16 overflow
def check_precision16_overflow_leaves_the_average(dev, graph=False):
    """An inf pitch target (check_precision16_overflow_skips_the_window's) at precision 16: the skipped step leaves `flat.ema` bitwise
    alone (skipped == 1, t == 0); the next clean step moves it; a second overflow -- now that weights and average differ, so that an
    update launch that ignored the flag WOULD move the average -- leaves it bitwise alone again."""
    train, _, net, x, y = _setup(dev)
    step = train.TrainStep(net, **step_kw(16, graph=graph))
    f = step.flat
    bad = dict(x, pitch=x["pitch"].clone())
    bad["pitch"][0, 0] = float("inf")
    e0 = f.ema.clone()
    step.step(bad, y)
    assert step.skipped == 1 and step.t == 0 and same_bits(f.ema, e0)
    step.step(x, y)
    assert step.skipped == 1 and step.t == 1 and not torch.equal(f.ema, e0) and bool(torch.isfinite(f.ema).all())
    e1, p1 = f.ema.clone(), f.data.clone()
    assert not torch.equal(e1, p1)
    step.step(bad, y)
    assert step.skipped == 2 and step.t == 1 and same_bits(f.ema, e1) and same_bits(f.data, p1)


# ------------------------------------------------------------------------------------------------ 11. off is off
def check_off_is_off(dev, records=None):
    out = []
    for kw in ({}, {"ema_decay": None}):
        train, _, net, x, y = _setup(dev)
        step = train.TrainStep(net, lr=LR, **kw)
        assert not hasattr(step.flat, "ema")
        got = None
        if records is not None:
            with records() as got:
                step.step(x, y)
        else:
            step.step(x, y)
        assert "ema" not in step.state_dict()
        out.append((sorted(vars(step)), sorted(vars(step.flat)), sorted(vars(step._opt)), step.flat.data.cpu().clone(), got))
    a, b = out
    assert a[:3] == b[:3] and same_bits(a[3], b[3]) and a[4] == b[4] and (records is None or len(a[4]) > 100)
    assert not any("ema" in name for name in a[0] + a[1] + a[2])
    assert records is None or not any("ema" in name or "swap" in name for name, _ in a[4])


# ------------------------------------------------------------------------------------------------ 12. ema_weights()
def _eval_mel(net, x):
    xe = {"phoneme": x["phoneme"], "phoneme_mask": x["phoneme_mask"], "duration_forced": x["duration"]}
    net.eval()
    with torch.no_grad():
        mel = net(xe)[0].clone()
    net.train()
    return mel


def _net_from(sd, dev):
    """A fresh fixture net holding the 'phoneme2mel.<key>' weights `sd`."""
    _, _, net, _, _ = _setup(dev)
    net.load_state_dict({k[len("phoneme2mel."):]: v for k, v in sd.items()}, strict=True)
    return net


def check_ema_weights(dev, bitwise):
    """Inside the context the two buffers are exchanged and `net` computes what a fresh net loaded from ema_state_dict() computes; after
    it both are bitwise back, and the next step is the step of a twin that never opened it.  bitwise: the simulator's comparisons; on the
    GPU the mel is held to 1e-4 (the inference tests' bound against the oracle) and the next step to the captured-step tolerances."""
    import pytest
    steps = []
    for _ in range(2):
        train, _, net, x, y = _setup(dev)
        steps.append(train.TrainStep(net, **step_kw(32)))
        steps[-1].step(x, y)
    a, twin = steps
    f = a.flat
    p, e = f.data.clone(), f.ema.clone()
    want = _eval_mel(_net_from(a.ema_state_dict(), dev), x)
    raw = _eval_mel(a.net, x)                                     # (fills the inference path's packed copies with the RAW weights)
    with a.ema_weights() as inside:
        assert inside is a and same_bits(f.data, e) and same_bits(f.ema, p)
        got = _eval_mel(a.net, x)
        for call in (lambda: a.step(x, y), a.flush, a.state_dict, lambda: a.load_state_dict({}), lambda: a.ema_weights().__enter__()):
            with pytest.raises(RuntimeError, match=r"ema_weights\(\)"):
                call()
        assert same_bits(f.data, e) and same_bits(f.ema, p)
    assert same_bits(f.data, p) and same_bits(f.ema, e)
    diff = float((got - want).abs().max())
    print(f"mel on the averaged weights vs a fresh net loaded from ema_state_dict(): largest difference {diff:.3e}")
    assert float((got - raw).abs().max()) > 1e-4, "the averaged weights compute what the raw ones do: the check shows nothing"
    assert torch.equal(got, want) if bitwise else diff <= 1e-4, diff
    assert torch.equal(_eval_mel(a.net, x), raw)                  # ... and the packed copies followed the weights back
    la, lt = a.step(x, y), twin.step(x, y)
    if bitwise:
        assert same_bits(la, lt) and same_bits(f.data, twin.flat.data) and same_bits(f.ema, twin.flat.ema)
    else:
        assert torch.allclose(la, lt, rtol=1e-5, atol=0) and torch.allclose(f.data, twin.flat.data, rtol=1e-4, atol=1e-6)
        assert torch.allclose(f.ema, twin.flat.ema, rtol=1e-4, atol=1e-6)
    p, e = f.data.clone(), f.ema.clone()
    with pytest.raises(RuntimeError, match="boom"):               # an exception inside still exchanges back
        with a.ema_weights():
            raise RuntimeError("boom")
    assert same_bits(f.data, p) and same_bits(f.ema, e) and not a._ema_open


def check_ema_weights_needs_ema_decay(dev):
    import pytest
    train, _, net, x, y = _setup(dev)
    step = train.TrainStep(net)
    for call in (lambda: step.ema_weights().__enter__(), step.ema_state_dict, lambda: step.evaluate(x, y, ema=True)):
        with pytest.raises(AttributeError, match="ema_decay"):
            call()


# ------------------------------------------------------------------------------------------------ 13. evaluate
def check_evaluate_returns_the_steps_losses(dev, precision, bitwise):
    """evaluate(ema=False) then step(): the same five losses (the step's forward reads the same weights).  -> the largest relative
    difference."""
    train, _, net, x, y = _setup(dev)
    kw = step_kw(precision)
    del kw["ema_decay"]
    step = train.TrainStep(net, **kw)                             # (a step without the average: evaluate works there too)
    step.step(x, y)
    ev = step.evaluate(x, y, ema=False).clone()
    assert same_bits(ev, step.evaluate(x, y))                     # (ema=None without an average: the raw weights)
    st = step.step(x, y)
    rel = float(((ev - st).abs() / st.abs()).max())
    print(f"precision {precision}: evaluate vs step, largest relative difference {rel:.3e}")
    assert ev.shape == (5,) and (same_bits(ev, st) if bitwise else rel <= 1e-6), (ev, st)
    return rel


def check_evaluate_on_the_average(dev, bitwise):
    """evaluate(ema=True) == evaluate(ema=False) of a twin step whose net was loaded from ema_state_dict(); ema=None means True here."""
    train, _, net, x, y = _setup(dev)
    step = train.TrainStep(net, **step_kw(32))
    step.step(x, y)
    twin = train.TrainStep(_net_from(step.ema_state_dict(), dev), lr=LR)
    got, want, raw = step.evaluate(x, y, ema=True), twin.evaluate(x, y, ema=False), step.evaluate(x, y, ema=False)
    assert same_bits(got, step.evaluate(x, y)) and not torch.equal(got, raw)
    assert same_bits(got, want) if bitwise else torch.allclose(got, want, rtol=1e-6, atol=0), (got, want)
    with step.ema_weights():                                      # inside the context the weights already are the average
        assert same_bits(step.evaluate(x, y), got) and same_bits(step.evaluate(x, y, ema=False), got)


def check_evaluate_changes_nothing(dev):
    """Precision 16 (a scaler block and a hyper block), N = 2 with the window open, an average that differs from the weights: every
    buffer and counter is bitwise what it was after evaluate on either set of weights."""
    micro = [(_to(a, dev), _to(b, dev)) for a, b in fixture_micro()[0]]
    train, _, net, _, _ = _setup(dev)
    step = train.TrainStep(net, **step_kw(16, accumulate_grad_batches=2))
    for x, y in micro:
        step.step(x, y)
    f, o = step.flat, step._opt
    assert step.micro == 1 and step.t == 1 and bool(f.acc.any()) and bool(f.grad.any()) and not torch.equal(f.ema, f.data)
    buffers = {"data": f.data, "ema": f.ema, "grad": f.grad, "m": f.m, "v": f.v, "acc": f.acc, "scaler": o.scaler, "hyper": o.hyper,
               "count": o._count, "absmax": o.absmax}
    snap = {k: v.clone() for k, v in buffers.items()}
    losses = [step.evaluate(*micro[0], ema=e) for e in (True, False, None)]
    assert all(bool(torch.isfinite(l).all()) for l in losses) and not torch.equal(losses[0], losses[1])
    for k, v in buffers.items():
        assert same_bits(v, snap[k]), k
    assert step.micro == 1 and step.t == 1 and step.skipped == 0
    step.step(*micro[1])                                          # the window closes as if nothing had happened
    assert step.micro == 0 and step.t == 2


# ------------------------------------------------------------------------------------------------ 14. checkpoint
def check_checkpoint(dev, bitwise, graph=False):
    """Two steps, state_dict(), a fresh EMA step (graph: captured) loads it, one more step on both: the same weights and averages."""
    import pytest
    from efficientspeech_amd import EfficientSpeech
    train, _, net, x, y = _setup(dev)
    a = train.TrainStep(net, **step_kw(32, graph=graph))
    for _ in range(2):
        a.step(x, y)
    ckpt = a.state_dict()
    assert ckpt["ema"]["decay"] == DECAY and set(ckpt["ema"]["state_dict"]) == set(ckpt["state_dict"])
    t2, _, net2, _, _ = _setup(dev)
    b = t2.TrainStep(net2, **step_kw(32, graph=graph))
    b.load_state_dict(ckpt)
    assert same_bits(b.flat.ema, a.flat.ema) and same_bits(b.flat.data, a.flat.data) and not torch.equal(b.flat.ema, b.flat.data)
    a.step(x, y)
    b.step(x, y)
    assert a.t == b.t == 3
    for name in ("data", "ema"):
        ta, tb = getattr(a.flat, name), getattr(b.flat, name)
        assert same_bits(ta, tb) if bitwise else torch.allclose(ta, tb, rtol=1e-4, atol=1e-6), name
    # a checkpoint without an average: it starts from the loaded weights
    plain = {k: v for k, v in ckpt.items() if k != "ema"}
    b.load_state_dict(plain)
    assert same_bits(b.flat.ema, b.flat.data) and same_bits(b.flat.data, _flat_of(b, ckpt["state_dict"]))
    # another decay is refused, before anything is loaded; a step without an average ignores the entry
    t3, _, net3, _, _ = _setup(dev)
    c = t3.TrainStep(net3, lr=LR, ema_decay=0.99)
    before = c.flat.data.clone()
    with pytest.raises(RuntimeError, match="ema_decay"):
        c.load_state_dict(ckpt)
    assert same_bits(c.flat.data, before)
    t4, _, net4, _, _ = _setup(dev)
    d = t4.TrainStep(net4, lr=LR)
    d.load_state_dict(ckpt)
    assert not hasattr(d.flat, "ema") and "ema" not in d.state_dict()
    # the exported average builds a model
    model = EfficientSpeech.load_from_checkpoint({"state_dict": a.ema_state_dict(), "hyper_parameters": a.hyper_parameters()})
    got = dict(model.phoneme2mel.named_parameters())
    for k, p, sl in zip(a.flat.names, a.flat.params, a.flat.slices):
        assert same_bits(got[k], a.flat.ema[sl].view(p.shape)), k
    outside = [k for k in got if k not in set(a.flat.names)]
    assert outside and all(same_bits(got[k], dict(a.net.named_parameters())[k]) for k in outside)


def _flat_of(step, sd):
    out = torch.zeros_like(step.flat.data)
    for k, sl in zip(step.flat.names, step.flat.slices):
        out[sl] = sd["phoneme2mel." + k].reshape(-1).to(out.device)
    return out


# ------------------------------------------------------------------------------------------------ 16. fit
def check_fit(dev):
    """Two epochs, check_val_every_n_epoch = 2, a two-batch val_loader: only the second record has `val_losses`, the mean of evaluate
    over the two batches at the end of that epoch; without a val_loader the records' keys are today's."""
    micro = [(_to(a, dev), _to(b, dev)) for a, b in fixture_micro()[0]]
    train, _, net, _, _ = _setup(dev)
    step = train.TrainStep(net, lr=LR, ema_decay=DECAY)
    hist = train.fit(step, micro[2:], epochs=2, device=dev, first_epoch=60, val_loader=micro[:2], check_val_every_n_epoch=2)
    assert [sorted(r) for r in hist] == [["epoch", "losses", "lr"], ["epoch", "losses", "lr", "val_losses"]] and step.t == 2
    want = torch.stack([step.evaluate(x, y) for x, y in micro[:2]]).mean(0).cpu()
    assert torch.allclose(torch.tensor(hist[1]["val_losses"]), want, rtol=1e-6, atol=0), (hist[1], want)
    on_raw = torch.stack([step.evaluate(x, y, ema=False) for x, y in micro[:2]]).mean(0).cpu()
    assert not torch.allclose(want, on_raw, rtol=1e-6, atol=0)    # (the validation ran on the average)
    train, _, net, _, _ = _setup(dev)
    step = train.TrainStep(net, lr=LR)
    hist = train.fit(step, micro[2:], epochs=2, device=dev, first_epoch=60)
    assert [sorted(r) for r in hist] == [["epoch", "losses", "lr"]] * 2


# ------------------------------------------------------------------------------------------------ 17. arguments
def check_arguments():
    import pytest
    from efficientspeech_amd import EfficientSpeech
    train, _, net, _, _ = _setup("cpu")
    before = [p.data_ptr() for p in net.parameters()]
    for bad in (True, False, "0.9", 0.0, 1.0, -0.5, 1.5, 0, 1, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="ema_decay"):
            train.TrainStep(net, ema_decay=bad)
    assert before == [p.data_ptr() for p in net.parameters()]      # (refused before the parameters were re-homed)
    step = train.TrainStep(net, ema_decay=0.999)
    assert step.flat.ema.data_ptr() % 16 == 0 and same_bits(step.flat.ema, step.flat.data)
    assert step._opt.on_device is False                            # the average alone does not move the optimizer's scalars to the device
    via = EfficientSpeech.from_config("tiny").make_train_step(ema_decay=0.9)
    assert via.flat.ema.shape == via.flat.data.shape
