"""Checks of the per-phoneme prosody curves: a (B, T) tensor under `pitch_control` / `energy_control` / `duration_control`
(esmi_prosody_curves and the three *_curve_f32 entry points).  tests/test_prosody_curves.py runs them twice: through the wave simulator
(host tensors, inside `tests.simlib.use_sim()`) and on the device.

The method is tests/prosody_control_checks.py's: what is bucketized is `pred[b,t] * curve[b,t]`, what is rounded is
`rintf(duration_pred[b,t] * curve[b,t])`, one fp32 multiply of the fp32 prediction the kernels write to their taps -- so the expected
decisions are computed in numpy fp32 from the path's OWN raw predictions, and the mel is compared with the oracle run teacher-forced
on those same products and durations.  A padding position never uses its entry (the scale there is 1): the expectation says so too."""
import contextlib
import ctypes as C
import os

import numpy as np
import pytest
import torch

from efficientspeech_amd import _lib, networks
from oracle import oracle
from tests import helpers as H
from tests import prosody_control_checks as P

SHAPE = P.SHAPE                                              # B = 3, T = 17, lengths (17, 9, 1)
VALUES = np.array([0.5, 0.75, 1.25, 1.5], np.float32)
# The seed of the curve values.  test_curve_seed_moves_half_of_the_oracles_decisions (CPU, no kernels) shows that on the ORACLE's
# free-running predictions alone these values move at least half of the live decisions of each kind, for tiny, small and base, at
# the fixed shape, at B == 1 and at the device tier's other shapes: the guard `changed >= 0.5` of check_case is a condition the inputs meet, not a measurement.
CURVE_SEED = 5
QUANTITIES = ("pitch", "energy", "duration")
DECISIONS = ("pitch_idx", "energy_idx", "dur", "cum", "mel_len")

_plain = {}


def clear():
    _plain.clear()
    P.clear()


def curve_values(B, T, seed=CURVE_SEED):
    """{quantity: (B, T) fp32}: each phoneme's value drawn from VALUES by a fixed seed"""
    return {k: VALUES[np.random.default_rng([seed, q]).integers(0, len(VALUES), size=(B, T))] for q, k in enumerate(QUANTITIES)}


def as_controls(curves, device):
    return {k + "_control": torch.from_numpy(np.ascontiguousarray(v, np.float32)).to(device) for k, v in curves.items()}


def plain(name, plan, entry, device, shape, build=""):
    """the call without controls (shared by the checks of a case; `build`: the bound library when it is not the default one)"""
    key = (name, plan, entry, device, shape, build)
    if key not in _plain:
        net, _, _ = P.net_of(name, device)
        _plain[key] = P.run(net, P.inputs(*shape, device)[0], entry, plan)
    return _plain[key]


def expected_decisions(raw, sd, mask, curves):
    """numpy fp32 restatement of the semantics on raw predictions (a dict with pitch / energy / duration (B, T)); `curves` may leave a
    quantity out (scale 1) or give it as (B,) / a number.  -> dict: the scaled pitch / energy (vp, ve) and the five decisions"""
    B, T = raw["pitch"].shape
    s = {}
    for k in QUANTITIES:
        c = np.asarray(curves.get(k, 1.0), np.float32)
        c = np.broadcast_to(c[:, None] if c.ndim == 1 else c, (B, T)).copy()
        if mask is not None and np.asarray(curves.get(k, 1.0)).ndim == 2:
            c[mask] = 1.0                                    # a curve's entry at a padding position is never used
        s[k] = c
    vp, ve = raw["pitch"] * s["pitch"], raw["energy"] * s["energy"]
    assert vp.dtype == np.float32 and ve.dtype == np.float32
    pi = np.searchsorted(sd["encoder.pitch_decoder.pitch_bins"].astype(np.float32), vp, side="left").astype(np.int32)
    ei = np.searchsorted(sd["encoder.energy_decoder.energy_bins"].astype(np.float32), ve, side="left").astype(np.int32)
    d = np.maximum(np.rint(raw["duration"] * s["duration"]), 0.0).astype(np.int32)
    if mask is not None:
        d[mask] = 0
    cum = np.cumsum(d, 1).astype(np.int32)
    return dict(vp=vp, ve=ve, pitch_idx=pi, energy_idx=ei, dur=d, cum=cum, mel_len=cum[:, -1].copy())


def live_of(mask, B, T):
    return np.ones((B, T), bool) if mask is None else ~mask


def changed_fraction(a, b, live):
    return {k: float((a[k] != b[k])[live].mean()) for k in ("dur", "pitch_idx", "energy_idx")}


def check_seed_on_the_oracle(name, shape):
    """the guard's condition on the oracle's free-running predictions alone (CPU, no kernel)"""
    B, T, _ = shape
    _, cfg, sd = P.net_of(name, "cpu")
    _, ids, mask = P.inputs(B, T, shape[2], "cpu")
    o = P.free_running(name, shape)
    raw = {k: np.ascontiguousarray(getattr(o, k)[..., 0], np.float32) for k in QUANTITIES}
    with_curves = expected_decisions(raw, sd, mask, curve_values(B, T))
    without = expected_decisions(raw, sd, mask, {})
    changed = changed_fraction(with_curves, without, live_of(mask, B, T))
    print(f"{name} {shape}: oracle decisions changed {changed}")
    assert min(changed.values()) >= 0.5, changed


def check_case(name, plan, entry, device, shape=SHAPE, build=""):
    """Check 1 of one (config, plan, entry point, shape): decisions bit-exact and really changed, raw predictions untouched, mel
    against the teacher-forced oracle, exact zeros behind mel_len, the serving call.  -> the run with curves."""
    B, T, lens = shape
    net, cfg, sd = P.net_of(name, device)
    x, ids, mask = P.inputs(B, T, lens, device)
    curves = curve_values(B, T)
    base = plain(name, plan, entry, device, shape, build)
    got = P.run(net, dict(x, **as_controls(curves, device)), entry, plan)
    e = expected_decisions(got, sd, mask, curves)
    changed = changed_fraction(got, base, live_of(mask, B, T))
    print(f"{name} plan {plan} {entry} {shape}: changed {changed}, mel_len {base['mel_len'].tolist()} -> {got['mel_len'].tolist()}")
    for k in DECISIONS:
        assert np.array_equal(got[k], e[k]), (k, np.argwhere(got[k] != e[k])[:4].tolist())
    assert min(changed.values()) >= 0.5, changed             # (a condition, not a measurement: see CURVE_SEED)
    o_free = P.free_running(name, shape)
    for k in QUANTITIES:                                     # the raw predictions are the plain call's, and the oracle's
        assert np.array_equal(got[k], base[k]), k
        np.testing.assert_allclose(got[k], getattr(o_free, k)[..., 0], atol=H.PRED_TOL, rtol=0)
    o = oracle.phoneme2mel(cfg, oracle.Weights(sd), ids, mask, pitch=e["vp"], energy=e["ve"], duration=e["dur"])
    assert np.array_equal(o.pitch_idx, e["pitch_idx"]) and np.array_equal(o.energy_idx, e["energy_idx"]) and np.array_equal(o.dur, e["dur"])
    assert np.array_equal(got["mel_len"], o.mel_len)
    assert got["mel"].shape == o.mel.shape, (got["mel"].shape, o.mel.shape)
    err = float(np.abs(got["mel"] - o.mel).max())
    print(f"    mel L-inf vs teacher-forced oracle {err:.2e}")
    assert err < H.MEL_TOL, err
    for b in range(B):
        assert not got["mel"][b, int(got["mel_len"][b]):].any(), b
    if entry == "forward":      # the serving call (no taps: the one-launch kernel skips the stores nobody reads) gives the same result
        with torch.no_grad(), _lib.launch_plan(plan):
            mel, ml, dp = net(dict(x, **as_controls(curves, device)))
        assert np.array_equal(mel.cpu().numpy(), got["mel"]) and np.array_equal(ml.cpu().numpy(), got["mel_len"])
        assert np.array_equal(dp.cpu().numpy()[..., 0], got["duration"])
    return got


# ---------------------------------------------------------------------------------------------------------------- 2. row indexing
ROW_SHAPE = (2, 21, (21, 19))        # T = 21: no multiple of 4 or 16, two 16-row tiles; utterance 1 (b > 0) ends at row 18
ROW_B = 1
ROW_TS = (0, 15, 16, 18)             # first row, both sides of the 16-row tile edge, the last live row
_PITCH_TRY = (1.5, 0.5, 2.0, 0.25, 4.0, -1.0, 8.0, -8.0, 64.0, -64.0)
_DUR_TRY = (1.5, 0.5, 2.0, 3.0, 0.0, 8.0, 64.0, 1e3, 1e6)


def _moving_values(base, sd, mask, b, t):
    """a value per quantity that moves the decision at (b, t), chosen from the raw prediction there (the first of a fixed list that
    does): the test must not pass on a value that happens to leave the decision where it was"""
    B, T = base["pitch"].shape
    out = {}
    for k, tries, dec in (("pitch", _PITCH_TRY, "pitch_idx"), ("energy", _PITCH_TRY, "energy_idx"), ("duration", _DUR_TRY, "dur")):
        for v in tries:
            c = np.ones((B, T), np.float32)
            c[b, t] = v
            if expected_decisions(base, sd, mask, {k: c})[dec][b, t] != base[dec][b, t]:
                out[k] = np.float32(v)
                break
        else:
            raise AssertionError(f"no value moves {dec} at {(b, t)}: raw prediction {base[k][b, t]!r}")
    return out


def check_row_indexing(name, plan, entry, device, ts=ROW_TS, shape=ROW_SHAPE, b=ROW_B):
    """2. curves of 1.0 except at ONE phoneme (b, t): the decisions differ from the plain call's at that phoneme only (duration: `dur`
    there, `cum` from t on, mel_len[b]), and are the expected ones"""
    B, T, lens = shape
    net, _, sd = P.net_of(name, device)
    x, _, mask = P.inputs(B, T, lens, device)
    base = plain(name, plan, entry, device, shape)
    for t in ts:
        assert t < lens[b]
        vals = _moving_values(base, sd, mask, b, t)
        curves = {k: np.ones((B, T), np.float32) for k in QUANTITIES}
        for k in QUANTITIES:
            curves[k][b, t] = vals[k]
        got = P.run(net, dict(x, **as_controls(curves, device)), entry, plan)
        e = expected_decisions(got, sd, mask, curves)
        for k in DECISIONS:
            assert np.array_equal(got[k], e[k]), (k, t, np.argwhere(got[k] != e[k])[:4].tolist())
        for k in ("pitch_idx", "energy_idx", "dur"):
            diff = np.argwhere(got[k] != base[k]).tolist()
            assert diff == [[b, t]], (k, t, diff)
        delta = int(got["dur"][b, t]) - int(base["dur"][b, t])
        want_cum = base["cum"].copy()
        want_cum[b, t:] += delta
        assert delta != 0 and np.array_equal(got["cum"], want_cum), t
        assert got["mel_len"].tolist() == [int(m) + (delta if r == b else 0) for r, m in enumerate(base["mel_len"])]
        for k in QUANTITIES:
            assert np.array_equal(got[k], base[k]), k


# ---------------------------------------------------------------------------------------------------------------- 3. identities
def same(a, b, keys=P.TAPS + ("mel",)):
    for k in keys:
        assert np.array_equal(a[k], b[k]), k


def same_where_it_counts(a, b, mask):
    """everything bit for bit; the pitch / energy index at the live positions (at a padding position a curve is not used -- the index
    stored there is the raw prediction's -- while a (B,) control scales the padding rows' predictions too; the embedding row is zero
    there either way)"""
    same(a, b, ("pitch", "energy", "duration", "dur", "cum", "mel_len", "mel"))
    live = live_of(mask, *a["pitch_idx"].shape)
    for k in ("pitch_idx", "energy_idx"):
        assert np.array_equal(a[k][live], b[k][live]), k


def check_identities(name, plan, entry, device, shape=SHAPE):
    """3. all-ones curves == the plain call; curves constant per utterance == the (B,) controls; a mixed call (pitch curve, (B,)
    energy, a number for the duration) == the same three as curves, and the expected decisions"""
    B, T, lens = shape
    net, _, sd = P.net_of(name, device)
    x, _, mask = P.inputs(B, T, lens, device)
    base = plain(name, plan, entry, device, shape)
    ones = {k: np.ones((B, T), np.float32) for k in QUANTITIES}
    same(P.run(net, dict(x, **as_controls(ones, device)), entry, plan), base)
    per_utt = P.run(net, dict(x, **P.controls(B, device)), entry, plan)
    const = {k: np.repeat(np.asarray(P.SCALES[k][:B], np.float32)[:, None], T, 1) for k in QUANTITIES}
    got = P.run(net, dict(x, **as_controls(const, device)), entry, plan)
    same_where_it_counts(got, per_utt, mask)
    assert not np.array_equal(got["dur"], base["dur"])
    # mixed forms
    curves = curve_values(B, T)
    mixed = dict(pitch=curves["pitch"], energy=np.asarray(P.SCALES["energy"][:B], np.float32), duration=0.75)
    xm = dict(x, pitch_control=torch.from_numpy(mixed["pitch"]).to(device), energy_control=torch.from_numpy(mixed["energy"]).to(device),
              duration_control=0.75)
    got = P.run(net, xm, entry, plan)
    e = expected_decisions(got, sd, mask, mixed)
    for k in DECISIONS:
        assert np.array_equal(got[k], e[k]), (k, np.argwhere(got[k] != e[k])[:4].tolist())
    as_curves = dict(pitch=mixed["pitch"], energy=np.repeat(mixed["energy"][:, None], T, 1), duration=np.full((B, T), 0.75, np.float32))
    same_where_it_counts(P.run(net, dict(x, **as_controls(as_curves, device)), entry, plan), got, mask)
    assert not np.array_equal(got["pitch_idx"], base["pitch_idx"]) and not np.array_equal(got["dur"], base["dur"])


# ---------------------------------------------------------------------------------------------------------------- 4. padding
def check_padding_is_never_used(name, plan, entry, device, shape=SHAPE):
    """4. NaN and 1e30 at the masked positions: bit-identical to 1.0 there, taps and mel (B > 1)"""
    B, T, lens = shape
    net, _, _ = P.net_of(name, device)
    x, _, mask = P.inputs(B, T, lens, device)
    assert B > 1 and mask.any()
    curves = curve_values(B, T)
    clean = {k: np.where(mask, np.float32(1.0), v) for k, v in curves.items()}
    want = P.run(net, dict(x, **as_controls(clean, device)), entry, plan)
    for junk in (np.float32("nan"), np.float32(1e30)):
        dirty = {k: np.where(mask, junk, v) for k, v in curves.items()}
        same(P.run(net, dict(x, **as_controls(dirty, device)), entry, plan), want)


def check_single_utterance(name, plan, entry, device):
    """5. B == 1 takes no mask (the reference's path, networks.py:338, :383-384)"""
    check_case(name, plan, entry, device, shape=(1, 17, (17,)))


# ---------------------------------------------------------------------------------------------------------------- 8. errors
def check_value_errors(device):
    """8a. what the Python layer refuses, on both paths, before anything is launched"""
    net, _, _ = P.net_of("tiny", device)
    B, T, _ = SHAPE
    x = P.inputs(*SHAPE, device)[0]
    forced = torch.full((B, T), 2, dtype=torch.int32, device=device)
    calls = (lambda xx: net(xx), lambda xx: net.encoder._encode(xx))
    ones = lambda *s: torch.ones(s, dtype=torch.float32, device=device)      # noqa: E731
    with torch.no_grad():
        for k in networks.CONTROL_KEYS:
            for bad in (ones(B, T + 1), ones(B, T - 1), ones(T), ones(B, T, 1), ones(T, B)):
                for call in calls:
                    with pytest.raises(ValueError, match=rf"\({B}, {T}\)"):      # (the message names every accepted shape)
                        call(dict(x, **{k: bad}))
            with pytest.raises(ValueError, match="train"):
                net(dict(x, **{k: ones(B, T)}), train=True)
            with pytest.raises(ValueError, match="train"):
                net.encoder._encode(dict(x, **{k: ones(B, T)}), train=True)
        for call in calls:
            with pytest.raises(ValueError, match="duration_forced"):
                call(dict(x, duration_control=ones(B, T), duration_forced=forced))
            call(dict(x, pitch_control=ones(B, T), energy_control=ones(B, T), duration_forced=forced))   # (allowed: other quantities)


def check_abi_errors(device, launches=None):
    """8b. through ctypes: a curve together with the same quantity's teacher / forced pointer is ESMI_ERR_ARG from each of the three
    *_curve_f32 entry points, nothing launched (`launches`, simulator: a context manager collecting launch names), the output buffers
    untouched.  The same arguments without the conflict are a valid call."""
    net, cfg, _ = P.net_of("tiny", device)
    B, T, _ = SHAPE
    x = P.inputs(*SHAPE, device)[0]
    dim = cfg.dim
    with torch.no_grad(), networks._on_device_of(net.decoder.mel_linear.weight):
        net(x)                                                   # (weights packed, attributes set: not part of what is counted below)
        lib, stream = networks._runtime(net.decoder.mel_linear.weight)
        f32 = lambda *s: torch.full(s, -7.0, dtype=torch.float32, device=device)     # noqa: E731
        i32 = lambda *s: torch.full(s, -7, dtype=torch.int32, device=device)         # noqa: E731
        curve = torch.full((B, T), 1.5, dtype=torch.float32, device=device)
        p = lambda t: t.data_ptr()                                                   # noqa: E731
        (pw, _), (ew, _), (dw, _) = net.encoder._predictors(lib, stream)
        feat, preds, idx, dur = f32(B, T, 4 * dim), f32(3, B, T), i32(2, B, T), i32(B, T)
        ws = torch.empty(lib.esmi_fuse_variance_adaptor_workspace_bytes(B, T, dim, cfg.depth), dtype=torch.uint8, device=device)
        tgt_f, tgt_i = torch.zeros((B, T), dtype=torch.float32, device=device), torch.zeros((B, T), dtype=torch.int32, device=device)
        fw, _ = net.encoder.fuse._packed(lib, stream)
        feats, bm = net.encoder.encoder._run(x["phoneme"], x["phoneme_mask"])
        fp = (C.c_void_p * cfg.depth)(*[p(f) for f in feats])
        ni = (C.c_int * cfg.depth)(*[f.shape[1] for f in feats])
        outputs = (feat, preds, idx, dur)
        before = [t.clone() for t in outputs]
        with (launches() if launches else contextlib.nullcontext([])) as seen:
            for which in range(3):
                ctl = _lib.ProsodyCurves()
                setattr(ctl, ("pitch_scale", "energy_scale", "duration_scale")[which], p(curve))
                setattr(ctl, ("pitch_per_phoneme", "energy_per_phoneme", "duration_per_phoneme")[which], 1)
                tg = [p(tgt_f) if which == 0 else None, p(tgt_f) if which == 1 else None, p(tgt_i) if which == 2 else None]
                with pytest.raises(RuntimeError, match="ESMI_ERR_ARG"):
                    lib.esmi_variance_adaptor_curve_f32(C.byref(pw), C.byref(ew), C.byref(dw), dim, B, T, p(bm[0]), *tg, p(feat), p(preds[0]),
                                                        p(preds[1]), p(preds[2]), p(idx[0]), p(idx[1]), p(dur), p(ws), ws.numel(), stream,
                                                        C.byref(ctl))
                with pytest.raises(RuntimeError, match="ESMI_ERR_ARG"):
                    lib.esmi_fuse_variance_adaptor_curve_f32(C.byref(fw), cfg.depth, dim, net.encoder.fuse.kernel_size, B, T, fp, ni,
                                                             C.byref(pw), C.byref(ew), C.byref(dw), p(bm[0]), *tg, p(feat), p(preds[0]),
                                                             p(preds[1]), p(preds[2]), p(idx[0]), p(idx[1]), p(dur), None, None, None, None,
                                                             _lib.current_plan(), p(ws), ws.numel(), stream, C.byref(ctl))
            # the one-call forward: a duration curve next to dur_forced.  The Python layer refuses that combination itself, so hand the
            # library the curve behind its back
            real = networks._prosody_controls
            ctl = _lib.ProsodyCurves()
            ctl.duration_scale, ctl.duration_per_phoneme = p(curve), 1
            networks._prosody_controls = lambda *a, **k: (ctl, (curve,))
            try:
                with pytest.raises(RuntimeError, match="esmi_phoneme2mel_forward_curve_f32 failed: ESMI_ERR_ARG"):
                    net._launch(dict(x, duration_forced=tgt_i + 2))
            finally:
                networks._prosody_controls = real
        assert not [k for k in seen if not k.startswith(("hip", "memset"))], seen
        if str(device).startswith("cuda"):
            torch.cuda.synchronize()
        for t, b4 in zip(outputs, before):
            assert torch.equal(t, b4)
        # ... and the same arguments without the conflict are a valid call that writes them
        ctl = _lib.ProsodyCurves()
        ctl.pitch_scale, ctl.pitch_per_phoneme = p(curve), 1
        lib.esmi_fuse_variance_adaptor_curve_f32(C.byref(fw), cfg.depth, dim, net.encoder.fuse.kernel_size, B, T, fp, ni, C.byref(pw),
                                                 C.byref(ew), C.byref(dw), p(bm[0]), None, p(tgt_f), p(tgt_i), p(feat), p(preds[0]), p(preds[1]),
                                                 p(preds[2]), p(idx[0]), p(idx[1]), p(dur), None, None, None, None, _lib.current_plan(), p(ws),
                                                 ws.numel(), stream, C.byref(ctl))
        if str(device).startswith("cuda"):
            torch.cuda.synchronize()
        assert not torch.equal(dur, before[3]) and not torch.equal(idx[0], before[2][0])


# ---------------------------------------------------------------------------------------------------------------- 9. host plumbing
SCHED_LENGTHS = [9, 4, 9, 7, 3, 8, 13]     # (max_batch 2, granularity 4: three pairs and a single request, the B == 1 path)


def scheduler_controls(lengths):
    """per request: a curve of its own length, or a number -- every second request's pitch is a number, request 5 has no curve at all"""
    rng = np.random.default_rng(11)
    pitch = [VALUES[rng.integers(0, 4, size=n)] if i % 2 == 0 else float(VALUES[i % 4]) for i, n in enumerate(lengths)]
    dur = [VALUES[rng.integers(0, 4, size=n)] if i != 5 else 1.25 for i, n in enumerate(lengths)]
    return {"pitch_control": pitch, "duration_control": dur}


def batch_controls_by_hand(ctl, idx, lengths, T):
    """what a batch must get: (B,) while every request of it carries a number, else (B, T) rows in batch order, 1.0 behind each end"""
    out = {}
    for k, per in ctl.items():
        if all(np.ndim(per[i]) == 0 for i in idx):
            out[k] = np.array([per[i] for i in idx], np.float32)
            continue
        c = np.ones((len(idx), T), np.float32)
        for r, i in enumerate(idx):
            c[r, :lengths[i]] = per[i]
        out[k] = c
    return out


def check_scheduler_batches():
    """9a. (host only: a recording stand-in for the network) per-request curves of different lengths land in their batches padded
    with 1.0 and in batch order; numbers fill their request's row, and a batch of numbers only keeps the (B,) form"""
    from types import SimpleNamespace
    from efficientspeech_amd.scheduler import BucketedSynthesizer
    lengths = SCHED_LENGTHS
    seqs = [np.arange(1, n + 1, dtype=np.int32) for n in lengths]
    seen = []

    def net(x):
        seen.append(x)
        B, T = x["phoneme"].shape
        return torch.zeros(B, 2, 80), torch.full((B,), 2, dtype=torch.int32), torch.zeros(B, T, 1)
    net.decoder = SimpleNamespace(mel_linear=SimpleNamespace(weight=torch.zeros(1)))
    synth = BucketedSynthesizer(net, max_batch=2, granularity=4)
    ctl = scheduler_controls(lengths)
    ctl["energy_control"] = np.linspace(0.5, 1.5, len(lengths)).astype(np.float32)      # (the array-of-numbers form of before, alongside)
    synth(seqs, controls=ctl)
    batches = synth.plan(lengths)
    assert len(seen) == len(batches)
    forms = set()
    for x, (idx, T) in zip(seen, batches):
        want = batch_controls_by_hand({k: v for k, v in ctl.items() if k != "energy_control"}, idx, lengths, T)
        for k, w in want.items():
            assert x[k].dtype == torch.float32 and np.array_equal(x[k].numpy(), w), (k, idx)
            forms.add((k, w.ndim))
        assert np.array_equal(x["energy_control"].numpy(), ctl["energy_control"][idx])
    assert ("pitch_control", 2) in forms and ("duration_control", 2) in forms
    with pytest.raises(ValueError):
        synth(seqs, controls={"pitch_control": [np.ones(n + 1, np.float32) for n in lengths]})       # not the request's own length
    with pytest.raises(ValueError):
        synth(seqs, controls={"pitch_control": [np.ones(n, np.float32) for n in lengths][:-1]})      # not one entry per request


def check_scheduler(device):
    """9b. BucketedSynthesizer(..., controls=...) with per-request curves equals direct net(x) calls on the same plan() batches"""
    from efficientspeech_amd.scheduler import BucketedSynthesizer
    net, _, _ = P.net_of("tiny", device)
    rng = np.random.default_rng(5)
    lengths = SCHED_LENGTHS
    seqs = [rng.integers(1, 40, size=n).astype(np.int32) for n in lengths]
    ctl = scheduler_controls(lengths)
    synth = BucketedSynthesizer(net, max_batch=2, granularity=4)
    got = synth(seqs, controls=ctl)
    plain_out = synth(seqs)
    batches = synth.plan(lengths)
    assert len(batches) >= 3 and any(len(idx) > 1 for idx, _ in batches) and any(len(idx) == 1 for idx, _ in batches)
    differs = 0
    for idx, T in batches:
        ids = np.zeros((len(idx), T), np.int32)
        for r, i in enumerate(idx):
            ids[r, :lengths[i]] = seqs[i]
        x = {"phoneme": torch.from_numpy(ids).to(device)}
        if len(idx) > 1:
            x["phoneme_mask"] = networks.get_mask_from_lengths(torch.tensor([lengths[i] for i in idx], device=device), T)
        for k, v in batch_controls_by_hand(ctl, idx, lengths, T).items():
            x[k] = torch.from_numpy(v).to(device)
        with torch.no_grad():
            mel, mel_len, dur = net(x)
        for r, i in enumerate(idx):
            L = int(mel_len[r])
            assert torch.equal(got[i][0], mel[r, :L]) and torch.equal(got[i][1], dur[r, :lengths[i], 0]), i
            differs += got[i][0].shape != plain_out[i][0].shape
    assert differs >= 3                                           # (the curves reached the requests: most lengths moved)


# ---------------------------------------------------------------------------------------------------------------- 10. the other builds
def check_other_build(which, device):
    """10. libesmi_fp32mfma.so / libesmi_checked.so serve curves: check 1 of tiny ES on that build (its own plain call, its own raw
    predictions)"""
    path = os.path.join(os.path.dirname(_lib.LIB_PATH), which)
    with _lib.use_library(path):
        for entry in ("forward", "encode"):
            check_case("tiny", 63, entry, device, build=which)
    if which == "libesmi_checked.so":        # ... and the validation call itself takes the key
        net, _, _ = P.net_of("tiny", device)
        x = P.inputs(*SHAPE, device)[0]
        xc = dict(x, **as_controls(curve_values(*SHAPE[:2]), device))
        with _lib.use_library(path), torch.no_grad():
            mel, mel_len, _ = net(xc)
        got, got_len, _ = net.check_activation_range(xc)
        assert torch.equal(got_len, mel_len) and torch.equal(got, mel)
