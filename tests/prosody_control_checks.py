"""Checks of the per-utterance prosody controls (`pitch_control`, `energy_control`, `duration_control`; esmi_prosody_control and the
three *_ctl_f32 entry points).  tests/test_prosody_control.py runs them twice: through the wave simulator (host tensors, inside
`tests.simlib.use_sim()`) and on the device.

What is bucketized is `pred * s[b]`, what is rounded is `rintf(duration_pred * s[b])`: one fp32 multiply of the fp32 prediction the
kernels write to their taps.  So the expected decisions are computed in numpy fp32 from the HIP path's OWN raw predictions (one pitch
prediction of small ES sits 2.4e-5 from a bucket edge at the fixed shape: the oracle's prediction, 2e-5 away, may fall on the other
side), and the mel is compared with the oracle run teacher-forced on those same products and durations."""
import ctypes as C

import numpy as np
import pytest
import torch

from efficientspeech_amd import _lib, networks
from efficientspeech_amd.synth import synth_phonemes
from oracle import oracle
from tests import helpers as H

SEED = 1234
SHAPE = (3, 17, (17, 9, 1))                                  # B, T, lengths
SCALES = {"pitch": (1.5, 0.5, 1.25), "energy": (0.5, 1.5, 0.75), "duration": (1.5, 0.75, 1.25)}
PH_SEED = 1234
TAPS = ("pitch", "energy", "duration", "pitch_idx", "energy_idx", "dur", "cum", "mel_len")

_nets, _free, _plain = {}, {}, {}


def clear():
    _nets.clear(), _free.clear(), _plain.clear()


def net_of(name, device):
    if (name, device) not in _nets:
        _nets[name, device] = H.make_net(name, device, SEED)
    return _nets[name, device]


def inputs(B, T, lens, device):
    ids, mask = synth_phonemes(B, T, PH_SEED, list(lens) if B > 1 else None)
    x = {"phoneme": torch.from_numpy(ids).to(device)}
    if B > 1:
        x["phoneme_mask"] = torch.from_numpy(mask).to(device)
    return x, ids, (mask if B > 1 else None)


def controls(B, device, scales=None, rows=None):
    """the three (B,) control tensors: utterance b carries the scales of column rows[b] (default: its own)"""
    scales = scales or SCALES
    rows = list(range(B)) if rows is None else rows
    return {k + "_control": torch.tensor([scales[k][r] for r in rows], dtype=torch.float32, device=device) for k in scales}


def run(net, x, entry, plan):
    """One inference call -> numpy dict: the raw predictions pitch / energy / duration (B,T), the decisions pitch_idx, energy_idx, dur,
    cum (B,T), mel_len (B) and mel (B,L,80).  entry "forward": the one-call forward with its taps; "encode": the module path
    (PhonemeEncoder._encode for the taps, PhonemeEncoder.forward + MelDecoder.forward + the final masked_fill for the mel)."""
    n = lambda t: t.detach().cpu().numpy()      # noqa: E731
    with torch.no_grad(), _lib.launch_plan(plan):
        if entry == "forward":
            with networks._on_device_of(net.decoder.mel_linear.weight):
                st = net._launch(x, taps=True)
            out = {k: n(v) for k, v in st.taps.items()}
            out.update(duration=n(st.duration)[..., 0], mel_len=n(st.mel_len), mel=n(st.mel))
        else:
            with networks._on_device_of(net.decoder.mel_linear.weight):
                enc = net.encoder._encode(x)
            out = {k: n(enc[k]) for k in ("pitch_idx", "energy_idx", "dur", "cum", "mel_len")}
            out.update({k: n(enc[k])[..., 0] for k in ("pitch", "energy", "duration")})
            pe = net.encoder(x)
            mel = net.decoder(pe["features"])
            if pe["masks"] is not None and mel.shape[0] > 1:
                mel = mel.masked_fill(pe["masks"][:, :, :1].expand_as(mel), 0.0)
            assert np.array_equal(n(pe["mel_len"]), out["mel_len"]) and np.array_equal(n(pe["duration"])[..., 0], out["duration"])
            out["mel"] = n(mel)
    return out


def plain(name, plan, entry, device, shape):
    """the call without controls (shared by the checks of a case)"""
    key = (name, plan, entry, device, shape)
    if key not in _plain:
        net, _, _ = net_of(name, device)
        _plain[key] = run(net, inputs(*shape, device)[0], entry, plan)
    return _plain[key]


def free_running(name, shape):
    """the oracle's own eval run on the case's phonemes (shared)"""
    if (name, shape) not in _free:
        _, cfg, sd = net_of(name, "cpu")
        _, ids, mask = inputs(*shape, "cpu")
        _free[name, shape] = oracle.phoneme2mel(cfg, oracle.Weights(sd), ids, mask)
    return _free[name, shape]


def expected_decisions(got, sd, mask, scales):
    """numpy fp32 restatement of the issue's semantics on the path's own raw predictions -> (scaled pitch, scaled energy, pitch_idx,
    energy_idx, dur, cum, mel_len)"""
    s = {k: np.asarray(v, np.float32)[:, None] for k, v in scales.items()}
    vp, ve = got["pitch"] * s["pitch"], got["energy"] * s["energy"]
    assert vp.dtype == np.float32 and ve.dtype == np.float32
    pi = np.searchsorted(sd["encoder.pitch_decoder.pitch_bins"].astype(np.float32), vp, side="left").astype(np.int32)
    ei = np.searchsorted(sd["encoder.energy_decoder.energy_bins"].astype(np.float32), ve, side="left").astype(np.int32)
    d = np.maximum(np.rint(got["duration"] * s["duration"]), 0.0).astype(np.int32)
    if mask is not None:
        d[mask] = 0
    cum = np.cumsum(d, 1).astype(np.int32)
    return vp, ve, pi, ei, d, cum, cum[:, -1].copy()


def check_case(name, plan, entry, device, shape=SHAPE, scales=None):
    """Checks 1-3 of one (config, plan, entry point, shape): decisions bit-exact and really changed, raw predictions untouched, mel
    against the teacher-forced oracle.  -> the controlled run."""
    B, T, lens = shape
    scales = {k: v[:B] for k, v in (scales or SCALES).items()}
    net, cfg, sd = net_of(name, device)
    x, ids, mask = inputs(B, T, lens, device)
    base = plain(name, plan, entry, device, shape)
    got = run(net, dict(x, **controls(B, device, scales)), entry, plan)
    # 1. decisions
    vp, ve, pi, ei, d, cum, mel_len = expected_decisions(got, sd, mask, scales)
    live = np.ones((B, T), bool) if mask is None else ~mask
    changed = {k: float((got[k] != base[k])[live].mean()) for k in ("dur", "pitch_idx", "energy_idx")}
    print(f"{name} plan {plan} {entry} {shape}: changed {changed}, mel_len {base['mel_len'].tolist()} -> {got['mel_len'].tolist()}")
    for k, e in (("pitch_idx", pi), ("energy_idx", ei), ("dur", d), ("cum", cum), ("mel_len", mel_len)):
        assert np.array_equal(got[k], e), (k, np.argwhere(got[k] != e)[:4].tolist())
    assert min(changed.values()) >= 0.5, changed             # (not a measurement: the test must not pass on ignored controls)
    # 2. the raw predictions are untouched, and the oracle's
    o_free = free_running(name, shape)
    for k in ("pitch", "energy", "duration"):
        assert np.array_equal(got[k], base[k]), k
        np.testing.assert_allclose(got[k], getattr(o_free, k)[..., 0], atol=H.PRED_TOL, rtol=0)
    # 3. mel against the oracle teacher-forced on the same fp32 products and the expected durations
    o = oracle.phoneme2mel(cfg, oracle.Weights(sd), ids, mask, pitch=vp, energy=ve, duration=d)
    assert np.array_equal(o.pitch_idx, pi) and np.array_equal(o.energy_idx, ei) and np.array_equal(o.dur, d)
    assert np.array_equal(got["mel_len"], o.mel_len)
    assert got["mel"].shape == o.mel.shape, (got["mel"].shape, o.mel.shape)
    err = float(np.abs(got["mel"] - o.mel).max())
    print(f"    mel L-inf vs teacher-forced oracle {err:.2e}")
    assert err < H.MEL_TOL, err
    for b in range(B):
        assert not got["mel"][b, int(got["mel_len"][b]):].any(), b
    if entry == "forward":      # the serving call (no taps: the one-launch kernel skips the stores nobody reads) gives the same result
        with torch.no_grad(), _lib.launch_plan(plan):
            mel, ml, dp = net(dict(x, **controls(B, device, scales)))
        assert np.array_equal(mel.cpu().numpy(), got["mel"]) and np.array_equal(ml.cpu().numpy(), got["mel_len"])
        assert np.array_equal(dp.cpu().numpy()[..., 0], got["duration"])
    return got


def same(a, b, keys=TAPS + ("mel",)):
    for k in keys:
        assert np.array_equal(a[k], b[k]), k


def check_identity(name, plan, entry, device, shape=SHAPE):
    """4. no keys, the float 1.0 and a ones tensor: bit-identical outputs"""
    B = shape[0]
    net, _, _ = net_of(name, device)
    x = inputs(*shape, device)[0]
    base = plain(name, plan, entry, device, shape)
    same(run(net, dict(x, pitch_control=1.0, energy_control=1.0, duration_control=1.0), entry, plan), base)
    ones = torch.ones((B,), dtype=torch.float32, device=device)
    same(run(net, dict(x, pitch_control=ones, energy_control=ones.clone(), duration_control=torch.ones((), device=device)), entry, plan), base)


def check_per_utterance(name, plan, entry, device, mixed, shape=SHAPE):
    """5. a batch in which every utterance carries utterance b's scales gives row b of the mixed batch: no utterance sees another's"""
    B = shape[0]
    net, _, _ = net_of(name, device)
    x = inputs(*shape, device)[0]
    for b in range(B):
        got = run(net, dict(x, **controls(B, device, rows=[b] * B)), entry, plan)
        for k in TAPS:
            assert np.array_equal(got[k][b], mixed[k][b]), (k, b)
        L = int(mixed["mel_len"][b])
        assert int(got["mel_len"][b]) == L and np.array_equal(got["mel"][b, :L], mixed["mel"][b, :L]), b
        # one Python number per key = the same scale for every utterance
        num = run(net, dict(x, **{k + "_control": SCALES[k][b] for k in SCALES}), entry, plan)
        same(num, got)


def check_single_utterance(name, plan, entry, device):
    """6. B == 1 takes no mask (the reference's path, networks.py:338, :383-384)"""
    check_case(name, plan, entry, device, shape=(1, 17, (17,)))


def check_value_errors(device):
    """7a. what the Python layer refuses, on both paths, before anything is launched"""
    net, _, _ = net_of("tiny", device)
    B, T, _ = SHAPE
    x = inputs(*SHAPE, device)[0]
    forced = torch.full((B, T), 2, dtype=torch.int32, device=device)
    calls = (lambda xx: net(xx), lambda xx: net.encoder._encode(xx))
    bad = [dict(duration_control=1.2, duration_forced=forced),
           dict(pitch_control=torch.ones((B + 1,), device=device)),
           dict(energy_control=torch.ones((B, 1), device=device)),
           dict(duration_control=torch.ones((1, B), device=device)),
           dict(pitch_control=float("nan")), dict(energy_control=float("inf")), dict(duration_control=-0.5),
           dict(pitch_control="high")]
    with torch.no_grad():
        for extra in bad:
            for call in calls:
                with pytest.raises(ValueError):
                    call(dict(x, **extra))
        for k in networks.CONTROL_KEYS:                          # any control key while training
            with pytest.raises(ValueError, match="train"):
                net(dict(x, **{k: 1.1}), train=True)
            with pytest.raises(ValueError, match="train"):
                net.encoder._encode(dict(x, **{k: 1.1}), train=True)
        for call in calls:                                       # pitch / energy control next to forced durations is allowed
            call(dict(x, pitch_control=1.2, energy_control=0.8, duration_forced=forced))


def check_abi_errors(device, launches=None):
    """7b. a scale together with the matching teacher / forced pointer: ESMI_ERR_ARG from each of the three entry points, reached through
    _lib with arguments that are complete otherwise.  `launches` (simulator): a context manager collecting launch names -- none."""
    import contextlib
    net, cfg, _ = net_of("tiny", device)
    B, T, _ = SHAPE
    x = inputs(*SHAPE, device)[0]
    dim = cfg.dim
    with torch.no_grad(), networks._on_device_of(net.decoder.mel_linear.weight):
        net(x)                                                   # (weights packed, attributes set: not part of what is counted below)
        lib, stream = networks._runtime(net.decoder.mel_linear.weight)
        f32 = lambda *s: torch.zeros(s, dtype=torch.float32, device=device)     # noqa: E731
        i32 = lambda *s: torch.zeros(s, dtype=torch.int32, device=device)       # noqa: E731
        ones = torch.ones((B,), dtype=torch.float32, device=device)
        p = lambda t: t.data_ptr()                                              # noqa: E731
        (pw, _), (ew, _), (dw, _) = net.encoder._predictors(lib, stream)
        feat, preds, idx, dur = f32(B, T, 4 * dim), f32(3, B, T), i32(2, B, T), i32(B, T)
        ws = torch.empty(lib.esmi_fuse_variance_adaptor_workspace_bytes(B, T, dim, cfg.depth), dtype=torch.uint8, device=device)
        tgt_f, tgt_i = f32(B, T), i32(B, T)
        fw, _ = net.encoder.fuse._packed(lib, stream)
        feats, bm = net.encoder.encoder._run(x["phoneme"], x["phoneme_mask"])
        fp = (C.c_void_p * cfg.depth)(*[p(f) for f in feats])
        ni = (C.c_int * cfg.depth)(*[f.shape[1] for f in feats])
        with (launches() if launches else contextlib.nullcontext([])) as seen:
            for which in range(3):
                ctl = _lib.ProsodyControl()
                setattr(ctl, ("pitch_scale", "energy_scale", "duration_scale")[which], p(ones))
                tg = [p(tgt_f) if which == 0 else None, p(tgt_f) if which == 1 else None, p(tgt_i) if which == 2 else None]
                with pytest.raises(RuntimeError, match="ESMI_ERR_ARG"):
                    lib.esmi_variance_adaptor_ctl_f32(C.byref(pw), C.byref(ew), C.byref(dw), dim, B, T, p(bm[0]), *tg, p(feat), p(preds[0]),
                                                      p(preds[1]), p(preds[2]), p(idx[0]), p(idx[1]), p(dur), p(ws), ws.numel(), stream,
                                                      C.byref(ctl))
                with pytest.raises(RuntimeError, match="ESMI_ERR_ARG"):
                    lib.esmi_fuse_variance_adaptor_ctl_f32(C.byref(fw), cfg.depth, dim, net.encoder.fuse.kernel_size, B, T, fp, ni, C.byref(pw),
                                                           C.byref(ew), C.byref(dw), p(bm[0]), *tg, p(feat), p(preds[0]), p(preds[1]),
                                                           p(preds[2]), p(idx[0]), p(idx[1]), p(dur), None, None, None, None,
                                                           _lib.current_plan(), p(ws), ws.numel(), stream, C.byref(ctl))
            # the one-call forward: duration_scale next to dur_forced.  The Python layer refuses that combination itself, so hand the
            # library the scale behind its back
            real = networks._prosody_controls
            ctl = _lib.ProsodyCurves()
            ctl.duration_scale = p(ones)
            networks._prosody_controls = lambda *a, **k: (ctl, (ones,))
            try:
                with pytest.raises(RuntimeError, match="esmi_phoneme2mel_forward_curve_f32 failed: ESMI_ERR_ARG"):
                    net._launch(dict(x, duration_forced=tgt_i + 2))
            finally:
                networks._prosody_controls = real
        assert not [k for k in seen if not k.startswith(("hip", "memset"))], seen
        # ... and the same arguments without the conflict are a valid call (the refusal above was the conflict's)
        ctl = _lib.ProsodyControl()
        ctl.pitch_scale = p(ones)
        lib.esmi_fuse_variance_adaptor_ctl_f32(C.byref(fw), cfg.depth, dim, net.encoder.fuse.kernel_size, B, T, fp, ni, C.byref(pw), C.byref(ew),
                                               C.byref(dw), p(bm[0]), None, p(tgt_f), p(tgt_i), p(feat), p(preds[0]), p(preds[1]), p(preds[2]),
                                               p(idx[0]), p(idx[1]), p(dur), None, None, None, None, _lib.current_plan(), p(ws), ws.numel(),
                                               stream, C.byref(ctl))


def check_scheduler(device):
    """8. BucketedSynthesizer(..., controls=...) equals direct net(x) calls on the same plan() batches with the scales gathered by hand"""
    from efficientspeech_amd.scheduler import BucketedSynthesizer
    net, _, _ = net_of("tiny", device)
    rng = np.random.default_rng(5)
    lengths = [9, 4, 9, 7, 3, 8, 13]                     # (max_batch 2, granularity 4: three pairs and a single request, the B == 1 path)
    seqs = [rng.integers(1, 40, size=n).astype(np.int32) for n in lengths]
    ctl = {"pitch_control": np.array([1.5, 0.5, 1.25, 0.75, 2.0, 1.0, 0.5], np.float32),
           "duration_control": np.array([1.5, 0.75, 1.25, 2.0, 0.5, 1.0, 1.5], np.float32)}
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
        for k, v in ctl.items():
            x[k] = torch.from_numpy(v[idx]).to(device)
        with torch.no_grad():
            mel, mel_len, dur = net(x)
        for r, i in enumerate(idx):
            L = int(mel_len[r])
            assert torch.equal(got[i][0], mel[r, :L]) and torch.equal(got[i][1], dur[r, :lengths[i], 0]), i
            differs += got[i][0].shape != plain_out[i][0].shape
    assert differs >= 3                                           # (the controls reached the requests: most lengths moved)
    with pytest.raises(ValueError):
        synth(seqs, controls={"pitch_control": np.ones(len(seqs) - 1, np.float32)})
    with pytest.raises(ValueError):
        synth(seqs, controls={"speed": np.ones(len(seqs), np.float32)})
