"""The dx2 = 128 mel decoder's K loops on 16 x 16 x 32 MFMA tiles (ESMI_DEC_MFMA16, mel_decoder_body.h `M16`): the wave's 64 x 32
output tile as 4 row tiles x 2 column tiles, the weight fragments picked out of the 32x32x16 packing, the accumulators' row / column
map in the tanh / store / mel epilogues, and the mel Linear's skipped 16-column tiles.  The shapes are the smallest at which that
layout can go wrong; every result is held to `oracle.mel_decoder` / `oracle.phoneme2mel` at the bound the existing decoder tests use
for the same mode: 1e-4 on the mel at the default precision (tests/helpers.py MEL_TOL; the trained-looking profile through
tests/test_weight_profiles.py's `within_budget`), the E_q band of tests/precision_checks.py at precision 16 and bf16.

Gather mode: B = 3, T = 24, forced durations with mel_len = (113, 130, 7) -- for k = 5 a window boundary at frame 112, a second window
with 18 live rows, an utterance shorter than one 16-row tile, rows beyond mel_len that must be exactly zero.  Direct mode (the in-kernel
`proj` stage: `mma_sub`): B = 2, L = 40 and L = 129.  n_mel = 80 is five 16-column tiles (the sixth is not computed); 78 and 33 (the
widths tests/test_gpu_parity.py builds) end inside a tile and take the scalar store path.

The tests run the forms the library was built with, like every other decoder test: by default the three-product mode on the 16-row
tiles and the one-product modes on the 32-row tiles (ESMI_DEC_MFMA16 = 1, a mask of modes; profiles/r25_decoder_mfma16.md has the
same cases with all three modes on the 16-row tiles).  A `test_simulated_*` test runs the same kernel sources on the wave simulator
(no GPU)."""
import dataclasses

import numpy as np
import pytest
import torch

from efficientspeech_amd import CONFIGS, build_phoneme2mel, load_numpy_state_dict
from efficientspeech_amd.synth import synth_phonemes, synth_state_dict
from oracle import oracle
from tests import helpers as H
from tests import precision_checks as V
from tests import weight_profiles as WP
from tests.precision_checks import BF16, R16, device, on_the_device, yard   # noqa: F401 (fixtures)
from tests.test_weight_profiles import within_budget

T, LENS, MEL_LEN = 24, (24, 24, 5), (113, 130, 7)
PROFILE = "ln_affine+common_offset"       # the trained-looking profile of tests/test_weight_profiles.py's end-to-end check


def forced_durations():
    """(3, 24) int32, zero behind each utterance's last phoneme; the rows sum to MEL_LEN"""
    dur = np.zeros((3, T), np.int32)
    dur[0] = [5] * 17 + [4] * 7
    dur[1] = [6] * 10 + [5] * 14
    dur[2, :5] = [1, 2, 1, 2, 1]
    assert tuple(dur.sum(1)) == MEL_LEN
    return dur


def config_of(name, n_mel=80):
    cfg = V.config_of(name)
    return cfg if n_mel == 80 else dataclasses.replace(cfg, n_mel_channels=n_mel)


_NETS = {}


def make_net(name, device, profile=None, n_mel=80):
    """(net, cfg, sd): synth_state_dict weights, optionally through a weight profile; shared between the tests of a tier"""
    key = (name, str(device), profile, n_mel)
    if key not in _NETS:
        cfg = config_of(name, n_mel)
        sd = synth_state_dict(cfg, 1234)
        if profile:
            sd = WP.ACOUSTIC[profile](cfg, sd)
        net = build_phoneme2mel(cfg)
        load_numpy_state_dict(net, sd)
        _NETS[key] = (net.to(device).eval(), cfg, sd)
    return _NETS[key]


def gather_inputs(device):
    ids, mask = synth_phonemes(3, T, 12, list(LENS))
    dur = forced_durations()
    assert not dur[mask].any()
    x = {"phoneme": torch.from_numpy(ids).to(device), "phoneme_mask": torch.from_numpy(mask).to(device),
         "duration_forced": torch.from_numpy(dur).to(device)}
    return ids, mask, dur, x


# ---------------------------------------------------------------------------------------------------------------- gather mode
def check_gather(device, name, profile=None):
    """the whole forward (the decoder gathers the phoneme-rate h0) against oracle.phoneme2mel teacher-forced with the kernels' own
    pitch / energy and the forced durations: no bucket decision can flip"""
    net, cfg, sd = make_net(name, device, profile)
    ids, mask, dur, x = gather_inputs(device)
    with torch.no_grad():
        enc = net.encoder._encode(x)
        mel, mel_len, _ = net(x)
    kw = dict(pitch=enc["pitch"][..., 0].cpu().numpy(), energy=enc["energy"][..., 0].cpu().numpy(), duration=dur)
    w = oracle.Weights(sd)
    o = oracle.phoneme2mel(cfg, w, ids, mask, **kw)
    mel = mel.cpu().numpy()
    assert tuple(mel_len.cpu().tolist()) == MEL_LEN and np.array_equal(o.mel_len, MEL_LEN)
    assert mel.shape == o.mel.shape == (3, 130, 80)
    for b, n in enumerate(MEL_LEN):
        assert not mel[b, n:].any(), b                     # rows beyond mel_len: exactly zero
        assert np.abs(mel[b, :n]).sum() > 0
    err = float(np.abs(mel - o.mel).max())
    print(f"{name}{'+' + profile if profile else ''} gather (3, 130): mel L-inf {err:.2e}, |ref|max {np.abs(o.mel).max():.2f}")
    if profile:
        within_budget(mel, o.mel, oracle.phoneme2mel(cfg, w, ids, mask, f32=True, **kw).mel, H.MEL_TOL, f"{name}+{profile} gather mel")
    else:
        assert np.isfinite(mel).all() and err < H.MEL_TOL, err


def test_simulated_gather_k5(device):
    check_gather(device, "tiny")


@pytest.mark.parametrize("name", ["tiny", "tiny_k3"])
@pytest.mark.gpu
def test_gather(name, device):
    """k = 5: windows [0, 112) and [112, 130); k = 3: [0, 120) and [120, 130)"""
    check_gather(device, name)


@pytest.mark.gpu
def test_gather_trained_looking_weights(device):
    check_gather(device, "tiny", PROFILE)


def check_precision_modes(yard, device):
    """precision 32, 16 and bf16 on the gather shape: mel_len, duration and cum identical across the three, rows beyond mel_len
    exactly zero, the reduced mels inside their E_q band (the yardstick's input is this tier's own encoder output)"""
    net, cfg, sd = make_net("tiny", device)
    _ids, _mask, dur, x = gather_inputs(device)
    with torch.no_grad():
        enc = net.encoder._encode(x)
        s32 = net._launch(x, taps=True)
        runs = {r: net._launch(dict(x, decoder_precision=r.value), taps=True) for r in (R16, BF16)}
    ml = s32.mel_len.cpu()
    assert tuple(ml.tolist()) == MEL_LEN
    feats = V.frame_features(enc["feat"], s32.taps["dur"], 130)
    for rule, s in runs.items():
        assert torch.equal(s.mel_len, s32.mel_len) and torch.equal(s.duration, s32.duration)
        assert torch.equal(s.taps["cum"], s32.taps["cum"]) and torch.equal(s.taps["dur"], s32.taps["dur"])
        assert not torch.equal(s.mel, s32.mel)
        for b, n in enumerate(MEL_LEN):
            assert not bool(s.mel[b, n:].any())
        exact, eq, _ = yard.decoder(rule, ("m16 gather", str(device)), cfg, sd, feats, proj_rounded=False, mel_len=ml)
        assert float((s32.mel.cpu().double() - exact).abs().max()) < H.MEL_TOL
        V.judge(f"{rule} tiny gather (3, 130)", s.mel, exact, eq)


def test_simulated_precision_modes(yard, device):
    check_precision_modes(yard, device)


test_precision_modes = on_the_device(test_simulated_precision_modes)


# ---------------------------------------------------------------------------------------------------------------- direct mode
@pytest.mark.parametrize("L", [40, 129])
@pytest.mark.parametrize("name", ["tiny", "tiny_k3"])
@pytest.mark.gpu
def test_direct(name, L, device):
    """MelDecoder.forward on frame-rate features: the `proj` stage shares the accumulators"""
    net, cfg, sd = make_net(name, device)
    feats = np.random.default_rng(7).standard_normal((2, L, cfg.d4)).astype(np.float32)
    with torch.no_grad():
        mel = net.decoder(torch.from_numpy(feats).to(device)).cpu().numpy()
    ref = oracle.mel_decoder(cfg, oracle.Weights(sd), feats)
    err = float(np.abs(mel - ref).max())
    print(f"{name} direct (2, {L}): mel L-inf {err:.2e}")
    assert mel.shape == ref.shape and np.isfinite(mel).all() and err < H.MEL_TOL, err


@pytest.mark.parametrize("L", [40, 129])
@pytest.mark.parametrize("rule", [R16, BF16], ids=str)
@pytest.mark.gpu
def test_direct_reduced_precision(rule, L, yard, device):
    V.check_direct(yard, rule, "tiny", 2, L, device)


@pytest.mark.parametrize("n_mel", [78, 33])
@pytest.mark.gpu
def test_direct_mel_widths_inside_a_tile(n_mel, device):
    """78: the fifth 16-column tile ends inside a float4 group; 33: the second column slice keeps one of its two tiles, one column wide"""
    net, cfg, sd = make_net("tiny", device, n_mel=n_mel)
    feats = np.random.default_rng(2).standard_normal((2, 40, cfg.d4)).astype(np.float32)
    with torch.no_grad():
        mel = net.decoder(torch.from_numpy(feats).to(device)).cpu().numpy()
    ref = oracle.mel_decoder(cfg, oracle.Weights(sd), feats)
    assert mel.shape == ref.shape == (2, 40, n_mel)
    err = float(np.abs(mel - ref).max())
    print(f"tiny n_mel = {n_mel} direct (2, 40): mel L-inf {err:.2e}")
    assert np.isfinite(mel).all() and err < H.MEL_TOL, err
