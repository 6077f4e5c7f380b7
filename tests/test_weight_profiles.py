"""The kernels on trained-looking weights (tests/weight_profiles.py) against the double-accumulator oracle.

Bound, the same everywhere: with e32 = max|oracle_f32 - oracle_f64| of the compared tensor,

    max|kernel - oracle_f64| <= max(T max(1, |ref|max), 4 e32),    T = MEL_TOL (mel) / PRED_TOL (predictions, taps) / 5e-5 (audio)

(4 = the two significand bits by which the split-f16 products are coarser than fp32) and, first, the CONDITIONING rule
4 e32 <= T max(1, |ref|max): a profile the reference's own fp32 arithmetic cannot hold is a mistake of the test, not a looser bound.

Measured worst kernel / e32 ratio per group (sim = CPU wave simulator at the twins' shapes, gpu = MI355X at every GPU shape and
plan; the tests print every figure):

    group                      profile            sim    gpu
    decoder tiny               saturated rows     2.96   0.87
    decoder small              saturated rows     2.67   1.40
    decoder base               saturated rows     1.85   0.96
    decoder tiny/small/base    common_offset      1.64   0.65
    decoder tiny/small/base    ln_affine          2.00   0.90
    encoder tiny               common_offset      1.75   1.15
    encoder tiny               ln_affine          2.00   2.29
    encoder tiny               peaky_attention    2.07   2.90
    encoder tiny               row_outliers       2.75   2.17
    encoder small              common_offset      2.00   1.62
    encoder small              ln_affine          2.47   1.95
    encoder small              peaky_attention    2.13   2.26
    encoder small              row_outliers       1.72   1.47
    encoder base               common_offset      1.94   0.97
    encoder base               ln_affine          2.73   2.27
    encoder base               peaky_attention    2.72   1.41
    encoder base               row_outliers       2.23   1.28
    end to end tiny/small/base ln_affine + offset 2.00   1.33
    vocoder v2                 common_offset      2.65   2.32
    vocoder v2                 row_outliers       6.73   2.92
    vocoder v3                 common_offset      5.28   3.48
    vocoder v3                 row_outliers       5.73   2.56

Nothing needs the 4 e32 term on the GPU.  The simulated vocoder is 5 .. 7 e32 off, with absolute errors <= 2.8e-5 inside the 5e-5 audio
tolerance, so it passes on the T term: e32 is very small there (1e-6 .. 4e-6: no normalisation amplifies the oracle's rounding), and the
simulator's MFMA model rounds after every product where the device's matrix pipe does not -- the same kernels are 2.3 .. 3.5 e32 off on
the device.  (That reading of the gap is not verified further.)

What these tests found.  Until round 7 the dx2 = 256 decoder (small, base) took its LayerNorm variance in one pass, E[x^2] - mean^2.
Mel L-inf against the f64 oracle with that kernel / with the variance about the slices' own means, (B, L) = (1, 40); budget 1e-4
max(1, |ref|max) = 3.3e-4 .. 4.2e-4:

    model  profile          e32      before: sim / gpu      after: sim / gpu
    small  sat+2x0.3        1.8e-5   3.3e-4 / 3.0e-4        1.5e-5 / 8.7e-6
    small  sat+3x0.3        6.1e-5   1.2e-2 / 1.1e-2        6.9e-5 / 4.4e-5
    small  sat+3x0.3_last   1.5e-5   5.5e-3 / 5.6e-3        2.5e-5 / 8.1e-6
    small  sat+4x1          7.8e-5   1.5e-2 / 1.4e-2        1.5e-4 / 1.1e-4
    small  sat+4x1_last     8.8e-6         - / 1.5e-3       2.4e-5 / 4.2e-6
    base   sat+2x0.3        2.6e-5   4.1e-4 / 4.6e-4        1.7e-5 / 1.5e-5
    base   sat+3x0.3        8.7e-5   1.2e-2 / 1.1e-2        1.1e-4 / 8.4e-5
    base   sat+3x0.3_last   1.6e-5   4.7e-3 / 6.2e-3        2.7e-5 / 7.8e-6
    base   sat+4x1_last     9.0e-6         - / 4.6e-3       1.7e-5 / 6.7e-6

(dx2 = 128, tiny, always had the two-pass form: 1.1e-5 .. 6.7e-5 on the same profiles, before and after.)
"""
import functools

import numpy as np
import pytest
import torch

from efficientspeech_amd import CONFIGS, _lib, build_phoneme2mel, load_numpy_state_dict
from efficientspeech_amd.hifigan import HIFIGAN_CONFIGS, Generator, synth_hifigan_state_dict
from efficientspeech_amd.synth import synth_phonemes, synth_state_dict
from oracle import oracle
from tests import helpers as H
from tests import weight_profiles as WP
from tests.simlib import launched_kernels, use_sim

DEV = "cuda:0"
AUDIO_TOL = 5e-5          # as check_hifigan_golden
MODELS = ["tiny", "small", "base"]
SEED = 77                 # the synthetic checkpoint every profile starts from


def within_budget(got, ref64, ref32, tol, what):
    """the module's bound on one tensor; prints the figures first"""
    got, ref64, ref32 = (np.asarray(a, np.float64) for a in (got, ref64, ref32))
    assert got.shape == ref64.shape == ref32.shape, (what, got.shape, ref64.shape)
    budget = tol * max(1.0, float(np.abs(ref64).max()))
    e32 = float(np.abs(ref32 - ref64).max())
    err = float(np.abs(got - ref64).max())
    print(f"{what}: kernel {err:.2e}  e32 {e32:.2e}  ratio {err / max(e32, 1e-30):.2f}  budget {budget:.2e}  |ref|max {np.abs(ref64).max():.2f}")
    assert 4.0 * e32 <= budget, f"{what}: ill-conditioned profile, the fp32 oracle itself is {e32:.2e} off (budget {budget:.2e}): retune it"
    assert np.isfinite(got).all() and err <= max(budget, 4.0 * e32), f"{what}: {err:.2e} > {max(budget, 4.0 * e32):.2e} (e32 {e32:.2e})"
    return err


def make_net(name, profile, device):
    cfg = CONFIGS[name]
    sd = WP.ACOUSTIC[profile](cfg, synth_state_dict(cfg, SEED))
    net = build_phoneme2mel(cfg)
    load_numpy_state_dict(net, sd)
    return net.to(device), cfg, sd


def _sim(device):
    """(the simulated twins run the same check on host tensors)"""
    import contextlib
    return use_sim() if device == "cpu" else contextlib.nullcontext()


# ---------------------------------------------------------------------- decoder, direct mode
DEC_PROFILES = ["sat+2x0.3", "sat+3x0.3", "sat+3x0.3_last", "sat+4x1", "sat+4x1_last", "common_offset", "ln_affine"]
# (+4, x1) on EVERY layer is more than the reference's own fp32 arithmetic holds on the wide decoders: every LayerNorm divides the
# rounding of tanh rows with std ~ 1e-3 by that std, and the layers stack.  Oracle alone, 4 e32 / budget: base 6.3 at (1, 40) and 6.2 at
# (2, 300) (e32 5.9e-4 / 6.9e-4), small 1.43 at (2, 300) (e32 1.55e-4; 0.87 at (1, 40), kept).  Those three combinations are retuned to
# the same offset on the LAST layer only (`sat+4x1_last`: 0.08 .. 0.11 everywhere), which every model and shape runs.
ILL_CONDITIONED = {("base", "sat+4x1", (1, 40)), ("base", "sat+4x1", (2, 300)), ("small", "sat+4x1", (2, 300))}


def decoder_cases(shapes):
    return [pytest.param(n, p, B, L, id=f"{n}-{p}-b{B}_l{L}") for n in MODELS for p in DEC_PROFILES for B, L in shapes
            if (n, p, (B, L)) not in ILL_CONDITIONED]


@functools.lru_cache(maxsize=None)
def decoder_reference(name, profile, B, L):
    """(features, f64 mel, f32 mel): computed once, shared by the GPU test and its simulated twin"""
    cfg = CONFIGS[name]
    sd = WP.ACOUSTIC[profile](cfg, synth_state_dict(cfg, SEED))
    w = oracle.Weights(sd)
    feats = np.random.default_rng(9).standard_normal((B, L, cfg.d4)).astype(np.float32)
    return feats, oracle.mel_decoder(cfg, w, feats), oracle.mel_decoder(cfg, w, feats, f32=True)


def check_decoder(device, name, profile, B, L):
    feats, ref64, ref32 = decoder_reference(name, profile, B, L)
    with _sim(device), torch.no_grad():
        net, cfg, sd = make_net(name, profile, device)
        mel = net.decoder(torch.from_numpy(feats).to(device)).cpu().numpy()
    return within_budget(mel, ref64, ref32, H.MEL_TOL, f"decoder {name} {profile} ({B},{L}) mel")


@pytest.mark.parametrize("name,profile,B,L", decoder_cases([(1, 40)]))
def test_simulated_decoder_profiles(name, profile, B, L):
    check_decoder("cpu", name, profile, B, L)


@pytest.mark.gpu
@pytest.mark.parametrize("name,profile,B,L", decoder_cases([(1, 40), (2, 300)]))
def test_decoder_profiles(name, profile, B, L):
    """(2, 300): several chunks of the dx2 = 256 walk with block skew, both `stat` exchange buffers in use; several windows for tiny"""
    check_decoder(DEV, name, profile, B, L)


# ---------------------------------------------------------------------- encoder side
ENC_PROFILES = ["common_offset", "ln_affine", "peaky_attention", "row_outliers"]
ENC_SHAPES = {"tiny": (3, 40, [40, 29, 7]), "small": (2, 150, [150, 97]), "base": (2, 150, [150, 97])}
ENC_KERNELS = {"tiny": {"enc_b0_16_kernel<4>", "enc_b1_16_kernel", "enc_va16_kernel<3>"},
               "small": {"enc_va64_kernel<2>", "enc_post_attn64_kernel<2>"}, "base": {"enc_pred128_kernel"}}


def _enc_inputs(name):
    B, T, lens = ENC_SHAPES[name]
    ids, mask = synth_phonemes(B, T, 4321, lens)
    dur = np.random.default_rng(5).integers(1, 5, size=(B, T)).astype(np.int32)
    return ids, mask, dur


def compare_encoder(cfg, sd, ids, mask, dur, enc, what):
    """`_encode`'s taps and predictions against the oracle teacher-forced with the kernel's own pitch / energy and the forced
    durations: no bucket or rounding decision can flip"""
    kw = dict(pitch=enc["pitch"][..., 0].cpu().numpy(), energy=enc["energy"][..., 0].cpu().numpy(), duration=dur, taps=True)
    w = oracle.Weights(sd)
    o64 = oracle.phoneme_encoder(cfg, w, ids, mask, **kw)
    o32 = oracle.phoneme_encoder(cfg, w, ids, mask, f32=True, **kw)
    assert np.array_equal(enc["pitch_idx"].cpu().numpy(), o64.pitch_idx) and np.array_equal(enc["energy_idx"].cpu().numpy(), o64.energy_idx)
    assert np.array_equal(enc["dur"].cpu().numpy(), o64.dur) and np.array_equal(enc["mel_len"].cpu().numpy(), o64.mel_len)
    for i, f in enumerate(enc["feats"]):
        within_budget(f.cpu().numpy(), o64.f_taps[i], o32.f_taps[i], H.PRED_TOL, f"{what} f{i}")
    within_budget(enc["feat"].cpu().numpy(), o64.feat, o32.feat, H.PRED_TOL, f"{what} feat")
    for key in ("pitch", "energy", "duration"):
        within_budget(enc[key].cpu().numpy(), getattr(o64, key), getattr(o32, key), H.PRED_TOL, f"{what} {key}")
    return o64, o32


def check_encoder(device, name, profile, plans=(_lib.FUSE_ALL,)):
    ids, mask, dur = _enc_inputs(name)
    launched = {}
    with _sim(device), torch.no_grad():
        net, cfg, sd = make_net(name, profile, device)
        x = {"phoneme": torch.from_numpy(ids).to(device), "phoneme_mask": torch.from_numpy(mask).to(device),
             "duration_forced": torch.from_numpy(dur).to(device)}
        for plan in plans:
            with _lib.launch_plan(plan):
                if device == "cpu":
                    with launched_kernels() as names:
                        enc = net.encoder._encode(x)
                    launched[plan] = set(names)
                else:
                    enc = net.encoder._encode(x)
                o64, o32 = compare_encoder(cfg, sd, ids, mask, dur, enc, f"encoder {name} {profile} plan {plan}")
        if name == "tiny":      # the one-call forward runs tiny's encoder side as ONE launch: its duration prediction, same bound
            if device == "cpu":
                with launched_kernels() as names:
                    _, _, dpred = net(x)
                launched["one_call"] = set(names)
            else:
                _, _, dpred = net(x)
            within_budget(dpred.cpu().numpy(), o64.duration, o32.duration, H.PRED_TOL, f"encoder {name} {profile} one-launch duration")
    return launched


@pytest.mark.parametrize("profile", ENC_PROFILES)
@pytest.mark.parametrize("name", MODELS)
def test_simulated_encoder_profiles(name, profile):
    launched = check_encoder("cpu", name, profile)
    assert ENC_KERNELS[name] <= launched[_lib.FUSE_ALL], sorted(launched[_lib.FUSE_ALL])
    if name == "tiny":
        assert any(k.startswith("enc_all16_kernel") for k in launched["one_call"]), sorted(launched["one_call"])


@pytest.mark.gpu
@pytest.mark.parametrize("profile", ENC_PROFILES)
@pytest.mark.parametrize("name", MODELS)
def test_encoder_profiles(name, profile):
    """default plan and plan 0: the per-op kernels (convgemm.h, attention.h) see the profiles too"""
    check_encoder(DEV, name, profile, plans=(_lib.FUSE_ALL, 0))


# ---------------------------------------------------------------------- end to end
E2E_T = {"tiny": 40, "small": 60, "base": 60}


def check_end_to_end(device, name, profile="ln_affine+common_offset"):
    T = E2E_T[name]
    ids, mask = synth_phonemes(2, T, 12, [T, T - 13])
    dur = np.random.default_rng(3).integers(1, 6, size=(2, T)).astype(np.int32)       # U[1, 5]
    with _sim(device), torch.no_grad():
        net, cfg, sd = make_net(name, profile, device)
        x = {"phoneme": torch.from_numpy(ids).to(device), "phoneme_mask": torch.from_numpy(mask).to(device),
             "duration_forced": torch.from_numpy(dur).to(device)}
        enc = net.encoder._encode(x)
        mel, mel_len, dpred = net(x)
    kw = dict(pitch=enc["pitch"][..., 0].cpu().numpy(), energy=enc["energy"][..., 0].cpu().numpy(), duration=dur)
    w = oracle.Weights(sd)
    o64 = oracle.phoneme2mel(cfg, w, ids, mask, **kw)
    o32 = oracle.phoneme2mel(cfg, w, ids, mask, f32=True, **kw)
    assert np.array_equal(mel_len.cpu().numpy(), o64.mel_len)
    within_budget(dpred.cpu().numpy(), o64.duration, o32.duration, H.PRED_TOL, f"end to end {name} duration")
    within_budget(mel.cpu().numpy(), o64.mel, o32.mel, H.MEL_TOL, f"end to end {name} mel")


@pytest.mark.parametrize("name", MODELS)
def test_simulated_end_to_end_profiles(name):
    check_end_to_end("cpu", name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", MODELS)
def test_end_to_end_profiles(name):
    check_end_to_end(DEV, name)


# ---------------------------------------------------------------------- vocoder
VOC_SHAPES = {"v2": (2, 40), "v3": (1, 40)}


@functools.lru_cache(maxsize=None)
def vocoder_reference(config, profile):
    h = HIFIGAN_CONFIGS[config]
    sd = WP.VOCODER[profile](h, synth_hifigan_state_dict(h, SEED))
    B, L = VOC_SHAPES[config]
    mel = WP.log_mel(B, L, h.num_mels)
    w = oracle.Weights(sd)
    return sd, mel, oracle.hifigan(h, w, mel), oracle.hifigan(h, w, mel, f32=True)


def check_vocoder(device, config, profile):
    h = HIFIGAN_CONFIGS[config]
    sd, mel, ref64, ref32 = vocoder_reference(config, profile)
    with _sim(device), torch.no_grad():
        voc = Generator(h)
        voc.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
        voc = voc.to(device).eval()
        m = torch.from_numpy(mel).to(device).transpose(1, 2)
        for fused in (True, False):                                    # one launch per ResBlock / one per convolution
            voc.fuse_resblocks = fused
            voc._cache.invalidate()
            wav = voc(m)
            assert wav.shape == (mel.shape[0], 1, mel.shape[1] * h.hop)
            within_budget(wav[:, 0].cpu().numpy(), ref64, ref32, AUDIO_TOL, f"vocoder {config} {profile} {'fused' if fused else 'conv-by-conv'}")


@pytest.mark.parametrize("profile", sorted(WP.VOCODER))
@pytest.mark.parametrize("config", sorted(VOC_SHAPES))
def test_simulated_vocoder_profiles(config, profile):
    check_vocoder("cpu", config, profile)


@pytest.mark.gpu
@pytest.mark.parametrize("profile", sorted(WP.VOCODER))
@pytest.mark.parametrize("config", sorted(VOC_SHAPES))
def test_vocoder_profiles(config, profile):
    check_vocoder(DEV, config, profile)
