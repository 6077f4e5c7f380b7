"""Parity tests proper: the HIP path on a real MI355X, through the C-ABI, against
(1) the committed golden vectors (outputs of the reference itself) and (2) the CPU oracle.

Tolerances: mel L-inf < 1e-4 (north_star), continuous predictions 2e-5, discrete decisions
(bucket ids, rounded durations, mel_len, length-regulator rows) bit-exact.
"""
import glob
import os

import numpy as np
import pytest
import torch

from efficientspeech_amd import CONFIGS, _lib
from efficientspeech_amd.synth import synth_phonemes
from oracle import oracle
from tests import helpers as H

pytestmark = pytest.mark.gpu
GOLDEN = sorted(p for p in glob.glob(os.path.join(os.path.dirname(__file__), "golden", "*.npz"))
                if os.path.basename(p).startswith(("tiny_", "small_", "base_")) and "_train_step" not in os.path.basename(p))   # forward
#                              fixtures of the acoustic model (the vocoder, the training step and the loader have their own tests)
DEV = "cuda:0"


@pytest.fixture(scope="module", autouse=True)
def _hip_library_loaded():
    lib = _lib.load()
    assert _lib.backend(lib) == "hip:gfx950", "GPU tests must run on the HIP library, nothing else"
    assert torch.cuda.is_available()


@pytest.fixture(scope="module")
def nets():
    cache = {}

    def get(name, g=None):
        if name not in cache:
            cache[name] = H.make_net(name, DEV, golden=g)
        return cache[name]
    return get


# launch plans: everything fused (default: whole-block kernels, column split, scan inside the variance kernel), one chain
# kernel per stage (merge+qkv | attention+FFN | fuse+variance; also what long sequences use), one kernel per reference op
PLANS = [_lib.FUSE_ALL, 31, 7, 0]     # round-5 chain16 kernels | round-1..4 chain kernels | per-stage | per-op
PLAN_IDS = ["fused", "fused_r4", "staged", "unfused"]


@pytest.mark.parametrize("fusion", PLANS, ids=PLAN_IDS)
@pytest.mark.parametrize("path", GOLDEN, ids=[os.path.basename(p)[:-4] for p in GOLDEN])
def test_golden_vectors(path, fusion, nets):
    """All launch plans against the reference-generated vectors."""
    g = np.load(path)
    name = os.path.basename(path).split("_")[0]
    net, cfg, sd = nets(name, g)
    with _lib.launch_plan(fusion):
        H.check_against_golden(net, g, DEV)


@pytest.mark.parametrize("name,B,T,lens", [
    ("tiny", 8, 70, [70, 66, 51, 40, 33, 17, 9, 2]),      # 3 row tiles, N=70/35 keys, 3 decoder windows
    ("tiny", 5, 128, [128, 128, 100, 64, 1]),
    ("small", 4, 100, [100, 77, 50, 13]),
    ("base", 3, 64, [64, 40, 7]),
    ("base", 2, 256, [256, 200]),                         # T=256: 8 key tiles (attn_kernel<8>)
])
@pytest.mark.parametrize("fusion", PLANS, ids=PLAN_IDS)
def test_eval_path_vs_oracle(name, B, T, lens, fusion, nets):
    with _lib.launch_plan(fusion):
        _eval_path_vs_oracle(name, B, T, lens, nets)


def _eval_path_vs_oracle(name, B, T, lens, nets):
    net, cfg, sd = nets(name)
    ids, mask = synth_phonemes(B, T, 4321, lens)
    x = {"phoneme": torch.from_numpy(ids).to(DEV), "phoneme_mask": torch.from_numpy(mask).to(DEV)}
    with torch.no_grad():
        enc = net.encoder._encode(x)
        mel, mel_len, _ = net(x)
    o = oracle.phoneme2mel(cfg, oracle.Weights(sd), ids, mask)
    # (margin-aware: a flip within helpers.MARGIN of an edge or a .5 is accepted here.  Exact boundaries -- a value ON an edge, a duration
    #  product ON a .5 -- are held bit for bit by tests/test_va_ties.py.)
    err = H.compare_eval_with_oracle(cfg, o, enc, mel, mel_len, sd)
    assert err == err, "a discrete decision flipped inside its margin; pick another seed for this case"
    # rows beyond mel_len are exactly zero (final masked_fill)
    m = mel.cpu().numpy()
    for b in range(B):
        assert not m[b, int(o.mel_len[b]):].any()


@pytest.mark.parametrize("B,T", [(1, 31), (1, 32), (2, 64), (1, 128)])
@pytest.mark.parametrize("fusion", [_lib.FUSE_ALL, 31], ids=["chain16", "chain32"])
def test_variance_adaptor_last_rows_of_every_tile(B, T, fusion, nets):
    """Regression test for the wrong-rows mode of round 4 (profiles/r05_probes/fuse_va_wrong_rows.md): a build of enc_fuse_va_kernel whose
    predictor LayerNorms ran their 32-lane reductions in batches of 8 or 16 rows returned wrong predictions at positions 25..33 of
    every 32-position tile on the GPU (0.4 .. 1.5 off), right everywhere else and right on the simulator.  Every position's pitch /
    energy / duration prediction and duration features against the oracle, for the round-5 kernels and for the fallback kernels."""
    net, cfg, sd = nets("tiny")
    ids, mask = synth_phonemes(B, T, 11)
    x = {"phoneme": torch.from_numpy(ids).to(DEV)}
    if B > 1:
        x["phoneme_mask"] = torch.from_numpy(mask).to(DEV)
    with _lib.launch_plan(fusion), torch.no_grad():
        enc = net.encoder._encode(x, need_lmax=False)
    o = oracle.phoneme2mel(cfg, oracle.Weights(sd), ids, mask if B > 1 else None)
    for key, ref in (("pitch", o.pitch), ("energy", o.energy), ("duration", o.duration)):
        d = np.abs(enc[key].cpu().numpy().reshape(B, T) - ref.reshape(B, T))
        bad = sorted(set(np.argwhere(d > H.PRED_TOL)[:, 1].tolist()))
        assert not bad, (key, "positions", bad, float(d.max()))
    d = np.abs(enc["feat"].cpu().numpy() - o.feat).max(-1)
    bad = sorted(set(np.argwhere(d > H.PRED_TOL)[:, 1].tolist()))
    assert not bad, ("feat", "positions", bad, float(d.max()))


def test_b1_path_has_no_masks(nets):
    net, cfg, sd = nets("tiny")
    ids, _ = synth_phonemes(1, 50, 5)
    with torch.no_grad():
        mel, mel_len, dur = net({"phoneme": torch.from_numpy(ids).to(DEV)})
        pe = net.encoder({"phoneme": torch.from_numpy(ids).to(DEV)})
    assert pe["masks"] is None
    o = oracle.phoneme2mel(cfg, oracle.Weights(sd), ids, None)
    assert np.array_equal(mel_len.cpu().numpy(), o.mel_len)
    assert np.abs(mel.cpu().numpy() - o.mel).max() < H.MEL_TOL


def test_batch_gt1_requires_mask(nets):
    net, _, _ = nets("tiny")
    with pytest.raises(KeyError):
        net({"phoneme": torch.ones((2, 8), dtype=torch.int32, device=DEV)})


def test_list_input_quirk(nets):
    net, _, _ = nets("tiny")
    ids, _ = synth_phonemes(1, 12, 5)
    x = {"phoneme": torch.from_numpy(ids).to(DEV)}
    with torch.no_grad():
        a = net([x])[0]
        b = net(x)[0]
    assert torch.equal(a, b)


def test_decoder_direct_mode_vs_oracle(nets):
    """MelDecoder.forward(features) stand-alone (the reference's module-level API)."""
    for name, L in (("tiny", 300), ("small", 150), ("base", 131)):
        net, cfg, sd = nets(name)
        rng = np.random.default_rng(3)
        feats = rng.standard_normal((3, L, cfg.d4)).astype(np.float32)
        with torch.no_grad():
            mel = net.decoder(torch.from_numpy(feats).to(DEV)).cpu().numpy()
        ref = oracle.mel_decoder(cfg, oracle.Weights(sd), feats)
        assert np.abs(mel - ref).max() < H.MEL_TOL


def test_length_regulator_bit_exact():
    lib = _lib.load()
    rng = np.random.default_rng(11)
    for B, T in ((64, 128), (3, 257), (1, 1)):
        dur = rng.integers(-2, 12, size=(B, T)).astype(np.int32)
        dur[rng.random((B, T)) < 0.2] = 0
        d = torch.from_numpy(dur).to(DEV)
        cum = torch.empty((B, T), dtype=torch.int32, device=DEV)
        mel_len = torch.empty((B,), dtype=torch.int32, device=DEV)
        lmax = torch.empty((1,), dtype=torch.int32, device=DEV)
        s = torch.cuda.current_stream().cuda_stream
        lib.esmi_length_regulate_i32(d.data_ptr(), B, T, cum.data_ptr(), mel_len.data_ptr(), lmax.data_ptr(), s)
        ref_cum = np.cumsum(np.maximum(dur, 0), 1).astype(np.int32)
        assert np.array_equal(cum.cpu().numpy(), ref_cum)
        assert np.array_equal(mel_len.cpu().numpy(), ref_cum[:, -1])
        L = int(lmax.item())
        assert L == ref_cum[:, -1].max()
        for Lq in (L, L + 5, max(L - 3, 1)):
            idx = torch.empty((B, Lq), dtype=torch.int32, device=DEV)
            lib.esmi_length_regulator_indices_i32(cum.data_ptr(), B, T, Lq, idx.data_ptr(), s)
            assert np.array_equal(idx.cpu().numpy(), oracle.length_regulate(dur, Lq))


def test_upsampler_module_vs_oracle(nets):
    net, cfg, _ = nets("tiny")
    rng = np.random.default_rng(5)
    B, T, Cc = 4, 33, 128
    feat = rng.standard_normal((B, T, Cc)).astype(np.float32)
    dur = rng.integers(0, 7, size=(B, T)).astype(np.int32)
    mask = np.arange(T)[None] >= np.array([33, 20, 11, 5])[:, None]
    dur[mask] = 0
    fm = np.repeat(mask[:, :, None], Cc, 2)
    f, m, ml = net.encoder.feature_upsampler(torch.from_numpy(feat).to(DEV), torch.from_numpy(fm).to(DEV),
                                             torch.from_numpy(dur).to(DEV))
    L = int(dur.sum(1).max())
    idx = oracle.length_regulate(dur, L)
    rf, rm = oracle.upsample(feat, mask, idx)
    assert ml.dtype == torch.int32 and np.array_equal(ml.cpu().numpy(), dur.sum(1))
    assert np.array_equal(f.cpu().numpy(), rf)
    assert m.dtype == torch.bool and np.array_equal(m[:, :, 0].cpu().numpy(), rm)


def test_full_size_tiny_properties(nets):
    """BASELINE configs[1]: tiny ES, B=256 T=128, D-const 6 (L=768): spot-check against the oracle and
    size-independent properties (determinism, batch-split invariance, mel_len == sum of durations)."""
    net, cfg, sd = nets("tiny")
    B, T, D = 256, 128, 6
    ids, mask = synth_phonemes(B, T, 1234)
    dur = torch.full((B, T), D, dtype=torch.int32, device=DEV)
    x = {"phoneme": torch.from_numpy(ids).to(DEV), "phoneme_mask": torch.from_numpy(mask).to(DEV),
         "duration_forced": dur, "max_mel_len": T * D}
    with torch.no_grad():
        enc = net.encoder._encode(x)
        mel, mel_len, _ = net(x)
        mel2, _, _ = net(x)
    assert mel.shape == (B, T * D, 80)
    assert torch.equal(mel, mel2), "non-deterministic kernel"
    assert (mel_len == T * D).all()
    assert torch.isfinite(mel).all()
    # batch-split invariance: a 32-utterance shard with the same padded length is bit-identical
    xs = {k: (v[64:96] if torch.is_tensor(v) else v) for k, v in x.items()}
    with torch.no_grad():
        mel_s, _, _ = net(xs)
    assert torch.equal(mel_s, mel[64:96])
    # oracle spot check on 6 utterances (teacher-forced with the HIP path's own predictions so that the
    # bucket decisions are identical; durations forced)
    sel = [0, 1, 77, 128, 200, 255]
    o = oracle.phoneme2mel(cfg, oracle.Weights(sd), ids[sel], mask[sel],
                           pitch=enc["pitch"][sel, :, 0].cpu().numpy(), energy=enc["energy"][sel, :, 0].cpu().numpy(),
                           duration=np.full((len(sel), T), D, np.int32), max_mel_len=T * D)
    np.testing.assert_allclose(enc["pitch"][sel].cpu().numpy(), o.pitch, atol=H.PRED_TOL, rtol=0)
    err = np.abs(mel[sel].cpu().numpy() - o.mel).max()
    assert err < H.MEL_TOL, err


def test_smoke_entry():
    import __graft_entry__ as g
    g.smoke()


def test_edge_cases(nets):
    """T = 1; all durations zero (empty mel); an output-length hint above the true batch maximum (the decoder then derives
    the padded length L from mel_len itself); T = 256 on tiny ES (8 key tiles, three workgroups per utterance)."""
    net, cfg, sd = nets("tiny")
    w = oracle.Weights(sd)
    # T = 1, B = 1 and B = 3
    for B in (1, 3):
        ids, mask = synth_phonemes(B, 1, 3)
        x = {"phoneme": torch.from_numpy(ids).to(DEV)}
        if B > 1:
            x["phoneme_mask"] = torch.from_numpy(mask).to(DEV)
        with torch.no_grad():
            mel, mel_len, _ = net(x)
        o = oracle.phoneme2mel(cfg, w, ids, mask if B > 1 else None)
        assert np.array_equal(mel_len.cpu().numpy(), o.mel_len) and mel.shape == o.mel.shape
        if o.mel.size:
            assert np.abs(mel.cpu().numpy() - o.mel).max() < H.MEL_TOL
    # every duration zero: L = 0
    ids, mask = synth_phonemes(2, 9, 4, [9, 5])
    x = {"phoneme": torch.from_numpy(ids).to(DEV), "phoneme_mask": torch.from_numpy(mask).to(DEV),
         "duration_forced": torch.zeros((2, 9), dtype=torch.int32, device=DEV)}
    with torch.no_grad():
        mel, mel_len, _ = net(x)
    assert mel.shape == (2, 0, 80) and not mel_len.any()
    # hint above the batch maximum
    B, T = 3, 40
    ids, mask = synth_phonemes(B, T, 9, [40, 31, 7])
    dur = np.full((B, T), 5, np.int32)
    x = {"phoneme": torch.from_numpy(ids).to(DEV), "phoneme_mask": torch.from_numpy(mask).to(DEV),
         "duration_forced": torch.from_numpy(dur).to(DEV), "max_mel_len": 230}
    with torch.no_grad():
        enc = net.encoder._encode(x)
        mel, mel_len, _ = net(x)
    o = oracle.phoneme2mel(cfg, w, ids, mask, pitch=enc["pitch"][..., 0].cpu().numpy(),
                           energy=enc["energy"][..., 0].cpu().numpy(), duration=dur)
    assert mel.shape == (B, 230, 80) and np.array_equal(mel_len.cpu().numpy(), o.mel_len) and o.mel.shape[1] == 200
    assert np.abs(mel[:, :200].cpu().numpy() - o.mel).max() < H.MEL_TOL and not mel[:, 200:].any()
    # T = 256
    ids, mask = synth_phonemes(2, 256, 21, [256, 190])
    dur = np.ones((2, 256), np.int32)
    x = {"phoneme": torch.from_numpy(ids).to(DEV), "phoneme_mask": torch.from_numpy(mask).to(DEV),
         "duration_forced": torch.from_numpy(dur).to(DEV)}
    with torch.no_grad():
        enc = net.encoder._encode(x)
        mel, mel_len, _ = net(x)
    o = oracle.phoneme2mel(cfg, w, ids, mask, pitch=enc["pitch"][..., 0].cpu().numpy(),
                           energy=enc["energy"][..., 0].cpu().numpy(), duration=dur)
    np.testing.assert_allclose(enc["pitch"].cpu().numpy(), o.pitch, atol=H.PRED_TOL, rtol=0)
    assert np.array_equal(mel_len.cpu().numpy(), o.mel_len)
    assert np.abs(mel.cpu().numpy() - o.mel).max() < H.MEL_TOL


@pytest.mark.parametrize("seed", list(range(12)))
def test_random_shapes_vs_oracle(seed, nets):
    """Seeded random batch shapes, ragged lengths and forced durations (0..7, zeros included) on tiny ES: every tiling /
    halo / gather branch of the default plan (T <= 128: whole-block kernels, phoneme-rate decoder head, scan inside the
    variance kernel; T > 128: per-stage kernels with halo workgroups, in-kernel proj) against the oracle."""
    rng = np.random.default_rng(1000 + seed)
    net, cfg, sd = nets("tiny")
    B = int(rng.integers(1, 9))
    T = int(rng.integers(1, 200)) if seed % 3 else int(rng.integers(97, 129))
    lens = sorted((int(v) for v in rng.integers(1, T + 1, size=B)), reverse=True)
    lens[0] = T
    ids, mask = synth_phonemes(B, T, 50 + seed, lens)
    dur = rng.integers(0, 8, size=(B, T)).astype(np.int32)
    dur[rng.random((B, T)) < 0.15] = 0
    x = {"phoneme": torch.from_numpy(ids).to(DEV), "duration_forced": torch.from_numpy(dur).to(DEV)}
    if B > 1:
        x["phoneme_mask"] = torch.from_numpy(mask).to(DEV)
    if seed % 2:
        x["max_mel_len"] = int(dur.sum(1).max()) + int(rng.integers(0, 40))
    with torch.no_grad():
        enc = net.encoder._encode(x)
        mel, mel_len, _ = net(x)
    o = oracle.phoneme2mel(cfg, oracle.Weights(sd), ids, mask if B > 1 else None,
                           pitch=enc["pitch"][..., 0].cpu().numpy(), energy=enc["energy"][..., 0].cpu().numpy(), duration=dur)
    np.testing.assert_allclose(enc["pitch"].cpu().numpy(), o.pitch, atol=H.PRED_TOL, rtol=0)
    np.testing.assert_allclose(enc["duration"].cpu().numpy(), o.duration, atol=H.PRED_TOL, rtol=0)
    assert np.array_equal(mel_len.cpu().numpy(), o.mel_len)
    L = o.mel.shape[1]
    m = mel.cpu().numpy()
    assert m.shape[1] >= L and not m[:, L:].any()
    if L:
        assert np.abs(m[:, :L] - o.mel).max() < H.MEL_TOL


@pytest.mark.parametrize("seed", list(range(6)))
@pytest.mark.parametrize("name", ["small", "base"])
def test_random_shapes_wide_models_vs_oracle(name, seed, nets):
    """The same on small / base ES (round 6: the register-resident dim-64 / dim-128 kernels -- enc_va64, enc_post_attn64, enc_pred128,
    enc_fuse128, enc_post_attn128, enc_merge_q256 -- own one workgroup per utterance for T <= 256): odd and short lengths, ragged masks,
    B = 1 without a mask, zero durations, length hints; teacher-forced with the HIP path's own pitch / energy so that bucket decisions
    cannot disagree (predictions held to PRED_TOL)."""
    rng = np.random.default_rng(7000 + 31 * seed + (0 if name == "small" else 1))
    net, cfg, sd = nets(name)
    B = 1 if seed == 0 else int(rng.integers(2, 6))
    T = [1, 17, 255, 256][seed] if seed < 4 else int(rng.integers(2, 257))
    lens = sorted((int(v) for v in rng.integers(1, T + 1, size=B)), reverse=True)
    lens[0] = T
    ids, mask = synth_phonemes(B, T, 90 + seed, lens)
    dur = rng.integers(0, 5, size=(B, T)).astype(np.int32)
    dur[rng.random((B, T)) < 0.15] = 0
    x = {"phoneme": torch.from_numpy(ids).to(DEV), "duration_forced": torch.from_numpy(dur).to(DEV)}
    if B > 1:
        x["phoneme_mask"] = torch.from_numpy(mask).to(DEV)
    if seed % 2:
        x["max_mel_len"] = int(dur.sum(1).max()) + int(rng.integers(0, 40))
    with torch.no_grad():
        enc = net.encoder._encode(x)
        mel, mel_len, _ = net(x)
    o = oracle.phoneme2mel(cfg, oracle.Weights(sd), ids, mask if B > 1 else None,
                           pitch=enc["pitch"][..., 0].cpu().numpy(), energy=enc["energy"][..., 0].cpu().numpy(), duration=dur)
    np.testing.assert_allclose(enc["pitch"].cpu().numpy(), o.pitch, atol=H.PRED_TOL, rtol=0)
    np.testing.assert_allclose(enc["energy"].cpu().numpy(), o.energy, atol=H.PRED_TOL, rtol=0)
    np.testing.assert_allclose(enc["duration"].cpu().numpy(), o.duration, atol=H.PRED_TOL, rtol=0)
    assert np.array_equal(mel_len.cpu().numpy(), o.mel_len)
    L = o.mel.shape[1]
    m = mel.cpu().numpy()
    assert m.shape[1] >= L and not m[:, L:].any()
    if L:
        assert np.abs(m[:, :L] - o.mel).max() < H.MEL_TOL


def test_large_batch_uses_other_kernels(nets):
    """B = 512, T = 64: too many waves for the column-split block-1 kernel, so the plain whole-block instantiation runs;
    four utterances against the oracle (teacher-forced with the HIP path's own pitch / energy, durations forced)."""
    net, cfg, sd = nets("tiny")
    B, T = 512, 64
    ids, mask = synth_phonemes(B, T, 5)
    dur = np.full((B, T), 2, np.int32)
    x = {"phoneme": torch.from_numpy(ids).to(DEV), "phoneme_mask": torch.from_numpy(mask).to(DEV),
         "duration_forced": torch.from_numpy(dur).to(DEV), "max_mel_len": 2 * T}
    with torch.no_grad():
        enc = net.encoder._encode(x)
        mel, mel_len, _ = net(x)
    sel = [0, 100, 300, 511]
    o = oracle.phoneme2mel(cfg, oracle.Weights(sd), ids[sel], mask[sel], pitch=enc["pitch"][sel, :, 0].cpu().numpy(),
                           energy=enc["energy"][sel, :, 0].cpu().numpy(), duration=dur[sel], max_mel_len=2 * T)
    np.testing.assert_allclose(enc["pitch"][sel].cpu().numpy(), o.pitch, atol=H.PRED_TOL, rtol=0)
    assert (mel_len == 2 * T).all()
    assert np.abs(mel[sel].cpu().numpy() - o.mel).max() < H.MEL_TOL


def test_exact_fp32_mfma_build():
    """The alternative build (mel-decoder contractions on v_mfma_f32_32x32x2_f32 instead of split 16-bit products) is the same
    ABI; run two golden fixtures, one saturated-row decoder case on base ES (tests/test_weight_profiles.py) and the smoke check
    through it in a fresh interpreter (ESMI_LIB selects the library)."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib = os.path.join(root, "efficientspeech_amd", "libesmi_fp32mfma.so")
    if not os.path.exists(lib):
        pytest.skip("libesmi_fp32mfma.so not built")
    code = (
        "import numpy as np, os, sys; sys.path.insert(0, %r)\n"
        "from tests import helpers as H\n"
        "from efficientspeech_amd import _lib\n"
        "assert _lib.load().esmi_build_config().decode().startswith('dec_gemm=fp32-mfma,enc_gemm=fp32-mfma')\n"
        "for f in ('tiny_eval_pad_t17.npz', 'tiny_forced_d6_t16.npz'):\n"
        "    g = np.load(os.path.join(%r, 'tests', 'golden', f))\n"
        "    net, cfg, sd = H.make_net('tiny', 'cuda', golden=g)\n"
        "    H.check_against_golden(net, g, 'cuda')\n"
        "from tests import test_weight_profiles as WP\n"      # this build shares the dx2 = 256 LayerNorm on the accumulators
        "WP.check_decoder('cuda', 'base', 'sat+3x0.3', 1, 40)\n"
        "import __graft_entry__ as ge; ge.smoke()\n" % (root, root))
    env = dict(os.environ, ESMI_LIB=lib)
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "smoke ok" in r.stdout


@pytest.mark.parametrize("s_w,s_g", [(8.0, 1.0), (0.02, 1.0), (1.0, 30.0), (1.0, 1e-3), (5.0, 0.01)])
def test_split_contraction_operand_scales(s_w, s_g):
    """The split-f16 contractions (esmi_dev.h) keep fp32-level accuracy when weights and activations sit far from O(1): pointwise
    / mel weights scaled by s_w, LayerNorm gains (= the magnitude of the activations feeding the next contraction) by s_g."""
    from efficientspeech_amd import build_phoneme2mel, load_numpy_state_dict
    from efficientspeech_amd.synth import synth_state_dict
    cfg = CONFIGS["tiny"]
    sd = synth_state_dict(cfg, 77)
    for k in list(sd):
        if not k.startswith("decoder."):
            continue
        if k.endswith(".0.1.weight") or k == "decoder.mel_linear.weight" or k == "decoder.proj.0.weight":
            sd[k] = (sd[k] * np.float32(s_w)).astype(np.float32)              # pointwise conv / Linear weights
        elif k.endswith(".weight") and sd[k].ndim == 1:
            sd[k] = (sd[k] * np.float32(s_g)).astype(np.float32)              # LayerNorm gains
    net = build_phoneme2mel(cfg)
    load_numpy_state_dict(net, sd)
    net = net.to(DEV)
    rng = np.random.default_rng(9)
    feats = rng.standard_normal((2, 200, cfg.d4)).astype(np.float32)
    with torch.no_grad():
        mel = net.decoder(torch.from_numpy(feats).to(DEV)).cpu().numpy()
    ref = oracle.mel_decoder(cfg, oracle.Weights(sd), feats)
    assert np.isfinite(mel).all()
    assert np.abs(mel - ref).max() < H.MEL_TOL * max(1.0, float(np.abs(ref).max())), (np.abs(mel - ref).max(), np.abs(ref).max())


@pytest.mark.parametrize("n_mel", [78, 33, 96])
def test_decoder_other_mel_widths(n_mel):
    """n_mel not a multiple of 4 takes the scalar mel-store path of the decoder (rows are not 16-byte multiples); 96 is the
    widest supported (three column tiles)."""
    import dataclasses
    from efficientspeech_amd import build_phoneme2mel, load_numpy_state_dict
    from efficientspeech_amd.synth import synth_state_dict
    cfg = dataclasses.replace(CONFIGS["tiny"], n_mel_channels=n_mel)
    sd = synth_state_dict(cfg, 5)
    net = build_phoneme2mel(cfg)
    load_numpy_state_dict(net, sd)
    net = net.to(DEV)
    rng = np.random.default_rng(2)
    feats = rng.standard_normal((2, 150, cfg.d4)).astype(np.float32)
    with torch.no_grad():
        mel = net.decoder(torch.from_numpy(feats).to(DEV)).cpu().numpy()
    ref = oracle.mel_decoder(cfg, oracle.Weights(sd), feats)
    assert mel.shape == ref.shape == (2, 150, n_mel)
    assert np.abs(mel - ref).max() < H.MEL_TOL
    ids, mask = synth_phonemes(3, 40, 9, [40, 31, 7])       # and through the fused encoder -> decoder path (h0 gather)
    dur = np.random.default_rng(4).integers(0, 6, size=(3, 40)).astype(np.int32)   # forced: no rounding decision can flip
    x = {"phoneme": torch.from_numpy(ids).to(DEV), "phoneme_mask": torch.from_numpy(mask).to(DEV),
         "duration_forced": torch.from_numpy(dur).to(DEV)}
    with torch.no_grad():
        enc = net.encoder._encode(x)
        mel2, mel_len, _ = net(x)
    o = oracle.phoneme2mel(cfg, oracle.Weights(sd), ids, mask, pitch=enc["pitch"][..., 0].cpu().numpy(),
                           energy=enc["energy"][..., 0].cpu().numpy(), duration=dur)
    assert np.array_equal(mel_len.cpu().numpy(), o.mel_len)
    assert mel2.shape == o.mel.shape and np.abs(mel2.cpu().numpy() - o.mel).max() < H.MEL_TOL


def _full_size_properties(name, B, T, D, nets, n_spot=4):
    """BASELINE shape of one model size under ALL THREE launch plans: determinism, batch-shard invariance at the same padded
    length, mel_len, and an oracle spot check on `n_spot` utterances (teacher-forced with the HIP path's own pitch / energy so
    that bucket decisions agree; durations forced D-const)."""
    net, cfg, sd = nets(name)
    ids, mask = synth_phonemes(B, T, 1234)
    x = {"phoneme": torch.from_numpy(ids).to(DEV), "phoneme_mask": torch.from_numpy(mask).to(DEV),
         "duration_forced": torch.full((B, T), D, dtype=torch.int32, device=DEV), "max_mel_len": T * D}
    sel = sorted({0, 1, B // 3, B // 2, B - 1})[:max(n_spot, 4)]
    ref = None
    for plan in PLANS:
        with _lib.launch_plan(plan), torch.no_grad():
            enc = net.encoder._encode(x)
            mel, mel_len, _ = net(x)
            mel2, _, _ = net(x)
            lo = B // 4
            xs = {k: (v[lo:lo + 32] if torch.is_tensor(v) else v) for k, v in x.items()}
            mel_s, _, _ = net(xs)
        assert mel.shape == (B, T * D, 80) and (mel_len == T * D).all() and torch.isfinite(mel).all()
        assert torch.equal(mel, mel2), f"plan {plan}: non-deterministic"
        assert torch.equal(mel_s, mel[lo:lo + 32]), f"plan {plan}: result depends on the batch split"
        if ref is None:
            o = oracle.phoneme2mel(cfg, oracle.Weights(sd), ids[sel], mask[sel],
                                   pitch=enc["pitch"][sel, :, 0].cpu().numpy(), energy=enc["energy"][sel, :, 0].cpu().numpy(),
                                   duration=np.full((len(sel), T), D, np.int32), max_mel_len=T * D)
            np.testing.assert_allclose(enc["pitch"][sel].cpu().numpy(), o.pitch, atol=H.PRED_TOL, rtol=0)
            np.testing.assert_allclose(enc["energy"][sel].cpu().numpy(), o.energy, atol=H.PRED_TOL, rtol=0)
            np.testing.assert_allclose(enc["duration"][sel].cpu().numpy(), o.duration, atol=H.PRED_TOL, rtol=0)
            ref = o.mel
        err = np.abs(mel[sel].cpu().numpy() - ref).max()
        assert err < H.MEL_TOL, (plan, err)
        del mel, mel2, mel_s, enc


def _full_size_drand(name, B, T, nets):
    """BASELINE shape of one model size on the robustness workload: ragged phoneme lengths, durations U[1, 11]
    seed 1234 (0 on padded phonemes), the padded length derived on the device.  Against the oracle on >= 4 utterances incl. the
    shortest, the longest and one whose last decoder windows are all padding (the decoder skips those): mel < 1e-4; on the WHOLE
    batch: mel_len bit-exact, rows >= mel_len exactly zero.  The spot check is teacher-forced with the HIP path's own pitch /
    energy predictions so that bucket decisions cannot disagree (the predictions themselves are held to PRED_TOL); the
    free-running comparison -- no forced values at all, discrete decisions margin-aware -- is `_full_size_free_running`."""
    net, cfg, sd = nets(name)
    rng = np.random.default_rng(1234)
    lens = rng.integers(max(T // 8, 1), T + 1, size=B)
    lens[0], lens[B - 1] = T, max(T // 8, 1)
    ids, mask = synth_phonemes(B, T, 1234, lens)
    dur = rng.integers(1, 12, size=(B, T)).astype(np.int32)
    dur[mask] = 0
    ref_len = dur.sum(1).astype(np.int32)
    L = int(ref_len.max())
    x = {"phoneme": torch.from_numpy(ids).to(DEV), "phoneme_mask": torch.from_numpy(mask).to(DEV),
         "duration_forced": torch.from_numpy(dur).to(DEV)}
    all_pad_tail = np.flatnonzero(ref_len < L - 256)          # at least one whole 128-row tile of padding behind the last valid frame
    assert all_pad_tail.size, "pick lengths that leave an utterance with an all-padding window"
    sel = sorted({int(ref_len.argmin()), int(ref_len.argmax()), int(all_pad_tail[len(all_pad_tail) // 2]), 0, B // 2})
    ref = None
    for plan in (_lib.FUSE_ALL, 0):
        for hint in (None, L + 37):      # the reference's call (host sync for L) / an allocation hint above the batch maximum
            xx = dict(x) if hint is None else dict(x, max_mel_len=hint)
            with _lib.launch_plan(plan), torch.no_grad():
                enc = net.encoder._encode(xx)
                mel, mel_len, _ = net(xx)
            assert mel_len.dtype == torch.int32 and np.array_equal(mel_len.cpu().numpy(), ref_len), plan
            assert mel.shape == (B, hint or L, 80) and torch.isfinite(mel).all()
            beyond = torch.arange(mel.shape[1], device=DEV)[None, :] >= mel_len[:, None].long()
            assert not mel[beyond].any(), f"plan {plan}: rows >= mel_len are not exactly zero"
            if ref is None:
                ref = oracle.phoneme2mel(cfg, oracle.Weights(sd), ids[sel], mask[sel], pitch=enc["pitch"][sel, :, 0].cpu().numpy(),
                                         energy=enc["energy"][sel, :, 0].cpu().numpy(), duration=dur[sel], max_mel_len=L)
                np.testing.assert_allclose(enc["pitch"][sel].cpu().numpy(), ref.pitch, atol=H.PRED_TOL, rtol=0)
                np.testing.assert_allclose(enc["energy"][sel].cpu().numpy(), ref.energy, atol=H.PRED_TOL, rtol=0)
                np.testing.assert_allclose(enc["duration"][sel].cpu().numpy(), ref.duration, atol=H.PRED_TOL, rtol=0)
                assert np.array_equal(ref.mel_len, ref_len[sel])
            err = np.abs(mel[sel, :L].cpu().numpy() - ref.mel).max()
            assert err < H.MEL_TOL, (plan, hint, err)
            del mel, enc


def _full_size_free_running(name, B, T, nets, n_free=3):
    """The BASELINE batch with NOTHING forced (predicted durations, predicted pitch / energy buckets) against the oracle's own eval
    run on `n_free` of its utterances: discrete decisions may differ only inside their margins (helpers.compare_eval_with_oracle);
    at least one utterance must come through without any flip and is then compared to < 1e-4."""
    net, cfg, sd = nets(name)
    lens = np.full(B, T)
    lens[1::2] = np.random.default_rng(77).integers(T // 2, T + 1, size=B // 2)
    ids, mask = synth_phonemes(B, T, 99, lens)
    x = {"phoneme": torch.from_numpy(ids).to(DEV), "phoneme_mask": torch.from_numpy(mask).to(DEV)}
    with torch.no_grad():
        enc = net.encoder._encode(x)
        mel, mel_len, _ = net(x)
    compared = 0
    L = int(mel_len.max())
    assert mel.shape == (B, L, 80)
    for b in (0, B // 2 + 1, B - 1)[:n_free]:
        s = [b, b]        # the oracle's masked (B > 1) flow on this utterance alone, padded to the batch's length: the frames in
        #                   [mel_len, L) are computed and reach the last valid frames through the k-tap convolutions
        o = oracle.phoneme2mel(cfg, oracle.Weights(sd), ids[s], mask[s], max_mel_len=L)
        e1 = {k: v[s] for k, v in enc.items() if torch.is_tensor(v) and v.dim() >= 1 and v.shape[0] == B}
        err = H.compare_eval_with_oracle(cfg, o, e1, mel[s], mel_len[s], sd)      # (margin-aware; exact ties: tests/test_va_ties.py)
        compared += err == err
        assert not mel[b, int(mel_len[b]):].any()
    assert compared, "every free-running utterance had a decision inside its margin; pick other seeds"


def test_full_size_tiny_drand(nets):
    """BASELINE configs[1] shape on the D-rand / ragged workload + a free-running batch."""
    _full_size_drand("tiny", 256, 128, nets)
    _full_size_free_running("tiny", 256, 128, nets)


def test_full_size_small_drand(nets):
    _full_size_drand("small", 256, 256, nets)
    _full_size_free_running("small", 256, 256, nets)


def test_full_size_base_drand(nets):
    _full_size_drand("base", 512, 256, nets)
    _full_size_free_running("base", 512, 256, nets, n_free=2)
    torch.cuda.empty_cache()


def test_full_size_small_properties(nets):
    """BASELINE configs[2]: small ES, B=256 T=256, D-const 6 (L=1536): the dim-64 halo-plan instantiations at size."""
    _full_size_properties("small", 256, 256, 6, nets)


def test_full_size_base_properties(nets):
    """BASELINE configs[3] (per-node batch): base ES, B=512 T=256, D-const 6."""
    _full_size_properties("base", 512, 256, 6, nets)
    torch.cuda.empty_cache()


@pytest.mark.parametrize("name", ["tiny", "small", "base"])
def test_submodule_forwards(name, nets):
    """SelfAttention / MixFFN / AcousticDecoder.forward and get_embedding on their own (reference module-level API)."""
    net, cfg, sd = nets(name)
    H.check_submodule_forwards(net, cfg, sd, DEV)


@pytest.mark.parametrize("name", ["tiny", "small", "base"])
def test_decoder_head_at_phoneme_rate(name, nets):
    """esmi_decoder_head_f32 vs torch fp32, and the h0-gathering decoder vs the decoder that runs its first stage per frame
    (dx2 = 128 and 256)."""
    net, cfg, sd = nets(name)
    H.check_decoder_head(net, cfg, DEV)


@pytest.mark.parametrize("name", ["tiny", "small", "base"])
def test_embedding_folded_into_merge_conv(name, nets):
    """Block 0's table path (emb_conv) == the gather + composed-conv path, for the chain kernels of every size."""
    net, cfg, sd = nets(name)
    H.check_embedding_folded_into_merge_conv(net, cfg, DEV)


@pytest.mark.parametrize("name", ["tiny", "small", "base"])
def test_ffn_linear_folded_into_conv(name, nets):
    """MixFFN's folded front (ffn_cw) == Linear + conv, chain kernels and per-op plan, padded batches and one-position sequences."""
    net, cfg, sd = nets(name)
    H.check_ffn_linear_folded_into_conv(net, cfg, DEV)


@pytest.mark.parametrize("name", ["small", "base"])
def test_decoder_chunk_walk_equals_windows(name, nets):
    """The dx2 = 256 decoder with carried rows (workspace) == the same kernel with every window's halos recomputed: several
    segments per utterance (B = 3), whole-utterance walks (B = 256: one workgroup per utterance, 6 chunks)."""
    net, cfg, sd = nets(name)
    H.check_decoder_chunk_walk(net, cfg, DEV, cases=((3, 70, 9), (256, 100, 6)))


def test_split_range_guard_and_encoder_operand_scales():
    """(1) a weight outside the split-f16 range is refused at pack time; (2) encoder-side operands far from O(1): embedding
    rows x 40 (the un-normalised conv output that feeds qkv grows with them), merge / qkv / MixFFN weights x 0.05 .. x 6."""
    from efficientspeech_amd import build_phoneme2mel, load_numpy_state_dict
    from efficientspeech_amd.synth import synth_state_dict
    cfg = CONFIGS["tiny"]
    if _lib.load().esmi_split_weight_limit() != float("inf"):
        sd = synth_state_dict(cfg, 5)
        sd["encoder.encoder.attn_blocks.1.3.mlp1.weight"] = sd["encoder.encoder.attn_blocks.1.3.mlp1.weight"] * np.float32(4000.0)
        net = build_phoneme2mel(cfg)
        load_numpy_state_dict(net, sd)
        net = net.to(DEV)
        ids, mask = synth_phonemes(2, 9, 1, [9, 4])
        with pytest.raises(ValueError, match="libesmi_fp32mfma"), torch.no_grad():
            net({"phoneme": torch.from_numpy(ids).to(DEV), "phoneme_mask": torch.from_numpy(mask).to(DEV)})
    for s_e, s_w in ((40.0, 1.0), (1.0, 6.0), (0.02, 1.0), (3.0, 0.05), (25.0, 3.0)):
        sd = synth_state_dict(cfg, 77)
        sd["encoder.encoder.embed.weight"] = (sd["encoder.encoder.embed.weight"] * np.float32(s_e)).astype(np.float32)
        for k in list(sd):
            if k.startswith("encoder.encoder.attn_blocks.") and k.endswith("weight") and sd[k].ndim >= 2:
                sd[k] = (sd[k] * np.float32(s_w)).astype(np.float32)
        net = build_phoneme2mel(cfg)
        load_numpy_state_dict(net, sd)
        net = net.to(DEV)
        ids, mask = synth_phonemes(3, 50, 8, [50, 37, 12])
        x = {"phoneme": torch.from_numpy(ids).to(DEV), "phoneme_mask": torch.from_numpy(mask).to(DEV)}
        with torch.no_grad():
            feats, _ = net.encoder.encoder(x["phoneme"], x["phoneme_mask"])
        o = oracle.phoneme_encoder(cfg, oracle.Weights(sd), ids, mask, taps=True)
        for i, f in enumerate(feats):
            got, ref = f.cpu().numpy(), o.f_taps[i]
            assert np.isfinite(got).all()
            # the block outputs are LayerNorm'd (O(1)); the tolerance is the predictors' one
            np.testing.assert_allclose(got, ref, atol=5 * H.PRED_TOL, rtol=0, err_msg=f"embed x{s_e}, weights x{s_w}, block {i}")


def test_two_stream_pipeline_matches_single_stream(nets):
    """ShardedMelPipeline(two_stream=True): encoder side of step i+1 under the decoder of step i.  DIFFERENT inputs every
    step (a recycled h0 / feat block would show), results compared with plain single-stream forwards."""
    from efficientspeech_amd.sharded import ShardedMelPipeline
    net, cfg, sd = nets("tiny")
    B, T, D = 64, 96, 5
    xs = []
    for step in range(6):
        ids, mask = synth_phonemes(B, T, 500 + step)
        xs.append({"phoneme": torch.from_numpy(ids).to(DEV), "phoneme_mask": torch.from_numpy(mask).to(DEV),
                   "duration_forced": torch.full((B, T), D, dtype=torch.int32, device=DEV), "max_mel_len": T * D})
    with torch.no_grad():
        refs = [net(x)[0].clone() for x in xs]
        pipe = ShardedMelPipeline(net, world_size=1, gather=False, two_stream=True)
        got = []
        for x in xs:
            mel, _ = pipe.step(x)
            with torch.cuda.stream(pipe.s_dec):          # a consumer on the producing stream: no wait on the caller's stream,
                got.append(mel.clone())                   # so step i+1's encoder side really runs under step i's decoder
        pipe.flush()
        pipe.wait_last()
        torch.cuda.synchronize()
    for step, (a, b) in enumerate(zip(refs, got)):
        assert torch.equal(a, b), f"step {step}"


@pytest.mark.parametrize("name,B,T,lens", [("tiny", 3, 300, [300, 257, 31]), ("base", 2, 260, [260, 200]), ("small", 1, 513, [513])])
def test_long_sequences_beyond_256(name, B, T, lens, nets):
    """The reference has no sequence limit (README: long text).  T > 256: block 0 attends over more than 256 keys -- the
    key-chunked two-sweep attention kernel (attention.h) behind the per-op plan; everything else tiles as usual."""
    net, cfg, sd = nets(name)
    ids, mask = synth_phonemes(B, T, 77, lens)
    dur = np.random.default_rng(5).integers(0, 4, size=(B, T)).astype(np.int32)
    x = {"phoneme": torch.from_numpy(ids).to(DEV), "duration_forced": torch.from_numpy(dur).to(DEV)}
    if B > 1:
        x["phoneme_mask"] = torch.from_numpy(mask).to(DEV)
    with torch.no_grad():
        enc = net.encoder._encode(x)
        mel, mel_len, _ = net(x)
    o = oracle.phoneme2mel(cfg, oracle.Weights(sd), ids, mask if B > 1 else None, pitch=enc["pitch"][..., 0].cpu().numpy(),
                           energy=enc["energy"][..., 0].cpu().numpy(), duration=dur)
    np.testing.assert_allclose(enc["pitch"].cpu().numpy(), o.pitch, atol=H.PRED_TOL, rtol=0)
    np.testing.assert_allclose(enc["duration"].cpu().numpy(), o.duration, atol=H.PRED_TOL, rtol=0)
    assert np.array_equal(mel_len.cpu().numpy(), o.mel_len)
    assert mel.shape == o.mel.shape and np.abs(mel.cpu().numpy() - o.mel).max() < H.MEL_TOL


def test_model_wrapper_and_bucket_scheduler():
    """model.py-shaped wrapper on a padded B > 1 batch and a B == 1 call, and the length-bucketed scheduler, vs the oracle."""
    H.check_wrapper_and_scheduler(DEV)


HIFIGAN_GOLDEN = sorted(glob.glob(os.path.join(os.path.dirname(__file__), "golden", "hifigan_*.npz")))


@pytest.mark.parametrize("path", HIFIGAN_GOLDEN, ids=[os.path.basename(p)[:-4] for p in HIFIGAN_GOLDEN])
def test_hifigan_generator_golden(path):
    """HiFi-GAN generator v1 / v2 / v3 against the waveforms of the reference's hifigan.Generator."""
    H.check_hifigan_golden(path, DEV)


def test_hifigan_end_to_end_vs_oracle():
    """phonemes -> mel -> waveform through the model.py-shaped wrapper with the HIP vocoder plugged in as `.hifigan`
    (model.py:159-164), against oracle acoustic model + oracle vocoder; a batch large enough for several row tiles."""
    from efficientspeech_amd import EfficientSpeech
    from efficientspeech_amd.hifigan import HIFIGAN_CONFIGS, Generator, synth_hifigan_state_dict
    from efficientspeech_amd.synth import synth_state_dict
    cfg, h = CONFIGS["tiny"], HIFIGAN_CONFIGS["v2"]
    sd, vsd = synth_state_dict(cfg, 1234), synth_hifigan_state_dict(h, 1234)
    voc = Generator(h)
    model = EfficientSpeech.from_config("tiny", hifigan=voc)
    model.phoneme2mel.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    voc.load_state_dict({k: torch.from_numpy(v) for k, v in vsd.items()}, strict=True)
    model = model.to(DEV).eval()
    B, T = 3, 40
    ids, mask = synth_phonemes(B, T, 12, [40, 29, 11])
    dur = np.random.default_rng(3).integers(1, 5, size=(B, T)).astype(np.int32)
    x = {"phoneme": torch.from_numpy(ids).to(DEV), "phoneme_mask": torch.from_numpy(mask).to(DEV),
         "duration_forced": torch.from_numpy(dur).to(DEV)}
    with torch.no_grad():
        enc = model.phoneme2mel.encoder._encode(x)
        wav, mel_len, _ = model(x)
    o = oracle.phoneme2mel(cfg, oracle.Weights(sd), ids, mask, pitch=enc["pitch"][..., 0].cpu().numpy(),
                           energy=enc["energy"][..., 0].cpu().numpy(), duration=dur)
    ref = oracle.hifigan(h, oracle.Weights(vsd), o.mel)
    assert wav.shape == ref.shape == (B, o.mel.shape[1] * 256)
    assert np.array_equal(mel_len.cpu().numpy(), o.mel_len)
    assert np.abs(wav.cpu().numpy() - ref).max() < 2e-4


@pytest.mark.parametrize("config,B,L", [("v2", 16, 768), ("v1", 2, 300), ("v3", 3, 411), ("v2", 1, 1), ("v2", 3, 7), ("v2", 1, 2500)])
def test_hifigan_one_launch_resblocks_match_conv_by_conv(config, B, L):
    """The one-launch ResBlock kernel (csrc/hifigan_resblock.h: windows with halos, several per utterance at these lengths,
    ragged last window) against the conv-by-conv chain of the same library -- two independent HIP paths, at the size the
    bench's vocoder leg runs (v2) and through the channel counts that have / have no fused instantiation (v1, v3)."""
    from efficientspeech_amd.hifigan import HIFIGAN_CONFIGS, Generator, synth_hifigan_state_dict
    h = HIFIGAN_CONFIGS[config]
    voc = Generator(h)
    voc.load_state_dict({k: torch.from_numpy(v) for k, v in synth_hifigan_state_dict(h, 1234).items()}, strict=True)
    voc = voc.to(DEV).eval()
    g = torch.Generator(device=DEV).manual_seed(5)
    mel = torch.randn((B, L, h.num_mels), device=DEV, generator=g) * 2 - 4
    outs = []
    for fused in (True, False):
        voc.fuse_resblocks = fused
        voc._cache.invalidate()
        with torch.no_grad():
            outs.append(voc(mel.transpose(1, 2)))
    assert outs[0].shape == (B, 1, L * h.hop) and bool(torch.isfinite(outs[0]).all())
    assert float((outs[0] - outs[1]).abs().max()) < 2e-5
    assert float(outs[0].abs().max()) > 1e-3      # a real signal, not zeros


def test_hip_forward_matches_stock_pytorch_ops_on_the_gpu():
    """The HIP path against the same forward written with stock PyTorch-ROCm operators (tests/torch_mirror.py, what bench.py
    reports as `pytorch_rocm_ops`) on the same device: a second, independent implementation next to the C oracle."""
    from tests import torch_mirror as M
    net, cfg, sd = H.make_net("tiny", DEV)
    ids, mask = synth_phonemes(16, 128, 1234)
    x = {"phoneme": torch.from_numpy(ids).to(DEV), "phoneme_mask": torch.from_numpy(mask).to(DEV),
         "duration_forced": torch.full((16, 128), 6, dtype=torch.int32, device=DEV)}
    with torch.no_grad():
        mel, mel_len, _ = net(x)
        ref, ref_len, _ = M.eval_forward(net, x)
    assert torch.equal(mel_len.long().cpu(), ref_len.long().cpu())
    per_utt = (mel - ref).abs().amax(dim=(1, 2))
    assert int((per_utt > 1e-4).sum()) <= 1          # (a pitch / energy prediction on a bucket edge may flip one utterance's embedding)
    assert float(per_utt.median()) < 2e-5


@pytest.mark.parametrize("name", ["tiny", "base"])
def test_lds_staged_attention_at_size(name):
    """>= 128 (utterance, head) pairs so that the GPU dispatch takes attn_lds_kernel: 3, 4, 7 and 8 key tiles, widths 32 .. 256."""
    net, cfg, sd = H.make_net(name, DEV)
    H.check_attention_sizes(net, cfg, sd, DEV, sizes=((128, 96), (64, 128), (40, 200), (32, 256)) if name == "tiny" else ((32, 100), (16, 250)))


def test_lds_gemm_edge_shapes():
    """>= 2048 rows each (the launcher's threshold for the LDS-staged kernel)."""
    H.check_lds_gemm_edges(DEV, [(2048, 1, 128, 1), (1100, 2, 128, 2), (700, 3, 160, 1), (300, 7, 128, 2), (63, 33, 256, 1),
                                 (33, 64, 96, 2), (9, 255, 160, 2), (5, 513, 128, 1), (4100, 1, 96, 1), (17, 129, 224, 1)])

