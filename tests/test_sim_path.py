"""CPU coverage of the HIP kernels' logic: the unmodified kernel sources compiled for the lane-level
wave simulator (tools/wavesim) are driven through the same C-ABI and the same host-side modules,
and compared with the golden vectors and the oracle.  This does NOT replace the GPU parity tests
(tests/test_gpu_parity.py) -- it lets index math, MFMA fragment layouts, LDS protocols and the host
logic be checked in the GPU-less build container.
"""
import glob
import os

import numpy as np
import pytest
import torch

from efficientspeech_amd import _lib
from efficientspeech_amd.synth import synth_phonemes
from oracle import oracle
from tests import helpers as H
from tests.simlib import launched_kernels, use_sim

GOLD = os.path.join(os.path.dirname(__file__), "golden")
# all tiny fixtures + a padded / teacher-forced one for the wider models (keeps the CPU suite short)
CASES = sorted(p for p in glob.glob(os.path.join(GOLD, "tiny_*.npz")) if "_train_step" not in os.path.basename(p)) + \
    [os.path.join(GOLD, f) for f in ("small_eval_pad_t17.npz", "small_train_tf_padtail.npz",
                                     "base_eval_pad_t17.npz", "base_eval_b1_fox.npz")]


@pytest.fixture(scope="module")
def nets():
    cache = {}

    def get(name, g=None):
        if name not in cache:
            cache[name] = H.make_net(name, "cpu", golden=g)
        return cache[name]
    return get


@pytest.mark.parametrize("path", CASES, ids=[os.path.basename(p)[:-4] for p in CASES])
def test_simulated_kernels_match_golden(path, nets):
    g = np.load(path)
    net, cfg, sd = nets(os.path.basename(path).split("_")[0], g)
    with use_sim():
        H.check_against_golden(net, g, "cpu")


UNFUSED = [os.path.join(GOLD, f) for f in ("tiny_eval_pad_t17.npz", "tiny_train_tf_t17.npz", "tiny_eval_b1_fox.npz",
                                           "small_eval_pad_t17.npz")]


@pytest.mark.parametrize("path", UNFUSED, ids=[os.path.basename(p)[:-4] for p in UNFUSED])
def test_simulated_unfused_path_matches_golden(path, nets):
    """launch plan 0: one kernel per reference op (the fallback for shapes the chain kernels do not cover)."""
    g = np.load(path)
    net, cfg, sd = nets(os.path.basename(path).split("_")[0], g)
    with use_sim(), _lib.launch_plan(0):
        H.check_against_golden(net, g, "cpu")


@pytest.mark.parametrize("name,B,T,lens,seed", [
    ("tiny", 3, 70, [70, 41, 9], 4321),        # 3 row tiles; 70 / 35 keys; multi-window decoder (L > 112)
    ("small", 2, 40, [40, 23], 4321),
    ("small", 2, 150, [150, 97], 4321),        # round 6: enc_va64_kernel<2> (two 16-row tiles per wave, head inside) + enc_post_attn64_kernel<2>
    ("base", 2, 150, [150, 97], 77),           # round 6: enc_pred128_kernel, five waves x two tiles, the last tile partly / wholly outside
])
def test_simulated_eval_vs_oracle_multi_tile(name, B, T, lens, seed, nets):
    kernels = {("small", 150): {"enc_va64_kernel<2>", "enc_post_attn64_kernel<2>"}, ("base", 150): {"enc_pred128_kernel"}}.get((name, T), set())
    net, cfg, sd = nets(name)
    ids, mask = synth_phonemes(B, T, seed, lens)
    x = {"phoneme": torch.from_numpy(ids), "phoneme_mask": torch.from_numpy(mask)}
    with use_sim(), torch.no_grad(), launched_kernels() as launched:
        enc = net.encoder._encode(x)
        mel, mel_len, _ = net(x)
    assert kernels <= set(launched)
    o = oracle.phoneme2mel(cfg, oracle.Weights(sd), ids, mask)
    err = H.compare_eval_with_oracle(cfg, o, enc, mel, mel_len, sd)
    assert err == err
    assert int(mel_len.max()) > 128 - 2 * cfg.halo or name != "tiny"   # really multi-window for tiny


def test_simulated_forced_durations_and_hint(nets):
    """`duration_forced` + `max_mel_len` (bench path): padded length larger than every utterance."""
    net, cfg, sd = nets("tiny")
    B, T = 2, 24
    ids, mask = synth_phonemes(B, T, 9, [24, 15])
    dur = np.full((B, T), 6, np.int32)
    x = {"phoneme": torch.from_numpy(ids), "phoneme_mask": torch.from_numpy(mask),
         "duration_forced": torch.from_numpy(dur), "max_mel_len": 150}
    with use_sim(), torch.no_grad():
        enc = net.encoder._encode(x)
        mel, mel_len, _ = net(x)
    assert mel.shape == (B, 150, 80)
    # the reference semantics for a hint larger than the batch max: L = true batch max (144), rows beyond are 0
    o = oracle.phoneme2mel(cfg, oracle.Weights(sd), ids, mask, pitch=enc["pitch"][..., 0].numpy(),
                           energy=enc["energy"][..., 0].numpy(), duration=dur)
    assert np.array_equal(mel_len.numpy(), o.mel_len) and o.mel.shape[1] == 144
    assert np.abs(mel[:, :144].numpy() - o.mel).max() < H.MEL_TOL
    assert not mel[:, 144:].any()


def test_simulated_module_level_apis(nets):
    """Encoder / Fuse / MelDecoder / FeatureUpsampler / PhonemeEncoder called stand-alone like the reference's."""
    net, cfg, sd = nets("tiny")
    w = oracle.Weights(sd)
    ids, mask = synth_phonemes(2, 19, 3, [19, 12])
    o = oracle.phoneme2mel(cfg, w, ids, mask, taps=True)
    with use_sim(), torch.no_grad():
        feats, dmask = net.encoder.encoder(torch.from_numpy(ids), mask=torch.from_numpy(mask))
        fused = net.encoder.fuse(feats, mask=dmask)
        mel = net.decoder(torch.from_numpy(o.features))
        pe = net.encoder({"phoneme": torch.from_numpy(ids), "phoneme_mask": torch.from_numpy(mask)})
        f, m, ml = net.encoder.feature_upsampler(torch.from_numpy(o.feat),
                                                 torch.from_numpy(np.repeat(mask[:, :, None], cfg.d4, 2)),
                                                 torch.from_numpy(o.dur))
    for a, b in zip(feats, o.f_taps):
        np.testing.assert_allclose(a.numpy(), b, atol=H.PRED_TOL, rtol=0)
    assert dmask.shape == (2, 19, cfg.dim) and np.array_equal(dmask[:, :, 0].numpy(), mask)
    np.testing.assert_allclose(fused.numpy(), o.fused, atol=H.PRED_TOL, rtol=0)
    raw = oracle.mel_decoder(cfg, w, o.features)               # decoder alone: no final masked_fill
    assert np.abs(mel.numpy() - raw).max() < H.MEL_TOL
    assert set(pe) == {"pitch", "energy", "duration", "mel_len", "features", "masks"}
    np.testing.assert_allclose(pe["features"].numpy(), o.features, atol=H.PRED_TOL, rtol=0)
    assert pe["masks"].dtype == torch.bool and pe["masks"].shape == pe["features"].shape
    assert np.array_equal(pe["masks"][:, :, 0].numpy(), o.masks)
    assert np.array_equal(f.numpy(), o.features) and np.array_equal(m[:, :, 0].numpy(), o.masks)
    assert np.array_equal(ml.numpy(), o.mel_len)


def test_simulated_length_regulator_bit_exact():
    from efficientspeech_amd import _lib  # noqa: F401
    rng = np.random.default_rng(11)
    with use_sim() as lib:
        for B, T in ((5, 70), (2, 129), (1, 1)):
            dur = rng.integers(-2, 9, size=(B, T)).astype(np.int32)
            dur[rng.random((B, T)) < 0.25] = 0
            d = torch.from_numpy(dur)
            cum = torch.empty((B, T), dtype=torch.int32)
            mel_len = torch.empty((B,), dtype=torch.int32)
            lmax = torch.empty((1,), dtype=torch.int32)
            lib.esmi_length_regulate_i32(d.data_ptr(), B, T, cum.data_ptr(), mel_len.data_ptr(), lmax.data_ptr(), None)
            ref = np.cumsum(np.maximum(dur, 0), 1).astype(np.int32)
            assert np.array_equal(cum.numpy(), ref) and int(lmax) == ref[:, -1].max()
            L = max(int(lmax) + 3, 1)
            idx = torch.empty((B, L), dtype=torch.int32)
            lib.esmi_length_regulator_indices_i32(cum.data_ptr(), B, T, L, idx.data_ptr(), None)
            assert np.array_equal(idx.numpy(), oracle.length_regulate(dur, L))


def test_simulated_errors(nets):
    net, cfg, _ = nets("tiny")
    with use_sim():
        with pytest.raises(KeyError):                            # B>1 without phoneme_mask (networks.py:338)
            net({"phoneme": torch.ones((2, 8), dtype=torch.int32)})


@pytest.mark.parametrize("B,T,lens", [(3, 64, [64, 50, 7]), (2, 96, [96, 40]), (1, 32, None), (2, 128, [128, 77]), (3, 40, [40, 33, 9]), (1, 31, None),
                                      (2, 17, [17, 5]), (1, 1, None)])
def test_simulated_one_launch_encoder_side(B, T, lens, nets):
    """Round 5: for T <= 128 the one-call forward runs the whole encoder side of tiny ES as ONE launch (enc_all16_kernel: the three
    chain16 bodies behind each other on one wave count -- surplus waves of a body see rows outside the sequence; key tiles beyond a short sequence
    read zeroed planes).  Against the oracle, and against the round-1..4
    chain kernels (launch plan 31) and the three chain16 launches of the module path."""
    net, cfg, sd = nets("tiny")
    ids, mask = synth_phonemes(B, T, 5, lens)
    x = {"phoneme": torch.from_numpy(ids)}
    if B > 1:
        x["phoneme_mask"] = torch.from_numpy(mask)
    with use_sim(), torch.no_grad():
        with launched_kernels() as one_call:
            mel, mel_len, dur = net(x)                                # one-call forward: enc_all16_kernel
        with launched_kernels() as module:
            enc = net.encoder._encode(x)                              # module path: three chain16 launches
        with _lib.launch_plan(31):
            mel31, _, dur31 = net(x)
    o = oracle.phoneme2mel(cfg, oracle.Weights(sd), ids, mask if B > 1 else None)
    err = H.compare_eval_with_oracle(cfg, o, enc, mel, mel_len, sd)
    assert err == err
    np.testing.assert_allclose(dur.numpy(), o.duration, atol=H.PRED_TOL, rtol=0)
    assert float((mel - mel31).abs().max()) < 2e-5 and float((dur - dur31).abs().max()) < 2e-5
    assert [k.split("<")[0] for k in one_call if k.startswith("enc_")] == ["enc_all16_kernel"]
    assert [k.split("<")[0] for k in module if k.startswith("enc_")] == ["enc_b0_16_kernel", "enc_b1_16_kernel", "enc_va16_kernel"]


@pytest.mark.parametrize("fusion", [7, 31 - 8, 31], ids=["staged", "no-split", "chain32"])
def test_simulated_intermediate_plans(fusion, nets):
    """Fusion masks between 'everything fused' and 'one kernel per op': per-stage chain kernels (7), whole-block
    without the column-split variant (23), the round-1..4 chain kernels on the shapes the chain16 kernels took over in round 5 (31)."""
    g = np.load(os.path.join(GOLD, "tiny_eval_pad_t17.npz"))
    net, cfg, sd = nets("tiny", g)
    with use_sim(), _lib.launch_plan(fusion):
        H.check_against_golden(net, g, "cpu")


def test_simulated_long_sequence_halo_paths(nets):
    """T = 150 > 128: every cooperative chain kernel needs several workgroups per utterance, i.e. the halo-recompute
    branches of enc_attn_ffn_split (block 1, N = 75 > 64) and enc_fuse_va (halo 2).  (Block 0, N = 150, is past
    enc_attn_ffn_supported's N <= 128 gate: attention + GEMM launches.)"""
    net, cfg, sd = nets("tiny")
    B, T = 2, 150
    ids, mask = synth_phonemes(B, T, 77, [150, 97])
    dur = np.ones((B, T), np.int32)
    dur[:, ::7] = 2
    x = {"phoneme": torch.from_numpy(ids), "phoneme_mask": torch.from_numpy(mask), "duration_forced": torch.from_numpy(dur)}
    with use_sim(), torch.no_grad(), launched_kernels() as launched:
        enc = net.encoder._encode(x)
        mel, mel_len, _ = net(x)
    assert {"enc_attn_ffn_split_kernel<4,2,1>", "enc_fuse_va_kernel<1,3>"} <= set(launched)
    o = oracle.phoneme2mel(cfg, oracle.Weights(sd), ids, mask, duration=dur, taps=True)
    np.testing.assert_allclose(enc["duration"].numpy(), o.duration, atol=H.PRED_TOL, rtol=0)
    np.testing.assert_allclose(enc["pitch"].numpy(), o.pitch, atol=H.PRED_TOL, rtol=0)
    np.testing.assert_allclose(enc["feat"].numpy()[..., :cfg.dim], o.fused, atol=H.PRED_TOL, rtol=0)
    if np.array_equal(enc["pitch_idx"].numpy(), o.pitch_idx) and np.array_equal(enc["energy_idx"].numpy(), o.energy_idx):
        assert np.array_equal(mel_len.numpy(), o.mel_len)
        assert np.abs(mel.numpy() - o.mel).max() < H.MEL_TOL


def test_simulated_weight_packers():
    """esmi_pack_bfrag_f32 / esmi_compose_merge_f32 against their definitions in include/esmi.h."""
    rng = np.random.default_rng(5)
    with use_sim() as lib:
        for taps, n, k in ((1, 96, 32), (3, 40, 64), (5, 32, 128)):
            w = rng.standard_normal((taps, n, k)).astype(np.float32)
            nt = (n + 31) // 32
            assert lib.esmi_pack_bfrag_floats(n, k, taps) == taps * k * 32 * nt
            dst = torch.empty(taps * k * 32 * nt, dtype=torch.float32)
            lib.esmi_pack_bfrag_f32(torch.from_numpy(w).data_ptr(), dst.data_ptr(), n, k, taps, None)
            d = dst.numpy().reshape(taps, k // 8, nt, 64, 4)
            t, kc, t32, lane, s = np.meshgrid(np.arange(taps), np.arange(k // 8), np.arange(nt), np.arange(64), np.arange(4),
                                              indexing="ij")
            row = 32 * t32 + (lane & 31)
            if "enc_gemm=split-f16x2" in lib.esmi_build_config().decode():
                # split operands: slot kc & 3 of a 32-channel group = (16-channel step, piece); dword s = two binary16 values
                st, pl = (kc >> 1) & 1, kc & 1
                ch0 = 32 * (kc >> 2) + 16 * st + 4 * (lane >> 5) + np.where(s < 2, 2 * s, 8 + 2 * (s - 2))
                word = np.zeros(d.shape, np.uint32)
                for j in range(2):
                    x = np.where(row < n, w[t, np.minimum(row, n - 1), ch0 + j], 0.0).astype(np.float32) * np.float32(256.0)
                    h1 = x.astype(np.float16)
                    piece = np.where(pl == 0, h1, (x - h1.astype(np.float32)).astype(np.float16)).astype(np.float16)
                    word |= piece.view(np.uint16).astype(np.uint32) << np.uint32(16 * j)
                assert np.array_equal(d.view(np.uint32), word)
            else:
                col = 8 * kc + 4 * (lane >> 5) + s
                ref = np.where(row < n, w[t, np.minimum(row, n - 1), col], 0.0)
                assert np.array_equal(d, ref.astype(np.float32))
        k, cin, cout = 3, 64, 32
        wm = rng.standard_normal((k, cin, cin)).astype(np.float32)
        w1 = rng.standard_normal((cout, cin)).astype(np.float32)
        dst = torch.empty((k, cout, cin), dtype=torch.float32)
        lib.esmi_compose_merge_f32(torch.from_numpy(wm).data_ptr(), torch.from_numpy(w1).data_ptr(), k, cin, cout, dst.data_ptr(), None)
        ref = np.einsum("om,jmi->joi", w1.astype(np.float64), wm.astype(np.float64)).astype(np.float32)
        assert np.array_equal(dst.numpy(), ref)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_simulated_random_shapes(seed, nets):
    """Small seeded random shapes / ragged lengths / forced durations (zeros included) through the simulated default plan."""
    rng = np.random.default_rng(2000 + seed)
    net, cfg, sd = nets("tiny")
    B, T = int(rng.integers(1, 4)), int(rng.integers(1, 60))
    lens = sorted((int(v) for v in rng.integers(1, T + 1, size=B)), reverse=True)
    lens[0] = T
    ids, mask = synth_phonemes(B, T, 70 + seed, lens)
    dur = rng.integers(0, 4, size=(B, T)).astype(np.int32)
    x = {"phoneme": torch.from_numpy(ids), "duration_forced": torch.from_numpy(dur)}
    if B > 1:
        x["phoneme_mask"] = torch.from_numpy(mask)
    with use_sim(), torch.no_grad():
        enc = net.encoder._encode(x)
        mel, mel_len, _ = net(x)
    o = oracle.phoneme2mel(cfg, oracle.Weights(sd), ids, mask if B > 1 else None, pitch=enc["pitch"][..., 0].numpy(),
                           energy=enc["energy"][..., 0].numpy(), duration=dur)
    assert np.array_equal(mel_len.numpy(), o.mel_len) and mel.shape == o.mel.shape
    if o.mel.size:
        assert np.abs(mel.numpy() - o.mel).max() < H.MEL_TOL


@pytest.mark.parametrize("name", ["tiny", "base"])
def test_simulated_submodule_forwards(name, nets):
    """SelfAttention / MixFFN / AcousticDecoder called on their own (the reference's module-level API)."""
    net, cfg, sd = nets(name)
    with use_sim():
        H.check_submodule_forwards(net, cfg, sd, "cpu")


@pytest.mark.parametrize("name", ["small", "base"])
def test_simulated_decoder_head_at_phoneme_rate(name, nets):
    net, cfg, sd = nets(name)
    with use_sim():
        H.check_decoder_head(net, cfg, "cpu")


def test_simulated_embedding_folded_into_merge_conv(nets):
    with use_sim():
        net, cfg, sd = nets("tiny")
        H.check_embedding_folded_into_merge_conv(net, cfg, "cpu")


@pytest.mark.parametrize("name", ["tiny", "base"])
def test_simulated_ffn_linear_folded_into_conv(name, nets):
    with use_sim():
        net, cfg, sd = nets(name)
        H.check_ffn_linear_folded_into_conv(net, cfg, "cpu")


def test_simulated_decoder_chunk_walk_equals_windows(nets):
    net, cfg, sd = nets("small")
    with use_sim():
        H.check_decoder_chunk_walk(net, cfg, "cpu", cases=((2, 40, 9),))


@pytest.mark.parametrize("name,B,T,D", [("small", 2, 60, 9), ("base", 1, 70, 9)])
def test_simulated_decoder_whole_utterance_walk_with_block_skew(name, B, T, D, nets, monkeypatch):
    """The dx2 = 256 chunk walk with carried rows AND the block skew over several chunks of one segment (ESMI_DEC_STREAM_WGS=1: whole-
    utterance walks at any batch size; on the GPU that is the B >= 256 geometry): conv-layer carries in LDS, block carries through the
    workspace, shifted block-end LayerNorm, skip rows re-read -- against the window form of the same kernel."""
    monkeypatch.setenv("ESMI_DEC_STREAM_WGS", "1")
    net, cfg, sd = nets(name)
    with use_sim():
        H.check_decoder_chunk_walk(net, cfg, "cpu", cases=((B, T, D),))


def test_simulated_split_range_guard(nets):
    """A weight outside the split-f16 operand range is refused at pack time (ValueError naming the fp32 build), not
    silently turned into inf."""
    from efficientspeech_amd import CONFIGS, build_phoneme2mel, load_numpy_state_dict
    from efficientspeech_amd.synth import synth_state_dict
    cfg = CONFIGS["tiny"]
    for key in ("encoder.encoder.attn_blocks.0.2.qkv.weight", "decoder.blocks.1.0.0.0.1.weight", "encoder.fuse.fuse.weight",
                "encoder.pitch_decoder.conv2.0.weight"):
        sd = synth_state_dict(cfg, 5)
        sd[key] = sd[key].copy()
        sd[key].flat[7] = 300.0
        net = build_phoneme2mel(cfg)
        load_numpy_state_dict(net, sd)
        ids, mask = synth_phonemes(2, 9, 1, [9, 4])
        with use_sim(), torch.no_grad():
            with pytest.raises(ValueError, match="libesmi_fp32mfma"):
                net({"phoneme": torch.from_numpy(ids), "phoneme_mask": torch.from_numpy(mask)})


def test_simulated_long_sequence_beyond_256_keys(nets):
    """T = 270: block 0 attends over 270 keys -> the key-chunked attention kernel of the per-op plan."""
    net, cfg, sd = nets("tiny")
    B, T = 1, 270
    ids, _ = synth_phonemes(B, T, 78)
    dur = np.ones((B, T), np.int32)
    dur[:, ::5] = 0
    x = {"phoneme": torch.from_numpy(ids), "duration_forced": torch.from_numpy(dur)}
    with use_sim(), torch.no_grad():
        enc = net.encoder._encode(x)
        mel, mel_len, _ = net(x)
    o = oracle.phoneme2mel(cfg, oracle.Weights(sd), ids, None, pitch=enc["pitch"][..., 0].numpy(),
                           energy=enc["energy"][..., 0].numpy(), duration=dur)
    np.testing.assert_allclose(enc["pitch"].numpy(), o.pitch, atol=H.PRED_TOL, rtol=0)
    assert np.array_equal(mel_len.numpy(), o.mel_len)
    assert np.abs(mel.numpy() - o.mel).max() < H.MEL_TOL


def test_simulated_model_wrapper_and_bucket_scheduler():
    with use_sim():
        H.check_wrapper_and_scheduler("cpu")


@pytest.mark.parametrize("fixture", ["hifigan_v2_b2_l24.npz", "hifigan_v3_b1_l17.npz"])
def test_simulated_hifigan_generator_matches_reference(fixture):
    """HiFi-GAN generator: ResBlock1 (v2) and ResBlock2 (v3) chains through esmi_hifigan_generator_f32."""
    with use_sim():
        H.check_hifigan_golden(os.path.join(GOLD, fixture), "cpu")


def test_simulated_lds_staged_attention():
    """attn_lds_kernel<4> / <8> (K and V staged once per head in LDS) through SelfAttention.forward, tiny ES widths 32 / 64."""
    with use_sim():
        net, cfg, sd = H.make_net("tiny", "cpu")
        H.check_attention_sizes(net, cfg, sd, "cpu", sizes=((1, 100), (1, 200)))


def test_simulated_lds_gemm_edge_shapes():
    """(the simulator build sends every row count through the LDS-staged kernel)"""
    with use_sim():
        H.check_lds_gemm_edges("cpu", [(5, 1, 96, 1), (3, 2, 128, 1), (2, 7, 96, 2), (1, 70, 128, 1)])


def check_activation_range_guard(dev):
    """ESMI_ERR_RANGE (include/esmi.h): on the range-checked build a value that enters a split-f16 contraction outside the binary16
    range is reported by esmi_phoneme2mel_forward_f32 -- the product build would saturate it silently.  In-range checkpoints pass
    (and give the product build's output); embedding rows x 1e5 push the first convolution's operands to ~4e5 and are refused."""
    from efficientspeech_amd import _lib
    net, cfg, sd = H.make_net("tiny", dev)
    ids, mask = synth_phonemes(3, 24, 5, [24, 17, 9])
    x = {"phoneme": torch.from_numpy(ids).to(dev), "phoneme_mask": torch.from_numpy(mask).to(dev)}
    with torch.no_grad():
        ref = net(x)[0]
    mel, mel_len, _ = net.check_activation_range(x)
    if "split-f16" in _lib.load().esmi_build_config().decode():
        # same kernels, same operations: the check only observes.  Not bit for bit since the attention operands of the chain kernels
        # go through the split too (round 4): the checks' branches sit between a product and the sum it feeds, and hipcc contracts
        # a*b + c into an fma in one build and not in the other -- block 0's output differs by 4 ulp (4.8e-7), the mel by 2e-6.
        assert float((mel - ref).abs().max()) < 1e-5
    else:                                                          # (ESMI_LIB = the exact-fp32 build: the checked build is the split-f16 one)
        assert float((mel - ref).abs().max()) < 1e-4
    sd2 = {k: v.copy() for k, v in sd.items()}
    sd2["encoder.encoder.embed.weight"] = sd2["encoder.encoder.embed.weight"] * np.float32(1e5)
    bad = H.build_phoneme2mel(cfg)
    H.load_numpy_state_dict(bad, sd2)
    bad = bad.to(dev)
    with pytest.raises(_lib.ActivationRange):
        bad.check_activation_range(x)
    net.check_activation_range(x)                                  # the flag pointer was cleared again: a good network still passes
    # ESMI_DEBUG_RANGE=1: the first forward of a set of weights validates itself, later ones run the product build
    os.environ["ESMI_DEBUG_RANGE"] = "1"
    try:
        with torch.no_grad():
            with pytest.raises(_lib.ActivationRange):
                bad(x)
            first = net(x)[0]
            assert getattr(net, "_range_ok_key", None) is not None
            again = net(x)[0]
        assert float((first - ref).abs().max()) < 1e-4 and torch.equal(again, ref)
    finally:
        del os.environ["ESMI_DEBUG_RANGE"]


def test_simulated_activation_range_guard():
    with use_sim():
        check_activation_range_guard("cpu")


@pytest.mark.gpu
def test_gpu_activation_range_guard():
    check_activation_range_guard("cuda")
    # the product library refuses the request instead of ignoring it
    from efficientspeech_amd import _lib
    net, cfg, sd = H.make_net("tiny", "cuda")
    ids, mask = synth_phonemes(2, 8, 5)
    x = {"phoneme": torch.from_numpy(ids).cuda(), "phoneme_mask": torch.from_numpy(mask).cuda()}
    net._range_flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    try:
        with pytest.raises(_lib.Unsupported):
            net(x)
    finally:
        net._range_flag = None


def test_simulated_tiny_with_expansion_2_takes_the_per_block_path():
    """the one-launch encoder side (enc_all16_kernel) is built for MixFFN expansion 1 only; a depth-2, dim-32
    model with the reference's `--expansion 2` must fall through to the per-block path under the default plan instead of running
    the chain16 bodies on twice-as-wide FFN weights.  Plans 63 (default), 31 and 0 against each other and against the oracle."""
    import dataclasses
    from efficientspeech_amd import CONFIGS, build_phoneme2mel, load_numpy_state_dict
    from efficientspeech_amd.synth import synth_state_dict
    cfg = dataclasses.replace(CONFIGS["tiny"], name="tiny_e2", expansion=2)
    sd = synth_state_dict(cfg, 1234)
    net = build_phoneme2mel(cfg)
    load_numpy_state_dict(net, sd)
    ids, mask = synth_phonemes(2, 40, 11, [40, 23])
    x = {"phoneme": torch.from_numpy(ids), "phoneme_mask": torch.from_numpy(mask)}
    res = {}
    with use_sim(), torch.no_grad():
        for plan in (_lib.FUSE_ALL, 31, 0):
            with _lib.launch_plan(plan), launched_kernels() as launched:
                enc = net.encoder._encode(x)
                mel, mel_len, dpred = net(x)
            assert not any(k.startswith("enc_all16_kernel") for k in launched), f"plan {plan}"
            res[plan] = (mel.numpy().copy(), mel_len.numpy().copy(), dpred.numpy().copy(), enc)
    o = oracle.phoneme2mel(cfg, oracle.Weights(sd), ids, mask)
    for plan, (mel, mel_len, dpred, enc) in res.items():
        np.testing.assert_allclose(dpred, o.duration, atol=H.PRED_TOL, rtol=0, err_msg=f"plan {plan}")
        err = H.compare_eval_with_oracle(cfg, o, enc, torch.from_numpy(mel), torch.from_numpy(mel_len), sd)
        assert err == err, f"plan {plan}: a discrete decision inside its margin; pick another seed"


def test_simulated_dim128_model_with_kernel_3_and_odd_length():
    """enc_fuse128_kernel<3> (the reference's default --kernel-size with base's width) at an odd T spread over three waves: the last
    odd position lies outside the sequence, level-1 rows n - 1 cross two tile boundaries.  Plans 63 (enc_fuse128 + enc_pred128) and
    31 (per-op launches) against the oracle."""
    import dataclasses
    from efficientspeech_amd import CONFIGS, build_phoneme2mel, load_numpy_state_dict
    from efficientspeech_amd.synth import synth_state_dict
    cfg = dataclasses.replace(CONFIGS["base"], name="base_k3", kernel_size=3)
    sd = synth_state_dict(cfg, 1234)
    net = build_phoneme2mel(cfg)
    load_numpy_state_dict(net, sd)
    ids, mask = synth_phonemes(2, 71, 77, [71, 38])
    x = {"phoneme": torch.from_numpy(ids), "phoneme_mask": torch.from_numpy(mask)}
    o = oracle.phoneme2mel(cfg, oracle.Weights(sd), ids, mask)
    with use_sim(), torch.no_grad():
        for plan in (_lib.FUSE_ALL, 31):
            with _lib.launch_plan(plan), launched_kernels() as launched:
                enc = net.encoder._encode(x)
                mel, mel_len, _ = net(x)
            round6 = {"enc_fuse128_kernel<3>", "enc_pred128_kernel"}
            assert round6 <= set(launched) if plan == _lib.FUSE_ALL else not round6 & set(launched), f"plan {plan}"
            err = H.compare_eval_with_oracle(cfg, o, enc, mel, mel_len, sd)
            assert err == err, f"plan {plan}: a discrete decision inside its margin; pick another seed"
