"""Inference at bf16: precision = ESMI_PRECISION_BF16 in esmi_mel_decoder_prec_f32, esmi_phoneme2mel_forward_prec_f32 / _curve_f32 and
esmi_hifigan_generator_prec_f32; `precision="bf16"` ("bf16-mixed") in MelDecoder, Generator / get_hifigan, the inference key
x["decoder_precision"], EfficientSpeech.synthesize, BucketedSynthesizer, the staged forward and the graph-replay path.  The checks and the
fp64 yardsticks live in tests/inference_bf16_checks.py; the GPU tier runs them on the device, the CPU tier through the wave simulator (the
same kernel sources compiled for the host).  `-s` prints every measured ratio (profiles/r15_inference_bf16.md records them).
"""
import os
import re
import shutil
import subprocess
import sys

import pytest

from tests import inference_bf16_checks as V
from tests.simlib import use_sim

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "efficientspeech_amd", "libesmi.so")
TOOLS = ["/opt/rocm/lib/llvm/bin/clang-offload-bundler", "/opt/rocm/lib/llvm/bin/llvm-readelf"]
# the precision-16 decoder suite's direct-mode shapes: base ES; one k = 3 decoder per dx2; tiny with row outliers
DIRECT = [("base", 2, 131, None), ("tiny_k3", 1, 140, None), ("small_k3", 1, 140, None), ("tiny", 2, 40, "row_outliers")]


@pytest.fixture(scope="module")
def dec_yard():
    y = V.DecYard()
    yield y
    y.clear()


@pytest.fixture(scope="module")
def voc_yard():
    y = V.VocYard()
    yield y
    y.clear()


# ---------------------------------------------------------------------------------------------------------------- test 0 (CPU, no kernels)
@pytest.mark.parametrize("name", ["tiny", "small", "tiny_k3"])
def test_decoder_mirror_matches_the_oracle(name):
    V.check_dec_mirror_matches_oracle(name)


@pytest.mark.parametrize("config", ["v1", "v2", "v3"])
def test_vocoder_mirror_matches_the_reference_fixtures(config, voc_yard):
    V.check_voc_mirror_matches_fixture(voc_yard, config)


def test_the_two_weight_rules_differ_by_one_ulp_on_few_weights():
    V.check_rules_agree_almost_everywhere()


# ---------------------------------------------------------------------------------------------------------------- GPU tier
@pytest.mark.gpu
def test_bf16_forward_with_h0_error_and_invariants(dec_yard):
    """Tests 1 and 3, tiny ES, the whole forward, free-running ragged B = 3, L ~ 150 (two windows, edge rows, padding frames)."""
    V.check_forward_with_h0(dec_yard, DEV)


@pytest.mark.gpu
def test_bf16_chunk_walk_and_window_form(dec_yard, monkeypatch):
    """Test 1, small ES: whole-utterance walks (several chunks per segment, carried rows, block skew) against the window form."""
    monkeypatch.setenv("ESMI_DEC_STREAM_WGS", "1")
    V.check_chunk_walk(dec_yard, "small", 2, 60, 9, DEV)


@pytest.mark.gpu
@pytest.mark.parametrize("name,B,L,profile", DIRECT)
def test_bf16_direct_mode_error(name, B, L, profile, dec_yard):
    V.check_direct(dec_yard, name, B, L, DEV, profile)


@pytest.mark.gpu
def test_bf16_beyond_the_binary16_range(dec_yard):
    """Test 2"""
    V.check_beyond_binary16(dec_yard, DEV)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["tiny", "small"])
def test_decoder_precisions_through_the_prec_entry_point(name):
    """Test 3"""
    V.check_entry_points(name, DEV)


@pytest.mark.gpu
def test_range_checked_build_runs_bf16():
    V.check_range_check_runs_bf16(DEV)


@pytest.mark.gpu
@pytest.mark.parametrize("fused", [True, False], ids=["fused", "convs"])
@pytest.mark.parametrize("config", ["v1", "v2", "v3"])
def test_bf16_vocoder_error_is_the_bfloat16_operand_error(config, fused, voc_yard):
    """Test 4 on the three fixture shapes (the precision-16 vocoder suite's)"""
    V.check_voc_accuracy(voc_yard, config, DEV, fused)


@pytest.mark.gpu
def test_bf16_vocoder_two_resblock_windows(voc_yard):
    """Test 4, v2 at B = 1, L = 50: two windows per utterance in the first stage's k = 11 block"""
    V.check_voc_accuracy(voc_yard, "v2", DEV, True, 1, 50)


@pytest.mark.gpu
def test_bf16_vocoder_ragged_keeps_its_contract():
    """Test 5: v2, B = 3, L = 64, lengths [64, 33, 9], one launch per ResBlock and conv by conv"""
    V.check_voc_ragged_contract("v2", 3, 64, [64, 33, 9], DEV)


@pytest.mark.gpu
def test_vocoder_precision_0_and_32_are_the_existing_entry_points():
    V.check_voc_default_untouched("v2", 2, 24, [24, 5], DEV)


@pytest.mark.gpu
def test_bf16_through_synthesize():
    V.check_synthesize(DEV)


@pytest.mark.gpu
def test_bf16_through_the_scheduler():
    V.check_scheduler(DEV)


@pytest.mark.gpu
def test_bf16_through_the_staged_forward_and_the_pipeline():
    V.check_staged_forward(DEV)


@pytest.mark.gpu
def test_bf16_graph_replay_captures_or_refuses():
    V.check_graph_replay(DEV)


@pytest.mark.gpu
def test_python_refusals_on_the_device():
    V.check_python_refusals(DEV)


@pytest.mark.gpu
def test_precision16_keeps_the_parent_commits_bits_on_the_device():
    """Test 3: the committed outputs of the previous commit's libesmi.so"""
    V.check_precision16_keeps_the_parents_bits(DEV, "gpu")


# ---------------------------------------------------------------------------------------------------------------- CPU tier (simulator)
def test_simulated_precision16_keeps_the_parent_commits_bits():
    """Test 3: the committed outputs of the previous commit's simulator build"""
    with use_sim():
        V.check_precision16_keeps_the_parents_bits("cpu", "sim")


def test_fused_kernels_weight_rule_bit_for_bit(tmp_path):
    V.check_plane_rule_bit_for_bit(tmp_path)


def test_simulated_bf16_through_synthesize():
    """Test 6 on the simulator, with the smallest 80-mel generator behind tiny ES (v2 takes a minute there)"""
    with use_sim():
        V.check_synthesize("cpu", small=True)


def test_simulated_bf16_forward_with_h0_error_and_invariants(dec_yard):
    with use_sim():
        V.check_forward_with_h0(dec_yard, "cpu")


def test_simulated_bf16_chunk_walk_and_window_form(dec_yard, monkeypatch):
    monkeypatch.setenv("ESMI_DEC_STREAM_WGS", "1")
    with use_sim():
        V.check_chunk_walk(dec_yard, "small", 2, 60, 9, "cpu")


@pytest.mark.parametrize("name,B,L,profile", DIRECT)
def test_simulated_bf16_direct_mode_error(name, B, L, profile, dec_yard):
    with use_sim():
        V.check_direct(dec_yard, name, B, L, "cpu", profile)


def test_simulated_bf16_beyond_the_binary16_range(dec_yard):
    with use_sim():
        V.check_beyond_binary16(dec_yard, "cpu")


@pytest.mark.parametrize("name", ["tiny", "small"])
def test_simulated_decoder_precisions_through_the_prec_entry_point(name):
    with use_sim():
        V.check_entry_points(name, "cpu")


def test_simulated_range_checked_build_runs_bf16():
    with use_sim():
        V.check_range_check_runs_bf16("cpu")


def test_simulated_bf16_vocoder_accuracy_v2_two_windows(voc_yard):
    """Test 4, v2 with one launch per ResBlock at B = 1, L = 50 (all twelve (C, K) bf16 ResBlock1 instantiations; two windows in the
    first stage's k = 11 block)"""
    with use_sim():
        V.check_voc_accuracy(voc_yard, "v2", "cpu", True, 1, 50)


@pytest.mark.parametrize("name", ["reduced1", "reduced2"])
def test_simulated_bf16_vocoder_accuracy_reduced_generator_conv_by_conv(name, voc_yard):
    """Test 4, the reduced generators one launch per convolution, B = 2, L = 6"""
    with use_sim():
        V.check_voc_accuracy(voc_yard, name, "cpu", False, 2, 6)


def test_simulated_bf16_vocoder_accuracy_reduced_generator_fused(voc_yard):
    with use_sim():
        V.check_voc_accuracy(voc_yard, "reduced2", "cpu", True, 2, 6)


def test_simulated_bf16_vocoder_ragged_keeps_its_contract():
    """Test 5 on the reduced generator, B = 3, lengths [6, 2, 0], both modes"""
    with use_sim():
        V.check_voc_ragged_contract("reduced1", 3, 6, [6, 2, 0], "cpu", module=False)


def test_simulated_vocoder_precision_0_and_32_are_the_existing_entry_points():
    with use_sim():
        V.check_voc_default_untouched("small", 2, 6, [6, 2], "cpu")


def test_simulated_bf16_through_the_scheduler():
    with use_sim():
        V.check_scheduler("cpu")


def test_simulated_bf16_through_the_staged_forward_and_the_pipeline():
    with use_sim():
        V.check_staged_forward("cpu")


def test_simulated_python_refusals():
    with use_sim():
        V.check_python_refusals("cpu")


def test_c_refusals_launch_nothing():
    with use_sim():
        V.check_c_refusals()


def test_get_hifigan_takes_the_precision(tmp_path):
    V.check_get_hifigan(tmp_path)


def test_exact_fp32_build_refuses_bf16():
    import __graft_entry__ as g
    g.build()
    V.check_fp32mfma_refuses(os.path.join(os.path.dirname(g.LIB), "libesmi_fp32mfma.so"))


def test_graph_replay_refuses_an_invalid_key_before_capturing():
    import torch
    from efficientspeech_amd.sharded import ShardedMelPipeline
    from tests import decoder_precision16_checks as D
    pipe = ShardedMelPipeline(D.make_net("tiny", "cpu")[0], use_graph=True)
    for bad in (8, True, "fp8"):
        with pytest.raises(ValueError, match="precision"):
            pipe.step({"phoneme": torch.ones((1, 4), dtype=torch.int32), "max_mel_len": 16, "decoder_precision": bad})
    assert pipe.graphed is None


# ---------------------------------------------------------------------------------------------------------------- test 7 (simulator's launch log)
@pytest.mark.parametrize("name", ["tiny", "small"])
def test_bf16_forward_launches_differ_in_the_decoder_name_only(name):
    with use_sim():
        V.check_decoder_dispatch(name)


@pytest.mark.parametrize("name,fused,ragged", [("reduced1", True, False), ("reduced1", True, True), ("reduced1", False, True),
                                               ("reduced2", True, True), ("small", True, True)])
def test_bf16_vocoder_launches_are_the_precision16_launches_renamed(name, fused, ragged):
    V.check_vocoder_dispatch(name, fused, ragged)


# ---------------------------------------------------------------------------------------------------------------- test 8 (CPU, the built library)
@pytest.mark.skipif(not os.path.exists(LIB) or not all(os.path.exists(t) for t in TOOLS) or shutil.which("objcopy") is None,
                    reason="needs the built libesmi.so and the ROCm LLVM tools")
def test_bf16_kernels_have_no_scratch():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), LIB, "--all"], capture_output=True, text=True, check=True).stdout
    rows = {m.group(1): int(m.group(2)) for m in re.finditer(r"^\| `(.+?)` \| [^|]+ \| (\d+) \|", out, re.M)}
    dec = {k: v for k, v in rows.items() if k.startswith("mel_decoder_bf16_kernel<")}
    rb = {k: v for k, v in rows.items() if re.search(r"^hifigan_resblock(16)?_bf16_kernel<", k)}
    assert sorted(dec) == [f"mel_decoder_bf16_kernel<{d}, {k}, 8>" for d in (128, 256) for k in (3, 5)], sorted(dec)
    assert len(rb) == 12, sorted(rb)
    assert all(v == 0 for v in {**dec, **rb}.values()), {k: v for k, v in {**dec, **rb}.items() if v}
    assert sum(k.startswith("convgemm_bf16_len_kernel<") for k in rows) == 2
    # the existing decoder kernels keep their names (pinned by the launch-log tests) and stay without scratch
    old = {k: v for k, v in rows.items() if k.startswith("mel_decoder_kernel<")}
    assert len(old) == 8 and all(v == 0 for v in old.values()), old
