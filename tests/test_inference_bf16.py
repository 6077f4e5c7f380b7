"""Inference at bf16: precision = ESMI_PRECISION_BF16 in esmi_mel_decoder_prec_f32, esmi_phoneme2mel_forward_prec_f32 / _curve_f32 and
esmi_hifigan_generator_prec_f32; `precision="bf16"` ("bf16-mixed") in MelDecoder, Generator / get_hifigan, the inference key
x["decoder_precision"], EfficientSpeech.synthesize, BucketedSynthesizer, the staged forward and the graph-replay path.  The checks, the
operand rule `BF16` and the fp64 yardsticks live in tests/precision_checks.py, which the two precision-16 suites run with their rule.  A
test that takes `device` runs on the wave simulator (the same kernel sources compiled for the host); `on_the_device` makes its GPU-tier
twin.  `-s` prints every measured ratio (profiles/r17_precision_tests.md).
"""
import os
import re
import shutil
import subprocess
import sys

import pytest

from tests import precision_checks as V
from tests.precision_checks import BF16, device, on_the_device, yard   # noqa: F401 (fixtures)
from tests.simlib import use_sim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "efficientspeech_amd", "libesmi.so")
TOOLS = ["/opt/rocm/lib/llvm/bin/clang-offload-bundler", "/opt/rocm/lib/llvm/bin/llvm-readelf"]
# the precision-16 decoder suite's direct-mode shapes: base ES; one k = 3 decoder per dx2; tiny with row outliers
DIRECT = [("base", 2, 131, None), ("tiny_k3", 1, 140, None), ("small_k3", 1, 140, None), ("tiny", 2, 40, "row_outliers")]


# ---------------------------------------------------------------------------------------------------------------- CPU, no kernels
@pytest.mark.parametrize("name", ["tiny", "small", "tiny_k3"])
def test_decoder_mirror_matches_the_oracle(name):
    V.check_mirror_matches_oracle(BF16, name)


@pytest.mark.parametrize("config", ["v1", "v2", "v3"])
def test_vocoder_mirror_matches_the_reference_fixtures(config, yard):
    V.check_mirror_matches_fixture(yard, BF16, config)


def test_the_two_weight_rules_differ_by_one_ulp_on_few_weights():
    V.check_rules_agree_almost_everywhere()


def test_fused_kernels_weight_rule_bit_for_bit(tmp_path):
    V.check_plane_rule_bit_for_bit(tmp_path)


def test_get_hifigan_takes_the_precision(tmp_path):
    V.check_get_hifigan(tmp_path)


# ---------------------------------------------------------------------------------------------------------------- both tiers
def test_simulated_bf16_forward_with_h0_error_and_invariants(yard, device):
    """tiny ES, the whole forward, free-running ragged B = 3, L ~ 150 (two windows, edge rows, padding frames)"""
    V.check_forward_with_h0(yard, BF16, device)


def test_simulated_bf16_chunk_walk_and_window_form(yard, monkeypatch, device):
    """small ES: whole-utterance walks (several chunks per segment, carried rows, block skew) against the window form"""
    monkeypatch.setenv("ESMI_DEC_STREAM_WGS", "1")
    V.check_chunk_walk(yard, BF16, "small", 2, 60, 9, device)


@pytest.mark.parametrize("name,B,L,profile", DIRECT)
def test_simulated_bf16_direct_mode_error(name, B, L, profile, yard, device):
    V.check_direct(yard, BF16, name, B, L, device, profile)


def test_simulated_bf16_beyond_the_binary16_range(yard, device):
    V.check_beyond_binary16(yard, device)


@pytest.mark.parametrize("name", ["tiny", "small"])
def test_simulated_decoder_precisions_through_the_prec_entry_point(name, device):
    V.check_entry_points(name, device)


def test_simulated_range_checked_build_runs_bf16(device):
    V.check_range_check_honours_the_key(BF16, device)


def test_simulated_bf16_vocoder_accuracy_v2_two_windows(yard, device):
    """v2 with one launch per ResBlock at B = 1, L = 50 (all twelve (C, K) bf16 ResBlock1 instantiations; two windows in the first
    stage's k = 11 block)"""
    V.check_vocoder_accuracy(yard, BF16, "v2", device, True, 1, 50)


def test_simulated_bf16_through_synthesize(device):
    """tiny ES + v2; on the simulator the smallest 80-mel generator behind tiny ES (v2 takes a minute there)"""
    V.check_synthesize(BF16, device, small=device == "cpu")


def test_simulated_bf16_through_the_scheduler(device):
    V.check_scheduler(BF16, device)


def test_simulated_bf16_through_the_staged_forward_and_the_pipeline(device):
    V.check_staged_forward(BF16, device)


def test_simulated_python_refusals(device):
    V.check_python_refusals(BF16, device)


def test_simulated_precision16_keeps_the_parent_commits_bits(device):
    """the committed outputs of the build of the commit before bf16 inference: its simulator build, its libesmi.so on the device"""
    V.check_precision16_keeps_the_parents_bits(device, "sim" if device == "cpu" else "gpu")


test_bf16_forward_with_h0_error_and_invariants = on_the_device(test_simulated_bf16_forward_with_h0_error_and_invariants)
test_bf16_chunk_walk_and_window_form = on_the_device(test_simulated_bf16_chunk_walk_and_window_form)
test_bf16_direct_mode_error = on_the_device(test_simulated_bf16_direct_mode_error)
test_bf16_beyond_the_binary16_range = on_the_device(test_simulated_bf16_beyond_the_binary16_range)
test_decoder_precisions_through_the_prec_entry_point = on_the_device(test_simulated_decoder_precisions_through_the_prec_entry_point)
test_range_checked_build_runs_bf16 = on_the_device(test_simulated_range_checked_build_runs_bf16)
test_bf16_vocoder_two_resblock_windows = on_the_device(test_simulated_bf16_vocoder_accuracy_v2_two_windows)
test_bf16_through_synthesize = on_the_device(test_simulated_bf16_through_synthesize)
test_bf16_through_the_scheduler = on_the_device(test_simulated_bf16_through_the_scheduler)
test_bf16_through_the_staged_forward_and_the_pipeline = on_the_device(test_simulated_bf16_through_the_staged_forward_and_the_pipeline)
test_python_refusals_on_the_device = on_the_device(test_simulated_python_refusals)
test_precision16_keeps_the_parent_commits_bits_on_the_device = on_the_device(test_simulated_precision16_keeps_the_parent_commits_bits)


# ---------------------------------------------------------------------------------------------------------------- GPU tier only
@pytest.mark.gpu
@pytest.mark.parametrize("fused", [True, False], ids=["fused", "convs"])
@pytest.mark.parametrize("config", ["v1", "v2", "v3"])
def test_bf16_vocoder_error_is_the_bfloat16_operand_error(config, fused, yard, device):
    """the three fixture shapes (the precision-16 vocoder suite's)"""
    V.check_vocoder_accuracy(yard, BF16, config, device, fused)


@pytest.mark.gpu
def test_bf16_vocoder_ragged_keeps_its_contract(device):
    """v2, B = 3, L = 64, lengths [64, 33, 9], one launch per ResBlock and conv by conv"""
    V.check_ragged_contract(BF16, "v2", 3, 64, [64, 33, 9], device)


@pytest.mark.gpu
def test_vocoder_precision_0_and_32_are_the_existing_entry_points(device):
    V.check_default_untouched(BF16, "v2", 2, 24, [24, 5], device)


@pytest.mark.gpu
def test_bf16_graph_replay_captures_or_refuses(device):
    V.check_graph_replay(BF16, device)


# ---------------------------------------------------------------------------------------------------------------- simulator tier only
@pytest.mark.parametrize("name", ["reduced1", "reduced2"])
def test_simulated_bf16_vocoder_accuracy_reduced_generator_conv_by_conv(name, yard, device):
    """the reduced generators one launch per convolution, B = 2, L = 6"""
    V.check_vocoder_accuracy(yard, BF16, name, device, False, 2, 6)


def test_simulated_bf16_vocoder_accuracy_reduced_generator_fused(yard, device):
    V.check_vocoder_accuracy(yard, BF16, "reduced2", device, True, 2, 6)


def test_simulated_bf16_vocoder_ragged_keeps_its_contract(device):
    """the reduced generator, B = 3, lengths [6, 2, 0], both modes"""
    V.check_ragged_contract(BF16, "reduced1", 3, 6, [6, 2, 0], device, module=False)


def test_simulated_vocoder_precision_0_and_32_are_the_existing_entry_points(device):
    V.check_default_untouched(BF16, "small", 2, 6, [6, 2], device)


def test_c_refusals_launch_nothing():
    with use_sim():
        V.check_refusals_launch_nothing(BF16)


def test_exact_fp32_build_refuses_bf16():
    import __graft_entry__ as g
    g.build()
    V.check_fp32mfma_refuses(BF16, os.path.join(os.path.dirname(g.LIB), "libesmi_fp32mfma.so"))


def test_graph_replay_refuses_an_invalid_key_before_capturing():
    V.check_graph_replay_refuses_an_invalid_key()


@pytest.mark.parametrize("name", ["tiny", "small"])
def test_bf16_forward_launches_differ_in_the_decoder_name_only(name):
    with use_sim():
        V.check_decoder_dispatch(BF16, name, key32=name == "tiny")


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
