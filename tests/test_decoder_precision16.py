"""The mel decoder at precision 16: esmi_mel_decoder_prec_f32, esmi_phoneme2mel_forward_prec_f32, MelDecoder.precision /
MelDecoder.forward(..., precision), the inference key x["decoder_precision"], EfficientSpeech.synthesize(..., decoder_precision).  The
checks, the operand rule `R16` and the fp64 yardstick live in tests/precision_checks.py, which tests/test_inference_bf16.py runs with the
bf16 rule.  A test that takes `device` runs on the wave simulator (the same kernel sources compiled for the host); `on_the_device` makes
its GPU-tier twin.  `-s` prints every measured ratio (profiles/r17_precision_tests.md).
"""
import os

import pytest

from tests import precision_checks as V
from tests.precision_checks import R16, device, on_the_device, yard   # noqa: F401 (fixtures)
from tests.simlib import use_sim

DIRECT = [("base", 2, 131, None), ("tiny_k3", 1, 140, None), ("small_k3", 1, 140, None), ("tiny", 2, 40, "row_outliers")]


@pytest.mark.parametrize("name", ["tiny", "small", "base", "tiny_k3"])
def test_fp64_mirror_matches_the_oracle(name):
    """the yardstick's exact mode against oracle.mel_decoder (fp64): < 1e-6 L-inf, three orders below E_q"""
    V.check_mirror_matches_oracle(R16, name)


# ---------------------------------------------------------------------------------------------------------------- both tiers
def test_simulated_precision16_forward_with_h0_error_and_invariants(yard, device):
    """tiny ES, the whole forward, free-running ragged B = 3, L ~ 150 (two windows, edge rows, padding frames)"""
    V.check_forward_with_h0(yard, R16, device)


def test_simulated_precision16_chunk_walk_and_window_form(yard, monkeypatch, device):
    """small ES: whole-utterance walks (several chunks per segment, carried rows, block skew) and the window form"""
    monkeypatch.setenv("ESMI_DEC_STREAM_WGS", "1")
    V.check_chunk_walk(yard, R16, "small", 2, 60, 9, device)


@pytest.mark.parametrize("name,B,L,profile", DIRECT)
def test_simulated_precision16_direct_mode_error(name, B, L, profile, yard, device):
    """direct mode (the in-kernel `proj` stage: mma_sub): base ES; one k = 3 decoder per dx2; tiny with row outliers"""
    V.check_direct(yard, R16, name, B, L, device, profile)


@pytest.mark.parametrize("name", ["tiny", "small"])
def test_simulated_precision_0_and_32_are_the_existing_entry_point(name, device):
    V.check_entry_points(name, device)


def test_simulated_range_check_honours_the_key(device):
    V.check_range_check_honours_the_key(R16, device)


def test_simulated_precision16_through_the_scheduler(device):
    V.check_scheduler(R16, device)


def test_simulated_precision16_through_the_staged_forward_and_the_pipeline(device):
    V.check_staged_forward(R16, device)


def test_simulated_train_forward_runs_the_decoder_at_32(device):
    V.check_train_forward_ignores_the_attribute(device)


test_precision16_forward_with_h0_error_and_invariants = on_the_device(test_simulated_precision16_forward_with_h0_error_and_invariants)
test_precision16_chunk_walk_and_window_form = on_the_device(test_simulated_precision16_chunk_walk_and_window_form)
test_precision16_direct_mode_error = on_the_device(test_simulated_precision16_direct_mode_error)
test_precision_0_and_32_are_the_existing_entry_point = on_the_device(test_simulated_precision_0_and_32_are_the_existing_entry_point)
test_range_checked_build_honours_the_key = on_the_device(test_simulated_range_check_honours_the_key)
test_precision16_through_the_scheduler = on_the_device(test_simulated_precision16_through_the_scheduler)
test_precision16_through_the_staged_forward_and_the_pipeline = on_the_device(test_simulated_precision16_through_the_staged_forward_and_the_pipeline)
test_train_forward_runs_the_decoder_at_32 = on_the_device(test_simulated_train_forward_runs_the_decoder_at_32)


# ---------------------------------------------------------------------------------------------------------------- one tier
@pytest.mark.gpu
def test_precision16_through_synthesize(device):
    """(GPU tier only: the v2 vocoder behind it takes a minute on the simulator)"""
    V.check_synthesize(R16, device)


@pytest.mark.gpu
def test_precision16_graph_replay_captures_or_refuses(device):
    V.check_graph_replay(R16, device)


@pytest.mark.parametrize("name", ["tiny", "small"])
def test_precision16_launches_differ_in_the_decoder_name_only(name):
    """(simulator's launch log) one model per dx2 -- tiny, the one-launch encoder side + the window form; small, the encoder side launch
    by launch + the chunk walk"""
    with use_sim():
        V.check_decoder_dispatch(R16, name, key32=name == "tiny")


def test_precision_refusals_launch_nothing():
    with use_sim():
        V.check_refusals_launch_nothing(R16)


def test_exact_fp32_build_refuses_precision16():
    """libesmi_fp32mfma.so -> ESMI_ERR_UNSUPPORTED, decided on the host (runs without a GPU)"""
    import __graft_entry__ as g
    g.build()
    V.check_fp32mfma_refuses(R16, os.path.join(os.path.dirname(g.LIB), "libesmi_fp32mfma.so"))


def test_graph_replay_refuses_an_invalid_key_before_capturing():
    V.check_graph_replay_refuses_an_invalid_key()
