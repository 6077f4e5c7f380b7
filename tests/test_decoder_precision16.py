"""The mel decoder at precision 16: esmi_mel_decoder_prec_f32, esmi_phoneme2mel_forward_prec_f32, MelDecoder.precision /
MelDecoder.forward(..., precision), the inference key x["decoder_precision"], EfficientSpeech.synthesize(..., decoder_precision).  The
checks and the fp64 yardstick live in tests/decoder_precision16_checks.py; the GPU tier runs them on the device, the CPU tier through the
wave simulator (the same kernel sources compiled for the host).  `-s` prints every measured ratio (profiles/r11_decoder_precision16.md).
"""
import os

import pytest

from tests import decoder_precision16_checks as V
from tests.simlib import use_sim

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALE = None      # (no duration_control on the free-running batch)


@pytest.fixture(scope="module")
def yard():
    """the fp64 yardsticks the accuracy tests share (computed on first use), released when this module's tests are done"""
    y = V.Yardsticks()
    yield y
    y.clear()


# ---------------------------------------------------------------------------------------------------------------- test 0 (CPU, no kernels)
@pytest.mark.parametrize("name", ["tiny", "small", "base", "tiny_k3"])
def test_fp64_mirror_matches_the_oracle(name):
    """the yardstick's exact mode against oracle.mel_decoder (fp64): < 1e-6 L-inf, three orders below E_q"""
    V.check_mirror_matches_oracle(name)


# ---------------------------------------------------------------------------------------------------------------- GPU tier
@pytest.mark.gpu
def test_precision16_forward_with_h0_error_and_invariants(yard):
    """Tests 1 and 2, tiny ES, the whole forward, free-running ragged B = 3, L ~ 150 (two windows, edge rows, padding frames)."""
    V.check_forward_with_h0(yard, DEV, SCALE)


@pytest.mark.gpu
def test_precision16_chunk_walk_and_window_form(yard, monkeypatch):
    """Tests 1 and 2, small ES: whole-utterance walks (several chunks per segment, carried rows, block skew) and the window form."""
    monkeypatch.setenv("ESMI_DEC_STREAM_WGS", "1")
    V.check_chunk_walk(yard, "small", 2, 60, 9, DEV)


@pytest.mark.gpu
@pytest.mark.parametrize("name,B,L,profile", [("base", 2, 131, None), ("tiny_k3", 1, 140, None), ("small_k3", 1, 140, None),
                                              ("tiny", 2, 40, "row_outliers")])
def test_precision16_direct_mode_error(name, B, L, profile, yard):
    """Test 1, direct mode (the in-kernel `proj` stage: mma_sub): base ES; one k = 3 decoder per dx2; tiny with row outliers."""
    V.check_direct(yard, name, B, L, DEV, profile)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["tiny", "small"])
def test_precision_0_and_32_are_the_existing_entry_point(name):
    V.check_entry_points_at_32(name, DEV)


@pytest.mark.gpu
def test_range_checked_build_honours_the_key():
    V.check_range_check_honours_the_key(DEV)


@pytest.mark.gpu
def test_precision16_through_synthesize():
    V.check_wrappers(DEV)


@pytest.mark.gpu
def test_precision16_through_the_scheduler():
    V.check_scheduler(DEV)


@pytest.mark.gpu
def test_precision16_through_the_staged_forward_and_the_pipeline():
    V.check_staged_forward(DEV)


@pytest.mark.gpu
def test_precision16_graph_replay_captures_or_refuses():
    V.check_graph_replay(DEV)


@pytest.mark.gpu
def test_train_forward_runs_the_decoder_at_32():
    V.check_train_forward_ignores_the_attribute(DEV)


# ---------------------------------------------------------------------------------------------------------------- CPU tier (simulator)
def test_simulated_precision16_forward_with_h0_error_and_invariants(yard):
    with use_sim():
        V.check_forward_with_h0(yard, "cpu", SCALE)


def test_simulated_precision16_chunk_walk_and_window_form(yard, monkeypatch):
    monkeypatch.setenv("ESMI_DEC_STREAM_WGS", "1")
    with use_sim():
        V.check_chunk_walk(yard, "small", 2, 60, 9, "cpu")


@pytest.mark.parametrize("name,B,L,profile", [("base", 2, 131, None), ("tiny_k3", 1, 140, None), ("small_k3", 1, 140, None),
                                              ("tiny", 2, 40, "row_outliers")])
def test_simulated_precision16_direct_mode_error(name, B, L, profile, yard):
    with use_sim():
        V.check_direct(yard, name, B, L, "cpu", profile)


@pytest.mark.parametrize("name", ["tiny", "small"])
def test_simulated_precision_0_and_32_are_the_existing_entry_point(name):
    with use_sim():
        V.check_entry_points_at_32(name, "cpu")


@pytest.mark.parametrize("name", ["tiny", "small"])
def test_precision16_launches_differ_in_the_decoder_name_only(name):
    """Test 3 (simulator's launch log): one model per dx2 -- tiny, the one-launch encoder side + the window form; small, the encoder side
    launch by launch + the chunk walk."""
    with use_sim():
        V.check_dispatch(name, key32=name == "tiny")


def test_simulated_range_check_honours_the_key():
    with use_sim():
        V.check_range_check_honours_the_key("cpu")


def test_precision_refusals_launch_nothing():
    """Test 4: precision 8 (ESMI_ERR_ARG / ValueError) and the key with train=True (ValueError); nothing launched."""
    with use_sim():
        V.check_refusals()


def test_exact_fp32_build_refuses_precision16():
    """Test 4: libesmi_fp32mfma.so -> ESMI_ERR_UNSUPPORTED, decided on the host (runs without a GPU)."""
    import __graft_entry__ as g
    g.build()
    V.check_fp32mfma_refuses(os.path.join(os.path.dirname(g.LIB), "libesmi_fp32mfma.so"))


def test_simulated_precision16_through_the_scheduler():
    """Test 5, the scheduler half (synthesize() runs on the GPU tier only: the vocoder behind it takes a minute on the simulator)."""
    with use_sim():
        V.check_scheduler("cpu")


def test_simulated_precision16_through_the_staged_forward_and_the_pipeline():
    with use_sim():
        V.check_staged_forward("cpu")


def test_simulated_train_forward_runs_the_decoder_at_32():
    with use_sim():
        V.check_train_forward_ignores_the_attribute("cpu")


def test_graph_replay_refuses_an_invalid_key_before_capturing():
    """(host side only: the graph path validates the key before it touches the device)"""
    import torch
    from efficientspeech_amd.sharded import ShardedMelPipeline
    pipe = ShardedMelPipeline(V.make_net("tiny", "cpu")[0], use_graph=True)
    with pytest.raises(ValueError, match="precision"):
        pipe.step({"phoneme": torch.ones((1, 4), dtype=torch.int32), "max_mel_len": 16, "decoder_precision": 8})
    assert pipe.graphed is None
