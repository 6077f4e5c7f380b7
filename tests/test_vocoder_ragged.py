"""Length-aware HiFi-GAN vocoding: esmi_hifigan_generator_ragged_f32, Generator.forward(x, lengths, pcm16), EfficientSpeech.synthesize
and BucketedSynthesizer(net, vocoder=...).  The checks live in tests/vocoder_ragged_checks.py; the GPU tier runs them on the device,
the CPU tier runs the bit-for-bit and the lengths == L checks through the wave simulator (the same kernel sources compiled for the host)."""
import pytest

from tests import vocoder_ragged_checks as V
from tests.simlib import use_sim

DEV = "cuda:0"


@pytest.fixture(scope="module")
def runs():
    """the plain runs the checks share (computed on first use), released when this module's tests are done"""
    r = V.PlainRuns()
    yield r
    r.clear()


# ---------------------------------------------------------------------------------------------------------------- GPU tier
@pytest.mark.gpu
@pytest.mark.parametrize("config", ["v2", "v1", "v3"])
def test_ragged_kept_samples_are_the_full_runs_bit_for_bit(config, runs):
    """B = 4, L = 64, lengths [64, 33, 9, 0]: every stage has several windows per utterance (v2 stage 1: 512 positions at TL = 136; the
    last stage 16,384 at TL = 392), the length-9 row skips windows at every stage, the length-33 row ends inside one.  Workspace and
    output are NaN-filled before the call; one launch per ResBlock and conv by conv."""
    V.check_kept_bit_identical(runs, config, 4, 64, [64, 33, 9, 0], DEV)


@pytest.mark.gpu
def test_ragged_kept_samples_vs_oracle():
    """v2, B = 3, L = 40, lengths [40, 21, 6] against oracle.hifigan on the same padded mel: < 2e-4, the bound
    test_hifigan_end_to_end_vs_oracle uses for this chain."""
    V.check_oracle(DEV)


@pytest.mark.gpu
def test_ragged_reads_nothing_behind_the_margin_it_claims():
    V.check_margin_is_tight(DEV)


@pytest.mark.gpu
def test_ragged_edges():
    V.check_edges(DEV)


@pytest.mark.gpu
@pytest.mark.parametrize("config,B,L", [("v2", 4, 64), ("v1", 2, 20), ("v3", 2, 20)])
def test_ragged_with_full_lengths_equals_plain_forward(config, B, L, runs):
    V.check_full_lengths_identity(runs, config, B, L, DEV)


@pytest.mark.gpu
def test_ragged_pcm16_plane():
    V.check_pcm(DEV)


@pytest.mark.gpu
def test_synthesize_and_bucketed_synthesizer_return_trimmed_waveforms():
    V.check_wrapper_and_scheduler(DEV)


# ---------------------------------------------------------------------------------------------------------------- CPU tier
def test_simulated_ragged_kept_samples_are_the_full_runs_bit_for_bit(runs):
    """v2 at the existing simulated fixture's shape, one launch per ResBlock: B = 2, L = 24, lengths [24, 5] -- the first stage already
    has two windows (192 positions at TL = 136), and the second is skipped for the short row (5 * 8 + 74 = 114 positions).  B = 2, not 3:
    at B = 3 with both modes the simulated tests of this file cost 95 s against the 35 s of the existing simulated vocoder tests; as
    they stand, 27 s + 14 s -- still over those 35 s, accepted: the L = 24 plain run and its length-aware run are the issue's case.  Row 0 is the lengths == L case on the one-launch kernels.  The zero-length row, the conv-by-conv mode
    (convgemm_len_kernel) and lengths == L through Generator.forward are in the next test, at a length the simulator runs quickly."""
    with use_sim():
        V.check_kept_bit_identical(runs, "v2", 2, 24, [24, 5], "cpu", modes=(True,))


def test_simulated_ragged_conv_by_conv_short_shape(runs):
    """B = 2, L = 7, one launch per convolution: every ConvTranspose1d and ResBlock convolution of the limited stages on
    convgemm_len_kernel (the last stage has 1,792 positions: 56 row tiles per utterance, most of them skipped), lengths [3, 0] -- a row
    that ends inside a tile and a zero-length row --, then lengths == L through Generator.forward on the same plain run."""
    with use_sim():
        V.check_kept_bit_identical(runs, "v2", 2, 7, [3, 0], "cpu", modes=(False,))
        V.check_full_lengths_identity(runs, "v2", 2, 7, "cpu", fused=False, module_plain=False)


def test_ragged_margins_match_the_receptive_field_walk():
    """The host-side walk (no kernels): conv_post 3; per stage the largest ResBlock halo; ConvTranspose1d(k, u) maps m to
    ceil((m + (k - u) / 2) / u); conv_pre 3."""
    from efficientspeech_amd.hifigan import HIFIGAN_CONFIGS, ragged_margins
    adds, frames = ragged_margins(HIFIGAN_CONFIGS["v2"])
    # ResBlock1 halos: k = 3: 9 + 3, k = 7: 27 + 9, k = 11: 45 + 15 = 60
    assert adds == [74, 107, 92, 63] and frames == 13
    # 63 = 3 + 60; 92 = ceil(64 / 2) + 60; 107 = ceil(93 / 2) + 60; 74 = ceil(111 / 8) + 60; ceil(78 / 8) = 10 frames + conv_pre's 3
    assert ragged_margins(HIFIGAN_CONFIGS["v1"]) == (adds, 13)
    # v3, ResBlock2 halos: k = 3: 1 + 2, k = 5: 4 + 12, k = 7: 9 + 36 = 45; stages (8, 8, 4) with kernels (16, 16, 8)
    assert ragged_margins(HIFIGAN_CONFIGS["v3"]) == ([53, 58, 48], 11)
