"""Per-phoneme prosody curves: a (B, T) tensor under `pitch_control` / `energy_control` / `duration_control` -- esmi_prosody_curves
through the five kernels that make the discrete decisions (enc_va16 -- also inside the one-launch enc_all16 --, enc_va64, enc_pred128,
enc_fuse_va, va_tail), the three *_curve_f32 entry points, both Python paths, BucketedSynthesizer(controls=...) with per-request
curves, the sharded helpers and `prosody_curve`.  The checks live in tests/prosody_curve_checks.py; the CPU tier runs them through the
wave simulator (the same kernel sources compiled for the host), the GPU tier on the device.
Without the feature every kernel test here fails at the (B, T) shape check of `networks._prosody_controls`."""
import numpy as np
import pytest
import torch

from tests import prosody_curve_checks as Q
from tests.simlib import launched_kernels, use_sim
from tests.test_prosody_control import DECIDES, ENTRIES, GPU_SHAPES, SIM_CASES

DEV = "cuda:0"
_ran = set()


@pytest.fixture(scope="module", autouse=True)
def shared_runs():
    yield
    Q.clear()


# ---------------------------------------------------------------------------------------------------------------- CPU tier
@pytest.mark.parametrize("name,shape", [(n, s) for n in ("tiny", "small", "base") for s in (Q.SHAPE, (1, 17, (17,)))] +
                         [(n, (B, T, lens)) for n, B, T, lens in GPU_SHAPES], ids=lambda v: v if isinstance(v, str) else f"B{v[0]}-T{v[1]}")
def test_curve_seed_moves_half_of_the_oracles_decisions(name, shape):
    """The values that CURVE_SEED draws move at least half of the live decisions of each kind on the ORACLE's free-running predictions
    (no kernel involved), at every shape the decision checks run: their `changed >= 0.5` guard is a condition the inputs meet
    (0.85 or more at each shape)."""
    Q.check_seed_on_the_oracle(name, shape)


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("name,plan", SIM_CASES, ids=[f"{n}-{p}" for n, p in SIM_CASES])
def test_simulated_curves_decide_bit_exactly(name, plan, entry):
    """B = 3, T = 17, lengths (17, 9, 1), every phoneme's three values drawn from {0.5, 0.75, 1.25, 1.5}: bucket indices, durations,
    scan and mel_len equal the numpy fp32 restatement on the path's own raw predictions (and at least half of them moved), the raw
    predictions are the plain call's, the mel is the teacher-forced oracle's within 1e-4, zeros behind mel_len, the serving call."""
    with use_sim(), launched_kernels() as seen:
        Q.check_case(name, plan, entry, "cpu")
    kernels = {k.split("<")[0] for k in seen}
    assert DECIDES[name, plan, entry] in kernels, sorted(kernels)
    _ran.update(kernels)


def test_simulated_cases_cover_the_kernels_that_decide():
    """every kernel that bucketizes / rounds ran with curves in the cases above"""
    for (name, plan, entry), kernel in DECIDES.items():          # (run on its own: whatever the cases above have not run yet)
        if kernel not in _ran:
            test_simulated_curves_decide_bit_exactly(name, plan, entry)
    assert {"enc_all16_kernel", "enc_va16_kernel", "enc_va64_kernel", "enc_pred128_kernel", "enc_fuse_va_kernel", "va_tail_kernel"} <= _ran


# one case per deciding kernel (base ES: its row indexing and identities run on the device -- a simulated base forward costs ten seconds)
SIM_KERNEL_CASES = [("tiny", 63, "forward"), ("tiny", 63, "encode"), ("tiny", 31, "forward"), ("tiny", 0, "encode"), ("small", 63, "forward")]


@pytest.mark.parametrize("name,plan,entry", SIM_KERNEL_CASES + [("base", 63, "forward")])
def test_simulated_one_phoneme_moves_one_row(name, plan, entry):
    """B = 2, T = 21, utterance 1: a curve of 1.0 except at row 0 / 15 / 16 / 18 changes that row's decisions and nothing else
    (base ES: the two rows at the tile edge)"""
    with use_sim():
        Q.check_row_indexing(name, plan, entry, "cpu", ts=(15, 16) if name == "base" else Q.ROW_TS)


@pytest.mark.parametrize("name,plan,entry", SIM_KERNEL_CASES)
def test_simulated_identities_and_padding(name, plan, entry):
    """all-ones == plain, constant per utterance == the (B,) control, the mixed forms; NaN / 1e30 under the mask == 1.0 there"""
    with use_sim():
        Q.check_identities(name, plan, entry, "cpu")
        Q.check_padding_is_never_used(name, plan, entry, "cpu")


def test_simulated_padding_is_never_used_by_base():
    with use_sim():
        Q.check_padding_is_never_used("base", 63, "forward", "cpu")


@pytest.mark.parametrize("name,plan,entry", [("tiny", 63, "forward"), ("tiny", 31, "encode"), ("tiny", 0, "forward"), ("small", 63, "encode"),
                                             ("base", 63, "forward")])
def test_simulated_single_utterance_without_mask(name, plan, entry):
    with use_sim():
        Q.check_single_utterance(name, plan, entry, "cpu")


def test_simulated_errors():
    with use_sim():
        Q.check_value_errors("cpu")
        Q.check_abi_errors("cpu", launches=launched_kernels)


def test_scheduler_pads_each_requests_curve_into_its_batch():
    Q.check_scheduler_batches()


def test_simulated_scheduler_equals_the_direct_batches():
    with use_sim():
        Q.check_scheduler("cpu")


def test_sharding_keeps_each_utterances_curve():
    """shard_batch: (B, T) curves travel with their utterances (padding copies included) next to (B,) tensors and numbers; a
    one-utterance shard duplicates its row; the graph-replay path refuses a curve instead of dropping it."""
    from efficientspeech_amd import sharded
    B, T = 5, 6
    curve = torch.arange(B * T, dtype=torch.float32).reshape(B, T)
    x = {"phoneme": torch.arange(B * T).reshape(B, T), "phoneme_mask": torch.zeros(B, T, dtype=torch.bool),
         "pitch_control": curve, "energy_control": torch.arange(B, dtype=torch.float32), "duration_control": 0.9}
    rows = []
    for rank in range(3):
        s = sharded.shard_batch(x, rank, 3)
        assert s["pitch_control"].shape == (2, T) and torch.equal(s["pitch_control"], s["phoneme"].float())
        assert torch.equal(s["energy_control"], s["phoneme"][:, 0].float() / T) and s["duration_control"] == 0.9
        rows += s["pitch_control"][:, 0].tolist()
    assert rows == [0, 6, 12, 18, 24, 24]
    one, dup = sharded._masked_path_inputs(sharded.shard_batch(x, 2, 5))
    assert dup and one["pitch_control"].shape == (2, T) and torch.equal(one["pitch_control"][0], curve[2])
    assert torch.equal(one["pitch_control"][1], curve[2]) and torch.equal(one["pitch_control"], one["phoneme"].float())
    pipe = sharded.ShardedMelPipeline(None, use_graph=True)
    for k in ("pitch_control", "energy_control", "duration_control"):
        with pytest.raises(NotImplementedError, match=k):
            pipe.step({"phoneme": x["phoneme"], "phoneme_mask": x["phoneme_mask"], "max_mel_len": 64, k: torch.ones(B, T)})
    assert pipe.graphed is None


def test_prosody_curve_spans():
    """prosody_curve: (B, T) fp32 from (b, start, stop, value) spans -- later spans win, `stop` is clipped, the default elsewhere"""
    import efficientspeech_amd
    from efficientspeech_amd import prosody_curve
    assert "prosody_curve" in efficientspeech_amd.__all__
    c = prosody_curve((2, 8), [(0, 2, 5, 1.5), (0, 4, 6, 0.5), (1, 6, 99, 2.0), (1, 0, 1, 0.25)])
    assert c.dtype == torch.float32 and c.shape == (2, 8)
    assert c[0].tolist() == [1, 1, 1.5, 1.5, 0.5, 0.5, 1, 1]
    assert c[1].tolist() == [0.25, 1, 1, 1, 1, 1, 2, 2]
    c = prosody_curve([5, 3], [(1, 1, None, 1.25)], default=0.9)            # lengths: T = the longest; stop None = to the end
    assert c.shape == (2, 5) and c[0].tolist() == pytest.approx([0.9] * 5) and c[1].tolist() == pytest.approx([0.9, 1.25, 1.25, 1.25, 1.25])
    assert prosody_curve(torch.tensor([4, 2]), []).shape == (2, 4) and bool((prosody_curve(np.array([4, 2]), []) == 1).all())
    assert prosody_curve((1, 3), [(0, 1, 1, 7.0)]).tolist() == [[1, 1, 1]]  # an empty span
    for bad in ([(2, 0, 1, 1.0)], [(0, -1, 2, 1.0)], [(0, 3, 2, 1.0)]):
        with pytest.raises(ValueError):
            prosody_curve((2, 8), bad)


def test_synthesize_passes_a_curve_on():
    """EfficientSpeech.synthesize(pitch_control=curve) only fills the key (host side: a recording stand-in)"""
    from types import SimpleNamespace
    from efficientspeech_amd import EfficientSpeech, prosody_curve
    seen = {}

    def p2m(batch, train=False):
        seen.update(batch)
        return torch.zeros(1, 4, 80), torch.tensor([4], dtype=torch.int32), torch.zeros(1, 3, 1)
    voc = lambda mel, lengths=None, pcm16=False: torch.zeros(1, 1, 4 * 256)     # noqa: E731
    voc.h = SimpleNamespace(hop=256)
    curve = prosody_curve((1, 3), [(0, 1, 2, 1.3)])
    EfficientSpeech.synthesize(SimpleNamespace(hifigan=voc, phoneme2mel=p2m), {"phoneme": torch.ones(1, 3, dtype=torch.int32)},
                               pitch_control=curve)
    assert seen["pitch_control"] is curve


# ---------------------------------------------------------------------------------------------------------------- GPU tier
@pytest.mark.gpu
@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("plan", [63, 31, 7, 0])
@pytest.mark.parametrize("name", ["tiny", "small", "base"])
def test_curves_on_the_device(name, plan, entry):
    """every check of the fixed cases on the device, per config, plan and entry point"""
    Q.check_case(name, plan, entry, DEV)
    Q.check_row_indexing(name, plan, entry, DEV)
    Q.check_identities(name, plan, entry, DEV)
    Q.check_padding_is_never_used(name, plan, entry, DEV)
    Q.check_single_utterance(name, plan, entry, DEV)


@pytest.mark.gpu
@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("name,B,T,lens", GPU_SHAPES, ids=[f"{n}-T{t}" for n, _, t, _ in GPU_SHAPES])
def test_curves_on_the_device_at_the_kernels_other_shapes(name, B, T, lens, entry):
    """enc_all16<8>, the second tile per wave, multi-workgroup enc_fuse_va with the scan as its own launch, va_tail"""
    shape = (B, T, lens)
    Q.check_case(name, 63, entry, DEV, shape)
    Q.check_padding_is_never_used(name, 63, entry, DEV, shape)
    Q.check_row_indexing(name, 63, entry, DEV, ts=(0, lens[1] - 1), shape=shape)


@pytest.mark.gpu
def test_errors_on_the_device():
    Q.check_value_errors(DEV)
    Q.check_abi_errors(DEV)


@pytest.mark.gpu
def test_scheduler_equals_the_direct_batches_on_the_device():
    Q.check_scheduler(DEV)


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["libesmi_fp32mfma.so", "libesmi_checked.so"])
def test_the_other_builds_serve_curves(which):
    Q.check_other_build(which, DEV)
