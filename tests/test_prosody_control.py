"""Per-utterance pitch / energy / speed controls at inference: esmi_prosody_control through the five kernels that make the discrete
decisions (enc_va16 -- also inside the one-launch enc_all16 --, enc_va64, enc_pred128, enc_fuse_va, va_tail), the three *_ctl_f32
entry points, the `pitch_control` / `energy_control` / `duration_control` keys of both Python paths, EfficientSpeech.synthesize,
BucketedSynthesizer(controls=...) and the sharded helpers.  The checks live in tests/prosody_control_checks.py; the CPU tier runs them
through the wave simulator (the same kernel sources compiled for the host), the GPU tier on the device."""
import numpy as np
import pytest
import torch

from tests import prosody_control_checks as P
from tests.simlib import launched_kernels, use_sim

DEV = "cuda:0"
SIM_CASES = [("tiny", 63), ("tiny", 31), ("tiny", 0), ("small", 63), ("base", 63)]
ENTRIES = ["forward", "encode"]
# the kernel that makes the decisions in each simulated case (tests/test_dispatch.py pins the whole sequences)
DECIDES = {("tiny", 63, "forward"): "enc_all16_kernel", ("tiny", 63, "encode"): "enc_va16_kernel", ("tiny", 31, "forward"): "enc_fuse_va_kernel",
           ("tiny", 31, "encode"): "enc_fuse_va_kernel", ("tiny", 0, "forward"): "va_tail_kernel", ("tiny", 0, "encode"): "va_tail_kernel",
           ("small", 63, "forward"): "enc_va64_kernel", ("small", 63, "encode"): "enc_va64_kernel",
           ("base", 63, "forward"): "enc_pred128_kernel", ("base", 63, "encode"): "enc_pred128_kernel"}
_ran = set()


@pytest.fixture(scope="module", autouse=True)
def shared_runs():
    yield
    P.clear()


# ---------------------------------------------------------------------------------------------------------------- CPU tier
@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("name,plan", SIM_CASES, ids=[f"{n}-{p}" for n, p in SIM_CASES])
def test_simulated_controls_decide_bit_exactly(name, plan, entry):
    """B = 3, T = 17, lengths (17, 9, 1), scales pitch (1.5, 0.5, 1.25), energy (0.5, 1.5, 0.75), duration (1.5, 0.75, 1.25):
    bucket indices, durations, scan and mel_len equal the numpy fp32 restatement on the path's own raw predictions (and at least half
    of them moved), the raw predictions are the uncontrolled call's, the mel is the teacher-forced oracle's within 1e-4.
    Without the feature the kernels ignore the scales: the decisions are the uncontrolled ones and this fails."""
    with use_sim(), launched_kernels() as seen:
        P.check_case(name, plan, entry, "cpu")
    kernels = {k.split("<")[0] for k in seen}
    assert DECIDES[name, plan, entry] in kernels, sorted(kernels)
    _ran.update(kernels)


def test_simulated_cases_cover_the_kernels_that_decide():
    """every kernel that bucketizes / rounds ran with controls in the cases above"""
    for (name, plan, entry), kernel in DECIDES.items():          # (run on its own: whatever the cases above have not run yet)
        if kernel not in _ran:
            test_simulated_controls_decide_bit_exactly(name, plan, entry)
    assert {"enc_all16_kernel", "enc_va16_kernel", "enc_va64_kernel", "enc_pred128_kernel", "enc_fuse_va_kernel", "va_tail_kernel"} <= _ran


@pytest.mark.parametrize("name,plan,entry", [("tiny", 63, "forward"), ("tiny", 63, "encode"), ("tiny", 31, "forward"), ("tiny", 0, "encode"),
                                             ("small", 63, "forward")])
def test_simulated_identity_and_per_utterance_indexing(name, plan, entry):
    """No keys, 1.0 and a ones tensor are bit-identical; every utterance reads its own scale and nobody else's.  (base ES: on the device
    only -- a simulated base forward costs ten seconds, this check eleven of them.)"""
    with use_sim():
        P.check_identity(name, plan, entry, "cpu")
        mixed = P.check_case(name, plan, entry, "cpu")
        P.check_per_utterance(name, plan, entry, "cpu", mixed)


@pytest.mark.parametrize("name,plan,entry", [("tiny", 63, "forward"), ("tiny", 31, "encode"), ("tiny", 0, "forward"), ("small", 63, "encode"),
                                             ("base", 63, "forward")])
def test_simulated_single_utterance_without_mask(name, plan, entry):
    with use_sim():
        P.check_single_utterance(name, plan, entry, "cpu")


def test_simulated_errors():
    with use_sim():
        P.check_value_errors("cpu")
        P.check_abi_errors("cpu", launches=launched_kernels)


def test_simulated_scheduler_gathers_the_controls_per_batch():
    with use_sim():
        P.check_scheduler("cpu")


def test_synthesize_fills_the_control_keys():
    """EfficientSpeech.synthesize(pitch_control=, energy_control=, duration_control=): the arguments become the input-dict keys (host
    side only: a recording stand-in for the acoustic model and the vocoder)."""
    from types import SimpleNamespace
    from efficientspeech_amd import EfficientSpeech
    seen = {}

    def p2m(batch, train=False):
        seen.update(batch)
        return torch.zeros(1, 4, 80), torch.tensor([4], dtype=torch.int32), torch.zeros(1, 3, 1)
    voc = lambda mel, lengths=None, pcm16=False: torch.zeros(1, 1, 4 * 256)     # noqa: E731
    model = SimpleNamespace(hifigan=voc, phoneme2mel=p2m)
    voc.h = SimpleNamespace(hop=256)
    batch = {"phoneme": torch.ones(1, 3, dtype=torch.int32), "energy_control": 0.5}
    EfficientSpeech.synthesize(model, batch, pitch_control=1.2, duration_control=torch.tensor([0.8]))
    assert seen["pitch_control"] == 1.2 and seen["energy_control"] == 0.5 and torch.equal(seen["duration_control"], torch.tensor([0.8]))
    assert "pitch_control" not in batch                          # (the caller's dict is left alone)
    seen.clear()
    EfficientSpeech.synthesize(model, batch)
    assert "pitch_control" not in seen and "duration_control" not in seen


def test_sharding_keeps_each_utterances_controls():
    """shard_batch: (B,) control tensors travel with their utterances (padding copies included), numbers and () tensors unchanged; a
    one-utterance shard duplicates its scale with its utterance; the graph-replay path refuses a control instead of dropping it."""
    from efficientspeech_amd import sharded
    B, T = 5, 6
    x = {"phoneme": torch.arange(B * T).reshape(B, T), "phoneme_mask": torch.zeros(B, T, dtype=torch.bool),
         "pitch_control": torch.arange(B, dtype=torch.float32) + 1, "duration_control": 1.25, "energy_control": torch.tensor(0.5)}
    seen = []
    for rank in range(3):
        s = sharded.shard_batch(x, rank, 3)
        assert s["duration_control"] == 1.25 and s["energy_control"].shape == ()
        assert s["pitch_control"].shape == (2,) and torch.equal(s["pitch_control"], s["phoneme"][:, 0].float() / T + 1)
        seen += s["pitch_control"].tolist()
    assert seen == [1, 2, 3, 4, 5, 5]
    one, dup = sharded._masked_path_inputs(sharded.shard_batch(x, 2, 5))
    assert dup and torch.equal(one["pitch_control"], torch.tensor([3.0, 3.0])) and one["phoneme"].shape[0] == 2
    pipe = sharded.ShardedMelPipeline(None, use_graph=True)
    for k in ("pitch_control", "energy_control", "duration_control"):
        with pytest.raises(NotImplementedError, match=k):
            pipe.step({"phoneme": x["phoneme"], "phoneme_mask": x["phoneme_mask"], "max_mel_len": 64, k: 1.1})
    assert pipe.graphed is None


# ---------------------------------------------------------------------------------------------------------------- GPU tier
GPU_SHAPES = [("tiny", 2, 128, (128, 77)),      # enc_all16_kernel<8>
              ("tiny", 2, 150, (150, 97)),      # long-sequence enc_fuse_va: several workgroups per utterance, the scan as its own launch
              ("small", 2, 150, (150, 97)),     # second tile per wave (enc_va64)
              ("base", 2, 150, (150, 97)),      # second tile per wave (enc_pred128)
              ("small", 2, 270, (270, 131)),    # dim-64 enc_fuse_va
              ("base", 2, 270, (270, 131))]     # va_tail


@pytest.mark.gpu
@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("plan", [63, 31, 7, 0])
@pytest.mark.parametrize("name", ["tiny", "small", "base"])
def test_controls_on_the_device(name, plan, entry):
    """every check of the fixed case (B = 3, T = 17) on the device, per config, plan and entry point"""
    P.check_identity(name, plan, entry, DEV)
    mixed = P.check_case(name, plan, entry, DEV)
    P.check_per_utterance(name, plan, entry, DEV, mixed)
    P.check_single_utterance(name, plan, entry, DEV)


@pytest.mark.gpu
@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("name,B,T,lens", GPU_SHAPES, ids=[f"{n}-T{t}" for n, _, t, _ in GPU_SHAPES])
def test_controls_on_the_device_at_the_kernels_other_shapes(name, B, T, lens, entry):
    shape = (B, T, lens)
    P.check_identity(name, 63, entry, DEV, shape)
    P.check_case(name, 63, entry, DEV, shape)


@pytest.mark.gpu
def test_errors_on_the_device():
    P.check_value_errors(DEV)
    P.check_abi_errors(DEV)


@pytest.mark.gpu
def test_scheduler_gathers_the_controls_per_batch_on_the_device():
    P.check_scheduler(DEV)


@pytest.mark.gpu
def test_number_and_tensor_controls_agree_with_synthesize():
    """EfficientSpeech.synthesize with keyword controls = the dict keys through predict_step's path (mel_len * hop, same durations)"""
    from efficientspeech_amd import EfficientSpeech
    from efficientspeech_amd.hifigan import HIFIGAN_CONFIGS, Generator, synth_hifigan_state_dict
    net, _, _ = P.net_of("tiny", DEV)
    h = HIFIGAN_CONFIGS["v2"]
    voc = Generator(h)
    voc.load_state_dict({k: torch.from_numpy(v) for k, v in synth_hifigan_state_dict(h, 1234).items()})
    model = EfficientSpeech.from_config("tiny", hifigan=voc.to(DEV).eval())
    model.phoneme2mel = net
    x = P.inputs(*P.SHAPE, DEV)[0]
    ctl = P.controls(3, DEV)
    with torch.no_grad():
        wav, wav_len, dur = model.synthesize(x, **ctl)
        mel, mel_len, dur2 = net(dict(x, **ctl))
        _, plain_len, _ = net(x)
    assert torch.equal(wav_len, mel_len * h.hop) and torch.equal(dur, dur2) and wav.shape == (3, mel.shape[1] * h.hop)
    assert not torch.equal(mel_len, plain_len)
    assert np.isfinite(wav.cpu().numpy()).all()
