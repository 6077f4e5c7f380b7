"""Checks of the HiFi-GAN generator at precision 16 (esmi_hifigan_generator_prec_f32, Generator.forward(..., precision=16)), shared by
the GPU tier and the wave-simulator tier of tests/test_vocoder_precision16.py.  Every check takes the device ("cuda:0", or "cpu"
inside `use_sim()`).

The yardstick is `mirror()`: a torch fp64 restatement of Generator.forward with two modes -- exact, and rounded operands (the input and
the weight of every convolution but conv_post through `.to(float16)`).  E_q = rounded - exact is the error any ideal binary16-operand
implementation has; the kernels are held to it through their error against the EXACT run (they cannot match the rounded mirror
closely: fp32 accumulation flips binary16 rounding boundaries of the next layer's operands).
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from efficientspeech_amd import networks
from efficientspeech_amd.hifigan import HIFIGAN_CONFIGS, Generator, HifiGanConfig, synth_hifigan_state_dict
from efficientspeech_amd.networks import _on_device_of, _ptr
from tests.vocoder_ragged_checks import assert_kept_and_tails, make_mel

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURES = {"v1": "hifigan_v1_b1_l9.npz", "v2": "hifigan_v2_b2_l24.npz", "v3": "hifigan_v3_b1_l17.npz"}


def reduced_config(resblock=1):
    """the reduced generator of tests/test_vocoder_dispatch.py: 256 -> 128 / 64 / 32 channels, rates (2, 2, 2), k = 3 and 7, 16 mels"""
    return HifiGanConfig(resblock=str(resblock), upsample_rates=(2, 2, 2), upsample_kernel_sizes=(4, 4, 4), upsample_initial_channel=256,
                         resblock_kernel_sizes=(3, 7), resblock_dilation_sizes=((1, 3, 5),) * 2 if resblock == 1 else ((1, 3),) * 2,
                         num_mels=16)


def small_config():
    """the smallest generator with both launch families: 32 -> 16 / 8 channels (one-launch ResBlocks on the 16-row tiles), rates (2, 2),
    one k = 3 ResBlock1 per stage, 8 mels -- for checks that only compare calls with each other on the simulator"""
    return HifiGanConfig(resblock="1", upsample_rates=(2, 2), upsample_kernel_sizes=(4, 4), upsample_initial_channel=32,
                         resblock_kernel_sizes=(3,), resblock_dilation_sizes=((1, 3, 5),), num_mels=8)


def config_of(name):
    if name in HIFIGAN_CONFIGS:
        return HIFIGAN_CONFIGS[name]
    return small_config() if name == "small" else reduced_config(int(name[-1]))   # "reduced1" / "reduced2"


def make_vocoder(name, device, fused=True, precision=32):
    h = config_of(name)
    voc = Generator(h, precision=precision)
    voc.load_state_dict({k: torch.from_numpy(v) for k, v in synth_hifigan_state_dict(h, 1234).items()}, strict=True)
    voc = voc.to(device).eval()
    voc.fuse_resblocks = fused
    return voc


# ---------------------------------------------------------------------------------------------------------------- the yardstick
def mirror(h, sd, mel, rounded):
    """Generator.forward in fp64 on host tensors.  mel (B, L, num_mels) -> wav (B, L * hop).  The mean over a stage's ResBlocks is folded
    into the next input scale, as the library does.  rounded: every convolution's input (after its leaky_relu) and weight through
    binary16, except conv_post's."""
    q = (lambda t: t.to(torch.float16).to(torch.float64)) if rounded else (lambda t: t)
    W = lambda key: torch.as_tensor(sd[key]).to(torch.float64)   # noqa: E731
    pad = lambda k, d: (k * d - d) // 2                          # noqa: E731
    x = torch.as_tensor(mel).to(torch.float64).transpose(1, 2)
    x = F.conv1d(q(x), q(W("conv_pre.weight")), W("conv_pre.bias"), padding=3)
    scale, n, nk = 1.0, 0, len(h.resblock_kernel_sizes)
    for i, (u, k) in enumerate(zip(h.upsample_rates, h.upsample_kernel_sizes)):
        x = F.conv_transpose1d(q(F.leaky_relu(scale * x, 0.1)), q(W(f"ups.{i}.weight")), W(f"ups.{i}.bias"), stride=u, padding=(k - u) // 2)
        xs = 0.0
        for kk, dil in zip(h.resblock_kernel_sizes, h.resblock_dilation_sizes):
            r = x
            for m, d in enumerate(dil):
                if h.resblock == "1":
                    t = F.conv1d(q(F.leaky_relu(r, 0.1)), q(W(f"resblocks.{n}.convs1.{m}.weight")), W(f"resblocks.{n}.convs1.{m}.bias"),
                                 dilation=d, padding=pad(kk, d))
                    t = F.conv1d(q(F.leaky_relu(t, 0.1)), q(W(f"resblocks.{n}.convs2.{m}.weight")), W(f"resblocks.{n}.convs2.{m}.bias"),
                                 padding=pad(kk, 1))
                else:
                    t = F.conv1d(q(F.leaky_relu(r, 0.1)), q(W(f"resblocks.{n}.convs.{m}.weight")), W(f"resblocks.{n}.convs.{m}.bias"),
                                 dilation=d, padding=pad(kk, d))
                r = t + r
            xs = xs + r
            n += 1
        x, scale = xs, 1.0 / nk
    x = F.conv1d(F.leaky_relu(scale * x, 0.01), W("conv_post.weight"), W("conv_post.bias"), padding=3)
    return torch.tanh(x)[:, 0]


class Yardsticks:
    """(mel, exact, E_q) per (generator, B, L): computed once, shared, never modified (a module-scoped fixture owns it)."""

    def __init__(self):
        self.runs = {}

    def get(self, name, B=None, L=None):
        """name in FIXTURES with B None: the committed fixture's mel; else make_mel(h, B, L)"""
        key = (name, B, L)
        if key not in self.runs:
            h = config_of(name)
            sd = synth_hifigan_state_dict(h, 1234)
            if B is None:
                g = np.load(os.path.join(GOLD, FIXTURES[name]))
                assert str(g["config"]) == name
                mel = torch.from_numpy(g["mel"])
            else:
                mel = make_mel(h, B, L, "cpu")
            exact = mirror(h, sd, mel, False)
            self.runs[key] = (mel, exact, mirror(h, sd, mel, True) - exact)
        return self.runs[key]

    def clear(self):
        self.runs.clear()


def rms(t):
    return float(t.to(torch.float64).pow(2).mean().sqrt())


def check_mirror_matches_fixture(yard, name):
    """Test 0: the exact mode against the reference-generated waveform (measured: 1.9e-7 / 2.7e-7 / 4.4e-7 L-inf for v1 / v2 / v3)."""
    _mel, exact, eq = yard.get(name)
    ref = torch.from_numpy(np.load(os.path.join(GOLD, FIXTURES[name]))["wav"]).to(torch.float64)
    err = float((exact - ref).abs().max())
    print(f"{name}: mirror vs fixture L-inf {err:.2e}; E_q L-inf {float(eq.abs().max()):.2e} rms {rms(eq):.2e}")
    assert err < 2e-6, err


def check_accuracy(yard, name, device, fused, B=None, L=None):
    """Test 1: e = wav16 - exact against E_q: rms(e) <= 1.25 rms(E_q), max|e| <= 2 max|E_q|, and rms(e) >= 0.5 rms(E_q) -- the
    one-product path really ran (the default path sits at 5e-8 rms)."""
    mel, exact, eq = yard.get(name, B, L)
    voc = make_vocoder(name, device, fused=fused)
    with torch.no_grad():
        wav = voc(mel.to(device).transpose(1, 2), precision=16)
    assert wav.shape == (mel.shape[0], 1, mel.shape[1] * voc.h.hop) and wav.dtype == torch.float32
    e = wav[:, 0].cpu().to(torch.float64) - exact
    r_rms, r_max = rms(e) / rms(eq), float(e.abs().max()) / float(eq.abs().max())
    print(f"{name} fused={fused} {tuple(mel.shape)}: rms(e) {rms(e):.3e} = {r_rms:.3f} rms(E_q); max|e| {float(e.abs().max()):.3e} = {r_max:.3f} max|E_q|")
    assert bool(torch.isfinite(wav).all())
    assert r_rms <= 1.25, r_rms
    assert r_max <= 2.0, r_max
    assert r_rms >= 0.5, r_rms
    return r_rms, r_max


# ---------------------------------------------------------------------------------------------------------------- the C-ABI, driven directly
def run_prec(voc, mel, precision, lengths=None, want_wav=True, want_pcm=False, lib=None):
    """esmi_hifigan_generator_prec_f32 on test-owned, NaN-filled workspace and outputs -> (wav (B, L * hop) or None, pcm or None)"""
    wt = voc.conv_post.weight
    rt_lib, stream = networks._runtime(wt)
    lib = lib or rt_lib
    B, L, _ = mel.shape
    n = L * voc.h.hop
    with _on_device_of(wt), torch.no_grad():
        w, s, _keep = voc._packed(lib, stream)
        nbytes = lib.esmi_hifigan_workspace_bytes(C.byref(s), B, L)
        ws = torch.full((nbytes // 4,), float("nan"), dtype=torch.float32, device=mel.device)
        wav = torch.full((B, n), float("nan"), dtype=torch.float32, device=mel.device) if want_wav else None
        pcm = torch.full((B, n), -12345, dtype=torch.int16, device=mel.device) if want_pcm else None
        ln = None if lengths is None else torch.as_tensor(lengths, dtype=torch.int32).to(mel.device)
        lib.esmi_hifigan_generator_prec_f32(C.byref(w), C.byref(s), _ptr(mel), B, L, _ptr(ln), _ptr(wav), _ptr(pcm), precision, _ptr(ws),
                                            nbytes, stream)
        if mel.is_cuda:
            torch.cuda.synchronize()
    return wav, pcm


def check_ragged_contract(name, B, L, lengths, device, modes=(True, False), module=True):
    """Test 2: at precision 16 the length-aware call's kept samples are the plain precision-16 run's bit for bit, the tails exact zeros
    (workspace and outputs NaN-filled), and the PCM plane is trunc(clamp(wav16 * 32768, -32768, 32767))."""
    for fused in modes:
        voc = make_vocoder(name, device, fused=fused)
        mel = make_mel(voc.h, B, L, device)
        full, _ = run_prec(voc, mel, 16)
        assert float(full.abs().max()) > 1e-3
        got, pcm = run_prec(voc, mel, 16, lengths, want_pcm=True)
        assert_kept_and_tails(got, full, lengths, voc.h.hop, f"{name} fused={fused} precision 16")
        assert torch.equal(pcm, (got * 32768).clamp(-32768, 32767).trunc().to(torch.int16))
        assert int(pcm.abs().max()) > 30
        if not module:
            continue
        with torch.no_grad():   # precision 16 is not precision 32 (and the module passes it on)
            assert not torch.equal(voc(mel.transpose(1, 2))[:, 0], full)
            assert torch.equal(voc(mel.transpose(1, 2), precision=16)[:, 0], full)


def check_default_untouched(name, B, L, lengths, device, fused=True):
    """Test 3: precision 0 and 32 through the new entry point are the two existing entry points, bit for bit."""
    from tests.vocoder_ragged_checks import run_abi
    voc = make_vocoder(name, device, fused=fused)
    assert voc.precision == 32 and Generator().precision == 32
    mel = make_mel(voc.h, B, L, device)
    plain, _ = run_abi(voc, mel)
    rag, rag_pcm = run_abi(voc, mel, lengths, want_pcm=True)
    assert bool(torch.isfinite(plain).all())
    for precision in (0, 32):
        a, none = run_prec(voc, mel, precision)
        assert none is None and torch.equal(a, plain), precision
        b, b_pcm = run_prec(voc, mel, precision, lengths, want_pcm=True)
        assert torch.equal(b, rag) and torch.equal(b_pcm, rag_pcm), precision


def check_refusals(device):
    """Test 5 (simulator: the launch log shows that nothing was enqueued)."""
    from tests.simlib import launch_records
    with pytest.raises(ValueError, match="precision"):
        Generator(reduced_config(), precision=8)
    voc = make_vocoder("reduced1", device)
    mel = make_mel(voc.h, 2, 6, device)
    with pytest.raises(ValueError, match="precision"), torch.no_grad():
        voc(mel.transpose(1, 2), precision=8)
    run_prec(voc, mel, 32)                        # (weights packed: the records below are the calls' alone)
    with launch_records() as records:
        with pytest.raises(RuntimeError, match="esmi_hifigan_generator_prec_f32 failed: ESMI_ERR_ARG"):
            run_prec(voc, mel, 8)
        with pytest.raises(RuntimeError, match="esmi_hifigan_generator_prec_f32 failed: ESMI_ERR_ARG"):
            run_prec(voc, mel, 16, None, want_pcm=True)      # a PCM plane without lengths
    assert records == []


def check_wrappers(device):
    """Test 6: EfficientSpeech.synthesize(batch, precision=16) and a BucketedSynthesizer whose vocoder has precision = 16, tiny ES + v2,
    B = 3, T = 12, against Generator.forward(..., precision=16) on the same mel: kept samples bit for bit, wav_len unchanged."""
    from efficientspeech_amd import BucketedSynthesizer, EfficientSpeech
    from efficientspeech_amd.config import CONFIGS
    from efficientspeech_amd.synth import synth_phonemes, synth_state_dict
    voc = make_vocoder("v2", device)
    hop = voc.h.hop
    model = EfficientSpeech.from_config("tiny", hifigan=voc)
    model.phoneme2mel.load_state_dict({k: torch.from_numpy(v) for k, v in synth_state_dict(CONFIGS["tiny"], 1234).items()}, strict=True)
    model = model.to(device).eval()
    B, T, plens = 3, 12, [12, 7, 3]
    ids, mask = synth_phonemes(B, T, 12, plens)
    dur = np.random.default_rng(3).integers(1, 4, size=(B, T)).astype(np.int32)
    x = {"phoneme": torch.from_numpy(ids).to(device), "phoneme_mask": torch.from_numpy(mask).to(device),
         "duration_forced": torch.from_numpy(dur).to(device)}
    with torch.no_grad():
        mel, mel_len, _ = model.phoneme2mel(x, train=False)
        ref16 = voc(mel.transpose(1, 2), precision=16)[:, 0]
        wav32, len32, _ = model.synthesize(x)
        wav16, len16, _ = model.synthesize(x, precision=16)
        with pytest.raises(ValueError, match="precision"):
            model.synthesize(x, precision=8)
    ml = mel_len.cpu().numpy()
    assert torch.equal(len16, len32) and np.array_equal(len16.cpu().numpy(), ml * hop)
    assert_kept_and_tails(wav16, ref16, ml, hop, "synthesize(precision=16)")
    assert not torch.equal(wav16, wav32)
    # the scheduler calls the vocoder it was given: one whose default is 16
    voc16 = make_vocoder("v2", device, precision=16)
    assert voc16.precision == 16
    lens = [12, 7, 3]
    seqs = [ids[b, :n].astype(np.int32) for b, n in enumerate(lens)]

    def extra(idx, T_):
        d = np.zeros((len(idx), T_), np.int32)
        for r, i in enumerate(idx):
            d[r, :lens[i]] = dur[i, :lens[i]]
        return {"duration_forced": torch.from_numpy(d).to(device)}
    res = BucketedSynthesizer(model.phoneme2mel, max_batch=1, granularity=4, vocoder=voc16)(seqs, extra=extra)
    for i, (wav_i, mel_i, _dur_i) in enumerate(res):
        n = int(dur[i, :lens[i]].sum())
        assert wav_i.shape == (n * hop,) and mel_i.shape == (n, 80)
        with torch.no_grad():
            alone = voc(mel_i[None].transpose(1, 2), precision=16)[0, 0]
        assert torch.equal(wav_i, alone), i


# ---------------------------------------------------------------------------------------------------------------- launches (simulator)
_PREP = ("pack_", "absmax_kernel")


def run_row(resblock, fused, ragged):
    """the launch records of one Generator.forward(..., precision=16) of the reduced generator on the simulator (B = 2, L = 6, lengths
    [6, 2]; weight preparation left out), run-length encoded in the format of tests/test_vocoder_dispatch.py"""
    from tests.simlib import launch_records, use_sim
    h = reduced_config(resblock)
    mel = make_mel(h, 2, 6, "cpu")
    with use_sim(), torch.no_grad(), launch_records() as records:
        voc = make_vocoder(f"reduced{resblock}", "cpu", fused=fused)
        wav = voc(mel.transpose(1, 2), lengths=torch.tensor([6, 2], dtype=torch.int32) if ragged else None, precision=16)
    assert wav.shape == (2, 1, 6 * h.hop)
    runs = []
    for name, dims in records:
        if name.startswith(_PREP):
            continue
        rec = f"{name}[{dims}]"
        if runs and runs[-1][0] == rec:
            runs[-1][1] += 1
        else:
            runs.append([rec, 1])
    return " ".join(r if k == 1 else f"{k}x {r}" for r, k in runs)
