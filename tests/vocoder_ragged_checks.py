"""Checks of the length-aware HiFi-GAN generator (esmi_hifigan_generator_ragged_f32), shared by the GPU tier and the wave-simulator
tier of tests/test_vocoder_ragged.py.  Every check takes the device ("cuda:0", or "cpu" inside `use_sim()`).

The C-ABI is driven directly where the state of the workspace matters: workspace and outputs are test-owned and filled with NaN before
the length-aware call.  With a caching allocator a margin one frame short would otherwise read the previous run's (correct) values out
of a recycled block and pass.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from efficientspeech_amd import networks
from efficientspeech_amd.hifigan import HIFIGAN_CONFIGS, Generator, ragged_margins, synth_hifigan_state_dict
from efficientspeech_amd.networks import _on_device_of, _ptr


def make_vocoder(config, device, post_bias=0.0, fused=True):
    h = HIFIGAN_CONFIGS[config]
    sd = {k: torch.from_numpy(v) for k, v in synth_hifigan_state_dict(h, 1234).items()}
    if post_bias:
        sd["conv_post.bias"] = sd["conv_post.bias"] + post_bias
    voc = Generator(h)
    voc.load_state_dict(sd, strict=True)
    voc = voc.to(device).eval()
    voc.fuse_resblocks = fused
    return voc


def make_mel(h, B, L, device, seed=5):
    """randn * 2 - 4, as test_hifigan_one_launch_resblocks_match_conv_by_conv (host generator: the same values on both tiers)."""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn((B, L, h.num_mels), generator=g) * 2 - 4).to(device)


def run_abi(voc, mel, lengths=None, want_wav=True, want_pcm=False):
    """One C-ABI call on test-owned, NaN-filled workspace and outputs.  lengths None: esmi_hifigan_generator_f32.
    -> (wav (B, L * hop) float or None, pcm int16 or None)"""
    wt = voc.conv_post.weight
    lib, stream = networks._runtime(wt)
    B, L, _ = mel.shape
    n = L * voc.h.hop
    with _on_device_of(wt), torch.no_grad():
        w, s, _keep = voc._packed(lib, stream)
        nbytes = lib.esmi_hifigan_workspace_bytes(C.byref(s), B, L)
        assert nbytes > 0 and nbytes % 4 == 0
        ws = torch.full((nbytes // 4,), float("nan"), dtype=torch.float32, device=mel.device)
        wav = torch.full((B, n), float("nan"), dtype=torch.float32, device=mel.device) if want_wav else None
        pcm = torch.full((B, n), -12345, dtype=torch.int16, device=mel.device) if want_pcm else None
        if lengths is None:
            lib.esmi_hifigan_generator_f32(C.byref(w), C.byref(s), _ptr(mel), B, L, _ptr(wav), _ptr(ws), nbytes, stream)
        else:
            ln = torch.as_tensor(lengths, dtype=torch.int32).to(mel.device)
            lib.esmi_hifigan_generator_ragged_f32(C.byref(w), C.byref(s), _ptr(mel), B, L, _ptr(ln), _ptr(wav), _ptr(pcm), _ptr(ws),
                                                  nbytes, stream)
        if mel.is_cuda:
            torch.cuda.synchronize()
    return wav, pcm


def assert_kept_and_tails(got, full, lengths, hop, what=""):
    """samples < len * hop: the full run's, bit for bit; samples >= len * hop: exactly zero (so: not NaN)."""
    L = full.shape[1] // hop
    for b, ln in enumerate(lengths):
        k = min(max(int(ln), 0), L) * hop
        assert torch.equal(got[b, :k], full[b, :k]), f"{what} row {b} (len {ln}): kept samples differ from the full run"
        assert not bool(torch.isnan(got[b, k:]).any()), f"{what} row {b} (len {ln}): NaN in the tail"
        assert int(torch.count_nonzero(got[b, k:])) == 0, f"{what} row {b} (len {ln}): tail is not exactly zero"
    assert bool(torch.isfinite(full).all())


class PlainRuns:
    """The plain esmi_hifigan_generator_f32 runs the checks compare against: (vocoder, mel, waveform) per shape, computed once, shared
    and never modified.  Owned by a module-scoped fixture of the test file, which clears it when the module is done."""

    def __init__(self):
        self.runs = {}

    def get(self, config, B, L, device, fused=True):
        key = (config, B, L, str(device), fused)
        if key not in self.runs:
            voc = make_vocoder(config, device, fused=fused)
            mel = make_mel(voc.h, B, L, device)
            full, _ = run_abi(voc, mel)
            assert float(full.abs().max()) > 1e-3                   # a real signal
            self.runs[key] = (voc, mel, full)
        return self.runs[key]

    def clear(self):
        self.runs.clear()


def check_kept_bit_identical(runs, config, B, L, lengths, device, modes=(True, False)):
    """Test 1: kept samples are the full run's bit for bit, tails are zero, nothing stale is read (NaN-filled workspace / output)."""
    for fused in modes:
        voc, mel, full = runs.get(config, B, L, device, fused)
        got, _ = run_abi(voc, mel, lengths)
        assert_kept_and_tails(got, full, lengths, voc.h.hop, f"{config} fused={fused}")


def check_full_lengths_identity(runs, config, B, L, device, fused=True, module_plain=True):
    """Test 4: `lengths = full((B,), L)` through Generator.forward equals forward(x) bit for bit.  (module_plain False: the plain
    waveform is the shared esmi_hifigan_generator_f32 run alone -- the simulator tier does not pay for a second plain forward.)"""
    voc, mel, full = runs.get(config, B, L, device, fused)
    with torch.no_grad():
        b = voc(mel.transpose(1, 2), lengths=torch.full((B,), L, dtype=torch.int32, device=mel.device))
        if module_plain:
            assert torch.equal(voc(mel.transpose(1, 2))[:, 0], full)
    assert b.shape == (B, 1, L * voc.h.hop) and b.dtype == torch.float32
    assert torch.equal(b[:, 0], full)


def check_oracle(device):
    """Test 2: kept samples against the C oracle's generator on the same padded mel."""
    from oracle import oracle
    voc = make_vocoder("v2", device)
    B, L, lengths = 3, 40, [40, 21, 6]
    mel = make_mel(voc.h, B, L, device)
    got, _ = run_abi(voc, mel, lengths)
    vsd = synth_hifigan_state_dict(voc.h, 1234)
    ref = oracle.hifigan(voc.h, oracle.Weights(vsd), mel.cpu().numpy())
    got = got.cpu().numpy()
    for b, ln in enumerate(lengths):
        k = ln * voc.h.hop
        err = float(np.abs(got[b, :k] - ref[b, :k]).max())
        print(f"row {b} len {ln}: L-inf vs oracle {err:.3e}")
        assert err < 2e-4, (b, err)
        assert not got[b, k:].any()


def check_margin_is_tight(device):
    """Test 3: the mel rows from len + margin_frames on reach no kept sample (a condition on the margin the library claims; with
    test 1 it pins the margin between 'too short' and 'unused')."""
    voc = make_vocoder("v2", device)
    B, L, lengths = 4, 64, [64, 33, 9, 0]
    margin = ragged_margins(voc.h)[1]
    assert margin == 13                                             # v2: 3 (conv_pre) + 10 frames behind the first ConvTranspose
    mel = make_mel(voc.h, B, L, device)
    other = mel.clone()
    g = torch.Generator().manual_seed(11)
    for b, ln in enumerate(lengths):
        if ln + margin < L:
            other[b, ln + margin:] = (torch.randn((L - ln - margin, voc.h.num_mels), generator=g) * 3 + 1).to(device)
    assert not torch.equal(other[2], mel[2])
    a, _ = run_abi(voc, mel, lengths)
    b_, _ = run_abi(voc, other, lengths)
    assert torch.equal(a, b_)


def check_edges(device):
    """Test 4: clamping, empty batches of lengths, the short shapes, NULL arguments."""
    voc = make_vocoder("v2", device)
    hop = voc.h.hop
    mel = make_mel(voc.h, 3, 7, device)
    full, _ = run_abi(voc, mel)
    got, _ = run_abi(voc, mel, [7, 3, 0])
    assert_kept_and_tails(got, full, [7, 3, 0], hop, "L = 7")
    over, _ = run_abi(voc, mel, [12, 7 + 2 ** 20, 8])               # above L: clamp to L
    assert torch.equal(over, full)
    neg, _ = run_abi(voc, mel, [-1, -2 ** 31, 2])                   # negative: clamp to 0
    assert_kept_and_tails(neg, full, [0, 0, 2], hop, "negative")
    zero, _ = run_abi(voc, mel, [0, 0, 0])
    assert not bool(torch.isnan(zero).any()) and int(torch.count_nonzero(zero)) == 0
    mel1 = make_mel(voc.h, 1, 1, device, seed=6)
    full1, _ = run_abi(voc, mel1)
    got1, _ = run_abi(voc, mel1, [1])
    assert torch.equal(got1, full1) and float(full1.abs().max()) > 0
    # the module: shapes, dtypes, any integer dtype for the lengths
    with torch.no_grad():
        y = voc(mel.transpose(1, 2), lengths=torch.tensor([7, 3, 0], device=mel.device))
        p = voc(mel.transpose(1, 2), lengths=torch.tensor([7, 3, 0], dtype=torch.int32, device=mel.device), pcm16=True)
        p_all = voc(mel.transpose(1, 2), pcm16=True)               # no lengths: every utterance is L frames long
    assert y.shape == p.shape == (3, 1, 7 * hop) and y.dtype == torch.float32 and p.dtype == torch.int16
    assert torch.equal(y[:, 0], got)
    assert torch.equal(p[:, 0], (got * 32768).clamp(-32768, 32767).trunc().to(torch.int16))
    assert p_all.dtype == torch.int16 and torch.equal(p_all[:, 0], (full * 32768).clamp(-32768, 32767).trunc().to(torch.int16))
    # ESMI_ERR_ARG: no output plane, no lengths
    with pytest.raises(RuntimeError, match="esmi_hifigan_generator_ragged_f32"):
        run_abi(voc, mel, [7, 3, 0], want_wav=False, want_pcm=False)
    lib, stream = networks._runtime(voc.conv_post.weight)
    w, s, _keep = voc._packed(lib, stream)
    nbytes = lib.esmi_hifigan_workspace_bytes(C.byref(s), 3, 7)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=mel.device)
    with pytest.raises(RuntimeError, match="esmi_hifigan_generator_ragged_f32"):
        lib.esmi_hifigan_generator_ragged_f32(C.byref(w), C.byref(s), _ptr(mel), 3, 7, None, _ptr(full.clone()), None, _ptr(ws), nbytes, stream)


def check_pcm(device):
    """Test 5: the int16 plane is trunc(clamp(wav * 32768)) of the float plane of the same call, zeros in the tails; full scale
    clamps to 32767 (the reference's numpy cast would wrap it)."""
    lengths = [24, 5, 0]
    voc = make_vocoder("v2", device)
    mel = make_mel(voc.h, 3, 24, device)
    wav, pcm = run_abi(voc, mel, lengths, want_pcm=True)
    assert torch.equal(pcm, (wav * 32768).clamp(-32768, 32767).trunc().to(torch.int16))
    assert int(pcm.abs().max()) > 30                                # a real signal
    only, _p = run_abi(voc, mel, lengths, want_wav=False, want_pcm=True)
    assert only is None and torch.equal(_p, pcm)
    for b, ln in enumerate(lengths):
        assert int(torch.count_nonzero(pcm[b, ln * voc.h.hop:])) == 0
    sat = make_vocoder("v2", device, post_bias=20.0)                # conv_post + 20: tanh == 1.0f on every kept sample
    wav, pcm = run_abi(sat, mel, lengths, want_pcm=True)
    k = 5 * voc.h.hop
    assert bool((wav[0] == 1.0).all()) and bool((wav[1, :k] == 1.0).all())
    assert bool((pcm[0] == 32767).all()) and bool((pcm[1, :k] == 32767).all())
    assert int(torch.count_nonzero(pcm[1, k:])) == 0 and int(torch.count_nonzero(pcm[2])) == 0
    neg = make_vocoder("v2", device, post_bias=-20.0)
    wav, pcm = run_abi(neg, mel, lengths, want_pcm=True)
    assert bool((pcm[0] == -32768).all())


def check_wrapper_and_scheduler(device):
    """Test 6: EfficientSpeech.synthesize and BucketedSynthesizer(net, vocoder=voc) on tiny ES + v2, ragged phoneme lengths and forced
    durations, against predict_step on the same padded batches."""
    from efficientspeech_amd import BucketedSynthesizer, EfficientSpeech
    from efficientspeech_amd.synth import synth_phonemes, synth_state_dict
    from efficientspeech_amd.config import CONFIGS
    voc = make_vocoder("v2", device)
    hop = voc.h.hop
    model = EfficientSpeech.from_config("tiny", hifigan=voc)
    model.phoneme2mel.load_state_dict({k: torch.from_numpy(v) for k, v in synth_state_dict(CONFIGS["tiny"], 1234).items()}, strict=True)
    model = model.to(device).eval()
    rng = np.random.default_rng(3)
    B, T, plens = 3, 20, [20, 13, 4]
    ids, mask = synth_phonemes(B, T, 12, plens)
    dur = rng.integers(1, 4, size=(B, T)).astype(np.int32)
    x = {"phoneme": torch.from_numpy(ids).to(device), "phoneme_mask": torch.from_numpy(mask).to(device),
         "duration_forced": torch.from_numpy(dur).to(device)}
    with torch.no_grad():
        ref, mel_len, _ = model.predict_step(x)
        wav, wav_len, duration = model.synthesize(x)
        pcm, _, _ = model.synthesize(x, pcm16=True)
    ml = mel_len.cpu().numpy()
    assert len(set(ml.tolist())) == B and wav.shape == ref.shape == (B, int(ml.max()) * hop)
    assert np.array_equal(wav_len.cpu().numpy(), ml * hop) and duration.shape[:2] == (B, T)
    assert_kept_and_tails(wav, ref, ml, hop, "synthesize")
    assert pcm.dtype == torch.int16 and torch.equal(pcm, (wav * 32768).clamp(-32768, 32767).trunc().to(torch.int16))
    model.hifigan = None
    with pytest.raises(RuntimeError, match="vocoder"):
        model.synthesize(x)
    model.hifigan = voc
    # the scheduler: per request a waveform trimmed to mel_len_i * hop = the row of a plain padded predict_step of its bucket
    lens = [9, 9, 5, 9, 5, 12, 11, 3]
    seqs = [rng.integers(1, 150, size=n).astype(np.int32) for n in lens]
    forced = {i: rng.integers(1, 4, size=n).astype(np.int32) for i, n in enumerate(lens)}

    def extra(idx, T):
        d = np.zeros((len(idx), T), np.int32)
        for r, i in enumerate(idx):
            d[r, :lens[i]] = forced[i]
        return {"duration_forced": torch.from_numpy(d).to(device)}
    sched = BucketedSynthesizer(model.phoneme2mel, max_batch=3, granularity=4, vocoder=voc)
    res = sched(seqs, extra=extra)
    plain = BucketedSynthesizer(model.phoneme2mel, max_batch=3, granularity=4)(seqs, extra=extra)
    assert len(res) == len(plain) == len(lens) and all(len(r) == 3 for r in res) and all(len(r) == 2 for r in plain)
    for idx, T in sched.plan(lens):
        ids_b = np.zeros((len(idx), T), np.int32)
        for r, i in enumerate(idx):
            ids_b[r, :lens[i]] = seqs[i]
        xb = {"phoneme": torch.from_numpy(ids_b).to(device)}
        if len(idx) > 1:
            xb["phoneme_mask"] = torch.from_numpy(np.arange(T)[None, :] >= np.array([lens[i] for i in idx])[:, None]).to(device)
        xb.update(extra(idx, T))
        with torch.no_grad():
            wb, mlb, _ = model.predict_step(xb)
        for r, i in enumerate(idx):
            n = int(forced[i].sum())
            wav_i, mel_i, dur_i = res[i]
            assert int(mlb[r]) == n and wav_i.shape == (n * hop,) and mel_i.shape == (n, 80) and dur_i.shape == (lens[i],)
            assert torch.equal(wav_i, wb[r, :n * hop])
            assert torch.equal(mel_i, plain[i][0])
