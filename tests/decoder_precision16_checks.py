"""Checks of the mel decoder at precision 16 (esmi_mel_decoder_prec_f32, esmi_phoneme2mel_forward_prec_f32, MelDecoder.forward(...,
precision=16), the input-dict key `decoder_precision`), shared by the GPU tier and the wave-simulator tier of
tests/test_decoder_precision16.py.  Every check takes the device ("cuda:0", or "cpu" inside `use_sim()`).

The yardstick is `mirror()`: a torch fp64 restatement of MelDecoder.forward with two modes -- exact, and rounded operands (at every
contraction of the decoder kernel the input through `.to(float16)`, the weight through round16(2^8 w) / 2^8).  E_q = rounded - exact is
the error any ideal binary16-operand implementation has; the kernels are held to it through their error e = kernel - exact (they cannot
match the rounded mirror closely: fp32 accumulation flips binary16 rounding boundaries of the next layer's operands).
"""
import ctypes as C
import dataclasses

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from efficientspeech_amd import CONFIGS, build_phoneme2mel, load_numpy_state_dict, networks
from efficientspeech_amd.networks import _on_device_of, _ptr
from efficientspeech_amd.synth import synth_phonemes, synth_state_dict
from tests import weight_profiles as WP

RMS_LO, RMS_HI, MAX_HI = 0.5, 1.25, 2.0       # rms(e) / rms(E_q) in [0.5, 1.25], max|e| / max|E_q| <= 2 (tests/test_vocoder_precision16.py's)


def config_of(name):
    """"tiny" / "small" / "base", or "<name>_k3": the same model with the reference class default's depthwise kernel 3"""
    if name.endswith("_k3"):
        return dataclasses.replace(CONFIGS[name[:-3]], name=name, decoder_kernel_size=3)
    return CONFIGS[name]


def state_dict_of(name, profile=None):
    cfg = config_of(name)
    sd = synth_state_dict(cfg, 1234)
    return cfg, (sd if profile is None else getattr(WP, profile)(cfg, sd))


_NETS = {}


def make_net(name, device, profile=None):
    """(net, cfg, sd); host nets are shared between the simulator tests (their pack caches follow the bound library)"""
    key = (name, profile, str(device))
    if key not in _NETS:
        cfg, sd = state_dict_of(name, profile)
        net = build_phoneme2mel(cfg)
        load_numpy_state_dict(net, sd)
        _NETS[key] = (net.to(device).eval(), cfg, sd)
    return _NETS[key]


# ---------------------------------------------------------------------------------------------------------------- the yardstick
def mirror(cfg, sd, feats, rounded, proj_rounded=None):
    """MelDecoder.forward (layers/networks.py:291-304) in fp64 on host tensors: feats (B, L, 4 dim) -> mel (B, L, n_mel); every Conv1d
    zero-pads outside [0, L).  rounded: at the pointwise convolutions, the mel Linear and (proj_rounded, default = rounded: the kernel
    runs the stage itself; False when it gathers a phoneme-rate h0, which the encoder side computes fp32-accurately) the proj Linear, the
    input goes through binary16 and the weight through round16(2^8 w) / 2^8.  Everything else is exact."""
    proj_rounded = rounded if proj_rounded is None else proj_rounded
    q = lambda t, on: t.to(torch.float16).to(torch.float64) if on else t                       # noqa: E731
    qw = lambda t, on: (t * 256.0).to(torch.float16).to(torch.float64) / 256.0 if on else t    # noqa: E731
    W = lambda key: torch.as_tensor(sd["decoder." + key]).to(torch.float64)                    # noqa: E731
    dx2, k = cfg.dx2, cfg.decoder_kernel_size
    ln = lambda t, pre: F.layer_norm(t, (dx2,), W(pre + ".weight"), W(pre + ".bias"), 1e-5)    # noqa: E731
    x = torch.as_tensor(feats).to(torch.float64)
    skip = ln(torch.tanh(F.linear(q(x, proj_rounded), qw(W("proj.0.weight"), proj_rounded), W("proj.0.bias"))), "proj.2")
    for b in range(cfg.n_blocks):
        x = skip
        for d in range(cfg.block_depth):
            pre = f"blocks.{b}.0.{d}"
            y = F.conv1d(x.transpose(1, 2), W(pre + ".0.0.weight"), W(pre + ".0.0.bias"), padding=k // 2, groups=dx2).transpose(1, 2)
            y = F.linear(q(y, rounded), qw(W(pre + ".0.1.weight")[:, :, 0], rounded), W(pre + ".0.1.bias"))
            x = ln(torch.tanh(y), pre + ".1")
        skip = ln(x + skip, f"blocks.{b}.1")
    return F.linear(q(skip, rounded), qw(W("mel_linear.weight"), rounded), W("mel_linear.bias"))


def rms(t):
    return float(t.to(torch.float64).pow(2).mean().sqrt())


def frame_features(feat, dur, L):
    """the length regulator on the host: phoneme-rate feat (B, T, C) + durations (B, T) -> (B, L, C), zero rows behind each utterance"""
    feat, dur = torch.as_tensor(feat).cpu(), torch.as_tensor(dur).cpu().long()
    out = torch.zeros((feat.shape[0], L, feat.shape[2]), dtype=feat.dtype)
    for b in range(feat.shape[0]):
        rows = torch.repeat_interleave(feat[b], dur[b], dim=0)[:L]
        out[b, :rows.shape[0]] = rows
    return out


class Yardsticks:
    """(exact, E_q) per case key: computed once, shared, never modified (a module-scoped fixture owns it)."""

    def __init__(self):
        self.runs = {}

    def get(self, key, cfg, sd, feats, proj_rounded=True, mel_len=None):
        if key not in self.runs:
            exact = mirror(cfg, sd, feats, False)
            eq = mirror(cfg, sd, feats, True, proj_rounded) - exact
            if mel_len is not None:                       # the final masked_fill: rows behind an utterance's end are zero in both
                keep = torch.arange(exact.shape[1])[None, :] < torch.as_tensor(mel_len).cpu().long()[:, None]
                exact, eq = exact * keep[..., None], eq * keep[..., None]
            self.runs[key] = (exact, eq)
        return self.runs[key]

    def clear(self):
        self.runs.clear()


def judge(what, mel16, exact, eq):
    """Test 1's verdict: e = mel16 - exact against E_q.  The lower bound proves that the one-product path ran (precision 32 sits three
    orders below E_q); the upper bounds catch a truncating conversion or a wrong plane."""
    assert mel16.dtype == torch.float32 and tuple(mel16.shape) == tuple(exact.shape)
    assert bool(torch.isfinite(mel16).all())
    e = mel16.cpu().to(torch.float64) - exact
    r_rms, r_max = rms(e) / rms(eq), float(e.abs().max()) / float(eq.abs().max())
    print(f"{what} {tuple(exact.shape)}: rms(e) {rms(e):.3e} = {r_rms:.3f} rms(E_q); max|e| {float(e.abs().max()):.3e} = {r_max:.3f} max|E_q|; "
          f"max|mel| {float(exact.abs().max()):.2f}")
    assert r_rms <= RMS_HI, r_rms
    assert r_max <= MAX_HI, r_max
    assert r_rms >= RMS_LO, r_rms
    return r_rms, r_max


def check_mirror_matches_oracle(name):
    """Test 0: the exact mode against oracle.mel_decoder (fp64) < 1e-6 L-inf -- three orders below E_q."""
    from oracle import oracle
    cfg, sd = state_dict_of(name)
    feats = np.random.default_rng(5).standard_normal((2, 37, cfg.d4)).astype(np.float32)
    ref = oracle.mel_decoder(cfg, oracle.Weights(sd), feats)
    exact = mirror(cfg, sd, feats, False)
    eq = mirror(cfg, sd, feats, True) - exact
    err = float((exact - torch.from_numpy(ref).double()).abs().max())
    print(f"{name}: mirror vs oracle L-inf {err:.2e}; E_q L-inf {float(eq.abs().max()):.2e} rms {rms(eq):.2e}")
    assert err < 1e-6, err
    assert rms(eq) > 1e-4                      # (the rounded mode rounds)


# ---------------------------------------------------------------------------------------------------------------- the C-ABI, driven directly
def run_decoder(net, cfg, feat, precision, cum=None, mel_len=None, h0=None, workspace=True, entry="prec", lib=None):
    """esmi_mel_decoder_prec_f32 (entry "prec") or esmi_mel_decoder_f32 ("plain") on a NaN-filled output and workspace: direct mode
    (cum None: feat (B, L, d4)) or the fused gather (feat (B, T, d4), cum, mel_len; the final mask applied) -> mel (B, L, n_mel)"""
    dec = net.decoder
    rt_lib, stream = networks._runtime(feat)
    lib = lib or rt_lib
    B = feat.shape[0]
    with _on_device_of(dec.mel_linear.weight), torch.no_grad():
        shape, blob = dec._shape(), dec._packed(rt_lib, stream)
        if cum is None:
            T, L = 0, feat.shape[1]
        else:
            T, L = feat.shape[1], int(mel_len.max())
        mel = torch.full((B, L, dec.n_mel_channels), float("nan"), dtype=torch.float32, device=feat.device)
        n = rt_lib.esmi_mel_decoder_workspace_bytes(C.byref(shape), B, L) if workspace else 0
        ws = torch.full((max(n // 4, 1),), float("nan"), dtype=torch.float32, device=feat.device) if n else None
        args = [_ptr(blob), C.byref(shape), _ptr(feat), _ptr(h0), _ptr(cum), _ptr(mel_len), None, L, 0 if cum is None else 1,
                B, T, L, _ptr(mel), _ptr(ws), n]
        if entry == "prec":
            lib.esmi_mel_decoder_prec_f32(*args, precision, stream)
        else:
            lib.esmi_mel_decoder_f32(*args, stream)
        if feat.is_cuda:
            torch.cuda.synchronize()
    return mel, n


def ragged_durations(B, T, D, device, seed=17):
    """durations in [1, D], utterance 1 cut short (padding frames, all-padding chunks) -> (dur, cum, mel_len) int32 on `device`"""
    dur = torch.from_numpy(np.random.default_rng(seed).integers(1, D + 1, size=(B, T)).astype(np.int32))
    if B > 1:
        dur[1, T // 2:] = 0
    cum = torch.cumsum(dur, 1).to(torch.int32).contiguous()
    return dur.to(device), cum.to(device), cum[:, -1].contiguous().to(device)


def check_direct(yard, name, B, L, device, profile=None):
    """Test 1, direct mode (the kernel runs its first stage itself: `proj` through mma_sub) through MelDecoder.forward(precision=16)."""
    net, cfg, sd = make_net(name, device, profile)
    feats = torch.from_numpy(np.random.default_rng(7).standard_normal((B, L, cfg.d4)).astype(np.float32))
    exact, eq = yard.get(("direct", name, profile, B, L), cfg, sd, feats)
    with torch.no_grad():
        mel16 = net.decoder(feats.to(device), precision=16)
        mel32 = net.decoder(feats.to(device))
    assert float((mel32.cpu().double() - exact).abs().max()) < 1e-4      # (the default is untouched by the call before it)
    return judge(f"{name}{'+' + profile if profile else ''} direct", mel16, exact, eq)


def check_chunk_walk(yard, name, B, T, D, device):
    """Test 1 + the chunk-walk invariant: the fused gather without h0 (in-kernel `proj`) with a workspace (dx2 = 256: the chunk walk) and
    without one (the window form), both at precision 16: each within the bounds, and the two agree to 2e-6 -- a kept row's operand values
    are the same values in both forms, so they round to the same binary16 (the bound of check_decoder_chunk_walk)."""
    net, cfg, sd = make_net(name, device)
    feat = torch.from_numpy(np.random.default_rng(17).standard_normal((B, T, cfg.d4)).astype(np.float32))
    dur, cum, mel_len = ragged_durations(B, T, D, device)
    L = int(mel_len.max())
    exact, eq = yard.get(("walk", name, B, T, D), cfg, sd, frame_features(feat, dur, L), mel_len=mel_len)
    outs = []
    for use_ws in (True, False):
        mel, n = run_decoder(net, cfg, feat.to(device), 16, cum, mel_len, workspace=use_ws)
        assert (n > 0) == (use_ws and cfg.dx2 == 256)
        judge(f"{name} fused gather, {'chunk walk' if n else 'window form'}", mel, exact, eq)
        outs.append(mel.cpu())
    d = float((outs[0] - outs[1]).abs().max())
    print(f"{name}: chunk walk vs window form at precision 16: L-inf {d:.2e}")
    assert d < 2e-6, d


def free_running_batch(device, T=42, lengths=(42, 27, 6), scale=None):
    """a ragged free-running batch for tiny ES: predicted durations (the synthetic weights predict about 3.6 frames per phoneme: the batch
    is about 150 frames long; `scale`: an optional duration_control)"""
    ids, mask = synth_phonemes(len(lengths), T, 7, list(lengths))
    x = {"phoneme": torch.from_numpy(ids).to(device), "phoneme_mask": torch.from_numpy(mask).to(device)}
    if scale is not None:
        x["duration_control"] = float(scale)
    return x


def check_forward_with_h0(yard, device, scale):
    """Test 1 + the invariants, tiny ES, the whole forward, free-running, B = 3 ragged, L ~ 150: the decoder gathers the phoneme-rate h0
    (two windows; edge rows outside [0, L); one utterance short enough to leave padding frames).
    Invariants: mel_len, duration, dur and cum bit-identical between precision 16 and 32; rows >= mel_len[b] exactly 0; precision 16
    twice the same bits; the key at 32 (the new entry point) the bits of the call without the key (the old entry points)."""
    net, cfg, sd = make_net("tiny", device)
    x = free_running_batch(device, scale=scale)
    with torch.no_grad():
        enc = net.encoder._encode(x)
        s32 = net._launch(x, taps=True)
        s16 = net._launch(dict(x, decoder_precision=16), taps=True)
        s16b = net._launch(dict(x, decoder_precision=16))
        s32k = net._launch(dict(x, decoder_precision=32))
    ml = s32.mel_len.cpu()
    L = int(ml.max())
    print(f"tiny free-running: mel_len {ml.tolist()}")
    assert 113 <= L <= 224 and int(ml.min()) < L - 20 and s16.mel.shape == (3, L, cfg.n_mel_channels)
    assert torch.equal(s16.mel_len, s32.mel_len) and torch.equal(s16.duration, s32.duration)
    for k in ("dur", "cum", "pitch_idx", "energy_idx"):
        assert torch.equal(s16.taps[k], s32.taps[k]), k
    assert torch.equal(s16.mel, s16b.mel) and torch.equal(s32k.mel, s32.mel) and not torch.equal(s16.mel, s32.mel)
    for b in range(3):
        assert not bool(s16.mel[b, int(ml[b]):].any()) and bool(s16.mel[b, :int(ml[b])].abs().sum() > 0)
    assert torch.equal(enc["dur"].cpu(), s32.taps["dur"].cpu())
    feats = frame_features(enc["feat"], s32.taps["dur"], L)
    exact, eq = yard.get(("fwd", "tiny", scale), cfg, sd, feats, proj_rounded=False, mel_len=ml)
    assert float((s32.mel.cpu().double() - exact).abs().max()) < 1e-4
    return judge("tiny forward, fused gather with h0", s16.mel, exact, eq)


def check_entry_points_at_32(name, device, B=2, T=12, D=5):
    """Precision 0 and 32 through esmi_mel_decoder_prec_f32 are esmi_mel_decoder_f32, bit for bit (fused gather, ragged)."""
    net, cfg, sd = make_net(name, device)
    feat = torch.from_numpy(np.random.default_rng(3).standard_normal((B, T, cfg.d4)).astype(np.float32)).to(device)
    _dur, cum, mel_len = ragged_durations(B, T, D, device)
    plain, _ = run_decoder(net, cfg, feat, 32, cum, mel_len, entry="plain")
    assert bool(torch.isfinite(plain).all())
    for precision in (0, 32):
        got, _ = run_decoder(net, cfg, feat, precision, cum, mel_len)
        assert torch.equal(got, plain), precision
    p16, _ = run_decoder(net, cfg, feat, 16, cum, mel_len)
    assert not torch.equal(p16, plain) and float((p16 - plain).abs().max()) < 0.1


def check_range_check_honours_the_key(device):
    """Phoneme2Mel.check_activation_range (the range-checked build; what ESMI_DEBUG_RANGE=1 runs first) with the key returns that build's
    precision-16 forward, bit for bit, not its precision-32 one.  Compared inside ONE build: the checked build's encoder side differs
    from the product build's by fp32 rounding (2e-6, at either precision), and at precision 16 such a difference crosses binary16
    rounding boundaries in the decoder -- two precision-16 mels from inputs 2e-6 apart are 1e-3 apart, a third of max|E_q| (measured;
    the decoder kernels of the two builds agree bit for bit on equal inputs).  The lower bound 1e-4 on the distance to precision 32 is
    30 times below max|E_q| and 100 times above fp32 noise."""
    import contextlib
    import os
    from efficientspeech_amd import _lib
    net, cfg, sd = make_net("tiny", device)
    ids, mask = synth_phonemes(2, 12, 3, [12, 6])
    x = {"phoneme": torch.from_numpy(ids).to(device), "phoneme_mask": torch.from_numpy(mask).to(device), "decoder_precision": 16}
    checked = os.path.join(os.path.dirname(_lib.LIB_PATH), "libesmi_checked.so")
    with torch.no_grad():
        with (_lib.use_library(checked) if str(device).startswith("cuda") else contextlib.nullcontext()):
            mel16, len16, _ = net(x)
            mel32, _len32, _ = net(dict(x, decoder_precision=32))
        got, got_len, _ = net.check_activation_range(x)
    d32 = float((got - mel32).abs().max())
    print(f"checked build with the key: L-inf to its precision-32 mel {d32:.2e}")
    assert torch.equal(got_len, len16) and torch.equal(got, mel16)
    assert d32 > 1e-4


# ---------------------------------------------------------------------------------------------------------------- launches, refusals (simulator)
_PREP = ("pack_", "absmax_kernel", "copy_pad_kernel")


def forward_records(name, extra, B=2, T=12):
    """the launch records of one inference forward on the simulator (weights packed before: preparation launches left out)"""
    from tests.simlib import launch_records
    net, cfg, sd = make_net(name, "cpu")
    ids, mask = synth_phonemes(B, T, 3, [T, T // 2])
    x = {"phoneme": torch.from_numpy(ids), "phoneme_mask": torch.from_numpy(mask),
         "duration_forced": torch.from_numpy(np.random.default_rng(2).integers(1, 4, size=(B, T)).astype(np.int32))}
    with torch.no_grad():
        if name not in _WARM:                    # (the first forward packs the weights)
            net(x)
            _WARM.add(name)
        with launch_records() as records:
            out = net(dict(x, **extra))
    return [r for r in records if not r[0].startswith(_PREP)], out


_WARM = set()


def check_dispatch(name, key32=True):
    """Test 3: a precision-16 forward's records differ from the precision-32 one's only in the decoder's name (`...,true>`): grid, block
    and LDS bytes identical, encoder-side records identical."""
    r32, _ = forward_records(name, {})
    r16, _ = forward_records(name, {"decoder_precision": 16})
    if key32:                                    # (the key at 32: the new entry point, the old launches)
        assert forward_records(name, {"decoder_precision": 32})[0] == r32
    assert len(r16) == len(r32) and r16[:-1] == r32[:-1]
    (n32, d32), (n16, d16) = r32[-1], r16[-1]
    assert n32 == "mel_decoder_kernel<DX2,KD,NW>" and n16 == "mel_decoder_kernel<DX2,KD,NW,true>", (n32, n16)
    assert d16 == d32
    assert sum(r[0].startswith("mel_decoder_kernel") for r in r16) == 1


def check_refusals():
    """Test 4 on the simulator: precision 8 is ESMI_ERR_ARG from both entry points and a ValueError from Python; the key with train=True
    is a ValueError; the launch log shows that nothing was enqueued in any of them."""
    from tests.simlib import launch_records
    net, cfg, sd = make_net("tiny", "cpu")
    feat = torch.from_numpy(np.random.default_rng(3).standard_normal((2, 9, cfg.d4)).astype(np.float32))
    run_decoder(net, cfg, feat, 32)                      # (weights packed: the records below are the calls' alone)
    ids, mask = synth_phonemes(2, 9, 1, [9, 4])
    x = {"phoneme": torch.from_numpy(ids), "phoneme_mask": torch.from_numpy(mask)}
    with torch.no_grad():
        net(x)
    with launch_records() as records:
        with pytest.raises(RuntimeError, match="esmi_mel_decoder_prec_f32 failed: ESMI_ERR_ARG"):
            run_decoder(net, cfg, feat, 8)
        for bad in (8, 0, "16", True):
            with pytest.raises(ValueError, match="precision"), torch.no_grad():
                net(dict(x, decoder_precision=bad))
        with pytest.raises(ValueError, match="precision"), torch.no_grad():
            net.decoder(feat, precision=8)
        xt = dict(x, decoder_precision=16, pitch=torch.zeros((2, 9)), energy=torch.zeros((2, 9)),
                  duration=torch.ones((2, 9), dtype=torch.int32), mel_len=torch.tensor([9, 4], dtype=torch.int32))
        with pytest.raises(ValueError, match="decoder_precision"), torch.no_grad():
            net(xt, train=True)
        # the whole-forward entry point itself: precision 8 is refused before the encoder side is enqueued
        a = net._static_args(*networks._runtime(net.decoder.mel_linear.weight))
        lib, stream = networks._runtime(net.decoder.mel_linear.weight)
        with pytest.raises(RuntimeError, match="esmi_phoneme2mel_forward_prec_f32 failed: ESMI_ERR_ARG"):
            lib.esmi_phoneme2mel_forward_prec_f32(C.byref(a), None, 8, 0, stream)
    assert records == []


def check_fp32mfma_refuses(lib_path):
    """Test 4: libesmi_fp32mfma.so has no binary16 products: precision 16 is ESMI_ERR_UNSUPPORTED from both entry points, decided on the
    host before anything is enqueued (no device is touched: this runs without a GPU)."""
    from efficientspeech_amd import _lib
    lib = _lib.bind(C.CDLL(lib_path))
    assert lib.esmi_build_config().decode().startswith("dec_gemm=fp32-mfma")
    shape = _lib.DecoderShape(128, 128, 5, 2, 2, 80)
    buf = (C.c_float * 64)()                             # aligned stand-ins: a refused call reads none of them
    p = C.cast(C.byref(buf), C.c_void_p)
    with pytest.raises(_lib.Unsupported):
        lib.esmi_mel_decoder_prec_f32(p, C.byref(shape), p, None, None, None, None, 4, 0, 1, 0, 4, p, None, 0, 16, None)
    with pytest.raises(RuntimeError, match="ESMI_ERR_ARG"):
        lib.esmi_mel_decoder_prec_f32(p, C.byref(shape), p, None, None, None, None, 4, 0, 1, 0, 4, p, None, 0, 8, None)
    a = _lib.ForwardArgs()
    with pytest.raises(_lib.Unsupported):
        lib.esmi_phoneme2mel_forward_prec_f32(C.byref(a), None, 16, 0, None)


# ---------------------------------------------------------------------------------------------------------------- wrappers
def check_wrappers(device):
    """Test 5, first half: EfficientSpeech.synthesize(decoder_precision=16) is hifigan(mel16) -- the vocoder's own precision untouched;
    the attribute is the default and the key overrides it; tiny ES + v2, B = 3, T = 12, forced durations."""
    from efficientspeech_amd import EfficientSpeech
    from tests.vocoder_precision16_checks import make_vocoder
    voc = make_vocoder("v2", device)
    model = EfficientSpeech.from_config("tiny", hifigan=voc)
    model.phoneme2mel.load_state_dict({k: torch.from_numpy(v) for k, v in synth_state_dict(CONFIGS["tiny"], 1234).items()}, strict=True)
    model = model.to(device).eval()
    B, T, lens = 3, 12, [12, 7, 3]
    ids, mask = synth_phonemes(B, T, 12, lens)
    dur = np.random.default_rng(3).integers(1, 4, size=(B, T)).astype(np.int32)
    dur[mask] = 0
    x = {"phoneme": torch.from_numpy(ids).to(device), "phoneme_mask": torch.from_numpy(mask).to(device),
         "duration_forced": torch.from_numpy(dur).to(device)}
    with torch.no_grad():
        mel32, len32, _ = model.phoneme2mel(x, train=False)
        mel16, len16, _ = model.phoneme2mel(dict(x, decoder_precision=16), train=False)
        assert model.phoneme2mel.decoder.precision == 32
        wav16, wlen16, _ = model.synthesize(x, decoder_precision=16)
        wav32, wlen32, _ = model.synthesize(x)
        ref16 = voc(mel16.transpose(1, 2), lengths=len16)[:, 0]
        with pytest.raises(ValueError, match="precision"):
            model.synthesize(x, decoder_precision=8)
        model.phoneme2mel.decoder.precision = 16                   # the attribute is the default; the key overrides it
        try:
            assert "precision" not in " ".join(model.phoneme2mel.decoder.state_dict())
            assert torch.equal(model.phoneme2mel(x, train=False)[0], mel16)
            assert torch.equal(model.phoneme2mel(dict(x, decoder_precision=32), train=False)[0], mel32)
        finally:
            model.phoneme2mel.decoder.precision = 32
    assert torch.equal(len16, len32) and torch.equal(wlen16, wlen32) and not torch.equal(mel16, mel32)
    assert torch.equal(wav16, ref16) and not torch.equal(wav16, wav32)


def _forced_batch(device, B=3, T=12, lens=(12, 7, 3)):
    ids, mask = synth_phonemes(B, T, 12, list(lens))
    dur = np.random.default_rng(3).integers(1, 4, size=(B, T)).astype(np.int32)
    dur[mask] = 0
    x = {"phoneme": torch.from_numpy(ids).to(device), "phoneme_mask": torch.from_numpy(mask).to(device),
         "duration_forced": torch.from_numpy(dur).to(device)}
    return ids, dur, x


def check_scheduler(device):
    """Test 5, second half (no vocoder): a BucketedSynthesizer whose `extra` adds the key gives the direct precision-16 call's mels, bit
    for bit, and not the precision-32 ones; tiny ES, three requests of 12 / 7 / 3 phonemes, forced durations."""
    from efficientspeech_amd import BucketedSynthesizer
    net, cfg, sd = make_net("tiny", device)
    lens = [12, 7, 3]
    ids, dur, _x = _forced_batch(device, lens=lens)
    seqs = [ids[b, :n].astype(np.int32) for b, n in enumerate(lens)]

    def extra(idx, T_):
        d = np.zeros((len(idx), T_), np.int32)
        for r, i in enumerate(idx):
            d[r, :lens[i]] = dur[i, :lens[i]]
        return {"duration_forced": torch.from_numpy(d).to(device), "decoder_precision": 16}
    res = BucketedSynthesizer(net, max_batch=1, granularity=4)(seqs, extra=extra)
    for i, (mel_i, _dur_i) in enumerate(res):
        xi = {"phoneme": torch.from_numpy(seqs[i][None]).to(device), "duration_forced": torch.from_numpy(dur[i:i + 1, :lens[i]]).to(device)}
        with torch.no_grad():
            alone16 = net(dict(xi, decoder_precision=16))[0][0]
            alone32 = net(xi)[0][0]
        assert mel_i.shape == (int(dur[i, :lens[i]].sum()), 80) and torch.equal(mel_i, alone16) and not torch.equal(mel_i, alone32), i


def check_staged_forward(device):
    """The key through the staged calls that sharded_forward / ShardedMelPipeline make (`_launch(stage=1)`, then `_launch(stage=2)` on
    the returned state: the state carries the precision) and through a ShardedMelPipeline step: the one-call forward's precision-16
    bits, with and without a caller-supplied output length; and the decoder's attribute as the default of the same paths."""
    from efficientspeech_amd.sharded import ShardedMelPipeline
    net, cfg, sd = make_net("tiny", device)
    _ids, dur, x = _forced_batch(device)
    x16 = dict(x, decoder_precision=16)
    with torch.no_grad():
        one16, one32 = net._launch(x16), net._launch(x)
        assert not torch.equal(one16.mel, one32.mel)
        for more in ({}, {"max_mel_len": int(dur.sum(1).max()) + 5}):
            ref = one16.mel if not more else net._launch(dict(x16, **more)).mel
            st = net._launch(dict(x16, **more), stage=1)
            assert st.precision == 16 and st.mel is None
            st = net._launch(None, stage=2, state=st)
            assert torch.equal(st.mel, ref) and torch.equal(st.mel_len, one32.mel_len), more
        mel, mel_len = ShardedMelPipeline(net).step(x16)
        assert torch.equal(mel, one16.mel) and torch.equal(mel_len, one32.mel_len)
        net.decoder.precision = 16
        try:
            st = net._launch(None, stage=2, state=net._launch(x, stage=1))
            assert torch.equal(st.mel, one16.mel)
            st = net._launch(None, stage=2, state=net._launch(dict(x, decoder_precision=32), stage=1))
            assert torch.equal(st.mel, one32.mel)
        finally:
            net.decoder.precision = 32


def check_train_forward_ignores_the_attribute(device):
    """`train=True` runs the decoder at precision 32 whatever `decoder.precision` says (the attribute is inference's default)."""
    net, cfg, sd = make_net("tiny", device)
    ids, mask = synth_phonemes(2, 9, 1, [9, 4])
    dur = np.random.default_rng(4).integers(1, 4, size=(2, 9)).astype(np.int32)
    dur[mask] = 0
    xt = {"phoneme": torch.from_numpy(ids).to(device), "phoneme_mask": torch.from_numpy(mask).to(device),
          "pitch": torch.zeros((2, 9), device=device), "energy": torch.zeros((2, 9), device=device),
          "duration": torch.from_numpy(dur).to(device), "mel_len": torch.from_numpy(dur.sum(1).astype(np.int32)).to(device)}
    with torch.no_grad():
        ref = net(xt, train=True)["mel"]
        net.decoder.precision = 16
        try:
            got = net(xt, train=True)["mel"]
        finally:
            net.decoder.precision = 32
    assert torch.equal(got, ref) and float(ref.abs().max()) > 0.1


def check_graph_replay(device):
    """The graph-replay path (GPU only): GraphedForward / ShardedMelPipeline(use_graph=True) capture the decoder at the precision the
    first batch asks for -- the eager precision-16 bits -- and refuse a later step that asks for another one; nothing is dropped."""
    from efficientspeech_amd.sharded import GraphedForward, ShardedMelPipeline, _encode_with_head
    net, cfg, sd = make_net("tiny", device)
    _ids, dur, x = _forced_batch(device)
    x = dict(x, max_mel_len=int(dur.sum(1).max()))
    x16 = dict(x, decoder_precision=16)
    L = x["max_mel_len"]

    def eager(precision):                             # the two calls the graphs capture, run eagerly
        enc = _encode_with_head(net, x)
        return net.decoder._fused(enc["feat"], enc["cum"], enc["mel_len"], enc["lmax"], L, True, L, h0=enc["h0"], precision=precision)
    with torch.no_grad():
        ref16, ref32 = eager(16), eager(32)
        assert not torch.equal(ref16, ref32)
        pipe = ShardedMelPipeline(net, use_graph=True)
        mel, _len = pipe.step(x16)
        torch.cuda.synchronize()
        assert pipe.graphed is not None and pipe.graphed.precision == 16
        assert torch.equal(mel, ref16) and not torch.equal(mel, ref32)
        for bad in (x, dict(x, decoder_precision=32)):
            with pytest.raises(NotImplementedError, match="decoder_precision"):
                pipe.step(bad)
        g = GraphedForward(net, x)
        assert g.precision == 32
        g.load(x)
        g.encode()
        mel32 = g.decode()
        torch.cuda.synchronize()
        assert torch.equal(mel32, ref32)
        with pytest.raises(NotImplementedError, match="decoder_precision"):
            g.load(x16)
        net.decoder.precision = 16                    # the attribute changed behind a captured graph: refused too
        try:
            with pytest.raises(NotImplementedError, match="decoder_precision"):
                g.load(x)
        finally:
            net.decoder.precision = 32
    with pytest.raises(ValueError, match="precision"):
        GraphedForward(net, dict(x, decoder_precision=8))
