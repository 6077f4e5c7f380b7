"""Checks of inference at bf16 (precision = ESMI_PRECISION_BF16 in esmi_mel_decoder_prec_f32, esmi_phoneme2mel_forward_prec_f32 / _curve_f32
and esmi_hifigan_generator_prec_f32; `precision="bf16"` in MelDecoder, Generator, the key `decoder_precision`, synthesize()), shared by the
GPU tier and the wave-simulator tier of tests/test_inference_bf16.py.  Every check takes the device ("cuda:0", or "cpu" inside `use_sim()`).

The yardsticks are the fp64 mirrors of the precision-16 suites with a bf16 mode: at every contraction of the contract (include/esmi.h,
"Inference at bf16") the input goes through `.to(torch.bfloat16)` and the weight through the rule of its kernel family -- RNE bfloat16 of
(plane0 + plane1) * 2^-8 of the two-plane binary16 blob for the fused kernels (mel decoder, one-launch ResBlocks), bfloat16(w) for the
per-convolution launches; everything else is exact.  E_q = rounded - exact, e = kernel - exact, and the verdict is the project's band:
rms(e) / rms(E_q) in [0.5, 1.25], max|e| / max|E_q| <= 2.  E_q(bf16) is about 2^3 times E_q(f16), so the precision-16 path and the default
path both fall below the lower bound: it is what proves that the bf16 product ran.
"""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from efficientspeech_amd import _lib, networks
from efficientspeech_amd.hifigan import Generator, synth_hifigan_state_dict
from tests import decoder_precision16_checks as D
from tests import vocoder_precision16_checks as VV
from tests.vocoder_ragged_checks import assert_kept_and_tails, make_mel

BF = "bf16"
BF_CODE = _lib.PRECISION_BF16
RMS_LO, RMS_HI, MAX_HI = D.RMS_LO, D.RMS_HI, D.MAX_HI      # [0.5, 1.25] and 2: the band of both precision-16 suites
rms = D.rms


# ---------------------------------------------------------------------------------------------------------------- the operand rules
def q_bf16(t):
    """an activation operand: RNE bfloat16 (fp64 in, fp64 out; the kernels round an fp32 value, the mirror's fp64 one -- the difference
    is a boundary case far below E_q)"""
    return t.to(torch.float32).to(torch.bfloat16).to(torch.float64)


def w_bf16(w):
    """the per-convolution launches' weight operand: RNE bfloat16 of the fp32 weight"""
    return torch.as_tensor(w, dtype=torch.float32).to(torch.bfloat16).to(torch.float64)


def w_two_plane(w):
    """the fused kernels' weight operand: RNE bfloat16 of (plane0 + plane1) * 2^-8, the planes being the nearest binary16 of 2^8 w and of
    its residual (what the packers write); the sum is exact in fp32"""
    x = torch.as_tensor(w, dtype=torch.float32) * 256.0
    h1 = x.to(torch.float16).to(torch.float32)
    h2 = (x - h1).to(torch.float16).to(torch.float32)
    return ((h1 + h2) / 256.0).to(torch.bfloat16).to(torch.float64)


def check_rules_agree_almost_everywhere():
    """the two weight rules differ on about one weight in 2^13, by one bfloat16 ulp (include/esmi.h says so): on 2^20 normal weights
    fewer than 2^20 / 2^11 differ, and none by more than one ulp"""
    w = torch.from_numpy(np.random.default_rng(0).standard_normal(1 << 20).astype(np.float32) * 0.1)
    a, b = w_bf16(w), w_two_plane(w)
    differ = a != b
    assert int(differ.sum()) < (1 << 9), int(differ.sum())
    ulp = torch.ldexp(torch.ones_like(a), torch.floor(torch.log2(a.abs().clamp_min(1e-30))) - 7)
    assert bool(((a - b).abs() <= ulp * 1.0001)[differ].all())


# ---------------------------------------------------------------------------------------------------------------- decoder yardstick
def dec_mirror(cfg, sd, feats, rounded, proj_rounded=None, stats=None):
    """tests/decoder_precision16_checks.mirror with the bf16 rules: every contraction of the decoder kernel rounds its input through
    bfloat16 and takes the two-plane weight.  stats (a dict): receives "operand_max", the largest |input| of a rounded contraction."""
    proj_rounded = rounded if proj_rounded is None else proj_rounded

    def q(t, on):
        if on and stats is not None:
            stats["operand_max"] = max(stats.get("operand_max", 0.0), float(t.abs().max()))
        return q_bf16(t) if on else t
    qw = lambda key, on: w_two_plane(sd["decoder." + key]) if on else W(key)                   # noqa: E731
    W = lambda key: torch.as_tensor(sd["decoder." + key]).to(torch.float64)                    # noqa: E731
    dx2, k = cfg.dx2, cfg.decoder_kernel_size
    ln = lambda t, pre: F.layer_norm(t, (dx2,), W(pre + ".weight"), W(pre + ".bias"), 1e-5)    # noqa: E731
    x = torch.as_tensor(feats).to(torch.float64)
    skip = ln(torch.tanh(F.linear(q(x, proj_rounded), qw("proj.0.weight", proj_rounded), W("proj.0.bias"))), "proj.2")
    for b in range(cfg.n_blocks):
        x = skip
        for d in range(cfg.block_depth):
            pre = f"blocks.{b}.0.{d}"
            y = F.conv1d(x.transpose(1, 2), W(pre + ".0.0.weight"), W(pre + ".0.0.bias"), padding=k // 2, groups=dx2).transpose(1, 2)
            y = F.linear(q(y, rounded), qw(pre + ".0.1.weight", rounded)[:, :, 0], W(pre + ".0.1.bias"))
            x = ln(torch.tanh(y), pre + ".1")
        skip = ln(x + skip, f"blocks.{b}.1")
    return F.linear(q(skip, rounded), qw("mel_linear.weight", rounded), W("mel_linear.bias"))


class DecYard:
    """(exact, E_q, stats) per case key: computed once, shared, never modified (a module-scoped fixture owns it)"""

    def __init__(self):
        self.runs = {}

    def get(self, key, cfg, sd, feats, proj_rounded=True, mel_len=None):
        if key not in self.runs:
            stats = {}
            exact = dec_mirror(cfg, sd, feats, False)
            eq = dec_mirror(cfg, sd, feats, True, proj_rounded, stats) - exact
            if mel_len is not None:
                keep = torch.arange(exact.shape[1])[None, :] < torch.as_tensor(mel_len).cpu().long()[:, None]
                exact, eq = exact * keep[..., None], eq * keep[..., None]
            self.runs[key] = (exact, eq, stats)
        return self.runs[key]

    def clear(self):
        self.runs.clear()


def judge(what, got, exact, eq):
    """e = got - exact against the bf16 E_q: every figure is printed before it is asserted"""
    assert got.dtype == torch.float32 and tuple(got.shape) == tuple(exact.shape)
    e = got.cpu().to(torch.float64) - exact
    finite = bool(torch.isfinite(got).all())
    r_rms, r_max = rms(e) / rms(eq), float(e.abs().max()) / float(eq.abs().max())
    print(f"bf16 {what} {tuple(exact.shape)}: rms(e) {rms(e):.3e} = {r_rms:.3f} rms(E_q); max|e| {float(e.abs().max()):.3e} = {r_max:.3f} max|E_q|; "
          f"max|exact| {float(exact.abs().max()):.2f} finite={finite}")
    assert finite
    assert r_rms <= RMS_HI, r_rms
    assert r_max <= MAX_HI, r_max
    assert r_rms >= RMS_LO, r_rms
    return r_rms, r_max


def check_dec_mirror_matches_oracle(name):
    """the exact mode against oracle.mel_decoder (< 1e-6 L-inf), and E_q(bf16) is several times E_q(f16)"""
    from oracle import oracle
    cfg, sd = D.state_dict_of(name)
    feats = np.random.default_rng(5).standard_normal((2, 37, cfg.d4)).astype(np.float32)
    ref = oracle.mel_decoder(cfg, oracle.Weights(sd), feats)
    exact = dec_mirror(cfg, sd, feats, False)
    eq = dec_mirror(cfg, sd, feats, True) - exact
    eq16 = D.mirror(cfg, sd, feats, True) - exact
    err = float((exact - torch.from_numpy(ref).double()).abs().max())
    print(f"{name}: mirror vs oracle L-inf {err:.2e}; E_q(bf16) rms {rms(eq):.2e} = {rms(eq) / rms(eq16):.1f} x E_q(f16)")
    assert err < 1e-6, err
    assert rms(eq) > 4 * rms(eq16)


# ---------------------------------------------------------------------------------------------------------------- decoder checks
def check_forward_with_h0(yard, device):
    """Tests 1 and 3, tiny ES, the whole forward, free-running ragged B = 3, L ~ 150 (two windows, edge rows, padding frames): the band;
    mel_len, duration, dur and cum bit for bit those of precision 32; rows behind mel_len exact zeros; bf16 twice the same bits; not the
    precision-16 or precision-32 mel."""
    net, cfg, sd = D.make_net("tiny", device)
    x = D.free_running_batch(device)
    with torch.no_grad():
        enc = net.encoder._encode(x)
        s32 = net._launch(x, taps=True)
        sb = net._launch(dict(x, decoder_precision=BF), taps=True)
        sb2 = net._launch(dict(x, decoder_precision="bf16-mixed"))
        s16 = net._launch(dict(x, decoder_precision=16))
    ml = s32.mel_len.cpu()
    L = int(ml.max())
    assert 113 <= L <= 224 and int(ml.min()) < L - 20 and sb.mel.shape == (3, L, cfg.n_mel_channels)
    assert torch.equal(sb.mel_len, s32.mel_len) and torch.equal(sb.duration, s32.duration)
    for k in ("dur", "cum", "pitch_idx", "energy_idx"):
        assert torch.equal(sb.taps[k], s32.taps[k]), k
    assert np.array_equal(sb.taps["cum"].cpu().numpy(), s32.taps["cum"].cpu().numpy())
    assert torch.equal(sb.mel, sb2.mel) and not torch.equal(sb.mel, s32.mel) and not torch.equal(sb.mel, s16.mel)
    for b in range(3):
        assert not bool(sb.mel[b, int(ml[b]):].any()) and bool(sb.mel[b, :int(ml[b])].abs().sum() > 0)
    feats = D.frame_features(enc["feat"], s32.taps["dur"], L)
    exact, eq, _ = yard.get(("fwd", "tiny"), cfg, sd, feats, proj_rounded=False, mel_len=ml)
    assert float((s32.mel.cpu().double() - exact).abs().max()) < 1e-4
    return judge("tiny forward, fused gather with h0", sb.mel, exact, eq)


def check_chunk_walk(yard, name, B, T, D_, device):
    """Test 1 + the chunk-walk invariant at bf16: the fused gather without h0 (in-kernel `proj`) with a workspace (dx2 = 256: the chunk
    walk) and without one (the window form): each within the band, and the two agree to 2e-5 -- a kept row's operand values are the same
    values in both forms up to fp32 accumulation order (1e-6), and one crossed bfloat16 rounding boundary moves the mel by 2^3 times what
    a crossed binary16 boundary does (precision 16's bound is 2e-6 on the same reasoning)."""
    net, cfg, sd = D.make_net(name, device)
    feat = torch.from_numpy(np.random.default_rng(17).standard_normal((B, T, cfg.d4)).astype(np.float32))
    dur, cum, mel_len = D.ragged_durations(B, T, D_, device)
    L = int(mel_len.max())
    exact, eq, _ = yard.get(("walk", name, B, T, D_), cfg, sd, D.frame_features(feat, dur, L), mel_len=mel_len)
    outs, ratios = [], []
    for use_ws in (True, False):
        mel, n = D.run_decoder(net, cfg, feat.to(device), BF_CODE, cum, mel_len, workspace=use_ws)
        assert (n > 0) == (use_ws and cfg.dx2 == 256)
        ratios.append(judge(f"{name} fused gather, {'chunk walk' if n else 'window form'}", mel, exact, eq))
        outs.append(mel.cpu())
    d = float((outs[0] - outs[1]).abs().max())
    print(f"{name}: chunk walk vs window form at bf16: L-inf {d:.2e}")
    assert d < 2e-5, d
    return ratios


def check_direct(yard, name, B, L, device, profile=None):
    """Test 1, direct mode (the kernel runs `proj` itself) through MelDecoder.forward(precision="bf16")"""
    net, cfg, sd = D.make_net(name, device, profile)
    feats = torch.from_numpy(np.random.default_rng(7).standard_normal((B, L, cfg.d4)).astype(np.float32))
    exact, eq, _ = yard.get(("direct", name, profile, B, L), cfg, sd, feats)
    with torch.no_grad():
        mel = net.decoder(feats.to(device), precision=BF)
    return judge(f"{name}{'+' + profile if profile else ''} direct", mel, exact, eq)


def check_beyond_binary16(yard, device):
    """Test 2: direct mode, tiny, B = 2, L = 40, one feature entry per utterance set to 1e5 -- out of binary16's range (the mirror's
    largest rounded operand is >= 65520), inside bfloat16's: the bf16 mel is finite and inside the band."""
    net, cfg, sd = D.make_net("tiny", device)
    feats = torch.from_numpy(np.random.default_rng(7).standard_normal((2, 40, cfg.d4)).astype(np.float32))
    feats[0, 11, 5] = 1e5
    feats[1, 29, 77] = -1e5
    exact, eq, stats = yard.get(("beyond", "tiny"), cfg, sd, feats)
    assert stats["operand_max"] >= 65520.0, stats
    with torch.no_grad():
        mel = net.decoder(feats.to(device), precision=BF)
    return judge("tiny direct, |x| = 1e5", mel, exact, eq)


def check_entry_points(name, device, B=2, T=12, D_=5):
    """Test 3: precision 0 / 32 through esmi_mel_decoder_prec_f32 are esmi_mel_decoder_f32 bit for bit; 16 and bf16 are each reproducible,
    differ from each other and from 32, and bf16 is further from 32 than 16 is."""
    net, cfg, sd = D.make_net(name, device)
    feat = torch.from_numpy(np.random.default_rng(3).standard_normal((B, T, cfg.d4)).astype(np.float32)).to(device)
    _dur, cum, mel_len = D.ragged_durations(B, T, D_, device)
    plain, _ = D.run_decoder(net, cfg, feat, 32, cum, mel_len, entry="plain")
    assert bool(torch.isfinite(plain).all())
    for precision in (0, 32):
        got, _ = D.run_decoder(net, cfg, feat, precision, cum, mel_len)
        assert torch.equal(got, plain), precision
    p16, _ = D.run_decoder(net, cfg, feat, 16, cum, mel_len)
    pb, _ = D.run_decoder(net, cfg, feat, BF_CODE, cum, mel_len)
    pb2, _ = D.run_decoder(net, cfg, feat, BF_CODE, cum, mel_len)
    p16b, _ = D.run_decoder(net, cfg, feat, 16, cum, mel_len)
    assert torch.equal(pb, pb2) and torch.equal(p16, p16b)
    d16, db = float((p16 - plain).abs().max()), float((pb - plain).abs().max())
    print(f"{name}: L-inf to precision 32: 16 {d16:.2e}, bf16 {db:.2e}")
    assert 0 < d16 < db < 0.5


def check_range_check_runs_bf16(device):
    """check_activation_range with the key at bf16 returns the range-checked build's bf16 forward bit for bit (it has nothing to check
    there, and does not fall back to 32)"""
    import contextlib
    import os
    net, cfg, sd = D.make_net("tiny", device)
    from efficientspeech_amd.synth import synth_phonemes
    ids, mask = synth_phonemes(2, 12, 3, [12, 6])
    x = {"phoneme": torch.from_numpy(ids).to(device), "phoneme_mask": torch.from_numpy(mask).to(device), "decoder_precision": BF}
    checked = os.path.join(os.path.dirname(_lib.LIB_PATH), "libesmi_checked.so")
    with torch.no_grad():
        with (_lib.use_library(checked) if str(device).startswith("cuda") else contextlib.nullcontext()):
            melb, lenb, _ = net(x)
            mel32, _len32, _ = net(dict(x, decoder_precision=32))
        got, got_len, _ = net.check_activation_range(x)
    assert torch.equal(got_len, lenb) and torch.equal(got, melb)
    assert float((got - mel32).abs().max()) > 1e-3


# ---------------------------------------------------------------------------------------------------------------- vocoder yardstick
def voc_mirror(h, sd, mel, rounded, fused):
    """tests/vocoder_precision16_checks.mirror with the bf16 rules.  Weight operand: bfloat16(w) in conv_pre, the ConvTranspose1d's and a
    ResBlock that runs conv by conv; the two-plane value in a ResBlock that runs as one launch (`fused` and its stage has 8 / 16 / 32 /
    64 channels and k in {3, 7, 11}: the library's resblock_fused_ok -- the launch-log test pins which kernels ran)."""
    q = q_bf16 if rounded else (lambda t: t)
    W = lambda key: torch.as_tensor(sd[key]).to(torch.float64)   # noqa: E731
    qw = (lambda key, one_launch: w_two_plane(sd[key]) if one_launch else w_bf16(sd[key])) if rounded else (lambda key, one_launch: W(key))
    pad = lambda k, d: (k * d - d) // 2                          # noqa: E731
    x = torch.as_tensor(mel).to(torch.float64).transpose(1, 2)
    x = F.conv1d(q(x), qw("conv_pre.weight", False), W("conv_pre.bias"), padding=3)
    scale, n, nk, c = 1.0, 0, len(h.resblock_kernel_sizes), h.upsample_initial_channel
    for i, (u, k) in enumerate(zip(h.upsample_rates, h.upsample_kernel_sizes)):
        x = F.conv_transpose1d(q(F.leaky_relu(scale * x, 0.1)), qw(f"ups.{i}.weight", False), W(f"ups.{i}.bias"), stride=u, padding=(k - u) // 2)
        c //= 2
        xs = 0.0
        for kk, dil in zip(h.resblock_kernel_sizes, h.resblock_dilation_sizes):
            one = fused and c in (8, 16, 32, 64) and kk in (3, 7, 11)
            r = x
            for m, d in enumerate(dil):
                if h.resblock == "1":
                    t = F.conv1d(q(F.leaky_relu(r, 0.1)), qw(f"resblocks.{n}.convs1.{m}.weight", one), W(f"resblocks.{n}.convs1.{m}.bias"),
                                 dilation=d, padding=pad(kk, d))
                    t = F.conv1d(q(F.leaky_relu(t, 0.1)), qw(f"resblocks.{n}.convs2.{m}.weight", one), W(f"resblocks.{n}.convs2.{m}.bias"),
                                 padding=pad(kk, 1))
                else:
                    t = F.conv1d(q(F.leaky_relu(r, 0.1)), qw(f"resblocks.{n}.convs.{m}.weight", one), W(f"resblocks.{n}.convs.{m}.bias"),
                                 dilation=d, padding=pad(kk, d))
                r = t + r
            xs = xs + r
            n += 1
        x, scale = xs, 1.0 / nk
    x = F.conv1d(F.leaky_relu(scale * x, 0.01), W("conv_post.weight"), W("conv_post.bias"), padding=3)
    return torch.tanh(x)[:, 0]


class VocYard:
    """(mel, exact, E_q) per (generator, B, L, fused): computed once, shared, never modified"""

    def __init__(self):
        self.runs, self.exact = {}, {}

    def get(self, name, B, L, fused):
        key = (name, B, L, fused)
        if key not in self.runs:
            h = VV.config_of(name)
            sd = synth_hifigan_state_dict(h, 1234)
            if B is None:
                import os
                g = np.load(os.path.join(VV.GOLD, VV.FIXTURES[name]))
                mel = torch.from_numpy(g["mel"])
            else:
                mel = make_mel(h, B, L, "cpu")
            if (name, B, L) not in self.exact:
                self.exact[(name, B, L)] = voc_mirror(h, sd, mel, False, fused)
            exact = self.exact[(name, B, L)]
            self.runs[key] = (mel, exact, voc_mirror(h, sd, mel, True, fused) - exact)
        return self.runs[key]

    def clear(self):
        self.runs.clear()
        self.exact.clear()


def check_voc_mirror_matches_fixture(yard, name):
    """the exact mode against the reference-generated waveform (< 2e-6 L-inf, the precision-16 suite's bound)"""
    import os
    _mel, exact, eq = yard.get(name, None, None, True)
    ref = torch.from_numpy(np.load(os.path.join(VV.GOLD, VV.FIXTURES[name]))["wav"]).to(torch.float64)
    err = float((exact - ref).abs().max())
    print(f"{name}: mirror vs fixture L-inf {err:.2e}; E_q(bf16) L-inf {float(eq.abs().max()):.2e} rms {rms(eq):.2e}")
    assert err < 2e-6, err


def check_voc_accuracy(yard, name, device, fused, B=None, L=None):
    """Test 4: e = wav_bf16 - exact against the bf16 E_q, the band"""
    mel, exact, eq = yard.get(name, B, L, fused)
    voc = VV.make_vocoder(name, device, fused=fused)
    with torch.no_grad():
        wav = voc(mel.to(device).transpose(1, 2), precision=BF)
    assert wav.shape == (mel.shape[0], 1, mel.shape[1] * voc.h.hop)
    return judge(f"vocoder {name} fused={fused}", wav[:, 0], exact, eq)


def check_voc_ragged_contract(name, B, L, lengths, device, modes=(True, False), module=True):
    """Test 5: at bf16 the length-aware call's kept samples are the plain bf16 run's bit for bit, the tails exact zeros (workspace and
    outputs NaN-filled on entry), and the PCM plane is trunc(clamp(wav * 32768, -32768, 32767))."""
    for fused in modes:
        voc = VV.make_vocoder(name, device, fused=fused)
        mel = make_mel(voc.h, B, L, device)
        full, _ = VV.run_prec(voc, mel, BF_CODE)
        assert float(full.abs().max()) > 1e-3 and bool(torch.isfinite(full).all())
        got, pcm = VV.run_prec(voc, mel, BF_CODE, lengths, want_pcm=True)
        assert_kept_and_tails(got, full, lengths, voc.h.hop, f"{name} fused={fused} bf16")
        assert torch.equal(pcm, (got * 32768).clamp(-32768, 32767).trunc().to(torch.int16))
        assert int(pcm.abs().max()) > 30
        p16, _ = VV.run_prec(voc, mel, 16)
        assert not torch.equal(p16, full)
        if not module:
            continue
        with torch.no_grad():
            assert not torch.equal(voc(mel.transpose(1, 2))[:, 0], full)
            assert torch.equal(voc(mel.transpose(1, 2), precision=BF)[:, 0], full)
            assert torch.equal(voc(mel.transpose(1, 2), precision="bf16-mixed")[:, 0], full)


def check_voc_default_untouched(name, B, L, lengths, device, fused=True):
    """Test 3, vocoder: precision 0 and 32 through the _prec entry point are the two older entry points bit for bit (with bf16 calls in
    between), and precision 16 is reproducible"""
    from tests.vocoder_ragged_checks import run_abi
    voc = VV.make_vocoder(name, device, fused=fused)
    mel = make_mel(voc.h, B, L, device)
    plain, _ = run_abi(voc, mel)
    rag, rag_pcm = run_abi(voc, mel, lengths, want_pcm=True)
    p16, _ = VV.run_prec(voc, mel, 16)
    VV.run_prec(voc, mel, BF_CODE)
    for precision in (0, 32):
        a, none = VV.run_prec(voc, mel, precision)
        assert none is None and torch.equal(a, plain), precision
        b, b_pcm = VV.run_prec(voc, mel, precision, lengths, want_pcm=True)
        assert torch.equal(b, rag) and torch.equal(b_pcm, rag_pcm), precision
    assert torch.equal(VV.run_prec(voc, mel, 16)[0], p16)


# ---------------------------------------------------------------------------------------------------------------- interfaces
def _vocoder80(device, small, precision=32):
    """the vocoder behind tiny ES in the wrapper checks: v2, or (small: the simulator tier) the smallest generator that takes 80 mels and
    has both launch families -- 32 -> 16 / 8 channels, rates (2, 2), one k = 3 ResBlock1 per stage"""
    if not small:
        return VV.make_vocoder("v2", device, precision=precision)
    from efficientspeech_amd.hifigan import HifiGanConfig
    h = HifiGanConfig(resblock="1", upsample_rates=(2, 2), upsample_kernel_sizes=(4, 4), upsample_initial_channel=32,
                      resblock_kernel_sizes=(3,), resblock_dilation_sizes=((1, 3, 5),), num_mels=80)
    voc = Generator(h, precision=precision)
    voc.load_state_dict({k: torch.from_numpy(v) for k, v in synth_hifigan_state_dict(h, 1234).items()}, strict=True)
    return voc.to(device).eval()


def _model(device, voc_precision=32, small=False):
    from efficientspeech_amd import EfficientSpeech
    from efficientspeech_amd.config import CONFIGS
    from efficientspeech_amd.synth import synth_state_dict
    voc = _vocoder80(device, small, voc_precision)
    model = EfficientSpeech.from_config("tiny", hifigan=voc)
    model.phoneme2mel.load_state_dict({k: torch.from_numpy(v) for k, v in synth_state_dict(CONFIGS["tiny"], 1234).items()}, strict=True)
    return model.to(device).eval(), voc


def check_synthesize(device, small=False):
    """Test 6: synthesize(precision="bf16", decoder_precision="bf16") is Generator.forward(mel_bf16, lengths, precision="bf16") bit for
    bit; finite; wav_len and duration those of precision 32; each argument alone changes only its half; Generator(h, precision="bf16")
    and the attribute `decoder.precision = "bf16"` are the defaults; tiny ES + v2, B = 3, T = 12, forced durations."""
    model, voc = _model(device, small=small)
    _ids, _dur, x = D._forced_batch(device)
    net = model.phoneme2mel
    with torch.no_grad():
        mel32, len32, _ = net(x, train=False)
        melb, lenb, _ = net(dict(x, decoder_precision=BF), train=False)
        wav32, wlen32, dur32 = model.synthesize(x)
        wavbb, wlenbb, durbb = model.synthesize(x, precision=BF, decoder_precision=BF)
        wavb_, _, _ = model.synthesize(x, precision="bf16-mixed")
        wav_b, _, _ = model.synthesize(x, decoder_precision="bf16-mixed")
        assert torch.equal(wavbb, voc(melb.transpose(1, 2), lengths=lenb, precision=BF)[:, 0])
        assert torch.equal(wavb_, voc(mel32.transpose(1, 2), lengths=len32, precision=BF)[:, 0])
        assert torch.equal(wav_b, voc(melb.transpose(1, 2), lengths=lenb)[:, 0])
        for bad in (8, True, "fp8"):
            with pytest.raises(ValueError, match="precision"):
                model.synthesize(x, precision=bad)
            with pytest.raises(ValueError, match="precision"):
                model.synthesize(x, decoder_precision=bad)
        net.decoder.precision = BF
        try:
            assert "precision" not in " ".join(net.decoder.state_dict())
            assert torch.equal(net(x, train=False)[0], melb)
            assert torch.equal(net(dict(x, decoder_precision=32), train=False)[0], mel32)
        finally:
            net.decoder.precision = 32
        vocb = _vocoder80(device, small, "bf16-mixed")
        assert vocb.precision == BF
        assert torch.equal(vocb(melb.transpose(1, 2), lengths=lenb)[:, 0], wavbb)
    assert bool(torch.isfinite(wavbb).all()) and float(wavbb.abs().max()) > 1e-3
    assert torch.equal(lenb, len32) and torch.equal(wlenbb, wlen32) and torch.equal(durbb, dur32)
    assert not torch.equal(melb, mel32) and not torch.equal(wavbb, wav32) and not torch.equal(wavbb, wavb_) and not torch.equal(wavbb, wav_b)


def check_get_hifigan(tmp_path):
    """Test 6 (host only): get_hifigan(..., precision=) builds a generator whose default is bf16, under either spelling"""
    import dataclasses
    import json
    from efficientspeech_amd.hifigan import get_hifigan
    h = VV.small_config()
    ckpt = tmp_path / "generator_small"
    (tmp_path / "config.json").write_text(json.dumps(dataclasses.asdict(h)))
    torch.save({"generator": {k: torch.from_numpy(v) for k, v in synth_hifigan_state_dict(h, 1234).items()}}, str(ckpt))
    assert get_hifigan(str(ckpt), precision=BF).precision == BF
    assert get_hifigan(str(ckpt), precision="bf16-mixed").precision == BF
    assert get_hifigan(str(ckpt)).precision == 32
    with pytest.raises(ValueError, match="precision"):
        get_hifigan(str(ckpt), precision=8)


def check_scheduler(device):
    """Test 6: a BucketedSynthesizer whose `extra` adds the key at bf16 gives the direct bf16 call's mels bit for bit"""
    from efficientspeech_amd import BucketedSynthesizer
    net, cfg, sd = D.make_net("tiny", device)
    lens = [12, 7, 3]
    ids, dur, _x = D._forced_batch(device, lens=lens)
    seqs = [ids[b, :n].astype(np.int32) for b, n in enumerate(lens)]

    def extra(idx, T_):
        d = np.zeros((len(idx), T_), np.int32)
        for r, i in enumerate(idx):
            d[r, :lens[i]] = dur[i, :lens[i]]
        return {"duration_forced": torch.from_numpy(d).to(device), "decoder_precision": BF}
    res = BucketedSynthesizer(net, max_batch=1, granularity=4)(seqs, extra=extra)
    for i, (mel_i, _dur_i) in enumerate(res):
        xi = {"phoneme": torch.from_numpy(seqs[i][None]).to(device), "duration_forced": torch.from_numpy(dur[i:i + 1, :lens[i]]).to(device)}
        with torch.no_grad():
            alone_b = net(dict(xi, decoder_precision=BF))[0][0]
            alone32 = net(xi)[0][0]
        assert torch.equal(mel_i, alone_b) and not torch.equal(mel_i, alone32), i


def check_staged_forward(device):
    """Test 6: the key through `_launch(stage=1)` / `_launch(stage=2)` (the state carries "bf16"), sharded_forward's staged calls and a
    ShardedMelPipeline step: the one-call forward's bf16 bits; the attribute as the default of the same paths."""
    from efficientspeech_amd.sharded import ShardedMelPipeline
    net, cfg, sd = D.make_net("tiny", device)
    _ids, dur, x = D._forced_batch(device)
    xb = dict(x, decoder_precision=BF)
    with torch.no_grad():
        oneb, one32 = net._launch(xb), net._launch(x)
        assert not torch.equal(oneb.mel, one32.mel)
        for more in ({}, {"max_mel_len": int(dur.sum(1).max()) + 5}):
            ref = oneb.mel if not more else net._launch(dict(xb, **more)).mel
            st = net._launch(dict(xb, **more), stage=1)
            assert st.precision == BF and st.mel is None
            st = net._launch(None, stage=2, state=st)
            assert torch.equal(st.mel, ref) and torch.equal(st.mel_len, one32.mel_len), more
        mel, mel_len = ShardedMelPipeline(net).step(xb)
        assert torch.equal(mel, oneb.mel) and torch.equal(mel_len, one32.mel_len)
        from efficientspeech_amd.sharded import sharded_forward
        mel, mel_len, _dur = sharded_forward(net, xb)            # (one rank: its world-size-1 form; the staged calls are the ones above)
        assert torch.equal(mel, oneb.mel) and torch.equal(mel_len, one32.mel_len)
        net.decoder.precision = BF
        try:
            st = net._launch(None, stage=2, state=net._launch(x, stage=1))
            assert torch.equal(st.mel, oneb.mel)
        finally:
            net.decoder.precision = 32


def check_graph_replay(device):
    """Test 6 (GPU only): the graph-replay path captures the decoder at bf16 -- the eager bf16 bits -- and refuses a later step that asks
    for 16 or 32 (NotImplementedError)"""
    from efficientspeech_amd.sharded import ShardedMelPipeline, _encode_with_head
    net, cfg, sd = D.make_net("tiny", device)
    _ids, dur, x = D._forced_batch(device)
    x = dict(x, max_mel_len=int(dur.sum(1).max()))
    xb = dict(x, decoder_precision=BF)
    L = x["max_mel_len"]
    with torch.no_grad():
        enc = _encode_with_head(net, x)
        ref = net.decoder._fused(enc["feat"], enc["cum"], enc["mel_len"], enc["lmax"], L, True, L, h0=enc["h0"], precision=BF)
        pipe = ShardedMelPipeline(net, use_graph=True)
        mel, _len = pipe.step(xb)
        torch.cuda.synchronize()
        assert pipe.graphed is not None and pipe.graphed.precision == BF
        assert torch.equal(mel, ref)
        mel2, _len = pipe.step(dict(x, decoder_precision="bf16-mixed"))     # (the same precision under its other spelling: replayed)
        torch.cuda.synchronize()
        assert torch.equal(mel2, ref)
        for bad in (x, dict(x, decoder_precision=32), dict(x, decoder_precision=16)):
            with pytest.raises(NotImplementedError, match="decoder_precision"):
                pipe.step(bad)


def check_python_refusals(device):
    """Test 6: ValueError (text contains "precision") for 8, True and "fp8" from every Python entry; the key with train=True"""
    from efficientspeech_amd.synth import synth_phonemes
    net, cfg, sd = D.make_net("tiny", device)
    feat = torch.from_numpy(np.random.default_rng(3).standard_normal((2, 9, cfg.d4)).astype(np.float32)).to(device)
    ids, mask = synth_phonemes(2, 9, 1, [9, 4])
    x = {"phoneme": torch.from_numpy(ids).to(device), "phoneme_mask": torch.from_numpy(mask).to(device)}
    for bad in (8, True, "fp8"):
        with pytest.raises(ValueError, match="precision"), torch.no_grad():
            net(dict(x, decoder_precision=bad))
        with pytest.raises(ValueError, match="precision"), torch.no_grad():
            net.decoder(feat, precision=bad)
        with pytest.raises(ValueError, match="precision"):
            Generator(VV.reduced_config(), precision=bad)
        with pytest.raises(ValueError, match="precision"):
            networks._decoder_precision(bad)
    voc = VV.make_vocoder("small", device)
    mel = make_mel(voc.h, 1, 4, device)
    for bad in (8, True, "fp8"):
        with pytest.raises(ValueError, match="precision"), torch.no_grad():
            voc(mel.transpose(1, 2), precision=bad)
    xt = dict(x, decoder_precision=BF, pitch=torch.zeros((2, 9), device=device), energy=torch.zeros((2, 9), device=device),
              duration=torch.ones((2, 9), dtype=torch.int32, device=device), mel_len=torch.tensor([9, 4], dtype=torch.int32, device=device))
    with pytest.raises(ValueError, match="decoder_precision"), torch.no_grad():
        net(xt, train=True)
    from efficientspeech_amd import train
    assert train.normalize_precision is _lib.normalize_precision and train.normalize_precision("bf16-mixed") == BF
    assert networks._decoder_precision("bf16-mixed") == BF and networks._decoder_precision("16-mixed") == 16 and networks._decoder_precision(None, BF) == BF


def check_c_refusals():
    """Test 6 on the simulator: precision 8 is ESMI_ERR_ARG from each of the four C entry points, and the launch log stays empty"""
    from efficientspeech_amd.synth import synth_phonemes
    from tests.simlib import launch_records
    net, cfg, sd = D.make_net("tiny", "cpu")
    feat = torch.from_numpy(np.random.default_rng(3).standard_normal((2, 9, cfg.d4)).astype(np.float32))
    D.run_decoder(net, cfg, feat, 32)                      # (weights packed: the records below are the calls' alone)
    ids, mask = synth_phonemes(2, 9, 1, [9, 4])
    with torch.no_grad():
        net({"phoneme": torch.from_numpy(ids), "phoneme_mask": torch.from_numpy(mask)})
    voc = VV.make_vocoder("small", "cpu")
    mel = make_mel(voc.h, 1, 4, "cpu")
    VV.run_prec(voc, mel, 32)
    lib, stream = networks._runtime(net.decoder.mel_linear.weight)
    a = net._static_args(lib, stream)
    with launch_records() as records:
        with pytest.raises(RuntimeError, match="esmi_mel_decoder_prec_f32 failed: ESMI_ERR_ARG"):
            D.run_decoder(net, cfg, feat, 8)
        with pytest.raises(RuntimeError, match="esmi_phoneme2mel_forward_prec_f32 failed: ESMI_ERR_ARG"):
            lib.esmi_phoneme2mel_forward_prec_f32(C.byref(a), None, 8, 0, stream)
        with pytest.raises(RuntimeError, match="esmi_phoneme2mel_forward_curve_f32 failed: ESMI_ERR_ARG"):
            lib.esmi_phoneme2mel_forward_curve_f32(C.byref(a), None, 8, 0, stream)
        with pytest.raises(RuntimeError, match="esmi_hifigan_generator_prec_f32 failed: ESMI_ERR_ARG"):
            VV.run_prec(voc, mel, 8)
    assert records == []


def check_fp32mfma_refuses(lib_path):
    """Test 6: libesmi_fp32mfma.so has no one-product path: bf16 is ESMI_ERR_UNSUPPORTED from the four entry points, decided on the host
    before anything is enqueued (no device is touched: this runs without a GPU); 8 stays ESMI_ERR_ARG"""
    lib = _lib.bind(C.CDLL(lib_path))
    assert lib.esmi_build_config().decode().startswith("dec_gemm=fp32-mfma")
    shape = _lib.DecoderShape(128, 128, 5, 2, 2, 80)
    buf = (C.c_float * 64)()
    p = C.cast(C.byref(buf), C.c_void_p)
    with pytest.raises(_lib.Unsupported):
        lib.esmi_mel_decoder_prec_f32(p, C.byref(shape), p, None, None, None, None, 4, 0, 1, 0, 4, p, None, 0, BF_CODE, None)
    with pytest.raises(RuntimeError, match="ESMI_ERR_ARG"):
        lib.esmi_mel_decoder_prec_f32(p, C.byref(shape), p, None, None, None, None, 4, 0, 1, 0, 4, p, None, 0, 8, None)
    a = _lib.ForwardArgs()
    with pytest.raises(_lib.Unsupported):
        lib.esmi_phoneme2mel_forward_prec_f32(C.byref(a), None, BF_CODE, 0, None)
    with pytest.raises(_lib.Unsupported):
        lib.esmi_phoneme2mel_forward_curve_f32(C.byref(a), None, BF_CODE, 0, None)
    s = _lib.HifiGanShape(n_mel=8, initial_channel=32, n_up=1, n_kernels=1, resblock=1)
    s.up_rates[0], s.up_kernels[0], s.rb_kernels[0] = 2, 4, 3
    w = _lib.HifiGanWeights()
    with pytest.raises(_lib.Unsupported):
        lib.esmi_hifigan_generator_prec_f32(C.byref(w), C.byref(s), p, 1, 4, None, p, None, BF_CODE, p, 1 << 20, None)


# ---------------------------------------------------------------------------------------------------------------- launches (simulator)
def check_decoder_dispatch(name):
    """Test 7: a bf16 forward's records differ from the precision-32 one's only in the decoder kernel's name"""
    r32, _ = D.forward_records(name, {})
    rb, _ = D.forward_records(name, {"decoder_precision": BF})
    assert len(rb) == len(r32) and rb[:-1] == r32[:-1]
    (n32, d32), (nb, db) = r32[-1], rb[-1]
    assert n32 == "mel_decoder_kernel<DX2,KD,NW>" and nb == "mel_decoder_bf16_kernel<DX2,KD,NW>", (n32, nb)
    assert db == d32
    assert sum("mel_decoder" in r[0] for r in rb) == 1


_BF_OF_16 = {"convgemm_kernel<1,true>": "convgemm_bf16_kernel<1>", "convgemm_kernel<2,true>": "convgemm_bf16_kernel<2>",
             "convgemm_kernel<4,true>": "convgemm_bf16_kernel<4>", "convgemm_kernel<8,true>": "convgemm_bf16_kernel<8>",
             "convgemm_dma_kernel<4,1,NWV,true,false>": "convgemm_dma_bf16_kernel<4,1,NWV>",
             "convgemm_dma_kernel<4,2,NWV,true,false>": "convgemm_dma_bf16_kernel<4,2,NWV>",
             "convgemm_dma_kernel<8,1,NWV,true,false>": "convgemm_dma_bf16_kernel<8,1,NWV>",
             "convgemm_len_amp_kernel<1>": "convgemm_bf16_len_kernel<1>", "convgemm_len_amp_kernel<2>": "convgemm_bf16_len_kernel<2>",
             "hifigan_resblock_amp_kernel<C,K>": "hifigan_resblock_bf16_kernel<C,K>",
             "hifigan_resblock16_amp_kernel<C,K>": "hifigan_resblock16_bf16_kernel<C,K>",
             "conv_to1_kernel": "conv_to1_kernel", "conv_to1_len_kernel": "conv_to1_len_kernel"}


def vocoder_records(name, precision, fused, ragged, B=2, L=6, lengths=(6, 2)):
    from tests.simlib import launch_records, use_sim
    h = VV.config_of(name)
    mel = make_mel(h, B, L, "cpu")
    with use_sim(), torch.no_grad(), launch_records() as records:
        voc = VV.make_vocoder(name, "cpu", fused=fused)
        voc(mel.transpose(1, 2), lengths=torch.tensor(list(lengths), dtype=torch.int32) if ragged else None, precision=precision)
    return [r for r in records if not r[0].startswith(VV._PREP)]


def check_vocoder_dispatch(name, fused, ragged):
    """Test 7: a bf16 vocoder call's records are the precision-16 call's with every kernel's name replaced by its bf16 twin's: same
    number, same order, same grid / block / LDS bytes"""
    r16 = vocoder_records(name, 16, fused, ragged)
    rb = vocoder_records(name, BF, fused, ragged)
    assert len(rb) == len(r16) > 3
    for (n16, d16), (nb, db) in zip(r16, rb):
        assert n16 in _BF_OF_16, n16
        assert nb == _BF_OF_16[n16] and db == d16, (n16, d16, nb, db)
    assert any("resblock" in n for n, _ in rb) == fused


# ---------------------------------------------------------------------------------------------------------------- precision 16 keeps its bits
P16_GOLDEN = "precision16_parent_bits.npz"     # tests/golden/: tools/gen_golden_precision16.py, run on the commit before bf16 inference


def precision16_cases(device):
    """name -> precision-16 output (host fp32) of four small deterministic calls: the decoder in direct mode, tiny (2, 40) and small
    (1, 40), and the vocoder one launch per ResBlock, "small" (2, 6: the 16-row-tile kernels) and "reduced1" (2, 6: the 32-row-tile
    kernels at 64 / 32 channels behind the per-convolution GEMMs).  Inputs and weights come from fixed seeds."""
    out = {}
    for name, B, L in (("tiny", 2, 40), ("small", 1, 40)):
        net, cfg, _sd = D.make_net(name, device)
        feats = torch.from_numpy(np.random.default_rng(7).standard_normal((B, L, cfg.d4)).astype(np.float32))
        with torch.no_grad():
            out[f"dec_{name}"] = net.decoder(feats.to(device), precision=16).cpu().numpy()
    for name in ("small", "reduced1"):
        voc = VV.make_vocoder(name, device, fused=True)
        mel = make_mel(voc.h, 2, 6, device)
        wav, _ = VV.run_prec(voc, mel, 16)
        out[f"voc_{name}"] = wav.cpu().numpy()
    return out


def check_precision16_keeps_the_parents_bits(device, tier):
    """Issue test 3: precision 16 through the `_prec` entry points gives, bit for bit, what the commit before this feature gave: the
    committed outputs of that commit's own build (tier "sim": its wave-simulator build; "gpu": its libesmi.so on an MI355X)."""
    import os
    gold = np.load(os.path.join(VV.GOLD, P16_GOLDEN))
    got = precision16_cases(device)
    for name, a in got.items():
        ref = gold[f"{tier}_{name}"]
        assert a.dtype == ref.dtype and a.shape == ref.shape, name
        assert float(np.abs(ref).max()) > 1e-3 and bool(np.isfinite(a).all()), name
        d = float(np.abs(a - ref).max())
        print(f"precision 16, {tier} {name} {a.shape}: L-inf to the parent commit's bits {d:.1e}")
        assert np.array_equal(a, ref), (name, d)


# ---------------------------------------------------------------------------------------------------------------- the fused kernels' weight rule
_PROBE_SRC = r"""
// stand-alone host program: the kernels' own helpers on the host (the simulator's branch of wavesim_shim.h) -- packs each weight as the
// packers do (split_f16_pair_rn of 2^8 w) and forms the bf16 operand as the fused kernels do (bf16_of_f16_planes)
#include <cstdio>
#include <vector>
#include "esmi_dev.h"
int main(int argc, char** argv) {
    FILE* in = std::fopen(argv[1], "rb");
    FILE* out = std::fopen(argv[2], "wb");
    std::vector<float> w(8);
    while (std::fread(w.data(), sizeof(float), 8, in) == 8) {
        esmi::u32x4 p0, p1;
        for (int j = 0; j < 4; ++j) {
            unsigned h1, h2;
            esmi::split_f16_pair_rn(w[2 * j] * esmi::kF16WScale, w[2 * j + 1] * esmi::kF16WScale, h1, h2);
            p0[j] = h1;
            p1[j] = h2;
        }
        const esmi::u32x4 o = esmi::bf16_of_f16_planes(p0, p1);
        unsigned v[4] = {o[0], o[1], o[2], o[3]};
        std::fwrite(v, sizeof(unsigned), 4, out);
    }
    std::fclose(in);
    std::fclose(out);
    return 0;
}
"""


def check_plane_rule_bit_for_bit(tmp_path):
    """`bf16_of_f16_planes` (wavesim_shim.h) on packed planes, bit for bit against `w_two_plane`, over 2^20 weights: normal ones, and
    2^19 built so that the SECOND plane decides the rounding -- 2^8 w = an exact bfloat16 tie in binary16 (plane 0) plus a residual
    below binary16's ulp (plane 1): converting plane 0 alone rounds those to even, the contract rounds them away.  The program is
    compiled here from the kernels' headers for the host (the simulator's branch; the device's branch is held by the accuracy tests)."""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cxx = os.environ.get("CXX", "/opt/rocm/lib/llvm/bin/clang++")
    if not os.path.exists(cxx):
        pytest.skip("needs the host compiler the simulator build uses")
    rng = np.random.default_rng(11)
    normal = (rng.standard_normal(1 << 19) * 0.1).astype(np.float32)
    m = rng.integers(128, 256, size=1 << 19).astype(np.float64)            # 8-bit bfloat16 significands
    e = rng.integers(-10, 0, size=1 << 19)                                  # (the residual stays a normal or exact subnormal binary16)
    sign = rng.choice([-1.0, 1.0], size=1 << 19)
    ties = (sign * (m + 0.5 + rng.choice([-1.0, 1.0], size=1 << 19) * 2.0 ** -6) * 2.0 ** (e - 7)).astype(np.float32)   # tie +- 2^-13 relative
    w = np.concatenate([normal, ties])
    src, exe, fin, fout = (str(tmp_path / n) for n in ("probe.cpp", "probe", "w.bin", "o.bin"))
    open(src, "w").write(_PROBE_SRC)
    w.tofile(fin)
    subprocess.run([cxx, "-x", "c++", "-std=c++17", "-O1", "-DESMI_WAVESIM", "-I", os.path.join(root, "tools", "wavesim"),
                    "-I", os.path.join(root, "efficientspeech_amd", "csrc"), "-Wno-unused-value", src, "-o", exe], check=True)
    subprocess.run([exe, fin, fout], check=True)
    got = np.fromfile(fout, dtype=np.uint16)                              # low half first: the weight order
    assert got.shape == w.shape
    want = w_two_plane(w).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    plane0 = (torch.from_numpy(w) * 256.0).to(torch.float16).to(torch.float32).div(256.0).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    print(f"weight rule: {int((got != want).sum())} of {w.size} differ from the contract; plane 0 alone would differ on {int((plane0 != want).sum())}, "
          f"bfloat16(w) on {int((w_bf16(w).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16) != want).sum())}")
    assert np.array_equal(got, want)
    assert int((plane0[1 << 19:] != want[1 << 19:]).sum()) > (1 << 17)     # (the set does tell the rule from its neighbour)
