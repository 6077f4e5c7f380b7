"""Checks of inference at the reduced precisions -- 16 (one binary16 product per contraction) and "bf16" (one bfloat16 product) -- of the
mel decoder (esmi_mel_decoder_prec_f32, esmi_phoneme2mel_forward_prec_f32 / _curve_f32, MelDecoder.forward(..., precision), the input-dict
key `decoder_precision`) and of the HiFi-GAN generator (esmi_hifigan_generator_prec_f32, Generator(h, precision) / .forward(..., precision),
get_hifigan, EfficientSpeech.synthesize), shared by the GPU tier and the wave-simulator tier of tests/test_decoder_precision16.py,
tests/test_vocoder_precision16.py and tests/test_inference_bf16.py.  Every check takes the device ("cuda:0", or "cpu" inside
`use_sim()`), and those that exist for both precisions take the `Rule`.

The yardsticks are fp64 restatements of MelDecoder.forward and Generator.forward with two modes: exact, and rounded operands -- at every
contraction of the contract (include/esmi.h) the input and the weight go through the `Rule` of the precision; everything else is exact.
E_q = rounded - exact is the error any ideal implementation with such operands has.  The kernels are held to it through their error
e = kernel - exact (they cannot match the rounded mirror closely: fp32 accumulation flips rounding boundaries of the next layer's
operands), and the verdict is one band: rms(e) / rms(E_q) in [0.5, 1.25], max|e| / max|E_q| <= 2.  Precision 32 sits three orders below
E_q(f16), and E_q(bf16) is about 2^3 times E_q(f16): the lower bound is what proves that the precision's own product ran.
"""
import contextlib
import ctypes as C
import dataclasses
import os
import types
import typing

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from efficientspeech_amd import CONFIGS, _lib, build_phoneme2mel, load_numpy_state_dict, networks
from efficientspeech_amd.hifigan import HIFIGAN_CONFIGS, Generator, HifiGanConfig, synth_hifigan_state_dict
from efficientspeech_amd.networks import _on_device_of, _ptr
from efficientspeech_amd.synth import synth_phonemes, synth_state_dict
from tests import weight_profiles as WP
from tests.vocoder_ragged_checks import assert_kept_and_tails, make_mel, run_abi

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURES = {"v1": "hifigan_v1_b1_l9.npz", "v2": "hifigan_v2_b2_l24.npz", "v3": "hifigan_v3_b1_l17.npz"}
RMS_LO, RMS_HI, MAX_HI = 0.5, 1.25, 2.0       # the band: rms(e) / rms(E_q) in [0.5, 1.25], max|e| / max|E_q| <= 2
BAD = (8, 0, "16", True, "fp8")               # what no Python entry takes as a precision (None is "the default")


# ---------------------------------------------------------------------------------------------------------------- what the drivers share
@pytest.fixture
def device(request):
    """the tier of the test that asks for it: "cuda:0" for a test marked `gpu`, else "cpu" with the wave simulator bound during the test"""
    if request.node.get_closest_marker("gpu"):
        yield "cuda:0"
    else:
        from tests.simlib import use_sim
        with use_sim():
            yield "cpu"


@pytest.fixture(scope="module")
def yard():
    """the fp64 yardsticks the accuracy tests of a module share (computed on first use), released when that module's tests are done"""
    y = Yardsticks()
    yield y
    y.clear()


def on_the_device(test):
    """the GPU tier's twin of a simulator-tier test: the same code and parameters under the name it is assigned to, marked `gpu`"""
    twin = types.FunctionType(test.__code__, test.__globals__, test.__name__, test.__defaults__, test.__closure__)
    twin.__doc__, twin.pytestmark = test.__doc__, list(getattr(test, "pytestmark", ()))
    return pytest.mark.gpu(twin)


# ---------------------------------------------------------------------------------------------------------------- the operand rules
def _f64(w):
    return torch.as_tensor(w).to(torch.float64)


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


@dataclasses.dataclass(frozen=True)
class Rule:
    """one reduced precision: how it is spelled, and how the yardstick rounds the operands of a contraction (fp64 out)"""
    name: str                       # in labels and test ids
    value: object                   # Python's value, and `code`, the C entry points'
    code: int
    spellings: tuple                # what else Python takes for `value`
    q: typing.Callable              # an activation operand (fp64 in)
    dec_weight: typing.Callable     # a decoder weight operand, from the checkpoint's fp32 weight
    voc_weight: typing.Callable     # a vocoder weight operand, from (weight, "its convolution runs inside a one-launch ResBlock")
    walk_bound: float               # L-inf between the decoder's chunk walk and its window form (check_chunk_walk)
    far_from_32: float              # a lower bound on the L-inf between a tiny-ES mel at this precision and at 32
    decoder_kernel: str             # the decoder kernel's name in the launch log

    def __str__(self):
        return self.name


# A kept row's operand values are the same values in the chunk walk and in the window form up to fp32 accumulation order (1e-6), so they
# round to the same binary16: 2e-6 (the bound of check_decoder_chunk_walk).  One crossed bfloat16 rounding boundary moves the mel by 2^3
# times what a crossed binary16 boundary does: 2e-5 on the same reasoning.  far_from_32: 20 to 30 times below max|E_q| of tiny ES and at least
# 100 times above fp32 noise.
R16 = Rule("16", 16, 16, ("16-mixed",), q=lambda t: t.to(torch.float16).to(torch.float64),
           dec_weight=lambda w: (_f64(w) * 256.0).to(torch.float16).to(torch.float64) / 256.0,     # round16(2^8 w) / 2^8: plane 0
           voc_weight=lambda w, one_launch: _f64(w).to(torch.float16).to(torch.float64),           # binary16(w) in either family
           walk_bound=2e-6, far_from_32=1e-4, decoder_kernel="mel_decoder_kernel<DX2,KD,NW,true>")
BF16 = Rule("bf16", "bf16", _lib.PRECISION_BF16, ("bf16-mixed",), q=q_bf16, dec_weight=w_two_plane,
            voc_weight=lambda w, one_launch: w_two_plane(w) if one_launch else w_bf16(w),
            walk_bound=2e-5, far_from_32=1e-3, decoder_kernel="mel_decoder_bf16_kernel<DX2,KD,NW>")
RULES = (R16, BF16)


def other(rule):
    return BF16 if rule is R16 else R16


def check_rules_agree_almost_everywhere():
    """the two bf16 weight rules differ on about one weight in 2^13, by one bfloat16 ulp (include/esmi.h says so): on 2^20 normal weights
    fewer than 2^20 / 2^11 differ, and none by more than one ulp"""
    w = torch.from_numpy(np.random.default_rng(0).standard_normal(1 << 20).astype(np.float32) * 0.1)
    a, b = w_bf16(w), w_two_plane(w)
    differ = a != b
    assert int(differ.sum()) < (1 << 9), int(differ.sum())
    ulp = torch.ldexp(torch.ones_like(a), torch.floor(torch.log2(a.abs().clamp_min(1e-30))) - 7)
    assert bool(((a - b).abs() <= ulp * 1.0001)[differ].all())


# ---------------------------------------------------------------------------------------------------------------- models
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


def reduced_config(resblock=1):
    """the reduced generator of tests/test_vocoder_dispatch.py: 256 -> 128 / 64 / 32 channels, rates (2, 2, 2), k = 3 and 7, 16 mels"""
    return HifiGanConfig(resblock=str(resblock), upsample_rates=(2, 2, 2), upsample_kernel_sizes=(4, 4, 4), upsample_initial_channel=256,
                         resblock_kernel_sizes=(3, 7), resblock_dilation_sizes=((1, 3, 5),) * 2 if resblock == 1 else ((1, 3),) * 2,
                         num_mels=16)


def small_config(num_mels=8):
    """the smallest generator with both launch families: 32 -> 16 / 8 channels (one-launch ResBlocks on the 16-row tiles), rates (2, 2),
    one k = 3 ResBlock1 per stage, 8 mels -- for checks that only compare calls with each other on the simulator (80 mels: behind tiny ES)"""
    return HifiGanConfig(resblock="1", upsample_rates=(2, 2), upsample_kernel_sizes=(4, 4), upsample_initial_channel=32,
                         resblock_kernel_sizes=(3,), resblock_dilation_sizes=((1, 3, 5),), num_mels=num_mels)


def vocoder_config_of(name):
    """"v1" / "v2" / "v3", "small", "small80", "reduced1" / "reduced2\""""
    if name in HIFIGAN_CONFIGS:
        return HIFIGAN_CONFIGS[name]
    return small_config(80 if name == "small80" else 8) if name.startswith("small") else reduced_config(int(name[-1]))


def make_vocoder(name, device, fused=True, precision=32):
    h = vocoder_config_of(name)
    voc = Generator(h, precision=precision)
    voc.load_state_dict({k: torch.from_numpy(v) for k, v in synth_hifigan_state_dict(h, 1234).items()}, strict=True)
    voc = voc.to(device).eval()
    voc.fuse_resblocks = fused
    return voc


# ---------------------------------------------------------------------------------------------------------------- the yardsticks
def decoder_mirror(cfg, sd, feats, rule, proj_rounded=None, stats=None):
    """MelDecoder.forward (layers/networks.py:291-304) in fp64 on host tensors: feats (B, L, 4 dim) -> mel (B, L, n_mel); every Conv1d
    zero-pads outside [0, L).  rule None: exact.  Else the input and the weight of the pointwise convolutions, of the mel Linear and
    (proj_rounded, default True: the kernel runs the stage itself; False when it gathers a phoneme-rate h0, which the encoder side computes
    fp32-accurately) of the proj Linear go through the rule.  stats (a dict): receives "operand_max", the largest |input| of a rounded
    contraction."""
    proj_rounded = rule is not None and proj_rounded is not False

    def q(t, on):
        if on and stats is not None:
            stats["operand_max"] = max(stats.get("operand_max", 0.0), float(t.abs().max()))
        return rule.q(t) if on else t
    rounded = rule is not None
    W = lambda key: _f64(sd["decoder." + key])                                                 # noqa: E731
    qw = lambda key, on: rule.dec_weight(sd["decoder." + key]) if on else W(key)               # noqa: E731
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


def vocoder_mirror(h, sd, mel, rule, fused):
    """Generator.forward in fp64 on host tensors.  mel (B, L, num_mels) -> wav (B, L * hop).  The mean over a stage's ResBlocks is folded
    into the next input scale, as the library does.  rule None: exact.  Else every convolution's input (after its leaky_relu) and weight go
    through the rule, except conv_post's; a ResBlock runs as one launch when `fused` and its stage has 8 / 16 / 32 / 64 channels and k in
    {3, 7, 11} (the library's resblock_fused_ok -- the launch-log tests pin which kernels ran)."""
    q = rule.q if rule is not None else (lambda t: t)
    W = lambda key: _f64(sd[key])                                # noqa: E731
    qw = (lambda key, one_launch: rule.voc_weight(sd[key], one_launch)) if rule is not None else (lambda key, one_launch: W(key))
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


def rms(t):
    return float(t.to(torch.float64).pow(2).mean().sqrt())


class Yardsticks:
    """(exact, E_q, stats) per (rule, case key): computed once, shared, never modified (a module-scoped fixture owns it).  The exact run
    is shared between the rules, and between the case keys that name the same `exact_key`."""

    def __init__(self):
        self.exact, self.runs = {}, {}

    def get(self, rule, key, run, mel_len=None, exact_key=None):
        """run(rule or None, stats) -> the mirror's output.  mel_len: the final masked_fill -- rows behind an utterance's end are zero
        in both modes."""
        exact_key = key if exact_key is None else exact_key
        if exact_key not in self.exact:
            self.exact[exact_key] = run(None, None)
        if (rule.name, key) not in self.runs:
            stats = {}
            exact = self.exact[exact_key]
            eq = run(rule, stats) - exact
            if mel_len is not None:
                keep = torch.arange(exact.shape[1])[None, :] < torch.as_tensor(mel_len).cpu().long()[:, None]
                exact, eq = exact * keep[..., None], eq * keep[..., None]
            self.runs[(rule.name, key)] = (exact, eq, stats)
        return self.runs[(rule.name, key)]

    def decoder(self, rule, key, cfg, sd, feats, proj_rounded=True, mel_len=None):
        return self.get(rule, key, lambda r, stats: decoder_mirror(cfg, sd, feats, r, proj_rounded, stats), mel_len)

    def vocoder(self, rule, name, B, L, fused):
        """name in FIXTURES with B None: the committed fixture's mel; else make_mel(h, B, L) -> (mel, exact, E_q)"""
        h = vocoder_config_of(name)
        sd = synth_hifigan_state_dict(h, 1234)
        if B is None:
            g = np.load(os.path.join(GOLD, FIXTURES[name]))
            assert str(g["config"]) == name
            mel = torch.from_numpy(g["mel"])
        else:
            mel = make_mel(h, B, L, "cpu")
        exact, eq, _ = self.get(rule, ("voc", name, B, L, fused), lambda r, stats: vocoder_mirror(h, sd, mel, r, fused),
                                exact_key=("voc", name, B, L))
        return mel, exact, eq

    def clear(self):
        self.exact.clear()
        self.runs.clear()


def judge(what, got, exact, eq):
    """The verdict: e = got - exact against E_q; every figure is printed before it is asserted.  The lower bound proves that the
    precision's own product ran; the upper bounds catch a truncating conversion or a wrong plane."""
    assert got.dtype == torch.float32 and tuple(got.shape) == tuple(exact.shape)
    e = got.cpu().to(torch.float64) - exact
    finite = bool(torch.isfinite(got).all())
    r_rms, r_max = rms(e) / rms(eq), float(e.abs().max()) / float(eq.abs().max())
    print(f"{what} {tuple(exact.shape)}: rms(e) {rms(e):.3e} = {r_rms:.3f} rms(E_q); max|e| {float(e.abs().max()):.3e} = {r_max:.3f} max|E_q|; "
          f"max|exact| {float(exact.abs().max()):.2f} finite={finite}")
    assert finite
    assert r_rms <= RMS_HI, r_rms
    assert r_max <= MAX_HI, r_max
    assert r_rms >= RMS_LO, r_rms
    return r_rms, r_max


def check_mirror_matches_oracle(rule, name):
    """Test 0: the decoder mirror's exact mode against oracle.mel_decoder (fp64) < 1e-6 L-inf -- three orders below E_q; the rounded mode
    rounds, and E_q(bf16) is several times E_q(f16)."""
    from oracle import oracle
    cfg, sd = state_dict_of(name)
    feats = np.random.default_rng(5).standard_normal((2, 37, cfg.d4)).astype(np.float32)
    ref = oracle.mel_decoder(cfg, oracle.Weights(sd), feats)
    exact = decoder_mirror(cfg, sd, feats, None)
    eq = {r: decoder_mirror(cfg, sd, feats, r) - exact for r in RULES}
    err = float((exact - torch.from_numpy(ref).double()).abs().max())
    print(f"{name}: mirror vs oracle L-inf {err:.2e}; E_q({rule}) L-inf {float(eq[rule].abs().max()):.2e} rms {rms(eq[rule]):.2e}; "
          f"E_q(bf16) = {rms(eq[BF16]) / rms(eq[R16]):.1f} x E_q(16)")
    assert err < 1e-6, err
    assert rms(eq[rule]) > 1e-4
    assert rms(eq[BF16]) > 4 * rms(eq[R16])


def check_mirror_matches_fixture(yard, rule, name):
    """Test 0: the vocoder mirror's exact mode against the reference-generated waveform (measured: 1.9e-7 / 2.7e-7 / 4.4e-7 L-inf for
    v1 / v2 / v3)."""
    _mel, exact, eq = yard.vocoder(rule, name, None, None, True)
    ref = torch.from_numpy(np.load(os.path.join(GOLD, FIXTURES[name]))["wav"]).to(torch.float64)
    err = float((exact - ref).abs().max())
    print(f"{name}: mirror vs fixture L-inf {err:.2e}; E_q({rule}) L-inf {float(eq.abs().max()):.2e} rms {rms(eq):.2e}")
    assert err < 2e-6, err


# ---------------------------------------------------------------------------------------------------------------- decoder: the C-ABI, driven directly
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


def frame_features(feat, dur, L):
    """the length regulator on the host: phoneme-rate feat (B, T, C) + durations (B, T) -> (B, L, C), zero rows behind each utterance"""
    feat, dur = torch.as_tensor(feat).cpu(), torch.as_tensor(dur).cpu().long()
    out = torch.zeros((feat.shape[0], L, feat.shape[2]), dtype=feat.dtype)
    for b in range(feat.shape[0]):
        rows = torch.repeat_interleave(feat[b], dur[b], dim=0)[:L]
        out[b, :rows.shape[0]] = rows
    return out


def free_running_batch(device, T=42, lengths=(42, 27, 6), scale=None):
    """a ragged free-running batch for tiny ES: predicted durations (the synthetic weights predict about 3.6 frames per phoneme: the batch
    is about 150 frames long; `scale`: an optional duration_control)"""
    ids, mask = synth_phonemes(len(lengths), T, 7, list(lengths))
    x = {"phoneme": torch.from_numpy(ids).to(device), "phoneme_mask": torch.from_numpy(mask).to(device)}
    if scale is not None:
        x["duration_control"] = float(scale)
    return x


def _forced_batch(device, B=3, T=12, lens=(12, 7, 3)):
    ids, mask = synth_phonemes(B, T, 12, list(lens))
    dur = np.random.default_rng(3).integers(1, 4, size=(B, T)).astype(np.int32)
    dur[mask] = 0
    x = {"phoneme": torch.from_numpy(ids).to(device), "phoneme_mask": torch.from_numpy(mask).to(device),
         "duration_forced": torch.from_numpy(dur).to(device)}
    return ids, dur, x


@contextlib.contextmanager
def decoder_default(net, precision):
    """`net.decoder.precision`, the default of the inference paths, set inside the block"""
    net.decoder.precision = precision
    try:
        yield
    finally:
        net.decoder.precision = 32


# ---------------------------------------------------------------------------------------------------------------- decoder: accuracy and invariants
def check_direct(yard, rule, name, B, L, device, profile=None):
    """Test 1, direct mode (the kernel runs its first stage itself: `proj` through mma_sub) through MelDecoder.forward(precision=); the
    default call made after it is untouched by it."""
    net, cfg, sd = make_net(name, device, profile)
    feats = torch.from_numpy(np.random.default_rng(7).standard_normal((B, L, cfg.d4)).astype(np.float32))
    exact, eq, _ = yard.decoder(rule, ("direct", name, profile, B, L), cfg, sd, feats)
    with torch.no_grad():
        mel = net.decoder(feats.to(device), precision=rule.value)
        mel32 = net.decoder(feats.to(device))
    assert float((mel32.cpu().double() - exact).abs().max()) < 1e-4
    return judge(f"{rule} {name}{'+' + profile if profile else ''} direct", mel, exact, eq)


def check_beyond_binary16(yard, device):
    """bf16's test 2: direct mode, tiny, B = 2, L = 40, one feature entry per utterance set to 1e5 -- out of binary16's range (the
    mirror's largest rounded operand is >= 65520), inside bfloat16's: the bf16 mel is finite and inside the band."""
    net, cfg, sd = make_net("tiny", device)
    feats = torch.from_numpy(np.random.default_rng(7).standard_normal((2, 40, cfg.d4)).astype(np.float32))
    feats[0, 11, 5] = 1e5
    feats[1, 29, 77] = -1e5
    exact, eq, stats = yard.decoder(BF16, ("beyond", "tiny"), cfg, sd, feats)
    assert stats["operand_max"] >= 65520.0, stats
    with torch.no_grad():
        mel = net.decoder(feats.to(device), precision=BF16.value)
    return judge("bf16 tiny direct, |x| = 1e5", mel, exact, eq)


def check_chunk_walk(yard, rule, name, B, T, D, device):
    """Test 1 + the chunk-walk invariant: the fused gather without h0 (in-kernel `proj`) with a workspace (dx2 = 256: the chunk walk) and
    without one (the window form), both at the rule's precision: each within the band, and the two agree to `rule.walk_bound`."""
    net, cfg, sd = make_net(name, device)
    feat = torch.from_numpy(np.random.default_rng(17).standard_normal((B, T, cfg.d4)).astype(np.float32))
    dur, cum, mel_len = ragged_durations(B, T, D, device)
    L = int(mel_len.max())
    exact, eq, _ = yard.decoder(rule, ("walk", name, B, T, D), cfg, sd, frame_features(feat, dur, L), mel_len=mel_len)
    outs = []
    for use_ws in (True, False):
        mel, n = run_decoder(net, cfg, feat.to(device), rule.code, cum, mel_len, workspace=use_ws)
        assert (n > 0) == (use_ws and cfg.dx2 == 256)
        judge(f"{rule} {name} fused gather, {'chunk walk' if n else 'window form'}", mel, exact, eq)
        outs.append(mel.cpu())
    d = float((outs[0] - outs[1]).abs().max())
    print(f"{name}: chunk walk vs window form at {rule}: L-inf {d:.2e}")
    assert d < rule.walk_bound, d


def check_forward_with_h0(yard, rule, device):
    """Test 1 + the invariants, tiny ES, the whole forward, free-running, B = 3 ragged, L ~ 150: the decoder gathers the phoneme-rate h0
    (two windows; edge rows outside [0, L); one utterance short enough to leave padding frames).
    Invariants: mel_len, duration, dur and cum bit-identical between the rule's precision and 32; rows >= mel_len[b] exactly 0; the
    precision twice, and under its other spellings, the same bits; the key at 32 (the general entry point) the bits of the call without
    the key; neither the mel of 32 nor that of the other reduced precision.  (The yardstick is keyed by the device: its input is that
    tier's own encoder output.)"""
    net, cfg, sd = make_net("tiny", device)
    x = free_running_batch(device)
    with torch.no_grad():
        enc = net.encoder._encode(x)
        s32 = net._launch(x, taps=True)
        sr = net._launch(dict(x, decoder_precision=rule.value), taps=True)
        again = [net._launch(dict(x, decoder_precision=p)) for p in (rule.value,) + rule.spellings]
        s32k = net._launch(dict(x, decoder_precision=32))
        so = net._launch(dict(x, decoder_precision=other(rule).value))
    ml = s32.mel_len.cpu()
    L = int(ml.max())
    print(f"tiny free-running: mel_len {ml.tolist()}")
    assert 113 <= L <= 224 and int(ml.min()) < L - 20 and sr.mel.shape == (3, L, cfg.n_mel_channels)
    assert torch.equal(sr.mel_len, s32.mel_len) and torch.equal(sr.duration, s32.duration)
    for k in ("dur", "cum", "pitch_idx", "energy_idx"):
        assert torch.equal(sr.taps[k], s32.taps[k]), k
    assert np.array_equal(sr.taps["cum"].cpu().numpy(), s32.taps["cum"].cpu().numpy())
    assert all(torch.equal(sr.mel, s.mel) for s in again) and torch.equal(s32k.mel, s32.mel)
    assert not torch.equal(sr.mel, s32.mel) and not torch.equal(sr.mel, so.mel)
    for b in range(3):
        assert not bool(sr.mel[b, int(ml[b]):].any()) and bool(sr.mel[b, :int(ml[b])].abs().sum() > 0)
    assert torch.equal(enc["dur"].cpu(), s32.taps["dur"].cpu())
    feats = frame_features(enc["feat"], s32.taps["dur"], L)
    exact, eq, _ = yard.decoder(rule, ("fwd", "tiny", str(device)), cfg, sd, feats, proj_rounded=False, mel_len=ml)
    assert float((s32.mel.cpu().double() - exact).abs().max()) < 1e-4
    return judge(f"{rule} tiny forward, fused gather with h0", sr.mel, exact, eq)


def check_entry_points(name, device, B=2, T=12, D=5):
    """Test 3: precision 0 / 32 through esmi_mel_decoder_prec_f32 are esmi_mel_decoder_f32 bit for bit (fused gather, ragged); 16 and bf16
    are each reproducible, differ from each other and from 32, bf16 is further from 32 than 16 is, and 16 stays within 0.1 of it."""
    net, cfg, sd = make_net(name, device)
    feat = torch.from_numpy(np.random.default_rng(3).standard_normal((B, T, cfg.d4)).astype(np.float32)).to(device)
    _dur, cum, mel_len = ragged_durations(B, T, D, device)
    plain, _ = run_decoder(net, cfg, feat, 32, cum, mel_len, entry="plain")
    assert bool(torch.isfinite(plain).all())
    for precision in (0, 32):
        got, _ = run_decoder(net, cfg, feat, precision, cum, mel_len)
        assert torch.equal(got, plain), precision
    p16, pb, pb2, p16b = (run_decoder(net, cfg, feat, r.code, cum, mel_len)[0] for r in (R16, BF16, BF16, R16))
    assert torch.equal(pb, pb2) and torch.equal(p16, p16b)
    d16, db = float((p16 - plain).abs().max()), float((pb - plain).abs().max())
    print(f"{name}: L-inf to precision 32: 16 {d16:.2e}, bf16 {db:.2e}")
    assert 0 < d16 < db < 0.5 and d16 < 0.1


def check_range_check_honours_the_key(rule, device):
    """Phoneme2Mel.check_activation_range (the range-checked build; what ESMI_DEBUG_RANGE=1 runs first) with the key returns that build's
    forward at the rule's precision, bit for bit, not its precision-32 one (at bf16 it has nothing to check, and does not fall back).
    Compared inside ONE build: the checked build's encoder side differs from the product build's by fp32 rounding (2e-6, at any
    precision), and at precision 16 such a difference crosses binary16 rounding boundaries in the decoder -- two precision-16 mels from
    inputs 2e-6 apart are 1e-3 apart, a third of max|E_q| (measured; the decoder kernels of the two builds agree bit for bit on equal
    inputs)."""
    net, cfg, sd = make_net("tiny", device)
    ids, mask = synth_phonemes(2, 12, 3, [12, 6])
    x = {"phoneme": torch.from_numpy(ids).to(device), "phoneme_mask": torch.from_numpy(mask).to(device), "decoder_precision": rule.value}
    checked = os.path.join(os.path.dirname(_lib.LIB_PATH), "libesmi_checked.so")
    with torch.no_grad():
        with (_lib.use_library(checked) if str(device).startswith("cuda") else contextlib.nullcontext()):
            mel, mel_len, _ = net(x)
            mel32, _len32, _ = net(dict(x, decoder_precision=32))
        got, got_len, _ = net.check_activation_range(x)
    d32 = float((got - mel32).abs().max())
    print(f"checked build with the key at {rule}: L-inf to its precision-32 mel {d32:.2e}")
    assert torch.equal(got_len, mel_len) and torch.equal(got, mel)
    assert d32 > rule.far_from_32


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
        with decoder_default(net, 16):
            got = net(xt, train=True)["mel"]
    assert torch.equal(got, ref) and float(ref.abs().max()) > 0.1


# ---------------------------------------------------------------------------------------------------------------- decoder: the interfaces
def check_synthesize(rule, device, small=False):
    """synthesize(precision=p, decoder_precision=p) is Generator.forward(mel_p, lengths, precision=p) bit for bit; finite; wav_len and
    duration those of precision 32; each argument alone (under the other spelling) changes only its half; the key leaves the attribute
    alone; Generator(h, precision=p) and the attribute `decoder.precision = p` are the defaults and the key overrides the attribute; tiny
    ES + v2 (small: the smallest 80-mel generator), B = 3, T = 12, forced durations."""
    from efficientspeech_amd import EfficientSpeech
    name, p, spelled = "small80" if small else "v2", rule.value, rule.spellings[0]
    voc = make_vocoder(name, device)
    model = EfficientSpeech.from_config("tiny", hifigan=voc)
    model.phoneme2mel.load_state_dict({k: torch.from_numpy(v) for k, v in synth_state_dict(CONFIGS["tiny"], 1234).items()}, strict=True)
    model = model.to(device).eval()
    _ids, _dur, x = _forced_batch(device)
    net = model.phoneme2mel
    with torch.no_grad():
        mel32, len32, _ = net(x, train=False)
        melp, lenp, _ = net(dict(x, decoder_precision=p), train=False)
        assert net.decoder.precision == 32
        wav32, wlen32, dur32 = model.synthesize(x)
        wavpp, wlenpp, durpp = model.synthesize(x, precision=p, decoder_precision=p)
        wavp_, _, _ = model.synthesize(x, precision=spelled)
        wav_p, _, _ = model.synthesize(x, decoder_precision=spelled)
        assert torch.equal(wavpp, voc(melp.transpose(1, 2), lengths=lenp, precision=p)[:, 0])
        assert torch.equal(wavp_, voc(mel32.transpose(1, 2), lengths=len32, precision=p)[:, 0])
        assert torch.equal(wav_p, voc(melp.transpose(1, 2), lengths=lenp)[:, 0])
        for bad in BAD:
            with pytest.raises(ValueError, match="precision"):
                model.synthesize(x, precision=bad)
            with pytest.raises(ValueError, match="precision"):
                model.synthesize(x, decoder_precision=bad)
        with decoder_default(net, p):
            assert "precision" not in " ".join(net.decoder.state_dict())
            assert torch.equal(net(x, train=False)[0], melp)
            assert torch.equal(net(dict(x, decoder_precision=32), train=False)[0], mel32)
        vocp = make_vocoder(name, device, precision=spelled)
        assert vocp.precision == p
        assert torch.equal(vocp(melp.transpose(1, 2), lengths=lenp)[:, 0], wavpp)
    assert bool(torch.isfinite(wavpp).all()) and float(wavpp.abs().max()) > 1e-3
    assert torch.equal(lenp, len32) and torch.equal(wlenpp, wlen32) and torch.equal(durpp, dur32)
    assert not torch.equal(melp, mel32) and not torch.equal(wavpp, wav32) and not torch.equal(wavpp, wavp_) and not torch.equal(wavpp, wav_p)
    assert not torch.equal(wav_p, wav32)


def check_scheduler(rule, device):
    """(no vocoder) a BucketedSynthesizer whose `extra` adds the key gives the direct call's mels at the rule's precision, bit for bit,
    and not the precision-32 ones; tiny ES, three requests of 12 / 7 / 3 phonemes, forced durations."""
    from efficientspeech_amd import BucketedSynthesizer
    net, cfg, sd = make_net("tiny", device)
    lens = [12, 7, 3]
    ids, dur, _x = _forced_batch(device, lens=lens)
    seqs = [ids[b, :n].astype(np.int32) for b, n in enumerate(lens)]

    def extra(idx, T_):
        d = np.zeros((len(idx), T_), np.int32)
        for r, i in enumerate(idx):
            d[r, :lens[i]] = dur[i, :lens[i]]
        return {"duration_forced": torch.from_numpy(d).to(device), "decoder_precision": rule.value}
    res = BucketedSynthesizer(net, max_batch=1, granularity=4)(seqs, extra=extra)
    for i, (mel_i, _dur_i) in enumerate(res):
        xi = {"phoneme": torch.from_numpy(seqs[i][None]).to(device), "duration_forced": torch.from_numpy(dur[i:i + 1, :lens[i]]).to(device)}
        with torch.no_grad():
            alone = net(dict(xi, decoder_precision=rule.value))[0][0]
            alone32 = net(xi)[0][0]
        assert mel_i.shape == (int(dur[i, :lens[i]].sum()), 80) and torch.equal(mel_i, alone) and not torch.equal(mel_i, alone32), i


def check_staged_forward(rule, device):
    """The key through the staged calls that sharded_forward / ShardedMelPipeline make (`_launch(stage=1)`, then `_launch(stage=2)` on
    the returned state: the state carries the precision), through a ShardedMelPipeline step and through sharded_forward: the one-call
    forward's bits at the rule's precision, with and without a caller-supplied output length; and the decoder's attribute as the default
    of the same paths, which the key at 32 overrides."""
    from efficientspeech_amd.sharded import ShardedMelPipeline, sharded_forward
    net, cfg, sd = make_net("tiny", device)
    _ids, dur, x = _forced_batch(device)
    xr = dict(x, decoder_precision=rule.value)
    with torch.no_grad():
        one, one32 = net._launch(xr), net._launch(x)
        assert not torch.equal(one.mel, one32.mel)
        for more in ({}, {"max_mel_len": int(dur.sum(1).max()) + 5}):
            ref = one.mel if not more else net._launch(dict(xr, **more)).mel
            st = net._launch(dict(xr, **more), stage=1)
            assert st.precision == rule.value and st.mel is None
            st = net._launch(None, stage=2, state=st)
            assert torch.equal(st.mel, ref) and torch.equal(st.mel_len, one32.mel_len), more
        mel, mel_len = ShardedMelPipeline(net).step(xr)
        assert torch.equal(mel, one.mel) and torch.equal(mel_len, one32.mel_len)
        mel, mel_len, _dur = sharded_forward(net, xr)            # (one rank: its world-size-1 form; the staged calls are the ones above)
        assert torch.equal(mel, one.mel) and torch.equal(mel_len, one32.mel_len)
        with decoder_default(net, rule.value):
            st = net._launch(None, stage=2, state=net._launch(x, stage=1))
            assert torch.equal(st.mel, one.mel)
            st = net._launch(None, stage=2, state=net._launch(dict(x, decoder_precision=32), stage=1))
            assert torch.equal(st.mel, one32.mel)


def check_graph_replay(rule, device):
    """The graph-replay path (GPU only): GraphedForward / ShardedMelPipeline(use_graph=True) capture the decoder at the precision the
    first batch asks for -- the eager bits of that precision --, replay it under its other spellings, and refuse a later step that asks
    for 32 or for the other reduced precision (NotImplementedError), also when the attribute changed behind a captured graph; nothing is
    dropped."""
    from efficientspeech_amd.sharded import GraphedForward, ShardedMelPipeline, _encode_with_head
    net, cfg, sd = make_net("tiny", device)
    _ids, dur, x = _forced_batch(device)
    x = dict(x, max_mel_len=int(dur.sum(1).max()))
    xr = dict(x, decoder_precision=rule.value)
    L = x["max_mel_len"]

    def eager(precision):                             # the two calls the graphs capture, run eagerly
        enc = _encode_with_head(net, x)
        return net.decoder._fused(enc["feat"], enc["cum"], enc["mel_len"], enc["lmax"], L, True, L, h0=enc["h0"], precision=precision)
    with torch.no_grad():
        ref, ref32 = eager(rule.value), eager(32)
        assert not torch.equal(ref, ref32)
        pipe = ShardedMelPipeline(net, use_graph=True)
        mel, _len = pipe.step(xr)
        torch.cuda.synchronize()
        assert pipe.graphed is not None and pipe.graphed.precision == rule.value
        assert torch.equal(mel, ref) and not torch.equal(mel, ref32)
        for spelled in rule.spellings:                # (the same precision under its other spelling: replayed)
            mel2, _len = pipe.step(dict(x, decoder_precision=spelled))
            torch.cuda.synchronize()
            assert torch.equal(mel2, ref)
        for bad in (x, dict(x, decoder_precision=32), dict(x, decoder_precision=other(rule).value)):
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
            g.load(xr)
        with decoder_default(net, rule.value):        # the attribute changed behind a captured graph: refused too
            with pytest.raises(NotImplementedError, match="decoder_precision"):
                g.load(x)
    with pytest.raises(ValueError, match="precision"):
        GraphedForward(net, dict(x, decoder_precision=8))


def check_graph_replay_refuses_an_invalid_key():
    """(host side only: the graph path validates the key before it touches the device)"""
    from efficientspeech_amd.sharded import ShardedMelPipeline
    pipe = ShardedMelPipeline(make_net("tiny", "cpu")[0], use_graph=True)
    for bad in BAD:
        with pytest.raises(ValueError, match="precision"):
            pipe.step({"phoneme": torch.ones((1, 4), dtype=torch.int32), "max_mel_len": 16, "decoder_precision": bad})
    assert pipe.graphed is None


# ---------------------------------------------------------------------------------------------------------------- refusals
def python_refusals(rule, device):
    """ValueError (its text contains "precision") for every value of BAD from every Python entry, and for the key at the rule's precision
    with train=True"""
    net, cfg, sd = make_net("tiny", device)
    feat = torch.from_numpy(np.random.default_rng(3).standard_normal((2, 9, cfg.d4)).astype(np.float32)).to(device)
    ids, mask = synth_phonemes(2, 9, 1, [9, 4])
    x = {"phoneme": torch.from_numpy(ids).to(device), "phoneme_mask": torch.from_numpy(mask).to(device)}
    voc = make_vocoder("small", device)
    mel = make_mel(voc.h, 1, 4, device)
    for bad in BAD:
        with pytest.raises(ValueError, match="precision"), torch.no_grad():
            net(dict(x, decoder_precision=bad))
        with pytest.raises(ValueError, match="precision"), torch.no_grad():
            net.decoder(feat, precision=bad)
        with pytest.raises(ValueError, match="precision"):
            Generator(reduced_config(), precision=bad)
        with pytest.raises(ValueError, match="precision"):
            networks._decoder_precision(bad)
        with pytest.raises(ValueError, match="precision"), torch.no_grad():
            voc(mel.transpose(1, 2), precision=bad)
    xt = dict(x, decoder_precision=rule.value, pitch=torch.zeros((2, 9), device=device), energy=torch.zeros((2, 9), device=device),
              duration=torch.ones((2, 9), dtype=torch.int32, device=device), mel_len=torch.tensor([9, 4], dtype=torch.int32, device=device))
    with pytest.raises(ValueError, match="decoder_precision"), torch.no_grad():
        net(xt, train=True)


def check_python_refusals(rule, device):
    """python_refusals, and the one validator behind them: training's is inference's, and it knows the reference's spellings"""
    from efficientspeech_amd import train
    python_refusals(rule, device)
    assert train.normalize_precision is _lib.normalize_precision
    for r in RULES:
        assert all(train.normalize_precision(s) == r.value and networks._decoder_precision(s) == r.value for s in r.spellings)
        assert networks._decoder_precision(None, r.value) == r.value


def check_refusals_launch_nothing(rule):
    """On the simulator: precision 8 is ESMI_ERR_ARG from each of the four C entry points (the whole-forward ones refuse before the encoder
    side is enqueued), the Python entries refuse as python_refusals says, and the launch log shows that nothing was enqueued in any of
    them."""
    from tests.simlib import launch_records
    net, cfg, sd = make_net("tiny", "cpu")
    feat = torch.from_numpy(np.random.default_rng(3).standard_normal((2, 9, cfg.d4)).astype(np.float32))
    run_decoder(net, cfg, feat, 32)                      # (weights packed: the records below are the calls' alone)
    ids, mask = synth_phonemes(2, 9, 1, [9, 4])
    with torch.no_grad():
        net({"phoneme": torch.from_numpy(ids), "phoneme_mask": torch.from_numpy(mask)})
    voc = make_vocoder("small", "cpu")
    mel = make_mel(voc.h, 1, 4, "cpu")
    run_prec(voc, mel, 32)
    lib, stream = networks._runtime(net.decoder.mel_linear.weight)
    a = net._static_args(lib, stream)
    with launch_records() as records:
        with pytest.raises(RuntimeError, match="esmi_mel_decoder_prec_f32 failed: ESMI_ERR_ARG"):
            run_decoder(net, cfg, feat, 8)
        with pytest.raises(RuntimeError, match="esmi_phoneme2mel_forward_prec_f32 failed: ESMI_ERR_ARG"):
            lib.esmi_phoneme2mel_forward_prec_f32(C.byref(a), None, 8, 0, stream)
        with pytest.raises(RuntimeError, match="esmi_phoneme2mel_forward_curve_f32 failed: ESMI_ERR_ARG"):
            lib.esmi_phoneme2mel_forward_curve_f32(C.byref(a), None, 8, 0, stream)
        with pytest.raises(RuntimeError, match="esmi_hifigan_generator_prec_f32 failed: ESMI_ERR_ARG"):
            run_prec(voc, mel, 8)
        python_refusals(rule, "cpu")
    assert records == []


def check_vocoder_refusals(device):
    """The vocoder's own (simulator: the launch log shows that nothing was enqueued): ESMI_ERR_ARG for precision 8 and for a PCM plane
    without lengths."""
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


def check_fp32mfma_refuses(rule, lib_path):
    """libesmi_fp32mfma.so has no one-product path: the rule's precision is ESMI_ERR_UNSUPPORTED from the four entry points, decided on
    the host before anything is enqueued (no device is touched: this runs without a GPU); 8 stays ESMI_ERR_ARG"""
    lib = _lib.bind(C.CDLL(lib_path))
    assert lib.esmi_build_config().decode().startswith("dec_gemm=fp32-mfma")
    shape = _lib.DecoderShape(128, 128, 5, 2, 2, 80)
    buf = (C.c_float * 64)()                             # aligned stand-ins: a refused call reads none of them
    p = C.cast(C.byref(buf), C.c_void_p)
    with pytest.raises(_lib.Unsupported):
        lib.esmi_mel_decoder_prec_f32(p, C.byref(shape), p, None, None, None, None, 4, 0, 1, 0, 4, p, None, 0, rule.code, None)
    with pytest.raises(RuntimeError, match="ESMI_ERR_ARG"):
        lib.esmi_mel_decoder_prec_f32(p, C.byref(shape), p, None, None, None, None, 4, 0, 1, 0, 4, p, None, 0, 8, None)
    a = _lib.ForwardArgs()
    with pytest.raises(_lib.Unsupported):
        lib.esmi_phoneme2mel_forward_prec_f32(C.byref(a), None, rule.code, 0, None)
    with pytest.raises(_lib.Unsupported):
        lib.esmi_phoneme2mel_forward_curve_f32(C.byref(a), None, rule.code, 0, None)
    s = _lib.HifiGanShape(n_mel=8, initial_channel=32, n_up=1, n_kernels=1, resblock=1)
    s.up_rates[0], s.up_kernels[0], s.rb_kernels[0] = 2, 4, 3
    w = _lib.HifiGanWeights()
    with pytest.raises(_lib.Unsupported):
        lib.esmi_hifigan_generator_prec_f32(C.byref(w), C.byref(s), p, 1, 4, None, p, None, rule.code, p, 1 << 20, None)


# ---------------------------------------------------------------------------------------------------------------- vocoder
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


def check_vocoder_accuracy(yard, rule, name, device, fused, B=None, L=None):
    """Test 1: e = wav - exact against E_q, the band (the default path sits at 5e-8 rms)"""
    mel, exact, eq = yard.vocoder(rule, name, B, L, fused)
    voc = make_vocoder(name, device, fused=fused)
    with torch.no_grad():
        wav = voc(mel.to(device).transpose(1, 2), precision=rule.value)
    assert wav.shape == (mel.shape[0], 1, mel.shape[1] * voc.h.hop)
    return judge(f"{rule} vocoder {name} fused={fused}", wav[:, 0], exact, eq)


def check_ragged_contract(rule, name, B, L, lengths, device, modes=(True, False), module=True):
    """Test 2: at the rule's precision the length-aware call's kept samples are the plain run's bit for bit, the tails exact zeros
    (workspace and outputs NaN-filled on entry), and the PCM plane is trunc(clamp(wav * 32768, -32768, 32767)); it is neither the other
    reduced precision's run nor the default's, and the module passes the precision on under every spelling."""
    for fused in modes:
        voc = make_vocoder(name, device, fused=fused)
        mel = make_mel(voc.h, B, L, device)
        full, _ = run_prec(voc, mel, rule.code)
        assert float(full.abs().max()) > 1e-3 and bool(torch.isfinite(full).all())
        got, pcm = run_prec(voc, mel, rule.code, lengths, want_pcm=True)
        assert_kept_and_tails(got, full, lengths, voc.h.hop, f"{name} fused={fused} precision {rule}")
        assert torch.equal(pcm, (got * 32768).clamp(-32768, 32767).trunc().to(torch.int16))
        assert int(pcm.abs().max()) > 30
        assert not torch.equal(run_prec(voc, mel, other(rule).code)[0], full)
        if not module:
            continue
        with torch.no_grad():
            assert not torch.equal(voc(mel.transpose(1, 2))[:, 0], full)
            for p in (rule.value,) + rule.spellings:
                assert torch.equal(voc(mel.transpose(1, 2), precision=p)[:, 0], full)


def check_default_untouched(rule, name, B, L, lengths, device, fused=True):
    """Test 3: precision 0 and 32 through the `_prec` entry point are the two older entry points, bit for bit, with calls at both reduced
    precisions (the rule's first) before them; and both are reproducible across them."""
    voc = make_vocoder(name, device, fused=fused)
    assert voc.precision == 32 and Generator().precision == 32
    mel = make_mel(voc.h, B, L, device)
    plain, _ = run_abi(voc, mel)
    rag, rag_pcm = run_abi(voc, mel, lengths, want_pcm=True)
    assert bool(torch.isfinite(plain).all())
    first = {r: run_prec(voc, mel, r.code)[0] for r in (rule, other(rule))}
    for precision in (0, 32):
        a, none = run_prec(voc, mel, precision)
        assert none is None and torch.equal(a, plain), precision
        b, b_pcm = run_prec(voc, mel, precision, lengths, want_pcm=True)
        assert torch.equal(b, rag) and torch.equal(b_pcm, rag_pcm), precision
    for r, wav in first.items():
        assert torch.equal(run_prec(voc, mel, r.code)[0], wav), r


def check_vocoder_wrappers(device):
    """EfficientSpeech.synthesize(batch, precision=16) and a BucketedSynthesizer whose vocoder has precision = 16, tiny ES + v2,
    B = 3, T = 12, against Generator.forward(..., precision=16) on the same mel: kept samples bit for bit, wav_len unchanged."""
    from efficientspeech_amd import BucketedSynthesizer, EfficientSpeech
    voc = make_vocoder("v2", device)
    hop = voc.h.hop
    model = EfficientSpeech.from_config("tiny", hifigan=voc)
    model.phoneme2mel.load_state_dict({k: torch.from_numpy(v) for k, v in synth_state_dict(CONFIGS["tiny"], 1234).items()}, strict=True)
    model = model.to(device).eval()
    B, T, lens = 3, 12, [12, 7, 3]
    ids, mask = synth_phonemes(B, T, 12, lens)
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


def check_get_hifigan(tmp_path):
    """(host only) get_hifigan(..., precision=) builds a generator whose default is bf16, under either spelling"""
    import json
    from efficientspeech_amd.hifigan import get_hifigan
    h = small_config()
    ckpt = tmp_path / "generator_small"
    (tmp_path / "config.json").write_text(json.dumps(dataclasses.asdict(h)))
    torch.save({"generator": {k: torch.from_numpy(v) for k, v in synth_hifigan_state_dict(h, 1234).items()}}, str(ckpt))
    assert get_hifigan(str(ckpt), precision="bf16").precision == "bf16"
    assert get_hifigan(str(ckpt), precision="bf16-mixed").precision == "bf16"
    assert get_hifigan(str(ckpt)).precision == 32
    with pytest.raises(ValueError, match="precision"):
        get_hifigan(str(ckpt), precision=8)


# ---------------------------------------------------------------------------------------------------------------- launches (simulator)
_PREP = ("pack_", "absmax_kernel")            # weight preparation: left out of every record list below
_WARM = set()


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
    return [r for r in records if not r[0].startswith(_PREP + ("copy_pad_kernel",))], out


def check_decoder_dispatch(rule, name, key32=True):
    """A forward's records at the rule's precision differ from the precision-32 one's only in the decoder's name: grid, block and LDS
    bytes identical, encoder-side records identical."""
    r32, _ = forward_records(name, {})
    rr, _ = forward_records(name, {"decoder_precision": rule.value})
    if key32:                                    # (the key at 32: the general entry point, the old launches)
        assert forward_records(name, {"decoder_precision": 32})[0] == r32
    assert len(rr) == len(r32) and rr[:-1] == r32[:-1]
    (n32, d32), (nr, dr) = r32[-1], rr[-1]
    assert n32 == "mel_decoder_kernel<DX2,KD,NW>" and nr == rule.decoder_kernel, (n32, nr)
    assert dr == d32
    assert sum("mel_decoder" in r[0] for r in rr) == 1


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
    """the launch records of one Generator.forward(..., precision) on the simulator (weight preparation left out)"""
    from tests.simlib import launch_records, use_sim
    h = vocoder_config_of(name)
    mel = make_mel(h, B, L, "cpu")
    with use_sim(), torch.no_grad(), launch_records() as records:
        voc = make_vocoder(name, "cpu", fused=fused)
        wav = voc(mel.transpose(1, 2), lengths=torch.tensor(list(lengths), dtype=torch.int32) if ragged else None, precision=precision)
    assert wav.shape == (B, 1, L * h.hop)
    return [r for r in records if not r[0].startswith(_PREP)]


def check_vocoder_dispatch(name, fused, ragged):
    """A bf16 vocoder call's records are the precision-16 call's with every kernel's name replaced by its bf16 twin's: same number, same
    order, same grid / block / LDS bytes"""
    r16 = vocoder_records(name, 16, fused, ragged)
    rb = vocoder_records(name, "bf16", fused, ragged)
    assert len(rb) == len(r16) > 3
    for (n16, d16), (nb, db) in zip(r16, rb):
        assert n16 in _BF_OF_16, n16
        assert nb == _BF_OF_16[n16] and db == d16, (n16, d16, nb, db)
    assert any("resblock" in n for n, _ in rb) == fused


def run_row(resblock, fused, ragged):
    """the launch records of one Generator.forward(..., precision=16) of the reduced generator on the simulator (B = 2, L = 6, lengths
    [6, 2]; weight preparation left out), run-length encoded in the format of tests/test_vocoder_dispatch.py"""
    runs = []
    for name, dims in vocoder_records(f"reduced{resblock}", 16, fused, ragged):
        rec = f"{name}[{dims}]"
        if runs and runs[-1][0] == rec:
            runs[-1][1] += 1
        else:
            runs.append([rec, 1])
    return " ".join(r if k == 1 else f"{k}x {r}" for r, k in runs)


# ---------------------------------------------------------------------------------------------------------------- precision 16 keeps its bits
P16_GOLDEN = "precision16_parent_bits.npz"     # tests/golden/: tools/gen_golden_precision16.py, run on the commit before bf16 inference


def precision16_cases(device):
    """name -> precision-16 output (host fp32) of four small deterministic calls: the decoder in direct mode, tiny (2, 40) and small
    (1, 40), and the vocoder one launch per ResBlock, "small" (2, 6: the 16-row-tile kernels) and "reduced1" (2, 6: the 32-row-tile
    kernels at 64 / 32 channels behind the per-convolution GEMMs).  Inputs and weights come from fixed seeds."""
    out = {}
    for name, B, L in (("tiny", 2, 40), ("small", 1, 40)):
        net, cfg, _sd = make_net(name, device)
        feats = torch.from_numpy(np.random.default_rng(7).standard_normal((B, L, cfg.d4)).astype(np.float32))
        with torch.no_grad():
            out[f"dec_{name}"] = net.decoder(feats.to(device), precision=16).cpu().numpy()
    for name in ("small", "reduced1"):
        voc = make_vocoder(name, device, fused=True)
        mel = make_mel(voc.h, 2, 6, device)
        wav, _ = run_prec(voc, mel, 16)
        out[f"voc_{name}"] = wav.cpu().numpy()
    return out


def check_precision16_keeps_the_parents_bits(device, tier):
    """Precision 16 through the `_prec` entry points gives, bit for bit, what the commit before bf16 inference gave: the committed outputs
    of that commit's own build (tier "sim": its wave-simulator build; "gpu": its libesmi.so on an MI355X)."""
    gold = np.load(os.path.join(GOLD, P16_GOLDEN))
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
