#!/usr/bin/env python3
"""Development: time the HiFi-GAN generator (esmi_hifigan_generator_f32) alone.  python tools/bench_vocoder.py [--config v2] [--batch 16] [--frames 768]
--ragged lo:hi[:seed]: utterance lengths uniform in [lo, hi] frames, the batch padded to hi; the full run and the length-aware run
(esmi_hifigan_generator_ragged_f32) of that batch alternate, and the ideal ratio sum(min(len + margin, L)) / (B L) is printed.
--precision {32,16}: 16 (esmi_hifigan_generator_prec_f32: one binary16 product per contraction) times precision 32 and 16 of the same call,
alternating in one process, and prints the ratio and the difference of the two waveforms; with --ragged both are the length-aware call.
--precision bf16 (ESMI_PRECISION_BF16: one bfloat16 product per contraction): legs 32 / 16 / bf16 / 32 per round; prints the ratios, the
spread of the two precision-32 legs, whether bf16 beats both of them by more than that spread, and the difference between the two
waveforms of each pair of precisions."""
import argparse, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
from efficientspeech_amd.hifigan import HIFIGAN_CONFIGS, Generator, synth_hifigan_state_dict, flops_per_mel_frame

ap = argparse.ArgumentParser()
ap.add_argument("--config", default="v2"); ap.add_argument("--batch", type=int, default=16); ap.add_argument("--frames", type=int, default=768)
ap.add_argument("--iters", type=int, default=5)
ap.add_argument("--ragged", default=None, metavar="lo:hi[:seed]"); ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--precision", default="32", choices=("32", "16", "bf16"))
a = ap.parse_args()
a.precision = a.precision if a.precision == "bf16" else int(a.precision)
h = HIFIGAN_CONFIGS[a.config]
if a.ragged:
    lo, hi, *seed = (int(v) for v in a.ragged.split(":"))
    assert 0 <= lo <= hi and hi >= 1
    a.frames = hi


voc = Generator(h)
voc.load_state_dict({k: torch.from_numpy(v) for k, v in synth_hifigan_state_dict(h, 1234).items()})
voc = voc.cuda().eval()
mel = torch.randn((a.batch, a.frames, h.num_mels), device="cuda") * 2 - 4

def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / a.iters


def precision_abc(what, call):
    """call(precision) in legs 32 / 16 / bf16 / 32, repeated a.rounds times (every precision sees the same clocks and neighbours)"""
    ta, t16, tb, tc = [], [], [], []
    with torch.no_grad():
        for _ in range(2):
            w32, w16, wb = call(32), call(16), call("bf16")
        for _ in range(a.rounds):
            ta.append(timed(lambda: call(32)))
            t16.append(timed(lambda: call(16)))
            tb.append(timed(lambda: call("bf16")))
            tc.append(timed(lambda: call(32)))
    ms = lambda v: " ".join(f"{x * 1e3:.2f}" for x in v)      # noqa: E731
    rms = lambda t: float(t.double().pow(2).mean().sqrt())    # noqa: E731
    ma, m16, mb, mc = (float(np.median(v)) for v in (ta, t16, tb, tc))
    m32, noise = (ma + mc) / 2, abs(ma - mc)
    print(f"hifigan {a.config}: B={a.batch} L={a.frames} {what}")
    for name, v in (("32 (first leg)", ta), ("16", t16), ("bf16", tb), ("32 (last leg)", tc)):
        print(f"  precision {name} ms: {ms(v)}   median {np.median(v) * 1e3:.2f}")
    print(f"  precision-32 legs' spread {noise * 1e3:.3f} ms = {noise / m32 * 100:.2f} %   bf16 / 32 = {mb / m32:.3f}   bf16 / 16 = {mb / m16:.3f}   16 / 32 = {m16 / m32:.3f}")
    print(f"  gate (bf16 faster than both precision-32 legs by more than their spread): {'PASS' if min(ma, mc) - mb > noise else 'FAIL'}")
    for na, wa, nb, wb_ in (("bf16", wb, "32", w32), ("16", w16, "32", w32), ("bf16", wb, "16", w16)):
        d = (wa - wb_).double()
        print(f"  wav{na} - wav{nb}: L-inf {float(d.abs().max()):.2e} rms {rms(d):.2e}")
    print(f"  wav32 rms {rms(w32):.3f}   finite={bool(torch.isfinite(wb).all())}")
    sys.exit(0)


def precision_ab(what, call):
    """call(precision) at 32 and 16, alternating (both see the same clocks and neighbours)"""
    t32, t16 = [], []
    with torch.no_grad():
        for _ in range(2):
            w32, w16 = call(32), call(16)
        for _ in range(a.rounds):
            t32.append(timed(lambda: call(32)))
            t16.append(timed(lambda: call(16)))
    d = (w16 - w32).double()
    ms = lambda v: " ".join(f"{x * 1e3:.2f}" for x in v)      # noqa: E731
    print(f"hifigan {a.config}: B={a.batch} L={a.frames} {what}")
    print(f"  precision 32 ms: {ms(t32)}   median {np.median(t32) * 1e3:.2f}")
    print(f"  precision 16 ms: {ms(t16)}   median {np.median(t16) * 1e3:.2f}")
    print(f"  16 / 32 = {np.median(t16) / np.median(t32):.3f}   wav16 - wav32: L-inf {float(d.abs().max()):.2e} rms {float(d.pow(2).mean().sqrt()):.2e} "
          f"(wav32 rms {float(w32.double().pow(2).mean().sqrt()):.3f})   finite={bool(torch.isfinite(w16).all())}")
    sys.exit(0)


if a.ragged:
    from efficientspeech_amd.hifigan import ragged_margins
    lens = np.random.default_rng(seed[0] if seed else 0).integers(lo, hi + 1, size=a.batch)
    lengths = torch.from_numpy(lens.astype(np.int32)).cuda()
    margin = ragged_margins(h)[1]
    ideal = float(np.minimum(lens + margin, a.frames).sum()) / (a.batch * a.frames)
    if a.precision == "bf16":
        precision_abc(f"lengths U[{lo},{hi}] mean {lens.mean():.1f}, length-aware call", lambda pr: voc(mel.transpose(1, 2), lengths=lengths, precision=pr))
    if a.precision == 16:
        precision_ab(f"lengths U[{lo},{hi}] mean {lens.mean():.1f}, length-aware call", lambda pr: voc(mel.transpose(1, 2), lengths=lengths, precision=pr))
    full, rag = [], []
    with torch.no_grad():
        for _ in range(2):
            ref, wav = voc(mel.transpose(1, 2)), voc(mel.transpose(1, 2), lengths=lengths)
        for _ in range(a.rounds):                       # alternating: both see the same clocks and neighbours
            full.append(timed(lambda: voc(mel.transpose(1, 2))))
            rag.append(timed(lambda: voc(mel.transpose(1, 2), lengths=lengths)))
    keep = torch.arange(a.frames * h.hop, device="cuda")[None, :] < lengths[:, None] * h.hop
    same = bool(torch.equal(wav[:, 0][keep], ref[:, 0][keep])) and not bool(wav[:, 0][~keep].any())
    ms = lambda v: " ".join(f"{x * 1e3:.2f}" for x in v)      # noqa: E731
    print(f"hifigan {a.config}: B={a.batch} L={a.frames} lengths U[{lo},{hi}] mean {lens.mean():.1f} margin {margin} frames")
    print(f"  full   ms: {ms(full)}   median {np.median(full) * 1e3:.2f}")
    print(f"  ragged ms: {ms(rag)}   median {np.median(rag) * 1e3:.2f}")
    print(f"  ragged / full = {np.median(rag) / np.median(full):.3f}   ideal ratio = {ideal:.3f}   kept samples identical, tails zero: {same}")
    sys.exit(0)
if a.precision == "bf16":
    precision_abc("plain call", lambda pr: voc(mel.transpose(1, 2), precision=pr))
if a.precision == 16:
    precision_ab("plain call", lambda pr: voc(mel.transpose(1, 2), precision=pr))
with torch.no_grad():
    for _ in range(2):
        wav = voc(mel.transpose(1, 2))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.iters):
        wav = voc(mel.transpose(1, 2))
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / a.iters
fl = flops_per_mel_frame(h)
frames = a.batch * a.frames
print(f"hifigan {a.config}: B={a.batch} L={a.frames}: {dt*1e3:.2f} ms  {frames/dt:.3e} mel-frames/s  {frames*h.hop/dt/22050:.1f}x real time  "
      f"{fl/1e6:.1f} MFLOP/frame -> {fl*frames/dt/1e12:.1f} TFLOP/s   finite={bool(torch.isfinite(wav).all())}")
