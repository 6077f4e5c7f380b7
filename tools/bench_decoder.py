#!/usr/bin/env python3
"""Development tool: time mel_decoder_kernel alone (fused-LR mode, D-const) for one or more library builds.
   python tools/bench_decoder.py [--config tiny] [--libs a.so b.so ...]
--precision 16 (esmi_mel_decoder_prec_f32: one binary16 product per contraction): times precision 32 and 16 of the same call in alternating
legs 32 / 16 / 32 / 16 in one process, and prints per-leg medians, the spread of the two precision-32 legs (the noise a ratio has to
beat), the ratio and the difference of the two mels.
--precision bf16 (ESMI_PRECISION_BF16: one bfloat16 product per contraction): legs 32 / 16 / bf16 / 32; prints the ratios bf16 / 32 and
bf16 / 16, the spread of the two precision-32 legs, whether the bf16 leg beats BOTH of them by more than that spread, and the
difference between the two mels of each pair of precisions."""
import argparse, ctypes as C, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
from efficientspeech_amd import CONFIGS, _lib, build_phoneme2mel, load_numpy_state_dict
from efficientspeech_amd.synth import synth_state_dict

ap = argparse.ArgumentParser()
ap.add_argument("--config", default="tiny"); ap.add_argument("--batch", type=int, default=256)
ap.add_argument("--phonemes", type=int, default=128); ap.add_argument("--dur", type=int, default=6)
ap.add_argument("--zeros", action="store_true", help="zero activations (DVFS probe: same instruction stream, less switching power)"); ap.add_argument("--iters", type=int, default=30); ap.add_argument("--h0", action="store_true", help="phoneme-rate first stage supplied (what the full forward does for tiny, T <= 128)"); ap.add_argument("--burst", type=int, default=20, help="launches per timed burst (back-to-back, one event pair)"); ap.add_argument("--libs", nargs="*", default=[_lib.LIB_PATH])
ap.add_argument("--precision", default="32", choices=("32", "16", "bf16"))
a = ap.parse_args()
a.precision = a.precision if a.precision == "bf16" else int(a.precision)
cfg = CONFIGS[a.config]
B, T, L = a.batch, a.phonemes, a.phonemes * a.dur
flops = {"tiny": 189_440, "small": 973_824, "base": 1_505_792}[a.config]
ref = None
for path in a.libs:
    _lib._LIB = _lib.bind(C.CDLL(os.path.abspath(path)))
    net = build_phoneme2mel(cfg); load_numpy_state_dict(net, synth_state_dict(cfg)); net = net.cuda()
    g = torch.Generator(device="cuda").manual_seed(1)
    feat = torch.randn((B, T, cfg.d4), device="cuda", generator=g)
    cum = (torch.arange(1, T + 1, device="cuda", dtype=torch.int32) * a.dur).repeat(B, 1).contiguous()
    mel_len = torch.full((B,), L, dtype=torch.int32, device="cuda")
    dec = net.decoder
    h0 = torch.randn((B, T, cfg.dx2), device="cuda", generator=g) if a.h0 else None
    if a.zeros:
        feat.zero_()
        if h0 is not None: h0.zero_()
    if a.precision in (16, "bf16"):
        def leg(pr):
            ts = []
            for _ in range(a.iters):
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                for _ in range(a.burst):
                    m = dec._fused(feat, cum, mel_len, None, L, True, L, h0=h0, precision=pr)
                e.record()
                torch.cuda.synchronize(); ts.append(s.elapsed_time(e) / a.burst)
            return float(np.median(ts)) * 1e3, m
        for _ in range(3):
            for pr in (32, 16, a.precision):
                dec._fused(feat, cum, mel_len, None, L, True, L, h0=h0, precision=pr)
        torch.cuda.synchronize()
        if a.precision == "bf16":
            legs = [(pr,) + leg(pr) for pr in (32, 16, "bf16", 32)]      # alternating: the bf16 leg sits between the two precision-32 legs
            (_, ta, m32), (_, t16, m16), (_, tb, mb), (_, tc, _m) = legs
            noise = abs(ta - tc)
            rms = lambda t: float(t.double().pow(2).mean().sqrt())       # noqa: E731
            print(f"{os.path.basename(path)} {a.config} B={B} T={T} D={a.dur} h0={bool(a.h0)}: legs us " + "  ".join(f"p{pr} {t:.1f}" for pr, t, _ in legs))
            print(f"  precision 32 {(ta + tc) / 2:8.1f} us (two legs, spread {noise:.1f} us = {noise / ((ta + tc) / 2) * 100:.2f} %)   16 {t16:8.1f} us   bf16 {tb:8.1f} us   "
                  f"bf16 / 32 = {tb / ((ta + tc) / 2):.3f}   bf16 / 16 = {tb / t16:.3f}   16 / 32 = {t16 / ((ta + tc) / 2):.3f}")
            print(f"  gate (bf16 faster than both precision-32 legs by more than their spread): {'PASS' if min(ta, tc) - tb > noise else 'FAIL'}")
            for na, ma, nb, mb_ in (("bf16", mb, "32", m32), ("16", m16, "32", m32), ("bf16", mb, "16", m16)):
                d = ma.double() - mb_.double()
                print(f"  mel{na} - mel{nb}: L-inf {float(d.abs().max()):.2e} rms {rms(d):.2e}")
            print(f"  mel32 rms {rms(m32):.3f} max {float(m32.abs().max()):.2f}   finite={bool(torch.isfinite(mb).all())}", flush=True)
            continue
        legs = [(pr,) + leg(pr) for pr in (32, 16, 32, 16)]      # alternating: both precisions see the same clocks and neighbours
        t32, t16 = [t for pr, t, _ in legs if pr == 32], [t for pr, t, _ in legs if pr == 16]
        m32, m16 = legs[0][2].double(), legs[1][2].double()
        d = m16 - m32
        noise = abs(t32[0] - t32[1]) / np.mean(t32)
        print(f"{os.path.basename(path)} {a.config} B={B} T={T} D={a.dur} h0={bool(a.h0)}: legs us " + "  ".join(f"p{pr} {t:.1f}" for pr, t, _ in legs))
        print(f"  precision 32 {np.mean(t32):8.1f} us (two legs, spread {noise * 100:.2f} %)   precision 16 {np.mean(t16):8.1f} us (spread "
              f"{abs(t16[0] - t16[1]) / np.mean(t16) * 100:.2f} %)   16 / 32 = {np.mean(t16) / np.mean(t32):.3f}   speed-up {np.mean(t32) / np.mean(t16):.3f}x")
        print(f"  mel16 - mel32: L-inf {float(d.abs().max()):.2e} rms {float(d.pow(2).mean().sqrt()):.2e} (mel32 rms {float(m32.pow(2).mean().sqrt()):.3f}, "
              f"max {float(m32.abs().max()):.2f})   finite={bool(torch.isfinite(legs[1][2]).all())}", flush=True)
        continue
    for _ in range(5):
        mel = dec._fused(feat, cum, mel_len, None, L, True, L, h0=h0)
    torch.cuda.synchronize()
    ts = []
    for _ in range(a.iters):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(a.burst):
            mel = dec._fused(feat, cum, mel_len, None, L, True, L, h0=h0)
        e.record()
        torch.cuda.synchronize(); ts.append(s.elapsed_time(e) / a.burst)
    ms = float(np.median(ts))
    if ref is None: ref = mel.clone()
    diff = float((mel - ref).abs().max())
    print(f"{os.path.basename(path):32s} {ms*1e3:8.1f} us  min {min(ts)*1e3:8.1f}  {flops*B*L/ms/1e9:6.1f} TF  "
          f"{flops*B*L/ms/1e9/157.3*100:5.1f}% fp32 peak   max|diff vs first| {diff:.2e}", flush=True)
