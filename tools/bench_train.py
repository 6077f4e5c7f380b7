#!/usr/bin/env python3
"""Development: time the training step (efficientspeech_amd.train.TrainStep) on a synthetic teacher-forced batch.
python tools/bench_train.py [--config tiny] [--batch 32] [--phonemes 128] [--dur 6] [--iters 5] [--accumulate N]
--accumulate N times whole windows of N micro-batches (TrainStep(accumulate_grad_batches=N)) and prints ms per micro-batch and per window.
--ema-decay D compares the REPLAYED step (graph=True) without and with the weight average (TrainStep(ema_decay=D)) in alternating legs off / on /
off, at the tool's default shape (32 x 128 phonemes) and at 128 x 100: per shape the legs' ms per step, the ratio on / mean(off) and the spread of
the two off legs (what the ratio has to be read against).  --timeline DB adds the update launch's own duration from a rocprofv3 result database
(rocprofv3 --kernel-trace -d DIR -o NAME -- python tools/bench_train.py --ema-decay D ...: DIR/NAME_results.db; tools/train_timeline.py lists
the whole step from the same file); with --timeline alone nothing runs on the GPU."""
import argparse, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
from efficientspeech_amd import CONFIGS, build_phoneme2mel, train
from efficientspeech_amd.synth import synth_state_dict


def _fresh_net(cfg):
    net = build_phoneme2mel(cfg)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in synth_state_dict(cfg, 1234).items()})
    return net.cuda().train()


def _ms_per_step(step, x, y, iters):
    for _ in range(3):                      # (the third call replays the graph)
        step.step(x, y)
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(iters):
        step.step(x, y)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3


def ema_legs(a):
    """Alternating legs off / on / off of the replayed step: three steps on three fresh nets, each warmed up before any leg is timed, then
    the three legs one after the other."""
    cfg = CONFIGS[a.config]
    for B, T in ((32, 128), (128, 100)):
        x, y = train.synthetic_batch(B, T, a.dur, "cuda")
        kw = dict(graph=True, precision=a.precision, init_scale=2048.0, gradient_clip_val=a.clip_grad_norm)
        steps = [train.TrainStep(_fresh_net(cfg), **kw, ema_decay=d) for d in (None, a.ema_decay, None)]
        for s in steps:
            _ms_per_step(s, x, y, 3)
        off1, on, off2 = (_ms_per_step(s, x, y, a.iters) for s in steps)
        off = 0.5 * (off1 + off2)
        print(f"replayed step {a.config} precision {a.precision} B={B} T={T}: off {off1:.4f} ms  on (ema_decay={a.ema_decay}) {on:.4f} ms  off {off2:.4f} ms  "
              f"on / off {on / off:.4f}  spread of the off legs {abs(off1 - off2) / off:.4f}  ({a.iters} steps per leg, "
              f"{steps[1].flat.data.numel()} floats in the flat buffer)")


def ema_launch_from_timeline(path):
    import sqlite3
    db = sqlite3.connect(path)
    cols = [r[1] for r in db.execute("pragma table_info(kernels)")]
    rows = [dict(zip(cols, r)) for r in db.execute("select * from kernels order by start")]
    us = sorted((r["end"] - r["start"]) / 1e3 for r in rows if "train_ema_update_kernel" in r["name"])
    if not us:
        raise SystemExit(f"{path}: no train_ema_update_kernel launch in the trace")
    print(f"train_ema_update_kernel in {os.path.basename(path)}: {len(us)} launches, median {us[len(us) // 2]:.2f} us, min {us[0]:.2f} us, max {us[-1]:.2f} us")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="tiny"); ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--phonemes", type=int, default=128); ap.add_argument("--dur", type=int, default=6); ap.add_argument("--iters", type=int, default=5); ap.add_argument("--graph", action="store_true"); ap.add_argument("--precision", default="32", choices=["32", "16", "bf16"]); ap.add_argument("--clip-grad-norm", type=float, default=None, metavar="V", help="TrainStep(gradient_clip_val=V): clip the gradients' 2-norm to V on the device (inf: measure only)"); ap.add_argument("--accumulate", type=int, default=None, metavar="N", help="TrainStep(accumulate_grad_batches=N): --iters counts windows of N micro-batches"); ap.add_argument("--torch-mirror", action="store_true", help="time plain PyTorch-ROCm ops (tests/torch_mirror.py + torch.optim.AdamW) on the same batch instead")
    ap.add_argument("--ema-decay", type=float, default=None, metavar="D", help="TrainStep(ema_decay=D): legs off / on / off of the replayed step at 32 x 128 and 128 x 100 (--batch / --phonemes / --graph / --accumulate are not read)")
    ap.add_argument("--timeline", default=None, metavar="DB", help="a rocprofv3 --kernel-trace result database: print train_ema_update_kernel's duration from it")
    a = ap.parse_args()
    if a.timeline:
        ema_launch_from_timeline(a.timeline)
        sys.exit(0)
    if a.ema_decay is not None:
        ema_legs(a)
        sys.exit(0)
    cfg = CONFIGS[a.config]
    net = _fresh_net(cfg)
    x, y = train.synthetic_batch(a.batch, a.phonemes, a.dur, "cuda")
    if a.torch_mirror:
        from tests import torch_mirror as M
        for k, p in net.named_parameters():
            p.requires_grad_(not k.endswith("_bins"))
        opt = torch.optim.AdamW([p for p in net.parameters() if p.requires_grad], lr=1e-3, weight_decay=1e-6)

        class _S:
            def step(self, x, y):
                opt.zero_grad(set_to_none=True)
                parts, total = M.loss(M.train_forward(net, dict(x, mel=y["mel"])), x, y)
                total.backward()
                opt.step()
                return torch.stack([*[p.detach() for p in parts], total.detach()])
        step = _S()
    else:
        step = train.TrainStep(net, graph=a.graph, precision=a.precision, init_scale=2048.0, gradient_clip_val=a.clip_grad_norm,
                               accumulate_grad_batches=a.accumulate)
    per = a.accumulate if a.accumulate and a.accumulate > 1 and not a.torch_mirror else 1     # step() calls per optimizer step
    for _ in range(3 * per):                # (whole windows: the third one replays every graph, the boundary's included)
        l0 = step.step(x, y)
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(a.iters * per):
        l1 = step.step(x, y)
    torch.cuda.synchronize(); dt = (time.perf_counter() - t0) / (a.iters * per)
    frames = a.batch * a.phonemes * a.dur
    mode = " (plain PyTorch-ROCm ops)" if a.torch_mirror else (" (hipGraph)" if a.graph else "")
    print(f"train step{mode} {a.config}: B={a.batch} T={a.phonemes} L={a.phonemes * a.dur}: "
          + (f"{dt * 1e3:.3f} ms/micro-batch  {dt * per * 1e3:.3f} ms/window of {per}" if per > 1 else f"{dt * 1e3:.3f} ms/step") + f"  {frames / dt:.3e} mel-frames/s  "
          f"loss {float(l0[4]):.3f} -> {float(l1[4]):.3f}"
          + (f"  grad norm {step.grad_norm:.4g} clip coef {step.clip_coef:.4g}" if a.clip_grad_norm and not a.torch_mirror else ""))
