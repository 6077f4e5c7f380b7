#!/usr/bin/env python3
"""Development: the bits the training kernels produce, as one text file of `name sha256` lines -- to compare two builds of the library
with `cmp` (profiles/r21_train_ops_split.md: a refactor that reorders no sum must leave every line as it was).

    tools/train_bits.py OUT.txt [--sim] [--at-size]

 (a) every tensor every row of tests/train_variant_checks.ROWS hands to its judge;
 (b) the losses and the flat parameter buffer after 3 steps of train.TrainStep on train.synthetic_batch, tiny at B = 2, T = 17:
     precision 32, 16, bf16, precision 32 with gradient_clip_val, with accumulate_grad_batches=2 (one boundary crossed, one window left open;
     `flat.acc` too), with ema_decay (`flat.ema` too), all of these together at precision 16; precision 32, the accumulating and the combined
     run as captured graphs (device only);
 (c) --at-size: (b)'s precision-32 runs at B = 128, T = 100, the size tools/bench_train.py is timed at (device only).
--sim runs on the CPU wave simulator (tests/simlib.py); otherwise on cuda:0 through libesmi.so, or the library ESMI_LIB names."""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from efficientspeech_amd import CONFIGS, build_phoneme2mel, train  # noqa: E402
from efficientspeech_amd.synth import synth_state_dict  # noqa: E402
from tests import train_variant_checks as K  # noqa: E402
from tests.simlib import use_sim  # noqa: E402


def digest(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def rows(dev, out):
    for row in K.ROWS:
        seen = {}

        def note(name, t, row=row, seen=seen):
            seen[name] = seen.get(name, 0) + 1
            out.append(f"row/{row.id}/{name}#{seen[name]} {digest(t)}")
            return t
        K.run_row(dev, row, perturb=note)


def steps(dev, out, tag, B, T, **kw):
    cfg = CONFIGS["tiny"]
    net = build_phoneme2mel(cfg)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in synth_state_dict(cfg, 1234).items()})
    net = net.to(dev).train()
    x, y = train.synthetic_batch(B, T, 3, dev)
    ts = train.TrainStep(net, **kw)
    for i in range(3):
        out.append(f"step/{tag}/loss{i} {digest(ts.step(x, y))}")
    if dev != "cpu":
        torch.cuda.synchronize()
    out.append(f"step/{tag}/params {digest(ts.flat.data)}")
    for name in ("acc", "ema"):
        if hasattr(ts.flat, name):
            out.append(f"step/{tag}/{name} {digest(getattr(ts.flat, name))}")


def main():
    sim, at_size = "--sim" in sys.argv, "--at-size" in sys.argv
    path = [a for a in sys.argv[1:] if not a.startswith("--")][0]
    dev, out = ("cpu" if sim else "cuda"), []
    runs = [("p32", {}), ("p16", dict(precision="16")), ("bf16", dict(precision="bf16")), ("p32_clip", dict(gradient_clip_val=1.0))]
    accum, every = dict(accumulate_grad_batches=2), dict(precision=16, init_scale=2048.0, gradient_clip_val=1.0, accumulate_grad_batches=2, ema_decay=0.9)
    runs += [("p32_accum2", accum), ("p32_ema", dict(ema_decay=0.9)), ("p16_clip_accum2_ema", every)]
    if not sim:
        runs += [("p32_graph", dict(graph=True)), ("p32_accum2_graph", dict(accum, graph=True)), ("p16_clip_accum2_ema_graph", dict(every, graph=True))]
    rows(dev, out)
    for tag, kw in runs:
        steps(dev, out, f"B2_T17/{tag}", 2, 17, **kw)
    if at_size and not sim:
        for tag, kw in runs:
            if "precision" not in kw:
                steps(dev, out, f"B128_T100/{tag}", 128, 100, **kw)
    open(path, "w").write("\n".join(out) + "\n")
    print(f"{len(out)} lines -> {path}")


if __name__ == "__main__":
    if "--sim" in sys.argv:
        with use_sim():
            main()
    else:
        main()
