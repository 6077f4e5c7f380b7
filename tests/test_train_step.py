"""Training step against the reference-generated fixture tests/golden/tiny_train_step.npz
(tools/gen_golden_train.py: the reference's train=True forward, model.py's loss arithmetic, torch autograd, torch AdamW).
The same checks run on the MI355X through libesmi.so (-m gpu) and on the CPU wave-simulator build of the same kernels;
the data-parallel step runs as two gloo ranks on the simulator (RCCL on the node: the same torch.distributed call)."""
import contextlib
import os
import socket
import sys

import numpy as np
import pytest
import torch

from efficientspeech_amd import CONFIGS, build_phoneme2mel
from efficientspeech_amd.synth import synth_state_dict
from tests.simlib import use_sim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(os.path.dirname(__file__), "golden", "tiny_train_step.npz")
GOLD_SMALL = os.path.join(os.path.dirname(__file__), "golden", "small_train_step.npz")   # 3 blocks, reduction 2; sample of gradients
GOLD_BASE = os.path.join(os.path.dirname(__file__), "golden", "base_train_step.npz")     # heads 2/4/6, expansion 2, k = 5, depth 3
GOLD_B1 = os.path.join(os.path.dirname(__file__), "golden", "tiny_train_step_b1.npz")   # one utterance (the mask-free code path of
#                                                        networks.py:338), two zero-length phonemes; a sample of the gradients


def _setup(dev, gold=GOLD):
    from efficientspeech_amd import train
    g = np.load(gold)
    cfg = CONFIGS[os.path.basename(gold).split("_")[0]]
    net = build_phoneme2mel(cfg)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in synth_state_dict(cfg, 1234).items()}, strict=True)
    net = net.to(dev).train()
    t = lambda k: torch.from_numpy(g["in_" + k]).to(dev)     # noqa: E731
    x = {"phoneme": t("phoneme"), "phoneme_mask": t("phoneme_mask"), "pitch": t("pitch"), "energy": t("energy"),
         "duration": t("duration"), "mel_len": t("mel_len"), "mel_mask": t("mel_mask")}
    y = {"mel": t("mel")}
    return train, g, net, x, y


def check_loss_and_gradients(dev, gold=GOLD):
    train, g, net, x, y = _setup(dev, gold)
    step = train.TrainStep(net)
    step.flat.zero_grad()
    parts, total = train.training_loss(net, x, y)
    total.backward()
    got = train.loss_vector(parts, total).cpu().numpy().astype(np.float64)
    assert np.allclose(got[:4], g["losses"], rtol=2e-5, atol=1e-6), (got, g["losses"])
    assert abs(got[4] - float(g["total"])) < 2e-5 * abs(float(g["total"]))
    named = dict(net.named_parameters())
    n = 0
    for k in g.files:
        if not k.startswith("grad."):
            continue
        ref = g[k]
        mine = named[k[5:]].grad.detach().cpu().numpy()
        scale = max(1e-6, float(np.abs(ref).max()))
        err = float(np.abs(mine - ref).max()) / scale
        assert err < 5e-5, (k, err, scale)
        n += 1
    if gold == GOLD:
        assert n == 101 and len(step.flat.names) == 101                # every parameter the reference's autograd reaches
    else:
        assert n >= 8                                                  # the other fixtures carry a sample of the gradients
    for k in g["no_grad_params"]:
        assert str(k) not in step.flat.names, k                        # left out of the optimizer: torch's grad-is-None rule
    out = train.train_forward(net, dict(x, mel=y["mel"]))
    nf = g["mel_pred"].shape[1]                                        # (the wider configs keep the first frames only)
    assert np.abs(out["mel"].detach().cpu().numpy()[:, :nf] - g["mel_pred"]).max() < 1e-4
    assert np.array_equal(out["mel_len"].cpu().numpy(), g["in_mel_len"])


def check_loss_kernel_against_oracle(dev):
    """esmi_train_loss_f32 on the reference's own predictions vs the oracle's float64 restatement (values and gradient seeds)."""
    from oracle import oracle
    train, g, net, x, y = _setup(dev)
    t = lambda k: torch.from_numpy(g[k]).to(dev)     # noqa: E731
    B, T = g["in_pitch"].shape
    preds = [t("mel_pred").requires_grad_(), t("pitch_pred").reshape(B, T).requires_grad_(), t("energy_pred").reshape(B, T).requires_grad_(),
             t("duration_pred").reshape(B, T).requires_grad_()]
    parts, total = train._Loss.apply(*preds, y["mel"], x["pitch"], x["energy"], x["duration"].to(torch.int32),
                                     x["mel_mask"].view(torch.uint8), x["phoneme_mask"].view(torch.uint8))
    out = train.loss_vector(parts, total)
    ref, rg = oracle.training_loss(g["mel_pred"], g["in_mel"], g["in_mel_mask"], g["pitch_pred"], g["in_pitch"], g["energy_pred"],
                                   g["in_energy"], g["duration_pred"], g["in_duration"], g["in_phoneme_mask"])
    assert np.allclose(out.cpu().numpy(), ref, rtol=2e-6)
    for a, r in zip(torch.autograd.grad(0.5 * total, preds), rg):        # a seed other than 1 scales the gradients
        assert np.allclose(a.cpu().numpy(), 0.5 * r.reshape(a.shape), rtol=1e-5, atol=1e-9)


def check_adamw_step(dev, reproducible=True):
    train, g, net, x, y = _setup(dev)
    step = train.TrainStep(net, lr=1e-3, weight_decay=1e-6)
    losses = step.step(x, y)
    assert abs(float(losses[4]) - float(g["total"])) < 2e-5 * abs(float(g["total"]))
    named = dict(net.named_parameters())
    n = 0
    for k in g.files:
        if k.startswith("after."):
            ref, mine = g[k], named[k[6:]].detach().cpu().numpy()
            assert np.abs(mine - ref).max() < 2e-6, (k, float(np.abs(mine - ref).max()))
            n += 1
    assert n >= 5
    if not reproducible:
        return
    again = step.step(x, y)                                            # bitwise reproducible: no atomics anywhere in the step
    t2, g2, net2, x2, y2 = _setup(dev)
    s2 = t2.TrainStep(net2, lr=1e-3, weight_decay=1e-6)
    s2.step(x2, y2)
    assert torch.equal(s2.step(x2, y2), again)
    assert torch.equal(s2.flat.data, step.flat.data)


@pytest.mark.gpu
@pytest.mark.parametrize("gold", [GOLD, GOLD_B1, GOLD_SMALL, GOLD_BASE], ids=["b2_padded", "b1_zero_durations", "small", "base"])
def test_gpu_loss_and_gradients_match_reference(gold):
    check_loss_and_gradients("cuda", gold)


@pytest.mark.gpu
def test_gpu_adamw_step_matches_reference():
    check_adamw_step("cuda")


def check_inference_sees_the_update(dev, steps):
    """An eval forward BEFORE training fills every packed-weight cache of the inference path (encoder blocks, fuse, predictors,
    decoder blob, the decoder HEAD the fused variance-adaptor kernel reads on tiny ES, the one-call argument block).  The AdamW
    kernel then writes the weights through raw pointers -- no torch version counter moves -- so `TrainStep` must drop every one
    of those copies: the eval output after training has to equal a FRESH net loaded from net.state_dict()."""
    train, g, net, x, y = _setup(dev)
    xe = {"phoneme": x["phoneme"], "phoneme_mask": x["phoneme_mask"], "duration_forced": x["duration"]}
    net.eval()
    with torch.no_grad():
        before = net(xe)[0].clone()
    net.train()
    step = train.TrainStep(net, lr=1e-3)
    first = float(step.step(x, y)[4])
    for _ in range(steps - 1):
        last = float(step.step(x, y)[4])
    net.eval()
    with torch.no_grad():
        after = net(xe)[0].clone()
    cfg = CONFIGS["tiny"]
    fresh = build_phoneme2mel(cfg)
    fresh.load_state_dict({k: v.detach().cpu().clone() for k, v in net.state_dict().items()}, strict=True)
    fresh = fresh.to(dev).eval()
    with torch.no_grad():
        want = fresh(xe)[0]
    assert bool(torch.isfinite(before).all()) and after.shape == before.shape
    assert float((after - before).abs().max()) > 1e-3                  # the weights moved ...
    assert torch.equal(after, want), float((after - want).abs().max())  # ... and every packed copy followed them (same kernels, same weights: bitwise)
    return first, last


@pytest.mark.gpu
def test_gpu_training_reduces_the_loss_and_inference_sees_the_update():
    first, last = check_inference_sees_the_update("cuda", 21)
    assert last < 0.9 * first, (first, last)


def test_simulated_inference_sees_the_update():
    with use_sim():
        check_inference_sees_the_update("cpu", 3)


@pytest.mark.gpu
def test_gpu_loss_kernel_matches_oracle():
    check_loss_kernel_against_oracle("cuda")


def test_simulated_loss_kernel_matches_oracle():
    with use_sim():
        check_loss_kernel_against_oracle("cpu")


@pytest.mark.parametrize("gold", [GOLD, GOLD_B1, GOLD_SMALL], ids=["b2_padded", "b1_zero_durations", "small"])
def test_simulated_loss_and_gradients_match_reference(gold):
    with use_sim():
        check_loss_and_gradients("cpu", gold)


@contextlib.contextmanager
def fused_conv_ln(train):
    """train.FUSE_CONV_LN for one check: conv + LayerNorm as ONE forward launch (esmi_train_conv_ln_fwd_f32)."""
    train.FUSE_CONV_LN = True
    try:
        yield
    finally:
        train.FUSE_CONV_LN = False


@pytest.mark.gpu
@pytest.mark.parametrize("gold", [GOLD, GOLD_SMALL], ids=["b2_padded", "small"])
def test_gpu_fused_conv_layernorm_matches_reference(gold):
    """The same golden losses / gradients with the norm in the convolution's launch (off by default: train.FUSE_CONV_LN)."""
    from efficientspeech_amd import train
    with fused_conv_ln(train):
        check_loss_and_gradients("cuda", gold)


def test_simulated_fused_conv_layernorm_matches_reference():
    from efficientspeech_amd import train
    with use_sim(), fused_conv_ln(train):
        check_loss_and_gradients("cpu", GOLD)


def test_simulated_adamw_step_matches_reference():
    with use_sim():
        check_adamw_step("cpu", reproducible=False)      # (the run-to-run check costs three more simulated steps: GPU only)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _ddp_worker(rank, world, port, out_path):
    import torch.distributed as dist
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), WAVESIM_THREADS="2")
    dist.init_process_group("gloo", rank=rank, world_size=world)
    train, g, net, x, y = _setup("cpu")
    sel = slice(rank, rank + 1)                                        # rank r trains on utterance r of the fixture batch
    cut = lambda d: {k: (torch.cat([v[sel], v[sel]]) if torch.is_tensor(v) and v.dim() > 0 and v.shape[0] == 2 else v)   # noqa: E731
                     for k, v in d.items()}                            # (doubled: B = 1 takes the reference's mask-free code path)
    with use_sim():
        step = train.TrainStep(net, world_size=world)
        losses = step.step(cut(x), cut(y))
        flat = step.flat.data.clone()
        gather = [torch.empty_like(flat) for _ in range(world)]
        dist.all_gather(gather, flat)
        lg = [torch.empty_like(losses) for _ in range(world)]
        dist.all_gather(lg, losses)
        # epoch-level means are averaged over the ranks (model.py:227-242, sync_dist=True): one epoch of one batch per rank
        hist = train.fit(step, [(cut(x), cut(y))], epochs=1, device="cpu", first_epoch=60)
        ep = torch.tensor(hist[0]["losses"])
        eg = [torch.empty_like(ep) for _ in range(world)]
        dist.all_gather(eg, ep)
    if rank == 0:
        np.save(out_path, np.array([int(torch.equal(gather[0], gather[1])), int(not torch.equal(lg[0], lg[1])),
                                    int(bool(torch.isfinite(flat).all())), int(torch.equal(eg[0], eg[1]))]))
    dist.barrier()
    dist.destroy_process_group()


def test_two_rank_data_parallel_step_keeps_replicas_identical(tmp_path):
    """Different batches per rank, ONE all-reduce of the flat gradient buffer, identical parameters afterwards."""
    import torch.multiprocessing as mp
    out = str(tmp_path / "ddp.npy")
    mp.spawn(_ddp_worker, args=(2, _free_port(), out), nprocs=2, join=True)
    same_params, different_losses, finite, same_epoch_means = np.load(out)
    assert same_params == 1 and different_losses == 1 and finite == 1 and same_epoch_means == 1


@pytest.mark.gpu
def test_gpu_captured_step_equals_eager_step():
    """graph=True: the whole step replayed from one hipGraph gives the eager step's losses and parameters."""
    train, g, net, x, y = _setup("cuda")
    eager = train.TrainStep(net, lr=1e-3)
    ref = [eager.step(x, y).clone() for _ in range(4)]
    t2, g2, net2, x2, y2 = _setup("cuda")
    cap = t2.TrainStep(net2, lr=1e-3, graph=True)
    got = [cap.step(x2, y2).clone() for _ in range(4)]      # step 1 captures (and runs eagerly), steps 2-4 replay
    for a, b in zip(ref, got):                               # (bias corrections: powf on the device vs on the host, ~1 ulp)
        assert torch.allclose(a, b, rtol=1e-5, atol=0), (a, b)
    assert torch.allclose(eager.flat.data, cap.flat.data, rtol=1e-4, atol=1e-6)


@pytest.mark.gpu
def test_gpu_step_count_set_on_a_captured_step_reaches_the_optimizer():
    """`step.t = k` sets the ONE counter the optimizer reads, captured or not: from t = 7 a captured step gives the eager step's
    parameters (with zero moments the bias corrections of step 1 and step 8 differ by about half a learning rate per element)."""
    train, g, net, x, y = _setup("cuda")
    a = train.TrainStep(net, lr=1e-3)
    a.t = 7
    a.step(x, y)
    t2, g2, net2, x2, y2 = _setup("cuda")
    b = t2.TrainStep(net2, lr=1e-3, graph=True)
    b.t = 7
    b.step(x2, y2)
    assert a.t == b.t == 8
    assert torch.allclose(a.flat.data, b.flat.data, rtol=1e-4, atol=1e-6)


@pytest.mark.gpu
@pytest.mark.parametrize("precision", [32, 16])
def test_gpu_checkpoint_resumes_into_a_captured_step(precision):
    """check_checkpoint_resume's first paragraph with graph=True on both sides: 2 steps, save, a 3rd; a fresh captured step resumed
    from the checkpoint takes one step to the same losses and parameters, and counts 3.  Precision 16 starts at a scale the fixture
    batch does not overflow at (check_precision16_step's) and grows it after 3 clean steps, so that the 3rd step's growth happens in
    the resumed step only if the scaler's interval and its count of clean steps came back with the checkpoint."""
    kw = dict(lr=1e-3, graph=True, precision=precision)
    train, g, net, x, y = _setup("cuda")
    a = train.TrainStep(net, init_scale=2048.0, growth_interval=3, **kw)
    for _ in range(2):
        a.step(x, y)
    ckpt = a.state_dict()
    assert ckpt["global_step"] == 2
    last_a = a.step(x, y)
    t2, g2, net2, x2, y2 = _setup("cuda")
    b = t2.TrainStep(net2, **kw)
    b.load_state_dict(ckpt)
    last_b = b.step(x2, y2)
    assert a.t == 3 and b.t == 3
    assert torch.allclose(last_a, last_b, rtol=1e-4, atol=1e-6), (last_a, last_b)
    assert torch.allclose(a.flat.data, b.flat.data, rtol=1e-4, atol=1e-6)
    assert a.skipped == b.skipped == 0 and a.scale == b.scale == (4096.0 if precision == 16 else 1.0)


def test_simulated_optimizer_state_counts_once_on_the_device_and_on_the_host():
    """The CPU twin of the two tests above (capture itself cannot run on the simulator): `AdamWState` with its scalars in device
    memory, as a captured precision-32 step has them, and with them on the host takes the same AdamW step from t = 7 to t = 8."""
    import types
    from efficientspeech_amd import train
    from tests.simlib import launched_kernels
    n, lr = 1003, 1e-3                                       # four blocks of 256, the last one partial
    gen = torch.Generator().manual_seed(7)
    p0, g0 = torch.randn(n, generator=gen), 1e-2 * torch.randn(n, generator=gen)
    got = {}
    with use_sim():
        for graph in (True, False):
            flat = types.SimpleNamespace(data=p0.clone(), grad=g0.clone(), m=torch.zeros(n), v=torch.zeros(n))
            opt = train.AdamWState("cpu", precision=32, graph=graph, lr=lr)
            assert opt.on_device == graph and (opt.hyper is not None) == graph and opt.scaler is None and opt.absmax is None
            opt.t = 7
            opt.set_lr(lr)
            with launched_kernels() as names:
                opt.launch(flat, (0.9, 0.999), 1e-8, 1e-6)
            assert names == (["train_bump_step_kernel", "train_adamw_dev_kernel"] if graph else ["train_adamw_kernel"])
            assert opt.t == 8
            got[graph] = flat
    for k in ("data", "m", "v"):
        assert torch.allclose(getattr(got[True], k), getattr(got[False], k), rtol=1e-4, atol=1e-6), k
    # ... and it is step 8's update: from zero moments m = 0.1 g and v = 0.001 g^2, so every element moves by
    # lr (0.1 / bc1) sqrt(bc2 / 0.001) = 0.4958 lr with bc1 = 1 - 0.9^8, bc2 = 1 - 0.999^8 (step 1 would move it by lr); eps = 1e-8
    # against |g| ~ 1e-2 and the decay lr wd |p| ~ 1e-9 are below the 1 % allowed here
    for flat in got.values():
        moved = (flat.data - p0).abs()
        assert 0.99 * 0.4958 * lr < float(moved.median()) < 1.01 * 0.4958 * lr, float(moved.median())


def test_lr_schedule_matches_reference_lambda():
    """model.py:77-101: linear warm-up (50 epochs) then cosine decay, evaluated per epoch."""
    import math
    from efficientspeech_amd.train import lr_at_epoch
    assert lr_at_epoch(0) == 0.0 and abs(lr_at_epoch(25) - 0.5e-3) < 1e-12 and abs(lr_at_epoch(50) - 1e-3) < 1e-12
    assert abs(lr_at_epoch(2525) - 1e-3 * 0.5 * (1 + math.cos(math.pi * 0.5))) < 1e-12 and lr_at_epoch(5000) < 1e-12


def test_simulated_fit_over_the_datamodule(tmp_path):
    """Loader -> training step (8f-2), end to end on the simulator: a synthetic preprocessed_data directory in the
    reference's on-disk format, `LJSpeechDataset` + `collate_fn`, two epochs of `fit` (epoch 0 at lr 0, as the reference's
    LambdaLR gives it, epoch 1 at the warm-up rate)."""
    import json
    from efficientspeech_amd import train
    from efficientspeech_amd.data import LJSpeechDataset, collate_fn, ARPABET
    root = tmp_path / "pre"
    for d in ("mel", "pitch", "energy", "duration"):
        (root / d).mkdir(parents=True)
    rng = np.random.default_rng(0)
    lines = []
    for i, n in enumerate((7, 5, 6)):
        phones = [ARPABET[j] for j in rng.integers(0, len(ARPABET), n)]
        dur = rng.integers(1, 4, n).astype(np.int64)
        base = f"LJ00{i}"
        np.save(root / "duration" / f"LJSpeech-duration-{base}.npy", dur)
        np.save(root / "pitch" / f"LJSpeech-pitch-{base}.npy", rng.normal(0, 1, n).astype(np.float32))
        np.save(root / "energy" / f"LJSpeech-energy-{base}.npy", rng.normal(0, 1, n).astype(np.float32))
        np.save(root / "mel" / f"LJSpeech-mel-{base}.npy", rng.normal(-5, 2, (int(dur.sum()), 80)).astype(np.float32))
        lines.append(f"{base}|LJSpeech|{{{' '.join(phones)}}}|some text {i}")
    (root / "train.txt").write_text("\n".join(lines) + "\n")
    (root / "speakers.json").write_text(json.dumps({"LJSpeech": 0}))
    cfg = {"path": {"preprocessed_path": str(root)}, "preprocessing": {"text": {"text_cleaners": ["english_cleaners"], "max_length": 4096}}}
    ds = LJSpeechDataset("train.txt", cfg)
    loader = torch.utils.data.DataLoader(ds, batch_size=3, shuffle=False, collate_fn=collate_fn)
    tr, g, net, _, _ = _setup("cpu")
    with use_sim():
        step = tr.TrainStep(net, lr=1e-3)
        before = step.flat.data.clone()
        hist = train.fit(step, loader, epochs=2, device="cpu", warmup=2, total=10)
    assert hist[0]["lr"] == 0.0 and abs(hist[1]["lr"] - 0.5e-3) < 1e-12
    assert all(np.isfinite(h["losses"]).all() for h in hist) and hist[0]["losses"][4] > 0
    assert not torch.equal(step.flat.data, before)                     # epoch 1 moved the weights (epoch 0 ran at lr 0: decay only)


def check_wrapper_training_api(dev):
    """The model.py-shaped wrapper: forward (training mode) -> dict, loss(y_hat, y, x) -> 4 losses, training_step -> total, as
    the reference's LightningModule exposes them (model.py:155-226)."""
    from efficientspeech_amd import EfficientSpeech
    train, g, net, x, y = _setup(dev)
    model = EfficientSpeech.from_config("tiny")
    model.phoneme2mel.load_state_dict(net.state_dict())
    model = model.to(dev).train()
    y_hat = model(x)
    assert set(y_hat) >= {"mel", "pitch", "energy", "duration", "mel_len"} and y_hat["pitch"].shape == (2, 13, 1)
    losses = model.loss(y_hat, y, x)
    assert np.allclose([float(v.detach()) for v in losses], g["losses"], rtol=2e-5)
    total = model.training_step((x, y))
    assert abs(float(total.detach()) - float(g["total"])) < 2e-5 * float(g["total"])
    total.backward()
    k = "decoder.mel_linear.bias"
    got = dict(model.phoneme2mel.named_parameters())[k].grad.cpu().numpy()
    assert np.abs(got - g["grad." + k]).max() < 5e-5 * np.abs(g["grad." + k]).max()
    step = model.make_train_step()
    assert step.lr == 1e-3 and step.wd == 1e-6
    # gradient accumulation through the public route: two backwards before an optimizer step add up (torch semantics), also
    # after make_train_step re-homed the gradients in the flat buffer
    p = dict(model.phoneme2mel.named_parameters())[k]
    step.flat.zero_grad()
    model.training_step((x, y)).backward()
    once = p.grad.detach().clone()
    model.training_step((x, y)).backward()
    assert torch.allclose(p.grad, 2 * once, rtol=1e-6, atol=0)


@pytest.mark.gpu
def test_gpu_wrapper_training_api():
    check_wrapper_training_api("cuda")


def test_simulated_wrapper_training_api():
    with use_sim():
        check_wrapper_training_api("cpu")


def check_checkpoint_resume(dev):
    """Train 2 steps, save, resume in a fresh TrainStep, 1 more step == 3 uninterrupted steps (bitwise); the saved weights load
    into the inference wrapper."""
    from efficientspeech_amd import EfficientSpeech
    train, g, net, x, y = _setup(dev)
    a = train.TrainStep(net, lr=1e-3)
    for _ in range(2):
        a.step(x, y)
    ckpt = a.state_dict()
    last_a = a.step(x, y)
    t2, g2, net2, x2, y2 = _setup(dev)
    b = t2.TrainStep(net2, lr=1e-3)
    b.load_state_dict(ckpt)
    last_b = b.step(x2, y2)
    assert torch.equal(last_a, last_b) and torch.equal(a.flat.data, b.flat.data) and b.t == 3
    model = EfficientSpeech.load_from_checkpoint(a.state_dict())     # (its own hyper_parameters describe the network)
    for k, v in model.phoneme2mel.state_dict().items():
        assert torch.equal(v.cpu(), net.state_dict()[k].cpu()), k
    # the optimizer state is a torch AdamW state_dict: it loads into torch.optim.AdamW over the same parameter list, and one
    # torch step from there equals one step of the AdamW kernel (same gradients) to round-off
    ck = a.state_dict()
    ref_net = build_phoneme2mel(CONFIGS["tiny"])
    ref_net.load_state_dict({k[len("phoneme2mel."):]: v.cpu() for k, v in ck["state_dict"].items()})
    opt = torch.optim.AdamW(ref_net.parameters(), lr=1e-3, weight_decay=1e-6)
    opt.load_state_dict({"state": {j: {k: v.cpu() if torch.is_tensor(v) else v for k, v in st.items()}
                                   for j, st in ck["optimizer_states"][0]["state"].items()},
                         "param_groups": ck["optimizer_states"][0]["param_groups"]})
    assert len(opt.state) == len(a.flat.names) and ck["global_step"] == 3
    named, mine = dict(ref_net.named_parameters()), dict(net.named_parameters())
    a.flat.zero_grad()
    _, total = train.training_loss(net, x, y)
    total.backward()
    for k in a.flat.names:
        named[k].grad = mine[k].grad.detach().cpu().clone()
    opt.step()
    a.t += 1
    lib, st = train._rt(a.flat.data)
    f = a.flat
    lib.esmi_train_adamw_f32(train._ptr(f.data), train._ptr(f.grad), train._ptr(f.m), train._ptr(f.v), f.data.numel(), a.lr, a.betas[0],
                             a.betas[1], a.eps, a.wd, a.t, 1.0, st)
    for k in a.flat.names:
        assert torch.allclose(mine[k].detach().cpu(), named[k].detach(), rtol=0, atol=2e-7), k
    # the schedule resumes where it stopped: two epochs through fit() -> the checkpoint records epoch 12, a fresh
    # TrainStep resumed from it trains its first epoch at lr_at_epoch(12), not at epoch 0's lr of 0
    hist = train.fit(a, [(x, y)], epochs=2, device=dev, first_epoch=10)
    assert [h["epoch"] for h in hist] == [10, 11] and a.state_dict()["epoch"] == 12
    t3, g3, net3, x3, y3 = _setup(dev)
    c = t3.TrainStep(net3, lr=1e-3)
    first = c.load_state_dict(a.state_dict())
    assert first == 12 and c.epoch == 12
    h3 = t3.fit(c, [(x3, y3)], epochs=1, device=dev, first_epoch=first)
    assert h3[0]["epoch"] == 12 and h3[0]["lr"] == train.lr_at_epoch(12, 1e-3) > 0 and c.state_dict()["epoch"] == 13


@pytest.mark.gpu
def test_gpu_checkpoint_resume():
    check_checkpoint_resume("cuda")


def test_simulated_checkpoint_resume():
    with use_sim():
        check_checkpoint_resume("cpu")


@pytest.mark.parametrize("gold", [GOLD, GOLD_B1, GOLD_SMALL, GOLD_BASE], ids=["b2_padded", "b1_zero_durations", "small", "base"])
def test_torch_mirror_matches_reference_fixture(gold):
    """The plain-PyTorch restatement used as the checker at large sizes (tests/torch_mirror.py) is itself pinned to the
    reference-generated fixtures: losses and gradients (CPU, torch ops only -- no kernels of ours involved)."""
    from tests import torch_mirror as M
    train, g, net, x, y = _setup("cpu", gold)
    for k, p in net.named_parameters():
        p.requires_grad_(not k.endswith("_bins"))
    out = M.train_forward(net, dict(x, mel=y["mel"]))
    parts, total = M.loss(out, x, y)
    assert np.allclose([float(v.detach()) for v in parts], g["losses"], rtol=1e-5)
    assert abs(float(total.detach()) - float(g["total"])) < 1e-5 * float(g["total"])
    total.backward()
    named = dict(net.named_parameters())
    for k in g.files:
        if k.startswith("grad."):
            ref, mine = g[k], named[k[5:]].grad.numpy()
            assert np.abs(mine - ref).max() < 2e-5 * max(1e-6, np.abs(ref).max()), k


# ------------------------------------------------------------------------------------------------------- precision 16 (AMP)
GOLD_AMP = os.path.join(os.path.dirname(__file__), "golden", "tiny_train_step_amp16.npz")   # tools/gen_golden_train.py --amp


def check_precision16_step(dev):
    """TrainStep(precision=16) -- binary16 GEMM operands, fp32 master weights, GradScaler-style dynamic loss scaling -- against the
    reference's own step under torch.autocast(float16) + torch.amp.GradScaler (what its default `--precision 16` runs).  Half
    precision is noisy by construction: the reference's fp16 gradients differ from its own fp32 gradients by 1.7e-2 (median
    tensor) to 0.30 (worst) of each tensor's scale on this batch, so the bar is statistical -- losses to 1e-3, every tensor's
    gradient aligned with the reference's (cosine), our error vs the fp16 reference no larger than the fp16 reference's own
    distance from fp32 -- plus the exact mechanics: the scaled seed, the unscale inside AdamW, skip + back-off on overflow."""
    train, g, net, x, y = _setup(dev, GOLD_AMP)
    f32 = np.load(GOLD)
    step = train.TrainStep(net, lr=1e-3, weight_decay=1e-6, precision=16, init_scale=2048.0)
    before = {k: v.detach().clone() for k, v in net.state_dict().items()}
    losses = step.step(x, y).cpu().numpy().astype(np.float64)
    assert np.allclose(losses[:4], g["losses"], rtol=1e-3, atol=1e-5), (losses, g["losses"])
    assert abs(losses[4] - float(g["total"])) < 1e-3 * float(g["total"])
    assert step.skipped == 0 and step.scale == 2048.0 and step.t == 1
    named = dict(net.named_parameters())
    n, worse = 0, []
    for k in g.files:
        if not k.startswith("grad."):
            continue
        ref16 = g[k].astype(np.float64).ravel()
        mine = (named[k[5:]].grad.detach().cpu().numpy().astype(np.float64) / 2048.0).ravel()      # the buffer holds scaled gradients
        scale = max(1e-9, np.abs(ref16).max())
        if ref16.size >= 32 and np.linalg.norm(ref16) > 1e-6 * ref16.size ** 0.5:
            cos = float(mine @ ref16 / (np.linalg.norm(mine) * np.linalg.norm(ref16) + 1e-30))
            assert cos > 0.98, (k, cos)
        if k in f32.files:
            ref32 = f32[k].astype(np.float64).ravel()
            d_mine, d_ref = np.abs(mine - ref16).max() / scale, np.abs(ref16 - ref32).max() / scale
            worse.append((d_mine - max(d_ref, 2e-3), k))      # ours vs fp16 reference, against the fp16 reference's own noise
        n += 1
    assert n >= 60
    assert max(worse)[0] < 0.05, sorted(worse)[-3:]
    # the update itself: AdamW on the unscaled gradients.  A FIRST AdamW step moves a weight by -lr g / (|g| + eps) (+ lr wd w): every
    # element whose gradient is clear of zero moves by -lr sign(g).  So the check is the SIGN PATTERN of the update on the elements
    # whose reference gradient exceeds what half precision can blur (the fp16 reference's own distance from fp32 on that tensor, plus
    # the slack granted to our gradients above), and there |delta_mine - delta_ref| against lr; elements with a near-zero gradient
    # (either sign is legitimate) are exempt.  (Round 3 bounded |after_mine - after_ref| by 2.5e-3 at lr 1e-3: it could not fail.)
    lr, checked, total = 1e-3, 0, 0
    for k in g.files:
        if not k.startswith("after."):
            continue
        name = k[6:]
        b4 = before[name].cpu().numpy().astype(np.float64)
        d_mine = named[name].detach().cpu().numpy().astype(np.float64) - b4
        d_ref = g[k].astype(np.float64) - b4
        moved = np.abs(d_mine).max()
        assert 0.5 * lr < moved < 1.5 * lr, (k, moved)
        total += d_ref.size
        gk = "grad." + name
        if gk not in g.files:
            continue
        ref16 = g[gk].astype(np.float64)
        scale = max(1e-9, np.abs(ref16).max())
        blur = (np.abs(ref16 - f32[gk].astype(np.float64)).max() if gk in f32.files else 2e-3 * scale) + 0.06 * scale
        clear = np.abs(ref16) > 2.0 * blur
        if not clear.any():
            continue
        checked += int(clear.sum())
        assert np.array_equal(np.sign(d_mine[clear]), np.sign(d_ref[clear])), (k, "update sign pattern differs")
        assert np.array_equal(np.sign(d_ref[clear]), -np.sign(ref16[clear])), k          # (the reference itself: -lr sign(g))
        assert np.abs(d_mine[clear] - d_ref[clear]).max() < 0.02 * lr, (k, np.abs(d_mine[clear] - d_ref[clear]).max())
    assert checked > 0.05 * total, (checked, total)            # the exemption must not swallow the test
    # overflow: an inf in the scaled gradients skips the update and halves the scale; the optimizer's step count stays
    snap = step.flat.data.clone()
    xb = dict(x, pitch=x["pitch"].clone())
    xb["pitch"][0, 0] = float("inf")
    step.step(xb, y)
    assert step.skipped == 1 and step.scale == 1024.0 and step.t == 1 and torch.equal(step.flat.data, snap)
    step.growth_interval = 2
    step.step(x, y)
    step.step(x, y)
    assert step.scale == 2048.0 and step.t == 3                 # two clean steps in a row: the scale doubles


@pytest.mark.gpu
def test_gpu_precision16_step_matches_reference_amp():
    check_precision16_step("cuda")


def test_simulated_precision16_step_matches_reference_amp():
    with use_sim():
        check_precision16_step("cpu")


# ---------------------------------------------------------------------------------------------------------------- at size
# Seeds of the at-size cases, chosen by tools/find_margin_seed.py so that every kink of the training graph (the predictor ReLUs,
# the duration head's ReLU, the L1 loss's |.|) sits at least KINK_MARGIN away from zero in the fp64 reference run: SURVEY 7
# "discrete decisions ... tests must exempt/flag elements within 1e-5 of a boundary".  Round 2's seed had an
# energy_decoder.conv1 pre-activation 3.7e-7 from zero; two correct fp32 implementations landed on opposite sides of it and the
# test's verdict depended on the box's MIOpen build.
KINK_MARGIN = 2e-5
AT_SIZE = {"tiny": (6, 97, 26), "small": (3, 61, 15), "base": (2, 150, 247)}           # name -> (B, T, seed)


def at_size_case(name, seed=None):
    """A ragged teacher-forced batch with ~100 phonemes / ~350 frames per utterance: several row chunks in every reduction, odd
    lengths through the stride-2 blocks, pooled masks, cropped ConvTranspose outputs, zero-length phonemes -- what the
    13-phoneme reference fixtures cannot reach.  -> (cfg, numpy state dict, x, y) on the CPU."""
    B, T, seed0 = AT_SIZE[name]
    seed = seed0 if seed is None else seed
    cfg = CONFIGS[name]
    from efficientspeech_amd.synth import synth_phonemes
    rng = np.random.default_rng(seed)
    lens = sorted(rng.integers(T // 3, T + 1, B).tolist(), reverse=True)
    lens[0] = T
    ids, mask = synth_phonemes(B, T, 11 + seed, lens)
    dur = rng.integers(0, 7, (B, T)).astype(np.int32)
    dur[mask] = 0
    mel_len = dur.sum(1)
    L = int(mel_len.max())
    t = torch.from_numpy
    x = {"phoneme": t(ids), "phoneme_mask": t(mask), "pitch": t(rng.uniform(-3, 11, (B, T)).astype(np.float32)),
         "energy": t(rng.uniform(-2, 8, (B, T)).astype(np.float32)), "duration": t(dur), "mel_len": t(mel_len.astype(np.int32)),
         "mel_mask": t(np.arange(L)[None, :] >= mel_len[:, None])}
    y = {"mel": t(rng.normal(-5, 2, (B, L, 80)).astype(np.float32))}
    return cfg, synth_state_dict(cfg, 1234), x, y


def fp64_reference(cfg, sd, x, y, backward=True):
    """Loss, every parameter gradient and the kink margins of the case from the plain-PyTorch mirror on the CPU in float64:
    deterministic on every box (no MIOpen / hipBLASLt in the checker), round-off 1e-15 -- the reference the fp32 kernels are
    measured against.  -> (total, {name: grad or None}, {kink: min |input|})."""
    from tests import torch_mirror as M
    net = build_phoneme2mel(cfg)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    net = net.double().train()
    for k, p in net.named_parameters():
        p.requires_grad_(not k.endswith("_bins"))
    dbl = lambda d: {k: (v.double() if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in d.items()}   # noqa: E731
    x64, y64 = dbl(x), dbl(y)
    M.TAPS = {}
    try:
        out = M.train_forward(net, dict(x64, mel=y64["mel"]))
        _, total = M.loss(out, x64, y64)
        taps = dict(M.TAPS)
    finally:
        M.TAPS = None
    if backward:
        total.backward()
    return float(total.detach()), {k: (None if p.grad is None else p.grad.clone()) for k, p in net.named_parameters()}, taps


def check_gradients_at_size(dev, name, perturb=None):
    """Every parameter gradient of the training step's kernels (both operator paths) against the fp64 mirror, per parameter,
    relative to the parameter's largest gradient.  `perturb`: a function applied to the kernels' gradients before the
    comparison (the self-test below shows the bounds catch a 1e-3 error in one tensor)."""
    from efficientspeech_amd import train
    cfg, sd, x, y = at_size_case(name)
    rtotal, ref, taps = fp64_reference(cfg, sd, x, y)
    assert len(taps) == 11 and min(taps.values()) > KINK_MARGIN, (
        "the at-size case has a kink input within the margin; pick another seed with tools/find_margin_seed.py", taps)
    net = build_phoneme2mel(cfg)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    net = net.to(dev).train()
    xd, yd = ({k: v.to(dev) for k, v in d.items()} for d in (x, y))
    worst = {}
    old = train.USE_MATRIX_PIPE
    try:
        for matrix_pipe, bound in ((False, FP32_BOUND), (True, SPLIT_BOUND)):
            train.USE_MATRIX_PIPE = matrix_pipe
            for p in net.parameters():
                p.grad = None
            parts, total = train.training_loss(net, xd, yd)
            total.backward()
            assert abs(float(total.detach()) - rtotal) < 2e-5 * rtotal, (float(total.detach()), rtotal)
            errs = []
            for k, p in net.named_parameters():
                if ref[k] is None:
                    assert p.grad is None or float(p.grad.abs().max()) == 0.0, k
                    continue
                m = p.grad.detach().double().cpu()
                if perturb is not None:
                    m = perturb(k, m)
                errs.append((float((m - ref[k]).abs().max()) / max(1e-6, float(ref[k].abs().max())), k))
            assert len(errs) >= 100
            worst[matrix_pipe] = max(errs)
            assert max(errs)[0] < bound, (matrix_pipe, sorted(errs)[-5:])
    finally:
        train.USE_MATRIX_PIPE = old
    return worst


# per-parameter bounds (max |g - g_ref| / max |g_ref|) against the fp64 reference, no kink within the margin.  Measured on the
# simulator (tools/find_margin_seed.py --errors): plain-fp32 kernels 1.1e-6, split-f16 GEMMs 3.6e-6 (tiny); 1.4e-6 / 3.2e-6 (small).
# base (B = 2, T = 150: both encoder stages on the global-memory attention pair, N = 150 at C = 128 and N = 75 at C = 256) on the device:
# 2.2e-6 / 4.0e-6, the fp32 plain-PyTorch mirror 1.4e-6 (profiles/r20_train_variants.md); 39 s on the simulator, so its twin stays with tiny.
FP32_BOUND = 1e-5
SPLIT_BOUND = 2e-5


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["tiny", "small", "base"])
def test_gpu_gradients_match_fp64_mirror_at_size(name):
    check_gradients_at_size("cuda", name)


def test_simulated_gradients_match_fp64_mirror_at_size():
    """The CPU-tier twin of the GPU test above (tiny ES, the same case, the same bounds) on the wave simulator."""
    with use_sim():
        check_gradients_at_size("cpu", "tiny")


def test_at_size_check_catches_a_perturbed_gradient():
    """The bounds are tight enough to see a kernel that is wrong by 1e-3 of one tensor's scale in one element."""
    def perturb(k, m):
        if k == "encoder.energy_decoder.conv1.0.weight":
            m = m.clone()
            m.view(-1)[7] += 1e-3 * float(m.abs().max())
        return m
    with use_sim():
        with pytest.raises(AssertionError, match="energy_decoder.conv1.0.weight"):
            check_gradients_at_size("cpu", "tiny", perturb)


@pytest.mark.parametrize("B,T,lens", [(2, 1, [1, 1]), (1, 2, [2]), (3, 5, [5, 2, 1])], ids=["T1", "B1_T2", "ragged_T5"])
def test_simulated_edge_shapes_match_torch_mirror(B, T, lens):
    """One-phoneme utterances, a single two-phoneme utterance, a ragged 5 / 2 / 1 batch: loss and every gradient of the simulated
    kernels against torch.autograd over the plain-PyTorch mirror (the stride-2 block sees N = 1, the pooled masks their edge cases)."""
    from efficientspeech_amd import train
    from efficientspeech_amd.synth import synth_phonemes
    from tests import torch_mirror as M
    cfg = CONFIGS["tiny"]
    sd = synth_state_dict(cfg, 1234)
    nets = []
    for _ in range(2):
        n = build_phoneme2mel(cfg)
        n.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
        nets.append(n.train())
    for k, p in nets[1].named_parameters():
        p.requires_grad_(not k.endswith("_bins"))
    rng = np.random.default_rng(0)
    ids, mask = synth_phonemes(B, T, 3, lens)
    dur = rng.integers(1, 4, (B, T)).astype(np.int32)
    dur[mask] = 0
    ml = dur.sum(1)
    L = int(ml.max())
    t = torch.from_numpy
    x = {"phoneme": t(ids), "phoneme_mask": t(mask), "pitch": t(rng.normal(0, 3, (B, T)).astype(np.float32)),
         "energy": t(rng.normal(0, 3, (B, T)).astype(np.float32)), "duration": t(dur), "mel_len": t(ml.astype(np.int32)),
         "mel_mask": t(np.arange(L)[None] >= ml[:, None])}
    y = {"mel": t(rng.normal(-5, 2, (B, L, 80)).astype(np.float32))}
    with use_sim():
        parts, total = train.training_loss(nets[0], x, y)
        total.backward()
    _, rt = M.loss(M.train_forward(nets[1], dict(x, mel=y["mel"])), x, y)
    rt.backward()
    assert abs(float(total.detach()) - float(rt.detach())) < 2e-5 * float(rt.detach())
    ref = dict(nets[1].named_parameters())
    bad = [k for k, p in nets[0].named_parameters() if ref[k].grad is not None and
           float((p.grad - ref[k].grad).abs().max()) > 1e-4 * max(1e-6, float(ref[k].grad.abs().max()))]
    assert len(bad) <= 2, bad          # (a ReLU input on zero may take the other branch: see the at-size GPU test)


def _ddp_gpu_worker(rank, world, port, out_path, backend="gloo"):
    """Two data-parallel ranks on cuda:0 (gloo carries device tensors): the hipGraph-replayed step (forward + loss + backward captured,
    all-reduce + optimizer eager) against the eager step, different batches per rank."""
    import torch.distributed as dist
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    if backend == "nccl":          # RCCL: one rank per GPU; the flat gradient buffer's all-reduce goes over xGMI
        torch.cuda.set_device(rank)
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", rank))
    else:
        torch.cuda.set_device(0)
        dist.init_process_group("gloo", rank=rank, world_size=world)
    res = {}
    for mode in ("eager", "graph"):
        train, g, net, x, y = _setup("cuda")
        sel = slice(rank, rank + 1)
        cut = lambda d: {k: (torch.cat([v[sel], v[sel]]) if torch.is_tensor(v) and v.dim() > 0 and v.shape[0] == 2 else v)   # noqa: E731
                         for k, v in d.items()}
        step = train.TrainStep(net, world_size=world, graph=(mode == "graph"))
        losses = [step.step(cut(x), cut(y)).clone() for _ in range(4)]
        res[mode] = (step.flat.data.clone(), torch.stack(losses))
        flat = step.flat.data
        gather = [torch.empty_like(flat) for _ in range(world)]
        dist.all_gather(gather, flat)
        res[mode + "_same"] = torch.equal(gather[0], gather[1])
    if rank == 0:
        ok_params = torch.allclose(res["eager"][0], res["graph"][0], rtol=1e-4, atol=1e-6)
        ok_losses = torch.allclose(res["eager"][1], res["graph"][1], rtol=1e-5, atol=0)
        np.save(out_path, np.array([int(res["eager_same"]), int(res["graph_same"]), int(ok_params), int(ok_losses)]))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.gpu
def test_gpu_two_rank_captured_step_equals_eager_step(tmp_path):
    """Data-parallel + hipGraph: replicas stay identical and the replayed steps equal the eager ones."""
    import torch.multiprocessing as mp
    out = str(tmp_path / "ddp_graph.npy")
    mp.spawn(_ddp_gpu_worker, args=(2, _free_port(), out), nprocs=2, join=True)
    assert np.load(out).tolist() == [1, 1, 1, 1]


@pytest.mark.gpu
@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="RCCL needs one device per rank: runs on the first multi-GPU lease")
def test_gpu_rccl_data_parallel_step_keeps_replicas_identical(tmp_path):
    """BASELINE configs[4]'s collective on the real backend: two ranks, one GPU each, `TrainStep`'s ONE all-reduce of the flat
    gradient buffer over RCCL (eager and around the hipGraph-replayed step): replicas bit-identical after four steps, replayed ==
    eager.  Auto-skips on a 1-GPU box."""
    import torch.multiprocessing as mp
    out = str(tmp_path / "ddp_rccl.npy")
    mp.spawn(_ddp_gpu_worker, args=(2, _free_port(), out, "nccl"), nprocs=2, join=True)
    assert np.load(out).tolist() == [1, 1, 1, 1]
