"""Opt-in gradient-norm clipping of the training step (`TrainStep(gradient_clip_val=c)`: torch.nn.utils.clip_grad_norm_(params, c, 2)
between the unscale and the AdamW update, on the device).  The checks live in tests/grad_clip_checks.py; each runs on the MI355X
through libesmi.so (-m gpu) and on the CPU wave-simulator build of the same kernels; the data-parallel step runs as two gloo ranks on
the simulator."""
import os
import sys

import numpy as np
import pytest
import torch

from tests import grad_clip_checks as K
from tests.simlib import launch_records, launched_kernels, use_sim
from tests.test_train_step import ROOT, _free_port, _setup

PRECISIONS = [32, 16, "bf16"]


def test_partials_constant_is_the_headers():
    from efficientspeech_amd import _lib
    assert _lib.TRAIN_GRAD_NORM_PARTIALS == K.PARTIALS == _lib.MIRRORED["ESMI_TRAIN_GRAD_NORM_PARTIALS"]
    assert (_lib.HYPER_GRAD_NORM, _lib.HYPER_CLIP_COEF, _lib.TRAIN_ADAMW_HYPER_FLOATS) == (6, 7, 8)


# ---------------------------------------------------------------------------------------------- 1. the reduction alone
@pytest.mark.parametrize("n", K.SIZES)
def test_simulated_sumsq_matches_float64_norm(n):
    with use_sim():
        K.check_sumsq("cpu", n)


@pytest.mark.gpu
@pytest.mark.parametrize("n", K.SIZES + (K.SIZE_SECOND_TRIP,))
def test_gpu_sumsq_matches_float64_norm(n):
    K.check_sumsq("cuda", n)


# ---------------------------------------------------------------------------------------------- 2. the optimizer launch alone
def test_simulated_clipped_optimizer_launch_matches_torch():
    with use_sim():
        K.check_optimizer_launch("cpu", launched_kernels)


@pytest.mark.gpu
def test_gpu_clipped_optimizer_launch_matches_torch():
    K.check_optimizer_launch("cuda")


def test_simulated_inactive_clip_is_bitwise_the_unclipped_launch():
    with use_sim():
        K.check_inactive_clip_is_bitwise_the_unclipped_launch("cpu")


@pytest.mark.gpu
def test_gpu_inactive_clip_is_bitwise_the_unclipped_launch():
    K.check_inactive_clip_is_bitwise_the_unclipped_launch("cuda")


# ---------------------------------------------------------------------------------------------- 3. the whole step
@pytest.mark.parametrize("precision", PRECISIONS)
def test_simulated_clipped_step_matches_torch_clip_and_adamw(precision):
    with use_sim():
        K.check_whole_step("cpu", precision)


@pytest.mark.gpu
@pytest.mark.parametrize("precision", PRECISIONS)
def test_gpu_clipped_step_matches_torch_clip_and_adamw(precision):
    K.check_whole_step("cuda", precision)


def test_simulated_check_catches_a_wrong_clip_value():
    """The same comparison against a reference that clips by 1.1 c must fail: the moments see the coefficient."""
    with use_sim():
        with pytest.raises(AssertionError, match="'m'"):
            K.check_whole_step("cpu", 32, c_factor=1.1)


@pytest.mark.gpu
def test_gpu_check_catches_a_wrong_clip_value():
    with pytest.raises(AssertionError, match="'m'"):
        K.check_whole_step("cuda", 32, c_factor=1.1)


# ---------------------------------------------------------------------------------------------- 4. GPU only
@pytest.mark.gpu
def test_gpu_captured_clipped_step_equals_eager_clipped_step():
    K.check_captured_clipped_step_equals_eager("cuda")


@pytest.mark.gpu
@pytest.mark.parametrize("how", ["scale", "target"])
def test_gpu_precision16_overflow_still_skips_with_clipping(how):
    K.check_precision16_overflow_still_skips("cuda", how)


@pytest.mark.parametrize("how", ["scale", "target"])
def test_simulated_precision16_overflow_still_skips_with_clipping(how):
    with use_sim():
        K.check_precision16_overflow_still_skips("cpu", how)


# ---------------------------------------------------------------------------------------------- 5. two gloo ranks on the simulator
def _ddp_clip_worker(rank, world, port, out_path):
    import torch.distributed as dist
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), WAVESIM_THREADS="2")
    dist.init_process_group("gloo", rank=rank, world_size=world)
    train, g, net, x, y = _setup("cpu")
    sel = slice(rank, rank + 1)                                        # rank r trains on utterance r of the fixture batch
    cut = lambda d: {k: (torch.cat([v[sel], v[sel]]) if torch.is_tensor(v) and v.dim() > 0 and v.shape[0] == 2 else v)   # noqa: E731
                     for k, v in d.items()}
    with use_sim():
        step = train.TrainStep(net, world_size=world, gradient_clip_val=100.0)      # (the fixture's gradient norm is ~300)
        before = step.flat.data.clone()
        step.step(cut(x), cut(y))
        mine = torch.tensor([step.grad_norm, step.clip_coef, float(step.flat.grad.double().norm())], dtype=torch.float64)
        stats = [torch.empty_like(mine) for _ in range(world)]
        dist.all_gather(stats, mine)
        flat = step.flat.data.clone()
        gather = [torch.empty_like(flat) for _ in range(world)]
        dist.all_gather(gather, flat)
    if rank == 0:
        np.save(out_path, np.array([float(torch.equal(gather[0], gather[1])), float(not torch.equal(flat, before)),
                                    *stats[0].tolist(), *stats[1].tolist()]))
    dist.barrier()
    dist.destroy_process_group()


def test_two_rank_clipped_step_clips_every_replica_by_the_same_coefficient(tmp_path):
    """The norm is taken after the all-reduce and the division by the world size: both ranks report the same norm -- the float64 norm
    of the averaged buffer -- and the same coefficient, and the replicas stay identical."""
    import torch.multiprocessing as mp
    out = str(tmp_path / "ddp_clip.npy")
    mp.spawn(_ddp_clip_worker, args=(2, _free_port(), out), nprocs=2, join=True)
    same_params, moved, n0, c0, ref0, n1, c1, ref1 = np.load(out)
    assert same_params == 1 and moved == 1
    assert n0 == n1 and c0 == c1 and ref0 == ref1 and c0 < 1.0
    assert abs(n0 - ref0) <= K.NORM_RTOL * ref0, (n0, ref0)


# ---------------------------------------------------------------------------------------------- 6. launch pin
@pytest.mark.parametrize("precision", [32, "bf16"])
def test_clipped_step_adds_exactly_the_reduction_launch(precision):
    """Beside tests/test_train_dispatch.py's rows: the clipped step's launches are those of the unclipped step with its optimizer's
    scalars on the device (what a captured step runs; its micro-batch and boundary are run eagerly here, capture cannot run on the simulator) plus exactly
    one launch, the reduction, directly in front of the bookkeeping kernel -- every other record (name, grid, block, LDS) unchanged."""
    with use_sim():
        train, _, net, x, y = _setup("cpu")
        plain = train.TrainStep(net, precision=precision, graph=True)
        plain._opt.set_lr(plain.lr)
        with launch_records() as base:
            plain._micro_batch(x, y)
            plain._boundary()
        train, _, net, x, y = _setup("cpu")
        clipped = train.TrainStep(net, precision=precision, gradient_clip_val=1.0)
        n = clipped.flat.grad.numel()
        with launch_records() as got:
            clipped.step(x, y)
    names = [name for name, _ in base]
    assert names.count("train_bump_step_kernel") == 1 and names[-2:] == ["train_bump_step_kernel", "train_adamw_dev_kernel"]
    at = names.index("train_bump_step_kernel")
    blocks = min(K.PARTIALS, (n // 4 + 255) // 256)
    assert n % 4 == 0 and 1 < blocks < K.PARTIALS
    want = base[:at] + [("train_grad_sumsq_kernel", f"{blocks},1,1|256,1,1|2048"), ("train_bump_clip_kernel", "1,1,1|256,1,1|2048")] + base[at + 1:]
    assert got == want and len(got) == len(base) + 1


# ---------------------------------------------------------------------------------------------- 7. arguments
def test_gradient_clip_val_arguments():
    K.check_arguments()
    train, _, net, x, y = _setup("cpu")
    with pytest.raises(ValueError):
        train.TrainStep(net, gradient_clip_val=-0.5)
    step = train.TrainStep(net)                      # clipping off: the read-outs do not exist, as `growth_interval` without a scaler
    for name in ("grad_norm", "clip_coef"):
        with pytest.raises(AttributeError):
            getattr(step, name)
