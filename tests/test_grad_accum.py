"""Opt-in gradient accumulation of the training step (`TrainStep(accumulate_grad_batches=N)`, Lightning's Trainer knob of that name: the
micro-batches' gradients / N add up in a buffer of their own, and unscale, clipping, AdamW and the data-parallel exchange run once per
window on the sum).  The checks live in tests/grad_accum_checks.py; each runs on the MI355X through libesmi.so (-m gpu) and on the CPU
wave-simulator build of the same kernels; the data-parallel window runs as two gloo ranks on the simulator."""
import os
import sys

import numpy as np
import pytest
import torch

from tests import grad_accum_checks as K
from tests.simlib import launch_records, launched_kernels, use_sim
from tests.test_train_step import ROOT, _free_port, _setup

PRECISIONS = [32, 16, "bf16"]
OPTIMIZER_KERNELS = {"train_adamw_kernel", "train_adamw_dev_kernel", "train_bump_step_kernel", "train_bump_clip_kernel", "train_grad_sumsq_kernel"}


def test_entry_point_is_declared_exported_and_version_stays():
    from efficientspeech_amd import _lib
    from tests.test_abi_exports import header_constants, header_functions
    assert "esmi_train_grad_accumulate_f32" in _lib.EXPORTS and "esmi_train_grad_accumulate_f32" in header_functions()
    assert header_constants()["ESMI_VERSION"] == 501


# ---------------------------------------------------------------------------------------------- 1. the kernel alone
@pytest.mark.parametrize("n", K.SIZES)
def test_simulated_accumulate_kernel_matches_float64(n):
    with use_sim():
        K.check_kernel("cpu", n)


@pytest.mark.gpu
@pytest.mark.parametrize("n", K.SIZES + (K.SIZE_SECOND_TRIP,))
def test_gpu_accumulate_kernel_matches_float64(n):
    K.check_kernel("cuda", n)


def test_simulated_accumulate_kernel_passes_inf_and_nan_on_and_launches_nothing_for_n_0():
    with use_sim():
        K.check_kernel_nonfinite_and_empty("cpu", launched_kernels)


@pytest.mark.gpu
def test_gpu_accumulate_kernel_passes_inf_and_nan_on():
    K.check_kernel_nonfinite_and_empty("cuda")


def test_simulated_accumulate_launch_geometry():
    """One workgroup of 256 per 256 float4s (or per 256 scalars on the misaligned path), at most 1024 of them, no LDS."""
    with use_sim():
        for n, off, blocks in ((2051, 0, 2), (2051, 1, 9), (3, 0, 1), (K.GRID_CAP * 256 * 4 + 5, 0, K.GRID_CAP)):
            buf, g = torch.zeros(n + off), torch.ones(n)
            with launch_records() as got:
                K._accumulate(buf[off:], g, n, 0.5)
            assert got == [("train_grad_accumulate_kernel", f"{blocks},1,1|256,1,1|0")], (n, off, got)
            assert bool((buf[off:] == 0.5).all()) and bool((buf[:off] == 0).all())


# ---------------------------------------------------------------------------------------------- 2. one window against torch
@pytest.mark.parametrize("clip", [False, True], ids=["unclipped", "clipped"])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_simulated_window_matches_torch_clip_and_adamw_on_the_sum(precision, clip):
    with use_sim():
        K.check_window("cpu", precision, clip)


@pytest.mark.gpu
@pytest.mark.parametrize("clip", [False, True], ids=["unclipped", "clipped"])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_gpu_window_matches_torch_clip_and_adamw_on_the_sum(precision, clip):
    K.check_window("cuda", precision, clip)


# ---------------------------------------------------------------------------------------------- 3. the check catches a wrong weight
def test_simulated_check_catches_a_wrong_weight():
    """The same comparison against a reference that weighs every micro-batch by 1 / (N + 1) must fail: the first moment sees the weight.
    (Unclipped: a clipped window's coefficient would scale a uniformly wrong weight away again.)"""
    with use_sim():
        with pytest.raises(AssertionError, match="'m'"):
            K.check_window("cpu", 32, False, wrong_n=K.N_WINDOW + 1)


@pytest.mark.gpu
def test_gpu_check_catches_a_wrong_weight():
    with pytest.raises(AssertionError, match="'m'"):
        K.check_window("cuda", 32, False, wrong_n=K.N_WINDOW + 1)


# ---------------------------------------------------------------------------------------------- 4. the accumulated gradient against autograd
def test_simulated_accumulated_gradient_matches_fp64_mirror_at_size():
    with use_sim():
        K.check_accumulated_gradient_at_size("cpu")


@pytest.mark.gpu
def test_gpu_accumulated_gradient_matches_fp64_mirror_at_size():
    K.check_accumulated_gradient_at_size("cuda")


# ---------------------------------------------------------------------------------------------- 5. off is off
def test_simulated_off_is_off():
    with use_sim():
        K.check_off_is_off("cpu", launch_records)


@pytest.mark.gpu
def test_gpu_off_is_off():
    K.check_off_is_off("cuda")


# ---------------------------------------------------------------------------------------------- 6. launch pin
@pytest.mark.parametrize("precision", [32, "bf16"])
def test_micro_batch_adds_exactly_the_accumulate_launch(precision):
    """Beside tests/test_train_dispatch.py's rows: a non-boundary call launches what the plain step launches up to and including the
    reduction flush, then exactly one train_grad_accumulate_kernel and no optimizer kernel; the boundary call launches the same and
    then the plain step's optimizer records, unchanged."""
    with use_sim():
        train, _, net, x, y = _setup("cpu")
        plain = train.TrainStep(net, precision=precision)
        with launch_records() as base:
            plain.step(x, y)
        train, _, net, x, y = _setup("cpu")
        step = train.TrainStep(net, precision=precision, accumulate_grad_batches=2)
        n = step.flat.grad.numel()
        with launch_records() as first:
            step.step(x, y)
        with launch_records() as second:
            step.step(x, y)
    names = [name for name, _ in base]
    at = max(j for j, name in enumerate(names) if name == "train_reduce_batch_kernel")
    head, optimizer = base[:at + 1], base[at + 1:]
    assert optimizer and {name for name, _ in optimizer} <= OPTIMIZER_KERNELS and not OPTIMIZER_KERNELS & set(names[:at + 1])
    blocks = (n // 4 + 255) // 256
    assert n % 4 == 0 and 1 < blocks < K.GRID_CAP
    add = [("train_grad_accumulate_kernel", f"{blocks},1,1|256,1,1|0")]
    assert first == head + add and len(first) == len(base) - len(optimizer) + 1
    assert second == head + add + optimizer


# ---------------------------------------------------------------------------------------------- 7. GPU only
@pytest.mark.gpu
def test_gpu_captured_window_equals_eager_window():
    K.check_captured_window_equals_eager("cuda")


@pytest.mark.gpu
def test_gpu_checkpoint_between_windows_resumes_into_a_captured_step():
    K.check_checkpoint_between_windows_resumes_into_a_captured_step("cuda")


# ---------------------------------------------------------------------------------------------- 8. precision-16 overflow
def test_simulated_precision16_overflow_in_one_micro_batch_skips_the_window():
    with use_sim():
        K.check_precision16_overflow_skips_the_window("cpu")


@pytest.mark.gpu
def test_gpu_precision16_overflow_in_one_micro_batch_skips_the_window():
    K.check_precision16_overflow_skips_the_window("cuda")


# ---------------------------------------------------------------------------------------------- 9. two gloo ranks on the simulator
def _ddp_accum_worker(rank, world, port, out_path):
    import torch.distributed as dist
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), WAVESIM_THREADS="2")
    dist.init_process_group("gloo", rank=rank, world_size=world)
    train, g, net, x, y = _setup("cpu")
    sel = slice(rank, rank + 1)                                        # rank r: utterance r twice, then the whole fixture batch
    cut = lambda d: {k: (torch.cat([v[sel], v[sel]]) if torch.is_tensor(v) and v.dim() > 0 and v.shape[0] == 2 else v)   # noqa: E731
                     for k, v in d.items()}
    entered, inner = [], dist.all_reduce

    def counting(tensor, *a, **kw):
        entered.append(tensor.numel())
        return inner(tensor, *a, **kw)
    dist.all_reduce = counting
    try:
        with use_sim():
            step = train.TrainStep(net, world_size=world, gradient_clip_val=100.0, accumulate_grad_batches=2)   # (the fixture's norm is ~300)
            before = step.flat.data.clone()
            step.step(cut(x), cut(y))
            inside = (len(entered), step.t, step.micro, float(torch.equal(step.flat.data, before)))
            step.step(x, y)
            calls, size = len(entered), (entered[0] if entered else 0)
    finally:
        dist.all_reduce = inner
    mine = torch.tensor([step.grad_norm, step.clip_coef, float(calls), float(size == step.flat.acc.numel()), float(inside == (0, 0, 1, 1.0)),
                         float(step.t), float(step.micro), float(step.flat.acc.abs().max())], dtype=torch.float64)
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


def test_two_rank_window_exchanges_once_and_keeps_the_replicas_identical(tmp_path):
    """N = 2 with clipping on two ranks: nothing is exchanged (and nothing moves) after the first micro-batch, the all-reduce is entered
    exactly once per window, on the accumulator; both ranks report the same norm and coefficient and the replicas stay identical."""
    import torch.multiprocessing as mp
    out = str(tmp_path / "ddp_accum.npy")
    mp.spawn(_ddp_accum_worker, args=(2, _free_port(), out), nprocs=2, join=True)
    res = np.load(out)
    same_params, moved = res[:2]
    r0, r1 = res[2:10], res[10:18]
    assert same_params == 1 and moved == 1
    for norm, coef, calls, on_acc, quiet_inside, t, micro, acc_max in (r0, r1):
        assert calls == 1 and on_acc == 1 and quiet_inside == 1 and t == 1 and micro == 0 and acc_max == 0
        assert np.isfinite(norm) and 0 < coef < 1.0
    assert r0[0] == r1[0] and r0[1] == r1[1]


# ---------------------------------------------------------------------------------------------- 10. fit
def test_simulated_fit_flushes_every_epoch_and_logs_per_micro_batch():
    with use_sim():
        K.check_fit("cpu")


# ---------------------------------------------------------------------------------------------- 11. state_dict() and arguments
def test_simulated_state_dict_refuses_an_open_window_and_load_clears_one():
    with use_sim():
        K.check_state_dict_and_flush("cpu")


def test_accumulate_grad_batches_arguments():
    K.check_arguments()
