"""Opt-in exponential moving average of the weights in the training step (`TrainStep(ema_decay=d)`: torch.optim.swa_utils.AveragedModel with
get_ema_multi_avg_fn(d), one launch behind the optimizer's), running the model on it (`ema_weights()`, an in-place exchange), the
validation loss (`evaluate`) and `fit`'s validation pass.  The checks live in tests/weight_ema_checks.py; each runs on the MI355X through
libesmi.so (-m gpu) and on the CPU wave-simulator build of the same kernels; the data-parallel run is two gloo ranks on the simulator."""
import os
import sys

import numpy as np
import pytest
import torch

from tests import weight_ema_checks as K
from tests.simlib import launch_records, launched_kernels, use_sim
from tests.test_grad_accum import OPTIMIZER_KERNELS
from tests.test_train_step import ROOT, _free_port, _setup

PRECISIONS = [32, 16, "bf16"]


# ---------------------------------------------------------------------------------------------- 1. ABI
def test_entry_points_are_declared_exported_and_version_stays():
    from efficientspeech_amd import _lib
    from tests.test_abi_exports import header_constants, header_functions
    for name in ("esmi_train_ema_update_f32", "esmi_train_swap_f32"):
        assert name in _lib.EXPORTS and name in header_functions()
    assert header_constants()["ESMI_VERSION"] == 501


# ---------------------------------------------------------------------------------------------- 2. the update kernel alone
@pytest.mark.parametrize("n", K.SIZES)
def test_simulated_update_kernel_matches_float64(n):
    with use_sim():
        K.check_update_kernel("cpu", n)


@pytest.mark.gpu
@pytest.mark.parametrize("n", K.SIZES + (K.SIZE_SECOND_TRIP,))
def test_gpu_update_kernel_matches_float64(n):
    K.check_update_kernel("cuda", n)


# ---------------------------------------------------------------------------------------------- 3. the skip flag
def test_simulated_update_kernel_obeys_the_skip_flag():
    with use_sim():
        K.check_skip_flag("cpu")


@pytest.mark.gpu
def test_gpu_update_kernel_obeys_the_skip_flag():
    K.check_skip_flag("cuda")


# ---------------------------------------------------------------------------------------------- 4. non-finite values, empty input, overlap
def test_simulated_update_kernel_passes_inf_and_nan_on_and_launches_nothing_for_n_0():
    with use_sim():
        K.check_update_nonfinite_and_empty("cpu", launched_kernels)


@pytest.mark.gpu
def test_gpu_update_kernel_passes_inf_and_nan_on():
    K.check_update_nonfinite_and_empty("cuda")


# ---------------------------------------------------------------------------------------------- 5. the exchange
@pytest.mark.parametrize("n", K.SIZES)
def test_simulated_swap_kernel_exchanges_every_bit(n):
    with use_sim():
        K.check_swap_kernel("cpu", n)


@pytest.mark.gpu
@pytest.mark.parametrize("n", K.SIZES + (K.SIZE_SECOND_TRIP,))
def test_gpu_swap_kernel_exchanges_every_bit(n):
    K.check_swap_kernel("cuda", n)


def test_simulated_swap_kernel_launches_nothing_for_n_0_and_refuses_overlap():
    with use_sim():
        K.check_swap_empty_and_overlap("cpu", launched_kernels)


@pytest.mark.gpu
def test_gpu_swap_kernel_takes_n_0_and_refuses_overlap():
    K.check_swap_empty_and_overlap("cuda")


# ---------------------------------------------------------------------------------------------- 6. launch geometry
def test_simulated_launch_geometry():
    """Both kernels: one workgroup of 256 per 256 float4s (or per 256 scalars on the misaligned path), at most 1024 of them, no LDS."""
    with use_sim():
        for n, off, blocks in ((2051, 0, 2), (2051, 1, 9), (3, 0, 1), (K.GRID_CAP * 256 * 4 + 5, 0, K.GRID_CAP)):
            buf, p = torch.zeros(n + off), torch.ones(n)
            with launch_records() as got:
                K._update(buf[off:], p, n, 0.5)
            assert got == [("train_ema_update_kernel", f"{blocks},1,1|256,1,1|0")], (n, off, got)
            assert bool((buf[off:] == 0.5).all()) and bool((buf[:off] == 0).all())
            with launch_records() as got:
                K._swap(buf[off:], p, n)
            assert got == [("train_swap_kernel", f"{blocks},1,1|256,1,1|0")], (n, off, got)
            assert bool((buf[off:] == 1).all()) and bool((buf[:off] == 0).all()) and bool((p == 0.5).all())


# ---------------------------------------------------------------------------------------------- 7. the average follows the steps
@pytest.mark.parametrize("precision", PRECISIONS)
def test_simulated_average_follows_the_steps(precision):
    with use_sim():
        K.check_average_follows_the_steps("cpu", precision)


@pytest.mark.gpu
@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_gpu_average_follows_the_steps(precision, graph):
    K.check_average_follows_the_steps("cuda", precision, graph)


def test_simulated_check_catches_a_wrong_decay():
    """The same comparison against a reference with decay 0.99 must fail: one AdamW step moves a weight by about lr, far above the bound."""
    with use_sim():
        with pytest.raises(AssertionError):
            K.check_average_follows_the_steps("cpu", 32, decay=0.99)


@pytest.mark.gpu
def test_gpu_check_catches_a_wrong_decay():
    with pytest.raises(AssertionError):
        K.check_average_follows_the_steps("cuda", 32, decay=0.99)


# ---------------------------------------------------------------------------------------------- 8. accumulation
def test_simulated_average_moves_only_on_a_windows_boundary_and_on_flush():
    with use_sim():
        K.check_accumulation("cpu")


@pytest.mark.gpu
def test_gpu_average_moves_only_on_a_windows_boundary_and_on_flush():
    K.check_accumulation("cuda")


# ---------------------------------------------------------------------------------------------- 9. precision-16 overflow
def test_simulated_precision16_overflow_leaves_the_average():
    with use_sim():
        K.check_precision16_overflow_leaves_the_average("cpu")


@pytest.mark.gpu
@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_gpu_precision16_overflow_leaves_the_average(graph):
    K.check_precision16_overflow_leaves_the_average("cuda", graph)


# ---------------------------------------------------------------------------------------------- 10. launch pin
def _update_record(step):
    n = step.flat.data.numel()
    blocks = (n // 4 + 255) // 256
    assert n % 4 == 0 and 1 < blocks < K.GRID_CAP
    return [("train_ema_update_kernel", f"{blocks},1,1|256,1,1|0")]


@pytest.mark.parametrize("precision", [32, 16])
def test_step_adds_exactly_the_update_launch(precision):
    """Beside tests/test_train_dispatch.py's rows: a step with the average launches the plain step's records and then exactly one
    train_ema_update_kernel; with accumulate_grad_batches=2 the first call launches no update, the second the plain step's records up
    to the reduction flush, the accumulate launch, the optimizer's records and then the update."""
    with use_sim():
        train, _, net, x, y = _setup("cpu")
        with launch_records() as base:
            train.TrainStep(net, precision=precision).step(x, y)
        train, _, net, x, y = _setup("cpu")
        step = train.TrainStep(net, precision=precision, ema_decay=K.DECAY)
        with launch_records() as got:
            step.step(x, y)
        train, _, net, x, y = _setup("cpu")
        acc = train.TrainStep(net, precision=precision, ema_decay=K.DECAY, accumulate_grad_batches=2)
        with launch_records() as first:
            acc.step(x, y)
        with launch_records() as second:
            acc.step(x, y)
    update = _update_record(step)
    assert got == base + update
    names = [name for name, _ in base]
    at = max(j for j, name in enumerate(names) if name == "train_reduce_batch_kernel")
    head, optimizer = base[:at + 1], base[at + 1:]
    assert OPTIMIZER_KERNELS & {name for name, _ in optimizer} and not OPTIMIZER_KERNELS & set(names[:at + 1])
    add = [("train_grad_accumulate_kernel", update[0][1])]
    assert first == head + add
    assert second == head + add + optimizer + update


# ---------------------------------------------------------------------------------------------- 11. off is off
def test_simulated_off_is_off():
    with use_sim():
        K.check_off_is_off("cpu", launch_records)


@pytest.mark.gpu
def test_gpu_off_is_off():
    K.check_off_is_off("cuda")


# ---------------------------------------------------------------------------------------------- 12. ema_weights()
def test_simulated_ema_weights_exchanges_and_restores():
    with use_sim():
        K.check_ema_weights("cpu", bitwise=True)


@pytest.mark.gpu
def test_gpu_ema_weights_exchanges_and_restores():
    K.check_ema_weights("cuda", bitwise=False)


def test_simulated_ema_weights_needs_ema_decay():
    with use_sim():
        K.check_ema_weights_needs_ema_decay("cpu")


# ---------------------------------------------------------------------------------------------- 13. evaluate
@pytest.mark.parametrize("precision", [32, 16])
def test_simulated_evaluate_returns_the_steps_losses(precision):
    with use_sim():
        K.check_evaluate_returns_the_steps_losses("cpu", precision, bitwise=True)


@pytest.mark.gpu
@pytest.mark.parametrize("precision", PRECISIONS)
def test_gpu_evaluate_returns_the_steps_losses(precision):
    K.check_evaluate_returns_the_steps_losses("cuda", precision, bitwise=False)


def test_simulated_evaluate_on_the_average():
    with use_sim():
        K.check_evaluate_on_the_average("cpu", bitwise=True)


@pytest.mark.gpu
def test_gpu_evaluate_on_the_average():
    K.check_evaluate_on_the_average("cuda", bitwise=False)


def test_simulated_evaluate_changes_nothing():
    with use_sim():
        K.check_evaluate_changes_nothing("cpu")


@pytest.mark.gpu
def test_gpu_evaluate_changes_nothing():
    K.check_evaluate_changes_nothing("cuda")


def test_simulated_evaluate_launches_no_optimizer_kernel():
    with use_sim():
        train, _, net, x, y = _setup("cpu")
        step = train.TrainStep(net, ema_decay=K.DECAY)
        step.step(x, y)
        with launched_kernels() as raw:
            step.evaluate(x, y, ema=False)
        with launched_kernels() as avg:
            step.evaluate(x, y)
    for names in (raw, avg):
        assert len(names) > 50 and not OPTIMIZER_KERNELS & set(names) and "train_ema_update_kernel" not in names
        assert "train_grad_accumulate_kernel" not in names and "train_reduce_batch_kernel" not in names
    assert "train_swap_kernel" not in raw
    assert avg[0] == avg[-1] == "train_swap_kernel" and avg[1:-1] == raw


# ---------------------------------------------------------------------------------------------- 14. checkpoint
def test_simulated_checkpoint_carries_the_average():
    with use_sim():
        K.check_checkpoint("cpu", bitwise=True)


@pytest.mark.gpu
def test_gpu_checkpoint_resumes_the_average_into_a_captured_step():
    K.check_checkpoint("cuda", bitwise=False, graph=True)


# ---------------------------------------------------------------------------------------------- 15. two gloo ranks on the simulator
def _ddp_ema_worker(rank, world, port, out_path):
    import torch.distributed as dist
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), WAVESIM_THREADS="2")
    dist.init_process_group("gloo", rank=rank, world_size=world)
    sel = slice(rank, rank + 1)                                        # rank r trains on utterance r twice: the ranks' gradients differ
    cut = lambda d: {k: (torch.cat([v[sel], v[sel]]) if torch.is_tensor(v) and v.dim() > 0 and v.shape[0] == 2 else v)   # noqa: E731
                     for k, v in d.items()}
    calls, inner = {}, dist.all_reduce

    def counting(tensor, *a, **kw):
        calls[key] += 1
        return inner(tensor, *a, **kw)
    dist.all_reduce = counting
    try:
        with use_sim():
            for key, kw in (("off", {}), ("on", {"ema_decay": K.DECAY})):
                calls[key] = 0
                train, g, net, x, y = _setup("cpu")
                step = train.TrainStep(net, world_size=world, **kw)
                before = step.flat.data.clone()
                step.step(cut(x), cut(y))
    finally:
        dist.all_reduce = inner
    ema = step.flat.ema.clone()
    gather = [torch.empty_like(ema) for _ in range(world)]
    dist.all_gather(gather, ema)
    mine = torch.tensor([float(calls["off"]), float(calls["on"]), float(not torch.equal(ema, before)),
                         float(not torch.equal(ema, step.flat.data))], dtype=torch.float64)
    stats = [torch.empty_like(mine) for _ in range(world)]
    dist.all_gather(stats, mine)
    if rank == 0:
        np.save(out_path, np.array([float(torch.equal(gather[0], gather[1])), *stats[0].tolist(), *stats[1].tolist()]))
    dist.barrier()
    dist.destroy_process_group()


def test_two_rank_average_adds_no_collective_and_stays_identical(tmp_path):
    import torch.multiprocessing as mp
    out = str(tmp_path / "ddp_ema.npy")
    mp.spawn(_ddp_ema_worker, args=(2, _free_port(), out), nprocs=2, join=True)
    res = np.load(out)
    assert res[0] == 1                                               # both ranks hold the same average
    for off, on, moved, differs in (res[1:5], res[5:9]):
        assert off == on == 1 and moved == 1 and differs == 1


# ---------------------------------------------------------------------------------------------- 16. fit
def test_simulated_fit_validates_every_n_epochs():
    with use_sim():
        K.check_fit("cpu")


# ---------------------------------------------------------------------------------------------- 17. arguments
def test_ema_decay_arguments():
    K.check_arguments()
