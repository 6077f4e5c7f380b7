"""Every training kernel variant against float64 at the edge shapes of its dispatch: the table and the checks live in
tests/train_variant_checks.py.  Each row runs on the CPU wave-simulator build of the kernels, where the launched kernels' names are
checked against the row, and on the MI355X through libesmi.so (-m gpu); a completeness test ties the table to csrc/train_ops.h, so a
kernel added without a row fails here."""
import functools
import importlib
import os
import re

import pytest

from tests import train_variant_checks as K
from tests.simlib import ROOT, launched_kernels, use_sim

IDS = [r.id for r in K.ROWS]


@functools.lru_cache(maxsize=None)
def simulated_row(row_id):
    """One row on the simulator, run once and shared with the completeness test -> the names of the kernels it launched."""
    with use_sim():
        with launched_kernels() as names:
            K.run_row("cpu", K.BY_ID[row_id])
    return tuple(names)


@pytest.mark.parametrize("row_id", IDS)
def test_simulated_variant_matches_float64(row_id):
    row, names = K.BY_ID[row_id], set(simulated_row(row_id))
    print(f"    launched: {sorted(names)}")
    assert set(row.must) <= names, (row_id, "not launched", sorted(set(row.must) - names))
    assert not set(row.absent) & names, (row_id, "launched, but the row is about its alternative", sorted(set(row.absent) & names))


@pytest.mark.gpu
@pytest.mark.parametrize("row_id", IDS)
def test_gpu_variant_matches_float64(row_id):
    K.run_row("cuda", K.BY_ID[row_id])


# ------------------------------------------------------------------------------------------------------------------ self-check
@pytest.mark.parametrize("row_id,what,message", [("ln_70x50", "dgamma", "'dgamma'"), ("conv_cin32_cout32_k7_s1_g32_n21_pipe", "wgrad", "'wgrad'"),
                                                 ("attn_B1_N30_C640_h1", "dqkv", "'dqkv'"), ("reduce_batch", "item 17", "'reduce_batch', 17,")])
def test_variant_check_catches_a_perturbed_gradient(row_id, what, message):
    """The bounds are tight enough to see a kernel that is wrong by 1e-3 of one tensor's scale in one element: the row fails, and its
    message names the tensor."""
    def perturb(name, t):
        if name == what:
            t.view(-1)[t.numel() // 3] += 1e-3 * float(t.abs().max())
        return t
    with use_sim():
        with pytest.raises(AssertionError, match=message):
            K.run_row("cpu", K.BY_ID[row_id], perturb=perturb)


# ---------------------------------------------------------------------------------------------------------------- completeness
def kernels_of_train_ops():
    """The `__global__` kernels of the family headers csrc/train_ops.h includes (its `#include "train_*.h"` lines are the list), templates
    as the instantiations tu_train.hip launches."""
    csrc = os.path.join(ROOT, "efficientspeech_amd", "csrc")
    headers = re.findall(r'^#include "(train_\w+\.h)"', open(os.path.join(csrc, "train_ops.h")).read(), re.M)
    src = "".join(open(os.path.join(csrc, h)).read() for h in headers)
    found = re.findall(r"__global__\s+(?:__launch_bounds__\([^)]*\)\s+)?void\s+(\w+)\s*\(", src)
    assert len(found) == len(set(found)) >= 40 and set(K.INSTANTIATIONS) <= set(found)
    out = []
    for name in found:
        out += [f"{name}<{a}>" for a in K.INSTANTIATIONS[name]] if name in K.INSTANTIATIONS else [name]
    return out


def _test_exists(test_id):
    path, _, rest = test_id.partition("::")
    name, _, param = rest.partition("[")
    if not os.path.exists(os.path.join(ROOT, path)):
        return False
    fn = getattr(importlib.import_module(path[:-3].replace("/", ".")), name, None)
    if fn is None or not param:
        return fn is not None
    ids = []
    for mark in getattr(fn, "pytestmark", []):
        if mark.name == "parametrize":
            ids += [str(i) for i in (mark.kwargs.get("ids") or mark.args[1])]
    return param[:-1] in ids


def uncovered_kernels(rows):
    launched = set()
    for r in rows:
        launched |= set(simulated_row(r.id))
    return [k for k in kernels_of_train_ops() if k not in launched and k not in K.COVERED_ELSEWHERE], launched


def test_every_training_kernel_has_a_row_or_a_named_test():
    missing, launched = uncovered_kernels(K.ROWS)
    assert not missing, ("kernels of csrc/train_ops.h that no row of tests/train_variant_checks.py launches and COVERED_ELSEWHERE does not "
                         "name a test for", missing)
    for kernel, test_id in K.COVERED_ELSEWHERE.items():
        assert kernel in kernels_of_train_ops(), (kernel, "is no kernel of train_ops.h")
        assert kernel not in launched, (kernel, "is reached by the table: the table counts, take it out of COVERED_ELSEWHERE")
        assert _test_exists(test_id), (kernel, test_id, "no such test")


def test_completeness_notices_a_removed_row():
    """Without the global-memory attention rows the completeness check names both kernels of the pair."""
    rows = [r for r in K.ROWS if "train_attn_fwd_kernel" not in r.must]
    assert len(rows) == len(K.ROWS) - 3
    missing, _ = uncovered_kernels(rows)
    assert missing == ["train_attn_fwd_kernel", "train_attn_bwd_rows_kernel"]
