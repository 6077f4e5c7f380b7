"""The older entry points of the inference C ABI -- esmi_phoneme2mel_forward_{f32, ctl_f32, prec_f32}, esmi_fuse_variance_adaptor_{f32,
ctl_f32}, esmi_variance_adaptor_{f32, ctl_f32} -- give, bit for bit, what the *_curve_f32 call that include/esmi.h names for each of
them gives.  The Python modules call the general forms only, so these tests are what runs the older ones.  The checks live in
tests/legacy_entry_points_checks.py; the CPU tier runs them through the wave simulator (the same sources compiled for the host), the GPU
tier on the device."""
import pytest

from tests import legacy_entry_points_checks as L
from tests import prosody_control_checks as P
from tests.simlib import launched_kernels, use_sim

DEV = "cuda:0"
DECIDES = {63: "enc_all16_kernel", 0: "va_tail_kernel"}      # the kernel that makes the one-call forward's decisions under each plan
_cases = {}


def case(device):
    if device not in _cases:
        _cases[device] = L.Case(device)
    return _cases[device]


@pytest.fixture(scope="module", autouse=True)
def shared_runs():
    yield
    _cases.clear()
    P.clear()


def test_scales_move_the_oracles_decisions():
    """the inputs' condition: without it "the ctl form equals the curve form" could hold on ignored scales"""
    L.check_scales_move_the_oracles_decisions()


# ---------------------------------------------------------------------------------------------------------------- CPU tier
@pytest.mark.parametrize("plan", L.PLANS)
def test_simulated_forward_forms_equal_the_general_one(plan):
    """_f32 == _curve_f32(NULL, 32); _ctl_f32 == _curve_f32 with the same (B,) pointers; _prec_f32 at 0 / 32 / 16 == _curve_f32 at that
    precision -- as one call and as stages 1 then 2, every output and tap"""
    with use_sim(), launched_kernels() as seen:
        case("cpu").check_forward(plan)
    assert DECIDES[plan] in {k.split("<")[0] for k in seen}


@pytest.mark.parametrize("plan", L.PLANS)
def test_simulated_stage_forms_equal_the_general_one(plan):
    """esmi_fuse_variance_adaptor_{f32, ctl_f32} and esmi_variance_adaptor_{f32, ctl_f32} against their _curve_f32 forms"""
    with use_sim(), launched_kernels() as seen:
        case("cpu").check_stages(plan)
    assert "va_tail_kernel" in seen                              # (esmi_variance_adaptor_*: one kernel per op under every plan)


# ---------------------------------------------------------------------------------------------------------------- GPU tier
@pytest.mark.gpu
@pytest.mark.parametrize("plan", L.PLANS)
def test_forward_forms_equal_the_general_one_on_the_device(plan):
    case(DEV).check_forward(plan)


@pytest.mark.gpu
@pytest.mark.parametrize("plan", L.PLANS)
def test_stage_forms_equal_the_general_one_on_the_device(plan):
    case(DEV).check_stages(plan)
