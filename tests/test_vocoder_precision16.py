"""The HiFi-GAN generator at precision 16: esmi_hifigan_generator_prec_f32, Generator(h, precision) / Generator.forward(..., precision),
get_hifigan(..., precision), EfficientSpeech.synthesize(..., precision).  The checks, the operand rule `R16` and the fp64 yardstick live
in tests/precision_checks.py, which tests/test_inference_bf16.py runs with the bf16 rule.  A test marked `gpu` gets the device from the
`device` fixture, the others "cpu" with the wave simulator bound (the same kernel sources compiled for the host).

To re-record the launch table after an intended change of the launches: `python -m tests.test_vocoder_precision16` prints it.
"""
import os
import re
import shutil
import subprocess
import sys
import textwrap

import pytest

from tests import precision_checks as V
from tests.precision_checks import R16, device, yard   # noqa: F401 (fixtures)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "efficientspeech_amd", "libesmi.so")
TOOLS = ["/opt/rocm/lib/llvm/bin/clang-offload-bundler", "/opt/rocm/lib/llvm/bin/llvm-readelf"]


@pytest.mark.parametrize("config", ["v1", "v2", "v3"])
def test_fp64_mirror_matches_the_reference_fixtures(config, yard):
    """the yardstick's exact mode against the committed reference waveforms: < 2e-6 L-inf"""
    V.check_mirror_matches_fixture(yard, R16, config)


# ---------------------------------------------------------------------------------------------------------------- GPU tier
@pytest.mark.gpu
@pytest.mark.parametrize("fused", [True, False], ids=["fused", "convs"])
@pytest.mark.parametrize("config", ["v1", "v2", "v3"])
def test_precision16_error_is_the_binary16_operand_error(config, fused, yard, device):
    """the three fixture shapes.  v2 covers all twelve (C, K) one-product ResBlock1 instantiations; v3 ResBlock2 with n_conv = 2 and its
    k = 5 blocks conv by conv; v1 the 256- / 128-channel stages on convgemm_dma_kernel<..., true, ...>."""
    V.check_vocoder_accuracy(yard, R16, config, device, fused)


@pytest.mark.gpu
def test_precision16_ragged_keeps_its_contract(device):
    """v2, B = 4, L = 64, lengths [64, 33, 9, 0], one launch per ResBlock and conv by conv"""
    V.check_ragged_contract(R16, "v2", 4, 64, [64, 33, 9, 0], device)


@pytest.mark.gpu
def test_precision_0_and_32_are_the_existing_entry_points(device):
    """v2, B = 2, L = 24 (two windows in the first stage of the default path), lengths [24, 5]"""
    V.check_default_untouched(R16, "v2", 2, 24, [24, 5], device)


@pytest.mark.gpu
def test_precision16_through_synthesize_and_the_scheduler(device):
    V.check_vocoder_wrappers(device)


# ---------------------------------------------------------------------------------------------------------------- CPU tier (simulator)
def test_simulated_precision16_accuracy_v2_two_windows(yard, device):
    """v2 with one launch per ResBlock at B = 1, L = 50: the one-product kernels take windows of up to 512 rows at every channel count
    (16 waves at C = 64), so the first stage's k = 11 block (halo 60) has TL = 392 output rows per window and 8 L = 400 positions are
    the smallest length with two windows per utterance there."""
    V.check_vocoder_accuracy(yard, R16, "v2", device, True, 1, 50)


def test_simulated_precision16_accuracy_reduced_generator_conv_by_conv(yard, device):
    """the reduced generator of tests/test_vocoder_dispatch.py one launch per convolution, B = 2, L = 6"""
    V.check_vocoder_accuracy(yard, R16, "reduced1", device, False, 2, 6)


def test_simulated_precision16_ragged_keeps_its_contract(device):
    """the reduced generator, lengths [6, 2], both modes (the C call alone: the module's forward is in the accuracy tests)"""
    V.check_ragged_contract(R16, "reduced1", 2, 6, [6, 2], device, module=False)


def test_simulated_precision_0_and_32_are_the_existing_entry_points(device):
    """a small generator (32 -> 16 / 8 channels; one launch per ResBlock), B = 2, L = 6, lengths [6, 2]"""
    V.check_default_untouched(R16, "small", 2, 6, [6, 2], device)


def test_precision_refusals(device):
    """ValueError from Python; ESMI_ERR_ARG from the C call for precision 8 and for a PCM plane without lengths, nothing launched"""
    V.check_vocoder_refusals(device)


# (ResBlock type, fuse_resblocks, length-aware) -> the launch records of the reduced generator at precision 16, in order
ROWS = {
    (1, True, False):
        "convgemm_kernel<1,true>[1,8,1|256,1,1|0] convgemm_kernel<1,true>[1,4,1|256,1,1|0] 4x "
        "convgemm_dma_kernel<4,1,NWV,true,false>[8,1,1|256,1,1|61440] "
        "convgemm_dma_kernel<4,1,NWV,true,false>[8,1,1|256,1,1|65536] 3x "
        "convgemm_dma_kernel<4,1,NWV,true,false>[8,1,1|256,1,1|61440] "
        "convgemm_dma_kernel<4,1,NWV,true,false>[8,1,1|256,1,1|57344] "
        "convgemm_dma_kernel<4,1,NWV,true,false>[8,1,1|256,1,1|61440] "
        "convgemm_dma_kernel<4,1,NWV,true,false>[8,1,1|256,1,1|57344] "
        "convgemm_dma_kernel<4,1,NWV,true,false>[8,1,1|256,1,1|61440] convgemm_kernel<1,true>[1,2,1|256,1,1|0] "
        "hifigan_resblock_amp_kernel<C,K>[2,1,1|1024,1,1|9216] hifigan_resblock_amp_kernel<C,K>[2,1,1|1024,1,1|18432] "
        "convgemm_kernel<1,true>[1,1,1|256,1,1|0] 2x hifigan_resblock_amp_kernel<C,K>[2,1,1|512,1,1|10240] "
        "conv_to1_kernel[1,1,1|256,1,1|0] ",
    (1, True, True):
        "convgemm_kernel<1,true>[1,8,1|256,1,1|0] convgemm_kernel<1,true>[1,4,1|256,1,1|0] 4x "
        "convgemm_dma_kernel<4,1,NWV,true,false>[8,1,1|256,1,1|61440] "
        "convgemm_dma_kernel<4,1,NWV,true,false>[8,1,1|256,1,1|65536] 3x "
        "convgemm_dma_kernel<4,1,NWV,true,false>[8,1,1|256,1,1|61440] "
        "convgemm_dma_kernel<4,1,NWV,true,false>[8,1,1|256,1,1|57344] "
        "convgemm_dma_kernel<4,1,NWV,true,false>[8,1,1|256,1,1|61440] "
        "convgemm_dma_kernel<4,1,NWV,true,false>[8,1,1|256,1,1|57344] "
        "convgemm_dma_kernel<4,1,NWV,true,false>[8,1,1|256,1,1|61440] convgemm_len_amp_kernel<2>[1,1,1|256,1,1|0] "
        "hifigan_resblock_amp_kernel<C,K>[2,1,1|1024,1,1|9216] hifigan_resblock_amp_kernel<C,K>[2,1,1|1024,1,1|18432] "
        "convgemm_len_amp_kernel<1>[1,1,1|256,1,1|0] 2x hifigan_resblock_amp_kernel<C,K>[2,1,1|512,1,1|10240] "
        "conv_to1_len_kernel[1,1,1|256,1,1|0] ",
    (1, False, True):
        "convgemm_kernel<1,true>[1,8,1|256,1,1|0] convgemm_kernel<1,true>[1,4,1|256,1,1|0] 4x "
        "convgemm_dma_kernel<4,1,NWV,true,false>[8,1,1|256,1,1|61440] "
        "convgemm_dma_kernel<4,1,NWV,true,false>[8,1,1|256,1,1|65536] 3x "
        "convgemm_dma_kernel<4,1,NWV,true,false>[8,1,1|256,1,1|61440] "
        "convgemm_dma_kernel<4,1,NWV,true,false>[8,1,1|256,1,1|57344] "
        "convgemm_dma_kernel<4,1,NWV,true,false>[8,1,1|256,1,1|61440] "
        "convgemm_dma_kernel<4,1,NWV,true,false>[8,1,1|256,1,1|57344] "
        "convgemm_dma_kernel<4,1,NWV,true,false>[8,1,1|256,1,1|61440] 13x convgemm_len_amp_kernel<2>[1,1,1|256,1,1|0] 13x "
        "convgemm_len_amp_kernel<1>[1,1,1|256,1,1|0] conv_to1_len_kernel[1,1,1|256,1,1|0] ",
    (2, True, True):
        "convgemm_kernel<1,true>[1,8,1|256,1,1|0] convgemm_kernel<1,true>[1,4,1|256,1,1|0] 3x "
        "convgemm_dma_kernel<4,1,NWV,true,false>[8,1,1|256,1,1|61440] "
        "convgemm_dma_kernel<4,1,NWV,true,false>[8,1,1|256,1,1|57344] convgemm_len_amp_kernel<2>[1,1,1|256,1,1|0] 2x "
        "hifigan_resblock_amp_kernel<C,K>[2,1,1|1024,1,1|9216] convgemm_len_amp_kernel<1>[1,1,1|256,1,1|0] "
        "hifigan_resblock_amp_kernel<C,K>[2,1,1|512,1,1|5120] hifigan_resblock_amp_kernel<C,K>[2,1,1|512,1,1|10240] "
        "conv_to1_len_kernel[1,1,1|256,1,1|0] ",
}


def _id(row):
    resblock, fused, ragged = row
    return f"resblock{resblock}-{'fused' if fused else 'convs'}-{'ragged' if ragged else 'plain'}"


@pytest.mark.parametrize("row", list(ROWS), ids=_id)
def test_precision16_launches(row):
    """Test 4: the complete launch records; and in every row every convgemm record is an amp instantiation, every one-launch ResBlock
    the one-product kernel, conv_post unchanged."""
    got = V.run_row(*row).split()
    assert got == ROWS[row].split()
    names = [g.split("[")[0] for g in got if "[" in g]
    for n in names:
        if n.startswith("convgemm_kernel"):
            assert re.fullmatch(r"convgemm_kernel<\d,true>", n), n
        elif n.startswith("convgemm_dma_kernel"):
            assert re.fullmatch(r"convgemm_dma_kernel<\d,\d,NWV,true,(true|false)>", n), n
        elif n.startswith("convgemm_len"):
            assert re.fullmatch(r"convgemm_len_amp_kernel<\d>", n), n
        elif "resblock" in n:
            assert n in ("hifigan_resblock_amp_kernel<C,K>", "hifigan_resblock16_amp_kernel<C,K>"), n
        else:
            assert n == ("conv_to1_len_kernel" if row[2] else "conv_to1_kernel"), n
    assert names[-1].startswith("conv_to1") and (any("resblock" in n for n in names) == row[1])


# ---------------------------------------------------------------------------------------------------------------- test 7 (CPU, the built library)
@pytest.mark.skipif(not os.path.exists(LIB) or not all(os.path.exists(t) for t in TOOLS) or shutil.which("objcopy") is None,
                    reason="needs the built libesmi.so and the ROCm LLVM tools")
def test_one_product_resblock_kernels_have_no_scratch():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), LIB, "--all"], capture_output=True, text=True, check=True).stdout
    rows = {m.group(1): int(m.group(2)) for m in re.finditer(r"^\| `(.+?)` \| [^|]+ \| (\d+) \|", out, re.M)}
    new = {k: v for k, v in rows.items() if re.search(r"^hifigan_resblock(16)?_amp_kernel<", k)}
    assert len(new) == 12, sorted(new)
    assert all(v == 0 for v in new.values()), {k: v for k, v in new.items() if v}
    old = [k for k in rows if re.search(r"^hifigan_resblock(16)?_kernel<", k)]
    assert len(old) == 12, sorted(old)
    assert any(k.startswith("convgemm_len_amp_kernel<") for k in rows) and any(k.startswith("convgemm_len_kernel<") for k in rows)


if __name__ == "__main__":
    os.environ.setdefault("WAVESIM_THREADS", "16")
    for row in [(1, True, False), (1, True, True), (1, False, True), (2, True, True)]:
        lines = textwrap.wrap(V.run_row(*row), 112, break_long_words=False, break_on_hyphens=False)
        print(f"    {row}:")
        print("\n".join(f'        "{ln} "' for ln in lines) + ",")
