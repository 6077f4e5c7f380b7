"""Which kernels the HiFi-GAN generator's host side launches, and with which grids (CPU, wave simulator): the vocoder's twin of
tests/test_dispatch.py.

The plain and the length-aware call, one launch per ResBlock and one per convolution, ResBlock1 and ResBlock2 all compute the same
waveform by design, so the parity tests pass whichever launches a call makes: a stage that lost its length limit or a ResBlock that
fell back to six launches shows up only as a slowdown.  Each row pins the complete launch records of one Generator.forward -- kernel
name, grid, block and dynamic LDS bytes, written `name[gx,gy,gz|bx,by,bz|lds]` and run-length (`5x ...`): the one-launch ResBlock is
logged as `hifigan_resblock_kernel<C,K>` whatever its instantiation, so only its LDS bytes and grid tell the instantiations apart.
Weight preparation (packing, range scans) is left out: it runs once per weight set, not per call.

The generator is a reduced one: three stages of rates (2, 2, 2) from 256 channels, so 128 channels (never limited), then 64 and 32
(limited in a length-aware call); two ResBlocks per stage (k = 3 and 7); 16 mel channels; B = 2, L = 6, lengths [6, 2].  Both stage
classes occur, and so do convgemm_len_kernel<2> and <1>.  Measured: 9 rows, 1 to 5 s each, 32 s for the module on 8 cores.

To re-record after an intended change of the launches: `python -m tests.test_vocoder_dispatch` prints the table.
"""
import ctypes
import os
import textwrap

import pytest
import torch

from efficientspeech_amd import _lib
from efficientspeech_amd.hifigan import Generator, HifiGanConfig, synth_hifigan_state_dict
from tests.simlib import launch_records, use_sim

_PREP = ("pack_", "absmax_kernel")
B, L, LENGTHS = 2, 6, [6, 2]

# (ResBlock type, fuse_resblocks, length-aware, pcm16) -> the launch records, in order
ROWS = {
    (1, True, False, False):
        "convgemm_kernel<1,false>[1,8,1|256,1,1|0] convgemm_kernel<1,false>[1,4,1|256,1,1|0] 4x "
        "convgemm_dma_kernel<4,1,NWV,false,false>[8,1,1|256,1,1|61440] "
        "convgemm_dma_kernel<4,1,NWV,false,false>[8,1,1|256,1,1|65536] 3x "
        "convgemm_dma_kernel<4,1,NWV,false,false>[8,1,1|256,1,1|61440] "
        "convgemm_dma_kernel<4,1,NWV,false,false>[8,1,1|256,1,1|57344] "
        "convgemm_dma_kernel<4,1,NWV,false,false>[8,1,1|256,1,1|61440] "
        "convgemm_dma_kernel<4,1,NWV,false,false>[8,1,1|256,1,1|57344] "
        "convgemm_dma_kernel<4,1,NWV,false,false>[8,1,1|256,1,1|61440] convgemm_kernel<1,false>[1,2,1|256,1,1|0] "
        "hifigan_resblock_kernel<C,K>[2,1,1|512,1,1|18432] hifigan_resblock_kernel<C,K>[2,1,1|512,1,1|36864] "
        "convgemm_kernel<1,false>[1,1,1|256,1,1|0] 2x hifigan_resblock_kernel<C,K>[2,1,1|512,1,1|20480] "
        "conv_to1_kernel[1,1,1|256,1,1|0] ",
    (1, True, True, False):
        "convgemm_kernel<1,false>[1,8,1|256,1,1|0] convgemm_kernel<1,false>[1,4,1|256,1,1|0] 4x "
        "convgemm_dma_kernel<4,1,NWV,false,false>[8,1,1|256,1,1|61440] "
        "convgemm_dma_kernel<4,1,NWV,false,false>[8,1,1|256,1,1|65536] 3x "
        "convgemm_dma_kernel<4,1,NWV,false,false>[8,1,1|256,1,1|61440] "
        "convgemm_dma_kernel<4,1,NWV,false,false>[8,1,1|256,1,1|57344] "
        "convgemm_dma_kernel<4,1,NWV,false,false>[8,1,1|256,1,1|61440] "
        "convgemm_dma_kernel<4,1,NWV,false,false>[8,1,1|256,1,1|57344] "
        "convgemm_dma_kernel<4,1,NWV,false,false>[8,1,1|256,1,1|61440] convgemm_len_kernel<2>[1,1,1|256,1,1|0] "
        "hifigan_resblock_kernel<C,K>[2,1,1|512,1,1|18432] hifigan_resblock_kernel<C,K>[2,1,1|512,1,1|36864] "
        "convgemm_len_kernel<1>[1,1,1|256,1,1|0] 2x hifigan_resblock_kernel<C,K>[2,1,1|512,1,1|20480] "
        "conv_to1_len_kernel[1,1,1|256,1,1|0] ",
    (1, False, False, False):
        "convgemm_kernel<1,false>[1,8,1|256,1,1|0] convgemm_kernel<1,false>[1,4,1|256,1,1|0] 4x "
        "convgemm_dma_kernel<4,1,NWV,false,false>[8,1,1|256,1,1|61440] "
        "convgemm_dma_kernel<4,1,NWV,false,false>[8,1,1|256,1,1|65536] 3x "
        "convgemm_dma_kernel<4,1,NWV,false,false>[8,1,1|256,1,1|61440] "
        "convgemm_dma_kernel<4,1,NWV,false,false>[8,1,1|256,1,1|57344] "
        "convgemm_dma_kernel<4,1,NWV,false,false>[8,1,1|256,1,1|61440] "
        "convgemm_dma_kernel<4,1,NWV,false,false>[8,1,1|256,1,1|57344] "
        "convgemm_dma_kernel<4,1,NWV,false,false>[8,1,1|256,1,1|61440] 13x convgemm_kernel<1,false>[1,2,1|256,1,1|0] 13x "
        "convgemm_kernel<1,false>[1,1,1|256,1,1|0] conv_to1_kernel[1,1,1|256,1,1|0] ",
    (1, False, True, False):
        "convgemm_kernel<1,false>[1,8,1|256,1,1|0] convgemm_kernel<1,false>[1,4,1|256,1,1|0] 4x "
        "convgemm_dma_kernel<4,1,NWV,false,false>[8,1,1|256,1,1|61440] "
        "convgemm_dma_kernel<4,1,NWV,false,false>[8,1,1|256,1,1|65536] 3x "
        "convgemm_dma_kernel<4,1,NWV,false,false>[8,1,1|256,1,1|61440] "
        "convgemm_dma_kernel<4,1,NWV,false,false>[8,1,1|256,1,1|57344] "
        "convgemm_dma_kernel<4,1,NWV,false,false>[8,1,1|256,1,1|61440] "
        "convgemm_dma_kernel<4,1,NWV,false,false>[8,1,1|256,1,1|57344] "
        "convgemm_dma_kernel<4,1,NWV,false,false>[8,1,1|256,1,1|61440] 13x convgemm_len_kernel<2>[1,1,1|256,1,1|0] 13x "
        "convgemm_len_kernel<1>[1,1,1|256,1,1|0] conv_to1_len_kernel[1,1,1|256,1,1|0] ",
    (2, True, False, False):
        "convgemm_kernel<1,false>[1,8,1|256,1,1|0] convgemm_kernel<1,false>[1,4,1|256,1,1|0] 3x "
        "convgemm_dma_kernel<4,1,NWV,false,false>[8,1,1|256,1,1|61440] "
        "convgemm_dma_kernel<4,1,NWV,false,false>[8,1,1|256,1,1|57344] convgemm_kernel<1,false>[1,2,1|256,1,1|0] 2x "
        "hifigan_resblock_kernel<C,K>[2,1,1|512,1,1|18432] convgemm_kernel<1,false>[1,1,1|256,1,1|0] "
        "hifigan_resblock_kernel<C,K>[2,1,1|512,1,1|10240] hifigan_resblock_kernel<C,K>[2,1,1|512,1,1|20480] "
        "conv_to1_kernel[1,1,1|256,1,1|0] ",
    (2, True, True, False):
        "convgemm_kernel<1,false>[1,8,1|256,1,1|0] convgemm_kernel<1,false>[1,4,1|256,1,1|0] 3x "
        "convgemm_dma_kernel<4,1,NWV,false,false>[8,1,1|256,1,1|61440] "
        "convgemm_dma_kernel<4,1,NWV,false,false>[8,1,1|256,1,1|57344] convgemm_len_kernel<2>[1,1,1|256,1,1|0] 2x "
        "hifigan_resblock_kernel<C,K>[2,1,1|512,1,1|18432] convgemm_len_kernel<1>[1,1,1|256,1,1|0] "
        "hifigan_resblock_kernel<C,K>[2,1,1|512,1,1|10240] hifigan_resblock_kernel<C,K>[2,1,1|512,1,1|20480] "
        "conv_to1_len_kernel[1,1,1|256,1,1|0] ",
    (2, False, False, False):
        "convgemm_kernel<1,false>[1,8,1|256,1,1|0] convgemm_kernel<1,false>[1,4,1|256,1,1|0] 3x "
        "convgemm_dma_kernel<4,1,NWV,false,false>[8,1,1|256,1,1|61440] "
        "convgemm_dma_kernel<4,1,NWV,false,false>[8,1,1|256,1,1|57344] 5x convgemm_kernel<1,false>[1,2,1|256,1,1|0] 5x "
        "convgemm_kernel<1,false>[1,1,1|256,1,1|0] conv_to1_kernel[1,1,1|256,1,1|0] ",
    (2, False, True, False):
        "convgemm_kernel<1,false>[1,8,1|256,1,1|0] convgemm_kernel<1,false>[1,4,1|256,1,1|0] 3x "
        "convgemm_dma_kernel<4,1,NWV,false,false>[8,1,1|256,1,1|61440] "
        "convgemm_dma_kernel<4,1,NWV,false,false>[8,1,1|256,1,1|57344] 5x convgemm_len_kernel<2>[1,1,1|256,1,1|0] 5x "
        "convgemm_len_kernel<1>[1,1,1|256,1,1|0] conv_to1_len_kernel[1,1,1|256,1,1|0] ",
    (2, True, True, True):
        "convgemm_kernel<1,false>[1,8,1|256,1,1|0] convgemm_kernel<1,false>[1,4,1|256,1,1|0] 3x "
        "convgemm_dma_kernel<4,1,NWV,false,false>[8,1,1|256,1,1|61440] "
        "convgemm_dma_kernel<4,1,NWV,false,false>[8,1,1|256,1,1|57344] convgemm_len_kernel<2>[1,1,1|256,1,1|0] 2x "
        "hifigan_resblock_kernel<C,K>[2,1,1|512,1,1|18432] convgemm_len_kernel<1>[1,1,1|256,1,1|0] "
        "hifigan_resblock_kernel<C,K>[2,1,1|512,1,1|10240] hifigan_resblock_kernel<C,K>[2,1,1|512,1,1|20480] "
        "conv_to1_len_kernel[1,1,1|256,1,1|0] ",
}


def _config(resblock):
    return HifiGanConfig(resblock=str(resblock), upsample_rates=(2, 2, 2), upsample_kernel_sizes=(4, 4, 4), upsample_initial_channel=256,
                         resblock_kernel_sizes=(3, 7), resblock_dilation_sizes=((1, 3, 5),) * 2 if resblock == 1 else ((1, 3),) * 2,
                         num_mels=16)


def _vocoder(resblock, fused):
    h = _config(resblock)
    voc = Generator(h)
    voc.load_state_dict({k: torch.from_numpy(v) for k, v in synth_hifigan_state_dict(h, 1234).items()}, strict=True)
    voc.eval()
    voc.fuse_resblocks = fused
    mel = torch.randn((B, L, h.num_mels), generator=torch.Generator().manual_seed(5)) * 2 - 4
    return h, voc, mel


def run_row(resblock, fused, ragged, pcm16):
    """the launch records of one Generator.forward on the simulator (weight preparation left out), run-length encoded"""
    h, voc, mel = _vocoder(resblock, fused)
    lengths = torch.tensor(LENGTHS, dtype=torch.int32) if ragged else None
    with use_sim(), torch.no_grad(), launch_records() as records:
        wav = voc(mel.transpose(1, 2), lengths=lengths, pcm16=pcm16)
    assert wav.shape == (B, 1, L * h.hop) and wav.dtype == (torch.int16 if pcm16 else torch.float32)
    runs = []
    for name, dims in records:
        if name.startswith(_PREP):
            continue
        rec = f"{name}[{dims}]"
        if runs and runs[-1][0] == rec:
            runs[-1][1] += 1
        else:
            runs.append([rec, 1])
    return " ".join(r if k == 1 else f"{k}x {r}" for r, k in runs)


def _id(row):
    resblock, fused, ragged, pcm16 = row
    return f"resblock{resblock}-{'fused' if fused else 'convs'}-{'ragged' if ragged else 'plain'}" + ("-pcm16" if pcm16 else "")


@pytest.mark.parametrize("row", list(ROWS), ids=_id)
def test_vocoder_launches(row):
    assert run_row(*row).split() == ROWS[row].split()


def test_missing_weight_is_refused_before_the_first_launch():
    """conv_post's weight, the last one the call reads, NULL: ESMI_ERR_ARG, and nothing has been enqueued by then."""
    h, voc, mel = _vocoder(2, False)
    with use_sim() as lib, torch.no_grad():
        w, s, _keep = voc._packed(lib, None)
        w2 = _lib.HifiGanWeights()
        ctypes.pointer(w2)[0] = w
        w2.post_w = None
        nbytes = lib.esmi_hifigan_workspace_bytes(ctypes.byref(s), B, L)
        ws, wav = torch.empty(nbytes, dtype=torch.uint8), torch.empty((B, L * h.hop))
        with launch_records() as records:
            with pytest.raises(RuntimeError, match="esmi_hifigan_generator_f32"):
                lib.esmi_hifigan_generator_f32(ctypes.byref(w2), ctypes.byref(s), mel.data_ptr(), B, L, wav.data_ptr(), ws.data_ptr(), nbytes, None)
    assert records == []


if __name__ == "__main__":
    os.environ.setdefault("WAVESIM_THREADS", "16")
    rows = [(rb, fused, ragged, False) for rb in (1, 2) for fused in (True, False) for ragged in (False, True)] + [(2, True, True, True)]
    for row in rows:
        lines = textwrap.wrap(run_row(*row), 112, break_long_words=False, break_on_hyphens=False)
        print(f"    {row}:")
        print("\n".join(f'        "{ln} "' for ln in lines) + ",")
