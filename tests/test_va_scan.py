"""The length regulator's scan as the kernels that end a Fuse + variance-adaptor call run it (csrc/va_decide.h wg_scan_durations in
enc_va16; the same scan spelled out in enc_fuse_va, enc_va64 and enc_pred128; length_regulate_kernel behind va_tail), through
esmi_fuse_variance_adaptor_f32 with forced durations drawn from {-2, 0, 1, 7}, B = 2 ragged, at the T where the scan can go wrong:
the positions per lane ceil(T / 64) changing (64 | 65, 128 | 129), lanes that hold no position (T = 1, 31), a last lane that holds
fewer than the others (63, 65, 127, 129, 255) and the kernels' T limits (128, 256).

`cum` lives inside a larger int32 buffer filled with a sentinel.  Every workgroup walks 64 * ceil(T / 64) positions whatever its
utterance's length, and a store at a position >= T is dropped by the buffer resource's range check alone; were it not, the last
utterance's workgroup would write the words behind its row -- the sentinel (the first utterance's would write the second's row, which
the comparison with numpy sees unless the right value lands later).

The encoder's feature maps are random tensors of the right shapes: the scan sees only the forced durations and the mask, and a
simulated encoder block costs more than everything checked here."""
import ctypes as C

import numpy as np
import pytest
import torch

from efficientspeech_amd import networks
from tests import helpers as H
from tests.simlib import launched_kernels, use_sim

DEV = "cuda:0"
SENTINEL, PAD = -123456789, 256
# (config, plan) -> the kernel that scans, the simulated T, the T the device adds
CASES = {("tiny", 63): ("enc_va16_kernel", (1, 63, 65), (127, 128)),
         ("tiny", 31): ("enc_fuse_va_kernel", (31, 65), (128,)),
         ("small", 63): ("enc_va64_kernel", (65,), (129, 255, 256)),
         ("base", 63): ("enc_pred128_kernel", (65,), (129, 255, 256)),
         ("tiny", 0): ("length_regulate_kernel", (65,), ())}
SIM = [(n, p, T) for (n, p), (_, ts, _) in CASES.items() for T in ts]
GPU = [(n, p, T) for (n, p), (_, ts, more) in CASES.items() for T in ts + more]
_nets = {}


@pytest.fixture(scope="module", autouse=True)
def shared_nets():
    yield
    _nets.clear()


def run_scan(name, plan, T, device):
    """one esmi_fuse_variance_adaptor_f32 call -> (dur, cum, mel_len, the guard words before and behind cum) as numpy"""
    if (name, device) not in _nets:
        _nets[name, device] = H.make_net(name, device, 1234)
    net, cfg, _ = _nets[name, device]
    pe, B, dim = net.encoder, 2, cfg.dim
    lens = (T, max(1, T // 2 - 1))
    g = torch.Generator().manual_seed(1000 * T + plan)
    forced = torch.tensor([-2, 0, 1, 7], dtype=torch.int32)[torch.randint(0, 4, (B, T), generator=g)].to(device)
    mask = (torch.arange(T)[None, :] >= torch.tensor(lens)[:, None]).to(torch.uint8).to(device)
    depth = len(pe.encoder.dim_outs)
    feats = [(0.5 * torch.randn((B, pe.encoder.block_len(T, i), c), generator=g)).to(device) for i, c in enumerate(pe.encoder.dim_outs)]
    p = lambda t: t.data_ptr()                                              # noqa: E731
    with torch.no_grad(), networks._on_device_of(net.decoder.mel_linear.weight):
        lib, stream = networks._runtime(net.decoder.mel_linear.weight)
        fw, _kf = pe.fuse._packed(lib, stream)
        (pw, _k0), (ew, _k1), (dw, _k2) = pe._predictors(lib, stream)
        feat = torch.empty((B, T, 4 * dim), dtype=torch.float32, device=device)
        preds = torch.empty((3, B, T), dtype=torch.float32, device=device)
        idx = torch.empty((2, B, T), dtype=torch.int32, device=device)
        dur = torch.empty((B, T), dtype=torch.int32, device=device)
        guarded = torch.full((PAD + B * T + PAD,), SENTINEL, dtype=torch.int32, device=device)
        cum = guarded[PAD:PAD + B * T]
        mel_len = torch.empty((B,), dtype=torch.int32, device=device)
        ws = torch.empty(lib.esmi_fuse_variance_adaptor_workspace_bytes(B, T, dim, depth), dtype=torch.uint8, device=device)
        fp = (C.c_void_p * depth)(*[p(f) for f in feats])
        ni = (C.c_int * depth)(*[f.shape[1] for f in feats])
        lib.esmi_fuse_variance_adaptor_f32(C.byref(fw), depth, dim, pe.fuse.kernel_size, B, T, fp, ni, C.byref(pw), C.byref(ew), C.byref(dw),
                                           p(mask), None, None, p(forced), p(feat), p(preds[0]), p(preds[1]), p(preds[2]), p(idx[0]),
                                           p(idx[1]), p(dur), p(cum), p(mel_len), None, None, plan, p(ws), ws.numel(), stream)
        if device != "cpu":
            torch.cuda.synchronize()
    n = lambda t: t.cpu().numpy()                                           # noqa: E731
    return n(dur), n(cum).reshape(B, T), n(mel_len), n(guarded[:PAD]), n(guarded[PAD + B * T:]), n(forced), lens


def check_scan(name, plan, T, device):
    dur, cum, mel_len, before, behind, forced, lens = run_scan(name, plan, T, device)
    for b, n in enumerate(lens):                                             # (the durations the scan sums really are the forced ones)
        assert np.array_equal(dur[b, :n], np.maximum(forced[b, :n], 0)) and not dur[b, n:].any(), b
        assert np.array_equal(cum[b], np.cumsum(np.maximum(dur[b], 0))), (b, np.argwhere(cum[b] != np.cumsum(np.maximum(dur[b], 0)))[:4].tolist())
    assert np.array_equal(mel_len, cum[:, -1])
    assert (behind == SENTINEL).all(), np.argwhere(behind != SENTINEL)[:4].tolist()
    assert (before == SENTINEL).all(), np.argwhere(before != SENTINEL)[:4].tolist()


@pytest.mark.parametrize("name,plan,T", SIM, ids=[f"{n}-{p}-T{T}" for n, p, T in SIM])
def test_simulated_scan(name, plan, T):
    with use_sim(), launched_kernels() as seen:
        check_scan(name, plan, T, "cpu")
    kernels = {k.split("<")[0] for k in seen}
    assert CASES[name, plan][0] in kernels, sorted(kernels)
    if plan:                                                                 # (the fused kernels scan themselves: no scan launch behind them)
        assert "length_regulate_kernel" not in kernels, sorted(kernels)


@pytest.mark.gpu
@pytest.mark.parametrize("name,plan,T", GPU, ids=[f"{n}-{p}-T{T}" for n, p, T in GPU])
def test_scan_on_the_device(name, plan, T):
    """(which kernel serves a shape is the host's decision, the same code in both builds: tests/test_dispatch.py pins it)"""
    check_scan(name, plan, T, DEV)
