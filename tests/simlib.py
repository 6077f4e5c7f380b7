"""Test helper: build + bind the CPU wave-simulator build of the kernel sources (tools/wavesim).

Only tests use this.  `use_sim()` temporarily swaps the library handle inside
efficientspeech_amd._lib so the very same host-side modules drive the simulated kernels on
host tensors; the product never does this (it loads libesmi.so or raises).
"""
import contextlib
import ctypes
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIM_SO = os.path.join(ROOT, "tools", "wavesim", "_build", "libesmi_sim.so")
_CSRC = os.path.join(ROOT, "efficientspeech_amd", "csrc")
_SRCS = [os.path.join(_CSRC, f) for f in os.listdir(_CSRC) if f.endswith((".hip", ".h"))] + \
        [os.path.join(ROOT, "tools", "wavesim", f) for f in ("wavesim.h", "wavesim.cpp")] + \
        [os.path.join(ROOT, "include", "esmi.h")]
_handle = None


def sim_lib():
    global _handle
    if _handle is None:
        stale = not os.path.exists(SIM_SO) or any(os.path.getmtime(s) > os.path.getmtime(SIM_SO) for s in _SRCS)
        if stale:
            subprocess.check_call([os.path.join(ROOT, "tools", "wavesim", "build.sh")], stdout=subprocess.DEVNULL)
        from efficientspeech_amd import _lib
        _handle = _lib.bind(ctypes.CDLL(SIM_SO))
        assert _handle.esmi_backend() == b"wavesim"
        _handle.wavesim_launch_log.restype = ctypes.c_char_p
    return _handle


def _sim_runtime(t):
    """Stand-in for efficientspeech_amd.networks._runtime while the simulator is bound: host tensors only, no stream."""
    if t.is_cuda:
        raise RuntimeError("wave-simulator backend only accepts host tensors")
    return sim_lib(), None


@contextlib.contextmanager
def use_sim():
    from efficientspeech_amd import _lib, networks
    old_lib, old_rt = _lib._LIB, networks._runtime
    _lib._LIB, networks._runtime = sim_lib(), _sim_runtime
    try:
        yield _lib._LIB
    finally:
        _lib._LIB, networks._runtime = old_lib, old_rt


@contextlib.contextmanager
def launch_records():
    """The launches the simulator makes inside the block, in order, as `(name, "gx,gy,gz|bx,by,bz|lds")`: the list is filled when the
    block exits.  Names are the launch sites' spelling without the outer parentheses and blanks, e.g. `enc_va64_kernel<2>`; the
    second field is the grid, the block and the dynamic LDS bytes of that launch."""
    lib = sim_lib()
    lib.wavesim_launch_log_clear()
    records = []
    try:
        yield records
    finally:
        for rec in lib.wavesim_launch_log().decode().splitlines():
            name, *num = rec.rsplit(" ", 7)                    # (grid, block and LDS bytes follow the name)
            name = name.replace(" ", "")
            records.append((name[1:-1] if name.startswith("(") else name,
                            f"{','.join(num[0:3])}|{','.join(num[3:6])}|{num[6]}"))
        lib.wavesim_launch_log_clear()


@contextlib.contextmanager
def launched_kernels():
    """launch_records() without the numbers: the kernels' names alone."""
    names, records = [], []
    try:
        with launch_records() as records:
            yield names
    finally:
        names.extend(name for name, _ in records)
