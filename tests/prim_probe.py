"""TEST INFRASTRUCTURE -- ctypes wrapper of libcadnip_probe.so (cadnip.jl_amd/csrc/probe/prim_probe.hip): the device-side helpers of
tran_ctrl.hpp, devices.hpp and va_runtime.hpp behind trivial kernels.

Every entry takes rows of doubles / ints ([rows][n]) and a shared table, and returns rows.  n is padded here to a multiple of the
workgroup size (the kernels have no tail guard: the cross-lane helpers need whole waves) and the padding is cut off again.
CADNIP_PROBE_LIB overrides the library path."""
import ctypes as C
import os

import numpy as np

from cadnip_jl_amd import hip

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("CADNIP_PROBE_LIB") or os.path.join(os.path.dirname(_HERE), "cadnip.jl_amd", "libcadnip_probe.so")

# entry -> rows of (in, out, iin, iout); the library checks them against its own before it launches
SHAPES = {
    "fast_div": (2, 1, 0, 0), "step_root": (1, 1, 1, 0),
    "lane_sums": (1, 10, 0, 0), "readlane": (1, 64, 0, 0), "ddx_tl": (1, 49, 0, 0), "grp": (2, 3, 2, 2),
    "dual_ops1": (4, 26, 0, 0), "dual_ops3": (8, 52, 0, 0),
    "va_unary1": (2, 3, 2, 0), "va_unary3": (4, 5, 2, 0), "va_binary1": (4, 2, 2, 0), "va_binary3": (8, 4, 2, 0),
    "limiters": (4, 4, 0, 0), "pwl": (1, 1, 3, 1), "pulse": (8, 1, 0, 0), "sind": (1, 1, 0, 0),
    "source_value": (3, 1, 5, 1), "bsrc": (2, 1, 3, 0),
}
_D = C.POINTER(C.c_double)
_I = C.POINTER(C.c_int32)
_lib = None


def load():
    """dlopen the probe library after the product's own (hip.load_library): one HIP runtime per process."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError("probe library %s is missing: run build()" % LIB_PATH)
        hip.load_library()
        _lib = C.CDLL(LIB_PATH)
    return _lib


def run(name, din=(), iin=(), tab=(), block=64, pad=1.0, ipad=0):
    """Call probe_<name>.  ``din`` / ``iin``: the input rows (sequences of equal length n).  Returns (out [nout, n], iout [niout, n])."""
    nin, nout, niin, niout = SHAPES[name]
    din = [np.asarray(r, dtype=np.float64).ravel() for r in din]
    iin = [np.asarray(r, dtype=np.int32).ravel() for r in iin]
    assert len(din) == nin and len(iin) == niin, (name, len(din), len(iin))
    n = (din[0] if din else iin[0]).size
    assert n > 0 and all(r.size == n for r in din + iin)
    npad = -(-n // block) * block
    a = np.full((max(nin, 1), npad), pad, dtype=np.float64)
    b = np.full((max(niin, 1), npad), ipad, dtype=np.int32)
    for k, r in enumerate(din):
        a[k, :n] = r
    for k, r in enumerate(iin):
        b[k, :n] = r
    out = np.zeros((max(nout, 1), npad), dtype=np.float64)
    iout = np.zeros((max(niout, 1), npad), dtype=np.int32)
    t = np.ascontiguousarray(tab, dtype=np.float64).ravel()
    tt = t if t.size else np.zeros(1)
    rc = getattr(load(), "probe_" + name)(C.c_int(npad), C.c_int(block), nin, nout, niin, niout, a.ctypes.data_as(_D), out.ctypes.data_as(_D),
                                          b.ctypes.data_as(_I), iout.ctypes.data_as(_I), tt.ctypes.data_as(_D), C.c_int(t.size))
    if rc > 0:
        # a HIP error (a fault included) ends the session: nothing more may be started on a GPU that has just faulted
        import pytest
        pytest.exit("probe_%s: HIP error %d" % (name, rc), returncode=3)
    if rc != 0:
        raise RuntimeError("probe_%s refused its arguments" % name)
    return out[:nout, :n], iout[:niout, :n]
