"""TEST INFRASTRUCTURE -- ctypes wrapper of libcadnip_probe.so (cadnip.jl_amd/csrc/probe/prim_probe.hip): the device-side helpers of
tran_ctrl.hpp, devices.hpp and va_runtime.hpp behind trivial kernels.

Every entry takes rows of doubles / ints ([rows][n]) and a shared table, and returns rows.  n is padded here to a multiple of the
workgroup size (the kernels have no tail guard: the cross-lane helpers need whole waves) and the padding is cut off again.
One entry has a shape of its own: ``run_tran_ctrl`` calls the transient controller (prepare_step or tran_update_body) once per instance
on states of the caller's choosing and returns everything the call may have written, guards included.
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


# ---- the transient controller, one call on a given state (prim_probe.hip: probe_tran_ctrl) ----------------------------------------------------
TC_POLICIES = {"g64": 0, "g256": 1, "fixed": 2}          # GlobalVecsT<64>, GlobalVecsT<256>, the fixed form over GlobalVecsT<64>
TC_NT = {"g64": 64, "g256": 256, "fixed": 64}
TC_DS = ("t", "h", "hprev", "hpp", "tcur", "gamma", "mn_a0f", "mn_ss", "mn_dnp", "hp3", "dsc", "p_t", "p_h", "p_hprev", "p_hpp")
TC_IS = ("nhist", "order", "k", "status", "bp_idx", "save_idx", "flags", "mn_flags", "active", "p_nhist")
TC_VEC = ("u", "du", "delta", "limit_w", "u0", "u1", "u2", "u3", "up", "beta")
TC_ISC = ("n_limits", "n_break", "n_save", "n_obs", "n_err", "max_newton", "max_order", "use_pcnr", "newton_mode", "step_rule")
TC_DSC = ("t0", "t1", "reltol", "h0", "hmin", "hmax", "newton_tol")
TC_GUARD = 64
# the guard words behind every instance's n: a quiet NaN with a payload no computation produces
TC_GUARD_BITS = np.uint64(0x7FF8DEADBEEF0001)
_L = C.POINTER(C.c_int64)


def run_tran_ctrl(policy, op, shared, states, vecs):
    """One launch of the controller probe: ``op`` 0 = prepare_step, 1 = tran_update_body, B = len(states) instances.

    shared: dict with TC_ISC / TC_DSC scalars (n_break / n_save / n_obs are taken from the arrays) and the arrays atol, emask [n],
            breaks, save_t, obs.
    states: list of dicts with the TC_DS / TC_IS names (``active`` need not be given: it is an output) and ``cnt`` (4 ints).
    vecs:   dict name -> [B, n] for the TC_VEC names.
    Returns a dict: every TC_DS / TC_IS name -> [B], cnt [B, 4], every TC_VEC name -> [B, n], out [B, n_save, n_obs], nactive (int),
    and the guards for the caller to check: ``vec_guard`` ([10, B, 64] as uint64 bit patterns, must all equal TC_GUARD_BITS),
    ``out_guard`` ([64] uint64, must be all ones), ``active_in`` (the sentinel -1 ``active`` carried in)."""
    atol = np.ascontiguousarray(shared["atol"], dtype=np.float64)
    emask = np.ascontiguousarray(shared["emask"], dtype=np.float64)
    n, B = atol.size, len(states)
    assert emask.size == n and B > 0
    breaks = np.ascontiguousarray(shared.get("breaks", ()), dtype=np.float64).ravel()
    save_t = np.ascontiguousarray(shared.get("save_t", ()), dtype=np.float64).ravel()
    obs = np.ascontiguousarray(shared.get("obs", ()), dtype=np.int32).ravel()
    sizes = {"n_break": breaks.size, "n_save": save_t.size, "n_obs": obs.size}
    isc = np.array([sizes[k] if k in sizes else int(shared[k]) for k in TC_ISC], dtype=np.int32)
    dsc = np.array([float(shared[k]) for k in TC_DSC], dtype=np.float64)
    ds = np.array([[float(s[k]) for k in TC_DS] for s in states], dtype=np.float64)
    is_ = np.array([[-1 if k == "active" else int(s[k]) for k in TC_IS] for s in states], dtype=np.int32)
    cnt = np.array([[int(c) for c in s["cnt"]] for s in states], dtype=np.int64).reshape(B, 4)
    stride = n + TC_GUARD
    vec = np.empty((len(TC_VEC), B, stride), dtype=np.float64)
    vec.view(np.uint64)[...] = TC_GUARD_BITS
    for k, name in enumerate(TC_VEC):
        v = np.asarray(vecs[name], dtype=np.float64)
        assert v.shape == (B, n), (name, v.shape)
        vec[k, :, :n] = v
    nout = B * save_t.size * obs.size
    out = np.zeros(nout + TC_GUARD, dtype=np.float64)
    nactive = np.zeros(1, dtype=np.int32)
    pad = lambda x, dt: x if x.size else np.zeros(1, dtype=dt)
    breaks_p, save_p, obs_p = pad(breaks, np.float64), pad(save_t, np.float64), pad(obs, np.int32)
    fn = load().probe_tran_ctrl
    fn.restype = C.c_int
    rc = fn(C.c_int(TC_POLICIES[policy]), C.c_int(op), C.c_int(B), C.c_int(n), C.c_int(stride), isc.ctypes.data_as(_I), dsc.ctypes.data_as(_D),
            ds.ctypes.data_as(_D), is_.ctypes.data_as(_I), cnt.ctypes.data_as(_L), vec.ctypes.data_as(_D), atol.ctypes.data_as(_D),
            emask.ctypes.data_as(_D), breaks_p.ctypes.data_as(_D), save_p.ctypes.data_as(_D), obs_p.ctypes.data_as(_I), out.ctypes.data_as(_D),
            nactive.ctypes.data_as(_I))
    if rc > 0:
        # a HIP error (a fault included) ends the session: nothing more may be started on a GPU that has just faulted
        import pytest
        pytest.exit("probe_tran_ctrl: HIP error %d" % rc, returncode=3)
    if rc != 0:
        raise RuntimeError("probe_tran_ctrl refused its arguments")
    res = {name: ds[:, k].copy() for k, name in enumerate(TC_DS)}
    res.update({name: is_[:, k].copy() for k, name in enumerate(TC_IS)})
    res["cnt"] = cnt
    res.update({name: vec[k, :, :n].copy() for k, name in enumerate(TC_VEC)})
    res["vec_guard"] = vec[:, :, n:].copy().view(np.uint64)
    res["out"] = out[:nout].reshape(B, save_t.size, obs.size).copy()
    res["out_guard"] = out[nout:].copy().view(np.uint64)
    res["nactive"] = int(nactive[0])
    return res
