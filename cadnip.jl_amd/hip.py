"""ctypes binding of libcadnip_hip.so (include/cadnip_hip.h).

The library is the product; this module only marshals numpy arrays across the C ABI.  There
is no CPU fallback: if the extension is missing or no GPU is present, the calls fail loudly.
"""
import ctypes as C
import os

import numpy as np

from .structure import Structure, TYPE_ID, type_id

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("CADNIP_HIP_LIB") or os.path.join(_HERE, "libcadnip_hip.so")   # same override as julia/CadnipHIP.jl

OK, BADARG, SINGULAR, NONFINITE, HIPERROR, NOTREADY, NOCONV = range(7)
STATUS_NAMES = {0: "CADNIP_OK", 1: "CADNIP_BADARG", 2: "CADNIP_SINGULAR", 3: "CADNIP_NONFINITE",
                4: "CADNIP_HIPERROR", 5: "CADNIP_NOTREADY", 6: "CADNIP_NOCONV"}

# cadnip_ac_arnoldi's default breakdown tolerance: the geometric middle of the gap measured with the numpy port (tests/pz_ref.py,
# tests/test_pz_cpu.py) over the test circuits, the MOS linearisations included.  At a step where the dense pencil says the space has closed
# the norm ratio after / before orthogonalisation is at most 1.2e-14 (the eight-section ladder); at every other step it is at least 3.0e-3 (the
# inverter's MOS linearisations; the linear circuits: 4.5e-2).  The flip-flop has steps as low as 1.5e-9 that do not close its space and is
# not among the circuits the figure is taken from
AC_BREAKDOWN_TOL = 6e-9
AC_MEMORY = {"lds": 0, "hbm": 1, "auto": 2}     # CADNIP_AC_LDS / _HBM / _AUTO (Handle.ac_set_memory)

# every symbol declared in include/cadnip_hip.h
EXPORTS = [
    "cadnip_create", "cadnip_destroy", "cadnip_set_params", "cadnip_set_spec", "cadnip_set_initjct",
    "cadnip_rebuild", "cadnip_residual", "cadnip_jacobian", "cadnip_jacobian_dense", "cadnip_ode_rhs", "cadnip_ode_jacobian", "cadnip_get_GCb", "cadnip_get_contributions", "cadnip_analyze",
    "cadnip_analyze_values", "cadnip_factor", "cadnip_solve", "cadnip_factor_solve", "cadnip_lu_order", "cadnip_ac_solve", "cadnip_ac_adjoint", "cadnip_ac_solve_multi", "cadnip_ac_adjoint_multi", "cadnip_ac_sens", "cadnip_ac_arnoldi", "cadnip_ac_set_memory", "cadnip_ac_set_overlay", "cadnip_ac_plan_info", "cadnip_newton_step", "cadnip_newton_step_fused", "cadnip_debug_step_time", "cadnip_lu_stats", "cadnip_dc_run",
    "cadnip_dc_log_size", "cadnip_dc_log_get", "cadnip_tran_set_delay", "cadnip_tran_delay_info", "cadnip_tran_set_sens", "cadnip_tran_sens_init", "cadnip_tran_sens_get", "cadnip_tran_sens_info", "cadnip_tran_run", "cadnip_tran_state", "cadnip_dev_ptr", "cadnip_stream", "cadnip_set_u", "cadnip_get_u", "cadnip_get_flags",
    "cadnip_sync", "cadnip_debug_copy", "cadnip_debug_stamp_time", "cadnip_profile_enable", "cadnip_profile_read", "cadnip_version",
    "cadnip_host_lu_analyze", "cadnip_host_lu_analyze_leaves", "cadnip_host_lu_size", "cadnip_host_lu_blocks", "cadnip_host_lu_get", "cadnip_host_lu_free", "cadnip_host_lu_transpose",
    "cadnip_host_f2_build", "cadnip_host_f2_size", "cadnip_host_f2_get", "cadnip_host_f2_free", "cadnip_host_f2_team_steps", "cadnip_host_f2_steps",
]


class CadnipError(RuntimeError):
    def __init__(self, code, where):
        self.code = code
        super().__init__("%s returned %s" % (where, STATUS_NAMES.get(code, code)))


class SingularException(CadnipError):
    """Maps CADNIP_SINGULAR like the Julia shim maps it to LinearAlgebra.SingularException."""


class DeviceBlockC(C.Structure):
    _fields_ = [("type", C.c_int32), ("count", C.c_int32),
                ("n_nodes", C.c_int32), ("nodes", C.POINTER(C.c_int32)),
                ("n_ipar", C.c_int32), ("ipar", C.POINTER(C.c_int32)),
                ("n_par", C.c_int32),
                ("g_base", C.c_int32), ("c_base", C.c_int32), ("b_base", C.c_int32),
                ("n_g", C.c_int32), ("n_c", C.c_int32), ("n_b", C.c_int32)]


_I = C.POINTER(C.c_int32)
_D = C.POINTER(C.c_double)


class StructureC(C.Structure):
    _fields_ = [("n", C.c_int32), ("n_nodes", C.c_int32), ("n_currents", C.c_int32), ("n_charges", C.c_int32),
                ("n_limits", C.c_int32), ("nnz", C.c_int32), ("rowptr", _I), ("colidx", _I), ("to_ref_nz", _I),
                ("n_blocks", C.c_int32), ("blocks", C.POINTER(DeviceBlockC)),
                ("n_wave_data", C.c_int32), ("wave_data", _D),
                ("ns_g", C.c_int32), ("ns_c", C.c_int32), ("ns_b", C.c_int32),
                ("g_ptr", _I), ("g_slots", _I), ("c_ptr", _I), ("c_slots", _I), ("b_ptr", _I), ("b_slots", _I),
                ("diag_nz", _I), ("limit_init", _D)]


class SpecC(C.Structure):
    _fields_ = [("mode", C.c_int32), ("gmin", C.c_double), ("gshunt", C.c_double), ("srcFact", C.c_double)]


DC_COLD_ZERO = 2   # include/cadnip_hip.h: CADNIP_DC_COLD_ZERO


class DCOptsC(C.Structure):
    _fields_ = [("abstol", C.c_double), ("maxiters", C.c_int32), ("use_pcnr", C.c_int32), ("cold_start", C.c_int32),
                ("use_stepping", C.c_int32), ("fused", C.c_int32), ("participate", _I)]


class TranOptsC(C.Structure):
    _fields_ = [("t0", C.c_double), ("t1", C.c_double), ("reltol", C.c_double), ("abstol", _D), ("err_mask", _D), ("h0", C.c_double),
                ("hmin", C.c_double), ("hmax", C.c_double), ("max_newton", C.c_int32), ("max_order", C.c_int32),
                ("use_pcnr", C.c_int32), ("newton_tol", C.c_double), ("n_break", C.c_int32), ("breaks", _D),
                ("n_save", C.c_int32), ("save_t", _D), ("n_obs", C.c_int32), ("obs", _I),
                ("max_iterations", C.c_int64), ("fused", C.c_int32), ("newton_mode", C.c_int32), ("step_rule", C.c_int32)]


class DelaySpecC(C.Structure):
    _fields_ = [("n_pos", C.c_int32), ("pos", _I), ("n_term", C.c_int32), ("term_pos", _I), ("term_row", _I), ("term_col", _I),
                ("tau", _D), ("w", _D), ("depth", C.c_int32)]


class SensSpecC(C.Structure):
    _fields_ = [("n_group", C.c_int32), ("K", C.c_int32), ("members", _I), ("delta", _D), ("nh", C.c_int32), ("n_save", C.c_int32), ("n_obs", C.c_int32)]


# per-instance status of a transient (cadnip_tran_run's per_inst_host[:, 3]): CADNIP_TRAN_DELAY_OVERFLOW
TRAN_DELAY_OVERFLOW = -4


class RunStatsC(C.Structure):
    _fields_ = [("newton_iters", C.c_int64), ("steps_accepted", C.c_int64), ("steps_rejected", C.c_int64),
                ("newton_failures", C.c_int64), ("launches", C.c_int64), ("n_failed", C.c_int32),
                ("wall_seconds", C.c_double)]


_lib = None


def _share_hip_runtime():
    """One HIP runtime per process.  The library links /opt/rocm's libamdhip64.so.7; a PyTorch wheel carries its own copy and
    asks for it by file name (libamdhip64.so), which the dynamic loader does not match against a copy that was loaded under
    its soname -- so a torch imported AFTER this library brought a second HIP / HSA runtime into the process and found no
    device (round 1 had to order its tests around that).  If torch is installed but not loaded yet, its copy is loaded
    first, globally, under the name torch will ask for: the library (which asks for the soname) and a later torch then
    resolve to the same runtime, exactly as when torch comes first.  CADNIP_HIP_RUNTIME=<path> names another runtime to
    share, CADNIP_HIP_RUNTIME=system skips this."""
    import importlib.util
    import sys
    want = os.environ.get("CADNIP_HIP_RUNTIME", "")
    if want == "system" or "torch" in sys.modules:
        return
    cand = want
    if not cand:
        try:
            spec = importlib.util.find_spec("torch")
        except (ImportError, ValueError):
            spec = None
        if spec is None or not spec.origin:
            return
        cand = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
    if os.path.exists(cand):
        try:
            C.CDLL(cand, mode=C.RTLD_GLOBAL)
        except OSError:
            pass


def load_library():
    """dlopen the in-tree extension; raises if it has not been built (no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError("HIP extension %s is missing: run `python -c 'import __graft_entry__ as g; g.build()'`" % LIB_PATH)
    _share_hip_runtime()
    lib = C.CDLL(LIB_PATH)
    lib.cadnip_version.restype = C.c_char_p
    lib.cadnip_dev_ptr.restype = C.c_void_p
    lib.cadnip_stream.restype = C.c_void_p
    lib.cadnip_destroy.restype = None
    lib.cadnip_host_lu_free.restype = None
    lib.cadnip_host_lu_size.restype = C.c_int32
    lib.cadnip_dev_ptr.argtypes = [C.c_void_p, C.c_int32]
    lib.cadnip_stream.argtypes = [C.c_void_p]
    _lib = lib
    return lib


def _ip(a):
    return a.ctypes.data_as(_I)


def _dp(a):
    return a.ctypes.data_as(_D)


def _check(code, where):
    if code == OK:
        return
    if code == SINGULAR:
        raise SingularException(code, where)
    raise CadnipError(code, where)


def _ac_info(info=(0, 0, 0, 0)):
    """the ``info`` of the AC entry points from the four integers the library fills in; without them that of a call that launched nothing"""
    return dict(zip(("wpb", "lds_bytes", "systems", "workgroups"), (int(v) for v in info)))


MODE ={"dcop": 0, "tran": 1, "tranop": 2}

# cadnip_factor_solve's kernel argument (CADNIP_LUK_*): auto, k_lu_steps<4>, k_lu_f2_mw<4>, k_lu_f2s<W>, k_lu_f2<W>, k_lu with the fused Jacobian
LU_KERNELS = ("auto", "steps4", "mw4", "f2s", "f2", "plain")

MODE_NAMES = ("dcop", "tran", "tranop")


def structure_c(st: Structure):
    """The CadnipStructure of ``st`` (include/cadnip_hip.h) and the arrays it points into, which the caller keeps alive as long as
    the struct is in use.  Loads no library: the host-only tests feed the same struct to code compiled with the host compiler."""
    keep = []
    blocks = (DeviceBlockC * max(1, len(st.blocks)))()
    for k, blk in enumerate(st.blocks):
        nodes = np.ascontiguousarray(blk.nodes, dtype=np.int32)
        ipar = np.ascontiguousarray(blk.ipar, dtype=np.int32)
        keep += [nodes, ipar]
        b = blocks[k]
        b.type, b.count = type_id(blk.type), blk.count
        b.n_nodes, b.nodes = nodes.shape[0], _ip(nodes)
        b.n_ipar, b.ipar = ipar.shape[0], _ip(ipar)
        b.n_par = blk.n_par
        b.g_base, b.c_base, b.b_base = blk.g_base, blk.c_base, blk.b_base
        b.n_g, b.n_c, b.n_b = blk.n_g, blk.n_c, blk.n_b
    s = StructureC()
    s.n, s.n_nodes, s.n_currents, s.n_charges, s.n_limits = st.n, st.n_nodes, st.n_currents, st.n_charges, st.n_limits
    s.nnz = st.nnz
    arrs = {}
    for nm in ("rowptr", "colidx", "to_ref_nz", "g_ptr", "g_slots", "c_ptr", "c_slots", "b_ptr", "b_slots", "diag_nz"):
        a = np.ascontiguousarray(getattr(st, nm), dtype=np.int32)
        if a.size == 0:
            a = np.zeros(1, dtype=np.int32)
        arrs[nm] = a
        setattr(s, nm, _ip(a))
    wd = np.ascontiguousarray(st.wave_data, dtype=np.float64)
    wdp = wd if wd.size else np.zeros(1)
    li = np.ascontiguousarray(st.limit_init, dtype=np.float64)
    lip = li if li.size else np.zeros(1)
    keep += [arrs, wdp, lip, blocks]
    s.n_blocks, s.blocks = len(st.blocks), blocks
    s.n_wave_data, s.wave_data = wd.size, _dp(wdp)
    s.ns_g, s.ns_c, s.ns_b = st.ns_g, st.ns_c, st.ns_b
    s.limit_init = _dp(lip)
    return s, keep


class Handle:
    """One (structure, GPU) handle with ``B`` resident sweep instances."""

    def __init__(self, st: Structure, B: int = 1, device: int = 0):
        self.lib = load_library()
        self.st = st
        self.B = int(B)
        s, self._keep = structure_c(st)
        self.h = C.c_void_p()
        _check(self.lib.cadnip_create(C.byref(s), C.c_int32(self.B), C.c_int32(device), C.byref(self.h)), "cadnip_create")
        self.spec = dict(mode="tran", gmin=1e-12, gshunt=0.0, srcFact=1.0)

    def close(self):
        if getattr(self, "h", None) is not None and self.h:
            self.lib.cadnip_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- parameters / spec --------------------------------------------------------------
    def set_params(self, packed):
        for k, arr in enumerate(packed):
            a = np.ascontiguousarray(arr, dtype=np.float64)
            want = (self.B, self.st.blocks[k].n_par, self.st.blocks[k].count)
            if a.shape != want:
                raise ValueError("parameter block %d has shape %r, the structure needs %r" % (k, a.shape, want))
            _check(self.lib.cadnip_set_params(self.h, C.c_int32(k), _dp(a)), "cadnip_set_params")

    def set_spec(self, mode=None, gmin=None, gshunt=None, srcFact=None):
        for k, v in (("mode", mode), ("gmin", gmin), ("gshunt", gshunt), ("srcFact", srcFact)):
            if v is not None:
                self.spec[k] = v
        sp = SpecC(MODE[self.spec["mode"]], self.spec["gmin"], self.spec["gshunt"], self.spec["srcFact"])
        _check(self.lib.cadnip_set_spec(self.h, C.byref(sp)), "cadnip_set_spec")

    def set_initjct(self, on):
        _check(self.lib.cadnip_set_initjct(self.h, C.c_int32(1 if on else 0)), "cadnip_set_initjct")

    # -- the three callbacks --------------------------------------------------------------
    def _bn(self, x):
        a = np.ascontiguousarray(np.broadcast_to(np.asarray(x, dtype=np.float64), (self.B, self.st.n)))
        return a

    def _b(self, x):
        return np.ascontiguousarray(np.broadcast_to(np.asarray(x, dtype=np.float64), (self.B,)))

    def rebuild(self, u, t=0.0):
        """fast_rebuild!(ws, u, t)"""
        ua, ta = self._bn(u), self._b(t)
        _check(self.lib.cadnip_rebuild(self.h, _dp(ua), _dp(ta)), "cadnip_rebuild")

    def residual(self, du, u):
        """fast_residual! minus the restamp: resid = C*du + G*u - b at the last rebuild."""
        dua, ua = self._bn(du), self._bn(u)
        r = np.empty((self.B, self.st.n))
        _check(self.lib.cadnip_residual(self.h, _dp(dua), _dp(ua), _dp(r)), "cadnip_residual")
        return r

    def jacobian(self, gamma, readback=True):
        """fast_jacobian! minus the restamp: J = G + gamma*C; returned in the reference's CSC nz order."""
        g = self._b(gamma)
        J = np.empty((self.B, self.st.nnz)) if readback else None
        _check(self.lib.cadnip_jacobian(self.h, _dp(g), _dp(J) if readback else None), "cadnip_jacobian")
        return J

    def jacobian_dense(self, gamma):
        """fast_jacobian!(J::Matrix, ...) of a dense structure (precompile.jl:588-603) minus the restamp: [B, n, n] with J[b, i, j]."""
        g = self._b(gamma)
        J = np.empty((self.B, self.st.n * self.st.n))
        _check(self.lib.cadnip_jacobian_dense(self.h, _dp(g), _dp(J)), "cadnip_jacobian_dense")
        return J.reshape(self.B, self.st.n, self.st.n).transpose(0, 2, 1)        # column-major blocks -> [i, j]

    def ode_rhs(self, u, t=0.0):
        """rhs!(du, u, p, t) of the ODE form (src/mna/solve.jl:2241-2248): restamp, du = b - G*u."""
        ua, ta = self._bn(u), self._b(t)
        du = np.empty((self.B, self.st.n))
        _check(self.lib.cadnip_ode_rhs(self.h, _dp(ua), _dp(ta), _dp(du)), "cadnip_ode_rhs")
        return du

    def ode_jacobian(self, u, t=0.0):
        """jac!(J, u, p, t) of the ODE form (src/mna/solve.jl:2251-2276): restamp, J = -G in the reference's nz order."""
        ua, ta = self._bn(u), self._b(t)
        J = np.empty((self.B, self.st.nnz))
        _check(self.lib.cadnip_ode_jacobian(self.h, _dp(ua), _dp(ta), _dp(J)), "cadnip_ode_jacobian")
        return J

    def get_GCb(self):
        B, st = self.B, self.st
        G, Cm, b = np.empty((B, st.nnz)), np.empty((B, st.nnz)), np.empty((B, st.n))
        lw = np.empty((B, max(st.n_limits, 1)))
        _check(self.lib.cadnip_get_GCb(self.h, _dp(G), _dp(Cm), _dp(b), _dp(lw)), "cadnip_get_GCb")
        return G, Cm, b, lw[:, :st.n_limits]

    def get_contributions(self):
        """Per-device contributions of one restamp at the current state: (S_g [B, ns_g], S_c [B, ns_c], S_b [B, ns_b])."""
        st = self.st
        ns = st.ns_g + st.ns_c + st.ns_b
        S = np.zeros((self.B, max(ns, 1)))
        _check(self.lib.cadnip_get_contributions(self.h, _dp(S)), "cadnip_get_contributions")
        return S[:, :st.ns_g], S[:, st.ns_g:st.ns_g + st.ns_c], S[:, st.ns_g + st.ns_c:ns]

    # -- LU ----------------------------------------------------------------------------------
    def analyze(self, sample_instance=0):
        _check(self.lib.cadnip_analyze(self.h, C.c_int32(sample_instance)), "cadnip_analyze")

    def analyze_values(self, J_ref_nz):
        """``J_ref_nz``: sample values in the reference's CSC nz order."""
        csr = np.ascontiguousarray(np.asarray(J_ref_nz, dtype=np.float64)[self.st.to_ref_nz])
        _check(self.lib.cadnip_analyze_values(self.h, _dp(csr)), "cadnip_analyze_values")

    def factor(self):
        _check(self.lib.cadnip_factor(self.h), "cadnip_factor")

    def solve(self, rhs):
        r = self._bn(rhs)
        x = np.empty_like(r)
        _check(self.lib.cadnip_solve(self.h, _dp(r), _dp(x)), "cadnip_solve")
        return x

    def factor_solve(self, gamma, rhs, kernel="auto", active=None, x0=None):
        """cadnip_factor_solve: the drivers' per-op refactor + solve x = (G + gamma C)^-1 rhs on the G / C of the last rebuild, with one chosen
        kernel (``LU_KERNELS``; plain launches).  ``active``: [B] (None = all); an inactive instance returns its row of ``x0`` (default zeros).
        Returns (x [B, n], flags [B], info) with info = {kernel, wpb, wpi, nc, n_pre, n_post} of the kernel that ran.  A forced kernel that does
        not apply to this circuit raises CadnipError(CADNIP_BADARG)."""
        k = LU_KERNELS.index(kernel) if isinstance(kernel, str) else int(kernel)
        g, r = self._b(gamma), self._bn(rhs)
        x = np.array(self._bn(0.0 if x0 is None else x0))
        act = None if active is None else np.ascontiguousarray(np.broadcast_to(np.asarray(active, dtype=np.int32), (self.B,)))
        flags = np.zeros(self.B, dtype=np.int32)
        info = np.zeros(6, dtype=np.int32)
        _check(self.lib.cadnip_factor_solve(self.h, _dp(g), _dp(r), None if act is None else _ip(act), C.c_int32(k), _dp(x), _ip(flags), _ip(info)),
               "cadnip_factor_solve")
        return x, flags, dict(zip(("kernel", "wpb", "wpi", "nc", "n_pre", "n_post"), [LU_KERNELS[info[0]]] + [int(v) for v in info[1:]]))

    def newton_step(self, u, du, gamma=None, t=None, refresh=True, want_resid=False, fused=False):
        """cadnip_newton_step: resid = C du + G u - b, [J = G + gamma C refactored,] delta = J^-1 resid -- one call, one synchronisation.
        ``fused``: cadnip_newton_step_fused (one kernel; agrees to rounding).  Returns (delta [B, n], ||resid||_2 [B]) and resid [B, n]
        with ``want_resid``."""
        uu, dd = self._bn(u), self._bn(du)
        delta, nrm = np.empty_like(uu), np.empty(self.B)
        resid = np.empty_like(uu) if want_resid else None
        g = None if gamma is None else np.ascontiguousarray(np.broadcast_to(np.asarray(gamma, dtype=np.float64), (self.B,)))
        tt = None if t is None else np.ascontiguousarray(np.broadcast_to(np.asarray(t, dtype=np.float64), (self.B,)))
        fn = self.lib.cadnip_newton_step_fused if fused else self.lib.cadnip_newton_step
        _check(fn(self.h, _dp(uu), _dp(dd), None if g is None else _dp(g), None if tt is None else _dp(tt), C.c_int32(1 if refresh else 0),
                  _dp(delta), _dp(nrm), None if resid is None else _dp(resid)), "cadnip_newton_step_fused" if fused else "cadnip_newton_step")
        return (delta, nrm, resid) if want_resid else (delta, nrm)

    def lu_order(self):
        """(rperm, cperm) of the handle's current pivot order: pivot k uses original row rperm[k] and column cperm[k]."""
        rp, cp = np.zeros(self.st.n, dtype=np.int32), np.zeros(self.st.n, dtype=np.int32)
        _check(self.lib.cadnip_lu_order(self.h, _ip(rp), _ip(cp)), "cadnip_lu_order")
        return rp, cp

    def ac_solve(self, omega, gmin, b_ac, wpb=0):
        """cadnip_ac_solve: x[b, f] = (G[b] + gmin on the node diagonals + j omega[f] C[b])^-1 b_ac[b] on the G / C of the last rebuild, with
        the handle's pivot order -- B x F complex sparse systems in one batched kernel (csrc/ac_lu.hip).  ``omega`` [F] angular frequencies,
        ``b_ac`` [B, n] complex (or [n], broadcast), ``wpb`` systems per workgroup (0: the launch plan's choice).  Returns (x complex128
        [B, F, n], berr [B, F], flags [B, F], info) with berr the componentwise backward error of x, flags bit 0 a zero / non-finite pivot or a
        non-finite solution, and info = {wpb, lds_bytes, systems, workgroups}.  An empty grid launches nothing.  A circuit whose work arrays
        exceed LDS (under the default memory: ``ac_set_memory``), or an invalid ``wpb``, raises CadnipError(CADNIP_BADARG)."""
        om = np.ascontiguousarray(np.asarray(omega, dtype=np.float64).ravel())
        B, n, F = self.B, self.st.n, om.size
        if F == 0:
            return np.zeros((B, 0, n), dtype=complex), np.zeros((B, 0)), np.zeros((B, 0), dtype=np.int32), _ac_info()
        b = np.ascontiguousarray(np.broadcast_to(np.asarray(b_ac, dtype=np.complex128), (B, n)))
        x = np.empty((B, F, n), dtype=np.complex128)
        berr, flags, info = np.empty((B, F)), np.zeros((B, F), dtype=np.int32), np.zeros(4, dtype=np.int32)
        _check(self.lib.cadnip_ac_solve(self.h, C.c_int32(F), _dp(om), C.c_double(gmin), b.ctypes.data_as(_D), C.c_int32(int(wpb)),
                                        x.ctypes.data_as(_D), _dp(berr), _ip(flags), _ip(info)), "cadnip_ac_solve")
        return x, berr, flags, _ac_info(info)

    def ac_adjoint(self, omega, gmin, c, pairs, wpb=0, want_x=False):
        """cadnip_ac_adjoint: x[b, f] solves A^T x = c[b] with A = G[b] + gmin on the node diagonals + j omega[f] C[b] as ``ac_solve`` -- same pivot
        order, same factors, the solves run transposed (csrc/ac_lu.hip: k_ac_adj).  ``c`` [B, n] complex (or [n], broadcast), ``pairs`` [K, 2]
        unknown indices (-1 = ground).  Returns (h complex128 [B, F, K] with h[..., k] = x[p_k] - x[n_k], x [B, F, n] or None without
        ``want_x``, berr [B, F], flags [B, F], info) -- berr, flags and info as ``ac_solve``.  An empty grid launches nothing.  No pairs, a pair
        index outside [-1, n), a circuit beyond LDS or an invalid ``wpb`` raise CadnipError(CADNIP_BADARG)."""
        om = np.ascontiguousarray(np.asarray(omega, dtype=np.float64).ravel())
        pr = np.ascontiguousarray(np.asarray(pairs, dtype=np.int32).reshape(-1, 2))
        B, n, F, K = self.B, self.st.n, om.size, pr.shape[0]
        if F == 0:
            return (np.zeros((B, 0, K), dtype=complex), np.zeros((B, 0, n), dtype=complex) if want_x else None, np.zeros((B, 0)),
                    np.zeros((B, 0), dtype=np.int32), _ac_info())
        cc = np.ascontiguousarray(np.broadcast_to(np.asarray(c, dtype=np.complex128), (B, n)))
        hh = np.empty((B, F, K), dtype=np.complex128)
        x = np.empty((B, F, n), dtype=np.complex128) if want_x else None
        berr, flags, info = np.empty((B, F)), np.zeros((B, F), dtype=np.int32), np.zeros(4, dtype=np.int32)
        _check(self.lib.cadnip_ac_adjoint(self.h, C.c_int32(F), _dp(om), C.c_double(gmin), cc.ctypes.data_as(_D), C.c_int32(K),
                                          _ip(pr) if K else None, C.c_int32(int(wpb)), hh.ctypes.data_as(_D), None if x is None else x.ctypes.data_as(_D),
                                          _dp(berr), _ip(flags), _ip(info)), "cadnip_ac_adjoint")
        return hh, x, berr, flags, _ac_info(info)

    def ac_solve_multi(self, omega, gmin, b, pairs=None, wpb=0, want_x=True, x_out=None):
        """cadnip_ac_solve_multi: x[b, f, k] = A[b, f]^-1 b[b, k] for K right-hand sides per instance against ONE factorisation per system, A and
        the pivot order as ``ac_solve`` (csrc/ac_lu.hip: k_ac_lu_multi) -- column k is bit-identical to ``ac_solve(omega, gmin, b[:, k])``.
        ``b`` [B, K, n] complex (or [K, n], broadcast), ``pairs`` [P, 2] unknown indices (-1 = ground) or None.  Returns (h complex128
        [B, F, K, P] with h[..., j] = x[p_j] - x[n_j], or None without pairs; x [B, F, K, n], or None without ``want_x``; berr [B, F, K];
        flags [B, F, K]; info) -- berr, flags (per column; a bad pivot flags all K columns of its system) and info as ``ac_solve``.  An empty
        grid launches nothing.  ``x_out``: a C-contiguous complex128 array [B, F, K, n] to receive x (and be returned) instead of a new one -- a
        caller that sweeps repeatedly spares the first touch of a fresh array, which above 32 MiB costs more than the sweep;
        it implies ``want_x``.  No column, neither pairs nor x, a pair index outside [-1, n), a circuit the memory setting refuses or an
        invalid ``wpb`` raise CadnipError(CADNIP_BADARG)."""
        return self._ac_multi("cadnip_ac_solve_multi", omega, gmin, b, pairs, wpb, want_x, x_out)

    def ac_adjoint_multi(self, omega, gmin, c, pairs=None, wpb=0, want_x=False, x_out=None):
        """cadnip_ac_adjoint_multi: x[b, f, k] solves A[b, f]^T x = c[b, k] for K right-hand sides per instance against ONE factorisation per
        system, A, the pivot order and the transposed solves as ``ac_adjoint`` (csrc/ac_lu.hip: k_ac_adj_multi) -- column k is bit-identical
        to ``ac_adjoint(omega, gmin, c[:, k], pairs)``.  ``c`` [B, K, n] complex (or [K, n], shared by all instances); everything else --
        ``pairs``, ``x_out``, the returned (h [B, F, K, P] or None, x [B, F, K, n] or None, berr [B, F, K], flags [B, F, K], info) and what
        raises -- as ``ac_solve_multi``, except that x is returned only when asked for."""
        return self._ac_multi("cadnip_ac_adjoint_multi", omega, gmin, c, pairs, wpb, want_x, x_out)

    def _ac_multi(self, entry, omega, gmin, b, pairs, wpb, want_x, x_out):
        """the two multi-column entry points: one argument list, one layout"""
        om = np.ascontiguousarray(np.asarray(omega, dtype=np.float64).ravel())
        bb = np.asarray(b, dtype=np.complex128)
        B, n, F = self.B, self.st.n, om.size
        if bb.ndim < 2 or bb.shape[-1] != n:
            raise ValueError("b must be [K, n] or [B, K, n]")
        K = bb.shape[-2]
        bb = np.ascontiguousarray(np.broadcast_to(bb, (B, K, n)))
        pr = None if pairs is None else np.ascontiguousarray(np.asarray(pairs, dtype=np.int32).reshape(-1, 2))
        P = 0 if pr is None else pr.shape[0]
        hh = np.empty((B, F, K, P), dtype=np.complex128) if P else None
        if x_out is not None and (not isinstance(x_out, np.ndarray) or x_out.dtype != np.complex128 or x_out.shape != (B, F, K, n) or not x_out.flags.c_contiguous):
            raise ValueError("x_out must be a C-contiguous complex128 array of shape [B, F, K, n]")
        x = x_out if x_out is not None else np.empty((B, F, K, n), dtype=np.complex128) if want_x else None
        berr, flags, info = np.empty((B, F, K)), np.zeros((B, F, K), dtype=np.int32), np.zeros(4, dtype=np.int32)
        if F == 0:
            return hh, x, berr, flags, _ac_info()
        _check(getattr(self.lib, entry)(self.h, C.c_int32(F), _dp(om), C.c_double(gmin), C.c_int32(K), bb.ctypes.data_as(_D), C.c_int32(P),
                                        _ip(pr) if P else None, C.c_int32(int(wpb)), None if hh is None else hh.ctypes.data_as(_D),
                                        None if x is None else x.ctypes.data_as(_D), _dp(berr), _ip(flags), _ip(info)), entry)
        return hh, x, berr, flags, _ac_info(info)

    def ac_sens(self, omega, gmin, base, plus, minus, scale, b_ac, c, pair, db=None, wpb=0, want_x=False):
        """cadnip_ac_sens: per (base instance, frequency) the response y = x[p] - x[n] of A x = b_ac and its derivatives with respect to K
        parameters from ONE factorisation (csrc/ac_lu.hip: k_ac_sens): s[b, f, k] = lambda^T (db[b, k] - (dG + j omega[f] dC) x) with
        A^T lambda = c, dG = (G[plus[b, k]] - G[minus[b, k]]) scale[b, k] and dC likewise, on the G / C of the last rebuild.  ``base`` [NB]
        instance indices, ``plus`` / ``minus`` [NB, K] instance indices, ``scale`` [NB, K], ``b_ac`` [NB, n] complex (or [n], broadcast),
        ``c`` [n] complex, ``pair`` (p, n) unknown indices (-1 = ground), ``db`` [NB, K, n] complex or None (zeros).  Returns (y complex128
        [NB, F], s [NB, F, K], x [NB, F, 2, n] -- x and lambda -- or None without ``want_x``, berr [NB, F, 2] (forward, adjoint), flags
        [NB, F, K] (bit 0: the system, bit 1: a non-finite s), info as ``ac_solve``).  x and lambda are bit-identical to ``ac_solve`` /
        ``ac_adjoint`` on instance base[b].  An empty grid launches nothing.  Arrays of the wrong shape raise ValueError; no base, no parameter,
        an instance index outside [0, B), a pair index outside [-1, n), the pair (-1, -1), a circuit the memory setting refuses or an invalid
        ``wpb`` raise CadnipError(CADNIP_BADARG)."""
        om = np.ascontiguousarray(np.asarray(omega, dtype=np.float64).ravel())
        bs = np.ascontiguousarray(np.asarray(base, dtype=np.int32).ravel())
        pl, mi = np.ascontiguousarray(plus, dtype=np.int32), np.ascontiguousarray(minus, dtype=np.int32)
        sc = np.ascontiguousarray(scale, dtype=np.float64)
        n, F, NB = self.st.n, om.size, bs.size
        if pl.ndim != 2 or pl.shape[0] != NB or mi.shape != pl.shape or sc.shape != pl.shape:
            raise ValueError("plus, minus and scale must be [NB, K] for NB base instances")
        K = pl.shape[1]
        pr = np.ascontiguousarray(np.asarray(pair, dtype=np.int32).ravel())
        cc = np.ascontiguousarray(np.asarray(c, dtype=np.complex128))
        if pr.shape != (2,) or cc.shape != (n,):
            raise ValueError("pair must be (p, n) and c an [n] column")
        bb = np.asarray(b_ac, dtype=np.complex128)
        if bb.shape not in ((n,), (NB, n)):
            raise ValueError("b_ac must be [n] or [NB, n]")
        bb = np.ascontiguousarray(np.broadcast_to(bb, (NB, n)))
        dd = None if db is None else np.ascontiguousarray(db, dtype=np.complex128)
        if dd is not None and dd.shape != (NB, K, n):
            raise ValueError("db must be [NB, K, n]")
        y, s = np.empty((NB, F), dtype=np.complex128), np.empty((NB, F, K), dtype=np.complex128)
        x = np.empty((NB, F, 2, n), dtype=np.complex128) if want_x else None
        berr, flags, info = np.empty((NB, F, 2)), np.zeros((NB, F, K), dtype=np.int32), np.zeros(4, dtype=np.int32)
        if F == 0:
            return y, s, x, berr, flags, _ac_info()
        _check(self.lib.cadnip_ac_sens(self.h, C.c_int32(F), _dp(om), C.c_double(gmin), C.c_int32(NB), _ip(bs), C.c_int32(K), _ip(pl), _ip(mi), _dp(sc),
                                       bb.ctypes.data_as(_D), None if dd is None else dd.ctypes.data_as(_D), cc.ctypes.data_as(_D), _ip(pr),
                                       C.c_int32(int(wpb)), y.ctypes.data_as(_D), s.ctypes.data_as(_D), None if x is None else x.ctypes.data_as(_D),
                                       _dp(berr), _ip(flags), _ip(info)), "cadnip_ac_sens")
        return y, s, x, berr, flags, _ac_info(info)

    def ac_arnoldi(self, omega, gmin, b, m, pairs=None, breakdown_tol=AC_BREAKDOWN_TOL, wpb=0, want_v=False):
        """cadnip_ac_arnoldi: per (instance, shift) m steps of shift-invert Arnoldi on K = A^-1 C started at A^-1 b, A = G + gmin + j omega[s] C as
        ``ac_solve`` -- one factorisation and m_eff + 1 columns per system, all in one launch (csrc/ac_lu.hip: k_ac_arnoldi).  ``omega`` [S] the
        shifts' angular frequencies, ``b`` [B, n] complex (or [n], broadcast), ``pairs`` [P, 2] unknown indices (-1 = ground) or None.  Returns
        (H complex128 [B, S, m+1, m], beta [B, S], m_eff int32 [B, S], l [B, S, m, P] -- l[.., j, p] = v_j[p_p] - v_j[n_p] -- or None without
        pairs, V [B, S, m+1, n] or None without ``want_v``, berr [B, S], flags [B, S], info).  beta v_0 is ``ac_solve``'s x; the eigenvalues theta
        of H[:m_eff, :m_eff] give the poles j omega[s] - 1 / theta.  flags: bit 0 a zero / non-finite pivot or non-finite output, bit 1 beta zero
        or non-finite (m_eff = 0), bit 2 the Krylov space closed at step m_eff (informational).  berr and info as ``ac_solve``.  An empty shift
        list launches nothing.  A ``b`` of the wrong shape raises ValueError; m outside [1, n], a tolerance outside (0, 1), a pair index outside
        [-1, n), a circuit the memory setting refuses or an invalid ``wpb`` raise CadnipError(CADNIP_BADARG)."""
        om = np.ascontiguousarray(np.asarray(omega, dtype=np.float64).ravel())
        B, n, S, m = self.B, self.st.n, om.size, int(m)
        bb = np.asarray(b, dtype=np.complex128)
        if bb.shape not in ((n,), (B, n)):
            raise ValueError("b must be [n] or [B, n]")
        bb = np.ascontiguousarray(np.broadcast_to(bb, (B, n)))
        pr = None if pairs is None else np.ascontiguousarray(np.asarray(pairs, dtype=np.int32).reshape(-1, 2))
        P = 0 if pr is None else pr.shape[0]
        mm = max(m, 0)
        H = np.zeros((B, S, mm + 1, mm), dtype=np.complex128)
        beta, meff = np.zeros((B, S)), np.zeros((B, S), dtype=np.int32)
        ll = np.zeros((B, S, mm, P), dtype=np.complex128) if P else None
        V = np.zeros((B, S, mm + 1, n), dtype=np.complex128) if want_v else None
        berr, flags, info = np.zeros((B, S)), np.zeros((B, S), dtype=np.int32), np.zeros(4, dtype=np.int32)
        if S == 0:
            return H, beta, meff, ll, V, berr, flags, _ac_info()
        _check(self.lib.cadnip_ac_arnoldi(self.h, C.c_int32(S), _dp(om), C.c_double(gmin), bb.ctypes.data_as(_D), C.c_int32(m), C.c_double(breakdown_tol),
                                          C.c_int32(P), _ip(pr) if P else None, C.c_int32(int(wpb)), H.ctypes.data_as(_D), _dp(beta), _ip(meff),
                                          None if ll is None else ll.ctypes.data_as(_D), None if V is None else V.ctypes.data_as(_D),
                                          _dp(berr), _ip(flags), _ip(info)), "cadnip_ac_arnoldi")
        return H, beta, meff, ll, V, berr, flags, _ac_info(info)

    def ac_set_memory(self, mode="lds", max_waves=0):
        """cadnip_ac_set_memory: where ``ac_solve`` / ``ac_adjoint`` keep a system's work arrays from now on.  "lds" (the default of a new handle):
        in LDS, every call as without the setting; "hbm": in a workspace in device memory, by persistent waves (k_ac_lu_hbm / k_ac_adj_hbm:
        the same doubles; ``wpb`` is then waves per workgroup, 0 = 4, and info["lds_bytes"] is 0); "auto": LDS when its launch plan accepts the
        circuit, else HBM.  ``max_waves`` > 0 caps the waves (= workspaces) of a launch, 0: the plan's choice (csrc/ac_hbm_plan.hpp).  An
        unknown mode or a negative ``max_waves`` raises CadnipError(CADNIP_BADARG) and leaves the setting as it was."""
        code = AC_MEMORY.get(mode, -1) if isinstance(mode, str) else int(mode)
        _check(self.lib.cadnip_ac_set_memory(self.h, C.c_int32(code), C.c_int32(int(max_waves))), "cadnip_ac_set_memory")

    def ac_set_overlay(self, pos, omegas, val):
        """cadnip_ac_set_overlay: from now on ``ac_solve``, ``ac_adjoint``, ``ac_solve_multi`` and ``ac_adjoint_multi`` solve
        A[b, f] = G[b] + gmin + j omega[f] C[b] + D[b, f], with D non-zero at the CSR positions ``pos`` [O] (distinct, in the order of the
        structure's rowptr / colidx) and ``val`` [B, F, O] complex (or [F, O], broadcast) its values on the grid ``omegas`` [F] -- how a delayed
        stamp's e^{-j w tau} enters (api.ac_delay_overlay computes such a table).  The overlay kernels (csrc/ac_lu.hip: k_ac_lu_ovl and its
        kin) add it in the load, the residuals and the backward error; results stay bit-identical across ``wpb``, memory homes and between the
        multi calls' columns and the single-column calls.  While it is set those four calls must be made on exactly ``omegas``, and
        ``ac_sens`` / ``ac_arnoldi`` raise CadnipError(CADNIP_BADARG).  A non-finite value flags its own system (bit 0).  An empty ``pos``
        clears the setting, as ``ac_clear_overlay``.  A ``val`` of the wrong shape raises ValueError; a position outside [0, nnz) or named
        twice, an empty grid or a table beyond 256 MiB raise CadnipError(CADNIP_BADARG) and leave the previous setting in force."""
        ps = np.ascontiguousarray(np.asarray(pos, dtype=np.int32).ravel())
        om = np.ascontiguousarray(np.asarray(omegas, dtype=np.float64).ravel())
        if ps.size == 0:
            return self.ac_clear_overlay()
        vv = np.asarray(val, dtype=np.complex128)
        if vv.shape not in ((om.size, ps.size), (self.B, om.size, ps.size)):
            raise ValueError("val must be [F, O] or [B, F, O] for F frequencies and O positions")
        vv = np.ascontiguousarray(np.broadcast_to(vv, (self.B, om.size, ps.size)))
        _check(self.lib.cadnip_ac_set_overlay(self.h, C.c_int32(ps.size), _ip(ps), C.c_int32(om.size), _dp(om), vv.ctypes.data_as(_D)), "cadnip_ac_set_overlay")

    def ac_clear_overlay(self):
        """cadnip_ac_set_overlay with n_ovl = 0: no overlay; every AC call is again exactly what it is on a new handle."""
        _check(self.lib.cadnip_ac_set_overlay(self.h, C.c_int32(0), None, C.c_int32(0), None, None), "cadnip_ac_set_overlay")

    def ac_plan_info(self):
        """cadnip_ac_plan_info: {memory ("lds" / "hbm"), n_waves, work_bytes, lds_bytes} of the last ``ac_solve`` / ``ac_adjoint`` call that launched."""
        out = (C.c_int64 * 4)()
        _check(self.lib.cadnip_ac_plan_info(self.h, out), "cadnip_ac_plan_info")
        return dict(memory={v: k for k, v in AC_MEMORY.items()}[int(out[0])], n_waves=int(out[1]), work_bytes=int(out[2]), lds_bytes=int(out[3]))

    def lu_stats(self):
        v = [C.c_int32() for _ in range(5)]
        _check(self.lib.cadnip_lu_stats(self.h, *[C.byref(x) for x in v]), "cadnip_lu_stats")
        return dict(zip(("nnz_lu", "n_terms", "n_levels", "n_fwd_levels", "n_bwd_levels"), [x.value for x in v]))

    # -- drivers -------------------------------------------------------------------------------
    def dc_run(self, u0=None, abstol=1e-10, maxiters=100, use_pcnr=True, cold_start=True, use_stepping=True,
               raise_on_fail=False, fused=False, participate=None):
        """``participate``: boolean mask [B]; instances with False sit the run out (u unchanged, converged False)."""
        # a cold start of everyone from zero: the device makes the zeros (CADNIP_DC_COLD_ZERO), u is output only
        zero = u0 is None and bool(cold_start) and participate is None
        u = np.empty((self.B, self.st.n)) if zero else self._bn(0.0 if u0 is None else u0).copy()
        conv = np.zeros(self.B, dtype=np.int32)
        st = RunStatsC()
        pm = None if participate is None else np.ascontiguousarray(np.asarray(participate, dtype=bool).astype(np.int32))
        o = DCOptsC(abstol, maxiters, int(use_pcnr), DC_COLD_ZERO if zero else int(cold_start), int(use_stepping), int(fused), None if pm is None else _ip(pm))
        rc = self.lib.cadnip_dc_run(self.h, C.byref(o), _dp(u), _ip(conv), C.byref(st))
        if rc not in (OK, NOCONV) or (rc == NOCONV and raise_on_fail):
            _check(rc, "cadnip_dc_run")
        return u, conv.astype(bool), _stats(st)

    def dc_log(self):
        """The fallback chain of the last ``dc_run``: list of (instance, stage, rung value, converged, Newton solves)."""
        k = int(self.lib.cadnip_dc_log_size(self.h))
        inst, stage, ok = (np.zeros(max(k, 1), dtype=np.int32) for _ in range(3))
        val, it = np.zeros(max(k, 1)), np.zeros(max(k, 1), dtype=np.int64)
        _check(self.lib.cadnip_dc_log_get(self.h, _ip(inst), _ip(stage), _dp(val), _ip(ok), it.ctypes.data_as(C.POINTER(C.c_int64))), "cadnip_dc_log_get")
        return [(int(inst[j]), int(stage[j]), float(val[j]), bool(ok[j]), int(it[j])) for j in range(k)]

    def tran_run(self, t0, t1, abstol, reltol=1e-4, breaks=(), save_t=(), obs=None, h0=0.0, hmin=0.0, hmax=0.0,
                 max_newton=10, max_order=2, use_pcnr=False, newton_tol=1e-3, max_iterations=0, fused=False,
                 err_mask="differential", newton_mode=0, step_rule=0):
        at = np.ascontiguousarray(np.broadcast_to(np.asarray(abstol, dtype=np.float64), (self.st.n,)))
        if isinstance(err_mask, str):
            em = self.st.differential_mask() if err_mask == "differential" else np.ones(self.st.n)
        else:
            em = np.ones(self.st.n) if err_mask is None else np.asarray(err_mask, dtype=np.float64)
        em = np.ascontiguousarray(em, dtype=np.float64)
        br = np.ascontiguousarray(np.asarray(breaks, dtype=np.float64))
        sv = np.ascontiguousarray(np.asarray(save_t, dtype=np.float64))
        ob = np.ascontiguousarray(np.asarray(obs if obs is not None else [], dtype=np.int32))
        n_obs = ob.size if ob.size else self.st.n
        out = np.zeros((self.B, sv.size, n_obs))
        per = np.zeros((self.B, 4), dtype=np.int64)
        st = RunStatsC()
        o = TranOptsC(t0, t1, reltol, _dp(at), _dp(em), h0, hmin, hmax, max_newton, max_order, int(use_pcnr), newton_tol,
                      br.size, _dp(br) if br.size else None, sv.size, _dp(sv) if sv.size else None,
                      ob.size, _ip(ob) if ob.size else None, max_iterations, int(fused), int(newton_mode), int(step_rule))  # fused: 0 = one kernel per op, non-zero = fused Newton kernel
        rc = self.lib.cadnip_tran_run(self.h, C.byref(o), _dp(out), per.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(st))
        if rc not in (OK, NOCONV):
            _check(rc, "cadnip_tran_run")
        return out, per, _stats(st)

    def tran_set_delay(self, pos, term_pos, term_row, term_col, tau, w, depth=0):
        """cadnip_tran_set_delay: from now on ``tran_run`` treats the stamps ``w`` [B, T] (or [T], broadcast) at the CSR positions
        ``pos[term_pos[t]]`` = (``term_row[t]``, ``term_col[t]``) as delayed by ``tau`` [B, T] seconds: G_tran = G - W and
        b_tran[row] = b[row] - sum w u[col](tn - tau), the delayed values read from a ring of ``depth`` (0 = 1024) accepted points per
        instance in device memory, linearly interpolated (csrc/delay.hip, csrc/delay_plan.hpp; api.ac_delay_overlay computes such terms).
        Such a run clamps its steps to min(tau), runs on the per-op kernels whatever ``fused`` says, and an instance whose look-up falls
        off the ring ends with status TRAN_DELAY_OVERFLOW.  No terms clears the setting, as ``tran_clear_delay``.  Arrays of the wrong
        shape raise ValueError; an index out of range, a term that does not sit on its position or a tau that is not positive and finite
        raise CadnipError(CADNIP_BADARG) and leave the previous setting in force."""
        ps = np.ascontiguousarray(np.asarray(pos, dtype=np.int32).ravel())
        tp, tr, tc = (np.ascontiguousarray(np.asarray(a, dtype=np.int32).ravel()) for a in (term_pos, term_row, term_col))
        if tp.size == 0:
            return self.tran_clear_delay()
        if not (tp.size == tr.size == tc.size):
            raise ValueError("term_pos, term_row and term_col must have one entry per term")
        tt, ww = np.asarray(tau, dtype=np.float64), np.asarray(w, dtype=np.float64)
        for a in (tt, ww):
            if a.shape not in ((tp.size,), (self.B, tp.size)):
                raise ValueError("tau and w must be [T] or [B, T] for T terms")
        tt = np.ascontiguousarray(np.broadcast_to(tt, (self.B, tp.size)))
        ww = np.ascontiguousarray(np.broadcast_to(ww, (self.B, tp.size)))
        spec = DelaySpecC(ps.size, _ip(ps), tp.size, _ip(tp), _ip(tr), _ip(tc), _dp(tt), _dp(ww), int(depth))
        _check(self.lib.cadnip_tran_set_delay(self.h, C.byref(spec)), "cadnip_tran_set_delay")

    def tran_delay_info(self):
        """cadnip_tran_delay_info: {n_pos, n_rows, n_taps, n_term, depth} of the plan built from the delay spec in force (zeros without one):
        the sizes the delay kernels index by."""
        out = (C.c_int32 * 5)()
        _check(self.lib.cadnip_tran_delay_info(self.h, out), "cadnip_tran_delay_info")
        return dict(zip(("n_pos", "n_rows", "n_taps", "n_term", "depth"), (int(x) for x in out)))

    def tran_clear_delay(self):
        """cadnip_tran_set_delay with no spec: ``tran_run`` is again exactly what it is on a new handle."""
        _check(self.lib.cadnip_tran_set_delay(self.h, None), "cadnip_tran_set_delay")

    def tran_set_sens(self, members, delta, n_save, n_obs=None, max_order=2):
        """cadnip_tran_set_sens: from now on ``tran_run`` computes the forward sensitivities of the groups ``members`` [G, 2 + 2 K] -- rows
        {base, twin, p_0 + delta_0, p_0 - delta_0, ...} of instance indices whose parameters the caller has set accordingly -- with the
        parameter steps ``delta`` [G, K] (csrc/tran_sens.hip, csrc/tran_sens_plan.hpp).  Only the bases integrate; the other members are
        parked and their rows of ``tran_run``'s results mean nothing.  ``n_save`` / ``n_obs`` (None: all n) / ``max_order``: those of the
        runs to come.  Each run needs a ``tran_sens_init`` before it, runs on the per-op kernels whatever ``fused`` says, and leaves its
        results to ``tran_sens_get``.  Arrays of the wrong shape raise ValueError; an index out of range, an instance named twice, a delta
        that is not positive and finite, results beyond 256 MiB or a delay spec in force raise CadnipError(CADNIP_BADARG) and leave the
        previous setting in force."""
        mem = np.ascontiguousarray(np.asarray(members, dtype=np.int32))
        dl = np.ascontiguousarray(np.asarray(delta, dtype=np.float64))
        if mem.ndim != 2 or dl.ndim != 2 or dl.shape[0] != mem.shape[0] or mem.shape[1] != 2 + 2 * dl.shape[1] or dl.shape[1] == 0:
            raise ValueError("members must be [G, 2 + 2 K] and delta [G, K] for G groups and K >= 1 parameters")
        if mem.shape[0] == 0:
            return self.tran_clear_sens()
        spec = SensSpecC(mem.shape[0], dl.shape[1], _ip(mem), _dp(dl), 4 if max_order >= 3 else 3, int(n_save), self.st.n if n_obs is None else int(n_obs))
        _check(self.lib.cadnip_tran_set_sens(self.h, C.byref(spec)), "cadnip_tran_set_sens")

    def tran_clear_sens(self):
        """cadnip_tran_set_sens with no spec: ``tran_run`` is again exactly what it is on a new handle."""
        _check(self.lib.cadnip_tran_set_sens(self.h, None), "cadnip_tran_set_sens")

    def tran_sens_init(self, zero=False):
        """cadnip_tran_sens_init: s(t0) of every group -- zeros with ``zero`` (the start state was given), else -G^-1 d(G u - b)/dp at the
        handle's current state, an operating point (call it after the tranop ``dc_run``, before the mode is switched)."""
        _check(self.lib.cadnip_tran_sens_init(self.h, C.c_int32(1 if zero else 0)), "cadnip_tran_sens_init")

    def tran_sens_info(self):
        """cadnip_tran_sens_info: {n_group, K, per (members of a group), nh, n_save, n_obs} of the spec in force (zeros without one)."""
        out = (C.c_int32 * 6)()
        _check(self.lib.cadnip_tran_sens_info(self.h, out), "cadnip_tran_sens_info")
        return dict(zip(("n_group", "K", "per", "nh", "n_save", "n_obs"), (int(x) for x in out)))

    def tran_sens_get(self):
        """cadnip_tran_sens_get: (s [G, K, n_save, n_obs], flags [G]) of the last ``tran_run``; flag 1: a solve of the group met a bad pivot
        or a non-finite value, its sensitivities are NaN from that step on."""
        i = self.tran_sens_info()
        s = np.zeros((i["n_group"], i["K"], i["n_save"], i["n_obs"]))
        fl = np.zeros(max(i["n_group"], 1), dtype=np.int32)
        _check(self.lib.cadnip_tran_sens_get(self.h, _dp(s) if s.size else None, _ip(fl)), "cadnip_tran_sens_get")
        return s, fl[:i["n_group"]]

    def tran_state(self):
        t, hh, o = np.empty(self.B), np.empty(self.B), np.empty(self.B, dtype=np.int32)
        _check(self.lib.cadnip_tran_state(self.h, _dp(t), _dp(hh), _ip(o)), "cadnip_tran_state")
        return t, hh, o

    # -- misc ------------------------------------------------------------------------------------
    def set_u(self, u):
        _check(self.lib.cadnip_set_u(self.h, _dp(self._bn(u))), "cadnip_set_u")

    def get_u(self):
        u = np.empty((self.B, self.st.n))
        _check(self.lib.cadnip_get_u(self.h, _dp(u)), "cadnip_get_u")
        return u

    def debug_copy(self, n_doubles, reps=1):
        _check(self.lib.cadnip_debug_copy(self.h, C.c_int64(n_doubles), C.c_int32(reps)), "cadnip_debug_copy")

    def stamp_time(self, block=-1, reps=20):
        """Milliseconds of ``reps`` back-to-back launches of one block's stamping kernel (block < 0: the whole restamp)."""
        ms = C.c_double()
        _check(self.lib.cadnip_debug_stamp_time(self.h, C.c_int32(block), C.c_int32(reps), C.byref(ms)), "cadnip_debug_stamp_time")
        return ms.value

    def profile(self, on=True):
        _check(self.lib.cadnip_profile_enable(self.h, C.c_int32(1 if on else 0)), "cadnip_profile_enable")

    def profile_read(self):
        names = (C.c_char_p * 64)()
        ms = (C.c_double * 64)()
        calls = (C.c_int64 * 64)()
        k = self.lib.cadnip_profile_read(self.h, C.c_int32(64), names, ms, calls)
        return {names[i].decode(): (ms[i], calls[i]) for i in range(k)}


def _stats(st):
    return {f: getattr(st, f) for f, _ in RunStatsC._fields_}


LU_ARRAYS = ("rperm", "cperm", "rowptr", "col", "diag", "load_src", "load_dst", "ent_pos", "ent_diag", "ent_ptr",
             "term_a", "term_b", "lev_ptr", "fwd_rows", "fwd_lev_ptr", "bwd_rows", "bwd_lev_ptr")
# host_lu_analyze(..., transpose=True): the transposed-solve tables (csrc/lu_transpose.hpp), CADNIP_LUT_COLPTR onwards
LUT_ARRAYS = ("t_colptr", "t_pos", "t_row", "t_diag", "ut_rows", "ut_lev_ptr", "lt_rows", "lt_lev_ptr", "a_colptr", "a_row", "a_pos")
LUT_FIRST = 32


F2_ARRAYS = (("posW", np.int32), ("lanes", np.uint64), ("passes", np.uint64), ("terms", np.uint32), ("meta", np.int32))


def leaves_of(st):
    """(q_begin, lim_begin, unit_ok) of a Structure: the leaf-first pivot order a handle built from it uses (csrc/api.hip: cadnip_create)."""
    q0, l0 = st.n_nodes + st.n_currents, st.n - st.n_limits
    ok = np.zeros(st.n, dtype=np.uint8)
    rows = np.repeat(np.arange(st.n), np.diff(st.rowptr))
    for e in np.flatnonzero((rows == np.asarray(st.colidx)) & (rows >= q0)):
        ok[rows[e]] = 1 if (st.g_ptr[e + 1] - st.g_ptr[e] == 1 and st.c_ptr[e + 1] == st.c_ptr[e]) else 0
    return q0, l0, ok


def host_lu_analyze(n, rowptr, colidx, vals, pivot_tol=1e-3, sample=False, f2_nc=None, leaves=None, order=None, transpose=False):
    """Host-only symbolic phase (no GPU needed): returns the LU program as a dict of int32 arrays.  ``leaves``: ``leaves_of(st)`` for
    the pivot order of a handle (device-local unknowns first), None for the plain Markowitz search.  ``order``: "klu" | "markowitz" forces
    the ordering (csrc/symbolic.cpp: default Markowitz up to 4 096 unknowns, KLU's block triangular form + minimum degree beyond);
    ``out["n_blocks"]`` = diagonal blocks found (0 with the Markowitz search).  ``transpose``: also the tables of the transposed solve
    through the same factors (``LUT_ARRAYS``: the column view of L\\U, the level schedules of U^T and L^T, the column view of the pattern)."""
    if order is not None:
        prev = os.environ.get("CADNIP_LU_ORDER")
        os.environ["CADNIP_LU_ORDER"] = order
        try:
            return host_lu_analyze(n, rowptr, colidx, vals, pivot_tol, sample, f2_nc, leaves, transpose=transpose)
        finally:
            if prev is None:
                os.environ.pop("CADNIP_LU_ORDER", None)
            else:
                os.environ["CADNIP_LU_ORDER"] = prev
    lib = load_library()
    rp = np.ascontiguousarray(rowptr, dtype=np.int32)
    ci = np.ascontiguousarray(colidx, dtype=np.int32)
    v = np.ascontiguousarray(vals, dtype=np.float64)
    p = C.c_void_p()
    if leaves is None or os.environ.get("CADNIP_LU_NOLEAF"):
        _check(lib.cadnip_host_lu_analyze(C.c_int32(n), _ip(rp), _ip(ci), _dp(v), C.c_double(pivot_tol), C.c_int32(int(sample)), C.byref(p)),
               "cadnip_host_lu_analyze")
    else:
        ok = np.ascontiguousarray(leaves[2], dtype=np.uint8)
        _check(lib.cadnip_host_lu_analyze_leaves(C.c_int32(n), _ip(rp), _ip(ci), _dp(v), C.c_double(pivot_tol), C.c_int32(int(sample)),
                                                 C.c_int32(int(leaves[0])), C.c_int32(int(leaves[1])), ok.ctypes.data_as(C.c_void_p), C.byref(p)),
               "cadnip_host_lu_analyze_leaves")
    out = {}
    try:
        for k, nm in enumerate(LU_ARRAYS):
            sz = lib.cadnip_host_lu_size(p, C.c_int32(k))
            a = np.zeros(max(sz, 1), dtype=np.int32)
            _check(lib.cadnip_host_lu_get(p, C.c_int32(k), _ip(a)), "cadnip_host_lu_get")
            out[nm] = a[:sz]
        lib.cadnip_host_lu_blocks.restype = C.c_int32
        out["n_blocks"] = int(lib.cadnip_host_lu_blocks(p))
        if transpose:
            _check(lib.cadnip_host_lu_transpose(p), "cadnip_host_lu_transpose")
            for k, nm in enumerate(LUT_ARRAYS):
                sz = lib.cadnip_host_lu_size(p, C.c_int32(LUT_FIRST + k))
                a = np.zeros(max(sz, 1), dtype=np.int32)
                _check(lib.cadnip_host_lu_get(p, C.c_int32(LUT_FIRST + k), _ip(a)), "cadnip_host_lu_get")
                out[nm] = a[:sz]
        if f2_nc is not None:
            ts = (C.c_int32 * 4)()
            out["team_steps"] = {}
            for nw in (1, 2, 4):
                if lib.cadnip_host_f2_team_steps(p, C.c_int32(int(f2_nc)), C.c_int32(nw), ts) == 0:
                    out["team_steps"][nw] = tuple(int(v) for v in ts)
            # ... as straight-line steps: "steps" = {nw: (counts, uint64 descriptor words)}; nw = 1 is the sweep kernel's three-term layout
            out["steps"] = {}
            for nw in (1, 2, 4, 12, 14):
                if lib.cadnip_host_f2_steps(p, C.c_int32(int(f2_nc)), C.c_int32(nw), ts, None) == 0:
                    words = np.zeros(max(int(ts[3]), 1), dtype=np.uint64)
                    _check(lib.cadnip_host_f2_steps(p, C.c_int32(int(f2_nc)), C.c_int32(nw), ts, words.ctypes.data_as(C.c_void_p)), "cadnip_host_f2_steps")
                    out["steps"][nw] = (tuple(int(v) for v in ts[:3]), words[:int(ts[3])])
            # the fused kernel's entry program for this LU and core size (csrc/f2_program.cpp)
            lib.cadnip_host_f2_free.restype = None
            q = C.c_void_p()
            _check(lib.cadnip_host_f2_build(p, C.c_int32(int(f2_nc)), C.byref(q)), "cadnip_host_f2_build")
            try:
                f2 = {}
                for k, (nm, dt) in enumerate(F2_ARRAYS):
                    sz = lib.cadnip_host_f2_size(q, C.c_int32(k))
                    a = np.zeros(max(sz, 1), dtype=dt)
                    _check(lib.cadnip_host_f2_get(q, C.c_int32(k), a.ctypes.data_as(C.c_void_p)), "cadnip_host_f2_get")
                    f2[nm] = a[:sz]
                out["f2"] = f2
            finally:
                lib.cadnip_host_f2_free(q)
    finally:
        lib.cadnip_host_lu_free(p)
    return out
