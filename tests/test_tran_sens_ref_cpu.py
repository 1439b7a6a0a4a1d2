"""Transient parameter sensitivities, the parts that need no GPU:

(a) the two references of tests/tran_sens_ref.py -- ``trajectory_derivative`` (the definition) and ``direct_dense`` (the method) -- against
    the closed-form derivative of the backward-Euler recursion of the RC circuit, with respect to R, C and V;
(b) for every case of tests/tran_sens_cases.py the reference's own uncertainty (``U_REF``), the distance of the method from the definition
    (``T_CASE``) and what double arithmetic costs the method (``AMP``): measured <= recorded in tran_sens_ref.py; and T_CASE, as the
    truncation of the central difference in the parameter, falling by about 4 when the step halves;
(c) csrc/tran_sens_plan.hpp compiled with the host compiler: BDF coefficients, save-point weights, the checks of a group table;
(d) everything ``api.tran(..., sens=)`` refuses, before any device work.

(b), measured (worst over the first and last instance, every order): rc U_REF 1.45e-10, T_CASE 8.6e-9 -> 2.2e-9 at half the step;
linear_zoo 6.7e-12, 5.7e-10 -> 1.4e-10; inverter 1.87e-10, 1.46e-8 -> 3.6e-9.  Without the method's defect pass the inverter's figure
was 2.68e-6 at both steps, in the supply current alone: G + a0 C is not the Jacobian of F where a voltage-dependent capacitance sits in C
(tran_sens_ref.py has the details)."""
import ctypes
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import cadnip_jl_amd as cj
from cadnip_jl_amd import api
from tests import tran_exact_cases as X
from tests import tran_ref as TR
from tests import tran_sens_cases as K
from tests import tran_sens_ref as SR
from tests.test_lds_layout import CSRC


# ---- (a) RC closed form ---------------------------------------------------------------------------------------------------------------------
def test_both_references_match_the_closed_form_of_backward_euler_on_rc():
    case = K.CASES["rc"]
    grid, orders = case.schedule(1)
    # a trajectory is known to Newton's stop, 1e-13 (1 + |u|); a scaled central difference divides the difference of two by 2 rel_step, and
    # Richardson takes (4 x the half-step difference, whose noise is twice as large, + the full-step one) / 3: three times the noise
    def_tol = 3.0 * (2.0 * TR.NEWTON_RTOL * (1.0 + case.umax)) / (2.0 * SR.REL_STEP)
    for i in range(len(case.points)):
        pt = [case.points[i]]
        _, dR, dC, dV = K.be_closed_form(pt, grid)
        exact = np.array([dR[0], dC[0], dV[0]]).astype(float)
        j = TR.Equations(case.make(), case.params(i)).index_of("out")
        sc = K.scales_of("rc", i)[:, None]
        e_def = float(X.rel_err(K.definition("rc", 1, i)[:, :, j] * sc, exact * sc).max())
        # F is linear in C and in V: the method's central differences in them are exact.  In R it is linear in 1 / R, whose central
        # difference is off by rel_step^2: the recorded truncation of the case
        e_dir = X.rel_err(K.direct("rc", 1, i)[:, :, j] * sc, exact * sc).max(axis=1)
        print("rc instance %d: definition against the closed form %.2e (bound %.1e), method R %.2e, C %.2e, V %.2e" % ((i, e_def, def_tol) + tuple(e_dir)))
        assert e_def <= def_tol
        assert e_dir[0] <= SR.T_CASE["rc"] and e_dir[1] <= X.REL_TOL_PORT and e_dir[2] <= X.REL_TOL_PORT


# ---- (b) reference uncertainty ----------------------------------------------------------------------------------------------------------------
def _ends(case):
    return [case.checked[0], case.checked[-1]]


def _figures(name):
    """(U_ref, T_case, T_case at half the step, AMP): worst over the first and last checked instance and every order"""
    case = K.CASES[name]
    u = t = th = amp = 0.0
    for order in case.orders:
        for i in _ends(case):
            r12, r24 = K.definition(name, order, i, SR.REL_STEP, True)
            S = K.direct(name, order, i)
            u = max(u, K.scaled_err(name, i, r24, r12))
            t = max(t, K.scaled_err(name, i, S, r12))
            th = max(th, K.scaled_err(name, i, K.direct(name, order, i, SR.LD, SR.REL_STEP / 2), r24))
            amp = max(amp, K.scaled_err(name, i, K.direct(name, order, i, float), S))
    print("%s: U_ref %.3e  T_case %.3e  at half the step %.3e (ratio %.2f)  AMP %.3e" % (name, u, t, th, t / th, amp))
    return u, t, th, amp


_FIG = {}


def figures(name):
    if name not in _FIG:
        _FIG[name] = _figures(name)
    return _FIG[name]


@pytest.mark.parametrize("name", list(K.CASES))
def test_measured_reference_figures_stay_inside_the_recorded_ones(name):
    u, t, _, amp = figures(name)
    assert u <= SR.U_REF[name]
    assert t <= SR.T_CASE[name]
    assert amp <= SR.AMP[name]
    assert SR.AMP[name] <= X.REL_TOL_GPU        # ... so tests/test_gpu_tran_sens.py keeps the project's bound


@pytest.mark.parametrize("name", list(K.CASES))
def test_truncation_falls_by_four_when_the_step_halves(name):
    _, t, th, _ = figures(name)
    assert 3.0 <= t / th <= 5.0, (name, t, th)


# ---- (c) the plan header ------------------------------------------------------------------------------------------------------------------------
SHIM = r"""
#include "tran_sens_plan.hpp"
using namespace cadnip;
extern "C" {
void t_alphas(int order, double h, double hprev, double hpp, double* al) { sens_bdf_alphas(order, h, hprev, hpp, al); }
void t_weights(int nhist, double told, double tn, double hprev, double ts, double* w) { sens_out_weights(nhist, told, tn, hprev, ts, w); }
int t_check(int B, int n, int G, int K, const int* members, const double* delta, int nh, int n_save, int n_obs) {
  return sens_spec_check(B, n, G, K, members, delta, nh, n_save, n_obs);
}
int t_layout(int K, int k, int* out) { out[0] = sens_group_size(K); out[1] = sens_plus(k); out[2] = sens_minus(k); return SENS_TWIN - SENS_BASE; }
}
"""


@pytest.fixture(scope="module")
def L(tmp_path_factory):
    d = tmp_path_factory.mktemp("tran_sens_plan")
    src, lib = str(d / "shim.cpp"), str(d / "libshim.so")
    with open(src, "w") as f:
        f.write(SHIM)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", "-I", CSRC, "-o", lib, src])
    lib = ctypes.CDLL(lib)
    lib.t_alphas.argtypes = [ctypes.c_int] + [ctypes.c_double] * 3 + [ctypes.c_void_p]
    lib.t_weights.argtypes = [ctypes.c_int] + [ctypes.c_double] * 4 + [ctypes.c_void_p]
    lib.t_check.argtypes = [ctypes.c_int] * 4 + [ctypes.c_void_p] * 2 + [ctypes.c_int] * 3
    return lib


def _ulps(got, ref):
    return np.abs(np.asarray(got) - np.asarray(ref)) / np.spacing(np.abs(np.asarray(ref)))


def test_plan_alphas_are_the_textbook_bdf_coefficients(L):
    """the closed forms against the Lagrange definition in exact rational arithmetic: each is at most eight rounded operations deep"""
    rng = np.random.default_rng(7)
    al = np.zeros(4)
    for _ in range(300):
        h, hprev, hpp = (float(x) for x in 10.0 ** rng.uniform(-12, -3) * rng.uniform(0.2, 5.0, size=3))
        fh, fp, fpp = Fraction(h), Fraction(hprev), Fraction(hpp)              # the grid the three step sizes span, exactly
        nodes = [Fraction(0), -fh, -(fh + fp), -(fh + fp + fpp)]
        for order in (1, 2, 3):
            L.t_alphas(order, h, hprev, hpp, al.ctypes.data)
            ref = TR.bdf_alphas(nodes[:order + 1])
            assert np.all(_ulps(al[:order + 1], ref) <= 8), (order, h, hprev, hpp, al, ref)
            assert np.all(al[order + 1:] == 0.0)
    L.t_alphas(0, 1.0, 1.0, 1.0, al.ctypes.data)
    assert np.all(al == 0.0)


def test_plan_save_weights_are_the_lagrange_values(L):
    rng = np.random.default_rng(8)
    w = np.zeros(3)
    for _ in range(300):
        told = float(rng.uniform(0.0, 1e-3))
        h, hprev = (float(x) for x in rng.uniform(1e-7, 1e-5, size=2))
        tn = told + h
        for ts in (tn, told + 0.25 * h, told + 0.8 * h):
            L.t_weights(3, told, tn, hprev, ts, w.ctypes.data)
            ref = np.array([float(x) for x in TR.lagrange_values([tn, told, told - hprev], ts)])
            # the weights are products of differences of times near 1e-3: a difference of size d carries an absolute error of ulp(1e-3)
            assert np.all(np.abs(w - ref) <= 16 * np.spacing(1e-3) / min(h, hprev) * np.maximum(np.abs(ref), 1.0)), (told, h, hprev, ts, w, ref)
            L.t_weights(1, told, tn, hprev, ts, w.ctypes.data)
            ref = np.array([float(x) for x in TR.lagrange_values([tn, told], ts)])
            assert np.all(np.abs(w[:2] - ref) <= 16 * np.spacing(1e-3) / h) and w[2] == 0.0
    L.t_weights(3, 1.0, 2.0, 0.5, 2.0, w.ctypes.data)
    assert np.array_equal(w, [1.0, 0.0, 0.0])       # a save time on the grid point is that point


def test_plan_checks_the_group_table(L):
    OK, SHAPE, INDEX, TWICE, DELTA, LARGE = range(6)
    out = (ctypes.c_int * 3)()
    assert L.t_layout(3, 2, out) == 1 and list(out) == [8, 6, 7]
    mem = np.arange(12, dtype=np.int32).reshape(2, 6)
    dl = np.full((2, 2), 1e-3)

    def check(B=12, n=5, G=2, K=2, members=mem, delta=dl, nh=3, n_save=10, n_obs=5):
        members, delta = np.ascontiguousarray(members, dtype=np.int32), np.ascontiguousarray(delta, dtype=np.float64)
        return L.t_check(B, n, G, K, members.ctypes.data, delta.ctypes.data, nh, n_save, n_obs)

    assert check() == OK and check(nh=4) == OK and check(n_save=0) == OK
    assert check(nh=2) == SHAPE and check(K=0) == SHAPE and check(G=0) == SHAPE and check(n_obs=0) == SHAPE and check(n_obs=6) == SHAPE
    assert check(B=11) == INDEX
    bad = mem.copy()
    bad[0, 1] = -1
    assert check(members=bad) == INDEX
    bad = mem.copy()
    bad[1, 5] = 0
    assert check(members=bad) == TWICE
    for v in (0.0, -1e-3, np.inf, np.nan):
        bad = dl.copy()
        bad[1, 1] = v
        assert check(delta=bad) == DELTA
    # 8 G K (nh n + n_save n_obs) bytes against 256 MiB
    assert check(n=1 << 20, n_obs=1, n_save=1 << 20) == OK             # 8 * 4 * (3 + 1) * 2^20 = 128 MiB
    assert check(n=1 << 20, n_obs=1, n_save=5 << 20) == OK             # 256 MiB exactly
    assert check(n=1 << 20, n_obs=1, n_save=(5 << 20) + 1) == LARGE
    assert check(n=1 << 30, n_obs=1 << 30, n_save=1 << 30) == LARGE    # no overflow on the way


# ---- (d) refusals, before any device work -----------------------------------------------------------------------------------------------------
@pytest.fixture
def no_device(monkeypatch):
    class Stub:
        def __init__(self, *a, **k):
            raise AssertionError("device work before the refusal")
    monkeypatch.setattr(api, "BatchSimulator", Stub)


def _rc():
    return api.MNACircuit(K.rc_param(), K.RC_DEFAULTS)


@pytest.mark.parametrize("sens", [[], ["R", "R"], ["nope"], ["R", "Temp"]], ids=["empty", "twice", "unknown", "unknown-case"])
def test_bad_names_are_value_errors(no_device, sens):
    with pytest.raises(ValueError):
        api.tran(_rc(), (0.0, 1e-3), sens=sens)
    with pytest.raises(ValueError):
        api.tran(api.CircuitSweep(_rc(), api.Sweep(R=[1e3, 2e3])), (0.0, 1e-3), sens=sens)


def test_a_step_that_is_not_positive_is_a_value_error(no_device):
    with pytest.raises(ValueError):
        api.tran(_rc(), (0.0, 1e-3), sens=["R"], sens_rel_step=0.0)


@pytest.mark.parametrize("delays", ["refuse", "history"])
def test_a_delayed_element_is_refused(no_device, delays):
    c = K.rc_param()
    c.E("e1", "x", "0", "out", "0", 1.0, delay=1e-6)
    c.R("rx", "x", "0", 1e3)
    with pytest.raises(NotImplementedError):
        api.tran(api.MNACircuit(c, K.RC_DEFAULTS), (0.0, 1e-3), sens=["R"], delays=delays)


def test_a_behavioural_source_is_refused(no_device):
    c = K.rc_param()
    c.BI("b1", "out", "0", "1e-6 * V(out)")
    with pytest.raises(NotImplementedError, match="b1"):
        api.tran(api.MNACircuit(c, K.RC_DEFAULTS), (0.0, 1e-3), sens=["R"])


def test_a_step_across_a_structure_class_names_the_parameter(no_device):
    """sp_mos1's rd at 0: the drain node is collapsed; rd = +-delta brings it back (tests/test_sensitivity_cpu.py)"""
    circ = cj.Circuit("rd at zero")
    circ.V("vd", "d", "0", dc=2.0)
    circ.V("vg", "g", "0", dc=cj.Param("vg"))
    circ.MOS1("m1", "d", "g", "0", "0", dict(type=1, vto=0.7, kp=100e-6, rd=cj.Param("rd")), w=10e-6, l=1e-6)
    with pytest.raises(ValueError, match="rd"):
        api.tran(api.MNACircuit(circ, {"rd": 0.0, "vg": 1.5}), (0.0, 1e-6), sens=["vg", "rd"])


def test_a_step_that_moves_a_break_point_is_a_value_error(no_device, monkeypatch):
    """no waveform takes a parameter today: the comparison is driven through the function that lists a point's break points"""
    real = api.sens_breaks
    monkeypatch.setattr(api, "sens_breaks", lambda mc, pt, tspan: real(mc, pt, tspan) + [1e-4 * pt.get("C", 1e-6) / 1e-6])
    with pytest.raises(ValueError, match="break point"):
        api.tran(api.MNACircuit(K.rc_pulse(), K.RC_DEFAULTS), (0.0, 2e-3), sens=["C"])
    api.sens_prepare(api.MNACircuit(K.rc_pulse(), K.RC_DEFAULTS), [{}], ["R"], 1e-4, (0.0, 2e-3))      # R does not move it: accepted


def test_the_expansion_is_the_one_of_sensitivity():
    mc = api.MNACircuit(bm_inverter(), {"vdd": 5.0})
    pts = [{"vdd": 4.5, "temp": 85.0}, {"vdd": 0.0}]
    v, d, ex, per = api.sens_expand(mc, pts, ["vdd", "temp"], 1e-4)
    assert per == 5 and len(ex) == 10 and ex[0] == pts[0] and ex[5] == pts[1]
    assert np.array_equal(v, [[4.5, 85.0], [0.0, 27.0]])
    assert np.array_equal(d, [[1e-4 * 4.5, 1e-4 * (85.0 + 273.15)], [1e-4, 1e-4 * (27.0 + 273.15)]])
    assert ex[1]["vdd"] == 4.5 + d[0, 0] and ex[2]["vdd"] == 4.5 - d[0, 0] and ex[3]["temp"] == 85.0 + d[0, 1] and ex[4]["temp"] == 85.0 - d[0, 1]
    v2, d2, ex2, per2 = api.sens_expand(mc, pts, ["vdd", "temp"], 1e-4, twin=True)
    assert per2 == 6 and np.array_equal(d2, d) and ex2[0] == ex2[1] == pts[0] and ex2[2:6] == ex[1:5] and ex2[6] == ex2[7] == pts[1]


def bm_inverter():
    from cadnip_jl_amd import benchmarks as bm
    return bm.inverter_circuit()
