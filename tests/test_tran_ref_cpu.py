"""The textbook transient reference (tests/tran_ref.py) against closed forms, and the CPU port (oracle/cpu_port.cpp) against the reference on
the forced step grids of tests/tran_exact_cases.py.  No GPU.

The first half shows that the reference is what it claims to be: its coefficients differentiate polynomials exactly on any grid, and on
uniform grids its global error falls by 2, 4 and 8 per halving of the step at orders 1, 2 and 3.  The second half shows that the inputs
chosen for the GPU test (tests/test_gpu_tran_exact.py) keep the reference's own side clean: the port, whose controller mirrors the
product's operation for operation, takes exactly the scheduled steps and lands within 1e-10 of the reference, ten times inside the GPU
bound.  Measured here: 1e-15 .. 4e-15 in Newton mode 0 (every case), up to 1.1e-11 in mode 1 on its own windows."""
import math
from fractions import Fraction

import numpy as np
import pytest

import cadnip_jl_amd as cj
from tests import tran_exact_cases as X
from tests import tran_ref as TR
from tests.port_util import make_port, analyze_port


# ---- the reference is textbook ------------------------------------------------------------------------------------------------------------
def test_schedule_is_the_three_line_rule():
    grid, orders = TR.schedule(0.25, 2.0 ** -10, 2.0 ** -7, 9, 3)
    h = np.diff(grid)
    assert list(h / 2.0 ** -10) == [1, 2, 4, 8, 8, 8, 8, 8, 8] and grid[0] == 0.25
    assert list(orders) == [1, 1, 2, 3, 3, 3, 3, 3, 3]
    assert list(TR.schedule(0.0, 1.0, 1.0, 5, 2)[1]) == [1, 1, 2, 2, 2] and list(TR.schedule(0.0, 1.0, 1.0, 4, 1)[1]) == [1, 1, 1, 1]


def test_coefficients_on_a_uniform_grid_are_the_tabulated_ones():
    h = 0.125
    for k, tab in ((1, [1, -1]), (2, [Fraction(3, 2), -2, Fraction(1, 2)]), (3, [Fraction(11, 6), -3, Fraction(3, 2), Fraction(-1, 3)])):
        al = TR.lagrange_derivatives([1.0 - j * h for j in range(k + 1)], 1.0)
        assert al == [Fraction(c) / Fraction(h) for c in tab], k


@pytest.mark.parametrize("k", [1, 2, 3])
def test_coefficients_differentiate_polynomials_exactly_on_a_variable_grid(k):
    """The defining property of the order-k formula on ANY grid: exact for polynomials up to degree k, not for degree k + 1."""
    times = [Fraction(7, 8), Fraction(13, 16), Fraction(5, 8), Fraction(9, 32)][:k + 1]       # ratios 1 : 3 : 5.5
    al = TR.lagrange_derivatives([float(t) for t in times], float(times[0]))
    for deg in range(k + 2):
        got = sum(a * t ** deg for a, t in zip(al, times))
        want = deg * times[0] ** (deg - 1) if deg else 0
        assert (got == want) == (deg <= k), (k, deg)
    vals = TR.lagrange_values([float(t) for t in times], 0.5)
    assert sum(vals) == 1 and sum(v * t ** k for v, t in zip(vals, times)) == Fraction(1, 2) ** k


def _rc():
    c = cj.Circuit()
    c.V("v1", "vin", "0", dc=5.0)
    c.R("r1", "vin", "out", 1e3)
    c.C("c1", "out", "0", 1e-6)

    def exact(eq, t):
        u = np.zeros(eq.n)
        u[eq.index_of("vin")] = 5.0
        u[eq.index_of("out")] = 5.0 * (1.0 - math.exp(-t / 1e-3))
        return u
    return c, exact, ["out"], 1e-3


def _rlc():
    """Series R L C, the capacitor charged to 1 V, no source: v_C = e^(-a t) (cos wd t + a / wd sin wd t), i = e^(-a t) sin(wd t) / (L wd)."""
    R, L, C = 10.0, 1e-3, 1e-6
    c = cj.Circuit()
    c.C("c1", "a", "0", C)
    c.R("r1", "a", "b", R)
    c.L("l1", "b", "0", L)
    a, w0 = R / (2 * L), 1.0 / math.sqrt(L * C)
    wd = math.sqrt(w0 * w0 - a * a)

    def exact(eq, t):
        u = np.zeros(eq.n)
        v = math.exp(-a * t) * (math.cos(wd * t) + a / wd * math.sin(wd * t))
        i = math.exp(-a * t) * math.sin(wd * t) / (L * wd)
        u[eq.index_of("a")], u[eq.index_of("b")], u[eq.index_of("I_l1")] = v, v - R * i, i      # the branch current flows from b to ground
        return u
    return c, exact, ["a", "I_l1"], 1e-4


def _rc_sin():
    """R C driven by sin(w t) from v = 0: v = A sin w t + B (cos w t - e^(-t / tau)), A = 1 / (1 + (w tau)^2), B = -w tau A."""
    tau, f = 1e-3, 500.0
    w = 2 * math.pi * f
    c = cj.Circuit()
    c.V("v1", "vin", "0", dc=0.0, wave=("sin", 0.0, 1.0, f, 0.0, 0.0, 0.0))
    c.R("r1", "vin", "out", 1e3)
    c.C("c1", "out", "0", 1e-6)
    A = 1.0 / (1.0 + (w * tau) ** 2)
    B = -w * tau * A

    def exact(eq, t):
        u = np.zeros(eq.n)
        u[eq.index_of("vin")] = math.sin(w * t)
        u[eq.index_of("out")] = A * math.sin(w * t) + B * (math.cos(w * t) - math.exp(-t / tau))
        return u
    return c, exact, ["out"], 1e-3


PROBLEMS = {"rc": _rc, "rlc": _rlc, "rc_sin": _rc_sin}
STEPS = {1: 400, 2: 100, 3: 50}      # steps of the coarsest grid: asymptotic (ratios within a few per cent of 2^k), errors 1e-3 .. 1e-9 of the signal


@pytest.mark.parametrize("k", [1, 2, 3])
@pytest.mark.parametrize("problem", list(PROBLEMS))
def test_global_error_falls_with_the_order(problem, k):
    """Uniform grids h, h / 2, h / 4 over the same interval, order k throughout, the first k points from the closed form (the textbook's
    exact starting values: start-up steps of lower order would leave an O(h^2) term that never leaves a third-order error): the error at
    the end of the interval falls by 2^k per halving, within 15 %."""
    circ, exact, names, T = PROBLEMS[problem]()
    eq = TR.Equations(circ, {})
    idx = [eq.index_of(nm) for nm in names]
    errs = []
    for N in (STEPS[k], 2 * STEPS[k], 4 * STEPS[k]):
        grid, _ = TR.schedule(0.0, T / N, T / N, N, k)
        start = np.array([exact(eq, t) for t in grid[:k]])
        tr = TR.integrate(eq, None, grid, np.full(N, k), start=start)
        ref = exact(eq, grid[-1])
        scale = np.maximum(np.abs(ref[idx]), 1e-3 * np.max(np.abs(tr.U[:, idx]), axis=0))
        errs.append(float(np.max(np.abs(tr.U[-1, idx] - ref[idx]) / scale)))
    ratios = [errs[0] / errs[1], errs[1] / errs[2]]
    print(problem, "order", k, "errors", errs, "ratios", ratios)
    assert errs[2] > 1e-10                                   # still above rounding
    for r in ratios:
        assert abs(r / 2.0 ** k - 1.0) <= 0.15, (problem, k, errs, ratios)


def test_interpolant_is_linear_in_step_one_and_quadratic_after():
    tr = TR.Trajectory(np.array([0.0, 1.0, 3.0, 7.0]), np.array([1, 1, 2]), np.array([[1.0], [2.0], [10.0], [50.0]]), None)
    assert tr.at(0.0)[0] == 1.0 and tr.at(0.25)[0] == 1.25 and tr.at(1.0)[0] == 2.0          # the straight line through (0, 1), (1, 2)
    # step 2: the parabola through (0, 1), (1, 2), (3, 10) is 1 + t^2;  step 3: through (1, 2), (3, 10), (7, 50) it is 1 + t^2 too
    assert tr.at(2.0)[0] == 5.0 and tr.at(3.0)[0] == 10.0 and tr.at(5.0)[0] == 26.0 and tr.at(7.0)[0] == 50.0
    assert [tr.step_of(t) for t in (0.0, 0.5, 1.0, 1.5, 3.0, 6.9)] == [1, 1, 1, 2, 2, 3]


# ---- the port follows the reference on the forced schedule ---------------------------------------------------------------------------
def _port_modes(case):
    # Newton mode 1 of the fused kernels is the port's mode 1 (Jacobian reuse); the per-op path's mode 1 is the port's mode 2 (same test,
    # a refactorisation every round)
    return (1, 2) if case.mode else (0,)


@pytest.mark.parametrize("name,order", [(c.name, k) for c in X.CASES.values() for k in c.orders])
def test_port_follows_the_reference_on_the_forced_schedule(name, order):
    case = X.CASES[name]
    ts, on = case.save_times()
    assert (~on).sum() == 4 and case.tau <= 1e-11 and case.n_steps * 0.33 * case.tau * (1.0 + case.umax) <= 1e-10 * (1 + 1e-12)
    assert case.n_steps <= (64 if name.startswith("dff") else 160)
    worst = {}
    for i in case.checked:
        ref = X.reference(name, order, i)
        R = ref.sample(ts)
        assert list(ref.orders[:4]) == [1, 1, min(order, 2), order] and ref.grid[-1] == case.t1
        st, port = make_port(case.make(), case.params(i), case.temp(i), "tran")
        assert st.n == R.shape[1] and [st.index_of(nm) for nm in ref.names] == list(range(len(ref.names)))      # same unknowns, same order
        analyze_port(st, port, 5.0)
        for pm in _port_modes(case):
            out, _, stats, _ = port.tran(X.start_state(case, i), case.t0, case.t1, case.tau, case.tau, breaks=(), save_t=ts, obs=None,
                                         err_mask=np.zeros(st.n), h0=case.h0, hmax=case.hmax, max_newton=case.max_newton, max_order=order,
                                         use_pcnr=False, newton_tol=1.0, newton_mode=pm, step_rule=0)
            assert stats["status"] == 1
            assert (stats["accepted"], stats["rejected"], stats["newton_failures"]) == (case.n_steps, 0, 0), (name, order, i, pm, stats)
            e = X.rel_err(out, R)
            worst[pm] = max(worst.get(pm, 0.0), float(e.max()))
            assert e[on].max() <= X.REL_TOL_PORT, (name, order, i, pm, e[on].max())
            assert e[~on].max() <= X.REL_TOL_PORT, (name, order, i, pm, e[~on].max(axis=1))
        port.close()
        assert float(np.max(np.abs(ref.U - ref.U[0]))) > 1e-3            # the trajectory moves: a wrong coefficient would show
    print(name, "order", order, "worst error per port Newton mode", worst)
