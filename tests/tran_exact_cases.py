"""The cases of the forced-grid transient pins (tests/test_tran_ref_cpu.py: CPU port against tests/tran_ref.py; tests/test_gpu_tran_exact.py:
every GPU launch path against it): circuits, corners, grids, save times, tolerances -- and the reference trajectories, computed once
per process and shared by both files.

Every run switches the step controller's decisions off (``err_mask`` all zero: no error test, every converged step is accepted and the
next one is min(2 h, hmax); ``breaks=()``: nothing restarts the order), so the step grid is known in advance (tran_ref.schedule) and
what is compared is the discretisation, the stamps inside the time loop, the linear solve and the Newton iteration.

* h0 = 2^-p, hmax = 2^m h0, t0 = k0 hmax: every grid time is an exact double; t1 is the last scheduled grid point, so the controller's
  clipping at the end of the interval never halves a step.
* abstol = reltol = tau, newton_tol = 1: Newton mode 0 stops on a weighted update norm below 1, about tau (1 + |u|) per step; tau is chosen
  with n_steps 0.33 tau (1 + max|u|) <= 1e-10, a tenth of the GPU bound, and tau <= 1e-11.
* save times: every grid point, plus off-grid times at fractions 0.25 / 0.25 / 0.5 / 0.8 of a step: inside step 1 (only two points
  exist: the straight line), inside step 2 (the first quadratic), in the doubling phase and in the constant-step phase.

Windows.  The nonlinear circuits start from their DC point at a t0 before the first source edge (the sources are constant up to it, so
the DC point IS the state at t0) with steps small enough for Newton to cross the edge on the forced grid: at 0.93 ns steps from t = 0
the port's Newton fails inside the inverter's 10 ns edge and the flip-flop's 1 ns clock edge, and a failed step leaves the grid.

Newton mode 1 has windows of its own, and they end where the first transistor turns on.  Its convergence test is IDA's
``ss ||delta|| <= 0.33`` with the rate constant ss carried from step to step: an ss measured on fresh factors (quadratic convergence:
1e-6 and less) also judges the first round of later steps that solve with stale factors, whose true contraction is 0.05 .. 0.3, and that
round is accepted with (1e4 .. 1e6) tau left.  Measured with the port against the reference on the inverter's edge, 160 steps:
1.3e-6 (h = 29 ps, tau = 1e-11), 1.8e-7 (tau = 3e-13), 7e-11 at best (h = 7 ps), growing from the moment V(in) passes the n-channel
threshold; with a refactorisation every round (the per-op path's mode 1) 2e-8 at h = 116 ps.  That is the mode's policy, not an
error of the discretisation, and no tau repairs it, so through switching events mode 1 stays pinned between port and GPU only
(tests/test_gpu_tran_parity.py).  Before the turn-on the factors age slowly and the mode holds 1e-11: there it is compared with the
reference -- the register-held history, BDF2 / BDF3 coefficients, interpolants and launch seams of the fused kernels' mode 1 forms (the
fixed form that bench.py times among them) on a trajectory that moves by tens of millivolts.
"""
import functools

import numpy as np

from cadnip_jl_amd import benchmarks as bm
from tests import circuits as tc
from tests import tran_ref as TR

REL_TOL_GPU = 1e-9      # tests/test_gpu_tran_parity.REL_TOL: the project's transient tolerance
REL_TOL_PORT = 1e-10    # the port against the reference: ten times inside it

# nine distinct corners (vdd, temp); a batch of B takes the first B.  (The inverter's are all above 3.6 C: below, the oracle's charge
# detection -- the reference's, with its absolute 1e-15 F threshold on a 1 fF junction -- stops giving the n-channel drain junction a charge
# unknown, 14 unknowns instead of the 15 the product discovers once at 27 C for every corner: another, equally valid discretisation of
# that junction, which this comparison cannot cross.)
INV_CORNERS = [(5.0, 27.0), (4.5, 125.0), (5.5, 10.0), (4.7, 85.0), (5.3, 15.0), (4.9, 60.0), (5.1, 100.0), (4.6, 110.0), (5.4, 40.0)]
DFF_CORNERS = [(5.0, 27.0), (4.5, 125.0), (5.5, -40.0)]


class Case:
    def __init__(self, name, make, points, p, m, k0, n_steps, umax, orders, mode=0, start="dc", max_newton=10, checked=None):
        self.name, self.make, self.points = name, make, points
        self.h0, self.hmax, self.n_steps = 2.0 ** -p, 2.0 ** (m - p), n_steps
        self.t0 = k0 * self.hmax                      # a multiple of hmax: the grid times stay exact doubles
        self.umax, self.orders, self.mode, self.start, self.max_newton = umax, orders, mode, start, max_newton
        self.checked = list(range(len(points))) if checked is None else checked     # instances with a reference
        # n_steps 0.33 tau (1 + max|u|) <= 1e-10 and tau <= 1e-11
        self.tau = min(1e-11, 1e-10 / (n_steps * 0.33 * (1.0 + umax)))

    def params(self, i):
        return {k: v for k, v in self.points[i].items() if k != "temp"}

    def temp(self, i):
        return self.points[i].get("temp", 27.0)

    def schedule(self, max_order):
        return TR.schedule(self.t0, self.h0, self.hmax, self.n_steps, max_order)

    @property
    def t1(self):
        return float(self.schedule(1)[0][-1])

    def save_times(self):
        """(save_t sorted, on_grid mask): every grid point and the four off-grid times."""
        g = self.schedule(1)[0]
        k_dbl = 4                                       # step 4 doubles step 3 in every case (m >= 3)
        k_const = self.n_steps - 3
        assert g[k_dbl] - g[k_dbl - 1] == 2.0 * (g[k_dbl - 1] - g[k_dbl - 2]) and g[k_const] - g[k_const - 1] == self.hmax
        off = [g[n - 1] + f * (g[n] - g[n - 1]) for n, f in ((1, 0.25), (2, 0.25), (k_dbl, 0.5), (k_const, 0.8))]
        ts = np.sort(np.concatenate([g, off]))
        return ts, np.isin(ts, g)


def _pts(corners):
    return [{"vdd": v, "temp": t} for v, t in corners]


# the smallest that still reach each mechanism (grids: h0 = 2^-p, hmax = 2^m h0, t0 = k0 hmax, steps)
CASES = {c.name: c for c in (
    # tau_RC = 1 ms; 3 unknowns, no dense core, inconsistent algebraic start (u = 0 with the source at 5 V); 0 .. 3.8 ms
    Case("rc", tc.rc_charge, [{}] * 3, p=20, m=5, k0=0, n_steps=128, umax=5.0, orders=(1, 2, 3), start="zero"),
    # every linear builtin; PWL, PULSE and SIN b(t) evaluated inside the loop (their corners at 0.1 .. 2 ms lie inside the window, none on the grid)
    Case("linear_zoo", tc.linear_zoo, [{}] * 3, p=20, m=5, k0=0, n_steps=128, umax=4.0, orders=(1, 2, 3)),
    # sp_mos1 through cut-off, saturation and triode: 96.0 .. 112.7 ns holds the whole input edge (100 .. 110 ns), 116 ps steps
    Case("inverter", bm.inverter_circuit, _pts(INV_CORNERS), p=36, m=3, k0=825, n_steps=144, umax=6.0, orders=(2, 3)),
    # Newton mode 1: 99.7 .. 100.8 ns, 14.6 ps steps -- V(in) rises to 0.4 V (vdd / 5), the output moves through the gate-drain capacitors
    Case("inverter_mode1", bm.inverter_circuit, _pts(INV_CORNERS), p=39, m=3, k0=6852, n_steps=80, umax=6.0, orders=(2, 3), mode=1),
    # the benchmark circuit (dense core of 8): 49.6 .. 51.4 ns holds the first clock edge (50 .. 51.02 ns), 29 ps steps; the port's Newton
    # needs more than 10 rounds at one step inside the edge (max_newton = 25); reference for the first and the last corner
    Case("dff", bm.dff_circuit, _pts(DFF_CORNERS), p=38, m=3, k0=1704, n_steps=64, umax=6.0, orders=(2,), max_newton=25, checked=[0, 2]),
    # Newton mode 1 (the fixed form): 49.91 .. 50.36 ns, 7.3 ps steps -- the clock falls to 3.2 V (vdd / 5), the clock inverter's p-channel turns on
    Case("dff_mode1", bm.dff_circuit, _pts(DFF_CORNERS), p=40, m=3, k0=6860, n_steps=64, umax=6.0, orders=(2,), mode=1, checked=[0, 2]),
)}


def start_state(case, i):
    """u at t0 of instance i: zeros, or the tranop DC point (from the CPU port's DC solve: an input of both sides)."""
    return _start_state(case.make, case.start, tuple(sorted(case.points[i].items()))).copy()


@functools.lru_cache(maxsize=None)
def _start_state(make, start, point):
    from tests.port_util import make_port, analyze_port
    pt = dict(point)
    st, port = make_port(make(), {k: v for k, v in pt.items() if k != "temp"}, pt.get("temp", 27.0), "tranop")
    try:
        if start == "zero":
            return np.zeros(st.n)
        analyze_port(st, port, 5.0)
        u0, ok, _ = port.dc(abstol=1e-9)
        assert ok, (make, point)
        return u0
    finally:
        port.close()


@functools.lru_cache(maxsize=None)
def reference(name, max_order, i):
    """The reference trajectory of instance i of a case (tests/tran_ref.py), computed once per process."""
    case = CASES[name]
    eq = TR.Equations(case.make(), case.params(i), case.temp(i))
    grid, orders = case.schedule(max_order)
    tr = TR.integrate(eq, start_state(case, i), grid, orders)
    assert np.max(np.abs(tr.U)) <= case.umax, (name, np.max(np.abs(tr.U)))     # tau was chosen for this bound
    tr.names = list(eq.cs.node_names) + list(eq.cs.current_names)
    return tr


def rel_err(got, ref):
    return np.abs(got - ref) / np.maximum(np.abs(ref), 1.0)
