"""TEST INFRASTRUCTURE -- parameter sensitivities of a transient on a GIVEN step grid, for tests/test_tran_sens_ref_cpu.py and
tests/test_gpu_tran_sens.py.  Built on tests/tran_ref.py (the literal oracle's equations, textbook BDF from the Lagrange definition);
shares nothing with the product.

Two references:

* ``trajectory_derivative`` is the DEFINITION: the derivative of the discrete trajectory with respect to a parameter, as the
  Richardson-extrapolated central difference (steps delta and delta / 2: error O(delta^4)) of ``TR.integrate`` trajectories at
  p +- delta on the same forced grid.  With ``start="dc"`` every variant starts from ITS OWN operating point: the given start state
  polished by a dense Newton on the :tranop equations to an update below 1e-13 (1 + |u|).
* ``direct_dense`` is the METHOD (the forward / direct / staggered sensitivity recursion)
      (G + a0 C) s_n = -dF/dp |(u_n, u'_n, t_n) - C sum_{j >= 1} a_j s_{n-j},        F = C u' + G u - b
  in dense numpy with extended-precision residuals: G, C at the accepted point, a_j from ``TR.bdf_alphas`` on the grid, dF/dp the central
  difference of F at p +- delta with the SAME delta the product uses -- so it carries the product's truncation error and can be held
  against it to the project's tolerance, while ``trajectory_derivative`` measures that truncation (``T_CASE`` below).
  The solve is followed by the product's one DEFECT PASS: G + a0 C need not be the Jacobian of F (a capacitance that depends on u but
  sits in C leaves (dC/du) u' out), so F is differenced once more at (u_n +- delta s, u'_n +- delta s', p +- delta) -- the total central
  difference along the trajectory, zero for the exact s -- and s -= (G + a0 C)^-1 of it.

A parameter is a (name, value, delta) triple; name "temp" moves the temperature, any other name a circuit parameter.  Scaled
sensitivities p ds/dp use ``scale_of``: |p|, 1 for p = 0, T + 273.15 for "temp" -- the steps of api.sensitivity divided by rel_step."""
import numpy as np

from oracle import mna_ref as M
from oracle.netlist_ref import make_builder
from tests import tran_ref as TR

LD = np.longdouble
REL_STEP = 1e-4       # the product's default (api.tran: sens_rel_step)


def scale_of(name, value):
    return value + 273.15 if name == "temp" else abs(value) if value != 0 else 1.0


def delta_of(name, value, rel_step=REL_STEP):
    return rel_step * scale_of(name, value)


class OpEquations(TR.Equations):
    """the :tranop equations of the same circuit: what the start state of a run with ``start="dc"`` solves"""

    def __init__(self, circ, params, temp=27.0):
        bld = make_builder(circ.to_dicts(params))
        spec = M.MNASpec(mode="tranop", temp=float(temp))
        ctx = M.build_with_detection(bld, {}, spec)
        self.cs = M.compile_structure(bld, {}, spec, ctx=ctx)
        self.ws = M.create_workspace(self.cs, ctx=ctx)
        self.n = self.cs.n


def moved(params, temp, name, value):
    """(params, temp) with the parameter ``name`` at ``value``"""
    if name == "temp":
        return dict(params), float(value)
    q = dict(params)
    q[name] = float(value)
    return q, temp


def polish(eq_op, u, t0):
    """the operating point near ``u``: dense Newton on G u - b = 0 of the :tranop equations, to an update below 1e-13 (1 + |u|)"""
    u = np.array(u, dtype=float)
    for _ in range(TR.NEWTON_MAX):
        G, _, b = eq_op.stamps(u, t0)
        F = G.astype(LD) @ u.astype(LD) - b.astype(LD)
        d = TR._solve_refined(G, F)
        u = u - d
        if np.all(np.abs(d) < TR.NEWTON_RTOL * (1.0 + np.abs(u))):
            return u
    raise RuntimeError("the operating point near the given start state was not found")


def _trajectory(circ, params, temp, grid, orders, u0, start):
    eq = TR.Equations(circ, params, temp)
    if start == "dc":
        u0 = polish(OpEquations(circ, params, temp), u0, grid[0])
    return TR.integrate(eq, u0, grid, orders).U


def central(circ, params, temp, par, delta, grid, orders, u0, start):
    """(U(p + delta) - U(p - delta)) / (2 delta) at every grid point [n_steps + 1, n]"""
    name, value = par
    up = _trajectory(circ, *moved(params, temp, name, value + delta), grid, orders, u0, start)
    um = _trajectory(circ, *moved(params, temp, name, value - delta), grid, orders, u0, start)
    return ((up.astype(LD) - um.astype(LD)) / LD(2.0 * delta)).astype(float)


def richardson(d1, d2):
    """the O(delta^4) combination of central differences at delta (d1) and delta / 2 (d2)"""
    return ((4.0 * d2.astype(LD) - d1.astype(LD)) / 3.0).astype(float)


def trajectory_derivative(circ, params, temp, par, delta, grid, orders, u0, start, levels=False):
    """dU/dp at every grid point [n_steps + 1, n]: Richardson on (delta, delta / 2).  ``levels``: also the same on (delta / 2, delta / 4)
    -- the disagreement of the two is the reference's own uncertainty."""
    d1 = central(circ, params, temp, par, delta, grid, orders, u0, start)
    d2 = central(circ, params, temp, par, 0.5 * delta, grid, orders, u0, start)
    r12 = richardson(d1, d2)
    if not levels:
        return r12
    d4 = central(circ, params, temp, par, 0.25 * delta, grid, orders, u0, start)
    return r12, richardson(d2, d4)


def _solve_ld(J, r, passes=3):
    """J x = r with r in extended precision: LAPACK's pivoted LU plus ``passes`` refinements on extended-precision residuals"""
    r = np.asarray(r, dtype=LD)
    Jl = J.astype(LD)
    x = np.linalg.solve(J, r.astype(float)).astype(LD)
    for _ in range(passes):
        x = x + np.linalg.solve(J, (r - Jl @ x).astype(float)).astype(LD)
    return x


def _residual(eq, u, udot, t, dtype):
    G, C, b = eq.stamps(u, t)
    return C.astype(dtype) @ udot.astype(dtype) + G.astype(dtype) @ u.astype(dtype) - b.astype(dtype)


def direct_dense(circ, params, temp, pars, deltas, grid, orders, U, start, dtype=LD, passes=1):
    """The forward sensitivity recursion on the trajectory ``U`` [n_steps + 1, n] (of the base parameters, on ``grid`` / ``orders``):
    S [K, n_steps + 1, n].  ``pars``: [(name, value)], ``deltas``: the central-difference steps.  s_0 = 0 with ``start="zero"``;
    with "dc" s_0 = -G^-1 d(G u - b)/dp on the :tranop equations at U[0].  ``dtype``: the precision of the residuals, their difference
    and the history sum (np.longdouble: the reference; float: what double arithmetic makes of the same recursion).  ``passes``: defect
    passes after each step's solve (module docstring; the product makes one, s_0 gets none: at an operating point u' = 0)."""
    grid = np.asarray(grid, dtype=float)
    eq = TR.Equations(circ, params, temp)
    K, n_steps = len(pars), len(grid) - 1
    var = [[TR.Equations(circ, *moved(params, temp, nm, v + sg * d)) for sg in (1.0, -1.0)] for (nm, v), d in zip(pars, deltas)]
    for pair in var:
        for e in pair:
            assert e.n == eq.n, "a perturbed variant has another structure"
    S = np.zeros((K, n_steps + 1, eq.n), dtype=LD)
    if start == "dc":
        op = OpEquations(circ, params, temp)
        G0, _, _ = op.stamps(U[0], grid[0])
        zero = np.zeros(eq.n)
        for k, ((nm, v), d) in enumerate(zip(pars, deltas)):
            fp, fm = (_residual(OpEquations(circ, *moved(params, temp, nm, v + sg * d)), U[0], zero, grid[0], dtype) for sg in (1.0, -1.0))
            S[k, 0] = _solve_ld(G0, -((fp - fm) / dtype(2.0 * d)))
    for m in range(1, n_steps + 1):
        k_ord = int(orders[m - 1])
        idx = list(range(m, m - k_ord - 1, -1))
        al = TR.bdf_alphas(grid[idx])
        u = U[m]
        udot = TR._combine(al, [U[i] for i in idx])
        G, C, _ = eq.stamps(u, grid[m])
        J = G + al[0] * C
        for k, d in enumerate(deltas):
            fp, fm = (_residual(e, u, udot, grid[m], dtype) for e in var[k])
            hist = np.zeros(eq.n, dtype=dtype)
            for a_j, i in zip(al[1:], idx[1:]):
                hist = hist + dtype(a_j) * S[k, i].astype(dtype)
            rhs = -((fp - fm) / dtype(2.0 * d)) - C.astype(dtype) @ hist
            solve = (lambda r: _solve_ld(J, r)) if dtype is LD else (lambda r: np.linalg.solve(J, np.asarray(r, dtype=float)).astype(LD))
            s0 = solve(rhs)
            for _ in range(passes):
                # the defect of s0 in the TOTAL central difference along the trajectory: F at (u + d s, u' + d s', p + d) against (-, -, -)
                sd = (dtype(al[0]) * s0.astype(dtype) + hist)
                fp, fm = (_residual(e, (u.astype(LD) + sg * d * s0).astype(float), (udot.astype(LD) + sg * d * sd.astype(LD)), grid[m], dtype)
                          for e, sg in zip(var[k], (1.0, -1.0)))
                s0 = s0 - solve((fp - fm) / dtype(2.0 * d))
            S[k, m] = s0
    return S.astype(float)


def sample(grid, S, save_t):
    """S [.., n_steps + 1, n] at the save times: the interpolant of the step that reaches each (``TR.Trajectory.at``)"""
    tr = TR.Trajectory(np.asarray(grid, dtype=float), None, None, None)
    out = []
    for ts in np.atleast_1d(save_t):
        m = tr.step_of(ts)
        idx = [m, m - 1] if m == 1 else [m, m - 1, m - 2]
        w = TR.lagrange_values(tr.grid[idx], ts)
        out.append(sum(float(wj) * S[..., i, :] for wj, i in zip(w, idx)))
    return np.moveaxis(np.array(out), 0, -2)


# ---- recorded figures (tests/test_tran_sens_ref_cpu.py asserts measured <= recorded; tests/tran_sens_cases.py names the cases) ----------
# All on scaled sensitivities p ds/dp, rel_err = |a - b| / max(|b|, 1), worst over the checked instances, orders, parameters, grid points
# and unknowns; recorded = measured with headroom (4 x where the figure is rounding noise, 1.25 x where it is deterministic).
# U_REF: the disagreement of the Richardson levels (delta, delta / 2) and (delta / 2, delta / 4) of trajectory_derivative.
#        Measured 1.45e-10 / 6.7e-12 / 1.87e-10.
# T_CASE: direct_dense against trajectory_derivative at (delta, delta / 2): the truncation of the central differences, O(delta^2).
#        Measured 8.64e-9 / 5.70e-10 / 1.46e-8, and 2.16e-9 / 1.43e-10 / 3.58e-9 at delta / 2: the factor 4.
#        WITHOUT the defect pass (passes = 0) the inverter's figure is 2.68e-6 at delta AND at delta / 2 -- not a truncation.  It sits in
#        one unknown, the supply current I_VVDD, from the moment the transistors conduct (everything below 4e-10 before that; every other
#        unknown below 1.4e-8 throughout): the entry of G + a0 C for the supply node onto itself is 1.0720e-4 S where the derivative of
#        the stamped F is 1.0686e-4 S (step 80, first corner; central difference of F, every other row agrees to 6e-11).  The size fits a
#        capacitance that depends on u but sits in C: C moves by 4.8e-18 F per 0.1 V of V(Q) there, and (dC/du) u' with u' = -3.3e9 V/s
#        is 1.6e-7 S, a term G + a0 C does not hold (a junction below the charge detection's threshold stays a C entry; supposed, not
#        traced into the model).  Newton converges all the same; the recursion alone is exact only where G + a0 C is the Jacobian of F.
#        One pass takes the figure to the truncation's size.
# AMP:   direct_dense in float64 against extended precision -- what differencing residuals in double arithmetic costs.  Measured
#        3.7e-12 / 1.9e-12 / 7.1e-11: inside REL_TOL_GPU, so the GPU comparison keeps the project's 1e-9.
U_REF = {"rc": 6e-10, "linear_zoo": 3e-11, "inverter": 8e-10}
T_CASE = {"rc": 1.1e-8, "linear_zoo": 7.2e-10, "inverter": 1.9e-8}
AMP = {"rc": 1.5e-11, "linear_zoo": 7.5e-12, "inverter": 2.9e-10}
