"""TEST INFRASTRUCTURE -- a textbook BDF transient on a GIVEN step grid, for the transient pins that must not go through the product
or through oracle/cpu_port.cpp (tests/test_tran_ref_cpu.py, tests/test_gpu_tran_exact.py).

What it shares with the product: nothing but the circuit description (``Circuit``) and, through ``schedule``, the three-line rule by
which the controller of csrc/tran_ctrl.hpp lays out its steps when its error test is switched off (``err_mask`` all zero, no break
points): h_1 = h0, h_{m+1} = min(2 h_m, hmax), order of step m = min(max_order, max(1, m - 1)) -- two backward-Euler steps, BDF2 on the
third, BDF3 from the fourth.  THE SCHEDULE IS THE ONLY THING TAKEN FROM THE CONTROLLER.  Everything else is restated from the textbook:

* equations: the literal oracle (oracle/mna_ref.py) -- its own structure discovery, parameter derivation and temperature handling;
  at a point F(u) = C(u) u' + G(u) u - b(u, t), Newton matrix G + alpha_0 C, dense;
* discretisation: u'_n = sum_j alpha_j u_{n-j}, alpha_j the derivative at t_n of the j-th Lagrange basis polynomial on the k + 1 newest
  grid points (t_n included), from that definition, with exact rational node differences (``fractions.Fraction``: a double is a
  rational).  No closed expression of a variable-step BDF coefficient appears here;
* Newton: dense partial-pivoting solves with one step of iterative refinement (residual in extended precision), until the update is
  below 1e-13 (1 + |u|) in every component, started from the polynomial through the newest points and, if that does not get there,
  from the last point; more than 50 iterations from both is an error of the input, not a result;
* output between grid points: the quadratic through the three newest accepted points (t_n, t_{n-1}, t_{n-2}) of the step that reaches
  the save time, the straight line while only two points exist (the first step), weights from the Lagrange definition, exact.
"""
from fractions import Fraction

import numpy as np

from oracle import mna_ref as M
from oracle.netlist_ref import make_builder

LD = np.longdouble
NEWTON_RTOL = 1e-13
NEWTON_MAX = 50


# ---- Lagrange weights from the definition, exact -------------------------------------------------------------------------------------
def _exact(v):
    """A double or a Fraction as the rational it is (a Fraction passes through unrounded: node distances that are sums of doubles)."""
    return v if isinstance(v, Fraction) else Fraction(float(v))


def lagrange_values(nodes, x):
    """[l_j(x)] for the Lagrange basis on ``nodes`` (distinct doubles or Fractions), as Fractions."""
    xs = [_exact(v) for v in nodes]
    x = _exact(x)
    out = []
    for j, xj in enumerate(xs):
        w = Fraction(1)
        for m, xm in enumerate(xs):
            if m != j:
                w *= (x - xm) / (xj - xm)
        out.append(w)
    return out


def lagrange_derivatives(nodes, x):
    """[l_j'(x)]: l_j' = sum_{m != j} 1 / (x_j - x_m) prod_{l != j, m} (x - x_l) / (x_j - x_l), as Fractions."""
    xs = [_exact(v) for v in nodes]
    x = _exact(x)
    out = []
    for j, xj in enumerate(xs):
        s = Fraction(0)
        for m, xm in enumerate(xs):
            if m == j:
                continue
            p = Fraction(1) / (xj - xm)
            for l, xl in enumerate(xs):
                if l != j and l != m:
                    p *= (x - xl) / (xj - xl)
            s += p
        out.append(s)
    return out


def bdf_alphas(times):
    """alpha_0 .. alpha_k of the BDF formula of order k = len(times) - 1 at times[0] = t_n, times[1:] = t_{n-1}, t_{n-2}, ...: doubles
    (each the correctly rounded value of the exact rational)."""
    return [float(a) for a in lagrange_derivatives(times, times[0])]


def _combine(weights, vectors):
    """sum_j w_j v_j, accumulated in extended precision, rounded once."""
    acc = np.zeros(len(vectors[0]), dtype=LD)
    for w, v in zip(weights, vectors):
        acc += LD(float(w)) * np.asarray(v, dtype=LD)
    return acc


# ---- the forced step grid ---------------------------------------------------------------------------------------------------------------
def schedule(t0, h0, hmax, n_steps, max_order):
    """(grid [n_steps + 1], orders [n_steps]): the steps the product's controller takes with its error test off and no break points --
    h_1 = h0, h_{m+1} = min(2 h_m, hmax); order of step m (from 1) = min(max_order, max(1, m - 1)).  The one thing this module takes
    from csrc/tran_ctrl.hpp (prepare_step's start-up rule, tran_update_body's untested ``hnext = 2 h``); see the module docstring."""
    grid, orders = [float(t0)], []
    h = float(h0)
    for m in range(1, n_steps + 1):
        grid.append(grid[-1] + h)
        orders.append(min(int(max_order), max(1, m - 1)))
        h = min(2.0 * h, float(hmax))
    return np.array(grid), np.array(orders, dtype=int)


# ---- equations: the literal oracle ------------------------------------------------------------------------------------------------------
class Equations:
    """F, G, C, b of one circuit instance from oracle/mna_ref.py (built as tests/test_gpu_parity.py:_oracle builds it)."""

    def __init__(self, circ, params, temp=27.0):
        bld = make_builder(circ.to_dicts(params))
        spec = M.MNASpec(mode="tran", temp=float(temp))
        ctx = M.build_with_detection(bld, {}, spec)
        self.cs = M.compile_structure(bld, {}, spec, ctx=ctx)
        self.ws = M.create_workspace(self.cs, ctx=ctx)
        self.n = self.cs.n

    def index_of(self, name):
        cs = self.cs
        if name in cs.node_names:
            return cs.node_names.index(name)
        return cs.n_nodes + cs.current_names.index(name)

    def stamps(self, u, t):
        """(G, C, b) at (u, t), dense."""
        M.fast_rebuild(self.ws, np.asarray(u, dtype=float), float(t))
        return self.cs.G.toarray(), self.cs.C.toarray(), self.ws.dctx.b.copy()


def _solve_refined(J, r):
    """J d = r by LAPACK's partial-pivoting LU, plus one step of iterative refinement on the residual in extended precision."""
    d = np.linalg.solve(J, np.asarray(r, dtype=float))
    rr = np.asarray(r, dtype=LD) - J.astype(LD) @ d.astype(LD)
    return d + np.linalg.solve(J, rr.astype(float))


class Trajectory:
    """Result of ``integrate``: the grid, the order of every step, u at every grid point, Newton iterations per step."""

    def __init__(self, grid, orders, U, iters):
        self.grid, self.orders, self.U, self.iters = grid, orders, U, iters

    def step_of(self, ts):
        """The step (from 1) that reaches the save time ``ts``: the first with ts <= t_n (a save time at t_0 belongs to step 1)."""
        n = int(np.searchsorted(self.grid, float(ts), side="left"))
        n = max(n, 1)
        if n >= len(self.grid):
            raise ValueError("save time %r beyond the grid" % ts)
        return n

    def at(self, ts):
        """u at the save time ``ts``: the interpolant of the step that reaches it (module docstring); on a grid point, that point."""
        n = self.step_of(ts)
        idx = [n, n - 1] if n == 1 else [n, n - 1, n - 2]
        w = lagrange_values(self.grid[idx], ts)
        return _combine(w, [self.U[i] for i in idx]).astype(float)

    def sample(self, save_t):
        return np.array([self.at(ts) for ts in np.atleast_1d(save_t)])


def integrate(eq, u0, grid, orders, start=None):
    """BDF on ``grid`` with the given order per step (orders[m - 1] for the step that ends at grid[m]).  ``start``: known values at the
    first grid points ([k, n], start[0] at grid[0]) -- the steps that end there are not taken (the textbook's exact starting values for
    a convergence-order measurement); by default only u0 at grid[0] is known."""
    grid = np.asarray(grid, dtype=float)
    n_steps = len(grid) - 1
    U = np.zeros((n_steps + 1, eq.n))
    known = 1
    if start is not None:
        start = np.atleast_2d(np.asarray(start, dtype=float))
        known = start.shape[0]
        U[:known] = start
    else:
        U[0] = np.asarray(u0, dtype=float)
    iters = np.zeros(n_steps, dtype=int)
    for m in range(known, n_steps + 1):
        k = int(orders[m - 1])
        if k < 1 or k > m:
            raise ValueError("order %d at step %d needs %d earlier points" % (k, m, k))
        idx = list(range(m, m - k - 1, -1))
        al = bdf_alphas(grid[idx])
        beta = _combine(al[1:], [U[i] for i in idx[1:]])          # the known part of u'_n
        # starting guess: the polynomial through the k + 1 newest known points, continued to t_n (where it leads Newton astray -- a corner
        # of a source inside the step -- the last accepted point); the converged u does not depend on it
        starts = [U[m - 1].copy()]
        if m - 1 - k >= 0:
            past = list(range(m - 1, m - k - 2, -1))
            starts.insert(0, _combine(lagrange_values(grid[past], grid[m]), [U[i] for i in past]).astype(float))
        total = 0
        for u in starts:
            done = False
            for it in range(1, NEWTON_MAX + 1):
                G, C, b = eq.stamps(u, grid[m])
                udot = LD(al[0]) * u.astype(LD) + beta
                F = C.astype(LD) @ udot + G.astype(LD) @ u.astype(LD) - b.astype(LD)
                if not np.all(np.isfinite(F.astype(float))):
                    break
                d = _solve_refined(G + al[0] * C, F)
                if not np.all(np.isfinite(d)):
                    break
                u = u - d
                if np.all(np.abs(d) < NEWTON_RTOL * (1.0 + np.abs(u))):
                    done = True
                    break
            total += it
            if done:
                break
        else:
            raise RuntimeError("Newton needs more than %d iterations at step %d (t = %r): badly chosen input" % (NEWTON_MAX, m, grid[m]))
        U[m] = u
        iters[m - 1] = total
    return Trajectory(grid, np.asarray(orders, dtype=int), U, iters)
