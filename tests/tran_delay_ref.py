"""TEST INFRASTRUCTURE -- a textbook delay-differential transient on a GIVEN step grid: tests/tran_ref.py's BDF with transport delays on
controlled sources (``Circuit.E/G/H/F(..., delay=)``; a ``Circuit.T`` line is made of them), for tests/test_tran_delay_cpu.py and
tests/test_gpu_tran_delay.py.

From tran_ref: the equations (the literal oracle, which ignores the delay as a DC analysis does), the BDF coefficients, the refined dense
solve, the schedule, the save-time interpolant.  Restated here, from the definitions and on the oracle's own indices
(``Equations.index_of``) -- nothing comes from api.ac_delay_overlay or from csrc/delay_plan.hpp:

* the delayed stamps.  With d = delay and x(t - d) the delayed controlling quantity:
    E (op, on, ip, in; branch current I_<name>):   row I:  V(op) - V(on) - gain (V(ip) - V(in))(t - d) = 0
    G (op, on, ip, in):                            rows op / on:  -/+ gm (V(ip) - V(in))(t - d)   (the sign of oracle/devices_ref.stamp_vccs)
    H (sense branch I_<name>_in, output branch I_<name>_out):   row I_out:  V(op) - V(on) - rm I_in(t - d) = 0
    F (sense branch I_<name>_in):                  rows op / on:  -/+ gain I_in(t - d)
  Each is a list of (row, col, w, d): the coefficient w that the undelayed stamp puts at G[row, col].  The system at the trial time t_n is
  (G - W) u + C u' = b - sum w ud(col, t_n - d), W the sum of the w at their places;
* the history rule: ud(col, tq) = u0[col] for tq <= t0 (the pre-history: the state the run starts from); otherwise the straight line between
  the two accepted grid points that bracket tq, v_j + (tq - t_j) / (t_{j+1} - t_j) (v_{j+1} - v_j); a tq at or beyond the newest accepted
  point takes the newest value.  The grid must keep every step at or below the smallest delay (checked), so tq never lies inside the step
  in flight.
"""
import numpy as np

from cadnip_jl_amd.circuit import resolve
from tests import tran_ref as TR

LD = TR.LD


def delayed_terms(eq, circ, params):
    """[(row, col, w, delay)] of the circuit's delayed stamps on the oracle's indices; terms on the ground node are dropped"""
    def node(name):
        return None if name == "0" else eq.index_of(name)

    out = []
    for d in circ.devices:
        if "delay" not in d.params:
            continue
        tau = float(resolve(d.params["delay"], params))
        op, on, ip, in_ = (node(x) for x in d.nodes)
        if d.type == "E":
            g, i = float(resolve(d.params["gain"], params)), eq.index_of("I_" + d.name)
            terms = [(i, ip, -g), (i, in_, g)]
        elif d.type == "G":
            g = float(resolve(d.params["gm"], params))
            terms = [(op, ip, -g), (op, in_, g), (on, ip, g), (on, in_, -g)]
        elif d.type == "H":
            terms = [(eq.index_of("I_%s_out" % d.name), eq.index_of("I_%s_in" % d.name), -float(resolve(d.params["rm"], params)))]
        elif d.type == "F":
            g, i = float(resolve(d.params["gain"], params)), eq.index_of("I_%s_in" % d.name)
            terms = [(op, i, -g), (on, i, g)]
        else:
            raise NotImplementedError("a delay on a %s element" % d.type)
        out += [(r, c, w, tau) for r, c, w in terms if r is not None and c is not None]
    return out


def history_value(times, values, t0, tq):
    """ud at tq from the accepted points (times ascending, values[j] at times[j]; times[0] = t0): the module docstring's rule"""
    if tq <= t0:
        return values[0]
    if tq >= times[-1]:
        return values[-1]
    j = int(np.searchsorted(times, tq, side="right")) - 1
    return values[j] + (tq - times[j]) / (times[j + 1] - times[j]) * (values[j + 1] - values[j])


class DelayedEquations:
    """the oracle's equations of one instance plus its delayed terms"""

    def __init__(self, circ, params, temp=27.0):
        self.eq = TR.Equations(circ, params, temp)
        self.n = self.eq.n
        self.terms = delayed_terms(self.eq, circ, params)
        self.W = np.zeros((self.n, self.n))
        for r, c, w, _ in self.terms:
            self.W[r, c] += w
        self.tau_min = min(t for _, _, _, t in self.terms)

    def index_of(self, name):
        return self.eq.index_of(name)

    def names(self):
        return list(self.eq.cs.node_names) + list(self.eq.cs.current_names)


def integrate(deq, u0, grid, orders, start=None):
    """tran_ref.integrate with the delayed terms: BDF on ``grid`` with the given order per step, Newton on (G - W) + alpha_0 C to 1e-13;
    ``start`` as there.  Returns a tran_ref.Trajectory."""
    grid = np.asarray(grid, dtype=float)
    n_steps = len(grid) - 1
    if np.max(np.diff(grid)) > deq.tau_min:
        raise ValueError("a step of the grid exceeds the smallest delay")
    U = np.zeros((n_steps + 1, deq.n))
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
        idx = list(range(m, m - k - 1, -1))
        al = TR.bdf_alphas(grid[idx])
        beta = TR._combine(al[1:], [U[i] for i in idx[1:]])
        rhs = np.zeros(deq.n)                                   # sum w ud(col, t_n - d): known for the whole step
        for r, c, w, tau in deq.terms:
            rhs[r] += w * history_value(grid[:m], U[:m, c], grid[0], grid[m] - tau)
        starts = [U[m - 1].copy()]
        if m - 1 - k >= 0:
            past = list(range(m - 1, m - k - 2, -1))
            starts.insert(0, TR._combine(TR.lagrange_values(grid[past], grid[m]), [U[i] for i in past]).astype(float))
        total = 0
        for u in starts:
            done = False
            for it in range(1, TR.NEWTON_MAX + 1):
                G, C, b = deq.eq.stamps(u, grid[m])
                G = G - deq.W
                udot = LD(al[0]) * u.astype(LD) + beta
                F = C.astype(LD) @ udot + G.astype(LD) @ u.astype(LD) - (b.astype(LD) - rhs.astype(LD))
                if not np.all(np.isfinite(F.astype(float))):
                    break
                d = TR._solve_refined(G + al[0] * C, F)
                if not np.all(np.isfinite(d)):
                    break
                u = u - d
                if np.all(np.abs(d) < TR.NEWTON_RTOL * (1.0 + np.abs(u))):
                    done = True
                    break
            total += it
            if done:
                break
        else:
            raise RuntimeError("Newton needs more than %d iterations at step %d (t = %r)" % (TR.NEWTON_MAX, m, grid[m]))
        U[m] = u
        iters[m - 1] = total
    return TR.Trajectory(grid, np.asarray(orders, dtype=int), U, iters)
