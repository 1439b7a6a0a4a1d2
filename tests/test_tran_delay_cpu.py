"""Transients with transport delays, the parts that need no GPU:

(a) csrc/delay_plan.hpp -- the history ring's index arithmetic, its look-up (pre-history, bracket search, newest value, overflow, linear
    weights) and the host plan of the kernels -- compiled with the host compiler, as tests/test_ac_hbm_plan_cpu.py compiles its header;
(b) the delay-differential reference (tests/tran_delay_ref.py) against the closed form of the delayed buffer on halved grids;
(c) the reference on a lossless line, where the discrete solution is the lattice diagram itself;
(d) the opt-in keyword of api.tran and the propagation of break points through the delays (pure host code)."""
import ctypes
import math
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import cadnip_jl_amd as cj
from cadnip_jl_amd import api, hip
from tests import tran_delay_cases as K
from tests import tran_delay_ref as DR
from tests import tran_ref as TR
from tests.test_lds_layout import CSRC

SHIM = r"""
#include "delay_plan.hpp"
using namespace cadnip;
extern "C" {
int t_default_depth() { return CADNIP_DELAY_DEFAULT_DEPTH; }
int t_slot(int head, int count, int depth, int j) { return delay_ring_slot(head, count, depth, j); }
int t_push(int* head, int* count, int depth) { return delay_ring_push(head, count, depth); }
void t_lookup(const double* ht, int head, int count, int depth, double t0, double tq, int* o, double* w) {
  const DelayLookup L = delay_lookup(ht, head, count, depth, t0, tq);
  o[0] = L.kind; o[1] = L.s0; o[2] = L.s1; *w = L.w;
}
double t_value(int kind, int s0, int s1, double w, const double* hv, double v_init) { return delay_value(DelayLookup{kind, s0, s1, w}, hv, v_init); }
double t_tau_min(const double* tau, int count) { return delay_tau_min(tau, (size_t)count); }
// sizes: n_pos, n_taps, n_rows, n_term; out: pos | taps | rows | row_ptr | term | term_tap | term_pos
int t_plan(int n, int nnz, const int* rowptr, const int* colidx, int n_pos, const int* pos, int n_term, const int* tp, const int* tr, const int* tc,
           int* sizes, int* out) {
  DelayPlan P;
  if (!delay_plan_build(n, nnz, rowptr, colidx, n_pos, pos, n_term, tp, tr, tc, P)) return 0;
  sizes[0] = (int)P.pos.size(); sizes[1] = (int)P.taps.size(); sizes[2] = (int)P.rows.size(); sizes[3] = (int)P.term.size();
  for (const std::vector<int>* v : {&P.pos, &P.taps, &P.rows, &P.row_ptr, &P.term, &P.term_tap, &P.term_pos}) for (int x : *v) *out++ = x;
  return 1;
}
}
"""
PRE, INTERP, NEWEST, OVERFLOW = 0, 1, 2, 3


@pytest.fixture(scope="module")
def L(tmp_path_factory):
    d = tmp_path_factory.mktemp("delay_plan")
    src, lib = str(d / "shim.cpp"), str(d / "libshim.so")
    with open(src, "w") as f:
        f.write(SHIM)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", "-I", CSRC, "-o", lib, src])
    lib = ctypes.CDLL(lib)
    lib.t_value.restype = lib.t_tau_min.restype = ctypes.c_double
    lib.t_value.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_void_p, ctypes.c_double]
    lib.t_lookup.argtypes = [ctypes.c_void_p] + [ctypes.c_int] * 3 + [ctypes.c_double] * 2 + [ctypes.c_void_p] * 2
    return lib


class Ring:
    """a ring of one tap driven through the header's own functions"""

    def __init__(self, L, depth, t0, v0):
        self.L, self.depth, self.t0, self.v_init = L, depth, t0, v0
        self.t, self.v = np.zeros(depth), np.zeros(depth)
        self.head, self.count = ctypes.c_int(0), ctypes.c_int(0)
        self.push(t0, v0)

    def push(self, t, v):
        s = self.L.t_push(ctypes.byref(self.head), ctypes.byref(self.count), self.depth)
        self.t[s], self.v[s] = t, v
        return s

    def look(self, tq):
        o, w = (ctypes.c_int * 3)(), ctypes.c_double()
        self.L.t_lookup(self.t.ctypes.data, self.head.value, self.count.value, self.depth, self.t0, tq, o, ctypes.byref(w))
        return o[0], o[1], o[2], w.value

    def value(self, tq):
        kind, s0, s1, w = self.look(tq)
        assert kind != OVERFLOW
        return self.L.t_value(kind, s0, s1, w, self.v.ctypes.data, self.v_init)


# ---- (a) the header -----------------------------------------------------------------------------------------------------------------------
def test_ring_wraps_and_brackets_across_the_wrap(L):
    """nine points into a ring of four: the four newest stay, in order, and a look-up between the two that straddle the wrap interpolates"""
    assert L.t_default_depth() == 1024
    times = [0.0, 1.0, 2.5, 3.0, 4.0, 6.0, 7.0, 7.5, 9.0]
    r = Ring(L, 4, times[0], 10.0)
    slots = [0] + [r.push(t, 10.0 + t * t) for t in times[1:]]
    assert slots == [0, 1, 2, 3, 0, 1, 2, 3, 0] and r.count.value == 4 and r.head.value == 1
    kept = [r.t[L.t_slot(r.head.value, r.count.value, 4, j)] for j in range(4)]
    assert kept == times[-4:]
    # 7.5 sits in slot 3, 9.0 in slot 0: the bracket of 8.0 crosses the wrap
    kind, s0, s1, w = r.look(8.0)
    assert (kind, s0, s1) == (INTERP, 3, 0) and w == (8.0 - 7.5) / (9.0 - 7.5)
    assert r.value(8.0) == (10.0 + 7.5 ** 2) + w * ((10.0 + 81.0) - (10.0 + 7.5 ** 2))
    # every bracket of the kept range
    for j in range(3):
        a, b = kept[j], kept[j + 1]
        kind, s0, s1, w = r.look(0.5 * (a + b))
        assert kind == INTERP and r.t[s0] == a and r.t[s1] == b and w == 0.5


def test_lookup_on_a_stored_time_and_an_ulp_above_the_newest(L):
    r = Ring(L, 8, 0.0, 1.0)
    for t, v in ((1.0, 2.0), (2.0, 4.0), (3.0, 8.0)):
        r.push(t, v)
    kind, s0, s1, w = r.look(2.0)                      # exactly on a stored time: weight zero, the stored value to the bit
    assert kind == INTERP and r.t[s0] == 2.0 and w == 0.0 and r.value(2.0) == 4.0
    assert r.look(3.0)[0] == NEWEST and r.value(3.0) == 8.0
    assert r.look(math.nextafter(3.0, 4.0))[0] == NEWEST and r.value(math.nextafter(3.0, 4.0)) == 8.0
    assert r.look(math.nextafter(3.0, 0.0))[0] == INTERP


def test_prehistory_survives_the_overwrite_of_t0_and_older_than_kept_is_overflow(L):
    r = Ring(L, 4, 1.0, -3.0)
    for k in range(1, 7):
        r.push(1.0 + k, float(k))                       # the t0 entry is gone after the fourth push
    assert min(r.t) == 4.0
    for tq in (1.0, 0.5, -7.0):
        assert r.look(tq)[0] == PRE and r.value(tq) == -3.0
    for tq in (math.nextafter(1.0, 2.0), 2.0, math.nextafter(4.0, 0.0)):
        assert r.look(tq)[0] == OVERFLOW                 # later than t0, older than the oldest point kept: no extrapolation
    assert r.look(4.0)[0] == INTERP and r.value(4.0) == 3.0


def test_interpolation_weights_against_exact_rationals(L):
    rng = np.random.default_rng(5)
    times = np.cumsum(rng.random(12) + 0.01)
    r = Ring(L, 16, times[0], 0.0)
    for t in times[1:]:
        r.push(t, 0.0)
    for tq in times[0] + (times[-1] - times[0]) * rng.random(200):
        kind, s0, s1, w = r.look(tq)
        if kind != INTERP:
            continue
        tj, tk = Fraction(r.t[s0]), Fraction(r.t[s1])
        assert tj <= Fraction(tq) < tk and s1 == s0 + 1
        exact = (Fraction(tq) - tj) / (tk - tj)
        # two roundings (the differences are exact or rounded once each, then the quotient): within 2 ulp of the exact weight, inside [0, 1)
        assert abs(Fraction(w) - exact) <= 2 * Fraction(math.ulp(max(w, 2.0 ** -60))) and 0.0 <= w < 1.0 + 1e-15


def test_tau_min_refuses_what_is_not_a_positive_finite_delay(L):
    tm = lambda xs: L.t_tau_min(np.array(xs, dtype=float).ctypes.data_as(ctypes.c_void_p), len(xs))
    assert tm([3.0, 1.5, 2.0]) == 1.5
    for bad in (0.0, -1.0, math.inf, math.nan):
        assert tm([3.0, bad]) <= 0.0


def _plan(L, n, rowptr, colidx, pos, tp, tr, tc):
    ia = lambda v: np.ascontiguousarray(v, dtype=np.int32)
    rowptr, colidx, pos, tp, tr, tc = map(ia, (rowptr, colidx, pos, tp, tr, tc))
    sizes, out = np.zeros(4, dtype=np.int32), np.zeros(4 * (len(pos) + 4 * len(tp)) + 8, dtype=np.int32)
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    ok = L.t_plan(n, len(colidx), ptr(rowptr), ptr(colidx), len(pos), ptr(pos), len(tp), ptr(tp), ptr(tr), ptr(tc), ptr(sizes), ptr(out))
    if not ok:
        return None
    npos, ntap, nrow, nterm = (int(x) for x in sizes)
    cuts = np.cumsum([0, npos, ntap, nrow, nrow + 1, nterm, nterm, nterm])
    return dict(zip(("pos", "taps", "rows", "row_ptr", "term", "term_tap", "term_pos"), (out[cuts[i]:cuts[i + 1]].tolist() for i in range(7))))


def test_plan_of_two_lines_that_share_a_node(L):
    """Two delayed stamps per line end, two lines with one node in common: rows 4 and 5 (branch currents) read the shared node 1 and their
    own far nodes -- one tap for the shared column, terms grouped by row in table order, positions ascending whatever order they came in."""
    n = 6
    dense = np.zeros((n, n), dtype=int)
    for r, c in ((4, 1), (4, 2), (5, 1), (5, 3), (0, 0), (1, 1), (2, 2), (3, 3), (4, 4), (5, 5)):
        dense[r, c] = 1
    rowptr = np.concatenate([[0], np.cumsum(dense.sum(axis=1))])
    colidx = np.concatenate([np.flatnonzero(dense[r]) for r in range(n)])
    at = lambda r, c: int(rowptr[r] + np.flatnonzero(colidx[rowptr[r]:rowptr[r + 1]] == c)[0])
    pos = [at(5, 3), at(4, 1), at(5, 1), at(4, 2)]                 # not ascending on purpose
    # terms in table order: (row 5, col 1), (row 4, col 2), (row 4, col 1), (row 5, col 3), and a second stamp on (4, 1)
    tp, tr, tc = [2, 3, 1, 0, 1], [5, 4, 4, 5, 4], [1, 2, 1, 3, 1]
    P = _plan(L, n, rowptr, colidx, pos, tp, tr, tc)
    assert P["pos"] == sorted(pos)
    assert P["taps"] == [1, 2, 3]                                   # the shared node once
    assert P["rows"] == [4, 5] and P["row_ptr"] == [0, 3, 5]
    assert P["term"] == [1, 2, 4, 0, 3]                             # row 4's terms in table order, then row 5's
    assert P["term_tap"] == [1, 0, 0, 0, 2]
    assert [P["pos"][k] for k in P["term_pos"]] == [at(4, 2), at(4, 1), at(4, 1), at(5, 1), at(5, 3)]
    # refusals: a term off its position, an index out of range, a position named twice
    assert _plan(L, n, rowptr, colidx, pos, tp, tr, [1, 2, 1, 3, 2]) is None
    assert _plan(L, n, rowptr, colidx, pos, [2, 3, 1, 0, 4], tr, tc) is None
    assert _plan(L, n, rowptr, colidx, pos, tp, [5, 4, 4, 5, 6], tc) is None
    assert _plan(L, n, rowptr, colidx, [pos[0], pos[1], pos[2], pos[1]], tp, tr, tc) is None
    assert _plan(L, n, rowptr, colidx, [pos[0], pos[1], pos[2], len(colidx)], tp, tr, tc) is None


def test_plan_of_a_real_circuit_with_two_lines_in_series(L):
    """the terms api.ac_delay_overlay makes of two Circuit.T lines that meet in node m: m is read by a stamp of each line and is one tap"""
    c = cj.Circuit("two lines")
    c.V("vs", "s", "0", dc=0.0)
    c.R("rs", "s", "p1", 30.0)
    c.T("t1", "p1", "0", "m", "0", 50.0, K.TD)
    c.T("t2", "m", "0", "p3", "0", 75.0, 2 * K.TD)
    c.R("rl", "p3", "0", 100.0)
    st = cj.discover(c, {})
    ovl = api.ac_delay_overlay(st, c, {}, (), 1)
    o = np.array([k for k, _, _ in ovl.terms])
    rows, cols = ovl.rows[o], ovl.cols[o]
    P = _plan(L, st.n, st.rowptr, st.colidx, ovl.pos, o, rows, cols)
    m = st.index_of("m")
    assert int(np.sum(cols == m)) == 2 and P["taps"].count(m) == 1
    assert P["taps"] == sorted(set(cols.tolist())) and P["rows"] == sorted(set(rows.tolist())) and P["pos"] == sorted(ovl.pos.tolist())
    assert len(P["term"]) == len(o) == 8 and P["row_ptr"][-1] == 8
    for r, row in enumerate(P["rows"]):
        mine = P["term"][P["row_ptr"][r]:P["row_ptr"][r + 1]]
        assert mine == [t for t in range(len(o)) if rows[t] == row]                      # table order inside a row
    assert [P["taps"][k] for k in P["term_tap"]] == [int(cols[t]) for t in P["term"]]
    assert [P["pos"][k] for k in P["term_pos"]] == [int(ovl.pos[o[t]]) for t in P["term"]]


# ---- (b) the reference against the closed form of the delayed buffer ------------------------------------------------------------------------
BUF_TA, BUF_TB, BUF_TAU, BUF_T1 = 0.5 * K.TD, 1.5 * K.TD, 0.75 * K.TD, 4.0 * K.TD
STEPS = {1: 512, 2: 128}             # coarsest grid (steps over 4 TD): the kinks (TD / 2, 3 TD / 2) and their images (5 TD / 4, 9 TD / 4) are on it


@pytest.mark.parametrize("k", [1, 2])
def test_reference_error_on_the_delayed_buffer_falls_with_the_order(k):
    """PWL ramp into E(gain 2, delay tau) into R C: V(out) is the R C response to the delayed ramp.  The tap is piecewise linear with its
    kinks on the grid, so the history rule is exact and what remains is the BDF error: a factor 2^k per halving, within the 15 % that
    tests/test_tran_ref_cpu.py asks of its own closed forms, exact starting values as there."""
    circ = K.buffer(K.pwl_ramp(BUF_TA, BUF_TB), BUF_TAU)
    deq = DR.DelayedEquations(circ, {})
    assert sorted((r, c, w) for r, c, w, _ in deq.terms) == [(deq.index_of("I_e1"), deq.index_of("a"), -K.BUF_GAIN)]
    G0 = deq.eq.stamps(np.zeros(deq.n), 0.0)[0]
    for r, c, w, _ in deq.terms:
        assert G0[r, c] == w                                         # the restated stamp is the oracle's own entry
    out = deq.index_of("out")

    def exact(t):
        u = np.zeros(deq.n)
        vin = float(K.ramp(t, BUF_TA, BUF_TB))
        vb = K.BUF_GAIN * float(K.ramp(t - BUF_TAU, BUF_TA, BUF_TB))
        vo = float(K.buffer_out(t, BUF_TA, BUF_TB, BUF_TAU))
        for nm, v in (("in", vin), ("a", vin), ("b", vb), ("out", vo)):
            u[deq.index_of(nm)] = v
        u[deq.index_of("I_e1")] = -(vb - vo) / K.BUF_R               # filled for completeness: only V(out) has a history of its own
        return u

    errs = []
    for N in (STEPS[k], 2 * STEPS[k], 4 * STEPS[k]):
        h = BUF_T1 / N
        grid, _ = TR.schedule(0.0, h, h, N, k)
        assert all(t in grid for t in (BUF_TA, BUF_TB, BUF_TA + BUF_TAU, BUF_TB + BUF_TAU)) and grid[-1] == BUF_T1
        tr = DR.integrate(deq, None, grid, np.full(N, k), start=np.array([exact(t) for t in grid[:k]]))
        ref = np.array([float(K.buffer_out(t, BUF_TA, BUF_TB, BUF_TAU)) for t in grid])
        errs.append(float(np.max(np.abs(tr.U[:, out] - ref)) / K.BUF_GAIN))
    ratios = [errs[0] / errs[1], errs[1] / errs[2]]
    print("delayed buffer order", k, "errors", errs, "ratios", ratios)
    assert errs[2] > 1e-10
    for r in ratios:
        assert abs(r / 2.0 ** k - 1.0) <= 0.15, (k, errs, ratios)


# ---- (c) a lossless line on the reference -----------------------------------------------------------------------------------------------------
LINE_TA, LINE_TB = 0.25 * K.TD, 0.75 * K.TD


@pytest.mark.parametrize("rs,rl", [(30.0, 100.0), (50.0, None)], ids=["mismatched", "matched-open"])
def test_reference_on_a_lossless_line_is_the_lattice_diagram(rs, rl):
    """No capacitor: every step solves an algebraic system whose right-hand side is the delayed wave, so on a grid that holds every kink
    image the reference IS the lattice diagram -- rho_s = -1/4, rho_l = 1/3: finite sums of delayed copies of the ramp; 50 ohm source and
    open end: far = vs(t - td), near = (vs(t) + vs(t - 2 td)) / 2.  1e-12 of the 1 V swing."""
    circ = K.line(K.pwl_ramp(LINE_TA, LINE_TB), rs, rl, K.TD)
    deq = DR.DelayedEquations(circ, {})
    assert len(deq.terms) == 4 and deq.tau_min == K.TD
    h = K.TD / 8
    grid, orders = TR.schedule(0.0, h, h, 48, 2)
    tr = DR.integrate(deq, np.zeros(deq.n), grid, orders)
    vs = lambda t: K.ramp(t, LINE_TA, LINE_TB)
    near, far = K.lattice(vs, grid, rs, rl, K.TD)
    if rl is None:
        assert np.max(np.abs(far - vs(grid - K.TD))) <= 1e-15 and np.max(np.abs(near - 0.5 * (vs(grid) + vs(grid - 2 * K.TD)))) <= 1e-15
    e1 = float(np.max(np.abs(tr.U[:, deq.index_of("p1")] - near)))
    e2 = float(np.max(np.abs(tr.U[:, deq.index_of("p2")] - far)))
    print("line rs %g rl %s: near-end error %.2e, far-end error %.2e" % (rs, rl, e1, e2))
    assert e1 <= 1e-12 and e2 <= 1e-12
    assert np.max(np.abs(far)) > 0.7                                # the wave did arrive


# ---- (d) the opt-in keyword and the break points --------------------------------------------------------------------------------------------
def test_tran_opt_in_gets_past_the_refusal():
    mc = api.MNACircuit(K.buffer(K.pwl_ramp(BUF_TA, BUF_TB), BUF_TAU), {})
    with pytest.raises(NotImplementedError, match="tran"):
        api.tran(mc, (0.0, BUF_T1))
    with pytest.raises(ValueError, match="delays"):
        api.tran(mc, (0.0, BUF_T1), delays="bogus")
    # with the opt-in the call reaches the device work: on a machine without a GPU it ends where every compute entry point ends there
    try:
        sol = api.tran(mc, (0.0, BUF_T1), abstol=1e-6, reltol=1e-3, saveat=np.linspace(0.0, BUF_T1, 9), delays="history")
    except NotImplementedError:
        raise
    except (hip.CadnipError, ImportError, OSError):
        return
    assert sol.retcode == "Success"


def test_a_sweep_with_a_zero_delay_is_a_value_error():
    mc = api.MNACircuit(K.line(K.pwl_ramp(LINE_TA, LINE_TB), 30.0, 100.0), {"td": K.TD})
    for bad in (0.0, -K.TD, math.inf):
        with pytest.raises(ValueError, match="delay"):
            api.tran(api.CircuitSweep(mc, api.Sweep(td=[K.TD, bad])), (0.0, 6 * K.TD), delays="history")
    with pytest.raises(ValueError, match="delay"):
        api.tran(api.MNACircuit(K.line(K.pwl_ramp(LINE_TA, LINE_TB), 30.0, 100.0), {"td": 0.0}), (0.0, 6 * K.TD), delays="history")


def test_break_points_of_the_mismatched_line_are_the_kink_images():
    """kinks at td / 4 and 3 td / 4, one delay td, six td: the start of the run and both kinks reappear every td"""
    td = K.TD
    got, n_new, truncated = api.delay_breakpoints([LINE_TA, LINE_TB], [[td, td, td, td]], (0.0, 6 * td))
    want = [0.25 * td, 0.75 * td] + [k * td + x for k in range(1, 6) for x in (0.0, 0.25 * td, 0.75 * td)]
    assert got == want and n_new == 15 and not truncated
    # a sweep: the list is the union over the instances' delays
    got2, n2, _ = api.delay_breakpoints([LINE_TA], [[td], [2 * td]], (0.0, 3 * td))
    assert got2 == [0.25 * td, td, 1.25 * td, 2 * td, 2.25 * td] and n2 == 4
    # nothing delayed, nothing added
    assert api.delay_breakpoints([LINE_TA], [], (0.0, td)) == ([LINE_TA], 0, False)


def test_break_point_cap_truncates_breadth_first_and_says_so():
    """delays 1 and 1.5 from t0 = 0: one delay gives {1, 1.5}, two {2, 2.5, 3}, three {3.5, 4, 4.5} (3 is known).  A cap of six keeps
    every time of the first two levels and the earliest of the third."""
    got, n_new, truncated = api.delay_breakpoints([], [1.0, 1.5], (0.0, 10.0), max_points=6)
    assert got == [1.0, 1.5, 2.0, 2.5, 3.0, 3.5] and n_new == 6 and truncated
    full, n_full, t_full = api.delay_breakpoints([], [1.0, 1.5], (0.0, 10.0))
    assert full == [0.5 * k for k in range(2, 20)] and n_full == 18 and not t_full
