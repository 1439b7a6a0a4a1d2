"""The reference of the transient controller (tests/tran_ctrl_ref.py) and its cases (tests/tran_ctrl_cases.py), checked without a GPU:
the error constant and the interpolants against polynomials, the margins and the coverage of the cases, and the comparison code itself --
it must accept a device that rounds every quantity once, and it must name a case when one rule is changed."""
import copy
import functools
import math
import random
from fractions import Fraction as F

import numpy as np
import pytest

from tests import tran_ctrl_cases as Cs
from tests import tran_ctrl_ref as R
from tests import tran_ref


@functools.lru_cache(maxsize=None)
def configs():
    return Cs.build()


@functools.lru_cache(maxsize=None)
def outcomes():
    """(config, case, Outcome) of every op-1 case: the reference, computed once."""
    return [(c, k, R.update(c.sh, k.st, k.vec, k.flags & 1)) for c in configs() if c.op == 1 for k in c.cases]


def _rational_grid(rnd, k):
    """k + 2 strictly decreasing rational times t_n > t_{n-1} > ... with step ratios over 0.1 .. 10."""
    t, h = F(rnd.randint(1, 1000), 997), F(rnd.randint(1, 1000), 1009)
    ts = [t]
    for _ in range(k + 1):
        ts.append(ts[-1] - h)
        h *= F(rnd.randint(10, 100), rnd.randint(10, 100))          # the next step back: 0.1 .. 10 times this one
    return ts


@pytest.mark.parametrize("k", [1, 2, 3])
def test_error_constant_on_monomials(k):
    """For y = t^(k+1) the BDF-k solution y_n (exact history) misses y(t_n) by -errc_k times (y(t_n) - p(t_n)), p the predictor through the
    k + 1 last points: exactly, on random rational grids -- which is what makes errc_k the constant of the error test."""
    rnd = random.Random(100 + k)
    for _ in range(20):
        ts = _rational_grid(rnd, k)
        steps = [ts[j] - ts[j + 1] for j in range(k + 1)] + [F(1)] * 3
        errc, _ = R.error_constant(k, steps[0], steps[1], steps[2], steps[3])
        y = lambda t: t ** (k + 1)
        al = tran_ref.lagrange_derivatives(ts[:k + 1], ts[0])
        # BDF-k for y' = f(t) = (k + 1) t^k:  al_0 y_n + sum_j al_j y(t_{n-j}) = f(t_n)
        yn = ((k + 1) * ts[0] ** k - sum(a * y(t) for a, t in zip(al[1:], ts[1:k + 1]))) / al[0]
        p = sum(w * y(t) for w, t in zip(tran_ref.lagrange_values(ts[1:k + 2], ts[0]), ts[1:k + 2]))
        assert y(ts[0]) - yn == -errc * (y(ts[0]) - p)


def test_positions_and_orders():
    assert R.positions(1.0, 2.0, 4.0, 8.0) == [1, 0, -2, -6, -14]
    assert [R.order_of(nh, mo) for nh in (1, 2, 3, 4) for mo in (1, 2, 3)] == [
        (1, 1)] * 3 + [(1, 2)] * 3 + [(1, 2), (2, 3), (2, 3)] + [(1, 2), (2, 3), (3, 4)]


@pytest.mark.parametrize("nhist", [1, 2, 3])
def test_interpolants_reproduce_polynomials(nhist):
    """The save-time weights reproduce every polynomial of their degree (1 at nhist = 1, 2 from nhist = 2 on) exactly, at save times inside
    the step, on its end and one double beyond it."""
    rnd = random.Random(7)
    sh = {"save_t": None}
    for _ in range(20):
        t, h, hprev = rnd.uniform(1e-6, 1e-3), 10.0 ** rnd.uniform(-12, -7), 10.0 ** rnd.uniform(-12, -7)
        tn = t + h
        st = dict(t=t, tn=tn, hprev=hprev, nhist=nhist)
        deg = 1 if nhist == 1 else 2
        coef = [F(rnd.randint(-9, 9)) for _ in range(deg + 1)]
        poly = lambda x: sum(c * x ** j for j, c in enumerate(coef))
        pts = [F(tn), F(t), F(t) - F(hprev)]
        for ts in (t + 0.3 * h, tn, float(np.nextafter(tn, math.inf)), t):
            sh["save_t"] = [ts]
            w, _ = R.interpolant_weights(sh, st, 0)
            assert sum(wj * poly(x) for (wj, _), x in zip(w, pts)) == poly(F(ts))


def test_prediction_and_derivative_weights_are_exact_on_polynomials():
    """prepare(): the predictor continues every polynomial of degree npts - 1 exactly, and a0 u_n + beta is its derivative at t_n."""
    rnd = random.Random(8)
    sh = dict(t1=1.0, breaks=[], max_order=3)
    for nhist in (1, 2, 3, 4):
        h, hprev, hpp, hp3 = [10.0 ** rnd.uniform(-9, -7) for _ in range(4)]
        pr = R.prepare(sh, 0.25, h, nhist, hprev, hpp, hp3, 0)
        pos = R.positions(pr.h, hprev, hpp, hp3)
        coef = [F(rnd.randint(-9, 9)) for _ in range(pr.npts)]
        poly = lambda x: sum(c * x ** j for j, c in enumerate(coef[:pr.ord + 1]))
        dpoly = lambda x: sum(j * c * x ** (j - 1) for j, c in enumerate(coef[:pr.ord + 1]) if j)
        if pr.npts > pr.ord:
            assert sum(w * poly(x) for (w, _), x in zip(pr.pred_w, pos[1:])) == poly(pos[0])
        assert pr.a0 * poly(pos[0]) + sum(a * poly(x) for (a, _), x in zip(pr.alpha, pos[1:])) == dpoly(pos[0])


def test_clipping_rule_on_doubles():
    sh = dict(t1=1e-3, breaks=np.array([5e-4, 2e-3]))
    t = 5e-4 - 1e-8
    rem = float(np.float64(5e-4) - np.float64(t))
    thr = float(np.float64(rem) * np.float64(1.0 - 1e-9))
    assert R.clip(sh, t, rem, 0) == (rem, 5e-4, "land")
    assert R.clip(sh, t, thr, 0) == (rem, 5e-4, "land")
    below = float(np.nextafter(thr, 0.0))
    assert R.clip(sh, t, below, 0) == (0.5 * rem, t + 0.5 * rem, "half")
    assert R.clip(sh, t, 0.5 * rem, 0)[2] == "free"
    assert R.clip(sh, t, float(np.nextafter(0.5 * rem, 1.0)), 0)[2] == "half"
    assert R.clip(sh, 1e-3 - 1e-8, 1.0, 1) == (float(np.float64(1e-3) - np.float64(1e-3 - 1e-8)), 1e-3, "land")     # a breakpoint beyond t1 is no stop


def test_every_robust_case_keeps_its_margin():
    """At least 1e-6 relative from every threshold compared, and the bound of the compared value well inside that margin."""
    n_robust = 0
    for cfg, case, o in outcomes():
        assert o.row == case.row, (cfg.name, case.name, o.row)
        if not case.robust:
            continue
        n_robust += 1
        assert R.margin_of(o) >= R.MARGIN, (cfg.name, case.name, [(a, float(b), c) for a, b, c in o.margins])
        nm = getattr(o, "norms", None)
        if nm and not nm["bad"]:
            assert nm["dnorm_rel"] < R.MARGIN / 100
            if nm["tested"] and nm["errn"] > 0:
                assert nm["errn_bound"] / nm["errn"] < R.MARGIN / 100, (cfg.name, case.name, float(nm["errn_bound"] / nm["errn"]))
        if o.next is not None and o.next["h"][0] == "real":
            assert R._branch_of_real(cfg.sh, o.next["t"], o.next["h"], o.next["bp"]) is not None, (cfg.name, case.name)
    assert n_robust > 200


def test_order2_steps_stay_inside_the_allowance():
    """What an order-2 step spends besides step_root's own error fits into the rest of the 1.0e-7 allowance."""
    seen = 0
    for cfg, case, o in outcomes():
        if o.next is not None and o.next["h"][0] == "real" and o.next["h"][2] == R.ROOT2_REL:
            nm = o.norms
            assert R.step_budget(2, nm["errn_bound"] / nm["errn"]) <= R.ROOT2_REL - R.ROOT2_OWN, (cfg.name, case.name)
            seen += 1
    assert seen >= 10


def test_coverage_of_rows_and_edges():
    """Every row of the decision table has a robust case under both Newton modes' configurations that can reach it, and every listed edge
    is present."""
    rows = {}
    for cfg, case, o in outcomes():
        if case.robust:
            rows.setdefault(o.row, set()).add((cfg.sh["newton_mode"], cfg.sh["step_rule"]))
    for row in R.ROWS:
        assert row in rows, row
    assert all((1, 0) in rows[r] for r in R.ROWS)
    assert all((0, 1) in rows[r] for r in R.ROWS if r not in ("retry_stale", "status_nonzero", "accept_end"))
    edges = {e for cfg in configs() for k in cfg.cases for e in k.edges}
    missing = [e for e in Cs.REQUIRED_EDGES if e not in edges]
    assert not missing, missing
    # every factor branch of both step rules
    kinds = set()
    for cfg, case, o in outcomes():
        if o.next is not None and o.row in ("accept", "reject") and getattr(o, "norms", {}).get("tested"):
            kinds.add((cfg.sh["step_rule"], o.row, case.st["ord"], o.next["h"][0]))
    for want in [(0, "accept", 1, "real"), (0, "accept", 2, "real"), (0, "accept", 3, "real"), (0, "accept", 2, "bits"), (0, "reject", 1, "real"),
                 (0, "reject", 2, "real"), (0, "reject", 3, "real"), (0, "reject", 1, "bits"), (1, "accept", 1, "real"), (1, "accept", 2, "real"),
                 (1, "accept", 3, "real"), (1, "accept", 3, "bits"), (1, "reject", 1, "real"), (1, "reject", 2, "real"), (1, "reject", 3, "real"),
                 (1, "reject", 3, "bits")]:
        assert want in kinds, want
    # the shapes
    assert {len(c.sh["atol"]) for c in configs() if "g64" in c.policies} >= set(Cs.N64)
    assert {len(c.sh["atol"]) for c in configs() if "g256" in c.policies} >= set(Cs.N256)


def _small_configs():
    return [c for c in configs() if len(c.sh["atol"]) <= 65]


def test_comparison_accepts_a_correctly_rounding_device():
    """emulate() rounds the reference's own values once: every comparison must pass, for every case of the small configurations, and no
    case may be left out of it."""
    n = 0
    for cfg in _small_configs():
        for case in cfg.cases:
            g = R.emulate(cfg.sh, case, cfg.op)
            ck = R.check_update_case(cfg.sh, case, g) if cfg.op == 1 else R.check_prepare_case(cfg.sh, case, g)
            assert ck.n_checked > 20
            assert all(v <= 1.0 for v in ck.worst.values())
            n += 1
    assert n == sum(len(c.cases) for c in _small_configs())


MUTATIONS = {
    # name -> (change of RULE, (config, case) that must fail, the quantity named in the failure)
    "order-2 error constant 1 % off": (lambda r: r["errc_scale"].__setitem__(2, F(101, 100)), ("A.n65", "accept.first"), "h_next"),
    "accept test < instead of <=": (lambda r: r.__setitem__("accept_strict", True), ("G.n1", "accept.errn_eq_1"), ""),
    "upper clamp of the accepted step 1.9": (lambda r: r.__setitem__("acc_hi", 1.9), ("A.n65", "accept.rate.fac_hi"), "h"),
    "history not reset on landing": (lambda r: r.__setitem__("land_nhist", None), ("A.n65", "accept.land"), "nhist"),
    "lower clamp of the rejected step 0.2": (lambda r: r.__setitem__("rej_lo", 0.2), ("A.n65", "reject.fac_lo"), "h"),
    "IDA rejected-step floor 0.3": (lambda r: r.__setitem__("eta_rej_lo", 0.3), ("B.n65", "reject.ord3.lo"), "h"),
    "rate limit 1.1": (lambda r: r.__setitem__("nl_rate", 1.1), ("A.n65", "diverge.retry"), ""),
}


@pytest.mark.parametrize("name", sorted(MUTATIONS))
def test_cases_tell_mutated_rules_apart(name):
    """A controller with one rule changed (emulate under a changed RULE) must fail the comparison at the named case."""
    change, (cfg_name, case_name), what = MUTATIONS[name]
    cfg = next(c for c in configs() if c.name == cfg_name)
    case = next(k for k in cfg.cases if k.name == case_name)
    saved = copy.deepcopy(R.RULE)
    try:
        change(R.RULE)
        g = R.emulate(cfg.sh, case, cfg.op)
    finally:
        R.RULE.clear()
        R.RULE.update(saved)
    with pytest.raises(AssertionError, match="case %s: %s" % (case_name.replace(".", r"\."), what)):
        R.check_update_case(cfg.sh, case, g)
