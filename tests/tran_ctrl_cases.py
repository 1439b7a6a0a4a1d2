"""TEST INFRASTRUCTURE -- the states on which the transient controller is called once (tests/test_gpu_tran_ctrl.py on the GPU,
tests/test_tran_ctrl_ref_cpu.py for the conditions the cases themselves must meet).  The reference is tests/tran_ctrl_ref.py.

A Config is one launch: the arrays and scalars every instance shares, and its cases (one instance each).  Values are seeded random:
magnitudes of the unknowns over 1e-12 .. 1e3 (atol and reltol |x| each dominate somewhere), steps over 1e-15 .. 1e-6 with ratios h / hprev
over 0.1 .. 10.  A ROBUST case is placed -- by scaling the Newton step and the distance from the predictor, aimed in doubles, verified by
the exact reference -- at least 1e-6 relative away from every threshold its row compares against; an EDGE case sits on a threshold that
doubles hit by construction (``edges`` names it) and is decided by the reference's exact rules.
"""
import math

import numpy as np

from tests import tran_ctrl_ref as R

T1 = 1e-3
BREAKS = (2e-4, 2.00001e-4, 5e-4, T1, 2e-3)        # two close together, one equal to t1, one beyond it
SAVE_T = (1e-5, 2e-5, 2.00001e-5, 2.00002e-5, 5e-5, 1e-4, 4e-4, 9e-4)
HMIN, HMAX = 2.5e-16, 1e-6
MAX_NEWTON = 10
N64 = (1, 63, 64, 65, 200)
N256 = (5, 256, 257, 600)
up_ = lambda x: float(np.nextafter(x, math.inf))
dn_ = lambda x: float(np.nextafter(x, -math.inf))


class Case:
    def __init__(self, name, st, vec, extra, flags, cnt, row, robust, edges):
        self.name, self.st, self.vec, self.extra, self.flags, self.cnt = name, st, vec, extra, flags, cnt
        self.row, self.robust, self.edges = row, robust, tuple(edges)


class Config:
    def __init__(self, name, op, sh, policies, cases):
        self.name, self.op, self.sh, self.policies, self.cases = name, op, sh, tuple(policies), cases

    @property
    def fixed_form(self):
        s = self.sh
        return s["newton_mode"] == 1 and s["step_rule"] == 0 and s["max_order"] == 2 and s["use_pcnr"] == 0 and len(s["atol"]) <= 256

    def states(self):
        out = []
        for c in self.cases:
            s, e = c.st, c.extra
            out.append(dict(t=s["t"], h=s["h"], hprev=s["hprev"], hpp=s["hpp"], tcur=s["tn"], gamma=s["a0"], mn_a0f=s["a0f"], mn_ss=s["ss"],
                            mn_dnp=s["dnp"], hp3=s["hp3"], dsc=e["dsc"], p_t=e["p_t"], p_h=e["p_h"], p_hprev=e["p_hprev"], p_hpp=e["p_hpp"],
                            nhist=s["nhist"], order=s["ord"], k=s["k"], status=s["status"], bp_idx=s["bp"], save_idx=s["si"], flags=c.flags,
                            mn_flags=s["mflags"], p_nhist=e["p_nhist"], cnt=c.cnt))
        return out

    def vecs(self):
        return {k: np.array([c.vec[k] for c in self.cases]) for k in R.VECS}


def make_shared(n, seed, mode, rule, max_order, pcnr=0, n_limits=0, n_obs=1, emask="mixed"):
    rng = np.random.default_rng(seed)
    atol = rng.choice([1e-12, 1e-9, 1e-6], n)
    if emask == "zero":
        em = np.zeros(n)
    else:
        em = (rng.random(n) < 0.6).astype(np.float64)
        em[rng.integers(n)] = 1.0
    if n_obs == 1:
        obs = np.array([n - 1], dtype=np.int32)
    else:
        obs = rng.integers(0, n, n_obs).astype(np.int32)       # unordered, with repeats
        obs[1] = obs[0]
        obs[-1] = n - 1
    return dict(n_limits=min(n_limits, n), n_err=int(em.sum()), max_newton=MAX_NEWTON, max_order=max_order, use_pcnr=pcnr, newton_mode=mode,
                step_rule=rule, t0=0.0, t1=T1, reltol=1e-4, h0=1e-9, hmin=HMIN, hmax=HMAX, newton_tol=1e-3, atol=atol, emask=em,
                breaks=np.array(BREAKS), save_t=np.array(SAVE_T), obs=obs)


def _signed(rng, n, lo=0.3, hi=3.0):
    return rng.uniform(lo, hi, n) * np.where(rng.random(n) < 0.5, -1.0, 1.0)


def _history(rng, n):
    u0 = 10.0 ** rng.uniform(-12, 3, n) * np.where(rng.random(n) < 0.5, -1.0, 1.0)
    u1 = u0 * (1 + 1e-2 * rng.standard_normal(n))
    u2 = u1 * (1 + 1e-2 * rng.standard_normal(n))
    u3 = u2 * (1 + 1e-2 * rng.standard_normal(n))
    return u0, u1, u2, u3


def update_case(sh, rng, name, row, t=3.0e-4, h=None, nhist=3, k=0, dn=1e-6, errn=0.3, jcur=True, since=3, ss=20.0, rate=None, dsc=1.0, flags=0,
                bp=None, si=None, status=0, robust=True, edges=(), tn=None, same_as_predictor=False, poke=None, cnt=(5, 3, 1, 0)):
    """A state in the middle of a step from t (a step of about ``h`` with random earlier steps), the iterate at the distance from the predictor
    that gives the error estimate ``errn`` and a Newton step of weighted norm ``dn``; ``rate``: dn / (the previous update's norm)."""
    n = len(sh["atol"])
    if h is None:
        h = 10.0 ** rng.uniform(-14, -6.7)
    r = 10.0 ** rng.uniform(-1, 1, 3)
    hprev = h / r[0]; hpp = hprev / r[1]; hp3 = hpp / r[2]
    if bp is None:
        bp = int(np.searchsorted(np.array(BREAKS), t, side="right"))
    h, tn0, _ = R.clip(sh, t, h, bp)
    hist = _history(rng, n)
    pr = R.prepare(sh, t, h, nhist, hprev, hpp, hp3, bp)
    up, beta = R.prepared_floats(pr, hist)
    a0 = float(pr.a0)
    wt = sh["atol"] + sh["reltol"] * np.abs(hist[0])
    if same_as_predictor:
        delta, u = np.zeros(n), up.copy()
    else:
        delta = _signed(rng, n) * wt
        delta *= dn / (abs(dsc) * math.sqrt(np.mean((delta / wt) ** 2)))
        E = _signed(rng, n) * wt
        u = up + E + delta * dsc
        if nhist >= 2 and sh["n_err"] > 0:
            errc = float(R.error_constant(pr.ord, h, hprev, hpp, hp3)[0])
            for _ in range(6):            # aim in doubles; the exact reference has the last word (margins, rows)
                un = u - delta * dsc
                w2 = sh["emask"] / (sh["atol"] + sh["reltol"] * np.maximum(np.abs(hist[0]), np.abs(un)))
                E *= errn / (errc * math.sqrt(np.sum(((un - up) * w2) ** 2) / sh["n_err"]))
                u = up + E + delta * dsc
    if si is None:
        si = int(np.searchsorted(np.array(SAVE_T), (tn0 if tn is None else tn) * (1 + 1e-9), side="right"))
    mflags = R.MN_VALID | (R.MN_JCUR if jcur else 0) | (since << R.MN_SINCE_SHIFT)
    st = dict(t=t, h=h, hprev=hprev, hpp=hpp, hp3=hp3, tn=tn0 if tn is None else tn, a0=a0, nhist=nhist, ord=pr.ord, k=k, status=status, bp=bp,
              si=si, a0f=a0 * float(rng.uniform(0.8, 1.2)), ss=ss, dnp=(dn / rate if rate else 0.0), dsc=dsc, mflags=mflags)
    vec = dict(u=u, du=a0 * u + beta, delta=delta, limit_w=_signed(rng, n), u0=hist[0], u1=hist[1], u2=hist[2], u3=hist[3], up=up, beta=beta)
    extra = dict(dsc=dsc, p_t=t, p_h=h, p_hprev=hprev, p_hpp=hpp, p_nhist=nhist)
    c = Case(name, st, vec, extra, flags, cnt, row, robust, edges)
    if poke:
        poke(c)
    return c


def prepare_case(sh, rng, name, t, h, nhist, bp, edges=(), jcur=True, status=0):
    """op 0: prepare_step(t, h, nhist, hprev, hpp) on a loaded state whose own t / h / tn differ from the arguments."""
    n = len(sh["atol"])
    r = 10.0 ** rng.uniform(-1, 1, 3)
    hprev = abs(h) / r[0] if h < 1e-3 else 1e-9 / r[0]
    hpp = hprev / r[1]; hp3 = hpp / r[2]
    hist = _history(rng, n)
    junk = lambda: _signed(rng, n)
    st = dict(t=t * 0.75, h=h * 3.0, hprev=hprev * 1.5, hpp=hpp * 0.5, hp3=hp3, tn=t * 0.8, a0=123.0, nhist=2, ord=2, k=4, status=status, bp=bp, si=3,
              a0f=7.0, ss=3.0, dnp=0.25, dsc=1.0, mflags=R.MN_VALID | (R.MN_JCUR if jcur else 0) | (5 << R.MN_SINCE_SHIFT))
    vec = dict(u=junk(), du=junk(), delta=junk(), limit_w=junk(), u0=hist[0], u1=hist[1], u2=hist[2], u3=hist[3], up=junk(), beta=junk())
    extra = dict(dsc=0.5, p_t=t, p_h=h, p_hprev=hprev, p_hpp=hpp, p_nhist=nhist)
    return Case(name, st, vec, extra, 1, (1, 2, 3, 4), None, False, edges)


# ---- the case lists ----------------------------------------------------------------------------------------------------------------------
def _find_h(target, fac):
    """A double h with fl(h * fac) == target."""
    h = target / fac
    for _ in range(64):
        p = float(np.float64(h) * np.float64(fac))
        if p == target:
            return h
        h = up_(h) if p < target else dn_(h)
    raise AssertionError("no h with h * %r == %r" % (fac, target))


def _poke_delta(i, val):
    def f(c):
        c.vec["delta"] = c.vec["delta"].copy()
        c.vec["delta"][i] = val
    return f


def cases_mode1(sh, rng, full, nt, bad_spots):
    """Newton mode 1, step rule 0, max_order 2 (what the fixed form fixes)."""
    n = len(sh["atol"])
    U = lambda *a, **k: update_case(sh, rng, *a, **k)
    cs = [
        U("continue.k0", "continue", dn=0.05, jcur=False),
        U("continue.rate", "continue", k=2, dn=1.0, rate=0.5),
        U("accept.first", "accept", dn=1e-5, errn=0.3),
        U("accept.ss_k0", "accept", dn=1e-3, errn=0.5),
        U("accept.rate.fac_hi", "accept", k=1, dn=0.1, rate=0.1, errn=1e-3),
        U("accept.ord1", "accept", nhist=2, errn=0.5),
        U("accept.untested", "accept", nhist=1),
        U("reject.mid", "reject", errn=3.0),
        U("reject.fac_lo", "reject", nhist=2, errn=200.0),
        U("diverge.retry", "retry_stale", k=1, dn=1.0, rate=1.0, jcur=False),
        U("diverge.shrink", "fail_shrink", k=1, dn=1.0, rate=1.0),
        U("accept.land", "accept", t=BREAKS[2] - 1e-9, h=2e-9, errn=0.3),
        U("accept_end", "accept_end", t=T1 - 1e-9, h=2e-9, bp=4, errn=0.3),
        U("accept.save3", "accept", t=1.99e-5, h=2e-7, si=1, errn=0.4),
    ]
    k_last = MAX_NEWTON - 1
    if full:
        cs += [
            U("reject.ord1", "reject", nhist=2, errn=4.0),
            U("reject_hmin", "reject_hmin", h=5 * HMIN, nhist=2, errn=200.0),
            U("maxnewton.shrink", "fail_shrink", k=k_last, dn=1.0, rate=0.5),
            U("maxnewton.retry", "retry_stale", k=k_last, dn=1.0, rate=0.5, jcur=False),
            U("maxnewton.before", "continue", k=k_last - 1, dn=1.0, rate=0.5, jcur=False, robust=False, edges=("k=max_newton-2",)),
            U("maxnewton.last", "fail_shrink", k=k_last, dn=1.0, rate=0.5, robust=False, edges=("k=max_newton-1",)),
            U("fail_hmin", "fail_hmin", h=2 * HMIN, flags=1),
            U("bad.retry", "retry_stale", flags=1, jcur=False, edges=("bad.flag", "retry.same_h")),
            U("bad.shrink", "fail_shrink", flags=1, edges=("bad.flag", "fail.quarter")),
            U("accept.land.close", "accept", t=BREAKS[0] - 1e-9, h=2e-9, bp=0, edges=("land.two_breaks",)),
            U("accept.land.hsmall", "accept", t=BREAKS[0] - 1e-10, h=2e-10, bp=0, edges=("land.two_breaks",)),
            U("accept_end.break_eq_t1", "accept_end", t=T1 - 1e-9, h=2e-9, bp=3, edges=("break==t1",)),
            U("accept_end.break_beyond", "accept_end", t=T1 - 1e-9, h=2e-9, bp=4, edges=("break>t1",)),
            U("accept.hmax", "accept", h=0.8e-6, errn=1e-3),
            U("accept.hmin_raise", "accept", h=HMIN, errn=0.9),
            U("accept.save1", "accept", t=0.99e-5, h=2e-7, si=0),
            U("accept.save1.nhist1", "accept", t=0.99e-5, h=2e-7, si=0, nhist=1, edges=("save.nhist1",)),
            U("accept.save0", "accept", t=6e-5, h=2e-7, si=5, edges=("save.none",)),
            U("accept.save.eq_tn", "accept", t=SAVE_T[4] - 1e-7, h=1e-7, si=4, tn=SAVE_T[4], robust=False, edges=("save==tn",)),
            U("accept.save.ulp_above", "accept", t=SAVE_T[4] - 1e-7, h=1e-7, si=4, tn=dn_(SAVE_T[4]), robust=False, edges=("save=tn+ulp",)),
            U("accept.save.4e-15", "accept", t=SAVE_T[4] - 1e-7, h=1e-7, si=4, tn=SAVE_T[4] * (1 - 4e-15), robust=False, edges=("save=tn(1+4e-15)",)),
            U("status_nonzero", "status_nonzero", status=1),
            U("accept.errn0", "accept", same_as_predictor=True, robust=False, edges=("errn==0",)),
            U("accept.dsc", "accept", dsc=0.7, errn=0.6, edges=("dsc!=1",)),
            U("continue.dsc", "continue", dsc=0.6, dn=0.05, edges=("dsc!=1",)),
            U("k0.below", "accept", dn=0.33e-4 * (1 - 1e-3), ss=2e4, edges=("k0.dnorm<0.33e-4",)),
            U("k0.above", "continue", dn=0.33e-4 * (1 + 1e-3), ss=2e4, edges=("k0.dnorm>0.33e-4",)),
            U("dnp0", "accept", k=1, dn=0.2, rate=None, edges=("dnp==0",)),
            U("accept.jcur_cleared", "accept", jcur=True, since=19, edges=("jcur.cleared", "since.advances")),
            U("fail.hn_eq_hmin", "fail_shrink", h=4 * HMIN, flags=1, robust=False, edges=("fail.hn==hmin",)),
            U("fail.hn_below_hmin", "fail_hmin", h=4 * dn_(HMIN), flags=1, robust=False, edges=("fail.hn<hmin",)),
            U("reject.hn_eq_hmin", "reject", h=_find_h(HMIN, 0.1), nhist=2, errn=200.0, robust=False, edges=("reject.hn==hmin",)),
            U("reject.hn_below_hmin", "reject_hmin", h=_find_h(dn_(HMIN), 0.1), nhist=2, errn=200.0, robust=False, edges=("reject.hn<hmin",)),
        ]
    # a NaN and an Inf in the Newton step: first element, last lane of the last wave, beyond NT, last element
    spots = sorted({0, min(nt, n) - 1, min(nt, n - 1), n - 1}) if bad_spots else ()
    for i in spots:
        for val, tag in ((math.nan, "nan"), (math.inf, "inf")):
            jc = (i + (tag == "inf")) % 2 == 0
            cs.append(U("bad.%s@%d" % (tag, i), "fail_shrink" if jc else "retry_stale", jcur=jc, poke=_poke_delta(i, val), robust=False,
                        edges=("bad.%s" % tag, "bad@first" if i == 0 else "bad@last" if i == n - 1 else "bad@lane%d" % i)))
    return cs


def cases_mode0(sh, rng, full):
    """Newton mode 0, step rule 1 (IDA's eta), max_order 3, PCNR copy."""
    U = lambda *a, **k: update_case(sh, rng, *a, **k)
    cs = [
        U("continue.pcnr", "continue", dn=0.05),
        U("accept.ord3.grow", "accept", nhist=4, errn=1e-3),
        U("accept.ord3.keep", "accept", nhist=4, errn=0.1),
        U("accept.ord3.shrink", "accept", nhist=4, errn=0.9),
        U("accept.ord2.shrink", "accept", nhist=3, errn=0.9),
        U("reject.ord3", "reject", nhist=4, errn=5.0),
        U("shrink.maxnewton", "fail_shrink", k=MAX_NEWTON - 1, dn=0.05),
    ]
    if not full:
        return cs
    cs += [
        U("accept.ord3.eta_hi", "accept", nhist=4, errn=0.6),
        U("accept.ord1.shrink", "accept", nhist=2, errn=0.9),
        U("accept.ord2.grow", "accept", nhist=3, errn=1e-3),
        U("reject.ord3.lo", "reject", nhist=4, errn=200.0),
        U("reject.ord2", "reject", nhist=3, errn=3.0),
        U("reject.ord1", "reject", nhist=2, errn=2.0),
        U("shrink.bad", "fail_shrink", flags=1),
        U("fail_hmin", "fail_hmin", h=3 * HMIN, flags=1),
        U("reject_hmin", "reject_hmin", h=3 * HMIN, errn=200.0, nhist=4),
        U("tol.below", "accept", dn=1e-3 * (1 - 1e-3), nhist=4, edges=("newton_tol.below",)),
        U("tol.above", "continue", dn=1e-3 * (1 + 1e-3), nhist=4, edges=("newton_tol.above",)),
        U("accept.depth4", "accept", nhist=3, errn=0.2, edges=("nhist 3->4",)),
        U("accept.ord3.land", "accept", nhist=4, t=BREAKS[2] - 1e-9, h=2e-9, errn=0.3),
        U("accept.ord3.save3", "accept", nhist=4, t=1.99e-5, h=2e-7, si=1),
        U("accept.errn0", "accept", nhist=4, same_as_predictor=True, robust=False, edges=("errn==0",)),
        U("accept.untested", "accept", nhist=1),
    ]
    return cs


def cases_small(sh, rng, rows):
    U = lambda *a, **k: update_case(sh, rng, *a, **k)
    return [U(*a, **k) for a, k in rows]


def cases_prepare(sh, rng):
    """op 0: every order the history allows, and the clipping rule on its edges (t, bp: the stop is BREAKS[2] unless said)."""
    P = lambda *a, **k: prepare_case(sh, rng, *a, **k)
    stop, t = BREAKS[2], BREAKS[2] - 1e-8
    rem = float(np.float64(stop) - np.float64(t))
    thr = float(np.float64(rem) * np.float64(R.RULE["land"]))
    cs = [P("free.nhist%d" % nh, 3e-4, 10.0 ** rng.uniform(-14, -6.7), nh, 2, edges=("nhist%d" % nh,)) for nh in (1, 2, 3, 4)]
    cs += [
        P("h==rem", t, rem, 3, 2, edges=("h==rem",)),
        P("h==rem(1-1e-9)", t, thr, 3, 2, edges=("h=land threshold",)),
        P("h<rem(1-1e-9)", t, dn_(thr), 4, 2, edges=("h<land threshold",)),
        P("h>rem", t, 1.0, 2, 2, edges=("h>rem",)),
        P("h==rem/2", t, 0.5 * rem, 3, 2, edges=("2h==rem",)),
        P("2h=rem+ulp", t, up_(0.5 * rem), 3, 2, edges=("2h=rem+ulp",)),
        P("break>t1", T1 - 1e-8, 2e-8, 3, 4, edges=("break>t1",)),
        P("break==t1", T1 - 1e-8, 2e-8, 3, 3, edges=("break==t1",)),
        P("no break left", T1 - 1e-8, 1e-9, 3, 5, edges=("bp==n_break",)),
        P("two breaks", BREAKS[0] - 1e-10, 1e-9, 4, 0, edges=("land.two_breaks",)),
        P("jcur clear", 3e-4, 1e-9, 3, 2, jcur=False),
        P("status_nonzero", 3e-4, 1e-9, 3, 2, status=-1),
    ]
    return cs


ROW = lambda *a, **k: (a, k)


def build():
    """Every Config of the suite.  Deterministic."""
    cfgs = []
    seed = 1000
    def rng_of():
        nonlocal seed
        seed += 1
        return np.random.default_rng(seed)
    # A: the fixed form's switches, every n of both group sizes; the full list at n = 65 (one wave) and n = 5 (four waves: the decisions do
    # not depend on n, the reference's cost does), the non-finite Newton steps also where n exceeds the group
    for n in N64 + N256:
        nt = 64 if n in N64 else 256
        sh = make_shared(n, 10 + n, mode=1, rule=0, max_order=2)
        # (n = 5 and 256 also fit one wave and the fixed form's 4 x 64 register-held elements: they run under all three policies)
        pol = ("g64", "fixed") if nt == 64 else ("g256", "g64", "fixed") if n <= 256 else ("g256",)
        cfgs.append(Config("A.n%d" % n, 1, sh, pol, cases_mode1(sh, rng_of(), n in (65, 5), nt, n in (65, 5, 257, 600))))
    # B: mode 0, IDA's step rule, order 3, PCNR
    for n, nlim, full in ((1, 1, False), (65, 1, True), (200, 70, False), (5, 1, True), (257, 70, False), (600, 70, False)):
        sh = make_shared(n, 20 + n, mode=0, rule=1, max_order=3, pcnr=1, n_limits=nlim)
        cfgs.append(Config("B.n%d" % n, 1, sh, ("g64",) if n in N64 else ("g256",), cases_mode0(sh, rng_of(), full)))
    # C: max_order 1 keeps order 1 and the linear predictor however deep the history;  D: order 3 under step rule 0 and Newton mode 1
    # E: nothing is error-tested (n_err = 0);  F: many observers, unordered and repeated
    for n, pol in ((63, "g64"), (257, "g256")):
        sh = make_shared(n, 30 + n, mode=0, rule=0, max_order=1)
        cfgs.append(Config("C.n%d" % n, 1, sh, (pol,), cases_small(sh, rng_of(), [
            ROW("accept.max_order1", "accept", nhist=3, errn=0.3, edges=("max_order=1",)), ROW("reject.max_order1", "reject", nhist=3, errn=3.0)])))
        sh = make_shared(n, 40 + n, mode=1, rule=0, max_order=3)
        cfgs.append(Config("D.n%d" % n, 1, sh, (pol,), cases_small(sh, rng_of(), [
            ROW("accept.ord3", "accept", nhist=4, errn=0.3, edges=("order3",)), ROW("reject.ord3", "reject", nhist=4, errn=3.0),
            ROW("accept.ord3.fac_hi", "accept", nhist=4, errn=1e-4), ROW("retry.ord3", "retry_stale", nhist=4, flags=1, jcur=False)])))
        sh = make_shared(n, 50 + n, mode=1, rule=0, max_order=2, emask="zero")
        cfgs.append(Config("E.n%d" % n, 1, sh, (pol, "fixed") if pol == "g64" else (pol,), cases_small(sh, rng_of(), [
            ROW("accept.n_err0", "accept", nhist=3, robust=False, edges=("n_err==0",)), ROW("accept.n_err0.nhist1", "accept", nhist=1, robust=False, edges=("nhist==1",))])))
    for n, pol in ((200, ("g64", "fixed")), (600, ("g256",))):
        sh = make_shared(n, 60 + n, mode=1, rule=0, max_order=2, n_obs=300)
        cfgs.append(Config("F.n%d" % n, 1, sh, pol, cases_small(sh, rng_of(), [
            ROW("accept.save3.obs300", "accept", t=1.99e-5, h=2e-7, si=1, edges=("n_obs=300",)),
            ROW("accept.save1.nhist1.obs300", "accept", t=0.99e-5, h=2e-7, si=0, nhist=1, edges=("n_obs=300",)),
            ROW("reject.obs300", "reject", t=1.99e-5, h=2e-7, si=1, errn=3.0)])))
    # G: an error estimate of exactly 1 -- order 1 with hprev = h (errc = 1 / 2), one tested unknown with atol = 1 / 2, u0 = 0, u_new = 0 and the
    # predictor at -1 (e w2 = 2): every operation is exact in doubles, and errn <= 1 accepts
    def errn_one(c):
        c.st.update(hprev=c.st["h"], nhist=2, ord=1, a0=1.0 / c.st["h"])
        for k in ("u", "u0", "delta", "up"):
            c.vec[k] = c.vec[k].copy()
        c.vec["delta"][:] = 0.0
        c.vec["u"][0], c.vec["u0"][0], c.vec["up"][0] = 0.0, 0.0, -1.0
    for n, pol in ((1, ("g64", "fixed")), (5, ("g256", "g64", "fixed"))):
        sh = make_shared(n, 95 + n, mode=1, rule=0, max_order=2)
        sh["atol"][:] = 0.5
        sh["emask"][:] = 0.0
        sh["emask"][0] = 1.0
        sh["n_err"] = 1
        cfgs.append(Config("G.n%d" % n, 1, sh, pol, cases_small(sh, rng_of(), [
            ROW("accept.errn_eq_1", "accept", nhist=2, h=2.0 ** -30, robust=False, edges=("errn==1",), poke=errn_one)])))
    # P: prepare_step alone -- every order, the clipping edges
    for n in N64 + N256:
        sh = make_shared(n, 70 + n, mode=0, rule=0, max_order=3)
        cfgs.append(Config("P3.n%d" % n, 0, sh, ("g64",) if n in N64 else ("g256",), cases_prepare(sh, rng_of())))
    for n, pol in ((65, ("g64", "fixed")), (257, ("g256",))):
        sh = make_shared(n, 80 + n, mode=1, rule=0, max_order=2)
        cfgs.append(Config("P2.n%d" % n, 0, sh, pol, cases_prepare(sh, rng_of())))
    sh = make_shared(63, 93, mode=0, rule=0, max_order=1)
    cfgs.append(Config("P1.n63", 0, sh, ("g64",), cases_prepare(sh, rng_of())))
    return cfgs


# every edge the suite must hold (tests/test_tran_ctrl_ref_cpu.py asserts that each is present)
REQUIRED_EDGES = (
    "errn==0", "errn==1", "n_err==0", "nhist==1", "h==rem", "h=land threshold", "h<land threshold", "2h==rem", "2h=rem+ulp", "break>t1", "break==t1",
    "land.two_breaks", "fail.hn==hmin", "fail.hn<hmin", "reject.hn==hmin", "reject.hn<hmin", "k=max_newton-2", "k=max_newton-1",
    "k0.dnorm<0.33e-4", "k0.dnorm>0.33e-4", "dnp==0", "retry.same_h", "fail.quarter", "jcur.cleared", "since.advances", "dsc!=1", "bad.flag",
    "bad.nan", "bad.inf", "bad@first", "bad@last", "order3", "nhist 3->4", "max_order=1", "save.none", "save.nhist1", "save==tn", "save=tn+ulp",
    "save=tn(1+4e-15)", "n_obs=300", "newton_tol.below", "newton_tol.above",
)
