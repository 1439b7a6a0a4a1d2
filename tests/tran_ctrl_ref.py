"""TEST INFRASTRUCTURE -- an independent reference of the transient step controller (csrc/tran_ctrl.hpp: prepare_step, tran_update_body,
save_outputs), for ONE call on a given state (tests/test_gpu_tran_ctrl.py runs the call on the GPU through tests/prim_probe.py,
tests/test_tran_ctrl_ref_cpu.py checks this reference itself).

Nothing here is taken from tran_ctrl.hpp or oracle/cpu_port.cpp but the RULES, restated from their definitions; all real arithmetic is
exact (``fractions.Fraction``: a double is a rational), the square / cube / fourth roots come from mpmath at 60 digits.

* Discretisation.  The step from t to t_n = t + h on the history t, t - hprev, t - hprev - hpp, t - hprev - hpp - hp3.  Order: 1 while fewer
  than three points are known (nhist <= 2) or max_order < 2; 3 when four are known and max_order >= 3; 2 otherwise.  a0 and the history
  weights are the derivatives at t_n of the Lagrange basis on the ord + 1 newest points, t_n among them (tran_ref.lagrange_derivatives, on the
  exact node distances); beta = sum_j alpha_j u_{n-j}; the predictor is the polynomial through the last ord + 1 accepted points continued
  to t_n (tran_ref.lagrange_values), the constant u_{n-1} while one point is known (nhist <= 1).
* Error constant, from its definition: errc_k = 1 / (a0 (t_n - t_{n-k-1})), the principal local-error coefficient of variable-step BDF-k
  against the (k + 1)-th divided difference (tests/test_tran_ctrl_ref_cpu.py checks it on monomials).
* Norms.  dnorm = sqrt(sum((d w)^2) / n), w = 1 / (atol + reltol |x0|), d = delta dsc;  errn = errc sqrt(sum((e w2)^2) / n_err),
  e = u_new - predictor, w2 = emask / (atol + reltol max(|x0|, |u_new|)), u_new = u - d.
* The decision table: ``update`` below, one row per outcome (ROWS), written as conditions -> next state.
* Clipping, landing and the save-time test are rules ON DOUBLES (``clip``, ``saves_due``): evaluated in numpy.float64, compared to the bit.
* Save-time interpolants: the quadratic through (t_n, u_new), (t, u0), (t - hprev, u1) when nhist >= 2, the straight line through the first
  two when nhist == 1; a save time is due while t_save <= t_n (1 + 1e-15).

Tolerance model (tests/prim_ref.py, tests/stamp_ref.py):  |got - ref| <= gamma_k * (sum of the absolute terms), gamma_k = k u / (1 - k u),
u = 2^-53, k counted from the operations an evaluation in doubles needs -- written next to every check.  A division counts as one operation
(fast_div is correctly rounded in the range of these cases, tests/test_gpu_primitives.py).  A difference of two node positions, each a
rounded sum of up to three step sizes, is charged 3 u (|a| + |b|): that is where the conditioning of a stencil enters (POS_OPS).
One bound is the project's, not derived: step_root at order 2 (tran_ctrl.hpp: relative error up to 9.33e-8, held to the port bit for bit by
tests/test_gpu_primitives.py) -- the next step of such cases is compared at 1.0e-7 relative (ROOT2_REL).
"""
import math
from fractions import Fraction as F

import numpy as np

from tests import tran_ref

U = F(1, 2 ** 53)
f64 = np.float64
MN_NEED, MN_JCUR, MN_VALID, MN_SINCE_SHIFT = 1, 2, 4, 8
ROOT2_REL = F(1, 10 ** 7)           # the allowance of a step that went through step_root at order 2 (module docstring)
ROOT2_OWN = F(933, 10 ** 10)        # what tran_ctrl.hpp states for step_root itself; the rest of ROOT2_REL is for errn and the products
POS_OPS = 3                         # roundings charged to a difference of two node positions (module docstring)
MARGIN = 1e-6                       # a robust case keeps this relative distance from every threshold it is compared against

# The constants of the rules (doubles, as the options and IDA's constants are given).  A scratch copy with one of them changed is how the
# cases are shown to bite (tests/test_tran_ctrl_ref_cpu.py: test_cases_tell_mutated_rules_apart).
RULE = {
    "land": 1.0 - 1e-9,        # h >= rem * land: take the whole remainder and land on the stop
    "save_slack": 1.0 + 1e-15,
    "safety": 0.9,
    "acc_lo": 0.2, "acc_hi": 2.0,          # step rule 0, accepted step
    "rej_lo": 0.1, "rej_hi": 0.9,          # step rule 0, rejected step
    "eta_eps": 1e-4, "eta_grow": 2.0, "eta_keep": 1.0, "eta_lo": 0.5, "eta_hi": 0.9,   # step rule 1 (IDA), accepted step
    "eta_rej_lo": 0.25, "eta_rej_hi": 0.9,                                                # step rule 1, rejected step
    "untested": 2.0, "land_frac": 0.1, "fail_frac": 0.25,
    "nl_first": 0.33e-4, "nl_tol": 0.33, "nl_rate": 0.9,                                  # Newton mode 1 (IDA's nonlinear convergence test)
    "errn_max": 1.0,
    "accept_strict": False,    # a scratch mutation: errn < 1 instead of errn <= 1
    "land_nhist": 1,           # history depth after landing on a breakpoint (None: not reset -- a scratch mutation)
    "errc_scale": {1: 1, 2: 1, 3: 1},      # a scratch mutation scales one order's error constant
}
ROWS = ("status_nonzero", "retry_stale", "fail_shrink", "fail_hmin", "continue", "reject", "reject_hmin", "accept", "accept_end")


def gamma(k):
    k = F(k)
    return k * U / (1 - k * U)


def fr(x):
    return x if isinstance(x, F) else F(float(x))


def _mp(x):
    import mpmath as mp
    return mp.mpf(x.numerator) / mp.mpf(x.denominator)


def _to_frac(x):
    """An mpmath number as a Fraction (its 60 digits: the error is 1e-60 relative, nothing next to 2^-53)."""
    import mpmath as mp
    m, e = mp.frexp(x)
    return F(int(mp.floor(mp.ldexp(m, 220)))) * F(2) ** (int(e) - 220)


def root(x, p):
    """x^(1/p) of a non-negative Fraction, at 60 digits."""
    import mpmath as mp
    if x == 0:
        return F(0)
    with mp.workdps(60):
        return _to_frac(mp.root(_mp(x), p))


# ---- stencils ------------------------------------------------------------------------------------------------------------------------------
def positions(h, hprev, hpp, hp3):
    """Exact positions relative to t of t_n and the four last accepted points."""
    h, hprev, hpp, hp3 = fr(h), fr(hprev), fr(hpp), fr(hp3)
    return [h, F(0), -hprev, -(hprev + hpp), -(hprev + hpp + hp3)]


def order_of(nhist, max_order):
    """(order, number of points of the predictor)."""
    if nhist <= 1:
        return 1, 1
    if nhist == 2 or max_order < 2:
        return 1, 2
    if nhist >= 4 and max_order >= 3:
        return 3, 4
    return 2, 3


def _diff_err(a, b):
    """Bound of the error of a computed difference of two node positions (module docstring)."""
    return POS_OPS * U * (abs(a) + abs(b))


def value_weights(nodes, x):
    """[(l_j(x), bound of its error in doubles)] for the Lagrange basis on ``nodes``.  l_j = prod (x - x_m) / prod (x_j - x_m): every factor
    is charged _diff_err (first order: each times the partial derivative of l_j with respect to it), the 2 (m - 1) products and the division
    2 m - 1 roundings on |l_j|; a factor that is exactly zero (a save time on a node) stays in the bound through the other factors."""
    w = tran_ref.lagrange_values(nodes, x)
    out = []
    m = len(nodes) - 1
    for j, xj in enumerate(nodes):
        others = [xm for i, xm in enumerate(nodes) if i != j]
        den = F(1)
        for xm in others:
            den *= xj - xm
        e = gamma(2 * m - 1) * abs(w[j]) if m else F(0)
        for i, xm in enumerate(others):
            rest = F(1)
            for l, xl in enumerate(others):
                if l != i:
                    rest *= x - xl
            e += _diff_err(x, xm) * abs(rest / den)                  # numerator factor x - x_m
            e += _diff_err(xj, xm) / abs(xj - xm) * abs(w[j])        # denominator factor x_j - x_m
        out.append((w[j], e))
    return out


def deriv_weights(nodes):
    """[(alpha_j, bound)]: derivatives at nodes[0] of the Lagrange basis.  alpha_j is a sum of m products of up to 2 m - 1 factors; with A_j
    the sum of the magnitudes of those products and kappa the worst (|a| + |b|) / |a - b| over the node pairs, every factor carries
    POS_OPS kappa roundings and every product its 2 m - 1 multiplications and divisions, the sum m - 1 more:
    k = (2 m - 1) (POS_OPS kappa + 1) + m - 1 on A_j."""
    al = tran_ref.lagrange_derivatives(nodes, nodes[0])
    m = len(nodes) - 1
    kappa = max((abs(a) + abs(b)) / abs(a - b) for i, a in enumerate(nodes) for b in nodes[i + 1:])
    k = (2 * m - 1) * (POS_OPS * math.ceil(kappa) + 1) + m - 1
    out = []
    x = nodes[0]
    for j, xj in enumerate(nodes):
        A = F(0)
        for i, xm in enumerate(nodes):
            if i == j:
                continue
            p = 1 / abs(xj - xm)
            for l, xl in enumerate(nodes):
                if l != j and l != i:
                    p *= abs(x - xl) / abs(xj - xl)
            A += p
        out.append((al[j], gamma(k) * A))
    return out


def error_constant(ord_, h, hprev, hpp, hp3):
    """(errc_k, relative bound): 1 / (a0 (t_n - t_{n-k-1})) -- a0 with its own bound, the k + 1 step sizes summed (k roundings), a product
    and a division."""
    pos = positions(h, hprev, hpp, hp3)
    a0, ea0 = deriv_weights(pos[:ord_ + 1])[0]
    span = pos[0] - pos[ord_ + 1]
    errc = 1 / (a0 * span) * RULE["errc_scale"][ord_]
    return errc, ea0 / abs(a0) + gamma(ord_ + 2)


# ---- rules on doubles ----------------------------------------------------------------------------------------------------------------------
def stop_of(sh, bp):
    """The next stop: the next breakpoint if it lies before t1, else t1."""
    br = sh["breaks"]
    tb = float(br[bp]) if bp < len(br) else math.inf
    return (tb if tb < sh["t1"] else float(sh["t1"])), tb


def clip(sh, t, h, bp):
    """(h, t_n, branch) of a proposed step: within (1 - 1e-9) of the remainder to the next stop (or beyond) the step takes the whole remainder
    and t_n IS the stop; a step that would leave less than itself takes half the remainder; else it stands.  In doubles, rem one subtraction."""
    tstop, _ = stop_of(sh, bp)
    t, h = f64(t), f64(h)
    rem = f64(tstop) - t
    if h >= rem * f64(RULE["land"]):
        return float(rem), float(tstop), "land"
    if f64(2.0) * h > rem:
        hh = f64(0.5) * rem
        return float(hh), float(t + hh), "half"
    return float(h), float(t + h), "free"


def saves_due(sh, si, tn):
    """Indices of the save times this step reaches: while save_t[si] <= t_n (1 + 1e-15), in doubles."""
    lim = f64(tn) * f64(RULE["save_slack"])
    out = []
    while si < len(sh["save_t"]) and f64(sh["save_t"][si]) <= lim:
        out.append(si)
        si += 1
    return out


# ---- prepare_step ---------------------------------------------------------------------------------------------------------------------------
class Prepared:
    """What the start of a step leaves behind: h, tn (doubles, exact rules), ord, a0 and the vectors with their bounds."""


def prepare(sh, t, h, nhist, hprev, hpp, hp3, bp):
    """The step that starts at t with the proposed size h.  The vectors are linear in the history: up = sum_j pred_w[j] u_{n-1-j} over the
    predictor's points, beta = sum_j alpha[j] u_{n-1-j} over ord points -- each weight with the bound of its own error (lincomb turns them into
    values and bounds per element)."""
    p = Prepared()
    p.h, p.tn, p.branch = clip(sh, t, h, bp)
    p.ord, p.npts = order_of(nhist, sh["max_order"])
    pos = positions(p.h, hprev, hpp, hp3)
    al = deriv_weights(pos[:p.ord + 1])
    p.a0, p.a0_bound = al[0]
    p.alpha = al[1:]
    p.pred_w = value_weights(pos[1:1 + p.npts], pos[0]) if p.npts > 1 else [(F(1), F(0))]
    # per term one product, then the sum: as many roundings as terms, on the magnitudes of the terms (none where the predictor is u0 itself)
    p.pred_ops = p.npts if p.npts > 1 else 0
    p.beta_ops = p.ord
    return p


def prepared_floats(p, hist):
    """up and beta in doubles (for building a consistent state: the controller takes both from memory)."""
    up = sum(float(w) * np.asarray(hist[j], dtype=np.float64) for j, (w, _) in enumerate(p.pred_w))
    beta = sum(float(a) * np.asarray(hist[j], dtype=np.float64) for j, (a, _) in enumerate(p.alpha))
    return up, beta


# ---- exact vectors: a double is an integer multiple of 2^-SCALE ---------------------------------------------------------------------------
SCALE = 1200
_ONE = 1 << SCALE
_CB = 256          # bits kept of a bound's coefficient (rounded up)


def ints_of(a):
    """[x 2^SCALE] as Python integers, exact, for finite doubles."""
    out = []
    for x in np.asarray(a, dtype=np.float64).ravel().tolist():
        n, d = x.as_integer_ratio()
        out.append(n * (_ONE // d))
    return out


def lincomb(weights, xs, ops):
    """For v_i = sum_j w_j x_j[i] with weights (w_j, bound of w_j's own error) and ``ops`` roundings on the magnitudes of the terms: returns
    (D, S, B) -- v_i = S[i] / (D 2^SCALE) exactly, and |computed - v_i| <= B[i] / (2^_CB 2^SCALE)."""
    D = 1
    for w, _ in weights:
        D = D * w.denominator // math.gcd(D, w.denominator)
    N = [int(w * D) for w, _ in weights]
    C = [math.ceil((ew + gamma(ops) * abs(w)) * (1 << _CB)) for w, ew in weights]
    X = [ints_of(x) for x in xs]
    n = len(X[0])
    S = [sum(N[j] * X[j][i] for j in range(len(N))) for i in range(n)]
    B = [sum(C[j] * abs(X[j][i]) for j in range(len(N))) for i in range(n)]
    return D, S, B


# ---- the update: norms, the decision table, the saves ------------------------------------------------------------------------------------------
class Outcome:
    """row, the exact next integers, the reals with bounds, the margins of every threshold compared, and the call of prepare that follows."""


def norms(sh, st, vec):
    """dnorm and errn with their bounds (module docstring).  Returns a dict; ``bad`` when a component of the Newton step is not finite.
    The differences (u - d, e) are exact rationals; the weights are reciprocals with unrelated denominators, so the terms of the sums are
    carried at 60 digits (mpmath), as the roots are."""
    import mpmath as mp
    n = len(vec["u"])
    dsc = st["dsc"]
    r = {"bad": False}
    r["fin"] = fin = [math.isfinite(float(x) * float(dsc)) for x in vec["delta"]]
    if not all(fin):
        r["bad"] = True
        return r
    fdsc = fr(dsc)
    d = [fr(x) * fdsc for x in vec["delta"]]
    tested = st["nhist"] >= 2 and sh["n_err"] > 0
    r["tested"] = tested
    with mp.workdps(60):
        rt = mp.mpf(float(sh["reltol"]))
        g2, g3, g4 = _mp(gamma(2)), _mp(gamma(3)), _mp(gamma(4))
        s1 = s2 = sb = mp.mpf(0)
        for i in range(n):
            at, x0 = mp.mpf(float(sh["atol"][i])), abs(mp.mpf(float(vec["u0"][i])))
            di = _mp(d[i])
            s1 += (di / (at + rt * x0)) ** 2
            if not tested or sh["emask"][i] == 0:
                continue
            u, up = fr(vec["u"][i]), fr(vec["up"][i])
            un = u - d[i]
            den = at + rt * max(x0, abs(_mp(un)))
            w2 = mp.mpf(float(sh["emask"][i])) / den
            a = _mp(un - up) * w2
            s2 += a * a
            # e = (u - d) - up: d (1), two subtractions: 3 on |u| + |d| + |up|.  w2: u_new moves the denominator by at most reltol times its own
            # error (2 on |u| + |d|), then product, sum, division, and the product e w2: 4.
            mag = abs(_mp(u)) + abs(di)
            de = g3 * (mag + abs(_mp(up)))
            th = rt * g2 * mag / den + g4
            sb += (abs(a) * th + de * w2 * (1 + th)) ** 2
        r["dnorm"] = _to_frac(mp.sqrt(s1 / n)) if s1 != 0 else F(0)
        if tested:
            ne = sh["n_err"]
            q2 = _to_frac(mp.sqrt(s2 / ne)) if s2 != 0 else F(0)
            qb = _to_frac(mp.sqrt(sb / ne)) if sb != 0 else F(0)
    # dnorm: d (1); reltol |x0| (1), + atol (1), 1 / . (1): w 3; d w: 5; its square: 11; the sum of n positive terms: n - 1; / n: 1;
    # the square root halves what stands under it and adds its own: (11 + n) / 2 + 1
    r["dnorm_rel"] = gamma(math.ceil((11 + n) / 2) + 1)
    if tested:
        errc, errc_rel = error_constant(st["ord"], st["h"], st["hprev"], st["hpp"], st["hp3"])
        r["errc"], r["errn"] = errc, errc * q2
        # | ||a + da|| - ||a|| | <= ||da||; then the squares (2 on each term, halved by the root), the sum of up to n terms, / n_err, the root,
        # the product with errc: (n + 1) / 2 + 3, and errc's own bound
        r["errn_bound"] = errc * qb * (1 + F(1, 10 ** 12)) + r["errn"] * (gamma(math.ceil((n + 1) / 2) + 3) + errc_rel)
    return r


def _rel(v, thr):
    return abs(float(v) / float(thr) - 1.0) if thr != 0 else math.inf


def step_factor(rule, ord_, errn, errn_rel, accepted, margins):
    """(kind, value, relative bound) of the factor of the next step after a tested step: kind "const" (the factor is one of the rule's
    constants: the step is ONE rounded product of doubles) or "real"."""
    R = RULE
    lo, hi = (R["acc_lo"], R["acc_hi"]) if accepted else (R["rej_lo"], R["rej_hi"])
    if rule == 0:
        # classical controller: 0.9 errn^(-1 / (ord + 1)), clamped to [0.2, 2] after an accepted step and to [0.1, 0.9] after a rejected one;
        # an estimate of exactly zero doubles the step
        if errn == 0:
            return "const", R["acc_hi"], F(0)
        fac = fr(R["safety"]) / root(errn, ord_ + 1)
        margins += [("fac_lo", fac, lo), ("fac_hi", fac, hi)]
        if fac <= fr(lo):
            return "const", lo, F(0)
        if fac >= fr(hi):
            return "const", hi, F(0)
        # root and reciprocal (ord 1: sqrt, division: 2; ord 3: 3), the product with 0.9: ord + 2 at most; the estimate's own error enters
        # divided by ord + 1.  Order 2 goes through step_root: ROOT2_REL in all
        return "real", fac, (ROOT2_REL if ord_ == 2 else errn_rel / (ord_ + 1) + gamma(ord_ + 2))
    # IDA: eta = 1 / ((2 errn)^(1 / (ord + 1)) + 1e-4).  Accepted: eta >= 2 doubles the step, eta in (1, 2) keeps it, eta <= 1 shrinks it by
    # eta held to [0.5, 0.9].  Rejected: 0.9 eta held to [0.25, 0.9].
    if errn == 0:
        return "const", R["eta_grow"], F(0)
    rt = root(2 * errn, ord_ + 1)
    eta = 1 / (rt + fr(R["eta_eps"]))
    # the root through its reciprocal and back (ord 1: 3 roundings, ord 3: 4), the sum, the division: ord + 4 at most, all terms positive; at
    # order 2 the root carries step_root's allowance instead, which the sum with 1e-4 only dilutes: ROOT2_REL in all (step_budget)
    eta_rel = ROOT2_REL if ord_ == 2 else errn_rel / (ord_ + 1) + gamma(ord_ + 4)
    if accepted:
        margins += [("eta_grow", eta, R["eta_grow"]), ("eta_keep", eta, R["eta_keep"])]
        if eta >= fr(R["eta_grow"]):
            return "const", R["eta_grow"], F(0)
        if eta > fr(R["eta_keep"]):
            return "const", 1.0, F(0)
        margins += [("eta_lo", eta, R["eta_lo"]), ("eta_hi", eta, R["eta_hi"])]
        if eta >= fr(R["eta_hi"]):
            return "const", R["eta_hi"], F(0)
        if eta <= fr(R["eta_lo"]):
            return "const", R["eta_lo"], F(0)
        return "real", eta, eta_rel
    fac = fr(R["safety"]) * eta
    margins += [("eta_rej_lo", fac, R["eta_rej_lo"]), ("eta_rej_hi", fac, R["eta_rej_hi"])]
    if fac >= fr(R["eta_rej_hi"]):
        return "const", R["eta_rej_hi"], F(0)
    if fac <= fr(R["eta_rej_lo"]):
        return "const", R["eta_rej_lo"], F(0)
    return "real", fac, eta_rel


def step_budget(ord_, errn_rel):
    """What a step through step_root at order 2 spends of ROOT2_REL besides step_root's own 9.33e-8: the estimate's error divided by 3 and up
    to eight roundings (reciprocal and back, the sum, the division, the products with 0.9 and h).  Must stay below ROOT2_REL - ROOT2_OWN
    (tests/test_tran_ctrl_ref_cpu.py asserts it for every such case)."""
    return errn_rel / (ord_ + 1) + gamma(8)


def _times(h, kind, fac, rel):
    """The step h * factor: ("bits", double) for a constant factor, ("real", value, relative bound incl. the product) else."""
    if kind == "const":
        return ("bits", float(f64(h) * f64(fac)))
    return ("real", fr(h) * fac, rel if rel == ROOT2_REL else rel + gamma(1))


def _margin(o, name, hn, thr):
    """A step that is a double (a constant factor, a clip) is compared exactly; one that carries a bound needs its distance."""
    if hn[0] == "real":
        o.margins.append((name, hn[1], thr))


def update(sh, st, vec, bad_in):
    """The decision table (``_update``); with Newton mode 0 the Newton-mode-1 words of the state are neither read nor written."""
    o = _update(sh, st, vec, bad_in)
    if sh["newton_mode"] == 0:
        o.ints["mflags"] = st["mflags"]
    return o


def _update(sh, st, vec, bad_in):
    """The decision table.  st: the state before the call (dict: t h hprev hpp hp3 tn a0 nhist ord k status bp si a0f ss dnp dsc mflags).
    Returns an Outcome:
      row, ints (the next nhist ord k status bp si, counter increments, mflags), reals (name -> ("bits", double) | ("real", value, abs bound)
      | ("same",)), margins [(name, value, threshold)], saves [save indices], next (the arguments of the prepare that follows, or None),
      hist_shift (True when the history moved), pcnr (True when the limit rows are copied)."""
    R = RULE
    o = Outcome()
    o.margins, o.saves, o.next, o.hist_shift, o.pcnr = [], [], None, False, False
    mode, rule = sh["newton_mode"], sh["step_rule"]
    h = st["h"]
    ints = {k: st[k] for k in ("nhist", "ord", "k", "status", "bp", "si")}
    ints.update(c_newton=0, c_accept=0, c_reject=0, c_fail=0, mflags=st["mflags"])
    reals = {k: ("same",) for k in ("t", "h", "hprev", "hpp", "hp3", "tn", "a0", "a0f", "ss", "dnp")}
    o.ints, o.reals = ints, reals
    if st["status"] != 0:
        o.row = "status_nonzero"
        return o
    nm = norms(sh, st, vec)
    o.norms = nm
    bad = bool(bad_in) or nm["bad"]
    ints["c_newton"] = 1
    # ---- did the iteration converge, did it fail?
    conv = diverge = False
    if mode == 0:
        if not bad:
            o.margins.append(("newton_tol", nm["dnorm"], sh["newton_tol"]))
            conv = nm["dnorm"] < fr(sh["newton_tol"])
    elif not bad:
        dn, ss = nm["dnorm"], fr(st["ss"])
        ss_bound = F(0)
        if st["k"] == 0:
            o.margins.append(("nl_first", dn, R["nl_first"]))
            conv = dn <= fr(R["nl_first"])
        else:
            # the rate between successive updates; above 0.9 the iteration diverges, else ss = rate / (1 - rate)
            rate = dn / fr(st["dnp"]) if st["dnp"] > 0.0 else F(0)
            o.margins.append(("nl_rate", rate, R["nl_rate"]))
            if rate > fr(R["nl_rate"]):
                diverge = True
            else:
                ss = rate / (1 - rate)
                # rate: dnorm's bound + 1; 1 - rate: that on 1 + rate, + 1; the quotient + 1
                rr = nm["dnorm_rel"] + gamma(1)
                ss_bound = ss * (rr + (rr + gamma(1)) * (1 + rate) / (1 - rate) + gamma(1))
                reals["ss"] = ("real", ss, ss_bound)
        if not diverge:
            o.margins.append(("nl_tol", ss * dn, R["nl_tol"]))
            if ss * dn <= fr(R["nl_tol"]):
                conv = True
        reals["dnp"] = ("real", dn, dn * nm["dnorm_rel"])
    failed = (not conv) and (bad or diverge or st["k"] + 1 >= sh["max_newton"])
    shift = 1 << MN_SINCE_SHIFT
    if not conv:
        if failed and mode == 1 and not (st["mflags"] & MN_JCUR):
            # failed on a Jacobian that was not refreshed in this attempt: the same step again, refactored first
            o.row = "retry_stale"
            ints["mflags"] = (st["mflags"] | MN_NEED) & ~MN_JCUR
            o.next = dict(t=st["t"], h=("bits", h), nhist=st["nhist"], hprev=st["hprev"], hpp=st["hpp"], hp3=st["hp3"], bp=st["bp"])
        elif failed:
            hn = float(f64(R["fail_frac"]) * f64(h))
            ints["c_fail"] = 1
            if hn < sh["hmin"]:
                o.row = "fail_hmin"
                ints["status"] = -2
            else:
                o.row = "fail_shrink"
                ints["mflags"] = st["mflags"] & ~MN_JCUR
                o.next = dict(t=st["t"], h=("bits", hn), nhist=st["nhist"], hprev=st["hprev"], hpp=st["hpp"], hp3=st["hp3"], bp=st["bp"])
        else:
            o.row = "continue"
            ints["k"] = st["k"] + 1
            o.pcnr = bool(sh["use_pcnr"]) and sh["n_limits"] > 0
        return o
    # ---- converged: the error test
    tested = nm["tested"]
    accept = True
    if tested:
        o.margins.append(("errn", nm["errn"], R["errn_max"]))
        accept = nm["errn"] < fr(R["errn_max"]) if R["accept_strict"] else nm["errn"] <= fr(R["errn_max"])
    errn_rel = nm["errn_bound"] / nm["errn"] if tested and nm["errn"] > 0 else F(0)
    if not accept:
        ints["c_reject"] = 1
        hn = _times(h, *step_factor(rule, st["ord"], nm["errn"], errn_rel, False, o.margins))
        _margin(o, "hmin", hn, sh["hmin"])
        if fr(hn[1]) < fr(sh["hmin"]):
            o.row = "reject_hmin"
            ints["status"] = -1
        else:
            o.row = "reject"
            ints["mflags"] = st["mflags"] & ~MN_JCUR
            o.next = dict(t=st["t"], h=hn, nhist=st["nhist"], hprev=st["hprev"], hpp=st["hpp"], hp3=st["hp3"], bp=st["bp"])
        return o
    # ---- accepted
    tn = st["tn"]
    o.saves = saves_due(sh, st["si"], tn)
    ints["si"] = st["si"] + len(o.saves)
    o.hist_shift = True
    cap = 4 if sh["max_order"] >= 3 else 3
    nh = min(st["nhist"] + 1, cap)
    hn = _times(h, *step_factor(rule, st["ord"], nm["errn"], errn_rel, True, o.margins)) if tested else ("bits", float(f64(R["untested"]) * f64(h)))
    tstop, tb = stop_of(sh, st["bp"])
    bp = st["bp"]
    if tn == tb:
        # landed on a breakpoint: the history restarts, the next step is a tenth of this one or of the way to the next stop
        bp += 1
        if R["land_nhist"] is not None:
            nh = R["land_nhist"]
        tstop2, _ = stop_of(sh, bp)
        hn = ("bits", float(f64(R["land_frac"]) * min(f64(h), f64(tstop2) - f64(tn))))
    _margin(o, "hmax", hn, sh["hmax"])
    if fr(hn[1]) > fr(sh["hmax"]):
        hn = ("bits", float(sh["hmax"]))
    ints.update(nhist=nh, bp=bp, c_accept=1, mflags=st["mflags"] + shift)
    reals.update(t=("bits", tn), hprev=("bits", h), hpp=("bits", st["hprev"]))
    if sh["max_order"] >= 3:
        reals["hp3"] = ("bits", st["hpp"])
    if tn >= sh["t1"]:
        o.row = "accept_end"
        ints["status"] = 1
        return o
    o.row = "accept"
    _margin(o, "hmin", hn, sh["hmin"])
    if fr(hn[1]) < fr(sh["hmin"]):
        hn = ("bits", float(sh["hmin"]))
    ints["mflags"] = (st["mflags"] + shift) & ~MN_JCUR
    o.next = dict(t=tn, h=hn, nhist=nh, hprev=h, hpp=st["hprev"], hp3=st["hpp"] if sh["max_order"] >= 3 else st["hp3"], bp=bp)
    return o


def interpolant_weights(sh, st, si):
    """(weights with their bounds over (u_new, u0[, u1]), roundings) of the save time ``si`` reached by the step st."""
    t, tn, hprev = fr(st["t"]), fr(st["tn"]), fr(st["hprev"])
    ts = fr(sh["save_t"][si])
    if st["nhist"] >= 2:
        # the weights' errors (ts - t and tn - t are one rounding each: inside POS_OPS), three products and two sums: 3
        return value_weights([tn - t, F(0), -hprev], ts - t), 3
    # u0 + sc (u_new - u0), sc = (ts - t) / (tn - t): two differences and a division (3); u_new - u0 (1), the product (1), the sum (1): 6 on
    # |u0| + |sc| (|u_new| + |u0|) -- as weights: sc on u_new, 1 - sc on u0, with 6 roundings on |sc| |u_new| + (1 + |sc|) |u0|
    sc = (ts - t) / (tn - t)
    return [(sc, F(0)), (1 - sc, gamma(6) * (1 + abs(sc) - abs(1 - sc)))], 6


def margin_of(o):
    """The smallest relative distance of an outcome's compared values from their thresholds."""
    return min([_rel(v, thr) for _, v, thr in o.margins] + [math.inf])


# ---- comparing one instance's outputs with the reference -----------------------------------------------------------------------------------
STATE_D = ("t", "h", "hprev", "hpp", "hp3", "tn", "a0", "a0f", "ss", "dnp")
GOT_D = {"t": "t", "h": "h", "hprev": "hprev", "hpp": "hpp", "hp3": "hp3", "tn": "tcur", "a0": "gamma", "a0f": "mn_a0f", "ss": "mn_ss", "dnp": "mn_dnp"}
VECS = ("u", "du", "delta", "limit_w", "u0", "u1", "u2", "u3", "up", "beta")
_ALL_ONES = np.uint64(0xFFFFFFFFFFFFFFFF)


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


class Checker:
    """Collects, per quantity, the worst |got - ref| / bound (exact comparisons count as 0) and fails with the case's name."""

    def __init__(self, name):
        self.name, self.worst, self.n_checked = name, {}, 0

    def fail(self, what, msg):
        raise AssertionError("case %s: %s: %s" % (self.name, what, msg))

    def exact(self, what, got, want):
        self.n_checked += 1
        if isinstance(want, (float, np.floating)) or isinstance(want, np.ndarray) and want.dtype == np.float64:
            ok = np.array_equal(_bits(got), _bits(want))
        else:
            ok = np.array_equal(np.asarray(got), np.asarray(want))
        if not ok:
            self.fail(what, "got %r, want %r (exact)" % (got, want))
        self.worst.setdefault(what, 0.0)

    def close(self, what, got, ref, bound, group=None):
        self.n_checked += 1
        got = float(got)
        if not math.isfinite(got):
            self.fail(what, "got %r, want %r" % (got, float(ref)))
        err = abs(F(got) - ref)
        if err > bound:
            self.fail(what, "got %r, want %r: error %.3g is %.3g of the bound %.3g" % (got, float(ref), float(err), float(err / bound) if bound else math.inf, float(bound)))
        r = float(err / bound) if bound else 0.0
        g = group or what
        self.worst[g] = max(self.worst.get(g, 0.0), r)
        return r

    def lin(self, what, got, weights, xs, ops, skip=None):
        """got[i] against sum_j w_j xs[j][i] within the bound of lincomb, every element (but those in ``skip``)."""
        got = np.asarray(got, dtype=np.float64)
        fin = np.isfinite(got)
        if skip is not None:
            fin = fin | skip
        if not fin.all():
            self.fail(what, "not finite at %r" % np.flatnonzero(~fin)[:4].tolist())
        if skip is not None:
            got = np.where(skip, 0.0, got)
            xs = [np.where(skip, 0.0, np.asarray(x, dtype=np.float64)) for x in xs]
        D, S, B = lincomb(weights, xs, ops)
        G = ints_of(got)
        worst = 0.0
        for i in range(len(G)):
            err, bnd = abs(G[i] * D - S[i]) << _CB, B[i] * D
            if err > bnd:
                self.fail("%s[%d]" % (what, i), "got %r, want %r: the error is %.3g of the bound" % (
                    float(got[i]), float(F(S[i], D * _ONE)), float(F(err, bnd)) if bnd else math.inf))
            if bnd:
                worst = max(worst, ((err << 40) // bnd) / 2.0 ** 40)
        self.n_checked += len(G)
        self.worst[what] = max(self.worst.get(what, 0.0), worst)


def _branch_of_real(sh, t, hn, bp):
    """The clipping branch of a step known with a bound: the same at both ends of the bound, or the case is not robust (None)."""
    v, rel = hn[1], hn[2]
    lo, hi = float(v * (1 - rel)), float(v * (1 + rel))
    a, b = clip(sh, t, lo, bp), clip(sh, t, hi, bp)
    return a if a[2] == b[2] and (a[2] == "free" or a[:2] == b[:2]) else None


def check_prepared(ck, sh, g, nx):
    """The outputs of a prepare_step call with the arguments ``nx`` (t, h as ("bits", x) or ("real", v, rel), nhist, hprev, hpp, hp3, bp), on
    the history the device holds afterwards (``g``: its outputs).  Staged: a0, the predictor and beta are functions of the step the device
    took (g["h"], itself held to the reference first); du of the device's own a0, u and beta."""
    hn = nx["h"]
    if hn[0] == "bits":
        h_used = hn[1]
    else:
        br = _branch_of_real(sh, nx["t"], hn, nx["bp"])
        if br is None:
            ck.fail("h", "the step %r +- %.3g straddles a clipping threshold: not a robust case" % (float(hn[1]), float(hn[1] * hn[2])))
        if br[2] == "free":
            ord2 = hn[2] == ROOT2_REL
            r = ck.close("h_next", g["h"], hn[1], hn[1] * hn[2], group="h_next.ord2" if ord2 else "h_next")
            if ord2:
                ck.worst["h_next.ord2.rel"] = max(ck.worst.get("h_next.ord2.rel", 0.0), r * float(hn[2]))
            h_used = float(g["h"])
        else:
            h_used = float(hn[1])
    pr = prepare(sh, nx["t"], h_used, nx["nhist"], nx["hprev"], nx["hpp"], nx["hp3"], nx["bp"])
    ck.exact("h", float(g["h"]), float(pr.h))
    ck.exact("tn", float(g["tcur"]), float(pr.tn))
    ck.exact("order", int(g["order"]), pr.ord)
    ck.exact("k", int(g["k"]), 0)
    ck.close("a0", g["gamma"], pr.a0, pr.a0_bound)
    hist = (g["u0"], g["u1"], g["u2"], g["u3"])
    ck.lin("up", g["up"], pr.pred_w, hist[:pr.npts], pr.pred_ops)
    ck.exact("u", g["u"], g["up"])                       # the iterate starts on the predictor: the same double
    ck.lin("beta", g["beta"], pr.alpha, hist[:pr.ord], pr.beta_ops)
    # du = a0 u + beta of the device's own a0, u, beta: a product and a sum (2) on |a0 u| + |beta|
    ck.lin("du", g["du"], [(fr(g["gamma"]), F(0)), (F(1), F(0))], (g["u"], g["beta"]), 2)
    return pr


def _unchanged(ck, g, vin, names):
    for nme in names:
        ck.exact(nme, g[nme], np.asarray(vin[nme], dtype=np.float64))


def _check_common(ck, sh, case, g, o_ints, status_nonzero=False, op=1):
    st = case.st
    for nme in ("dsc", "p_t", "p_h", "p_hprev", "p_hpp"):
        ck.exact(nme, float(g[nme]), float(case.extra[nme]))
    ck.exact("p_nhist", int(g["p_nhist"]), int(case.extra["p_nhist"]))
    for nme, key in (("nhist", "nhist"), ("status", "status"), ("bp_idx", "bp"), ("save_idx", "si")):
        ck.exact(nme, int(g[nme]), int(o_ints[key]))
    ck.exact("mn_flags", int(g["mn_flags"]), int(o_ints["mflags"]))
    inc = [o_ints["c_newton"], o_ints["c_accept"], o_ints["c_reject"], o_ints["c_fail"]]
    ck.exact("cnt", [int(x) for x in g["cnt"]], [int(c) + i for c, i in zip(case.cnt, inc)])
    if status_nonzero:
        ck.exact("active", int(g["active"]), -1)
        ck.exact("flags", int(g["flags"]), int(case.flags))
    else:
        ck.exact("active", int(g["active"]), 1 if o_ints["status"] == 0 else 0)
        ck.exact("flags", int(g["flags"]), int(case.flags) if op == 0 else 0)
    _unchanged(ck, g, case.vec, ("delta", "limit_w"))
    if sh["max_order"] < 3:
        ck.exact("hp3", float(g["hp3"]), float(st["hp3"]))


def _out_untouched(ck, rows):
    if rows.size and not (_bits(rows) == _ALL_ONES).all():
        ck.fail("out", "a row that was not due was written")
    ck.n_checked += 1


def check_prepare_case(sh, case, g):
    """op 0: prepare_step(t, h, nhist, hprev, hpp) on the loaded state.  Returns the Checker."""
    ck = Checker(case.name)
    st, ex = case.st, case.extra
    ints = dict(nhist=st["nhist"], status=st["status"], bp=st["bp"], si=st["si"], c_newton=0, c_accept=0, c_reject=0, c_fail=0,
                mflags=(st["mflags"] & ~MN_JCUR) if sh["newton_mode"] else st["mflags"])
    _out_untouched(ck, g["out"])
    if st["status"] != 0:
        ints["mflags"] = st["mflags"]
        _check_common(ck, sh, case, g, ints, status_nonzero=True, op=0)
        _unchanged(ck, g, case.vec, VECS)
        for nme in STATE_D:
            if nme != "hp3":
                ck.exact(nme, float(g[GOT_D[nme]]), float(st[nme]))
        return ck
    _check_common(ck, sh, case, g, ints, op=0)
    _unchanged(ck, g, case.vec, ("u0", "u1", "u2", "u3"))
    for nme in ("t", "hprev", "hpp", "a0f", "ss", "dnp"):
        ck.exact(nme, float(g[GOT_D[nme]]), float(st[nme]))
    if sh["max_order"] >= 3:
        ck.exact("hp3", float(g["hp3"]), float(st["hp3"]))
    nx = dict(t=ex["p_t"], h=("bits", float(ex["p_h"])), nhist=ex["p_nhist"], hprev=ex["p_hprev"], hpp=ex["p_hpp"], hp3=st["hp3"], bp=st["bp"])
    ck.prepared = check_prepared(ck, sh, g, nx)
    return ck


def check_update_case(sh, case, g, o=None, fixed=False):
    """op 1: tran_update_body on the given state (``o``: the reference's Outcome if the caller has it).  Returns the Checker."""
    ck = Checker(case.name)
    st, vec = case.st, case.vec
    if o is None:
        o = update(sh, st, vec, case.flags & 1)
    ck.outcome = o
    n = len(vec["u"])
    if case.row is not None and o.row != case.row:
        ck.fail("row", "the reference takes row %s, the case was built for %s" % (o.row, case.row))
    _check_common(ck, sh, case, g, o.ints, status_nonzero=o.row == "status_nonzero")
    for nme in STATE_D:
        kind = o.reals[nme]
        if nme in ("h", "tn", "a0") and o.next is not None:
            continue
        if nme == "hp3" and sh["max_order"] < 3:
            continue
        if kind[0] == "same":
            ck.exact(nme, float(g[GOT_D[nme]]), float(st[nme]))
        elif kind[0] == "bits":
            ck.exact(nme, float(g[GOT_D[nme]]), float(kind[1]))
        else:
            ck.close(nme, g[GOT_D[nme]], kind[1], kind[2])
    if o.row == "status_nonzero":
        _unchanged(ck, g, vec, VECS)
        ck.exact("order", int(g["order"]), st["ord"])
        ck.exact("k", int(g["k"]), st["k"])
        _out_untouched(ck, g["out"])
        return ck
    notfin = ~np.array(o.norms["fin"])

    def check_un(name, got, upto=n):
        # u_new = u - delta dsc: the product and the difference (2) on |u| + |delta dsc|; not finite where the Newton step is not
        got = np.asarray(got, dtype=np.float64)
        if np.isfinite(got[notfin]).any():
            ck.fail(name, "finite where the Newton step is not")
        ck.lin("u_new", got[:upto], [(F(1), F(0)), (-fr(st["dsc"]), F(0))], (vec["u"][:upto], vec["delta"][:upto]), 2, skip=notfin[:upto] if notfin.any() else None)

    # ---- the history and the saves
    if o.hist_shift:
        check_un("u0", g["u0"])
        ck.exact("u1", g["u1"], np.asarray(vec["u0"], dtype=np.float64))
        ck.exact("u2", g["u2"], np.asarray(vec["u1"], dtype=np.float64))
        if sh["max_order"] >= 3:
            ck.exact("u3", g["u3"], np.asarray(vec["u2"], dtype=np.float64))
        else:
            _unchanged(ck, g, vec, ("u3",))
        # the saves, on the u_new the device wrote into the history
        obs = np.asarray(sh["obs"], dtype=np.int64)
        pts = (np.asarray(g["u0"])[obs], np.asarray(vec["u0"])[obs], np.asarray(vec["u1"])[obs])
        for si in o.saves:
            w, ops = interpolant_weights(sh, st, si)
            ck.lin("out", g["out"][si], w, pts[:len(w)], ops)
        other = [s for s in range(len(sh["save_t"])) if s not in o.saves]
        _out_untouched(ck, g["out"][other])
    else:
        _unchanged(ck, g, vec, ("u0", "u1", "u2", "u3"))
        _out_untouched(ck, g["out"])
    # ---- the step that follows, or what stays
    if o.next is not None:
        ck.prepared = check_prepared(ck, sh, g, o.next)
        return ck
    ck.exact("order", int(g["order"]), st["ord"])
    ck.exact("k", int(g["k"]), o.ints["k"])
    _unchanged(ck, g, vec, ("up", "beta"))
    if o.row == "accept_end":
        ck.exact("u", g["u"], g["u0"])                   # no step follows: u stays u_new, the double the history received
        _unchanged(ck, g, vec, ("du",))
    elif o.row in ("fail_hmin", "reject_hmin"):
        check_un("u", g["u"])
        _unchanged(ck, g, vec, ("du",))
    else:   # continue
        nl = sh["n_limits"] if o.pcnr else 0
        if n - nl > 0:
            check_un("u", g["u"], n - nl)
        if nl:
            ck.exact("u(pcnr)", g["u"][n - nl:], np.asarray(vec["limit_w"], dtype=np.float64)[n - nl:])
        if fixed:
            _unchanged(ck, g, vec, ("du",))              # the fixed form leaves du to its caller
        else:
            # du = a0 u + beta on the device's own u: a product and a sum (2)
            ck.lin("du", g["du"], [(fr(st["a0"]), F(0)), (F(1), F(0))], (g["u"], vec["beta"]), 2)
    return ck


# ---- what a correctly rounding device would return (tests/test_tran_ctrl_ref_cpu.py: the comparison code and the cases, without a GPU) -------
def _round_lin(weights, xs):
    """[fl(sum_j w_j x_j[i])]: the exact value rounded once."""
    n = len(xs[0])
    return np.array([float(sum(w * fr(x[i]) for (w, _), x in zip(weights, xs))) for i in range(n)], dtype=np.float64)


def _emulate_prepare(sh, g, nx, h):
    pr = prepare(sh, nx["t"], h, nx["nhist"], nx["hprev"], nx["hpp"], nx["hp3"], nx["bp"])
    hist = (g["u0"], g["u1"], g["u2"], g["u3"])
    g.update(h=pr.h, tcur=pr.tn, order=pr.ord, k=0, gamma=float(pr.a0))
    g["up"] = _round_lin(pr.pred_w, hist[:pr.npts])
    g["u"] = g["up"].copy()
    g["beta"] = _round_lin(pr.alpha, hist[:pr.ord])
    g["du"] = _round_lin([(fr(g["gamma"]), 0), (F(1), 0)], (g["u"], g["beta"]))


def emulate(sh, case, op, fixed=False):
    """The outputs of one instance (the layout of prim_probe.run_tran_ctrl, one instance) of a device that follows RULE and rounds every
    quantity once.  With a changed RULE: the outputs of a controller with that change."""
    st, ex, vec = case.st, case.extra, case.vec
    g = {k: np.array(v, dtype=np.float64) for k, v in vec.items()}
    g.update(t=st["t"], h=st["h"], hprev=st["hprev"], hpp=st["hpp"], tcur=st["tn"], gamma=st["a0"], mn_a0f=st["a0f"], mn_ss=st["ss"], mn_dnp=st["dnp"],
             hp3=st["hp3"], nhist=st["nhist"], order=st["ord"], k=st["k"], status=st["status"], bp_idx=st["bp"], save_idx=st["si"], flags=case.flags,
             mn_flags=st["mflags"], active=-1, cnt=list(case.cnt), **ex)
    g["out"] = np.full((len(sh["save_t"]), len(sh["obs"])), np.nan)
    g["out"].view(np.uint64)[...] = _ALL_ONES
    if st["status"] != 0:
        return g
    if op == 0:
        g["active"] = 1
        if sh["newton_mode"]:
            g["mn_flags"] = st["mflags"] & ~MN_JCUR
        _emulate_prepare(sh, g, dict(t=ex["p_t"], nhist=ex["p_nhist"], hprev=ex["p_hprev"], hpp=ex["p_hpp"], hp3=st["hp3"], bp=st["bp"]), ex["p_h"])
        return g
    o = update(sh, st, vec, case.flags & 1)
    i_ = o.ints
    g.update(nhist=i_["nhist"], k=i_["k"], status=i_["status"], bp_idx=i_["bp"], save_idx=i_["si"], mn_flags=i_["mflags"], flags=0,
             active=1 if i_["status"] == 0 else 0)
    g["cnt"] = [c + i_[k] for c, k in zip(case.cnt, ("c_newton", "c_accept", "c_reject", "c_fail"))]
    for nme, kind in o.reals.items():
        if kind[0] != "same":
            g[GOT_D[nme]] = float(kind[1])
    with np.errstate(all="ignore"):
        d = np.asarray(vec["delta"], dtype=np.float64) * st["dsc"]
    un = np.array([float(fr(u) - fr(x) * fr(st["dsc"])) if math.isfinite(dd) else math.nan for u, x, dd in zip(vec["u"], vec["delta"], d)])
    if o.hist_shift:
        obs = np.asarray(sh["obs"], dtype=np.int64)
        for si in o.saves:
            w, _ = interpolant_weights(sh, st, si)
            g["out"][si] = _round_lin(w, (un[obs], g["u0"][obs], g["u1"][obs])[:len(w)])
        if sh["max_order"] >= 3:
            g["u3"] = g["u2"]
        g["u2"], g["u1"], g["u0"] = g["u1"], g["u0"], un.copy()
    if o.next is not None:
        _emulate_prepare(sh, g, o.next, float(o.next["h"][1]))
    else:
        g["u"] = un.copy()
        if o.row == "continue":
            if o.pcnr:
                nl = sh["n_limits"]
                g["u"][len(un) - nl:] = np.asarray(vec["limit_w"])[len(un) - nl:]
            if not fixed:
                g["du"] = _round_lin([(fr(st["a0"]), 0), (F(1), 0)], (g["u"], g["beta"]))
    return g
