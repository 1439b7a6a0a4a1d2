"""TEST INFRASTRUCTURE -- inputs, references and tolerances of the device-side primitives (tests/test_gpu_primitives.py runs them on
the GPU through tests/prim_probe.py, tests/test_prim_ref_cpu.py checks the references themselves).

Sources of truth: numpy / Python ``fractions`` where the operation is exact or correctly rounded, mpmath at 60 digits for the elementary
functions (written once to tests/golden/prim_*.npz by tools/make_prim_fixtures.py -- the GPU tests read only those), and the oracle's own
limiter and wave functions (oracle/devices_ref.py, oracle/va_mos1_ref.py).

Tolerance model (the shape of stamp_ref.slot_scales):   |got - ref| <= K * 2^-52 * scale
  scale  per case: the sum of the magnitudes of the terms of the formula under test, evaluated in the reference's precision;
  K      per function, derived below from the accuracy the device math library is specified to (the OpenCL double-precision table) --
         never measured from the code under test.
Where the formula evaluated in IEEE doubles is not finite, the result must show the same inf / NaN / sign pattern and no tolerance applies.
"""
import math
import os
from fractions import Fraction

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
EPS = 2.0 ** -52
MP_DIGITS = 60

# OpenCL C double-precision ulp bounds (the table the device math library targets; sqrt and division are correctly rounded)
SPEC = {"sqrt": 0, "div": 0, "exp": 3, "log": 3, "log10": 3, "sin": 4, "cos": 4, "sinh": 4, "cosh": 4, "asin": 4, "acos": 4, "hypot": 4,
        "tan": 5, "tanh": 5, "atan": 5, "asinh": 5, "acosh": 5, "atanh": 5, "atan2": 6, "pow": 16}
ARITH = 4     # the arithmetic around the calls: up to eight roundings of half an ulp each (products, sums, fused or not, reciprocals)

# K of every checked quantity: the specification bounds of the library calls in its expression, each with its sensitivity, + ARITH
K = {
    "arith": ARITH,                                   # +, -, *, / and their dual rules: no library call
    "sqrt.f": SPEC["sqrt"] + ARITH, "sqrt.d": SPEC["sqrt"] + ARITH,                 # 0.5 / f: f is correctly rounded
    "exp.f": SPEC["exp"] + ARITH, "exp.d": SPEC["exp"] + ARITH,                     # the derivative is f itself
    "ln.f": SPEC["log"] + ARITH, "ln.d": ARITH,                                     # 1 / x
    "log.f": SPEC["log10"] + ARITH, "log.d": ARITH,                                 # 1 / (x ln 10)
    "tanh.f": SPEC["tanh"] + ARITH, "tanh.d": 2 * SPEC["tanh"] + ARITH,             # 1 - f^2 on scale max(1, f^2): f enters squared
    "sinh.f": SPEC["sinh"] + ARITH, "sinh.d": SPEC["cosh"] + ARITH,
    "cosh.f": SPEC["cosh"] + ARITH, "cosh.d": SPEC["sinh"] + ARITH,
    "sin.f": SPEC["sin"] + ARITH, "sin.d": SPEC["cos"] + ARITH,
    "cos.f": SPEC["cos"] + ARITH, "cos.d": SPEC["sin"] + ARITH,
    "atan.f": SPEC["atan"] + ARITH, "atan.d": ARITH,                                # 1 / (1 + x^2)
    "tan.f": SPEC["tan"] + ARITH, "tan.d": 2 * SPEC["tan"] + ARITH,                 # 1 + f^2 on scale 1 + f^2
    "asin.f": SPEC["asin"] + ARITH, "asin.d": ARITH,                                # 1 / sqrt(1 - x^2) on scale |d| (1 + x^2) / |1 - x^2|
    "acos.f": SPEC["acos"] + ARITH, "acos.d": ARITH,
    "asinh.f": SPEC["asinh"] + ARITH, "asinh.d": ARITH,                             # 1 / sqrt(x^2 + 1): no cancellation
    "acosh.f": SPEC["acosh"] + ARITH, "acosh.d": ARITH,                             # 1 / sqrt(x^2 - 1) on scale |d| (x^2 + 1) / |x^2 - 1|
    "atanh.f": SPEC["atanh"] + ARITH, "atanh.d": ARITH,                             # 1 / (1 - x^2) on scale |d| (1 + x^2) / |1 - x^2|
    "limexp.f": SPEC["exp"] + ARITH, "limexp.d": SPEC["exp"] + ARITH,               # exp below 80; e^80 (1 + x - 80) on scale e^80 (81 + |x|) above
    "pow.f": SPEC["pow"] + ARITH,                                                   # general exponents; the shortcuts are held to 2 ulp
    "pow.da": SPEC["pow"] + ARITH,                                                  # b f / a
    "pow.db": SPEC["pow"] + SPEC["log"] + ARITH,                                    # f log(a)
    "atan2.f": SPEC["atan2"] + ARITH, "atan2.d": ARITH,                             # (y' x - x' y) / (x^2 + y^2)
    "hypot.f": SPEC["hypot"] + ARITH, "hypot.d": ARITH,                             # (a a' + b b') / h through sqrt(a a + b b)
    "pnjlim": SPEC["log"] + 1 + ARITH,   # vold + vt (2 + log(arg)): both sides hand log the same double; + 1 ulp for the oracle's own libm
    "sine": SPEC["exp"] + SPEC["sin"] + 2 + ARITH,   # vo + va exp() sind(): + 2 for the two libm calls of the Python reference
}
# bsrc_value: K of a program = the bounds of its library calls + ARITH, on the sum of the magnitudes of every value it produces
BOP_SPEC = {14: SPEC["pow"], 21: SPEC["exp"], 22: SPEC["log"], 23: SPEC["sqrt"], 25: SPEC["tanh"], 26: SPEC["sin"], 27: SPEC["cos"]}


def gamma(k):
    """Higham's gamma_k = k u / (1 - k u) of a sum of k + 1 terms in any order, u = 2^-53."""
    u = 2.0 ** -53
    return k * u / (1.0 - k * u)


def ulp_diff(got, ref):
    """|got - ref| in units of the spacing of doubles at ref."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return np.abs(got - ref) / np.spacing(np.abs(ref))


def same_pattern(got, ref):
    """inf / NaN / sign pattern of non-finite references: NaN where NaN, the same infinity where infinite."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return np.where(np.isnan(ref), np.isnan(got), got == ref)


def check_close(got, ref, scale, k, what=""):
    """The tolerance model; returns the worst |got - ref| / (2^-52 scale) over the finite references (for the printout)."""
    got, ref, scale = np.broadcast_arrays(np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64), np.asarray(scale, dtype=np.float64))
    fin = np.isfinite(ref)
    bad = ~same_pattern(got[~fin], ref[~fin])
    assert not bad.any(), "%s: non-finite pattern differs: got %r, want %r" % (what, got[~fin][bad][:4], ref[~fin][bad][:4])
    assert np.isfinite(got[fin]).all(), "%s: non-finite where the reference is finite: ref %r" % (what, ref[fin][~np.isfinite(got[fin])][:4])
    err = np.abs(got[fin] - ref[fin])
    tol = k * EPS * scale[fin]
    worst = float(np.max(np.where(tol > 0, err / np.where(tol > 0, tol, 1.0), np.where(err > 0, np.inf, 0.0)), initial=0.0)) * k
    j = np.argmax(err - tol) if err.size else 0
    assert (err <= tol).all(), "%s: %d of %d outside K = %g (worst %.3g x 2^-52 scale; got %r ref %r scale %r)" % (
        what, int((err > tol).sum()), err.size, k, worst, got[fin][j], ref[fin][j], scale[fin][j])
    return worst


# ------------------------------------------------------------------------------------------------------------------------------------------
# fast_div
# ------------------------------------------------------------------------------------------------------------------------------------------
def _in_contract(a, b):
    with np.errstate(all="ignore"):
        q = np.abs(a / b)
    tiny = np.finfo(np.float64).tiny
    return np.isfinite(a) & np.isfinite(b) & (np.abs(b) >= tiny) & ((a == 0) | ((q >= tiny) & np.isfinite(q))) & ((a == 0) | (np.abs(a) >= tiny))


def fast_div_exact_range(a, b):
    """Where fast_div is the correctly rounded quotient (tran_ctrl.hpp), inside the contract above: |b| <= 2^1022, so that 1 / b is a
    normal number (a subnormal reciprocal has lost bits no Newton step brings back), and |a| >= 2^-969, so that the residual a - b q -- a
    multiple of 2^(e_a - 105) -- is one too.  Outside it the quotient may be one ulp off."""
    return (np.abs(b) <= 2.0 ** 1022) & (np.abs(a) >= 2.0 ** -969)


def fast_div_random(n=1 << 16, seed=11):
    """Random pairs at exponent spreads +-{0, 3, 40, 300, 500} (tools/ubench/divcheck.hip), filtered to the contract."""
    rng = np.random.default_rng(seed)
    spread = np.array([0, 3, 40, 300, 500])[rng.integers(0, 5, n)]
    def draw():
        m = (1.0 + rng.random(n)) * np.where(rng.random(n) < 0.5, -1.0, 1.0)
        e = np.floor((2.0 * rng.random(n) - 1.0) * (spread + 0.999)).astype(np.int64)
        return np.ldexp(m, e)
    a, b = draw(), draw()
    ok = _in_contract(a, b)
    return a[ok], b[ok]


def fast_div_structured():
    up, dn = lambda x: np.nextafter(x, np.inf), lambda x: np.nextafter(x, -np.inf)
    bs = [3.0, 1.0 / 3.0, 10.0, 1e-12, 1e12]
    bs = bs + [up(x) for x in bs] + [dn(x) for x in bs]
    bs += [2.0 ** k for k in (-1022, -1021, -600, -1, 0, 1, 52, 600, 1022, 1023)]                 # powers of two
    bs += [dn(2.0 ** 1023), up(2.0 ** 1023), np.finfo(np.float64).max, up(2.0 ** -1022), 1.5 * 2.0 ** -1022]   # reciprocal subnormal / huge
    bs = np.array(bs + [-x for x in bs])
    rng = np.random.default_rng(12)
    a, b = [], []
    with np.errstate(over="ignore"):                                                # (pairs beyond the range are filtered out below)
        for x in bs:
            m = float(np.ldexp(1.0 + rng.random(), int(np.floor(np.log2(abs(x))))))    # a random number of b's magnitude
            for y in (x, -x, x * (1 + EPS), x * (1 - EPS), 0.0, -0.0, m, 3.0 * m, m / 3.0, 1.0, -1.0):
                a.append(y); b.append(x)
    a, b = np.array(a), np.array(b)
    ok = _in_contract(a, b)
    return a[ok], b[ok]


def fast_div_hard(n=100000, seed=13):
    """Pairs whose quotient lies within ~2^-106 relative of a rounding midpoint: an odd M in [2^53, 2^54) (M / 2^54 is the midpoint of two
    neighbouring doubles), an integer B in [2^52, 2^53) and A = round(M B / 2^54), kept when in [2^52, 2^53).  For A / B to come that close
    M B must miss a multiple of 2^54 by a small r only, so B is not drawn but solved for: B = r M^-1 mod 2^54, 1 <= |r| <= 8 -- then
    A / B = M / 2^54 - r / (2^54 B).  Both scaled by random powers of two.  The pairs a Newton-reciprocal division misses, if it misses any."""
    rng = np.random.default_rng(seed)
    a, b = [], []
    while len(a) < n:
        Ms = rng.integers(1 << 52, 1 << 53, 8192) * 2 + 1
        rs = rng.integers(1, 9, 8192) * np.where(rng.random(8192) < 0.5, -1, 1)
        for M, r in zip(Ms.tolist(), rs.tolist()):
            B = (r * pow(M, -1, 1 << 54)) % (1 << 54)
            A = (M * B + (1 << 53)) >> 54
            if (1 << 52) <= B < (1 << 53) and (1 << 52) <= A < (1 << 53):
                a.append(A); b.append(B)
    a, b = np.array(a[:n], dtype=np.float64), np.array(b[:n], dtype=np.float64)
    ea, eb = rng.integers(-400, 400, n), rng.integers(-400, 400, n)
    sa = np.where(rng.random(n) < 0.5, -1.0, 1.0)
    return np.ldexp(sa * a, ea - 52), np.ldexp(b, eb - 52)


def fast_div_out_of_contract():
    inf, nan = np.inf, np.nan
    a, b = [], []
    for x in (0.0, -0.0, inf, -inf, nan):
        for y in (1.0, -3.5, 1e300, 1e-300, 0.0):
            a.append(y); b.append(x)
    for y in (inf, -inf, nan):
        for x in (1.0, -3.5, 1e300, 1e-300):
            a.append(y); b.append(x)
    return np.array(a), np.array(b)


# ------------------------------------------------------------------------------------------------------------------------------------------
# step_root
# ------------------------------------------------------------------------------------------------------------------------------------------
def step_root_inputs():
    """x for every order: log-uniform over [1e-30, 1e30], the controller's errn range 1e-12 .. 1e6, and every binary exponent -8 .. 8
    (the floor division by 3 on negative exponents) with the mantissa at 0.5 exactly, just above it, inside and just below 1 -- which puts
    the reduced argument m at 0.5 exactly and just below 4."""
    rng = np.random.default_rng(21)
    x = [10.0 ** rng.uniform(-30, 30, 300), 10.0 ** rng.uniform(-12, 6, 200)]
    ms = np.array([0.5, np.nextafter(0.5, 1.0), 0.6180339887498949, 0.75, np.nextafter(1.0, 0.0)])
    x.append(np.array([math.ldexp(m, e) for e in range(-8, 10) for m in ms]))
    x = np.concatenate(x)
    return np.tile(x, 3), np.repeat(np.array([1, 2, 3], dtype=np.int32), x.size)


# ------------------------------------------------------------------------------------------------------------------------------------------
# cross-lane helpers: references on arrays shaped [waves, 64]
# ------------------------------------------------------------------------------------------------------------------------------------------
def lane_patterns():
    """Exact patterns, one wave (64 lanes) per row: every group sum is an integer below 2^53, so any summation order gives it exactly and
    its bits name the lanes that contributed."""
    lane = np.arange(64)
    rows = [np.eye(64)[j] * (j + 1) for j in range(64)]                                  # one-hot in lane j, worth j + 1
    rows.append(2.0 ** (lane % 16))                                                      # names the lane within its row of 16
    rows.append(np.where(lane < 32, 2.0 ** (lane % 32), 0.0))                            # names the lane within the wave, lower half
    rows.append(np.where(lane >= 32, 2.0 ** (lane % 32), 0.0))                           # ... upper half
    rows.append(2.0 ** (lane % 32) * (1 + (lane >= 32) * 2.0 ** 20))                     # both halves at once (52 bits)
    rows.append(lane + 1.0)
    rows.append(-(lane + 1.0) * (1 + lane % 3))
    return np.array(rows)


def lane_random(rows=32, seed=31):
    """Mixed signs over 40 decades."""
    rng = np.random.default_rng(seed)
    return np.where(rng.random((rows, 64)) < 0.5, -1.0, 1.0) * 10.0 ** rng.uniform(-20, 20, (rows, 64))


def group_fsum(v, width):
    """math.fsum over aligned groups of `width` lanes (v: [..., L], L a multiple of width), broadcast back to every lane."""
    g = v.reshape(-1, width)
    s = np.array([math.fsum(r) for r in g])
    return np.repeat(s, width).reshape(v.shape)


def group_abs(v, width):
    return np.repeat(np.abs(v).reshape(-1, width).sum(axis=1), width).reshape(v.shape)


# ------------------------------------------------------------------------------------------------------------------------------------------
# Dual<N> operators: exact rational references
# ------------------------------------------------------------------------------------------------------------------------------------------
DUAL_OPS = ("a+b", "a-b", "a*b", "a/b", "a+s", "s+a", "a-s", "s-a", "a*s", "s*a", "a/s", "s/a", "-a")


def dual_op_inputs(seed=41, n=96):
    """a, b as [n, 4] (value, three partials), finite, non-zero values over +-12 decades, partials with zeros and ones among them."""
    rng = np.random.default_rng(seed)
    def draw():
        x = np.where(rng.random((n, 4)) < 0.5, -1.0, 1.0) * 10.0 ** rng.uniform(-12, 12, (n, 4))
        x[:, 1:] *= 10.0 ** rng.uniform(-3, 3, (n, 1))
        x[::5, 2] = 0.0
        x[::7, 1] = 1.0
        x[1::9, 1:] = 0.0
        return x
    a, b = draw(), draw()
    a[:8, 0] = b[:8, 0] * np.array([1, -1, 1 + EPS, 1 - EPS, 2, 0.5, 3, 1 / 3.0])       # cancelling and near-equal values
    return a, b


def dual_ops_exact(a, b):
    """(ref, scale), each [13, n, 4], of DUAL_OPS for a, b [n, 4]: exact rational arithmetic rounded once; the scale is the sum of the
    magnitudes of the terms of each rule (a'b + b'a -> |a'b| + |b'a|, (a' - q b') / b -> (|a'| + |q b'|) / |b|, ...)."""
    n = a.shape[0]
    ref, sc = np.zeros((len(DUAL_OPS), n, 4)), np.zeros((len(DUAL_OPS), n, 4))
    F = Fraction
    for i in range(n):
        av, bv = F(float(a[i, 0])), F(float(b[i, 0]))
        ap, bp = [F(float(x)) for x in a[i, 1:]], [F(float(x)) for x in b[i, 1:]]
        z = [F(0)] * 3
        rows = [
            (av + bv, [x + y for x, y in zip(ap, bp)], abs(av) + abs(bv), [abs(x) + abs(y) for x, y in zip(ap, bp)]),
            (av - bv, [x - y for x, y in zip(ap, bp)], abs(av) + abs(bv), [abs(x) + abs(y) for x, y in zip(ap, bp)]),
            (av * bv, [x * bv + y * av for x, y in zip(ap, bp)], abs(av * bv), [abs(x * bv) + abs(y * av) for x, y in zip(ap, bp)]),
            (av / bv, [(x - av / bv * y) / bv for x, y in zip(ap, bp)], abs(av / bv), [(abs(x) + abs(av / bv * y)) / abs(bv) for x, y in zip(ap, bp)]),
            (av + bv, ap, abs(av) + abs(bv), [abs(x) for x in ap]),
            (bv + av, ap, abs(av) + abs(bv), [abs(x) for x in ap]),
            (av - bv, ap, abs(av) + abs(bv), [abs(x) for x in ap]),
            (bv - av, [-x for x in ap], abs(av) + abs(bv), [abs(x) for x in ap]),
            (av * bv, [x * bv for x in ap], abs(av * bv), [abs(x * bv) for x in ap]),
            (bv * av, [x * bv for x in ap], abs(av * bv), [abs(x * bv) for x in ap]),
            (av / bv, [x / bv for x in ap], abs(av / bv), [abs(x / bv) for x in ap]),
            (bv / av, [-bv / (av * av) * x for x in ap], abs(bv / av), [abs(bv / (av * av) * x) for x in ap]),
            (-av, [-x for x in ap], abs(av), [abs(x) for x in ap]),
        ]
        for k, (v, p, sv, sp) in enumerate(rows):
            ref[k, i] = [float(v)] + [float(x) for x in p]
            sc[k, i] = [float(sv)] + [float(x) for x in sp]
    return ref, sc


def dual_ops_ieee(a, b):
    """The same rules evaluated operation for operation in IEEE doubles ([13, n, 4]): the inf / NaN pattern a singular operand must give."""
    with np.errstate(all="ignore"):
        av, bv, ap, bp = a[:, :1], b[:, :1], a[:, 1:], b[:, 1:]
        ib, ia = 1.0 / bv, 1.0 / av
        q = av * ib
        q2 = bv * ia
        rows = [(av + bv, ap + bp), (av - bv, ap - bp), (av * bv, ap * bv + bp * av), (q, (ap - q * bp) * ib),
                (av + bv, ap), (av + bv, ap), (av - bv, ap), (bv - av, -ap), (av * bv, ap * bv), (av * bv, ap * bv), (av * ib, ap * ib),
                (q2, (-q2 * ia) * ap), (0.0 - av, -ap)]
        return np.array([np.concatenate([v, p], axis=1) for v, p in rows])


def dual_singular_inputs():
    """Operands whose quotient rules meet zero, infinity or NaN."""
    inf, nan = np.inf, np.nan
    vals = [0.0, -0.0, inf, -inf, nan, 2.0]
    a, b = [], []
    for x in vals:
        for y in vals:
            a.append([x, 1.0, 0.0, -2.0]); b.append([y, 0.5, 3.0, 0.0])
    return np.array(a), np.array(b)


# ------------------------------------------------------------------------------------------------------------------------------------------
# the va_* unary functions: code (prim_probe.hip: va_unary), K names, IEEE formulas (numpy) and exact formulas (mpmath)
# ------------------------------------------------------------------------------------------------------------------------------------------
E80 = 5.54062238439351e+34     # exp(80) as va_runtime.hpp writes it (relative error 1e-17)
LN10 = 2.302585092994046


def _np_limexp(x):
    return np.where(x < 80.0, np.exp(np.minimum(x, 80.0)), E80 * (1.0 + x - 80.0))


# name -> (probe code, K name, numpy f(x), numpy df(x, f))
UNARY = {
    "dsqrt": (0, "sqrt", np.sqrt, lambda x, f: 0.5 / f), "dexp": (1, "exp", np.exp, lambda x, f: f), "dlog": (2, "ln", np.log, lambda x, f: 1.0 / x),
    "exp": (3, "exp", np.exp, lambda x, f: f), "ln": (4, "ln", np.log, lambda x, f: 1.0 / x), "log": (5, "log", np.log10, lambda x, f: 1.0 / (x * LN10)),
    "sqrt": (6, "sqrt", np.sqrt, lambda x, f: 0.5 / f), "tanh": (7, "tanh", np.tanh, lambda x, f: 1.0 - f * f),
    "sinh": (8, "sinh", np.sinh, lambda x, f: np.cosh(x)), "cosh": (9, "cosh", np.cosh, lambda x, f: np.sinh(x)),
    "sin": (10, "sin", np.sin, lambda x, f: np.cos(x)), "cos": (11, "cos", np.cos, lambda x, f: -np.sin(x)),
    "atan": (12, "atan", np.arctan, lambda x, f: 1.0 / (1.0 + x * x)), "tan": (13, "tan", np.tan, lambda x, f: 1.0 + f * f),
    "asin": (14, "asin", np.arcsin, lambda x, f: 1.0 / np.sqrt(1.0 - x * x)), "acos": (15, "acos", np.arccos, lambda x, f: -1.0 / np.sqrt(1.0 - x * x)),
    "asinh": (16, "asinh", np.arcsinh, lambda x, f: 1.0 / np.sqrt(x * x + 1.0)), "acosh": (17, "acosh", np.arccosh, lambda x, f: 1.0 / np.sqrt(x * x - 1.0)),
    "atanh": (18, "atanh", np.arctanh, lambda x, f: 1.0 / (1.0 - x * x)),
    "limexp": (19, "limexp", _np_limexp, lambda x, f: np.where(x < 80.0, f, E80)),
}
# exact (value only, plain numbers): code, numpy function
UNARY_EXACT = {"abs": (20, np.abs), "neg": (21, np.negative), "floor": (22, np.floor), "ceil": (23, np.ceil), "int": (24, np.trunc)}


def unary_inputs(name):
    """The whole domain and its edges."""
    up, dn = lambda x: float(np.nextafter(x, np.inf)), lambda x: float(np.nextafter(x, -np.inf))
    tiny = float(np.finfo(np.float64).tiny)
    pm = lambda xs: list(xs) + [-x for x in xs]
    if name in ("dsqrt", "sqrt"):
        xs = list(10.0 ** np.linspace(-300, 300, 25)) + [0.0, tiny, 1.0, 2.0, 4.0, dn(1.0), up(1.0), -1.0]
    elif name in ("dexp", "exp"):
        xs = list(np.linspace(-700, 700, 29)) + [0.0, -0.0, 1e-300, -1e-17, 1.0, 709.0, 709.78, 710.0, 1000.0, -708.0]
    elif name in ("dlog", "ln", "log"):
        xs = list(10.0 ** np.linspace(-300, 300, 25)) + [0.0, tiny, 1e-310, 5e-324, dn(1.0), 1.0, up(1.0), 10.0, 1000.0, -1.0]
    elif name == "tanh":
        xs = list(np.linspace(-20, 20, 41)) + pm([1e-300, 1e-10, 0.3, 19.0, 19.06, 20.0, 50.0, 800.0]) + [0.0]
    elif name in ("sinh", "cosh"):
        xs = list(np.linspace(-30, 30, 31)) + pm([1e-300, 1e-9, 0.3, 700.0, 720.0]) + [0.0]
    elif name in ("sin", "cos", "tan"):
        xs = list(np.linspace(-10, 10, 41)) + pm([1e-300, 1e-9, math.pi / 2, math.pi, 1e6, 1e22]) + [0.0]
    elif name == "atan":
        xs = pm(list(10.0 ** np.linspace(-100, 100, 21))) + [0.0, 1.0, -1.0]
    elif name in ("asin", "acos", "atanh"):
        xs = list(np.linspace(-0.99, 0.99, 23)) + pm([1e-300, 1e-10, 1 - 2.0 ** -20, dn(1.0), 1.0, 1.5]) + [0.0]
    elif name == "asinh":
        xs = pm(list(10.0 ** np.linspace(-100, 100, 21))) + [0.0, 1.0, -1.0]
    elif name == "acosh":
        xs = list(10.0 ** np.linspace(0.01, 100, 21)) + [1.0, up(1.0), 1 + 2.0 ** -20, 2.0, 0.5]
    elif name == "limexp":
        xs = list(np.linspace(-50, 120, 35)) + [dn(80.0), 80.0, up(80.0), 81.0, 200.0, 700.0, 1000.0, -708.0, 0.0]
    else:
        raise KeyError(name)
    return np.array(xs, dtype=np.float64)


def unary_exact_inputs():
    return np.array([0.0, -0.0, 0.3, -0.3, 0.5, -0.5, 1.0, -1.0, 2.5, -2.5, 3.0, -3.0, 1e15 + 0.5, -(1e15 + 0.5), 2.0 ** 53, -2.0 ** 60, 1e-300, -1e-300, 7.999999999999999,
                     -7.999999999999999])


def _mp_unary(name, x):
    """(f, df, scale_f, scale_df) at 60 digits for a double x inside the open domain."""
    import mpmath as mp
    x = mp.mpf(float(x))
    one = mp.mpf(1)
    if name in ("dsqrt", "sqrt"):
        f = mp.sqrt(x); d = 0.5 / f; return f, d, abs(f), abs(d)
    if name in ("dexp", "exp"):
        f = mp.exp(x); return f, f, abs(f), abs(f)
    if name in ("dlog", "ln"):
        f = mp.log(x); d = one / x; return f, d, abs(f), abs(d)
    if name == "log":
        f = mp.log10(x); d = one / (x * mp.log(10)); return f, d, abs(f), abs(d)
    if name == "tanh":
        f = mp.tanh(x); return f, one - f * f, abs(f), max(one, f * f)
    if name == "sinh":
        f = mp.sinh(x); d = mp.cosh(x); return f, d, abs(f), abs(d)
    if name == "cosh":
        f = mp.cosh(x); d = mp.sinh(x); return f, d, abs(f), abs(d)
    if name == "sin":
        f = mp.sin(x); d = mp.cos(x); return f, d, abs(f), abs(d)
    if name == "cos":
        f = mp.cos(x); d = -mp.sin(x); return f, d, abs(f), abs(d)
    if name == "atan":
        f = mp.atan(x); d = one / (1 + x * x); return f, d, abs(f), abs(d)
    if name == "tan":
        f = mp.tan(x); return f, 1 + f * f, abs(f), 1 + f * f
    if name in ("asin", "acos"):
        f = mp.asin(x) if name == "asin" else mp.acos(x)
        d = one / mp.sqrt(1 - x * x) * (1 if name == "asin" else -1)
        return f, d, abs(f), abs(d) * (1 + x * x) / abs(1 - x * x)
    if name == "asinh":
        f = mp.asinh(x); d = one / mp.sqrt(x * x + 1); return f, d, abs(f), abs(d)
    if name == "acosh":
        f = mp.acosh(x); d = one / mp.sqrt(x * x - 1); return f, d, abs(f), abs(d) * (x * x + 1) / abs(x * x - 1)
    if name == "atanh":
        f = mp.atanh(x); d = one / (1 - x * x); return f, d, abs(f), abs(d) * (1 + x * x) / abs(1 - x * x)
    if name == "limexp":
        if x < 80:
            f = mp.exp(x); return f, f, abs(f), abs(f)
        e = mp.exp(80); return e * (1 + x - 80), e, e * (81 + abs(x)), e
    raise KeyError(name)


def _round(x):
    """An mpmath number rounded once to the nearest double (overflow -> inf)."""
    try:
        return float(x)
    except OverflowError:
        return math.copysign(math.inf, float(x > 0) - 0.5)


def build_unary():
    """The fixture of every UNARY function: code, x, f, df, scale_f, scale_df.  Where the IEEE evaluation of the formula is not finite (an
    edge of the domain, an overflow) f / df hold that IEEE result itself."""
    import mpmath as mp
    rows = []
    with mp.workdps(MP_DIGITS), np.errstate(all="ignore"):
        for name, (code, _, npf, npd) in UNARY.items():
            for x in unary_inputs(name):
                f_i = float(npf(np.float64(x)))
                d_i = float(npd(np.float64(x), np.float64(f_i)))
                f = d = sf = sd = None
                if math.isfinite(f_i) or math.isfinite(d_i):
                    try:
                        f, d, sf, sd = _mp_unary(name, x)
                    except (ZeroDivisionError, ValueError):
                        f = None
                ok = f is not None and all(mp.im(v) == 0 for v in (f, d))
                rows.append((code, x,
                             _round(f) if ok and math.isfinite(f_i) else f_i, _round(d) if ok and math.isfinite(d_i) else d_i,
                             _round(sf) if ok and math.isfinite(f_i) else 0.0, _round(sd) if ok and math.isfinite(d_i) else 0.0))
    r = np.array(rows)
    return {"code": r[:, 0].astype(np.int32), "x": r[:, 1], "f": r[:, 2], "df": r[:, 3], "sf": r[:, 4], "sdf": r[:, 5]}


def unary_partials(n, width, seed=51):
    """Partials of the argument: [n, width] with a one, a zero and a negative among them."""
    rng = np.random.default_rng(seed)
    p = np.round(rng.uniform(-2, 2, (n, width)), 3)
    p[:, 0] = np.where(np.arange(n) % 2 == 0, 1.0, p[:, 0])
    if width > 1:
        p[:, 1] = np.where(np.arange(n) % 3 == 0, 0.0, p[:, 1])
    return p


# ------------------------------------------------------------------------------------------------------------------------------------------
# the two-argument functions: pow, atan2, hypot (mpmath fixture); min / max / site are exact selections
# ------------------------------------------------------------------------------------------------------------------------------------------
POW_SHORTCUTS = (0.5, 1.0, 2.0, -1.0, -0.5, 0.0, 1.5, 3.0)


def binary_inputs():
    """(fn, a, b, kind): fn 0 pow, 1 atan2 (a = y, b = x), 2 hypot.  kind: 0 general, 1 pow shortcut exponent (value held to 2 ulp),
    2 pow with a negative base and an integer exponent (exponent partials must be zero: no logarithm exists), 3 pow at a = 0, 4 value only
    (the neighbours of the exponent 0 are subnormal, and so is b f / a)."""
    up, dn = lambda x: float(np.nextafter(x, np.inf)), lambda x: float(np.nextafter(x, -np.inf))
    rows = []
    bases = (0.3, 1.0, 2.7, 1e-5, 4e7, 0.9999999)
    for b in POW_SHORTCUTS:
        for a in bases:
            rows.append((0, a, b, 1))
            rows.append((0, a, up(b), 4 if b == 0.0 else 0)); rows.append((0, a, dn(b), 4 if b == 0.0 else 0))       # the neighbours take the general path
    for b in (0.3, 2.5, -1.7, 17.0, -0.01, 1e-300, -1e-300):
        for a in bases + (1e-100, 1e100):
            rows.append((0, a, b, 0))
    for b in (0.0, 0.5, 1.0, 1.5, 2.0, 3.0):
        rows.append((0, 0.0, b, 3))
    for a in (-2.0, -0.5, -3.25):
        for b in (3.0, 2.0, 1.0, -1.0, 4.0, -3.0, 5.0, 0.0):
            rows.append((0, a, b, 2))
    ax = (1.0, -1.0, 0.5, -0.5, 0.0, -0.0, 3e8, -1e-9)
    for y in ax:
        for x in ax:
            rows.append((1, y, x, 0))
            rows.append((2, y, x, 0))
    rows += [(2, 3e100, 4e100, 0), (2, 3e-100, -4e-100, 0), (2, 1e10, 1e-10, 0)]
    r = np.array(rows)
    return r[:, 0].astype(np.int32), r[:, 1], r[:, 2], r[:, 3].astype(np.int32)


def binary_ieee(fn, a, b):
    """(f, da, db) as va_runtime.hpp's formulas give them in IEEE doubles (scalars)."""
    with np.errstate(all="ignore"):
        a, b = np.float64(a), np.float64(b)
        if fn == 0:
            f = np.float64(1.0) if b == 0.0 else np.power(a, b)
            if b == 0.0:
                da = np.float64(0.0)
            elif a != 0.0:
                da = b * f / a
            else:
                da = b * (np.float64(1.0) if b - 1.0 == 0.0 else np.power(a, b - 1.0))
            return f, da, f * np.log(a)
        if fn == 1:
            d = b * b + a * a
            return np.arctan2(a, b), b / d, -a / d
        h = np.sqrt(a * a + b * b)
        return np.hypot(a, b), a / h, b / h


def _mp_binary(fn, a, b):
    import mpmath as mp
    a, b = mp.mpf(float(a)), mp.mpf(float(b))
    if fn == 0:
        f = mp.power(a, b) if b != 0 else mp.mpf(1)
        if b == 0:
            da = mp.mpf(0)
        elif a != 0:
            da = b * f / a
        else:
            da = b * (mp.power(a, b - 1) if b != 1 else mp.mpf(1))
        db = f * mp.log(a) if a > 0 else mp.mpf(0)
        return f, da, db
    if fn == 1:
        d = a * a + b * b
        return mp.atan2(a, b), b / d, -a / d
    h = mp.sqrt(a * a + b * b)
    return h, a / h, b / h


def build_binary():
    import mpmath as mp
    fn, a, b, kind = binary_inputs()
    out = np.zeros((fn.size, 3))
    with mp.workdps(MP_DIGITS):
        for i in range(fn.size):
            ie = [float(v) for v in binary_ieee(fn[i], a[i], b[i])]
            if kind[i] == 2:
                ie[2] = 0.0                     # negative base: the exponent carries no partial, nothing is asked of f log(a)
            try:
                ex = _mp_binary(fn[i], a[i], b[i])
            except (ZeroDivisionError, ValueError):
                ex = (None, None, None)
            if fn[i] == 1 and (a[i] == 0.0 or b[i] == 0.0):
                ex = (None,) + tuple(ex[1:])    # on the axes the signs of the zeros decide (mpmath has none): the IEEE value, a multiple of pi / 2
            for k in range(3):
                real = ex[k] is not None and mp.im(ex[k]) == 0
                out[i, k] = _round(mp.re(ex[k])) if (math.isfinite(ie[k]) and real) else ie[k]
    return {"fn": fn, "a": a, "b": b, "kind": kind, "f": out[:, 0], "da": out[:, 1], "db": out[:, 2]}


# ------------------------------------------------------------------------------------------------------------------------------------------
# limiters: inputs, the return path each takes, and the references
# ------------------------------------------------------------------------------------------------------------------------------------------
VT, VCRIT, VTO = 0.025852, 0.6145, 0.7


def _nb(x):
    """x, and one double to either side."""
    return [float(np.nextafter(x, -np.inf)), float(x), float(np.nextafter(x, np.inf))]


def limiter_inputs():
    """(vnew, vold, boundary): the grid -5 .. 10 V in both arguments, then every comparison's boundary -- exactly on it and one double
    to either side (boundary = True for those)."""
    g = np.arange(-5.0, 10.0 + 1e-9, 0.5)
    g = np.concatenate([g, [0.01, 0.03, 0.62, 0.65, 0.7, 1.3, 4.2, 4.3]])
    vn, vo = [x.ravel() for x in np.meshgrid(g, g)]
    ngrid = vn.size
    pn, po = [], []
    def add(vnews, volds):
        for a in vnews:
            for b in volds:
                pn.append(a); po.append(b)
    olds = [-3.0, -0.2, 0.0, 0.3, 0.65, 0.7, 2.0, 4.2, 5.0, 9.0]
    add(_nb(VCRIT), olds)                                           # vnew = vcrit
    for o in olds + [-1.0, 0.01]:
        add(_nb(o + 2 * VT) + _nb(o - 2 * VT), [o])                 # |vnew - vold| = 2 vt
        add(_nb(-o - 1.0) + _nb(2.0 * o - 1.0), [o])                # vnew = arg of the negative branch
        add(_nb(o), [o])                                            # delv = 0
        hi, lo = abs(2 * (o - VTO)) + 2, abs(o - VTO) + 1
        add(_nb(o + hi) + _nb(o - hi) + _nb(o + lo) + _nb(o - lo), [o])     # delv = +-vtsthi, +-vtstlo
        add(_nb(3 * o + 2), [o])                                    # limvds: vnew = 3 vold + 2
    news = [-6.0, -1.0, 0.0, 0.3, 0.9, 1.0, 1.2, 2.0, 3.0, 3.6, 4.5, 5.0, 8.0, 30.0]
    add(news, _nb(0.0) + _nb(VTO) + _nb(VTO + 3.5) + _nb(3.5))      # vold = 0, vto, vto + 3.5, 3.5
    add(_nb(VTO + 0.5) + _nb(3.5) + _nb(VTO + 3.5) + _nb(VTO + 2) + _nb(VTO - 0.5) + _nb(VTO + 4) + _nb(4.0) + _nb(2.0) + _nb(-0.5) + _nb(0.0), olds)
    vn, vo = np.concatenate([vn, pn]), np.concatenate([vo, po])
    return vn, vo, np.arange(vn.size) >= ngrid


def pnjlim_path(vnew, vold, vt, vcrit):
    """The return path of pnjlim / DEVpnjlim (same tests): 0..2 take a logarithm."""
    if vnew > vcrit and abs(vnew - vold) > vt + vt:
        if vold > 0.0:
            return 0 if (vnew - vold) / vt > 0.0 else 1
        return 2
    if vnew < 0.0:
        arg = -vold - 1.0 if vold > 0.0 else 2.0 * vold - 1.0
        return (3 if vold > 0.0 else 4) if vnew < arg else 5
    return 6


def fetlim_path(vnew, vold, vto):
    hi, lo, vtox, delv = abs(2 * (vold - vto)) + 2, abs(vold - vto) + 1, vto + 3.5, vnew - vold
    if vold >= vto:
        if vold >= vtox:
            if delv <= 0:
                if vnew >= vtox:
                    return 0 if -delv > lo else 1
                return 2
            return 3 if delv >= hi else 4
        return 5 if delv <= 0 else 6
    if delv <= 0:
        return 7 if -delv > hi else 8
    if vnew <= vto + 0.5:
        return 9 if delv > lo else 10
    return 11


def limvds_path(vnew, vold):
    if vold >= 3.5:
        if vnew > vold:
            return 0
        return 1 if vnew < 3.5 else 2
    return 3 if vnew > vold else 4


N_PATHS = {"pnjlim": 7, "fetlim": 12, "limvds": 5}
# two branches of DEVfetlim that no input reaches: path 0 needs vnew >= vto + 3.5 and vold - vnew > |vold - vto| + 1, i.e. vnew < vto - 1;
# path 9 needs vnew <= vto + 0.5 and vnew - vold > (vto - vold) + 1, i.e. vnew > vto + 1
UNREACHABLE = {"pnjlim": set(), "fetlim": {0, 9}, "limvds": set()}


def limiter_reference(vn, vo):
    """([4, n] references from the oracle: pnjlim, DEVpnjlim, DEVfetlim, DEVlimvds; [4, n] return paths; [n] scale of the two logarithmic
    results' tolerance: |vold| + vt (2 + |log term|))."""
    from oracle import devices_ref as D, va_mos1_ref as M
    n = vn.size
    ref, path, scale = np.zeros((4, n)), np.zeros((4, n), dtype=np.int32), np.zeros((2, n))
    for i in range(n):
        a, b = float(vn[i]), float(vo[i])
        ref[0, i] = D.pnjlim(a, b, VT, VCRIT)[0]
        ref[1, i] = M.DEVpnjlim(a, b, VT, VCRIT, 0)[0]
        ref[2, i] = M.DEVfetlim(a, b, VTO, 0)[0]
        ref[3, i] = M.DEVlimvds(a, b, 0)[0]
        p = pnjlim_path(a, b, VT, VCRIT)
        path[0, i] = path[1, i] = p
        path[2, i] = fetlim_path(a, b, VTO)
        path[3, i] = limvds_path(a, b)
        if p <= 2:
            for r in (0, 1):       # the terms: vold, (2 vt,) vt log(...)
                if p == 2:
                    scale[r, i] = abs(ref[r, i])
                else:
                    t = abs(ref[r, i] - b)
                    scale[r, i] = abs(b) + (abs(t - 2.0 * VT) + 2.0 * VT if r == 0 else t)
    return ref, path, scale


# ------------------------------------------------------------------------------------------------------------------------------------------
# source waves
# ------------------------------------------------------------------------------------------------------------------------------------------
def pwl_cases():
    """(ts, ys) tables: n = 1, n = 2, interior points, duplicated time points, flat segments, irrational slopes."""
    return [
        ([1.0], [2.5]),
        ([0.0, 1e-9], [0.0, 1.8]),
        ([0.0, 1e-9, 3e-9, 3.5e-9, 7e-9], [0.0, 1.8, 1.8, 0.3, 0.7]),                    # a flat segment inside
        ([0.0, 1.0, 1.0, 2.0, 2.0, 2.0, 3.0], [0.1, 0.7, -0.4, -0.4, 0.9, 0.2, 0.35]),   # steps: duplicated and triplicated points
        ([-2.0, -1.0, 0.5, 0.7, 1.1, 1.3, 1.9, 2.3, 3.1], [0.3, -0.7, 1.1, 1.1, 0.123456789, 2.0 / 3.0, -1.0 / 7.0, 0.9, 0.9]),
        ([0.1, 0.1], [1.0, 2.0]),                                                        # a step and nothing else
    ]


def pwl_inputs():
    """Flattened probe inputs: tab, and per element (t, off, len, hint); every t of a table with no hint (-1) and every hint 0 .. n + 1."""
    tab, rows = [], []
    for ts, ys in pwl_cases():
        off, n = len(tab), len(ts)
        tab += list(ts) + list(ys)
        tt = [ts[0] - 1.0, ts[-1] + 1.0, float(np.nextafter(ts[0], -np.inf)), float(np.nextafter(ts[-1], np.inf))]
        for k, t in enumerate(ts):
            tt += _nb(t)
            if k + 1 < n and ts[k + 1] > t:
                tt += [t + 0.5 * (ts[k + 1] - t), t + (ts[k + 1] - t) / 3.0]
        for t in tt:
            for hint in range(-1, n + 2):
                rows.append((t, off, n, hint))
    r = np.array(rows)
    return np.array(tab), r[:, 0], r[:, 1].astype(np.int32), r[:, 2].astype(np.int32), r[:, 3].astype(np.int32)


def pwl_reference(tab, t, off, ln):
    from oracle import devices_ref as D
    val, idx = np.zeros(t.size), np.zeros(t.size, dtype=np.int32)
    for i in range(t.size):
        ts, ys = list(tab[off[i]:off[i] + ln[i]]), list(tab[off[i] + ln[i]:off[i] + 2 * ln[i]])
        val[i] = D.pwl_at_time(ts, ys, float(t[i]))
        idx[i] = D.find_t_in_ts(ts, float(t[i]))
    return val, idx


def pulse_inputs():
    """[8, n]: v1 v2 td tr tf pw per t -- zero rise / fall, per = 0, t on every phase boundary and a double to either side, t < td, many periods."""
    cards = [(0.0, 1.8, 1e-9, 1e-10, 2e-10, 1e-9, 4e-9), (0.3, -1.1, 0.0, 0.0, 0.0, 1e-9, 3e-9), (1.0 / 3.0, 2.0 / 7.0, 2e-9, 3e-10, 0.0, 5e-10, 0.0),
             (-0.5, 0.7, 5e-10, 0.0, 1e-10, 2e-10, 1e-9), (0.1, 3.3, 1.0, 0.125, 0.25, 0.5, 2.0)]
    rows = []
    for v1, v2, td, tr, tf, pw, per in cards:
        tt = [-1.0, td - 1e-12] + _nb(td)
        for base in (td, td + per, td + 5 * per, td + 1000 * per, td + 123457 * per):
            for ph in (0.0, tr, tr + pw, tr + pw + tf, per, 0.5 * tr, tr + 0.3 * pw, tr + pw + tf / 3.0, 0.9 * per):
                tt += _nb(base + ph)
        rows += [(v1, v2, td, tr, tf, pw, per, t) for t in tt]
    return np.array(rows).T.copy()


def pulse_reference(x):
    from oracle import devices_ref as D
    return np.array([D.pulse_at_time(*[float(v) for v in x[:, i]]) for i in range(x.shape[1])])


def sind_inputs():
    rng = np.random.default_rng(61)
    m30 = np.arange(-720.0, 721.0, 30.0)
    return np.concatenate([m30, [90.0, -90.0, 180.0, -180.0, 270.0, -270.0, 360.0, 1e6, -1e6, 1e6 + 90.0, 999990.0, 1e6 + 0.5, 123456.789, 0.0, 1e-300, 45.0, 1.0],
                           rng.uniform(-1e6, 1e6, 40), rng.uniform(-360, 360, 40)])


def build_sind():
    import mpmath as mp
    deg = sind_inputs()
    with mp.workdps(MP_DIGITS):
        ref = np.array([_round(mp.sin(mp.pi * mp.mpf(float(d)) / 180)) for d in deg])
    return {"deg": deg, "ref": ref}


def build_step_root():
    import mpmath as mp
    x, order = step_root_inputs()
    with mp.workdps(MP_DIGITS):
        ref = np.array([_round(mp.power(mp.mpf(float(a)), -mp.mpf(1) / (int(o) + 1))) for a, o in zip(x, order)])
    return {"x": x, "order": order, "ref": ref}


def source_inputs():
    """The waves of source_value as (tab, rows of (t, dc, scale, kind, off, len, mode)): dc sources, every kind in every mode, the damped sine
    on both sides of its delay."""
    tab = [0.0, 1e-9, 2e-9, 0.0, 1.0, 0.25]                         # PWL: 3 points at 0
    pulse_off = len(tab); tab += [0.0, 1.8, 1e-9, 1e-10, 1e-10, 1e-9, 4e-9]
    sine_off = len(tab); tab += [0.9, 0.45, 1e8, 2e-9, 3e7, 30.0]   # vo va freq td theta phase
    sine2_off = len(tab); tab += [0.0, 1.0, 2.5e8, 0.0, 0.0, 0.0]
    rows = []
    for mode in (0, 1, 2):
        for t in (0.0, 5e-10, 1e-9, 1.5e-9, 1.999e-9, 2e-9, 2.001e-9, 3.3e-9, 7.77e-9, 1.2345e-8):
            for kind, off, ln in ((0, 0, 0), (1, 0, 3), (2, pulse_off, 7), (3, sine_off, 6), (3, sine2_off, 6)):
                rows.append((t, 0.77, 1.5, kind, off, ln, mode))
    return np.array(tab), np.array(rows)


def source_reference(tab, rows):
    """(value, scale) in Python doubles, operation for operation (oracle waves; the sine as devices.hpp writes it)."""
    from oracle import devices_ref as D
    val, sc = np.zeros(len(rows)), np.zeros(len(rows))
    for i, (t, dc, scale, kind, off, ln, mode) in enumerate(rows):
        kind, off, ln = int(kind), int(off), int(ln)
        w = tab[off:]
        if kind == 0 or mode == 0:
            val[i] = dc; continue
        if kind == 1:
            v = D.pwl_at_time(list(w[:ln]), list(w[ln:2 * ln]), t)
        elif kind == 2:
            v = D.pulse_at_time(*[float(x) for x in w[:7]], t)
        else:
            vo, va, freq, td, theta, phase = [float(x) for x in w[:6]]
            if t < td:
                s, e, arg = D.sind(phase), 1.0, phase
            else:
                arg = 360 * freq * (t - td) + phase
                s, e = D.sind(arg), math.exp(-theta * (t - td))
            v = vo + va * e * s
            # a fused multiply-add in the argument moves it by half an ulp: |arg| 2^-53 degrees, pi / 180 of that in the sine
            sc[i] = abs(scale) * (abs(vo) + abs(va) * e * (1.0 + abs(math.radians(arg))))
        val[i] = scale * v
    return val, sc


# ------------------------------------------------------------------------------------------------------------------------------------------
# behavioural sources: postfix programs (include/cadnip_hip.h: CADNIP_BOP_*)
# ------------------------------------------------------------------------------------------------------------------------------------------
CONST, V, TIME, ADD, SUB, MUL, DIV, POW, MIN, MAX, NEG, EXP, LOG, SQRT, ABS, TANH, SIN, COS = 0, 1, 2, 10, 11, 12, 13, 14, 15, 16, 20, 21, 22, 23, 24, 25, 26, 27
BSRC_MAX_STACK = 16
BSRC_U = (0.8125, -1.3, 2.0 / 3.0, 0.05)
BSRC_T = 1.25


def bsrc_programs():
    """(name, gain, program): one per opcode, the probe V(a, b) with either node grounded, one of the full stack depth, one mixing every
    opcode.  The operands of the one-opcode programs are probes, not constants (nothing to fold)."""
    x, y = [V, 0, -1], [V, 2, 1]                     # 0.8125, 2/3 + 1.3
    P = [("const", 1.0, [CONST, 0.3]), ("v", 1.0, [V, 0, 1]), ("v_gnd_n", 1.0, [V, 1, -1]), ("v_gnd_p", 1.0, [V, -1, 1]), ("v_gnd_both", 1.0, [V, -1, -1]),
         ("time", 1.0, [TIME]), ("gain", -2.5, [V, 3, 0])]
    for nm, op in (("add", ADD), ("sub", SUB), ("mul", MUL), ("div", DIV), ("pow", POW), ("min", MIN), ("max", MAX)):
        P.append((nm, 1.0, x + y + [op]))
        P.append((nm + "_r", 1.0, y + x + [op]))     # operand order: x op y with y on top
    for nm, op in (("neg", NEG), ("exp", EXP), ("log", LOG), ("sqrt", SQRT), ("abs", ABS), ("tanh", TANH), ("sin", SIN), ("cos", COS)):
        P.append((nm, 1.0, y + [op]))
    P.append(("abs_neg", 1.0, [V, 1, -1, ABS]))
    deep = []
    for k in range(BSRC_MAX_STACK):
        deep += [CONST, 1.0 + k / 7.0] if k % 2 else [V, k % 4, -1]
    deep += [ADD, MUL, SUB, ADD, MAX, ADD, SUB, MIN, ADD, MUL, ADD, SUB, ADD, ADD, SUB]
    P.append(("full_stack", 1.0, deep))
    mixed = (x + [EXP] + y + [LOG, ADD] + [V, 0, 1, TANH, MUL] + [TIME, CONST, 0.75, MUL, SIN, SUB] + [V, 2, -1, SQRT] + [V, 3, -1, COS, DIV, ADD]
             + [V, 1, -1, ABS, CONST, 1.7, POW, ADD] + [CONST, 1.0, MAX] + [V, 1, -1, NEG, CONST, 4.0, MUL, MIN] + [CONST, 0.5, ADD])
    P.append(("mixed", 2.5, mixed))
    return P


def bsrc_eval(prog, u, t, lib):
    """The stack evaluator (devices.hpp: bsrc_value).  ``lib``: name -> function for pow exp log sqrt tanh sin cos; the arithmetic is the
    number type's own.  Returns (st[0], deepest stack, every value produced)."""
    st, seen, deep, i = [], [], 0, 0
    volt = lambda k: u[k] if k >= 0 else u[0] * 0
    while i < len(prog):
        op = int(prog[i]); i += 1
        if op == CONST:
            st.append(u[0] * 0 + prog[i]); i += 1
        elif op == V:
            st.append(volt(int(prog[i])) - volt(int(prog[i + 1]))); i += 2
        elif op == TIME:
            st.append(u[0] * 0 + t)
        elif op < NEG:
            y = st.pop(); x = st[-1]
            st[-1] = {ADD: lambda: x + y, SUB: lambda: x - y, MUL: lambda: x * y, DIV: lambda: x / y, POW: lambda: lib["pow"](x, y),
                      MIN: lambda: y if y < x else x, MAX: lambda: y if y > x else x}[op]()
        else:
            x = st[-1]
            st[-1] = {NEG: lambda: -x, EXP: lambda: lib["exp"](x), LOG: lambda: lib["log"](x), SQRT: lambda: lib["sqrt"](x), ABS: lambda: abs(x),
                      TANH: lambda: lib["tanh"](x), SIN: lambda: lib["sin"](x), COS: lambda: lib["cos"](x)}[op]()
        deep = max(deep, len(st))
        seen.append(st[-1])
    return st[0], deep, seen


def bsrc_uses_library(prog):
    """True when the program calls the math library (its result carries a tolerance); walks the program as the evaluator does."""
    i, lib = 0, False
    while i < len(prog):
        op = int(prog[i]); i += 1
        i += {CONST: 1, V: 2}.get(op, 0)
        lib = lib or op in BOP_SPEC and op != SQRT
    return lib


def bsrc_k(prog):
    i, k = 0, ARITH
    while i < len(prog):
        op = int(prog[i]); i += 1
        i += {CONST: 1, V: 2}.get(op, 0)
        k += BOP_SPEC.get(op, 0)
    return k


def bsrc_float_reference():
    """Programs in Python doubles (math library): exact for the arithmetic opcodes."""
    lib = {"pow": math.pow, "exp": math.exp, "log": math.log, "sqrt": math.sqrt, "tanh": math.tanh, "sin": math.sin, "cos": math.cos}
    return np.array([g * bsrc_eval(p, list(BSRC_U), BSRC_T, lib)[0] for _, g, p in bsrc_programs()])


def build_bsrc():
    """Per program: the value with mpmath behind every opcode, and the scale (the magnitudes of every value produced, times |gain|)."""
    import mpmath as mp
    lib = {"pow": mp.power, "exp": mp.exp, "log": mp.log, "sqrt": mp.sqrt, "tanh": mp.tanh, "sin": mp.sin, "cos": mp.cos}
    ref, sc = [], []
    with mp.workdps(MP_DIGITS):
        for _, g, p in bsrc_programs():
            r, _, seen = bsrc_eval(p, [mp.mpf(x) for x in BSRC_U], mp.mpf(BSRC_T), lib)
            ref.append(_round(g * r)); sc.append(_round(abs(g) * sum(abs(s) for s in seen)))
    return {"ref": np.array(ref), "scale": np.array(sc)}


# ------------------------------------------------------------------------------------------------------------------------------------------
# fixtures
# ------------------------------------------------------------------------------------------------------------------------------------------
BUILDERS = {"prim_unary": build_unary, "prim_binary": build_binary, "prim_sind": build_sind, "prim_step_root": build_step_root, "prim_bsrc": build_bsrc}


def fixture_path(name):
    return os.path.join(GOLD, name + ".npz")


def load_fixture(name):
    with np.load(fixture_path(name)) as z:
        return {k: z[k] for k in z.files}
