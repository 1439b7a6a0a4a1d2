"""The references of tests/test_gpu_primitives.py checked on their own (no GPU): the committed mpmath fixtures are current, every analytic
derivative agrees with numerical differentiation at 60 digits, the dual rules agree with oracle/dual.py, the limiter inputs reach every
return path, and the structured inputs have the properties their tests rely on."""
import math
import os
from fractions import Fraction

import numpy as np
import pytest

from oracle import cpu_port, devices_ref as D, dual as OD
from tests import prim_ref as R


def _bits(x):
    x = np.asarray(x)
    return x.view(np.int64) if x.dtype == np.float64 else x


def test_fixtures_are_current():
    """tools/make_prim_fixtures.py would write the same arrays, bit for bit; the files stay small."""
    pytest.importorskip("mpmath")
    total = 0
    for name, build in R.BUILDERS.items():
        have, want = R.load_fixture(name), build()
        assert sorted(have) == sorted(want), name
        for k in want:
            assert have[k].dtype == want[k].dtype and np.array_equal(_bits(have[k]), _bits(want[k])), "%s[%s] is stale: run tools/make_prim_fixtures.py" % (name, k)
        total += os.path.getsize(R.fixture_path(name))
    assert total < 200 * 1024


def test_k_table():
    for name, (_, kname, _, _) in R.UNARY.items():
        assert R.K[kname + ".f"] >= R.ARITH and R.K[kname + ".d"] >= R.ARITH, name
    assert all(v >= R.ARITH for v in R.K.values())
    assert R.K["tanh.d"] == 2 * R.SPEC["tanh"] + R.ARITH and R.K["pow.db"] == R.SPEC["pow"] + R.SPEC["log"] + R.ARITH


def test_unary_derivatives_agree_with_numerical_differentiation():
    mp = pytest.importorskip("mpmath")
    fns = {"dsqrt": mp.sqrt, "dexp": mp.exp, "dlog": mp.log, "exp": mp.exp, "ln": mp.log, "log": mp.log10, "sqrt": mp.sqrt, "tanh": mp.tanh, "sinh": mp.sinh,
           "cosh": mp.cosh, "sin": mp.sin, "cos": mp.cos, "atan": mp.atan, "tan": mp.tan, "asin": mp.asin, "acos": mp.acos, "asinh": mp.asinh,
           "acosh": mp.acosh, "atanh": mp.atanh, "limexp": lambda x: mp.exp(x) if x < 80 else mp.exp(80) * (1 + x - 80)}
    pts = {"acosh": (1.5, 7.0), "limexp": (-3.0, 79.0, 81.0, 300.0), "dlog": (0.2, 30.0), "ln": (0.2, 30.0), "log": (0.2, 30.0), "dsqrt": (0.2, 30.0), "sqrt": (0.2, 30.0)}
    with mp.workdps(R.MP_DIGITS):
        for name in R.UNARY:
            for x in pts.get(name, (-0.7, 0.3)):
                f, d, _, _ = R._mp_unary(name, x)
                assert abs(f - fns[name](mp.mpf(x))) <= mp.mpf(10) ** -50 * (1 + abs(f)), name
                assert abs(d - mp.diff(fns[name], mp.mpf(x))) <= mp.mpf(10) ** -30 * (1 + abs(d)), name


def test_binary_derivatives_agree_with_numerical_differentiation():
    mp = pytest.importorskip("mpmath")
    fns = {0: lambda a, b: mp.power(a, b), 1: lambda y, x: mp.atan2(y, x), 2: lambda a, b: mp.sqrt(a * a + b * b)}
    with mp.workdps(R.MP_DIGITS):
        for fn, f in fns.items():
            for a, b in ((0.7, 1.3), (2.5, -0.4), (1.9, 3.0)):
                v, da, db = R._mp_binary(fn, a, b)
                assert abs(v - f(mp.mpf(a), mp.mpf(b))) <= mp.mpf(10) ** -50
                assert abs(da - mp.diff(f, (mp.mpf(a), mp.mpf(b)), (1, 0))) <= mp.mpf(10) ** -30
                assert abs(db - mp.diff(f, (mp.mpf(a), mp.mpf(b)), (0, 1))) <= mp.mpf(10) ** -30


def test_fixture_values_agree_with_numpy():
    """The IEEE formulas (which decide the non-finite patterns) and the mpmath values describe the same functions."""
    fx = R.load_fixture("prim_unary")
    with np.errstate(all="ignore"):
        for name, (code, kname, npf, npd) in R.UNARY.items():
            m = fx["code"] == code
            f = npf(fx["x"][m])
            R.check_close(f, fx["f"][m], fx["sf"][m], 4 + R.ARITH, name)           # the host libm: within 4 ulp
            R.check_close(npd(fx["x"][m], f), fx["df"][m], fx["sdf"][m], 2 * 4 + R.ARITH, name + " derivative")
    fb = R.load_fixture("prim_binary")
    for i in range(fb["a"].size):
        ie = R.binary_ieee(fb["fn"][i], fb["a"][i], fb["b"][i])
        if fb["kind"][i] in (2, 4):
            ie = ie[:1]
        for got, ref in zip(ie, (fb["f"][i], fb["da"][i], fb["db"][i])):
            R.check_close(got, ref, abs(ref), 2 * (4 + R.ARITH), "binary %d (%r, %r)" % (fb["fn"][i], fb["a"][i], fb["b"][i]))
    # every edge the GPU test promises is in the fixture
    x = {name: set(fx["x"][fx["code"] == code]) for name, (code, _, _, _) in R.UNARY.items()}
    assert {20.0, -20.0} <= x["tanh"] and {709.0, 710.0} <= x["exp"] and {0.0} <= x["ln"] and {0.0} <= x["log"]
    for name in ("asin", "acos", "atanh"):
        assert {1.0, -1.0, 1 - 2.0 ** -20, -(1 - 2.0 ** -20)} <= x[name]
    assert {1.0, 1 + 2.0 ** -20} <= x["acosh"]
    assert {float(np.nextafter(80.0, 0.0)), 80.0, float(np.nextafter(80.0, 100.0)), 700.0} <= x["limexp"]
    pw = fb["fn"] == 0
    for b in R.POW_SHORTCUTS:
        for nb in (b, float(np.nextafter(b, np.inf)), float(np.nextafter(b, -np.inf))):
            assert np.any(pw & (fb["b"] == nb)), nb
    assert set(fb["b"][pw & (fb["a"] == 0.0)]) == {0.0, 0.5, 1.0, 1.5, 2.0, 3.0}
    assert np.all(np.isfinite(fb["f"][fb["kind"] == 2])) and np.all(fb["a"][fb["kind"] == 2] < 0)


def test_dual_rules_agree_with_the_oracle():
    """oracle/dual.py carries the same rules: its doubles agree with the exact rational results within K, and its elementary functions
    with the fixture."""
    a, b = R.dual_op_inputs()
    ref, sc = R.dual_ops_exact(a, b)
    ops = [lambda x, y, s: x + y, lambda x, y, s: x - y, lambda x, y, s: x * y, lambda x, y, s: x / y, lambda x, y, s: x + s, lambda x, y, s: s + x,
           lambda x, y, s: x - s, lambda x, y, s: s - x, lambda x, y, s: x * s, lambda x, y, s: s * x, lambda x, y, s: x / s, lambda x, y, s: s / x,
           lambda x, y, s: -x]
    got = np.zeros_like(ref)
    for i in range(a.shape[0]):
        x, y = OD.Dual(a[i, 0], a[i, 1:].copy()), OD.Dual(b[i, 0], b[i, 1:].copy())
        for k, op in enumerate(ops):
            r = op(x, y, float(b[i, 0]))
            got[k, i, 0], got[k, i, 1:] = r.v, r.p
    for k, name in enumerate(R.DUAL_OPS):
        R.check_close(got[k], ref[k], sc[k], R.K["arith"], "oracle Dual " + name)
    ie = R.dual_ops_ieee(a, b)
    for k, name in enumerate(R.DUAL_OPS):
        R.check_close(ie[k], ref[k], sc[k], R.K["arith"], "IEEE rules " + name)
    fx = R.load_fixture("prim_unary")
    for name, fn in (("dsqrt", OD.dsqrt), ("dexp", OD.dexp), ("dlog", OD.dln)):
        m = (fx["code"] == R.UNARY[name][0]) & np.isfinite(fx["f"]) & np.isfinite(fx["df"])
        r = [fn(OD.Dual(x, np.array([1.0, -0.5]))) for x in fx["x"][m]]
        kname = R.UNARY[name][1]
        R.check_close([q.v for q in r], fx["f"][m], fx["sf"][m], 1 + R.ARITH, name)
        R.check_close([q.p[1] for q in r], -0.5 * fx["df"][m], 0.5 * fx["sdf"][m], 1 + R.ARITH, name + " partial")
    # ties of min / max take the first operand, there as here
    x, y = OD.Dual(1.0, np.array([1.0])), OD.Dual(1.0, np.array([2.0]))
    assert OD.dmax(x, y) is x and OD.dmin(x, y) is x and OD.dabs(OD.Dual(-0.0, np.array([1.0]))).p[0] == 1.0


def test_limiter_inputs_reach_every_return_path():
    """The reference takes every reachable return path of every limiter, and at most one path in ten is reached by boundary points only."""
    vn, vo, boundary = R.limiter_inputs()
    ref, path, scale = R.limiter_reference(vn, vo)
    assert vn[~boundary].min() == -5.0 and vn[~boundary].max() == 10.0 and np.all(np.abs(vn[~boundary]) <= 10.0) and np.all(np.abs(vo[~boundary]) <= 10.0)
    n_paths = n_boundary_only = 0
    for r, name in ((0, "pnjlim"), (2, "fetlim"), (3, "limvds")):
        reach = set(range(R.N_PATHS[name])) - R.UNREACHABLE[name]
        assert set(path[r]) == reach, name
        n_paths += len(reach)
        n_boundary_only += len(reach - set(path[r][~boundary]))
    assert n_boundary_only * 10 <= n_paths, (n_boundary_only, n_paths)
    assert np.array_equal(ref[0][path[0] >= 3], ref[1][path[1] >= 3])          # the two junction limiters differ in their logarithms only
    assert np.all(scale[:, path[0] <= 2] > 0) and np.all(scale[:, path[0] > 2] == 0)
    # a limited point reports a value different from vnew, an unlimited one vnew itself
    for r in range(4):
        unl = {0: 6, 1: 6}.get(r)
        if unl is not None:
            assert np.array_equal(ref[r][path[r] == unl], vn[path[r] == unl])
    # each boundary is met on both sides: the neighbouring doubles of a boundary point take different paths somewhere
    for r in (0, 2, 3):
        b = path[r][boundary]
        assert np.any(b[:-1] != b[1:])


def test_fast_div_inputs():
    a, b = R.fast_div_hard(n=2000)
    tiny = np.finfo(np.float64).tiny
    assert np.all((np.abs(b) >= tiny) & np.isfinite(b)) and np.all(np.abs(a / b) >= tiny)
    for x, y in zip(a[:300], b[:300]):
        q = abs(Fraction(float(x)) / Fraction(float(y)))
        e = math.frexp(float(q))[1]
        s = q * Fraction(2) ** (54 - e)                 # in [2^53, 2^54): the midpoints of doubles are the odd integers
        near = round(s)
        assert near % 2 == 1 and 0 < abs(s - near) <= Fraction(1, 2 ** 48), "not within 2^-102 of a rounding midpoint"
    for fn in (R.fast_div_random, R.fast_div_structured):
        a, b = fn()
        q = np.abs(a / b)
        assert np.all(np.isfinite(b) & (np.abs(b) >= tiny) & ((a == 0) | (q >= tiny)) & np.isfinite(q))
    for fn in (R.fast_div_random, R.fast_div_hard):
        assert R.fast_div_exact_range(*fn()).all()
    a, b = R.fast_div_structured()
    assert 0 < (~R.fast_div_exact_range(a, b) & (a != 0)).sum() < a.size // 4
    a, b = R.fast_div_random()
    assert a.size > 50000 and np.ptp(np.log2(np.abs(a / b))) > 1200
    a, b = R.fast_div_structured()
    assert np.any(a == b) and np.any(a == -b) and np.any(a == 0) and np.any(np.abs(b) == 2.0 ** 1023) and np.any(np.abs(b) == 2.0 ** -1022)


def test_step_root_of_the_port():
    """The port's step_root against x^(-1/(ord+1)) at 60 digits: 2 ulp for orders 1 and 3; order 2 stays below 1.0e-7 and its worst case,
    at a reduced argument just below 4, is the documented 9.33e-8 (not the 1e-13 the comments used to claim)."""
    fx = R.load_fixture("prim_step_root")
    got = np.array([cpu_port.step_root(x, o) for x, o in zip(fx["x"], fx["order"])])
    assert np.all(np.isfinite(got) & (got > 0))
    for o in (1, 3):
        assert np.max(R.ulp_diff(got[fx["order"] == o], fx["ref"][fx["order"] == o])) <= 2.0
    m = fx["order"] == 2
    rel = np.abs(got[m] - fx["ref"][m]) / fx["ref"][m]
    assert 9.2e-8 <= rel.max() <= 9.4e-8
    worst = fx["x"][m][np.argmax(rel)]
    mant, e = math.frexp(worst)
    assert mant == float(np.nextafter(1.0, 0.0)) and e % 3 == 2               # m = 4 (1 - 2^-53)
    es = {math.frexp(x)[1] for x in fx["x"]}
    assert set(range(-8, 9)) <= es


def test_lane_patterns_are_exact():
    v = R.lane_patterns()
    assert np.all(v == np.round(v))
    for w in (2, 4, 8, 16, 32, 64):
        s = np.abs(v).reshape(v.shape[0], -1, w).sum(axis=2)
        assert np.all(s < 2.0 ** 53)
    # the powers of two name their lanes: all 64 group sums of the one-hot rows differ from each other and from zero
    assert len({float(r.sum()) for r in v[:64]}) == 64


def test_wave_inputs():
    tab, t, off, ln, hint = R.pwl_inputs()
    val, idx = R.pwl_reference(tab, t, off, ln)
    assert set(ln) >= {1, 2} and np.all((idx >= 1) & (idx <= ln + 1))
    for n in set(ln):
        assert set(hint[ln == n]) == set(range(-1, n + 2))
    assert any(len(set(ts)) < len(ts) for ts, _ in R.pwl_cases()) and any(a == b for _, ys in R.pwl_cases() for a, b in zip(ys, ys[1:]))
    x = R.pulse_inputs()
    assert np.any((x[3] == 0) & (x[4] == 0)) and np.any(x[6] == 0) and np.any(x[7] < x[2]) and np.any(x[7] > 1e5 * x[6])
    fx = R.load_fixture("prim_sind")
    assert np.max(np.abs(np.array([D.sind(d) for d in fx["deg"]]) - fx["ref"])) <= 8 * 2.0 ** -53
    assert {90.0, -90.0, 180.0, -180.0, 270.0, -270.0, 1e6, 30.0, 150.0} <= set(fx["deg"])


def test_bsrc_programs():
    progs = R.bsrc_programs()
    fx = R.load_fixture("prim_bsrc")
    flt = R.bsrc_float_reference()
    ops_seen, depth = set(), {}
    for i, (name, g, p) in enumerate(progs):
        _, deep, _ = R.bsrc_eval(p, list(R.BSRC_U), R.BSRC_T, {k: (lambda *a: 1.0) for k in ("pow", "exp", "log", "sqrt", "tanh", "sin", "cos")})
        depth[name] = deep
        assert deep <= R.BSRC_MAX_STACK
        R.check_close(flt[i], fx["ref"][i], fx["scale"][i], R.bsrc_k(p) - sum(v for k, v in R.BOP_SPEC.items() if k in p) + len(p), name)
        j, here = 0, set()
        while j < len(p):
            op = int(p[j]); here.add(op); j += 1 + {R.CONST: 1, R.V: 2}.get(op, 0)
            if op == R.V:
                assert -1 <= p[j - 2] < len(R.BSRC_U) and -1 <= p[j - 1] < len(R.BSRC_U)
        ops_seen |= here
        if name == "mixed":
            assert here == {0, 1, 2, 10, 11, 12, 13, 14, 15, 16, 20, 21, 22, 23, 24, 25, 26, 27}
    assert depth["full_stack"] == R.BSRC_MAX_STACK
    assert {"v_gnd_n", "v_gnd_p"} <= set(depth)
