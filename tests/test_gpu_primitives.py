"""The device-side numeric primitives, one helper at a time, against exact or multiprecision references (tests/prim_ref.py).

Each helper of tran_ctrl.hpp, devices.hpp and va_runtime.hpp runs inside a trivial kernel of the probe library
(csrc/probe/prim_probe.hip, tests/prim_probe.py).  References: numpy's correctly rounded division, the CPU port's exported step_root,
exact integer lane patterns and math.fsum, exact rational arithmetic for the dual rules, mpmath fixtures (tests/golden/prim_*.npz) for the
elementary functions, and the oracle's limiters and waves.  Tolerances are prim_ref.K, derived there; every test prints the figures it
asserts on."""
import functools
import math

import numpy as np
import pytest

from oracle import cpu_port
from tests import prim_probe as P
from tests import prim_ref as R

pytestmark = pytest.mark.gpu
EPS = R.EPS


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.int64)


def assert_bits_equal(got, ref, what):
    """Bit for bit, NaN payloads aside."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    same = (bits(got) == bits(ref)) | (np.isnan(got) & np.isnan(ref))
    j = np.flatnonzero(~same.ravel())
    assert j.size == 0, "%s: %d of %d differ, first at %d: got %r, want %r" % (what, j.size, same.size, j[0], got.ravel()[j[0]], ref.ravel()[j[0]])


# ------------------------------------------------------------------------------------------------------------------------------------------
# a. fast_div
# ------------------------------------------------------------------------------------------------------------------------------------------
def _fast_div(a, b):
    return P.run("fast_div", [a, b], block=256)[0][0]


@pytest.mark.parametrize("which", ["random", "structured", "hard"])
def test_fast_div_is_the_correctly_rounded_quotient(which):
    """In contract (b finite, non-zero, normal; the quotient normal or a = 0): bit for bit numpy's a / b, which is the exact quotient
    rounded once.  `hard`: 1e5 quotients within ~2^-106 relative of a rounding midpoint -- none is missed.

    The structured set found the three places where fast_div is NOT IEEE division (fast_div itself stays as it is: the hot path):
      * -0 / b with b > 0 gives +0 (the residual step adds +0 * r to the quotient -0); every other zero has IEEE's sign;
      * |b| > 2^1022: the reciprocal is subnormal and has lost bits -- 2^1023 / (2^1023 (1 - 2^-53)) comes out one ulp low;
      * |a| < 2^-969: the residual a - b q is subnormal -- 0x1.14ea81bb5ac2ep-1022 / -0x1.8p-1022 comes out one ulp off.
    So: bit equality for a != 0 inside prim_ref.fast_div_exact_range (all of `random` and `hard` lies there), at most one ulp outside
    it, and for a = 0 a zero with IEEE's sign except in the first case."""
    a, b = {"random": R.fast_div_random, "structured": R.fast_div_structured, "hard": R.fast_div_hard}[which]()
    got, ref = _fast_div(a, b), a / b
    exact = R.fast_div_exact_range(a, b)
    assert which == "structured" or exact.all()
    ne = bits(got) != bits(ref)
    print("\nfast_div %s: %d pairs, %d differ from a / b (%d of them zeros, %d outside the exact range), worst %.3g ulp" % (
        which, a.size, int(ne.sum()), int((ne & (a == 0)).sum()), int((ne & ~exact & (a != 0)).sum()), float(np.max(R.ulp_diff(got, ref), initial=0.0))))
    assert_bits_equal(got[exact], ref[exact], "fast_div " + which)
    edge = ~exact & (a != 0)
    assert np.all(R.ulp_diff(got[edge], ref[edge]) <= 1.0), "fast_div %s: beyond one ulp outside the exact range" % which
    zero = a == 0
    lost = zero & np.signbit(a) & (b > 0)                      # -0 / b, b > 0
    assert np.all(got[zero] == 0.0)
    assert_bits_equal(got[zero & ~lost], ref[zero & ~lost], "fast_div %s: sign of a zero quotient" % which)
    assert not np.signbit(got[lost]).any()


def test_fast_div_out_of_contract_is_never_a_finite_number():
    """b in {+-0, +-inf, NaN} or a non-finite: the isfinite guards downstream must still see a singular pivot."""
    a, b = R.fast_div_out_of_contract()
    got = _fast_div(a, b)
    bad = np.isfinite(got)
    assert not bad.any(), "finite results: a %r b %r -> %r" % (a[bad], b[bad], got[bad])


# ------------------------------------------------------------------------------------------------------------------------------------------
# b. step_root
# ------------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _step_root():
    fx = R.load_fixture("prim_step_root")
    got = P.run("step_root", [fx["x"]], [fx["order"]])[0][0]
    return fx, got


def test_step_root_equals_the_port_bit_for_bit():
    fx, got = _step_root()
    port = np.array([cpu_port.step_root(x, o) for x, o in zip(fx["x"], fx["order"])])
    assert_bits_equal(got, port, "step_root vs cadnip_port_step_root")


def test_step_root_accuracy():
    """Against x^(-1/(ord+1)) at 60 digits.  Orders 1 and 3 are square roots and exact divisions: 2 ulp.  Order 2 is four Newton steps from
    a linear start, whose error reaches 9.33e-8 as the reduced argument m approaches 4 from below: 1.0e-7 relative."""
    fx, got = _step_root()
    assert np.all(np.isfinite(got) & (got > 0.0))
    for o in (1, 2, 3):
        m = fx["order"] == o
        ulp = float(np.max(R.ulp_diff(got[m], fx["ref"][m])))
        rel = float(np.max(np.abs(got[m] - fx["ref"][m]) / fx["ref"][m]))
        print("\nstep_root order %d: %d arguments, worst %.3g ulp, %.3g relative" % (o, int(m.sum()), ulp, rel))
        if o == 2:
            assert rel <= 1.0e-7
        else:
            assert ulp <= 2.0


# ------------------------------------------------------------------------------------------------------------------------------------------
# c. cross-lane helpers
# ------------------------------------------------------------------------------------------------------------------------------------------
LANE = np.arange(64)
# rows of probe_lane_sums: name, group width (None: not a sum)
LANE_ROWS = [("group_sum16 w=1", 1), ("group_sum16 w=2", 2), ("group_sum16 w=4", 4), ("group_sum16 w=8", 8), ("group_sum16 w=16", 16),
             ("wave_sum", 64), ("uniform_f64", None), ("dpp_pair_swap", None), ("va_group_sum<16>", 16), ("va_group_sum<32>", 32)]


def _lane_sums(v):
    """v [waves, 64] -> [10, waves, 64]"""
    return P.run("lane_sums", [v.ravel()])[0].reshape(10, -1, 64)


def test_lane_helpers_exact_patterns():
    """One-hot in every lane, powers of two that name the contributing lanes, lane + 1: every sum is an integer below 2^53, so the
    expected result is exact whatever the order -- no tolerance."""
    v = R.lane_patterns()
    got = _lane_sums(v)
    for k, (name, w) in enumerate(LANE_ROWS):
        if w is not None:
            ref = np.repeat(v.reshape(v.shape[0], -1, w).sum(axis=2), w, axis=1)
        elif name == "uniform_f64":
            ref = np.repeat(v[:, :1], 64, axis=1)
        else:
            ref = v[:, LANE ^ 1]
        assert_bits_equal(got[k], ref, name)


def test_lane_sums_random_within_gamma_and_identical_in_every_lane():
    """Mixed signs over 40 decades against math.fsum: |err| <= gamma_(w-1) sum|v|; all lanes of a group hold the same bits (the
    controller's decisions depend on that)."""
    v = R.lane_random()
    got = _lane_sums(v)
    for k, (name, w) in enumerate(LANE_ROWS):
        if w is None or w == 1:
            continue
        err = np.abs(got[k] - R.group_fsum(v, w))
        bound = R.gamma(w - 1) * R.group_abs(v, w)
        print("\n%s: worst error / (gamma_%d sum|v|) = %.3g" % (name, w - 1, float(np.max(err / bound))))
        assert np.all(err <= bound), name
        g = bits(got[k]).reshape(-1, w)
        assert np.all(g == g[:, :1]), name + ": lanes of one group differ"
    assert_bits_equal(got[0], v, "group_sum16 w=1")


@pytest.mark.parametrize("special", [np.inf, -np.inf, np.nan])
def test_lane_sums_nonfinite_reaches_its_group_only(special):
    base = R.lane_random(rows=1, seed=32)
    v = np.repeat(base, 64, axis=0)
    v[LANE, LANE] = special                                  # row j: the special value in lane j
    got, clean = _lane_sums(v), _lane_sums(base)
    for k, (name, w) in enumerate(LANE_ROWS):
        if w is None:
            continue
        hit = (LANE[None, :] // w) == (LANE[:, None] // w)   # [row j, lane]: lane in the group of j
        want = np.where(hit, special, np.repeat(clean[k], 64, axis=0))
        assert_bits_equal(np.where(np.isnan(want), np.nan, got[k]), want, name)
        assert np.all(np.isnan(got[k][hit])) if np.isnan(special) else np.all(got[k][hit] == special), name


def test_readlane_every_lane():
    v = np.concatenate([R.lane_random(rows=2, seed=33), (LANE + 1.0)[None, :]])
    got = P.run("readlane", [v.ravel()])[0].reshape(64, -1, 64)
    for l in range(64):
        assert_bits_equal(got[l], np.repeat(v[:, l:l + 1], 64, axis=1), "readlane_f64(v, %d)" % l)


def test_va_ddx_tl_every_direction():
    """va_ddx_tl<LANES>(a, k) is the partial held by lane k of the caller's group of LANES lanes."""
    v = np.concatenate([R.lane_random(rows=2, seed=34), (LANE + 1.0)[None, :]])
    got = P.run("ddx_tl", [v.ravel()])[0].reshape(49, -1, 64)
    for k in range(16):
        assert_bits_equal(got[k], v[:, (LANE & ~15) + k], "va_ddx_tl<16>(a, %d)" % k)
    for k in range(32):
        assert_bits_equal(got[16 + k], v[:, (LANE & ~31) + k], "va_ddx_tl<32>(a, %d)" % k)
    assert np.all(got[48] == 0.0)


@pytest.mark.parametrize("nt", [64, 256])
def test_group_reductions(nt):
    """grp_sum / grp_any / grp_reduce3 over GlobalVecsT<NT>, one group per workgroup, nt + 2 workgroups in one launch: a leak between
    blocks would show.  Block b < nt: one-hot (worth b + 1) in thread b, flag in thread b of the even blocks only; block nt: random
    values; block nt + 1: a NaN in one thread."""
    nb = nt + 2
    rng = np.random.default_rng(35)
    s1, s2 = np.zeros((nb, nt)), np.tile(np.arange(nt) + 1.0, (nb, 1))
    f1, f2 = np.zeros((nb, nt), dtype=np.int32), np.zeros((nb, nt), dtype=np.int32)
    idx = np.arange(nt)
    s1[idx, idx] = idx + 1.0
    f1[idx[::2], idx[::2]] = 1
    f2[idx[1::2], idx[1::2]] = 7
    s1[nt] = np.where(rng.random(nt) < 0.5, -1.0, 1.0) * 10.0 ** rng.uniform(-20, 20, nt)
    s2[nt] = s1[nt][::-1]
    s1[nt + 1] = 1.0
    s1[nt + 1, nt // 2 + 3] = np.nan
    out, iout = P.run("grp", [s1.ravel(), s2.ravel()], [f1.ravel(), f2.ravel()], block=nt)
    out, iout = out.reshape(3, nb, nt), iout.reshape(2, nb, nt)
    for k in range(3):
        assert np.all((bits(out[k]) == bits(out[k][:, :1])) | np.isnan(out[k])), "threads of one group differ"
    # exact blocks
    want1 = np.concatenate([idx + 1.0])
    assert_bits_equal(out[0][:nt, 0], want1, "grp_sum one-hot")
    assert_bits_equal(out[1][:nt, 0], want1, "grp_reduce3 s1 one-hot")
    assert_bits_equal(out[2][:nt, 0], np.full(nt, nt * (nt + 1) / 2.0), "grp_reduce3 s2 = sum(lane + 1)")
    assert np.array_equal(iout[0][:nt, 0] != 0, idx % 2 == 0) and np.all((iout[0] != 0) == (iout[0][:, :1] != 0)), "grp_any"
    assert np.array_equal(iout[1][:nt, 0] != 0, idx % 2 == 1) and np.all((iout[1] != 0) == (iout[1][:, :1] != 0)), "grp_reduce3 flag"
    # random block
    bound = R.gamma(nt - 1) * np.sum(np.abs(s1[nt]))
    for k, src in ((0, s1[nt]), (1, s1[nt]), (2, s2[nt])):
        err = abs(out[k][nt, 0] - math.fsum(src))
        print("\nNT=%d reduction %d: error / (gamma sum|v|) = %.3g" % (nt, k, err / bound))
        assert err <= bound
    # the NaN stays in its block
    assert np.all(np.isnan(out[0][nt + 1])) and np.all(np.isnan(out[1][nt + 1])) and np.all(np.isfinite(out[2][nt + 1]))
    assert np.all(np.isfinite(out[:, :nt + 1]))
    assert np.all(iout[:, nt:] == 0)


# ------------------------------------------------------------------------------------------------------------------------------------------
# d. Dual<N> and the va_* functions
# ------------------------------------------------------------------------------------------------------------------------------------------
def _dual_rows(a, width):
    """[n, 4] -> the probe's rows of a Dual<width>: value, width partials."""
    return [a[:, k] for k in range(1 + width)]


@functools.lru_cache(maxsize=None)
def _dual_exact():
    a, b = R.dual_op_inputs()
    return (a, b) + R.dual_ops_exact(a, b)


@pytest.mark.parametrize("width", [1, 3])
def test_dual_operators(width):
    """The four operators in every dual / double combination and unary minus against exact rational arithmetic: K = 4 on the sum of the
    magnitudes of each rule's terms."""
    a, b, ref, sc = _dual_exact()
    W = 1 + width
    out = P.run("dual_ops%d" % width, _dual_rows(a, width) + _dual_rows(b, width))[0].reshape(len(R.DUAL_OPS), W, -1)
    for k, name in enumerate(R.DUAL_OPS):
        worst = R.check_close(out[k].T, ref[k][:, :W], sc[k][:, :W], R.K["arith"], "Dual<%d> %s" % (width, name))
        print("\nDual<%d> %-4s worst %.3g x 2^-52 scale (K = %d)" % (width, name, worst, R.K["arith"]))


@pytest.mark.parametrize("width", [1, 3])
def test_dual_operators_singular_operands(width):
    """Zero, infinite and NaN operands: the inf / NaN / sign pattern of the rules evaluated in IEEE doubles."""
    a, b = R.dual_singular_inputs()
    ref = R.dual_ops_ieee(a, b)
    W = 1 + width
    out = P.run("dual_ops%d" % width, _dual_rows(a, width) + _dual_rows(b, width))[0].reshape(len(R.DUAL_OPS), W, -1)
    for k, name in enumerate(R.DUAL_OPS):
        R.check_close(out[k].T, ref[k][:, :W], np.abs(ref[k][:, :W]), R.K["arith"], "Dual<%d> %s (singular)" % (width, name))


@pytest.mark.parametrize("width", [1, 3])
def test_va_unary_functions(width):
    """dsqrt / dexp / dlog and every VA_UNARY function over its domain and at its edges: value (dual and double overload) and every
    partial p_i f'(x) against mpmath, K and scale per function (prim_ref.K)."""
    fx = R.load_fixture("prim_unary")
    n = fx["x"].size
    p = R.unary_partials(n, width)
    out = P.run("va_unary%d" % width, [fx["x"]] + [p[:, k] for k in range(width)], [fx["code"], np.zeros(n, dtype=np.int32)])[0]
    with np.errstate(all="ignore"):
        for name, (code, kname, _, _) in R.UNARY.items():
            m = fx["code"] == code
            wf = R.check_close(out[0][m], fx["f"][m], fx["sf"][m], R.K[kname + ".f"], "%s value" % name)
            R.check_close(out[1 + width][m], fx["f"][m], fx["sf"][m], R.K[kname + ".f"], "%s value (double overload)" % name)
            wd = 0.0
            for k in range(width):
                pk = p[m, k]
                wd = max(wd, R.check_close(out[1 + k][m], pk * fx["df"][m], np.abs(pk) * fx["sdf"][m], R.K[kname + ".d"], "%s partial %d" % (name, k)))
            print("\nDual<%d> %-7s %3d points: value %.3g (K = %d), partials %.3g (K = %d)" % (width, name, int(m.sum()), wf, R.K[kname + ".f"], wd, R.K[kname + ".d"]))


@pytest.mark.parametrize("width", [1, 3])
def test_va_exact_unary_functions(width):
    """va_abs (at +-0 and negatives), unary minus, va_floor / va_ceil / va_int (negatives, exact integers) and va_ddx: no rounding at all."""
    x = R.unary_exact_inputs()
    n = x.size
    p = R.unary_partials(n, width, seed=52)
    for name, (code, fn) in R.UNARY_EXACT.items():
        out = P.run("va_unary%d" % width, [x] + [p[:, k] for k in range(width)], [np.full(n, code), np.zeros(n)])[0]
        assert np.array_equal(out[0], fn(x)) and np.array_equal(out[1 + width], fn(x)), name
        if name == "abs":
            assert_bits_equal(out[1 + width], np.abs(x), "va_abs(double)")
            want = np.where((x >= 0.0)[:, None], p, -p)          # a.v >= 0 keeps a (so does -0.0, as the oracle's dabs)
        elif name == "neg":
            want = -p
        else:
            want = np.zeros_like(p)                              # piecewise constant: plain numbers
        assert_bits_equal(out[1:1 + width].T + 0.0, want + 0.0, name + " partials")
    for k in range(width):
        out = P.run("va_unary%d" % width, [x] + [p[:, j] for j in range(width)], [np.full(n, 25), np.full(n, k)])[0]
        assert_bits_equal(out[0], p[:, k], "va_ddx(a, %d)" % k)
        assert np.all(out[1 + width] == 0.0), "va_ddx(double)"


def _binary_partials(n, width):
    return R.unary_partials(n, width, seed=53), R.unary_partials(n, width, seed=54)[:, ::-1].copy()


@pytest.mark.parametrize("width", [1, 3])
def test_va_pow_atan2_hypot(width):
    """All four overloads of va_pow, va_atan2 and va_hypot against mpmath.  pow: the shortcut exponents within 2 ulp, their neighbouring
    doubles (general path) and general exponents within pow's bound, a = 0 (the b a^(b-1) branch of va_dpow), a negative base with an
    integer exponent carried in a dual whose partials are zero (no logarithm may be taken), live exponent partials."""
    fx = R.load_fixture("prim_binary")
    n = fx["a"].size
    pa, pb = _binary_partials(n, width)
    kind, fn = fx["kind"], fx["fn"]
    kda = np.array([R.K["pow.da"], R.K["atan2.d"], R.K["hypot.d"]], dtype=float)[fn]
    kdb = np.array([R.K["pow.db"], R.K["atan2.d"], R.K["hypot.d"]], dtype=float)[fn]
    with np.errstate(all="ignore"):
        for ov, oname in enumerate(("dual, dual", "dual, double", "double, dual", "double, double")):
            qa = pa if ov in (0, 1) else np.zeros_like(pa)
            qb = pb if ov in (0, 2) else np.zeros_like(pb)
            qb = np.where((kind == 2)[:, None] | (kind == 3)[:, None], 0.0, qb) if ov == 0 else qb
            live = np.ones(n, dtype=bool) if ov in (0, 1, 3) else (kind != 2)      # pow(double < 0, dual): f log(a) is NaN by definition, not a case
            rows = _dual_rows(np.column_stack([fx["a"], qa]), width) + _dual_rows(np.column_stack([fx["b"], qb]), width)
            out = P.run("va_binary%d" % width, rows, [fn * 4 + ov, np.zeros(n, dtype=np.int32)])[0]
            # values: K on |f|; the shortcut exponents of pow within 2 ulp
            for f_id, nm in enumerate(("pow", "atan2", "hypot")):
                m = live & (fn == f_id)
                w = R.check_close(out[0][m], fx["f"][m], np.abs(fx["f"][m]), R.K[nm + ".f"], "va_%s value (%s)" % (nm, oname))
                print("\nDual<%d> va_%s(%s): value worst %.3g x 2^-52 |f| (K = %d)" % (width, nm, oname, w, R.K[nm + ".f"]))
            sc = live & (kind == 1)
            ulp = R.ulp_diff(out[0][sc], fx["f"][sc])
            print("pow shortcuts (%s): worst %.3g ulp" % (oname, float(np.max(ulp))))
            assert np.all(ulp <= 2.0), "va_pow shortcut exponents beyond 2 ulp: a %r b %r" % (fx["a"][sc][ulp > 2], fx["b"][sc][ulp > 2])
            if ov == 3:
                assert np.all(out[1:] == 0.0)
                continue
            # partials: a.p da + b.p db; the dual-dual pow skips the exponent term where its partial is zero
            m = live & (kind != 4)
            for k in range(width):
                ta = qa[:, k] * fx["da"] if ov in (0, 1) else np.zeros(n)
                if ov == 1:
                    tb = np.zeros(n)
                elif ov == 0:
                    tb = np.where((qb[:, k] == 0.0) & (fn == 0), 0.0, qb[:, k] * fx["db"])
                else:
                    tb = qb[:, k] * fx["db"]
                ref = ta + tb
                scale = np.abs(ta) + np.abs(tb)
                kk = np.maximum(np.where(ta != 0, kda, 0.0), np.where(tb != 0, kdb, 0.0))
                kk = np.where(kk == 0, R.ARITH, kk)
                fin = np.isfinite(ref) & m
                R.check_close(out[1 + k][m & ~fin], ref[m & ~fin], 0.0, 1.0, "partial %d pattern (%s)" % (k, oname))
                err, tol = np.abs(out[1 + k][fin] - ref[fin]), kk[fin] * EPS * scale[fin]
                j = np.flatnonzero(err > tol)
                assert j.size == 0, "partial %d (%s): fn %r a %r b %r got %r ref %r" % (k, oname, fn[fin][j], fx["a"][fin][j], fx["b"][fin][j], out[1 + k][fin][j], ref[fin][j])
            # a negative base with an integer exponent: finite and correct
            nb = kind == 2
            assert np.all(np.isfinite(out[:, nb & live]))


@pytest.mark.parametrize("width", [1, 3])
def test_va_min_max_select_the_first_operand_on_ties(width):
    """All six dual overloads and the double pair: the selected operand's value (to the sign of zero) and partials; on a tie the first
    operand wins, as ForwardDiff's."""
    av = np.array([1.0, 2.0, 1.0, -0.0, 0.0, -3.0, 5.5, -1e300, 0.1, 1e-300])
    bv = np.array([2.0, 1.0, 1.0, 0.0, -0.0, -3.0, 5.5, -1e300, np.nextafter(0.1, 1.0), -1e-300])
    n = av.size
    pa, pb = _binary_partials(n, width)
    pb = pb + 10.0                                           # no partial of b equals one of a
    zero = np.zeros_like(pa)
    for f_id, (nm, take_b) in ((3, ("max", bv > av)), (4, ("min", bv < av))):
        for ov in range(4):
            qa, qb = (pa if ov in (0, 1) else zero), (pb if ov in (0, 2) else zero)
            rows = _dual_rows(np.column_stack([av, pa]), width) + _dual_rows(np.column_stack([bv, pb]), width)
            out = P.run("va_binary%d" % width, rows, [np.full(n, f_id * 4 + ov), np.zeros(n)])[0]
            assert_bits_equal(out[0], np.where(take_b, bv, av), "va_%s overload %d value" % (nm, ov))
            want = np.where(take_b[:, None], qb, qa) if ov < 3 else zero
            assert_bits_equal(out[1:].T, want, "va_%s overload %d partials" % (nm, ov))


@pytest.mark.parametrize("width", [1, 3])
def test_va_site(width):
    """va_site(probe, w, slot): value w, the probe's partials kept, a unit partial in the site's own slot."""
    n = 12
    pa, _ = _binary_partials(n, width)
    v, w = np.linspace(-1, 1, n), np.linspace(3, 4, n)
    for slot in range(width):
        rows = _dual_rows(np.column_stack([v, pa]), width) + _dual_rows(np.column_stack([w, pa * 0]), width)
        out = P.run("va_binary%d" % width, rows, [np.full(n, 20), np.full(n, slot)])[0]
        want = pa.copy()
        want[:, slot] = 1.0
        assert_bits_equal(out[0], w, "va_site value")
        assert_bits_equal(out[1:].T, want, "va_site partials")


# ------------------------------------------------------------------------------------------------------------------------------------------
# e. limiters
# ------------------------------------------------------------------------------------------------------------------------------------------
def test_limiters_against_the_oracle():
    """pnjlim against oracle.devices_ref.pnjlim, m1_pnjlim / m1_fetlim / m1_limvds against the DEV* functions of oracle/va_mos1_ref.py, on
    the grid -5 .. 10 V and on every comparison's boundary (prim_ref.limiter_inputs; coverage of the return paths is checked on the CPU).
    Results without a logarithm: bit for bit.  With one: K on |vold| + vt |log term| (both sides hand log the same double)."""
    vn, vo, _ = R.limiter_inputs()
    ref, path, scale = R.limiter_reference(vn, vo)
    n = vn.size
    got = P.run("limiters", [vn, vo, np.full(n, R.VT), np.full(n, R.VCRIT)])[0]
    # m1_fetlim takes vto where the junction limiters take vcrit
    got[2] = P.run("limiters", [vn, vo, np.full(n, R.VT), np.full(n, R.VTO)])[0][2]
    for r, name in enumerate(("pnjlim", "m1_pnjlim")):
        logp = path[r] <= 2
        assert_bits_equal(got[r][~logp], ref[r][~logp], name + " (paths without a logarithm)")
        worst = R.check_close(got[r][logp], ref[r][logp], scale[r][logp], R.K["pnjlim"], name + " (logarithmic paths)")
        print("\n%s: %d points on logarithmic paths, worst %.3g x 2^-52 scale (K = %d); %d bit-equal" % (name, int(logp.sum()), worst, R.K["pnjlim"], int((~logp).sum())))
    assert_bits_equal(got[2], ref[2], "m1_fetlim")
    assert_bits_equal(got[3], ref[3], "m1_limvds")


# ------------------------------------------------------------------------------------------------------------------------------------------
# f. sources and the behavioural program
# ------------------------------------------------------------------------------------------------------------------------------------------
def test_pwl_at_time_with_every_hint():
    """Before, after, on and between the points of every table (n = 1, n = 2, duplicated points, flat segments), without a hint and with
    every hint 0 .. n + 1, stale and out-of-range ones included: the value is the oracle's bit for bit whatever the hint, and the hint
    afterwards is the searched index."""
    tab, t, off, ln, hint = R.pwl_inputs()
    assert np.all(off + 2 * ln <= tab.size) and np.all(ln >= 1)
    val, idx = R.pwl_reference(tab, t, off, ln)
    out, iout = P.run("pwl", [t], [off, ln, hint], tab=tab)
    ne = bits(out[0]) != bits(val)
    print("\npwl_at_time: %d calls, %d differ from the oracle, worst %.3g ulp" % (t.size, int(ne.sum()), float(np.max(R.ulp_diff(out[0][val != 0], val[val != 0])))))
    assert_bits_equal(out[0], val, "pwl_at_time value")
    assert np.array_equal(iout[0], np.where(hint < 0, -1, idx)), "hint written back"


def test_pulse_at_time():
    x = R.pulse_inputs()
    ref = R.pulse_reference(x)
    got = P.run("pulse", list(x))[0][0]
    ne = bits(got) != bits(ref)
    print("\npulse_at_time: %d calls, %d differ from the oracle, worst %.3g ulp" % (ref.size, int(ne.sum()), float(np.max(R.ulp_diff(got[ref != 0], ref[ref != 0])))))
    assert_bits_equal(got, ref, "pulse_at_time")


def test_sind_deg():
    """Against sin(pi r / 180) at 60 digits: absolute error <= 8 * 2^-53, exact at the multiples of 90 degrees."""
    fx = R.load_fixture("prim_sind")
    got = P.run("sind", [fx["deg"]])[0][0]
    err = np.abs(got - fx["ref"])
    print("\nsind_deg: worst absolute error %.3g x 2^-53" % float(np.max(err) / 2.0 ** -53))
    assert np.all(err <= 8 * 2.0 ** -53)
    m90 = np.fmod(fx["deg"], 90.0) == 0.0
    assert m90.sum() >= 20
    assert np.array_equal(got[m90], np.round(fx["ref"][m90])) and np.all(np.abs(np.round(fx["ref"][m90]) - fx["ref"][m90]) < 1e-50)


def test_source_value():
    """Every kind of wave in every analysis mode, the damped sine on both sides of its delay, with and without a segment hint."""
    tab, rows = R.source_inputs()
    ref, sc = R.source_reference(tab, rows)
    ints = [rows[:, 3].astype(np.int32), rows[:, 4].astype(np.int32), rows[:, 5].astype(np.int32), rows[:, 6].astype(np.int32)]
    need = np.where(ints[0] == 1, 2 * ints[2], np.where(ints[0] == 2, 7, np.where(ints[0] == 3, 6, 0)))
    assert np.all(ints[1] + need <= tab.size)
    sine = (ints[0] == 3) & (ints[3] != 0)
    assert np.any(sine & (rows[:, 0] < 2e-9)) and np.any(sine & (rows[:, 0] > 2e-9))
    for hint in (-1, 0, 2, 3):
        got = P.run("source_value", [rows[:, 0], rows[:, 1], rows[:, 2]], ints + [np.full(len(rows), hint)], tab=tab)[0][0]
        assert_bits_equal(got[~sine], ref[~sine], "source_value (dc, pwl, pulse; hint %d)" % hint)
        worst = R.check_close(got[sine], ref[sine], sc[sine], R.K["sine"], "source_value (sine)")
    print("\nsource_value: sine worst %.3g x 2^-52 scale (K = %d)" % (worst, R.K["sine"]))


def test_bsrc_value():
    """One program per opcode, the probe with either node grounded, the full stack depth, one program mixing every opcode.  Programs of
    plain arithmetic: bit for bit the Python evaluation.  Programs that call the math library: mpmath, K = the calls' bounds + 4."""
    progs = R.bsrc_programs()
    fx = R.load_fixture("prim_bsrc")
    flt = R.bsrc_float_reference()
    tab, off, ln = list(R.BSRC_U), [], []
    for _, _, p in progs:
        off.append(len(tab)); ln.append(len(p)); tab += [float(x) for x in p]
        deep = R.bsrc_eval(p, list(R.BSRC_U), R.BSRC_T, {k: (lambda *a: 1.0) for k in ("pow", "exp", "log", "sqrt", "tanh", "sin", "cos")})[1]
        assert deep <= R.BSRC_MAX_STACK
    n = len(progs)
    got = P.run("bsrc", [[g for _, g, _ in progs], np.full(n, R.BSRC_T)], [off, ln, np.zeros(n)], tab=tab)[0][0]
    for i, (name, g, p) in enumerate(progs):
        if R.bsrc_uses_library(p):
            w = R.check_close(got[i], fx["ref"][i], fx["scale"][i], R.bsrc_k(p), "bsrc program " + name)
            print("bsrc %-10s worst %.3g x 2^-52 scale (K = %d)" % (name, w, R.bsrc_k(p)))
        else:
            assert_bits_equal(got[i:i + 1], flt[i:i + 1], "bsrc program " + name)
