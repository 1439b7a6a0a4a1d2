"""k_ac_sens / k_ac_sens_hbm (csrc/ac_lu.hip) through the C ABI (cadnip_ac_sens): the response and K parameter derivatives per factorisation.  The
solves inside are the very per-column functions of k_ac_lu and k_ac_adj, so x, y, lambda and the backward errors are held against
cadnip_ac_solve / cadnip_ac_adjoint TO THE BIT -- whose results tests/test_gpu_ac_lu.py and tests/test_gpu_ac_adjoint.py pin against the CPU
references -- and only the bilinear forms s need a bound of their own: d_s of tests/sens_ref.py against the direct form in extended precision
on the handle's own get_GCb arrays.  Systems: the Butterworth filter (three copies of its one point: dA = 0, only the db path runs) and the
flip-flop (its three corners: base 1, the outer two as plus and minus) of ac_ref.CASES, the cached DC points restamped on handles of their
own -- no DC solve; F = 3: omega = 0, the middle and the end of the case's grid.  Comparisons are on the 64-bit patterns."""
import ctypes as C

import numpy as np
import pytest

import cadnip_jl_amd as cj
from cadnip_jl_amd import api, hip
from tests import ac_ref as R
from tests import circuits as tc
from tests import noise_ref as N
from tests import sens_ref as SR
from tests import test_gpu_ac_lu as T
from tests.test_gpu_ac_multi import same, LDS_BUDGET

pytestmark = pytest.mark.gpu
GMIN = T.GMIN
EPS = R.EPS


class Sens:
    def __init__(self, name):
        c = self.c = T.case(name)
        mk, base, pts, _ = R.CASES[name]
        three = pts if len(pts) == 3 else [{}, {}, {}]
        src = [0, 1, 2] if len(pts) == 3 else [0, 0, 0]
        self.sim = api.BatchSimulator(api.MNACircuit(c.circ, dict(base), api.MNASpec(mode="dcop")), three)
        self.st, self.h, self.B, self.n = self.sim.st, self.sim.h, 3, c.st.n
        self.h.set_spec(mode="dcop")
        self.h.rebuild(c.u[src], 0.0)
        G, Cm, _, _ = self.h.get_GCb()
        to_ref = np.asarray(c.st.to_ref_nz)
        self.G, self.Cm = G[:, to_ref], Cm[:, to_ref]                                  # CSR order
        assert np.array_equal(self.G, c.G[src]) and np.array_equal(self.Cm, c.C[src])  # the cached systems, to the bit
        self.h.analyze_values(c.sample_ref)
        self.om = np.array([0.0, c.om[len(c.om) // 2], c.om[-1]])
        self.F = 3
        self.base, self.plus, self.minus, self.scale = [1], [[2, 0]], [[0, 2]], [[0.7, 0.7]]
        self.bac = c.bac[src]
        self.e = N.e_out(name, c.st)
        self.pair = (N.output_index(name, c.st), -1)
        rng = np.random.default_rng(5)
        self.db = rng.standard_normal((1, 3, self.n)) + 1j * rng.standard_normal((1, 3, self.n))
        self.per = 16 * (self.h.lu_stats()["nnz_lu"] + 4 * self.n)
        self.got0 = self.run()

    def run(self, wpb=0, db="two", want_x=True, **kw):
        a = dict(base=self.base, plus=self.plus, minus=self.minus, scale=self.scale)
        a.update(kw)
        K, NB = np.asarray(a["plus"]).shape[-1], len(a["base"])
        bac = self.bac[np.asarray(a["base"], dtype=int)]
        return self.h.ac_sens(self.om, GMIN, a["base"], a["plus"], a["minus"], a["scale"], bac, self.e, self.pair,
                              np.broadcast_to(self.db[:, :K], (NB, K, self.n)) if isinstance(db, str) else db, wpb, want_x)   # one db for every base

    def is_default(self, got, ref=None):
        ref = self.got0 if ref is None else ref
        return all(same(got[i], ref[i]) for i in (0, 1, 2, 3)) and np.array_equal(got[4], ref[4])


_SENS = {}


def sens(name):
    if name not in _SENS:
        _SENS[name] = Sens(name)
    return _SENS[name]


# four bases (S = 12: more than one workgroup at every W, a tail at W = 8), every instance in every role
WIDE = dict(base=[1, 0, 2, 1], plus=[[2, 0], [1, 2], [0, 1], [0, 2]], minus=[[0, 2], [2, 1], [1, 0], [2, 1]], scale=[[0.7, 0.7], [1.0, -2.0], [0.25, 3.0], [1e3, 1e-3]])


@pytest.mark.parametrize("name", ["butterworth", "dff"])
def test_the_solves_are_ac_solve_and_ac_adjoint_to_the_bit(name):
    m = sens(name)
    y, s, x, berr, flags, info = m.got0
    assert y.shape == (1, m.F) and s.shape == (1, m.F, 2) and x.shape == (1, m.F, 2, m.n) and berr.shape == (1, m.F, 2) and flags.shape == (1, m.F, 2)
    xs, berrs, flagss, _ = m.h.ac_solve(m.om, GMIN, m.bac)
    ha, xa, berra, flagsa, _ = m.h.ac_adjoint(m.om, GMIN, m.e, [m.pair], want_x=True)
    assert same(x[0, :, 0], xs[1]) and same(y[0], xs[1, :, m.pair[0]]) and same(berr[0, :, 0], berrs[1])
    assert same(x[0, :, 1], xa[1]) and same(berr[0, :, 1], berra[1])
    assert np.array_equal(flags[0, :, 0] & 1, flagss[1] | flagsa[1]) and not (flags[(flags & 1) == 0] & 2).any()      # (the filter at omega = 0: a zero pivot)
    assert np.isfinite(x[0, 1:]).all()
    # every base of a list, the pair form, and the outputs without x
    yw, sw, xw, berrw, flagsw, _ = m.run(**WIDE)
    for a, b in enumerate(WIDE["base"]):
        assert same(xw[a, :, 0], xs[b]) and same(xw[a, :, 1], xa[b]) and same(berrw[a, :, 0], berrs[b]) and same(berrw[a, :, 1], berra[b]), a
    assert same(sw[0], s[0]) and same(yw[0], y[0])                # row 0 of the list is the default setup
    y2, s2, x2, berr2, flags2, _ = m.run(want_x=False)
    assert x2 is None and same(y2, y) and same(s2, s) and same(berr2, berr) and np.array_equal(flags2, flags)
    q = (m.pair[0] + 1) % m.n
    y3 = m.h.ac_sens(m.om, GMIN, m.base, m.plus, m.minus, m.scale, m.bac[1], m.e, (m.pair[0], q))[0]
    assert same(y3[0, 1:], xs[1, 1:, m.pair[0]] - xs[1, 1:, q])          # (omega = 0 may be a flagged system: NaNs, whose sign bits mean nothing)
    y4 = m.h.ac_sens(m.om, GMIN, m.base, m.plus, m.minus, m.scale, m.bac[1], m.e, (-1, q))[0]
    assert same(y4[0, 1:], 0.0 - xs[1, 1:, q])


@pytest.mark.parametrize("name", ["butterworth", "dff"])
def test_launch_paths_are_bit_identical(name):
    m = sens(name)
    for kw in ({}, WIDE):
        ref = m.run(**kw)
        S = len(kw.get("base", m.base)) * m.F
        assert ref[5]["wpb"] in (1, 2, 4, 8) and ref[5]["systems"] == S and ref[5]["lds_bytes"] == ref[5]["wpb"] * m.per
        assert m.h.ac_plan_info() == dict(memory="lds", n_waves=0, work_bytes=0, lds_bytes=ref[5]["wpb"] * m.per)
        for wpb in (1, 2, 4, 8):
            if wpb * m.per > LDS_BUDGET:                          # the flip-flop at W = 8
                with pytest.raises(hip.CadnipError) as e:
                    m.run(wpb, **kw)
                assert e.value.code == hip.BADARG and name == "dff" and wpb == 8
                continue
            got = m.run(wpb, **kw)
            assert got[5] == dict(wpb=wpb, lds_bytes=wpb * m.per, systems=S, workgroups=-(-S // wpb)) and m.is_default(got, ref), wpb
        # HBM: two persistent waves over the systems, each running system after system in its one workspace
        m.h.ac_set_memory("hbm", 2)
        try:
            for wpb in (0, 1, 2, 4, 8):
                got = m.run(wpb, **kw)
                assert got[5] == dict(wpb=wpb or 4, lds_bytes=0, systems=S, workgroups=-(-2 // (wpb or 4)))
                assert m.h.ac_plan_info() == dict(memory="hbm", n_waves=2, work_bytes=2 * m.per, lds_bytes=0)
                assert m.is_default(got, ref), wpb
        finally:
            m.h.ac_set_memory("lds")
    assert name != "butterworth" or 8 * m.per <= LDS_BUDGET        # the small circuit reaches every width
    for wpb in (3, 16, -1):
        with pytest.raises(hip.CadnipError) as e:
            m.run(wpb)
        assert e.value.code == hip.BADARG


@pytest.mark.parametrize("name", ["butterworth", "dff"])
def test_the_forms_against_the_direct_form(name):
    m = sens(name)
    st = m.c.st
    for kw in ({}, WIDE):
        y, s, x, berr, flags, _ = m.run(**kw)
        assert not flags[:, 1:].any()
        a = dict(base=m.base, plus=m.plus, minus=m.minus, scale=m.scale)
        a.update(kw)
        for bi, b in enumerate(a["base"]):
            for f, w in enumerate(m.om):
                if flags[bi, f].any():
                    continue                                      # (omega = 0 on a circuit with a capacitor-only pivot: flagged, checked elsewhere)
                A = R.system(st, m.G[b], m.Cm[b], w, GMIN)
                dA = np.array([(R.dense_csr(st, m.G[p] - m.G[q]) + 1j * w * R.dense_csr(st, m.Cm[p] - m.Cm[q])) * sc
                               for p, q, sc in zip(a["plus"][bi], a["minus"][bi], a["scale"][bi])])
                ref, xr, lr, wk = SR.direct_form(A, m.bac[b], dA, m.db[0, :2], m.pair)
                for k in range(2):
                    d = SR.d_s(A, xr, lr, dA[k], wk[k])
                    print("%s base %d f %d k %d  |s| %.3g  err %.3g  d_s %.3g" % (name, b, f, k, abs(ref[k]), abs(s[bi, f, k] - ref[k]), d))
                    assert abs(s[bi, f, k] - ref[k]) <= d, (bi, f, k)
    if name == "butterworth":                                     # dA = 0: s is lambda^T db, and without db exactly 0
        assert not np.any(m.G - m.G[0]) and not np.any(m.run(db=None)[1][:, 1:])


def test_swapping_plus_and_minus_negates_to_the_bit():
    """Without db every term of s is odd in (G+ - G-, C+ - C-) and rounding is symmetric: column 1 of the flip-flop setup (plus and minus
    swapped) is the negative of column 0 -- compared as numbers on finite values (a zero has no sign to negate)."""
    m = sens("dff")

    def negated(a, b):                                            # (omega = 0 may be a flagged system: non-finite on both sides)
        fin = np.isfinite(a)
        return np.array_equal(fin, np.isfinite(b)) and np.array_equal(a[fin], -b[fin])
    for kw in ({}, WIDE):
        s = m.run(db=None, **kw)[1]
        assert np.isfinite(s[0, 1:]).all() and np.all(s[0, 1:, 0] != 0)
        assert negated(s[0, :, 1], s[0, :, 0])
    a = m.run(db=None)[1]
    assert negated(m.run(db=None, plus=m.minus, minus=m.plus)[1], a) and negated(m.run(db=None, scale=[[-0.7, -0.7]])[1], a)


@pytest.mark.parametrize("mode", ["lds", "hbm"])
def test_a_nan_in_db_flags_its_own_column_only(mode):
    m = sens("dff")
    kw = dict(plus=[[2, 0, 2]], minus=[[0, 2, 1]], scale=[[0.7, 0.7, 0.3]])
    clean = m.run(**kw)
    assert not (clean[4][(clean[4] & 1) == 0] & 2).any()
    db = m.db.copy()
    db[0, 1, m.n // 2] = np.nan
    m.h.ac_set_memory(mode, 1 if mode == "hbm" else 0)
    try:
        y, s, x, berr, flags, _ = m.run(db=db, **kw)
    finally:
        m.h.ac_set_memory("lds")
    assert np.all(flags[:, :, 1] == clean[4][:, :, 1] | 2) and np.array_equal(flags[:, :, [0, 2]], clean[4][:, :, [0, 2]])
    assert np.isnan(s[:, :, 1]).all()
    assert same(s[:, :, [0, 2]], clean[1][:, :, [0, 2]]) and same(y, clean[0]) and same(x, clean[2]) and same(berr, clean[3])


def test_a_zero_pivot_flags_every_column_of_its_system_only():
    circ = cj.Circuit("capacitor-only node")
    circ.V("v1", "a", "0", dc=0.0, ac=1.0)
    circ.R("r1", "a", "b", 1e3)
    circ.C("c1", "b", "c", 1e-9)
    circ.C("c2", "c", "0", 1e-9)                       # node c: capacitors only -- at w = 0 without gmin its row is empty
    sim = api.BatchSimulator(api.MNACircuit(circ, {}, api.MNASpec(mode="dcop")))
    try:
        st = sim.st
        sim.analyze()
        sim.h.set_spec(mode="dcop")
        sim.h.rebuild(np.zeros(st.n), 0.0)
        e = np.zeros(st.n, complex)
        e[st.index_of("b")] = 1.0
        db = np.ones((1, 2, st.n), complex)
        for mode in ("lds", "hbm"):
            sim.h.ac_set_memory(mode, 1 if mode == "hbm" else 0)      # hbm: the flagged system first, then its neighbour, in one workspace
            y, s, x, berr, flags, info = sim.h.ac_sens([0.0, 1e3], 0.0, [0], [[0, 0]], [[0, 0]], [[1.0, 1.0]], api.rhs_ac(st, circ, {}), e,
                                                       (st.index_of("b"), -1), db, want_x=True)      # the call returns: CADNIP_OK
            sim.h.ac_set_memory("lds")
            assert info["systems"] == 2 and np.all(flags[0, 0] & 1) and not flags[0, 1].any()
            x1, berr1, _, _ = sim.h.ac_solve([0.0, 1e3], 0.0, api.rhs_ac(st, circ, {}))
            assert same(x[0, 1, 0], x1[0, 1]) and np.isfinite(s[0, 1]).all()
    finally:
        sim.close()


def raw(m, out, **kw):
    """cadnip_ac_sens itself, on the caller's arrays: the status code"""
    a = dict(om=m.om, base=m.base, plus=m.plus, minus=m.minus, scale=m.scale, pair=m.pair, wpb=0, n_freq=None, n_base=None, n_par=None, h=m.h)
    a.update(kw)
    om = np.ascontiguousarray(a["om"], dtype=np.float64)
    base, plus, minus = (np.ascontiguousarray(a[k], dtype=np.int32) for k in ("base", "plus", "minus"))
    scale, pair = np.ascontiguousarray(a["scale"], dtype=np.float64), np.ascontiguousarray(a["pair"], dtype=np.int32)
    bac, e, db = np.ascontiguousarray(m.bac[[1]]), np.ascontiguousarray(m.e), np.ascontiguousarray(m.db[:, :2])
    y, s, x, berr, flags = out
    info = np.zeros(4, dtype=np.int32)
    D, I = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    h = a["h"]
    return h.lib.cadnip_ac_sens(h.h, C.c_int32(len(om) if a["n_freq"] is None else a["n_freq"]), om.ctypes.data_as(D), C.c_double(GMIN),
                                C.c_int32(len(base) if a["n_base"] is None else a["n_base"]), base.ctypes.data_as(I),
                                C.c_int32(plus.shape[1] if a["n_par"] is None else a["n_par"]), plus.ctypes.data_as(I), minus.ctypes.data_as(I),
                                scale.ctypes.data_as(D), bac.ctypes.data_as(D), db.ctypes.data_as(D), e.ctypes.data_as(D), pair.ctypes.data_as(I),
                                C.c_int32(a["wpb"]), y.ctypes.data_as(D), s.ctypes.data_as(D), x.ctypes.data_as(D), berr.ctypes.data_as(D),
                                flags.ctypes.data_as(I), info.ctypes.data_as(I))


@pytest.mark.parametrize("name", ["butterworth", "dff"])
def test_refusals_launch_nothing(name):
    m = sens(name)
    n = m.n
    out = lambda: tuple(np.array(v) for v in m.got0[:5])
    o = out()
    assert raw(m, o) == hip.OK and m.is_default(o + (None,))                        # the helper is the call
    plan = m.h.ac_plan_info()
    refused = [dict(n_freq=0), dict(n_freq=-1), dict(n_base=0), dict(n_base=-1), dict(n_par=0), dict(n_par=-1),
               dict(base=[3]), dict(base=[-1]), dict(plus=[[2, 3]]), dict(plus=[[-1, 0]]), dict(minus=[[3, 2]]), dict(minus=[[0, -1]]),
               dict(pair=(n, -1)), dict(pair=(0, n)), dict(pair=(-2, 0)), dict(pair=(-1, -1)),
               dict(wpb=3), dict(wpb=16), dict(wpb=-1)]
    if 8 * m.per > LDS_BUDGET:
        refused.append(dict(wpb=8))                                                # the LDS refusal
    for kw in refused:
        o = out()
        assert raw(m, o, **kw) == hip.BADARG, kw
        assert m.is_default(o + (None,)) and m.h.ac_plan_info() == plan, kw       # nothing written, nothing recorded
    assert m.is_default(m.run())                                                   # the handle is as usable as before
    for call in (lambda: m.h.ac_sens(m.om, GMIN, [3], m.plus, m.minus, m.scale, m.bac[1], m.e, m.pair), lambda: m.run(3), lambda: m.run(base=[], plus=np.zeros((0, 2)), minus=np.zeros((0, 2)), scale=np.zeros((0, 2)), db=None),
                 lambda: m.run(plus=np.zeros((1, 0)), minus=np.zeros((1, 0)), scale=np.zeros((1, 0)), db=None)):
        with pytest.raises(hip.CadnipError) as e:
            call()
        assert e.value.code == hip.BADARG
    for call in (lambda: m.run(plus=[2, 0]), lambda: m.run(scale=[[0.7]]), lambda: m.run(db=np.zeros((1, 2, n + 1), complex)),
                 lambda: m.h.ac_sens(m.om, GMIN, m.base, m.plus, m.minus, m.scale, m.bac[1], m.e[:-1], m.pair),
                 lambda: m.h.ac_sens(m.om, GMIN, m.base, m.plus, m.minus, m.scale, m.bac[:2], m.e, m.pair)):
        with pytest.raises(ValueError):
            call()
    fresh = hip.Handle(m.st, 3)                                                    # no analysis
    try:
        o = out()
        assert raw(m, o, h=fresh) == hip.BADARG and m.is_default(o + (None,))
    finally:
        fresh.close()
    empty = m.h.ac_sens([], GMIN, m.base, m.plus, m.minus, m.scale, m.bac[1], m.e, m.pair, want_x=True)     # an empty grid launches nothing
    assert empty[0].shape == (1, 0) and empty[1].shape == (1, 0, 2) and empty[2].shape == (1, 0, 2, n) and empty[5]["systems"] == 0
    assert m.h.ac_plan_info() == plan


def test_the_circuit_beyond_lds_is_refused_there_and_solved_in_device_memory():
    """chain200 as test_gpu_ac_lu sets it up, on two instances at different states: refused under "lds", solved under "hbm" and "auto"."""
    mk, params = tc.CHAIN_STAMP["chain200"]
    sim = api.BatchSimulator(api.MNACircuit(mk(), dict(params), api.MNASpec(mode="dcop")), [{}, {}])
    try:
        st = sim.st
        sim.analyze()
        per = 16 * (sim.h.lu_stats()["nnz_lu"] + 4 * st.n)
        assert per > LDS_BUDGET
        sim.h.set_spec(mode="dcop")
        u = np.zeros((2, st.n))
        u[1, :st.n_nodes] = 5.0 * np.random.default_rng(3).random(st.n_nodes)        # up to 5 V: transistors that conduct (at 0 V none does: gm = 0 exactly)
        sim.h.rebuild(u, 0.0)
        G, Cm, _, _ = sim.h.get_GCb()
        to_ref = np.asarray(st.to_ref_nz)
        G, Cm = G[:, to_ref], Cm[:, to_ref]
        assert np.any(G[1] != G[0])
        bac = np.zeros(st.n, complex)
        bac[st.index_of("I_vin")] = 1.0
        out = (st.index_of("n1"), -1)                                              # the first stage's output: the input reaches it at every state
        e = SR.e_pair(st.n, out)
        om = [1e3, 1e6]
        base, plus, minus, scale = [1, 0], [[0, 1], [1, 0]], [[1, 0], [0, 1]], [[1.0, 0.5], [1.0, 0.5]]
        args = (om, GMIN, base, plus, minus, scale, bac, e, out)
        plan = sim.h.ac_plan_info()
        for wpb in (0, 1):
            with pytest.raises(hip.CadnipError) as err:
                sim.h.ac_sens(*args, wpb=wpb)
            assert err.value.code == hip.BADARG and sim.h.ac_plan_info() == plan
        got = {}
        for mode in ("hbm", "auto"):
            sim.h.ac_set_memory(mode)
            y, s, x, berr, flags, info = got[mode] = sim.h.ac_sens(*args, want_x=True)
            assert info == dict(wpb=4, lds_bytes=0, systems=4, workgroups=1) and sim.h.ac_plan_info() == dict(memory="hbm", n_waves=4, work_bytes=4 * per, lds_bytes=0)
            assert not flags.any() and np.all(berr[..., 0] <= api.AC_BERR_MAX) and np.all(berr[..., 1] <= api.NOISE_BERR_MAX)
            xs = sim.h.ac_solve(om, GMIN, bac)[0]
            assert same(x[:, :, 0], xs[base]) and same(y, xs[base][:, :, out[0]])
        sim.h.ac_set_memory("lds")
        assert all(same(got["hbm"][i], got["auto"][i]) for i in range(4))
        y, s = got["hbm"][:2]
        assert np.all(s[0] != 0)
        for bi, b in enumerate(base):
            for f, w in enumerate(om):
                A = R.system(st, G[b], Cm[b], w, GMIN)
                dA = np.array([(R.dense_csr(st, G[p] - G[q]) + 1j * w * R.dense_csr(st, Cm[p] - Cm[q])) * sc for p, q, sc in zip(plus[bi], minus[bi], scale[bi])])
                ref, xr, lr, wk = SR.direct_form(A, bac, dA, None, out)
                for k in range(2):
                    d = SR.d_s(A, xr, lr, dA[k], wk[k])
                    print("chain200 base %d w %.0e k %d  |s| %.3g  err %.3g  d_s %.3g" % (b, w, k, abs(ref[k]), abs(s[bi, f, k] - ref[k]), d))
                    assert abs(s[bi, f, k] - ref[k]) <= d, (bi, f, k)
    finally:
        sim.close()
