"""k_ac_adj_multi / k_ac_adj_multi_hbm (csrc/ac_lu.hip) through the C ABI (cadnip_ac_adjoint_multi): K adjoint right-hand sides per
factorisation.  Column k of the multi call runs the very per-column function of k_ac_adj, so everything here is held against
cadnip_ac_adjoint TO THE BIT -- whose results tests/test_gpu_ac_adjoint.py pins against the CPU references: the multi kernel needs no tolerance
of its own (the one exception: chain200, which test_gpu_ac_adjoint only refuses, is checked against a dense adjoint solve).  The systems are
those of ac_ref.CASES at the linearisations test_gpu_ac_adjoint.adj caches -- B = 2 instances on a handle of their own (the cached DC points
restamped: no DC solve), F = 3 frequencies, K up to 3 columns: two different unit vectors and one dense complex column.  Comparisons are on
the 64-bit patterns, so a NaN equals itself.  Mirrors tests/test_gpu_ac_multi.py test for test."""
import ctypes as C

import numpy as np
import pytest

import cadnip_jl_amd as cj
from cadnip_jl_amd import api, hip
from tests import ac_ref as R
from tests import circuits as tc
from tests import noise_ref as N
from tests import test_gpu_ac_adjoint as TA
from tests import test_gpu_ac_lu as T
from tests.test_gpu_ac_multi import bits, same, same_numbers, LDS_BUDGET, CHUNK_BYTES

pytestmark = pytest.mark.gpu
GMIN = T.GMIN
EPS = R.EPS


class Multi:
    """Two instances of the case at the DC points ``TA.adj(name)`` holds (the filter has one point: twice that one), restamped on a handle
    of their own and analysed on the cached AC pivot sample; omega = 0, the middle and the end of the case's grid; K = 3 columns per
    instance -- e_out of tests/noise_ref.py, a dense complex column (different per instance), a unit vector on the first branch row --
    and the single-column adjoint sweeps of every column, once."""

    def __init__(self, name):
        a = self.a = TA.adj(name)
        c = a.c
        mk, base, pts, _ = R.CASES[name]
        two = [pts[0], pts[-1]] if len(pts) > 1 else [{}, {}]
        src = [0, len(pts) - 1] if len(pts) > 1 else [0, 0]
        self.sim = api.BatchSimulator(api.MNACircuit(c.circ, dict(base), api.MNASpec(mode="dcop")), two)
        self.st, self.h, self.B, self.n = self.sim.st, self.sim.h, 2, c.st.n
        assert self.sim.B == 2
        self.h.set_spec(mode="dcop")
        self.h.rebuild(c.u[src], 0.0)
        G, Cm, _, _ = self.h.get_GCb()
        to_ref = np.asarray(c.st.to_ref_nz)
        assert np.array_equal(G[:, to_ref], c.G[src]) and np.array_equal(Cm[:, to_ref], c.C[src])      # the cached systems, to the bit
        self.G, self.Cm = c.G[src], c.C[src]
        self.h.analyze_values(c.sample_ref)
        self.om = np.array([0.0, c.om[len(c.om) // 2], c.om[-1]])
        self.F, self.K = 3, 3
        rng = np.random.default_rng(7)
        self.c = np.zeros((self.B, self.K, self.n), complex)
        self.c[:, 0] = a.rhs
        self.c[:, 1] = rng.standard_normal((self.B, self.n)) + 1j * rng.standard_normal((self.B, self.n))
        self.c[:, 2, c.st.n_nodes] = 1.0                      # the first branch row
        self.pairs = TA.all_pairs(self.n)
        self.single = [self.h.ac_adjoint(self.om, GMIN, self.c[:, k], self.pairs, want_x=True) for k in range(self.K)]
        self.h0, self.x0, self.berr0, self.flags0, self.info0 = self.run()

    def run(self, wpb=0, c=None, pairs="all", want_x=True):
        return self.h.ac_adjoint_multi(self.om, GMIN, self.c if c is None else c, self.pairs if isinstance(pairs, str) else pairs, wpb, want_x)

    def is_default(self, got):
        h, x, berr, flags, _ = got
        return same(h, self.h0) and same(x, self.x0) and same(berr, self.berr0) and np.array_equal(flags, self.flags0)


_MULTI = {}


def multi(name):
    if name not in _MULTI:
        _MULTI[name] = Multi(name)
    return _MULTI[name]


@pytest.mark.parametrize("name", ["butterworth", "dff"])
def test_column_k_is_the_single_adjoint_sweep_to_the_bit(name):
    m = multi(name)
    assert m.om[0] == 0.0 and m.x0.shape == (m.B, m.F, m.K, m.n) and m.h0.shape == (m.B, m.F, m.K, len(m.pairs))
    assert m.berr0.shape == m.flags0.shape == (m.B, m.F, m.K)
    for K in (1, 2, 3):
        h, x, berr, flags, info = m.run(c=m.c[:, :K])
        for k in range(K):
            h1, x1, berr1, flags1, info1 = m.single[k]
            assert same(h[:, :, k], h1) and same(x[:, :, k], x1) and same(berr[:, :, k], berr1) and np.array_equal(flags[:, :, k], flags1), (K, k)
        assert info == m.single[0][4]                             # one wave per system, the same plan: W, LDS bytes, systems, workgroups
    assert np.isfinite(m.x0[:, 1:]).all()                         # (non-finite values: only at omega = 0, a flagged zero pivot)
    # the columns are different systems: all six on the flip-flop; on the filter the two instances are one point, so only the dense column differs
    assert len({bits(m.x0[b, 1, k]).tobytes() for b in range(m.B) for k in range(m.K)}) == (6 if name == "dff" else 4)


@pytest.mark.parametrize("name", ["butterworth", "dff"])
def test_one_column_is_ac_adjoint(name):
    m = multi(name)
    h1, x1, berr1, flags1, info1 = m.single[0]
    h, x, berr, flags, info = m.run(c=m.c[:, :1], pairs=None)
    assert h is None and info == info1
    assert same(x[:, :, 0], x1) and same(berr[:, :, 0], berr1) and np.array_equal(flags[:, :, 0], flags1)
    hp, xp, _, _, _ = m.h.ac_adjoint_multi(m.om, GMIN, m.c[:, :1], m.pairs)           # the defaults: probes, no x
    assert xp is None and same(hp[:, :, 0], h1)
    _, xb, _, _, _ = m.h.ac_adjoint_multi(m.om, GMIN, m.c[0, :1], want_x=True)         # [K, n]: shared by the instances
    assert same(xb[0], x[0])
    mine = np.full(x.shape, np.nan + 0j)                                              # x_out: the caller's array is filled and returned
    _, xo, berro, _, _ = m.h.ac_adjoint_multi(m.om, GMIN, m.c[:, :1], x_out=mine)
    assert xo is mine and same(mine, x) and same(berro, berr)
    for bad in (np.zeros(x.shape[:-1] + (m.n + 1,), complex), np.zeros(x.shape), np.zeros(x.shape, complex).transpose(1, 0, 2, 3)):
        with pytest.raises(ValueError):
            m.h.ac_adjoint_multi(m.om, GMIN, m.c[:, :1], x_out=bad)


@pytest.mark.parametrize("name", ["butterworth", "dff"])
def test_launch_paths_are_bit_identical(name):
    m = multi(name)
    S, per = m.B * m.F, 16 * (m.h.lu_stats()["nnz_lu"] + 3 * m.n)
    assert m.info0["wpb"] in (1, 2, 4, 8) and m.info0["systems"] == S
    for wpb in (1, 2, 4, 8):
        if wpb * per > LDS_BUDGET:                                # the flip-flop at W = 8, as in test_gpu_ac_lu
            with pytest.raises(hip.CadnipError) as e:
                m.run(wpb)
            assert e.value.code == hip.BADARG and name == "dff" and wpb == 8
            continue
        got = m.run(wpb)
        assert got[4]["wpb"] == wpb and got[4]["workgroups"] == -(-S // wpb) and got[4]["lds_bytes"] == wpb * per and m.is_default(got), wpb
    # HBM: two persistent waves for six systems, so each strides over several systems AND runs several columns in its one workspace
    m.h.ac_set_memory("hbm", 2)
    try:
        for wpb in (0, 1, 2, 4, 8):
            got = m.run(wpb)
            assert got[4] == dict(wpb=wpb or 4, lds_bytes=0, systems=S, workgroups=-(-2 // (wpb or 4)))
            assert m.h.ac_plan_info() == dict(memory="hbm", n_waves=2, work_bytes=2 * per, lds_bytes=0)
            assert m.is_default(got), wpb
    finally:
        m.h.ac_set_memory("lds")
    assert m.is_default(m.run()) and m.h.ac_plan_info()["memory"] == "lds"


@pytest.mark.parametrize("name", ["butterworth", "dff"])
def test_probe_pairs(name):
    m = multi(name)
    n = m.n
    assert m.h0.shape == (m.B, m.F, m.K, 2 * n - 1)
    assert same(m.h0[..., :n], m.x0)                              # (i, -1): ground contributes 0
    assert same_numbers(m.h0[..., n:], m.x0[..., :-1] - m.x0[..., 1:])   # (i, i + 1): the double-precision difference of the returned x
    h, x, berr, flags, _ = m.run(want_x=False)
    assert x is None and same(h, m.h0) and same(berr, m.berr0) and np.array_equal(flags, m.flags0)


@pytest.mark.parametrize("mode", ["lds", "hbm"])
def test_columns_do_not_leak(mode):
    """A NaN in column 1 of instance 1: columns 0 and 2 of that instance run before and AFTER it in the same work arrays.  Under hbm one wave
    runs all six systems."""
    m = multi("dff")
    c = m.c.copy()
    c[1, 1, m.n // 2] = np.nan
    m.h.ac_set_memory(mode, 1 if mode == "hbm" else 0)
    try:
        h, x, berr, flags, _ = m.run(c=c)
    finally:
        m.h.ac_set_memory("lds")
    poisoned = np.zeros((m.B, m.F, m.K), bool)
    poisoned[1, :, 1] = True
    assert np.all(flags[poisoned] & 1) and not m.flags0[poisoned].any() and np.array_equal(flags[~poisoned], m.flags0[~poisoned])
    for got, clean in ((h, m.h0), (x, m.x0), (berr, m.berr0)):
        assert same(got[~poisoned], clean[~poisoned])


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
        c = np.zeros((3, st.n), complex)
        c[0] = api.rhs_ac(st, circ, {})
        c[1, st.index_of("b")] = 1.0
        c[2, st.index_of("c")] = 1.0
        pair = [(st.index_of("b"), st.index_of("c"))]
        for mode in ("lds", "hbm"):
            sim.h.ac_set_memory(mode, 1 if mode == "hbm" else 0)      # hbm: the flagged system first, then its neighbour, in one workspace
            h, x, berr, flags, info = sim.h.ac_adjoint_multi([0.0, 1e3], 0.0, c, pair, want_x=True)     # the call returns: CADNIP_OK
            sim.h.ac_set_memory("lds")
            assert info["systems"] == 2 and np.all(flags[0, 0] & 1) and not flags[0, 1].any()
            for k in range(3):
                h1, x1, berr1, flags1, _ = sim.h.ac_adjoint([0.0, 1e3], 0.0, c[k], pair, want_x=True)
                assert np.array_equal(flags1, flags[:, :, k])
                assert same(x[0, 1, k], x1[0, 1]) and same(berr[0, 1, k:k + 1], berr1[0, 1:2]) and same(h[0, 1, k], h1[0, 1])
    finally:
        sim.close()


def raw(h, om, c, pairs, wpb, hh, x, berr, flags, n_rhs=None, n_pairs=None, n_freq=None):
    """cadnip_ac_adjoint_multi itself, on the caller's arrays: the status code"""
    om, c = np.ascontiguousarray(om, dtype=np.float64), np.ascontiguousarray(c, dtype=np.complex128)
    pr = None if pairs is None else np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
    info = np.zeros(4, dtype=np.int32)
    D, I = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    return h.lib.cadnip_ac_adjoint_multi(h.h, C.c_int32(len(om) if n_freq is None else n_freq), om.ctypes.data_as(D), C.c_double(GMIN),
                                         C.c_int32(c.shape[-2] if n_rhs is None else n_rhs), c.ctypes.data_as(D),
                                         C.c_int32((0 if pr is None else len(pr)) if n_pairs is None else n_pairs), None if pr is None else pr.ctypes.data_as(I),
                                         C.c_int32(wpb), None if hh is None else hh.ctypes.data_as(D), None if x is None else x.ctypes.data_as(D),
                                         berr.ctypes.data_as(D), flags.ctypes.data_as(I), info.ctypes.data_as(I))


def test_refusals_launch_nothing():
    m = multi("butterworth")
    n = m.n
    out = lambda: (m.h0.copy(), m.x0.copy(), m.berr0.copy(), m.flags0.copy())
    hh, x, berr, flags = out()
    assert raw(m.h, m.om, m.c, m.pairs, 0, hh, x, berr, flags) == hip.OK and m.is_default((hh, x, berr, flags, None))    # the helper is the call
    plan = m.h.ac_plan_info()
    refused = [dict(n_freq=0), dict(n_freq=-1),                                         # no frequency
               dict(wpb=3), dict(wpb=16), dict(wpb=-1),                                 # wpb
               dict(n_rhs=0), dict(n_rhs=-1),                                           # no column
               dict(n_pairs=-1),
               dict(pairs=None, x=None),                                                # n_pairs = 0 and no x: nothing to return
               dict(pairs=[(0, n)]), dict(pairs=[(-2, 0)]), dict(pairs=[(0, -1), (n, -1)])]     # a pair index outside [-1, n)
    for kw in refused:
        kw = dict(kw)
        hh, x, berr, flags = out()
        args = dict(pairs=m.pairs, wpb=0, x=x)
        args.update(kw)
        code = raw(m.h, m.om, m.c, args.pop("pairs"), args.pop("wpb"), hh, args.pop("x"), berr, flags, **args)
        assert code == hip.BADARG, kw
        assert m.is_default((hh, x, berr, flags, None)) and m.h.ac_plan_info() == plan, kw          # nothing written, nothing recorded
        assert m.is_default(m.run())                                                                # the handle is as usable as before
    # the binding raises what the call returns
    for call in (lambda: m.run(c=m.c[:, :0]), lambda: m.run(pairs=None, want_x=False), lambda: m.run(pairs=[(0, n)]), lambda: m.run(3)):
        with pytest.raises(hip.CadnipError) as e:
            call()
        assert e.value.code == hip.BADARG
    # no analysis
    fresh = hip.Handle(m.st, 2)
    try:
        hh, x, berr, flags = out()
        assert raw(fresh, m.om, m.c, m.pairs, 0, hh, x, berr, flags) == hip.BADARG and m.is_default((hh, x, berr, flags, None))
    finally:
        fresh.close()
    empty = m.h.ac_adjoint_multi([], GMIN, m.c, m.pairs, want_x=True)                    # an empty grid launches nothing
    assert empty[0].shape == (m.B, 0, m.K, len(m.pairs)) and empty[1].shape == (m.B, 0, m.K, n) and empty[4]["systems"] == 0
    with pytest.raises(ValueError):
        m.h.ac_adjoint_multi(m.om, GMIN, np.zeros(n + 1, complex))


def test_the_circuit_beyond_lds_is_refused_there_and_solved_in_device_memory():
    """chain200 as test_gpu_ac_lu.test_a_circuit_beyond_lds_is_refused sets it up (zero state): 208 KB of work arrays.  The single-column
    adjoint kernel in device memory is the bit reference; a dense adjoint solve holds both to the forward bound of tests/ac_ref.py,
    d = 16 cond_inf(A^T) eps max|x_ref| (what tests/test_gpu_ac_adjoint.py holds k_ac_adj to)."""
    mk, params = tc.CHAIN_STAMP["chain200"]
    sim = api.BatchSimulator(api.MNACircuit(mk(), dict(params), api.MNASpec(mode="dcop")))
    try:
        st = sim.st
        sim.analyze()
        per = 16 * (sim.h.lu_stats()["nnz_lu"] + 3 * st.n)
        assert per > LDS_BUDGET
        sim.h.set_spec(mode="dcop")
        sim.h.rebuild(np.zeros(st.n), 0.0)
        c = np.zeros((2, st.n), complex)
        c[0, st.index_of("n200")] = 1.0
        c[1, st.index_of("I_vin")] = 1.0
        om = [1e3, 1e6]
        plan = sim.h.ac_plan_info()
        for wpb in (0, 1):
            with pytest.raises(hip.CadnipError) as e:
                sim.h.ac_adjoint_multi(om, GMIN, c, None, wpb, want_x=True)
            assert e.value.code == hip.BADARG
            mine = np.full((1, 2, 2, st.n), 7.0 + 0j)                                   # refused: the caller's array and the plan record stay
            with pytest.raises(hip.CadnipError):
                sim.h.ac_adjoint_multi(om, GMIN, c, None, wpb, x_out=mine)
            assert np.all(mine == 7.0) and sim.h.ac_plan_info() == plan
        pair = [(st.index_of("n100"), -1)]
        G, Cm, _, _ = sim.h.get_GCb()
        to_ref = np.asarray(st.to_ref_nz)
        for mode in ("hbm", "auto"):
            sim.h.ac_set_memory(mode)
            h, x, berr, flags, info = sim.h.ac_adjoint_multi(om, GMIN, c, pair, want_x=True)
            assert info == dict(wpb=4, lds_bytes=0, systems=2, workgroups=1) and sim.h.ac_plan_info() == dict(memory="hbm", n_waves=2, work_bytes=2 * per, lds_bytes=0)
            assert not flags.any() and np.all(berr <= api.NOISE_BERR_MAX)    # (at the zero state cond(A^T) is such that d below says little: berr says it)
            for k in range(2):
                h1, x1, berr1, flags1, _ = sim.h.ac_adjoint(om, GMIN, c[k], pair, want_x=True)
                assert same(x[:, :, k], x1) and same(h[:, :, k], h1) and same(berr[:, :, k], berr1) and np.array_equal(flags[:, :, k], flags1)
                assert same(h[:, :, k, 0], x1[:, :, st.index_of("n100")])
                if mode == "hbm":
                    for f, w in enumerate(om):
                        A = R.system(st, G[0, to_ref], Cm[0, to_ref], w, GMIN)
                        xr = R.refined_solve_c(A.T, c[k])
                        d = 16 * R.cond_inf_c(A.T) * EPS * np.max(np.abs(xr))
                        print("chain200 column %d w %.0e  err %.3g  d %.3g  berr %.3g" % (k, w, np.max(np.abs(x[0, f, k] - xr)), d, berr[0, f, k]))
                        assert np.max(np.abs(x[0, f, k] - xr)) <= d, (k, f)
        sim.h.ac_set_memory("lds")
    finally:
        sim.close()


def test_the_chunk_seam():
    """Two launches: the device output of a system is 16 K n_pairs bytes, a launch holds at most 64 MiB of it.  K = 8 columns and 2050
    (repeated) pairs make a chunk 255 systems; F = 128 frequencies on the two-instance filter handle are 256 systems, the smallest grid
    that crosses the seam -- chunks of 255 and 1 systems, the seam inside instance 1.  At wpb = 2 that is 128 + 1 workgroups where a single
    launch would have 128: info says two launches ran."""
    m = multi("butterworth")
    n, K, P, F, wpb = m.n, 8, 2050, 128, 2
    assert m.B == 2 and n == 6
    S = m.B * F
    chunk = CHUNK_BYTES // (16 * K * P)
    assert chunk == 255 and S == chunk + 1
    om = np.logspace(-2, 1, F)
    c = np.zeros((K, n), complex)
    c[:n] = np.eye(n)
    c[n], c[n + 1] = m.c[0, 1], 1j * m.c[1, 1] + 1.0
    pairs = np.tile(TA.all_pairs(n), (P // (2 * n - 1) + 1, 1))[:P]
    h, x, berr, flags, info = m.h.ac_adjoint_multi(om, GMIN, c, pairs, wpb)
    assert x is None and info == dict(wpb=wpb, lds_bytes=info["lds_bytes"], systems=S, workgroups=-(-chunk // wpb) + 1) and info["workgroups"] != -(-S // wpb)
    _, xs, berrs, flagss, infos = m.h.ac_adjoint_multi(om, GMIN, c, None, wpb, want_x=True)     # 16 K n bytes per system: one launch
    assert infos["workgroups"] == -(-S // wpb)
    pp, qq = pairs[:, 0], pairs[:, 1]
    ref = np.where(pp >= 0, xs[..., pp], 0.0) - np.where(qq >= 0, xs[..., np.maximum(qq, 0)], 0.0)
    assert same(h, ref) and same(berr, berrs) and np.array_equal(flags, flagss) and not flags.any()
    for k in (0, n):                                                                    # and the unchunked call is the single-column kernel
        _, x1, berr1, _, _ = m.h.ac_adjoint(om, GMIN, c[k], [(0, -1)], wpb, want_x=True)
        assert same(xs[:, :, k], x1) and same(berrs[:, :, k], berr1)
