"""k_ac_lu_multi / k_ac_lu_multi_hbm (csrc/ac_lu.hip) through the C ABI (cadnip_ac_solve_multi): K right-hand sides per factorisation.  Column k
of the multi call executes the statements of k_ac_lu on the same doubles, so everything here is held against cadnip_ac_solve TO THE BIT --
on the handles of tests/test_gpu_ac_lu.py (butterworth, B = 1; the flip-flop, B = 3), whose single-column results that module pins against
the CPU references: the multi kernel needs no tolerance of its own.  Comparisons are on the 64-bit patterns, so a NaN equals itself."""
import numpy as np
import pytest

import cadnip_jl_amd as cj
from cadnip_jl_amd import api, hip
from tests import ac_ref as R
from tests import circuits as tc
from tests import test_gpu_ac_adjoint as TA
from tests import test_gpu_ac_lu as T

pytestmark = pytest.mark.gpu
GMIN = T.GMIN
LDS_BUDGET = 160 * 1024
CHUNK_BYTES = 64 << 20                     # cadnip_ac_solve_multi: device output of one launch (include/cadnip_hip.h)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def same(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def same_numbers(a, b):
    """as ``same`` where the values are numbers; a NaN must meet a NaN, whatever its payload -- for values the TEST computes from NaNs (a
    difference of two NaNs has no defined sign or payload), never for what two kernels store"""
    fa, fb = np.ascontiguousarray(a).view(np.float64), np.ascontiguousarray(b).view(np.float64)
    nan = np.isnan(fa)
    return fa.shape == fb.shape and np.array_equal(nan, np.isnan(fb)) and np.array_equal(bits(fa)[~nan], bits(fb)[~nan])


class Multi:
    """The handle of T.case(name) with K = 3 columns per instance -- the case's own b_ac, a unit vector on a node row, a unit vector on a
    branch row -- over at most 5 frequencies of the case's grid, omega = 0 among them; the single-column sweeps of every column, once."""

    def __init__(self, name):
        c = self.c = T.case(name)
        self.st, self.h, self.B, self.n = c.st, c.h, c.B, c.st.n
        self.om = np.concatenate([[0.0], c.om[:: max(1, len(c.om) // 4)][:4]])
        self.F, self.K = len(self.om), 3
        self.b = np.zeros((self.B, self.K, self.n), complex)
        self.b[:, 0] = c.bac
        self.b[:, 1, c.st.n_nodes // 2] = 1.0
        self.b[:, 2, c.st.n_nodes] = 1.0                      # the first branch row
        self.pairs = TA.all_pairs(self.n)
        self.single = [self.h.ac_solve(self.om, GMIN, self.b[:, k]) for k in range(self.K)]
        self.h0, self.x0, self.berr0, self.flags0, self.info0 = self.run()

    def run(self, wpb=0, b=None, pairs="all", want_x=True):
        return self.h.ac_solve_multi(self.om, GMIN, self.b if b is None else b, self.pairs if isinstance(pairs, str) else pairs, wpb, want_x)

    def is_default(self, got):
        h, x, berr, flags, _ = got
        return same(h, self.h0) and same(x, self.x0) and same(berr, self.berr0) and np.array_equal(flags, self.flags0)


_MULTI = {}


def multi(name):
    if name not in _MULTI:
        _MULTI[name] = Multi(name)
    return _MULTI[name]


@pytest.mark.parametrize("name", ["butterworth", "dff"])
def test_column_k_is_the_single_sweep_to_the_bit(name):
    m = multi(name)
    assert m.F <= 5 and m.om[0] == 0.0 and m.x0.shape == (m.B, m.F, m.K, m.n) and m.berr0.shape == m.flags0.shape == (m.B, m.F, m.K)
    for k in range(m.K):
        x, berr, flags, info = m.single[k]
        assert same(m.x0[:, :, k], x) and same(m.berr0[:, :, k], berr) and np.array_equal(m.flags0[:, :, k], flags), k
    assert m.info0 == m.single[0][3]                              # one wave per system, the same plan: W, LDS bytes, systems, workgroups


@pytest.mark.parametrize("name", ["butterworth", "dff"])
def test_one_column_is_ac_solve(name):
    m = multi(name)
    x1, berr1, flags1, info1 = m.single[0]
    h, x, berr, flags, info = m.run(b=m.b[:, :1], pairs=None)
    assert h is None and info == info1
    assert same(x[:, :, 0], x1) and same(berr[:, :, 0], berr1) and np.array_equal(flags[:, :, 0], flags1)
    _, xb, _, _, _ = m.h.ac_solve_multi(m.om, GMIN, m.b[0, :1])           # [K, n]: broadcast over the instances
    assert same(xb[0], x[0])
    mine = np.full(x.shape, np.nan + 0j)                                  # x_out: the caller's array is filled and returned
    _, xo, berro, _, _ = m.h.ac_solve_multi(m.om, GMIN, m.b[:, :1], x_out=mine)
    assert xo is mine and same(mine, x) and same(berro, berr)
    for bad in (np.zeros(x.shape[:-1] + (m.n + 1,), complex), np.zeros(x.shape), np.zeros(x.shape, complex).transpose(1, 0, 2, 3)):
        with pytest.raises(ValueError):
            m.h.ac_solve_multi(m.om, GMIN, m.b[:, :1], x_out=bad)


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
        assert got[4]["wpb"] == wpb and got[4]["workgroups"] == -(-S // wpb) and m.is_default(got), wpb
    # HBM: two persistent waves, so each runs several systems AND several columns in its one workspace
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
    assert np.isfinite(m.x0[:, 1:]).all()                         # (NaNs: only the filter's omega = 0 systems, a flagged zero pivot)
    h, x, berr, flags, _ = m.run(want_x=False)
    assert x is None and same(h, m.h0) and same(berr, m.berr0) and np.array_equal(flags, m.flags0)


@pytest.mark.parametrize("mode", ["lds", "hbm"])
def test_columns_do_not_leak(mode):
    """A NaN in column 1 of instance 1: columns 0 and 2 of that instance run before and AFTER it in the same work arrays.  Under hbm one wave
    runs all 15 systems."""
    m = multi("dff")
    b = m.b.copy()
    b[1, 1, m.n // 2] = np.nan
    m.h.ac_set_memory(mode, 1 if mode == "hbm" else 0)
    try:
        h, x, berr, flags, _ = m.run(b=b)
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
        b = np.zeros((3, st.n), complex)
        b[0] = api.rhs_ac(st, circ, {})
        b[1, st.index_of("b")] = 1.0
        b[2, st.index_of("c")] = 1.0
        for mode in ("lds", "hbm"):
            sim.h.ac_set_memory(mode, 1 if mode == "hbm" else 0)      # hbm: the flagged system first, then its neighbour, in one workspace
            h, x, berr, flags, info = sim.h.ac_solve_multi([0.0, 1e3], 0.0, b, [(st.index_of("b"), st.index_of("c"))])
            sim.h.ac_set_memory("lds")
            assert info["systems"] == 2 and np.all(flags[0, 0] & 1) and not flags[0, 1].any()
            for k in range(3):
                x1, berr1, flags1, _ = sim.h.ac_solve([0.0, 1e3], 0.0, b[k])
                assert np.array_equal(flags1, flags[:, :, k])
                assert same(x[0, 1, k], x1[0, 1]) and same(berr[0, 1, k:k + 1], berr1[0, 1:2])
                assert same(h[0, 1, k], np.array([x1[0, 1, st.index_of("b")] - x1[0, 1, st.index_of("c")]]))
    finally:
        sim.close()


def test_refusals_launch_nothing():
    m = multi("butterworth")
    n = m.n
    refused = [lambda: m.run(b=m.b[:, :0]),                                        # n_rhs = 0
               lambda: m.run(pairs=None, want_x=False),                            # n_pairs = 0 and no x: nothing to return
               lambda: m.run(pairs=[(0, n)]), lambda: m.run(pairs=[(-2, 0)]),      # a pair index outside [-1, n)
               lambda: m.run(3), lambda: m.run(16), lambda: m.run(-1)]             # wpb
    for call in refused:
        with pytest.raises(hip.CadnipError) as e:
            call()
        assert e.value.code == hip.BADARG
        assert m.is_default(m.run())                                               # the handle is as usable as before
    empty = m.h.ac_solve_multi([], GMIN, m.b, m.pairs)                             # an empty grid launches nothing
    assert empty[0].shape == (m.B, 0, m.K, len(m.pairs)) and empty[1].shape == (m.B, 0, m.K, n) and empty[4]["systems"] == 0
    with pytest.raises(ValueError):
        m.h.ac_solve_multi(m.om, GMIN, np.zeros(n + 1, complex))


def test_the_circuit_beyond_lds_is_refused_there_and_solved_in_device_memory():
    """chain200 as test_gpu_ac_lu.test_a_circuit_beyond_lds_is_refused sets it up (zero state): 208 KB of work arrays."""
    mk, params = tc.CHAIN_STAMP["chain200"]
    sim = api.BatchSimulator(api.MNACircuit(mk(), dict(params), api.MNASpec(mode="dcop")))
    try:
        st = sim.st
        sim.analyze()
        per = 16 * (sim.h.lu_stats()["nnz_lu"] + 3 * st.n)
        assert per > LDS_BUDGET
        sim.h.set_spec(mode="dcop")
        sim.h.rebuild(np.zeros(st.n), 0.0)
        b = np.zeros((2, st.n), complex)
        b[0, st.index_of("I_vin")] = 1.0
        b[1, st.index_of("n100")] = 1.0
        om = [1e3, 1e6]
        for wpb in (0, 1):
            with pytest.raises(hip.CadnipError) as e:
                sim.h.ac_solve_multi(om, GMIN, b, None, wpb)
            assert e.value.code == hip.BADARG
        sim.h.ac_set_memory("hbm")
        h, x, berr, flags, info = sim.h.ac_solve_multi(om, GMIN, b, [(st.index_of("n200"), -1)])
        assert info == dict(wpb=4, lds_bytes=0, systems=2, workgroups=1) and sim.h.ac_plan_info() == dict(memory="hbm", n_waves=2, work_bytes=2 * per, lds_bytes=0)
        assert not flags.any()
        for k in range(2):
            x1, berr1, flags1, _ = sim.h.ac_solve(om, GMIN, b[k])
            assert same(x[:, :, k], x1) and same(berr[:, :, k], berr1) and np.array_equal(flags[:, :, k], flags1)
            assert same(h[:, :, k, 0], x1[:, :, st.index_of("n200")])
    finally:
        sim.close()


def test_the_chunk_seam():
    """Two launches: the device output of a system is 16 K n_pairs bytes, a launch holds at most 64 MiB of it.  K = 8 columns and 2050
    (repeated) pairs make a chunk 255 systems; F = 256 frequencies on the one-instance filter are the smallest grid that crosses the seam --
    chunks of 255 and 1 systems.  At wpb = 2 that is 128 + 1 workgroups where a single launch would have 128: info says two launches ran."""
    m = multi("butterworth")
    n, K, P, F, wpb = m.n, 8, 2050, 256, 2
    assert m.B == 1 and n == 6
    chunk = CHUNK_BYTES // (16 * K * P)
    assert chunk == 255 and F == chunk + 1
    om = np.logspace(-2, 1, F)
    b = np.zeros((K, n), complex)
    b[:n] = np.eye(n)
    b[n], b[n + 1] = m.c.bac[0], 1j * m.c.bac[0] + 1.0
    pairs = np.tile(TA.all_pairs(n), (P // (2 * n - 1) + 1, 1))[:P]
    h, x, berr, flags, info = m.h.ac_solve_multi(om, GMIN, b, pairs, wpb, want_x=False)
    assert x is None and info == dict(wpb=wpb, lds_bytes=info["lds_bytes"], systems=F, workgroups=-(-chunk // wpb) + 1) and info["workgroups"] != -(-F // wpb)
    _, xs, berrs, flagss, infos = m.h.ac_solve_multi(om, GMIN, b, None, wpb)     # 16 K n bytes per system: one launch
    assert infos["workgroups"] == -(-F // wpb)
    pp, qq = pairs[:, 0], pairs[:, 1]
    ref = np.where(pp >= 0, xs[..., pp], 0.0) - np.where(qq >= 0, xs[..., np.maximum(qq, 0)], 0.0)
    assert same(h, ref) and same(berr, berrs) and np.array_equal(flags, flagss) and not flags.any()
