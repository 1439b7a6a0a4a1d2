"""k_ac_adj (csrc/ac_lu.hip) through the C ABI (cadnip_ac_adjoint): the adjoint systems A^T x = e_out of the cases of ac_ref.CASES -- the handles
and systems of tests/test_gpu_ac_lu.py, the output nodes of tests/noise_ref.py -- against the CPU references: the static-order complex LU
used transposed under the handle's own pivot order for the backward error, a refined dense solve of A^T for the solution.  The probe pairs
are (i, -1) for every unknown i, then (i, i + 1): K = 2 n - 1, beyond 64 on the flip-flop (the lane-stride loop wraps), and the first n
reproduce x.  Launch widths, batch independence, flags, refusals, and the factors shared with the plain kernel."""
import numpy as np
import pytest

import cadnip_jl_amd as cj
from cadnip_jl_amd import api, hip, netlist
from tests import ac_ref as R
from tests import circuits as tc
from tests import noise_ref as N
from tests import test_gpu_ac_lu as T

gpu = pytest.mark.gpu
EPS = R.EPS
GMIN = T.GMIN
_ADJ = {}


def all_pairs(n):
    return np.array([(i, -1) for i in range(n)] + [(i, i + 1) for i in range(n - 1)], dtype=np.int32).reshape(-1, 2)


class Adj:
    """The handle of test_gpu_ac_lu's case (DC points, AC pivot sample, order) with the adjoint right-hand side and its CPU references, once."""

    def __init__(self, name):
        self.c = T.case(name)
        c = self.c
        self.st, self.h, self.B, self.F, self.om = c.st, c.h, c.B, c.F, c.om
        self.rhs = N.e_out(name, c.st)
        self.pairs = all_pairs(c.st.n)
        self.ref = {}
        for (b, f), (A, _, _, _) in c.ref.items():
            xs = N.static_order_adjoint_c(A, self.rhs, c.rp, c.cp)
            self.ref[b, f] = (A, R.backward_error_c(A.T, xs, self.rhs), R.refined_solve_c(A.T, self.rhs), R.cond_inf_c(A.T))

    def run(self, wpb=0, rhs=None, pairs=None, want_x=True):
        return self.h.ac_adjoint(self.om, GMIN, self.rhs if rhs is None else rhs, self.pairs if pairs is None else pairs, wpb, want_x)


def adj(name):
    if name not in _ADJ:
        _ADJ[name] = Adj(name)
    return _ADJ[name]


def same(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.float64), np.ascontiguousarray(b).view(np.float64))


@gpu
@pytest.mark.parametrize("name", list(R.CASES))
def test_every_adjoint_system_against_the_cpu_references(name):
    """Exempt from the forward check (static-order backward error at or above gate / 16): none, on the CPU port (tests/test_lu_transpose_cpu.py:
    test_static_order_adjoint_agrees_...) with the output nodes of noise_ref.OUTPUTS -- 0 of 61, 0 of 78, 0 of 9, 0 of 21 systems."""
    a = adj(name)
    n, S = a.st.n, a.B * a.F
    h, x, berr, flags, info = a.run()
    assert h.shape == (a.B, a.F, 2 * n - 1) and x.shape == (a.B, a.F, n) and not flags.any()
    assert info["systems"] == S and info["workgroups"] == -(-S // info["wpb"]) and info["lds_bytes"] == 16 * info["wpb"] * (a.h.lu_stats()["nnz_lu"] + 3 * n)
    exempt = 0
    for (b, f), (A, berr_static, xref, kappa) in a.ref.items():
        host = R.backward_error_c(A.T, x[b, f], a.rhs)
        print("%s b %d f %d berr gpu %.3g host-recomputed %.3g static %.3g fwd %.3g kappa eps %.3g" % (
            name, b, f, berr[b, f], host, berr_static, np.max(np.abs(x[b, f] - xref)) / np.max(np.abs(xref)), kappa * EPS))
        assert berr[b, f] <= 16 * berr_static + 64 * EPS, (b, f)
        assert host / 2 - 8 * EPS <= berr[b, f] <= 2 * host + 8 * EPS, (b, f)                # the reported figure is the figure
        if berr_static < api.NOISE_BERR_MAX / 16:
            assert np.max(np.abs(x[b, f] - xref)) <= 16 * kappa * EPS * np.max(np.abs(xref)), (b, f)
        else:
            exempt += 1
    assert exempt <= 0.05 * S
    # the pairs: (i, -1) reproduces x; (i, i + 1) is the double-precision difference of the returned x -- both to the bit
    assert same(h[:, :, :n], x)
    assert same(h[:, :, n:], x[:, :, :-1] - x[:, :, 1:])
    # without x: the same h, berr and flags
    h2, x2, berr2, flags2, _ = a.run(want_x=False)
    assert x2 is None and same(h2, h) and np.array_equal(berr2, berr) and np.array_equal(flags2, flags)


@gpu
@pytest.mark.parametrize("name", ["butterworth", "dff"])
def test_adjoint_launch_paths_are_bit_identical(name):
    a = adj(name)
    h0, x0, berr0, flags0, info0 = a.run()
    assert info0["wpb"] in (1, 2, 4, 8)
    per = 16 * (a.h.lu_stats()["nnz_lu"] + 3 * a.st.n)
    assert name != "butterworth" or 8 * per <= 160 * 1024          # the small circuit reaches every width
    for wpb in (1, 2, 4, 8):
        if wpb * per > 160 * 1024:                                  # the flip-flop at W = 8
            with pytest.raises(hip.CadnipError) as e:
                a.run(wpb)
            assert e.value.code == hip.BADARG and name == "dff" and wpb == 8
            continue
        h, x, berr, flags, info = a.run(wpb)
        assert info["wpb"] == wpb and info["workgroups"] == -(-a.B * a.F // wpb) and info["lds_bytes"] == wpb * per
        assert same(h, h0) and same(x, x0) and np.array_equal(berr, berr0) and np.array_equal(flags, flags0)
    for wpb in (3, 16, -1):
        with pytest.raises(hip.CadnipError) as e:
            a.run(wpb)
        assert e.value.code == hip.BADARG


@gpu
def test_an_adjoint_system_alone_equals_the_same_system_in_the_batch():
    a = adj("dff")
    c = a.c
    h, x, berr, _, _ = a.run()
    mk, base, pts, _ = R.CASES["dff"]
    b, f = 2, 5
    one = api.BatchSimulator(api.MNACircuit(c.circ, dict(base), api.MNASpec(mode="dcop")), [pts[b]])
    try:
        one.h.set_spec(mode="dcop")
        one.h.rebuild(c.u[b], 0.0)
        G1, C1, _, _ = one.h.get_GCb()
        to_ref = np.asarray(c.st.to_ref_nz)
        assert np.array_equal(G1[0, to_ref], c.G[b]) and np.array_equal(C1[0, to_ref], c.C[b])     # the same system, to the bit
        one.h.analyze_values(c.sample_ref)
        h1, x1, berr1, flags1, info1 = one.h.ac_adjoint(c.om[f:f + 1], GMIN, a.rhs, a.pairs, want_x=True)
        assert info1["systems"] == 1 and info1["workgroups"] == 1 and not flags1.any()
        assert same(x1[0, 0], x[b, f]) and same(h1[0, 0], h[b, f]) and berr1[0, 0] == berr[b, f]
    finally:
        one.close()


@gpu
def test_a_nan_right_hand_side_flags_its_own_instance_only():
    a = adj("dff")
    h, x, berr, flags, _ = a.run()
    rhs = np.tile(a.rhs, (a.B, 1))
    rhs[1, a.st.n // 2] = np.nan
    hn, xn, berrn, flagsn, _ = a.run(rhs=rhs)
    assert np.all(flagsn[1] & 1) and not flagsn[0].any() and not flagsn[2].any()
    for b in (0, 2):
        assert same(xn[b], x[b]) and same(hn[b], h[b]) and np.array_equal(berrn[b], berr[b])


@gpu
def test_a_zero_pivot_is_flagged_in_the_adjoint_sweep_and_the_call_returns():
    circ = cj.Circuit("capacitor-only node")
    circ.V("v1", "a", "0", dc=0.0, ac=1.0)
    circ.R("r1", "a", "b", 1e3)
    circ.C("c1", "b", "c", 1e-9)
    circ.C("c2", "c", "0", 1e-9)                       # node c: capacitors only -- at w = 0 without gmin its row is empty
    sim = api.BatchSimulator(api.MNACircuit(circ, {}, api.MNASpec(mode="dcop")))
    try:
        st = sim.st
        sim.analyze()                                  # on G + 1e9 C: a usable order
        sim.h.set_spec(mode="dcop")
        sim.h.rebuild(np.zeros(st.n), 0.0)
        rhs = np.zeros(st.n, complex)
        rhs[st.index_of("b")] = 1.0
        h, x, berr, flags, info = sim.h.ac_adjoint([0.0, 1e3], 0.0, rhs, all_pairs(st.n), want_x=True)
        assert flags[0, 0] & 1 and flags[0, 1] == 0 and info["systems"] == 2
        G, C, _, _ = sim.h.get_GCb()
        to_ref = np.asarray(st.to_ref_nz)
        A = R.system(st, G[0, to_ref], C[0, to_ref], 1e3, 0.0)
        xr = R.refined_solve_c(A.T, rhs)
        assert np.max(np.abs(x[0, 1] - xr)) <= 16 * R.cond_inf_c(A.T) * EPS * np.max(np.abs(xr))
    finally:
        sim.close()


@gpu
def test_refusals_launch_nothing():
    a = adj("butterworth")
    n = a.st.n
    for bad in ([(0, n)], [(-2, 0)], [(0, -1), (n, -1)], np.zeros((0, 2), dtype=np.int32)):
        with pytest.raises(hip.CadnipError) as e:
            a.run(pairs=bad)
        assert e.value.code == hip.BADARG
    mk, params = tc.CHAIN_STAMP["chain200"]
    sim = api.BatchSimulator(api.MNACircuit(mk(), dict(params), api.MNASpec(mode="dcop")))
    try:
        st = sim.st
        sim.analyze()
        assert 16 * (sim.h.lu_stats()["nnz_lu"] + 3 * st.n) > 160 * 1024
        sim.h.set_spec(mode="dcop")
        sim.h.rebuild(np.zeros(st.n), 0.0)
        rhs = np.zeros(st.n, complex)
        rhs[st.index_of("n200")] = 1.0
        for wpb in (0, 1):
            with pytest.raises(hip.CadnipError) as e:
                sim.h.ac_adjoint([1e6], GMIN, rhs, [(0, -1)], wpb)
            assert e.value.code == hip.BADARG
    finally:
        sim.close()


@gpu
@pytest.mark.parametrize("text", ["* divider\nV1 in 0 DC 0 AC 1\nR1 in out 1k\nR2 out 0 1k\n", "* rc\nV1 in 0 DC 0 AC 1\nR1 in out 1k\nC1 out 0 1u\n"])
def test_plain_and_adjoint_factors_coincide_on_symmetric_systems(text):
    """The MNA matrices of R, C and a grounded voltage source are symmetric: A^T x = b_ac is A x = b_ac, and the adjoint kernel -- same
    load, same factors, transposed solves -- returns the plain kernel's solution to rounding."""
    circ, _ = netlist.read_spice(text)
    sim = api.BatchSimulator(api.MNACircuit(circ, {}, api.MNASpec(mode="dcop")))
    try:
        st = sim.st
        sim.analyze()
        sim.h.set_spec(mode="dcop")
        sim.h.rebuild(np.zeros(st.n), 0.0)
        G, C, _, _ = sim.h.get_GCb()
        to_ref = np.asarray(st.to_ref_nz)
        om = 2 * np.pi * np.array([1.0, 1e3, 1e6])
        b_ac = api.rhs_ac(st, circ, {})
        xp, _, fp, _ = sim.h.ac_solve(om, GMIN, b_ac)
        _, xa, _, fa, _ = sim.h.ac_adjoint(om, GMIN, b_ac, [(0, -1)], want_x=True)
        assert not fp.any() and not fa.any()
        for f, w in enumerate(om):
            A = R.system(st, G[0, to_ref], C[0, to_ref], w, GMIN)
            assert np.array_equal(A, A.T)
            assert np.max(np.abs(xa[0, f] - xp[0, f])) <= 16 * R.cond_inf_c(A) * EPS * np.max(np.abs(xp[0, f]))
    finally:
        sim.close()
