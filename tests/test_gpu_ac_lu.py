"""k_ac_lu (csrc/ac_lu.hip) through the C ABI (cadnip_ac_solve): the batched complex sparse LU of the AC sweep against the CPU references of
tests/ac_ref.py -- the static-order complex LU under the handle's own pivot order (cadnip_lu_order) for the backward error, a refined
dense solve for the solution -- on the Butterworth filter, the sp_mos1 inverter at three supplies, linear_zoo and the flip-flop at three
corners x 7 frequencies (S = 21: a tail workgroup for every W > 1).  Launch paths, batch independence, flags, the circuit that does not fit
(tests/circuits.py CHAIN_STAMP["chain200"]: 16 (nnz(L+U) + 3 n) = 208 KB on the CPU port's order; chain40 needs 42 KB and fits) and the
LDS layout of the new shape."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import cadnip_jl_amd as cj
from cadnip_jl_amd import api, hip
from tests import ac_ref as R
from tests import circuits as tc

gpu = pytest.mark.gpu
EPS = R.EPS
GMIN = 1e-12
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cadnip.jl_amd", "csrc")


class Case:
    """One handle at the DC points of a case of ac_ref.CASES, analysed on the AC pivot sample; the CPU references of every system, once."""

    def __init__(self, name):
        mk, base, pts, grid = R.CASES[name]
        self.circ = mk()
        self.sim = api.BatchSimulator(api.MNACircuit(self.circ, dict(base), api.MNASpec(mode="dcop")), pts if pts != [{}] else None)
        self.st, self.h, self.B = self.sim.st, self.sim.h, self.sim.B
        self.u, conv, _ = self.sim.dc()
        assert np.all(conv), name
        self.h.rebuild(self.u, 0.0)
        G, C, _, _ = self.h.get_GCb()
        to_ref = np.asarray(self.st.to_ref_nz)
        self.G, self.C = G[:, to_ref], C[:, to_ref]                  # CSR order
        self.om = 2.0 * np.pi * np.asarray(grid(), dtype=float)
        self.F = len(self.om)
        self.bac = np.array([api.rhs_ac(self.st, self.circ, {k: float(v[i]) for k, v in self.sim.params.items()}) for i in range(self.B)])
        self.sample_ref = np.empty(self.st.nnz)
        self.sample_ref[to_ref] = api.ac_pivot_sample(self.st, self.G, self.C, self.om, GMIN)
        self.h.analyze_values(self.sample_ref)
        self.rp, self.cp = self.h.lu_order()
        self.ref = {}
        for b in range(self.B):
            for f, w in enumerate(self.om):
                A = R.system(self.st, self.G[b], self.C[b], w, GMIN)
                xs = R.static_order_solve_c(A, self.bac[b], self.rp, self.cp)
                self.ref[b, f] = (A, R.backward_error_c(A, xs, self.bac[b]), R.refined_solve_c(A, self.bac[b]), R.cond_inf_c(A))

    def run(self, wpb=0, bac=None):
        return self.h.ac_solve(self.om, GMIN, self.bac if bac is None else bac, wpb)


_CASES = {}


def case(name):
    if name not in _CASES:
        _CASES[name] = Case(name)
    return _CASES[name]


@gpu
@pytest.mark.parametrize("name", list(R.CASES))
def test_every_system_against_the_cpu_references(name):
    c = case(name)
    x, berr, flags, info = c.run()
    S = c.B * c.F
    assert x.shape == (c.B, c.F, c.st.n) and not flags.any()
    assert info["systems"] == S and info["workgroups"] == -(-S // info["wpb"]) and info["lds_bytes"] == 16 * info["wpb"] * (c.h.lu_stats()["nnz_lu"] + 3 * c.st.n)
    exempt = 0
    for (b, f), (A, berr_static, xref, kappa) in c.ref.items():
        host = R.backward_error_c(A, x[b, f], c.bac[b])
        print("%s b %d f %d berr gpu %.3g host-recomputed %.3g static %.3g fwd %.3g kappa eps %.3g" % (
            name, b, f, berr[b, f], host, berr_static, np.max(np.abs(x[b, f] - xref)) / np.max(np.abs(xref)), kappa * EPS))
        assert berr[b, f] <= 16 * berr_static + 64 * EPS, (b, f)
        assert host / 2 - 8 * EPS <= berr[b, f] <= 2 * host + 8 * EPS, (b, f)                # the reported figure is the figure
        if berr_static < api.AC_BERR_MAX / 16:
            assert np.max(np.abs(x[b, f] - xref)) <= 16 * kappa * EPS * np.max(np.abs(xref)), (b, f)
        else:
            exempt += 1
    assert exempt <= 0.05 * S


@gpu
@pytest.mark.parametrize("name", ["butterworth", "dff"])
def test_launch_paths_are_bit_identical(name):
    c = case(name)
    x0, berr0, flags0, info0 = c.run()
    assert info0["wpb"] in (1, 2, 4, 8)
    per = 16 * (c.h.lu_stats()["nnz_lu"] + 3 * c.st.n)
    assert name != "butterworth" or 8 * per <= 160 * 1024          # the small circuit reaches every width
    for wpb in (1, 2, 4, 8):
        if wpb * per > 160 * 1024:                                  # the flip-flop at W = 8: 230 KB of work arrays, beyond the LDS budget
            with pytest.raises(hip.CadnipError) as e:
                c.run(wpb)
            assert e.value.code == hip.BADARG and name == "dff" and wpb == 8
            continue
        x, berr, flags, info = c.run(wpb)
        assert info["wpb"] == wpb and info["workgroups"] == -(-c.B * c.F // wpb)
        assert np.array_equal(x.view(np.float64), x0.view(np.float64)) and np.array_equal(berr, berr0) and np.array_equal(flags, flags0)
    for wpb in (3, 16, -1):
        with pytest.raises(hip.CadnipError) as e:
            c.run(wpb)
        assert e.value.code == hip.BADARG


@gpu
def test_a_system_alone_equals_the_same_system_in_the_batch():
    c = case("dff")
    x, berr, _, _ = c.run()
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
        x1, berr1, flags1, info1 = one.h.ac_solve(c.om[f:f + 1], GMIN, c.bac[b:b + 1])
        assert info1["systems"] == 1 and info1["workgroups"] == 1 and not flags1.any()
        assert np.array_equal(x1[0, 0].view(np.float64), x[b, f].view(np.float64)) and berr1[0, 0] == berr[b, f]
    finally:
        one.close()


@gpu
def test_a_nan_excitation_flags_its_own_instance_only():
    c = case("dff")
    x, berr, flags, _ = c.run()
    bac = c.bac.copy()
    bac[1, c.st.n // 2] = np.nan
    xn, berrn, flagsn, _ = c.run(bac=bac)
    assert np.all(flagsn[1] & 1) and not flagsn[0].any() and not flagsn[2].any()
    for b in (0, 2):
        assert np.array_equal(xn[b].view(np.float64), x[b].view(np.float64)) and np.array_equal(berrn[b], berr[b])


@gpu
def test_a_zero_pivot_is_flagged_and_the_call_returns():
    circ = cj.Circuit("capacitor-only node")
    circ.V("v1", "a", "0", dc=0.0, ac=1.0)
    circ.R("r1", "a", "b", 1e3)
    circ.C("c1", "b", "c", 1e-9)
    circ.C("c2", "c", "0", 1e-9)                       # node c: capacitors only -- at w = 0 without gmin its row is empty
    sim = api.BatchSimulator(api.MNACircuit(circ, {}, api.MNASpec(mode="dcop")))
    try:
        sim.analyze()                                  # on G + 1e9 C: a usable order
        sim.h.set_spec(mode="dcop")
        sim.h.rebuild(np.zeros(sim.st.n), 0.0)
        x, berr, flags, info = sim.h.ac_solve([0.0, 1e3], 0.0, api.rhs_ac(sim.st, circ, {}))
        assert flags[0, 0] & 1 and flags[0, 1] == 0 and info["systems"] == 2
        A = np.zeros((sim.st.n, sim.st.n), complex)
        G, C, _, _ = sim.h.get_GCb()
        to_ref = np.asarray(sim.st.to_ref_nz)
        A = R.system(sim.st, G[0, to_ref], C[0, to_ref], 1e3, 0.0)
        xr = R.refined_solve_c(A, api.rhs_ac(sim.st, circ, {}))
        assert np.max(np.abs(x[0, 1] - xr)) <= 16 * R.cond_inf_c(A) * EPS * np.max(np.abs(xr))
    finally:
        sim.close()


@gpu
def test_a_circuit_beyond_lds_is_refused():
    """chain200 is the smallest chain of tests/circuits.py whose work array exceeds the plan's budget.  The linearisation point is the zero
    state: the kernel's answer does not depend on it, and the chain's DC solve needs the fallback ladder."""
    mk, params = tc.CHAIN_STAMP["chain200"]
    circ = mk()
    sim = api.BatchSimulator(api.MNACircuit(circ, dict(params), api.MNASpec(mode="dcop")))
    try:
        st = sim.st
        sim.analyze()
        assert 16 * (sim.h.lu_stats()["nnz_lu"] + 3 * st.n) > 160 * 1024
        sim.h.set_spec(mode="dcop")
        sim.h.rebuild(np.zeros(st.n), 0.0)
        b_ac = np.zeros(st.n, complex)
        b_ac[st.index_of("I_vin")] = 1.0
        for wpb in (0, 1):
            with pytest.raises(hip.CadnipError) as e:
                sim.h.ac_solve([1e6], GMIN, b_ac, wpb)
            assert e.value.code == hip.BADARG
        G, C, _, _ = sim.h.get_GCb()
        to_ref = np.asarray(st.to_ref_nz)
        Gd = R.dense_csr(st, G[0, to_ref])
        Gd[np.arange(st.n_nodes), np.arange(st.n_nodes)] += GMIN
        freqs = np.array([1e6])
        sol = api.ACSol(st, Gd, R.dense_csr(st, C[0, to_ref]), b_ac, np.zeros(st.n), freqs)
        stats = {"gpu_systems": 0, "host_systems": 0, "max_berr": 0.0, "wpb": 0}
        api.ac_gpu_sweep(sim.h, st, [sol], G, C, 2 * np.pi * freqs, GMIN, "auto", stats)
        assert stats["gpu_systems"] == 0 and stats["host_systems"] == 1 and "fallback" in stats and not sol._cache
        assert np.array_equal(sol["n200"], np.linalg.solve(Gd + 2j * np.pi * 1e6 * sol.C, b_ac)[st.index_of("n200")][None])   # the host's result
        with pytest.raises(hip.CadnipError):
            api.ac_gpu_sweep(sim.h, st, [sol], G, C, 2 * np.pi * freqs, GMIN, "gpu", dict(stats))
    finally:
        sim.close()


SHIM = r"""
#include "lds_layout.hpp"
using namespace cadnip;
extern "C" void t_ac(int lu, int n, int w, int wpb, long long* o) {
  const LdsAc<size_t> L = lds_ac((size_t)0, lu, n, w, wpb);
  o[0] = L.lu; o[1] = L.x; o[2] = L.r; o[3] = L.y; o[4] = L.end; o[5] = L.per; o[6] = lds_bytes(L);
}
"""


def test_lds_layout_of_the_ac_shape(tmp_path):
    """Host compiler, as tests/test_lds_layout.py: per system the complex factors (nnz_lu x 16 B) and three complex n-vectors, nothing else;
    the regions tile the block and start on 16 bytes."""
    src, lib = str(tmp_path / "shim.cpp"), str(tmp_path / "libshim.so")
    with open(src, "w") as f:
        f.write(SHIM)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", "-I", CSRC, "-o", lib, src])
    L = ctypes.CDLL(lib)
    for (lu, n), wpb in [((a, b), w) for a, b in ((1091, 235), (1, 1), (14, 6), (6408, 2204), (31, 13)) for w in (1, 2, 4, 8)]:
        spans = []
        for w in range(wpb):
            o = (ctypes.c_longlong * 7)()
            L.t_ac(lu, n, w, wpb, o)
            per = 2 * (lu + 3 * n)
            assert list(o) == [w * per, w * per + 2 * lu, w * per + 2 * lu + 2 * n, w * per + 2 * lu + 4 * n, wpb * per, per, 16 * wpb * (lu + 3 * n)]
            assert all(v % 2 == 0 for v in o[:4])
            spans += [(o[0], 2 * lu), (o[1], 2 * n), (o[2], 2 * n), (o[3], 2 * n)]
        spans.sort()
        assert spans[0][0] == 0 and all(s + ln == s2 for (s, ln), (s2, _) in zip(spans, spans[1:])) and spans[-1][0] + spans[-1][1] == wpb * 2 * (lu + 3 * n)
    assert 16 * (1091 + 3 * 235) * 4 <= 160 * 1024 < 16 * (1091 + 3 * 235) * 8       # the flip-flop: four systems per workgroup at the most
