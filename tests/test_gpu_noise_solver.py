"""noise! with the adjoint sweep on the GPU (api.noise(..., solver="gpu" | "auto"); api.noise_solve_gpu -> cadnip_ac_adjoint, k_ac_adj): the
closed forms and fixtures of tests/test_gpu_noise.py at the same tolerances, the GPU sweep against the host's dense adjoint solves source
by source, a CircuitSweep as one resident batch, and the fallback / refusal of a circuit beyond the kernel's LDS budget.

GPU against host, per source name:  |c_gpu - c_host| <= sum_k S_k (2 |H_k| d + d^2),  d = 32 kappa eps max|x_adj| -- 16 kappa eps for each
of the two solves being compared -- with kappa = cond_inf(A^T) and x_adj, H_k from the host's matrices."""
import os

import numpy as np
import pytest

import cadnip_jl_amd as cj
from cadnip_jl_amd import api, netlist, structure as S
from cadnip_jl_amd.circuit import Circuit
from tests import ac_ref as R
from tests import circuits as tc

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
KT = api.K_BOLTZMANN * (27.0 + 273.15)
KINDS = ("thermal", "shot", "white", "flicker")
EPS = R.EPS


def assert_within_the_solves_bound(st, Gd, Cd, srcs, output, temp, gpu, host):
    """the bound of the module docstring on every contribution, on onoise, and through the same d on the gain"""
    out_idx, in_idx = api.noise_indices(st, output, host.input)
    e_out = np.zeros(st.n, dtype=complex)
    e_out[out_idx] = 1.0
    assert list(gpu.contributions) == list(host.contributions)
    for fi, f in enumerate(host.freqs):
        AT = (Gd + 2j * np.pi * f * Cd).T
        x_adj = np.linalg.solve(AT, e_out)
        d = 32 * R.cond_inf_c(AT) * EPS * np.max(np.abs(x_adj))
        tol = {s[5]: 0.0 for s in srcs}
        for s in srcs:
            Hk = (x_adj[s[0]] if s[0] >= 0 else 0.0) - (x_adj[s[1]] if s[1] >= 0 else 0.0)
            tol[s[5]] += api.noise_psd(s, temp, f) * (2 * abs(Hk) * d + d * d)
        for nm in tol:
            assert abs(gpu[nm][fi] - host[nm][fi]) <= tol[nm], (nm, fi)
        assert abs(gpu["onoise"][fi] - host["onoise"][fi]) <= sum(tol.values()), fi
        if host.input is not None:
            assert abs(gpu.gain[fi] - host.gain[fi]) <= d


def linearise(mc, pts=None, gmin=1e-12, at_zero=False):
    """What api.noise does before the sweep: DC points (``at_zero``: the zero state instead), restamp, dense G (gmin on the node diagonals)
    and C.  The simulator stays open."""
    import scipy.sparse as sp
    mc = api.MNACircuit(mc.circuit, mc.params, api.MNASpec(temp=mc.spec.temp, mode="dcop", gmin=mc.spec.gmin))
    sim = api.BatchSimulator(mc, pts)
    st = sim.st
    if at_zero:
        sim.analyze()
        sim.h.set_spec(mode="dcop")
        u = np.zeros((sim.B, st.n))
    else:
        u, conv, _ = sim.dc()
        assert np.all(conv)
    sim.h.rebuild(u, 0.0)
    G, C, _, _ = sim.h.get_GCb()
    dense = lambda nz: sp.csc_matrix((nz, st.ref_rowval, st.ref_colptr), shape=(st.n, st.n)).toarray()
    Gd, Cd = [dense(g) for g in G], [dense(c) for c in C]
    for g in Gd:
        g[np.arange(st.n_nodes), np.arange(st.n_nodes)] += gmin
    return sim, st, u, G, C, Gd, Cd


def common_source(vdd=5.0):
    c = Circuit("SimpleMOSFET common-source stage")
    c.V("vdd", "vdd", "0", dc=vdd)
    c.V("vg", "in", "0", dc=1.0)
    c.R("rd", "vdd", "out", 10e3)
    c.SMOS("m1", "out", "in", "0", Vth=0.5, K=1e-3, lambda_=0.02, KF=1e-14, AF=1.2, FFE=0.9)
    return c


def test_divider_and_rc_closed_forms_on_the_gpu():
    circ, _ = netlist.read_spice("* divider\nV1 in 0 DC 0\nR1 in out 1k\nR2 out 0 1k\n")
    ns = api.noise(api.MNACircuit(circ, {}), "out", [1.0, 1e3, 1e6], input="V1", solver="gpu")
    assert ns.stats["gpu_systems"] == 3 and ns.stats["host_systems"] == 0 and ns.stats["wpb"] in (1, 2, 4, 8) and "fallback" not in ns.stats
    assert 0 <= ns.stats["max_berr"] <= api.NOISE_BERR_MAX
    assert np.allclose(ns["onoise"], 4 * KT * 500.0, rtol=1e-6) and np.allclose(ns["r1"], ns["r2"]) and np.allclose(ns["r1"] + ns["r2"], ns["onoise"])
    assert np.allclose(ns.gain.real, 0.5, rtol=1e-6) and np.allclose(ns.gain.imag, 0.0, atol=1e-9)
    assert np.allclose(ns["inoise"], 4 * KT * 500.0 / 0.25, rtol=1e-6)
    circ, _ = netlist.read_spice("* rc\nV1 in 0 DC 0\nR1 in out 1k\nC1 out 0 1u\n")
    freqs = api.acdec(10, 1.0, 1e7)
    ns = api.noise(api.MNACircuit(circ, {}), "out", freqs, input="V1", solver="gpu")
    assert ns.stats["gpu_systems"] == len(freqs) and ns.stats["host_systems"] == 0
    assert np.allclose(ns["onoise"], 4 * KT * 1e3 / (1 + (2 * np.pi * freqs * 1e3 * 1e-6) ** 2), rtol=1e-6) and np.allclose(ns["r1"], ns["onoise"])
    assert np.allclose(ns["inoise"], 4 * KT * 1e3, rtol=1e-6)
    assert api.total_noise(ns, referred="input") ** 2 == pytest.approx(4 * KT * 1e3 * (freqs[-1] - freqs[0]), rel=1e-6)
    with pytest.raises(ValueError):
        api.noise(api.MNACircuit(circ, {}), "out", [], solver="gpu")
    with pytest.raises(KeyError):
        api.noise(api.MNACircuit(circ, {}), "out", [1e3], input="R1", solver="gpu")
    with pytest.raises(ValueError):
        api.noise(api.MNACircuit(circ, {}), "out", [1e3], solver="fpga")


def test_common_source_closed_form_on_the_gpu_and_against_the_host_source_by_source():
    mc = api.MNACircuit(common_source(), {})
    freqs = np.array([1.0, 10.0, 1e3, 1e5])
    ns = api.noise(mc, "out", freqs, solver="gpu")
    assert ns.stats["gpu_systems"] == 4 and ns.stats["host_systems"] == 0
    vds = api.dc(mc)["out"]
    ids = 1e-3 / 2 * 0.5 ** 2 * (1 + 0.02 * vds)
    gm, gds = 1e-3 * 0.5 * (1 + 0.02 * vds), 1e-3 / 2 * 0.5 ** 2 * 0.02
    rout = 1.0 / (1.0 / 10e3 + gds)
    assert np.allclose(ns["onoise"], (4 * KT / 10e3 + 4 * KT * (2.0 / 3.0) * gm + 1e-14 * ids ** 1.2 / freqs ** 0.9) * rout ** 2, rtol=1e-6)
    assert np.allclose(ns["m1"] + ns["rd"], ns["onoise"])
    sim, st, u, G, C, Gd, Cd = linearise(mc)
    try:
        srcs = api.noise_sources(st, mc.circuit, {}, u[0], 27.0, 1e-12)
        host = api.noise_solve(st, Gd[0], Cd[0], srcs, "out", freqs, "vg", 27.0)
        gpu, = api.noise_solve_gpu(sim.h, st, G, C, Gd, Cd, [srcs], "out", freqs, "vg", 27.0)
        assert_within_the_solves_bound(st, Gd[0], Cd[0], srcs, "out", 27.0, gpu, host)
        assert np.allclose(gpu["onoise"], ns["onoise"], rtol=1e-9)
    finally:
        sim.close()


@pytest.mark.parametrize("name", ["noise_diode", "noise_bjt"])
def test_fixture_noise_through_the_split_out_solve(name):
    """test/noise.jl:161-189 with the GPU's operating point, linearisation AND adjoint sweep; the oracle's registered sources travel as data"""
    import scipy.sparse as sp
    st, x = S.load_structure(os.path.join(GOLD, "va_%s.npz" % name))
    packed = [x["packed%d" % i] for i in range(int(x["n_packed"][0]))]
    sim = api.BatchSimulator.from_packed(st, packed, api.MNASpec(mode="dcop", temp=27.0), vscale=2.0)
    try:
        u, conv, _ = sim.dc(abstol=1e-10, mode="dcop")
        assert conv[0]
        sim.h.rebuild(u, 0.0)
        G, C, _, _ = sim.h.get_GCb()
        dense = lambda nz: sp.csc_matrix((nz, st.ref_rowval, st.ref_colptr), shape=(st.n, st.n)).toarray()
        Gd, Cd = dense(G[0]), dense(C[0])
        Gd[np.arange(st.n_nodes), np.arange(st.n_nodes)] += 1e-12
        names = bytes(x["noise_names"]).decode().split(",")
        srcs = [(int(p) - 1, int(n) - 1, KINDS[int(k)], float(a), float(b), nm)
                for p, n, k, a, b, nm in zip(x["noise_p"], x["noise_n"], x["noise_kind"], x["noise_a"], x["noise_b"], names)]
        output, freqs = bytes(x["noise_output"]).decode(), x["noise_freqs"]
        stats = {"gpu_systems": 0, "host_systems": 0, "max_berr": 0.0, "wpb": 0}
        ns, = api.noise_solve_gpu(sim.h, st, G, C, [Gd], [Cd], [srcs], output, freqs, None, 27.0, 1e-12, "gpu", stats)
        host = api.noise_solve(st, Gd, Cd, srcs, output, freqs, None, 27.0)
    finally:
        sim.close()
    assert stats["gpu_systems"] == len(freqs) and stats["host_systems"] == 0 and ns.stats is stats
    assert np.allclose(ns["onoise"], x["noise_onoise"], rtol=1e-6)
    assert np.allclose(sum(ns.contributions.values()), ns["onoise"]) and np.all(ns["onoise"] > 0)
    assert_within_the_solves_bound(st, Gd, Cd, srcs, output, 27.0, ns, host)


def test_a_circuit_sweep_is_one_resident_batch(monkeypatch):
    c = common_source(cj.Param("vdd"))
    vdds, freqs = [4.5, 5.0, 5.5], np.array([1.0, 1e2, 1e4, 1e6])
    mc = api.MNACircuit(c, {"vdd": 5.0})
    made = []
    real = api.BatchSimulator

    class Counting(real):
        def __init__(self, *a, **k):
            made.append(1)
            super().__init__(*a, **k)
    monkeypatch.setattr(api, "BatchSimulator", Counting)
    res = api.noise(api.CircuitSweep(mc, api.Sweep(vdd=vdds)), "out", freqs, input="vg", solver="gpu")
    assert len(made) == 1 and len(res) == 3                                                   # one batch
    monkeypatch.setattr(api, "BatchSimulator", real)
    stats = res[0].stats
    assert stats["gpu_systems"] == 12 and stats["host_systems"] == 0 and all(ns.stats is stats for _, ns in res)
    host = api.noise(api.CircuitSweep(mc, api.Sweep(vdd=vdds)), "out", freqs, input="vg")     # solver="host": the loop over the points
    assert all(ns.stats == {} for _, ns in host)
    sim, st, u, G, C, Gd, Cd = linearise(mc, [{"vdd": v} for v in vdds])
    try:
        for k, v in enumerate(vdds):
            srcs = api.noise_sources(st, c, {"vdd": v}, u[k], 27.0, 1e-12)
            assert res.points[k] == {"vdd": v}
            assert_within_the_solves_bound(st, Gd[k], Cd[k], srcs, "out", 27.0, res[k], host[k])
            # the single circuit at that supply: another batch, another pivot sample -- the same two-solves bound
            single = api.noise(api.MNACircuit(c, {"vdd": v}), "out", freqs, input="vg", solver="gpu")
            assert single.stats["gpu_systems"] == 4
            assert_within_the_solves_bound(st, Gd[k], Cd[k], srcs, "out", 27.0, res[k], single)
    finally:
        sim.close()
    assert np.all(np.abs(res[0]["onoise"] / res[2]["onoise"] - 1.0) > 1e-3)                   # the supply does move the noise (PSDs ~1e-11: a relative test)


def test_a_circuit_beyond_lds_takes_the_host_path_with_auto_and_raises_with_gpu():
    """chain200 as in tests/test_gpu_ac_lu.py, linearised at the zero state (its DC solve needs the fallback ladder; the sweep does not care)"""
    from cadnip_jl_amd import hip
    mk, params = tc.CHAIN_STAMP["chain200"]
    sim, st, u, G, C, Gd, Cd = linearise(api.MNACircuit(mk(), dict(params)), at_zero=True)
    try:
        srcs = [(st.index_of("n200"), -1, "thermal", 1e-3, 0.0, "rload"), (st.index_of("n100"), st.index_of("n200"), "white", 1e-20, 0.0, "x")]
        freqs = [1e3, 1e6]
        stats = {"gpu_systems": 0, "host_systems": 0, "max_berr": 0.0, "wpb": 0}
        ns, = api.noise_solve_gpu(sim.h, st, G, C, Gd, Cd, [srcs], "n200", freqs, None, 27.0, 1e-12, "auto", stats)
        assert stats["gpu_systems"] == 0 and stats["host_systems"] == 2 and "LDS" in stats["fallback"] and ns.stats is stats
        host = api.noise_solve(st, Gd[0], Cd[0], srcs, "n200", freqs, None, 27.0)
        assert np.array_equal(ns["onoise"], host["onoise"]) and np.array_equal(ns["x"], host["x"])       # the host's result
        with pytest.raises(hip.CadnipError) as e:
            api.noise_solve_gpu(sim.h, st, G, C, Gd, Cd, [srcs], "n200", freqs, None, 27.0, 1e-12, "gpu")
        assert e.value.code == hip.BADARG
    finally:
        sim.close()
