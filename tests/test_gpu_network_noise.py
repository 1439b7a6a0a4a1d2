"""api.network_noise and api.noise(output=[...]) on the GPU (cadnip_ac_adjoint_multi under the product API): the passive pi two-ports of
tests/test_network_cpu.py against the Twiss identity, a common-source amplifier as a two-port over a supply sweep against the host path, the
memory homes against each other, and the several-output noise call against the single-output one.

Tolerances.  A GPU column and a host column are two solves of the same A^T: every entry of l_i within d = 32 cond_inf(A^T) eps max|l| of the
other (tests/test_gpu_noise_solver.py: assert_within_the_solves_bound; tests/test_gpu_ac_adjoint.py holds the kernel to 16 cond eps max|x|
of the exact solution).  Propagated: an entry of y is an entry of l -- d; a transfer T[i, s] is one entry (a grounded source: d) or the
difference of two (2 d), so an entry of cy moves by dcy = sum_s S_s (2 max|T[:, s]| dT_s + dT_s^2).  The chain form is ca = M cy M^H with
M = [[0, B], [1, D]], B = -1 / y21, D = -y11 / y21: with |dB| <= d / (|y21| (|y21| - d)) and |dD| <= d (|B| + dB) + |y11| dB, entrywise
dca = (|M| + dM)(|cy| + dcy)(|M| + dM)^T - |M| |cy| |M|^T.  rn and nf(zs) are linear in ca: drn = dca00 / (4 k T0),
dnf(zs) = |z|^T dca |z| / (4 k T0 Re zs).  nfmin is the minimum of nf over the source admittance: two functions within dnf of each other at
either one's minimiser have minima within max(dnf(1 / yopt_host), dnf(1 / yopt_gpu)) of each other, plus the 1e-9 relative to which
tests/test_network_noise_cpu.py holds nf(1 / yopt) == nfmin on each side."""
import numpy as np
import pytest

import cadnip_jl_amd as cj
from cadnip_jl_amd import api, hip
from tests import ac_ref as R
from tests import test_network_cpu as NC
from tests import test_network_noise_cpu as NN
from tests import test_gpu_noise_solver as TN

pytestmark = pytest.mark.gpu
EPS = R.EPS
GMIN = NC.GMIN
FREQS = NC.FREQS
K4T0 = 4 * api.K_BOLTZMANN * api.T0


def same(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


@pytest.mark.parametrize("coupling", ["r", "c"])
def test_pi_two_ports_satisfy_the_twiss_identity(coupling):
    circ = NC.pi_circuit(coupling)
    mc = api.MNACircuit(circ, {})
    net = api.network_noise(mc, ["v1", "v2"], FREQS, gmin=GMIN, solver="gpu")
    lin = api.ac(mc, FREQS, gmin=GMIN)                                   # G (gmin on the node diagonals) and C of the same linearisation
    assert isinstance(net, api.NetworkNoiseSol) and np.array_equal(net.dc_x, lin.dc_x)
    assert net.stats["gpu_systems"] == len(FREQS) * 2 and net.stats["host_systems"] == 0 and net.stats["rhs"] == 2 and net.stats["memory"] == "lds"
    assert 0 <= net.stats["max_berr"] <= api.NOISE_BERR_MAX
    srcs = NN.resistor_sources(lin.st, circ)
    got = api.noise_sources(lin.st, circ, {}, lin.dc_x, 27.0, 1e-12)
    assert sorted(got) == sorted(srcs)                                   # what the call itself collected
    NN.assert_twiss("gpu pi-" + coupling, lin.st, lin.G, lin.C, srcs, ["v1", "v2"], net)
    for fi, f in enumerate(FREQS):                                       # and y is network's
        ref = NC.y_pi(coupling, f)
        assert np.max(np.abs(net.y[fi] - ref)) <= 16 * R.cond_inf_c((lin.G + 2j * np.pi * f * lin.C).T) * EPS * np.max(np.abs(ref)), f
    host = api.network_noise(mc, ["v1", "v2"], FREQS, gmin=GMIN)
    assert host.stats == {} and sorted(host.cy_by_source) == sorted(net.cy_by_source)
    with pytest.raises(ValueError):
        api.network_noise(mc, ["ra"], FREQS, solver="gpu")


VDDS = [4.5, 5.0, 5.5]
AMP_FREQS = np.array([1e3, 1e8, 3e9])
AMP_PORTS = ["vg", "vout"]


def amplifier_sweep():
    """tests/test_network_noise_cpu.py's amplifier with the supply a parameter, the output port biased at 0.6 vdd -- so the supply moves the
    operating point of the device -- and a 100 kOhm gate bias resistor: the stage's one noise source at the input (without it v_n and i_n are
    fully correlated, Re(yopt) = gmin and nfmin - 1 vanishes: nothing to compare)"""
    c = NN.amplifier_circuit(cj.Param("vdd"), cj.Param("vdd", 0.6))
    c.R("rb", "in", "0", 100e3)
    mc = api.MNACircuit(c, {"vdd": 5.0})
    return c, mc, api.CircuitSweep(mc, api.Sweep(vdd=VDDS))


_AMP = {}


def amp(solver, memory="lds"):
    if (solver, memory) not in _AMP:
        _AMP[solver, memory] = api.network_noise(amplifier_sweep()[2], AMP_PORTS, AMP_FREQS, solver=solver, memory=memory)
    return _AMP[solver, memory]


def bounds(st, Gd, Cd, srcs, temp, f, y, cy):
    """(d, dcy, dca) of the module docstring at one frequency, from the host's matrices"""
    lam, d, rows = NN.adjoint_columns(st, Gd, Cd, AMP_PORTS, f)
    dcy = 0.0
    for s in srcs:
        T = (lam[s[0]] if s[0] >= 0 else 0.0) - (lam[s[1]] if s[1] >= 0 else 0.0)
        dT = d if min(s[0], s[1]) < 0 else 2 * d
        dcy += api.noise_psd(s, temp, f) * (2 * np.max(np.abs(T)) * dT + dT * dT)
    y11, y21 = abs(y[0, 0]), abs(y[1, 0])
    assert d < 0.5 * y21
    B = 1.0 / y21
    dB = d / (y21 * (y21 - d))
    dD = d * (B + dB) + y11 * dB
    aM, dM = np.array([[0.0, B], [1.0, y11 * B]]), np.array([[0.0, dB], [0.0, dD]])
    dca = (aM + dM) @ (np.abs(cy) + dcy) @ (aM + dM).T - aM @ np.abs(cy) @ aM.T
    return d, dcy, dca


def dnf(dca, zs):
    z = np.array([1.0, abs(zs)])
    return float(z @ dca @ z) / (K4T0 * np.real(zs))


def test_the_amplifier_as_a_noisy_two_port_over_a_supply_sweep():
    c, mc, cs = amplifier_sweep()
    gpu, host = amp("gpu"), amp("host")
    F = len(AMP_FREQS)
    assert len(gpu) == len(host) == 3
    st_ = gpu[0].stats
    assert st_["rhs"] == 2 and st_["host_systems"] == 0 and st_["gpu_systems"] == 3 * F * 2 and st_["memory"] == "lds" and "fallback" not in st_
    assert 0 <= st_["max_berr"] <= api.NOISE_BERR_MAX and all(n.stats is st_ for _, n in gpu) and all(n.stats == {} for _, n in host)
    sim, st, u, G, C, Gd, Cd = TN.linearise(mc, [{"vdd": v} for v in VDDS])
    try:
        for k, v in enumerate(VDDS):
            g, h = gpu[k], host[k]
            assert gpu.points[k] == {"vdd": v} and np.array_equal(g.dc_x, h.dc_x) and g.temp == h.temp == 27.0
            assert isinstance(g, api.NetworkNoiseSol) and g.y.shape == g.cy.shape == (F, 2, 2) and list(g.cy_by_source) == list(h.cy_by_source)
            srcs = api.noise_sources(st, c, {"vdd": v}, u[k], 27.0, 1e-12)
            assert sorted({s[5] for s in srcs}) == ["m1", "rb", "rd"] == sorted(g.cy_by_source)
            g_nfmin, h_nfmin, g_rn, h_rn, g_yopt, h_yopt = g.nfmin, h.nfmin, g.rn, h.rn, g.yopt, h.yopt
            for fi, f in enumerate(AMP_FREQS):
                d, dcy, dca = bounds(st, Gd[k], Cd[k], srcs, 27.0, f, h.y[fi], h.cy[fi])
                print("vdd %.1f f %.0e  |dy| %.3g (d %.3g)  |dcy| %.3g (%.3g)  |drn| %.3g (%.3g)  |dnfmin| %.3g  nfmin %.6f rn %.4g" % (
                    v, f, np.max(np.abs(g.y[fi] - h.y[fi])), d, np.max(np.abs(g.cy[fi] - h.cy[fi])), dcy, abs(g_rn[fi] - h_rn[fi]), dca[0, 0] / K4T0,
                    abs(g_nfmin[fi] - h_nfmin[fi]), h_nfmin[fi], h_rn[fi]))
                assert np.max(np.abs(g.y[fi] - h.y[fi])) <= d, (v, f)
                assert np.max(np.abs(g.cy[fi] - h.cy[fi])) <= dcy, (v, f)
                assert np.max(np.abs(sum(p[fi] for p in g.cy_by_source.values()) - g.cy[fi])) <= 8 * EPS * np.max(np.abs(g.cy[fi]))
                assert abs(g_rn[fi] - h_rn[fi]) <= dca[0, 0] / K4T0, (v, f)
                for zs in (50.0, 200.0 + 300.0j, 1.0 / h_yopt[fi]):
                    assert abs(g.nf(zs)[fi] - h.nf(zs)[fi]) <= dnf(dca, zs), (v, f, zs)
                tol = max(dnf(dca, 1.0 / h_yopt[fi]), dnf(dca, 1.0 / g_yopt[fi])) + 2e-9 * h_nfmin[fi]
                assert abs(g_nfmin[fi] - h_nfmin[fi]) <= tol, (v, f)
                assert h_nfmin[fi] > 1.0 and h_rn[fi] > 0 and h_yopt[fi].real > 0
    finally:
        sim.close()
    assert len({float(np.round(gpu[k].y[0, 1, 0].real, 9)) for k in range(3)}) == 3          # the supply moves the transconductance


def test_memory_hbm_gives_the_same_cy_to_the_bit():
    lds, hbm = amp("gpu"), amp("gpu", "hbm")
    auto = api.network_noise(amplifier_sweep()[2], AMP_PORTS, AMP_FREQS, solver="auto", memory="auto", z0=[75.0, 50.0])
    assert lds[0].stats["memory"] == "lds" and hbm[0].stats["memory"] == "hbm" and auto[0].stats["memory"] == "lds" and hbm[0].stats["host_systems"] == 0
    for k in range(3):
        assert same(hbm[k].cy, lds[k].cy) and same(hbm[k].y, lds[k].y) and same(auto[k].cy, lds[k].cy)
        assert all(same(hbm[k].cy_by_source[nm], lds[k].cy_by_source[nm]) for nm in lds[k].cy_by_source)
        assert np.array_equal(auto[k].nf(), lds[k].nf(75.0))
    with pytest.raises(ValueError):
        api.network_noise(amplifier_sweep()[2], AMP_PORTS, AMP_FREQS, solver="gpu", memory="l2")


def counting(monkeypatch):
    calls = {"ac_adjoint": 0, "ac_adjoint_multi": 0}
    for nm in calls:
        real = getattr(hip.Handle, nm)

        def wrapped(self, *a, _real=real, _nm=nm, **k):
            calls[_nm] += 1
            return _real(self, *a, **k)
        monkeypatch.setattr(hip.Handle, nm, wrapped)
    return calls


def same_noise(a, b):
    return (same(a.onoise, b.onoise) and same(a.gain, b.gain) and same(a.inoise, b.inoise) and list(a.contributions) == list(b.contributions)
            and all(same(a.contributions[nm], b.contributions[nm]) for nm in a.contributions) and a.output == b.output and a.temp == b.temp)


def test_noise_at_several_outputs_is_one_call_and_each_output_the_single_call_to_the_bit(monkeypatch):
    mc = api.MNACircuit(TN.common_source(), {})
    freqs = np.array([1.0, 1e3, 1e6])
    outputs = ["out", "in", "I_vdd"]
    calls = counting(monkeypatch)
    many = api.noise(mc, outputs, freqs, input="vg", solver="gpu")
    assert calls == {"ac_adjoint": 0, "ac_adjoint_multi": 1}                              # ONE call for the class
    assert isinstance(many, dict) and list(many) == outputs
    stats = many["out"].stats
    assert stats["rhs"] == 3 and stats["gpu_systems"] == 3 * len(freqs) and stats["host_systems"] == 0 and all(ns.stats is stats for ns in many.values())
    for o in outputs:
        single = api.noise(mc, o, freqs, input="vg", solver="gpu")
        assert isinstance(single, api.NoiseSol) and "rhs" not in single.stats and same_noise(many[o], single), o
    assert calls == {"ac_adjoint": 3, "ac_adjoint_multi": 1}                              # a string is today's call, down to the entry point
    assert np.all(many["out"]["onoise"] > 0) and np.all(many["in"]["onoise"] <= 1e-20 * many["out"]["onoise"])     # the input node is held by its source
    hostd = api.noise(mc, outputs, freqs, input="vg")
    assert list(hostd) == outputs and calls == {"ac_adjoint": 3, "ac_adjoint_multi": 1}
    for o in outputs:
        assert hostd[o].stats == {} and same_noise(hostd[o], api.noise(mc, o, freqs, input="vg"))
    for bad in ([], ["out", "out"]):
        with pytest.raises(ValueError):
            api.noise(mc, bad, freqs, solver="gpu")
    with pytest.raises(KeyError):
        api.noise(mc, ["out", "nope"], freqs, solver="gpu")


def test_several_outputs_over_a_sweep_without_an_input():
    c = TN.common_source(cj.Param("vdd"))
    cs = api.CircuitSweep(api.MNACircuit(c, {"vdd": 5.0}), api.Sweep(vdd=VDDS))
    freqs = np.array([1e2, 1e5])
    many = api.noise(cs, ["out", "I_vdd"], freqs, solver="gpu", memory="hbm")
    one = api.noise(cs, "out", freqs, solver="gpu")
    assert len(many) == 3 and many[0]["out"].stats["memory"] == "hbm" and many[0]["out"].stats["gpu_systems"] == 3 * 2 * 2
    for k in range(3):
        assert list(many[k]) == ["out", "I_vdd"] and same_noise(many[k]["out"], one[k]) and many[k]["out"].input is None
