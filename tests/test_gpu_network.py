"""api.network and api.ac(..., sources=) on the GPU (cadnip_ac_solve_multi under the product API): the pi two-ports of
tests/test_network_cpu.py against their closed forms, the sp_mos1 inverter of tests/ac_ref.py as a two-port (input source, supply source)
over a supply sweep against the host path, the two new interfaces against each other, and the memory homes against each other.

Tolerances: a GPU column and a host column are two solves of the same system A = G + j w C, each within tests/ac_ref.py's forward bound
16 cond_inf(A) eps max|ref| of the exact solution (tests/test_gpu_ac_lu.py holds the kernel to it); against a closed form that bound
applies once, between the two solves twice."""
import numpy as np
import pytest

from cadnip_jl_amd import api
from tests import ac_ref as R
from tests import test_network_cpu as NC

pytestmark = pytest.mark.gpu
EPS = R.EPS
GMIN = NC.GMIN
FREQS = NC.FREQS


@pytest.mark.parametrize("coupling", ["r", "c"])
def test_pi_two_ports_against_their_closed_forms(coupling):
    mc = api.MNACircuit(NC.pi_circuit(coupling), {})
    net = api.network(mc, ["v1", "v2"], FREQS, gmin=GMIN, solver="gpu")
    lin = api.ac(mc, FREQS, gmin=GMIN)                                   # G (gmin on the node diagonals) and C of the same linearisation
    assert isinstance(net, api.NetworkSol) and net.y.shape == (3, 2, 2) and np.array_equal(net.dc_x, lin.dc_x)
    assert net.stats["gpu_systems"] == len(FREQS) * 2 and net.stats["host_systems"] == 0 and net.stats["rhs"] == 2 and net.stats["memory"] == "lds"
    for fi, f in enumerate(FREQS):
        ref = NC.y_pi(coupling, f)
        bound = 16 * R.cond_inf_c(lin.G + 2j * np.pi * f * lin.C) * EPS * np.max(np.abs(ref))
        print("pi-%s f %.0e  err %.3g  bound %.3g" % (coupling, f, np.max(np.abs(net.y[fi] - ref)), bound))
        assert np.max(np.abs(net.y[fi] - ref)) <= bound, f
        assert net.y[fi, 0, 0].real > 0                                  # the current into the port
    host = api.network(mc, ["v1", "v2"], FREQS, gmin=GMIN)
    assert host.stats == {} and np.max(np.abs(host.y - net.y)) <= 2 * 16 * max(R.cond_inf_c(lin.G + 2j * np.pi * f * lin.C) for f in FREQS) * EPS * np.max(np.abs(host.y))


def inverter_sweep():
    mk, base, pts, grid = R.CASES["inverter"]
    return api.CircuitSweep(api.MNACircuit(mk(), dict(base)), api.Sweep(vdd=[p["vdd"] for p in pts])), np.asarray(grid())[[0, len(grid()) // 2, -1]]


def test_the_inverter_as_a_two_port_over_a_supply_sweep():
    cs, freqs = inverter_sweep()
    ports = ["vin", "vdd"]                                               # input and supply: both V sources of tc.cmos_inverter_ac
    gpu = api.network(cs, ports, freqs, solver="gpu")
    host = api.network(cs, ports, freqs)
    one = api.ac(cs, freqs, solver="gpu", sources=["vin"])
    assert len(gpu) == len(host) == len(one) == 3 and len(freqs) == 3
    st = gpu[0].stats
    assert st["gpu_systems"] + st["host_systems"] == 3 * len(freqs) * 2 and st["rhs"] == 2 and st["host_systems"] == 0
    assert one[0]["vin"].stats["gpu_systems"] == 3 * len(freqs) and one[0]["vin"].stats["rhs"] == 1
    for i in range(3):
        sol = one[i]["vin"]
        assert isinstance(one[i], dict) and list(one[i]) == ["vin"] and isinstance(sol, api.ACSol)
        assert np.array_equal(gpu[i].dc_x, host[i].dc_x) and gpu[i].y.shape == (len(freqs), 2, 2)
        for fi, f in enumerate(freqs):
            kappa = R.cond_inf_c(sol.G + 2j * np.pi * f * sol.C)         # this point's A
            bound = 16 * kappa * EPS * np.max(np.abs(host[i].y[fi]))
            print("inverter point %d f %.3g  |gpu - host| %.3g  bound %.3g" % (i, f, np.max(np.abs(gpu[i].y[fi] - host[i].y[fi])), bound))
            assert np.max(np.abs(gpu[i].y[fi] - host[i].y[fi])) <= bound, (i, f)
        # the two interfaces: column `vin` of the network IS the response to vin alone -- the same kernel, the same column, the same doubles
        assert list(sol._cache) == [tuple(2 * np.pi * freqs)]
        assert np.array_equal(gpu[i].y[:, 1, 0], -sol["I_vdd"]) and np.array_equal(gpu[i].y[:, 0, 0], -sol["I_vin"])
        assert np.all(np.abs(gpu[i].y[:, 1, 0]) > 0)
    assert len({complex(np.round(gpu[i].y[0, 1, 0], 12)) for i in range(3)}) == 3          # the supply moves the transadmittance


def test_ac_without_sources_is_what_it_was_and_with_sources_solves_each_alone():
    """The pin for the unchanged ``sources=None`` path is tests/test_gpu_ac.py's own bar -- the Butterworth transfer function at rtol 1e-9 --
    plus ``array_equal`` between that path and the new V1-alone column, which is the same excitation through the multi-column kernel."""
    mk, base, pts, grid = R.CASES["butterworth"]
    mc = api.MNACircuit(mk(), dict(base))
    freqs = np.asarray(grid())[::15]
    sol = api.ac(mc, freqs, solver="gpu")
    assert isinstance(sol, api.ACSol) and not isinstance(sol, dict) and sol.stats["gpu_systems"] == len(freqs) and "rhs" not in sol.stats
    got = api.ac(mc, freqs, solver="gpu", sources=["V1"])
    assert isinstance(got, dict) and list(got) == ["V1"] and got["V1"].stats["rhs"] == 1
    # V1 carries AC 1: alone at unit magnitude it is the circuit's own excitation -- the single-column kernel's doubles
    assert np.array_equal(got["V1"].b_ac, sol.b_ac) and np.array_equal(got["V1"]["vout"], sol["vout"])
    hostd = api.ac(mc, freqs, sources=["V1"])
    assert hostd["V1"].stats == {} and not hostd["V1"]._cache
    H = R.butterworth_h(2 * np.pi * freqs)
    assert np.allclose(hostd["V1"]["vout"], H, rtol=1e-9, atol=0.0) and np.allclose(got["V1"]["vout"], H, rtol=1e-9, atol=0.0)   # tests/test_gpu_ac.py's bar
    for bad in (["R4"], ["nope"]):
        with pytest.raises(ValueError):
            api.ac(mc, freqs, sources=bad)
    with pytest.raises(ValueError):
        api.network(mc, ["R4"], freqs)


def test_memory_hbm_gives_the_same_y_to_the_bit():
    cs, freqs = inverter_sweep()
    lds = api.network(cs, ["vin", "vdd"], freqs, solver="gpu")
    hbm = api.network(cs, ["vin", "vdd"], freqs, solver="gpu", memory="hbm")
    auto = api.network(cs, ["vin", "vdd"], freqs, solver="auto", memory="auto", z0=[50.0, 75.0])
    assert lds[0].stats["memory"] == "lds" and hbm[0].stats["memory"] == "hbm" and auto[0].stats["memory"] == "lds"
    for i in range(3):
        assert np.array_equal(hbm[i].y.view(np.float64), lds[i].y.view(np.float64)) and np.array_equal(auto[i].y.view(np.float64), lds[i].y.view(np.float64))
        assert np.array_equal(auto[i].z0, [50.0, 75.0]) and np.all(np.isfinite(auto[i].s))
    with pytest.raises(ValueError):
        api.network(cs, ["vin"], freqs, solver="gpu", memory="l2")
