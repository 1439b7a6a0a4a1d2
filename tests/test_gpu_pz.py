"""api.pz on the GPU: solver="gpu" (one cadnip_ac_arnoldi call per structure class, csrc/ac_lu.hip: k_ac_arnoldi) against solver="host" (the
dense pencils) on the linear circuits of tests/pz_ref.py, a CircuitSweep over the inverter's supply, the memory homes, the "auto" fallback, the
redo gate, and the flip-flop with one shift per decade of its grid.  Bound of a GPU pole against the dense pencil, relative to |p - j w0|:
16 x the worst error the numpy port leaves on the same case, and not below 64 eps."""
import numpy as np
import pytest

import cadnip_jl_amd as cj
from cadnip_jl_amd import api, hip
from tests import ac_ref as R
from tests import circuits as tc
from tests import pz_ref as Z
from tests.test_pz_cpu import hook, DFF_MIN_ACCEPTED

pytestmark = pytest.mark.gpu
EPS = R.EPS
GMIN = 1e-12


def port_solution(st, G, C, b, out, omegas, m):
    c = np.zeros(st.n)
    c[out] = 1.0
    return api.pz_solve(st, G, C, b, (out, -1), omegas, m, hook(G, C, b, c[None], m))[0]


@pytest.mark.parametrize("name", ["butterworth", "ladder8", "leadlag"])
def test_gpu_against_host_on_the_linear_circuits(name):
    mk, out = Z.LINEAR[name]
    mc = api.MNACircuit(mk(), {})
    host = api.pz(mc, out)
    f0 = float(abs(host.poles[0])) / (2.0 * np.pi)
    shifts = [0.0 if name != "butterworth" else f0 / 8, f0]         # (the filter's A is singular at 0: that system would be flagged and redone, see below)
    gpu = api.pz(mc, out, shifts=shifts, order=16, solver="gpu")
    st, G, C, b, c = Z.linear_system(name)
    port = port_solution(st, G, C, b, st.index_of(out), 2.0 * np.pi * np.array(shifts), min(16, st.n))
    w_of = lambda sol: 2.0 * np.pi * sol.pole_shift
    bound = max(16 * float(Z.match_error(port.poles, host.poles, port.pole_shift).max()), 64 * EPS)
    err = Z.match_error(gpu.poles, host.poles, w_of(gpu))
    print("%s: gpu pole errors %s bound %.3g stats %s" % (name, err, bound, gpu.stats))
    assert len(gpu.poles) == len(host.poles) == len(port.poles) and np.all(err <= bound)
    assert np.all(Z.match_error(host.poles, gpu.poles, 0.0) <= bound * np.abs(host.poles).max() / np.abs(host.poles).min())     # every host pole was found
    assert len(gpu.zeros) == len(host.zeros) == (1 if name == "leadlag" else 0)
    if len(host.zeros):
        zb = max(16 * float(Z.match_error(port.zeros, host.zeros).max()), 64 * EPS)
        assert np.all(Z.match_error(gpu.zeros, host.zeros) <= zb)
    gb = max(16 * abs(port.gain - host.gain), 64 * EPS * abs(host.gain))
    assert abs(gpu.gain - host.gain) <= gb
    s = gpu.stats
    assert s["gpu_systems"] == 2 and s["host_systems"] == 0 and s["breakdowns"] == 2 and s["order"] == 16 and s["shifts"] == 2 and s["wpb"] in (1, 2, 4, 8)
    assert s["max_berr"] <= api.AC_BERR_MAX and "fallback" not in s
    H, beta, l = gpu.reduced(shifts[1])
    assert H.shape[0] == len(host.poles) + 1 and np.all(gpu.pole_resid == 0.0) and set(gpu.pole_shift) <= set(shifts)
    if name == "butterworth":
        exact = np.array([-1.0, -0.5 + 0.5j * np.sqrt(3.0), -0.5 - 0.5j * np.sqrt(3.0)])
        assert np.all(Z.match_error(gpu.poles, exact, w_of(gpu)) <= bound + 16 * GMIN)          # gmin moves a pole by its order
    hbm = api.pz(mc, out, shifts=shifts, order=16, solver="gpu", memory="hbm")
    assert hbm.stats["memory"] == "hbm" and np.array_equal(hbm.poles, gpu.poles) and np.array_equal(hbm.zeros, gpu.zeros) and hbm.gain == gpu.gain
    named = api.pz(mc, out, input="vin" if name != "butterworth" else "V1", shifts=shifts, solver="gpu")     # ac = 1 on that source: the same excitation
    assert np.array_equal(named.poles, gpu.poles) and named.gain == gpu.gain


def test_a_sweep_gives_one_result_per_point_equal_to_single_calls():
    mk, base, pts, _ = R.CASES["inverter"]
    circ = mk()
    mc = api.MNACircuit(circ, dict(base))
    vdds = [p["vdd"] for p in pts]
    shifts = [0.0, 1e7]
    res = api.pz(api.CircuitSweep(mc, api.Sweep(vdd=vdds)), "vout", shifts=shifts, solver="gpu")
    host = api.pz(api.CircuitSweep(mc, api.Sweep(vdd=vdds)), "vout")
    sols, hs = list(res.solutions), list(host.solutions)
    assert len(sols) == 3 and sols[0].stats["gpu_systems"] == 6 and sols[0].stats["host_systems"] == 0
    for k, v in enumerate(vdds):
        one = api.pz(api.alter(mc, vdd=v), "vout", shifts=shifts, solver="gpu")
        assert len(one.poles) == len(sols[k].poles) == len(hs[k].poles) == 1
        assert np.allclose(one.poles, sols[k].poles, rtol=1e-6, atol=0) and np.isclose(one.gain, sols[k].gain, rtol=1e-6)     # another batch: the DC point agrees to its Newton tolerance
        assert np.all(Z.match_error(sols[k].poles, hs[k].poles, 2.0 * np.pi * sols[k].pole_shift) <= 1e-9)
        assert np.isclose(sols[k].gain, hs[k].gain, rtol=1e-9) and sols[k].dc_x is not None
    assert len({complex(s.poles[0]) for s in sols}) == 3             # the supply moves the pole


def test_auto_falls_back_for_a_circuit_lds_refuses_and_says_why():
    """chain200 as in tests/test_gpu_ac_lu.py, linearised at the zero state (its DC solve needs the fallback ladder; the reduction does not care)"""
    mk, params = tc.CHAIN_STAMP["chain200"]
    sim = api.BatchSimulator(api.MNACircuit(mk(), dict(params), api.MNASpec(mode="dcop")))
    try:
        st = sim.st
        sim.analyze()
        sim.h.set_spec(mode="dcop")
        sim.h.rebuild(np.zeros(st.n), 0.0)
        G, C, _, _ = sim.h.get_GCb()
        rhs, out, om = api.source_rhs(st, sim.mc.circuit, "vin")[None], (st.index_of("n1"), -1), 2.0 * np.pi * np.array([1e6])
        new = lambda: {"gpu_systems": 0, "host_systems": 0, "max_berr": 0.0, "wpb": 0}
        with pytest.raises(hip.CadnipError):
            api.pz_gpu_sweep(sim.h, st, G, C, rhs, out, om, 2, GMIN, "gpu", new())
        stats = new()
        assert api.pz_gpu_sweep(sim.h, st, G, C, rhs, out, om, 2, GMIN, "auto", stats) is None
        assert "fallback" in stats and stats["gpu_systems"] == 0 and stats["host_systems"] == 1
        stats = new()
        got = api.pz_gpu_sweep(sim.h, st, G, C, rhs, out, om, 2, GMIN, "auto", stats, memory="auto")      # device memory takes it
        assert "fallback" not in stats and stats["memory"] == "hbm" and stats["gpu_systems"] == 1 and not got[4].any()
        to_ref = np.asarray(st.to_ref_nz)
        Gd, Cd = R.system(st, G[0, to_ref], C[0, to_ref], 0.0, GMIN).real, R.dense_csr(st, C[0, to_ref])
        c = np.zeros((1, st.n))
        c[0, out[0]] = 1.0
        Hh, bh, mh, lh = api.arnoldi_host(Gd, Cd, rhs[0], om[0], 2, c)
        # (every transistor is off at the zero state: the space is all but closed after one step, and only that step is compared)
        assert got[2][0, 0] >= 1 and np.isclose(got[0][0, 0, 0, 0], Hh[0, 0], rtol=1e-6) and np.isclose(got[1][0, 0], bh, rtol=1e-9)
    finally:
        sim.close()


def test_a_flagged_system_is_redone_on_the_host():
    """A capacitor-only node with gmin = 0: at the shift 0 its pivot is zero, the kernel flags the system, and the host Arnoldi -- whose dense
    LU meets the same singular matrix -- is what pz reports for it; the other shift stays on the GPU."""
    circ = cj.Circuit("capacitor-only node")
    circ.V("v1", "a", "0", dc=0.0, ac=1.0)
    circ.R("r1", "a", "b", 1e3)
    circ.C("c1", "b", "c", 1e-9)
    circ.C("c2", "c", "0", 1e-9)
    calls = []
    real = api.arnoldi_host
    api.arnoldi_host = lambda *a, **k: (calls.append(a[3]), real(*a, **k))[1]
    try:
        with np.errstate(all="ignore"):
            import warnings
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                sol = api.pz(api.MNACircuit(circ, {}), "b", shifts=[0.0, 1e3], order=3, gmin=0.0, solver="gpu")
    finally:
        api.arnoldi_host = real
    assert sol.stats["host_systems"] == 1 and sol.stats["gpu_systems"] == 1 and calls == [0.0]
    assert len(sol.poles) == 1 and abs(sol.poles[0] + 1.0 / (1e3 * 0.5e-9)) <= 1e-9 * 2e6 and sol.pole_shift[0] == 1e3


def test_the_flip_flops_poles_are_the_ports_and_the_dense_pencils():
    mk, base, pts, grid = R.CASES["dff"]
    circ = mk()
    shifts = np.logspace(3, 12, 10)                                  # one per decade of the case's grid
    from tests.port_util import make_port, analyze_port
    for k, pt in enumerate(pts):
        p = dict(base)
        p.update({kk: v for kk, v in pt.items() if kk != "temp"})
        mc = api.MNACircuit(circ, p, api.MNASpec(temp=pt.get("temp", 27.0)))
        gpu = api.pz(mc, Z.MOS_OUT["dff"], shifts=shifts, order=16, solver="gpu")
        st, cpu = make_port(circ, p, pt.get("temp", 27.0), "dcop")                              # the reference's matrices: the CPU port's stamps at the SAME operating point
        analyze_port(st, cpu, 5.5)
        Gc, Cc, _, _ = cpu.rebuild(gpu.dc_x, 0.0)
        cpu.close()
        out = st.index_of(Z.MOS_OUT["dff"])
        G, C = R.system(st, Gc, Cc, 0.0, GMIN).real, R.dense_csr(st, np.asarray(Cc, dtype=float))
        port = port_solution(st, G, C, api.rhs_ac(st, circ, p), out, 2.0 * np.pi * shifts, 16)
        dense = api.poles_dense(G, C)
        bound = max(16 * float(Z.match_error(port.poles, dense, port.pole_shift).max()), 64 * EPS)
        err = Z.match_error(gpu.poles, dense, 2.0 * np.pi * gpu.pole_shift)
        print("dff corner %d: gpu accepts %d, port %d; worst gpu error %.3g bound %.3g; stats %s" % (k, len(gpu.poles), len(port.poles), err.max(), bound, gpu.stats))
        assert np.all(gpu.pole_resid <= api.PZ_RESID_MAX) and np.all(err <= bound)
        assert len(gpu.poles) >= len(port.poles) >= DFF_MIN_ACCEPTED
        # the same set: a pole of the port and its nearest GPU pole lie within the bound of one pole of the dense pencil, each relative to its shift
        wp, wg = port.pole_shift, 2.0 * np.pi * gpu.pole_shift                    # (pz_solve names shifts in rad/s, pz in hertz)
        for pp, w0 in zip(port.poles, wp):
            q = int(np.argmin(np.abs(gpu.poles - pp)))
            assert abs(gpu.poles[q] - pp) <= bound * (abs(pp - 1j * w0) + abs(gpu.poles[q] - 1j * wg[q])), (pp, gpu.poles[q])
        assert gpu.stats["gpu_systems"] == 10 and gpu.stats["host_systems"] == 0
