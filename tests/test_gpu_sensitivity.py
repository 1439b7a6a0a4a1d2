"""api.sensitivity on the GPU: the perturbed resident batch (DC solves, restamp) with the host path, and solver="gpu" (cadnip_ac_sens, one call
per structure class) against it.  The circuit is the sp_mos1 inverter of tests/ac_ref.py over three supplies, its parameters vdd and the
temperature, three frequencies: 9 systems."""
import numpy as np
import pytest

import cadnip_jl_amd as cj
from cadnip_jl_amd import api
from tests import ac_ref as R
from tests import sens_ref as SR

pytestmark = pytest.mark.gpu
EPS = R.EPS
GMIN = 1e-12
VDDS = [3.0, 3.3, 3.6]
FREQS = np.array([1e3, 1e8, 1e10])
PARAMS = ["vdd", "temp"]
REL = 1e-4
DC_ABSTOL = 1e-10                      # BatchSimulator.dc's default: the Newton update every unknown has converged to
_RUNS = {}


def circuit():
    return api.MNACircuit(R.inverter_with_param_vdd(), {"vdd": 3.3})


def run(solver, memory="lds"):
    key = (solver, memory)
    if key not in _RUNS:
        _RUNS[key] = api.sensitivity(api.CircuitSweep(circuit(), api.Sweep(vdd=VDDS)), "vout", PARAMS, FREQS, rel_step=REL, solver=solver, memory=memory)
    return _RUNS[key]


def test_gpu_against_host_within_the_bound_of_the_forms():
    """Both calls build the same batch and meet the same stamps; what differs is the solve.  The bound d_s (tests/sens_ref.py) is evaluated on
    the CPU port's systems at the same 15 points -- it depends on magnitudes and condition numbers, which the two paths share to many digits."""
    host, gpu = run("host"), run("gpu")
    assert len(gpu) == 3 and gpu[0].stats["gpu_systems"] == 9 and gpu[0].stats["host_systems"] == 0 and gpu[0].stats["params"] == 2
    assert gpu[0].stats["memory"] == "lds" and gpu[0].stats["wpb"] in (1, 2, 4, 8) and gpu[0].stats["max_berr"] <= api.AC_BERR_MAX
    assert host[0].stats == {}
    pts = []
    for v in VDDS:
        dv, dT = REL * v, REL * (27.0 + 273.15)
        pts += [{"vdd": v}, {"vdd": v + dv}, {"vdd": v - dv}, {"vdd": v, "temp": 27.0 + dT}, {"vdd": v, "temp": 27.0 - dT}]
    st, G, C, bac, _ = SR.port_points("inverter", pts)
    out = (st.index_of("vout"), -1)
    for i, v in enumerate(VDDS):
        h, g = host[i], gpu[i]
        assert g.params == PARAMS and np.array_equal(g.values, [v, 27.0]) and np.allclose(g.steps, [REL * v, REL * 300.15], rtol=1e-15)
        assert np.array_equal(g.steps, h.steps) and abs(g.dc_value - h.dc_value) <= 16 * DC_ABSTOL     # two runs of the same DC solves
        assert np.all(np.abs(g.dc_dy - h.dc_dy) <= 16 * 4 * DC_ABSTOL / (2.0 * g.steps))
        for f, w in enumerate(2.0 * np.pi * FREQS):
            A = R.system(st, G[5 * i], C[5 * i], w, GMIN)
            dA = np.array([(R.dense_csr(st, G[5 * i + 1 + 2 * k] - G[5 * i + 2 + 2 * k]) + 1j * w * R.dense_csr(st, C[5 * i + 1 + 2 * k] - C[5 * i + 2 + 2 * k]))
                           / (2.0 * g.steps[k]) for k in range(2)])
            ref, x, lam, wk = SR.direct_form(A, bac[5 * i], dA, None, out)
            assert abs(g.y[f] - h.y[f]) <= 16 * R.cond_inf_c(A) * EPS * np.max(np.abs(x))          # the forward bound of tests/test_gpu_ac_lu.py
            for k in range(2):
                d = SR.d_s(A, x, lam, dA[k], wk[k])
                print("vdd %.1f f %.0e %s  dy gpu %r host %r  diff %.3g  d_s %.3g  (port direct form %r)" % (
                    v, FREQS[f], PARAMS[k], g.dy[f, k], h.dy[f, k], abs(g.dy[f, k] - h.dy[f, k]), d, ref[k]))
                assert abs(g.dy[f, k] - h.dy[f, k]) <= d, (i, f, k)
                assert g.dy[f, k] != 0


def test_y_is_the_ac_response():
    """ac(..., solver="gpu") solves the same points in a batch of 3 instead of 15: another pivot sample, so another order, and Newton runs of
    its own.  Every unknown of a DC point is converged to DC_ABSTOL; the response moves with a node voltage about as it moves with the supply
    (dy/dvdd, which this very call provides), and n unknowns may each be off: |dy| <= 16 n DC_ABSTOL |dy/dvdd|, plus the solves' own rounding."""
    gpu = run("gpu")
    ac = api.ac(api.CircuitSweep(circuit(), api.Sweep(vdd=VDDS)), FREQS, solver="gpu")
    for i in range(3):
        n = ac[i].st.n
        assert np.all(np.abs(gpu[i].y - ac[i]["vout"]) <= 16 * n * DC_ABSTOL * np.abs(gpu[i].dy[:, 0]) + 1e-12 * np.abs(gpu[i].y)), i
        assert abs(gpu[i].dc_value - ac[i].dc_x[ac[i].st.index_of("vout")]) <= 16 * n * DC_ABSTOL * max(abs(gpu[i].dc_dy[0]), 1.0)


def test_dc_dy_is_the_slope_of_the_operating_point():
    """Two converged solves differenced over 2 delta: each end within DC_ABSTOL, on both sides of the comparison -- 4 DC_ABSTOL / (2 delta), times 16."""
    gpu = run("gpu")
    v, d = VDDS[1], REL * VDDS[1]
    sols = api.dc(api.CircuitSweep(circuit(), api.Sweep(vdd=[v - d, v + d])), continuation=False)
    slope = (sols[1]["vout"] - sols[0]["vout"]) / (2 * d)
    print("dc_dy %r slope %r" % (gpu[1].dc_dy[0], slope))
    assert abs(gpu[1].dc_dy[0] - slope) <= 16 * 4 * DC_ABSTOL / (2 * d) and slope != 0


def test_hbm_gives_the_same_doubles():
    lds, hbm = run("gpu"), run("gpu", "hbm")
    assert hbm[0].stats["memory"] == "hbm" and hbm[0].stats["gpu_systems"] == 9
    for a, b in zip(lds.solutions, hbm.solutions):
        assert np.array_equal(a.dy.view(np.float64), b.dy.view(np.float64)) and np.array_equal(a.y.view(np.float64), b.y.view(np.float64))
    auto = api.sensitivity(circuit(), ("vout", "0"), "vdd", FREQS, solver="auto", memory="auto")       # one circuit, a pair, one name
    assert auto.stats["memory"] == "lds" and auto.stats["gpu_systems"] == 3 and auto.dy.shape == (3, 1)
    k = 0
    assert np.array_equal(auto.normalized("vdd"), 3.3 * auto.dy[:, k])
    assert np.allclose(auto.dmag(k), np.real(np.conj(auto.y) * auto.dy[:, k]) / np.abs(auto.y), rtol=1e-15)
    assert np.allclose(auto.dphase("vdd"), np.imag(auto.dy[:, k] / auto.y), rtol=1e-15)


def test_a_step_across_a_structure_class_raises():
    circ = cj.Circuit("rd at zero")
    circ.V("vd", "d", "0", dc=2.0)
    circ.V("vg", "g", "0", dc=cj.Param("vg"), ac=1.0)
    circ.MOS1("m1", "d", "g", "0", "0", dict(type=1, vto=0.7, kp=100e-6, rd=cj.Param("rd")), w=10e-6, l=1e-6)
    mc = api.MNACircuit(circ, {"rd": 0.0, "vg": 1.5})
    with pytest.raises(ValueError, match="rd"):
        api.sensitivity(mc, "I_vd", ["rd"], [1e3], solver="gpu")
    sol = api.sensitivity(mc, "I_vd", ["vg"], [1e3], solver="gpu")                  # the other parameter is fine: the transconductance
    assert sol.stats["gpu_systems"] == 1 and abs(sol.dc_dy[0]) > 0
