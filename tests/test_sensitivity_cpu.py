"""api.sensitivity_solve -- the host path of api.sensitivity, the adjoint form dy/dp = lambda^T (db - dA x) in dense numpy -- against closed
forms, against the direct form e^T A^-1 (db - dA x) in extended precision (tests/sens_ref.py), and against a Richardson-extrapolated difference
quotient of the response itself on a nonlinear circuit; and the argument handling of api.sensitivity, which needs no GPU.  The systems are the
CPU port's (tests/ac_ref.py)."""
import types

import numpy as np
import pytest

import cadnip_jl_amd as cj
from cadnip_jl_amd import api, hip
from tests import ac_ref as R
from tests import noise_ref as N
from tests import sens_ref as SR

EPS = R.EPS
GMIN = 1e-12


def rc_system(Rv, Cv):
    """V1 in 0 ac=1; R in out; C out 0.  Unknowns [V(in), V(out), I(V1)]: KCL in, KCL out, the source row.  G and C as functions of (R, C)."""
    G = np.array([[1.0 / Rv, -1.0 / Rv, 1.0], [-1.0 / Rv, 1.0 / Rv, 0.0], [1.0, 0.0, 0.0]])
    Cm = np.zeros((3, 3))
    Cm[1, 1] = Cv
    return G, Cm


def test_rc_low_pass_closed_forms():
    """y = V(out) = 1 / (1 + j w R C): dy/dR = -j w C / (1 + j w R C)^2, dy/dC = -j w R / (1 + j w R C)^2, both 0 at w = 0.  dG / dC are
    central differences at rel_step e = 1e-5, as api.sensitivity forms them.  The bound: the central difference of 1 / R has a relative
    truncation error e^2 (that of C none: the stamp is linear in it) and a rounding error about eps / e (an eps-sized error of each stamp
    over a step of relative size e); the solves add their forward error, hence max(1, cond_inf(A)); 16 as everywhere in this project."""
    Rv, Cv, e = 1e3, 1e-9, 1e-5
    st = types.SimpleNamespace(n=3)
    b = np.array([0.0, 0.0, 1.0], dtype=complex)
    G0, C0 = rc_system(Rv, Cv)
    dR, dCs = e * Rv, e * Cv
    dG = np.array([(rc_system(Rv + dR, Cv)[0] - rc_system(Rv - dR, Cv)[0]) / (2 * dR), np.zeros((3, 3))])
    dC = np.array([np.zeros((3, 3)), (rc_system(Rv, Cv + dCs)[1] - rc_system(Rv, Cv - dCs)[1]) / (2 * dCs)])
    om = np.array([0.0, 1.0, 100.0]) / (Rv * Cv)
    y, dy = api.sensitivity_solve(st, G0, C0, b, dG, dC, None, (1, -1), om)
    for f, w in enumerate(om):
        den = 1.0 + 1j * w * Rv * Cv
        ref = np.array([-1j * w * Cv / den ** 2, -1j * w * Rv / den ** 2])
        bound = 16 * (e ** 2 + EPS / e) * max(1.0, R.cond_inf_c(G0 + 1j * w * C0))
        assert abs(y[f] - 1.0 / den) <= bound * abs(1.0 / den)
        for k in range(2):
            print("rc w RC %g k %d  got %r ref %r  rel %.3g  bound %.3g" % (w * Rv * Cv, k, dy[f, k], ref[k], abs(dy[f, k] - ref[k]) / max(abs(ref[k]), 1e-300), bound))
            if w == 0.0:
                assert dy[f, k] == 0.0
            else:
                assert abs(dy[f, k] - ref[k]) <= bound * abs(ref[k]), (f, k)
    # a (p, n) pair: V(in) - V(out) = 1 - y, so the derivatives change sign; and db enters: b = [0, 0, a], db/da = e_2 gives y itself
    y2, dy2 = api.sensitivity_solve(st, G0, C0, b, dG, dC, None, (0, 1), om)
    assert np.allclose(y2, 1.0 - y, rtol=0, atol=64 * EPS) and np.allclose(dy2, -dy, rtol=1e-12, atol=0)
    db = np.zeros((1, 3), dtype=complex)
    db[0, 2] = 1.0
    y3, dy3 = api.sensitivity_solve(st, G0, C0, b, np.zeros((1, 3, 3)), np.zeros((1, 3, 3)), db, (1, -1), om)
    assert np.allclose(dy3[:, 0], y, rtol=64 * EPS, atol=0)


@pytest.mark.parametrize("name", ["inverter", "dff"])
def test_adjoint_form_equals_direct_form(name):
    """The three points of the case: the outer two are the plus and minus of the middle one (scale 1: the bound does not care what the
    difference means), db a dense complex column so that both parts of w are exercised."""
    st, G, C, bac, om = R.port_case(name)
    out = (N.output_index(name, st), -1)
    Gd, Cd = SR.dense_G(st, G[1], GMIN), R.dense_csr(st, C[1])
    dG = np.array([R.dense_csr(st, G[2] - G[0]), R.dense_csr(st, G[0] - G[2])])
    dC = np.array([R.dense_csr(st, C[2] - C[0]), R.dense_csr(st, C[0] - C[2])])
    rng = np.random.default_rng(11)
    db = np.array([bac[2] - bac[0], rng.standard_normal(st.n) + 1j * rng.standard_normal(st.n)])
    oms = np.array([0.0, om[len(om) // 2], om[-1]])
    y, s = api.sensitivity_solve(st, Gd, Cd, bac[1], dG, dC, db, out, oms)
    assert np.array_equal(api.sensitivity_solve(st, Gd, Cd, bac[1], dG[:1], dC[:1], None, out, oms)[1][:, 0],
                          -api.sensitivity_solve(st, Gd, Cd, bac[1], dG[1:], dC[1:], None, out, oms)[1][:, 0])
    for f, w in enumerate(oms):
        A = Gd + 1j * w * Cd
        dA = dG + 1j * w * dC
        ref, x, lam, wk = SR.direct_form(A, bac[1], dA, db, out)
        assert abs(y[f] - x[out[0]]) <= 16 * R.cond_inf_c(A) * EPS * np.max(np.abs(x))
        for k in range(2):
            d = SR.d_s(A, x, lam, dA[k], wk[k])
            print("%s f %d k %d  |s| %.3g  err %.3g  d_s %.3g" % (name, f, k, abs(ref[k]), abs(s[f, k] - ref[k]), d))
            assert abs(s[f, k] - ref[k]) <= d, (f, k)


# dy/dvdd of the inverter at vdd = 3.3 from sensitivity_solve (rel_step 1e-4) against the Richardson-extrapolated difference quotient of the
# response: the largest relative disagreement measured over the three frequencies below on the CPU port (DC solves at abstol 1e-13) is
# 3.82e-9 (at 1 kHz; 1.7e-10 at 100 MHz, 2.4e-13 at 10 GHz), held here rounded up to two digits -- the central difference's own truncation
# term (delta^2 y''' / 6 at delta = 3.3e-4) and the DC solves' convergence noise over 2 delta, which enter both sides.  16 x that, as
# everywhere in this project; DESIGN.md section 6 records the measurement.
NONLINEAR_MEASURED = 3.9e-9


def test_the_derivative_is_the_slope_of_the_response():
    v0, rel = 3.3, 1e-4
    d = rel * v0
    D = 64 * d                       # the quotient's own step: large against the DC noise, its delta^2 term removed by the extrapolation
    vs = [v0, v0 + d, v0 - d, v0 + D, v0 - D, v0 + D / 2, v0 - D / 2]
    st, G, C, bac, _ = SR.port_points("inverter", [{"vdd": v} for v in vs])
    out = (N.output_index("inverter", st), -1)
    assert not np.any(bac - bac[0])                                     # the excitation does not depend on vdd
    freqs = np.array([1e3, 1e8, 1e10])
    om = 2.0 * np.pi * freqs
    Gd, Cd = SR.dense_G(st, G[0], GMIN), R.dense_csr(st, C[0])
    dG = np.array([R.dense_csr(st, G[1] - G[2]) / (2 * d)])
    dC = np.array([R.dense_csr(st, C[1] - C[2]) / (2 * d)])
    y, dy = api.sensitivity_solve(st, Gd, Cd, bac[0], dG, dC, None, out, om)
    resp = lambda i: np.array([np.linalg.solve(SR.dense_G(st, G[i], GMIN) + 1j * w * R.dense_csr(st, C[i]), bac[i])[out[0]] for w in om])
    q1, q2 = (resp(3) - resp(4)) / (2 * D), (resp(5) - resp(6)) / D
    rich = (4.0 * q2 - q1) / 3.0
    worst = 0.0
    for f in range(len(om)):
        rel_err = abs(dy[f, 0] - rich[f]) / abs(rich[f])
        worst = max(worst, rel_err)
        print("inverter f %.0e  dy/dvdd %r  richardson %r  rel %.3g" % (freqs[f], dy[f, 0], rich[f], rel_err))
        assert abs(dy[f, 0] - rich[f]) <= max(16 * NONLINEAR_MEASURED, 64 * EPS) * abs(rich[f]), f
    print("largest disagreement %.3g (recorded: %.3g)" % (worst, NONLINEAR_MEASURED))
    assert np.all(np.abs(dy[:, 0]) > 0)


def test_argument_handling():
    mc = api.MNACircuit(R.inverter_with_param_vdd(), {"vdd": 3.3})
    f = [1e3, 1e6]
    for kw in (dict(params=["nope"]), dict(params=[]), dict(params=["vdd", "vdd"]), dict(freqs=[]), dict(output="nope"), dict(output="0"),
               dict(output=("vout", "nope")), dict(solver="cuda"), dict(memory="l2"), dict(rel_step=0.0)):
        args = dict(output="vout", params=["vdd"], freqs=f)
        args.update(kw)
        with pytest.raises(ValueError):
            api.sensitivity(mc, args.pop("output"), args.pop("params"), args.pop("freqs"), **args)
    with pytest.raises(ValueError):
        api.sensitivity(api.CircuitSweep(mc, api.Sweep(vdd=[3.0, 3.6])), "vout", ["temp", "gain"], f)
    st = cj.discover(mc.circuit, {"vdd": 3.3})
    assert api.sens_output(st, "vout") == (st.index_of("vout"), -1)
    assert api.sens_output(st, ("vout", "0")) == (st.index_of("vout"), -1)
    assert api.sens_output(st, ("0", "vout")) == (-1, st.index_of("vout"))


def test_a_step_across_a_structure_class_names_the_parameter():
    """sp_mos1's rd at 0: the drain node is collapsed; rd = +-delta brings it back, so no difference of stamps exists."""
    circ = cj.Circuit("rd at zero")
    circ.V("vd", "d", "0", dc=2.0)
    circ.V("vg", "g", "0", dc=cj.Param("vg"), ac=1.0)
    circ.MOS1("m1", "d", "g", "0", "0", dict(type=1, vto=0.7, kp=100e-6, rd=cj.Param("rd")), w=10e-6, l=1e-6)
    mc = api.MNACircuit(circ, {"rd": 0.0, "vg": 1.5})
    with pytest.raises(ValueError, match="rd"):
        api.sensitivity(mc, "I_vd", ["vg", "rd"], [1e3])


class StubHandle:
    """Handle.analyze_values / ac_sens of the gate test: ``solve(a, omegas)`` -- sensitivity_solve per base -- with chosen (base, frequency)
    systems spoiled; ``fit`` False: the call raises as for a circuit the memory setting refuses"""

    def __init__(self, solve, spoil, fit=True):
        self.solve, self.spoil, self.fit, self.calls, self.samples = solve, spoil, fit, 0, 0

    def analyze_values(self, sample_ref):
        self.samples += 1

    def ac_sens(self, omega, gmin, base, plus, minus, scale, b_ac, c, pair, db=None, wpb=0, want_x=False):
        self.calls += 1
        if not self.fit:
            raise hip.CadnipError(hip.BADARG, "cadnip_ac_sens")
        NB, F, K = len(base), len(omega), np.shape(plus)[1]
        got = [self.solve(a, omega) for a in range(NB)]
        y, s = np.array([g[0] for g in got]), np.array([g[1] for g in got])
        berr, flags = np.zeros((NB, F, 2)), np.zeros((NB, F, K), dtype=np.int32)
        for (a, f), kind in self.spoil.items():
            if kind != "control":
                y[a, f], s[a, f] = 123.0, 123.0
            if kind == "flag":
                flags[a, f, 1] = 2
            elif kind == "adjoint":
                berr[a, f, 1] = 2 * api.NOISE_BERR_MAX
            else:
                berr[a, f, 0] = np.nan if kind == "nan" else 2 * api.AC_BERR_MAX if kind == "forward" else 2 * api.NOISE_BERR_MAX
        return y, s, None, berr, flags, dict(wpb=4, lds_bytes=0, systems=NB * F, workgroups=0)


def test_sens_gpu_sweep_gate_on_a_stub_handle():
    """sens_gpu_sweep on a stub handle, the inverter's three points as two bases of K = 2 parameters: a system with a flag in one column, a
    forward backward error above AC_BERR_MAX, an adjoint one above NOISE_BERR_MAX or a NaN is solved again by the host; a forward error of
    2 NOISE_BERR_MAX -- far below AC_BERR_MAX -- is accepted (the two bounds must not be swapped); the accounting; the fallback of "auto\""""
    st, G, C, bac, om = R.port_case("inverter")
    out = (N.output_index("inverter", st), -1)
    omegas = om[:: len(om) // 4][:4]
    NB, K = 2, 2
    Gd, Cd = [SR.dense_G(st, G[a], GMIN) for a in range(NB)], [R.dense_csr(st, C[a]) for a in range(NB)]
    dG = np.array([R.dense_csr(st, G[2] - G[0]), R.dense_csr(st, G[1] - G[0])])
    dC = np.array([R.dense_csr(st, C[2] - C[0]), R.dense_csr(st, C[1] - C[0])])
    solves = []
    host = lambda a: lambda w: (solves.append((a, tuple(w))), api.sensitivity_solve(st, Gd[a], Cd[a], bac[a], dG, dC, None, out, w))[1]
    want = [api.sensitivity_solve(st, Gd[a], Cd[a], bac[a], dG, dC, None, out, omegas) for a in range(NB)]
    spoil = {(0, 0): "flag", (0, 2): "forward", (1, 1): "adjoint", (1, 3): "nan", (0, 3): "control"}
    stub = StubHandle(lambda a, w: api.sensitivity_solve(st, Gd[a], Cd[a], bac[a], dG, dC, None, out, w), spoil)
    base, plus, minus, scale = np.array([0, 3], dtype=np.int32), np.zeros((NB, K), dtype=np.int32), np.zeros((NB, K), dtype=np.int32), np.ones((NB, K))
    ref = np.zeros((6, st.nnz))
    stats = {"gpu_systems": 0, "host_systems": 0, "max_berr": 0.0, "wpb": 0, "params": K}
    got = api.sens_gpu_sweep(stub, st, ref, ref, base, plus, minus, scale, bac[:NB], out, None, omegas, GMIN, "gpu", stats, host)
    assert stub.calls == 1 and stub.samples == 1
    assert stats == {"gpu_systems": 4, "host_systems": 4, "max_berr": 2 * api.NOISE_BERR_MAX, "wpb": 4, "params": K, "memory": "lds"}
    assert sorted(solves) == [(0, (omegas[0], omegas[2])), (1, (omegas[1], omegas[3]))]      # one host call per base, at its rejected frequencies
    for a in range(NB):
        y, s = got[a]
        assert y.shape == (4,) and s.shape == (4, K)
        # the stub's numbers are sensitivity_solve's: a redone system and an untouched one both equal them, a spoiled one that was kept does not
        assert np.array_equal(y, want[a][0]) and np.array_equal(s, want[a][1]), a
    stats = {"gpu_systems": 0, "host_systems": 0, "max_berr": 0.0, "wpb": 0, "params": K}
    refused = StubHandle(None, {}, fit=False)
    assert api.sens_gpu_sweep(refused, st, ref, ref, base, plus, minus, scale, bac[:NB], out, None, omegas, GMIN, "auto", stats, host) is None
    assert refused.calls == 1 and stats["gpu_systems"] == 0 and stats["host_systems"] == 8 and "host solve" in stats["fallback"] and "memory" not in stats
    with pytest.raises(hip.CadnipError):
        api.sens_gpu_sweep(refused, st, ref, ref, base, plus, minus, scale, bac[:NB], out, None, omegas, GMIN, "gpu", dict(stats), host)
