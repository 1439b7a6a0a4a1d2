"""api.network's host path (api.network_solve, api.NetworkSol) on the CPU port's G and C (oracle/cpu_port.py; tests/ac_ref.port_case's way
of getting them): the sign and the closed forms of Y on a resistive and an RC pi two-port, reciprocity, passivity, Z and S, per-port
reference impedances, and NetworkSol's algebra on matrices given directly.

Tolerances.  y comes from one dense complex solve of a 2 to 4 unknown system A = G + j w C: 16 cond_inf(A) eps max|ref| (tests/ac_ref.py's
bound for such a solve, R.cond_inf_c).  z and s are computed from y by one more inversion -- of y, of I + Z0 y -- so an error dy of y moves
them by |inv| |dy| |inv| resp. 2 |(I + Z0 y)^-1| |Z0 dy| |(I + Z0 y)^-1| to first order, and the inversion adds its own cond eps: their bound
is 16 (cond_inf(A) + cond_inf(M)) cond_inf(M) eps max|ref| with M the matrix inverted.  The closed forms are evaluated in the same double
arithmetic; their own rounding (a few eps) is inside the factor 16."""
import numpy as np
import pytest

import cadnip_jl_amd as cj
from cadnip_jl_amd import api, hip
from tests import ac_ref as R
from tests.port_util import make_port, analyze_port

EPS = R.EPS
GMIN = 1e-12
RA, RB, RC, CC = 75.0, 120.0, 330.0, 2.2e-9
FREQS = np.array([1e3, 1e6, 1e9])


def pi_circuit(coupling="r"):
    c = cj.Circuit("pi two-port")
    c.V("v1", "p1", "0", dc=0.0, ac=1.0)              # ac= is ignored by network
    c.V("v2", "p2", "0", dc=0.0)
    c.R("ra", "p1", "0", RA)
    c.R("rb", "p2", "0", RB)
    if coupling == "r":
        c.R("rc", "p1", "p2", RC)
    else:
        c.C("cc", "p1", "p2", CC)
    return c


def one_port_circuit():
    c = cj.Circuit("one-port")
    c.V("v1", "p1", "0", dc=0.0)
    c.R("r1", "p1", "0", RA)
    return c


def linearise(circ):
    """(st, G dense with GMIN on the node diagonals, C dense) at the DC point, from the CPU port"""
    st, port = make_port(circ, {}, 27.0, "dcop")
    analyze_port(st, port, 1.0)
    u, ok, _ = port.dc()
    assert ok
    G, C, _, _ = port.rebuild(u, 0.0)
    port.close()
    Gd = R.dense_csr(st, np.asarray(G, dtype=float))
    Gd[np.arange(st.n_nodes), np.arange(st.n_nodes)] += GMIN
    return st, Gd, R.dense_csr(st, np.asarray(C, dtype=float))


def y_pi(coupling, f):
    """the pi network's Y by inspection; GMIN is a conductance from either port node to ground"""
    yc = 1.0 / RC if coupling == "r" else 2j * np.pi * f * CC
    return np.array([[1.0 / RA + GMIN + yc, -yc], [-yc, 1.0 / RB + GMIN + yc]])


_LIN = {}


def solved(coupling):
    if coupling not in _LIN:
        st, Gd, Cd = linearise(pi_circuit(coupling))
        _LIN[coupling] = (st, Gd, Cd, api.network_solve(st, Gd, Cd, ["v1", "v2"], FREQS))
    return _LIN[coupling]


def tol_y(Gd, Cd, f, ref):
    return 16 * R.cond_inf_c(Gd + 2j * np.pi * f * Cd) * EPS * np.max(np.abs(ref))


def test_sign_and_closed_form_of_the_resistive_pi():
    st, Gd, Cd, net = solved("r")
    assert net.y.shape == (3, 2, 2) and net.ports == ["v1", "v2"] and net.z0 == 50.0 and np.array_equal(net.freqs, FREQS)
    for fi, f in enumerate(FREQS):
        ref = y_pi("r", f)
        assert np.max(np.abs(net.y[fi] - ref)) <= tol_y(Gd, Cd, f, ref), f
        assert net.y[fi, 0, 0].real > 0 and net.y[fi, 0, 1].real < 0                     # the current INTO the port
    st1, G1, C1 = linearise(one_port_circuit())
    one = api.network_solve(st1, G1, C1, ["v1"], FREQS[:1])
    ref = 1.0 / RA + GMIN
    assert one.y.shape == (1, 1, 1) and abs(one.y[0, 0, 0] - ref) <= tol_y(G1, C1, FREQS[0], ref) and one.y[0, 0, 0].real > 0


def test_rc_pi_over_three_frequencies():
    st, Gd, Cd, net = solved("c")
    for fi, f in enumerate(FREQS):
        ref = y_pi("c", f)
        assert np.max(np.abs(net.y[fi] - ref)) <= tol_y(Gd, Cd, f, ref), f
        assert abs(net.y[fi, 0, 1] - (-2j * np.pi * f * CC)) <= tol_y(Gd, Cd, f, ref)


@pytest.mark.parametrize("coupling", ["r", "c"])
def test_reciprocity_passivity_and_z(coupling):
    st, Gd, Cd, net = solved(coupling)
    z, s = net.z, net.s
    for fi, f in enumerate(FREQS):
        ref = y_pi(coupling, f)
        ty = tol_y(Gd, Cd, f, ref)
        assert np.max(np.abs(net.y[fi] - net.y[fi].T)) <= 2 * ty
        kA, ky = R.cond_inf_c(Gd + 2j * np.pi * f * Cd), R.cond_inf_c(ref)
        assert np.max(np.abs(z[fi] @ net.y[fi] - np.eye(2))) <= 16 * ky * EPS
        zref = np.linalg.inv(ref)
        assert np.max(np.abs(z[fi] - zref)) <= 16 * (kA + ky) * ky * EPS * np.max(np.abs(zref))
        M = np.eye(2) + 50.0 * ref
        kM = R.cond_inf_c(M)
        sref = (np.eye(2) - 50.0 * ref) @ np.linalg.inv(M)
        assert np.max(np.abs(s[fi] - sref)) <= 16 * (kA + kM) * kM * EPS * np.max(np.abs(sref))
        assert np.all(np.linalg.svd(s[fi], compute_uv=False) <= 1.0 + 16 * (kA + kM) * kM * EPS)      # passive
        assert np.max(np.abs(s[fi] - s[fi].T)) <= 2 * 16 * (kA + kM) * kM * EPS
    assert np.array_equal(net.s_db(0, 1), 20.0 * np.log10(np.abs(s[:, 0, 1]))) and np.array_equal(net.s_db("v2", "v1"), net.s_db(1, 0))
    assert np.all(net.s_db(1, 0) < 0.0)


def test_a_singular_y_raises_from_z_and_not_from_s():
    y = np.array([[[1.0, -1.0], [-1.0, 1.0]]]) / 330.0                                  # a series element alone: det y = 0
    net = api.NetworkSol([1e3], ["a", "b"], y)
    with pytest.raises(np.linalg.LinAlgError):
        net.z
    s = net.s                                                                            # I + z0 y is far from singular
    g = 50.0 / 330.0                                                                     # a series impedance Z: S11 = Z / (Z + 2 z0), S21 = 2 z0 / (Z + 2 z0)
    ref = np.array([[1.0, 2.0 * g], [2.0 * g, 1.0]]) / (1.0 + 2.0 * g)
    assert s.shape == (1, 2, 2) and np.max(np.abs(s[0] - ref)) <= 16 * R.cond_inf_c(np.eye(2) + 50.0 * y[0]) * EPS * np.max(np.abs(ref))


def test_unequal_reference_impedances_against_the_formula_by_hand():
    st, Gd, Cd, _ = solved("r")
    z0 = np.array([50.0, 75.0])
    net = api.network_solve(st, Gd, Cd, ["v1", "v2"], FREQS[:2], z0=z0)
    assert np.array_equal(net.z0, z0)
    for fi, f in enumerate(FREQS[:2]):
        (a, b), (c, d) = y_pi("r", f)
        # (I - Z0 y)(I + Z0 y)^-1 written out for two ports, then scaled by F = diag(1 / (2 sqrt(z0))) from the left and F^-1 from the right
        n11, n12, n21, n22 = 1 - z0[0] * a, -z0[0] * b, -z0[1] * c, 1 - z0[1] * d
        m11, m12, m21, m22 = 1 + z0[0] * a, z0[0] * b, z0[1] * c, 1 + z0[1] * d
        det = m11 * m22 - m12 * m21
        i11, i12, i21, i22 = m22 / det, -m12 / det, -m21 / det, m11 / det
        t = np.array([[n11 * i11 + n12 * i21, n11 * i12 + n12 * i22], [n21 * i11 + n22 * i21, n21 * i12 + n22 * i22]])
        k = np.sqrt(z0[1] / z0[0])                                                       # F_1 / F_2
        ref = np.array([[t[0, 0], t[0, 1] * k], [t[1, 0] / k, t[1, 1]]])
        kA, kM = R.cond_inf_c(Gd + 2j * np.pi * f * Cd), R.cond_inf_c(np.array([[m11, m12], [m21, m22]]))
        assert np.max(np.abs(net.s[fi] - ref)) <= 16 * (kA + kM) * kM * EPS * np.max(np.abs(ref)), f
        assert abs(net.s[fi, 0, 1] - net.s[fi, 1, 0]) <= 2 * 16 * (kA + kM) * kM * EPS   # power waves keep a reciprocal network's S symmetric
    for bad in (0.0, -50.0, [50.0], [50.0, 75.0, 100.0], [[50.0, 75.0]]):
        with pytest.raises(ValueError):
            api.NetworkSol([1.0], ["a", "b"], np.zeros((1, 2, 2)), bad)


def test_ports_are_resolved_like_the_noise_input():
    st, Gd, Cd, _ = solved("r")
    assert api.port_rows(st, ["V1", "v2"]) == [st.index_of("I_v1"), st.index_of("I_v2")]
    for bad in (["ra"], ["p1"], ["v1", "nope"], ["v1", "V1"]):
        with pytest.raises(ValueError):
            api.network_solve(st, Gd, Cd, bad, FREQS)
    c = pi_circuit("r")
    c.I("i1", "p1", "0", dc=0.0)
    b = api.source_rhs(st, c, "v2")
    assert b[st.index_of("I_v2")] == 1.0 and np.count_nonzero(b) == 1                    # unit magnitude whatever ac= says
    bi = api.source_rhs(st, c, "I1")
    assert bi[st.index_of("p1")] == 1.0 and np.count_nonzero(bi) == 1
    with pytest.raises(ValueError):
        api.source_rhs(st, c, "ra")
    with pytest.raises(ValueError):
        api.network(None, ["v1"], FREQS, solver="fpga")


class StubHandle:
    """Handle.analyze_values / ac_solve_multi of the merge test: dense solves, with chosen (point, frequency, column)s spoiled."""

    def __init__(self, Gd, Cd, spoil, fit=True):
        self.Gd, self.Cd, self.spoil, self.fit, self.calls, self.samples = Gd, Cd, spoil, fit, 0, 0

    def analyze_values(self, sample_ref):
        self.samples += 1

    def ac_solve_multi(self, omega, gmin, b, pairs=None, wpb=0, want_x=True):
        self.calls += 1
        if not self.fit:
            raise hip.CadnipError(hip.BADARG, "cadnip_ac_solve_multi")
        B, F, (K, n) = len(self.Gd), len(omega), b.shape
        x, berr, flags = np.zeros((B, F, K, n), complex), np.zeros((B, F, K)), np.zeros((B, F, K), dtype=np.int32)
        for i in range(B):
            for f, w in enumerate(omega):
                x[i, f] = np.linalg.solve(self.Gd[i] + 1j * w * self.Cd[i], b.T).T
        for (i, f, k), kind in self.spoil.items():
            x[i, f, k] = 123.0
            if kind == "flag":
                flags[i, f, k] = 1
            else:
                berr[i, f, k] = np.nan if kind == "nan" else 2 * api.AC_BERR_MAX
        pr = None if pairs is None else np.asarray(pairs).reshape(-1, 2)
        h = None if pr is None else np.where(pr[:, 0] >= 0, x[..., pr[:, 0]], 0.0) - np.where(pr[:, 1] >= 0, x[..., pr[:, 1]], 0.0)
        return h, x if want_x else None, berr, flags, dict(wpb=4, lds_bytes=0, systems=B * F, workgroups=0)


def test_the_multi_column_merge_keeps_gpu_columns_and_redoes_rejected_ones_on_the_host():
    st, Gd, Cd, net = solved("c")
    omegas = 2.0 * np.pi * FREQS
    rows = api.port_rows(st, ["v1", "v2"])
    rhs = np.zeros((2, st.n), complex)
    rhs[[0, 1], rows] = 1.0
    G_ref = C_ref = np.zeros((2, st.nnz))
    spoil = {(0, 1, 0): "flag", (1, 0, 1): "berr", (1, 2, 0): "nan"}
    for want_x in (False, True):
        stub = StubHandle([Gd, 2.0 * Gd], [Cd, Cd], spoil)
        stats = {"gpu_systems": 0, "host_systems": 0, "max_berr": 0.0, "wpb": 0}
        h, x = api.ac_multi_gpu_sweep(stub, st, stub.Gd, stub.Cd, G_ref, C_ref, omegas, GMIN, rhs, [(r, -1) for r in rows], want_x, "gpu", stats)
        assert stub.calls == 1 and stub.samples == 1 and (x is not None) == want_x
        assert stats == {"gpu_systems": 9, "host_systems": 3, "max_berr": 0.0, "wpb": 4, "rhs": 2, "memory": "lds"}
        for i in range(2):
            for f, w in enumerate(omegas):
                ref = np.linalg.solve(stub.Gd[i] + 1j * w * stub.Cd[i], rhs.T).T           # host column, bit for bit -- spoiled or not
                assert np.array_equal(h[i, f], ref[:, rows]) and (x is None or np.array_equal(x[i, f], ref))
        assert np.array_equal(-np.swapaxes(h[0], 1, 2), net.y)                             # network's own arrangement: h[f, column, port] -> y[f, port, column]
    stats = {"gpu_systems": 0, "host_systems": 0, "max_berr": 0.0, "wpb": 0}
    assert api.ac_multi_gpu_sweep(StubHandle([Gd], [Cd], {}, fit=False), st, [Gd], [Cd], G_ref[:1], C_ref[:1], omegas, GMIN, rhs, None, True, "auto", stats) is None
    assert stats["host_systems"] == 6 and stats["gpu_systems"] == 0 and "fallback" in stats
    with pytest.raises(hip.CadnipError):
        api.ac_multi_gpu_sweep(StubHandle([Gd], [Cd], {}, fit=False), st, [Gd], [Cd], G_ref[:1], C_ref[:1], omegas, GMIN, rhs, None, True, "gpu", dict(stats))
