"""api.network_noise's host path (api.network_noise_solve, api.NetworkNoiseSol) on the CPU port's G and C, obtained as
tests/test_network_cpu.py obtains its own: the Twiss / Bosma identity of passive RC multiports, y from the adjoint columns against
network_solve's y, closed-form noise figures, and the consistency of the two-port noise parameters.

Tolerances.  Every adjoint column l_i is one dense complex solve of A^T: within d = 32 cond_inf(A^T) eps max|l| of another solve of the
same system -- the bound of tests/test_gpu_noise_solver.py: assert_within_the_solves_bound, 16 cond eps max|l| for each of the two solves
compared (against exact algebra that is generous by 2).  It is propagated the same way: a product l_i[a] conj(l_j[b]) with both factors
off by at most d moves by 2 max|l| d + d^2, weighted by what multiplies it."""
import numpy as np
import pytest

import cadnip_jl_amd as cj
from cadnip_jl_amd import api
from tests import ac_ref as R
from tests import test_network_cpu as NC
from tests.test_gpu_noise_solver import common_source

EPS = R.EPS
GMIN = NC.GMIN
FREQS = NC.FREQS
KB = api.K_BOLTZMANN
TEMP = 27.0
R1, R2, R3, C1, C2 = 220.0, 470.0, 1.5e3, 1e-9, 4.7e-12


def star_circuit():
    """three ports into one inner node: two resistors, one series RC, a capacitor from the star point to ground"""
    c = cj.Circuit("RC star three-port")
    for k in (1, 2, 3):
        c.V("v%d" % k, "p%d" % k, "0", dc=0.0)
    c.R("r1", "p1", "m", R1)
    c.R("r2", "p2", "m", R2)
    c.R("r3", "p3", "q", R3)
    c.C("c1", "q", "m", C1)
    c.C("c2", "m", "0", C2)
    return c


def resistor_sources(st, circ):
    """the thermal sources of a circuit of resistors, as api.noise_sources registers them: (p, n, "thermal", 1 / R, 0, name)"""
    at = lambda nm: -1 if nm in ("0", "gnd") else st.index_of(nm)
    return [(at(d.nodes[0]), at(d.nodes[1]), "thermal", 1.0 / float(d.params["r"]), 0.0, d.name.lower()) for d in circ.devices if d.type == "R"]


def passive_cases():
    return {"pi-r": (NC.pi_circuit("r"), ["v1", "v2"]), "pi-c": (NC.pi_circuit("c"), ["v1", "v2"]), "star": (star_circuit(), ["v1", "v2", "v3"])}


_SOLVED = {}


def solved(name):
    if name not in _SOLVED:
        circ, ports = passive_cases()[name]
        st, Gd, Cd = NC.linearise(circ)
        srcs = resistor_sources(st, circ)
        _SOLVED[name] = (st, Gd, Cd, srcs, ports, api.network_noise_solve(st, Gd, Cd, srcs, ports, FREQS, 50.0, TEMP))
    return _SOLVED[name]


def adjoint_columns(st, Gd, Cd, ports, f):
    """(lambda [n, P] from a dense solve of A^T, d of the module docstring)"""
    rows = api.port_rows(st, ports)
    E = np.zeros((st.n, len(rows)), complex)
    E[rows, np.arange(len(rows))] = 1.0
    AT = (Gd + 2j * np.pi * f * Cd).T
    lam = np.linalg.solve(AT, E)
    return lam, 32 * R.cond_inf_c(AT) * EPS * np.max(np.abs(lam)), rows


def assert_twiss(name, st, Gd, Cd, srcs, ports, net, temp=TEMP, gmin=GMIN, freqs=FREQS):
    """2 k T (y + y^H) = cy + 4 k T gmin sum_{v < n_nodes} l_i[v] conj(l_j[v]): the second term is the noise the gmin conductances would
    make -- they are in G, and noiseless.  Per entry the left side moves by 2 k T 2 d (y's entries are entries of l), the right side by
    sum_s S_s (2 |T| 2d + (2d)^2) over the sources (a probe difference of two entries, each within d and at most max|l|: |T| <= 2 max|l|,
    off by at most 2 d) plus 4 k T gmin n_nodes (2 max|l| d + d^2) for the gmin term."""
    kT = KB * (temp + 273.15)
    assert net.cy.shape == (len(freqs), len(ports), len(ports)) and net.temp == temp and isinstance(net, api.NetworkSol)
    for fi, f in enumerate(freqs):
        lam, d, rows = adjoint_columns(st, Gd, Cd, ports, f)
        big = np.max(np.abs(lam))
        nodes = lam[:st.n_nodes]
        gmin_term = 4 * kT * gmin * (nodes.T @ np.conj(nodes))
        lhs = 2 * kT * (net.y[fi] + np.conj(net.y[fi].T))
        tol = 2 * kT * 2 * d + sum(api.noise_psd(s, temp, f) for s in srcs) * (2 * 2 * big * 2 * d + 4 * d * d) + 4 * kT * gmin * st.n_nodes * (2 * big * d + d * d)
        err = np.max(np.abs(lhs - net.cy[fi] - gmin_term))
        print("%s f %.0e  |2kT(y + y^H) - cy - gmin term| %.3g  tol %.3g  max|cy| %.3g" % (name, f, err, tol, np.max(np.abs(net.cy[fi]))))
        assert err <= tol, f
        assert tol <= 1e-6 * np.max(np.abs(net.cy[fi]))                                   # the bound is a real one: far below what it bounds


@pytest.mark.parametrize("name", ["pi-r", "pi-c", "star"])
def test_twiss_identity_of_a_passive_network_at_one_temperature(name):
    st, Gd, Cd, srcs, ports, net = solved(name)
    assert_twiss(name, st, Gd, Cd, srcs, ports, net)


@pytest.mark.parametrize("name", ["pi-r", "pi-c", "star"])
def test_y_from_the_adjoint_columns_is_network_solves_y(name):
    st, Gd, Cd, srcs, ports, net = solved(name)
    ref = api.network_solve(st, Gd, Cd, ports, FREQS)
    for fi, f in enumerate(FREQS):
        _, d, _ = adjoint_columns(st, Gd, Cd, ports, f)
        assert np.max(np.abs(net.y[fi] - ref.y[fi])) <= d, f
    assert net.y[0, 0, 0].real > 0                                                        # the current INTO the port, as network's
    if name != "star":
        for fi, f in enumerate(FREQS):
            yref = NC.y_pi(name[-1], f)
            assert np.max(np.abs(net.y[fi] - yref)) <= NC.tol_y(Gd, Cd, f, yref)
    assert np.array_equal(net.z, np.linalg.inv(net.y)) and net.s.shape == net.y.shape and net.z0 == 50.0


@pytest.mark.parametrize("name", ["pi-r", "pi-c", "star"])
def test_cy_is_hermitian_positive_semidefinite_and_the_sum_of_its_sources(name):
    st, Gd, Cd, srcs, ports, net = solved(name)
    assert sorted(net.cy_by_source) == sorted(s[5] for s in srcs)
    total = sum(net.cy_by_source.values())
    scale = np.max(np.abs(net.cy))
    assert np.max(np.abs(total - net.cy)) <= 4 * len(srcs) * EPS * scale                  # the same terms in another order of summation
    for fi in range(len(FREQS)):
        assert np.max(np.abs(net.cy[fi] - np.conj(net.cy[fi].T))) <= 4 * EPS * scale
        assert np.min(np.linalg.eigvalsh(0.5 * (net.cy[fi] + np.conj(net.cy[fi].T)))) >= -4 * len(srcs) * len(ports) * EPS * scale
        for part in net.cy_by_source.values():                                           # S_s T T^H: rank one, positive semidefinite
            assert np.min(np.linalg.eigvalsh(0.5 * (part[fi] + np.conj(part[fi].T)))) >= -4 * len(ports) * EPS * scale


def series_circuit(r):
    c = cj.Circuit("series resistor between two ports")
    c.V("v1", "p1", "0", dc=0.0)
    c.V("v2", "p2", "0", dc=0.0)
    c.R("rs", "p1", "p2", r)
    return c


def test_a_series_resistor_at_290_kelvin():
    """F = 1 + R / Rs exactly when the resistor sits at T0: rn = R, nfmin = 1 (at an open source).  gmin from either port node to ground is
    noiseless and sits across the ports' own sources: it moves nothing at the 1e-6 of tests/test_gpu_noise.py's closed forms."""
    r = 330.0
    circ = series_circuit(r)
    st, Gd, Cd = NC.linearise(circ)
    temp = api.T0 - 273.15
    assert abs(temp - 16.85) < 1e-12
    net = api.network_noise_solve(st, Gd, Cd, resistor_sources(st, circ), ["v1", "v2"], FREQS, 50.0, temp)
    assert net.temp == temp
    for rs in (50.0, 75.0, 1e3):
        assert np.allclose(net.nf(rs), 1.0 + r / rs, rtol=1e-6, atol=0.0)
        assert np.allclose(net.nf_db(rs), 10 * np.log10(1.0 + r / rs), rtol=1e-6, atol=0.0)
    assert np.allclose(net.nf(), 1.0 + r / 50.0, rtol=1e-6, atol=0.0)                      # zs defaults to z0 of port 0
    assert np.allclose(net.rn, r, rtol=1e-6, atol=0.0)
    assert np.allclose(net.nfmin, 1.0, rtol=1e-6, atol=0.0) and np.allclose(net.nfmin_db, 0.0, atol=1e-5)
    assert np.all(np.abs(net.yopt) <= 1e-6 / r) and np.allclose(net.gamma_opt, 1.0, rtol=1e-6)      # the optimum source is an open circuit
    hot = api.network_noise_solve(st, Gd, Cd, resistor_sources(st, circ), ["v1", "v2"], FREQS, 75.0, 2 * api.T0 - 273.15)
    assert np.allclose(hot.nf(), 1.0 + 2 * r / 75.0, rtol=1e-6, atol=0.0)                  # twice the temperature, z0 = 75


def test_a_matched_pad_has_its_insertion_loss_as_noise_figure():
    """the pi attenuator of N dB for z0 = 50 at T0: matched on both sides, so F = 1 / |s21|^2 = 10^(N / 10)"""
    for n_db in (6.0, 10.0):
        k = 10.0 ** (n_db / 20.0)
        shunt, series = 50.0 * (k + 1) / (k - 1), 50.0 * (k * k - 1) / (2 * k)
        c = cj.Circuit("matched pi pad")
        c.V("v1", "p1", "0", dc=0.0)
        c.V("v2", "p2", "0", dc=0.0)
        c.R("ra", "p1", "0", shunt)
        c.R("rb", "p2", "0", shunt)
        c.R("rc", "p1", "p2", series)
        st, Gd, Cd = NC.linearise(c)
        net = api.network_noise_solve(st, Gd, Cd, resistor_sources(st, c), ["v1", "v2"], FREQS, 50.0, api.T0 - 273.15)
        assert np.allclose(np.abs(net.s[:, 0, 0]), 0.0, atol=1e-6) and np.allclose(net.s_db(1, 0), -n_db, rtol=1e-6)
        assert np.allclose(net.nf(50.0), 1.0 / np.abs(net.s[:, 1, 0]) ** 2, rtol=1e-6, atol=0.0)
        assert np.allclose(net.nf_db(), n_db, rtol=1e-6, atol=0.0)


def amplifier_circuit(vdd=5.0, vout=3.0):
    """the common-source stage of tests/test_gpu_noise_solver.py with gate capacitances and a second port source at the output"""
    c = common_source(vdd)
    m1 = next(d for d in c.devices if d.name == "m1")
    m1.params["Cgs"], m1.params["Cgd"] = 2e-12, 0.5e-12
    c.V("vout", "out", "0", dc=vout)
    return c


def amplifier_sources(st, vds, vgs=1.0):
    """the stage's noise sources as data: rd's thermal noise, the channel's thermal and flicker noise at the square-law operating point
    (saturation), and the shot noise of 1 uA of gate leakage -- without a source at the input every noise current is the output's, v_n and
    i_n are fully correlated and Re(yopt) = Re(y11) = gmin: nothing to test"""
    gm, ids = 1e-3 * (vgs - 0.5) * (1 + 0.02 * vds), 1e-3 / 2 * (vgs - 0.5) ** 2 * (1 + 0.02 * vds)
    out, vdd = st.index_of("out"), st.index_of("vdd")
    return [(vdd, out, "thermal", 1.0 / 10e3, 0.0, "rd"), (out, -1, "thermal", 2.0 / 3.0 * gm, 0.0, "m1"),
            (out, -1, "flicker", 1e-14 * ids ** 1.2, 0.9, "m1"), (st.index_of("in"), -1, "shot", 1e-6, 0.0, "ig")], gm


def amplifier():
    st, Gd, Cd = NC.linearise(amplifier_circuit())
    srcs, gm = amplifier_sources(st, 3.0)
    return st, Gd, Cd, srcs, gm


def test_the_noise_parameters_are_consistent_on_an_amplifier():
    st, Gd, Cd, srcs, gm = amplifier()
    freqs = np.array([1e3, 1e8, 3e9])
    net = api.network_noise_solve(st, Gd, Cd, srcs, ["vg", "vout"], freqs, 50.0, TEMP)
    assert np.allclose(net.y[:, 1, 0].real, gm, rtol=1e-3) and np.all(net.y[:, 0, 0].imag > 0)      # a transconductance and a capacitive input
    assert sorted(net.cy_by_source) == ["ig", "m1", "rd"] and np.allclose(sum(net.cy_by_source.values()), net.cy, rtol=1e-14, atol=0.0)
    ca, rn, yopt, nfmin = net.ca, net.rn, net.yopt, net.nfmin
    assert ca.shape == (3, 2, 2) and np.all(rn > 0) and np.all(nfmin > 1.0) and np.all(yopt.real > 0)
    assert np.allclose(rn, ca[:, 0, 0].real / (4 * KB * api.T0), rtol=1e-15)
    assert np.allclose(net.nf(1.0 / yopt), nfmin, rtol=1e-9, atol=0.0)                    # one source impedance per frequency
    for ys in (1.0 / 50.0, 2e-3 - 5e-3j, 1e-4 + 3e-2j):
        want = nfmin + rn / np.real(ys) * np.abs(ys - yopt) ** 2
        assert np.allclose(net.nf(1.0 / ys), want, rtol=1e-9, atol=0.0), ys
        assert np.all(net.nf(1.0 / ys) >= nfmin * (1 - 1e-9))
    assert np.allclose(net.gamma_opt, (1 / 50.0 - yopt) / (1 / 50.0 + yopt), rtol=1e-12) and np.all(np.abs(net.gamma_opt) < 1.0)
    assert np.array_equal(net.nfmin_db, 10 * np.log10(nfmin)) and np.array_equal(net.nf_db(75.0), 10 * np.log10(net.nf(75.0)))
    two = api.network_noise_solve(st, Gd, Cd, srcs, ["vg", "vout"], freqs, [75.0, 50.0], TEMP)      # per-port z0: port 0's counts
    assert np.array_equal(two.nf(), net.nf(75.0))


def test_other_port_counts_and_a_vanishing_y21():
    st, Gd, Cd, srcs, ports, net = solved("star")
    for get in (lambda n: n.ca, lambda n: n.rn, lambda n: n.yopt, lambda n: n.gamma_opt, lambda n: n.nfmin, lambda n: n.nfmin_db,
                lambda n: n.nf(), lambda n: n.nf_db(50.0)):
        with pytest.raises(ValueError):
            get(net)
    st1, G1, C1 = NC.linearise(NC.one_port_circuit())
    one = api.network_noise_solve(st1, G1, C1, resistor_sources(st1, NC.one_port_circuit()), ["v1"], FREQS[:1], 50.0, TEMP)
    assert one.cy.shape == (1, 1, 1) and abs(one.cy[0, 0, 0] - 4 * KB * (TEMP + 273.15) / NC.RA) <= 1e-6 * abs(one.cy[0, 0, 0])
    with pytest.raises(ValueError):
        one.nfmin
    # two ports with nothing between them: y21 = 0, no chain form -- inf / nan, no exception and no warning turned error
    iso = api.NetworkNoiseSol([1e3], ["a", "b"], np.diag([1e-2, 2e-2]).astype(complex)[None], np.diag([1e-22, 2e-22]).astype(complex)[None], {}, TEMP)
    with np.errstate(all="raise"):
        vals = [iso.ca, iso.rn, iso.yopt, iso.gamma_opt, iso.nfmin, iso.nf(), iso.nfmin_db, iso.nf_db()]
    assert all(not np.all(np.isfinite(v)) for v in vals)


def test_ports_and_arguments():
    st, Gd, Cd, srcs, ports, net = solved("pi-r")
    for bad in (["ra"], ["p1"], ["v1", "nope"], ["v1", "V1"]):
        with pytest.raises(ValueError):
            api.network_noise_solve(st, Gd, Cd, srcs, bad, FREQS)
    with pytest.raises(ValueError):
        api.network_noise(None, ["v1"], FREQS, solver="fpga")
    with pytest.raises(ValueError):
        api.network_noise(None, ["v1"], FREQS, memory="l2")
    empty = api.network_noise_solve(st, Gd, Cd, srcs, ports, [])
    assert empty.y.shape == empty.cy.shape == (0, 2, 2)
    assert cj.network_noise is api.network_noise and cj.NetworkNoiseSol is api.NetworkNoiseSol and api.T0 == 290.0
    # the pairs of a class: every source's (p, n) once, then the port rows against ground
    pairs, index = api.network_noise_pairs([7, 8], [srcs, srcs])
    assert len(pairs) == len(index) == len({(s[0], s[1]) for s in srcs}) + 2 and index[(7, -1)] == len(pairs) - 2 and index[(8, -1)] == len(pairs) - 1


class StubHandle:
    """Handle.analyze_values / ac_adjoint_multi of the merge test: dense adjoint solves, with chosen (point, frequency, column)s spoiled"""

    def __init__(self, Gd, Cd, spoil):
        self.Gd, self.Cd, self.spoil, self.calls = Gd, Cd, spoil, 0

    def analyze_values(self, sample_ref):
        pass

    def ac_adjoint_multi(self, omega, gmin, c, pairs=None, wpb=0, want_x=False, x_out=None):
        self.calls += 1
        B, F, (K, n) = len(self.Gd), len(omega), c.shape
        x, berr, flags = np.zeros((B, F, K, n), complex), np.zeros((B, F, K)), np.zeros((B, F, K), dtype=np.int32)
        for i in range(B):
            for f, w in enumerate(omega):
                x[i, f] = np.linalg.solve((1j * w * self.Cd[i] + self.Gd[i]).T, c.T).T
        for (i, f, k), kind in self.spoil.items():
            x[i, f, k] = 123.0
            if kind == "flag":
                flags[i, f, k] = 1
            else:
                berr[i, f, k] = np.nan if kind == "nan" else 2 * api.NOISE_BERR_MAX
        pr = np.asarray(pairs).reshape(-1, 2)
        h = np.where(pr[:, 0] >= 0, x[..., pr[:, 0]], 0.0) - np.where(pr[:, 1] >= 0, x[..., pr[:, 1]], 0.0)
        return h, None, berr, flags, dict(wpb=4, lds_bytes=0, systems=B * F, workgroups=0)


def test_the_gpu_merge_keeps_accepted_columns_and_redoes_rejected_ones_on_the_host():
    """network_noise_gpu on a stub handle: one call for the class, the gate per column, and -- the weighting being network_noise_solve's own
    statements -- the host path's numbers for both points, whether a column was spoiled or not"""
    st, Gd, Cd, srcs, ports, net = solved("pi-c")
    stub = StubHandle([Gd, 2.0 * Gd], [Cd, Cd], {(0, 1, 0): "flag", (1, 0, 1): "berr", (1, 2, 0): "nan"})
    stats = {"gpu_systems": 0, "host_systems": 0, "max_berr": 0.0, "wpb": 0}
    G_ref = C_ref = np.zeros((2, st.nnz))
    got = api.network_noise_gpu(stub, st, G_ref, C_ref, stub.Gd, stub.Cd, [srcs, srcs], ports, FREQS, 50.0, [TEMP, 85.0], GMIN, "gpu", stats)
    assert stub.calls == 1 and stats == {"gpu_systems": 9, "host_systems": 3, "max_berr": 0.0, "wpb": 4, "rhs": 2, "memory": "lds"}
    for k, temp in enumerate([TEMP, 85.0]):
        host = api.network_noise_solve(st, stub.Gd[k], stub.Cd[k], srcs, ports, FREQS, 50.0, temp)
        scale = np.max(np.abs(host.cy))
        # the host solves all P columns in one call of LAPACK, the stub and the redo column by column: the same LU, the same columns
        assert np.allclose(got[k].y, host.y, rtol=1e-13, atol=0.0) and np.max(np.abs(got[k].cy - host.cy)) <= 1e-13 * scale
        assert got[k].temp == temp and got[k].stats is stats
    assert np.allclose(got[0].y, net.y, rtol=1e-13, atol=0.0)
