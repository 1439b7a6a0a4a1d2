"""Delayed controlled sources and ideal transmission lines in the AC analyses, on the CPU: the dense host path (api.ac_delay_overlay behind
ACSol, network_solve, noise_solve, network_noise_solve) against closed forms on the CPU port's matrices, the Branin expansion of Circuit.T in
plain numpy, the static-order reference of the overlay kernels on every system of the three cases of tests/ac_delay_ref.py, the netlist
syntax, the helper's table entry by entry, what a line registers as noise, and the analyses that refuse a delayed circuit."""
import numpy as np
import pytest

import cadnip_jl_amd as cj
from cadnip_jl_amd import api, netlist
from tests import ac_delay_ref as D
from tests import ac_ref as R

EPS = R.EPS


def test_the_host_path_meets_the_closed_forms():
    """The figures behind every closed-form bound of the GPU tests: measured here on every run and held to the recorded constants
    (ac_delay_ref.HOST_MEASURED; two units of slack for another LAPACK's last bit, the bounds themselves take 16 x the recorded figure)."""
    got = D.closed_form_errors(D.HostBackend())
    for key, err in got.items():
        print("%s: host path against the closed form %.3g (recorded %.3g, bound of the other paths %.3g)" % (key, err, D.HOST_MEASURED[key], D.closed_form_bound(key)))
    assert set(got) == set(D.HOST_MEASURED)
    for key, err in got.items():
        assert err <= 2.0 * D.HOST_MEASURED[key], key
        assert D.HOST_MEASURED[key] <= 64 * EPS, key              # the recorded figures are rounding, not a formulation error


def test_the_cascade_form_is_the_textbook_line_without_series_resistors():
    """S11 = 0, S21 = e^{-j w td} against z0 and the mismatch expressions against 50 ohm are ``cascade_s`` at rs = 0: the form the line is
    tested against differs from them by the series resistors the ports need, and by nothing else."""
    w = 2.0 * np.pi * D.TL_FREQS
    for td in D.TL_TDS:
        s75 = D.line_s(w, td, D.Z0)
        assert np.all(s75[:, 0, 0] == 0.0) and np.max(np.abs(s75[:, 1, 0] - np.exp(-1j * w * td))) <= 4 * EPS
        for zref in (D.Z0, 50.0):
            assert np.max(np.abs(D.cascade_s(w, td, zref, rs=0.0) - D.line_s(w, td, zref))) <= 16 * EPS


def branin_zin(w, td, z0, zl):
    """Input impedance of the expansion Circuit.T documents, as a plain MNA system in numpy: unknowns p1 x1 m1 p2 x2 m2 and the four VCVS
    currents; 1 A into p1, the load zl from p2 to ground."""
    p1, x1, m1, p2, x2, m2, ia1, ib1, ia2, ib2 = range(10)
    A = np.zeros((10, 10), dtype=complex)
    d = np.exp(-1j * w * td)
    for p, x in ((p1, x1), (p2, x2)):
        A[p, p] += 1 / z0; A[p, x] -= 1 / z0; A[x, p] -= 1 / z0; A[x, x] += 1 / z0
    for x, m, ia, ib, q, xo in ((x1, m1, ia1, ib1, p2, x2), (x2, m2, ia2, ib2, p1, x1)):
        A[x, ia] += 1; A[m, ia] -= 1; A[ia, x] += 1; A[ia, m] -= 1; A[ia, q] -= 2 * d        # V(x) - V(m) = 2 V(q) delayed
        A[m, ib] += 1; A[ib, m] += 1; A[ib, xo] += d                                        # V(m) = -V(xo) delayed
    A[p2, p2] += 1 / zl
    b = np.zeros(10, dtype=complex)
    b[p1] = 1.0
    return np.linalg.solve(A, b)[p1]


def test_branin_expansion_against_the_input_impedance():
    worst = 0.0
    for zl in (75.0, 30.0, 200.0 + 50.0j):
        for f in (0.0, 1e7, 1.25e8, 2.5e8, 3.3e8, 5e8, 7.7e8):               # 250 MHz: the quarter wave of 1 ns
            w = 2.0 * np.pi * f
            ref = D.zin_line(w, 1e-9, zl)
            worst = max(worst, abs(branin_zin(w, 1e-9, D.Z0, zl) - ref) / abs(ref))
    print("Branin expansion against the input impedance: %.3g" % worst)
    assert worst <= max(16 * 1.5e-15, 64 * EPS)                            # 1.5e-15: the figure the expansion was checked to before it was built


def test_circuit_T_is_that_expansion():
    c = D.tline()
    names = [(d.type, d.name) for d in c.devices]
    assert names == [("V", "v1"), ("V", "v2"), ("R", "r1"), ("G", "t1_g1"), ("E", "t1_a1"), ("E", "t1_b1"), ("G", "t1_g2"), ("E", "t1_a2"), ("E", "t1_b2"),
                     ("R", "r2")]
    assert all(d.type != "R" for d in c.devices if d.name.startswith("t1_"))
    e = {d.name: d for d in c.devices}
    assert e["t1_a1"].nodes == ("t1_x1", "t1_m1", "p2", "0") and e["t1_a1"].params["gain"] == 2.0 and e["t1_a1"].params["delay"] == cj.Param("td")
    assert e["t1_b1"].nodes == ("t1_m1", "0", "t1_x2", "0") and e["t1_b1"].params["gain"] == -1.0
    assert e["t1_g1"].nodes == ("p1", "t1_x1", "t1_x1", "p1")               # a VCCS across its own control: a conductance
    # at DC the line is a through connection and the system regular: 1 V through rs + rs, half at each end of the line
    sol = D.HostBackend().ac(c, {"td": 1e-9}, [{}], [0.0])[0]
    assert abs(sol["p1"][0] - 0.5) <= 8 * EPS and abs(sol["p2"][0] - 0.5) <= 8 * EPS


def test_a_delay_changes_nothing_the_stamping_reads():
    plain, delayed = cj.Circuit("e"), cj.Circuit("e")
    for c, kw in ((plain, {}), (delayed, {"delay": 1e-9})):
        c.V("v", "a", "0", dc=1.0)
        c.E("e1", "b", "0", "a", "0", 3.0, **kw)
        c.G("g1", "b", "0", "a", "0", 1e-3, **kw)
        c.H("h1", "c", "0", "a", "b", 5.0, **kw)
        c.F("f1", "c", "0", "b", "0", 2.0, **kw)
        c.R("r", "c", "0", 1e3)
    assert all("delay" not in d.params for d in plain.devices) and sum("delay" in d.params for d in delayed.devices) == 4
    assert cj.Circuit().E("e", "a", "0", "b", "0", 1.0, delay=0.0).devices[0].params == {"gain": 1.0}
    sp, sd = cj.discover(plain, {}), cj.discover(delayed, {})
    assert np.array_equal(sp.rowptr, sd.rowptr) and np.array_equal(sp.colidx, sd.colidx) and np.array_equal(sp.g_slots, sd.g_slots)
    pp, pd = cj.pack_params(sp, plain, {}, np.array([27.0]), 1), cj.pack_params(sd, delayed, {}, np.array([27.0]), 1)
    assert len(pp) == len(pd) and all(np.array_equal(a, b) for a, b in zip(pp, pd))
    assert api.ac_delay_overlay(sp, plain, {}, [1.0]) is None and not api.has_delay(plain) and api.has_delay(delayed)


def test_the_helper_entry_by_entry_on_the_buffer():
    st, circ, G, C, bac, om, ovl = D.port_case("buffer")
    i_e, a = st.index_of("I_e1"), st.index_of("a")
    assert ovl.B == 1 and list(ovl.rows) == [i_e] and list(ovl.cols) == [a]                 # the branch row's gain entry; the control's ground side has none
    p = int(ovl.pos[0])
    assert st.rowptr[i_e] <= p < st.rowptr[i_e + 1] and st.colidx[p] == a
    assert G[0][p] == -D.BUF_GAIN                                                            # the stamp the delay multiplies
    assert ovl.val.shape == (1, len(om), 1)
    for f, w in enumerate(om):
        ref = (np.exp(-1j * w * D.BUF_TAU) - 1.0) * -D.BUF_GAIN
        assert abs(ovl.val[0, f, 0] - ref) <= 4 * EPS * D.BUF_GAIN
        dense = ovl.dense(0, w)
        assert dense[i_e, a] == ovl.val[0, f, 0] and np.count_nonzero(dense) == (1 if w else 0)
        assert np.array_equal(ovl.of(0)(w), dense)
    assert ovl.val[0, 0, 0] == 0.0                                                           # DC: the delay is ignored, exactly
    # the whole entry is the gain times e^{-j w tau}
    A = D.system(st, G[0], C[0], om[4], 0.0, ovl, 0)
    assert abs(A[i_e, a] - -D.BUF_GAIN * np.exp(-1j * om[4] * D.BUF_TAU)) <= 4 * EPS * D.BUF_GAIN
    # the pivot sample gains max_f |D| there, and only there
    base = api.ac_pivot_sample(st, G, C, om, D.GMIN)
    smp = D.sample(st, G, C, om, D.GMIN, ovl)
    assert smp[p] == base[p] + np.max(np.abs(ovl.val)) and np.array_equal(np.delete(smp, p), np.delete(base, p))


def test_the_helper_sums_the_devices_that_share_a_position_and_sweeps_tau():
    c = cj.Circuit("two on one")
    c.V("v", "a", "0", ac=1.0)
    c.G("g1", "b", "0", "a", "0", 2e-3, delay=cj.Param("t1"))
    c.G("g2", "b", "0", "a", "0", cj.Param("gm"), delay=3e-9)
    c.R("r", "b", "0", 1e3)
    st = cj.discover(c, {"t1": 1e-9, "gm": 1e-3})
    params = {"t1": np.array([1e-9, 2e-9]), "gm": np.array([1e-3, 4e-3])}
    w = np.array([0.0, 1e8, 3e9])
    ovl = api.ac_delay_overlay(st, c, params, w)
    b, a = st.index_of("b"), st.index_of("a")
    assert list(zip(ovl.rows, ovl.cols)) == [(b, a)] and ovl.val.shape == (2, 3, 1)
    for k in range(2):
        ref = (np.exp(-1j * w * params["t1"][k]) - 1.0) * -2e-3 + (np.exp(-1j * w * 3e-9) - 1.0) * -params["gm"][k]
        assert np.max(np.abs(ovl.val[k, :, 0] - ref)) <= 8 * EPS * 6e-3


@pytest.mark.parametrize("name", list(D.CASES))
def test_static_order_reference_on_every_system(name):
    """What the overlay kernels compute -- a static-order complex LU of G + gmin + j w C + D under the host symbolic phase's own order on the
    overlay's pivot sample, one refinement step -- on the CPU: on ``buffer`` and ``tline`` every system is far inside the gate, so the GPU
    test exempts none of them; on ``dff_delay`` at most 5 % may sit at the gate, as on the flip-flop without the buffer, and the reference
    meets the forward bound on the others by itself."""
    st, circ, G, C, bac, om, ovl = D.port_case(name)
    rp, cp = R.order_of(st, D.sample(st, G, C, om, D.GMIN, ovl))
    S, exempt, worst = len(G) * len(om), 0, 0.0
    for b in range(len(G)):
        for f, w in enumerate(om):
            A = D.system(st, G[b], C[b], w, D.GMIN, ovl, b)
            xs = R.static_order_solve_c(A, bac[b], rp, cp)
            berr = R.backward_error_c(A, xs, bac[b])
            worst = max(worst, berr)
            if berr < api.AC_BERR_MAX / 16:
                xr = R.refined_solve_c(A, bac[b])
                assert np.max(np.abs(xs - xr)) <= 16 * R.cond_inf_c(A) * EPS * np.max(np.abs(xr)), (b, f)
            else:
                exempt += 1
    print("%s: %d systems, largest static-order backward error %.3g, %d at the gate" % (name, S, worst, exempt))
    assert exempt <= (0.05 * S if name == "dff_delay" else 0)
    assert name != "dff_delay" or (st.n == 235 + 3 and len(ovl.pos) == 1)      # the flip-flop's 235 unknowns, two nodes and the buffer's branch


def test_netlist_T_and_TD():
    c, info = netlist.read_spice("""* line and delayed sources
.param td=2n zc=75
V1 in 0 AC 1
R1 in p1 50
T1 p1 0 p2 0 Z0='zc' TD='td'
E1 o 0 p2 0 2 TD=1n
G1 o 0 p2 0 1m td = 0.5n
E2 o2 0 o 0 3
R2 o 0 1k
R3 o2 0 1k
R4 p2 0 75
""")
    d = {x.name.lower(): x for x in c.devices}
    assert [x.name.lower() for x in c.devices if x.name.lower().startswith("t1_")] == ["t1_g1", "t1_a1", "t1_b1", "t1_g2", "t1_a2", "t1_b2"]
    from cadnip_jl_amd.circuit import resolve
    num = lambda v: float(resolve(v, info["params"]))
    assert num(d["t1_a1"].params["delay"]) == 2e-9 and num(d["t1_b2"].params["delay"]) == 2e-9 and num(d["t1_g1"].params["gm"]) == 1.0 / 75.0
    assert num(d["e1"].params["delay"]) == 1e-9 and d["e1"].params["gain"] == 2.0 and num(d["g1"].params["delay"]) == 0.5e-9
    assert "delay" not in d["e2"].params
    for bad in ("T1 a 0 b 0 Z0=75", "T1 a 0 b Z0=75 TD=1n", "E1 a 0 b 0 2 TX=1n"):
        with pytest.raises(ValueError):
            netlist.read_spice("* bad\nV1 a 0 1\n%s\nR1 b 0 1\n" % bad)


def test_a_line_registers_no_noise():
    c = D.tline_noise()
    st = cj.discover(c, {"td": 1e-9})
    srcs = api.noise_sources(st, c, {"td": 1e-9}, np.zeros(st.n))
    assert sorted(s[5] for s in srcs) == ["ra", "rb"]


def test_analyses_that_need_more_than_a_frequency_refuse():
    mc = api.MNACircuit(D.buffer(), {})
    with pytest.raises(NotImplementedError, match="tran"):
        api.tran(mc, (0.0, 1e-9))
    with pytest.raises(NotImplementedError, match="tran"):
        api.tran(api.CircuitSweep(api.MNACircuit(D.tline(), {"td": 1e-9}), api.Sweep(td=[1e-9, 2e-9])), (0.0, 1e-9))
    with pytest.raises(NotImplementedError, match="pz"):
        api.pz(mc, "out")
    with pytest.raises(NotImplementedError, match="sensitivity"):
        api.sensitivity(api.MNACircuit(D.tline(), {"td": 1e-9}), "p2", ["td"], [1e6])
    sol = D.HostBackend().ac(D.buffer(), {}, [{}], D.BUF_FREQS)[0]
    with pytest.raises(NotImplementedError, match="subsystem"):
        api.subsystem(sol, "out")
    with pytest.raises(NotImplementedError, match="poles_dense"):
        api.poles_dense(sol.G, sol.C, delay=sol.delay)
    with pytest.raises(NotImplementedError, match="zeros_dense"):
        api.zeros_dense(sol.G, sol.C, sol.b_ac, np.eye(sol.st.n)[0], delay=sol.delay)
    # and circuits without a delay are taken as ever
    plain = api.ACSol(sol.st, sol.G, sol.C, sol.b_ac, sol.dc_x, sol.freqs)
    assert plain.delay is None and len(api.subsystem(plain, "out")) == 5 and api.poles_dense(sol.G, sol.C).size == 1
