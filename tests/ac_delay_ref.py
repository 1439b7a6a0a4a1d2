"""The cases of the delayed-element tests (tests/test_ac_delay_cpu.py, tests/test_gpu_ac_delay.py, tests/test_gpu_ac_delay_api.py): circuits
with delayed controlled sources and ideal transmission lines, their closed forms, and their systems A = G + gmin + j w C + D(w) on the CPU
port -- tests/ac_ref.py's references with the overlay of api.ac_delay_overlay added.  Defined here, once."""
import numpy as np

import cadnip_jl_amd as cj
from cadnip_jl_amd import api
from tests import ac_ref as R

EPS = R.EPS
GMIN = 1e-12

# ---- buffer: V (AC 1) -> R -> delayed E (gain 2) -> R -> C: 6 unknowns, H = 2 e^{-j w tau} / (1 + j w R C) ---------------------------------
BUF_R, BUF_C, BUF_TAU, BUF_GAIN = 1e3, 1e-12, 0.7e-9, 2.0
BUF_FREQS = np.concatenate([[0.0], np.logspace(6, 9, 8)])          # 9 frequencies, DC among them


def buffer():
    c = cj.Circuit("delayed buffer")
    c.V("vin", "in", "0", dc=0.0, ac=1.0)
    c.R("r1", "in", "a", BUF_R)
    c.E("e1", "b", "0", "a", "0", BUF_GAIN, delay=BUF_TAU)
    c.R("r2", "b", "out", BUF_R)
    c.C("c1", "out", "0", BUF_C)
    return c


def buffer_h(w):
    w = np.asarray(w, dtype=float)
    return BUF_GAIN * np.exp(-1j * w * BUF_TAU) / (1.0 + 1j * w * BUF_R * BUF_C)


# ---- tline: two V-source ports, series resistors, a 75 ohm line whose delay is swept -------------------------------------------------------
Z0 = 75.0
TL_RS = 30.0                                                        # the series resistors: the source impedance of port 1, the load of port 2
TL_TDS = (0.5e-9, 1e-9, 2e-9)
TL_FREQS = np.array([0.0, 5e7, 1.25e8, 2.5e8, 5e8, 7.7e8, 1e9])     # 250 MHz: the quarter-wave point of the middle delay


def tline(rs=TL_RS):
    """v1 - r1 - line - r2 - v2.  The series resistors are part of the two-port: the admittance matrix of a bare lossless line does not exist
    where sin(w td) = 0 -- at DC and at every half wave, both on the grid -- so ports on the line's own terminals cannot be measured through y"""
    c = cj.Circuit("transmission line")
    c.V("v1", "s1", "0", dc=0.0, ac=1.0)
    c.V("v2", "s2", "0", dc=0.0)
    c.R("r1", "s1", "p1", rs)
    c.T("t1", "p1", "0", "p2", "0", Z0, cj.Param("td"))
    c.R("r2", "p2", "s2", rs)
    return c


def zin_line(w, td, zl, z0=Z0):
    """Z0 (ZL + j Z0 tan wt) / (Z0 + j ZL tan wt) in the form that stays finite at the quarter wave"""
    cth, sth = np.cos(w * td), np.sin(w * td)
    return z0 * (zl * cth + 1j * z0 * sth) / (z0 * cth + 1j * zl * sth)


def line_s(w, td, zref, z0=Z0):
    """S of the bare line against zref: the textbook mismatch expressions (S11 = 0, S21 = e^{-j w td} for zref = z0)"""
    gam = (z0 - zref) / (z0 + zref)
    e1, e2 = np.exp(-1j * w * td), np.exp(-2j * w * td)
    s11 = gam * (1.0 - e2) / (1.0 - gam * gam * e2)
    s21 = (1.0 - gam * gam) * e1 / (1.0 - gam * gam * e2)
    return np.array([[s11, s21], [s21, s11]]).transpose(2, 0, 1) if np.ndim(w) else np.array([[s11, s21], [s21, s11]])


def cascade_s(w, td, zref, rs=TL_RS, z0=Z0):
    """S of series rs - line - series rs against zref, from the chain matrix [[1, rs], [0, 1]] [[cos, j z0 sin], [j sin / z0, cos]] [[1, rs],
    [0, 1]]: S11 = (A + B / zref - C zref - D) / den, S21 = 2 / den, den = A + B / zref + C zref + D.  rs = 0 is ``line_s``."""
    cth, sth = np.cos(w * td), np.sin(w * td)
    a = cth + 1j * rs * sth / z0
    b = 2.0 * rs * cth + 1j * sth * (z0 + rs * rs / z0)
    c = 1j * sth / z0
    den = 2.0 * a + b / zref + c * zref
    s11, s21 = (b / zref - c * zref) / den, 2.0 / den
    return np.array([[s11, s21], [s21, s11]]).transpose(2, 0, 1)


def tline_noise():
    """the line between two matched noisy resistors: S_v at the far end = 2 k T z0 at every frequency, half from each resistor"""
    c = cj.Circuit("matched line")
    c.R("ra", "p1", "0", Z0)
    c.T("t1", "p1", "0", "p2", "0", Z0, cj.Param("td"))
    c.R("rb", "p2", "0", Z0)
    return c


# ---- dff_delay: the flip-flop with a delayed buffer on Q into an RC load ---------------------------------------------------------------------
DFF_TAU = 50e-12


def dff_delay():
    c = R.dff_ac()
    c.E("ebuf", "qd", "0", "Q", "0", 1.0, delay=DFF_TAU)
    c.R("rld", "qd", "qo", 1e3)
    c.C("cld", "qo", "0", 1e-13)
    return c


# name -> (circuit, base parameters, sweep points, frequency grid in hertz), as ac_ref.CASES
CASES = {
    "buffer": (buffer, {}, [{}], lambda: BUF_FREQS),
    "tline": (tline, {"td": TL_TDS[1]}, [{"td": t} for t in TL_TDS], lambda: TL_FREQS),          # S = 21: a tail workgroup for W = 2, 4, 8
    "dff_delay": (dff_delay, R.CASES["dff"][1], R.CASES["dff"][2], R.CASES["dff"][3]),
}


def port_points(circ, base, pts):
    """The circuit at its DC points on the CPU port, as ac_ref.port_case: (st, G [B, nnz], C [B, nnz] in CSR order, the points' parameters,
    the DC solutions)."""
    from tests.port_util import make_port, analyze_port
    Gs, Cs, st, ps, us = [], [], None, [], []
    for pt in pts:
        p = dict(base)
        p.update({k: v for k, v in pt.items() if k != "temp"})
        st, port = make_port(circ, p, pt.get("temp", 27.0), "dcop")
        vs = [abs(float(v)) for v in p.values()] + [abs(float(d.params["dc"])) for d in circ.devices
                                                    if d.type == "V" and not hasattr(d.params.get("dc", 0.0), "name")] + [1.0]
        analyze_port(st, port, max(vs))
        u, ok, _ = port.dc()
        assert ok, (circ.title, pt)
        G, C, _, _ = port.rebuild(u, 0.0)
        port.close()
        Gs.append(G), Cs.append(C), ps.append(p), us.append(u)
    return st, np.array(Gs), np.array(Cs), ps, us


def overlay_of(st, circ, ps, om):
    return api.ac_delay_overlay(st, circ, {k: np.array([p[k] for p in ps], dtype=float) for k in ps[0]}, om, len(ps))


def port_case(name):
    """The case on the CPU port and its overlay from the host helper: (st, circuit, G [B, nnz], C [B, nnz], b_ac [B, n], omegas,
    AcDelayOverlay)."""
    mk, base, pts, grid = CASES[name]
    circ = mk()
    st, G, C, ps, _ = port_points(circ, base, pts)
    om = 2.0 * np.pi * np.asarray(grid(), dtype=float)
    return st, circ, G, C, np.array([api.rhs_ac(st, circ, p) for p in ps]), om, overlay_of(st, circ, ps, om)


def system(st, G_csr, C_csr, w, gmin, ovl, b):
    """ac_ref.system plus the overlay's addend of point b at w"""
    return R.system(st, G_csr, C_csr, w, gmin) + ovl.dense(b, w)


def sample(st, G, C, om, gmin, ovl):
    """the pivot sample of the GPU path under an overlay (CSR order)"""
    return api._overlay_sample(api.ac_pivot_sample(st, G, C, om, gmin), ovl)


# ---- the closed forms, through any path --------------------------------------------------------------------------------------------------
# A backend is four callables that return one result per point: ac(circ, base, pts, freqs) -> [ACSol], network(circ, base, pts, ports, freqs,
# z0) -> [NetworkSol], noise(circ, base, pts, output, freqs) -> [NoiseSol], network_noise(circ, base, pts, ports, freqs, z0) -> [NetworkNoiseSol].
# The closed-form checks run with gmin = 0: a gmin of 1e-12 S on a node fed through 75 ohm is itself an error of 1e-10, not rounding.
TL_PTS = [{"td": t} for t in TL_TDS]
TEMP_C = 27.0
KT = api.K_BOLTZMANN * (TEMP_C + 273.15)


class HostBackend:
    """the dense host path on the CPU port's matrices"""

    def _dense(self, circ, base, pts, freqs):
        st, G, C, ps, us = port_points(circ, base, pts)
        ovl = overlay_of(st, circ, ps, 2.0 * np.pi * np.asarray(freqs, dtype=float))
        return st, [R.dense_csr(st, g) for g in G], [R.dense_csr(st, c) for c in C], ps, us, ovl

    def ac(self, circ, base, pts, freqs):
        st, G, C, ps, us, ovl = self._dense(circ, base, pts, freqs)
        return [api.ACSol(st, G[k], C[k], api.rhs_ac(st, circ, ps[k]), us[k], freqs, ovl.of(k)) for k in range(len(pts))]

    def network(self, circ, base, pts, ports, freqs, z0):
        st, G, C, ps, us, ovl = self._dense(circ, base, pts, freqs)
        return [api.network_solve(st, G[k], C[k], ports, freqs, z0, us[k], ovl.of(k)) for k in range(len(pts))]

    def noise(self, circ, base, pts, output, freqs):
        st, G, C, ps, us, ovl = self._dense(circ, base, pts, freqs)
        return [api.noise_solve(st, G[k], C[k], api.noise_sources(st, circ, ps[k], us[k], TEMP_C), output, freqs, None, TEMP_C, delay=ovl.of(k))
                for k in range(len(pts))]

    def network_noise(self, circ, base, pts, ports, freqs, z0):
        st, G, C, ps, us, ovl = self._dense(circ, base, pts, freqs)
        return [api.network_noise_solve(st, G[k], C[k], api.noise_sources(st, circ, ps[k], us[k], TEMP_C), ports, freqs, z0, TEMP_C, us[k], None,
                                        ovl.of(k)) for k in range(len(pts))]


def closed_form_errors(be):
    """The largest error of a backend against each closed form, relative to the closed form's own size: {figure: error}.  ``buffer`` and
    ``tline_zin`` are relative per frequency; the S-parameter figures are absolute (|S| <= 1, S11 = 0 is among them); the noise figures are
    relative to 2 k T z0 and to the largest entry of cy."""
    out = {}
    sol = be.ac(buffer(), {}, [{}], BUF_FREQS)[0]
    href = buffer_h(2.0 * np.pi * BUF_FREQS)
    out["buffer"] = float(np.max(np.abs(sol["out"] - href) / np.abs(href)))
    err = 0.0
    for td, sol in zip(TL_TDS, be.ac(tline(), {"td": TL_TDS[1]}, TL_PTS, TL_FREQS)):
        vin, vs = sol["p1"], sol["s1"]
        zin, zref = vin * TL_RS / (vs - vin), zin_line(2.0 * np.pi * TL_FREQS, td, TL_RS)
        err = max(err, float(np.max(np.abs(zin - zref) / np.abs(zref))))
    out["tline_zin"] = err
    for zref, key in ((Z0, "tline_s75"), (50.0, "tline_s50")):
        err = 0.0
        for td, ns in zip(TL_TDS, be.network(tline(), {"td": TL_TDS[1]}, TL_PTS, ["v1", "v2"], TL_FREQS, zref)):
            err = max(err, float(np.max(np.abs(ns.s - cascade_s(2.0 * np.pi * TL_FREQS, td, zref)))))
        out[key] = err
    err = 0.0
    for ns in be.noise(tline_noise(), {"td": TL_TDS[1]}, TL_PTS, "p2", TL_FREQS):
        err = max(err, float(np.max(np.abs(ns["onoise"] - 2.0 * KT * Z0))) / (2.0 * KT * Z0))
        for nm in ("ra", "rb"):
            err = max(err, float(np.max(np.abs(ns[nm] - KT * Z0))) / (2.0 * KT * Z0))
    out["tline_noise"] = err
    err = 0.0
    for td, nn in zip(TL_TDS, be.network_noise(tline(rs=Z0), {"td": TL_TDS[1]}, TL_PTS, ["v1", "v2"], TL_FREQS, Z0)):
        e1 = np.exp(-1j * 2.0 * np.pi * TL_FREQS * td)
        t1 = np.stack([-0.5 * np.ones_like(e1), 0.5 * e1], axis=1)           # transfers of r1's noise current to the two port currents
        t2 = np.stack([0.5 * e1, -0.5 * np.ones_like(e1)], axis=1)           # ... of r2's
        cref = 4.0 * KT / Z0 * (t1[:, :, None] * np.conj(t1[:, None, :]) + t2[:, :, None] * np.conj(t2[:, None, :]))
        err = max(err, float(np.max(np.abs(nn.cy - cref)) / np.max(np.abs(cref))))
    out["tline_netnoise"] = err
    return out


# what HostBackend measures (tests/test_ac_delay_cpu.py re-measures and asserts it on every run); the bound of any other path against the same
# closed form is 16 x the figure and not below 64 eps -- the project's margin for another summation order
HOST_MEASURED = {"buffer": 3.2e-16, "tline_zin": 1.1e-15, "tline_s75": 5.0e-16, "tline_s50": 4.8e-16, "tline_noise": 3.1e-16, "tline_netnoise": 2.2e-16}


def closed_form_bound(key):
    return max(16.0 * HOST_MEASURED[key], 64.0 * EPS)
