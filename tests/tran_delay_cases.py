"""The circuits, cases and closed forms of the delayed-transient tests (tests/test_tran_delay_cpu.py, tests/test_gpu_tran_delay.py,
tests/test_tran_delay_port_cpu.py, tests/test_gpu_tran_delay_port.py).  Defined here, once.

Every time constant is a power of two times another, so grid points, kinks and their images are exact doubles."""
import math

import numpy as np

import cadnip_jl_amd as cj
from cadnip_jl_amd import benchmarks as bm
from tests import tran_ref as TR

TD = 2.0 ** -30                      # 0.93 ns: the unit of every delay here


def ramp(t, ta, tb, v=1.0):
    """the PWL ramp 0 -> v between ta and tb"""
    return v * np.clip((np.asarray(t, dtype=float) - ta) / (tb - ta), 0.0, 1.0)


def pwl_ramp(ta, tb, v=1.0, t_end=1.0):
    return ("pwl", [0.0, ta, tb, t_end], [0.0, 0.0, v, v])


# ---- buffer: PWL ramp -> R -> E(gain 2, delay tau) -> R -> C: tests/ac_delay_ref.buffer()'s topology ---------------------------------------
BUF_R, BUF_C, BUF_GAIN = 1e3, 2.0 ** -30 / 1e3, 2.0          # R C = TD


def buffer(wave, tau=cj.Param("tau")):
    c = cj.Circuit("delayed buffer, transient")
    c.V("vin", "in", "0", dc=0.0, wave=wave)
    c.R("r1", "in", "a", BUF_R)
    c.E("e1", "b", "0", "a", "0", BUF_GAIN, delay=tau)
    c.R("r2", "b", "out", BUF_R)
    c.C("c1", "out", "0", BUF_C)
    return c


def rc_ramp_response(t, ta, tb, v, rc):
    """v_C of an R C driven from rest by the ramp 0 -> v between ta and tb: the ramp response from ta minus the one from tb"""
    def from_(t0):
        x = np.maximum(np.asarray(t, dtype=float) - t0, 0.0)
        return x - rc * (-np.expm1(-x / rc))
    return v / (tb - ta) * (from_(ta) - from_(tb))


def buffer_out(t, ta, tb, tau, v=1.0):
    """V(out) of ``buffer(pwl_ramp(ta, tb, v), tau)``: the R C response to the gained ramp, tau later"""
    return rc_ramp_response(np.asarray(t, dtype=float) - tau, ta, tb, BUF_GAIN * v, BUF_R * BUF_C)


# ---- line: PWL ramp -> rs -> ideal line (z0 = 50) -> rl to ground (None: open end) ----------------------------------------------------------
LINE_Z0 = 50.0


def line(wave, rs, rl, td=cj.Param("td")):
    c = cj.Circuit("line")
    c.V("vs", "s", "0", dc=0.0, wave=wave)
    c.R("rs", "s", "p1", rs)
    c.T("t1", "p1", "0", "p2", "0", LINE_Z0, td)
    if rl is not None:
        c.R("rl", "p2", "0", rl)
    return c


def lattice(vs, t, rs, rl, td, z0=LINE_Z0):
    """(near end, far end) of the lattice diagram: the wave A vs launched into the line (A = z0 / (z0 + rs)) bounces between the reflection
    coefficients rho_l at the far and rho_s at the near end,
      far  = A (1 + rho_l) sum_k (rho_s rho_l)^k vs(t - (2 k + 1) td),   near = A [vs(t) + (1 + rho_s) rho_l sum_k (rho_s rho_l)^k vs(t - (2 k + 2) td)],
    finite sums for a vs that is zero before t = 0.  ``vs``: a function of time; ``rl`` None: the open end (rho_l = 1)."""
    t = np.asarray(t, dtype=float)
    a, rho_s = z0 / (z0 + rs), (rs - z0) / (rs + z0)
    rho_l = 1.0 if rl is None else (rl - z0) / (rl + z0)
    near, far = a * vs(t), np.zeros_like(t)
    for k in range(int(math.ceil(float(np.max(t)) / (2.0 * td))) + 1):
        g = (rho_s * rho_l) ** k
        far = far + a * (1.0 + rho_l) * g * vs(t - (2 * k + 1) * td)
        near = near + a * (1.0 + rho_s) * rho_l * g * vs(t - (2 * k + 2) * td)
    return near, far


# ---- the forced-grid cases (tests/test_gpu_tran_delay.py: the GPU; tests/test_tran_delay_port_cpu.py: the CPU port) --------------------------
def _sin(freq):
    return ("sin", 0.0, 1.0, freq, 0.0, 0.0, 0.0)


def buffer_case():
    """SIN into the delayed buffer; tau per instance: 3 final steps (tq lands on ring times), exactly hmax, and 2.3 steps"""
    hmax = TD / 16
    return dict(make=lambda: buffer(_sin(0.5 / TD)), base={"tau": 3 * hmax}, points=[{"tau": 3 * hmax}, {"tau": hmax}, {"tau": 2.3 * hmax}],
                h0=hmax / 64, hmax=hmax, n_steps=96, umax=2.5, start="zero")


def line_case():
    """the mismatched line (30 ohm into 50 ohm into 100 ohm), td swept"""
    hmax = TD / 8
    return dict(make=lambda: line(pwl_ramp(0.3 * TD, 0.9 * TD), 30.0, 100.0), base={"td": TD}, points=[{"td": TD}, {"td": 2.5 * TD}],
                h0=hmax / 64, hmax=hmax, n_steps=128, umax=1.5, start="zero")


def line_inverter(wave=("pwl", [0.0, 4 * TD, 16 * TD, 1.0], [0.0, 0.0, 5.0, 5.0])):
    """a 5 V ramp through 50 ohm and a matched line into the gates of tests/tran_exact_cases' sp_mos1 inverter"""
    c = cj.Circuit("line into an inverter")
    c.V("VVDD", "VDD", "0", dc=cj.Param("vdd"))
    c.V("VS", "S", "0", dc=0.0, wave=wave)
    c.R("RS", "S", "P1", 50.0)
    c.T("T1", "P1", "0", "D", "0", 50.0, cj.Param("td"))
    c.MOS1("X_tn", "Q", "D", "0", "0", bm.NFET_06V0, w=0.36e-6, l=0.6e-6)
    c.MOS1("X_tp", "Q", "D", "VDD", "VDD", bm.PFET_06V0, w=0.495e-6, l=0.5e-6)
    c.C("CQ", "Q", "0", 1e-15)
    for nm, d, g, s, W, L in (("tn", "Q", "D", "0", 0.36e-6, 0.6e-6), ("tp", "Q", "D", "VDD", 0.495e-6, 0.5e-6)):
        cg = bm.lumped_gate_cap(W, L)
        c.C("Cgs_" + nm, g, s, cg)
        c.C("Cgd_" + nm, g, d, cg)
    return c


def inverter_case():
    """nonlinear: several Newton rounds per step on one delayed value.  116 ps steps as tran_exact_cases' inverter; the edge reaches the gates
    after td = 4 TD / 5 TD and the window (0 .. 18 TD) holds the turn-on of both transistors"""
    hmax = TD / 8
    return dict(make=line_inverter, base={"vdd": 5.0, "td": 4 * TD}, points=[{"vdd": 5.0, "temp": 27.0, "td": 4 * TD}, {"vdd": 4.5, "temp": 125.0, "td": 5 * TD}],
                h0=hmax / 8, hmax=hmax, n_steps=144, umax=6.0, start="dc")


def ghf_circuit():
    """a delayed G, a delayed H and a delayed F in one chain: voltage- and current-controlled, current- and voltage-output stamps"""
    c = cj.Circuit("delayed G, H, F")
    c.V("vin", "in", "0", dc=0.0, wave=_sin(0.25 / TD))
    c.R("r1", "in", "a", 1e3)
    c.R("ra", "a", "0", 1e3)
    c.G("g1", "c", "0", "a", "0", 2e-3, delay=cj.Param("t1"))
    c.R("rc", "c", "0", 1e3)
    c.C("cc", "c", "0", TD / 1e3)
    c.R("rs", "c", "e", 1e3)
    c.H("h1", "d", "0", "e", "0", 2e3, delay=cj.Param("t2"))          # senses the current of rs into its zero-volt branch e -> 0
    c.R("rd", "d", "f", 1e3)
    c.F("f1", "g", "0", "f", "0", 1.5, delay=1.25 * TD)               # senses the current of rd
    c.R("rg", "g", "0", 1e3)
    c.C("cg", "g", "0", TD / 2e3)
    return c


def ghf_case():
    hmax = TD / 16
    return dict(make=ghf_circuit, base={"t1": TD, "t2": TD}, points=[{"t1": 0.5 * TD, "t2": 0.7 * TD}, {"t1": hmax, "t2": 2 * TD}],
                h0=hmax / 64, hmax=hmax, n_steps=96, umax=2.5, start="zero")


def tau_tol(case):
    return min(1e-11, 1e-10 / (case["n_steps"] * 0.33 * (1.0 + case["umax"])))


def case_params(case, i):
    p = dict(case["base"])
    p.update({k: v for k, v in case["points"][i].items() if k != "temp"})
    return p


def save_times(case, order):
    """every grid point, and off-grid times inside step 1, step 2, the doubling phase and the constant phase (tran_exact_cases.Case.save_times)"""
    g = TR.schedule(0.0, case["h0"], case["hmax"], case["n_steps"], order)[0]
    n = case["n_steps"]
    off = [g[k - 1] + f * (g[k] - g[k - 1]) for k, f in ((1, 0.25), (2, 0.25), (3, 0.5), (n - 3, 0.8))]
    return np.sort(np.concatenate([g, off]))


# ---- the error-controlled cases (tests/test_tran_delay_port_cpu.py: their conditions, on the port; tests/test_gpu_tran_delay_port.py) --------
# Controller on: err_mask = the differential unknowns, tests/test_gpu_tran_parity.ABSTOL, the tolerances below.  ``hmax`` is what the GPU is
# given; the run is clamped to the smallest delay of the BATCH (cadnip_tran_run), which the port is told
# (tests/port_util.batch_tau_min, port_ec_run's ``hmax_batch``).
EC_ABSTOL = dict(vntol=1e-6, iabstol=1e-9, chgtol=1e-6)


def ec_case(name):
    if name == "buffer_sin":
        # a sine of period 2 TD into R C = TD; tau = TD / 32 is the batch's smallest delay, far below hmax = TD and below the steps the error
        # test allows on the smooth stretches: the clamp binds.  The sine starts with a slope, so the delayed drive has a kink at t0 + tau
        # that no break point announces (breaks = ()): rejected steps
        return dict(make=lambda: buffer(_sin(0.5 / TD)), base={"tau": TD}, points=[{"tau": 0.75 * TD}, {"tau": TD / 32}, {"tau": 1.3 * TD}],
                    tspan=(0.0, 4 * TD), hmax=TD, h0=TD / 1024, reltol=1e-4, max_newton=10, max_order=2, breaks=None, vscale=1.0, start="zero",
                    save_extra=[TD / 32, 0.75 * TD, 1.3 * TD])
    if name == "buffer_sin_five":
        # the batch shapes: five settings in a cycle (5 is coprime with 64), the second the smallest delay
        return dict(ec_case("buffer_sin"), points=[{"tau": 0.75 * TD}, {"tau": TD / 32}, {"tau": 1.3 * TD}, {"tau": 0.4 * TD}, {"tau": 2.1 * TD}],
                    save_extra=[TD / 32, 0.4 * TD, 0.75 * TD, 1.3 * TD, 2.1 * TD])
    if name == "buffer_sin_depth":
        # the ring-depth rule: instance 1 has the longest delay, in seconds and in steps
        return dict(ec_case("buffer_sin"), points=[{"tau": 0.25 * TD}, {"tau": 1.3 * TD}, {"tau": 0.5 * TD}], save_extra=[0.25 * TD, 0.5 * TD, 1.3 * TD])
    if name == "ghf_five":
        return dict(ec_case("ghf"), max_order=2,
                    points=[{"t1": 0.5 * TD, "t2": 0.7 * TD}, {"t1": TD / 16, "t2": 2 * TD}, {"t1": 0.3 * TD, "t2": TD}, {"t1": TD, "t2": 0.2 * TD}, {"t1": 1.7 * TD, "t2": 0.9 * TD}])
    if name == "ghf":
        return dict(make=ghf_circuit, base={"t1": TD, "t2": TD}, points=[{"t1": 0.5 * TD, "t2": 0.7 * TD}, {"t1": TD / 16, "t2": 2 * TD}],
                    tspan=(0.0, 6 * TD), hmax=TD, h0=TD / 1024, reltol=1e-4, max_newton=10, max_order=(2, 3), breaks=None, vscale=1.0, start="zero",
                    save_extra=[0.5 * TD, 0.7 * TD, 1.25 * TD, 2 * TD])
    if name in ("line_inverter_breaks", "line_inverter_tight_newton"):
        tight = name.endswith("tight_newton")
        return dict(make=lambda: line_inverter(("pwl", [0.0, 2 * TD, 3 * TD, 1.0], [0.0, 0.0, 5.0, 5.0])), base={"vdd": 5.0, "td": 4 * TD},
                    points=[{"vdd": 5.0, "temp": 27.0, "td": 4 * TD}, {"vdd": 4.5, "temp": 125.0, "td": 5 * TD}],
                    tspan=(0.0, 12 * TD), hmax=TD, h0=TD / 1024, reltol=1e-4, max_newton=3 if tight else 10, max_order=2, breaks="delayed", vscale=5.0,
                    start="dc", save_extra=[4 * TD, 5 * TD])
    raise KeyError(name)


def ec_point(case, i):
    """(params, temp) of point i (points may cycle: i is taken modulo their number)"""
    pt = case["points"][i % len(case["points"])]
    p = dict(case["base"])
    p.update({k: v for k, v in pt.items() if k != "temp"})
    return p, pt.get("temp", 27.0)
