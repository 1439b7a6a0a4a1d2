"""The circuits and closed forms of the delayed-transient tests (tests/test_tran_delay_cpu.py, tests/test_gpu_tran_delay.py).  Defined here, once.

Every time constant is a power of two times another, so grid points, kinks and their images are exact doubles."""
import math

import numpy as np

import cadnip_jl_amd as cj

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
