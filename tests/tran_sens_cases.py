"""The cases of the transient-sensitivity pins (tests/test_tran_sens_ref_cpu.py: the two references of tests/tran_sens_ref.py against each
other and against a closed form; tests/test_gpu_tran_sens.py: the GPU stage against them) -- circuits with named parameters, points,
grids and the reference results, computed once per process and shared by both files.

The forced-grid conventions are those of tests/tran_exact_cases.py (whose ``Case`` carries them): ``err_mask`` all zero and no break
points, so the grid is ``TR.schedule``'s; every grid time an exact double; save times on and off the grid."""
import functools

import numpy as np

import cadnip_jl_amd as cj
from cadnip_jl_amd import benchmarks as bm
from cadnip_jl_amd.circuit import Param
from tests import tran_exact_cases as X
from tests import tran_ref as TR
from tests import tran_sens_ref as SR


def rc_param():
    """tests/circuits.py: rc_charge with its three numbers as circuit parameters"""
    c = cj.Circuit()
    c.V("v1", "vin", "0", dc=Param("V"))
    c.R("r1", "vin", "out", Param("R"))
    c.C("c1", "out", "0", Param("C"))
    return c


def rc_pulse():
    """the same behind a PULSE source (period 1 ms, edges of 50 us): break points inside every window used here"""
    c = cj.Circuit()
    c.V("v1", "vin", "0", dc=0.0, wave=("pulse", 0.0, 1.0, 1e-4, 5e-5, 5e-5, 4e-4, 1e-3), scale=Param("V"))
    c.R("r1", "vin", "out", Param("R"))
    c.C("c1", "out", "0", Param("C"))
    return c


def linear_zoo_param():
    """tests/circuits.py: linear_zoo with r2 and c1 as circuit parameters -- PWL, PULSE and SIN b(t) evaluated inside the stage"""
    c = cj.Circuit()
    c.V("v1", "a", "0", dc=1.5, wave=("pwl", [0.0, 1e-3, 2e-3, 2e-3, 5e-3], [0.0, 1.0, 1.0, 3.0, -1.0]))
    c.V("v2", "b", "0", dc=0.3, wave=("pulse", 0.0, 2.0, 1e-4, 2e-4, 3e-4, 5e-4, 2e-3))
    c.I("i1", "c", "0", dc=1e-3, wave=("sin", 0.1e-3, 1e-3, 1e3, 2e-4, 50.0, 30.0))
    c.R("r1", "a", "c", 1e3)
    c.R("r2", "b", "c", Param("r2"))
    c.C("c1", "c", "0", Param("c1"))
    c.L("l1", "c", "d", 1e-3)
    c.R("r3", "d", "0", 50.0)
    c.E("e1", "e", "0", "c", "d", 2.0)
    c.R("r4", "e", "f", 1e3)
    c.G("g1", "f", "0", "a", "b", 1e-3)
    c.R("r5", "f", "0", 3e3)
    c.H("h1", "g", "0", "f", "h", 100.0)
    c.R("r6", "h", "0", 1e3)
    c.R("r7", "g", "0", 1e3)
    c.F("f1", "k", "0", "g", "m", 3.0)
    c.R("r8", "m", "0", 500.0)
    c.R("r9", "k", "0", 1e3)
    return c


RC_DEFAULTS = {"R": 1e3, "C": 1e-6, "V": 5.0}
RC_POINTS = [{"R": 1e3, "C": 1e-6, "V": 5.0}, {"R": 2.2e3, "C": 0.5e-6, "V": 3.0}, {"R": 0.5e3, "C": 3e-6, "V": 4.0}]
ZOO_DEFAULTS = {"r2": 2.2e3, "c1": 1e-6}
ZOO_POINTS = [{"r2": 2.2e3, "c1": 1e-6}, {"r2": 1.5e3, "c1": 2e-6}, {"r2": 3.3e3, "c1": 0.5e-6}]

# grids as tests/tran_exact_cases.py; the inverter's window is shortened to 96 steps (96.0 .. 107.2 ns, picked on the CPU reference: V(in)
# passes 0.7 V at step 48, the output leaves the rail at step 56, falls from 4.3 V to 1.3 V between steps 72 and 80 and ends at 0.1 V), so
# cut-off, saturation and triode are all inside it and the references of both checked corners take seconds
CASES = {c.name: c for c in (
    X.Case("rc", rc_param, RC_POINTS, p=20, m=5, k0=0, n_steps=128, umax=5.0, orders=(1, 2, 3), start="zero"),
    X.Case("linear_zoo", linear_zoo_param, ZOO_POINTS, p=20, m=5, k0=0, n_steps=128, umax=4.0, orders=(2, 3)),
    X.Case("inverter", bm.inverter_circuit, X._pts(X.INV_CORNERS), p=36, m=3, k0=825, n_steps=96, umax=6.0, orders=(2, 3), checked=[0, 8]),
)}
DEFAULTS = {"rc": RC_DEFAULTS, "linear_zoo": ZOO_DEFAULTS, "inverter": {"vdd": 5.0}}
SENS = {"rc": ["R", "C", "V"], "linear_zoo": ["r2", "c1"], "inverter": ["vdd", "temp"]}


def pars_of(name, i):
    """[(parameter name, value)] of instance i, and the product's steps"""
    case = CASES[name]
    pars = [(nm, float(case.temp(i) if nm == "temp" else case.params(i)[nm])) for nm in SENS[name]]
    return pars, [SR.delta_of(nm, v) for nm, v in pars]


def scales_of(name, i):
    return np.array([SR.scale_of(nm, v) for nm, v in pars_of(name, i)[0]])


@functools.lru_cache(maxsize=None)
def trajectory(name, max_order, i):
    """the base trajectory of instance i on the forced grid (``TR.integrate``)"""
    case = CASES[name]
    grid, orders = case.schedule(max_order)
    tr = TR.integrate(TR.Equations(case.make(), case.params(i), case.temp(i)), X.start_state(case, i), grid, orders)
    assert np.max(np.abs(tr.U)) <= case.umax, (name, np.max(np.abs(tr.U)))
    return tr


@functools.lru_cache(maxsize=None)
def direct(name, max_order, i, dtype=SR.LD, rel_step=SR.REL_STEP):
    """``SR.direct_dense`` of instance i at the product's steps: S [K, n_steps + 1, n], unscaled"""
    case = CASES[name]
    grid, orders = case.schedule(max_order)
    pars, _ = pars_of(name, i)
    deltas = [SR.delta_of(nm, v, rel_step) for nm, v in pars]
    return SR.direct_dense(case.make(), case.params(i), case.temp(i), pars, deltas, grid, orders, trajectory(name, max_order, i).U, case.start, dtype)


@functools.lru_cache(maxsize=None)
def definition(name, max_order, i, rel_step=SR.REL_STEP, levels=False):
    """``SR.trajectory_derivative`` of instance i for every parameter: [K, n_steps + 1, n] (with ``levels`` a pair of them)"""
    case = CASES[name]
    grid, orders = case.schedule(max_order)
    pars, _ = pars_of(name, i)
    got = [SR.trajectory_derivative(case.make(), case.params(i), case.temp(i), par, SR.delta_of(par[0], par[1], rel_step), grid, orders,
                                    X.start_state(case, i), case.start, levels) for par in pars]
    return (np.array([g[0] for g in got]), np.array([g[1] for g in got])) if levels else np.array(got)


def scaled_err(name, i, got, ref):
    """worst rel_err of the scaled sensitivities p ds/dp: got, ref [K, .., n]"""
    sc = scales_of(name, i).reshape((-1,) + (1,) * (np.ndim(ref) - 1))
    return float(np.max(X.rel_err(got * sc, ref * sc)))


def be_closed_form(points, grid):
    """v(out) of the RC circuit under backward Euler, v_n = (v_{n-1} + a V) / (1 + a) with a = h / (R C) from v_0 = 0, and the exact
    derivatives of that recursion with respect to R, C and V at every grid point: (v, dv/dR, dv/dC, dv/dV), each [B, n_steps + 1], in
    extended precision"""
    LD = np.longdouble
    R, C, V = (np.array([p[k] for p in points], dtype=LD) for k in ("R", "C", "V"))
    v, dR, dC, dV = (np.zeros((len(points), len(grid)), dtype=LD) for _ in range(4))
    for m in range(1, len(grid)):
        a = LD(grid[m] - grid[m - 1]) / (R * C)
        for d, da in ((dR, -a / R), (dC, -a / C)):
            d[:, m] = ((d[:, m - 1] + da * V) * (1 + a) - (v[:, m - 1] + a * V) * da) / (1 + a) ** 2
        dV[:, m] = (dV[:, m - 1] + a) / (1 + a)
        v[:, m] = (v[:, m - 1] + a * V) / (1 + a)
    return v, dR, dC, dV
