"""Complex references of the AC sweep tests (tests/test_ac_ref_cpu.py, tests/test_gpu_ac_lu.py, tests/test_gpu_ac_solver.py): the systems
A = G + gmin [node diagonals] + j w C of a circuit at its DC point, a refined dense solve, the componentwise backward error with complex
moduli, and the static-order complex LU the kernel k_ac_lu computes (csrc/ac_lu.hip), done on the CPU.  The circuits and grids of those
tests are defined here, once."""
import numpy as np
import scipy.linalg as sla

import cadnip_jl_amd as cj
from cadnip_jl_amd import api, benchmarks as bm, hip, netlist
from tests import circuits as tc

CLD = np.clongdouble
EPS = np.finfo(np.float64).eps

BUTTERWORTH = """*Third order low pass filter, butterworth, with w_c = 1
.param res=1
V1 vin 0 AC 1
L1 vin n1 1.5
C2 n1 0 1.3333333333333333
L3 n1 vout 0.5
R4 vout 0 '2*res'
R5 vout 0 '2*res'
"""


def butterworth_h(w):
    s = 1j * np.asarray(w, dtype=float)
    return 1.0 / ((s + 1.0) * (s * s + s + 1.0))


def inverter_with_param_vdd():
    c = tc.cmos_inverter_ac()
    for d in c.devices:
        if d.name == "vdd":
            d.params["dc"] = cj.Param("vdd")
        if d.name == "vin":
            d.params["dc"] = cj.Param("vdd", scale=0.5)
            d.params["ac"] = 1.0
    return c


def linear_zoo_ac():
    c = tc.linear_zoo()
    next(d for d in c.devices if d.type == "V").params["ac"] = 1.0
    return c


def dff_ac():
    c = bm.dff_circuit()
    next(d for d in c.devices if d.type == "V" and d.name.lower() == "vd").params["ac"] = 1.0        # the data input
    return c


def ngspice_freqs():
    from tests.test_oracle_golden import load_ngspice_inverter
    return load_ngspice_inverter()[0]


# name -> (circuit, base parameters, sweep points, frequency grid in hertz)
CASES = {
    "butterworth": (lambda: netlist.read_spice(BUTTERWORTH)[0], {}, [{}], lambda: api.acdec(20, 0.01, 10)),
    "inverter": (inverter_with_param_vdd, {"vdd": 3.3}, [{"vdd": 3.0}, {"vdd": 3.3}, {"vdd": 3.6}], ngspice_freqs),
    "linear_zoo": (linear_zoo_ac, {}, [{}], lambda: np.logspace(0, 8, 9)),
    "dff": (dff_ac, {"vdd": 5.0}, [{"vdd": 4.5, "temp": -40.0}, {"vdd": 5.0, "temp": 27.0}, {"vdd": 5.5, "temp": 125.0}],
            lambda: np.logspace(3, 12, 7)),          # S = 21: a tail workgroup for W = 2, 4, 8
}


def dense_csr(st, vals):
    """One instance's values in the structure's CSR order -> n x n."""
    A = np.zeros((st.n, st.n), dtype=np.asarray(vals).dtype)
    rows = np.repeat(np.arange(st.n), np.diff(st.rowptr))
    A[rows, np.asarray(st.colidx)] = vals
    return A


def system(st, G_csr, C_csr, w, gmin):
    """A = G + gmin on the voltage-node diagonals + j w C (complex128, dense) from CSR-ordered values."""
    G = dense_csr(st, np.asarray(G_csr, dtype=float))
    G[np.arange(st.n_nodes), np.arange(st.n_nodes)] += gmin
    return G + 1j * w * dense_csr(st, np.asarray(C_csr, dtype=float))


def pivot_sample(st, G_csr, C_csr, omegas, gmin):
    """The sample the GPU path analyses on (api.ac): max over instances of |G| + w_g |C|, gmin on the node diagonals, w_g the geometric
    mean of the non-zero grid frequencies; CSR order."""
    return api.ac_pivot_sample(st, G_csr, C_csr, omegas, gmin)


def refined_solve_c(A, b, steps=2):
    """np.linalg.solve's LU plus `steps` refinements with the residual in complex long double."""
    A = np.asarray(A, dtype=complex)
    Al, bl = A.astype(CLD), np.asarray(b, dtype=complex).astype(CLD)
    lu = sla.lu_factor(A)
    x = sla.lu_solve(lu, np.asarray(b, dtype=complex)).astype(CLD)
    for _ in range(steps):
        r = bl - Al @ x
        x = x + sla.lu_solve(lu, r.astype(complex)).astype(CLD)
    return x.astype(complex)


def backward_error_c(A, x, b):
    """max_i |b - A x|_i / (|A| |x| + |b|)_i with complex moduli, in long double; 0 / 0 = 0 (tests/lu_ref.backward_error)."""
    Al, xl, bl = np.asarray(A).astype(CLD), np.asarray(x).astype(CLD), np.asarray(b).astype(CLD)
    num = np.abs(bl - Al @ xl)
    den = np.abs(Al) @ np.abs(xl) + np.abs(bl)
    with np.errstate(invalid="ignore", divide="ignore"):
        q = np.where(num == 0, np.longdouble(0), num / den)
    return float(np.max(q))


def static_order_solve_c(A, b, rperm, cperm):
    """x of A x = b by a complex128 LU WITHOUT pivoting of A[rperm][:, cperm], then one step of iterative refinement through the same
    factors with a complex128 residual: what k_ac_lu computes, on the CPU.  A zero pivot gives non-finite values, not an exception."""
    A = np.asarray(A, dtype=complex)
    b = np.asarray(b, dtype=complex)
    M = A[np.ix_(rperm, cperm)].copy()
    n = M.shape[0]
    with np.errstate(all="ignore"):
        for k in range(n - 1):
            nzr = np.flatnonzero(M[k + 1:, k]) + k + 1
            if nzr.size:
                M[nzr, k] /= M[k, k]
                M[np.ix_(nzr, np.arange(k + 1, n))] -= np.outer(M[nzr, k], M[k, k + 1:])

        def solve(v):
            y = sla.solve_triangular(M, v[rperm], lower=True, unit_diagonal=True, check_finite=False)
            z = sla.solve_triangular(M, y, lower=False, check_finite=False)
            out = np.empty(n, dtype=complex)
            out[cperm] = z
            return out
        x = solve(b)
        return x + solve(b - A @ x)


def cond_inf_c(A):
    A = np.asarray(A, dtype=complex)
    return np.linalg.norm(A, np.inf) * np.linalg.norm(np.linalg.inv(A), np.inf)


def port_case(name):
    """The case on the CPU port (oracle/cpu_port.py): (st, G [B, nnz], C [B, nnz], b_ac [B, n], omegas) at the DC points, CSR order."""
    from tests.port_util import make_port, analyze_port
    mk, base, pts, grid = CASES[name]
    circ = mk()
    Gs, Cs, bs, st = [], [], [], None
    for pt in pts:
        p = dict(base)
        p.update({k: v for k, v in pt.items() if k != "temp"})
        st, port = make_port(circ, p, pt.get("temp", 27.0), "dcop")
        vs = [abs(float(v)) for v in p.values()] + [abs(float(d.params["dc"])) for d in circ.devices
                                                    if d.type == "V" and not hasattr(d.params.get("dc", 0.0), "name")] + [1.0]
        analyze_port(st, port, max(vs))              # the port's Newton needs a pivot order (BatchSimulator.analyze's sample)
        u, ok, _ = port.dc()
        assert ok, (name, pt)
        G, C, _, _ = port.rebuild(u, 0.0)
        port.close()
        Gs.append(G), Cs.append(C), bs.append(api.rhs_ac(st, circ, p))
    return st, np.array(Gs), np.array(Cs), np.array(bs), 2.0 * np.pi * np.asarray(grid(), dtype=float)


def order_of(st, sample_csr):
    """rperm, cperm of the order a handle takes from cadnip_analyze_values on this sample (the host symbolic phase)."""
    prog = hip.host_lu_analyze(st.n, st.rowptr, st.colidx, sample_csr, sample=True, leaves=hip.leaves_of(st))
    return prog["rperm"], prog["cperm"]
