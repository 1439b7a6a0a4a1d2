"""CPU references of the adjoint (noise) sweep tests (tests/test_lu_transpose_cpu.py, tests/test_gpu_ac_adjoint.py,
tests/test_gpu_noise_solver.py), next to tests/ac_ref.py whose systems, refined solve and backward error they reuse: the static-order
complex LU used TRANSPOSED -- what k_ac_adj computes (csrc/ac_lu.hip) -- and a numpy interpreter of the LU program together with the
transposed-solve tables of csrc/lu_transpose.hpp, which follows the tables exactly as the kernel does.  The output node of every case of
ac_ref.CASES is chosen here, once."""
import numpy as np
import scipy.linalg as sla

from tests import ac_ref as R

EPS = R.EPS

# the adjoint right-hand side of a case is e_out at this unknown.  With these nodes the static-order adjoint solve on the CPU port keeps
# every system of every case inside the forward bound (tests/test_lu_transpose_cpu.py: test_static_order_adjoint_...): none is exempt
# (linear_zoo: k ends the chain of controlled sources; the flip-flop: the complementary output, Q itself being held by a source)
OUTPUTS = {"butterworth": "vout", "inverter": "vout", "linear_zoo": "k", "dff": "Q_neg"}


def output_index(name, st):
    return st.index_of(OUTPUTS[name])


def e_out(name, st):
    c = np.zeros(st.n, dtype=complex)
    c[output_index(name, st)] = 1.0
    return c


def static_order_adjoint_c(A, c, rperm, cperm):
    """x of A^T x = c by the complex128 LU WITHOUT pivoting of M = A[rperm][:, cperm] used transposed (M^T = U^T L^T: y = c[cperm],
    U^T z = y, L^T w = z, x[rperm] = w), then one refinement step through the same factors with a complex128 residual: what k_ac_adj
    computes, on the CPU.  A zero pivot gives non-finite values, not an exception."""
    A = np.asarray(A, dtype=complex)
    c = np.asarray(c, dtype=complex)
    M = A[np.ix_(rperm, cperm)].copy()
    n = M.shape[0]
    with np.errstate(all="ignore"):
        for k in range(n - 1):
            nzr = np.flatnonzero(M[k + 1:, k]) + k + 1
            if nzr.size:
                M[nzr, k] /= M[k, k]
                M[np.ix_(nzr, np.arange(k + 1, n))] -= np.outer(M[nzr, k], M[k, k + 1:])
        MT = M.T.copy()

        def solve(v):
            z = sla.solve_triangular(MT, v[cperm], lower=True, check_finite=False)
            w = sla.solve_triangular(MT, z, lower=False, unit_diagonal=True, check_finite=False)
            out = np.empty(n, dtype=complex)
            out[rperm] = w
            return out
        x = solve(c)
        return x + solve(c - A.T @ x)


# ---- the numpy interpreter of the LU program and the transposed tables (hip.host_lu_analyze(..., transpose=True)) ---------------------------
def program_factor(prog, vals_csr):
    """L\\U [nnz_lu] complex of the CSR-ordered values by the entry program, level by level: lu[pos] = (lu[pos] - sum lu[a] lu[b]) [/ pivot]."""
    lu = np.zeros(int(prog["rowptr"][-1]), dtype=complex)
    lu[prog["load_dst"]] = np.asarray(vals_csr, dtype=complex)[prog["load_src"]]
    ent_ptr = prog["ent_ptr"]
    for l in range(len(prog["lev_ptr"]) - 1):
        new = {}
        for e in range(prog["lev_ptr"][l], prog["lev_ptr"][l + 1]):
            acc = lu[prog["ent_pos"][e]]
            for t in range(ent_ptr[e], ent_ptr[e + 1]):
                acc = acc - lu[prog["term_a"][t]] * lu[prog["term_b"][t]]
            dg = prog["ent_diag"][e]
            new[int(prog["ent_pos"][e])] = acc / lu[dg] if dg >= 0 else acc
        for pos, v in new.items():          # a level reads only what earlier levels (or the load) left
            lu[pos] = v
    return lu


def tables_solve(prog, lu, y):
    """M^-T y through the tables: U^T forward, L^T backward, a gather per unknown over its column, level by level; a level's results are
    written only after every unknown of the level has read (the kernel's lanes run a level concurrently)."""
    y = np.array(y, dtype=complex)
    cp, tp, tr, td = prog["t_colptr"], prog["t_pos"], prog["t_row"], prog["t_diag"]
    for rows, ptr, upper in ((prog["ut_rows"], prog["ut_lev_ptr"], True), (prog["lt_rows"], prog["lt_lev_ptr"], False)):
        for l in range(len(ptr) - 1):
            new = {}
            for j in rows[ptr[l]:ptr[l + 1]]:
                d = cp[j] + td[j]
                q0, q1 = (cp[j], d) if upper else (d + 1, cp[j + 1])
                acc = y[j]
                for q in range(q0, q1):
                    acc = acc - lu[tp[q]] * y[tr[q]]
                new[int(j)] = acc / lu[tp[d]] if upper else acc
            for j, v in new.items():
                y[j] = v
    return y


def tables_residual(prog, vals_csr, x, c):
    """c - A^T x over the column view of the CSR pattern"""
    r = np.array(c, dtype=complex)
    for j in range(len(c)):
        for q in range(prog["a_colptr"][j], prog["a_colptr"][j + 1]):
            r[j] -= vals_csr[prog["a_pos"][q]] * x[prog["a_row"][q]]
    return r


def tables_adjoint_solve(prog, vals_csr, c):
    """A^T x = c the kernel's way: factor by the program, transposed solve by the tables, one refinement with the column-view residual."""
    lu = program_factor(prog, vals_csr)
    rp, cp = prog["rperm"], prog["cperm"]

    def solve(v):
        out = np.empty(len(v), dtype=complex)
        out[rp] = tables_solve(prog, lu, np.asarray(v)[cp])
        return out
    x = solve(c)
    return x + solve(tables_residual(prog, vals_csr, x, c))
