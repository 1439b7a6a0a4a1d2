"""High-precision reference of the per-op LU tests (tests/test_gpu_lu_kernels.py): J = G + gamma C per instance in long double, a float64
dense LU solve with two steps of iterative refinement whose residuals are long double, and the componentwise backward error."""
import numpy as np
import scipy.linalg as sla

LD = np.longdouble


def pattern(st):
    """(rows, cols) of the reference's CSC nz order (the order of Handle.get_GCb)."""
    return np.asarray(st.ref_rowval), np.repeat(np.arange(st.n), np.diff(st.ref_colptr))


def assemble(G, Cm, gamma):
    """[B, nnz] values of G + gamma C in long double."""
    return np.asarray(G, dtype=LD) + np.asarray(gamma, dtype=LD)[:, None] * np.asarray(Cm, dtype=LD)


def dense(vals, rows, cols, n):
    """One instance's [nnz] values -> n x n (long double)."""
    A = np.zeros((n, n), dtype=LD)
    np.add.at(A, (rows, cols), np.asarray(vals, dtype=LD))
    return A


def refined_solve(A, b, steps=2):
    """x of A x = b: float64 LU with partial pivoting, then `steps` refinements x += A^-1 (b - A x) with r = b - A x in long double."""
    A = np.asarray(A, dtype=LD)
    b = np.asarray(b, dtype=LD)
    lu = sla.lu_factor(A.astype(np.float64))
    x = sla.lu_solve(lu, b.astype(np.float64)).astype(LD)
    for _ in range(steps):
        r = b - A @ x
        x = x + sla.lu_solve(lu, r.astype(np.float64)).astype(LD)
    return x


def cond_inf(A):
    """kappa_inf(A) = ||A||_inf ||A^-1||_inf (float64)."""
    A64 = np.asarray(A, dtype=np.float64)
    return np.linalg.norm(A64, np.inf) * np.linalg.norm(np.linalg.inv(A64), np.inf)


def backward_error(vals, rows, cols, x, b):
    """omega = max_i |b - A x|_i / (|A| |x| + |b|)_i per instance, in long double; vals [B, nnz] (long double), x, b [B, n].
    A row with 0 / 0 counts as 0."""
    B, n = np.shape(x)
    xl, bl = np.asarray(x, dtype=LD), np.asarray(b, dtype=LD)
    order = np.argsort(rows, kind="stable")
    r_sorted = rows[order]
    starts = np.searchsorted(r_sorted, np.arange(n))
    assert np.all(np.diff(np.append(starts, len(rows))) > 0), "a row without entries"
    prod = vals[:, order] * xl[:, cols[order]]
    ax = np.add.reduceat(prod, starts, axis=1)
    aax = np.add.reduceat(np.abs(prod), starts, axis=1)
    num = np.abs(bl - ax)
    den = aax + np.abs(bl)
    with np.errstate(invalid="ignore", divide="ignore"):
        w = np.where(num == 0, LD(0), num / den)
    return np.max(w, axis=1).astype(np.float64)


def static_order_solve(A, b, rperm, cperm):
    """x of A x = b by a float64 LU WITHOUT pivoting of A[rperm][:, cperm]: the static pivot order the GPU kernels follow (row i of the
    factored matrix is row rperm[i], column j is column cperm[j]).  Its backward error is what that order allows, whatever the kernel."""
    M = np.asarray(A, dtype=np.float64)[np.ix_(rperm, cperm)].copy()
    n = M.shape[0]
    for k in range(n - 1):
        M[k + 1:, k] /= M[k, k]
        M[k + 1:, k + 1:] -= np.outer(M[k + 1:, k], M[k, k + 1:])
    y = sla.solve_triangular(M, np.asarray(b, dtype=np.float64)[rperm], lower=True, unit_diagonal=True)
    z = sla.solve_triangular(M, y, lower=False)
    x = np.empty(n)
    x[cperm] = z
    return x
