"""The transposed-solve tables of csrc/lu_transpose.hpp, host only (hip.host_lu_analyze(..., transpose=True)): on the LU programs of the
four patterns of ac_ref.CASES (the CPU port's pivot sample, the handle's leaf-first order) plus a 1 x 1 and a diagonal matrix -- the
column view, both level schedules, a numpy interpreter of the tables (tests/noise_ref.py) against a dense transposed solve, the transposed
residual -- and the CPU reference of the adjoint kernel (noise_ref.static_order_adjoint_c) against the refined dense solve on the port's
systems, with the measurement behind api.NOISE_BERR_MAX."""
import numpy as np
import pytest
import scipy.linalg as sla

from cadnip_jl_amd import api, hip
from tests import ac_ref as R
from tests import noise_ref as N

EPS = R.EPS
GMIN = 1e-12
_CASE, _PROG = {}, {}


def case(name):
    if name not in _CASE:
        st, G, C, bac, om = R.port_case(name)
        sample = R.pivot_sample(st, G, C, om, GMIN)
        prog = hip.host_lu_analyze(st.n, st.rowptr, st.colidx, sample, sample=True, leaves=hip.leaves_of(st), transpose=True)
        _CASE[name] = (st, G, C, om, sample, prog)
    return _CASE[name]


def pattern(name):
    """(n, rowptr, colidx, magnitudes the order was chosen on, program with the transposed tables)"""
    if name not in _PROG:
        if name == "one":
            n, rowptr, colidx, mag = 1, np.array([0, 1]), np.array([0]), np.array([2.0])
        elif name == "diagonal":
            n, rowptr, colidx, mag = 5, np.arange(6), np.arange(5), np.array([1.0, 3.0, 0.5, 2.0, 7.0])
        else:
            st, _, _, _, mag, prog = case(name)
            _PROG[name] = (st.n, np.asarray(st.rowptr), np.asarray(st.colidx), mag, prog)
            return _PROG[name]
        _PROG[name] = (n, rowptr, colidx, mag, hip.host_lu_analyze(n, rowptr, colidx, mag, sample=True, transpose=True))
    return _PROG[name]


PATTERNS = list(R.CASES) + ["one", "diagonal"]


@pytest.mark.parametrize("name", PATTERNS)
def test_column_view_is_a_permutation_with_ascending_rows_and_the_diagonal_in_place(name):
    n, rowptr, colidx, _, p = pattern(name)
    nnz_lu = int(p["rowptr"][-1])
    assert len(p["t_colptr"]) == n + 1 and p["t_colptr"][0] == 0 and p["t_colptr"][-1] == nnz_lu and len(p["t_diag"]) == n
    assert np.array_equal(np.sort(p["t_pos"]), np.arange(nnz_lu))
    row_of = np.repeat(np.arange(n), np.diff(p["rowptr"]))
    assert np.array_equal(p["t_row"], row_of[p["t_pos"]])
    for j in range(n):
        q0, q1 = p["t_colptr"][j], p["t_colptr"][j + 1]
        assert np.all(p["col"][p["t_pos"][q0:q1]] == j) and np.all(np.diff(p["t_row"][q0:q1]) > 0)
        d = q0 + p["t_diag"][j]
        assert q0 <= d < q1 and p["t_row"][d] == j and p["t_pos"][d] == p["diag"][j]
    # the column view of the CSR pattern
    nnz = int(rowptr[-1])
    assert np.array_equal(np.sort(p["a_pos"]), np.arange(nnz)) and p["a_colptr"][-1] == nnz
    assert np.array_equal(p["a_row"], np.repeat(np.arange(n), np.diff(rowptr))[p["a_pos"]])
    for j in range(n):
        assert np.all(colidx[p["a_pos"][p["a_colptr"][j]:p["a_colptr"][j + 1]]] == j)


@pytest.mark.parametrize("name", PATTERNS)
def test_every_dependency_lies_in_a_strictly_earlier_level(name):
    n, _, _, _, p = pattern(name)
    for rows, ptr, upper in ((p["ut_rows"], p["ut_lev_ptr"], True), (p["lt_rows"], p["lt_lev_ptr"], False)):
        assert np.array_equal(np.sort(rows), np.arange(n)) and ptr[0] == 0 and ptr[-1] == n and np.all(np.diff(ptr) > 0)
        level = np.empty(n, dtype=int)
        for l in range(len(ptr) - 1):
            level[rows[ptr[l]:ptr[l + 1]]] = l
        for j in range(n):
            d = p["t_colptr"][j] + p["t_diag"][j]
            deps = p["t_row"][p["t_colptr"][j]:d] if upper else p["t_row"][d + 1:p["t_colptr"][j + 1]]
            assert np.all(deps < j) if upper else np.all(deps > j)
            assert np.all(level[deps] < level[j]), (name, upper, j)
            assert level[j] == (level[deps].max() + 1 if deps.size else 0)         # ... and no later than it has to


@pytest.mark.parametrize("name", PATTERNS)
def test_interpreter_of_the_tables_solves_the_transposed_system(name):
    """Random complex values on the pattern -- the magnitudes the pivot order was chosen on, scaled by (0.5 .. 1) and turned by a random
    phase, so that the static order stays a sound one -- factor by the existing program, transposed solve by the new tables, one refinement.
    The own diagonal of a charge / limit unknown keeps its stamped constant 1: the program takes no division by such a pivot (LUProgram::unit)."""
    n, rowptr, colidx, mag, p = pattern(name)
    rng = np.random.default_rng(7)
    rows = np.repeat(np.arange(n), np.diff(rowptr))
    const = np.zeros(mag.size, dtype=bool)
    if name in R.CASES:
        const = (rows == colidx) & (hip.leaves_of(case(name)[0])[2][rows] != 0) & (mag == 1.0)
    for trial in range(3):
        vals = np.where(const, 1.0, mag * (0.5 + 0.5 * rng.random(mag.size)) * np.exp(2j * np.pi * rng.random(mag.size)))
        A = np.zeros((n, n), dtype=complex)
        A[np.repeat(np.arange(n), np.diff(rowptr)), colidx] = vals
        c = rng.standard_normal(n) + 1j * rng.standard_normal(n)
        x = N.tables_adjoint_solve(p, vals, c)
        xref = sla.solve(A.T, c)
        kappa = R.cond_inf_c(A.T)
        print("%s trial %d  n %d  err %.3g  kappa eps %.3g" % (name, trial, n, np.max(np.abs(x - xref)) / np.max(np.abs(xref)), kappa * EPS))
        assert np.max(np.abs(x - xref)) <= 16 * kappa * EPS * np.max(np.abs(xref))
        # the transposed residual over the column view
        r = N.tables_residual(p, vals, x, c)
        scale = np.abs(A.T) @ np.abs(x) + np.abs(c)
        assert np.all(np.abs(r - (c - A.T @ x)) <= 8 * (np.diff(p["a_colptr"]) + 1) * EPS * scale)


@pytest.mark.parametrize("name", list(R.CASES))
def test_static_order_adjoint_agrees_with_the_refined_dense_solve_on_the_port_systems(name):
    """noise_ref.static_order_adjoint_c against ac_ref.refined_solve_c(A^T, e_out) on every system of the case, and the condition the GPU
    test's forward check rests on: with the output node of noise_ref.OUTPUTS no system is exempt (backward error below gate / 16)."""
    st, G, C, om, _, p = case(name)
    c = N.e_out(name, st)
    for b in range(G.shape[0]):
        for w in om:
            A = R.system(st, G[b], C[b], w, GMIN)
            xr, xs = R.refined_solve_c(A.T, c), N.static_order_adjoint_c(A, c, p["rperm"], p["cperm"])
            assert R.backward_error_c(A.T, xr, c) <= 4 * EPS
            assert R.backward_error_c(A.T, xs, c) < api.NOISE_BERR_MAX / 16
            assert np.max(np.abs(xs - xr)) <= 16 * R.cond_inf_c(A.T) * EPS * np.max(np.abs(xr)), (b, w)


def test_static_order_adjoint_equals_the_interpreter_of_the_tables():
    """two routes to the same arithmetic: dense no-pivot LU used transposed, and the program + tables"""
    st, G, C, om, _, p = case("dff")
    c = N.e_out("dff", st)
    A = R.system(st, G[1], C[1], om[3], GMIN)
    vals = A[np.repeat(np.arange(st.n), np.diff(st.rowptr)), np.asarray(st.colidx)]
    xs, xt = N.static_order_adjoint_c(A, c, p["rperm"], p["cperm"]), N.tables_adjoint_solve(p, vals, c)
    assert np.max(np.abs(xs - xt)) <= 16 * R.cond_inf_c(A.T) * EPS * np.max(np.abs(xs))


def test_noise_berr_max_is_sixteen_times_the_dense_adjoint_solve_s_own_backward_error():
    """The measurement api.NOISE_BERR_MAX states: the largest componentwise backward error np.linalg.solve(A.T, e_out) -- the host path's
    solve -- leaves over the noise test systems (ac_ref.CASES on the CPU port, e_out at noise_ref.OUTPUTS), times 16, not below 64 eps."""
    worst = 0.0
    for name in R.CASES:
        st, G, C, om, _, _ = case(name)
        c = N.e_out(name, st)
        for b in range(G.shape[0]):
            for w in om:
                A = R.system(st, G[b], C[b], w, GMIN)
                worst = max(worst, R.backward_error_c(A.T, np.linalg.solve(A.T, c), c))
    print("largest backward error of the dense adjoint solve: %.3g" % worst)
    assert api.NOISE_BERR_MAX == max(16 * api.NOISE_BERR_MEASURED, 64 * EPS)
    assert api.NOISE_BERR_MEASURED / 2 <= worst <= api.NOISE_BERR_MEASURED, worst        # the constant is the measurement, rounded up


def test_transpose_tables_are_only_returned_when_asked_for():
    n, rowptr, colidx, mag, p = pattern("diagonal")
    plain = hip.host_lu_analyze(n, rowptr, colidx, mag, sample=True)
    assert not set(hip.LUT_ARRAYS) & set(plain) and set(hip.LUT_ARRAYS) <= set(p)
    for k in plain:
        if k != "n_blocks":
            assert np.array_equal(plain[k], p[k])
