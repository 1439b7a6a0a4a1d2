// lu_transpose.hpp -- the tables of a TRANSPOSED solve through row-stored factors, as host-only combinatorics (the manner of
// stamp_plan.hpp): no HIP, no handle.  The adjoint family AcAdjSys (ac_lu.hip) solves A^T x = c with the factors AcLuSys computes.  With
// M = A[rperm][:, cperm] = L U (LUProgram: row-major L\U, sorted columns, lu_diag[i] = position of U(i,i)):
//   A^T x = c  <=>  M^T x_r = c_c:   y[j] = c[cperm[j]],   U^T z = y (forward),   L^T w = z (backward),   x[rperm[i]] = w[i]
// -- rperm and cperm swap roles against the plain solve.  Row j of U^T is column j of U, so both substitutions need the factors by column:
//   * the column view: column j lists its LU positions t_pos and rows t_row in ascending row order; t_diag[j] is the index of the diagonal
//     inside the list.  Entries before it are U(i,j), i < j, entries behind it L(i,j), i > j,
//   * two level schedules in gather form (as fwd_rows / bwd_rows of the plain solves): unknown j of U^T z = y needs every z[i], i < j, with
//     U(i,j) != 0 and is divided by the pivot; unknown j of L^T w = z needs every w[i], i > j, with L(i,j) != 0 (unit diagonal).  Every
//     unknown appears once in either list, sorted by level; a level reads only earlier levels,
//   * the column view of the CSR pattern of A for the transposed residual r = c - A^T x: column j lists the rows a_row and the CSR
//     positions a_pos of its entries.
// tests/test_lu_transpose_cpu.py interprets the tables in numpy against a dense transposed solve.
#pragma once
#include <algorithm>
#include <vector>

namespace cadnip {

struct LUTranspose {
  std::vector<int> t_colptr, t_pos, t_row, t_diag;   // [n + 1], [nnz_lu], [nnz_lu], [n]
  std::vector<int> ut_rows, ut_lev_ptr;              // U^T forward: unknowns by level, level -> range
  std::vector<int> lt_rows, lt_lev_ptr;              // L^T backward
  std::vector<int> a_colptr, a_row, a_pos;           // [n + 1], [nnz], [nnz]
};

// P: anything with n, lu_rowptr, lu_col, lu_diag as LUProgram (internal.hpp) has them; rowptr / colidx: the CSR pattern of A
template <class Program>
void lu_transpose_build(const Program& P, const std::vector<int>& rowptr, const std::vector<int>& colidx, LUTranspose& T) {
  const int n = P.n, nnz_lu = P.lu_rowptr[n], nnz = rowptr[n];
  T = LUTranspose();
  // column view of L\U: a counting sort by column; rows are visited in ascending order, so every column's list is ascending
  T.t_colptr.assign(n + 1, 0);
  for (int p = 0; p < nnz_lu; ++p) ++T.t_colptr[P.lu_col[p] + 1];
  for (int j = 0; j < n; ++j) T.t_colptr[j + 1] += T.t_colptr[j];
  T.t_pos.resize(nnz_lu); T.t_row.resize(nnz_lu); T.t_diag.assign(n, -1);
  {
    std::vector<int> at(T.t_colptr.begin(), T.t_colptr.end() - 1);
    for (int i = 0; i < n; ++i)
      for (int p = P.lu_rowptr[i]; p < P.lu_rowptr[i + 1]; ++p) {
        const int j = P.lu_col[p], q = at[j]++;
        T.t_pos[q] = p; T.t_row[q] = i;
        if (p == P.lu_diag[i]) T.t_diag[j] = q - T.t_colptr[j];
      }
  }
  // levels: U^T forward in ascending j, L^T backward in descending j
  auto schedule = [n](const std::vector<int>& level, std::vector<int>& rows, std::vector<int>& lev_ptr) {
    const int n_lev = n ? *std::max_element(level.begin(), level.end()) + 1 : 0;
    lev_ptr.assign(n_lev + 1, 0);
    for (int j = 0; j < n; ++j) ++lev_ptr[level[j] + 1];
    for (int l = 0; l < n_lev; ++l) lev_ptr[l + 1] += lev_ptr[l];
    std::vector<int> at(lev_ptr.begin(), lev_ptr.end() - 1);
    rows.resize(n);
    for (int j = 0; j < n; ++j) rows[at[level[j]]++] = j;
  };
  std::vector<int> level(n, 0);
  for (int j = 0; j < n; ++j) {
    int l = 0;
    for (int q = T.t_colptr[j]; q < T.t_colptr[j] + T.t_diag[j]; ++q) l = std::max(l, level[T.t_row[q]] + 1);
    level[j] = l;
  }
  schedule(level, T.ut_rows, T.ut_lev_ptr);
  for (int j = n - 1; j >= 0; --j) {
    int l = 0;
    for (int q = T.t_colptr[j] + T.t_diag[j] + 1; q < T.t_colptr[j + 1]; ++q) l = std::max(l, level[T.t_row[q]] + 1);
    level[j] = l;
  }
  schedule(level, T.lt_rows, T.lt_lev_ptr);
  // column view of the CSR pattern
  T.a_colptr.assign(n + 1, 0);
  for (int p = 0; p < nnz; ++p) ++T.a_colptr[colidx[p] + 1];
  for (int j = 0; j < n; ++j) T.a_colptr[j + 1] += T.a_colptr[j];
  T.a_row.resize(nnz); T.a_pos.resize(nnz);
  std::vector<int> at(T.a_colptr.begin(), T.a_colptr.end() - 1);
  for (int i = 0; i < n; ++i)
    for (int p = rowptr[i]; p < rowptr[i + 1]; ++p) { const int q = at[colidx[p]]++; T.a_row[q] = i; T.a_pos[q] = p; }
}

}  // namespace cadnip
