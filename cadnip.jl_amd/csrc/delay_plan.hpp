// delay_plan.hpp -- transport delays in the transient (cadnip_tran_set_delay): the history ring's index arithmetic and look-up, and the host
// plan of the two kernels of delay.hip.  Plain inline C++ with no HIP in it: the kernels include it, and tests/test_tran_delay_cpu.py
// compiles it with the host compiler and drives it directly (as stamp_plan.hpp, dc_chain.hpp and ac_hbm_plan.hpp are built and tested).
//
// A delayed stamp w at G[row, col] with delay tau means, in the time domain: w is NOT a coefficient of u[col](tn) -- it multiplies
// u[col](tn - tau), a known number, so the system of a Newton round at the trial time tn is
//   G_tran = G - W            W[pos] = sum of w over the terms at that CSR position
//   b_tran[row] = b[row] - sum over the row's terms of w * ud(col, tn - tau)
// ud(col, tq): tq <= t0 -> the value at the start of the run (the pre-history); otherwise linear interpolation between the two ACCEPTED
// points that bracket tq.  The driver clamps the step to the smallest tau, so tq never lies beyond the newest accepted point by more than
// rounding: a tq at or above the newest time takes the newest value.
//
// The ring of one instance: `depth` slots of times (hist_t[depth]) and, per tap (a distinct col), of values (hist_v[tap][depth]); `head` is
// the slot the next point goes to, `count` <= depth the points kept; the j-th oldest point sits in slot (head - count + j) mod depth.  A tq
// later than t0 but older than the oldest point kept is not extrapolated: the look-up reports DELAY_OVERFLOW and the instance stops with
// CADNIP_TRAN_DELAY_OVERFLOW.
#pragma once
#include <algorithm>
#include <cmath>
#include <vector>

#if defined(__HIPCC__)
#define CADNIP_DLY_HD __host__ __device__
#else
#define CADNIP_DLY_HD
#endif

namespace cadnip {

#define CADNIP_DELAY_DEFAULT_DEPTH 1024

enum DelayKind { DELAY_PRE = 0, DELAY_INTERP = 1, DELAY_NEWEST = 2, DELAY_OVERFLOW = 3 };

// slot of the j-th oldest point kept (0 <= j < count)
CADNIP_DLY_HD inline int delay_ring_slot(int head, int count, int depth, int j) {
  int s = head - count + j;
  return s < 0 ? s + depth : s;
}

// makes room for one more point: returns the slot to write and moves head / count (the oldest point goes when the ring is full)
CADNIP_DLY_HD inline int delay_ring_push(int* head, int* count, int depth) {
  const int s = *head;
  *head = s + 1 == depth ? 0 : s + 1;
  if (*count < depth) *count += 1;
  return s;
}

// where ud(., tq) comes from: kind, the two slots and the weight of the second -- value = v[s0] + w (v[s1] - v[s0])
struct DelayLookup { int kind, s0, s1; double w; };

CADNIP_DLY_HD inline DelayLookup delay_lookup(const double* hist_t, int head, int count, int depth, double t0, double tq) {
  DelayLookup L{DELAY_PRE, 0, 0, 0.0};
  if (tq <= t0 || count <= 0) return L;
  const int newest = delay_ring_slot(head, count, depth, count - 1);
  if (tq >= hist_t[newest]) { L.kind = DELAY_NEWEST; L.s0 = L.s1 = newest; return L; }
  if (tq < hist_t[delay_ring_slot(head, count, depth, 0)]) { L.kind = DELAY_OVERFLOW; return L; }
  // the largest j with t_j <= tq; t_0 <= tq < t_{count-1} holds here
  int lo = 0, hi = count - 1;
  while (hi - lo > 1) {
    const int mid = lo + (hi - lo) / 2;
    if (hist_t[delay_ring_slot(head, count, depth, mid)] <= tq) lo = mid; else hi = mid;
  }
  L.kind = DELAY_INTERP;
  L.s0 = delay_ring_slot(head, count, depth, lo);
  L.s1 = delay_ring_slot(head, count, depth, hi);
  const double tj = hist_t[L.s0];
  L.w = (tq - tj) / (hist_t[L.s1] - tj);
  return L;
}

// the delayed value of one tap (hist_v: the tap's `depth` values; v_init: its value at the start of the run); DELAY_OVERFLOW has none
CADNIP_DLY_HD inline double delay_value(const DelayLookup& L, const double* hist_v, double v_init) {
  if (L.kind == DELAY_PRE) return v_init;
  if (L.kind == DELAY_NEWEST) return hist_v[L.s0];
  const double vj = hist_v[L.s0];
  return vj + L.w * (hist_v[L.s1] - vj);
}

// ---- host: the plan of a spec --------------------------------------------------------------------------------------------------------------
// positions ascending, taps (distinct cols) ascending, terms grouped by row (rows ascending), inside a row in table order
struct DelayPlan {
  std::vector<int> pos;        // [n_pos] CSR positions, ascending
  std::vector<int> taps;       // [n_taps] unknowns whose history is kept, ascending
  std::vector<int> rows;       // [n_rows] rows of b that receive a delayed term, ascending
  std::vector<int> row_ptr;    // [n_rows + 1] ranges of the grouped term list
  std::vector<int> term;       // [n_term] grouped list: index into the spec's term table
  std::vector<int> term_tap;   // [n_term] grouped list: index into taps
  std::vector<int> term_pos;   // [n_term] grouped list: index into pos (the plan's order)
};

// false: an index out of range, a position named twice, or a term whose (row, col) is not the coordinate of its position
inline bool delay_plan_build(int n, int nnz, const int* rowptr, const int* colidx, int n_pos, const int* pos, int n_term, const int* term_pos,
                             const int* term_row, const int* term_col, DelayPlan& P) {
  P = DelayPlan();
  if (n_pos <= 0 || n_term <= 0 || !pos || !term_pos || !term_row || !term_col) return false;
  std::vector<int> order((size_t)n_pos);
  for (int o = 0; o < n_pos; ++o) { if (pos[o] < 0 || pos[o] >= nnz) return false; order[o] = o; }
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return pos[a] < pos[b]; });
  std::vector<int> plan_of((size_t)n_pos);
  for (int k = 0; k < n_pos; ++k) {
    if (k > 0 && pos[order[k]] == pos[order[k - 1]]) return false;
    P.pos.push_back(pos[order[k]]);
    plan_of[order[k]] = k;
  }
  for (int t = 0; t < n_term; ++t) {
    const int o = term_pos[t], r = term_row[t], c = term_col[t];
    if (o < 0 || o >= n_pos || r < 0 || r >= n || c < 0 || c >= n) return false;
    if (pos[o] < rowptr[r] || pos[o] >= rowptr[r + 1] || colidx[pos[o]] != c) return false;
    P.taps.push_back(c);
    P.rows.push_back(r);
  }
  std::sort(P.taps.begin(), P.taps.end()); P.taps.erase(std::unique(P.taps.begin(), P.taps.end()), P.taps.end());
  std::sort(P.rows.begin(), P.rows.end()); P.rows.erase(std::unique(P.rows.begin(), P.rows.end()), P.rows.end());
  P.row_ptr.assign(P.rows.size() + 1, 0);
  for (size_t r = 0; r < P.rows.size(); ++r) {
    for (int t = 0; t < n_term; ++t) {
      if (term_row[t] != P.rows[r]) continue;
      P.term.push_back(t);
      P.term_tap.push_back((int)(std::lower_bound(P.taps.begin(), P.taps.end(), term_col[t]) - P.taps.begin()));
      P.term_pos.push_back(plan_of[term_pos[t]]);
    }
    P.row_ptr[r + 1] = (int)P.term.size();
  }
  return true;
}

// smallest delay of a [B][n_term] table; <= 0 or non-finite anywhere: returns a value <= 0 (the caller's CADNIP_BADARG)
inline double delay_tau_min(const double* tau, size_t count) {
  double m = INFINITY;
  for (size_t i = 0; i < count; ++i) {
    if (!(tau[i] > 0.0) || !std::isfinite(tau[i])) return 0.0;
    m = std::min(m, tau[i]);
  }
  return count ? m : 0.0;
}

}  // namespace cadnip
