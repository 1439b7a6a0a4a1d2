// delay.hip -- transport delays in the transient: cadnip_tran_set_delay, the history ring and the two kernels that cadnip_tran_run
// (driver.hip) adds to a per-op Newton round when a spec is set.  The formulation, the ring's index arithmetic and the look-up are
// delay_plan.hpp (host-tested); DESIGN.md section 9 has the reasons.
//
//   rebuild -> k_delay_apply -> residual -> factor + solve -> k_tran_update -> k_delay_record
//
// k_delay_apply turns the round's stamps into G_tran = G - W, b_tran = b - sum w ud(col, tcur - tau) for exactly the instances the rebuild
// stamped (activity mask, running status): where the rebuild skipped an instance G still holds last round's G - W.  One thread per
// (instance, position) and per (instance, delayed row); a row sums its terms in table order -- no atomics, the same bits on every run.
// A look-up that fell off the ring ends its instance there: k_delay_apply itself writes the status and clears the activity mask, so the
// round's residual, factorisation and k_tran_update leave the instance alone -- no counter, time, history or save slot moves on a right-hand
// side with a term missing.  k_delay_record appends (t, u0[tap]) whenever the controller has accepted a step (its t has moved past the
// ring's newest time).  Both are a few loads per thread and latency-bound: an instance's
// ring times are contiguous (the binary search stays in one or two cache lines for the ring depths a run fills), the term tables of
// an instance are contiguous, and consecutive threads write consecutive positions / rows.
#include <hip/hip_runtime.h>
#include <string.h>
#include <vector>
#include "internal.hpp"
#include "delay_plan.hpp"

namespace cadnip {

#define DELAY_RING_MAX_BYTES ((size_t)256 << 20)

struct DelayArgs {
  const int *pos, *taps, *rows, *row_ptr, *term_tap; const unsigned char* row_store;
  const double *tau, *w, *W;
  double *hist_t, *hist_v, *v_init; int *head, *count;
  double *G, *b; const double *tcur, *u; int* active;
  int B, n, nnz, n_pos, n_term, n_taps, n_rows, depth; double t0;
};

__global__ void __launch_bounds__(64) k_delay_init(DelayArgs a) {
  const int id = blockIdx.x * 64 + threadIdx.x;
  if (id >= a.B * a.n_taps) return;
  const int inst = id / a.n_taps, tap = id - inst * a.n_taps;
  const double v = a.u[(size_t)inst * a.n + a.taps[tap]];
  a.v_init[id] = v;
  a.hist_v[(size_t)id * a.depth] = v;
  if (tap == 0) { a.hist_t[(size_t)inst * a.depth] = a.t0; a.head[inst] = a.depth > 1 ? 1 : 0; a.count[inst] = 1; }
}

__global__ void __launch_bounds__(256) k_delay_apply(DelayArgs a, int* status) {
  const int per = a.n_pos + a.n_rows;
  const long id = (long)blockIdx.x * 256 + threadIdx.x;
  if (id >= (long)a.B * per) return;
  const int inst = (int)(id / per), k = (int)(id - (long)inst * per);
  if (!a.active[inst] || status[inst] != 0) return;     // the rebuild of this round left the instance alone: so must this
  if (k < a.n_pos) {
    a.G[(size_t)inst * a.nnz + a.pos[k]] -= a.W[(size_t)inst * a.n_pos + k];
    return;
  }
  const int r = k - a.n_pos;
  const double tn = a.tcur[inst];
  const double* ht = a.hist_t + (size_t)inst * a.depth;
  const int head = a.head[inst], count = a.count[inst];
  const double *tau = a.tau + (size_t)inst * a.n_term, *w = a.w + (size_t)inst * a.n_term;
  double acc = 0.0;
  for (int j = a.row_ptr[r]; j < a.row_ptr[r + 1]; ++j) {
    const DelayLookup L = delay_lookup(ht, head, count, a.depth, a.t0, tn - tau[j]);
    if (L.kind == DELAY_OVERFLOW) {
      // the instance ends here, before the round is solved.  Other threads of this launch may or may not see the two stores: whatever they
      // still write to G and b of the instance is never read (every later kernel of the run skips it, the next rebuild rewrites both)
      status[inst] = CADNIP_TRAN_DELAY_OVERFLOW;
      a.active[inst] = 0;
      return;
    }
    const size_t tap = (size_t)inst * a.n_taps + a.term_tap[j];
    acc += w[j] * delay_value(L, a.hist_v + tap * a.depth, a.v_init[tap]);
  }
  double* brow = a.b + (size_t)inst * a.n + a.rows[r];
  *brow = (a.row_store[r] ? 0.0 : *brow) - acc;         // a row no device stamps is never rewritten by the rebuild: store, do not accumulate
}

__global__ void __launch_bounds__(64) k_delay_record(DelayArgs a, const double* t, const double* u0, int* status) {
  const int inst = blockIdx.x * 64 + threadIdx.x;
  if (inst >= a.B) return;
  const int st = status[inst];
  if (st != 0 && st != 1) return;                                                   // (an overflow among them: k_delay_apply ended the instance)
  int head = a.head[inst], count = a.count[inst];
  const double tacc = t[inst];
  double* ht = a.hist_t + (size_t)inst * a.depth;
  if (!(tacc > ht[delay_ring_slot(head, count, a.depth, count - 1)])) return;      // rejected step / Newton goes on: nothing new
  const int s = delay_ring_push(&head, &count, a.depth);
  ht[s] = tacc;
  for (int tap = 0; tap < a.n_taps; ++tap)
    a.hist_v[((size_t)inst * a.n_taps + tap) * a.depth + s] = u0[(size_t)inst * a.n + a.taps[tap]];
  a.head[inst] = head; a.count[inst] = count;
}

__global__ void __launch_bounds__(256) k_delay_clear(DelayArgs a) {
  const long id = (long)blockIdx.x * 256 + threadIdx.x;
  if (id >= (long)a.B * a.n_rows) return;
  const int inst = (int)(id / a.n_rows), r = (int)(id - (long)inst * a.n_rows);
  if (a.row_store[r]) a.b[(size_t)inst * a.n + a.rows[r]] = 0.0;
}

static DelayArgs delay_args(CadnipHandle* h) {
  const DelayState& D = h->dly;
  DelayArgs a{};
  a.pos = D.d_pos; a.taps = D.d_taps; a.rows = D.d_rows; a.row_ptr = D.d_row_ptr; a.term_tap = D.d_term_tap; a.row_store = D.d_row_store;
  a.tau = D.d_tau; a.w = D.d_w; a.W = D.d_W;
  a.hist_t = D.d_hist_t; a.hist_v = D.d_hist_v; a.v_init = D.d_v_init; a.head = D.d_head; a.count = D.d_count;
  a.G = h->d_G; a.b = h->d_b; a.tcur = h->d_t; a.u = h->d_u; a.active = h->d_active;
  a.B = h->B; a.n = h->n; a.nnz = h->nnz; a.n_pos = D.n_pos; a.n_term = D.n_term; a.n_taps = D.n_taps; a.n_rows = D.n_rows; a.depth = D.depth;
  a.t0 = D.t0;
  return a;
}

void delay_release(CadnipHandle* h) {
  h->dly.each_buffer([](void** p) { if (*p) (void)hipFree(*p); *p = nullptr; });
  h->dly = DelayState();
}

int launch_delay_init(CadnipHandle* h, double t0) {
  h->dly.t0 = t0;
  const DelayArgs a = delay_args(h);
  const int total = h->B * a.n_taps;
  hipLaunchKernelGGL(k_delay_init, dim3((unsigned)((total + 63) / 64)), dim3(64), 0, h->stream, a);
  HIP_TRY(hipGetLastError());
  return CADNIP_OK;
}

int launch_delay_apply(CadnipHandle* h, int* d_status) {
  ProfScope ps(h, "delay_apply");
  const DelayArgs a = delay_args(h);
  const long total = (long)h->B * (a.n_pos + a.n_rows);
  hipLaunchKernelGGL(k_delay_apply, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, h->stream, a, d_status);
  return CADNIP_OK;
}

int launch_delay_record(CadnipHandle* h, const double* d_t, const double* d_u0, int* d_status) {
  ProfScope ps(h, "delay_record");
  const DelayArgs a = delay_args(h);
  hipLaunchKernelGGL(k_delay_record, dim3((unsigned)((h->B + 63) / 64)), dim3(64), 0, h->stream, a, d_t, d_u0, d_status);
  return CADNIP_OK;
}

int launch_delay_clear(CadnipHandle* h) {
  const DelayArgs a = delay_args(h);
  const long total = (long)h->B * a.n_rows;
  hipLaunchKernelGGL(k_delay_clear, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, h->stream, a);
  HIP_TRY(hipGetLastError());
  return CADNIP_OK;
}

template <class T> static int dly_upload(T** p, const T* src, size_t count) {
  if (hipMalloc((void**)p, (count ? count : 1) * sizeof(T)) != hipSuccess) { *p = nullptr; return CADNIP_HIPERROR; }
  if (count && src && hipMemcpy(*p, src, count * sizeof(T), hipMemcpyHostToDevice) != hipSuccess) return CADNIP_HIPERROR;
  if (!src && hipMemset(*p, 0, (count ? count : 1) * sizeof(T)) != hipSuccess) return CADNIP_HIPERROR;
  return CADNIP_OK;
}

}  // namespace cadnip

using namespace cadnip;

// Everything is checked before anything is touched, and the new buffers are complete before the old ones go (as cadnip_ac_set_overlay)
extern "C" int cadnip_tran_set_delay(CadnipHandle* h, const CadnipDelaySpec* s) {
  if (!h) return CADNIP_BADARG;
  if (!s || s->n_term == 0) {
    HIP_TRY(hipStreamSynchronize(h->stream));
    delay_release(h);
    return CADNIP_OK;
  }
  if (h->sns.n_group > 0) return CADNIP_BADARG;     // a sensitivity spec stands (cadnip_tran_set_sens): the two settings exclude each other
  if (s->n_term < 0 || s->n_pos <= 0 || s->depth < 0 || s->depth == 1 || !s->tau || !s->w) return CADNIP_BADARG;
  DelayPlan P;
  if (!delay_plan_build(h->n, h->nnz, h->h_rowptr.data(), h->h_colidx.data(), s->n_pos, s->pos, s->n_term, s->term_pos, s->term_row, s->term_col, P))
    return CADNIP_BADARG;
  const size_t B = (size_t)h->B, nt = (size_t)s->n_term, np = P.pos.size(), ntap = P.taps.size(), nr = P.rows.size();
  const double tau_min = delay_tau_min(s->tau, B * nt);
  if (!(tau_min > 0.0)) return CADNIP_BADARG;
  const size_t depth = s->depth ? (size_t)s->depth : (size_t)CADNIP_DELAY_DEFAULT_DEPTH;
  if (depth > DELAY_RING_MAX_BYTES / 8 / (ntap + 1) / B) return CADNIP_BADARG;
  // per-instance tables in the plan's grouped order; W sums a position's terms in table order
  std::vector<double> tau(B * nt), w(B * nt), W(B * np, 0.0);
  for (size_t b = 0; b < B; ++b)
    for (size_t j = 0; j < nt; ++j) { tau[b * nt + j] = s->tau[b * nt + P.term[j]]; w[b * nt + j] = s->w[b * nt + P.term[j]]; }
  std::vector<int> plan_of((size_t)s->n_pos);
  for (size_t j = 0; j < nt; ++j) plan_of[s->term_pos[P.term[j]]] = P.term_pos[j];
  for (size_t b = 0; b < B; ++b)
    for (size_t t = 0; t < nt; ++t) W[b * np + plan_of[s->term_pos[t]]] += s->w[b * nt + t];
  std::vector<unsigned char> store(nr);
  for (size_t r = 0; r < nr; ++r) store[r] = h->h_b_ptr[P.rows[r] + 1] == h->h_b_ptr[P.rows[r]] ? 1 : 0;
  HIP_TRY(hipStreamSynchronize(h->stream));
  DelayState D;
  D.n_pos = (int)np; D.n_term = (int)nt; D.n_taps = (int)ntap; D.n_rows = (int)nr; D.depth = (int)depth; D.tau_min = tau_min;
  int rc = dly_upload(&D.d_pos, P.pos.data(), np);
  if (!rc) rc = dly_upload(&D.d_taps, P.taps.data(), ntap);
  if (!rc) rc = dly_upload(&D.d_rows, P.rows.data(), nr);
  if (!rc) rc = dly_upload(&D.d_row_ptr, P.row_ptr.data(), nr + 1);
  if (!rc) rc = dly_upload(&D.d_term_tap, P.term_tap.data(), nt);
  if (!rc) rc = dly_upload(&D.d_row_store, store.data(), nr);
  if (!rc) rc = dly_upload(&D.d_tau, tau.data(), B * nt);
  if (!rc) rc = dly_upload(&D.d_w, w.data(), B * nt);
  if (!rc) rc = dly_upload(&D.d_W, W.data(), B * np);
  if (!rc) rc = dly_upload(&D.d_hist_t, (const double*)nullptr, B * depth);
  if (!rc) rc = dly_upload(&D.d_hist_v, (const double*)nullptr, B * ntap * depth);
  if (!rc) rc = dly_upload(&D.d_v_init, (const double*)nullptr, B * ntap);
  if (!rc) rc = dly_upload(&D.d_head, (const int*)nullptr, B);
  if (!rc) rc = dly_upload(&D.d_count, (const int*)nullptr, B);
  if (rc) { D.each_buffer([](void** p) { if (*p) (void)hipFree(*p); }); return rc; }
  delay_release(h);
  h->dly = D;
  return CADNIP_OK;
}

extern "C" int cadnip_tran_delay_info(CadnipHandle* h, int32_t out[5]) {
  if (!h || !out) return CADNIP_BADARG;
  const DelayState& D = h->dly;
  out[0] = D.n_pos; out[1] = D.n_rows; out[2] = D.n_taps; out[3] = D.n_term; out[4] = D.depth;
  return CADNIP_OK;
}
