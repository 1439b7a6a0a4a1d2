// driver.hip -- host drivers: DC operating point (PCNR Newton + fallbacks) and the transient
// loop (variable-step BDF1/BDF2 + Newton), standing in for the integrator that calls the hot
// path in the reference (Sundials IDA via SciML, /root/reference/src/sweeps.jl:588-665; DC:
// _dc_solve_with_fallbacks, /root/reference/src/mna/solve.jl:599-929).
//
// The loops run on the host and launch the hot-path kernels once per Newton iteration for
// the whole batch.  Each sweep instance walks its own step sequence (own t, h, order,
// Newton count); its convergence test, error test, step-size choice, history rotation,
// predictor and output interpolation are evaluated by one wave per instance in
// k_tran_update (per-op path) or inside the fused kernel (fused2.hip), so desynchronised instances never round-trip
// over PCIe.  The host reads one counter (instances still running) every few launches.
//
// Integration method (identical in oracle/cpu_port.cpp, which is what the 1e-9 parity bar is
// defined against -- SURVEY.md section 7 "hard parts"):
//   * BDF1 with constant predictor on the first step after a (re)start, no error test;
//     BDF1 + linear predictor on the second; variable-step BDF2 + quadratic predictor after.
//   * local error estimate from the predictor-corrector difference (Newton divided
//     difference):  order 1: h/(h+h1) (u-up);  order 2: (1+w)h/((1+2w)(h+h1+h2)) (u-up), w=h/h1.
//   * weighted RMS norms with w_i = 1/(atol_i + rtol*|u_i|); step factor 0.9*err^(-1/(k+1))
//     clipped to [0.2, 2]; Newton failure -> h/4; restart at order 1 on every breakpoint.
#include <hip/hip_runtime.h>
#include <chrono>
#include <string.h>
#include <vector>
#include "internal.hpp"
#include "dc_chain.hpp"

using namespace cadnip;

struct Driver {
  int n_save = 0, n_obs = 0, n_break = 0;
  double *t = nullptr, *h = nullptr, *hprev = nullptr, *hpp = nullptr;
  int *nhist = nullptr, *order = nullptr, *k = nullptr, *status = nullptr, *bp_idx = nullptr, *save_idx = nullptr, *dcstate = nullptr, *action = nullptr;
  long long* cnt = nullptr;   // [B][4]
  double *mn_a0f = nullptr, *mn_ss = nullptr, *mn_dnp = nullptr; int* mn_flags = nullptr;   // Newton mode 1 (tran_ctrl.hpp)
  double *u0 = nullptr, *u1 = nullptr, *u2 = nullptr, *up = nullptr, *beta = nullptr;
  double *u3 = nullptr, *hp3 = nullptr;   // max_order = 3 (allocated when first asked for)
  double *atol = nullptr, *emask = nullptr, *breaks = nullptr, *save_t = nullptr, *out = nullptr;
  int* obs = nullptr;
  int* nactive = nullptr;
  int* part = nullptr;        // [B] 1 = the instance takes part in the DC Newton run being started (k_dc_init)
  size_t out_cap = 0, brk_cap = 0, save_cap = 0, obs_cap = 0;
  std::vector<DCLogEntry> dc_log;   // what the DC fallback chain did, one entry per (instance, Newton run): cadnip_dc_log_*
  // The option arrays of cadnip_tran_run as the device holds them: host copies of what was last uploaded to breaks, save_t, obs, atol
  // and emask (`is` false: the device array holds something else).  A run with the same options as the last -- corner sweeps,
  // optimisation loops -- uploads nothing.  The writers of those five device arrays are dalloc's zero fill (through ensure_driver for
  // atol and emask, before anything is held; through drealloc for the others, which drops the copy) and sync_option; every kernel
  // takes them through TranArgs as pointers to const.
  template <class T> struct Held { std::vector<T> v; bool is = false; };
  Held<double> held_breaks, held_save_t, held_atol, held_emask;
  Held<int> held_obs;
  hipEvent_t ev[2] = {nullptr, nullptr};   // the fused transient's look-ahead (cadnip_tran_run); made on first use, released with the handle
  void* stage = nullptr; size_t stage_cap = 0;   // pinned host buffer the drivers' state and result transfers pass through (to_caller / from_caller)
};

namespace {
#define TRY(x) do { int _rc = (x); if (_rc) return _rc; } while (0)
template <class T> int dalloc(T** p, size_t c) { if (*p) return CADNIP_OK; HIP_TRY(hipMalloc((void**)p, (c ? c : 1) * sizeof(T))); HIP_TRY(hipMemset(*p, 0, (c ? c : 1) * sizeof(T))); return CADNIP_OK; }
// (`held`: the Driver::Held flag of the array -- a new allocation holds zeros, not the last upload)
template <class T> int drealloc(T** p, size_t* cap, size_t c, bool* held = nullptr) { if (*p && *cap >= c) return CADNIP_OK; if (held) *held = false; if (*p) (void)hipFree(*p); *p = nullptr; *cap = c; return dalloc(p, c); }
// Brings the device array `dev` to src[0..c): a blocking upload, unless the device holds exactly these bytes already.  *sent is set when
// something went up (the caller then synchronises once)
template <class T> int sync_option(T* dev, Driver::Held<T>& held, const T* src, size_t c, bool* sent) {
  if (held.is && held.v.size() == c && (c == 0 || memcmp(held.v.data(), src, c * sizeof(T)) == 0)) return CADNIP_OK;
  held.is = false;
  if (c) { HIP_TRY(hipMemcpy(dev, src, c * sizeof(T), hipMemcpyHostToDevice)); *sent = true; }
  held.v.assign(src, src + c);
  held.is = true;
  return CADNIP_OK;
}

// The drivers' transfers between device memory and memory of the caller's (or vectors of their own that live for one call) pass through
// one pinned buffer of the driver's, and a host copy.  Given a pageable array of this size the runtime's copy registers the array's
// pages with the device and keeps the registration for reuse; when the caller frees the array afterwards -- every sweep step frees the
// previous step's results -- unmapping registered pages makes the kernel driver evict and restore the process's queues, and the next call
// that waits for the device stands still for 20 - 30 ms (with results copied straight into fresh arrays,
// every second sweep step; how often depends on the caller's allocator).  Memory the driver owns is registered once and never unmapped
// while in use.  The price is the host copy, about 0.1 ms per MB into pages the caller has not touched yet.
int stage_fit(Driver* d, size_t bytes) {
  if (d->stage && d->stage_cap >= bytes) return CADNIP_OK;
  if (d->stage) (void)hipHostFree(d->stage);
  d->stage = nullptr; d->stage_cap = 0;
  HIP_TRY(hipHostMalloc(&d->stage, bytes ? bytes : 1, hipHostMallocDefault));
  d->stage_cap = bytes ? bytes : 1;
  return CADNIP_OK;
}
int to_caller(CadnipHandle* h, void* dst, const void* dev, size_t bytes) {
  TRY(stage_fit(h->drv, bytes));
  HIP_TRY(hipMemcpy(h->drv->stage, dev, bytes, hipMemcpyDeviceToHost));
  memcpy(dst, h->drv->stage, bytes);
  return CADNIP_OK;
}
int from_caller(CadnipHandle* h, void* dev, const void* src, size_t bytes) {
  TRY(stage_fit(h->drv, bytes));
  memcpy(h->drv->stage, src, bytes);
  HIP_TRY(hipMemcpy(dev, h->drv->stage, bytes, hipMemcpyHostToDevice));
  return CADNIP_OK;
}

// Every device buffer of the driver with the element count it is allocated with; ensure_driver allocates and cadnip_driver_free
// releases by walking this one list
template <class F> int each_buffer(Driver* d, size_t B, size_t n, F f) {
  const size_t later = 0;   // sized by the run that needs it (cadnip_tran_run: dalloc / drealloc)
  TRY(f(&d->t, B)); TRY(f(&d->h, B)); TRY(f(&d->hprev, B)); TRY(f(&d->hpp, B));
  TRY(f(&d->nhist, B)); TRY(f(&d->order, B)); TRY(f(&d->k, B)); TRY(f(&d->status, B));
  TRY(f(&d->bp_idx, B)); TRY(f(&d->save_idx, B)); TRY(f(&d->dcstate, B)); TRY(f(&d->action, B));
  TRY(f(&d->cnt, B * 4));
  TRY(f(&d->mn_a0f, B)); TRY(f(&d->mn_ss, B)); TRY(f(&d->mn_dnp, B)); TRY(f(&d->mn_flags, B));
  TRY(f(&d->u0, B * n)); TRY(f(&d->u1, B * n)); TRY(f(&d->u2, B * n)); TRY(f(&d->up, B * n)); TRY(f(&d->beta, B * n));
  TRY(f(&d->atol, n)); TRY(f(&d->emask, n)); TRY(f(&d->nactive, 2)); TRY(f(&d->part, B));
  TRY(f(&d->u3, later)); TRY(f(&d->hp3, later));
  TRY(f(&d->breaks, later)); TRY(f(&d->save_t, later)); TRY(f(&d->obs, later)); TRY(f(&d->out, later));
  return CADNIP_OK;
}

int ensure_driver(CadnipHandle* h) {
  if (!h->drv) h->drv = new Driver();
  return each_buffer(h->drv, h->B, h->n, [](auto** p, size_t c) { return c ? dalloc(p, c) : CADNIP_OK; });
}

}  // namespace
#include "tran_ctrl.hpp"
namespace {
__global__ void __launch_bounds__(64) k_tran_init(TranArgs a) {
  const int inst = blockIdx.x, tid = threadIdx.x, n = a.n;
  double* u = a.u + (size_t)inst * n;
  double* u0 = a.u0 + (size_t)inst * n;
  for (int i = tid; i < n; i += 64) { double v = u[i]; u0[i] = v; a.u1[(size_t)inst * n + i] = v; a.u2[(size_t)inst * n + i] = v; }
  int bp = 0;
  while (bp < a.n_break && a.breaks[bp] <= a.t0) ++bp;
  int si = 0;
  while (si < a.n_save && a.save_t[si] <= a.t0) {
    double* o = a.out + ((size_t)inst * a.n_save + si) * a.n_obs;
    for (int j = tid; j < a.n_obs; j += 64) o[j] = u[a.obs[j]];
    ++si;
  }
  __syncthreads();
  if (tid == 0) {
    a.flags[inst] = 0;
    for (int c = 0; c < 4; ++c) a.cnt[(size_t)inst * 4 + c] = 0;
  }
  __syncthreads();
  StepState s;
  s.t = a.t0; s.h = a.h0; s.hprev = a.h0; s.hpp = a.h0; s.hp3 = a.h0; s.tn = a.t0; s.a0 = 0.0;
  s.nhist = 1; s.ord = 1; s.k = 0; s.status = 0; s.bp = bp; s.si = si;
  s.c_newton = s.c_accept = s.c_reject = s.c_fail = 0;
  s.t_break = next_break(a, bp); s.t_save = next_save(a, si);
  s.a0f = 0.0; s.ss = 20.0; s.dnp = 0.0; s.dsc = 1.0; s.mflags = MN_NEED;
  GlobalVecs v(a, inst);
  prepare_step(a, v, s, tid, a.t0, a.h0, 1, a.h0, a.h0);
  store_state(a, inst, tid, s);
}

// NT threads per instance: one wave for the circuits of a sweep (n of a few hundred), a workgroup of four for a large one
template <int NT>
__global__ void __launch_bounds__(NT) k_tran_update(TranArgs a) {
  const int inst = blockIdx.x, tid = threadIdx.x;
  StepState s = load_state(a, inst);
  if (s.status != 0) return;
  const int bad = a.flags[inst] & 1;
  grp_sync<GlobalVecsT<NT>>();
  if (tid == 0) a.flags[inst] = 0;
  GlobalVecsT<NT> v(a, inst);
  if (a.newton_mode) {
    // per-op path: every round restamps and refactors (the factors live in LDS for the length of one k_lu_f2 launch), so the Jacobian is
    // always current -- a failed iteration halves the step at once, nothing is scaled.  The rate constant follows the same events as in
    // the fused kernel (reset to 20 where that one would refactor: first round, a0 outside IDA's window, 20 steps), so both paths accept
    // iterates by the same rule.  oracle/cpu_port.cpp mirrors this as newton_mode 2.
    const bool setup = !(s.mflags & MN_VALID) || (s.k == 0 && (s.a0 < 0.6 * s.a0f || s.a0 * 0.6 > s.a0f || (s.mflags >> MN_SINCE_SHIFT) >= 20));
    if (setup) { s.a0f = s.a0; s.ss = 20.0; s.mflags = MN_VALID | MN_JCUR; }
    else s.mflags |= MN_JCUR;
    s.dsc = 1.0;
  }
  tran_update_body(a, v, s, inst, tid, bad);
  store_state(a, inst, tid, s);
}

__global__ void k_count_running(const int* status, int B, int* nactive) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  int r = (i < B && status[i] == 0) ? 1 : 0;
  unsigned long long m = __ballot(r);
  if ((threadIdx.x & 63) == 0 && m) atomicAdd(nactive, __popcll(m));
}

// The running-instance count reaches the host through a store of this kernel into mapped pinned memory, not through an asynchronous
// device-to-host copy: under `rocprofv3 --pmc` (which serialises and re-queues the application's kernels) a copy queued behind the counting
// kernel was observed to run BEFORE it -- the host read 0, the Newton loop of cadnip_dc_run stopped at round 0 and every instance counted
// as failed.  Kernels of one stream stay ordered among themselves, and a finished kernel's stores to host memory are visible after the
// stream / event synchronisation.
__global__ void k_publish_int(const int* src, int* dst_host) {
  if (threadIdx.x == 0 && blockIdx.x == 0) { *dst_host = *src; __threadfence_system(); }
}

// ------------------------------------------------------------------------------------------
// DC: PCNR Newton state machine (solve.jl:599-698) / plain Newton (solve.jl:542-578)
// ------------------------------------------------------------------------------------------
struct DCArgs {
  double *u, *resid, *delta, *limit_w; const double* limit_init;
  int *active, *flags, *status, *dcstate, *action, *cold; long long* cnt;
  int B, n, n_limits, use_pcnr, maxiters; double abstol;
};

// `part` (may be null = everyone): an instance that sits this run out is parked -- status 2, inactive -- and none of the
// kernels of the run touches its state
__global__ void __launch_bounds__(64) k_dc_init(DCArgs a, int cold_start, const int* part) {
  const int inst = blockIdx.x, tid = threadIdx.x, n = a.n;
  if (part && !part[inst]) {
    if (tid == 0) { a.status[inst] = 2; a.dcstate[inst] = 0; a.action[inst] = 0; a.active[inst] = 0; }
    return;
  }
  double* u = a.u + (size_t)inst * n;
  int nz = 0;
  for (int i = tid; i < n; i += 64) if (u[i] != 0.0) nz = 1;
  nz = wave_any(nz);
  // cold start (iszero(u0)): seed the limit variables (solve.jl:620-625)
  if (cold_start && !nz && a.use_pcnr)
    for (int k = tid; k < a.n_limits; k += 64) u[n - a.n_limits + k] = a.limit_init[k];
  // initjct (armed by the host for the first stamping of the run) applies to the instances that start cold; a warm start --
  // a sweep point continued from its neighbour's solution -- is stamped at its start state (solve.jl:615-625)
  if (tid == 0) a.cold[inst] = (cold_start && !nz) ? 1 : 0;
  if (tid == 0) { a.status[inst] = 0; a.dcstate[inst] = 0; a.action[inst] = 0; a.active[inst] = 1; a.flags[inst] = 0; for (int c = 0; c < 4; ++c) a.cnt[(size_t)inst * 4 + c] = 0; }
}

__global__ void __launch_bounds__(64) k_dc_check(DCArgs a) {
  const int inst = blockIdx.x, tid = threadIdx.x, n = a.n;
  if (a.status[inst] != 0) return;
  const double* F = a.resid + (size_t)inst * n;
  double* u = a.u + (size_t)inst * n;
  double s = 0.0; int bad = 0;
  for (int i = tid; i < n; i += 64) { double f = F[i]; if (!isfinite(f)) bad = 1; s += f * f; }
  s = wave_sum(s); bad = wave_any(bad);
  const double nrm = sqrt(s);
  int st = a.dcstate[inst];
  long long it = a.cnt[(size_t)inst * 4 + 0];
  int action = 0, status = 0;
  // The PCNR loop tests convergence at the top of iterations 1..maxiters only (solve.jl:630-663): after its last solve it
  // returns unconverged without looking at the residual again.  The plain Newton stage gets the check after its last step.
  const bool pcnr = a.use_pcnr && a.n_limits > 0;
  if (bad) status = -1;
  else if (pcnr && st == 0 && it >= a.maxiters) status = -3;
  else if (nrm < a.abstol) {
    if (!a.use_pcnr || a.n_limits == 0) status = 1;
    else if (st == 0) {   // settle the limit slots, verify on the next rebuild (solve.jl:640-657)
      const double* lw = a.limit_w + (size_t)inst * n;
      for (int i = n - a.n_limits + tid; i < n; i += 64) u[i] = lw[i];
      st = 1; action = 1;
    } else status = 1;
  } else st = 0;
  if (status == 0 && action == 0 && it >= a.maxiters) status = -3;
  if (tid == 0) {
    a.dcstate[inst] = st; a.action[inst] = action; a.status[inst] = status;
    a.active[inst] = (status == 0 && action == 0) ? 1 : 0;   // mask for the LU + update kernels of this round
  }
}

__global__ void __launch_bounds__(64) k_dc_update(DCArgs a) {
  const int inst = blockIdx.x, tid = threadIdx.x, n = a.n;
  const int status = a.status[inst];
  if (status == 0 && a.action[inst] == 0) {
    double* u = a.u + (size_t)inst * n;
    const double* d = a.delta + (size_t)inst * n;
    int bad = (a.flags[inst] & 1);     // the refactorisation met a zero / non-finite pivot: leave u alone (the host may re-pivot)
    if (!bad)
      for (int i = tid; i < n; i += 64) { double dd = d[i]; if (!isfinite(dd)) bad = 1; u[i] -= dd; }
    bad = wave_any(bad);
    if (a.use_pcnr && a.n_limits > 0) {
      const double* lw = a.limit_w + (size_t)inst * n;
      for (int i = n - a.n_limits + tid; i < n; i += 64) u[i] = lw[i];
    }
    // a solve that failed (zero / non-finite pivot, non-finite step) is not an iteration: the reference's count is of the
    // updates applied (solve.jl:667-690; a SingularException leaves the loop before the counter moves)
    if (tid == 0) { if (bad) a.status[inst] = -2; else a.cnt[(size_t)inst * 4 + 0] += 1; }
  }
  __syncthreads();
  if (tid == 0) a.active[inst] = (a.status[inst] == 0) ? 1 : 0;   // next round's rebuild mask
}

// enqueues the count of the instances still running (status 0) and its publication in pinned slot `slot` (0 / 1)
int enqueue_running_count(CadnipHandle* h, int slot) {
  Driver* d = h->drv;
  TRY_RC(dev_zero_async(h, d->nactive + slot, sizeof(int)));
  hipLaunchKernelGGL(k_count_running, dim3((h->B + 255) / 256), dim3(256), 0, h->stream, d->status, h->B, d->nactive + slot);
  hipLaunchKernelGGL(k_publish_int, dim3(1), dim3(64), 0, h->stream, (const int*)(d->nactive + slot), h->d_pinned + slot);
  return CADNIP_OK;
}

int count_running(CadnipHandle* h, int* out) {
  TRY_RC(enqueue_running_count(h, 0));
  HIP_TRY(hipStreamSynchronize(h->stream));
  *out = ((volatile int*)h->h_pinned)[0];
  return CADNIP_OK;
}

DCArgs dc_args(CadnipHandle* h, double abstol, int maxiters, int use_pcnr) {
  Driver* d = h->drv;
  DCArgs a{};
  a.u = h->d_u; a.resid = h->d_resid; a.delta = h->d_delta; a.limit_w = h->d_limit_w; a.limit_init = h->d_limit_init;
  a.active = h->d_active; a.flags = h->d_flags; a.status = d->status; a.dcstate = d->dcstate; a.action = d->action; a.cold = h->d_cold; a.cnt = d->cnt;
  a.B = h->B; a.n = h->n; a.n_limits = h->n_limits; a.use_pcnr = (use_pcnr && h->n_limits > 0) ? 1 : 0; a.maxiters = maxiters; a.abstol = abstol;
  return a;
}

// The arguments of the transient kernels.  o = null: the DC mode of the fused kernel, which reads the state, its bookkeeping and the sizes only
TranArgs tran_args(CadnipHandle* h, const CadnipTranOpts* o = nullptr, int n_obs = 0, int n_err = 0) {
  Driver* d = h->drv;
  TranArgs a{};
  a.u = h->d_u; a.limit_w = h->d_limit_w; a.active = h->d_active; a.flags = h->d_flags; a.status = d->status; a.cnt = d->cnt;
  a.B = h->B; a.n = h->n; a.n_limits = h->n_limits;
  if (!o) return a;
  a.du = h->d_du; a.delta = h->d_delta; a.tcur = h->d_t; a.gamma = h->d_gamma;
  a.t = d->t; a.h = d->h; a.hprev = d->hprev; a.hpp = d->hpp; a.nhist = d->nhist; a.order = d->order; a.k = d->k; a.bp_idx = d->bp_idx; a.save_idx = d->save_idx;
  a.u0 = d->u0; a.u1 = d->u1; a.u2 = d->u2; a.up = d->up; a.beta = d->beta;
  a.atol = d->atol; a.emask = d->emask; a.breaks = d->breaks; a.save_t = d->save_t; a.obs = d->obs; a.out = d->out; a.nactive = d->nactive;
  a.n_break = o->n_break; a.n_save = o->n_save; a.n_obs = n_obs; a.n_err = n_err;
  const double span = o->t1 - o->t0;
  a.t0 = o->t0; a.t1 = o->t1; a.reltol = o->reltol;
  a.h0 = o->h0 > 0 ? o->h0 : span * 1e-6; a.hmin = o->hmin > 0 ? o->hmin : span * 1e-14; a.hmax = o->hmax > 0 ? o->hmax : span / 50.0;
  a.newton_tol = o->newton_tol > 0 ? o->newton_tol : 1e-3;
  a.max_newton = o->max_newton > 0 ? o->max_newton : 10; a.max_order = o->max_order > 0 ? (o->max_order > 3 ? 3 : o->max_order) : 2; a.use_pcnr = o->use_pcnr;
  a.newton_mode = o->newton_mode ? 1 : 0; a.mn_a0f = d->mn_a0f; a.mn_ss = d->mn_ss; a.mn_dnp = d->mn_dnp; a.mn_flags = d->mn_flags;
  a.step_rule = o->step_rule ? 1 : 0;
  if (a.max_order >= 3) { a.u3 = d->u3; a.hp3 = d->hp3; }   // variable-step BDF3: a fourth history vector and a third step size per instance
  return a;
}

// one DC Newton run on the whole batch with the handle's current spec; returns per-instance status in drv->status
int dc_newton(CadnipHandle* h, double abstol, int maxiters, int use_pcnr, int cold_start, int fused = 0, const int* d_part = nullptr) {
  Driver* d = h->drv;
  const DCArgs a = dc_args(h, abstol, maxiters, use_pcnr);
  hipLaunchKernelGGL(k_dc_init, dim3(h->B), dim3(64), 0, h->stream, a, cold_start, d_part);
  TRY_RC(dev_zero_async(h, h->d_gamma, (size_t)h->B * sizeof(double)));
  TRY_RC(dev_zero_async(h, h->d_du, (size_t)h->B * h->n * sizeof(double)));
  TRY_RC(dev_zero_async(h, h->d_t, (size_t)h->B * sizeof(double)));
  int saved_initjct = h->initjct;
  h->initjct = (cold_start && a.use_pcnr) ? 1 : 0;   // armed for the first stamping only (solve.jl:624,632)
  int rc = CADNIP_OK;
  if (fused && fused2_plan(h, F2_DC, 0).rc == CADNIP_OK) {
    // the whole Newton loop of every instance in the fused kernel; the host only looks at the running count
    const TranArgs ta = tran_args(h);
    int first = h->initjct;
    for (int launch = 0; launch < 4; ++launch) {
      rc = launch_fused2_dc(h, ta, 2 * maxiters + 4, abstol, maxiters, a.use_pcnr, h->spec.mode, first, d->dcstate); if (rc) break;
      first = 0;
      int running = 0;
      rc = count_running(h, &running); if (rc) break;
      if (running == 0) break;
    }
    h->initjct = saved_initjct;
    return rc;
  }
  int prev_running = h->B, repivots = 0;
  for (int round = 0; round < 2 * maxiters + 4; ++round) {
    rc = launch_rebuild(h); if (rc) break;
    h->initjct = 0;
    rc = launch_residual(h, h->d_du); if (rc) break;
    hipLaunchKernelGGL(k_dc_check, dim3(h->B), dim3(64), 0, h->stream, a);
    rc = launch_factor_solve(h, true, h->d_resid, h->d_delta); if (rc) break;
    hipLaunchKernelGGL(k_dc_update, dim3(h->B), dim3(64), 0, h->stream, a);
    int running = 0;
    rc = count_running(h, &running); if (rc) break;
    if (running < prev_running && repivots < 2) {
      // Some instance stopped.  If its refactorisation hit a zero pivot, the static pivot order does not fit this operating
      // point: choose a new one on the Jacobian at hand and let the instance repeat the iteration -- what KLU does when
      // klu_refactor fails and the caller falls back to klu_factor (solve.jl:667-670 keeps the symbolic object only as
      // long as refactoring works).  The new order serves every instance from here on.
      std::vector<int> stat((size_t)h->B);
      HIP_TRY(hipMemcpy(stat.data(), d->status, stat.size() * sizeof(int), hipMemcpyDeviceToHost));
      int victim = -1;
      for (int i = 0; i < h->B && victim < 0; ++i) if (stat[i] == -2) victim = i;
      if (victim >= 0) {
        ++repivots;
        std::vector<int> act((size_t)h->B);
        for (int i = 0; i < h->B; ++i) act[i] = (stat[i] == 0 || stat[i] == -2) ? 1 : 0;
        HIP_TRY(hipMemcpy(h->d_active, act.data(), act.size() * sizeof(int), hipMemcpyHostToDevice));
        rc = launch_jacobian(h); if (rc) break;                 // J = G + gamma C of this round (G, C are still the round's stamps)
        HIP_TRY(hipStreamSynchronize(h->stream));
        if (cadnip_analyze(h, victim) == CADNIP_OK) {
          for (int i = 0; i < h->B; ++i) if (stat[i] == -2) stat[i] = 0;
          HIP_TRY(hipMemcpy(d->status, stat.data(), stat.size() * sizeof(int), hipMemcpyHostToDevice));
          rc = count_running(h, &running); if (rc) break;
        } else {
          for (int i = 0; i < h->B; ++i) act[i] = stat[i] == 0 ? 1 : 0;
          HIP_TRY(hipMemcpy(h->d_active, act.data(), act.size() * sizeof(int), hipMemcpyHostToDevice));
        }
      }
    }
    prev_running = running;
    if (running == 0) break;
  }
  h->initjct = saved_initjct;
  return rc;
}

}  // namespace

extern "C" {

void cadnip_driver_free(CadnipHandle* h) {
  if (!h || !h->drv) return;
  Driver* d = h->drv;
  (void)each_buffer(d, 0, 0, [](auto** p, size_t) { if (*p) (void)hipFree(*p); return CADNIP_OK; });
  for (hipEvent_t e : d->ev) if (e) (void)hipEventDestroy(e);
  if (d->stage) (void)hipHostFree(d->stage);
  delete d;
  h->drv = nullptr;
}

int cadnip_tran_state(CadnipHandle* h, double* t_host, double* h_host, int32_t* order_host) {
  if (!h || !h->drv) return CADNIP_NOTREADY;
  Driver* d = h->drv;
  size_t B = h->B;
  if (t_host) HIP_TRY(hipMemcpy(t_host, d->t, B * sizeof(double), hipMemcpyDeviceToHost));
  if (h_host) HIP_TRY(hipMemcpy(h_host, d->h, B * sizeof(double), hipMemcpyDeviceToHost));
  if (order_host) HIP_TRY(hipMemcpy(order_host, d->order, B * sizeof(int), hipMemcpyDeviceToHost));
  return CADNIP_OK;
}

// DC operating point with the reference's fallback chain, per instance.  The chain itself -- who takes part in which stage, the gshunt
// ladder and the source ramp, the log -- is dc_chain.hpp; this is the device under it: every Newton run the chain asks for is one
// dc_newton on the batch, with the instances' start states, participation mask and homotopy terms (per-instance gshunt / srcFact,
// kernels.hip: k_assemble) uploaded before it and status, states and Newton counts downloaded after it.
int cadnip_dc_run(CadnipHandle* h, const CadnipDCOpts* o, double* u_host, int32_t* converged_host, CadnipRunStats* st) {
  if (!h || !o || !u_host) return CADNIP_BADARG;
  TRY(ensure_driver(h));
  Driver* d = h->drv;
  const size_t B = h->B, n = h->n;
  auto w0 = std::chrono::steady_clock::now();
  d->dc_log.clear();
  // CADNIP_DC_COLD_ZERO: the all-zero start state is made on the device, by the zero-fill kernel on the handle's stream (ordered with the
  // kernels queued behind it, kernels.hip: dev_zero_async) -- u_host is not read and B * n doubles of zeros do not cross the bus.
  // k_dc_init finds every row zero, as after an upload of zeros
  const bool zero_start = o->cold_start == CADNIP_DC_COLD_ZERO && !o->participate;
  // the symbolic phase needs one numeric Jacobian: stamp once at the start point
  if (!h->analyzed) {
    if (zero_start) TRY_RC(dev_zero_async(h, h->d_u, B * n * sizeof(double)));
    else TRY(from_caller(h, h->d_u, u_host, B * n * sizeof(double)));
    TRY(restore_masks(h, false));
    TRY_RC(dev_zero_async(h, h->d_gamma, B * sizeof(double)));
    TRY_RC(dev_zero_async(h, h->d_t, B * sizeof(double)));
    // pattern-complete sample: G + 1e9*C makes every structural entry of the unified pattern visible
    std::vector<double> g(B, 1e9);
    int ij = h->initjct;
    h->initjct = (o->cold_start && o->use_pcnr && h->n_limits > 0) ? 1 : 0;
    int rc = launch_rebuild(h);
    h->initjct = ij;
    if (rc) return rc;
    HIP_TRY(hipMemcpy(h->d_gamma, g.data(), B * sizeof(double), hipMemcpyHostToDevice));
    TRY(launch_jacobian(h));
    HIP_TRY(hipStreamSynchronize(h->stream));
    TRY(cadnip_analyze(h, 0));
  }
  // whatever happens below, the handle leaves with its own spec and no homotopy terms
  struct HomotopyGuard {
    CadnipHandle* h;
    ~HomotopyGuard() { (void)upload_homotopy(h, nullptr, nullptr); }
  } guard{h};
  std::vector<long long> cnt(B * 4);
  auto device_run = [&](const DCRun& r) -> int {
    // (blocking copies: the stream is idle here, and the start state must be in place before the first kernel is queued -- see k_publish_int)
    if (r.u) TRY(from_caller(h, h->d_u, r.u, B * n * sizeof(double)));
    else TRY_RC(dev_zero_async(h, h->d_u, B * n * sizeof(double)));   // (a zero start's first run)
    HIP_TRY(hipMemcpy(d->part, r.part, B * sizeof(int), hipMemcpyHostToDevice));
    TRY(upload_homotopy(h, r.gshunt, r.srcFact));
    TRY(dc_newton(h, o->abstol, o->maxiters, r.use_pcnr, r.cold_start, r.fused, d->part));
    TRY(to_caller(h, r.status, d->status, B * sizeof(int)));
    TRY(to_caller(h, r.dest(), h->d_u, B * n * sizeof(double)));   // (the caller's own array when the first run solved everybody)
    TRY(to_caller(h, cnt.data(), d->cnt, B * 4 * sizeof(long long)));
    for (size_t i = 0; i < B; ++i) r.iters[i] = cnt[i * 4];
    return CADNIP_OK;
  };
  const DCChainOpts chain{o->use_pcnr, o->cold_start, o->fused, o->use_stepping, h->n_limits > 0, h->spec.gshunt, h->spec.srcFact, o->participate};
  DCChainResult res;
  TRY(dc_chain(chain, h->B, h->n, u_host, converged_host, device_run, d->dc_log, res));
  // the device holds the final states (after a direct run it does already); every instance is left active for subsequent ABI calls
  // (and subject to a cadnip_set_initjct of the caller's)
  if (!res.direct) TRY(from_caller(h, h->d_u, u_host, B * n * sizeof(double)));
  TRY(restore_masks(h, true));
  if (st) {
    memset(st, 0, sizeof(*st));
    st->newton_iters = res.iters;
    st->n_failed = res.n_failed;
    st->wall_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - w0).count();
  }
  return res.n_failed ? CADNIP_NOCONV : CADNIP_OK;
}

// the log of the last cadnip_dc_run: entries in execution order, per (instance, Newton run)
int32_t cadnip_dc_log_size(CadnipHandle* h) { return (h && h->drv) ? (int32_t)h->drv->dc_log.size() : 0; }
int cadnip_dc_log_get(CadnipHandle* h, int32_t* inst, int32_t* stage, double* value, int32_t* ok, int64_t* iters) {
  if (!h || !h->drv) return CADNIP_NOTREADY;
  size_t k = 0;
  for (auto& e : h->drv->dc_log) {
    if (inst) inst[k] = e.inst; if (stage) stage[k] = e.stage; if (value) value[k] = e.value; if (ok) ok[k] = e.ok; if (iters) iters[k] = e.iters;
    ++k;
  }
  return CADNIP_OK;
}

int cadnip_tran_run(CadnipHandle* h, const CadnipTranOpts* o, double* out_host, int64_t* per_inst_host, CadnipRunStats* st) {
  if (!h || !o || !o->abstol || o->t1 <= o->t0 || o->n_save < 0 || o->n_break < 0) return CADNIP_BADARG;
  if (!h->analyzed) return CADNIP_NOTREADY;              // the symbolic LU phase (cadnip_analyze*) comes first
  for (int i = 1; i < o->n_break; ++i) if (!(o->breaks[i] > o->breaks[i - 1])) return CADNIP_BADARG;
  for (int i = 1; i < o->n_save; ++i) if (!(o->save_t[i] >= o->save_t[i - 1])) return CADNIP_BADARG;
  for (int i = 0; i < o->n_obs; ++i) if (o->obs[i] < 0 || o->obs[i] >= h->n) return CADNIP_BADARG;
  TRY(ensure_driver(h));
  Driver* d = h->drv;
  const size_t B = h->B, n = h->n;
  const int n_obs = o->n_obs > 0 ? o->n_obs : (int)n;
  TRY(drealloc(&d->breaks, &d->brk_cap, (size_t)o->n_break, &d->held_breaks.is));
  TRY(drealloc(&d->save_t, &d->save_cap, (size_t)o->n_save, &d->held_save_t.is));
  TRY(drealloc(&d->obs, &d->obs_cap, (size_t)n_obs, &d->held_obs.is));
  TRY(drealloc(&d->out, &d->out_cap, B * (size_t)o->n_save * n_obs));
  // the option arrays go up only where they differ from what the device holds (Driver::Held)
  bool sent = false;
  TRY(sync_option(d->breaks, d->held_breaks, o->breaks, (size_t)o->n_break, &sent));
  TRY(sync_option(d->save_t, d->held_save_t, o->save_t, (size_t)o->n_save, &sent));
  std::vector<int> obs(n_obs);
  for (int i = 0; i < n_obs; ++i) obs[i] = o->n_obs > 0 ? o->obs[i] : i;
  TRY(sync_option(d->obs, d->held_obs, (const int*)obs.data(), (size_t)n_obs, &sent));
  TRY(sync_option(d->atol, d->held_atol, o->abstol, n, &sent));
  std::vector<double> emask(n, 1.0);
  int n_err = (int)n;
  if (o->err_mask) { n_err = 0; for (size_t i = 0; i < n; ++i) { emask[i] = o->err_mask[i] != 0.0 ? 1.0 : 0.0; n_err += emask[i] != 0.0; } }
  TRY(sync_option(d->emask, d->held_emask, (const double*)emask.data(), n, &sent));
  if (sent) HIP_TRY(hipStreamSynchronize(h->stream));
  if (o->max_order >= 3) { TRY(dalloc(&d->u3, B * n)); TRY(dalloc(&d->hp3, B)); }
  TranArgs a = tran_args(h, o, n_obs, n_err);
  // Delayed stamps (cadnip_tran_set_delay, delay.hip): no step may reach past the smallest delay, so that the delayed value is a known number
  // for the whole step -- the same in every Newton round, the Jacobian G_tran + a0 C exact.  The rows of b that only k_delay_apply writes
  // are cleared on every exit path: the handle leaves with the b of its own stamps
  const bool delayed = h->dly.n_term > 0;
  if (delayed) { a.hmax = fmin(a.hmax, h->dly.tau_min); a.h0 = fmin(a.h0, a.hmax); }
  struct DelayGuard { CadnipHandle* h; bool on; ~DelayGuard() { if (on) { (void)launch_delay_clear(h); (void)hipStreamSynchronize(h->stream); } } } delay_guard{h, delayed};
  // the per-op kernels take over where the fused kernel cannot run: external generated models (they exist in the per-op stamping kernel only), a
  // circuit too large for the LDS-resident kernel, Newton mode 1 on a circuit outside the lean device set, a handle with delayed stamps or with
  // a sensitivity spec
  // Parameter sensitivities (cadnip_tran_set_sens, tran_sens.hip): the spec was sized for these save points, observers and history depth, and
  // s(t0) must have been given since the last run
  const bool sens = h->sns.n_group > 0;
  if (sens && (h->sns.n_save != o->n_save || h->sns.n_obs != n_obs || h->sns.nh != (a.max_order >= 3 ? 4 : 3))) return CADNIP_BADARG;
  if (sens && !h->sns.inited) return CADNIP_NOTREADY;
  const bool use_fused = !sens && o->fused && fused2_plan(h, F2_TRAN, o->newton_mode).circuit_ok;
  struct ModeGuard { CadnipHandle* h; int saved; ~ModeGuard() { h->spec.mode = saved; } } mode_guard{h, h->spec.mode};
  h->spec.mode = 1;   // :tran (restored on every exit path)
  hipLaunchKernelGGL(k_tran_init, dim3(h->B), dim3(64), 0, h->stream, a);
  if (delayed) TRY(launch_delay_init(h, a.t0));
  if (sens) { h->sns.inited = false; TRY(launch_sens_begin(h, a)); }
  HIP_TRY(hipStreamSynchronize(h->stream));
  auto w0 = std::chrono::steady_clock::now();
  int64_t launches = 0;
  const int64_t max_it = o->max_iterations > 0 ? o->max_iterations : 50000000;
  int rc = CADNIP_OK, running = h->B;
  // Newton rounds between two looks at the running-instance count.  A fused launch loads the structure tables and each
  // instance's state once and ends when its slowest wave has done its rounds (measured, DFF sweep: 8 rounds per launch
  // 38.8 M iterations/s, 64: 43.2, 1024: 44.8, one launch for the whole transient: 45.2).
  const int check_every = use_fused ? 1024 : 8;
  if (use_fused) {
    // The host stays one launch ahead: launch k+1 is queued before the running-instance count of launch k is read,
    // so the GPU never waits for the host between launches.  Once every instance has finished, the one launch
    // already in the queue finds nothing to do (each wave reads its status and exits).
    hipEvent_t* const ev = d->ev;
    for (int s = 0; s < 2; ++s) if (!ev[s]) HIP_TRY(hipEventCreateWithFlags(&ev[s], hipEventDisableTiming));
    int slot = 0;
    bool have_prev = false;
    while (launches < max_it) {
      rc = launch_fused2_rounds(h, a, check_every); if (rc) break;
      launches += check_every;
      rc = enqueue_running_count(h, slot); if (rc) break;
      if (hipEventRecord(ev[slot], h->stream) != hipSuccess) { rc = CADNIP_HIPERROR; break; }
      if (have_prev) {
        if (hipEventSynchronize(ev[1 - slot]) != hipSuccess) { rc = CADNIP_HIPERROR; break; }
        running = ((volatile int*)h->h_pinned)[1 - slot];
        if (running == 0) break;
      }
      have_prev = true;
      slot ^= 1;
    }
    hipError_t es = hipStreamSynchronize(h->stream);
    if (es != hipSuccess) { set_last_error("hipStreamSynchronize", es); return CADNIP_HIPERROR; }
    if (!rc && running > 0) rc = count_running(h, &running);
  }
  while (!use_fused && running > 0 && launches < max_it) {
    for (int c = 0; c < check_every; ++c) {
      rc = launch_rebuild(h); if (rc) break;
      if (delayed) { rc = launch_delay_apply(h, d->status); if (rc) break; }
      rc = launch_residual(h, h->d_du); if (rc) break;
      rc = launch_factor_solve(h, true, h->d_resid, h->d_delta); if (rc) break;
      if (sens) { rc = launch_sens_snapshot(h, a); if (rc) break; }
      { ProfScope ps(h, "tran_update");
        if (h->n >= 4096) hipLaunchKernelGGL(k_tran_update<256>, dim3(h->B), dim3(256), 0, h->stream, a);
        else hipLaunchKernelGGL(k_tran_update<64>, dim3(h->B), dim3(64), 0, h->stream, a); }
      if (delayed) { rc = launch_delay_record(h, d->t, d->u0, d->status); if (rc) break; }
      if (sens) { rc = launch_sens_stage(h, a); if (rc) break; }
      ++launches;
    }
    if (rc) break;
    rc = count_running(h, &running); if (rc) break;
  }
  HIP_TRY(hipStreamSynchronize(h->stream));
  double wall = std::chrono::duration<double>(std::chrono::steady_clock::now() - w0).count();
  if (rc) return rc;
  std::vector<long long> cnt(B * 4);
  std::vector<int> status(B);
  TRY(to_caller(h, cnt.data(), d->cnt, B * 4 * sizeof(long long)));
  TRY(to_caller(h, status.data(), d->status, B * sizeof(int)));
  if (out_host && o->n_save) TRY(to_caller(h, out_host, d->out, B * (size_t)o->n_save * n_obs * sizeof(double)));
  CadnipRunStats s; memset(&s, 0, sizeof(s));
  for (size_t i = 0; i < B; ++i) {
    s.newton_iters += cnt[i * 4 + 0]; s.steps_accepted += cnt[i * 4 + 1]; s.steps_rejected += cnt[i * 4 + 2]; s.newton_failures += cnt[i * 4 + 3];
    if (status[i] != 1) s.n_failed += 1;
    if (per_inst_host) { per_inst_host[i * 4 + 0] = cnt[i * 4 + 0]; per_inst_host[i * 4 + 1] = cnt[i * 4 + 1]; per_inst_host[i * 4 + 2] = cnt[i * 4 + 2]; per_inst_host[i * 4 + 3] = status[i]; }
  }
  s.launches = launches; s.wall_seconds = wall;
  if (st) *st = s;
  TRY(restore_masks(h, false));
  return s.n_failed ? CADNIP_NOCONV : CADNIP_OK;
}

}  // extern "C"
