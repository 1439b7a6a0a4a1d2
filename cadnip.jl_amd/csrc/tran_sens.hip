// tran_sens.hip -- forward (direct, staggered) parameter sensitivities of the transient: cadnip_tran_set_sens and the stage that
// cadnip_tran_run (driver.hip) adds to a per-op round when a spec is set.  The formulation, the group layout, the BDF coefficients and
// the save weights are tran_sens_plan.hpp (host-tested); DESIGN.md section 9 has the reasons.
//
//   k_sens_snapshot -> k_tran_update -> k_sens_gather -> rebuild -> residual -> k_sens_rhs -> factor + solve
//                   -> k_sens_defect_point -> rebuild -> residual -> k_sens_defect_rhs -> factor + solve -> k_sens_record
//
// Only the bases integrate; the other members of a group are parked (status 1) and their rows of u, du, t, gamma, G, C, b, resid and delta
// are the stage's scratch.  The base's own rows are never written: after k_tran_update they hold the next step's predictor.
// k_sens_snapshot keeps what the update is about to overwrite.  k_sens_gather finds the groups whose base accepted (its counter moved),
// gives their parked members the accepted point (u_n, u'_n, t_n, gamma = a0) and makes d_active exactly those members, so the restamp and
// the residual touch nothing else.  k_sens_rhs forms the K right-hand sides of a group from the residuals of the +- members and the twin's
// C, copies the twin's G and C over each + member's and narrows d_active to the + members; the handle's LU kernels then solve all systems
// of all accepting groups in one launch.  That solve is exact only where G + a0 C is the Jacobian of F; a capacitance that depends on u but
// sits in C (a junction below the charge detection's threshold) leaves (dC/du) u' out of it.  So one defect-correction pass follows: the +-
// members are moved to (u_n +- delta s, u'_n +- delta s') as well, the difference of their residuals is then the TOTAL central difference
// along the trajectory -- dF/dp + (dF/du) s + (dF/du') s', zero for the exact s -- and s -= (G + a0 C)^-1 of it.  k_sens_record rotates
// the history, writes the save points the step crossed and gives d_active back to the controller.  No atomics on data, fixed summation order: the same bits on every run and for every batch around a group.
#include <hip/hip_runtime.h>
#include <math.h>
#include <vector>
#include "internal.hpp"
#include "tran_ctrl.hpp"

namespace cadnip {

struct SensArgs {
  // the spec and its state
  const int *members, *slot_of; const double* delta;
  double *hist, *out, *snap, *alpha; int *snap_i, *accept, *flag; long long* snap_cnt;
  // the handle's per-instance arrays
  double *u, *du, *tcur, *gamma, *G, *C, *rhs; const double* x; int *active, *flags; const int *rowptr, *colidx;
  // the controller's (null in the DC form)
  const double *t, *h, *hprev, *hpp, *u0, *u1, *u2, *u3, *save_t; const int *nhist, *order, *save_idx, *status, *obs; const long long* cnt;
  int B, n, nnz, n_group, K, per, nh, n_save, n_obs, dc;
};

__global__ void __launch_bounds__(64) k_sens_park(SensArgs a, int* status) {
  const int inst = blockIdx.x * 64 + threadIdx.x;
  if (inst >= a.B) return;
  const int slot = a.slot_of[inst];
  if (slot < 0 || slot % a.per == SENS_BASE) return;
  status[inst] = 1;            // "done": the controller, the running count and n_failed pass it by
  a.active[inst] = 0;
}

// s(t0) at the save points k_tran_init has already written (save_t <= t0): one block per (group, k)
__global__ void __launch_bounds__(64) k_sens_start(SensArgs a) {
  const int g = blockIdx.x / a.K, k = blockIdx.x - g * a.K;
  const int n_done = a.save_idx[a.members[(size_t)g * a.per + SENS_BASE]];
  const double* H0 = a.hist + ((size_t)blockIdx.x * a.nh) * a.n;
  for (int si = 0; si < n_done; ++si) {
    double* o = a.out + ((size_t)blockIdx.x * a.n_save + si) * a.n_obs;
    for (int j = threadIdx.x; j < a.n_obs; j += 64) o[j] = H0[a.obs[j]];
  }
}

__global__ void __launch_bounds__(64) k_sens_snapshot(SensArgs a) {
  const int g = blockIdx.x * 64 + threadIdx.x;
  if (g >= a.n_group) return;
  const int base = a.members[(size_t)g * a.per + SENS_BASE];
  double* sd = a.snap + (size_t)g * 4;
  sd[0] = a.t[base]; sd[1] = a.h[base]; sd[2] = a.hprev[base]; sd[3] = a.hpp[base];
  int* si = a.snap_i + (size_t)g * 3;
  si[0] = a.nhist[base]; si[1] = a.order[base]; si[2] = a.save_idx[base];
  a.snap_cnt[g] = a.cnt[(size_t)base * 4 + 1];
}

// one wave per resident instance: every instance decides its own d_active word
__global__ void __launch_bounds__(64) k_sens_gather(SensArgs a) {
  const int inst = blockIdx.x, tid = threadIdx.x, n = a.n;
  const int slot = a.slot_of[inst];
  const int g = slot < 0 ? 0 : slot / a.per, m = slot < 0 ? SENS_BASE : slot - g * a.per;
  const int base = a.members[(size_t)g * a.per + SENS_BASE];
  const bool accepted = slot >= 0 && (a.dc || a.cnt[(size_t)base * 4 + 1] != a.snap_cnt[g]);
  if (m == SENS_TWIN && tid == 0) a.accept[g] = accepted ? 1 : 0;
  if (m == SENS_BASE || !accepted) { if (tid == 0) a.active[inst] = 0; return; }
  double al[4] = {0.0, 0.0, 0.0, 0.0};
  if (!a.dc) sens_bdf_alphas(a.snap_i[(size_t)g * 3 + 1], a.snap[(size_t)g * 4 + 1], a.snap[(size_t)g * 4 + 2], a.snap[(size_t)g * 4 + 3], al);
  const size_t ob = (size_t)base * n, oi = (size_t)inst * n;
  if (a.dc) {
    for (int i = tid; i < n; i += 64) { a.u[oi + i] = a.u[ob + i]; a.du[oi + i] = 0.0; }
  } else {
    // after the accepted step the history is rotated: u0 = u_n, u1 = u_n-1, ...
    for (int i = tid; i < n; i += 64) {
      const double x0 = a.u0[ob + i];
      double d = al[0] * x0 + al[1] * a.u1[ob + i];
      if (al[2] != 0.0) d += al[2] * a.u2[ob + i];
      if (al[3] != 0.0) d += al[3] * a.u3[ob + i];
      a.u[oi + i] = x0; a.du[oi + i] = d;
    }
  }
  if (tid == 0) {
    a.tcur[inst] = a.dc ? a.tcur[base] : a.t[base];
    a.gamma[inst] = al[0];
    a.active[inst] = 1;
    if (m == SENS_TWIN) for (int j = 0; j < 4; ++j) a.alpha[(size_t)g * 4 + j] = al[j];
  }
}

// one wave per (group, k), lanes over rows: rhs_k = -(r(+k) - r(-k)) / (2 delta_k) - C_twin sum_{j >= 1} a_j s_k,n-j into the + member's
// row of the residual array; the twin's G and C over the + member's; d_active narrowed to the + members
__global__ void __launch_bounds__(64) k_sens_rhs(SensArgs a) {
  const int g = blockIdx.x / a.K, k = blockIdx.x - g * a.K, tid = threadIdx.x, n = a.n;
  if (!a.accept[g]) return;
  const int* mem = a.members + (size_t)g * a.per;
  const int twin = mem[SENS_TWIN], ip = mem[sens_plus(k)], im = mem[sens_minus(k)];
  const double* al = a.alpha + (size_t)g * 4;
  const double a1 = al[1], a2 = al[2], a3 = al[3];
  const double* H = a.hist + ((size_t)blockIdx.x * a.nh) * n;
  const double *Ct = a.C + (size_t)twin * a.nnz, *Gt = a.G + (size_t)twin * a.nnz;
  const double two_d = 2.0 * a.delta[blockIdx.x];
  double* rp = a.rhs + (size_t)ip * n;
  const double* rm = a.rhs + (size_t)im * n;
  for (int i = tid; i < n; i += 64) {
    double acc = 0.0;
    if (a1 != 0.0)
      for (int p = a.rowptr[i]; p < a.rowptr[i + 1]; ++p) {
        const int j = a.colidx[p];
        double hs = a1 * H[j];
        if (a2 != 0.0) hs += a2 * H[n + j];
        if (a3 != 0.0) hs += a3 * H[2 * (size_t)n + j];
        acc += Ct[p] * hs;
      }
    rp[i] = -((rp[i] - rm[i]) / two_d) - acc;
  }
  double *Gp = a.G + (size_t)ip * a.nnz, *Cp = a.C + (size_t)ip * a.nnz;
  for (int p = tid; p < a.nnz; p += 64) { Gp[p] = Gt[p]; Cp[p] = Ct[p]; }
  if (tid == 0) { a.active[im] = 0; if (k == 0) a.active[twin] = 0; }
}

// one wave per (group, k): the solve's flags, the history, the save points of the step; every thread of the grid also gives its share of
// d_active back to the controller (status: null in the DC form, whose caller restores the masks itself)
__global__ void __launch_bounds__(64) k_sens_record(SensArgs a) {
  const int g = blockIdx.x / a.K, k = blockIdx.x - g * a.K, tid = threadIdx.x, n = a.n;
  if (a.status)
    for (int inst = blockIdx.x * 64 + tid; inst < a.B; inst += gridDim.x * 64) a.active[inst] = a.status[inst] == 0 ? 1 : 0;
  if (!a.accept[g]) return;
  const int* mem = a.members + (size_t)g * a.per;
  const int base = mem[SENS_BASE], ip = mem[sens_plus(k)];
  const double* x = a.x + (size_t)ip * n;
  const double* x0 = a.dc ? nullptr : a.x + (size_t)mem[sens_minus(k)] * n;    // the first solve's s, kept by k_sens_defect_point: s = x0 - x
  double* H = a.hist + ((size_t)blockIdx.x * a.nh) * n;
  int bad = (a.flags[ip] & 3) ? 1 : 0;
  for (int i = tid; i < n; i += 64) if (!isfinite(x0 ? x0[i] - x[i] : x[i])) bad = 1;
  bad = __any(bad);
  if (tid == 0) { a.flags[ip] = 0; if (bad) atomicOr(a.flag + g, 1); }
  const double nan = __builtin_nan("");
  if (a.dc) {
    for (int i = tid; i < n; i += 64) { const double v = bad ? nan : x[i]; for (int j = 0; j < a.nh; ++j) H[(size_t)j * n + i] = v; }
    return;
  }
  // (a step that landed on a break restarts at order 1, whose a_2 = a_3 = 0 and whose save points take the straight line: the older slots
  // are not read until two more steps have refilled them, so the collapse of the history needs no copy)
  for (int i = tid; i < n; i += 64) {
    for (int j = a.nh - 1; j > 0; --j) H[(size_t)j * n + i] = H[(size_t)(j - 1) * n + i];
    H[i] = bad ? nan : x0[i] - x[i];
  }
  __syncthreads();
  const int si0 = a.snap_i[(size_t)g * 3 + 2], si1 = a.save_idx[base], nhist = a.snap_i[(size_t)g * 3];
  const double told = a.snap[(size_t)g * 4], hprev = a.snap[(size_t)g * 4 + 2], tn = a.t[base];
  for (int si = si0; si < si1; ++si) {
    double w[3];
    sens_out_weights(nhist, told, tn, hprev, a.save_t[si], w);
    double* o = a.out + ((size_t)blockIdx.x * a.n_save + si) * a.n_obs;
    for (int j = tid; j < a.n_obs; j += 64) {
      const int i = a.obs[j];
      double v = w[0] * H[i] + w[1] * H[n + i];
      if (nhist >= 2) v += w[2] * H[2 * (size_t)n + i];
      o[j] = v;
    }
  }
}

// The defect pass, one wave per (group, k).  The first solve's s moves from the + member's row of the solution array to the - member's (the
// second solve writes only the + member's), and the +- members get (u_n +- delta s, u'_n +- delta s') with s' = a0 s + sum_{j >= 1} a_j s_n-j;
// u_n and u'_n are read from the twin's rows, where k_sens_gather put them.  d_active: the +- members of the accepting groups
__global__ void __launch_bounds__(64) k_sens_defect_point(SensArgs a, double* x) {
  const int g = blockIdx.x / a.K, k = blockIdx.x - g * a.K, tid = threadIdx.x, n = a.n;
  if (!a.accept[g]) return;
  const int* mem = a.members + (size_t)g * a.per;
  const int twin = mem[SENS_TWIN], ip = mem[sens_plus(k)], im = mem[sens_minus(k)];
  const double* al = a.alpha + (size_t)g * 4;
  const double a0 = al[0], a1 = al[1], a2 = al[2], a3 = al[3], d = a.delta[blockIdx.x];
  const double* H = a.hist + ((size_t)blockIdx.x * a.nh) * n;
  const double *ut = a.u + (size_t)twin * n, *dut = a.du + (size_t)twin * n;
  for (int i = tid; i < n; i += 64) {
    const double s = x[(size_t)ip * n + i];
    double sd = a0 * s + a1 * H[i];
    if (a2 != 0.0) sd += a2 * H[n + i];
    if (a3 != 0.0) sd += a3 * H[2 * (size_t)n + i];
    x[(size_t)im * n + i] = s;
    a.u[(size_t)ip * n + i] = ut[i] + d * s;  a.du[(size_t)ip * n + i] = dut[i] + d * sd;
    a.u[(size_t)im * n + i] = ut[i] - d * s;  a.du[(size_t)im * n + i] = dut[i] - d * sd;
  }
  if (tid == 0) { a.active[ip] = 1; a.active[im] = 1; }
}

// ... its right-hand side (r(+k) - r(-k)) / (2 delta_k) into the + member's row; the twin's G and C over the + member's again (the restamp
// at the moved point has overwritten them); d_active narrowed to the + members
__global__ void __launch_bounds__(64) k_sens_defect_rhs(SensArgs a) {
  const int g = blockIdx.x / a.K, k = blockIdx.x - g * a.K, tid = threadIdx.x, n = a.n;
  if (!a.accept[g]) return;
  const int* mem = a.members + (size_t)g * a.per;
  const int twin = mem[SENS_TWIN], ip = mem[sens_plus(k)], im = mem[sens_minus(k)];
  const double two_d = 2.0 * a.delta[blockIdx.x];
  double* rp = a.rhs + (size_t)ip * n;
  const double* rm = a.rhs + (size_t)im * n;
  for (int i = tid; i < n; i += 64) rp[i] = (rp[i] - rm[i]) / two_d;
  const double *Ct = a.C + (size_t)twin * a.nnz, *Gt = a.G + (size_t)twin * a.nnz;
  double *Gp = a.G + (size_t)ip * a.nnz, *Cp = a.C + (size_t)ip * a.nnz;
  for (int p = tid; p < a.nnz; p += 64) { Gp[p] = Gt[p]; Cp[p] = Ct[p]; }
  if (tid == 0) a.active[im] = 0;
}

static SensArgs sens_args(CadnipHandle* h, const TranArgs* t) {
  const SensState& S = h->sns;
  SensArgs a{};
  a.members = S.d_members; a.slot_of = S.d_slot_of; a.delta = S.d_delta;
  a.hist = S.d_hist; a.out = S.d_out; a.snap = S.d_snap; a.alpha = S.d_alpha; a.snap_i = S.d_snap_i; a.accept = S.d_accept; a.flag = S.d_flag; a.snap_cnt = S.d_snap_cnt;
  a.u = h->d_u; a.du = h->d_du; a.tcur = h->d_t; a.gamma = h->d_gamma; a.G = h->d_G; a.C = h->d_C; a.rhs = h->d_resid; a.x = h->d_delta;
  a.active = h->d_active; a.flags = h->d_flags; a.rowptr = h->d_rowptr; a.colidx = h->d_colidx;
  a.B = h->B; a.n = h->n; a.nnz = h->nnz; a.n_group = S.n_group; a.K = S.K; a.per = sens_group_size(S.K); a.nh = S.nh; a.n_save = S.n_save; a.n_obs = S.n_obs;
  a.dc = t ? 0 : 1;
  if (t) {
    a.t = t->t; a.h = t->h; a.hprev = t->hprev; a.hpp = t->hpp; a.u0 = t->u0; a.u1 = t->u1; a.u2 = t->u2; a.u3 = t->u3; a.save_t = t->save_t;
    a.nhist = t->nhist; a.order = t->order; a.save_idx = t->save_idx; a.status = t->status; a.obs = t->obs; a.cnt = t->cnt;
  }
  return a;
}

void sens_release(CadnipHandle* h) {
  h->sns.each_buffer([](void** p) { if (*p) (void)hipFree(*p); *p = nullptr; });
  h->sns = SensState();
}

int launch_sens_begin(CadnipHandle* h, const TranArgs& t) {
  const SensArgs a = sens_args(h, &t);
  hipLaunchKernelGGL(k_sens_park, dim3((unsigned)((h->B + 63) / 64)), dim3(64), 0, h->stream, a, t.status);
  hipLaunchKernelGGL(k_sens_start, dim3((unsigned)(a.n_group * a.K)), dim3(64), 0, h->stream, a);
  HIP_TRY(hipGetLastError());
  return CADNIP_OK;
}

int launch_sens_snapshot(CadnipHandle* h, const TranArgs& t) {
  ProfScope ps(h, "sens_snapshot");
  const SensArgs a = sens_args(h, &t);
  hipLaunchKernelGGL(k_sens_snapshot, dim3((unsigned)((a.n_group + 63) / 64)), dim3(64), 0, h->stream, a);
  return CADNIP_OK;
}

// the stage proper; t: the run's controller arguments, null for the DC form of cadnip_tran_sens_init
static int sens_stage(CadnipHandle* h, const TranArgs* t) {
  const SensArgs a = sens_args(h, t);
  const unsigned gk = (unsigned)(a.n_group * a.K);
  { ProfScope ps(h, "sens_gather"); hipLaunchKernelGGL(k_sens_gather, dim3((unsigned)h->B), dim3(64), 0, h->stream, a); }
  TRY_RC(launch_rebuild(h));
  TRY_RC(launch_residual(h, h->d_du));
  { ProfScope ps(h, "sens_rhs"); hipLaunchKernelGGL(k_sens_rhs, dim3(gk), dim3(64), 0, h->stream, a); }
  TRY_RC(launch_factor_solve(h, true, h->d_resid, h->d_delta));
  if (t) {
    // (the DC form has no u' and its G is the Jacobian of G u - b: nothing to correct)
    { ProfScope ps(h, "sens_defect_point"); hipLaunchKernelGGL(k_sens_defect_point, dim3(gk), dim3(64), 0, h->stream, a, h->d_delta); }
    TRY_RC(launch_rebuild(h));
    TRY_RC(launch_residual(h, h->d_du));
    { ProfScope ps(h, "sens_defect_rhs"); hipLaunchKernelGGL(k_sens_defect_rhs, dim3(gk), dim3(64), 0, h->stream, a); }
    TRY_RC(launch_factor_solve(h, true, h->d_resid, h->d_delta));
  }
  { ProfScope ps(h, "sens_record"); hipLaunchKernelGGL(k_sens_record, dim3(gk), dim3(64), 0, h->stream, a); }
  return CADNIP_OK;
}

int launch_sens_stage(CadnipHandle* h, const TranArgs& t) { return sens_stage(h, &t); }

template <class T> static int sns_upload(T** p, const T* src, size_t count) {
  if (hipMalloc((void**)p, (count ? count : 1) * sizeof(T)) != hipSuccess) { *p = nullptr; return CADNIP_HIPERROR; }
  if (src && count && hipMemcpy(*p, src, count * sizeof(T), hipMemcpyHostToDevice) != hipSuccess) return CADNIP_HIPERROR;
  if (!src && hipMemset(*p, 0, (count ? count : 1) * sizeof(T)) != hipSuccess) return CADNIP_HIPERROR;
  return CADNIP_OK;
}

}  // namespace cadnip

using namespace cadnip;

// Everything is checked before anything is touched, and the new buffers are complete before the old ones go (as cadnip_tran_set_delay)
extern "C" int cadnip_tran_set_sens(CadnipHandle* h, const CadnipSensSpec* s) {
  if (!h) return CADNIP_BADARG;
  if (!s || s->n_group == 0) {
    HIP_TRY(hipStreamSynchronize(h->stream));
    sens_release(h);
    return CADNIP_OK;
  }
  if (h->dly.n_term > 0) return CADNIP_BADARG;
  if (sens_spec_check(h->B, h->n, s->n_group, s->K, s->members, s->delta, s->nh, s->n_save, s->n_obs) != SENS_OK) return CADNIP_BADARG;
  const size_t G = (size_t)s->n_group, K = (size_t)s->K, per = (size_t)sens_group_size(s->K), n = (size_t)h->n;
  std::vector<int> slot_of((size_t)h->B, -1);
  for (size_t i = 0; i < G * per; ++i) slot_of[s->members[i]] = (int)i;
  HIP_TRY(hipStreamSynchronize(h->stream));
  SensState S;
  S.n_group = s->n_group; S.K = s->K; S.nh = s->nh; S.n_save = s->n_save; S.n_obs = s->n_obs;
  int rc = sns_upload(&S.d_members, (const int*)s->members, G * per);
  if (!rc) rc = sns_upload(&S.d_slot_of, (const int*)slot_of.data(), slot_of.size());
  if (!rc) rc = sns_upload(&S.d_delta, s->delta, G * K);
  if (!rc) rc = sns_upload(&S.d_hist, (const double*)nullptr, G * K * (size_t)s->nh * n);
  if (!rc) rc = sns_upload(&S.d_out, (const double*)nullptr, G * K * (size_t)s->n_save * (size_t)s->n_obs);
  if (!rc) rc = sns_upload(&S.d_snap, (const double*)nullptr, G * 4);
  if (!rc) rc = sns_upload(&S.d_alpha, (const double*)nullptr, G * 4);
  if (!rc) rc = sns_upload(&S.d_snap_i, (const int*)nullptr, G * 3);
  if (!rc) rc = sns_upload(&S.d_accept, (const int*)nullptr, G);
  if (!rc) rc = sns_upload(&S.d_flag, (const int*)nullptr, G);
  if (!rc) rc = sns_upload(&S.d_snap_cnt, (const long long*)nullptr, G);
  if (rc) { S.each_buffer([](void** p) { if (*p) (void)hipFree(*p); }); return rc; }
  sens_release(h);
  h->sns = S;
  return CADNIP_OK;
}

extern "C" int cadnip_tran_sens_init(CadnipHandle* h, int32_t zero) {
  if (!h) return CADNIP_BADARG;
  SensState& S = h->sns;
  if (S.n_group <= 0) return CADNIP_NOTREADY;
  const size_t GK = (size_t)S.n_group * S.K;
  TRY_RC(dev_zero_async(h, S.d_flag, (size_t)S.n_group * sizeof(int)));
  if (zero) {
    TRY_RC(dev_zero_async(h, S.d_hist, GK * S.nh * h->n * sizeof(double)));
    HIP_TRY(hipStreamSynchronize(h->stream));
    S.inited = true;
    return CADNIP_OK;
  }
  if (!h->analyzed) return CADNIP_NOTREADY;
  int rc = sens_stage(h, nullptr);
  const hipError_t es = hipStreamSynchronize(h->stream);
  const int rm = restore_masks(h, false);      // every instance takes part again, whatever happened above
  if (rc) return rc;
  if (es != hipSuccess) { set_last_error("hipStreamSynchronize", es); return CADNIP_HIPERROR; }
  if (rm) return rm;
  S.inited = true;
  return CADNIP_OK;
}

extern "C" int cadnip_tran_sens_get(CadnipHandle* h, double* out_s, int32_t* flags) {
  if (!h) return CADNIP_BADARG;
  const SensState& S = h->sns;
  if (S.n_group <= 0) return CADNIP_NOTREADY;
  HIP_TRY(hipStreamSynchronize(h->stream));
  const size_t cnt = (size_t)S.n_group * S.K * S.n_save * S.n_obs;
  if (out_s && cnt) HIP_TRY(hipMemcpy(out_s, S.d_out, cnt * sizeof(double), hipMemcpyDeviceToHost));
  if (flags) HIP_TRY(hipMemcpy(flags, S.d_flag, (size_t)S.n_group * sizeof(int), hipMemcpyDeviceToHost));
  return CADNIP_OK;
}

extern "C" int cadnip_tran_sens_info(CadnipHandle* h, int32_t out[6]) {
  if (!h || !out) return CADNIP_BADARG;
  const SensState& S = h->sns;
  out[0] = S.n_group; out[1] = S.K; out[2] = S.n_group > 0 ? sens_group_size(S.K) : 0; out[3] = S.nh; out[4] = S.n_save; out[5] = S.n_obs;
  return CADNIP_OK;
}
