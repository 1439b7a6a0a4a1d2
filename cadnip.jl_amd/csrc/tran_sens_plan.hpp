// tran_sens_plan.hpp -- forward (direct, staggered) parameter sensitivities of a transient (cadnip_tran_set_sens): the group layout, the BDF
// coefficients of an accepted step, the weights of a save point and the checks of a spec.  Plain inline C++ with no HIP in it: the kernels of
// tran_sens.hip include it, and tests/test_tran_sens_ref_cpu.py compiles it with the host compiler and drives it directly (as
// delay_plan.hpp and stamp_plan.hpp are built and tested).
//
// With F(u, u', p, t) = C u' + G u - b, the sensitivity s_k = du_n/dp_k of the DISCRETE trajectory on the steps the run took obeys
//   (G + a0 C) s_k,n = -dF/dp_k |(u_n, u'_n, t_n) - C sum_{j >= 1} a_j s_k,n-j
// with G, C at the accepted point and a_j the coefficients of the step just accepted.  dF/dp_k is the central difference of the residual
// at p_k +- delta_k, at the same (u_n, u'_n, t_n).  Where G + a0 C is not the Jacobian of F the solve leaves a defect, which one pass of
// tran_sens.hip takes out: F differenced again at (u_n +- delta_k s_k, u'_n +- delta_k s'_k, p_k +- delta_k), solved, subtracted.
//
// Group layout.  A point is a group of 2 + 2 K resident instances: the base (the only one that integrates), a twin with the base's
// parameters (its rows take the stamps at the accepted point: the base's own hold the next step's predictor), then p_k + delta_k and
// p_k - delta_k for k < K.  Everything but the base is parked for the whole run and its rows of the handle's arrays are scratch.
#pragma once
#include <cmath>
#include <cstddef>
#include <vector>

#if defined(__HIPCC__)
#define CADNIP_SNS_HD __host__ __device__
#else
#define CADNIP_SNS_HD
#endif

namespace cadnip {

#define CADNIP_SENS_MAX_BYTES ((size_t)256 << 20)   // history plus output: the cap of the delay ring

enum { SENS_BASE = 0, SENS_TWIN = 1 };
CADNIP_SNS_HD inline int sens_group_size(int K) { return 2 + 2 * K; }
CADNIP_SNS_HD inline int sens_plus(int k) { return 2 + 2 * k; }
CADNIP_SNS_HD inline int sens_minus(int k) { return 3 + 2 * k; }

// a0 .. a3 of the step of size h and the given order that follows steps hprev and hpp (u'_n = sum a_j u_{n-j}); the closed forms of
// tran_ctrl.hpp: prepare_step, coefficients beyond the order are zero.  order 0: all zero (the DC form of the stage)
CADNIP_SNS_HD inline void sens_bdf_alphas(int order, double h, double hprev, double hpp, double al[4]) {
  al[0] = al[1] = al[2] = al[3] = 0.0;
  if (order <= 0) return;
  if (order == 1) { al[0] = 1.0 / h; al[1] = -1.0 / h; return; }
  if (order == 2) {
    const double w = h / hprev;
    al[0] = (1.0 + 2.0 * w) / ((1.0 + w) * h);
    al[1] = -(1.0 + w) / h;
    al[2] = (w * w) / ((1.0 + w) * h);
    return;
  }
  const double d1 = h, d2 = h + hprev, d3 = d2 + hpp, s12 = hprev + hpp;
  al[0] = (1.0 / d1 + 1.0 / d2) + 1.0 / d3;
  al[1] = -(d2 * d3) / (d1 * (hprev * s12));
  al[2] = (d1 * d3) / (d2 * (hprev * hpp));
  al[3] = -(d1 * d2) / (d3 * (s12 * hpp));
}

// weights of (s_n, s_n-1, s_n-2) at the save time ts inside the step told -> tn, as tran_ctrl.hpp: save_outputs weighs the states: the
// quadratic through (tn, told, told - hprev) when two older points existed (nhist >= 2), the straight line otherwise (w[2] = 0)
CADNIP_SNS_HD inline void sens_out_weights(int nhist, double told, double tn, double hprev, double ts, double w[3]) {
  const double x = ts - told, xa = tn - told;
  if (nhist >= 2) {
    const double xc = -hprev;
    w[0] = ((x - 0.0) * (x - xc)) / ((xa - 0.0) * (xa - xc));
    w[1] = ((x - xa) * (x - xc)) / ((0.0 - xa) * (0.0 - xc));
    w[2] = ((x - xa) * (x - 0.0)) / ((xc - xa) * (xc - 0.0));
  } else {
    w[0] = x / xa; w[1] = 1.0 - w[0]; w[2] = 0.0;
  }
}

// bytes of the history [n_group][K][nh][n] plus the output [n_group][K][n_save][n_obs]; SIZE_MAX-safe: saturates at the cap + 1
inline size_t sens_bytes(size_t n_group, size_t K, size_t nh, size_t n, size_t n_save, size_t n_obs) {
  const long double b = 8.0L * (long double)n_group * (long double)K * ((long double)nh * (long double)n + (long double)n_save * (long double)n_obs);
  return b > (long double)CADNIP_SENS_MAX_BYTES ? CADNIP_SENS_MAX_BYTES + 1 : (size_t)b;
}

// The checks of cadnip_tran_set_sens on the group table members [n_group][2 + 2 K] and the steps delta [n_group][K].
enum SensSpecError { SENS_OK = 0, SENS_BAD_SHAPE = 1, SENS_BAD_INDEX = 2, SENS_TWICE = 3, SENS_BAD_DELTA = 4, SENS_TOO_LARGE = 5 };
inline int sens_spec_check(int B, int n, int n_group, int K, const int* members, const double* delta, int nh, int n_save, int n_obs) {
  if (n_group <= 0 || K <= 0 || !members || !delta || (nh != 3 && nh != 4) || n_save < 0 || n_obs <= 0 || n_obs > n) return SENS_BAD_SHAPE;
  const int per = sens_group_size(K);
  std::vector<char> seen((size_t)B, 0);
  for (size_t i = 0; i < (size_t)n_group * per; ++i) {
    const int m = members[i];
    if (m < 0 || m >= B) return SENS_BAD_INDEX;
    if (seen[m]) return SENS_TWICE;
    seen[m] = 1;
  }
  for (size_t i = 0; i < (size_t)n_group * K; ++i)
    if (!(delta[i] > 0.0) || !std::isfinite(delta[i])) return SENS_BAD_DELTA;
  if (sens_bytes(n_group, K, nh, n, n_save, n_obs) > CADNIP_SENS_MAX_BYTES) return SENS_TOO_LARGE;
  return SENS_OK;
}

}  // namespace cadnip
