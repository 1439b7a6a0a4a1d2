// prim_probe.hip -- TEST INFRASTRUCTURE, not product: libcadnip_probe.so wraps the __device__ helpers every kernel is built from
// (tran_ctrl.hpp, devices.hpp, va_runtime.hpp, included unchanged) in trivial elementwise or one-wave kernels, so that
// tests/test_gpu_primitives.py can compare each of them with an exact or multiprecision reference.  Nothing here is linked into
// libcadnip_hip.so or declared in include/cadnip_hip.h.
//
// Every entry has one shape:
//   int probe_<name>(int n, int block, int nin, int nout, int niin, int niout,
//                    const double* in, double* out, const int* iin, int* iout, const double* tab, int ntab)
// in / out / iin / iout are [rows][n] (row-major: element i of row k at k * n + i), tab a table every element may read (wave tables,
// behavioural programs, node voltages).  n must be a multiple of block (64 or 256): a kernel has no tail guard, because the cross-lane
// helpers need every lane of a wave active.  The row counts are the caller's view of the entry; a mismatch is refused (-1) before anything
// is launched.  Returns the HIP error code (0 = success).
//
// One entry has a signature of its own -- the transient controller called ONCE on a state of the caller's choosing:
//   int probe_tran_ctrl(int policy, int op, int B, int n, int stride, const int* isc, const double* dsc,
//                       double* ds, int* is, long long* cnt, double* vec,
//                       const double* atol, const double* emask, const double* breaks, const double* save_t, const int* obs,
//                       double* out, int* nactive)
// policy 0 = GlobalVecsT<64>, 1 = GlobalVecsT<256>, 2 = the fixed form (GlobalVecsT<64> with KPF = 4, FIXED = true: n <= 256, and the
// switches of isc must be the ones it fixes).  One workgroup of V::NT threads per instance, B instances: load_state, then
// op 0 = prepare_step(a, v, s, tid, t, h, nhist, hprev, hpp) with the five arguments from ds / is, op 1 = tran_update_body(a, v, s, inst, tid,
// bad) with bad = flags & 1 (flags cleared, as k_tran_update does); then store_state.  The Newton-mode setup lines of k_tran_update are NOT
// run: mn_* are the caller's, and s.dsc is set from ds after load_state.  An instance whose status is not 0 is left alone.
//   isc[10]: n_limits n_break n_save n_obs n_err max_newton max_order use_pcnr newton_mode step_rule   dsc[7]: t0 t1 reltol h0 hmin hmax newton_tol
//   ds [B][15] in/out: t h hprev hpp tcur gamma mn_a0f mn_ss mn_dnp hp3 | in: dsc, prepare_step's t h hprev hpp
//   is [B][10] in/out: nhist order k status bp_idx save_idx flags mn_flags | out: active | in: prepare_step's nhist
//   cnt [B][4] in/out;  vec [10][B][stride] in/out: u du delta limit_w u0 u1 u2 u3 up beta, stride >= n + 64 (the words behind n are guards
//   the caller fills and checks);  atol, emask [n], breaks [n_break], save_t [n_save], obs [n_obs] shared by all instances;
//   out [B n_save n_obs + 64] and nactive [1] are filled with 0xFF bytes on the device before the launch and copied back whole.
// Arguments that would let the controller index outside these arrays (obs outside [0, n), negative bp / save indices, a non-finite time or
// step: an infinite tn satisfies every save-time test) are refused with -1 before anything is launched.
#include "../devices.hpp"
#include "../tran_ctrl.hpp"

using namespace cadnip;

namespace {

struct Rows { int nin, nout, niin, niout; };

template <class K>
int run(K kernel, Rows want, int n, int block, Rows got, const double* in, double* out, const int* iin, int* iout, const double* tab, int ntab) {
  if (got.nin != want.nin || got.nout != want.nout || got.niin != want.niin || got.niout != want.niout) return -1;
  if (n <= 0 || n > (1 << 20) || (block != 64 && block != 256) || n % block != 0 || ntab < 0) return -1;
  const size_t N = (size_t)n;
  double *d_in = nullptr, *d_out = nullptr, *d_tab = nullptr;
  int *d_iin = nullptr, *d_iout = nullptr;
  hipError_t e = hipSuccess;
  auto ck = [&](hipError_t r) { if (e == hipSuccess) e = r; return e == hipSuccess; };
  auto rows = [](int k) { return (size_t)(k > 0 ? k : 1); };
  ck(hipMalloc(&d_in, rows(want.nin) * N * sizeof(double))) && ck(hipMalloc(&d_out, rows(want.nout) * N * sizeof(double))) &&
      ck(hipMalloc(&d_iin, rows(want.niin) * N * sizeof(int))) && ck(hipMalloc(&d_iout, rows(want.niout) * N * sizeof(int))) &&
      ck(hipMalloc(&d_tab, rows(ntab) * sizeof(double)));
  if (e == hipSuccess) {
    if (want.nin) ck(hipMemcpy(d_in, in, want.nin * N * sizeof(double), hipMemcpyHostToDevice));
    if (want.niin) ck(hipMemcpy(d_iin, iin, want.niin * N * sizeof(int), hipMemcpyHostToDevice));
    if (ntab) ck(hipMemcpy(d_tab, tab, (size_t)ntab * sizeof(double), hipMemcpyHostToDevice));
    // results never written read back as NaN / -1
    ck(hipMemset(d_out, 0xFF, rows(want.nout) * N * sizeof(double)));
    ck(hipMemset(d_iout, 0xFF, rows(want.niout) * N * sizeof(int)));
  }
  if (e == hipSuccess) {
    hipLaunchKernelGGL(kernel, dim3(n / block), dim3(block), 0, 0, n, d_in, d_out, d_iin, d_iout, d_tab);
    ck(hipGetLastError());
    ck(hipDeviceSynchronize());
  }
  if (e == hipSuccess) {
    if (want.nout) ck(hipMemcpy(out, d_out, want.nout * N * sizeof(double), hipMemcpyDeviceToHost));
    if (want.niout) ck(hipMemcpy(iout, d_iout, want.niout * N * sizeof(int), hipMemcpyDeviceToHost));
  }
  (void)hipFree(d_in); (void)hipFree(d_out); (void)hipFree(d_iin); (void)hipFree(d_iout); (void)hipFree(d_tab);
  return (int)e;
}

template <int N> __device__ __forceinline__ Dual<N> ld_dual(const double* in, int n, int i, int k0) {
  Dual<N> r; r.v = in[(size_t)k0 * n + i];
#pragma unroll
  for (int j = 0; j < N; ++j) r.p[j] = in[(size_t)(k0 + 1 + j) * n + i];
  return r;
}
template <int N> __device__ __forceinline__ void st_dual(double* out, int n, int i, int k0, const Dual<N>& r) {
  out[(size_t)k0 * n + i] = r.v;
#pragma unroll
  for (int j = 0; j < N; ++j) out[(size_t)(k0 + 1 + j) * n + i] = r.p[j];
}

// the minimal context of source_value / bsrc_value: ipar and par are [rows][count], one "device" per element
struct ProbeCtx {
  const int* ipar; const double* par; const double* wave;
  int count, dev; double t; int mode;
};

}  // namespace

#define IN(k) in[(size_t)(k) * n + i]
#define OUT(k) out[(size_t)(k) * n + i]
#define II(k) iin[(size_t)(k) * n + i]
#define IO(k) iout[(size_t)(k) * n + i]
#define PROBE(name, NIN, NOUT, NIIN, NIOUT, ...)                                                                                         \
  __global__ void k_##name(int n, const double* in, double* out, const int* iin, int* iout, const double* tab) {                         \
    const int i = blockIdx.x * blockDim.x + threadIdx.x;                                                                                 \
    __VA_ARGS__                                                                                                                          \
  }                                                                                                                                      \
  extern "C" int probe_##name(int n, int block, int nin, int nout, int niin, int niout, const double* in, double* out, const int* iin,  \
                              int* iout, const double* tab, int ntab) {                                                                  \
    return run(k_##name, Rows{NIN, NOUT, NIIN, NIOUT}, n, block, Rows{nin, nout, niin, niout}, in, out, iin, iout, tab, ntab);           \
  }

// ---- tran_ctrl.hpp: scalars -------------------------------------------------------------------------------------------------------------
PROBE(fast_div, 2, 1, 0, 0, OUT(0) = fast_div(IN(0), IN(1));)
PROBE(step_root, 1, 1, 1, 0, OUT(0) = step_root(IN(0), II(0));)

// ---- cross-lane helpers -----------------------------------------------------------------------------------------------------------------
// rows 0..4: group_sum16 at width 1, 2, 4, 8, 16; 5: wave_sum; 6: uniform_f64; 7: dpp_pair_swap; 8, 9: va_group_sum<16>, <32>
PROBE(lane_sums, 1, 10, 0, 0,
      const double v = IN(0);
      OUT(0) = group_sum16(v, 1); OUT(1) = group_sum16(v, 2); OUT(2) = group_sum16(v, 4); OUT(3) = group_sum16(v, 8); OUT(4) = group_sum16(v, 16);
      OUT(5) = wave_sum(v); OUT(6) = uniform_f64(v); OUT(7) = dpp_pair_swap(v);
      OUT(8) = va_group_sum<16>(v); OUT(9) = va_group_sum<32>(v);)
// row l: readlane_f64(v, l)
PROBE(readlane, 1, 64, 0, 0,
      const double v = IN(0);
      _Pragma("unroll") for (int l = 0; l < 64; ++l) OUT(l) = readlane_f64(v, l);)
// rows 0..15: va_ddx_tl<16>(a, k); rows 16..47: va_ddx_tl<32>(a, k); row 48: the double overload (a constant: 0)
PROBE(ddx_tl, 1, 49, 0, 0,
      Dual<1> a; a.v = 0.0; a.p[0] = IN(0);
      _Pragma("unroll") for (int k = 0; k < 16; ++k) OUT(k) = va_ddx_tl<16>(a, k);
      _Pragma("unroll") for (int k = 0; k < 32; ++k) OUT(16 + k) = va_ddx_tl<32>(a, k);
      OUT(48) = va_ddx_tl<16>(IN(0), 3) + va_ddx_tl<32>(IN(0), 17);)

template <int NT> __device__ void grp_body(int n, int i, const double* in, double* out, const int* iin, int* iout) {
  typedef GlobalVecsT<NT> V;
  TranArgs a = {};      // never dereferenced: the reductions use V::NT only
  V v(a, 0);
  OUT(0) = grp_sum<V>(IN(0));
  __syncthreads();
  IO(0) = grp_any<V>(II(0));
  __syncthreads();
  double s1 = IN(0), s2 = IN(1); int bad = II(1);
  grp_reduce3<V>(v, s1, s2, bad);
  OUT(1) = s1; OUT(2) = s2; IO(1) = bad;
}
// one group = one workgroup of `block` threads: out 0 = grp_sum(in 0), iout 0 = grp_any(iin 0), (out 1, out 2, iout 1) = grp_reduce3(in 0, in 1, iin 1)
PROBE(grp, 2, 3, 2, 2,
      if (blockDim.x == 64) grp_body<64>(n, i, in, out, iin, iout); else grp_body<256>(n, i, in, out, iin, iout);)

// ---- Dual<N> and the va_* functions -----------------------------------------------------------------------------------------------------
// in: a (1 + N rows), b (1 + N rows); s = b.v is the plain double.  out, 1 + N rows each:
// a+b a-b a*b a/b a+s s+a a-s s-a a*s s*a a/s s/a -a
template <int N> __device__ void dual_ops_body(int n, int i, const double* in, double* out) {
  const Dual<N> a = ld_dual<N>(in, n, i, 0), b = ld_dual<N>(in, n, i, 1 + N);
  const double s = b.v;
  const int W = 1 + N;
  st_dual(out, n, i, 0 * W, a + b); st_dual(out, n, i, 1 * W, a - b); st_dual(out, n, i, 2 * W, a * b); st_dual(out, n, i, 3 * W, a / b);
  st_dual(out, n, i, 4 * W, a + s); st_dual(out, n, i, 5 * W, s + a); st_dual(out, n, i, 6 * W, a - s); st_dual(out, n, i, 7 * W, s - a);
  st_dual(out, n, i, 8 * W, a * s); st_dual(out, n, i, 9 * W, s * a); st_dual(out, n, i, 10 * W, a / s); st_dual(out, n, i, 11 * W, s / a);
  st_dual(out, n, i, 12 * W, -a);
}
PROBE(dual_ops1, 4, 26, 0, 0, dual_ops_body<1>(n, i, in, out);)
PROBE(dual_ops3, 8, 52, 0, 0, dual_ops_body<3>(n, i, in, out);)

// in: a (1 + N rows); iin 0: the function, iin 1: k of va_ddx.  out: the dual result (1 + N rows), then the double overload's value
template <int N> __device__ void va_unary_body(int n, int i, const double* in, double* out, const int* iin) {
  const Dual<N> a = ld_dual<N>(in, n, i, 0);
  const double x = a.v;
  Dual<N> r(0.0); double f = 0.0;
  switch (II(0)) {
    case 0: r = dsqrt(a); f = r.v; break;
    case 1: r = dexp(a); f = r.v; break;
    case 2: r = dlog(a); f = r.v; break;
    case 3: r = va_exp(a); f = va_exp(x); break;
    case 4: r = va_ln(a); f = va_ln(x); break;
    case 5: r = va_log(a); f = va_log(x); break;
    case 6: r = va_sqrt(a); f = va_sqrt(x); break;
    case 7: r = va_tanh(a); f = va_tanh(x); break;
    case 8: r = va_sinh(a); f = va_sinh(x); break;
    case 9: r = va_cosh(a); f = va_cosh(x); break;
    case 10: r = va_sin(a); f = va_sin(x); break;
    case 11: r = va_cos(a); f = va_cos(x); break;
    case 12: r = va_atan(a); f = va_atan(x); break;
    case 13: r = va_tan(a); f = va_tan(x); break;
    case 14: r = va_asin(a); f = va_asin(x); break;
    case 15: r = va_acos(a); f = va_acos(x); break;
    case 16: r = va_asinh(a); f = va_asinh(x); break;
    case 17: r = va_acosh(a); f = va_acosh(x); break;
    case 18: r = va_atanh(a); f = va_atanh(x); break;
    case 19: r = va_limexp(a); f = va_limexp(x); break;
    case 20: r = va_abs(a); f = va_abs(x); break;
    case 21: r = -a; f = -x; break;
    case 22: r = Dual<N>(va_floor(a)); f = va_floor(x); break;
    case 23: r = Dual<N>(va_ceil(a)); f = va_ceil(x); break;
    case 24: r = Dual<N>(va_int(a)); f = va_int(x); break;
    default: { const int k = II(1); r = Dual<N>(k >= 0 && k < N ? va_ddx(a, k) : 0.0); f = va_ddx(x, k); } break;
  }
  st_dual(out, n, i, 0, r);
  OUT(1 + N) = f;
}
PROBE(va_unary1, 2, 3, 2, 0, va_unary_body<1>(n, i, in, out, iin);)
PROBE(va_unary3, 4, 5, 2, 0, va_unary_body<3>(n, i, in, out, iin);)

// in: a, b (1 + N rows each); iin 0: function * 4 + overload (0 dual-dual, 1 dual-double, 2 double-dual, 3 double-double; the double
// operand is the dual's value); function 0 pow, 1 atan2, 2 hypot, 3 max, 4 min; iin 0 = 20: va_site(a, b.v, slot = iin 1).  out: 1 + N rows
template <int N> __device__ void va_binary_body(int n, int i, const double* in, double* out, const int* iin) {
  const Dual<N> a = ld_dual<N>(in, n, i, 0), b = ld_dual<N>(in, n, i, 1 + N);
  const double x = a.v, y = b.v;
  Dual<N> r(0.0);
  switch (II(0)) {
    case 0: r = va_pow(a, b); break;
    case 1: r = va_pow(a, y); break;
    case 2: r = va_pow(x, b); break;
    case 3: r = Dual<N>(va_pow(x, y)); break;
    case 4: r = va_atan2(a, b); break;
    case 5: r = va_atan2(a, y); break;
    case 6: r = va_atan2(x, b); break;
    case 7: r = Dual<N>(va_atan2(x, y)); break;
    case 8: r = va_hypot(a, b); break;
    case 9: r = va_hypot(a, y); break;
    case 10: r = va_hypot(x, b); break;
    case 11: r = Dual<N>(va_hypot(x, y)); break;
    case 12: r = va_max(a, b); break;
    case 13: r = va_max(a, y); break;
    case 14: r = va_max(x, b); break;
    case 15: r = Dual<N>(va_max(x, y)); break;
    case 16: r = va_min(a, b); break;
    case 17: r = va_min(a, y); break;
    case 18: r = va_min(x, b); break;
    case 19: r = Dual<N>(va_min(x, y)); break;
    default: { const int k = II(1); if (k >= 0 && k < N) r = va_site(a, y, k); } break;
  }
  st_dual(out, n, i, 0, r);
}
PROBE(va_binary1, 4, 2, 2, 0, va_binary_body<1>(n, i, in, out, iin);)
PROBE(va_binary3, 8, 4, 2, 0, va_binary_body<3>(n, i, in, out, iin);)

// ---- limiters ---------------------------------------------------------------------------------------------------------------------------
// in: vnew, vold, vt, vcrit (= vto for fetlim).  out: pnjlim, m1_pnjlim, m1_fetlim, m1_limvds
PROBE(limiters, 4, 4, 0, 0,
      OUT(0) = pnjlim(IN(0), IN(1), IN(2), IN(3)); OUT(1) = m1_pnjlim(IN(0), IN(1), IN(2), IN(3));
      OUT(2) = m1_fetlim(IN(0), IN(1), IN(3)); OUT(3) = m1_limvds(IN(0), IN(1));)

// ---- sp_mos1: the parts of the load section, with the exact fast quotients (FQ = true, what the stamps run) and with IEEE division ----------
// (tests/test_gpu_mos1_quotients.py: the two must agree to the bit).  The parameter block is the product's own ([M1_NPAR] rows, devices.hpp M1_*).
namespace {
struct M1ProbeCtx { const double* par; int count, dev, initjct; };

// in: vgs, vds, vbs (type-adjusted, as the stamps seed them), then the parameter block.  out: cbs, cbd (m1_junction, source / drain side), dvon,
// vdsat, cdrain (m1_channel), qbs, qbd (m1_qdep) -- value and three partials each, rows 0..27 -- then mode and gmin / mfactor
template <bool FQ> __device__ void m1_parts_body(int n, int i, const double* in, double* out) {
  const M1ProbeCtx d{in + (size_t)3 * n, n, i, 0};
  const double type = par_of(d, M1_TYPE), vt = par_of(d, M1_VT), tPhi = par_of(d, M1_TPHI), tVbi = par_of(d, M1_TVBI), gamma = par_of(d, M1_GAMMA);
  const double gmin_m = m1_quot<FQ>(par_of(d, M1_GMIN), par_of(d, M1_MFACTOR));
  const D3 a = D3::seed(IN(0), 0), b = D3::seed(IN(1), 1), c = D3::seed(IN(2), 2);
  const D3 dvbd = c - b, dvgd = a - b;
  st_dual(out, n, i, 0, m1_junction<FQ>(c, vt, gmin_m, par_of(d, M1_SSATCUR)));
  st_dual(out, n, i, 4, m1_junction<FQ>(dvbd, vt, gmin_m, par_of(d, M1_DSATCUR)));
  int mode;
  D3 dvon, vdsat, cdrain;
  m1_channel<FQ>(a, b, c, dvbd, dvgd, tPhi, tVbi, type, gamma, par_of(d, M1_LAMBDA), par_of(d, M1_BETA), mode, dvon, vdsat, cdrain);
  st_dual(out, n, i, 8, dvon); st_dual(out, n, i, 12, vdsat); st_dual(out, n, i, 16, cdrain);
  st_dual(out, n, i, 20, m1_qdep<FQ>(c, par_of(d, M1_CBS), par_of(d, M1_CBSSW), par_of(d, M1_TBULKPOT), par_of(d, M1_TDEPCAP), par_of(d, M1_MJ),
                                     par_of(d, M1_MJSW), par_of(d, M1_F2S), par_of(d, M1_F3S), par_of(d, M1_F4S)));
  st_dual(out, n, i, 24, m1_qdep<FQ>(dvbd, par_of(d, M1_CBD), par_of(d, M1_CBDSW), par_of(d, M1_TBULKPOT), par_of(d, M1_TDEPCAP), par_of(d, M1_MJ),
                                     par_of(d, M1_MJSW), par_of(d, M1_F2D), par_of(d, M1_F3D), par_of(d, M1_F4D)));
  OUT(28) = (double)mode; OUT(29) = gmin_m;
}
// in: V(g), V(b), V(d_int), V(s_int), the four limit unknowns (the previous round's limited vgs, vds, vbs, vbd), then the parameter block.
// iin: initjct.  out: the limited vgs, vds, vbs, vbd (m1_limit).  (m1_limit holds no fast quotient at present -- devices.hpp says why -- so the two
// instantiations are the same code today; the pair stays in the macro so that a site converted later is compared like the others.)
template <bool FQ> __device__ void m1_limit_body(int n, int i, const double* in, double* out, const int* iin) {
  const M1ProbeCtx d{in + (size_t)8 * n, n, i, II(0)};
  const double uo[4] = {IN(4), IN(5), IN(6), IN(7)};
  double w[4];
  m1_limit(d, uo, par_of(d, M1_TYPE), par_of(d, M1_VT), par_of(d, M1_TPHI), par_of(d, M1_TVBI), par_of(d, M1_GAMMA), IN(0), IN(1), IN(2), IN(3),
               0, 1, 2, 3, w[0], w[1], w[2], w[3]);
  OUT(0) = w[0]; OUT(1) = w[1]; OUT(2) = w[2]; OUT(3) = w[3];
}
}  // namespace
#define M1_PROBES(tag, FQ)                                                             \
  PROBE(m1_parts_##tag, 3 + M1_NPAR, 30, 0, 0, m1_parts_body<FQ>(n, i, in, out);)      \
  PROBE(m1_limit_##tag, 8 + M1_NPAR, 4, 1, 0, m1_limit_body<FQ>(n, i, in, out, iin);)
M1_PROBES(fq, true)
M1_PROBES(ieee, false)

// ---- source waves -----------------------------------------------------------------------------------------------------------------------
// in: t.  iin: offset of ts in tab, number of points (ys follow ts), hint (-1: no hint pointer).  out: value.  iout: the hint afterwards
PROBE(pwl, 1, 1, 3, 1,
      const double* ts = tab + II(0); const int len = II(1); int seg = II(2);
      OUT(0) = seg < 0 ? pwl_at_time(ts, ts + len, len, IN(0)) : pwl_at_time(ts, ts + len, len, IN(0), &seg);
      IO(0) = seg;)
PROBE(pulse, 8, 1, 0, 0, OUT(0) = pulse_at_time(IN(0), IN(1), IN(2), IN(3), IN(4), IN(5), IN(6), IN(7));)
PROBE(sind, 1, 1, 0, 0, OUT(0) = sind_deg(IN(0));)
// in: t, dc, scale.  iin: kind, offset, length (the ipar rows source_value reads), mode, hint (-1: none).  iout: the hint afterwards
PROBE(source_value, 3, 1, 5, 1,
      ProbeCtx d; d.ipar = iin; d.par = in; d.wave = tab; d.count = n; d.dev = i; d.t = IN(0); d.mode = II(3);
      int seg = II(4);
      OUT(0) = seg < 0 ? source_value(d, IN(1), IN(2)) : source_value(d, IN(1), IN(2), &seg);
      IO(0) = seg;)
// in: gain (par 0), t.  iin: offset and length of the program in tab (the ipar rows bsrc_value reads), offset of u in tab
PROBE(bsrc, 2, 1, 3, 0,
      ProbeCtx d; d.ipar = iin; d.par = in; d.wave = tab; d.count = n; d.dev = i; d.t = IN(1); d.mode = 1;
      OUT(0) = bsrc_value(d, tab + II(2));)

// ---- tran_ctrl.hpp: the controller, one call on a given state (signature in the header comment) ----------------------------------------------
namespace {
// the fixed form's compile-time switches over the per-op path's vectors: what V::FIXED changes in prepare_step / tran_update_body, nothing else
struct FixedGlobalVecs : GlobalVecsT<64> {
  static constexpr int KPF = 4;
  static constexpr bool FIXED = true;
  __device__ FixedGlobalVecs(const TranArgs& a, int inst) : GlobalVecsT<64>(a, inst) {}
};
enum { TC_NDS = 15, TC_NIS = 10, TC_NVEC = 10, TC_GUARD = 64 };
struct CtrlIO { double* ds; int* is; long long* cnt; double* vec; double* out; int B, stride, op; };

template <class V>
__global__ void __launch_bounds__(V::NT) k_tran_ctrl(TranArgs a, CtrlIO io) {
  const int inst = blockIdx.x, tid = threadIdx.x;
  // the instance's own view: every per-instance pointer moved to this instance, which the controller then addresses as instance 0
  double* d = io.ds + (size_t)inst * TC_NDS;
  int* q = io.is + (size_t)inst * TC_NIS;
  a.t = d; a.h = d + 1; a.hprev = d + 2; a.hpp = d + 3; a.tcur = d + 4; a.gamma = d + 5; a.mn_a0f = d + 6; a.mn_ss = d + 7; a.mn_dnp = d + 8; a.hp3 = d + 9;
  a.nhist = q; a.order = q + 1; a.k = q + 2; a.status = q + 3; a.bp_idx = q + 4; a.save_idx = q + 5; a.flags = q + 6; a.mn_flags = q + 7; a.active = q + 8;
  a.cnt = io.cnt + (size_t)inst * 4;
  auto vec = [&](int k) { return io.vec + ((size_t)k * io.B + inst) * io.stride; };
  a.u = vec(0); a.du = vec(1); a.delta = vec(2); a.limit_w = vec(3); a.u0 = vec(4); a.u1 = vec(5); a.u2 = vec(6); a.u3 = vec(7); a.up = vec(8); a.beta = vec(9);
  a.out = io.out + (size_t)inst * a.n_save * a.n_obs;
  StepState s = load_state(a, 0);
  s.dsc = d[10];
  const double pt = d[11], ph = d[12], phprev = d[13], phpp = d[14];
  const int pnhist = q[9], bad = q[6] & 1;
  __syncthreads();            // every thread has read the state before thread 0 writes any of it
  if (s.status != 0) return;
  V v(a, 0);
  if (io.op == 0) prepare_step(a, v, s, tid, pt, ph, pnhist, phprev, phpp);
  else {
    if (tid == 0) q[6] = 0;
    tran_update_body(a, v, s, 0, tid, bad);
  }
  store_state(a, 0, tid, s);
}
}  // namespace

extern "C" int probe_tran_ctrl(int policy, int op, int B, int n, int stride, const int* isc, const double* dsc, double* ds, int* is, long long* cnt,
                               double* vec, const double* atol, const double* emask, const double* breaks, const double* save_t, const int* obs,
                               double* out, int* nactive) {
  TranArgs a = {};
  a.B = B; a.n = n;
  a.n_limits = isc[0]; a.n_break = isc[1]; a.n_save = isc[2]; a.n_obs = isc[3]; a.n_err = isc[4];
  a.max_newton = isc[5]; a.max_order = isc[6]; a.use_pcnr = isc[7]; a.newton_mode = isc[8]; a.step_rule = isc[9];
  a.t0 = dsc[0]; a.t1 = dsc[1]; a.reltol = dsc[2]; a.h0 = dsc[3]; a.hmin = dsc[4]; a.hmax = dsc[5]; a.newton_tol = dsc[6];
  // refuse whatever could make the controller index outside the arrays
  if (policy < 0 || policy > 2 || op < 0 || op > 1 || B <= 0 || B > 4096 || n <= 0 || n > (1 << 16) || stride < n + TC_GUARD) return -1;
  if (a.n_limits < 0 || a.n_limits > n || a.n_break < 0 || a.n_save < 0 || a.n_obs < 0 || a.n_err < 0 || a.n_break > 4096 || a.n_save > 4096 || a.n_obs > 4096) return -1;
  if (policy == 2 && (n > 256 || a.newton_mode != 1 || a.step_rule != 0 || a.max_order > 2 || a.use_pcnr != 0)) return -1;
  if (a.newton_mode != 0 && a.newton_mode != 1) return -1;
  for (int j = 0; j < a.n_obs; ++j) if (obs[j] < 0 || obs[j] >= n) return -1;
  if (!isfinite(a.t1)) return -1;
  for (int b = 0; b < B; ++b) {
    const double* d = ds + (size_t)b * TC_NDS;
    const int* q = is + (size_t)b * TC_NIS;
    for (int k = 0; k < 5; ++k) if (!isfinite(d[k])) return -1;
    for (int k = 11; k < 15; ++k) if (!isfinite(d[k])) return -1;
    if (!(d[1] > 0.0) || !(d[2] > 0.0) || !(d[3] > 0.0) || !(d[12] > 0.0) || !(d[13] > 0.0) || !(d[14] > 0.0)) return -1;
    if (q[4] < 0 || q[5] < 0 || q[4] > a.n_break || q[5] > a.n_save) return -1;
  }
  const size_t nds = (size_t)B * TC_NDS, nis = (size_t)B * TC_NIS, ncnt = (size_t)B * 4, nvec = (size_t)TC_NVEC * B * stride;
  const size_t nout = (size_t)B * a.n_save * a.n_obs + TC_GUARD;
  auto atleast = [](int k) { return (size_t)(k > 0 ? k : 1); };
  double *d_ds = nullptr, *d_vec = nullptr, *d_out = nullptr, *d_atol = nullptr, *d_emask = nullptr, *d_breaks = nullptr, *d_save = nullptr;
  int *d_is = nullptr, *d_obs = nullptr, *d_nactive = nullptr;
  long long* d_cnt = nullptr;
  hipError_t e = hipSuccess;
  auto ck = [&](hipError_t r) { if (e == hipSuccess) e = r; return e == hipSuccess; };
  ck(hipMalloc(&d_ds, nds * sizeof(double))) && ck(hipMalloc(&d_is, nis * sizeof(int))) && ck(hipMalloc(&d_cnt, ncnt * sizeof(long long))) &&
      ck(hipMalloc(&d_vec, nvec * sizeof(double))) && ck(hipMalloc(&d_out, nout * sizeof(double))) && ck(hipMalloc(&d_atol, (size_t)n * sizeof(double))) &&
      ck(hipMalloc(&d_emask, (size_t)n * sizeof(double))) && ck(hipMalloc(&d_breaks, atleast(a.n_break) * sizeof(double))) &&
      ck(hipMalloc(&d_save, atleast(a.n_save) * sizeof(double))) && ck(hipMalloc(&d_obs, atleast(a.n_obs) * sizeof(int))) &&
      ck(hipMalloc(&d_nactive, sizeof(int)));
  if (e == hipSuccess) {
    ck(hipMemcpy(d_ds, ds, nds * sizeof(double), hipMemcpyHostToDevice));
    ck(hipMemcpy(d_is, is, nis * sizeof(int), hipMemcpyHostToDevice));
    ck(hipMemcpy(d_cnt, cnt, ncnt * sizeof(long long), hipMemcpyHostToDevice));
    ck(hipMemcpy(d_vec, vec, nvec * sizeof(double), hipMemcpyHostToDevice));
    ck(hipMemcpy(d_atol, atol, (size_t)n * sizeof(double), hipMemcpyHostToDevice));
    ck(hipMemcpy(d_emask, emask, (size_t)n * sizeof(double), hipMemcpyHostToDevice));
    if (a.n_break) ck(hipMemcpy(d_breaks, breaks, (size_t)a.n_break * sizeof(double), hipMemcpyHostToDevice));
    if (a.n_save) ck(hipMemcpy(d_save, save_t, (size_t)a.n_save * sizeof(double), hipMemcpyHostToDevice));
    if (a.n_obs) ck(hipMemcpy(d_obs, obs, (size_t)a.n_obs * sizeof(int), hipMemcpyHostToDevice));
    // results never written read back as NaN / -1
    ck(hipMemset(d_out, 0xFF, nout * sizeof(double)));
    ck(hipMemset(d_nactive, 0xFF, sizeof(int)));
  }
  if (e == hipSuccess) {
    a.atol = d_atol; a.emask = d_emask; a.breaks = d_breaks; a.save_t = d_save; a.obs = d_obs; a.nactive = d_nactive;
    const CtrlIO io{d_ds, d_is, d_cnt, d_vec, d_out, B, stride, op};
    if (policy == 0) hipLaunchKernelGGL(k_tran_ctrl<GlobalVecsT<64>>, dim3(B), dim3(64), 0, 0, a, io);
    else if (policy == 1) hipLaunchKernelGGL(k_tran_ctrl<GlobalVecsT<256>>, dim3(B), dim3(256), 0, 0, a, io);
    else hipLaunchKernelGGL(k_tran_ctrl<FixedGlobalVecs>, dim3(B), dim3(64), 0, 0, a, io);
    ck(hipGetLastError());
    ck(hipDeviceSynchronize());
  }
  if (e == hipSuccess) {
    ck(hipMemcpy(ds, d_ds, nds * sizeof(double), hipMemcpyDeviceToHost));
    ck(hipMemcpy(is, d_is, nis * sizeof(int), hipMemcpyDeviceToHost));
    ck(hipMemcpy(cnt, d_cnt, ncnt * sizeof(long long), hipMemcpyDeviceToHost));
    ck(hipMemcpy(vec, d_vec, nvec * sizeof(double), hipMemcpyDeviceToHost));
    ck(hipMemcpy(out, d_out, nout * sizeof(double), hipMemcpyDeviceToHost));
    ck(hipMemcpy(nactive, d_nactive, sizeof(int), hipMemcpyDeviceToHost));
  }
  (void)hipFree(d_ds); (void)hipFree(d_is); (void)hipFree(d_cnt); (void)hipFree(d_vec); (void)hipFree(d_out); (void)hipFree(d_atol); (void)hipFree(d_emask);
  (void)hipFree(d_breaks); (void)hipFree(d_save); (void)hipFree(d_obs); (void)hipFree(d_nactive);
  return (int)e;
}
