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
