// src_cache.hpp -- the sweep kernel's per-instance SOURCE SEGMENT CACHE (k_fused2, transient mode, direct-residual variants).
//
// The value of an independent source is a function of time only, and between two points of a PWL wave it is one straight line.  The kernel
// used to re-read that line from global memory at every new time point (devices.hpp: source_value -- the block descriptor, ipar, then the
// dependent read of the PWL points: two L2 latencies on the round's critical path).  The cache keeps, for every lane of the pinned source
// block (the first min(count, 64) sources), the segment the lane's source is on, in LDS behind `beta` (lds_layout.hpp: lds_sweep):
//     t_lo, t_hi : the open interval of times the entry answers for       y_lo, y_hi : the values at its ends       scale
// It is filled when a wave picks an instance up (src_seg_fill), answers a new time point t when t_lo < t < t_hi (src_seg_hit /
// src_seg_value: LDS reads only, the expression of pwl_at_time with the same `/` and operand order, times scale), and is refilled after a
// miss -- which runs source_value unchanged -- from the segment the search found (src_seg_refill).  It lives for one residence of the
// instance on a wave and is never stored to HBM.
//   * a DC source (kind 0) answers every time: t_lo = -inf, t_hi = +inf, y_lo = y_hi = dc, scale = 1.0 (1.0 * dc is dc to the bit);
//   * a PWL source caches interior segments (2 <= i <= len, as pwl_at_time numbers them) and the two constant end regions (t < ts[0],
//     t > ts[len-1]) as half-infinite segments; a segment of zero width (a vertical jump: ts[i-1] == ts[i-2]) is never cached;
//   * pulse and sine sources are never cached: their entry cannot hit (t_lo = +inf).
// Plain C++ behind the __host__ __device__ markers, no HIP include and no handle type (tests/test_src_cache_cpu.py compiles it with the host
// compiler).  Layout of the region, structure of arrays: field k of lane l at word k * count + l (count = src_cache_lanes), so that the lanes
// of a wave read consecutive words.
#pragma once
#include "lds_layout.hpp"

namespace cadnip {

#define SRC_CACHE_FIELDS 5
#define SRC_CACHE_LANES 64   // the pinned source block: one source per lane

struct SrcSeg { double t_lo, t_hi, y_lo, y_hi, scale; };

LDS_HD int src_cache_lanes(int src_count) { return src_count < SRC_CACHE_LANES ? (src_count > 0 ? src_count : 0) : SRC_CACHE_LANES; }
// doubles of one instance's region (the trailing argument of lds_sweep): five per cached lane, rounded up to an even number
LDS_HD int src_cache_words(int src_count) { return (SRC_CACHE_FIELDS * src_cache_lanes(src_count) + 1) & ~1; }

LDS_HD SrcSeg src_seg_never() { SrcSeg e; e.t_lo = __builtin_inf(); e.t_hi = __builtin_inf(); e.y_lo = 0.0; e.y_hi = 0.0; e.scale = 1.0; return e; }
LDS_HD SrcSeg src_seg_make(double t_lo, double t_hi, double y_lo, double y_hi, double scale) {
  SrcSeg e; e.t_lo = t_lo; e.t_hi = t_hi; e.y_lo = y_lo; e.y_hi = y_hi; e.scale = scale; return e;
}
// the entry an instance starts its residence with: `kind` as in ipar row 0 (0 dc, 1 pwl, 2 pulse, 3 sine), `dc` the source's parameter 0
LDS_HD SrcSeg src_seg_fill(int kind, double dc) {
  return kind == 0 ? src_seg_make(-__builtin_inf(), __builtin_inf(), dc, dc, 1.0) : src_seg_never();
}
LDS_HD bool src_seg_hit(const SrcSeg& e, double t) { return e.t_lo < t && t < e.t_hi; }
// value at a time the entry answers for: pwl_at_time's expression, then source_value's scale
LDS_HD double src_seg_value(const SrcSeg& e, double t) {
#ifdef __clang__
#pragma clang fp contract(off)    // as pwl_at_time: one rounding per operation (the host test builds this header with -ffp-contract=off)
#endif
  double v;
  if (e.y_lo == e.y_hi) v = e.y_hi;
  else v = e.y_lo + (t - e.t_lo) * ((e.y_hi - e.y_lo) / (e.t_hi - e.t_lo));
  return e.scale * v;
}
// after a miss: the segment `i` that pwl_at_time's search left in its hint (1-based; i <= 1: before the first point, i > len: at or behind
// the last one); ts, ys: the wave's `len` points
LDS_HD SrcSeg src_seg_refill(int kind, const double* ts, const double* ys, int len, int i, double scale) {
  if (kind != 1 || len < 1) return src_seg_never();
  if (i <= 1) return src_seg_make(-__builtin_inf(), ts[0], ys[0], ys[0], scale);
  if (i > len) return src_seg_make(ts[len - 1], __builtin_inf(), ys[len - 1], ys[len - 1], scale);
  const double t_lo = ts[i - 2], t_hi = ts[i - 1];
  if (!(t_lo < t_hi)) return src_seg_never();            // a vertical jump (or a wave that is not sorted): never cached
  return src_seg_make(t_lo, t_hi, ys[i - 2], ys[i - 1], scale);
}

// region access; P: double* (kernel: LDS) or anything indexable
template <class P> LDS_HD SrcSeg src_seg_load(P base, int count, int lane) {
  return src_seg_make(base[lane], base[count + lane], base[2 * count + lane], base[3 * count + lane], base[4 * count + lane]);
}
template <class P> LDS_HD void src_seg_store(P base, int count, int lane, const SrcSeg& e) {
  base[lane] = e.t_lo; base[count + lane] = e.t_hi; base[2 * count + lane] = e.y_lo; base[3 * count + lane] = e.y_hi; base[4 * count + lane] = e.scale;
}

// ---- the plan's rule (launch_plan.hpp: f2_choose): the cache is taken only when it costs neither a wave per workgroup nor a workgroup per CU.
// Resident workgroups of the sweep kernel on one compute unit: by LDS, at most 32 waves
LDS_HD int sweep_wg_per_cu(size_t bytes, int wpb) {
  size_t k = bytes ? LDS_BUDGET / bytes : 0, cap = (size_t)(32 / wpb);
  if (k > cap) k = cap;
  return k < 1 ? 1 : (int)k;
}
// desc_words: the descriptor area as the launch stages it (lds_sweep_desc_words); wpb: the workgroup width the plan chose WITHOUT the cache
LDS_HD bool src_cache_fits(int tab_len, int desc_words, int lu_words, int n, int wpb, int src_words) {
  if (src_words <= 0) return false;
  const size_t without = lds_bytes(lds_sweep((size_t)0, tab_len, desc_words, lu_words, n, 0, wpb));
  const size_t with = lds_bytes(lds_sweep((size_t)0, tab_len, desc_words, lu_words, n, 0, wpb, src_words));
  return with <= LDS_BUDGET && sweep_wg_per_cu(with, wpb) == sweep_wg_per_cu(without, wpb);
}

}  // namespace cadnip
