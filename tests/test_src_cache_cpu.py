"""csrc/src_cache.hpp -- the sweep kernel's per-instance source segment cache -- on the CPU: the header is compiled with the host compiler
(-ffp-contract=off) together with a plain copy of the arithmetic of devices.hpp: pwl_at_time / source_value as the reference, and driven
the way k_fused2 drives it: fill at pick-up, at every new time point a hit answers from the entry and a miss runs the reference (with its
segment hint) and refills the entry from the segment it found.  Every value must equal the reference's to the bit, over time sequences
that step inside a segment, land on PWL points exactly, step back across a boundary (a rejected step), lie before the first and behind the
last point, cross a vertical jump, and for DC, pulse and sine sources (the last two must never hit).  Also: a refilled entry never answers a
time the reference resolves to another segment; lds_sweep with the new trailing argument at 0 is the layout it was; the plan's rule
refuses the cache when it would cost a resident instance."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cadnip.jl_amd", "csrc")

SHIM = r"""
#include <math.h>
#include "src_cache.hpp"
using namespace cadnip;
typedef long long i64;

// ---- reference: the arithmetic of devices.hpp (pwl_at_time with its segment hint, pulse_at_time, sind_deg, source_value), copied plainly
static double ref_pwl(const double* ts, const double* ys, int n, double t, int* seg) {
  if (seg) {
    const int i = *seg;
    if (i >= 2 && i <= n) {
      const double t_lo = ts[i - 2], t_hi = ts[i - 1], y_lo = ys[i - 2], y_hi = ys[i - 1];
      if (t_lo < t && t < t_hi) {
        if (y_lo == y_hi) return y_hi;
        return y_lo + (t - t_lo) * ((y_hi - y_lo) / (t_hi - t_lo));
      }
    }
  }
  int lo = 0, hi = n;
  while (lo < hi) { int mid = (lo + hi) >> 1; if (ts[mid] < t) lo = mid + 1; else hi = mid; }
  int i = lo + 1;
  if (i <= n && ts[i - 1] == t) i += 1;
  if (seg) *seg = i;
  if (i <= 1) return ys[0];
  if (i > n) return ys[n - 1];
  if (ys[i - 2] == ys[i - 1]) return ys[i - 1];
  if (ts[i - 1] == ts[i - 2]) return (ys[i - 2] + ys[i - 1]) / 2;
  double slope = (ys[i - 1] - ys[i - 2]) / (ts[i - 1] - ts[i - 2]);
  return ys[i - 2] + (t - ts[i - 2]) * slope;
}
static double ref_pulse(double v1, double v2, double td, double tr, double tf, double pw, double per, double t) {
  if (t < td) return v1;
  double phase;
  if (per > 0) { phase = fmod(t - td, per); if (phase < 0) phase += per; } else phase = t - td;
  if (phase < tr) return tr > 0 ? v1 + (v2 - v1) * (phase / tr) : v2;
  else if (phase < tr + pw) return v2;
  else if (phase < tr + pw + tf) return tf > 0 ? v2 + (v1 - v2) * ((phase - tr - pw) / tf) : v1;
  return v1;
}
static double ref_sind(double deg) {
  double r = fmod(deg, 360.0);
  if (r == 0.0 || r == 180.0 || r == -180.0) return 0.0;
  if (r == 90.0 || r == -270.0) return 1.0;
  if (r == -90.0 || r == 270.0) return -1.0;
  return sin(r * (3.14159265358979323846 / 180.0));
}
static double ref_source(int kind, const double* w, int len, double dc, double scale, double t, int* seg) {
  if (kind == 0) return dc;
  double v;
  if (kind == 1) v = ref_pwl(w, w + len, len, t, seg);
  else if (kind == 2) v = ref_pulse(w[0], w[1], w[2], w[3], w[4], w[5], w[6], t);
  else {
    double vo = w[0], va = w[1], freq = w[2], td = w[3], theta = w[4], phase = w[5];
    if (t < td) v = vo + va * ref_sind(phase);
    else v = vo + va * exp(-theta * (t - td)) * ref_sind(360 * freq * (t - td) + phase);
  }
  return scale * v;
}

extern "C" {
// One source through a sequence of time points, as k_fused2 drives the cache (one lane, region of `count` lanes, this one at `lane`).
// got[k]: the value the cached path hands the stamps; ref[k]: the reference without any cache or hint; hit[k]: 1 = answered from the entry;
// segref[k]: the segment an un-hinted reference search resolves t[k] to (PWL; 0 otherwise); seghit[k]: on a hit, the segment the entry was
// refilled from (-1: the fill at pick-up).  Returns the number of hits.
int sc_drive(int kind, const double* w, int len, double dc, double scale, const double* t, int nt, int count, int lane,
             double* got, double* ref, int* hit, int* segref, int* seghit) {
  double* region = new double[src_cache_words(count) + 2];
  for (int i = 0; i < src_cache_words(count) + 2; ++i) region[i] = -7.0;      // (+2: guard words behind the region)
  const int cl = src_cache_lanes(count);
  src_seg_store(region, cl, lane, src_seg_fill(kind, dc));
  int seg = 0, entry_seg = -1, hits = 0;
  for (int k = 0; k < nt; ++k) {
    int s0 = 0;
    ref[k] = ref_source(kind, w, len, dc, scale, t[k], nullptr);
    if (kind == 1) { (void)ref_pwl(w, w + len, len, t[k], &s0); }
    segref[k] = kind == 1 ? s0 : 0;
    const SrcSeg e = src_seg_load((const double*)region, cl, lane);
    if (src_seg_hit(e, t[k])) { got[k] = src_seg_value(e, t[k]); hit[k] = 1; seghit[k] = entry_seg; ++hits; }
    else {
      got[k] = ref_source(kind, w, len, dc, scale, t[k], &seg);               // the existing path, unchanged, with its hint
      src_seg_store(region, cl, lane, src_seg_refill(kind, w, w + len, len, seg, scale));
      entry_seg = kind == 1 ? seg : -1;
      hit[k] = 0; seghit[k] = -2;
    }
  }
  int guard_ok = region[src_cache_words(count)] == -7.0 && region[src_cache_words(count) + 1] == -7.0;
  delete[] region;
  return guard_ok ? hits : -1;
}
void sc_fill(int kind, double dc, double* o) { const SrcSeg e = src_seg_fill(kind, dc); o[0] = e.t_lo; o[1] = e.t_hi; o[2] = e.y_lo; o[3] = e.y_hi; o[4] = e.scale; }
void sc_refill(int kind, const double* w, int len, int i, double scale, double* o) {
  const SrcSeg e = src_seg_refill(kind, w, w + len, len, i, scale); o[0] = e.t_lo; o[1] = e.t_hi; o[2] = e.y_lo; o[3] = e.y_hi; o[4] = e.scale;
}
int sc_words(int count) { return src_cache_words(count); }
int sc_lanes(int count) { return src_cache_lanes(count); }
// o: desc, W, u, beta, end, nW, per, bytes | src (with the trailing argument)
void sc_sweep(int tab, int desc, int lu, int n, int w, int wpb, int src_words, int use_default, i64* o) {
  const LdsSweep<size_t> L = use_default ? lds_sweep((size_t)0, tab, desc, lu, n, w, wpb) : lds_sweep((size_t)0, tab, desc, lu, n, w, wpb, src_words);
  o[0] = L.desc; o[1] = L.W; o[2] = L.u; o[3] = L.beta; o[4] = L.end; o[5] = L.nW; o[6] = L.per; o[7] = lds_bytes(L); o[8] = L.src;
}
int sc_fits(int tab, int desc, int lu, int n, int wpb, int src_words) { return src_cache_fits(tab, desc, lu, n, wpb, src_words) ? 1 : 0; }
int sc_wg_per_cu(i64 bytes, int wpb) { return sweep_wg_per_cu((size_t)bytes, wpb); }
}
"""


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    d = tmp_path_factory.mktemp("src_cache")
    src, so = str(d / "shim.cpp"), str(d / "libshim.so")
    with open(src, "w") as f:
        f.write(SHIM)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-shared", "-fPIC", "-I", CSRC, "-o", so, src])
    return C.CDLL(so)


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _drive(lib, kind, wave, times, dc=0.3, scale=1.0, count=7, lane=3):
    w = np.ascontiguousarray(wave, dtype=np.float64)
    t = np.ascontiguousarray(times, dtype=np.float64)
    ln = len(w) // 2 if kind == 1 else len(w)
    got, ref = np.zeros(len(t)), np.zeros(len(t))
    hit, segref, seghit = (np.zeros(len(t), dtype=np.int32) for _ in range(3))
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
    hits = lib.sc_drive(kind, _dp(w), ln, C.c_double(dc), C.c_double(scale), _dp(t), len(t), count, lane, _dp(got), _dp(ref), ip(hit), ip(segref), ip(seghit))
    assert hits >= 0, "the region's guard words were written"
    # exact equality, every value; and a hit only ever answers from the segment the reference resolves that time to
    assert np.array_equal(got.view(np.uint64), ref.view(np.uint64)), (got, ref)
    on = (hit == 1) & (seghit >= 0)
    assert np.array_equal(seghit[on], segref[on])
    return hit, segref


# the flip-flop's kind of wave: ramps between flat stretches (8 points), and one with a vertical jump at t = 3 (two equal ts)
TS = np.array([0.0, 1e-9, 1.1e-9, 5e-9, 5.1e-9, 9e-9, 9.1e-9, 6e-7])
YS = np.array([0.0, 0.0, 5.0, 5.0, 0.0, 0.0, 3.3, 1.7])
PWL = np.concatenate([TS, YS])
JUMP = np.concatenate([[0.0, 1.0, 3.0, 3.0, 4.0, 6.0], [0.5, 1.5, 1.5, 2.5, 2.0, -1.0]])


def test_increasing_steps_inside_segments_hit_and_equal(lib):
    t = np.concatenate([np.linspace(a, b, 9)[1:-1] for a, b in zip(TS[:-1], TS[1:])])
    hit, seg = _drive(lib, 1, PWL, t, scale=0.7)
    # the first point of every segment misses (the entry is refilled), the six after it hit
    assert hit.reshape(7, 7)[:, 0].sum() == 0 and hit.reshape(7, 7)[:, 1:].all()
    assert seg.tolist() == sorted(seg.tolist()) and set(seg.tolist()) == set(range(2, 9))


def test_breakpoint_landings_never_hit(lib):
    """times equal to a PWL point to the bit: the open interval excludes both ends, the reference resolves the point (+1 on an exact hit)"""
    t = np.repeat(TS, 2)
    t[1::2] = np.nextafter(TS, np.inf)
    hit, seg = _drive(lib, 1, PWL, t)
    assert hit[0::2].sum() == 0
    assert seg[0::2].tolist() == list(range(2, 10))
    t = np.sort(np.concatenate([TS, np.nextafter(TS, -np.inf), np.nextafter(TS, np.inf), 0.5 * (TS[:-1] + TS[1:])]))
    _drive(lib, 1, PWL, t)
    _drive(lib, 1, PWL, t[::-1])


def test_step_back_across_a_boundary(lib):
    """a rejected step: the time goes back over a PWL point after the entry was refilled from the segment behind it"""
    t = [0.5e-9, 0.9e-9, 1.05e-9, 0.95e-9, 1.0e-9, 1.02e-9, 1.08e-9, 1.1e-9, 1.09e-9, 3e-9, 1.05e-9, 4e-9, 5.05e-9, 4.99e-9, 5.0e-9]
    hit, seg = _drive(lib, 1, PWL, t, scale=-2.5)
    assert hit.tolist() == [0, 1, 0, 0, 0, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0]
    assert seg.tolist() == [2, 2, 3, 2, 3, 3, 3, 4, 3, 4, 3, 4, 5, 4, 5]


def test_before_the_first_and_behind_the_last_point(lib):
    t = [-5.0, -1e-12, -1e-300, 0.0, 1e-12, 5.9e-7, 6e-7, 6.0000001e-7, 6.5e-7, 7e-7, 1.0, 6e-7, 5.9e-7, -1.0, -2.0]
    hit, seg = _drive(lib, 1, PWL, t, scale=1.25)
    # the constant end regions are cached as half-infinite segments: the long flat tail behind the last point hits -- from the landing on
    # the last point itself on, which the reference resolves behind it (segment len + 1) and which therefore refills the entry with (6e-7, inf)
    assert hit.tolist() == [0, 1, 1, 0, 1, 0, 0, 1, 1, 1, 1, 0, 0, 0, 1]
    assert seg[:4].tolist() == [1, 1, 1, 2] and seg[6:11].tolist() == [9] * 5


def test_vertical_jump_is_never_cached(lib):
    t = [2.0, 2.5, 3.0, 3.0, np.nextafter(3.0, 4.0), 3.5, np.nextafter(3.0, 0.0), 3.0, 3.25, 5.0, 3.0, 2.9]
    hit, seg = _drive(lib, 1, JUMP, t)
    assert hit.tolist() == [0, 1, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0]
    assert seg[2] == 4 and seg[3] == 4                      # t == 3.0 resolves to the zero-width segment between the two equal points (value: their mean)
    out = np.zeros(5)
    for i in range(1, 8):
        lib.sc_refill(1, _dp(JUMP), 6, i, C.c_double(1.0), _dp(out))
        if i == 4:                                          # the zero-width segment (ts[2] == ts[3]): an entry that cannot hit
            assert out[0] == np.inf
        else:
            assert out[0] < out[1]


def test_dc_source_always_hits(lib):
    t = [-1.0, 0.0, 1e-9, 1e-9, 5e-7, 1e300, -1e300]
    for dc in (0.0, 5.0, -3.3, 1e-300, np.nextafter(1.0, 2.0)):
        hit, _ = _drive(lib, 0, [0.0], t, dc=dc, scale=0.123)       # (source_value ignores the scale of a DC source)
        assert hit.all()
    out = np.zeros(5)
    lib.sc_fill(0, C.c_double(2.5), _dp(out))
    assert out.tolist() == [-np.inf, np.inf, 2.5, 2.5, 1.0]


def test_pulse_and_sine_never_hit(lib):
    t = np.linspace(-1e-9, 5e-8, 41)
    hit, _ = _drive(lib, 2, [0.0, 5.0, 1e-9, 1e-10, 2e-10, 4e-9, 1e-8], t, scale=0.9)
    assert hit.sum() == 0
    hit, _ = _drive(lib, 3, [0.5, 1.5, 1e8, 2e-9, 1e7, 30.0], t, scale=1.1)
    assert hit.sum() == 0
    out = np.zeros(5)
    for kind in (1, 2, 3):                                  # at pick-up only a DC source has an entry that answers
        lib.sc_fill(kind, C.c_double(2.5), _dp(out))
        assert out[0] == np.inf
    for kind in (0, 2, 3):                                  # and only a PWL source is ever refilled
        lib.sc_refill(kind, _dp(PWL), 8, 3, C.c_double(1.0), _dp(out))
        assert out[0] == np.inf


def test_random_walks_equal_the_reference(lib):
    rng = np.random.default_rng(5)
    for trial in range(20):
        n = int(rng.integers(1, 9))
        ts = np.sort(rng.random(n))
        if n > 2 and trial % 3 == 0:
            ts[1] = ts[2]                                   # a vertical jump
        ys = np.round(rng.random(n) * 4) / 2                # equal neighbours occur
        t = np.cumsum(rng.normal(0.02, 0.05, 300)) % 1.4 - 0.2
        t[::17] = ts[rng.integers(0, n, len(t[::17]))]      # exact landings
        _drive(lib, 1, np.concatenate([ts, ys]), t, scale=float(rng.normal()), count=int(rng.integers(1, 80)), lane=0)


def test_region_size(lib):
    assert [lib.sc_lanes(c) for c in (0, 1, 7, 64, 70)] == [0, 1, 7, 64, 64]
    assert [lib.sc_words(c) for c in (0, 1, 2, 7, 64, 70)] == [0, 6, 10, 36, 320, 320]


SIZES = [(1091, 235), (1, 1), (3, 1), (2, 2), (6000, 2000)]


def _sweep(lib, tab, desc, lu, n, w, wpb, src_words=0, use_default=0):
    o = (C.c_longlong * 9)()
    lib.sc_sweep(tab, desc, lu, n, w, wpb, src_words, use_default, o)
    return list(o)


def test_layout_with_the_argument_at_zero_is_the_parents(lib):
    for (lu, n), tab, desc, wpb in [(s, t, d, w) for s in SIZES for t in (0, 4096) for d in (0, 2432 + 152) for w in (1, 8)]:
        for w in range(wpb):
            nW = lu + n + 64
            per = nW + 2 + 2 * n
            W = tab // 2 + desc + w * per
            old = [tab // 2, W, W + nW + 2, W + nW + 2 + n, tab // 2 + desc + wpb * per, nW, per, 8 * (tab // 2 + desc + wpb * per)]
            assert _sweep(lib, tab, desc, lu, n, w, wpb, 0, 1)[:8] == old
            assert _sweep(lib, tab, desc, lu, n, w, wpb, 0, 0)[:8] == old
            # with the region: behind beta, inside the instance, everything before it where it was relative to W, W still on 16 bytes
            for sw in (6, 36, 320):
                L = _sweep(lib, tab, desc, lu, n, w, wpb, sw)
                assert L[6] == per + sw and L[1] == tab // 2 + desc + w * (per + sw) and L[1] % 2 == 0
                assert (L[2] - L[1], L[3] - L[1], L[8] - L[1]) == (nW + 2, nW + 2 + n, nW + 2 + 2 * n)
                assert L[8] + sw == L[1] + L[6] and L[4] == tab // 2 + desc + wpb * (per + sw)


def test_plan_rule_refuses_the_cache_when_it_costs_a_resident_instance(lib):
    BUDGET = 160 * 1024
    assert lib.sc_wg_per_cu(BUDGET, 8) == 1 and lib.sc_wg_per_cu(BUDGET // 2, 8) == 2 and lib.sc_wg_per_cu(BUDGET // 2 + 8, 8) == 1
    assert lib.sc_wg_per_cu(1000, 8) == 4 and lib.sc_wg_per_cu(1000, 1) == 32
    # the flip-flop as the benchmark runs it: lean tables of 4096 words, 19 pre-decoded steps, eight instances -- the 36 words fit
    assert lib.sc_fits(4096, 2432 + 152, 1091, 235, 8, 36) == 1
    assert lib.sc_fits(4096, 2432 + 152, 1091, 235, 8, 0) == 0
    # a workgroup that fills the LDS to the last 100 bytes: the region would push it over the budget
    lu, n = 1091, 235
    per = lu + n + 64 + 2 + 2 * n
    for wpb in (1, 8):
        room = BUDGET // 8 - wpb * per                      # doubles left for tables and descriptors
        tab = 2 * (room - 10) // 4 * 4
        used = _sweep(lib, tab, 0, lu, n, 0, wpb)[7]
        assert BUDGET - 200 < used <= BUDGET
        assert lib.sc_fits(tab, 0, lu, n, wpb, 36) == 0
        assert lib.sc_fits(tab, 0, lu, n, wpb, 2) == (1 if used + 16 * wpb <= BUDGET else 0)
    # three workgroups per CU by LDS with 64 bytes to spare in a third of the budget: 36 words per instance make it two
    wpb = 1
    third = BUDGET // 3 // 8
    tab = 2 * (third - per - 8) // 4 * 4
    used = _sweep(lib, tab, 0, lu, n, 0, wpb)[7]
    assert lib.sc_wg_per_cu(used, wpb) == 3 and lib.sc_wg_per_cu(used + 36 * 8, wpb) == 2
    assert lib.sc_fits(tab, 0, lu, n, wpb, 36) == 0
    assert lib.sc_fits(tab, 0, lu, n, wpb, 2) == 1
