"""The response and K parameter derivatives per factorisation against differencing responses, B points x the 61-point grid (acdec(10, 1e3, 1e9)),
on the same handle in the same run.  The handle holds B (1 + 2 K) instances -- per point the base and 2 K neighbours, as api.sensitivity lays
a perturbed batch out (here the neighbours are other corners of tools/ac_time.py's sweep: the kernels do the same work whatever the step) --
  sens      ONE ac_sens call (k_ac_sens: B x F systems, each factored once; forward and adjoint solve, K bilinear forms over the stamps of
            the neighbours) returning K + 1 numbers per system,
  brute     the 2 K + 1 ac_solve sweeps of B points a caller differences by hand -- made as ONE ac_solve call over all B (1 + 2 K) instances
            (k_ac_lu: the same (2 K + 1) B F factorisations, in one launch, which flatters the baseline) returning every x.
Whole calls (uploads, launches, downloads) by the wall clock, and the kernels alone by HIP events on the handle's stream (cadnip_profile_*).
After one warm-up of each, --reps rounds alternate the two and swap their order every round; every figure is the median with min..max.
  --circuit dff|chain200   as tools/ac_time.py (the flip-flop at B corners; the 200-stage chain at the zero state, beyond LDS: use --memory hbm)
  --memory lds|hbm|auto    where the kernels keep a system's work arrays
  --params K [K ...]       parameters per point (default 1 2 4)

usage:  timeout -k 10 600 python tools/sens_time.py [--circuit dff] [--memory lds] [--params 1 2 4] [--reps 5] [B]        (default B: 64)
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cadnip_jl_amd import api   # noqa: E402
from tools.ac_time import linearised, med   # noqa: E402
from tools.network_time import prof_ms   # noqa: E402


def run(B, circuit, memory, reps, K, gmin=1e-12):
    freqs = api.acdec(10, 1e3, 1e9)
    omegas = 2.0 * np.pi * freqs
    per = 1 + 2 * K
    sim, circ, pts, u, b_ac = linearised(circuit, B * per)
    try:
        st, h, n = sim.st, sim.h, sim.st.n
        G, C, _, _ = h.get_GCb()
        api.ac_analyze_pivots(h, st, G, C, omegas, gmin)
        h.ac_set_memory(memory)
        base = np.arange(B) * per
        plus = base[:, None] + 1 + 2 * np.arange(K)[None, :]
        minus = plus + 1
        scale = np.full((B, K), 0.5)
        out = (n // 2, -1)
        e = np.zeros(n, complex)
        e[out[0]] = 1.0
        calls = {"sens": lambda: h.ac_sens(omegas, gmin, base, plus, minus, scale, b_ac, e, out),
                 "brute": lambda: h.ac_solve(omegas, gmin, b_ac)}
        kernels = {"sens": ("ac_sens", "ac_sens_hbm"), "brute": ("ac_lu", "ac_lu_hbm")}
        ys = calls["sens"]()                                                                 # warm-up: allocation, code load -- and the check
        used = h.ac_plan_info()
        xb = calls["brute"]()
        same = np.array_equal(ys[0].view(np.float64), np.ascontiguousarray(xb[0][base][:, :, out[0]]).view(np.float64))
        wall, kern = {k: [] for k in calls}, {k: [] for k in calls}
        order = list(calls)
        h.profile(True)
        for r in range(reps):
            for name in (order if r % 2 == 0 else order[::-1]):
                k0 = prof_ms(h, kernels[name])
                t0 = time.perf_counter()
                calls[name]()
                wall[name].append(time.perf_counter() - t0)
                kern[name].append((prof_ms(h, kernels[name]) - k0) * 1e-3)
        h.profile(False)
        print("%s B %d  K %d  systems: sens %d, brute %d  memory %s  waves %d  flagged %d  y bit-identical to ac_solve: %s" % (
            circuit, B, K, B * len(freqs), B * per * len(freqs), used["memory"], used["n_waves"], int((ys[4] != 0).any(axis=2).sum()), same))
        for name in order:
            print("    %-6s call %s   kernel %s" % (name, med(wall[name]), med(kern[name])))
        print("    sens / brute: call %.3f  kernel %.3f   brute call spread %.1f%%" % (
            np.median(wall["sens"]) / np.median(wall["brute"]), np.median(kern["sens"]) / np.median(kern["brute"]),
            100 * (max(wall["brute"]) - min(wall["brute"])) / np.median(wall["brute"])), flush=True)
    finally:
        sim.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--circuit", choices=["dff", "chain200"], default="dff")
    ap.add_argument("--memory", choices=["lds", "hbm", "auto"], default="lds")
    ap.add_argument("--params", type=int, nargs="+", default=[1, 2, 4])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("B", type=int, nargs="?", default=64)
    a = ap.parse_args()
    for K in a.params:
        if K >= 1:
            run(a.B, a.circuit, a.memory, max(1, a.reps), K)
