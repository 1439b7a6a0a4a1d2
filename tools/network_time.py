"""K right-hand sides per factorisation against K sweeps, B points x the 61-point grid (acdec(10, 1e3, 1e9)), on the same handle in the same run:
  multi     ONE ac_solve_multi call (k_ac_lu_multi: each system factored once, K columns solved) returning x for every column,
  reuse     the same call into the caller's array (x_out): without the first touch of a fresh [B, F, K, n] array,
  probes    the same call returning only K probe values per column (want_x=False: what api.network moves),
  baseline  K back-to-back ac_solve calls (k_ac_lu: K factorisations of the same matrices) -- the same x, column by column.
Whole calls (uploads, launches, downloads) by the wall clock, and the kernels alone by HIP events on the handle's stream (cadnip_profile_*).
After one warm-up of each, --reps rounds alternate the four and swap their order every round; every figure is the median with min..max.
From the kernel times of K = 1 and K the split follows: t(K) = factor + K * column  =>  column = (t(K) - t(1)) / (K - 1).
  --circuit dff|chain200   as tools/ac_time.py (the flip-flop at B corners; the 200-stage chain at the zero state, beyond LDS: use --memory hbm)
  --memory lds|hbm|auto    where the kernels keep a system's work arrays
  --rhs K [K ...]          columns per system (default 1 2 4 8)

usage:  timeout -k 10 600 python tools/network_time.py [--circuit dff] [--memory lds] [--rhs 1 2 4 8] [--reps 5] [B]        (default B: 64)
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


def prof_ms(h, names):
    p = h.profile_read()
    return sum(p.get(nm, (0.0, 0))[0] for nm in names)


def run(B, circuit, memory, reps, rhs_counts, gmin=1e-12):
    freqs = api.acdec(10, 1e3, 1e9)
    omegas = 2.0 * np.pi * freqs
    sim, circ, pts, u, b_ac1 = linearised(circuit, B)
    try:
        st, h, n = sim.st, sim.h, sim.st.n
        G, C, _, _ = h.get_GCb()
        api.ac_analyze_pivots(h, st, G, C, omegas, gmin)
        h.ac_set_memory(memory)
        S = B * len(freqs)
        kernel1 = None
        for K in rhs_counts:
            rows = [(k * n) // K for k in range(K)]
            b = np.zeros((K, n), complex)
            b[np.arange(K), rows] = 1.0
            b[0] = b_ac1                                                                     # column 0: the circuit's own excitation
            pairs = [(r, -1) for r in rows]
            mine = np.zeros((B, len(freqs), K, n), complex)
            calls = {"multi": lambda: h.ac_solve_multi(omegas, gmin, b, None, 0, True),
                     "reuse": lambda: h.ac_solve_multi(omegas, gmin, b, None, 0, True, mine),
                     "probes": lambda: h.ac_solve_multi(omegas, gmin, b, pairs, 0, False),
                     "baseline": lambda: [h.ac_solve(omegas, gmin, b[k]) for k in range(K)]}
            kernels = {"multi": ("ac_lu_multi", "ac_lu_multi_hbm"), "reuse": ("ac_lu_multi", "ac_lu_multi_hbm"), "probes": ("ac_lu_multi", "ac_lu_multi_hbm"), "baseline": ("ac_lu", "ac_lu_hbm")}
            xm = calls["multi"]()                                                            # warm-up: allocation, code load -- and the check
            xb = calls["baseline"]()
            calls["probes"]()
            calls["reuse"]()
            same = all(np.array_equal(xm[1][:, :, k].view(np.float64), xb[k][0].view(np.float64)) for k in range(K))
            used = h.ac_plan_info()
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
            mk, bk = np.median(kern["multi"]), np.median(kern["baseline"])
            if K == 1:
                kernel1 = mk
            split = ""
            if K > 1 and kernel1 is not None:
                col = (mk - kernel1) / (K - 1)
                split = "  split (multi kernel): factor %.3f ms + %.3f ms per column (%.0f%% / %.0f%% of a single sweep's kernel)" % (
                    (kernel1 - col) * 1e3, col * 1e3, 100 * (kernel1 - col) / kernel1, 100 * col / kernel1)
            print("%s B %d  systems %d  K %d  memory %s  waves %d  columns bit-identical to ac_solve: %s" % (circuit, B, S, K, used["memory"], used["n_waves"], same))
            for name in order:
                print("    %-8s call %s   kernel %s" % (name, med(wall[name]), med(kern[name])))
            print("    multi / baseline: call %.3f  kernel %.3f   reuse / baseline: call %.3f   probes / baseline: call %.3f   baseline call spread %.1f%%%s" % (
                np.median(wall["multi"]) / np.median(wall["baseline"]), mk / bk, np.median(wall["reuse"]) / np.median(wall["baseline"]), np.median(wall["probes"]) / np.median(wall["baseline"]),
                100 * (max(wall["baseline"]) - min(wall["baseline"])) / np.median(wall["baseline"]), "\n  " + split if split else ""), flush=True)
    finally:
        sim.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--circuit", choices=["dff", "chain200"], default="dff")
    ap.add_argument("--memory", choices=["lds", "hbm", "auto"], default="lds")
    ap.add_argument("--rhs", type=int, nargs="+", default=[1, 2, 4, 8])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("B", type=int, nargs="?", default=64)
    a = ap.parse_args()
    run(a.B, a.circuit, a.memory, max(1, a.reps), [k for k in a.rhs if k >= 1])
