"""K adjoint right-hand sides per factorisation against K adjoint sweeps, B points x the 61-point grid (acdec(10, 1e3, 1e9)), on the same handle
in the same run:
  probes    ONE ac_adjoint_multi call (k_ac_adj_multi: each system factored once, K columns solved) returning the probe differences of
            every column -- what api.network_noise and api.noise(output=[...]) move,
  with_x    the same call returning x for every column as well (into the caller's array, x_out: no first touch of a fresh array),
  baseline  K back-to-back ac_adjoint calls without x (k_ac_adj: K factorisations of the same matrices) -- the same probes, column by column,
  base_x    K back-to-back ac_adjoint calls with x.
Column k is e of unknown (k n) // K; the probe pairs are (i, -1) for 16 unknowns spread over the circuit.
Whole calls (uploads, launches, downloads) by the wall clock, and the kernels alone by HIP events on the handle's stream (cadnip_profile_*).
After one warm-up of each, --reps rounds alternate the four and swap their order every round; every figure is the median with min..max.
From the kernel times of K = 1 and K the split follows: t(K) = factor + K * column  =>  column = (t(K) - t(1)) / (K - 1).
  --circuit dff|chain200   as tools/ac_time.py (the flip-flop at B corners; the 200-stage chain at the zero state, beyond LDS: use --memory hbm)
  --memory lds|hbm|auto    where the kernels keep a system's work arrays
  --rhs K [K ...]          columns per system (default 1 2 4)

usage:  timeout -k 10 600 python tools/network_noise_time.py [--circuit dff] [--memory lds] [--rhs 1 2 4] [--reps 5] [B]        (default B: 64)
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

MULTI, SINGLE = ("ac_adj_multi", "ac_adj_multi_hbm"), ("ac_adj", "ac_adj_hbm")


def run(B, circuit, memory, reps, rhs_counts, gmin=1e-12):
    freqs = api.acdec(10, 1e3, 1e9)
    omegas = 2.0 * np.pi * freqs
    sim, circ, pts, u, _ = linearised(circuit, B)
    try:
        st, h, n = sim.st, sim.h, sim.st.n
        G, C, _, _ = h.get_GCb()
        api.ac_analyze_pivots(h, st, G, C, omegas, gmin)
        h.ac_set_memory(memory)
        S = B * len(freqs)
        pairs = [((j * n) // 16, -1) for j in range(16)]
        kernel1 = None
        for K in rhs_counts:
            c = np.zeros((K, n), complex)
            c[np.arange(K), [(k * n) // K for k in range(K)]] = 1.0
            mine = np.zeros((B, len(freqs), K, n), complex)
            calls = {"probes": lambda: h.ac_adjoint_multi(omegas, gmin, c, pairs),
                     "with_x": lambda: h.ac_adjoint_multi(omegas, gmin, c, pairs, 0, True, mine),
                     "baseline": lambda: [h.ac_adjoint(omegas, gmin, c[k], pairs) for k in range(K)],
                     "base_x": lambda: [h.ac_adjoint(omegas, gmin, c[k], pairs, 0, True) for k in range(K)]}
            kernels = {"probes": MULTI, "with_x": MULTI, "baseline": SINGLE, "base_x": SINGLE}
            hm = calls["with_x"]()                                                           # warm-up: allocation, code load -- and the check
            hb = calls["base_x"]()
            calls["probes"]()
            calls["baseline"]()
            same = all(np.array_equal(hm[0][:, :, k].view(np.float64), hb[k][0].view(np.float64)) and
                       np.array_equal(hm[1][:, :, k].view(np.float64), hb[k][1].view(np.float64)) for k in range(K))
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
            mk = np.median(kern["probes"])
            if K == 1:
                kernel1 = mk
            split = ""
            if K > 1 and kernel1 is not None:
                col = (mk - kernel1) / (K - 1)
                split = "\n    split (multi kernel, probes): factor %.3f ms + %.3f ms per column (%.0f%% / %.0f%% of a single adjoint sweep's kernel)" % (
                    (kernel1 - col) * 1e3, col * 1e3, 100 * (kernel1 - col) / kernel1, 100 * col / kernel1)
            print("%s B %d  systems %d  K %d  memory %s  waves %d  columns bit-identical to ac_adjoint: %s" % (circuit, B, S, K, used["memory"], used["n_waves"], same))
            for name in order:
                print("    %-8s call %s   kernel %s" % (name, med(wall[name]), med(kern[name])))
            ratio = lambda a, b, t: np.median(t[a]) / np.median(t[b])
            print("    probes / baseline: call %.3f  kernel %.3f   with_x / base_x: call %.3f  kernel %.3f   baseline call spread %.1f%%%s" % (
                ratio("probes", "baseline", wall), ratio("probes", "baseline", kern), ratio("with_x", "base_x", wall), ratio("with_x", "base_x", kern),
                100 * (max(wall["baseline"]) - min(wall["baseline"])) / np.median(wall["baseline"]), split), flush=True)
    finally:
        sim.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--circuit", choices=["dff", "chain200"], default="dff")
    ap.add_argument("--memory", choices=["lds", "hbm", "auto"], default="lds")
    ap.add_argument("--rhs", type=int, nargs="+", default=[1, 2, 4])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("B", type=int, nargs="?", default=64)
    a = ap.parse_args()
    run(a.B, a.circuit, a.memory, max(1, a.reps), [k for k in a.rhs if k >= 1])
