"""The Arnoldi reduction in the wave against what a caller can do without it, B points x S shifts (one per decade from 1 kHz) of the flip-flop,
on the same handle in the same run:
  arnoldi   ONE ac_arnoldi call (k_ac_arnoldi: B x S systems, each factored once, then m + 1 columns whose right-hand sides are C times the
            previous solution, orthogonalised in the wave) returning H, beta, m_eff and the probe row,
  solves    the m + 1 ac_solve calls with host matvecs a caller would make today: per step one launch over the B x S systems (each factors
            again), the solutions down, two passes of modified Gram-Schmidt and the product with C on the host, the next right-hand sides up.
            ac_solve takes one right-hand side per INSTANCE, so the S shifts of a point cannot share a call: S calls per step,
  dense     the host's dense pencil per point (scipy.linalg.eig of (-G, C): every finite pole, O(n^3)), on --dense-points of the B points.
Whole calls by the wall clock, and the kernels alone by HIP events on the handle's stream (cadnip_profile_*).  After one warm-up of each,
--reps rounds alternate the GPU paths and swap their order every round; every figure is the median with min..max.
  --memory lds|hbm|auto    where the kernels keep a system's work arrays
  --orders m [m ...]       Arnoldi steps (default 8 16 32)

usage:  timeout -k 10 600 python tools/pz_time.py [--memory lds] [--orders 8 16 32] [--shifts 7] [--reps 5] [B]        (default B: 64)
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


def by_solves(h, st, Cd, omegas, gmin, b_ac, m):
    """m + 1 rounds of ac_solve calls with the Gram-Schmidt passes and C v on the host: the composition the kernel replaces (no breakdown test)"""
    B, S, n = len(Cd), len(omegas), st.n
    solve = lambda rhs: np.stack([h.ac_solve(omegas[s:s + 1], gmin, rhs[:, s])[0][:, 0] for s in range(S)], axis=1)      # [B, S, n]
    x = solve(np.broadcast_to(np.asarray(b_ac, complex), (B, S, n)))
    V = [x / np.linalg.norm(x, axis=2, keepdims=True)]
    H = np.zeros((B, S, m + 1, m), complex)
    for j in range(m):
        w = solve(np.einsum("bij,bsj->bsi", Cd, V[j]))
        for _ in range(2):
            for i in range(j + 1):
                hh = np.einsum("bsk,bsk->bs", V[i].conj(), w)
                w = w - hh[:, :, None] * V[i]
                H[:, :, i, j] += hh
        nu = np.linalg.norm(w, axis=2)
        H[:, :, j + 1, j] = nu
        V.append(w / np.where(nu > 0, nu, 1.0)[:, :, None])
    return H


def run(B, memory, reps, orders, n_shifts, dense_points, gmin=1e-12):
    omegas = 2.0 * np.pi * 1e3 * 10.0 ** np.arange(n_shifts)
    sim, circ, pts, u, b_ac = linearised("dff", B)
    try:
        st, h, n = sim.st, sim.h, sim.st.n
        G, C, _, _ = h.get_GCb()
        api.ac_analyze_pivots(h, st, G, C, omegas, gmin)
        to_ref = np.asarray(st.to_ref_nz)
        h.ac_set_memory(memory)
        rows = np.repeat(np.arange(n), np.diff(st.rowptr))
        Gd, Cd = np.zeros((B, n, n)), np.zeros((B, n, n))
        Gd[:, rows, np.asarray(st.colidx)] = np.asarray(G)[:, to_ref]
        Cd[:, rows, np.asarray(st.colidx)] = np.asarray(C)[:, to_ref]
        Gd[:, np.arange(st.n_nodes), np.arange(st.n_nodes)] += gmin
        out = [(n // 2, -1)]
        t0 = time.perf_counter()
        for k in range(min(dense_points, B)):
            api.poles_dense(Gd[k], Cd[k])
        dense = (time.perf_counter() - t0) / max(1, min(dense_points, B))
        print("dff B %d  shifts %d  n %d  memory %s   dense pencil: %.1f ms per point (x %d points = %.2f s)" % (B, n_shifts, n, memory, dense * 1e3, B, dense * B))
        for m in orders:
            calls = {"arnoldi": lambda: h.ac_arnoldi(omegas, gmin, b_ac, m, out), "solves": lambda: by_solves(h, st, Cd, omegas, gmin, b_ac, m)}
            kernels = {"arnoldi": ("ac_arnoldi", "ac_arnoldi_hbm"), "solves": ("ac_lu", "ac_lu_hbm")}
            got = calls["arnoldi"]()                                                             # warm-up: allocation, code load -- and the check
            used = h.ac_plan_info()
            Hs = calls["solves"]()
            full = got[2] == m                                                                   # systems without a breakdown: the same H to rounding
            dev = float(np.max(np.abs(got[0][full] - Hs[full]) / np.max(np.abs(got[0][full]), axis=(1, 2), keepdims=True))) if full.any() else 0.0
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
            print("  m %d  systems %d  wpb %d  waves %d  breakdowns %d  flagged %d  max berr %.2g  H against the composed solves (systems without breakdown) %.2g" % (
                m, B * n_shifts, got[7]["wpb"], used["n_waves"], int(((got[6] & 4) != 0).sum()), int(((got[6] & 3) != 0).sum()), float(np.nanmax(got[5])), dev))
            for name in order:
                print("    %-8s call %s   kernel %s" % (name, med(wall[name]), med(kern[name])))
            print("    arnoldi / solves: call %.3f  kernel %.3f    arnoldi call / dense pencils of the B points: %.4f" % (
                np.median(wall["arnoldi"]) / np.median(wall["solves"]), np.median(kern["arnoldi"]) / np.median(kern["solves"]),
                np.median(wall["arnoldi"]) / (dense * B)), flush=True)
    finally:
        sim.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--memory", choices=["lds", "hbm", "auto"], default="lds")
    ap.add_argument("--orders", type=int, nargs="+", default=[8, 16, 32])
    ap.add_argument("--shifts", type=int, default=7)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--dense-points", type=int, default=4)
    ap.add_argument("B", type=int, nargs="?", default=64)
    a = ap.parse_args()
    run(a.B, a.memory, max(1, a.reps), [m for m in a.orders if m >= 1], max(1, a.shifts), max(1, a.dense_points))
