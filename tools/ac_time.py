"""AC sweep of the flip-flop, B corners x the 61-point grid (acdec(10, 1e3, 1e9)): the GPU path of api.ac -- the kernel k_ac_lu alone (HIP
events on the handle's stream, cadnip_profile_*), the whole sweep (pivot analysis, transfers, kernel, merge) -- against the host path's dense
solves, on the same machine in the same run.  The host is timed on at most HOST_POINTS corners and scaled to B (its cost per corner does not
depend on B); the line says so.

usage:  timeout -k 10 600 python tools/ac_time.py [B ...]        (default: 1 64 1024)
"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cadnip_jl_amd import api, benchmarks as bm   # noqa: E402

HOST_POINTS = 4


def run(B, gmin=1e-12):
    circ = bm.dff_circuit()
    next(d for d in circ.devices if d.type == "V" and d.name.lower() == "vd").params["ac"] = 1.0
    pts = [{"vdd": 4.5 + (i * 0.6180339887) % 1.0, "temp": -40.0 + 165.0 * ((i * 0.3819660113 + 0.17) % 1.0)} for i in range(B)]
    freqs = api.acdec(10, 1e3, 1e9)
    omegas = 2.0 * np.pi * freqs
    sim = api.BatchSimulator(api.MNACircuit(circ, {"vdd": 5.0}, api.MNASpec(mode="dcop")), pts)
    try:
        st = sim.st
        u, conv, _ = sim.dc()
        assert np.all(conv), "DC failed for %d corner(s)" % int((~conv).sum())
        sim.h.rebuild(u, 0.0)
        G, C, _, _ = sim.h.get_GCb()
        import scipy.sparse as sp
        dense = lambda nz: sp.csc_matrix((nz, st.ref_rowval, st.ref_colptr), shape=(st.n, st.n)).toarray()
        sols = []
        for k in range(B if B <= HOST_POINTS else HOST_POINTS):
            Gd = dense(G[k])
            Gd[np.arange(st.n_nodes), np.arange(st.n_nodes)] += gmin
            sols.append(api.ACSol(st, Gd, dense(C[k]), api.rhs_ac(st, circ, {"vdd": pts[k]["vdd"]}), u[k], freqs))
        b_ac = np.tile(sols[0].b_ac, (B, 1))
        shells = [api.ACSol(st, None, None, b_ac[k], None, freqs) for k in range(B)]          # cache targets of the sweep (no host matrices)

        def sweep():
            stats = {"gpu_systems": 0, "host_systems": 0, "max_berr": 0.0, "wpb": 0}
            api.ac_gpu_sweep(sim.h, st, shells, G, C, omegas, gmin, "gpu", stats)
            return stats
        sweep()                                                                                # warm-up: allocation, code load
        t0 = time.perf_counter()
        stats = sweep()
        t_call = time.perf_counter() - t0
        sim.h.profile(True)
        sim.h.ac_solve(omegas, gmin, b_ac)
        t_kernel = sim.h.profile_read()["ac_lu"][0] * 1e-3
        sim.h.profile(False)
        t0 = time.perf_counter()
        for s in sols:
            s._solve(omegas)
        t_host = (time.perf_counter() - t0) * B / len(sols)
        S = B * len(freqs)
        print("B %5d  systems %6d  W %d  kernel %9.3f ms (%7.3f us/system)  gpu sweep %9.3f ms  host %10.1f ms%s  host/gpu %.1f  max berr %.2g  host rows %d" % (
            B, S, stats["wpb"], t_kernel * 1e3, t_kernel * 1e6 / S, t_call * 1e3, t_host * 1e3,
            " (scaled from %d corners)" % len(sols) if len(sols) < B else "", t_host / t_call, stats["max_berr"], stats["host_systems"]), flush=True)
    finally:
        sim.close()


if __name__ == "__main__":
    for B in [int(a) for a in sys.argv[1:]] or [1, 64, 1024]:
        run(B)
