"""Noise (adjoint) sweep of the flip-flop, B corners x the 61-point grid (acdec(10, 1e3, 1e9)), output Q_neg: the GPU path of api.noise -- the
kernel k_ac_adj alone (HIP events on the handle's stream, cadnip_profile_*), the whole sweep of api.noise_solve_gpu (pivot analysis,
transfers, kernel, merge, PSD weighting) -- against the host path's dense adjoint solves (api.noise_solve), on the same machine in the same
run.  The sources are the channel thermal noise of every transistor, recorded once as data (one white source per device between drain and
source: the timing does not depend on their strengths).  The host is timed on at most HOST_POINTS corners and scaled to B (its cost per
corner does not depend on B); the line says so.

usage:  timeout -k 10 600 python tools/noise_time.py [B ...]        (default: 1 64 1024)
"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cadnip_jl_amd import api, benchmarks as bm   # noqa: E402
from cadnip_jl_amd.opinfo import _index   # noqa: E402

HOST_POINTS = 4


def run(B, gmin=1e-12):
    circ = bm.dff_circuit()
    pts = [{"vdd": 4.5 + (i * 0.6180339887) % 1.0, "temp": -40.0 + 165.0 * ((i * 0.3819660113 + 0.17) % 1.0)} for i in range(B)]
    freqs = api.acdec(10, 1e3, 1e9)
    sim = api.BatchSimulator(api.MNACircuit(circ, {"vdd": 5.0}, api.MNASpec(mode="dcop")), pts)
    try:
        st = sim.st
        u, conv, _ = sim.dc()
        assert np.all(conv), "DC failed for %d corner(s)" % int((~conv).sum())
        sim.h.rebuild(u, 0.0)
        G, C, _, _ = sim.h.get_GCb()
        import scipy.sparse as sp
        dense = lambda nz: sp.csc_matrix((nz, st.ref_rowval, st.ref_colptr), shape=(st.n, st.n)).toarray()
        info = {d["name"]: d for d in st.opinfo}
        srcs = []
        for d in circ.devices:
            if d.type == "MOS1":
                gl = [_index(st, t) for t in info[d.name]["nodes"]]
                srcs.append((gl[0], gl[2], "white", 1e-24, 0.0, d.name.lower()))
        n_host = min(B, HOST_POINTS)
        Gd, Cd = [None] * B, [None] * B                   # host matrices of the timed corners only: the GPU path needs them for redone rows alone
        for k in range(n_host):
            Gd[k], Cd[k] = dense(G[k]), dense(C[k])
            Gd[k][np.arange(st.n_nodes), np.arange(st.n_nodes)] += gmin
        temps = [p["temp"] for p in pts]

        def sweep():
            stats = {"gpu_systems": 0, "host_systems": 0, "max_berr": 0.0, "wpb": 0}
            api.noise_solve_gpu(sim.h, st, G, C, Gd, Cd, [srcs] * B, "Q_neg", freqs, None, temps, gmin, "gpu", stats)
            return stats
        sweep()                                                                                # warm-up: allocation, code load
        t0 = time.perf_counter()
        stats = sweep()
        t_call = time.perf_counter() - t0
        pairs, _ = api.noise_probe_pairs([srcs])
        e_out = np.zeros(st.n, dtype=complex)
        e_out[st.index_of("Q_neg")] = 1.0
        sim.h.profile(True)
        sim.h.ac_adjoint(2.0 * np.pi * freqs, gmin, e_out, pairs)
        t_kernel = sim.h.profile_read()["ac_adj"][0] * 1e-3
        sim.h.profile(False)
        t0 = time.perf_counter()
        for k in range(n_host):
            api.noise_solve(st, Gd[k], Cd[k], srcs, "Q_neg", freqs, None, temps[k])
        t_host = (time.perf_counter() - t0) * B / n_host
        S = B * len(freqs)
        print("B %5d  systems %6d  pairs %d  W %d  kernel %9.3f ms (%7.3f us/system)  gpu sweep %9.3f ms  host %10.1f ms%s  host/gpu %.1f  max berr %.2g  host rows %d" % (
            B, S, len(pairs), stats["wpb"], t_kernel * 1e3, t_kernel * 1e6 / S, t_call * 1e3, t_host * 1e3,
            " (scaled from %d corners)" % n_host if n_host < B else "", t_host / t_call, stats["max_berr"], stats["host_systems"]), flush=True)
    finally:
        sim.close()


if __name__ == "__main__":
    for B in [int(a) for a in sys.argv[1:]] or [1, 64, 1024]:
        run(B)
