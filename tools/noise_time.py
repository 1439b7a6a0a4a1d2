"""Noise (adjoint) sweep, B points x the 61-point grid (acdec(10, 1e3, 1e9)): the GPU path of api.noise -- the kernel alone (HIP events on the
handle's stream, cadnip_profile_*), the whole sweep of api.noise_solve_gpu (pivot analysis, transfers, kernel, merge, PSD weighting) --
against the host path's dense adjoint solves (api.noise_solve), on the same machine in the same run.  Circuits, --memory, --reps and the
median (min..max) figures as tools/ac_time.py; the output is Q_neg (flip-flop) / n200 (chain200).  The sources are the channel thermal noise
of every transistor, recorded once as data (one white source per device between drain and source: the timing does not depend on their
strengths).  The host is timed on at most HOST_POINTS points (chain200: one point, HOST_FREQS frequencies) and scaled to the grid; the line
says so.

usage:  timeout -k 10 600 python tools/noise_time.py [--circuit dff] [--memory lds] [--reps 5] [B ...]        (default: 1 64 1024)
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from ac_time import HOST_FREQS, HOST_POINTS, kernel_times, linearised, med, timed   # noqa: E402  (puts the repository root on sys.path)
from cadnip_jl_amd import api, hip   # noqa: E402
from cadnip_jl_amd.opinfo import _index   # noqa: E402


def run(B, circuit, memory, reps, gmin=1e-12):
    freqs = api.acdec(10, 1e3, 1e9)
    sim, circ, pts, u, _ = linearised(circuit, B)
    try:
        st, h = sim.st, sim.h
        G, C, _, _ = h.get_GCb()
        import scipy.sparse as sp
        dense = lambda nz: sp.csc_matrix((nz, st.ref_rowval, st.ref_colptr), shape=(st.n, st.n)).toarray()
        big = circuit != "dff"
        output = "n200" if big else "Q_neg"
        info = {d["name"]: d for d in st.opinfo}
        srcs = []
        for d in circ.devices:
            if d.type == "MOS1":
                gl = [_index(st, t) for t in info[d.name]["nodes"]]
                srcs.append((gl[0], gl[2], "white", 1e-24, 0.0, d.name.lower()))
        n_host = min(B, 1 if big else HOST_POINTS)
        Gd, Cd = [None] * B, [None] * B                   # host matrices of the timed points only: the GPU path needs them for redone rows alone
        for k in range(n_host):
            Gd[k], Cd[k] = dense(G[k]), dense(C[k])
            Gd[k][np.arange(st.n_nodes), np.arange(st.n_nodes)] += gmin
        temps = [p.get("temp", 27.0) for p in pts]
        last = {}

        def sweep():
            stats = {"gpu_systems": 0, "host_systems": 0, "max_berr": 0.0, "wpb": 0}
            api.noise_solve_gpu(h, st, G, C, Gd, Cd, [srcs] * B, output, freqs, None, temps, gmin, "gpu", stats, memory=memory)
            last.update(stats)
        sweep()                                                                                # warm-up: allocation, code load
        t_call = timed(sweep, reps)
        used = last["memory"]
        pairs, _ = api.noise_probe_pairs([srcs])
        e_out = np.zeros(st.n, dtype=complex)
        e_out[st.index_of(output)] = 1.0
        adjoint = lambda: h.ac_adjoint(2.0 * np.pi * freqs, gmin, e_out, pairs)
        h.ac_set_memory(memory)
        t_kernel = kernel_times(h, adjoint, "ac_adj_hbm" if used == "hbm" else "ac_adj", reps)
        plan = h.ac_plan_info()
        t_lds = None
        h.ac_set_memory("lds")
        if used == "hbm":
            try:
                adjoint()
                t_lds = kernel_times(h, adjoint, "ac_adj", reps)
            except hip.CadnipError:
                pass                                                                           # beyond LDS: nothing to compare with
        hf = freqs[:HOST_FREQS] if big else freqs
        t_host = np.asarray(timed(lambda: [api.noise_solve(st, Gd[k], Cd[k], srcs, output, hf, None, temps[k]) for k in range(n_host)],
                                  1 if big else reps)) * B / n_host * len(freqs) / len(hf)
        S = B * len(freqs)
        print("%s B %5d  systems %6d  pairs %d  memory %s  W %d  waves %d  workspace %.1f MiB\n    kernel %s (%.3f us/system)%s\n    gpu sweep %s\n    host %s%s  host/gpu %.1f  max berr %.2g  host rows %d" % (
            circuit, B, S, len(pairs), used, last["wpb"], plan["n_waves"], plan["work_bytes"] / 2 ** 20, med(t_kernel), np.median(t_kernel) * 1e6 / S,
            "" if t_lds is None else "\n    kernel in LDS %s  hbm/lds %.2f" % (med(t_lds), np.median(t_kernel) / np.median(t_lds)),
            med(t_call), med(t_host), " (scaled from %d point(s) x %d frequencies)" % (n_host, len(hf)) if n_host < B or big else "",
            np.median(t_host) / np.median(t_call), last["max_berr"], last["host_systems"]), flush=True)
    finally:
        sim.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--circuit", choices=["dff", "chain200"], default="dff")
    ap.add_argument("--memory", choices=["lds", "hbm", "auto"], default="lds")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("B", type=int, nargs="*")
    a = ap.parse_args()
    for B in a.B or [1, 64, 1024]:
        run(B, a.circuit, a.memory, max(1, a.reps))
