"""AC sweep, B points x the 61-point grid (acdec(10, 1e3, 1e9)): the GPU path of api.ac -- the kernel alone (HIP events on the handle's stream,
cadnip_profile_*), the whole sweep (pivot analysis, transfers, kernel, merge) -- against the host path's dense solves, on the same machine in
the same run.  After one warm-up every figure is the median of --reps timed repetitions, printed with min..max.
  --circuit dff       the flip-flop at B corners (supply, temperature), linearised at its DC points
  --circuit chain200  the 200-stage inverter chain (tests/circuits.py) at B supplies, linearised at the zero state (its DC solve needs the
                      fallback ladder; the sweep does not care): 208 KB of work arrays, beyond the LDS kernels
  --memory lds|hbm|auto   where the kernel keeps a system's work arrays (hip.Handle.ac_set_memory).  With hbm / auto on a circuit that fits
                      LDS the LDS kernel is timed as well, in the same run: the price of leaving LDS.
  --overlay N         instead of the above: what an N-entry overlay (hip.Handle.ac_set_overlay: the delayed elements' addend) costs k_ac_lu
                      on the flip-flop at B = 64 x the 61 frequencies.  The baseline is the kernel without overlay -- the parent's, instruction
                      for instruction -- in the same process; the two are timed in ALTERNATING repetitions (plain, overlay, plain, ...)
                      so drift hits both alike.  The table is all zeros at N positions spread evenly over the pattern: the kernel's
                      work does not depend on the values, and the results must equal the plain kernel's.
The host is timed on at most HOST_POINTS points (chain200: one point, HOST_FREQS frequencies -- a dense solve of n = 2204 takes a second) and
scaled to the grid (its cost per system does not depend on B); the line says so.

usage:  timeout -k 10 600 python tools/ac_time.py [--circuit dff] [--memory lds] [--reps 5] [B ...]        (default: 1 64 1024)
        timeout -k 10 600 python tools/ac_time.py --overlay 8 [--memory lds] [--reps 5]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cadnip_jl_amd import api, benchmarks as bm, hip   # noqa: E402

HOST_POINTS = 4
HOST_FREQS = 4


def med(v):
    """'median (min..max)' of a list of seconds, in milliseconds"""
    v = np.asarray(v) * 1e3
    return "%9.3f (%.3f..%.3f) ms" % (np.median(v), v.min(), v.max())


def timed(fn, reps):
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append(time.perf_counter() - t0)
    return out


def linearised(circuit, B):
    """(sim, circ, point parameters, u [B, n], b_ac [n]) with the handle holding the restamp at u"""
    if circuit == "dff":
        circ = bm.dff_circuit()
        next(d for d in circ.devices if d.type == "V" and d.name.lower() == "vd").params["ac"] = 1.0
        pts = [{"vdd": 4.5 + (i * 0.6180339887) % 1.0, "temp": -40.0 + 165.0 * ((i * 0.3819660113 + 0.17) % 1.0)} for i in range(B)]
        sim = api.BatchSimulator(api.MNACircuit(circ, {"vdd": 5.0}, api.MNASpec(mode="dcop")), pts)
        u, conv, _ = sim.dc()
        assert np.all(conv), "DC failed for %d corner(s)" % int((~conv).sum())
        b_ac = api.rhs_ac(sim.st, circ, {"vdd": pts[0]["vdd"]})
    else:
        from tests import circuits as tc
        mk, params = tc.CHAIN_STAMP[circuit]
        circ = mk()
        pts = [{"vdd": 1.0 + 4.0 * ((i * 0.6180339887) % 1.0)} for i in range(B)]
        sim = api.BatchSimulator(api.MNACircuit(circ, dict(params), api.MNASpec(mode="dcop")), pts)
        sim.analyze()
        sim.h.set_spec(mode="dcop")
        u = np.zeros((B, sim.st.n))
        b_ac = np.zeros(sim.st.n, complex)
        b_ac[sim.st.index_of("I_vin")] = 1.0
    sim.h.rebuild(u, 0.0)
    return sim, circ, pts, u, b_ac


def kernel_times(h, call, name, reps):
    """seconds of kernel `name` in each of `reps` calls (HIP events around the launch)"""
    out = []
    h.profile(True)
    for _ in range(reps):
        before = h.profile_read().get(name, (0.0, 0))[0]
        call()
        out.append((h.profile_read()[name][0] - before) * 1e-3)
    h.profile(False)
    return out


def run(B, circuit, memory, reps, gmin=1e-12):
    freqs = api.acdec(10, 1e3, 1e9)
    omegas = 2.0 * np.pi * freqs
    sim, circ, pts, u, b_ac1 = linearised(circuit, B)
    try:
        st, h = sim.st, sim.h
        G, C, _, _ = h.get_GCb()
        import scipy.sparse as sp
        dense = lambda nz: sp.csc_matrix((nz, st.ref_rowval, st.ref_colptr), shape=(st.n, st.n)).toarray()
        big = circuit != "dff"
        sols = []
        for k in range(min(B, 1 if big else HOST_POINTS)):
            Gd = dense(G[k])
            Gd[np.arange(st.n_nodes), np.arange(st.n_nodes)] += gmin
            sols.append(api.ACSol(st, Gd, dense(C[k]), b_ac1, u[k], freqs))
        b_ac = np.tile(b_ac1, (B, 1))
        shells = [api.ACSol(st, None, None, b_ac[k], None, freqs) for k in range(B)]          # cache targets of the sweep (no host matrices)
        last = {}

        def sweep():
            stats = {"gpu_systems": 0, "host_systems": 0, "max_berr": 0.0, "wpb": 0}
            api.ac_gpu_sweep(h, st, shells, G, C, omegas, gmin, "gpu", stats, memory=memory)
            last.update(stats)
        sweep()                                                                                # warm-up: allocation, code load
        t_call = timed(sweep, reps)
        used = last["memory"]
        h.ac_set_memory(memory)
        t_kernel = kernel_times(h, lambda: h.ac_solve(omegas, gmin, b_ac), "ac_lu_hbm" if used == "hbm" else "ac_lu", reps)
        plan = h.ac_plan_info()
        t_lds = None
        h.ac_set_memory("lds")
        if used == "hbm":
            try:
                h.ac_solve(omegas, gmin, b_ac)
                t_lds = kernel_times(h, lambda: h.ac_solve(omegas, gmin, b_ac), "ac_lu", reps)
            except hip.CadnipError:
                pass                                                                           # beyond LDS: nothing to compare with
        hw = omegas[:HOST_FREQS] if big else omegas
        host = lambda: [(s._cache.clear(), s._solve(hw)) for s in sols]                        # (an ACSol caches the rows of a grid)
        t_host = np.asarray(timed(host, 1 if big else reps)) * B / len(sols) * len(omegas) / len(hw)
        S = B * len(freqs)
        print("%s B %5d  systems %6d  memory %s  W %d  waves %d  workspace %.1f MiB\n    kernel %s (%.3f us/system)%s\n    gpu sweep %s\n    host %s%s  host/gpu %.1f  max berr %.2g  host rows %d" % (
            circuit, B, S, used, last["wpb"], plan["n_waves"], plan["work_bytes"] / 2 ** 20, med(t_kernel), np.median(t_kernel) * 1e6 / S,
            "" if t_lds is None else "\n    kernel in LDS %s  hbm/lds %.2f" % (med(t_lds), np.median(t_kernel) / np.median(t_lds)),
            med(t_call), med(t_host), " (scaled from %d point(s) x %d frequencies)" % (len(sols), len(hw)) if len(sols) < B or big else "",
            np.median(t_host) / np.median(t_call), last["max_berr"], last["host_systems"]), flush=True)
    finally:
        sim.close()


def run_overlay(n_ovl, memory, reps, B=64, gmin=1e-12):
    omegas = 2.0 * np.pi * api.acdec(10, 1e3, 1e9)
    sim, circ, pts, u, b_ac1 = linearised("dff", B)
    try:
        st, h = sim.st, sim.h
        G, C, _, _ = h.get_GCb()
        api.ac_analyze_pivots(h, st, G, C, omegas, gmin)
        h.ac_set_memory(memory)
        b_ac = np.tile(b_ac1, (B, 1))
        pos = np.unique(np.linspace(0, st.nnz - 1, n_ovl).round().astype(np.int32))
        val = np.zeros((B, omegas.size, pos.size), dtype=complex)
        x0, berr0, _, _ = h.ac_solve(omegas, gmin, b_ac)                                       # warm-up of both kernels; the results must agree
        name = "ac_lu_hbm" if h.ac_plan_info()["memory"] == "hbm" else "ac_lu"
        h.ac_set_overlay(pos, omegas, val)
        x1, berr1, _, _ = h.ac_solve(omegas, gmin, b_ac)
        assert np.array_equal(x0, x1) and np.array_equal(berr0, berr1), "an all-zero overlay changed the results"
        t_plain, t_ovl = [], []
        for _ in range(reps):
            h.ac_clear_overlay()
            t_plain += kernel_times(h, lambda: h.ac_solve(omegas, gmin, b_ac), name, 1)
            h.ac_set_overlay(pos, omegas, val)
            t_ovl += kernel_times(h, lambda: h.ac_solve(omegas, gmin, b_ac), name, 1)
        h.ac_clear_overlay()
        S = B * omegas.size
        print("dff B %d  systems %d  memory %s  overlay entries %d (table %.1f KiB)\n    kernel without overlay %s\n    kernel with overlay    %s\n"
              "    overlay / plain %.3f  (+%.3f us/system)" % (B, S, h.ac_plan_info()["memory"], pos.size, val.nbytes / 1024, med(t_plain), med(t_ovl),
                                                               np.median(t_ovl) / np.median(t_plain), (np.median(t_ovl) - np.median(t_plain)) * 1e6 / S), flush=True)
    finally:
        sim.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--circuit", choices=["dff", "chain200"], default="dff")
    ap.add_argument("--memory", choices=["lds", "hbm", "auto"], default="lds")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--overlay", type=int, default=0, metavar="N")
    ap.add_argument("B", type=int, nargs="*")
    a = ap.parse_args()
    if a.overlay > 0:
        run_overlay(a.overlay, a.memory, max(1, a.reps))
        sys.exit(0)
    for B in a.B or [1, 64, 1024]:
        run(B, a.circuit, a.memory, max(1, a.reps))
