"""The cost of the two delay kernels per Newton round: the per-op transient of the delayed buffer (V -> R -> E(gain 2, delay tau) -> R -> C,
6 unknowns) with and without a delay spec on the same handle in the same run, at B = 1 and B = 4096 (or the sizes given).

Both runs take the same forced grid (``err_mask`` all zero, ``breaks=()``, h0 and hmax given: --steps accepted steps, the same Newton rounds
up to the odd extra iteration), so what differs is k_delay_apply after the restamp and k_delay_record after the controller in every round:
  plain     cadnip_tran_run with no spec (the E element acts at once)
  delayed   the same call after cadnip_tran_set_delay with the circuit's own terms (tau = 4 final steps)
Whole calls by the wall clock (the driver synchronises before it returns) over the launches the driver reports, and in a second, profiled
pass the two kernels alone by HIP events on the handle's stream (cadnip_profile_*: the events serialise the launches, so that pass gives
kernel times only).  After one warm-up of each, --reps rounds alternate the two and swap their order every round; every figure is the
median with min..max.

usage:  timeout -k 10 600 python tools/delay_time.py [--steps 2000] [--reps 5] [B ...]        (default B: 1 4096)
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import cadnip_jl_amd as cj      # noqa: E402
from cadnip_jl_amd import api   # noqa: E402
from tools.ac_time import med   # noqa: E402
from tools.network_time import prof_ms   # noqa: E402

TD = 2.0 ** -30


def buffer():
    c = cj.Circuit("delayed buffer")
    c.V("vin", "in", "0", dc=0.0, wave=("sin", 0.0, 1.0, 0.5 / TD, 0.0, 0.0, 0.0))
    c.R("r1", "in", "a", 1e3)
    c.E("e1", "b", "0", "a", "0", 2.0, delay=cj.Param("tau"))
    c.R("r2", "b", "out", 1e3)
    c.C("c1", "out", "0", TD / 1e3)
    return c


def run(B, steps, reps):
    hmax = TD / 16
    taus = 4 * hmax * (1.0 + 0.25 * np.arange(B) / max(B, 1))          # a sweep: every instance its own delay, all >= 4 steps
    sim = api.BatchSimulator(api.MNACircuit(buffer(), {"tau": 4 * hmax}), [{"tau": float(t)} for t in taus])
    try:
        h, n = sim.h, sim.st.n
        sim.analyze()
        h.set_spec(mode="tran")
        spec = sim.delay_spec()
        t1 = hmax * (steps - 6)                                          # six doubling steps from h0 = hmax / 64, then constant steps
        kw = dict(breaks=(), save_t=[t1], h0=hmax / 64, hmax=hmax, max_order=2, newton_tol=1.0, err_mask=np.zeros(n), fused=False)

        def call(delayed):
            h.set_u(np.zeros((B, n)))
            if delayed:
                h.tran_set_delay(**spec)
                sim.analyze_delayed(spec, 0.0)
            else:
                h.tran_clear_delay()
                h.analyze_values(sim.pivot_sample)
            t0 = time.perf_counter()
            out, per, stats = h.tran_run(0.0, t1, 1e-11, 1e-11, **kw)
            wall = time.perf_counter() - t0
            assert stats["n_failed"] == 0, stats
            return wall, stats["launches"], out

        names = ("plain", "delayed")
        for nm in names:
            call(nm == "delayed")                                        # warm-up: allocation, code load
        wall, rounds = {nm: [] for nm in names}, {}
        for r in range(reps):
            for nm in (names if r % 2 == 0 else names[::-1]):
                w, rounds[nm], _ = call(nm == "delayed")
                wall[nm].append(w)
        h.profile(True)
        k0 = prof_ms(h, ("delay_apply", "delay_record"))
        a0 = prof_ms(h, ("delay_apply",))
        call(True)
        k_all, k_apply = prof_ms(h, ("delay_apply", "delay_record")) - k0, prof_ms(h, ("delay_apply",)) - a0
        h.profile(False)
        per_round = {nm: np.median(wall[nm]) / rounds[nm] * 1e6 for nm in names}
        print("buffer B %d  n %d  steps %d  rounds: plain %d, delayed %d" % (B, n, steps, rounds["plain"], rounds["delayed"]))
        for nm in names:
            print("    %-8s call %s   %.2f us per round" % (nm, med(wall[nm]), per_round[nm]))
        print("    delayed - plain: %.2f us per round (%.1f%%)   plain call spread %.1f%%   kernels by events: k_delay_apply %.2f us, k_delay_record %.2f us per round" % (
            per_round["delayed"] - per_round["plain"], 100.0 * (per_round["delayed"] / per_round["plain"] - 1.0),
            100.0 * (max(wall["plain"]) - min(wall["plain"])) / np.median(wall["plain"]),
            k_apply / rounds["delayed"] * 1e3, (k_all - k_apply) / rounds["delayed"] * 1e3), flush=True)
    finally:
        sim.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("B", type=int, nargs="*", default=[1, 4096])
    a = ap.parse_args()
    for B in a.B:
        run(B, max(16, a.steps), max(1, a.reps))
