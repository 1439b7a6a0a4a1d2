#!/usr/bin/env python
"""Times a transient with K forward sensitivities (api.tran(..., sens=), csrc/tran_sens.hip) against the same run without them and
against the (2 K + 1)-point sweep a caller would difference today.  The inverter benchmark circuit over ``--points`` supplies; the
parameters are vdd and the temperature (``--params`` 1 or 2).  All three runs use the per-op kernels (a run with ``sens`` always does), so
the figures compare like with like; ``--fused`` adds the plain run and the sweep on the fused kernel, which is what a caller gets by
default.  Prints one JSON line: wall seconds of the driver loop (device-synchronised) and of the whole call, launches, accepted steps.

    python tools/tran_sens_time.py --points 64 --params 2"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cadnip_jl_amd import api, benchmarks as bm  # noqa: E402


def run(mc, points, tspan, saveat, fused, reps, **kw):
    sim = api.BatchSimulator(mc, points)
    try:
        sim.analyze()
        best = None
        for _ in range(reps + 1):                       # the first run warms the handle up
            t = time.perf_counter()
            out, per, stats = sim.tran(tspan, api._resolve_abstol(1e-10, sim.st), 1e-6, saveat, fused=fused, **dict(kw))
            total = time.perf_counter() - t
            assert np.all(per[:, 3] == 1), per[:, 3]
            if best is None or stats["wall_seconds"] < best["loop_s"]:
                best = dict(loop_s=stats["wall_seconds"], call_s=total, launches=int(stats["launches"]), accepted=int(stats["steps_accepted"]),
                            instances=int(sim.B if "sens" not in kw else sim.B * (2 + 2 * len(kw["sens"]))))
        return best
    finally:
        sim.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=64)
    ap.add_argument("--params", type=int, default=2, choices=(1, 2))
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--t1", type=float, default=120e-9)
    ap.add_argument("--fused", action="store_true")
    a = ap.parse_args()
    mc = api.MNACircuit(bm.inverter_circuit(), {"vdd": 5.0})
    points = [{"vdd": float(v)} for v in np.linspace(4.5, 5.5, a.points)]
    names = ["vdd", "temp"][:a.params]
    tspan, saveat = (0.0, a.t1), np.linspace(0.0, a.t1, 101)
    _, _, expanded, _ = api.sens_expand(mc, points, names, 1e-4)
    res = dict(points=a.points, K=a.params,
               plain=run(mc, points, tspan, saveat, 0, a.reps),
               sens=run(mc, points, tspan, saveat, 0, a.reps, sens=names),
               sweep=run(mc, expanded, tspan, saveat, 0, a.reps))
    if a.fused:
        res["plain_fused"] = run(mc, points, tspan, saveat, 1, a.reps)
        res["sweep_fused"] = run(mc, expanded, tspan, saveat, 1, a.reps)
    res["sens_over_plain"] = res["sens"]["loop_s"] / res["plain"]["loop_s"]
    res["sens_over_sweep"] = res["sens"]["loop_s"] / res["sweep"]["loop_s"]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
