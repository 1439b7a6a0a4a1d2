"""bench.py's output contract, run in-process (the library and torch share one HIP runtime in either load order:
hip.py _share_hip_runtime, tests/test_gpu_coexist.py -- this module no longer has to run first)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
def test_bench_line_contract(capsys):
    """bench.py --full in-process on a small sweep: ONE JSON line with the contract fields, the roofline object of the dominant
    kernel (live HIP-event timing) and the CPU baseline of the oracle's port."""
    import json
    import torch
    assert torch.cuda.is_available()
    import bench
    bench.main(["--full", "--steps", "1", "--warmup", "0", "--instances", "64", "--cpu-sample", "32", "--total-instances", "64"])
    lines = [l for l in capsys.readouterr().out.splitlines() if l.strip()]
    assert len(lines) == 1
    d = json.loads(lines[0])
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert key in d, key
    assert d["metric"] == "newton_iters_per_sec" and d["unit"] == "newton_iters/s" and d["n_gpus"] == 1 and d["steps"] == 1 and d["warmup"] == 0
    assert d["higher_is_better"] is True and d["scaling"] == "weak" and d["vs_baseline"] is None and d["dtype"] == "f64" and d["data"] == "synthetic"
    assert "workload" in d["config"] and d["config"]["instances_per_gpu"] == 64 and d["value"] > 1e6
    r = d["roofline"]
    # the fused kernel is bound by vector-instruction issue, not by HBM: frac is a utilisation, so it lies in (0, 1]
    assert r["bound"] == "valu_issue" and r["avg_launch_us"] > 0 and r["source"]
    assert r["frac"] is not None and 0.0 < r["frac"] <= 1.0 and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-3
    if "hbm" in r:
        assert r["hbm"]["bound"] == "hbm" and r["hbm"]["peak"] == 8000.0 and 0.0 < r["hbm"]["frac"] <= 1.0
    s = d["stamp_kernel"]
    # frac: the counter figure when a counter pass ran (HBM bytes moved / duration / peak), SURVEY 8d's algorithmic figure beside it
    assert s["bound"] == "hbm" and s["B"] == 8192 and 0.0 < s["frac"] <= 1.0 and abs(s["frac_algorithmic"] - s["achieved_GBps"] / 8000.0) < 1e-3
    assert abs(s["frac"] - (s["traffic_GBps"] if s.get("traffic") else s["achieved_GBps"]) / 8000.0) < 1e-3 and s["frac_source"]
    assert d["transients_per_s"] > 0 and 0.0 <= d["rejected_step_share"] < 0.5 and d["newton_iters_per_accepted_step"] > 1.0
    assert d["single_instance_one_wave_us_per_iter"] > d["single_instance_us_per_iter"]       # the team kernel is what a single transient gets
    assert d["strong_1024"]["instances_total"] == 64 and d["strong_1024"]["value"] > 0
    assert d["single_instance_us_per_iter"] > 0 and d["callback_us_per_iter"] > 0
    assert d["config"]["newton_mode"] == 1 and d["full_newton"]["newton_iters_per_step"] > d["config"]["newton_iters_per_step"]
    p = d["psp103_ring"]
    assert "error" not in p and p["B1"]["failed"] == 0 and p["B256"]["failed"] == 0 and p["B256"]["us_per_instance_iter"] < p["B1"]["us_per_instance_iter"] < 1376.0
    c = d["cpu_baseline"]
    assert c["kind"] == "port" and c["cores"] >= 1 and c["value"] > 0 and c["unit"] == d["unit"] and "sample" in c



def test_bench_plain_run_and_dumped_outputs(capsys, tmp_path):
    """A plain run: ONE JSON line with the headline fields and nothing that needs runs of its own; --steps sets the timed steps;
    --dump-outputs writes the last timed step's arrays, the same in two runs with the same arguments."""
    import json
    import torch
    assert torch.cuda.is_available()
    import bench
    dumps = []
    for k in range(2):
        d = tmp_path / ("run%d" % k)
        bench.main(["--steps", "2", "--warmup", "1", "--instances", "64", "--dump-outputs", str(d)])
        lines = [l for l in capsys.readouterr().out.splitlines() if l.strip()]
        assert len(lines) == 1
        r = json.loads(lines[0])
        assert r["metric"] == "newton_iters_per_sec" and r["unit"] == "newton_iters/s" and r["higher_is_better"] is True and r["dtype"] == "f64"
        assert r["steps"] == 2 and r["warmup"] == 1 and r["ms_per_step"] > 0 and r["value"] > 1e6
        assert abs(r["value"] - r["config"]["newton_iters_per_step"] / (r["ms_per_step"] * 1e-3)) <= 1e-2 * r["value"]
        for key in ("strong_1024", "roofline", "cpu_baseline", "full_newton", "stamp_kernel", "psp103_ring"):
            assert key not in r, key
        dumps.append({f.stem: np.load(f) for f in sorted(d.glob("*.npy"))})
    a, b = dumps
    assert sorted(a) == ["dc_u0", "tran_out", "tran_per_instance"]
    assert a["tran_out"].shape == (64, 71, 1) and a["dc_u0"].shape[0] == 64 and a["tran_per_instance"].shape == (64, 4)
    for k in a:
        assert a[k].dtype == np.float64 and np.all(np.isfinite(a[k])) and np.array_equal(a[k], b[k]), k
