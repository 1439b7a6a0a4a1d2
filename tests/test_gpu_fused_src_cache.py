"""The sweep kernel's source segment cache (csrc/src_cache.hpp; a per-instance LDS region behind beta, lds_layout.hpp) changes WHERE the
value of a source is read, never the value: every case runs the DC solve and the fused transient twice in one process on fresh simulators
-- with the cache, and with CADNIP_F2_SRC_CACHE=0 (the path without it) -- and requires np.array_equal on the recorded outputs and on
the per-instance counters.  The plan line of CADNIP_F2_DEBUG=1 proves which path ran.  (The early request of the first sp_mos1 parameter
group, the second mechanism asked for with the cache, was measured and left out -- DESIGN.md section 9, round 5; CADNIP_F2_M1_EARLY=0 is
still set for the reference runs, so that they stay the reference should it return.)

Cases: the flip-flop (two PWL and five DC sources) and the benchmark's inverter at B = 9 (k_fused2<1>) under both Newton modes; the inverter at the batch sizes that reach workgroup widths 2, 4 and 8; the flip-flop at more instances than the device has resident
waves under CADNIP_F2_WPB=1, so that the queue hands a wave a second instance after it cached the first one's sources; the flip-flop
with every node observed and the save times on the PWL points themselves; a lean circuit with 70 DC voltage sources (more than the 64
pinned lanes); and one run held to the CPU port with the counts and the 1e-9 bound of tests/test_gpu_tran_parity.py, which guards against
both paths being wrong together."""
import re

import numpy as np
import pytest

from cadnip_jl_amd import api, benchmarks as bm
from cadnip_jl_amd.circuit import Circuit, Param
from cadnip_jl_amd.structure import expand_breakpoints
from tests.port_util import make_port, analyze_port
from tests.test_gpu_tran_parity import REL_TOL, ABSTOL

pytestmark = pytest.mark.gpu

OFF = {"CADNIP_F2_SRC_CACHE": "0", "CADNIP_F2_M1_EARLY": "0"}


def many_sources_circuit(stubs=0):
    """70 DC voltage sources (six beyond the pinned lanes) feeding one node through resistors; a PWL current source moves that node.
    `stubs` RC branches hang off it side by side: they add unknowns and table words, not dependency levels -- the test's means of sizing
    the workgroup's LDS block"""
    c = Circuit("70 dc sources on a summing node")
    for k in range(70):
        c.V("V%d" % k, "a%d" % k, "0", dc=Param("vdd", scale=0.01 * (k + 1)))
        c.R("R%d" % k, "a%d" % k, "s", 1e3 * (1 + k % 7))
    c.R("RS", "s", "0", 2e3)
    c.C("CS", "s", "0", 2e-12)
    for k in range(stubs):
        c.R("RL%d" % k, "s", "l%d" % k, 500.0 * (1 + k % 5))
        c.C("CL%d" % k, "l%d" % k, "0", 1e-13 * (1 + k % 3))
    c.I("IS", "0", "s", dc=0.0, wave=("pwl", [0.0, 1e-8, 2e-8, 6e-8], [0.0, 0.0, 1e-3, -1e-3]), scale=1.0)
    return c


CIRCUITS = {
    "dff": (bm.dff_circuit, bm.DFF_TSPAN),
    "inverter": (bm.inverter_circuit, (0.0, 4e-7)),
    "sources70": (many_sources_circuit, (0.0, 8e-8)),      # (takes the number of stubs)
}


def _points(B):
    rng = np.random.default_rng(B)
    return [{"vdd": float(v), "temp": float(t)} for v, t in zip(4.5 + rng.random(B), -40.0 + 165.0 * rng.random(B))]


def _once(name, B, newton_mode, capfd, save_t=None, all_nodes=True, stubs=None):
    """DC + fused transient on a fresh simulator; returns DC state, outputs, per-instance counters, plan lines and what a port run needs"""
    mk, tspan = CIRCUITS[name]
    circ = mk() if stubs is None else mk(stubs)
    sim = api.BatchSimulator(api.MNACircuit(circ, {"vdd": 5.0}), _points(B))
    try:
        st = sim.st
        sim.analyze()
        u0, conv, _ = sim.dc(abstol=1e-9, mode="tranop")
        assert np.all(conv)
        ts = np.linspace(tspan[0], tspan[1], 15) if save_t is None else np.asarray(save_t)
        obs = list(range(st.n_nodes)) if all_nodes else [st.index_of("Q")]
        atol = st.state_abstol(**ABSTOL)
        breaks = expand_breakpoints(st.breakpoints, tspan)
        sim.h.set_spec(mode="tran")
        capfd.readouterr()
        out, per, stats = sim.h.tran_run(tspan[0], tspan[1], atol, 1e-4, breaks=breaks, save_t=ts, obs=obs, fused=1, newton_mode=newton_mode)
        plan = [ln for ln in capfd.readouterr().err.splitlines() if ln.startswith("[cadnip f2] B ")]
        assert stats["n_failed"] == 0
        aux = dict(circ=circ, st=st, ts=ts, obs=obs, atol=atol, breaks=breaks, vscale=sim.vscale(), tspan=tspan)
        return np.array(u0), np.array(out), np.array(per), plan, aux
    finally:
        sim.close()


def _env(monkeypatch, wpb=8, **extra):
    monkeypatch.setenv("CADNIP_F2_TEAM", "0")            # one wave per instance at every batch size: the sweep kernel
    monkeypatch.setenv("CADNIP_F2_WPB", str(wpb))
    monkeypatch.setenv("CADNIP_F2_DEBUG", "1")
    for k in OFF:
        monkeypatch.delenv(k, raising=False)
    for k, v in extra.items():
        monkeypatch.setenv(k, v)


def _cache_words(plan):
    """doubles of the source cache per instance (0: the launch ran without it) by every launch's plan line: the same in all of them"""
    assert plan and all("variant 0" in ln for ln in plan), plan
    return _field(plan, "src-cache")


def _field(plan, key):
    got = {int(re.search(r"\b%s (\d+)" % key, ln).group(1)) for ln in plan}
    assert len(got) == 1, plan
    return got.pop()


def _on_off(name, B, newton_mode, monkeypatch, capfd, wpb=8, src_words=None, **kw):
    _env(monkeypatch, wpb)
    u0, out, per, plan, aux = _once(name, B, newton_mode, capfd, **kw)
    assert _cache_words(plan) == src_words, plan
    _env(monkeypatch, wpb, **OFF)
    u0_p, out_p, per_p, plan_p, _ = _once(name, B, newton_mode, capfd, **kw)
    assert _cache_words(plan_p) == 0, plan_p
    assert _field(plan, "wpb") == _field(plan_p, "wpb") and _field(plan, "grid") == _field(plan_p, "grid")    # the cache cost no resident instance
    assert np.array_equal(u0, u0_p)
    assert np.array_equal(out, out_p) and np.array_equal(per, per_p)
    assert np.all(np.isfinite(out)) and np.ptp(out) > 0.1
    return out, per, plan, aux, u0


@pytest.mark.parametrize("newton_mode", [0, 1])
@pytest.mark.parametrize("name,src_words", [("dff", 36), ("inverter", 10)])
def test_one_instance_per_workgroup(name, src_words, newton_mode, monkeypatch, capfd):
    """B = 9: k_fused2<1>; the flip-flop caches seven sources (5 x 7 doubles, rounded up to 36), the inverter two"""
    out, per, plan, _, _ = _on_off(name, 9, newton_mode, monkeypatch, capfd, src_words=src_words)
    assert _field(plan, "wpb") == 1


def test_the_switch_alone(monkeypatch, capfd):
    """CADNIP_F2_SRC_CACHE=0 by itself restores the path without the cache"""
    _env(monkeypatch)
    u0, out, per, plan, _ = _once("dff", 9, 1, capfd)
    assert _cache_words(plan) == 36
    _env(monkeypatch, CADNIP_F2_SRC_CACHE="0")
    u0_s, out_s, per_s, plan_s, _ = _once("dff", 9, 1, capfd)
    assert _cache_words(plan_s) == 0, plan_s
    assert np.array_equal(u0, u0_s) and np.array_equal(out, out_s) and np.array_equal(per, per_s)


@pytest.mark.parametrize("wpb,B", [(2, 300), (4, 700), (8, 1100)])
def test_inverter_at_every_workgroup_width(wpb, B, monkeypatch, capfd):
    """the batch sizes of tests/test_gpu_fused_steps.py that keep widths 2, 4 and 8 on a 256-CU device"""
    out, per, plan, _, _ = _on_off("inverter", B, 1, monkeypatch, capfd, wpb=wpb, src_words=10, all_nodes=False)
    assert _field(plan, "wpb") <= wpb


def test_a_wave_takes_a_second_instance_from_the_queue(monkeypatch, capfd):
    """More flip-flops than resident waves under CADNIP_F2_WPB=1 (three workgroups per CU by LDS): waves that finish their instance pick the
    next one from the queue and rebuild the cache for it; its corner -- and with it the PWL scale and every DC value -- is another one"""
    import torch
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    B = max(800, 3 * n_cu + 32)
    out, per, plan, _, _ = _on_off("dff", B, 1, monkeypatch, capfd, wpb=1, src_words=36, all_nodes=False)
    assert _field(plan, "wpb") == 1 and _field(plan, "grid") < B, plan


def test_save_times_on_the_pwl_points(monkeypatch, capfd):
    """every node observed, the save times the PWL points of both stimuli: the accepted steps land on them to the bit"""
    ts = sorted(set(bm.CLKN_PWL[0]) | set(bm.D_PWL[0]))
    out, per, plan, _, _ = _on_off("dff", 9, 1, monkeypatch, capfd, src_words=36, save_t=ts)
    assert out.shape[1] == len(ts)


def _rule_admits(plan, src_words):
    """fused2_plan's rule on the numbers of a plan line of a launch WITHOUT the cache: the region may cost neither the launch (LDS budget)
    nor a resident workgroup per CU (by LDS, at most 32 waves)"""
    budget, shmem, wpb = 160 * 1024, _field(plan, "shmem"), _field(plan, "wpb")
    with_cache = shmem + wpb * 8 * src_words
    return with_cache <= budget and min(budget // with_cache, 32 // wpb) == min(budget // shmem, 32 // wpb)


def test_more_sources_than_pinned_lanes(monkeypatch, capfd):
    """70 DC voltage sources: 64 are pinned and cached (5 x 64 doubles), six take the block loop's own path as before; the current source is
    a block of its own.  2.5 KB per instance is what the rule can refuse: the bare circuit fits nine workgroups per CU without the region and
    eight with it, so its launch must stay without; RC stubs size the block until the region rides in the slack of the last workgroup (which
    count does depends on the core size the host picks, so the first admitted of a few is taken), and that launch must have it"""
    admitted = None
    for stubs in (0, 72, 84, 88, 96, 104):
        _env(monkeypatch, **OFF)
        ref = _once("sources70", 9, 1, capfd, stubs=stubs)
        assert _cache_words(ref[3]) == 0
        if stubs == 0 or _rule_admits(ref[3], 320):
            _env(monkeypatch)
            u0, out, per, plan, _ = _once("sources70", 9, 1, capfd, stubs=stubs)
            assert _cache_words(plan) == (320 if _rule_admits(ref[3], 320) else 0), (ref[3], plan)
            assert _field(plan, "grid") == _field(ref[3], "grid") and _field(plan, "wpb") == _field(ref[3], "wpb")
            assert np.array_equal(u0, ref[0]) and np.array_equal(out, ref[1]) and np.array_equal(per, ref[2])
            assert np.all(np.isfinite(out)) and np.ptp(out) > 0.1
            if _cache_words(plan):
                admitted = stubs
                break
    assert admitted is not None, "no circuit size let the cache in"


def test_cached_path_matches_the_port(monkeypatch, capfd):
    """the flip-flop at B = 9 against the CPU port: the same Newton, accepted and rejected counts, every recorded node within 1e-9"""
    _env(monkeypatch)
    B = 9
    u0, out, per, plan, aux = _once("dff", B, 1, capfd)
    assert _cache_words(plan) == 36
    pts = _points(B)
    for i in range(B):
        pst, port = make_port(aux["circ"], {"vdd": pts[i]["vdd"]}, pts[i]["temp"], "tran")
        analyze_port(pst, port, aux["vscale"])
        ref, _, rst, _ = port.tran(u0[i], aux["tspan"][0], aux["tspan"][1], aux["atol"], 1e-4, breaks=aux["breaks"], save_t=aux["ts"], obs=aux["obs"],
                                   err_mask=pst.differential_mask(), use_pcnr=False, newton_mode=1)
        port.close()
        assert rst["status"] == 1
        err = np.max(np.abs(out[i] - ref) / np.maximum(np.abs(ref), 1.0))
        print("instance", i, "gpu", per[i, :3].tolist(), "port", (rst["newton_iters"], rst["accepted"], rst["rejected"]), "err", err)
        assert (per[i, 0], per[i, 1], per[i, 2]) == (rst["newton_iters"], rst["accepted"], rst["rejected"]), (pts[i], per[i], rst)
        assert err <= REL_TOL, (pts[i], err)
