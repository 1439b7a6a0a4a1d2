"""GPU: the host paths of a sweep step that skip work no result needs -- cadnip_dc_run's zero start made on the device
(CADNIP_DC_COLD_ZERO) and cadnip_tran_run's option arrays, uploaded only where they differ from what the device holds.  Skipping must
not show: every result here is compared bit for bit with the same call done the long way -- an upload of explicit zeros, a fresh handle.
The flip-flop of the benchmark at B = 3 and B = 9 (nine is more than one 8-wave workgroup of the sweep kernel, so its queue pick-up
runs), and DC problems whose first Newton run leaves someone unsolved, so that the fallback stages start from the zero start too."""
import ctypes as C

import numpy as np
import pytest

from cadnip_jl_amd import api, benchmarks as bm, hip
from cadnip_jl_amd.structure import expand_breakpoints
from tests.test_gpu_dc_fallbacks import CASES, _rectifier_sweep

pytestmark = pytest.mark.gpu


def _dff(B):
    pts = list(bm.corner_grid(3, B // 3))
    assert len(pts) == B
    return api.BatchSimulator(api.MNACircuit(bm.dff_circuit(), {"vdd": 5.0}), pts)


def _rectifiers():
    """six rectifier points, 10 iterations: three solved by stage 0, two by stage 1, one on the gshunt ladder (tests/test_gpu_dc_fallbacks.py)"""
    pts = [{"vin": v} for v in (5.0, 0.8, 500.0, 0.7, 3.0, 0.5)]
    return api.BatchSimulator(api.MNACircuit(_rectifier_sweep(True), {"vin": 1.0}, api.MNASpec(mode="dcop")), pts)


def _case(name):
    return lambda: api.BatchSimulator(api.MNACircuit(CASES[name][0](), {}, api.MNASpec(mode="dcop")), None)


DC = {
    "dff3": (lambda: _dff(3), "tranop", dict(abstol=1e-9), {0}),
    "dff9": (lambda: _dff(9), "tranop", dict(abstol=1e-9), {0}),
    "rectifiers": (_rectifiers, "dcop", dict(maxiters=10), {0, 1, 2}),
    "rect_5_iterations": (_case("rect_5_iterations"), "dcop", CASES["rect_5_iterations"][1], {0, 1, 2, 3}),
}


def _no_wall(stats):
    return {k: v for k, v in stats.items() if k != "wall_seconds"}


def _dc_twice(make, mode, start, **kw):
    """dc_run on a fresh, unanalysed handle (the run takes its own pattern sample first) and once more on the analysed one"""
    sim = make()
    try:
        sim.h.set_spec(mode=mode)
        res = []
        for _ in range(2):
            u, conv, stats = sim.h.dc_run(start(sim), **kw)
            res.append((u, conv, _no_wall(stats), sim.h.dc_log()))
        return res
    finally:
        sim.close()


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("name", list(DC))
def test_zero_start_made_on_the_device_equals_uploaded_zeros(name, fused):
    make, mode, kw, stages = DC[name]
    dev = _dc_twice(make, mode, lambda sim: None, fused=fused, **kw)
    up = _dc_twice(make, mode, lambda sim: np.zeros((sim.B, sim.st.n)), fused=fused, **kw)
    assert {e[1] for e in up[0][3]} == stages
    for (u, conv, stats, log), (u_ref, conv_ref, stats_ref, log_ref) in zip(dev, up):
        assert log == log_ref and stats == stats_ref and np.array_equal(conv, conv_ref)
        assert np.array_equal(u, u_ref, equal_nan=True)


def _raw_dc(h, u, cold_start, mask, fused, **kw):
    """cadnip_dc_run with the given cold_start value as it is (Handle.dc_run passes 2 only without a mask)"""
    conv = np.zeros(h.B, dtype=np.int32)
    st = hip.RunStatsC()
    pm = np.ascontiguousarray(np.asarray(mask, dtype=np.int32))
    o = hip.DCOptsC(kw.get("abstol", 1e-10), kw.get("maxiters", 100), 1, cold_start, 1, int(fused), pm.ctypes.data_as(C.POINTER(C.c_int32)))
    rc = h.lib.cadnip_dc_run(h.h, C.byref(o), u.ctypes.data_as(C.POINTER(C.c_double)), conv.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(st))
    assert rc in (hip.OK, hip.NOCONV)
    return u, conv, _no_wall(hip._stats(st)), h.dc_log()


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("name", ["dff9", "rectifiers"])
def test_with_a_mask_the_zero_start_reads_u_and_leaves_masked_rows_alone(name, fused):
    make, mode, kw, _ = DC[name]
    res = []
    for cold_start in (hip.DC_COLD_ZERO, 1):
        sim = make()
        try:
            sim.h.set_spec(mode=mode)
            mask = np.arange(sim.B) % 3 != 1
            u0 = np.zeros((sim.B, sim.st.n))
            u0[~mask] = 0.25 + np.arange(sim.st.n) * 1e-3                     # theirs to keep
            res.append(_raw_dc(sim.h, u0.copy(), cold_start, mask, fused, **kw))
            # and through Handle.dc_run, which leaves the start to the caller's array as soon as there is a mask
            u, conv, stats = sim.h.dc_run(None, participate=mask, fused=fused, **kw)
            assert not np.any(u[~mask]) and not np.any(conv[~mask])
            assert np.array_equal(u[mask], res[-1][0][mask]) and np.array_equal(conv[mask], res[-1][1][mask].astype(bool))
        finally:
            sim.close()
    (u, conv, stats, log), (u_ref, conv_ref, stats_ref, log_ref) = res
    assert log == log_ref and stats == stats_ref and np.array_equal(conv, conv_ref) and np.array_equal(u, u_ref)
    assert np.array_equal(u[~mask], u0[~mask]) and not np.any(conv[~mask]) and np.all(conv[mask])


# ---- transient: the option arrays ------------------------------------------------------------------------------------------------
T1 = 4.8e-7          # past the clock edge at which the flip-flop's Q rises


class Tran:
    """The flip-flop batch with its operating point, and transient runs from it on this handle (`run`) or on a fresh one (`fresh`)."""

    def __init__(self, B):
        self.B = B
        self.sim = self._make()
        self.u0, conv, _ = self.sim.dc(abstol=1e-9, mode="tranop", fused=True)
        assert np.all(conv)
        st = self.sim.st
        self.base = dict(abstol=st.state_abstol(vntol=1e-6, iabstol=1e-9, chgtol=1e-6), breaks=np.asarray(expand_breakpoints(st.breakpoints, (0.0, T1)), dtype=float),
                         save_t=np.linspace(0.0, T1, 12), obs=[st.index_of("Q")], err_mask="differential")
        assert len(self.base["breaks"]) >= 3
        self._fresh = {}

    def _make(self):
        sim = _dff(self.B)
        sim.analyze()
        return sim

    def run(self, sim=None, fused=2, **changed):
        sim = sim or self.sim
        o = dict(self.base, **changed)
        sim.h.set_u(self.u0)
        sim.h.set_spec(mode="tran")
        out, per, stats = sim.h.tran_run(0.0, T1, o["abstol"], 1e-4, breaks=o["breaks"], save_t=o["save_t"], obs=o["obs"], err_mask=o["err_mask"],
                                         fused=fused, newton_mode=1 if fused else 0)
        assert stats["n_failed"] == 0
        return out, per, _no_wall(stats)

    def fresh(self, key, fused=2, **changed):
        """the same run as the first run of a new handle (made once per distinct option set)"""
        if (key, fused) not in self._fresh:
            sim = self._make()
            try:
                self._fresh[key, fused] = self.run(sim, fused, **changed)
            finally:
                sim.close()
        return self._fresh[key, fused]


@pytest.fixture(scope="module", params=[3, 9])
def tran(request):
    t = Tran(request.param)
    yield t
    t.sim.close()


def _same(got, ref):
    return np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]) and got[2] == ref[2]


@pytest.mark.parametrize("fused", [2, 0])
def test_a_run_repeated_with_the_same_options_equals_a_fresh_handles(tran, fused):
    ref = tran.fresh("base", fused)
    assert np.all(ref[1][:, 1] > 10) and np.ptp(ref[0]) > 1.0                 # steps were taken and Q moved
    for _ in range(3):
        assert _same(tran.run(fused=fused), ref)


def test_every_changed_option_array_reaches_the_device(tran):
    """One option array at a time, on one handle, each run against a fresh handle's with the same options -- a stale device array, or a
    host copy kept across a reallocation, would show as the previous run's result."""
    st, b = tran.sim.st, tran.base
    mid = 0.5 * (b["breaks"][:-1] + b["breaks"][1:])
    more_breaks = np.sort(np.concatenate([b["breaks"], mid]))
    n_all = st.n
    walk = [
        ("base", {}),
        ("abstol", dict(abstol=b["abstol"] * 4.0)),                           # same length, other bytes
        ("base", {}),
        ("err_mask", dict(err_mask="all")),
        ("breaks_longer", dict(breaks=more_breaks)),                          # grows: reallocated
        ("breaks_shorter", dict(breaks=b["breaks"][:-1])),                    # fits: a prefix of what was held two runs ago
        ("base", {}),
        ("save_longer", dict(save_t=np.linspace(0.0, T1, 30))),
        ("save_shorter", dict(save_t=np.linspace(0.0, T1, 7))),
        ("obs_other", dict(obs=[st.index_of("D")])),
        ("obs_longer", dict(obs=[st.index_of("Q"), st.index_of("D"), 0])),
        ("obs_all", dict(obs=None)),                                          # n_obs = 0: every unknown, the driver's own index list
        ("obs_other", dict(obs=[st.index_of("D")])),
        ("base", {}),
    ]
    assert n_all > 3
    seen = {}
    for key, changed in walk:
        got = tran.run(**changed)
        assert _same(got, tran.fresh(key, **changed)), key
        seen[key] = got
    # the changes are not no-ops: they change what a run returns (else a stale array could not show)
    assert seen["abstol"][2] != seen["base"][2] and seen["err_mask"][2] != seen["base"][2] and seen["breaks_longer"][2] != seen["base"][2]
    assert not np.array_equal(seen["obs_other"][0], seen["base"][0]) and seen["save_longer"][0].shape != seen["base"][0].shape
