"""The HBM-resident AC kernels k_ac_lu_hbm / k_ac_adj_hbm (csrc/ac_lu.hip) behind cadnip_ac_set_memory: the work arrays of a system in a
per-wave workspace in device memory, persistent waves walking the systems of a launch (csrc/ac_hbm_plan.hpp).  Held against the LDS kernels
to the bit where both apply -- the handles, systems and probe pairs of tests/test_gpu_ac_lu.py and tests/test_gpu_ac_adjoint.py -- and
against the refined dense solves of tests/ac_ref.py on chain200 (tests/circuits.py), whose 208 KB of work arrays the LDS kernels refuse.

chain200's references were checked on the CPU port before the bounds below were written (zero state, the I_vin excitation / e_n200, supplies
1 V and 5 V, omega = 1e3, 1e6, 1e9): the refined solves are finite, two and four refinement steps agree to the bit, and
|A^-1|_inf |b - A x_ref|_inf (residual in long double) is 0 for the plain systems and 2.3e-2, 5.9e-6, 1.3e-7 for the adjoint ones against
bounds 16 cond_inf eps max|x_ref| of 2.5e-3, 5.3e-6, 5.3e-9 (plain) and 8.2e11, 3.7e6, 3.7 (adjoint): every system is inside, no frequency
was replaced.  At the zero state the two supplies give the same matrices; they are two instances all the same."""
import numpy as np
import pytest

import cadnip_jl_amd as cj
from cadnip_jl_amd import api, hip
from tests import ac_ref as R
from tests import circuits as tc
from tests import noise_ref as N
from tests import test_gpu_ac_adjoint as TA
from tests import test_gpu_ac_lu as T
from tests import test_gpu_noise_solver as TN

pytestmark = pytest.mark.gpu
EPS = R.EPS
GMIN = T.GMIN
same = TA.same
LDS_BUDGET = 160 * 1024


class memory:
    """``with memory(h, mode, max_waves)``: the setting for the block; the handles of T.case are shared with other modules, so it goes back"""

    def __init__(self, h, mode, max_waves=0):
        self.h, self.mode, self.max_waves = h, mode, max_waves

    def __enter__(self):
        self.h.ac_set_memory(self.mode, self.max_waves)

    def __exit__(self, *exc):
        self.h.ac_set_memory("lds")


@pytest.mark.parametrize("name", list(R.CASES))
def test_bit_identity_with_the_lds_kernels(name):
    a = TA.adj(name)
    c = a.c
    S, per = c.B * c.F, 16 * (c.h.lu_stats()["nnz_lu"] + 3 * c.st.n)
    x0, berr0, flags0, info0 = c.run()
    h0, ax0, aberr0, aflags0, ainfo0 = a.run()
    assert info0["lds_bytes"] > 0 and c.h.ac_plan_info() == dict(memory="lds", n_waves=0, work_bytes=0, lds_bytes=ainfo0["lds_bytes"])
    for max_waves in (0, 1, 3):
        n_waves = min(S, max_waves) if max_waves else S          # S < 256 compute units x 8 for every case
        assert S <= 2048 and (name != "dff" or (S == 21 and S % 3 == 0 and 21 % 4 and 21 % 8))
        with memory(c.h, "hbm", max_waves):
            for wpb in (0, 1, 2, 4, 8):                          # the flip-flop's W = 8 is no refusal here: wpb shapes the grid only
                x, berr, flags, info = c.run(wpb)
                assert info == dict(wpb=wpb or 4, lds_bytes=0, systems=S, workgroups=-(-n_waves // (wpb or 4)))
                assert c.h.ac_plan_info() == dict(memory="hbm", n_waves=n_waves, work_bytes=n_waves * per, lds_bytes=0)
                assert same(x, x0) and np.array_equal(berr, berr0) and np.array_equal(flags, flags0), (max_waves, wpb)
                h, ax, aberr, aflags, ainfo = a.run(wpb)
                assert ainfo == info and c.h.ac_plan_info()["n_waves"] == n_waves
                assert same(h, h0) and same(ax, ax0) and np.array_equal(aberr, aberr0) and np.array_equal(aflags, aflags0), (max_waves, wpb)
    x, berr, flags, info = c.run()                               # and back: the default again
    assert info == info0 and same(x, x0)


def test_nothing_leaks_between_the_systems_of_a_wave():
    """One workspace for all 21 flip-flop systems; the middle instance's seven run between the others'."""
    a = TA.adj("dff")
    c = a.c
    x, berr, flags, _ = c.run()
    h, ax, aberr, aflags, _ = a.run()
    bac = c.bac.copy()
    bac[1, c.st.n // 2] = np.nan
    rhs = np.tile(a.rhs, (a.B, 1))
    rhs[1, a.st.n // 2] = np.nan
    with memory(c.h, "hbm", 1):
        xn, berrn, flagsn, _ = c.run(bac=bac)
        hn, axn, aberrn, aflagsn, _ = a.run(rhs=rhs)
        assert c.h.ac_plan_info()["n_waves"] == 1
    for fl, pairs in ((flagsn, ((xn, x), (berrn, berr))), (aflagsn, ((axn, ax), (hn, h), (aberrn, aberr)))):
        assert np.all(fl[1] & 1) and not fl[0].any() and not fl[2].any()
        for b in (0, 2):
            for got, clean in pairs:
                assert same(got[b], clean[b])


def test_a_flagged_zero_pivot_leaves_nothing_to_the_next_system_of_its_wave():
    """The circuit of test_a_zero_pivot_is_flagged_and_the_call_returns: the omega = 0 system (an empty row: zero pivot, NaNs in every work
    array) runs first on the wave that then solves omega = 1e3."""
    circ = cj.Circuit("capacitor-only node")
    circ.V("v1", "a", "0", dc=0.0, ac=1.0)
    circ.R("r1", "a", "b", 1e3)
    circ.C("c1", "b", "c", 1e-9)
    circ.C("c2", "c", "0", 1e-9)
    sim = api.BatchSimulator(api.MNACircuit(circ, {}, api.MNASpec(mode="dcop")))
    try:
        st = sim.st
        sim.analyze()
        sim.h.set_spec(mode="dcop")
        sim.h.rebuild(np.zeros(st.n), 0.0)
        b_ac = api.rhs_ac(st, circ, {})
        rhs = np.zeros(st.n, complex)
        rhs[st.index_of("b")] = 1.0
        x0, berr0, flags0, _ = sim.h.ac_solve([0.0, 1e3], 0.0, b_ac)
        h0, ax0, aberr0, aflags0, _ = sim.h.ac_adjoint([0.0, 1e3], 0.0, rhs, TA.all_pairs(st.n), want_x=True)
        sim.h.ac_set_memory("hbm", 1)
        x, berr, flags, info = sim.h.ac_solve([0.0, 1e3], 0.0, b_ac)
        h, ax, aberr, aflags, _ = sim.h.ac_adjoint([0.0, 1e3], 0.0, rhs, TA.all_pairs(st.n), want_x=True)
        assert info["systems"] == 2 and info["workgroups"] == 1 and sim.h.ac_plan_info()["n_waves"] == 1
        for fl in (flags, aflags):
            assert fl[0, 0] & 1 and fl[0, 1] == 0
        assert np.array_equal(flags, flags0) and np.array_equal(aflags, aflags0)
        assert same(x[0, 1], x0[0, 1]) and berr[0, 1] == berr0[0, 1] and same(ax[0, 1], ax0[0, 1]) and same(h[0, 1], h0[0, 1]) and aberr[0, 1] == aberr0[0, 1]
        G, C, _, _ = sim.h.get_GCb()
        to_ref = np.asarray(st.to_ref_nz)
        A = R.system(st, G[0, to_ref], C[0, to_ref], 1e3, 0.0)
        xr, axr = R.refined_solve_c(A, b_ac), R.refined_solve_c(A.T, rhs)
        assert np.max(np.abs(x[0, 1] - xr)) <= 16 * R.cond_inf_c(A) * EPS * np.max(np.abs(xr))
        assert np.max(np.abs(ax[0, 1] - axr)) <= 16 * R.cond_inf_c(A.T) * EPS * np.max(np.abs(axr))
    finally:
        sim.close()


class Chain200:
    """chain200 as test_a_circuit_beyond_lds_is_refused sets it up -- zero state, I_vin excitation; e_n200 for the adjoint -- at two supplies,
    omega = 1e3, 1e6, 1e9, with the refined dense references of its systems (one set for instances whose matrices coincide)."""
    OM = np.array([1e3, 1e6, 1e9])

    def __init__(self):
        mk, params = tc.CHAIN_STAMP["chain200"]
        self.sim = api.BatchSimulator(api.MNACircuit(mk(), dict(params), api.MNASpec(mode="dcop")), [{"vdd": 1.0}, {"vdd": 5.0}])
        st = self.st = self.sim.st
        self.h, self.B = self.sim.h, self.sim.B
        self.sim.analyze()
        self.per = 16 * (self.h.lu_stats()["nnz_lu"] + 3 * st.n)
        assert self.per > LDS_BUDGET and self.B == 2
        self.h.set_spec(mode="dcop")
        self.h.rebuild(np.zeros((self.B, st.n)), 0.0)
        self.b_ac = np.zeros(st.n, complex)
        self.b_ac[st.index_of("I_vin")] = 1.0
        self.e_out = np.zeros(st.n, complex)
        self.e_out[st.index_of("n200")] = 1.0
        G, C, _, _ = self.h.get_GCb()
        to_ref = np.asarray(st.to_ref_nz)
        self.ref = {}
        for b in range(self.B):
            twin = next((k for k in range(b) if np.array_equal(G[k], G[b]) and np.array_equal(C[k], C[b])), None)
            for f, w in enumerate(self.OM):
                if twin is not None:
                    self.ref[b, f] = self.ref[twin, f]
                    continue
                A = R.system(st, G[b, to_ref], C[b, to_ref], w, GMIN)
                self.ref[b, f] = (R.refined_solve_c(A, self.b_ac), R.cond_inf_c(A), R.refined_solve_c(A.T, self.e_out), R.cond_inf_c(A.T))


@pytest.fixture(scope="module")
def chain200():
    c = Chain200()
    yield c
    c.sim.close()


@pytest.mark.parametrize("mode", ["hbm", "auto"])
def test_the_circuit_the_lds_kernels_refuse(chain200, mode):
    c = chain200
    c.h.ac_set_memory(mode)
    try:
        x, berr, flags, info = c.h.ac_solve(c.OM, GMIN, c.b_ac)
        plan = c.h.ac_plan_info()
        h, ax, aberr, aflags, ainfo = c.h.ac_adjoint(c.OM, GMIN, c.e_out, [(c.st.index_of("n200"), -1)], want_x=True)
        aplan = c.h.ac_plan_info()
    finally:
        c.h.ac_set_memory("lds")
    for p, i in ((plan, info), (aplan, ainfo)):
        assert p == dict(memory="hbm", n_waves=6, work_bytes=6 * c.per, lds_bytes=0) and p["work_bytes"] > LDS_BUDGET
        assert i == dict(wpb=4, lds_bytes=0, systems=6, workgroups=2)
    for (b, f), (xr, kappa, axr, akappa) in c.ref.items():
        assert np.all(np.isfinite(xr)) and np.all(np.isfinite(axr))
        err, aerr = np.max(np.abs(x[b, f] - xr)), np.max(np.abs(ax[b, f] - axr))
        print("chain200 %s b %d omega %.0e  plain: flag %d berr %.3g fwd %.3g bound %.3g   adjoint: flag %d berr %.3g fwd %.3g bound %.3g" % (
            mode, b, c.OM[f], flags[b, f], berr[b, f], err, 16 * kappa * EPS * np.max(np.abs(xr)),
            aflags[b, f], aberr[b, f], aerr, 16 * akappa * EPS * np.max(np.abs(axr))))
    assert not flags.any() and not aflags.any()
    assert np.all(berr <= api.AC_BERR_MAX) and np.all(aberr <= api.AC_BERR_MAX)
    for (b, f), (xr, kappa, axr, akappa) in c.ref.items():
        assert np.max(np.abs(x[b, f] - xr)) <= 16 * kappa * EPS * np.max(np.abs(xr)), (b, f)
        assert np.max(np.abs(ax[b, f] - axr)) <= 16 * akappa * EPS * np.max(np.abs(axr)), (b, f)
        assert same(h[b, f, 0], ax[b, f, c.st.index_of("n200")])


def test_auto_keeps_a_circuit_that_fits_in_lds():
    c = T.case("butterworth")
    x0, berr0, _, info0 = c.run()
    with memory(c.h, "auto"):
        x, berr, _, info = c.run()
        assert c.h.ac_plan_info() == dict(memory="lds", n_waves=0, work_bytes=0, lds_bytes=info0["lds_bytes"])
    assert info == info0 and same(x, x0) and np.array_equal(berr, berr0)


def test_the_setting_and_its_refusals(chain200):
    c = T.case("butterworth")
    h = c.h
    try:
        h.ac_set_memory("hbm", 2)
        for bad in (("dram", 0), (3, 0), (-1, 0), ("hbm", -1), ("lds", -5)):
            with pytest.raises(hip.CadnipError) as e:
                h.ac_set_memory(*bad)
            assert e.value.code == hip.BADARG
        c.run()                                                  # ... and the setting is the one before them
        assert h.ac_plan_info()["memory"] == "hbm" and h.ac_plan_info()["n_waves"] == 2
        for wpb in (3, 16, -1):
            with pytest.raises(hip.CadnipError) as e:
                c.run(wpb)
            assert e.value.code == hip.BADARG
            with pytest.raises(hip.CadnipError) as e:
                TA.adj("butterworth").run(wpb)
            assert e.value.code == hip.BADARG
    finally:
        h.ac_set_memory("lds")
    c.run()
    assert h.ac_plan_info()["memory"] == "lds"
    k = chain200
    k.h.ac_set_memory("hbm")
    k.h.ac_solve(k.OM[:1], GMIN, k.b_ac)
    k.h.ac_set_memory("lds")
    for call in (lambda: k.h.ac_solve(k.OM[:1], GMIN, k.b_ac), lambda: k.h.ac_adjoint(k.OM[:1], GMIN, k.e_out, [(0, -1)])):
        with pytest.raises(hip.CadnipError) as e:                # refused again
            call()
        assert e.value.code == hip.BADARG


def test_the_product_api_on_circuits_that_fit():
    mk, params = tc.CHAIN_STAMP["chain40"]
    cs = lambda: api.CircuitSweep(api.MNACircuit(mk(), dict(params)), api.Sweep(vdd=[4.5, 5.5]))
    freqs = api.acdec(2, 1e3, 1e9)
    lds, hbm = api.ac(cs(), freqs, solver="gpu"), api.ac(cs(), freqs, solver="gpu", memory="hbm")
    assert lds[0].stats["memory"] == "lds" and hbm[0].stats["memory"] == "hbm"
    assert hbm[0].stats["gpu_systems"] == 2 * len(freqs) == lds[0].stats["gpu_systems"] and hbm[0].stats["host_systems"] == 0
    for i in range(2):
        assert list(hbm[i]._cache) == [tuple(2 * np.pi * freqs)] and same(hbm[i]["n40"], lds[i]["n40"])
    assert api.ac(cs(), freqs[:2], memory="hbm")[0].stats == {}                          # solver="host": the keyword is ignored
    for fn in (lambda: api.ac(cs(), freqs, solver="gpu", memory="l2"), lambda: api.noise(cs(), "n40", freqs, solver="gpu", memory="l2")):
        with pytest.raises(ValueError):
            fn()
    # api.noise, whole: the supply sweep of tests/test_gpu_noise_solver.py (a model whose sources the host collects without a model file)
    ncs = lambda: api.CircuitSweep(api.MNACircuit(TN.common_source(cj.Param("vdd")), {"vdd": 5.0}), api.Sweep(vdd=[4.5, 5.0, 5.5]))
    nf = np.array([1.0, 1e2, 1e4, 1e6])
    nl, nh = api.noise(ncs(), "out", nf, input="vg", solver="gpu"), api.noise(ncs(), "out", nf, input="vg", solver="gpu", memory="hbm")
    assert nl[0].stats["memory"] == "lds" and nh[0].stats["memory"] == "hbm" and nh[0].stats["gpu_systems"] == 12 and nh[0].stats["host_systems"] == 0
    for i in range(3):
        assert_same_noise(nh[i], nl[i])
    assert api.noise(ncs(), "out", nf, memory="hbm")[0].stats == {}


def assert_same_noise(a, b):
    assert np.array_equal(a["onoise"], b["onoise"]) and list(a.contributions) == list(b.contributions) and len(b.contributions) > 0
    for nm in b.contributions:
        assert np.array_equal(a[nm], b[nm])
    assert (a.gain is None and b.gain is None) or np.array_equal(a.gain, b.gain)


def test_noise_of_the_inverter_case_in_either_memory():
    """The inverter case of tests/noise_ref.py (three supplies, output vout) through api.noise_solve_gpu.  api.noise itself cannot run on
    this circuit in a GPU test: the host collects sp_mos1's sources from the model's Verilog-A text, which is not part of the repository
    (tests/test_noise_cpu.py does it where the text is at hand).  The sources travel as data instead, as in tools/noise_time.py -- the channel
    noise of either transistor, drain to source, and a flicker source -- through the same sweep, gates, merge and PSD weighting."""
    from cadnip_jl_amd.opinfo import _index
    mk, base, pts, grid = R.CASES["inverter"]
    circ = mk()
    sim, st, u, G, C, Gd, Cd = TN.linearise(api.MNACircuit(circ, dict(base)), pts)
    try:
        info = {d["name"]: d for d in st.opinfo}
        srcs = []
        for d in circ.devices:
            if d.type == "MOS1":
                gl = [_index(st, t) for t in info[d.name]["nodes"]]
                srcs += [(gl[0], gl[2], "white", 1e-24, 0.0, d.name.lower()), (gl[0], gl[2], "flicker", 1e-20, 1.0, d.name.lower() + ".fl")]
        assert len(srcs) == 4
        freqs, out = np.asarray(grid())[::5], N.OUTPUTS["inverter"]
        got = {}
        for mem in ("lds", "hbm", "auto"):
            stats = {"gpu_systems": 0, "host_systems": 0, "max_berr": 0.0, "wpb": 0}
            got[mem] = api.noise_solve_gpu(sim.h, st, G, C, Gd, Cd, [srcs] * len(pts), out, freqs, "vin", 27.0, GMIN, "gpu", stats, memory=mem)
            assert stats["memory"] == ("hbm" if mem == "hbm" else "lds") and stats["gpu_systems"] == len(pts) * len(freqs) and stats["host_systems"] == 0
        for k in range(len(pts)):
            assert_same_noise(got["hbm"][k], got["lds"][k])
            assert_same_noise(got["auto"][k], got["lds"][k])
            host = api.noise_solve(st, Gd[k], Cd[k], srcs, out, freqs, "vin", 27.0)
            TN.assert_within_the_solves_bound(st, Gd[k], Cd[k], srcs, out, 27.0, got["hbm"][k], host)
    finally:
        sim.close()


def test_the_product_api_on_the_circuit_beyond_lds():
    """chain200 at the zero state, built as tests/test_gpu_noise_solver.py builds it for the host-path test.  With memory="auto" every system is
    solved on the GPU; against the host path: the plain sweep within the sum of the two solves' forward bounds (tests/test_gpu_ac_solver.py:
    test_gpu_and_host_agree_on_the_flip_flop_sweep), the noise within that module's own bound, assert_within_the_solves_bound."""
    mk, params = tc.CHAIN_STAMP["chain200"]
    sim, st, u, G, C, Gd, Cd = TN.linearise(api.MNACircuit(mk(), dict(params)), at_zero=True)
    try:
        freqs = np.array([1e3, 1e6])
        b_ac = np.zeros(st.n, complex)
        b_ac[st.index_of("I_vin")] = 1.0
        sol = api.ACSol(st, Gd[0], Cd[0], b_ac, np.zeros(st.n), freqs)
        stats = {"gpu_systems": 0, "host_systems": 0, "max_berr": 0.0, "wpb": 0}
        api.ac_gpu_sweep(sim.h, st, [sol], G, C, 2 * np.pi * freqs, GMIN, "auto", stats, memory="auto")
        assert stats["gpu_systems"] == 2 and stats["host_systems"] == 0 and stats["memory"] == "hbm" and "fallback" not in stats
        assert stats["max_berr"] <= api.AC_BERR_MAX
        rows = sol._cache[tuple(2 * np.pi * freqs)]
        for f, w in enumerate(2 * np.pi * freqs):
            A = Gd[0] + 1j * w * Cd[0]
            xr, xh = R.refined_solve_c(A, b_ac), np.linalg.solve(A, b_ac)
            bound = 16 * R.cond_inf_c(A) * EPS * np.max(np.abs(xr))
            assert np.max(np.abs(rows[f] - xr)) <= bound and np.max(np.abs(rows[f] - xh)) <= 2 * bound
        srcs = [(st.index_of("n200"), -1, "thermal", 1e-3, 0.0, "rload"), (st.index_of("n100"), st.index_of("n200"), "white", 1e-20, 0.0, "x")]
        nstats = {"gpu_systems": 0, "host_systems": 0, "max_berr": 0.0, "wpb": 0}
        ns, = api.noise_solve_gpu(sim.h, st, G, C, Gd, Cd, [srcs], "n200", freqs, None, 27.0, 1e-12, "auto", nstats, memory="auto")
        assert nstats["gpu_systems"] == 2 and nstats["host_systems"] == 0 and nstats["memory"] == "hbm" and "fallback" not in nstats and ns.stats is nstats
        host = api.noise_solve(st, Gd[0], Cd[0], srcs, "n200", freqs, None, 27.0)
        TN.assert_within_the_solves_bound(st, Gd[0], Cd[0], srcs, "n200", 27.0, ns, host)
        # the default memory on the same handle: the host path, as ever
        stats = {"gpu_systems": 0, "host_systems": 0, "max_berr": 0.0, "wpb": 0}
        api.ac_gpu_sweep(sim.h, st, [api.ACSol(st, Gd[0], Cd[0], b_ac, np.zeros(st.n), freqs)], G, C, 2 * np.pi * freqs, GMIN, "auto", stats)
        assert stats["gpu_systems"] == 0 and stats["host_systems"] == 2 and "fallback" in stats
    finally:
        sim.close()
