"""The overlay forms of the AC kernels (csrc/ac_lu.hip: k_ac_lu_ovl, k_ac_adj_ovl, k_ac_lu_multi_ovl, k_ac_adj_multi_ovl and their _hbm forms)
through the C ABI (cadnip_ac_set_overlay): A = G + gmin + j w C + D with D the table api.ac_delay_overlay computes for the three cases of
tests/ac_delay_ref.py.  Every system against the CPU references of tests/ac_ref.py with D in the reference matrix, exactly as
tests/test_gpu_ac_lu.py / test_gpu_ac_adjoint.py hold the plain kernels; bit-identity across widths, memory homes, the multi calls' columns
and batch position; neutral overlays; the argument checks with the previous setting shown to survive; a NaN in the table."""
import numpy as np
import pytest

from cadnip_jl_amd import api, hip
from tests import ac_delay_ref as D
from tests import ac_ref as R
from tests import noise_ref as N

pytestmark = pytest.mark.gpu
EPS = R.EPS
GMIN = D.GMIN
OUTPUT = {"buffer": "out", "tline": "p2", "dff_delay": "qo"}
_CASES = {}


def same(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.float64), np.ascontiguousarray(b).view(np.float64))


class Case:
    """One handle at the DC points of a case of ac_delay_ref.CASES, analysed on the overlay's pivot sample; the CPU references, once."""

    def __init__(self, name):
        mk, base, pts, grid = D.CASES[name]
        self.name, self.circ = name, mk()
        self.sim = api.BatchSimulator(api.MNACircuit(self.circ, dict(base), api.MNASpec(mode="dcop")), pts if pts != [{}] else None)
        self.st, self.h, self.B = self.sim.st, self.sim.h, self.sim.B
        self.u, conv, _ = self.sim.dc()
        assert np.all(conv), name
        self.h.rebuild(self.u, 0.0)
        G, C, _, _ = self.h.get_GCb()
        to_ref = np.asarray(self.st.to_ref_nz)
        self.G, self.C = G[:, to_ref], C[:, to_ref]                  # CSR order
        self.om = 2.0 * np.pi * np.asarray(grid(), dtype=float)
        self.F = len(self.om)
        self.bac = np.array([api.rhs_ac(self.st, self.circ, {k: float(v[i]) for k, v in self.sim.params.items()}) for i in range(self.B)])
        self.ovl = api.ac_delay_overlay(self.st, self.circ, self.sim.params, self.om, self.B)
        self.sample_ref = np.empty(self.st.nnz)
        self.sample_ref[to_ref] = D.sample(self.st, self.G, self.C, self.om, GMIN, self.ovl)
        self.h.analyze_values(self.sample_ref)
        self.rp, self.cp = self.h.lu_order()
        self.e_out = np.zeros(self.st.n, dtype=complex)
        self.e_out[self.st.index_of(OUTPUT[name])] = 1.0
        self.pairs = np.array([(i, -1) for i in range(self.st.n)], dtype=np.int32)
        self.ref, self.adj_ref = {}, {}
        for b in range(self.B):
            for f, w in enumerate(self.om):
                A = D.system(self.st, self.G[b], self.C[b], w, GMIN, self.ovl, b)
                xs = R.static_order_solve_c(A, self.bac[b], self.rp, self.cp)
                self.ref[b, f] = (A, R.backward_error_c(A, xs, self.bac[b]), R.refined_solve_c(A, self.bac[b]), R.cond_inf_c(A))
                xa = N.static_order_adjoint_c(A, self.e_out, self.rp, self.cp)
                self.adj_ref[b, f] = (A, R.backward_error_c(A.T, xa, self.e_out), R.refined_solve_c(A.T, self.e_out), R.cond_inf_c(A.T))

    def set(self, val=None, om=None):
        self.h.ac_set_overlay(self.ovl.pos, self.om if om is None else om, self.ovl.val if val is None else val)

    def run(self, wpb=0, bac=None, om=None):
        return self.h.ac_solve(self.om if om is None else om, GMIN, self.bac if bac is None else bac, wpb)

    def run_adj(self, wpb=0, om=None):
        return self.h.ac_adjoint(self.om if om is None else om, GMIN, self.e_out, self.pairs, wpb, True)


class overlay:
    """``with overlay(c)``: the case's overlay for the block, cleared after it"""

    def __init__(self, c, val=None, om=None):
        self.c, self.val, self.om = c, val, om

    def __enter__(self):
        self.c.set(self.val, self.om)

    def __exit__(self, *exc):
        self.c.h.ac_clear_overlay()


def case(name):
    if name not in _CASES:
        _CASES[name] = Case(name)
    return _CASES[name]


@pytest.mark.parametrize("name", list(D.CASES))
def test_every_system_against_the_cpu_references(name):
    """Exempt from the forward check: none on ``buffer`` and ``tline`` (tests/test_ac_delay_cpu.py holds every one of their systems far inside
    the gate); on ``dff_delay`` the flip-flop's cap of 5 %."""
    c = case(name)
    S = c.B * c.F
    with overlay(c):
        x, berr, flags, info = c.run()
        h, xa, aberr, aflags, ainfo = c.run_adj()
    assert not flags.any() and not aflags.any() and info["systems"] == S == ainfo["systems"] and same(h, xa)
    for what, ref, xx, be, rhs, T, gate in (("forward", c.ref, x, berr, lambda b: c.bac[b], lambda A: A, api.AC_BERR_MAX),
                                            ("adjoint", c.adj_ref, xa, aberr, lambda b: c.e_out, lambda A: A.T, api.NOISE_BERR_MAX)):
        exempt = 0
        for (b, f), (A, berr_static, xref, kappa) in ref.items():
            host = R.backward_error_c(T(A), xx[b, f], rhs(b))
            print("%s %s b %d f %d berr gpu %.3g host-recomputed %.3g static %.3g fwd %.3g kappa eps %.3g" % (
                name, what, b, f, be[b, f], host, berr_static, np.max(np.abs(xx[b, f] - xref)) / np.max(np.abs(xref)), kappa * EPS))
            assert be[b, f] <= 16 * berr_static + 64 * EPS, (what, b, f)
            assert host / 2 - 8 * EPS <= be[b, f] <= 2 * host + 8 * EPS, (what, b, f)        # the reported figure is that of G + j w C + D
            if berr_static < gate / 16:
                assert np.max(np.abs(xx[b, f] - xref)) <= 16 * kappa * EPS * np.max(np.abs(xref)), (what, b, f)
            else:
                exempt += 1
        assert exempt <= (0.05 * S if name == "dff_delay" else 0), what
    # the overlay matters: without it the same call solves another matrix
    x0, _, _, _ = c.run()
    assert not same(x0, x)


@pytest.mark.parametrize("name", list(D.CASES))
def test_widths_and_memory_homes_are_bit_identical(name):
    c = case(name)
    per = 16 * (c.h.lu_stats()["nnz_lu"] + 3 * c.st.n)
    with overlay(c):
        x0, berr0, flags0, info0 = c.run()
        h0, xa0, aberr0, aflags0, _ = c.run_adj()
        for wpb in (1, 2, 4, 8):
            if wpb * per > 160 * 1024:
                with pytest.raises(hip.CadnipError) as e:
                    c.run(wpb)
                assert e.value.code == hip.BADARG and name == "dff_delay" and wpb == 8
                continue
            x, berr, flags, info = c.run(wpb)
            assert info["wpb"] == wpb and info["workgroups"] == -(-c.B * c.F // wpb)
            assert same(x, x0) and np.array_equal(berr, berr0) and np.array_equal(flags, flags0), wpb
            h, xa, aberr, aflags, _ = c.run_adj(wpb)
            assert same(h, h0) and same(xa, xa0) and np.array_equal(aberr, aberr0) and np.array_equal(aflags, aflags0), wpb
        try:
            for max_waves in (0, 2):
                c.h.ac_set_memory("hbm", max_waves)
                for wpb in (0, 1, 8):
                    x, berr, flags, info = c.run(wpb)
                    assert info["lds_bytes"] == 0 and c.h.ac_plan_info()["memory"] == "hbm"
                    assert c.h.ac_plan_info()["n_waves"] == (min(max_waves, c.B * c.F) if max_waves else c.B * c.F)
                    assert same(x, x0) and np.array_equal(berr, berr0) and np.array_equal(flags, flags0), (max_waves, wpb)
                    h, xa, aberr, aflags, _ = c.run_adj(wpb)
                    assert same(h, h0) and same(xa, xa0) and np.array_equal(aberr, aberr0) and np.array_equal(aflags, aflags0), (max_waves, wpb)
        finally:
            c.h.ac_set_memory("lds")


def test_hbm_waves_stride_over_six_systems_of_the_flip_flop():
    """Two persistent waves over 3 corners x 2 frequencies, on a sub-grid with its own table: the table is indexed by the system's own
    (instance, frequency), so the same systems come out to the bit in LDS, in device memory, and inside the full grid."""
    c = case("dff_delay")
    ff = [1, 5]
    with overlay(c):
        x_full, berr_full, _, _ = c.run()
    with overlay(c, c.ovl.val[:, ff], c.om[ff]):
        x0, berr0, flags0, _ = c.run(om=c.om[ff])
        try:
            c.h.ac_set_memory("hbm", 2)
            x, berr, flags, info = c.run(om=c.om[ff])
            assert info["systems"] == 6 and c.h.ac_plan_info()["n_waves"] == 2
        finally:
            c.h.ac_set_memory("lds")
    assert same(x, x0) and np.array_equal(berr, berr0) and not flags.any() and not flags0.any()
    assert same(x0, x_full[:, ff]) and np.array_equal(berr0, berr_full[:, ff])


@pytest.mark.parametrize("name", ["tline", "dff_delay"])
def test_columns_of_the_multi_calls_are_the_single_column_calls(name):
    c = case(name)
    n = c.st.n
    rng = np.random.default_rng(7)
    cols = np.stack([c.bac, rng.standard_normal((c.B, n)) + 1j * rng.standard_normal((c.B, n))], axis=1)       # [B, 2, n]
    acols = np.stack([np.broadcast_to(c.e_out, (c.B, n)), cols[:, 1]], axis=1)
    with overlay(c):
        singles = [c.h.ac_solve(c.om, GMIN, cols[:, k]) for k in range(2)]
        asingles = [c.h.ac_adjoint(c.om, GMIN, acols[:, k], c.pairs, 0, True) for k in range(2)]
        homes = [("lds", 0)] + ([("hbm", 2)] if name == "dff_delay" else [])
        try:
            for mode, mw in homes:
                c.h.ac_set_memory(mode, mw)
                hh, x, berr, flags, _ = c.h.ac_solve_multi(c.om, GMIN, cols, c.pairs)
                ah, ax, aberr, aflags, _ = c.h.ac_adjoint_multi(c.om, GMIN, acols, c.pairs, 0, True)
                for k in range(2):
                    assert same(x[:, :, k], singles[k][0]) and np.array_equal(berr[:, :, k], singles[k][1]) and same(hh[:, :, k], singles[k][0]), (mode, k)
                    assert same(ax[:, :, k], asingles[k][1]) and same(ah[:, :, k], asingles[k][0]) and np.array_equal(aberr[:, :, k], asingles[k][2]), (mode, k)
                assert not flags.any() and not aflags.any()
        finally:
            c.h.ac_set_memory("lds")


@pytest.mark.parametrize("adjoint", [False, True])
def test_the_multi_calls_under_an_overlay_at_a_forced_width_and_on_strided_waves(adjoint):
    """The two seams of the kernel pair for the multi families with an overlay, which the test above reaches only at the plan's own width:
    the smallest circuit of ac_ref.CASES, 2 instances x 3 frequencies = 6 systems, under a table of its own (two CSR positions, values that
    differ per instance and frequency).  W = 4 in LDS: two workgroups, the second with two waves that have no system.  Two persistent
    waves in device memory: each runs three systems, K columns each, in its one workspace.  Both to the bit against W = 1 in LDS."""
    from tests import test_gpu_ac_lu as T
    c = T.case("butterworth")
    sim = api.BatchSimulator(api.MNACircuit(c.circ, {}, api.MNASpec(mode="dcop")), [{}, {}])
    try:
        h, n = sim.h, c.st.n
        h.set_spec(mode="dcop")
        h.rebuild(c.u[[0, 0]], 0.0)
        h.analyze_values(c.sample_ref)
        om = c.om[[0, len(c.om) // 2, -1]]
        rng = np.random.default_rng(11)
        pos = np.array([0, c.st.nnz - 1], dtype=np.int32)
        val = 1e-3 * (rng.standard_normal((2, 3, 2)) + 1j * rng.standard_normal((2, 3, 2)))
        cols = rng.standard_normal((2, 2, n)) + 1j * rng.standard_normal((2, 2, n))
        pairs = np.array([(i, -1) for i in range(n)], dtype=np.int32)
        call = h.ac_adjoint_multi if adjoint else h.ac_solve_multi
        plain = call(om, GMIN, cols, pairs, 1, True)
        h.ac_set_overlay(pos, om, val)
        ref = call(om, GMIN, cols, pairs, 1, True)
        assert ref[4]["systems"] == 6 and ref[4]["workgroups"] == 6 and not ref[3].any() and not same(ref[1], plain[1])
        got = call(om, GMIN, cols, pairs, 4, True)
        assert got[4]["wpb"] == 4 and got[4]["workgroups"] == 2 and got[4]["lds_bytes"] > 0
        assert same(got[0], ref[0]) and same(got[1], ref[1]) and np.array_equal(got[2], ref[2]) and np.array_equal(got[3], ref[3])
        h.ac_set_memory("hbm", 2)
        for wpb in (1, 4):
            got = call(om, GMIN, cols, pairs, wpb, True)
            assert got[4]["lds_bytes"] == 0 and h.ac_plan_info()["memory"] == "hbm" and h.ac_plan_info()["n_waves"] == 2
            assert same(got[0], ref[0]) and same(got[1], ref[1]) and np.array_equal(got[2], ref[2]) and np.array_equal(got[3], ref[3]), wpb
    finally:
        sim.close()


def test_a_system_alone_equals_the_same_system_in_the_batch():
    c = case("tline")
    with overlay(c):
        x, berr, _, _ = c.run()
    mk, base, pts, _ = D.CASES["tline"]
    b, f = 2, 3
    one = api.BatchSimulator(api.MNACircuit(c.circ, dict(base), api.MNASpec(mode="dcop")), [pts[b]])
    try:
        one.h.rebuild(c.u[b:b + 1], 0.0)
        one.h.analyze_values(c.sample_ref)
        one.h.ac_set_overlay(c.ovl.pos, c.om[f:f + 1], c.ovl.val[b:b + 1, f:f + 1])
        x1, berr1, flags1, info1 = one.h.ac_solve(c.om[f:f + 1], GMIN, c.bac[b:b + 1])
        assert info1["systems"] == 1 and not flags1.any()
        assert same(x1[0, 0], x[b, f]) and berr1[0, 0] == berr[b, f]
    finally:
        one.close()


@pytest.mark.parametrize("name", ["buffer", "dff_delay"])
def test_neutral_overlays(name):
    c = case(name)
    fresh = api.BatchSimulator(api.MNACircuit(c.circ, dict(D.CASES[name][1]), api.MNASpec(mode="dcop")), D.CASES[name][2] if c.B > 1 else None)
    try:
        fresh.h.rebuild(c.u, 0.0)
        fresh.h.analyze_values(c.sample_ref)
        xf, berrf, flagsf, _ = fresh.h.ac_solve(c.om, GMIN, c.bac)
        hf, xaf, aberrf, _, _ = fresh.h.ac_adjoint(c.om, GMIN, c.e_out, c.pairs, 0, True)
    finally:
        fresh.close()
    with overlay(c, np.zeros_like(c.ovl.val)):
        xz, berrz, flagsz, _ = c.run()
        hz, xaz, aberrz, _, _ = c.run_adj()
    # an all-zero table: equal as numbers (x + 0 may turn a -0.0 into 0.0, nothing else)
    assert np.array_equal(xz, xf) and np.array_equal(berrz, berrf) and np.array_equal(flagsz, flagsf)
    assert np.array_equal(xaz, xaf) and np.array_equal(hz, hf) and np.array_equal(aberrz, aberrf)
    # after the overlay is cleared: the fresh handle's bits
    with overlay(c):
        c.run()
    x, berr, flags, _ = c.run()
    h, xa, aberr, _, _ = c.run_adj()
    assert same(x, xf) and np.array_equal(berr, berrf) and np.array_equal(flags, flagsf)
    assert same(xa, xaf) and same(h, hf) and np.array_equal(aberr, aberrf)


def test_bad_arguments_leave_the_previous_setting_in_force():
    c = case("tline")
    nnz, O = c.st.nnz, len(c.ovl.pos)
    assert O >= 2
    with overlay(c):
        x0, berr0, _, _ = c.run()
        lib, H = c.h.lib, c.h.h
        import ctypes as C
        pos = np.ascontiguousarray(c.ovl.pos, dtype=np.int32)
        val = np.ascontiguousarray(c.ovl.val)
        ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
        dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
        call = lambda n_ovl, p, F: lib.cadnip_ac_set_overlay(H, C.c_int32(n_ovl), ip(p), C.c_int32(F), dp(c.om), dp(val))
        twice, outside, below = pos.copy(), pos.copy(), pos.copy()
        twice[1], outside[0], below[0] = twice[0], nnz, -1
        assert call(-1, pos, c.F) == hip.BADARG
        assert call(O, twice, c.F) == hip.BADARG and call(O, outside, c.F) == hip.BADARG and call(O, below, c.F) == hip.BADARG
        assert call(O, pos, 0) == hip.BADARG and call(O, pos, -3) == hip.BADARG
        assert call(O, pos, (256 << 20) // (16 * O * c.B) + 1) == hip.BADARG           # the size check comes before any read of the arrays
        for bad in (lambda: c.h.ac_set_overlay(twice, c.om, c.ovl.val), lambda: c.h.ac_set_overlay(outside, c.om, c.ovl.val)):
            with pytest.raises(hip.CadnipError) as e:
                bad()
            assert e.value.code == hip.BADARG
        with pytest.raises(ValueError):
            c.h.ac_set_overlay(c.ovl.pos, c.om, c.ovl.val[:, :-1])
        # a solve on another grid: one frequency fewer, one moved by an ulp, -0.0 for 0.0
        x = np.full_like(x0, 7.0)
        for om in (c.om[:-1], np.concatenate([c.om[:-1], [np.nextafter(c.om[-1], np.inf)]]), np.concatenate([[-0.0], c.om[1:]])):
            for bad in (lambda: c.run(om=om), lambda: c.run_adj(om=om), lambda: c.h.ac_solve_multi(om, GMIN, c.bac[:, None], c.pairs),
                        lambda: c.h.ac_adjoint_multi(om, GMIN, c.bac[:, None], c.pairs)):
                with pytest.raises(hip.CadnipError) as e:
                    bad()
                assert e.value.code == hip.BADARG
        # the analyses without an overlay form
        with pytest.raises(hip.CadnipError) as e:
            c.h.ac_arnoldi(c.om[:1], GMIN, c.bac, 2)
        assert e.value.code == hip.BADARG
        with pytest.raises(hip.CadnipError) as e:
            c.h.ac_sens(c.om, GMIN, [0], [[1]], [[2]], [[1.0]], c.bac[0], c.e_out, (0, -1))
        assert e.value.code == hip.BADARG
        # after all of them the setting is the one made first
        x1, berr1, _, _ = c.run()
        assert same(x1, x0) and np.array_equal(berr1, berr0)
    # cleared: both refused calls run again
    H_, beta, meff, _, _, _, flags, _ = c.h.ac_arnoldi(c.om[:1], GMIN, c.bac, 2)
    assert H_.shape == (c.B, 1, 3, 2)


def test_a_nan_in_the_table_flags_its_own_system_only():
    c = case("dff_delay")
    with overlay(c):
        x0, berr0, flags0, _ = c.run()
        h0, xa0, aberr0, aflags0, _ = c.run_adj()
    val = c.ovl.val.copy()
    val[1, 4, 0] = np.nan
    with overlay(c, val):
        x, berr, flags, _ = c.run()
        h, xa, aberr, aflags, _ = c.run_adj()
    for fl, xx, x_0, be, be0 in ((flags, x, x0, berr, berr0), (aflags, xa, xa0, aberr, aberr0)):
        assert fl[1, 4] & 1 and fl.sum() == fl[1, 4]
        keep = np.ones((c.B, c.F), dtype=bool)
        keep[1, 4] = False
        assert same(xx[keep], x_0[keep]) and np.array_equal(be[keep], be0[keep])
