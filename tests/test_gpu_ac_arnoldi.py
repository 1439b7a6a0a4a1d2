"""k_ac_arnoldi / k_ac_arnoldi_hbm (csrc/ac_lu.hip) through the C ABI (cadnip_ac_arnoldi): m steps of shift-invert Arnoldi per (instance, shift)
from one factorisation.  Systems: the cases of ac_ref.CASES on the handles of tests/test_gpu_ac_lu.py -- the Butterworth filter (n = 6,
m = 6: the space closes after four steps), the inverter at its three supplies, the flip-flop (n = 235 > 64: the lane-strided loops wrap) at
3 corners x its 7 grid frequencies as shifts (S = 21: a tail workgroup for W = 2, 4, 8) with m = 8.  The start vector is held against
cadnip_ac_solve to the bit, the launch paths against each other to the bit, and the Arnoldi relation, the orthogonality and m_eff against the
numpy port of tests/pz_ref.py: a GPU figure may be 16 x the port's on the same system and not below 64 eps (api.AC_BERR_MAX's convention)."""
import ctypes as C

import numpy as np
import pytest

import cadnip_jl_amd as cj
from cadnip_jl_amd import api, hip
from tests import ac_ref as R
from tests import pz_ref as Z
from tests import test_gpu_ac_lu as T
from tests.test_gpu_ac_multi import same, LDS_BUDGET

pytestmark = pytest.mark.gpu
GMIN = T.GMIN
EPS = R.EPS
TOL = hip.AC_BREAKDOWN_TOL
ORDER = {"butterworth": 6, "inverter": 6, "dff": 8}


class Arn:
    def __init__(self, name):
        c = self.c = T.case(name)
        self.h, self.st, self.n, self.B, self.m = c.h, c.st, c.st.n, c.B, ORDER[name]
        self.om = c.om if name == "dff" else np.array([c.om[0], c.om[len(c.om) // 2], c.om[-1]])
        self.S = len(self.om)
        out = self.st.index_of(Z.MOS_OUT.get(name, "vout"))
        self.pairs = [(out, -1), (-1, out), (out, (out + 1) % self.n)]
        self.per = 16 * (self.h.lu_stats()["nnz_lu"] + 4 * self.n)
        self.Gd = [R.system(self.st, c.G[b], c.C[b], 0.0, GMIN).real for b in range(self.B)]
        self.Cd = [R.dense_csr(self.st, c.C[b]) for b in range(self.B)]
        self.got0 = self.run()
        self.port = {}

    def run(self, wpb=0, want_v=True, **kw):
        a = dict(omega=self.om, b=self.c.bac, m=self.m, pairs=self.pairs, breakdown_tol=TOL)
        a.update(kw)
        return self.h.ac_arnoldi(a["omega"], GMIN, a["b"], a["m"], a["pairs"], a["breakdown_tol"], wpb, want_v)

    def ported(self, b, s):
        if (b, s) not in self.port:
            cc = np.zeros((1, self.n))
            cc[0, self.pairs[0][0]] = 1.0
            self.port[b, s] = Z.arnoldi_port(self.Gd[b], self.Cd[b], self.c.bac[b], self.om[s], self.m, TOL, cc)
        return self.port[b, s]

    def is_default(self, got, ref=None):
        ref = self.got0 if ref is None else ref
        return all(same(got[i], ref[i]) for i in (0, 1, 3, 4, 5)) and np.array_equal(got[2], ref[2]) and np.array_equal(got[6], ref[6])


_ARN = {}


def arn(name):
    if name not in _ARN:
        _ARN[name] = Arn(name)
    return _ARN[name]


@pytest.mark.parametrize("name", list(ORDER))
def test_the_start_vector_is_ac_solve_to_the_bit(name):
    """r of the kernel is cadnip_ac_solve's x, so v_0 = x / beta in correctly rounded division, component by component -- the form of "beta v_0
    equals x" that holds to the bit (a division followed by a multiplication does not return the dividend's bits); beta v_0 itself is x to
    the rounding of those two operations.  An ac_solve before and one after the Arnoldi call return the same bits."""
    m = arn(name)
    x0, berr0, flags0, _ = m.h.ac_solve(m.om, GMIN, m.c.bac)
    H, beta, meff, l, V, berr, flags, info = m.run()
    x1, berr1, flags1, _ = m.h.ac_solve(m.om, GMIN, m.c.bac)
    assert same(x0, x1) and same(berr0, berr1) and np.array_equal(flags0, flags1)
    assert H.shape == (m.B, m.S, m.m + 1, m.m) and l.shape == (m.B, m.S, m.m, 3) and V.shape == (m.B, m.S, m.m + 1, m.n)
    assert info["systems"] == m.B * m.S and info["lds_bytes"] == info["wpb"] * m.per
    assert not (flags & 3).any() and not flags0.any() and np.all(berr <= api.AC_BERR_MAX) and np.all(meff >= 1)
    v0 = x0.real / beta[:, :, None] + 1j * (x0.imag / beta[:, :, None])
    assert same(V[:, :, 0], v0)
    assert np.all(np.abs(beta[:, :, None] * V[:, :, 0] - x0) <= 2 * EPS * np.abs(x0))
    nrm = np.sqrt(np.sum(x0.real ** 2 + x0.imag ** 2, axis=2))
    assert np.all(np.abs(beta - nrm) <= 4 * (m.n // 64 + 8) * EPS * nrm)


@pytest.mark.parametrize("name", ["butterworth", "dff"])
def test_launch_paths_are_bit_identical(name):
    m = arn(name)
    ref = m.run()
    S = m.B * m.S
    assert m.is_default(ref) and ref[7]["wpb"] in (1, 2, 4, 8) and ref[7]["systems"] == S
    assert m.h.ac_plan_info() == dict(memory="lds", n_waves=0, work_bytes=0, lds_bytes=ref[7]["wpb"] * m.per)
    for wpb in (1, 2, 4, 8):
        if wpb * m.per > LDS_BUDGET:                              # the flip-flop at W = 8
            with pytest.raises(hip.CadnipError) as e:
                m.run(wpb)
            assert e.value.code == hip.BADARG and name == "dff" and wpb == 8
            continue
        got = m.run(wpb)
        assert got[7] == dict(wpb=wpb, lds_bytes=wpb * m.per, systems=S, workgroups=-(-S // wpb)) and m.is_default(got), wpb
    m.h.ac_set_memory("hbm", 2)                                   # two persistent waves, each running system after system in its one workspace
    try:
        for wpb in (0, 1, 2, 4, 8):
            got = m.run(wpb)
            assert got[7] == dict(wpb=wpb or 4, lds_bytes=0, systems=S, workgroups=-(-2 // (wpb or 4)))
            assert m.h.ac_plan_info() == dict(memory="hbm", n_waves=2, work_bytes=2 * m.per, lds_bytes=0)
            assert m.is_default(got), wpb
    finally:
        m.h.ac_set_memory("lds")
    nov = m.run(want_v=False)                                     # the basis is the kernel's own storage: not asking for it changes nothing else
    assert nov[4] is None and all(same(nov[i], ref[i]) for i in (0, 1, 3, 5)) and np.array_equal(nov[2], ref[2]) and np.array_equal(nov[6], ref[6])
    nop = m.run(pairs=None)
    assert nop[3] is None and same(nop[0], ref[0]) and same(nop[4], ref[4])


@pytest.mark.parametrize("name", list(ORDER))
def test_the_reduction_against_the_port(name):
    m = arn(name)
    H, beta, meff, l, V, berr, flags, _ = m.got0
    worst = [0.0, 0.0]
    for b in range(m.B):
        for s, w0 in enumerate(m.om):
            p = m.ported(b, s)
            me = int(meff[b, s])
            assert me == p["m_eff"] and (flags[b, s] & 4) == p["flag"], (b, s, me, p["m_eff"], p["ratios"])
            nv = Z.n_vectors(m.m, me, int(flags[b, s]))
            rel, orth = Z.relation_error(m.Gd[b], m.Cd[b], w0, H[b, s], V[b, s], me), Z.orthogonality_error(V[b, s], nv)
            rel_p, orth_p = Z.relation_error(m.Gd[b], m.Cd[b], w0, p["H"], p["V"], me), Z.orthogonality_error(p["V"], nv)
            print("%s b %d s %d m_eff %d relation gpu %.3g port %.3g  orthogonality gpu %.3g port %.3g  berr %.3g" % (name, b, s, me, rel, rel_p, orth, orth_p, berr[b, s]))
            worst = [max(worst[0], rel / max(16 * rel_p, 64 * EPS)), max(worst[1], orth / max(16 * orth_p, 64 * EPS))]
            assert rel <= max(16 * rel_p, 64 * EPS) and orth <= max(16 * orth_p, 64 * EPS), (b, s)
            # the layout: zero beyond m_eff, the sub-diagonal real and positive, nothing below it
            assert not H[b, s, :, me:].any() and not l[b, s, me:].any() and not V[b, s, nv:].any() and not np.tril(H[b, s], -2).any()
            sub = np.diagonal(H[b, s], -1)
            assert np.all(sub.imag == 0) and np.all(sub.real[:nv - 1] > 0) and not sub[nv - 1:].any()
    print("%s: worst relation / bound %.3g, worst orthogonality / bound %.3g" % (name, worst[0], worst[1]))
    if name == "butterworth":
        assert np.all(meff == 4) and np.all(flags == 4)             # three poles and the algebraic part: the space closes early
    # l is the pair differences of the returned basis
    for k, (pp, pn) in enumerate(m.pairs):
        vp = V[:, :, :m.m, pp] if pp >= 0 else np.zeros_like(l[..., k])
        vn = V[:, :, :m.m, pn] if pn >= 0 else np.zeros_like(l[..., k])
        assert same(l[..., k], vp - vn)


def test_the_butterworth_poles_from_the_kernel():
    """-1 and -1/2 +- j sqrt(3)/2 from H of every shift; gmin = 1e-12 on the node diagonals moves a pole by that order, allowed for explicitly."""
    m = arn("butterworth")
    H, beta, meff, l = m.got0[:4]
    exact = np.array([-1.0, -0.5 + 0.5j * np.sqrt(3.0), -0.5 - 0.5j * np.sqrt(3.0)])
    for s, w0 in enumerate(m.om):
        sol, nb = api.pz_solve(m.st, m.Gd[0], m.Cd[0], m.c.bac[0], m.pairs[0], [w0], m.m, lambda w: (H[0, s], beta[0, s], meff[0, s], l[0, s, :, :1]))
        p = m.ported(0, s)
        ref, _ = api.pz_solve(m.st, m.Gd[0], m.Cd[0], m.c.bac[0], m.pairs[0], [w0], m.m, lambda w: (p["H"], p["beta"], p["m_eff"], p["l"]))
        dense = api.poles_dense(m.Gd[0], m.Cd[0])
        bound = max(16 * float(np.max(Z.match_error(ref.poles, dense, w0))), 64 * EPS)
        err = Z.match_error(sol.poles, dense, w0)
        print("butterworth shift %.3g poles" % w0, sol.poles, "err", err, "bound", bound)
        assert nb == 1 and len(sol.poles) == 3 and np.all(err <= bound) and np.all(sol.pole_resid == 0.0)
        assert np.all(Z.match_error(sol.poles, exact, w0) <= bound + 16 * GMIN)
        assert len(sol.zeros) == 0 and abs(sol.gain - 1.0) <= 1e-9


def test_a_zero_pivot_flags_its_system_and_the_call_returns():
    circ = cj.Circuit("capacitor-only node")
    circ.V("v1", "a", "0", dc=0.0, ac=1.0)
    circ.R("r1", "a", "b", 1e3)
    circ.C("c1", "b", "c", 1e-9)
    circ.C("c2", "c", "0", 1e-9)                       # node c: capacitors only -- at w = 0 without gmin its row is empty
    sim = api.BatchSimulator(api.MNACircuit(circ, {}, api.MNASpec(mode="dcop")))
    try:
        st = sim.st
        sim.analyze()
        sim.h.set_spec(mode="dcop")
        sim.h.rebuild(np.zeros(st.n), 0.0)
        bac = api.rhs_ac(st, circ, {})
        for mode in ("lds", "hbm"):
            sim.h.ac_set_memory(mode, 1 if mode == "hbm" else 0)      # hbm: the flagged system first, then its neighbour, in one workspace
            H, beta, meff, l, V, berr, flags, info = sim.h.ac_arnoldi([0.0, 1e3], 0.0, bac, 3, [(st.index_of("b"), -1)], want_v=True)   # the call returns: CADNIP_OK
            sim.h.ac_set_memory("lds")
            assert info["systems"] == 2 and flags[0, 0] & 1 and flags[0, 0] & 2 and meff[0, 0] == 0 and not H[0, 0].any() and not V[0, 0].any()
            assert (flags[0, 1] & 3) == 0 and meff[0, 1] >= 1 and np.isfinite(H[0, 1]).all()
            x1 = sim.h.ac_solve([0.0, 1e3], 0.0, bac)[0]
            assert same(V[0, 1, 0], x1[0, 1].real / beta[0, 1] + 1j * (x1[0, 1].imag / beta[0, 1]))
        zero = sim.h.ac_arnoldi([1e3], 0.0, np.zeros(st.n, complex), 3, None, want_v=True)     # no excitation: beta = 0 is bit 1 alone
        assert zero[6][0, 0] == 2 and zero[2][0, 0] == 0 and zero[1][0, 0] == 0.0 and not zero[0].any() and not zero[4].any()
    finally:
        sim.close()


def raw(arnx, out, **kw):
    """cadnip_ac_arnoldi itself, on the caller's arrays: the status code"""
    a = dict(om=arnx.om, m=arnx.m, tol=TOL, pairs=arnx.pairs, wpb=0, n_shift=None, n_pairs=None, h=arnx.h)
    a.update(kw)
    om = np.ascontiguousarray(a["om"], dtype=np.float64)
    pairs = np.ascontiguousarray(a["pairs"], dtype=np.int32)
    bac = np.ascontiguousarray(arnx.c.bac)
    H, beta, meff, l, V, berr, flags = out
    info = np.zeros(4, dtype=np.int32)
    D, I = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    h = a["h"]
    return h.lib.cadnip_ac_arnoldi(h.h, C.c_int32(len(om) if a["n_shift"] is None else a["n_shift"]), om.ctypes.data_as(D), C.c_double(GMIN),
                                   bac.ctypes.data_as(D), C.c_int32(a["m"]), C.c_double(a["tol"]), C.c_int32(len(pairs) if a["n_pairs"] is None else a["n_pairs"]),
                                   pairs.ctypes.data_as(I), C.c_int32(a["wpb"]), H.ctypes.data_as(D), beta.ctypes.data_as(D), meff.ctypes.data_as(I),
                                   l.ctypes.data_as(D), V.ctypes.data_as(D), berr.ctypes.data_as(D), flags.ctypes.data_as(I), info.ctypes.data_as(I))


@pytest.mark.parametrize("name", ["butterworth", "dff"])
def test_refusals_launch_nothing(name):
    m = arn(name)
    n = m.n
    out = lambda: tuple(np.array(v) for v in m.got0[:7])
    o = out()
    for v in o:
        v[...] = 0
    assert raw(m, o) == hip.OK and m.is_default(o)                                  # the helper is the call
    plan = m.h.ac_plan_info()
    refused = [dict(n_shift=0), dict(n_shift=-1), dict(m=0), dict(m=-1), dict(m=n + 1), dict(tol=0.0), dict(tol=1.0), dict(tol=-1e-9), dict(tol=2.0),
               dict(tol=float("nan")), dict(n_pairs=-1), dict(pairs=[(n, -1)]), dict(pairs=[(0, n)]), dict(pairs=[(-2, 0)]), dict(wpb=3), dict(wpb=16), dict(wpb=-1)]
    if 8 * m.per > LDS_BUDGET:
        refused.append(dict(wpb=8))                                                # the LDS refusal
    for kw in refused:
        o = out()
        assert raw(m, o, **kw) == hip.BADARG, kw
        assert m.is_default(o) and m.h.ac_plan_info() == plan, kw                  # nothing written, nothing recorded
    assert m.is_default(m.run())                                                   # the handle is as usable as before
    for call in (lambda: m.run(m=0), lambda: m.run(m=n + 1), lambda: m.run(breakdown_tol=1.0), lambda: m.run(pairs=[(n, 0)]), lambda: m.run(3)):
        with pytest.raises(hip.CadnipError) as e:
            call()
        assert e.value.code == hip.BADARG
    with pytest.raises(ValueError):
        m.run(b=m.c.bac[:, :-1])
    fresh = hip.Handle(m.st, m.B)                                                  # no analysis
    try:
        o = out()
        assert raw(m, o, h=fresh) == hip.BADARG and m.is_default(o)
    finally:
        fresh.close()
    empty = m.run(omega=[])                                                        # an empty shift list launches nothing
    assert empty[0].shape == (m.B, 0, m.m + 1, m.m) and empty[4].shape == (m.B, 0, m.m + 1, n) and empty[7]["systems"] == 0
    assert m.h.ac_plan_info() == plan
