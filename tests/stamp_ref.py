"""High-precision reference of the stamping tests (tests/test_stamp_ref_cpu.py, tests/test_gpu_stamp_kernels.py): the oracle's
individual contributions of one restamp, entry by entry in the handle's CSR order, and the error bounds an fp64 reduction of them
must meet whatever its summation order.

A stamped entry is a sum of k contributions c_i (COO order, value_only.jl:414-418), plus gshunt on a node diagonal, times srcFact
for b.  With u = 2^-53 and gamma_k = k u / (1 - k u), any order of the k - 1 additions and the srcFact product gives
|got - sum| <= gamma_{k+1} * S, S = sum |c_i| (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., section 4.2).
Reference sums are taken in long double (u_ld = 2^-64); their own error gamma^ld_k S is added to the bound."""
import math

import numpy as np

import cadnip_jl_amd as cj
from oracle import mna_ref as M
from oracle.dual import val
from oracle.netlist_ref import make_builder

LD = np.longdouble
# device-evaluation tolerance per block type: each GPU contribution may differ from the oracle's r by RHO * slot_scales (|r| plus the
# device's largest non-unit contribution for G and C; |r| plus the device's companion products in that row for b)
RHO = {"default": 1e-12}
# absolute allowance per (block type, array) on top of RHO: an sp_mos1 that is off carries b contributions of the size of its junction
# saturation currents (~1e-19 A), and these differ from the oracle's by up to ~2e-19 A
FLOOR = {("MOS1", "b"): 1e-18}
U = 2.0 ** -53
U_LD = float(np.finfo(np.longdouble).eps) / 2


def gamma(k, u=U):
    k = np.asarray(k, dtype=np.float64)
    return k * u / (1.0 - k * u)


class Recorder(M.DirectStampContext):
    """DirectStampContext that also keeps every stamp_G / stamp_C value in position (COO) order; the deferred b values are the
    context's own b_V."""

    def reset(self):
        super().reset()
        self.rec_G, self.rec_C = [], []

    def stamp_G(self, i, j, v):
        if M._iszero(i) or M._iszero(j):
            return
        if self.G_pos < len(self.G_mapping):
            self.rec_G.append(val(v))
        super().stamp_G(i, j, v)

    def stamp_C(self, i, j, v):
        if M._iszero(i) or M._iszero(j):
            return
        if self.C_pos < len(self.C_mapping):
            self.rec_C.append(val(v))
        super().stamp_C(i, j, v)


def _lists(n_out, targets, values):
    """values[p] -> per-output lists in p order, flattened output by output: (ptr, flat)."""
    targets = np.asarray(targets, dtype=np.int64)
    order = np.argsort(targets, kind="stable")
    ptr = np.zeros(n_out + 1, dtype=np.int64)
    np.add.at(ptr, targets + 1, 1)
    return np.cumsum(ptr), np.asarray(values, dtype=np.float64)[order]


class Stamp:
    """One oracle restamp.  G, C: [nnz] in the handle's CSR order; b: [n].  vg / vc / vb: the contributions, flattened entry by entry in
    COO order, with pointers pg / pc / pb -- the same layout as the Structure's g_ptr / g_slots (so vg[p] is the oracle's value of GPU
    slot g_slots[p] when the pointers agree)."""

    def __init__(self, st, cs, d, gshunt, srcFact):
        inv = np.empty(st.nnz, dtype=np.int64)
        inv[np.asarray(st.to_ref_nz)] = np.arange(st.nnz)
        self.G, self.C, self.b = cs.G.data[st.to_ref_nz].copy(), cs.C.data[st.to_ref_nz].copy(), d.b.copy()
        gm, cm = np.asarray(d.G_mapping[:len(d.rec_G)]), np.asarray(d.C_mapping[:len(d.rec_C)])
        assert np.all(gm > 0) and np.all(cm > 0)
        self.pg, self.vg = _lists(st.nnz, inv[gm - 1], d.rec_G)
        self.pc, self.vc = _lists(st.nnz, inv[cm - 1], d.rec_C)
        rows = np.asarray(d.b_resolved, dtype=np.int64)
        live = rows > 0
        self.pb, self.vb = _lists(st.n, rows[live] - 1, np.asarray(d.b_V)[live])
        self.gshunt, self.srcFact = float(gshunt), float(srcFact)
        self.limit_w = np.array(d.limit_w, dtype=np.float64)
        self.gdiag = gshunt_terms(st, gshunt)


def gshunt_terms(st, gshunt):
    """[nnz] gshunt on the node diagonals (precompile.jl:529-534), 0 elsewhere."""
    g = np.zeros(st.nnz)
    dn = np.asarray(st.diag_nz)
    g[dn[dn >= 0]] = gshunt
    return g


class OracleStamper:
    """The oracle of one circuit, restamped through a Recorder."""

    def __init__(self, circ, params, mode="tran", temp=27.0, st=None):
        self.st = st if st is not None else cj.discover(circ, params)
        bld = make_builder(circ.to_dicts(params))
        spec = M.MNASpec(mode=mode, temp=temp)
        ctx = M.build_with_detection(bld, {}, spec)
        self.cs = M.compile_structure(bld, {}, spec, ctx=ctx)
        self.ws = M.create_workspace(self.cs, ctx=ctx)
        d = self.ws.dctx
        self.ws.dctx = Recorder(ctx, d.G_nzval, d.C_nzval, d.b, d.G_mapping, d.C_mapping, d.b_resolved)
        assert self.st.n == self.cs.n and self.st.nnz == self.cs.G.nnz

    def rebuild(self, u, t, gshunt=0.0, srcFact=1.0, initjct=False):
        cs = self.cs
        if gshunt != 0.0 or srcFact != 1.0:
            cs = cs.with_spec(cs.spec.replace(gshunt=gshunt, srcFact=srcFact))
        self.ws.dctx.initjct = bool(initjct)
        try:
            M.fast_rebuild(self.ws, np.asarray(u, dtype=np.float64), float(t), cs)
        finally:
            self.ws.dctx.initjct = False
        return Stamp(self.st, self.cs, self.ws.dctx, gshunt, srcFact)


def coo_sums(vals, ptr, extra=None, scale=1.0):
    """The oracle's own evaluation order: 0.0 + c_0 + c_1 + ... per entry (float64, sequential), then + extra, then * scale when scale < 1."""
    out = np.zeros(len(ptr) - 1)
    for e in range(len(out)):
        s = 0.0
        for v in vals[ptr[e]:ptr[e + 1]]:
            s += float(v)
        out[e] = s
    if extra is not None:
        out = out + np.where(extra != 0.0, extra, 0.0)
    if scale < 1.0:
        out = out * scale
    return out


def fsum_entries(vals, ptr):
    """Correctly rounded sum of every entry's contributions (math.fsum)."""
    return np.array([math.fsum(vals[ptr[e]:ptr[e + 1]]) for e in range(len(ptr) - 1)])


def _segsum(x, ptr):
    """Per-entry sums of x[..., ptr[e]:ptr[e+1]] (any leading batch shape), zero for an empty entry."""
    x = np.asarray(x)
    out = np.zeros(x.shape[:-1] + (len(ptr) - 1,), dtype=x.dtype)
    cnt = np.diff(ptr)
    ne = np.nonzero(cnt > 0)[0]
    if ne.size:
        out[..., ne] = np.add.reduceat(x, np.asarray(ptr[:-1])[ne], axis=-1)
    return out


class Check:
    """Result of an entry-by-entry comparison: worst |got - ref| / bound, the failing entries (batch index, entry)."""

    def __init__(self, ratio, bad, what=""):
        self.ratio, self.bad, self.what = ratio, bad, what

    @property
    def ok(self):
        return self.bad.size == 0

    def __repr__(self):
        return "Check(%s worst ratio %.3g, %d failing %s)" % (self.what, self.ratio, self.bad.shape[0], self.bad[:5].tolist())


def sums_and_bounds(vals, ptr, shape, extra=None, scale=1.0, rho=0.0, slack=None):
    """(ref, bound, k) of check_sums for outputs of shape `shape` [..., n_out], all long double but k: the long-double sums
    (sum of vals per entry + extra) * scale, the entrywise bound (rho + gamma_{k+1} + gamma^ld_{k+1}) * S + slack and the term counts."""
    vals = np.asarray(vals, dtype=np.float64)
    ptr = np.asarray(ptr, dtype=np.int64)
    cnt = np.diff(ptr)
    ref = _segsum(vals.astype(LD), ptr)
    S = _segsum(np.abs(vals).astype(LD), ptr)
    k = np.broadcast_to(cnt, shape).astype(np.float64)
    if extra is not None:
        ex = np.broadcast_to(np.asarray(extra, dtype=np.float64), shape)
        ref = ref + ex.astype(LD)
        S = S + np.abs(ex).astype(LD)
        k = k + (ex != 0.0)
    sc = np.asarray(scale, dtype=np.float64)
    if sc.ndim:
        sc = sc.reshape(sc.shape + (1,) * (len(shape) - sc.ndim))
    ref = ref * sc.astype(LD)
    S = S * sc.astype(LD)
    bound = (rho + gamma(k + 1) + gamma(k + 1, U_LD)).astype(LD) * S
    if slack is not None:
        bound = bound + _segsum(np.asarray(slack, dtype=np.float64).astype(LD), ptr) * sc.astype(LD)
    return ref, bound, k


def check_sums(got, vals, ptr, extra=None, scale=1.0, rho=0.0, slack=None, what=""):
    """got [..., n_out] against (sum of vals per entry + extra) * scale.  vals [..., n_contrib] (flattened entry by entry, pointers ptr);
    extra [n_out] or [..., n_out] (gshunt), scale scalar or [...] (srcFact).  Bound per entry: (rho + gamma_{k+1} + gamma^ld_{k+1}) * S with
    S = (sum |c_i| + |extra|) * scale, k = number of terms; slack: per contribution allowance of the device evaluation, added to the bound (summed per entry, times scale).  An entry with no term at all
    must be exactly 0."""
    got = np.asarray(got, dtype=np.float64)
    ref, bound, k = sums_and_bounds(vals, ptr, got.shape, extra, scale, rho, slack)
    err = np.abs(got.astype(LD) - ref)
    empty = k == 0
    fin = np.isfinite(got) & np.isfinite(np.asarray(ref, dtype=np.float64))
    bad_mask = np.where(empty, got != 0.0, ~fin | (err > bound))
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(empty | ~fin, 0.0, np.asarray(err / np.where(bound > 0, bound, LD(1e-300)), dtype=np.float64))
    return Check(float(np.max(r)) if r.size else 0.0, np.argwhere(bad_mask), what)


def check_stamp(got_G, got_C, got_b, ref, rho=0.0, st=None, u=None):
    """End to end: one instance's G, C (CSR order) and b against a Stamp's contributions -- (G, C, b) Checks.  With a Structure and a
    device-evaluation tolerance rho (a number, or a {block type: rho} dict with a "default"), every contribution may be off by
    rho * its own scale (slot_scales; u: the state, for the companion part of b's), and the entry's bound grows by the sum of that over
    its contributions.  Without a Structure, rho multiplies S (the summation bound only)."""
    sc = slot_scales(st, ref, u) if st is not None and rho else None

    def slack(which, slots):
        return None if sc is None else rho_of(st, which, slots, rho) * sc[which] + floor_of(st, which, slots)
    r0 = 0.0 if st is not None else rho
    return (check_sums(got_G, ref.vg, ref.pg, extra=ref.gdiag, rho=r0, slack=slack("g", st.g_slots if st else None), what="G"),
            check_sums(got_C, ref.vc, ref.pc, rho=r0, slack=slack("c", st.c_slots if st else None), what="C"),
            check_sums(got_b, ref.vb, ref.pb, scale=ref.srcFact, rho=r0, slack=slack("b", st.b_slots if st else None), what="b"))


def stamp_bounds(ref, rho=0.0, st=None, u=None):
    """What check_stamp holds one instance's G, C and b to, as numbers: ((G_ref, E_G), (C_ref, E_C), (b_ref, E_b)), long double, G and C
    [nnz] in the handle's CSR order and b [n] -- the long-double sums of the Stamp's contributions and the entrywise bounds
    gamma_{k+1} S plus the RHO / FLOOR allowances of the slots (same arguments as check_stamp)."""
    sc = slot_scales(st, ref, u) if st is not None and rho else None

    def slack(which, slots):
        return None if sc is None else rho_of(st, which, slots, rho) * sc[which] + floor_of(st, which, slots)
    r0 = 0.0 if st is not None else rho
    g = sums_and_bounds(ref.vg, ref.pg, (len(ref.pg) - 1,), extra=ref.gdiag, rho=r0, slack=slack("g", st.g_slots if st else None))
    c = sums_and_bounds(ref.vc, ref.pc, (len(ref.pc) - 1,), rho=r0, slack=slack("c", st.c_slots if st else None))
    b = sums_and_bounds(ref.vb, ref.pb, (len(ref.pb) - 1,), scale=ref.srcFact, rho=r0, slack=slack("b", st.b_slots if st else None))
    return g[:2], c[:2], b[:2]


def slot_scales(st, ref, u=None):
    """{"g", "c", "b"}: per contribution (aligned with ref.vg / vc / vb), the magnitude its device-evaluation error is measured against.
    G and C: |r| plus M'_dev, the largest |r| of the same device's contributions to that array other than its structural +-1
    entries (the unit entries of charge and branch rows): a conductance made of several terms of the device may cancel to 0 in the
    oracle and to ~1e-19 in another evaluation order, while gmin-sized entries are still held to 1e-12 of the device's own largest
    conductance.  b: |r| plus M_dev (the device's largest |b| contribution) plus, with the state u, the sum of |g u_j| over the same
    device's G contributions to the same row: a b contribution is a companion current I - sum_j g_j v_j evaluated at the limited
    junction voltages, which cancels down to the rounding of the device's currents and products (a linear resistor's is exactly 0 in
    the oracle and ~1e-21 with a fused multiply-add).  The absolute FLOOR comes on top."""
    out = {}
    ndev = sum(b.count for b in st.blocks) + 1
    for which, vals, slots in (("g", ref.vg, st.g_slots), ("c", ref.vc, st.c_slots), ("b", ref.vb, st.b_slots)):
        a = np.abs(np.asarray(vals, dtype=np.float64))
        dev = slot_devices(st, which)[slots]
        md = np.zeros(ndev)
        np.maximum.at(md, dev, np.where((a == 1.0) & (which != "b"), 0.0, a))
        out[which] = a + md[dev]
    if u is not None and len(ref.vb):
        rows = np.repeat(np.arange(st.n), np.diff(st.rowptr))
        ent = np.repeat(np.arange(st.nnz), np.diff(st.g_ptr))
        kg = slot_devices(st, "g")[st.g_slots] * st.n + rows[ent]
        gu = np.abs(ref.vg * np.asarray(u, dtype=np.float64)[np.asarray(st.colidx)[ent]])
        kb = slot_devices(st, "b")[st.b_slots] * st.n + np.repeat(np.arange(st.n), np.diff(st.b_ptr))
        keys, inv = np.unique(kg, return_inverse=True)
        acc = np.zeros(len(keys))
        np.add.at(acc, inv, gu)
        pos = np.clip(np.searchsorted(keys, kb), 0, max(len(keys) - 1, 0))
        hit = (keys[pos] == kb) if len(keys) else np.zeros(len(kb), bool)
        out["b"] = out["b"] + np.where(hit, acc[pos] if len(keys) else 0.0, 0.0)
    return out


def floor_of(st, which, slots):
    """Per-slot absolute allowance of the device evaluation (FLOOR by block type and array, 0 elsewhere)."""
    ty = slot_types(st, which)[slots]
    return np.array([FLOOR.get((t, which), 0.0) for t in ty], dtype=np.float64)


def rho_of(st, which, slots, rho):
    """Per-slot device-evaluation tolerance: rho, or rho[type] (rho["default"] otherwise) by the slot's block type."""
    if not isinstance(rho, dict):
        return np.full(len(slots), float(rho))
    ty = slot_types(st, which)[slots]
    return np.array([rho.get(t, rho["default"]) for t in ty], dtype=np.float64)


def slot_devices(st, which):
    """Global device number of every slot of array `which` ("g", "c", "b")."""
    total = {"g": st.ns_g, "c": st.ns_c, "b": st.ns_b}[which]
    out = np.full(total, -1, dtype=np.int64)
    d0 = 0
    for blk in st.blocks:
        base, nk = {"g": (blk.g_base, blk.n_g), "c": (blk.c_base, blk.n_c), "b": (blk.b_base, blk.n_b)}[which]
        if blk.count:
            out[base:base + nk * blk.count] = d0 + np.tile(np.arange(blk.count), nk)
        d0 += blk.count
    return out


def slot_types(st, which):
    """Block type of every slot of array `which`."""
    total = {"g": st.ns_g, "c": st.ns_c, "b": st.ns_b}[which]
    out = np.empty(total, dtype=object)
    for blk in st.blocks:
        base, nk = {"g": (blk.g_base, blk.n_g), "c": (blk.c_base, blk.n_c), "b": (blk.b_base, blk.n_b)}[which]
        out[base:base + nk * blk.count] = blk.type
    return out


def slot_ratio(s, r, scale):
    """Per slot |s - r| / scale (slot_scales); where the scale is 0, 0 if s == r and inf otherwise."""
    s, r = np.asarray(s, dtype=np.float64), np.asarray(r, dtype=np.float64)
    den = np.asarray(scale, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(den > 0, np.abs(s - r) / np.where(den > 0, den, 1.0), np.where(s == r, 0.0, np.inf))
    return q


def residual_check(r, G, Cm, b, u, du, st, skip_rows=None):
    """r [B, n] of resid = C du + G u - b against the same product in long double, from the GPU's own G, C (reference CSC order) and b:
    bound gamma_{2m+1} (sum |C_p du_j| + sum |G_p u_j| + |b_i|) for a row of m entries."""
    rows = np.repeat(np.arange(st.n), np.diff(st.rowptr))
    cols = np.asarray(st.colidx, dtype=np.int64)
    perm = np.asarray(st.to_ref_nz, dtype=np.int64)
    Gc, Cc = np.asarray(G)[:, perm].astype(LD), np.asarray(Cm)[:, perm].astype(LD)
    u, du = np.asarray(u, dtype=np.float64).astype(LD), np.asarray(du, dtype=np.float64).astype(LD)
    pc, pg = Cc * du[:, cols], Gc * u[:, cols]
    rp = np.asarray(st.rowptr, dtype=np.int64)
    ref = _segsum(pc, rp) + _segsum(pg, rp) - np.asarray(b).astype(LD)
    S = _segsum(np.abs(pc), rp) + _segsum(np.abs(pg), rp) + np.abs(np.asarray(b)).astype(LD)
    m = np.diff(rp).astype(np.float64)
    bound = (gamma(2 * m + 1) + gamma(2 * m + 1, U_LD)).astype(LD) * S
    err = np.abs(np.asarray(r).astype(LD) - ref)
    bad = np.argwhere(err > bound)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1), np.where(err > 0, np.inf, 0.0))))
    return Check(ratio, bad, "residual")


def fma_exact(a, b, c):
    """round(a * b + c) for float64 arrays, exactly (fractions: one correctly rounded result per element)."""
    from fractions import Fraction
    a, b, c = (np.asarray(x, dtype=np.float64) for x in (a, b, c))
    out = np.empty(np.broadcast(a, b, c).shape)
    for idx in np.ndindex(out.shape):
        x, y, z = float(np.broadcast_to(a, out.shape)[idx]), float(np.broadcast_to(b, out.shape)[idx]), float(np.broadcast_to(c, out.shape)[idx])
        out[idx] = float(Fraction(x) * Fraction(y) + Fraction(z)) if all(map(math.isfinite, (x, y, z))) else x * y + z
    return out


def jacobian_ok(J, G, Cm, gam):
    """J == G + gamma C entry by entry, bit for bit, in the unfused (G + round(gamma C)) or the fused (one rounding) evaluation."""
    gam = np.asarray(gam, dtype=np.float64).reshape(-1, 1)
    unf = G + gam * Cm
    same = (J == unf) | (np.isnan(J) & np.isnan(unf))
    if np.all(same):
        return True
    idx = np.nonzero(~same)
    fused = fma_exact(np.broadcast_to(gam, J.shape)[idx], Cm[idx], G[idx])
    return bool(np.all(J[idx] == fused))
