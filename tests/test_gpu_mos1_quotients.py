"""The exact fast quotients of the sp_mos1 load section (devices.hpp: m1_quot) against IEEE division, bit for bit.

The probe library (csrc/probe/prim_probe.hip) compiles the parts of the load section -- m1_junction, m1_channel, m1_qdep, m1_limit -- twice from
one macro: with the quotients the stamps run (probe_m1_*_fq) and with IEEE division at every site (probe_m1_*_ieee).  The bias grid below reaches
every branch of the four functions, on both sides of each boundary and exactly on it, for n and p type cards with mj == 0.5 and mj != 0.5,
mjsw == mj and mjsw != mj, with and without junction capacitance, and two multiplicities.  The assertion is bit equality of every output of
every grid point, NaN patterns included; no point is left out of the comparison.  Coverage is asserted too: each branch the issue names must
have grid points on it, as told by the host from the inputs and the device's own threshold voltage (plain single subtractions and comparisons,
which the device cannot round differently)."""
import numpy as np
import pytest

from cadnip_jl_amd import mos1_params as m1
from tests import prim_probe as P

pytestmark = pytest.mark.gpu

M1_NPAR = 34                     # rows of the device's parameter block (devices.hpp: M1_NPAR); mos1_params.NPAR has two reserved rows more
P.SHAPES.setdefault("m1_parts_fq", (3 + M1_NPAR, 30, 0, 0))
P.SHAPES.setdefault("m1_parts_ieee", (3 + M1_NPAR, 30, 0, 0))
P.SHAPES.setdefault("m1_limit_fq", (8 + M1_NPAR, 4, 1, 0))
P.SHAPES.setdefault("m1_limit_ieee", (8 + M1_NPAR, 4, 1, 0))


def _cards():
    """(label, [M1_NPAR] parameter column): n / p type x (mj, mjsw) x multiplicity, and one card without junction capacitance."""
    out = []
    for typ in (1, -1):
        for mj, mjsw, mf in ((0.5, 0.5, 1.0), (0.5, 0.33, 3.0), (0.4, 0.4, 1.0), (0.4, 0.5, 3.0)):
            given = {"type": typ, "vto": 0.7 * typ, "kp": 1e-4, "gamma": 0.5, "phi": 0.7, "lambda": 0.02, "cbd": 1e-15, "cbs": 2e-15, "cjsw": 1e-10,
                     "pd": 2e-6, "ps": 3e-6, "pb": 0.8, "fc": 0.5, "is": 1e-14, "w": 1e-6, "l": 1e-6, "mj": mj, "mjsw": mjsw}
            par, info = m1.derive(given, 27.0 if mf == 1.0 else 85.0, 27.0, 1e-12, mfactor=mf)
            assert info["cbs_nonzero"] and info["cbd_nonzero"]
            out.append(("type%+d mj%g mjsw%g m%g" % (typ, mj, mjsw, mf), par[:M1_NPAR, 0].copy()))
    par, info = m1.derive({"type": 1, "vto": 0.7, "kp": 1e-4, "gamma": 0.5, "phi": 0.7, "lambda": 0.02, "w": 1e-6, "l": 1e-6}, 27.0, 27.0, 1e-12)
    assert not info["cbs_nonzero"] and not info["cbd_nonzero"]
    out.append(("no junction capacitance", par[:M1_NPAR, 0].copy()))
    return out


def _ulps(x, ks):
    """x moved by k units in the last place, for every k of ks"""
    out = []
    for k in ks:
        y = np.float64(x)
        for _ in range(abs(k)):
            y = np.nextafter(y, np.inf if k > 0 else -np.inf)
        out.append(float(y))
    return out


def _both(name, din, iin=()):
    fq = P.run(name + "_fq", din, iin)[0]
    ieee = P.run(name + "_ieee", din, iin)[0]
    return fq, ieee


def _assert_same_bits(fq, ieee, what):
    a, b = np.ascontiguousarray(fq).view(np.uint64), np.ascontiguousarray(ieee).view(np.uint64)
    bad = np.argwhere(a != b)
    print("%s: %d outputs of %d grid points compared, %d differ" % (what, a.size, a.shape[1], len(bad)))
    assert len(bad) == 0, "%s: output row / grid point of the first differences: %s" % (what, bad[:10].tolist())


def _rows(points, par):
    """input rows [k][n]: the bias columns of ``points`` ([n, nb]) followed by the parameter block, the same for every point"""
    pts = np.asarray(points, dtype=np.float64)
    return list(pts.T) + [np.full(len(pts), v) for v in par]


@pytest.mark.parametrize("card", _cards(), ids=lambda c: c[0])
def test_load_parts_fast_quotients_equal_ieee_division_bit_for_bit(card):
    label, par = card
    vt, tphi, depcap, has_cap = par[m1.P_VT], par[m1.P_TPHI], par[m1.P_TDEPCAP], par[m1.P_CBS] != 0
    # junction voltages: below / on / above -3 vt; reverse, zero, forward; on both sides of tDepCap and on it; beyond sel > 2 tPhi (sarg clamps to
    # zero); x = v / vt above the 709 clamp
    vj = sorted(set(_ulps(-3 * vt, (-1, 0, 1)) + _ulps(depcap, (-1, 0, 1)) + [-5.0, -1.0, -0.3, -0.0, 0.0, 1e-300, 0.2, 0.6, 0.9, 1.3, 3.0, 19.0, 25.0]))
    vds_set = [-3.0, -1.0, -0.5, -0.0, 0.0, 0.25, 0.5, 1.0, 4.0]
    base = [(0.0, vds, vbs) for vds in vds_set for vbs in vj] + [(0.0, vds, vbd + vds) for vds in vds_set for vbd in vj]
    # pass 1: the device's threshold voltage at every (vds, vbs) -- it does not depend on vgs
    dvon = P.run("m1_parts_ieee", _rows(base, par))[0][8]
    pts = []
    for (_, vds, vbs), von in zip(base, dvon):
        fwd = vds >= 0                                    # (b.v >= 0: -0.0 counts as forward)
        vdsm = vds if fwd else -vds
        # the device's vgst: (vgs - von) forward, ((vgs - vds) - von) reverse
        vgst = (lambda g: np.float64(g) - von) if fwd else (lambda g: (np.float64(g) - np.float64(vds)) - von)
        cand = [von - 2.0, von - 0.1, von + 0.5 * vdsm, von + vdsm + 0.3, von + 5.0]
        for target in (0.0, vdsm):                        # exactly on the cut-off and on the linear / saturation boundary, and one ulp to either side
            guess = von + target if fwd else (von + target) + vds
            near = _ulps(guess, range(-4, 5))
            hit = [g for g in near if vgst(g) == target]
            cand += hit[:1] + ([] if not hit else _ulps(hit[0], (-1, 1)))
        pts += [(g, vds, vbs) for g in cand]
    pts = np.array(pts)
    fq, ieee = _both("m1_parts", _rows(pts, par))
    _assert_same_bits(fq, ieee, "m1_junction / m1_channel / m1_qdep, " + label)
    # ---- coverage, from the inputs and the device's dvon
    vgs, vds, vbs = pts.T
    vbd, von, mode = vbs - vds, ieee[8], ieee[28]
    assert np.array_equal(mode, np.where(vds >= 0, 1.0, -1.0))
    for m in (1.0, -1.0):
        k = mode == m
        vgst = np.where(k, (vgs - von) if m > 0 else ((vgs - vds) - von), np.nan)
        vdsm = vds * m
        sel = vbs if m > 0 else vbd
        for name, c in (("cut-off", vgst < 0), ("on the cut-off boundary", vgst == 0), ("saturation", (vgst > 0) & (vgst < vdsm)),
                        ("on the linear / saturation boundary", (vgst > 0) & (vgst == vdsm)), ("linear", (vgst > 0) & (vgst > vdsm)),
                        ("sel < 0", k & (sel < 0)), ("sel == 0", k & (sel == 0)), ("sel > 0", k & (sel > 0)), ("sarg clamped", k & (sel > 2.5 * tphi))):
            assert np.any(c), "%s, mode %+d: no grid point %s" % (label, m, name)
        assert np.all(ieee[16][k & (vgst <= 0)] == 0) and np.all(ieee[16][k & (vgst > 0) & (vdsm > 0)] != 0)   # cdrain says the same
    ib = 1.0 / vt
    for name, v in (("vbs", vbs), ("vbd", vbd)):
        for what, c in (("below -3 vt", v < -3 * vt), ("on -3 vt", v == -3 * vt), ("above -3 vt", (v > -3 * vt) & (v < 0)), ("forward", v > 0),
                        ("above the 709 clamp", v * ib > 709.0), ("below tDepCap", v < depcap), ("on tDepCap", v == depcap), ("above tDepCap", v > depcap)):
            assert np.any(c), "%s: no grid point with %s %s" % (label, name, what)
    # the charges follow the two laws where there is capacitance and are zero where there is none
    assert (np.any(ieee[20][vbs < depcap] != 0) and np.any(ieee[20][vbs > depcap] != 0)) if has_cap else not np.any(ieee[20:28])
    assert np.all(np.isfinite(ieee)) and ieee[29, 0] == par[m1.P_GMIN] / par[m1.P_MFACTOR]


def _limit_points(par, quiet):
    """(rows of V(g), V(b), V(d_int), V(s_int), u_l0..3): previous limited voltages x moves.  quiet: every move within the limiters' quiet band."""
    typ, vt = par[m1.P_TYPE], par[m1.P_VT]
    old = [(ovgs, ovds, ovbs) for ovgs in (-1.0, 0.3, 1.2, 2.9, 4.5, 6.0) for ovds in (-4.0, -0.6, 0.0, 0.2, 3.0, 5.0) for ovbs in (-2.0, 0.0, 0.3, 0.66, 0.8)]
    if quiet:
        moves = [(a, b, c) for a in (-0.15, 0.0, 0.15) for b in (-0.02, 0.0, 0.02) for c in (-0.02, 0.0, 0.02)]   # |c - b| <= 0.04 < 2 vt: vbd is quiet too
    else:
        moves = [(a, b, c) for a in (-6.0, -1.5, -0.45, 0.0, 0.6, 3.0) for b in (-5.0, -0.7, 0.0, 0.45, 1.5, 6.0) for c in (-5.0, -1.0, -3 * vt, 0.0, vt, 0.1, 0.4, 2.0, 8.0)]
    rows = []
    for ovgs, ovds, ovbs in old:
        for k, (a, b, c) in enumerate(moves):
            vsi = 0.0 if k % 2 else 0.3
            vgs, vds, vbs = ovgs + a, ovds + b, ovbs + c
            # the fourth limit unknown is vbd: consistent with the others, or (every fifth point) a value of its own
            ovbd = ovbs - ovds if quiet or k % 5 else 0.5
            rows.append((typ * vgs + vsi, typ * vbs + vsi, typ * vds + vsi, vsi, typ * ovgs, typ * ovds, typ * ovbs, typ * ovbd))
    return np.array(rows)


@pytest.mark.parametrize("card", [c for c in _cards() if "m3" not in c[0] and "mj0.4" not in c[0]], ids=lambda c: c[0])
def test_limiting_fast_quotients_equal_ieee_division_bit_for_bit(card):
    """m1_limit: the limiters active (large moves: DEVfetlim, DEVlimvds and both branches of DEVpnjlim, the old-threshold square root on either side
    of osel = 0) and inactive (whole waves of quiet points: the quiet-round shortcut), with and without initjct.  (The limiters kept IEEE division
    in the end -- csrc/devices.hpp says why -- so the two probes run the same code today; the comparison stands for the day a site is converted.)"""
    label, par = card
    typ, vt, vcrit = par[m1.P_TYPE], par[m1.P_VT], par[m1.P_SVCRIT]
    act = _limit_points(par, quiet=False)
    qui = _limit_points(par, quiet=True)
    qui = qui[:len(qui) // 64 * 64]                      # whole waves: one lane that is not quiet sends its wave through the limiters
    assert len(qui) >= 64
    for pts, what in ((act, "active"), (qui, "inactive")):
        for initjct in (0, 1):
            fq, ieee = _both("m1_limit", _rows(pts, par), [np.full(len(pts), initjct)])
            _assert_same_bits(fq, ieee, "m1_limit, limiting %s, initjct %d, %s" % (what, initjct, label))
            vsi = pts[:, 3]
            new = np.stack([typ * (pts[:, 0] - vsi), typ * (pts[:, 2] - vsi), typ * (pts[:, 1] - vsi)])      # vgs, vds, vbs before limiting
            lim = typ * ieee[:3]
            # (a coverage classification only: m1_limit rebuilds vds and vgd from differences, so "unchanged" is to rounding; a clamp moves a voltage by 0.05 V and more)
            changed = np.any(np.abs(lim - new) > 1e-9, axis=0)
            if initjct:
                assert np.all(lim[2] == -1.0) and np.all(lim[1] == 0.0)
            elif what == "inactive":
                assert not np.any(changed)
            else:
                o_vds, o_vbs, o_vbd = typ * pts[:, 5], typ * pts[:, 6], typ * pts[:, 7]
                vbs_new, vbd_new = new[2], new[2] - new[1]
                pn_s = (vbs_new > vcrit) & (np.abs(vbs_new - o_vbs) > 2 * vt)
                pn_d = (vbd_new > vcrit) & (np.abs(vbd_new - o_vbd) > 2 * vt)
                for name, c in (("limited", changed), ("passed unchanged", ~changed), ("pnjlim vbs from a forward junction", pn_s & (o_vbs > 0)),
                                ("pnjlim vbs from a reverse junction", pn_s & (o_vbs <= 0)), ("pnjlim vbd from a forward junction", pn_d & (o_vbd > 0) & (new[1] < 0)),
                                ("old forward, osel > 0", (o_vds >= 0) & (o_vbs > 0)), ("old reverse, osel > 0", (o_vds < 0) & (o_vbd > 0)),
                                ("osel <= 0", (o_vds >= 0) & (o_vbs <= 0))):
                    assert np.any(c), "%s: no grid point %s" % (label, name)
            assert np.all(np.isfinite(ieee))
