"""Helpers that put one sweep instance of a product Structure onto the CPU port (oracle)."""
import numpy as np
from cadnip_jl_amd import api

import cadnip_jl_amd as cj
from cadnip_jl_amd import hip
from cadnip_jl_amd.structure import TYPE_ID
from oracle import cpu_port


def make_port(circ, params, temp=27.0, mode="tran", gmin=1e-12):
    st = cj.discover(circ, params)
    packed = cj.pack_params(st, circ, {k: np.array([float(v)]) for k, v in params.items()}, np.array([float(temp)]), 1, gmin=gmin)
    port = cpu_port.Port(st, [p[0] for p in packed], TYPE_ID)
    port.set_spec(mode=mode, gmin=gmin)
    return st, port


def analyze_port(st, port, vscale, gamma=1e9, seed=1234, n_samples=6, delayed=None):
    """Same sample construction as BatchSimulator.analyze (api.py), evaluated with the port's stamps;
    the symbolic phase itself is the product's host code (cadnip_host_lu_analyze).  ``delayed``: see analyze_port_delayed."""
    rng = np.random.default_rng(seed)
    acc = np.zeros(st.nnz)
    for k in range(n_samples):
        if k == 0:
            u = np.zeros(st.n)
            u[st.n - st.n_limits:] = st.limit_init
            port.set_spec(initjct=1)
        elif k == 1:
            u = np.zeros(st.n)
        else:
            u = (rng.random(st.n) * 1.2 - 0.1) * vscale
            u[st.n_nodes:st.n_nodes + st.n_currents] = 0.0
        G, C, b, lw = port.rebuild(u, 0.0)
        port.set_spec(initjct=0)
        acc = np.maximum(acc, api.clip_sample(G + gamma * C)[0])
    if delayed is not None:
        pos, left = delayed
        acc[pos] = left
    prog = hip.host_lu_analyze(st.n, st.rowptr, st.colidx, acc, sample=True, leaves=hip.leaves_of(st))   # the pivot order a handle uses
    port.set_lu(prog)
    return prog


def analyze_port_delayed(st, port, vscale, W_entries, u=None, t=0.0, **kw):
    """analyze_port for the matrix a delayed transient solves, G - W + a0 C.  ``W_entries``: [(row, col, w)] of the delayed stamps on the
    structure's indices.  The composite sample holds a delayed stamp as if it acted on the present state, and a pivot chosen on one --
    the gain entry of a line's E elements is the largest of its row -- is a pivot on an exact zero of G - W.  So the delayed positions of
    the sample are set to what G - W holds there, |G - W| on the port's stamps at ``u`` (zeros by default) and ``t``: a position filled
    only by delayed stamps is zero.  What BatchSimulator.analyze_delayed does on the GPU side, restated on the port's own stamps."""
    rowptr, colidx = np.asarray(st.rowptr), np.asarray(st.colidx)
    W = {}
    for r, c, w in W_entries:
        e = [q for q in range(rowptr[r], rowptr[r + 1]) if colidx[q] == c]
        assert len(e) == 1, (r, c)
        W[e[0]] = W.get(e[0], 0.0) + w
    pos = np.array(sorted(W), dtype=int)
    G = port.rebuild(np.zeros(st.n) if u is None else u, t)[0]
    left = np.abs(G[pos] - np.array([W[q] for q in pos]))
    return analyze_port(st, port, vscale, delayed=(pos, left), **kw)


def make_port_delayed(circ, params, temp, vscale, depth=0):
    """(st, port, terms): one instance on the port with its delayed stamps set and the pivot order of G - W.  The terms are the textbook
    reference's (tests/tran_delay_ref.delayed_terms), put on the product's indices by name through ``st.index_of``: nothing of them comes from
    api.ac_delay_overlay or BatchSimulator.delay_spec, which feed the GPU side only."""
    from tests import tran_delay_ref as DR
    st, port = make_port(circ, params, temp, "tran")
    terms = DR.delayed_terms(st, circ, params)
    port.set_delay(terms, depth)
    analyze_port_delayed(st, port, vscale, [(r, c, w) for r, c, w, _ in terms])
    return st, port, terms


def batch_tau_min(st, circ, params_list):
    """the smallest delay over the points of a batch, from the reference's terms: what cadnip_tran_run clamps hmax to"""
    from tests import tran_delay_ref as DR
    return min(tau for p in params_list for _, _, _, tau in DR.delayed_terms(st, circ, p))


def ec_breaks(st, circ, params_list, case):
    """the stop list of an error-controlled case, the same for both sides: none, or the sources' break points and their images"""
    from cadnip_jl_amd.structure import expand_breakpoints
    from tests import tran_delay_ref as DR
    if case["breaks"] is None:
        return []
    taus = [tau for p in params_list for _, _, _, tau in DR.delayed_terms(st, circ, p)]
    return list(api.delay_breakpoints(expand_breakpoints(st.breakpoints, case["tspan"]), taus, case["tspan"])[0])


def ec_save_times(case, breaks, n=33):
    """an even grid of n points, a point just after every break point (by a thousandth of the grid's spacing) and just after t0 + tau for the
    case's delays (``save_extra``)"""
    t0, t1 = case["tspan"]
    eps = (t1 - t0) / n * 1e-3
    ts = list(np.linspace(t0, t1, n)) + [b + eps for b in breaks if b + eps < t1] + [t0 + x + eps for x in case["save_extra"]]
    return np.unique(np.array(ts))


def port_ec_run(case, circ, params, temp, u0, hmax_batch, breaks, save_t, obs=None, depth=0, max_order=None, trace_cap=0):
    """one instance of an error-controlled delayed case on the port: (out, stats, accepted times).  ``hmax_batch``: the case's hmax clamped
    to the batch's smallest delay, as cadnip_tran_run clamps it (the port does not)."""
    from tests.tran_delay_cases import EC_ABSTOL
    st, port, terms = make_port_delayed(circ, params, temp, case["vscale"], depth)
    try:
        t0, t1 = case["tspan"]
        order = max_order or (case["max_order"] if isinstance(case["max_order"], int) else case["max_order"][0])
        out, _, stats, trace = port.tran(u0, t0, t1, st.state_abstol(**EC_ABSTOL), case["reltol"],
                                         breaks=breaks, save_t=save_t, obs=obs, err_mask=st.differential_mask(), h0=min(case["h0"], hmax_batch),
                                         hmax=hmax_batch, max_newton=case["max_newton"], max_order=order, use_pcnr=False, trace_cap=trace_cap)
        return out, stats, trace
    finally:
        port.close()


def dense_dc_start(circ, params, temp, abstol=1e-9, maxiters=100):
    """the tranop DC point of one instance by Newton with a dense pivoted solve on the port's stamps (the port's own PCNR loop, port_dc, with
    numpy's solve for the static-pivot LU: the line-into-inverter circuit's DC matrix meets an exact zero pivot under the composite order)"""
    st, port = make_port(circ, params, temp, "tranop")
    try:
        n, L = st.n, st.n_limits
        u = np.zeros(n)
        u[n - L:] = st.limit_init
        port.set_spec(initjct=1)
        settled = False
        for _ in range(2 * maxiters):
            G, _, b, lw = port.rebuild(u, 0.0)
            port.set_spec(initjct=0)
            A = np.zeros((n, n))
            for i in range(n):
                for q in range(st.rowptr[i], st.rowptr[i + 1]):
                    A[i, st.colidx[q]] += G[q]
            F = A @ u - b
            if np.sqrt(F @ F) < abstol:
                if L == 0 or settled:
                    return u
                u[n - L:], settled = lw, True
                continue
            settled = False
            u = u - np.linalg.solve(A, F)
            if L:
                u[n - L:] = lw
        raise RuntimeError("dense_dc_start: no convergence")
    finally:
        port.close()
