"""Delayed transients on the GPU under error control (csrc/delay.hip, the clamp and the DelayGuard of cadnip_tran_run) against the CPU port with
delays (oracle/cpu_port.cpp: port_set_delay), step for step -- the way tests/test_gpu_tran_parity.py holds the undelayed paths:
``err_mask="differential"`` on the GPU and ``st.differential_mask()`` on the port, test_gpu_tran_parity's ABSTOL, every saved unknown within
REL_TOL = 1e-9 relative to max(|ref|, 1), equal (Newton, accepted, rejected, status) per instance; the port starts from the GPU's start state.
The port's terms are the textbook reference's (tests/tran_delay_ref.delayed_terms through ``st.index_of``), the GPU's are the product's
(``BatchSimulator.delay_spec``); the port is told the clamped ``hmax`` (min(hmax, smallest delay of the BATCH)), the GPU the unclamped one.
The cases and why they reject, land and fail: tests/tran_delay_cases.ec_case; that they do, on the port alone: tests/test_tran_delay_port_cpu.py.

What each test would catch in a copy of the kernels with one line wrong (read, not run):
* ``>=`` for ``>`` in k_delay_record's acceptance test: every round that is no accepted step (t still equal to the ring's newest time: a Newton
  round that goes on, a rejected step, a Newton failure) appends a duplicate of the newest point.  The bracket search takes the LAST point at or
  below tq, so the values stay the same -- what changes is the capacity: the duplicates push accepted points off the ring.  test_ring_depth: at
  depth = D* (the port's count of ACCEPTED points) instance 1 overflows instead of being bit-equal to the default depth;
* ``blockIdx.x * 64`` -> ``* 32`` in k_delay_init or k_delay_record: three blocks then reach instances 0 .. 127 only; 128 .. 130 keep a zeroed ring
  (count 0: every look-up is the zero start value) or never record (every look-up is the start value): test_batch_of_131, instances 128 and 130.
  ``* 256`` -> ``* 128`` in k_delay_apply: threads 128 .. 255 of the id space run twice (G - 2 W for the buffer's instances 64 .. 127, ghf's 21 .. 42)
  and, with ghf's four blocks, ids from 640 (instance 107) on never: test_batch_of_131, instances 42, 64, 127, 128, 130;
* k_delay_apply's look-up at ``tcur`` replaced by the accepted time, or its value kept from the failed attempt: test_step_for_step_parity
  [buffer_sin] (62 rejected steps) and [line_inverter_tight_newton] (5 retries at h / 4);
* k_delay_clear or the DelayGuard dropped: test_handle_leaves_clean, b after the run -- on the successful exit the stored rows hold the arrived
  wave, on the CADNIP_NOCONV exit -w v_init of a non-zero start state (asserted non-zero there, from the spec and the start state);
* the overflow surfaced after k_tran_update again: test_ring_depth, one Newton round more than the port.
Not observable, and so held by no test: k_delay_apply's ``active / status`` guard.  In a transient the activity mask IS status == 0
(tran_ctrl.hpp: store_state), so the guard only keeps the kernel off instances that have ended, whose G and b nothing reads again (the next
rebuild rewrites them, k_delay_clear zeroes the stored rows); without it the results are the same bits.

The measured figures: DESIGN.md section 9."""
import functools

import numpy as np
import pytest

from cadnip_jl_amd import api, hip
from tests import port_util as PU
from tests import tran_delay_cases as K
from tests.test_gpu_tran_parity import REL_TOL, ABSTOL

pytestmark = pytest.mark.gpu
TD = K.TD
assert ABSTOL == K.EC_ABSTOL


def _points(case, B):
    return [case["points"][i % len(case["points"])] for i in range(B)]


def _order(case, order):
    return order or (case["max_order"] if isinstance(case["max_order"], int) else case["max_order"][0])


@functools.lru_cache(maxsize=None)
def _gpu(name, B=None, order=None, depth=0, fused=False):
    """the case on the GPU, controller on: dict(out [B, S, n], per [B, 4], stats, u0, st, breaks, ts, hb = the clamped hmax the port is told, shape =
    (n_pos, n_rows, n_taps) of the handle's plan)"""
    case = K.ec_case(name)
    pts = _points(case, B or len(case["points"]))
    circ = case["make"]()
    sim = api.BatchSimulator(api.MNACircuit(circ, case["base"]), pts)
    try:
        st = sim.st
        sim.analyze()
        if case["start"] == "dc":
            u0, conv, _ = sim.dc(abstol=1e-9, mode="tranop")
            assert np.all(conv)
        else:
            u0 = np.zeros((sim.B, st.n))
        params = [K.ec_point(case, i)[0] for i in range(len(pts))]
        breaks = PU.ec_breaks(st, circ, params, case)
        ts = PU.ec_save_times(case, breaks)
        hb = min(case["hmax"], PU.batch_tau_min(st, circ, params))
        sim.h.set_spec(mode="tran")
        sim.h.set_u(u0)
        spec = sim.delay_spec()
        sim.h.tran_set_delay(depth=depth, **spec)
        sim.analyze_delayed(spec, case["tspan"][0])
        out, per, stats = sim.h.tran_run(case["tspan"][0], case["tspan"][1], st.state_abstol(**ABSTOL), case["reltol"], breaks=breaks, save_t=ts, h0=case["h0"],
                                         hmax=case["hmax"], max_newton=case["max_newton"], max_order=_order(case, order), fused=fused, err_mask="differential")
        info = sim.h.tran_delay_info()                                 # the plan the handle built: what the kernels index by, not the spec's own counts
        shape = (info["n_pos"], info["n_rows"], info["n_taps"])
        assert info["n_term"] == len(spec["term_pos"]) and info["depth"] == (depth or 1024)
        return dict(out=out, per=per, stats=stats, u0=u0, st=st, breaks=breaks, ts=ts, hb=hb, shape=shape, vscale=sim.vscale())
    finally:
        sim.close()


@functools.lru_cache(maxsize=None)
def _port(name, setting, hb, order=None, depth=0, u0=None):
    """(out, stats, accepted times) of one setting of the case on the port; ``u0``: the start state as a tuple (None: zeros)"""
    case = K.ec_case(name)
    circ = case["make"]()
    params, temp = K.ec_point(case, setting)
    all_params = [K.ec_point(case, i)[0] for i in range(len(case["points"]))]
    st = PU.cj.discover(circ, params)
    breaks = PU.ec_breaks(st, circ, all_params, case)
    start = np.zeros(st.n) if u0 is None else np.array(u0)
    return PU.port_ec_run(case, circ, params, temp, start, hb, breaks, PU.ec_save_times(case, breaks), depth=depth, max_order=_order(case, order), trace_cap=100000)


def _assert_parity(name, g, i, order=None, depth=0, upto=None):
    """instance i of the GPU run ``g`` against the port: the four per-instance numbers equal, every saved unknown within REL_TOL; returns
    (error, port stats, port's accepted times).  ``upto``: compare the save times up to this time only."""
    case = K.ec_case(name)
    u0 = tuple(g["u0"][i]) if case["start"] == "dc" else None
    ref, rst, trace = _port(name, i % len(case["points"]), g["hb"], order, depth, u0)
    per = g["per"][i]
    assert (per[0], per[1], per[2], per[3]) == (rst["newton_iters"], rst["accepted"], rst["rejected"], rst["status"]), (name, i, per.tolist(), rst)
    keep = slice(None) if upto is None else g["ts"] <= upto
    err = float(np.max(np.abs(g["out"][i][keep] - ref[keep]) / np.maximum(np.abs(ref[keep]), 1.0)))
    assert err <= REL_TOL, (name, i, err)
    return err, rst, trace


# ---- a. step-for-step parity ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,order", [("buffer_sin", 2), ("ghf", 2), ("ghf", 3), ("line_inverter_breaks", 2), ("line_inverter_tight_newton", 2)])
def test_step_for_step_parity(name, order):
    case = K.ec_case(name)
    g = _gpu(name, order=order)
    assert np.all(g["per"][:, 3] == 1), g["per"].tolist()
    # the save times hold points just after every break point and just after t0 + tau
    eps = (case["tspan"][1] - case["tspan"][0]) / 33 * 1e-3
    for b in list(g["breaks"]) + list(case["save_extra"]):
        assert b + eps >= case["tspan"][1] or np.any(np.isclose(g["ts"], b + eps, rtol=0.0, atol=eps / 4)), b
    worst, landed, fails = 0.0, [], 0
    for i in range(len(case["points"])):
        err, rst, trace = _assert_parity(name, g, i, order)
        worst = max(worst, err)
        landed.append(len(set(trace.tolist()) & set(g["breaks"])))
        fails += rst["newton_failures"]
        assert rst["delay_need"] >= 3
    print("%s order %d: worst error against the port %.2e; per %s; landed %s; newton failures %d" % (name, order, worst, g["per"].tolist(), landed, fails))
    assert g["stats"]["newton_failures"] == fails                      # (per instance the GPU reports no failure count: the batch's sum)
    # the claimed event happened, on the GPU's own counters (equal to the port's above)
    if name == "buffer_sin":
        assert np.max(g["per"][:, 2]) >= 1                             # rejected steps, a retry re-reads the history at a new tn
        assert g["hb"] == TD / 32 < case["hmax"]                        # and the clamp binds: the port was told hb, the GPU hmax = TD
    if name == "line_inverter_breaks":
        assert min(landed) >= 3 and np.all(g["per"][:, 0] > 2 * g["per"][:, 1])     # landings (order-1 restarts) and several rounds on one delayed value
    if name == "line_inverter_tight_newton":
        assert case["max_newton"] == 3 and fails >= 1                   # a retry at h / 4 re-evaluates ud(tn - tau)


def test_fused_flag_changes_nothing():
    """a handle with a delay spec runs per-op whatever ``fused`` says: bit-equal"""
    a, b = _gpu("buffer_sin", order=2), _gpu("buffer_sin", order=2, fused=True)
    assert np.array_equal(a["out"], b["out"]) and np.array_equal(a["per"], b["per"])


# ---- b. batch shapes -----------------------------------------------------------------------------------------------------------------------------
def _straddler(shape):
    """the instance whose k_delay_apply threads lie on both sides of the first 256-thread block boundary, or None when the boundary falls between two"""
    per = shape[0] + shape[1]
    return None if 256 % per == 0 else 256 // per


@pytest.mark.parametrize("name", ["ghf_five", "buffer_sin_five"])
def test_batch_of_131(name):
    B = 131
    g = _gpu(name, B=B)
    n_pos, n_rows, n_taps = g["shape"]
    # a second block of each kernel: k_delay_init (64 threads over B n_taps), k_delay_apply (256 over B (n_pos + n_rows)), k_delay_record (64 over B)
    assert B * n_taps > 64 and B * (n_pos + n_rows) > 256 and B > 64
    assert np.all(g["per"][:, 3] == 1)
    for i in range(5, B):                                               # same setting, same bits
        assert np.array_equal(g["out"][i], g["out"][i % 5]) and np.array_equal(g["per"][i], g["per"][i % 5]), i
    assert len({g["per"][i].tobytes() for i in range(5)}) == 5          # and the five settings are five different runs
    checked = [0, 63, 64, 127, 128, 130]
    if name == "ghf_five":
        assert (n_pos, n_rows) == (3, 3) and _straddler(g["shape"]) == 42       # threads 252 .. 257: blocks 0 and 1
        checked.append(42)
    else:
        assert (n_pos, n_rows) == (1, 1) and _straddler(g["shape"]) is None     # the boundary falls between instances 127 and 128
    worst = max(_assert_parity(name, g, i)[0] for i in checked)
    print("%s B = 131: worst error against the port %.2e over instances %s" % (name, worst, checked))


@pytest.mark.parametrize("B", [1, 65])
def test_buffer_sin_at_other_batch_sizes(B):
    """the same hmax; the clamp is the batch's: B = 1 has tau = 0.75 TD alone, B = 65 holds the smallest delay"""
    g = _gpu("buffer_sin_five", B=B)
    assert g["hb"] == (0.75 * TD if B == 1 else TD / 32)
    assert np.all(g["per"][:, 3] == 1)
    worst = max(_assert_parity("buffer_sin_five", g, i)[0] for i in sorted({0, B // 2, B - 2 if B > 1 else 0, B - 1}))
    print("buffer_sin B = %d: worst error against the port %.2e" % (B, worst))


# ---- c. ring depth under error control ---------------------------------------------------------------------------------------------------------
def test_ring_depth():
    """The overflow round.  k_delay_apply meets the look-up that fell off the ring BEFORE the round is solved and ends the instance there (status,
    activity mask): k_tran_update returns at once on a status that is not 0 (driver.hip: ``if (s.status != 0) return``), so the flagged round moves no
    counter, no t, no history vector and no save slot -- the counts are the port's, which stops at the same look-up, exactly.  (Before this was so,
    the status was set by k_delay_record AFTER k_tran_update had run the round on a right-hand side with the term dropped: one Newton round more
    than the port, and, where that round's update happened to pass the convergence and error tests, an accepted step and save values computed
    without the term.)"""
    name = "buffer_sin_depth"
    g = _gpu(name)
    need = [_port(name, i, g["hb"])[1]["delay_need"] for i in range(3)]
    D = need[1]
    assert D == max(need) and D - 1 > max(need[0], need[2]) and D >= 3, need           # instance 1 has the longest delay in steps
    at = _gpu(name, depth=D)
    assert np.array_equal(at["out"], g["out"]) and np.array_equal(at["per"], g["per"])
    short = _gpu(name, depth=D - 1)
    assert short["per"][:, 3].tolist() == [1, hip.TRAN_DELAY_OVERFLOW, 1]
    for i in (0, 2):
        assert np.array_equal(short["out"][i], g["out"][i]) and np.array_equal(short["per"][i], g["per"][i])
    _, rst, trace = _port(name, 1, g["hb"], depth=D - 1)
    assert rst["status"] == -4 == hip.TRAN_DELAY_OVERFLOW and 0 < rst["accepted"] < g["per"][1, 1]
    # Newton rounds, accepted and rejected steps and the status equal the port's: the flagged round is inert; the values up to the last accepted time
    err, _, _ = _assert_parity(name, short, 1, depth=D - 1, upto=trace[-1])
    print("ring depth: D* = %d (needs %s), overflow after %d accepted steps, error up to then %.2e" % (D, need, rst["accepted"], err))


# ---- d. the handle leaves clean --------------------------------------------------------------------------------------------------------------------
def test_handle_leaves_clean():
    """After a delayed run -- one that succeeds, one that ends in CADNIP_NOCONV through an overflow -- and tran_clear_delay the handle stamps what a new
    handle stamps, to the bit: the row of b that only k_delay_apply writes (the line's branch rows have no device stamp: row_store = 1) is cleared on
    both exits (DelayGuard, k_delay_clear), and an undelayed transient on it is the new handle's.  Both runs leave something to clear: the successful
    one the arrived wave; the overflowing one starts from a non-zero state, so that until its look-up leaves the pre-history (td >= TD, steps <= TD / 8:
    every look-up before the overflow is the start value) k_delay_apply stores -sum w v_init, which is asserted non-zero for every stored row."""
    make = lambda: K.line(K.pwl_ramp(0.3 * TD, 0.9 * TD), 30.0, 100.0)
    pts = [{"td": TD}, {"td": 2.5 * TD}, {"td": 1.5 * TD}]
    rng = np.random.default_rng(7)
    tspan, ts = (0.0, 6 * TD), np.linspace(0.0, 6 * TD, 25)

    def undelayed(sim):
        """the circuit with its gains acting at once (no spec on the handle): td is irrelevant"""
        sim.h.set_spec(mode="tran")
        sim.h.set_u(np.zeros((sim.B, sim.st.n)))
        return sim.h.tran_run(tspan[0], tspan[1], 1e-9, 1e-6, breaks=(), save_t=ts, hmax=TD / 8, fused=False)[:2]

    fresh = api.BatchSimulator(api.MNACircuit(make(), {"td": TD}), pts)
    used = api.BatchSimulator(api.MNACircuit(make(), {"td": TD}), pts)
    try:
        st = fresh.st
        u = rng.standard_normal((3, st.n))
        fresh.analyze()
        fresh.h.rebuild(u, 0.7 * TD)
        want = fresh.h.get_GCb()
        out_f, per_f = undelayed(fresh)
        used.analyze()
        spec = used.delay_spec()
        stored = sorted({int(r) for r in spec["term_row"] if st.b_ptr[r + 1] == st.b_ptr[r]})       # rows of b that no device stamps
        assert stored and len(stored) == len(set(spec["term_row"].tolist()))
        start_nz = 0.5 + rng.random((3, st.n))
        for depth, status in ((0, [1, 1, 1]), (2, [hip.TRAN_DELAY_OVERFLOW] * 3)):
            start = np.zeros((3, st.n)) if depth == 0 else start_nz
            used.h.set_spec(mode="tran")
            used.h.set_u(start)
            used.h.tran_set_delay(depth=depth, **spec)
            base = used.analyze_delayed(spec, 0.0)
            out, per, stats = used.h.tran_run(tspan[0], tspan[1], 1e-9, 1e-6, breaks=(), save_t=ts, hmax=TD / 8, fused=False)
            assert per[:, 3].tolist() == status and stats["n_failed"] == (0 if depth == 0 else 3), per.tolist()
            if depth == 0:
                assert np.max(np.abs(out[:, :, st.index_of("p2")])) > 0.5            # the wave arrived: the delayed rows of b were written
            else:
                # what k_delay_apply stored in every solved round up to the overflow: -sum w v_init per stored row, not zero; and rounds were solved
                left = np.array([[sum(spec["w"][i, t] * start[i, spec["term_col"][t]] for t in range(len(spec["term_row"])) if spec["term_row"][t] == r)
                                  for r in stored] for i in range(3)])
                assert np.all(np.abs(left) > 0.1) and np.all(per[:, 1] >= 1), (left, per.tolist())
            used.h.tran_clear_delay()
            used.h.analyze_values(base)
            used.h.rebuild(u, 0.7 * TD)
            got = used.h.get_GCb()
            for a, b in zip(got, want):
                assert np.array_equal(a, b), depth
        out_u, per_u = undelayed(used)
        assert np.array_equal(out_u, out_f) and np.array_equal(per_u, per_f)
        assert np.all(per_f[:, 3] == 1), per_f.tolist()
    finally:
        fresh.close()
        used.close()
