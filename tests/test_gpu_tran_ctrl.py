"""The transient step controller of csrc/tran_ctrl.hpp (prepare_step, tran_update_body, save_outputs), decision by decision on the device:
ONE call per case on a state of the test's choosing (tests/prim_probe.py: run_tran_ctrl), against the independent reference of
tests/tran_ctrl_ref.py on the cases of tests/tran_ctrl_cases.py -- for the per-op path's two group sizes (GlobalVecsT<64>, GlobalVecsT<256>)
and for the compile-time form the fused sweep kernel takes (V::FIXED), which must return the same bits as the runtime form.

Every launch is checked for untouched guard words behind every vector and sentinels in every word it must not write; every case of every
launch is compared (the tests count them); each test prints its worst error as a fraction of its bound.

Measured on an MI355X (worst |error| / bound over all cases; the bounds are derived in tests/tran_ctrl_ref.py): see DESIGN.md section 3.
"""
import functools

import numpy as np
import pytest

from tests import prim_probe as P
from tests import tran_ctrl_cases as Cs
from tests import tran_ctrl_ref as R

pytestmark = pytest.mark.gpu

SCALARS = P.TC_DS + P.TC_IS


@functools.lru_cache(maxsize=None)
def configs():
    return Cs.build()


@functools.lru_cache(maxsize=None)
def launch(idx, policy):
    """One launch of configuration ``idx`` under ``policy``; the guards and sentinels are checked here, on every launch."""
    cfg = configs()[idx]
    res = P.run_tran_ctrl(policy, cfg.op, cfg.sh, cfg.states(), cfg.vecs())
    assert (res["vec_guard"] == P.TC_GUARD_BITS).all(), "%s/%s: a guard word behind a vector was written" % (cfg.name, policy)
    assert (res["out_guard"] == np.uint64(0xFFFFFFFFFFFFFFFF)).all(), "%s/%s: a word behind out was written" % (cfg.name, policy)
    assert res["nactive"] == -1, "%s/%s: nactive was written" % (cfg.name, policy)
    return res


def instance(res, b):
    g = {k: res[k][b] for k in SCALARS + P.TC_VEC}
    g["cnt"], g["out"] = res["cnt"][b], res["out"][b]
    return g


@functools.lru_cache(maxsize=None)
def outcome(idx, b):
    """The reference's decision for one op-1 case: computed once, shared by the policies."""
    cfg = configs()[idx]
    k = cfg.cases[b]
    return R.update(cfg.sh, k.st, k.vec, k.flags & 1)


def _report(title, worst, n_cases, n_checked):
    print("\n%s: %d cases, %d comparisons, none skipped; worst |error| / bound per quantity:" % (title, n_cases, n_checked))
    for k in sorted(worst):
        if k == "h_next.ord2.rel":
            print("  %-16s %.3e relative (allowance 1.0e-07)" % ("h_next at order 2", worst[k]))
        elif worst[k] > 0.0:
            print("  %-16s %.3f" % (k, worst[k]))
    print("  exact (to the bit): " + " ".join(k for k in sorted(worst) if worst[k] == 0.0 and "[" not in k))


def _run(policy, op):
    worst, n_cases, n_checked, total = {}, 0, 0, 0
    for idx, cfg in enumerate(configs()):
        if cfg.op != op or policy not in cfg.policies:
            continue
        total += len(cfg.cases)
        res = launch(idx, policy)
        for b, case in enumerate(cfg.cases):
            g = instance(res, b)
            try:
                if op == 1:
                    ck = R.check_update_case(cfg.sh, case, g, outcome(idx, b), fixed=policy == "fixed")
                else:
                    ck = R.check_prepare_case(cfg.sh, case, g)
            except AssertionError as e:
                raise AssertionError("%s / %s: %s" % (cfg.name, policy, e)) from None
            assert ck.n_checked > 20
            for k, v in ck.worst.items():
                assert v <= 1.0
                worst[k] = max(worst.get(k, 0.0), v)
            n_cases += 1
            n_checked += ck.n_checked
    assert n_cases == total and total > 0, "cases left out of the comparison: %d of %d" % (total - n_cases, total)
    _report("%s, %s" % (policy, "tran_update_body" if op == 1 else "prepare_step"), worst, n_cases, n_checked)


@pytest.mark.parametrize("policy", ["g64", "g256", "fixed"])
def test_update_against_reference(policy):
    """tran_update_body + save_outputs + the prepare_step that follows, every row of the decision table and every edge."""
    _run(policy, 1)


@pytest.mark.parametrize("policy", ["g64", "g256", "fixed"])
def test_prepare_against_reference(policy):
    """prepare_step alone: clipping to the stops on its edges, the order from the history, coefficients, predictor, beta, du."""
    _run(policy, 0)


def test_fixed_form_returns_the_same_bits():
    """Every case with Newton mode 1, step rule 0, max_order 2, no PCNR and n <= 256 through V::FIXED and through GlobalVecsT<64> with those
    runtime values: every output bit-equal -- but du where the iteration continues, which the fixed form leaves to its caller (there it must
    be what it was)."""
    n_cases = total = n_cont = 0
    for idx, cfg in enumerate(configs()):
        if not cfg.fixed_form or "g64" not in cfg.policies:
            continue
        assert "fixed" in cfg.policies, cfg.name
        total += len(cfg.cases)
        a, f = launch(idx, "g64"), launch(idx, "fixed")
        for b, case in enumerate(cfg.cases):
            cont = cfg.op == 1 and outcome(idx, b).row == "continue"
            for k in SCALARS + ("cnt", "out") + P.TC_VEC:
                x, y = np.ascontiguousarray(a[k][b]), np.ascontiguousarray(f[k][b])
                if k == "du" and cont:
                    assert np.array_equal(R._bits(y), R._bits(case.vec["du"])), "%s / %s: the fixed form wrote du" % (cfg.name, case.name)
                    n_cont += 1
                    continue
                same = np.array_equal(R._bits(x), R._bits(y)) if x.dtype == np.float64 else np.array_equal(x, y)
                assert same, "%s / %s: %s differs between the fixed and the runtime form" % (cfg.name, case.name, k)
            n_cases += 1
    assert n_cases == total and total > 100 and n_cont >= 5
    print("\nfixed form: %d cases bit-equal to the runtime form (du left alone in %d continuing cases)" % (n_cases, n_cont))
