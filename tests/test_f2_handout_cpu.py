"""tools/handout_replay.py: the replay of the sweep kernel's hand-out of instances to waves on per-instance round counts (DESIGN.md section 9,
round 7), held to count vectors whose optimum is known.  No GPU.

(The ranking header this file was meant to cover as well left the tree with the hand-out order itself, which measured no gain: DESIGN.md
section 9, round 7, "did not help".)"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _replay():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import handout_replay as hr
    finally:
        sys.path.pop(0)
    return hr


def test_replay_on_a_count_vector_with_a_known_optimum():
    """Two waves, four instances of 100, 100, 100, 300 rounds.  One launch: in index order the waves take 100 and 100, then the third 100 and the
    300 -- 400 rounds; most rounds left first gives one wave the 300 and the other the three 100s -- 300, the ideal 600 / 2.  With a budget of
    200 rounds per launch: index order 200 (the 300 is cut after 100 rounds) + 200 (its rest, alone); the oracle order 200 (the 300 cut after
    200, two 100s on the other wave) + 100 (the rest and the last 100 side by side)."""
    hr = _replay()
    rounds = np.array([100, 100, 100, 300])
    assert hr.makespans(rounds, 2, 10 ** 6) == {"index": 400, "oracle": 300, "ideal": 300.0}
    assert hr.makespans(rounds, 2, 200) == {"index": 400, "oracle": 300, "ideal": 300.0}
    # one wave: the order cannot matter
    assert hr.makespans(rounds, 1, 10 ** 6) == {"index": 600, "oracle": 600, "ideal": 600.0}


def test_replay_of_paired_instances_is_the_worst_pair():
    """Twice as many instances as waves and a budget no instance exhausts: every wave gets a pair, index order pairs i with i + waves, and the
    makespan is the worst pair -- the benchmark's situation (4096 instances on 2048 waves)."""
    hr = _replay()
    rounds = np.array([10, 20, 30, 40, 40, 30, 20, 100])          # pairs in index order: (10, 40) (20, 30) (30, 20) (40, 100)
    m = hr.makespans(rounds, 4, 10 ** 6)
    assert m["index"] == 140 and m["oracle"] == 100 and m["ideal"] == 72.5


def test_replay_resumes_an_unfinished_instance_in_the_next_launch():
    hr = _replay()
    assert hr.makespans(np.array([250]), 1, 100) == {"index": 250, "oracle": 250, "ideal": 250.0}
    assert hr.makespans(np.array([250, 50]), 2, 100)["index"] == 250      # 100 + 100 + 50: the second wave idles after its 50 rounds
