"""Replay of the sweep kernel's hand-out of instances to waves (csrc/fused2_kernel.hpp: k_fused2), on per-instance Newton round counts.  No GPU.

    python tools/handout_replay.py DUMP_DIR/tran_per_instance.npy [--waves 2048] [--budget 1024]

tran_per_instance.npy is what `bench.py --dump-outputs DUMP_DIR` writes; column 0 is an instance's transient Newton rounds.  The model: `waves`
resident waves, each with `budget` rounds per launch.  A launch gives slot s to wave s for s < waves and further slots to whichever wave is free
first; a wave works through its instances one after the other, an instance that is not finished when the budget runs out keeps its state and
is resumed by a later launch; a launch lasts as long as its busiest wave.  Printed: the makespan in rounds (the sum of the launches' lengths) for
  index order   slot s of a launch is the s-th unfinished instance in index order (the kernel without a hand-out order),
  oracle order  ... the unfinished instance with the s-th most rounds left (no kernel knows that),
  ideal         total rounds / waves.
For the benchmark's dump at 2048 waves and 1024 rounds: 4003 / 3859 / 3840.2."""
import argparse
import heapq

import numpy as np


def replay(rounds, waves, budget, key):
    """Makespan in rounds.  ``key(left, index)``: sort key of an unfinished instance at a launch seam (smallest first)."""
    left = [int(r) for r in rounds]
    total = 0
    while True:
        live = sorted((i for i in range(len(left)) if left[i] > 0), key=lambda i: key(left[i], i))
        if not live:
            return total
        # (rounds used, wave): the wave that is free first takes the next slot; resident slots go to their own wave at time 0
        heap = [(0, w) for w in range(waves)]
        heapq.heapify(heap)
        longest = 0
        for inst in live:
            used, w = heapq.heappop(heap)
            if used >= budget:                       # every wave is out of budget: the rest waits for the next launch
                heapq.heappush(heap, (used, w))
                break
            done = min(left[inst], budget - used)
            left[inst] -= done
            used += done
            longest = max(longest, used)
            heapq.heappush(heap, (used, w))
        total += longest


def makespans(rounds, waves, budget):
    return {"index": replay(rounds, waves, budget, lambda left, i: i), "oracle": replay(rounds, waves, budget, lambda left, i: (-left, i)),
            "ideal": float(np.sum(rounds)) / waves}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("per_instance")
    ap.add_argument("--waves", type=int, default=2048)
    ap.add_argument("--budget", type=int, default=1024)
    a = ap.parse_args()
    per = np.load(a.per_instance)
    rounds = np.asarray(per[:, 0] if per.ndim == 2 else per, dtype=np.int64)
    m = makespans(rounds, a.waves, a.budget)
    print("instances %d  rounds %d  min %d  max %d  mean %.1f  std %.1f" % (len(rounds), rounds.sum(), rounds.min(), rounds.max(), rounds.mean(), rounds.std()))
    print("waves %d  budget %d" % (a.waves, a.budget))
    print("index order  %d" % m["index"])
    print("oracle order %d" % m["oracle"])
    print("ideal        %.1f" % m["ideal"])


if __name__ == "__main__":
    main()
