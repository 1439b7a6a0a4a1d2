#!/usr/bin/env python3
"""Write tests/golden/launch_plans.json: what fused2_plan and the plan of launch_factor_solve choose for the matrix of tests/plan_cases.py,
read from the library's own reports (the `[cadnip f2]` lines of CADNIP_F2_DEBUG=1, the ``info`` of ``Handle.factor_solve``), together with
the compute-unit count of the device they were chosen for.  Needs the GPU.  Run it at the commit whose plans are to be kept -- a change
that means to leave every plan as it is runs it at its parent and commits the file unchanged; tests/test_gpu_launch_plan.py compares.

    python tools/make_plan_fixtures.py [output file]
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import plan_cases as P  # noqa: E402


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else P.FIXTURE
    doc = {"n_cu": P.device_cus(), "cases": {}}
    for name, B in P.CASES:
        doc["cases"]["%s/%d" % (name, B)] = P.record(name, B)
        print("%s/%d" % (name, B), flush=True)
    with open(path, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print("%s: %d bytes" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
