#!/usr/bin/env python3
"""Write tests/golden/prim_*.npz: the inputs and the mpmath (60 digits) references of the device-side primitives whose truth is not
exactly computable in doubles (tests/prim_ref.py: BUILDERS).  The GPU tests read these files, so they need no mpmath;
tests/test_prim_ref_cpu.py rebuilds every array and compares it with the files bit for bit.

    python tools/make_prim_fixtures.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import prim_ref as R  # noqa: E402


def main():
    total = 0
    for name, build in R.BUILDERS.items():
        path = R.fixture_path(name)
        np.savez_compressed(path, **build())
        total += os.path.getsize(path)
        print("%-16s %7d bytes" % (name, os.path.getsize(path)))
    print("total %d bytes" % total)


if __name__ == "__main__":
    main()
