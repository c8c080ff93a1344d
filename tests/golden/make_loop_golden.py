#!/usr/bin/env python3
"""Generates tests/golden/reference_loop.npz: what the REFERENCE's own FBstabAlgorithm<> loop returns on
tests/helpers.py:reference_loop_cases - z, l, v, y and the SolverOut fields of every QP of every case,
as `<case>_<name>` arrays.  The outputs come from oracle/_ref/libfbstab_ref.so, the oracle's components
driven by the reference's loop template (oracle/Makefile: `make ref`), so this only runs where the
reference tree is present; tests/test_oracle.py pins the restated loop on the stored outputs bit for bit.

Usage: python tests/golden/make_loop_golden.py
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from oracle.oracle_py import Oracle  # noqa: E402
from tests import helpers as H  # noqa: E402


def main():
    kats = json.load(open(os.path.join(HERE, "reference_kats.json")))
    ref = Oracle(True)
    arrays = {}
    for i, (kind, p, o) in enumerate(H.reference_loop_cases(kats)):
        r = H.solve_case(ref, kind, p, o)
        for j, n in enumerate("zlvy"):
            arrays["%d_%s" % (i, n)] = r[j]
        for f in H.LOOP_FIELDS:
            arrays["%d_%s" % (i, f)] = r[4][f]
    np.savez_compressed(os.path.join(HERE, "reference_loop.npz"), **arrays)
    print("wrote", len(arrays), "arrays")


if __name__ == "__main__":
    main()
