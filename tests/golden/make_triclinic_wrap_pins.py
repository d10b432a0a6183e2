"""Writes tests/golden/triclinic_wrap_pins.npz: per cell of tests/triclinic_cases.py, the sha256 of the compiled reference's
ApplyPBC (src/geometry_utils.f90:167-220) over tests.triclinic_cases.wrap_inputs.  Needs oracle/_ref/libmaniac_ref.so.

    python tests/golden/make_triclinic_wrap_pins.py
"""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import reflib  # noqa: E402
from tests import triclinic_cases as tc  # noqa: E402


def main():
    out = {}
    for name in tc.CELLS:
        s = tc.cell(name)
        R = reflib.Reference(s)
        pts = tc.wrap_inputs(s)
        wrapped = np.array([R.apply_pbc(p) for p in pts])
        R.close()
        out[name] = np.array(hashlib.sha256(np.ascontiguousarray(wrapped).tobytes()).hexdigest())
        out[name + "_n"] = np.array(len(pts))
    np.savez(os.path.join(ROOT, "tests", "golden", "triclinic_wrap_pins.npz"), **out)
    print({k: str(v) for k, v in out.items()})


if __name__ == "__main__":
    main()
