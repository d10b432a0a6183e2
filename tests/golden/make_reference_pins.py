"""Store the compiled reference's answers to the calls of tests/test_oracle_pin.py's live pins
(moves_trace on each of PIN_MAKERS, small_functions_trace on PIN_SMALL) as tests/golden/reference_pins.npz,
so that the pins hold the C restatement to the reference without a reference build.

Runs only where oracle/_ref exists (needs the reference sources + amdflang at build time).

    python tests/golden/make_reference_pins.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from oracle import reflib  # noqa: E402
from tests.test_oracle_pin import PIN_MAKERS, PIN_SMALL, moves_trace, small_functions_trace  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "reference_pins.npz")


def main():
    arrays = {}
    for i, maker in enumerate(PIN_MAKERS):
        s = maker()
        arrays.update(moves_trace(reflib.Reference(s), s).arrays(f"case{i}"))
    s = PIN_SMALL()
    arrays.update(small_functions_trace(reflib.Reference(s), s).arrays("small"))
    np.savez_compressed(OUT, **arrays)
    print(f"{OUT}: {len(arrays)} arrays, {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
