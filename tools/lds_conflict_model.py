#!/usr/bin/env python3
"""CPU model of the LDS bank conflicts of the pair sweep's Coulomb-table gather (numpy only; no GPU, no library).

    python tools/lds_conflict_model.py [--side 46.56] [--alpha 0.2346370178899813] [--cutoff-kelvin 1e-12] [--groups 6000]

A `ds_read_b128` is served per group of 16 lanes; the 256-byte bank row holds 16 slots of 16 bytes, and two lanes of a group
conflict when they read DIFFERENT addresses in the same slot column (identical addresses are one broadcast).  A group then
takes as many cycles as its fullest column holds distinct addresses.  The table row of a lane is (exponent | top 6
mantissa bits) of its r^2, 48 bytes per row, so sixteen random rows land on sixteen random columns: the model draws
uniform random pairs in the cubic box (minimum image), applies the engine's row index and counts that maximum.

Variants: every lane its own row (the table before the shared far row); lanes beyond the distance at which
167101 K A * erfc(alpha r)/r <= cutoff share ONE row (build_coulomb_table); and, for the record, C row-interleaved copies
of the table with lane l reading copy l mod C (measured worthless once the far row is shared; 8 copies do not fit LDS).
Prints the table profiles/r23/README.md quotes, and 1 - 1/cycles, the modelled share of conflict cycles.
"""
import argparse
import math

import numpy as np

KELVIN = 167101.0
ROW_BYTES, SLOT_BYTES, SLOTS, GROUP = 48, 16, 16, 16


def row_index(r2):
    """(hi32(r^2) >> 14): binary exponent and top 6 mantissa bits, as coul_lds forms it."""
    return (np.asarray(r2, dtype=np.float64).view(np.uint64) >> np.uint64(32 + 14)).astype(np.int64)


def far_index(alpha, cutoff_kelvin):
    """index and r of the first row start at which a term of unit charge product is worth <= cutoff_kelvin"""
    for e in range(-2, 20):
        for q in range(64):
            s = 2.0 ** e * (1.0 + q / 64.0)
            if KELVIN * math.erfc(alpha * math.sqrt(s)) / math.sqrt(s) <= cutoff_kelvin:
                return int(row_index(np.array([s]))[0]), math.sqrt(s)
    raise SystemExit("no far row below r^2 = 2^20")


def cycles_per_group(rows, copies):
    """mean over groups of the fullest slot column's count of distinct addresses; rows: (groups, 16)"""
    lane = np.arange(GROUP)[None, :]
    addr = (rows * copies + lane % copies) * ROW_BYTES            # first of the row's three reads; the others shift every lane alike
    col = (addr // SLOT_BYTES) % SLOTS
    worst = np.zeros(rows.shape[0], dtype=np.int64)
    for c in range(SLOTS):
        a = np.where(col == c, addr, -1)
        a.sort(axis=1)
        distinct = (np.diff(a, axis=1) != 0).sum(axis=1) + 1 - (a[:, 0] == -1)      # (-1 is not an address)
        worst = np.maximum(worst, distinct)
    return float(worst.mean())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=float, default=46.56, help="cubic box side, A")
    ap.add_argument("--alpha", type=float, default=0.2346370178899813)
    ap.add_argument("--cutoff-kelvin", type=float, default=1e-12, help="a far term's worth per unit charge product, K")
    ap.add_argument("--groups", type=int, default=6000)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--lds-kib", type=float, default=160.0)
    a = ap.parse_args()
    rng = np.random.default_rng(a.seed)
    d = rng.uniform(-a.side / 2, a.side / 2, (a.groups, GROUP, 3))     # separation of two uniform points, folded = uniform in the cell
    r2 = (d * d).sum(axis=2)
    rows = row_index(r2)
    i_far, r_far = far_index(a.alpha, a.cutoff_kelvin)
    base = int(row_index(np.array([0.25]))[0])
    # whole octaves up to that of the half diagonal squared, and the clamp row (build_coulomb_table)
    n_rows = (int(row_index(np.array([0.75 * a.side ** 2 * 1.0001]))[0]) - base) // 64 * 64 + 64 + 1
    far = np.minimum(rows, i_far)
    print(f"box side {a.side} A, alpha {a.alpha}: far row from r = {r_far:.2f} A, {np.mean(rows >= i_far) * 100:.1f} % of pairs beyond it; "
          f"table {n_rows} rows = {n_rows * ROW_BYTES / 1024:.1f} KiB, shared: {i_far - base + 1} rows")
    print("| far lanes | table copies | cycles per 16-lane group | conflict share |")
    print("|---|---|---|---|")
    for label, r, copies in [("own rows", rows, 1), (f"share one row beyond {r_far:.1f} A", far, 1), ("own rows", rows, 4),
                             (f"share one row beyond {r_far:.1f} A", far, 4), ("own rows", rows, 8)]:
        c = cycles_per_group(r - base, copies)
        fits = "" if n_rows * ROW_BYTES * copies <= a.lds_kib * 1024 else " (does not fit LDS)"
        print(f"| {label} | {copies}{fits} | {c:.2f} | {100 * (1 - 1 / c):.0f} % |")


if __name__ == "__main__":
    main()
