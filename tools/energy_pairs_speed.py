#!/usr/bin/env python3
"""The energy by residue-type pair of R replicas against the whole-system energy of the same replicas (not part of the
test-suite).

    python tools/energy_pairs_speed.py [--replicas 64,512] [--repeats 7] [--warmup 2]

Per shape and chain count, alternating in one process: one Engine.energy_pairs_replicas call against one
Engine.system_energy_replicas call (the yardstick: it visits the same pair terms); the first --warmup rounds are discarded,
each point is the median over --repeats rounds, in milliseconds, with the smallest and largest round beside it.  Shapes:
spce_box(10) with its one pair; framework_water_box() with the default selection (guest-framework + guest-guest) and with all
three pairs.  One JSON line per point."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from maniac_mc_amd import energy_pairs, synth  # noqa: E402
from maniac_mc_amd.engine import Engine  # noqa: E402


def shapes():
    spce = synth.spce_box(10)
    fw = synth.framework_water_box()
    return [("spce1000 one pair", spce, [(0, 0)]),
            ("framework_water default (guest-framework, guest-guest)", fw, energy_pairs.default_pairs(fw.topo)),
            ("framework_water all three pairs", fw, [(0, 0), (0, 1), (1, 1)])]


def measure(name, s, pairs, R, warmup, repeats):
    eng = Engine.from_system(s, n_replicas=R)
    try:
        eng.synchronize()
        t_pairs, t_total = [], []
        for i in range(warmup + repeats):
            t0 = time.perf_counter()
            got = eng.energy_pairs_replicas(pairs)
            t1 = time.perf_counter()
            total = eng.system_energy_replicas()
            t2 = time.perf_counter()
            if i >= warmup:
                t_pairs.append(t1 - t0)
                t_total.append(t2 - t1)
        ms = lambda v: dict(median=round(1e3 * float(np.median(v)), 3), min=round(1e3 * min(v), 3), max=round(1e3 * max(v), 3))
        p, t = ms(t_pairs), ms(t_total)
        return dict(shape=name, atoms=int(sum(int(n) * int(a) for n, a in zip(s.n_mol, s.topo.atoms_in_res))), nk=int(eng.nk),
                    replicas=R, pairs=[list(ab) for ab in pairs], energy_pairs_ms=p, system_energy_ms=t,
                    ratio=round(p["median"] / t["median"], 3),
                    non_coulomb_sum_minus_total=float(np.max(np.abs(got[:, :, 0].sum(axis=1) - total[:, 0])))
                    if len(pairs) == s.topo.n_res * (s.topo.n_res + 1) // 2 else None)
    finally:
        eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replicas", default="64,512")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    for name, s, pairs in shapes():
        for R in [int(v) for v in a.replicas.split(",")]:
            print(json.dumps(measure(name, s, pairs, R, a.warmup, a.repeats)), flush=True)


if __name__ == "__main__":
    main()
