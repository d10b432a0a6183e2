#!/usr/bin/env python3
"""Whole-system energies and S(k) of R replicas: the loop of per-replica calls against the one batched call (not part of the
test-suite).

    python tools/system_energy_speed.py [--boxes spce216,co2_64,spce3375] [--replicas 8,64,512] [--runs 2] [--big-limit 20]

Per box and chain count, alternating in one process: R x Engine.system_energy against Engine.system_energy_replicas (with
the deviation), R x Engine.init_structure_factor against Engine.init_structure_factor_replicas; milliseconds per run, and
that the batched results equal the loop's bit for bit.  A chain count is skipped on a box once the loops of the one before
took more than --big-limit seconds (the 10 125-atom box at 512 chains)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from maniac_mc_amd import synth  # noqa: E402
from maniac_mc_amd.engine import Engine  # noqa: E402

E_KEYS = ("non_coulomb", "coulomb", "recip_coulomb", "ewald_self", "intra_coulomb", "total")


def _spce216():
    from tests.util import golden_system
    return golden_system("spce216")[1]


BOXES = {"spce216": _spce216, "co2_64": lambda: synth.co2_box(64), "spce3375": lambda: synth.spce_box(15)}


def measure(name, s, R, runs):
    eng = Engine.from_system(s, n_replicas=R)
    try:
        eng.init_structure_factor_replicas()
        eng.synchronize()
        loop_e, batch_e, loop_s, batch_s = [], [], [], []
        same = True
        for _ in range(runs):
            t0 = time.perf_counter()
            single = np.array([[eng.system_energy(r)[k] for k in E_KEYS] for r in range(R)])
            loop_e.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            out, dev = eng.system_energy_replicas(a_deviation=True)
            batch_e.append(time.perf_counter() - t0)
            same = same and np.array_equal(out, single) and float(np.max(dev)) == 0.0
            t0 = time.perf_counter()
            for r in range(R):
                eng.init_structure_factor(r, True)
            loop_s.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            eng.init_structure_factor_replicas()
            batch_s.append(time.perf_counter() - t0)
        ms = lambda v: [round(1e3 * x, 3) for x in v]
        return dict(box=name, atoms=int(sum(int(n) * int(a) for n, a in zip(s.n_mol, s.topo.atoms_in_res))), nk=int(eng.nk),
                    replicas=R, energy_loop_ms=ms(loop_e), energy_batched_ms=ms(batch_e), sfactor_loop_ms=ms(loop_s),
                    sfactor_batched_ms=ms(batch_s), bit_equal=bool(same))
    finally:
        eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--boxes", default="spce216,co2_64,spce3375")
    ap.add_argument("--replicas", default="8,64,512")
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--big-limit", type=float, default=20.0)
    a = ap.parse_args()
    ok = True
    for name in a.boxes.split(","):
        s = BOXES[name]()
        last = 0.0
        for R in [int(v) for v in a.replicas.split(",")]:
            if last > a.big_limit:
                print(json.dumps(dict(box=name, replicas=R, skipped=f"the loops at the chain count before took {last:.1f} s")), flush=True)
                continue
            t0 = time.perf_counter()
            row = measure(name, s, R, a.runs)
            last = time.perf_counter() - t0
            ok = ok and row["bit_equal"]
            print(json.dumps(row), flush=True)
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
