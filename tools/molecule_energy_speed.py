#!/usr/bin/env python3
"""Per-molecule removal energies of R replicas: the one call against the composition of per-candidate calls (not part of the
test-suite).

    python tools/molecule_energy_speed.py [--boxes spce216,co2_64,spce3375] [--replicas 8,64,512] [--runs 2] [--big-limit 20]

Per box and chain count, alternating in one process, --runs times each, in milliseconds:
  new          Engine.molecule_energies_replicas over every active type;
  composed     what there was before it: Engine.pair_energy_candidates(use_resident), Engine.recip_energy_candidates(kind =
               MGPU_DELETION) -- and one MGPU_NONE candidate per replica for the energy of A(k) as it is --,
               Engine.intra_energy_candidates and Engine.self_energy, one set of calls over all molecules of all replicas, the
               candidate lists built on the host;
  accumulate   Engine.molecule_energy_accumulate alone (nothing comes back).
`agreement` is the largest difference between the two paths over all molecules and the four components they both form, in units
of tests/util.py's tol_for: reported, not asserted -- the composition's pair part takes the trial sweeps' shared far row and its
reciprocal part the difference of two sums over the running A(k).  A chain count is skipped on a box once the point before took
more than --big-limit seconds.  One JSON line per point."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from maniac_mc_amd import _lib, synth  # noqa: E402
from maniac_mc_amd.engine import Engine  # noqa: E402
from maniac_mc_amd.system import KB_KCALMOL  # noqa: E402

TOL_K = 1.0e-10 / KB_KCALMOL          # tests/util.py TOL_K (1e-10 kcal/mol in K)


def tol_for(a, b):
    return np.maximum(TOL_K, 16 * np.finfo(np.float64).eps * np.maximum(np.abs(a), np.abs(b)))


def _spce216():
    from tests.util import golden_system
    return golden_system("spce216")[1]


BOXES = {"spce216": _spce216, "co2_64": lambda: synth.co2_box(64), "spce3375": lambda: synth.spce_box(15)}


def composed(eng, types, R):
    """(n_mol_total, 5) in the new call's molecule order: replica, then selected type, then molecule"""
    rep, ty, mol = [], [], []
    for r in range(R):
        for t in types:
            n = eng.num_molecules(r, t)
            rep += [r] * n; ty += [t] * n; mol += list(range(n))
    rep, ty, mol = (np.asarray(v, dtype=np.int32) for v in (rep, ty, mol))
    nc, co = eng.pair_energy_candidates(rep, ty, mol, use_resident=np.ones(rep.size, dtype=np.int32))
    u_del = eng.recip_energy_candidates(rep, ty, mol, np.full(rep.size, _lib.MGPU_DELETION, dtype=np.int32))
    reps = np.arange(R, dtype=np.int32)
    u_all = eng.recip_energy_candidates(reps, np.full(R, types[0], dtype=np.int32), np.full(R, -1, dtype=np.int32),
                                        np.full(R, _lib.MGPU_NONE, dtype=np.int32))
    intra = eng.intra_energy_candidates(rep, ty, mol, use_resident=np.ones(rep.size, dtype=np.int32))
    self_of = np.array([eng.self_energy(t) for t in range(eng.topo.n_res)])
    return np.stack([nc, co, u_all[rep] - u_del, self_of[ty], intra], axis=1)


def measure(name, s, R, runs):
    eng = Engine.from_system(s, n_replicas=R)
    try:
        types = [t for t in range(s.topo.n_res) if s.topo.is_active[t] == 1]
        eng.init_structure_factor_replicas()
        eng.molecule_energy_configure(64, -2.0e4, 2.0e3, types)
        eng.synchronize()
        t_new, t_old, t_acc = [], [], []
        for _ in range(runs):
            t0 = time.perf_counter()
            full, counts = eng.molecule_energies_replicas(types)
            t_new.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            old = composed(eng, types, R)
            t_old.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            eng.molecule_energy_accumulate()
            t_acc.append(time.perf_counter() - t0)
        row0 = np.concatenate([[0], np.cumsum([int(eng.mol_capacity[t]) for t in types])[:-1]]).astype(int)
        new = np.concatenate([full[r, row0[k]:row0[k] + counts[r, k]] for r in range(R) for k in range(len(types))])
        worst = float(np.max(np.abs(new - old) / tol_for(new, old))) if new.size else 0.0
        ms = lambda v: [round(1e3 * x, 3) for x in v]
        return dict(box=name, atoms=int(sum(int(n) * int(a) for n, a in zip(s.n_mol, s.topo.atoms_in_res))), nk=int(eng.nk),
                    replicas=R, molecules=int(new.shape[0]), new_ms=ms(t_new), composed_ms=ms(t_old), accumulate_ms=ms(t_acc),
                    ratio=round(min(t_new) / min(t_old), 3), agreement_in_tol=round(worst, 4))
    finally:
        eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--boxes", default="spce216,co2_64,spce3375")
    ap.add_argument("--replicas", default="8,64,512")
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--big-limit", type=float, default=20.0)
    a = ap.parse_args()
    for name in a.boxes.split(","):
        s = BOXES[name]()
        last = 0.0
        for R in [int(v) for v in a.replicas.split(",")]:
            if last > a.big_limit:
                print(json.dumps(dict(box=name, replicas=R, skipped=f"the point before took {last:.1f} s")), flush=True)
                continue
            t0 = time.perf_counter()
            row = measure(name, s, R, a.runs)
            last = time.perf_counter() - t0
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
