#!/usr/bin/env python3
"""Density maps of R replicas: Engine.density_accumulate against what a user did before it -- the replicas' coordinates over
the link (Engine.farm_snapshot) and numpy.histogramdd on the host (not part of the test-suite).

    python tools/density_speed.py [--boxes spce216,co2_64,spce3375] [--replicas 8,64,512] [--runs 2] [--grid 32,32,32]
                                  [--framework 512] [--grids 8,32,128]

Per box and replica count, alternating in one process: one density_accumulate over all R replicas (the box's atom types as
channels, all replicas in one map) against snapshot + histogramdd of the same replicas; milliseconds per run.  The device's
counts are compared with the host route's wherever no atom lies within 1e-9 of a voxel face (the tests' precondition); where one
does, the row gives the margin and the number of voxels that differ instead.  Every replica holds its own perturbation of the
box.  --framework R: the framework box at R replicas in one map, guest channels only and then with a framework atom type beside
them -- every replica then adds into the same voxels, the one place contention can bite.  --grids: grids of n^3 voxels on the
first box at the last replica count."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from maniac_mc_amd import density, synth  # noqa: E402
from maniac_mc_amd.engine import Engine  # noqa: E402

MARGIN = 1.0e-9


def _spce216():
    from tests.util import golden_system
    return golden_system("spce216")[1]


BOXES = {"spce216": _spce216, "co2_64": lambda: synth.co2_box(64), "spce3375": lambda: synth.spce_box(15),
         "framework": lambda: synth.framework_water_box()}


def host_histogram(sites, ty, s, grid, types):
    """hist (n_channels, n2, n1, n0) of one configuration by histogramdd over the folded fractional coordinates, and the
    smallest distance of a u to an integer"""
    f = np.linalg.solve(s.box_matrix, (sites - s.bounds_lo[None, :]).T).T
    u = f * np.asarray(grid, dtype=np.float64)[None, :]
    hist = np.zeros((len(types), grid[2], grid[1], grid[0]), dtype=np.uint64)
    margin = np.inf
    for c, t in enumerate(types):
        sel = ty == t
        if not sel.any():
            continue
        margin = min(margin, float(np.abs(u[sel] - np.round(u[sel])).min()))
        h, _ = np.histogramdd(f[sel] - np.floor(f[sel]), bins=grid, range=[(0.0, 1.0)] * 3)
        hist[c] = h.transpose(2, 1, 0).astype(np.uint64)
    return hist, margin


def measure(name, s, R, runs, grid, types, host=True):
    topo = s.topo
    n_res = topo.n_res
    eng = Engine.from_system(s, n_replicas=R, extra_capacity=0)
    try:
        rng = np.random.default_rng(R)
        for r in range(R):
            for t in range(n_res):
                move = rng.uniform(-0.2, 0.2, s.com[t].shape) if (r and topo.is_active[t] == 1) else 0.0
                com = s.com[t] + move
                eng.set_molecules(r, t, com[:, None, :] + s.offsets[t])
                if topo.is_active[t] == 1:               # (a frozen framework carries no frames; its rows run no host route)
                    eng.set_frames(r, t, com, s.offsets[t])
        eng.density_configure(grid, types)
        eng.density_accumulate()                     # the first call: code object load, the replica list's block
        ty = np.concatenate([np.tile(topo.atom_types[t, :topo.atoms_in_res[t]] - 1, int(s.n_mol[t])) for t in range(n_res)]).astype(np.int64)
        counted = int(np.isin(ty, types).sum())
        dev_ms, host_ms, snap_ms = [], [], []
        same, worst = True, np.inf
        for _ in range(runs):
            eng.density_reset()
            t0 = time.perf_counter()
            eng.density_accumulate()
            dev_ms.append(1e3 * (time.perf_counter() - t0))
            if not host:
                continue
            hist, samples = eng.density_read()
            t0 = time.perf_counter()
            counts, com, off, _ = eng.farm_snapshot(list(range(R)))
            snap_ms.append(1e3 * (time.perf_counter() - t0))
            want = np.zeros_like(hist[0])
            for r in range(R):
                sites = np.concatenate([(com[r][t][:, None, :] + off[r][t]).reshape(-1, 3) for t in range(n_res)])
                h, margin = host_histogram(sites, ty, s, grid, types)
                want += h
                worst = min(worst, margin)
            host_ms.append(1e3 * (time.perf_counter() - t0))
            same = same and (np.array_equal(want, hist[0]) if worst > MARGIN else int(want.sum()) == int(hist[0].sum())) and int(samples[0]) == R
        best = min(dev_ms)
        return dict(box=name, atoms=int(s.n_atoms), replicas=R, grid=list(grid), types=list(types), adds=counted * R,
                    device_ms=[round(v, 3) for v in dev_ms], device_us_per_replica=round(1e3 * best / R, 3),
                    adds_per_second=float(f"{counted * R / (best * 1e-3):.3e}"), snapshot_ms=[round(v, 3) for v in snap_ms],
                    host_ms=[round(v, 1) for v in host_ms], smallest_margin=float(f"{worst:.3e}") if host_ms else None, equal=bool(same))
    finally:
        eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--boxes", default="spce216,co2_64,spce3375")
    ap.add_argument("--replicas", default="8,64,512")
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--grid", default="32,32,32")
    ap.add_argument("--framework", type=int, default=0, metavar="R")
    ap.add_argument("--grids", default="")
    a = ap.parse_args()
    grid = density.check_grid(a.grid.split(","))
    reps = [int(v) for v in a.replicas.split(",")]
    names = [n for n in a.boxes.split(",") if n]
    ok = True
    for name in names:
        s = BOXES[name]()
        types = list(range(s.topo.n_atom_types))[:density.MAX_CHANNELS]
        for R in reps:
            if s.n_atoms > 5000 and R > 64:
                print(json.dumps(dict(box=name, replicas=R, skipped="the large box is measured at R = 8 and 64")), flush=True)
                continue
            row = measure(name, s, R, a.runs, grid, types)
            ok = ok and row["equal"]
            print(json.dumps(row), flush=True)
    if a.framework:
        s = BOXES["framework"]()
        guest = density.default_types(s.topo)
        frame = next(t for t in range(s.topo.n_atom_types) if t not in guest)
        for types in (guest, guest + [frame]):
            row = measure("framework", s, a.framework, a.runs, grid, types, host=False)
            row["framework_channel"] = bool(frame in types)
            print(json.dumps(row), flush=True)
    if a.grids and names:
        s = BOXES[names[0]]()
        for n in [int(v) for v in a.grids.split(",")]:
            print(json.dumps(measure(names[0], s, reps[-1], a.runs, (n, n, n), list(range(s.topo.n_atom_types))[:8], host=False)), flush=True)
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
