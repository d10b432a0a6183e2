#!/usr/bin/env python3
"""Pair distribution histograms of R replicas: Engine.rdf_accumulate against what a user did before it -- the replicas'
coordinates over the link (Engine.farm_snapshot_raw) and a NumPy minimum-image histogram on the host (not part of the
test-suite).

    python tools/rdf_speed.py [--boxes spce216,co2_64,spce3375] [--replicas 8,64,512] [--runs 2] [--bins 512] [--host-max 8]

Per box and replica count, alternating in one process: one rdf_accumulate over all R replicas (every pair of the box's atom
types, r_max = half the smallest cell width) against snapshot + host histogram of the same replicas; milliseconds per run.  On a
box of more than 5000 atoms the host route is run on --host-max replicas only and scaled to R (the row says so; --host-max 0:
no host route at all, the device's time alone).  The device's
counts are compared with the host route's wherever no pair lies within 1e-9 A of a bin edge (the tests' precondition); where
one does, the row gives the margin and the number of bins that differ instead.  Every replica holds its own perturbation of the
box."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from maniac_mc_amd import rdf, synth  # noqa: E402
from maniac_mc_amd.engine import Engine  # noqa: E402

MARGIN = 1.0e-9


def _spce216():
    from tests.util import golden_system
    return golden_system("spce216")[1]


BOXES = {"spce216": _spce216, "co2_64": lambda: synth.co2_box(64), "spce3375": lambda: synth.spce_box(15)}


def host_histogram(sites, ty, key, L, pairs, n_bins, r_max, rows=512):
    """hist (n_pairs, n_bins), eligible (n_pairs,), the smallest distance of a counted r to a bin edge and the number of pairs
    within MARGIN of one: NumPy, orthorhombic fold"""
    n = sites.shape[0]
    hist = np.zeros((len(pairs), n_bins), dtype=np.uint64)
    elig = np.zeros(len(pairs), dtype=np.uint64)
    code = np.full((int(ty.max()) + 1,) * 2, -1, dtype=np.int64)
    for p, (a, b) in enumerate(pairs):
        code[a, b] = code[b, a] = p
    dr, inv_dr, margin, n_close = r_max / n_bins, n_bins / r_max, np.inf, 0
    j = np.arange(n)
    for i0 in range(0, n, rows):
        i = np.arange(i0, min(n, i0 + rows))
        d = sites[i][:, None, :] - sites[None, :, :]
        d -= L * np.rint(d / L)
        r = np.sqrt(np.einsum("ijk,ijk->ij", d, d))
        p = code[ty[i][:, None], ty[None, :]]
        ok = (j[None, :] > i[:, None]) & (p >= 0) & (key[i][:, None] != key[None, :])
        p, r = p[ok], r[ok]
        elig += np.bincount(p, minlength=len(pairs)).astype(np.uint64)
        near = r[r < r_max + dr]
        if near.size:
            edge = np.minimum(np.abs(near - np.round(near / dr) * dr), np.abs(near - r_max))
            margin = min(margin, float(edge.min()))
            n_close += int((edge <= MARGIN).sum())
        inside = r < r_max
        b = (r[inside] * inv_dr).astype(np.int64)
        keep = b < n_bins
        hist += np.bincount(p[inside][keep] * n_bins + b[keep], minlength=len(pairs) * n_bins).reshape(len(pairs), n_bins).astype(np.uint64)
    return hist, elig, margin, n_close


def measure(name, s, R, runs, n_bins, host_max):
    topo = s.topo
    n_res = topo.n_res
    pairs = rdf.default_pairs(topo)
    r_max = rdf.half_width(s.box_matrix)
    L = np.diag(s.box_matrix).copy()
    eng = Engine.from_system(s, n_replicas=R, extra_capacity=0)
    try:
        rng = np.random.default_rng(R)
        for r in range(R):
            for t in range(n_res):
                com = s.com[t] + (rng.uniform(-0.2, 0.2, s.com[t].shape) if r else 0.0)
                eng.set_molecules(r, t, com[:, None, :] + s.offsets[t])
                eng.set_frames(r, t, com, s.offsets[t])
        eng.rdf_configure(n_bins, r_max, pairs)
        eng.rdf_accumulate()                         # the first call: code object load, the replica list's block
        eng.rdf_reset()
        n_atoms = int(s.n_atoms)
        n_host = 0 if host_max == 0 else (R if n_atoms <= 5000 else min(R, host_max))
        ty = np.concatenate([np.tile(topo.atom_types[t, :topo.atoms_in_res[t]] - 1, int(s.n_mol[t])) for t in range(n_res)]).astype(np.int64)
        key = np.concatenate([t * (1 << 28) + np.repeat(np.arange(int(s.n_mol[t])), int(topo.atoms_in_res[t])) for t in range(n_res)])
        dev_ms, host_ms, snap_ms = [], [], []
        same, worst_margin, differing = True, np.inf, 0
        for _ in range(runs):
            eng.rdf_reset()
            t0 = time.perf_counter()
            eng.rdf_accumulate()
            dev_ms.append(1e3 * (time.perf_counter() - t0))
            hist, elig, samples = eng.rdf_read()
            if n_host == 0:
                continue
            t0 = time.perf_counter()
            counts, com, off, _ = eng.farm_snapshot(list(range(n_host)))
            snap_ms.append(1e3 * (time.perf_counter() - t0))
            for r in range(n_host):
                sites = np.concatenate([(com[r][t][:, None, :] + off[r][t]).reshape(-1, 3) for t in range(n_res)])
                h, e, margin, n_close = host_histogram(sites, ty, key, L, pairs, n_bins, r_max)
                worst_margin = min(worst_margin, margin)
                if n_close == 0:
                    same = same and np.array_equal(h, hist[r]) and np.array_equal(e, elig[r])
                else:
                    # a pair that close to an edge may fall into either neighbouring bin: at most two bins off by one per pair
                    moved = int(np.abs(h.astype(np.int64) - hist[r].astype(np.int64)).sum())
                    same = same and np.array_equal(e, elig[r]) and moved <= 2 * n_close
                    differing += int((h != hist[r]).sum())
            host_ms.append(1e3 * (time.perf_counter() - t0) * (R / n_host))
        return dict(box=name, atoms=n_atoms, replicas=R, pairs=len(pairs), bins=n_bins, r_max=round(r_max, 4),
                    pairs_per_replica=int(elig[0].sum()), device_ms=[round(v, 3) for v in dev_ms],
                    device_us_per_replica=round(1e3 * min(dev_ms) / R, 2), snapshot_ms=[round(v, 3) for v in snap_ms],
                    host_ms=[round(v, 1) for v in host_ms], host_replicas_measured=n_host, host_scaled=bool(n_host != R),
                    smallest_margin=float(f"{worst_margin:.3e}") if n_host else None, bins_differing_where_margin_not_met=differing, equal=bool(same))
    finally:
        eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--boxes", default="spce216,co2_64,spce3375")
    ap.add_argument("--replicas", default="8,64,512")
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--bins", type=int, default=512)
    ap.add_argument("--host-max", type=int, default=8)
    a = ap.parse_args()
    ok = True
    for name in a.boxes.split(","):
        s = BOXES[name]()
        for R in [int(v) for v in a.replicas.split(",")]:
            if s.n_atoms > 5000 and R > 64:
                print(json.dumps(dict(box=name, replicas=R, skipped="the large box is measured at R = 8 and 64")), flush=True)
                continue
            row = measure(name, s, R, a.runs, a.bins, a.host_max)
            ok = ok and row["equal"]
            print(json.dumps(row), flush=True)
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
