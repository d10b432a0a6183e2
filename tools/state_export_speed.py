#!/usr/bin/env python3
"""The whole resident state of R replicas out of the engine: the loop of per-replica getters against the one-call export (not
part of the test-suite).

    python tools/state_export_speed.py [--boxes spce216,co2_64,spce3375] [--replicas 8,64,512] [--runs 2] [--checkpoint 512]

Per box and replica count, alternating in one process: R x (get_molecules, get_frames, structure_factor, get_reservoir per
type) against Engine.state_export of all R (the engine's pinned block, not copied again); milliseconds per run, the block's
size, and that the pieces of the block are the getters' bit for bit (every replica, first run).  An engine's FIRST export also
allocates the pinned block and the device scratch: it is made before the timed runs and reported apart (first_call_ms).  --checkpoint R (0: skip): on the 10 125-atom box a farm of R window chains
runs one block of 400 steps and writes one checkpoint -- the seconds of the Monte Carlo, of FortranFarm.checkpoint_state (the
export and the driver's block) and of checkpoint.save (numpy.savez, flush, fsync, rename), and the file's size."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from maniac_mc_amd import checkpoint, synth  # noqa: E402
from maniac_mc_amd.engine import Engine, state_unpack  # noqa: E402


def _spce216():
    from tests.util import golden_system
    return golden_system("spce216")[1]


BOXES = {"spce216": _spce216, "co2_64": lambda: synth.co2_box(64), "spce3375": lambda: synth.spce_box(15)}


def measure(name, s, R, runs):
    eng = Engine.from_system(s, n_replicas=R)
    try:
        n_res = s.topo.n_res
        for t in range(n_res):
            if s.topo.is_active[t]:
                eng.set_frames(0, t, s.com[t], s.offsets[t])
        eng.init_structure_factor(0, True)
        for r in range(1, R):
            eng.replica_copy(r, 0)
        eng.synchronize()
        # the first export of an engine also allocates its pinned block and the device scratch: timed apart
        t0 = time.perf_counter()
        eng.state_export(np.arange(R, dtype=np.int32), copy=False)
        first = time.perf_counter() - t0
        loop, one = [], []
        same, nbytes = True, 0
        for run in range(runs):
            t0 = time.perf_counter()
            got = []
            for r in range(R):
                got.append([(eng.get_molecules(r, t), eng.get_frames(r, t) if s.topo.is_active[t] else None, eng.get_reservoir(r, t))
                            for t in range(n_res)] + [eng.structure_factor(r)])
            loop.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            block = eng.state_export(np.arange(R, dtype=np.int32), copy=False)     # (the C call's cost: the engine's own buffer)
            one.append(time.perf_counter() - t0)
            nbytes = int(block.shape[0])
            if run == 0:
                for r, rep in enumerate(state_unpack(block)):
                    for t in range(n_res):
                        mol, frames, _ = got[r][t]
                        same = same and np.array_equal(rep["pos"][t], mol)
                        if frames is not None:
                            same = same and np.array_equal(rep["com"][t], frames[0]) and np.array_equal(rep["off"][t], frames[1])
                    # (A(k): the same values in the engine's slot order -- the sorted parts agree)
                    same = same and np.array_equal(np.sort(rep["A"][:, 0][rep["A"][:, 0] != 0]), np.sort(got[r][-1].real[got[r][-1].real != 0]))
        ms = lambda v: [round(1e3 * x, 3) for x in v]
        return dict(box=name, atoms=int(sum(int(n) * int(a) for n, a in zip(s.n_mol, s.topo.atoms_in_res))), nk=int(eng.nk),
                    replicas=R, getters_loop_ms=ms(loop), one_call_ms=ms(one), first_call_ms=ms([first])[0], block_mb=round(nbytes / 1e6, 3),
                    one_call_gb_per_s=round(nbytes / 1e9 / min(one), 2), bit_equal=bool(same))
    finally:
        eng.close()


def checkpoint_block(R, steps=400):
    from maniac_mc_amd.fortran_host import FortranFarm
    s = synth.spce_box(15)
    farm = FortranFarm(s, R, seed=3, n_lanes=4, device_build=True, window=True)
    try:
        t0 = time.perf_counter()
        farm.run(steps)
        t_run = time.perf_counter() - t0
        t0 = time.perf_counter()
        state = farm.checkpoint_state()
        t_state = time.perf_counter() - t0
        with tempfile.TemporaryDirectory() as d:
            ident = checkpoint.identity(2, steps, 3, "windows", R, None, (0,), None, None, None, None)
            t0 = time.perf_counter()
            path = checkpoint.save(d, ident, 2, 3, "windows", state["engine"], state["driver"], {})
            t_save = time.perf_counter() - t0
            size = os.path.getsize(path)
        return dict(checkpoint_block=True, box="spce3375", replicas=R, steps=steps, window=bool(farm.window), run_s=round(t_run, 4),
                    checkpoint_state_s=round(t_state, 4), save_s=round(t_save, 4), file_mb=round(size / 1e6, 1),
                    engine_blocks=len(state["engine"]), driver_kb=round(len(state["driver"]) / 1e3, 1))
    finally:
        farm.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--boxes", default="spce216,co2_64,spce3375")
    ap.add_argument("--replicas", default="8,64,512")
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--checkpoint", type=int, default=512)
    a = ap.parse_args()
    ok = True
    for name in [b for b in a.boxes.split(",") if b]:
        s = BOXES[name]()
        for R in [int(v) for v in a.replicas.split(",")]:
            row = measure(name, s, R, a.runs)
            ok = ok and row["bit_equal"]
            print(json.dumps(row), flush=True)
    if a.checkpoint > 0:
        print(json.dumps(checkpoint_block(a.checkpoint)), flush=True)
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
