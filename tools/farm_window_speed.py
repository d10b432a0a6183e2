#!/usr/bin/env python3
"""Accepted moves/s of the Fortran farm (10 125-atom SPC/E box, or the CO2 insertion / deletion box) against the number of chains: batched path
(mgpu_move_trial_submit / wait + mgpu_commit_submit, five launches per lane step) against window mode (ONE launch per lane
step, mgpu_farm_window_submit), for several lane counts and windows in flight.

    python tools/farm_window_speed.py [--replicas 8,64,512] [--seconds 1.0] [--modes batched,w1,w2,w3] [--lanes 1,2,4]
    python tools/farm_window_speed.py --workload spce_triclinic --lanes 1 --replicas 8,64,512 --modes host,batched,w1,w2
    python tools/farm_window_speed.py --workload adsorbate24_triclinic --lanes 1 --replicas 8,64,512 --modes batched,w1,w2 --wide-triclinic --repeats 2

--workload spce_triclinic: bench.py's sheared 10 125-atom box.  Mode `host` is the farm as it runs such a box by default (moves
built on the host, batched evaluation); `batched` and `w1`.. switch the engine's triclinic moves on (FortranFarm
triclinic_moves): device-built batched steps, and one launch per lane step.
--workload adsorbate24_triclinic / adsorbate24_gcmc_triclinic: bench.py's 64 rigid 24-site adsorbates in the 60 A box, sheared by
spce_triclinic's tilt scaled to its edge (tilt_of(60.0), tools/chain_run_speed.py's box), the centres keeping their fractions: NVT,
and grand-canonical (30 % translations, 30 % rotations, 40 % insertions / deletions).  Mode `batched` is the only device-built mode
such a farm has without --wide-triclinic (FortranFarm wide_triclinic, Engine.farm_set_wide_triclinic); with it w1.. are one launch
per lane step, and a window mode the engine did not take stops the tool.  --repeats N runs every chain count's modes N times,
alternating (batched, w1, w2, batched, w1, w2): a difference smaller than the spread between the runs of one mode is none.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replicas", default="1,8,64,512")
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--modes", default="batched,w1,w2,w3")
    ap.add_argument("--lanes", default="1,2,4")
    ap.add_argument("--threads", type=int, default=2)
    ap.add_argument("--drivers", default="1", help="driver threads (each runs its own lanes' windows)")
    ap.add_argument("--side", type=int, default=15)
    ap.add_argument("--workload", default="spce", choices=("spce", "spce_triclinic", "co2_gcmc", "adsorbate24", "adsorbate24_triclinic", "adsorbate24_gcmc_triclinic"),
                    help="spce: the 10 125-atom box, translation / rotation; spce_triclinic: the same box sheared (tilt 3.0 / -2.0 / 1.5 A, "
                         "bench.py's), modes host | batched | w1..; co2_gcmc: bench.py's 50 A CO2 box, insertion / deletion only; "
                         "adsorbate24: bench.py's 64 rigid 24-site adsorbates in a 60 A box, translation / rotation; "
                         "adsorbate24_triclinic / adsorbate24_gcmc_triclinic: that box sheared, NVT / grand-canonical")
    ap.add_argument("--wide-triclinic", dest="wide_triclinic", action="store_true",
                    help="adsorbate24_triclinic / adsorbate24_gcmc_triclinic: window modes through the engine's farm windows for "
                         "molecules of 6 to 63 sites in a triclinic box (FortranFarm wide_triclinic=True)")
    ap.add_argument("--repeats", type=int, default=1, help="runs of every mode per chain count, the modes alternating")
    ap.add_argument("--reservoir", action="store_true",
                    help="co2_gcmc: every chain draws its insertions from a reservoir of 400 random rotations of CO2 (mfarm_set_reservoir)")
    ap.add_argument("--json", default="")
    args = ap.parse_args()
    from maniac_mc_amd import synth
    from maniac_mc_amd.fortran_host import FortranFarm
    if args.workload == "spce":
        s = synth.spce_box(args.side, seed=12345)
        kw = dict(translation_step=0.3, rotation_step=0.3, p_translation=0.5)
    elif args.workload == "spce_triclinic":
        s = synth.spce_box(args.side)
        L = float(s.box_matrix[0, 0])
        # bench.py's spce_triclinic: rows a = (lx, 0, 0), b = (xy, ly, 0), c = (xz, yz, lz), the centres sheared with the cell
        s.box_matrix = np.array([[L, 0.0, 0.0], [3.0, L, 0.0], [-2.0, 1.5, L]])
        frac = (s.com[0] - s.bounds_lo[None, :]) / L
        s.com[0] = s.bounds_lo[None, :] + frac @ s.box_matrix.T
        kw = dict(translation_step=0.3, rotation_step=0.3, p_translation=0.5, triclinic_moves=True)
    elif args.workload == "adsorbate24":
        s = synth.rigid_adsorbate_box(n_mol=64, L=60.0, seed=17)
        kw = dict(translation_step=0.3, rotation_step=0.3, p_translation=0.5)
    elif args.workload in ("adsorbate24_triclinic", "adsorbate24_gcmc_triclinic"):
        # tools/chain_run_speed.py's sheared box: spce_triclinic's tilt (3.0 / -2.0 / 1.5 A on its 46.56 A edge) scaled to the edge
        tilt_of = lambda L: tuple(x * L / 46.56 for x in (3.0, -2.0, 1.5))
        s = synth.rigid_adsorbate_box(n_mol=64, L=60.0, seed=17)
        xy, xz, yz = tilt_of(60.0)
        s.box_matrix = np.array([[60.0, 0.0, 0.0], [xy, 60.0, 0.0], [xz, yz, 60.0]])
        s.com[0] = s.bounds_lo[None, :] + ((s.com[0] - s.bounds_lo[None, :]) / 60.0) @ s.box_matrix.T
        kw = dict(translation_step=0.3, rotation_step=0.3, p_translation=0.5, triclinic_moves=True)
        if args.workload == "adsorbate24_gcmc_triclinic":
            V = abs(float(np.linalg.det(s.box_matrix)))
            kw.update(mol_capacity=[96], gcmc=dict(p_translation=0.3, p_rotation=0.3, fugacity=64.0 / V))
        if args.wide_triclinic:
            kw["wide_triclinic"] = True
    else:
        s = synth.co2_box(64, seed=13)
        kw = dict(translation_step=1.0, rotation_step=0.6, mol_capacity=[400],
                  gcmc=dict(p_translation=0.0, p_rotation=0.0, fugacity=100.0 / 50.0 ** 3))
    tri_wide = args.workload in ("adsorbate24_triclinic", "adsorbate24_gcmc_triclinic")
    if args.wide_triclinic and not tri_wide:
        ap.error("--wide-triclinic goes with --workload adsorbate24_triclinic / adsorbate24_gcmc_triclinic")
    rsv = None
    if args.reservoir:
        if args.workload != "co2_gcmc":
            ap.error("--reservoir goes with --workload co2_gcmc")
        rng = np.random.default_rng(5)
        q = rng.normal(size=(400, 4))
        q /= np.linalg.norm(q, axis=1)[:, None]
        w, x, y, z = q.T
        rot = np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], -1),
                        np.stack([2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)], -1),
                        np.stack([2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], -1)], 1)
        rsv = {0: np.einsum("mij,aj->mai", rot, s.offsets[0][0])}
    rows = []
    for R in [int(x) for x in args.replicas.split(",")]:
        for mode in args.modes.split(",") * max(1, args.repeats):
            for lanes, drivers in [(int(x), int(y)) for x in args.lanes.split(",") for y in args.drivers.split(",")]:
                if lanes > R or drivers > lanes:
                    continue
                window = mode.startswith("w")
                depth = int(mode[1:]) if window else 1
                if mode == "host" and args.workload != "spce_triclinic":
                    ap.error("mode host goes with --workload spce_triclinic")
                farm = FortranFarm(s, R, seed=77, n_threads=max(args.threads, drivers), n_lanes=lanes, n_drivers=drivers,
                                   device_build=mode != "host", window=window, window_depth=depth, reservoir=rsv, **kw)
                if args.workload == "spce_triclinic" or tri_wide:      # the switch took: no silent fall-back to the host construction
                    assert farm.device_build == (mode != "host") and farm.window == window, (mode, farm.device_build, farm.window)
                try:
                    farm.run(20)
                    chunk = (400 if R <= 64 else 200) if window else 50       # (see bench.py replicas_sweep: a chunk ends with a synchronise)
                    farm.run(chunk)
                    farm.eng.synchronize()
                    steps = acc = 0
                    t0 = time.perf_counter()
                    while True:
                        acc += farm.run(chunk)
                        steps += chunk
                        farm.eng.synchronize()
                        el = time.perf_counter() - t0
                        if el >= args.seconds:
                            break
                    row = {"replicas": R, "mode": mode, "lanes": lanes, "drivers": drivers, "window": farm.window, "accepted_per_s": acc / el,
                           "us_per_step": el / steps * 1e6, "nsplit_note": "engine constant", "timers": farm.timers()}
                    rows.append(row)
                    print(f"R {R:5d}  {mode:8s} lanes {lanes} drivers {drivers}  {acc / el / 1e6:8.4f} M accepted/s   {el / steps * 1e6:8.1f} us/step", flush=True)
                finally:
                    farm.close()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
