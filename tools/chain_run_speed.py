#!/usr/bin/env python3
"""Steps/s of the single-chain driver's Monte Carlo loop (mc_chain.f90, mchain_get_loop_seconds) in its default mode
(speculate 4, one-launch windows) against chain runs (run_simulation(chain_run=(k, depth)): launches queued back to back that
continue from the step cursor on the device).

    python tools/chain_run_speed.py [--blocks 2] [--steps 2000] [--ks 1,2,4,8] [--depths 2,3,4] [--cases spce_10125_nvt,framework_nvt]
    python tools/chain_run_speed.py --workload spce_triclinic
    python tools/chain_run_speed.py --workload co2_gcmc --chain-run-gcmc --ks 4,8 --depths 3
    python tools/chain_run_speed.py --workload co2_gcmc_triclinic --chain-run-triclinic --chain-run-gcmc --ks 4,8 --depths 3
    python tools/chain_run_speed.py --workload adsorbate24 --chain-run-wide --wide-chain-windows --ks 4,8 --depths 3
    python tools/chain_run_speed.py --workload adsorbate24_gcmc --chain-run-wide --chain-run-gcmc --wide-chain-windows --ks 4,8 --depths 3
    python tools/chain_run_speed.py --workload adsorbate24_triclinic --chain-run-triclinic --chain-run-wide --wide-chain-windows --ks 4,8 --depths 3
    python tools/chain_run_speed.py --workload adsorbate24_gcmc_triclinic --chain-run-triclinic --chain-run-wide --chain-run-gcmc --wide-chain-windows --ks 4,8 --depths 3

Boxes: bench.py's 10 125-atom SPC/E box and its framework box (2208 framework atoms + 40 four-site waters), NVT, 50 %
translations / 50 % rotations.  --workload spce_triclinic: bench.py's sheared 10 125-atom box (tilt 3.0 / -2.0 / 1.5 A) instead,
its chain runs with chain_run_triclinic=True (the default mode is the windows such a box runs through without the switch).
--workload co2_gcmc / framework_gcmc (with --chain-run-gcmc: their chain runs are those of by-count records, chain_run_gcmc=True): a
CO2 box (64 three-site molecules in 50 A) and the framework box with its waters, grand-canonical -- 30 % translations, 30 %
rotations, 40 % insertions / deletions; per run also the steps the run took through the windows (fallback).
--workload co2_gcmc_triclinic / framework_gcmc_triclinic (with --chain-run-triclinic AND --chain-run-gcmc, as on run.py's command
line: either alone leaves such a box its windows and the tool stops): the same two boxes sheared by spce_triclinic's tilt scaled to
their edge, the framework atoms and the centres keeping their fractions.
--workload adsorbate24 / adsorbate24_gcmc (with --chain-run-wide: chain_run_wide=True; the second with --chain-run-gcmc as well):
bench.py's 64 rigid 24-site adsorbates in a 60 A box, NVT and grand-canonical.  Without the switch such a box keeps its windows and
the tool stops.  --wide-chain-windows adds a second yardstick beside the default mode (whose windows of such molecules are made of
batched calls): the same box through the WIDE one-launch windows, wide_chain_windows=True.
--workload adsorbate24_triclinic / adsorbate24_gcmc_triclinic (with --chain-run-triclinic and --chain-run-wide, the second with
--chain-run-gcmc as well): the same 60 A box sheared by spce_triclinic's tilt scaled to its edge, the centres keeping their
fractions.  The default mode is the batched windows such a box runs through without wide_triclinic; every other mode (the WIDE
windows, the runs) sets wide_triclinic=True.  Every mode runs twice, the modes alternating (default, runs ..., default, runs ...), from one
build on one box in one session; per run: steps/s of the loop alone, mean steps per launch that did something, the share of
void launches, undecided steps.  The output files of every mode must be those of the default mode (checked here).  A
difference between two modes that is smaller than the spread between the two runs of one mode is no difference.
"""
import argparse
import filecmp
import os
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from maniac_mc_amd import io_maniac, run, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=2)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--ks", default="1,2,4,8")
    ap.add_argument("--depths", default="2,3,4")
    ap.add_argument("--cases", default="spce_10125_nvt,framework_nvt")
    ap.add_argument("--workload", default=None, choices=("spce", "framework", "spce_triclinic", "co2_gcmc", "framework_gcmc", "co2_gcmc_triclinic",
                                                     "framework_gcmc_triclinic", "adsorbate24", "adsorbate24_gcmc", "adsorbate24_triclinic",
                                                     "adsorbate24_gcmc_triclinic"),
                    help="one box instead of --cases")
    ap.add_argument("--chain-run-gcmc", dest="chain_run_gcmc", action="store_true",
                    help="the grand-canonical boxes' chain runs (chain_run_gcmc=True); without it such a box keeps its windows and the tool stops")
    ap.add_argument("--chain-run-triclinic", dest="chain_run_triclinic", action="store_true",
                    help="the sheared grand-canonical boxes' chain runs (chain_run_triclinic=True, with --chain-run-gcmc); the sheared NVT "
                         "box's chain runs take the switch by themselves, as they always did")
    ap.add_argument("--chain-run-wide", dest="chain_run_wide", action="store_true",
                    help="the chain runs of boxes of 6 to 63-site molecules (chain_run_wide=True); without it such a box keeps its windows and the tool stops")
    ap.add_argument("--wide-chain-windows", dest="wide_chain_windows", action="store_true",
                    help="a second yardstick: the box through the WIDE one-launch windows (wide_chain_windows=True) beside the default windows")
    ap.add_argument("--rounds", type=int, default=2)
    a = ap.parse_args()
    if a.workload is not None:
        a.cases = {"spce": "spce_10125_nvt", "framework": "framework_nvt", "spce_triclinic": "spce_triclinic_nvt",
                   "co2_gcmc": "co2_gcmc", "framework_gcmc": "framework_gcmc", "adsorbate24": "adsorbate24_nvt",
                   "adsorbate24_triclinic": "adsorbate24_triclinic_nvt"}.get(a.workload, a.workload)
    tmp = tempfile.mkdtemp()
    common = dict(nb_block=2, nb_step=100, translation_proba=0.5, rotation_proba=0.5)
    cases = {
        "spce_10125_nvt": (synth.spce_box(15), dict(translation_step=0.3, rotation_step_angle=0.3, masses=[15.9994, 1.008],
                                                    atom_names=["OW", "HW"])),
        "framework_nvt": (synth.framework_water_box(), dict(translation_step=0.5, rotation_step_angle=0.5,
                                                            masses=[12.0] * 7 + [15.9994, 1.008, 1e-4], fugacity_atm=[1.0, 1.0])),
    }
    gcmc = dict(nb_block=2, nb_step=100, translation_proba=0.3, rotation_proba=0.3, insertion_deletion_proba=0.4)
    gc_cases = {
        "co2_gcmc": (synth.co2_box(), dict(translation_step=1.0, rotation_step_angle=0.6, masses=[12.011, 15.9994], atom_names=["C", "O"],
                                           fugacity_atm=[30.0])),
        "framework_gcmc": (synth.framework_water_box(), dict(translation_step=0.5, rotation_step_angle=0.5,
                                                             masses=[12.0] * 7 + [15.9994, 1.008, 1e-4], fugacity_atm=[1.0, 0.05])),
    }
    # bench.py's adsorbate24: 64 rigid 24-site adsorbates (two atom types) in a 60 A box
    ads = dict(translation_step=0.8, rotation_step_angle=0.5, masses=[12.011, 15.9994], atom_names=["CA", "OA"])
    if "adsorbate24_nvt" in a.cases.split(","):
        cases["adsorbate24_nvt"] = (synth.rigid_adsorbate_box(n_mol=64, L=60.0, seed=17), ads)
    if "adsorbate24_gcmc" in a.cases.split(","):
        gc_cases["adsorbate24_gcmc"] = (synth.rigid_adsorbate_box(n_mol=64, L=60.0, seed=17), dict(ads, fugacity_atm=[5.0]))
    # the grand-canonical boxes sheared: spce_triclinic's tilt (3.0 / -2.0 / 1.5 A on its 46.56 A edge) scaled to the box's edge
    tilt_of = lambda L: tuple(x * L / 46.56 for x in (3.0, -2.0, 1.5))
    if "co2_gcmc_triclinic" in a.cases.split(","):
        s = synth.co2_box()
        L = float(s.box_matrix[0, 0])
        xy, xz, yz = tilt_of(L)
        s.box_matrix = np.array([[L, 0.0, 0.0], [xy, L, 0.0], [xz, yz, L]])
        s.com[0] = s.bounds_lo[None, :] + ((s.com[0] - s.bounds_lo[None, :]) / L) @ s.box_matrix.T
        gc_cases["co2_gcmc_triclinic"] = (s, gc_cases["co2_gcmc"][1])
    def sheared_adsorbates():
        s = synth.rigid_adsorbate_box(n_mol=64, L=60.0, seed=17)
        xy, xz, yz = tilt_of(60.0)
        s.box_matrix = np.array([[60.0, 0.0, 0.0], [xy, 60.0, 0.0], [xz, yz, 60.0]])
        s.com[0] = s.bounds_lo[None, :] + ((s.com[0] - s.bounds_lo[None, :]) / 60.0) @ s.box_matrix.T
        return s
    if "adsorbate24_triclinic_nvt" in a.cases.split(","):
        cases["adsorbate24_triclinic_nvt"] = (sheared_adsorbates(), ads)
    if "adsorbate24_gcmc_triclinic" in a.cases.split(","):
        gc_cases["adsorbate24_gcmc_triclinic"] = (sheared_adsorbates(), dict(ads, fugacity_atm=[5.0]))
    if "framework_gcmc_triclinic" in a.cases.split(","):
        gc_cases["framework_gcmc_triclinic"] = (synth.framework_water_box(tilt=tilt_of(34.0)), gc_cases["framework_gcmc"][1])
    cases.update(gc_cases)
    if "spce_triclinic_nvt" in a.cases.split(","):
        # bench.py's spce_triclinic: rows a = (lx, 0, 0), b = (xy, ly, 0), c = (xz, yz, lz), the centres sheared with the cell
        s = synth.spce_box(15)
        L = float(s.box_matrix[0, 0])
        s.box_matrix = np.array([[L, 0.0, 0.0], [3.0, L, 0.0], [-2.0, 1.5, L]])
        s.com[0] = s.bounds_lo[None, :] + ((s.com[0] - s.bounds_lo[None, :]) / L) @ s.box_matrix.T
        cases["spce_triclinic_nvt"] = (s, cases["spce_10125_nvt"][1])
    modes = [("default", None)] + ([("wide windows", "wide")] if a.wide_chain_windows else []) + [(f"run k={k} depth={d}", (k, d)) for k in map(int, a.ks.split(",")) for d in map(int, a.depths.split(","))]
    n = a.blocks * a.steps
    for name in a.cases.split(","):
        system, kw = cases[name]
        files = io_maniac.write_input_files(system, os.path.join(tmp, name + "_in"), **(gcmc if name in gc_cases else common), **kw)
        rates = {label: [] for label, _ in modes}
        base = None
        for rnd in range(a.rounds):
            for label, cr in modes:
                out = os.path.join(tmp, f"{name}_{label.replace(' ', '_').replace('=', '')}_{rnd}") + "/"
                ww = cr == "wide"
                if ww:
                    cr = None
                res = run.run_simulation(*files, out, seed=5, nb_block=a.blocks, nb_step=a.steps, chain_run=cr,
                                         chain_run_wide=cr is not None and a.chain_run_wide, **(dict(wide_chain_windows=True) if ww else {}),
                                         chain_run_triclinic=cr is not None and system.is_triclinic() and
                                         (a.chain_run_triclinic or name not in gc_cases),
                                         chain_run_gcmc=cr is not None and a.chain_run_gcmc,
                                         wide_triclinic=(ww or cr is not None) and name.startswith("adsorbate24") and system.is_triclinic())
                if cr is not None and not res["chain_run"]["on"]:
                    raise SystemExit(f"{name}: the engine did not take the chain run (Engine.chain_run_capacity)")
                rate = n / res["mc_seconds"]
                rates[label].append(rate)
                if base is None:
                    base = out
                diff = [f for f in sorted(os.listdir(out)) if f != "log.maniac" and not filecmp.cmp(os.path.join(out, f), os.path.join(base, f), shallow=False)]
                c = res["counters"]
                extra = f"windows {res['chain_windows'][0]}, left to the host {res['chain_windows'][1]}"
                if cr is not None:
                    r = res["chain_run"]
                    work = max(1, r["launches"] - r["void_launches"])
                    extra = (f"on {r['on']}, launches {r['launches']}, steps per working launch {r['steps'] / work:.2f}, "
                             f"void {r['void_launches'] / max(1, r['launches']):.1%}, undecided {r['undecided']}, "
                             f"fallback steps {r['fallback_steps']}")
                print(f"{name:16s} round {rnd} {label:18s}: {rate:9.0f} steps/s (loop {res['mc_seconds']:.3f} s of {n} steps; {extra}; "
                      f"acceptance {int(c[1] + c[3] + c[5] + c[7]) / n:.2f}; files as the first run's: {not diff}{' ' + str(diff) if diff else ''})", flush=True)
        print(f"\n{name}: steps/s of the loop alone, the rounds side by side")
        for label, _ in modes:
            v = rates[label]
            print(f"  {label:18s} {'  '.join(f'{x:9.0f}' for x in v)}   mean {sum(v) / len(v):9.0f}  spread {max(v) - min(v):8.0f}")
        print(flush=True)


if __name__ == "__main__":
    main()
