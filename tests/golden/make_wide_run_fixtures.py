"""Whole-run fixtures for rigid molecules of more than five sites (single-chain windows of 6 to 63 sites, DESIGN section
4.3): input files for two small synthetic boxes and the output files the REFERENCE writes for them, made exactly as
make_run_fixtures.py makes its own (io_maniac.write_input_files + oracle/run_ref_mc.py: the reference's MonteCarloLoop,
writers and log through oracle/_ref, A(k) initialised, the generator seeded by the reference's seed_rng).

    python tests/golden/make_wide_run_fixtures.py [case ...]      (no arguments: every case)

Runs only where oracle/_ref exists.  cage24_gcmc is a CHARGED grand-canonical run, so its files are the reference's
deletion as written (as_written: the chain driver reproduces them with mchain_set_as_written); cage6_nvt is the
same in both modes.
Layout: tests/golden/runs_wide/<case>/{inputs,expected}, tests/golden/runs_wide/summary.json (make_run_fixtures.py's)."""
import json
import os
import shutil
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from maniac_mc_amd import io_maniac, synth  # noqa: E402

RUNS = os.path.join(HERE, "runs_wide")
SEED = 20251017


def cases():
    cage = dict(masses=[12.011, 15.9994], atom_names=["CA", "CB"])
    yield "cage24_gcmc", synth.rigid_adsorbate_box(n_mol=6, n_sites=24, L=26.0), dict(
        nb_block=3, nb_step=150, translation_step=0.6, rotation_step_angle=0.4, translation_proba=0.3, rotation_proba=0.3,
        insertion_deletion_proba=0.4, fugacity_atm=[5.0], recalibrate_moves=True, **cage)
    yield "cage6_nvt", synth.rigid_adsorbate_box(n_mol=6, n_sites=6, L=26.0), dict(
        nb_block=3, nb_step=150, translation_step=0.6, rotation_step_angle=0.4, translation_proba=0.5, rotation_proba=0.5,
        recalibrate_moves=True, **cage)


AS_WRITTEN = {"cage24_gcmc"}


def main():
    only = set(sys.argv[1:])
    spath = os.path.join(RUNS, "summary.json")
    summary = json.load(open(spath)) if (only and os.path.exists(spath)) else {}
    if not only and os.path.isdir(RUNS):
        shutil.rmtree(RUNS)
    for name, system, kw in cases():
        if only and name not in only:
            continue
        if os.path.isdir(os.path.join(RUNS, name)):
            shutil.rmtree(os.path.join(RUNS, name))
        inputs = os.path.join(RUNS, name, "inputs")
        expected = os.path.join(RUNS, name, "expected")
        files = io_maniac.write_input_files(system, inputs, **kw)
        with tempfile.TemporaryDirectory() as tmp:
            out = os.path.join(tmp, "out", "")
            # (relative file names, from the inputs directory: the log echoes the names as given)
            rel = [os.path.basename(a) for a in files]
            cmd = [sys.executable, os.path.join(ROOT, "oracle", "run_ref_mc.py"), *rel, out, str(SEED)]
            p = subprocess.run(cmd, capture_output=True, text=True, cwd=inputs)
            assert "RUN_OK" in p.stdout, p.stdout[-2000:] + p.stderr[-2000:]
            os.makedirs(expected, exist_ok=True)
            for f in sorted(os.listdir(out)):
                if f == "log.maniac":
                    lines = open(os.path.join(out, f)).read().split("\n")
                    lines = ["<output path>" if out.rstrip("/") in ln else ln for ln in lines]
                    open(os.path.join(expected, "log.maniac"), "w").write("\n".join(lines))
                else:
                    shutil.copy(os.path.join(out, f), os.path.join(expected, f))
        last = open(os.path.join(expected, "moves.dat")).read().strip().split("\n")[-1].split()
        summary[name] = dict(seed=SEED, files=sorted(os.listdir(expected)), last_moves_record=last, reservoir=False,
                             as_written=name in AS_WRITTEN)
        print(name, last)
    json.dump(dict(sorted(summary.items())), open(spath, "w"), indent=1)


if __name__ == "__main__":
    main()
