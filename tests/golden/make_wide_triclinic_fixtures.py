"""Whole-run fixtures of rigid molecules of 6 and 24 sites in a TRICLINIC cell (one-launch windows and chain runs for such boxes,
DESIGN section 4.3): the committed inputs of tests/golden/runs_wide/{cage6_nvt, cage24_gcmc} with a tilt line added to
system.data, and the output files the REFERENCE writes for them, made as make_triclinic_gcmc_fixtures.py makes its own
(oracle/run_ref_mc.py: the reference's MonteCarloLoop, writers and log through oracle/_ref, A(k) initialised, the generator
seeded by the reference's seed_rng).  Same step counts as their parents (3 x 150).

    python tests/golden/make_wide_triclinic_fixtures.py

Runs only where oracle/_ref exists.  The 24-site molecule is charged: its grand-canonical files are those of the deletion as
written (as_written true), as its parent's are.
Layout: tests/golden/runs_wide_triclinic/<case>/{inputs,expected}, tests/golden/runs_wide_triclinic/summary.json
(make_run_fixtures.py's)."""
import json
import os
import shutil
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from tests.golden.make_triclinic_gcmc_fixtures import tilted  # noqa: E402

RUNS = os.path.join(HERE, "runs_wide_triclinic")
SOURCE = os.path.join(HERE, "runs_wide")
SEED = 20251017
TILT = "2.0 -1.5 1.0 xy xz yz"          # a few Angstrom in the 26 Angstrom box
CASES = {"cage6_tri_nvt": "cage6_nvt", "cage24_tri_gcmc": "cage24_gcmc"}   # case -> its parent in runs_wide
FILES = ("system.maniac", "system.data", "system.inc")


def main():
    parents = json.load(open(os.path.join(SOURCE, "summary.json")))
    if os.path.isdir(RUNS):
        shutil.rmtree(RUNS)
    summary = {}
    for case, parent in CASES.items():
        inputs = os.path.join(RUNS, case, "inputs")
        expected = os.path.join(RUNS, case, "expected")
        os.makedirs(inputs)
        os.makedirs(expected)
        for f in FILES:
            text = open(os.path.join(SOURCE, parent, "inputs", f)).read()
            open(os.path.join(inputs, f), "w").write(tilted(text, TILT) if f == "system.data" else text)
        with tempfile.TemporaryDirectory() as tmp:
            out = os.path.join(tmp, "out", "")
            # (relative file names, from the inputs directory: the log echoes the names as given)
            cmd = [sys.executable, os.path.join(ROOT, "oracle", "run_ref_mc.py"), *FILES, out, str(SEED)]
            p = subprocess.run(cmd, capture_output=True, text=True, cwd=inputs)
            assert "RUN_OK" in p.stdout, p.stdout[-2000:] + p.stderr[-2000:]
            for f in sorted(os.listdir(out)):
                if f == "log.maniac":
                    lines = open(os.path.join(out, f)).read().split("\n")
                    lines = ["<output path>" if out.rstrip("/") in ln else ln for ln in lines]
                    open(os.path.join(expected, "log.maniac"), "w").write("\n".join(lines))
                else:
                    shutil.copy(os.path.join(out, f), os.path.join(expected, f))
        last = open(os.path.join(expected, "moves.dat")).read().strip().split("\n")[-1].split()
        summary[case] = dict(seed=SEED, files=sorted(os.listdir(expected)), last_moves_record=last, reservoir=False,
                             as_written=bool(parents[parent]["as_written"]))
        print(case, last)
    json.dump(summary, open(os.path.join(RUNS, "summary.json"), "w"), indent=1)


if __name__ == "__main__":
    main()
