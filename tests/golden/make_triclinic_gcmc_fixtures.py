"""Whole-run fixture of a grand-canonical run in a TRICLINIC cell (chain runs for grand-canonical blocks of triclinic boxes,
DESIGN section 4.3): the committed inputs of tests/golden/runs/dumbbell_gcmc with a tilt line added to system.data, and the
output files the REFERENCE writes for them, made as make_wide_run_fixtures.py makes its own (oracle/run_ref_mc.py: the
reference's MonteCarloLoop, writers and log through oracle/_ref, A(k) initialised, the generator seeded by the reference's
seed_rng).

    python tests/golden/make_triclinic_gcmc_fixtures.py

Runs only where oracle/_ref exists.  The molecules are uncharged, so the files do not depend on SURVEY F3 (as_written false).
Layout: tests/golden/runs_triclinic_gcmc/<case>/{inputs,expected}, tests/golden/runs_triclinic_gcmc/summary.json
(make_run_fixtures.py's)."""
import json
import os
import shutil
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
RUNS = os.path.join(HERE, "runs_triclinic_gcmc")
SOURCE = os.path.join(HERE, "runs", "dumbbell_gcmc", "inputs")
SEED = 20251017
CASE = "dumbbell_tri_gcmc"
TILT = "-3.0 -2.0 2.0 xy xz yz"         # a few Angstrom in the 25 Angstrom box; five wrapped centres leave xlo..zhi along y,
                                       # so the log carries the reader's two "COM outside simulation box" warnings for each
FILES = ("system.maniac", "system.data", "system.inc")


def tilted(data_text, tilt=TILT):
    """system.data with the tilt line behind its zlo zhi line"""
    lines = data_text.split("\n")
    at = [i for i, ln in enumerate(lines) if ln.split()[2:] == ["zlo", "zhi"]]
    assert len(at) == 1 and "xy xz yz" not in data_text
    return "\n".join(lines[:at[0] + 1] + [tilt] + lines[at[0] + 1:])


def main():
    if os.path.isdir(RUNS):
        shutil.rmtree(RUNS)
    inputs = os.path.join(RUNS, CASE, "inputs")
    expected = os.path.join(RUNS, CASE, "expected")
    os.makedirs(inputs)
    os.makedirs(expected)
    for f in FILES:
        text = open(os.path.join(SOURCE, f)).read()
        open(os.path.join(inputs, f), "w").write(tilted(text) if f == "system.data" else text)
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
    summary = {CASE: dict(seed=SEED, files=sorted(os.listdir(expected)), last_moves_record=last, reservoir=False, as_written=False)}
    print(CASE, last)
    json.dump(summary, open(os.path.join(RUNS, "summary.json"), "w"), indent=1)


if __name__ == "__main__":
    main()
