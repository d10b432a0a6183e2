"""io_maniac.reservoir_offsets: a MANIAC reservoir data file as the offsets a farm takes (Engine.set_reservoir), exactly those
the single-chain front end hands to mchain_set_reservoir_residue (run.py).  CPU only."""
import os

import numpy as np

from maniac_mc_amd import io_maniac, run

INPUTS = os.path.join(os.path.dirname(__file__), "golden", "runs", "dumbbell_gcmc_reservoir", "inputs")


def test_reservoir_offsets_are_what_the_single_chain_driver_receives():
    inp = io_maniac.read_maniac_input(os.path.join(INPUTS, "system.maniac"))
    got = io_maniac.reservoir_offsets(os.path.join(INPUTS, "reservoir.data"), inp)
    rdat = io_maniac.read_lammps_data(os.path.join(INPUTS, "reservoir.data"), inp)
    assert got, "the fixture's reservoir holds molecules"
    for t, r in enumerate(inp.residues):
        _, off = run._mol_arrays(rdat["com"][t], rdat["off"][t], int(r.nb_atoms))
        if off.shape[0] == 0:
            assert t not in got
            continue
        assert got[t].dtype == np.float64 and got[t].flags.c_contiguous
        assert got[t].shape == (off.shape[0], r.nb_atoms, 3)
        assert np.array_equal(got[t], off)
