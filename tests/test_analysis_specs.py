"""CPU-only: the refusals of the farm analyses' options, to the letter and in their order.  Every ValueError run_replicas raises
for a bad ``rdf``, ``density`` or ``energy_pairs`` dict before it creates a farm, the three refusals of checkpoint.check for an
analysis the checkpoint has and the run lacks, and the command line's errors for a sub-option without its option.  The literals
were recorded from the build before the option checks moved into the analysis modules' samplers.

The co2_gcmc fixture inputs: two atom types, one residue type, a cubic cell of half width 25.0 Angstrom."""
import os

import numpy as np
import pytest

from maniac_mc_amd import checkpoint, run
from maniac_mc_amd.replicas import run_replicas
from tests.util import GOLDEN

D = os.path.join(GOLDEN, "runs", "co2_gcmc", "inputs")
INPUTS = (os.path.join(D, "system.maniac"), os.path.join(D, "system.data"), os.path.join(D, "system.inc"))
KW = dict(replicas=4, seed=5, nb_step=40, nb_block=1, fugacities=[12.0, 30.0])

RDF_NEEDS = "rdf: needs r_max and n_bins, and takes pairs, every and include_intra besides ({} unknown)"
DENSITY_NEEDS = "density: needs grid, and takes types, every and per_replica besides ({} unknown)"
TOO_LARGE = dict(grid=(1024, 1024, 16), per_replica=True)             # with replicas=16: 16 maps of two types
TOO_LARGE_TEXT = ("density: the accumulators would take 4294967424 bytes, the limit is 2147483648 "
                  "(16 groups x 2 types x 1024 x 1024 x 16 voxels)")

BAD = [
    (dict(rdf=dict(r_max=4.0, n_bins=8, bins=3)), RDF_NEEDS.format("['bins']")),
    (dict(rdf=dict(n_bins=8)), RDF_NEEDS.format("[]")),
    (dict(rdf=dict(r_max=4.0)), RDF_NEEDS.format("[]")),
    (dict(rdf=dict(r_max=0.0, n_bins=8)), "rdf: r_max must be greater than 0"),
    (dict(rdf=dict(r_max=4.0, n_bins=8, every=0)), "rdf: every must be at least 1"),
    (dict(rdf=dict(r_max=4.0, n_bins=0)), "rdf: n_bins must lie in [1, 1024]"),
    (dict(rdf=dict(r_max=4.0, n_bins=1025)), "rdf: n_bins must lie in [1, 1024]"),
    (dict(rdf=dict(r_max=26.0, n_bins=8)), "rdf: r_max 26.0 exceeds half the smallest perpendicular width of the cell, 25.0"),
    (dict(rdf=dict(r_max=4.0, n_bins=8, pairs=[(0, 0)] * 9)),
     "rdf: 9 atom-type pairs are selected, the limit is 8: name them with --rdf-pairs"),
    (dict(rdf=dict(r_max=4.0, n_bins=8, pairs=[(0, 2)])), "rdf: atom type pair (1, 3) is outside the data file's types"),
    (dict(density=dict(grid=(2, 2, 2), voxels=3)), DENSITY_NEEDS.format("['voxels']")),
    (dict(density=dict(types=[0])), DENSITY_NEEDS.format("[]")),
    (dict(density=dict(grid=(2, 2, 2), every=0)), "density: every must be at least 1"),
    (dict(density=dict(grid=(2, 2, 1025))), "density: grid axis 2 has 1025 voxels, outside [1, 1024]"),
    (dict(density=dict(grid=(2, 2, 2), types=list(range(9)))),
     "density: 9 atom types are selected, the limit is 8: name them with --density-types"),
    (dict(density=dict(TOO_LARGE), replicas=16), TOO_LARGE_TEXT),
    (dict(energy_pairs=dict(each=2)), "energy_pairs: takes every and pairs (['each'] unknown)"),
    (dict(energy_pairs=dict(every=0)), "energy_pairs: every must be at least 1"),
    (dict(energy_pairs=dict(pairs=[(0, 1)])), "energy_pairs: pair (0, 1): residue types must lie in [0, 0]"),
    (dict(energy_pairs=dict(pairs=[])), "energy_pairs: the selection is empty"),
    # two options wrong at once: rdf is refused before density, density before energy_pairs -- but the size of the density
    # accumulators, whose text names the group count, only once the groups are known: after energy_pairs
    (dict(rdf=dict(r_max=4.0, n_bins=0), density=dict(grid=(0, 2, 2))), "rdf: n_bins must lie in [1, 1024]"),
    (dict(rdf=dict(r_max=4.0, n_bins=8, every=0), energy_pairs=dict(every=0)), "rdf: every must be at least 1"),
    (dict(density=dict(grid=(0, 2, 2)), energy_pairs=dict(every=0)), "density: grid axis 0 has 0 voxels, outside [1, 1024]"),
    (dict(rdf=dict(n_bins=8), density=dict(types=[0]), energy_pairs=dict(each=2)), RDF_NEEDS.format("[]")),
    (dict(density=dict(TOO_LARGE), energy_pairs=dict(every=0), replicas=16), "energy_pairs: every must be at least 1"),
]


@pytest.mark.parametrize("options, text", BAD, ids=[str(i) for i in range(len(BAD))])
def test_run_replicas_refuses_a_bad_option_before_it_creates_a_farm(options, text, tmp_path):
    with pytest.raises(ValueError) as err:
        run_replicas(*INPUTS, str(tmp_path / "out"), **dict(KW, **options))
    assert str(err.value) == text
    assert not os.path.exists(tmp_path / "out")


CHECKPOINT = [
    ("rdf", np.array([4.0, 8.0, 1.0, 0.0, 0.0, 0.0]),
     "resume: rdf (--rdf, --rdf-pairs, --rdf-intra) differs from the checkpoint's (checkpoint [4.0, 8.0, 1.0, 0.0, 0.0, 0.0], "
     "this run without it)"),
    ("energy_pairs", np.array([1, 0, 0], dtype=np.int64),
     "resume: energy_pairs (--energy-pairs, --energy-pairs-select) differs from the checkpoint's (checkpoint [1, 0, 0], "
     "this run without it)"),
    ("density", np.array([5, 4, 3, 1, 0, 0, 1], dtype=np.int64),
     "resume: density (--density, --density-types, --density-per-replica) differs from the checkpoint's (checkpoint "
     "[5, 4, 3, 1, 0, 0, 1], this run without it)"),
]


def test_checkpoint_check_refuses_a_run_without_an_analysis_the_checkpoint_has():
    ident = dict(nb_step=40)
    base = dict(id_nb_step=np.asarray(40), next_block=np.asarray(2))
    checkpoint.check(base, ident, 3)
    for key, value, text in CHECKPOINT:
        with pytest.raises(ValueError) as err:
            checkpoint.check(dict(base, **{"id_" + key: value}), ident, 3)
        assert str(err.value) == text
    # all three at once: rdf is named first, then energy_pairs, then density
    every = dict(base, **{"id_" + key: value for key, value, _ in CHECKPOINT})
    for i, (key, value, text) in enumerate(CHECKPOINT):
        have = {k: v for k, v, _ in CHECKPOINT[:i]}
        with pytest.raises(ValueError) as err:
            checkpoint.check(every, dict(ident, **have), 3)
        assert str(err.value) == text
    checkpoint.check(every, dict(ident, **{k: v for k, v, _ in CHECKPOINT}), 3)


CLI = [
    (["--rdf-pairs", "1-1"], "--rdf-pairs and --rdf-intra need --rdf R_MAX,N_BINS[,EVERY]"),
    (["--rdf-intra"], "--rdf-pairs and --rdf-intra need --rdf R_MAX,N_BINS[,EVERY]"),
    (["--energy-pairs-select", "CO2:CO2"], "--energy-pairs-select needs --energy-pairs [EVERY]"),
    (["--density-types", "1"], "--density-types and --density-per-replica need --density N0,N1,N2[,EVERY]"),
    (["--density-per-replica"], "--density-types and --density-per-replica need --density N0,N1,N2[,EVERY]"),
    # several at once: rdf first, then energy_pairs, then density
    (["--rdf-intra", "--energy-pairs-select", "CO2:CO2", "--density-per-replica"],
     "--rdf-pairs and --rdf-intra need --rdf R_MAX,N_BINS[,EVERY]"),
    (["--energy-pairs-select", "CO2:CO2", "--density-per-replica"], "--energy-pairs-select needs --energy-pairs [EVERY]"),
    # an argument that does not parse is the command line's error too
    (["--rdf", "4.0"], "--rdf takes R_MAX,N_BINS[,EVERY], not '4.0'"),
    (["--density", "4,4"], "--density takes N0,N1,N2[,EVERY], not '4,4'"),
    (["--energy-pairs", "0"], "--energy-pairs: EVERY must be at least 1"),
]


@pytest.mark.parametrize("extra, text", CLI, ids=[str(i) for i in range(len(CLI))])
def test_the_command_line_refuses_a_sub_option_without_its_option(extra, text, capsys, tmp_path):
    base = ["-i", INPUTS[0], "-d", INPUTS[1], "-p", INPUTS[2], "-o", str(tmp_path / "out"), "--replicas", "2"]
    with pytest.raises(SystemExit) as err:
        run.main(base + extra)
    assert err.value.code == 2
    assert capsys.readouterr().err.rstrip("\n").endswith("error: " + text)
    assert not os.path.exists(tmp_path / "out")
