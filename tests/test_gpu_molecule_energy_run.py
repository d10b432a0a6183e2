"""run_replicas(molecule_energy=...): the two files exist and read back; per replica the slots of all sampled blocks add up to
the molecule counts the replica's number_<res>.dat records for those blocks (nothing is dropped); `every` follows rdf's
convention -- a sample after every block whose index is a multiple of it, so every=2 of 3 blocks samples block 2 only; a run cut
back to its checkpoint after block 1 and resumed writes the arrays and the table of the uninterrupted run; a resume with another
spec, or without the option, is refused by a text naming --molecule-energy; rdf and density switched on beside it change none
of its arrays; and energy.dat is byte-identical with and without the option.

The co2_gcmc fixture inputs at R = 4, two fugacity groups, 3 blocks of 40 steps."""
import os
import shutil

import numpy as np
import pytest

from maniac_mc_amd import checkpoint
from maniac_mc_amd import molecule_energy as me
from maniac_mc_amd.replicas import run_replicas
from tests.util import GOLDEN

pytestmark = pytest.mark.gpu
D = os.path.join(GOLDEN, "runs", "co2_gcmc", "inputs")
INPUTS = (os.path.join(D, "system.maniac"), os.path.join(D, "system.data"), os.path.join(D, "system.inc"))
R = 4
KW = dict(replicas=R, seed=5, nb_block=3, nb_step=40, fugacities=[12.0, 30.0])
SPEC = dict(e_min=-6.0, e_max=0.5, n_bins=26)
FILES = ("molecule_energy.dat", "molecule_energy_counts.npz")

_runs = {}


def _counts(out):
    return me.read_counts(os.path.join(out, "molecule_energy_counts.npz"))


def _molecules(out, r):
    """block -> molecule count of replica r, from its number_CO2.dat"""
    with open(os.path.join(out, f"replica_{r:04d}", "number_CO2.dat")) as f:
        rows = [ln.split() for ln in f if not ln.startswith("#")]
    return {int(b): int(n) for b, n in rows}


@pytest.fixture(scope="module")
def base(tmp_path_factory):
    """the run with the option and the run without it, once for the module"""
    root = tmp_path_factory.mktemp("molen")
    plain_dir, with_dir = str(root / "plain"), str(root / "with")
    plain = run_replicas(*INPUTS, plain_dir, **KW)
    with_me = run_replicas(*INPUTS, with_dir, molecule_energy=dict(SPEC), **KW)
    return plain_dir, with_dir, plain, with_me


def test_files_counts_and_unchanged_outputs(base):
    plain_dir, with_dir, plain, with_me = base
    assert all(os.path.isfile(os.path.join(with_dir, n)) for n in FILES)
    assert not any(os.path.exists(os.path.join(plain_dir, n)) for n in FILES)
    assert "molecule_energy" not in plain["seconds"] and with_me["seconds"]["molecule_energy"] > 0.0
    for r in range(R):
        for name in ("energy.dat", "number_CO2.dat", "moves.dat"):
            a, b = (open(os.path.join(d, f"replica_{r:04d}", name), "rb").read() for d in (plain_dir, with_dir))
            assert a == b, (r, name)
    for key in ("energy", "counts", "chain_counters", "group"):
        assert np.array_equal(plain[key], with_me[key]), key
    z = _counts(with_dir)
    assert z["hist"].shape == (R, 1, SPEC["n_bins"] + 2) and z["hist"].dtype == np.uint64
    assert np.array_equal(z["samples"], np.full(R, 3, dtype=np.uint64))
    assert z["group"].tolist() == [0, 1, 0, 1] and z["types"].tolist() == [0] and int(z["every"]) == 1
    assert (float(z["e_min"]), float(z["e_max"]), int(z["n_bins"])) == (SPEC["e_min"], SPEC["e_max"], SPEC["n_bins"])
    seen = []
    for r in range(R):
        n = _molecules(with_dir, r)
        assert int(z["hist"][r].sum()) == n[1] + n[2] + n[3], "nothing is dropped"
        seen.append([n[1], n[2], n[3]])
    print("molecules per sampled block", seen, "inside the range", int(z["hist"][:, :, 1:-1].sum()), "of", int(z["hist"].sum()))
    assert z["hist"][:, :, 1:-1].sum() > 0, "bound molecules lie inside the range"
    # molecule_energy.dat is the pooled table of those counts
    back = me.read_dat(os.path.join(with_dir, "molecule_energy.dat"))
    assert sorted(back) == [(0, 0), (1, 0)]
    for g, s, p, sem, count in me.pooled(z["hist"], z["group"], SPEC["e_min"], SPEC["e_max"]):
        d = back[(g, s)]
        assert d["type"] == 1 and d["name"] == "CO2" and d["below"] == int(count[0]) and d["above"] == int(count[-1])
        assert np.array_equal(d["count"], count[1:-1]) and np.allclose(d["density"], p, rtol=1e-8, atol=0)
        assert np.allclose(d["sem"], sem, rtol=1e-8, atol=0)
        assert np.allclose(d["e_mid"], me.bin_centres(SPEC["e_min"], SPEC["e_max"], SPEC["n_bins"]), rtol=0, atol=5e-9)


def test_every_two_samples_block_two_only(tmp_path):
    out = str(tmp_path / "every")
    run_replicas(*INPUTS, out, molecule_energy=dict(SPEC, every=2), **KW)
    z = _counts(out)
    assert np.array_equal(z["samples"], np.full(R, 1, dtype=np.uint64)) and int(z["every"]) == 2
    for r in range(R):
        assert int(z["hist"][r].sum()) == _molecules(out, r)[2]


def test_rdf_and_density_beside_it_change_nothing(base, tmp_path):
    out = str(tmp_path / "together")
    run_replicas(*INPUTS, out, molecule_energy=dict(SPEC), rdf=dict(r_max=20.0, n_bins=8), density=dict(grid=(4, 4, 4)), **KW)
    a, b = _counts(base[1]), _counts(out)
    assert sorted(a) == sorted(b) and all(np.array_equal(a[k], b[k]) for k in a)
    assert open(os.path.join(base[1], FILES[0]), "rb").read() == open(os.path.join(out, FILES[0]), "rb").read()
    assert os.path.isfile(os.path.join(out, "rdf.dat")) and os.path.isfile(os.path.join(out, "density_counts.npz"))


def test_a_run_cut_back_to_block_one_resumes_to_the_same_files(base, tmp_path, monkeypatch):
    a_dir, b_dir = base[1], str(tmp_path / "B")
    kept = {}
    save = checkpoint.save

    def keeping(outdir, ident, next_block, *a, **k):
        path = save(outdir, ident, next_block, *a, **k)
        kept[int(next_block)] = path + f".{int(next_block)}"
        shutil.copyfile(path, kept[int(next_block)])
        return path
    monkeypatch.setattr(checkpoint, "save", keeping)
    b = run_replicas(*INPUTS, b_dir, checkpoint_every=1, molecule_energy=dict(SPEC), **KW)
    monkeypatch.undo()
    assert sorted(kept) == [2, 3, 4]
    for name in FILES:                                      # checkpointing changes nothing
        assert open(os.path.join(a_dir, name), "rb").read() == open(os.path.join(b_dir, name), "rb").read(), name
    # back to the checkpoint after block 1: it carries the accumulators of one sample
    os.replace(kept[2], checkpoint.path_of(b_dir))
    ck = checkpoint.load(b_dir)
    assert int(ck["next_block"]) == 2 and sorted(ck["extra"]) == ["molecule_energy_hist", "molecule_energy_samples"]
    assert np.array_equal(ck["extra"]["molecule_energy_samples"], np.full(R, 1, dtype=np.uint64))
    assert ck["extra"]["molecule_energy_hist"].dtype == np.uint64 and "id_molecule_energy" in ck
    for name in FILES:
        os.remove(os.path.join(b_dir, name))
    # refused by a text naming the switch, before anything is touched: without the option, other bins, other limits
    for other in (None, dict(SPEC, n_bins=13), dict(SPEC, e_max=1.0), dict(SPEC, every=2)):
        with pytest.raises(ValueError, match="--molecule-energy"):
            run_replicas(*INPUTS, b_dir, resume=True, molecule_energy=other, **KW)
    c = run_replicas(*INPUTS, b_dir, resume=True, molecule_energy=dict(SPEC), **KW)
    za, zb = _counts(a_dir), _counts(b_dir)
    assert sorted(za) == sorted(zb) and all(np.array_equal(za[k], zb[k]) for k in za)
    for name in FILES:
        assert open(os.path.join(a_dir, name), "rb").read() == open(os.path.join(b_dir, name), "rb").read(), name
    for key in ("energy", "counts", "chain_counters"):
        assert np.array_equal(b[key], c[key]), key


def test_a_run_without_the_option_writes_todays_checkpoint_keys(base, tmp_path):
    out = str(tmp_path / "Z")
    run_replicas(*INPUTS, out, checkpoint_every=3, **KW)
    with np.load(checkpoint.path_of(out), allow_pickle=False) as z:
        assert not any(k.startswith("x_") or k == "id_molecule_energy" for k in z.files)
    assert not any(os.path.exists(os.path.join(out, n)) for n in FILES)
    with pytest.raises(ValueError, match="--molecule-energy"):
        run_replicas(*INPUTS, out, resume=True, molecule_energy=dict(SPEC), **dict(KW, nb_block=4))
