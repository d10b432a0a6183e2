"""run_replicas(density=...): density_counts.npz holds an independent recount of the coordinates at the same block ends, in
every farm mode; the three kinds of file exist, parse and agree with each other; the option changes nothing else; a run cut
back to its first checkpoint and resumed writes the files of the uninterrupted run, byte for byte; a resume without the option,
or with another grid, is refused by name; a run without the option writes no density file and no new checkpoint key.

The co2_gcmc fixture inputs at R = 4, two fugacity groups, 40 steps a block.  The coordinates at the block ends come from
Engine.farm_snapshot right after each sample (modes that keep molecule frames; the rounded sum com + offset is the engine's
coordinate) or Engine.get_molecules (host-built moves); the recount is the contract's rule in NumPy, after asserting that no
atom lies within 1e-9 of a voxel face (tests/test_gpu_density.py)."""
import os
import shutil

import numpy as np
import pytest

from maniac_mc_amd import checkpoint, density, io_maniac, run
from maniac_mc_amd.fortran_host import FortranFarm
from maniac_mc_amd.replicas import run_replicas
from tests.util import GOLDEN

pytestmark = pytest.mark.gpu
D = os.path.join(GOLDEN, "runs", "co2_gcmc", "inputs")
INPUTS = (os.path.join(D, "system.maniac"), os.path.join(D, "system.data"), os.path.join(D, "system.inc"))
R, STEPS = 4, 40
KW = dict(replicas=R, seed=5, nb_step=STEPS, fugacities=[12.0, 30.0])
SPEC = dict(grid=(5, 4, 3), types=[0, 1])
DENSITY_FILES = ("density_counts.npz", "density_profiles.dat", "density_g00_type01.cube", "density_g00_type02.cube",
                 "density_g01_type01.cube", "density_g01_type02.cube")


def _tree(path):
    out = {}
    for base, dirs, files in os.walk(path):
        dirs[:] = [d for d in dirs if not (base == path and d == checkpoint.DIR_NAME)]
        for f in files:
            p = os.path.join(base, f)
            out[os.path.relpath(p, path)] = open(p, "rb").read()
    return out


def _without_dir(data, root):
    return b"\n".join(ln for ln in data.split(b"\n") if str(root).encode() not in ln)


def _counts(out):
    with np.load(os.path.join(out, "density_counts.npz"), allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def _recount(s, sites, ty, grid, types):
    """hist (n_channels, n2, n1, n0) of the sites (n, 3) with atom types ty (n,) by the contract's rule"""
    n = np.asarray(grid, dtype=np.float64)
    u = np.linalg.solve(s.box_matrix, (sites - s.bounds_lo[None, :]).T).T * n[None, :]
    if u.size:
        assert np.abs(u - np.round(u)).min() > 1.0e-9
    v = np.mod(np.floor(u).astype(np.int64), np.asarray(grid, dtype=np.int64)[None, :])
    hist = np.zeros((len(types), grid[2], grid[1], grid[0]), dtype=np.uint64)
    for c, t in enumerate(types):
        sel = ty == t
        np.add.at(hist[c], (v[sel, 2], v[sel, 1], v[sel, 0]), np.uint64(1))
    return hist


@pytest.mark.parametrize("mode", ["windows", "device", "device_accept", "host"])
def test_counts_are_a_recount_of_the_block_ends_and_the_files_agree(mode, tmp_path, monkeypatch):
    out = str(tmp_path / "density")
    s = io_maniac.load_system(*INPUTS)[0]
    grid, types = SPEC["grid"], SPEC["types"]
    site_ty = np.array([int(s.topo.atom_types[0, a]) - 1 for a in range(int(s.topo.atoms_in_res[0]))])
    seen = []                                             # [block][replica] -> hist of that configuration
    sample = FortranFarm.density_sample

    def watched(self, *a, **k):
        sample(self, *a, **k)
        if self.device_build:
            counts, com, off, _ = self.eng.farm_snapshot(np.arange(R))
            sites = [com[r][0][:, None, :] + off[r][0] for r in range(R)]
            assert [len(x) for x in sites] == counts[:, 0].tolist()
        else:
            sites = [self.eng.get_molecules(r, 0) for r in range(R)]
        self._select()
        seen.append([_recount(s, x.reshape(-1, 3), np.tile(site_ty, len(x)), grid, types) for x in sites])
    monkeypatch.setattr(FortranFarm, "density_sample", watched)
    res = run_replicas(*INPUTS, out, nb_block=3, mode=mode, density=dict(SPEC), **KW)
    monkeypatch.undo()
    assert res["mode"] == mode and res["seconds"]["density"] > 0.0 and len(seen) == 3
    print(mode, "seconds", res["seconds"])
    z = _counts(out)
    want = np.zeros((2, len(types), grid[2], grid[1], grid[0]), dtype=np.uint64)
    for block in seen:
        for r in range(R):
            want[r % 2] += block[r]
    assert z["hist"].dtype == np.uint64 and np.array_equal(z["hist"], want) and want.sum() > 0
    assert np.array_equal(z["samples"], np.full(2, 6, dtype=np.uint64)), "two replicas a group, three blocks"
    assert z["group_of"].tolist() == [0, 1, 0, 1] and z["group"].tolist() == [0, 1, 0, 1]
    assert z["grid"].tolist() == list(grid) and z["types"].tolist() == types and int(z["every"]) == 1 and int(z["per_replica"]) == 0
    assert len({int(b[r].sum()) for b in seen for r in range(R)}) > 1, "insertions and deletions happened"
    # ---- the files exist; the profiles parse and sum to the counts
    assert all(os.path.isfile(os.path.join(out, n)) for n in DENSITY_FILES)
    prof = density.read_profiles(os.path.join(out, "density_profiles.dat"))
    assert sorted(prof) == [(g, c, k) for g in (0, 1) for c in (0, 1) for k in (0, 1, 2)]
    V = density.volume(s.box_matrix)
    for (g, c, k), d in prof.items():
        assert d["type"] == types[c] + 1 and d["count"].shape == (grid[k],)
        assert np.array_equal(d["count"], density.profiles(z["hist"])[k][g, c]) and int(d["count"].sum()) == int(z["hist"][g, c].sum())
        assert np.allclose(d["density"], d["count"] / (6.0 * V / grid[k]), rtol=1e-9, atol=0)
        assert np.allclose(d["s_mid"], (np.arange(grid[k]) + 0.5) / grid[k], rtol=0, atol=5e-9)
    # ---- the cube files reproduce the cell and hold the number density
    rho = density.number_density(z["hist"], z["samples"], s.box_matrix)
    for g in (0, 1):
        for c in (0, 1):
            cube = density.read_cube(os.path.join(out, density.cube_name(g, types[c])))
            assert "Angstrom^3" in cube["comments"][0] and cube["n"].tolist() == list(grid) and cube["atoms"] == []
            assert np.allclose(cube["origin"], s.bounds_lo, rtol=0, atol=1e-6)
            assert np.allclose(cube["vectors"].T * np.asarray(grid)[None, :], s.box_matrix, rtol=0, atol=1e-5)
            assert np.allclose(cube["rho"], rho[g, c], rtol=1e-5, atol=0)
            assert np.isclose(cube["rho"].sum() * V / np.prod(grid), z["hist"][g, c].sum() / 6.0, rtol=1e-5)


def test_the_option_changes_nothing_else_and_per_replica_maps(tmp_path):
    plain_dir, den_dir = str(tmp_path / "plain"), str(tmp_path / "density")
    plain = run_replicas(*INPUTS, plain_dir, nb_block=2, **KW)
    with_den = run_replicas(*INPUTS, den_dir, nb_block=2, density=dict(grid=(2, 2, 2), every=2, per_replica=True), **KW)
    ta, tb = _tree(plain_dir), _tree(den_dir)
    cubes = [density.cube_name(g, t) for g in range(R) for t in (0, 1)]
    assert sorted(set(tb) - set(ta)) == sorted(["density_counts.npz", "density_profiles.dat"] + cubes) and not set(ta) - set(tb)
    assert not any(n.startswith("density") for n in ta)
    for name in sorted(ta):
        assert _without_dir(ta[name], tmp_path) == _without_dir(tb[name], tmp_path), name
    for key in ("energy", "counts", "chain_counters", "group"):
        assert np.array_equal(plain[key], with_den[key]), key
    assert plain["counters"] == with_den["counters"] and plain["accepted"] == with_den["accepted"]
    assert "density" not in plain["seconds"]
    z = _counts(den_dir)
    assert z["types"].tolist() == [0, 1], "the default: the atom types of the active residue types"
    assert np.array_equal(z["samples"], np.ones(R, dtype=np.uint64)), "block 2 of 2, one map per replica"
    assert z["group_of"].tolist() == [0, 1, 2, 3] and z["group"].tolist() == [0, 1, 0, 1]
    # every map holds its replica's atoms: C once, O twice per molecule
    assert np.array_equal(z["hist"][:, 0].sum(axis=(1, 2, 3)), with_den["counts"][:, 0])
    assert np.array_equal(z["hist"][:, 1].sum(axis=(1, 2, 3)), 2 * with_den["counts"][:, 0])
    with pytest.raises(ValueError, match=r"outside \[1, 1024\]"):
        run_replicas(*INPUTS, den_dir, nb_block=1, density=dict(grid=(0, 2, 2)), **KW)
    with pytest.raises(ValueError, match="atom type 3 is outside the data file's types"):
        run_replicas(*INPUTS, den_dir, nb_block=1, density=dict(grid=(2, 2, 2), types=[0, 2]), **KW)


def test_a_run_cut_back_to_its_first_checkpoint_resumes_to_the_same_files(tmp_path, monkeypatch):
    a_dir, b_dir = str(tmp_path / "A"), str(tmp_path / "B")
    run_replicas(*INPUTS, a_dir, nb_block=4, density=dict(SPEC), **KW)
    kept = {}
    save = checkpoint.save

    def keeping(outdir, ident, next_block, *a, **k):
        path = save(outdir, ident, next_block, *a, **k)
        kept[int(next_block)] = path + f".{int(next_block)}"
        shutil.copyfile(path, kept[int(next_block)])
        return path
    monkeypatch.setattr(checkpoint, "save", keeping)
    b = run_replicas(*INPUTS, b_dir, nb_block=4, checkpoint_every=2, density=dict(SPEC), **KW)
    monkeypatch.undo()
    assert sorted(kept) == [3, 5]
    for name in DENSITY_FILES:                              # checkpointing changes nothing
        assert open(os.path.join(a_dir, name), "rb").read() == open(os.path.join(b_dir, name), "rb").read(), name
    # back to the first checkpoint (after block 2): it carries the accumulators of two samples of two replicas a group
    os.replace(kept[3], checkpoint.path_of(b_dir))
    ck = checkpoint.load(b_dir)
    assert int(ck["next_block"]) == 3 and sorted(ck["extra"]) == ["density_hist", "density_samples"]
    assert np.array_equal(ck["extra"]["density_samples"], np.full(2, 4, dtype=np.uint64)) and ck["extra"]["density_hist"].dtype == np.uint64
    assert np.array_equal(ck["id_density"], density.identity_array(dict(SPEC, every=1, per_replica=False)))
    for name in DENSITY_FILES:
        os.remove(os.path.join(b_dir, name))
    # refused by name, before anything is touched: no --density, another grid, other types, per replica
    for other in (None, dict(SPEC, grid=(5, 4, 4)), dict(SPEC, types=[0]), dict(SPEC, per_replica=True)):
        with pytest.raises(ValueError, match="--density"):
            run_replicas(*INPUTS, b_dir, nb_block=4, resume=True, density=other, **KW)
    c = run_replicas(*INPUTS, b_dir, nb_block=4, resume=True, density=dict(SPEC), **KW)
    for name in DENSITY_FILES:
        assert open(os.path.join(a_dir, name), "rb").read() == open(os.path.join(b_dir, name), "rb").read(), name
    for key in ("energy", "counts", "chain_counters"):
        assert np.array_equal(b[key], c[key]), key
    assert int(_counts(b_dir)["samples"][0]) == 8


def test_a_run_without_the_option_writes_todays_files_and_checkpoint_keys(tmp_path):
    out = str(tmp_path / "Z")
    run_replicas(*INPUTS, out, nb_block=1, checkpoint_every=1, **KW)
    with np.load(checkpoint.path_of(out), allow_pickle=False) as z:
        assert not any(k.startswith("x_") or k == "id_density" for k in z.files)
    assert not any(n.startswith("density") for n in os.listdir(out))
    # and a run with it cannot be resumed from there
    with pytest.raises(ValueError, match="--density"):
        run_replicas(*INPUTS, out, nb_block=2, resume=True, density=dict(SPEC), **KW)


def test_the_command_line_refuses_density_without_replicas(capsys, tmp_path):
    base = ["-i", INPUTS[0], "-d", INPUTS[1], "-p", INPUTS[2], "-o", str(tmp_path)]
    for extra in (["--density", "8,8,8"], ["--density-types", "1"], ["--density-per-replica"]):
        with pytest.raises(SystemExit) as err:
            run.main(base + extra)
        assert err.value.code == 2
        assert "--density, --density-types and --density-per-replica need --replicas" in capsys.readouterr().err
    assert not os.listdir(tmp_path)
