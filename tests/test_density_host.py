"""The host side of the density maps (maniac_mc_amd/density.py) without a device: the option's parsing and its error texts,
the normalisation of a hand-made count array (a uniform count gives N / V in an orthorhombic and in a sheared cell), the
profiles, the files' writers and readers -- the cube writer against a small expected file under tests/golden/ --, the identity
a checkpoint carries, and the command line's refusals."""
import os

import numpy as np
import pytest

from maniac_mc_amd import checkpoint, density, run, synth

GOLDEN_CUBE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "density", "small.cube")
SHEARED = np.array([[16.0, 0.0, 0.0], [8.0, 16.0, 0.0], [4.0, 8.0, 16.0]])


def test_spec_parsing_and_its_error_texts():
    assert density.parse_spec("32,16,8") == dict(grid=(32, 16, 8), every=1)
    assert density.parse_spec(" 1 , 1024 , 7 , 5 ") == dict(grid=(1, 1024, 7), every=5)
    for bad, text in (("32", "N0,N1,N2"), ("32,32", "N0,N1,N2"), ("1,2,3,4,5", "N0,N1,N2"), ("a,2,3", "integers"), ("2.5,2,3", "integers"),
                      ("0,2,3", "outside [1, 1024]"), ("2,1025,3", "outside [1, 1024]"), ("2,2,-3", "outside [1, 1024]"),
                      ("1024,1024,32", "exceeds the limit of 16777216"), ("2,2,2,0", "EVERY must be at least 1")):
        with pytest.raises(ValueError) as err:
            density.parse_spec(bad)
        assert "--density" in str(err.value) and text in str(err.value), (bad, str(err.value))
    assert density.parse_types("3,4") == [2, 3] and density.parse_types(" 1 ") == [0]
    for bad, text in (("", "T,T"), ("a", "T,T"), ("1-2", "T,T"), ("0,1", "start at 1"), ("2,2", "given twice"),
                      ("1,2,3,4,5,6,7,8,9", "the limit is 8")):
        with pytest.raises(ValueError) as err:
            density.parse_types(bad)
        assert text in str(err.value), (bad, str(err.value))
    with pytest.raises(ValueError, match="no atom type is selected"):
        density.check_types([])
    with pytest.raises(ValueError, match="atom type 5 is outside the data file's types"):
        density.check_types([0, 4], n_atom_types=4)
    assert density.check_types([3, 0], n_atom_types=4) == [3, 0]
    # the size: the limit and the size asked for are both named
    assert density.check_size((32, 32, 32), 8, 512) == (512 * 8 * 32 ** 3 + 512) * 8
    with pytest.raises(ValueError) as err:
        density.check_size((1024, 1024, 16), 8, 3)
    assert "the limit is 2147483648" in str(err.value) and str((3 * 8 * (1 << 24) + 3) * 8) in str(err.value)


def test_check_spec_defaults_and_identity():
    topo = synth.framework_water_box(n_water=4, n_frame=64).topo
    active = density.default_types(topo)
    assert active and all(t + 1 in topo.atom_types[1] for t in active) and active == sorted(active), "the guest's atom types"
    spec = density.check_spec(dict(grid=[8, 4, 2]), topo)
    assert spec == dict(grid=(8, 4, 2), types=active, every=1, per_replica=False)
    spec = density.check_spec(dict(grid=(8, 4, 2), types=[1, 0], every=3, per_replica=True), topo)
    assert density.identity_array(spec).tolist() == [8, 4, 2, 3, 1, 1, 0] and density.identity_array(spec).dtype == np.int64
    for bad, text in ((dict(types=[0]), "needs grid"), (dict(grid=(2, 2, 2), bins=3), "['bins'] unknown"),
                      (dict(grid=(2, 2)), "three voxel counts"), (dict(grid=(2, 2, 2), every=0), "every must be at least 1"),
                      (dict(grid=(2, 2, 2), types=[0, 0]), "given twice"), (dict(grid=(2, 2, 2), types=[99]), "outside the data file's types")):
        with pytest.raises(ValueError) as err:
            density.check_spec(bad, topo)
        assert text in str(err.value), (bad, str(err.value))
    # more than eight active atom types: an error that names the limit
    from maniac_mc_amd.system import Topology
    many = Topology(atoms_in_res=[9], atom_types=[list(range(1, 10))], charges=[[0.0] * 9], is_active=[1],
                    epsilon=np.ones((9, 9)), sigma=np.ones((9, 9)), names=["NINE"])
    assert density.default_types(many) == list(range(9))
    with pytest.raises(ValueError, match="9 atom types are selected, the limit is 8: name them with --density-types"):
        density.check_spec(dict(grid=(2, 2, 2)), many)
    assert density.check_spec(dict(grid=(2, 2, 2), types=[8]), many)["types"] == [8]
    with pytest.raises(ValueError, match="9 atom types are selected, the limit is 8"):
        density.check_types(list(range(9)))
    # the checkpoint names the option
    assert "--density" in checkpoint._NAMES["density"]
    with pytest.raises(ValueError, match="--density"):
        checkpoint.check({"id_density": density.identity_array(spec), "next_block": 1}, {}, 1)


@pytest.mark.parametrize("cell", ["orthorhombic", "sheared"])
def test_a_uniform_count_gives_n_over_v(cell):
    M = np.diag([18.0, 21.0, 24.0]) if cell == "orthorhombic" else SHEARED
    V = 18.0 * 21.0 * 24.0 if cell == "orthorhombic" else 4096.0
    assert density.volume(M) == pytest.approx(V, rel=1e-14)
    grid, per_voxel, samples = (5, 4, 3), 7, np.array([10, 4], dtype=np.uint64)
    hist = np.zeros((2, 2, grid[2], grid[1], grid[0]), dtype=np.uint64)
    hist[0, :] = per_voxel * 10                       # 10 samples of N = 7 x 60 sites each
    hist[1, 0] = per_voxel * 4
    rho = density.number_density(hist, samples, M)
    assert rho.shape == hist.shape
    assert np.allclose(rho[0], per_voxel * 60 / V, rtol=1e-14, atol=0) and np.allclose(rho[1, 0], per_voxel * 60 / V, rtol=1e-14, atol=0)
    assert not rho[1, 1].any()
    # the integral of the density is the mean number of sites
    assert np.isclose(rho[0, 0].sum() * V / 60, per_voxel * 60, rtol=1e-13)
    # no samples: zero, not a division by zero; one map with a scalar sample count
    assert not density.number_density(hist, np.zeros(2, dtype=np.uint64), M).any()
    assert np.allclose(density.number_density(hist[0, 0], 10, M), per_voxel * 60 / V, rtol=1e-14, atol=0)


def test_profiles_are_the_sums_along_each_axis():
    rng = np.random.default_rng(4)
    hist = rng.integers(0, 50, (2, 3, 4, 5, 6)).astype(np.uint64)       # (G, C, n2 = 4, n1 = 5, n0 = 6)
    p0, p1, p2 = density.profiles(hist)
    assert p0.shape == (2, 3, 6) and p1.shape == (2, 3, 5) and p2.shape == (2, 3, 4) and p0.dtype == np.uint64
    for v in range(6):
        assert np.array_equal(p0[..., v], hist[..., :, :, v].sum(axis=(-2, -1)))
    for v in range(5):
        assert np.array_equal(p1[..., v], hist[..., :, v, :].sum(axis=(-2, -1)))
    for v in range(4):
        assert np.array_equal(p2[..., v], hist[..., v, :, :].sum(axis=(-2, -1)))
    assert all(np.array_equal(p.sum(axis=-1), hist.sum(axis=(-3, -2, -1))) for p in (p0, p1, p2))


def test_profile_file_round_trip(tmp_path):
    rng = np.random.default_rng(5)
    hist = rng.integers(0, 1000, (2, 2, 3, 4, 5)).astype(np.uint64)
    samples = np.array([6, 0], dtype=np.uint64)
    path = str(tmp_path / "density_profiles.dat")
    density.write_profiles(path, hist, samples, [3, 0], SHEARED)
    lines = open(path).read().splitlines()
    assert lines[0].startswith("#") and len(lines) == 1 + 2 * 2 * (5 + 4 + 3) and len({len(ln) for ln in lines[1:]}) == 1, "fixed width"
    back = density.read_profiles(path)
    assert sorted(back) == [(g, c, k) for g in (0, 1) for c in (0, 1) for k in (0, 1, 2)]
    prof = density.profiles(hist)
    lengths = np.linalg.norm(SHEARED, axis=0)
    for (g, c, k), d in back.items():
        n = (5, 4, 3)[k]
        assert d["type"] == (4, 1)[c] and np.array_equal(d["count"], prof[k][g, c])
        assert np.allclose(d["s_mid"], (np.arange(n) + 0.5) / n, atol=5e-9) and np.allclose(d["x_mid"], d["s_mid"] * lengths[k], atol=1e-7)
        want = prof[k][g, c] / (6.0 * 4096.0 / n) if g == 0 else np.zeros(n)
        assert np.allclose(d["density"], want, rtol=1e-9, atol=0)
    with open(path, "w") as f:
        f.write("# something else\n")
    with pytest.raises(ValueError, match="not a density_profiles.dat"):
        density.read_profiles(path)


def _small_cube(path):
    rho = (np.arange(6, dtype=np.float64).reshape(3, 1, 2) + 0.5) * 1.0e-3          # (n2 = 3, n1 = 1, n0 = 2): rho[v2, 0, v0]
    atoms = [(14, 0.0, 0.0, 0.0), (8, 1.5, -2.25, 3.0), (0, -4.0, 2.0, -8.0)]
    density.write_cube(path, rho, SHEARED, [-4.0, 2.0, -8.0], atoms, title="map 0 atom type 2 samples 3")
    return rho, atoms


def test_cube_writer_against_the_expected_file(tmp_path):
    path = str(tmp_path / "small.cube")
    rho, atoms = _small_cube(path)
    assert open(path).read() == open(GOLDEN_CUBE).read()
    text = open(path).read().splitlines()
    assert "1/Angstrom^3" in text[0] and "bohr" in text[1]
    assert text[2].split()[0] == "3" and [ln.split()[0] for ln in text[3:6]] == ["2", "1", "3"]
    # the format's order: the first cell axis outermost, the third fastest
    values = [float(x) for ln in text[9:] for x in ln.split()]
    assert np.allclose(values, [rho[v2, 0, v0] for v0 in range(2) for v2 in range(3)], rtol=1e-5, atol=0)
    assert values == [0.0005, 0.0025, 0.0045, 0.0015, 0.0035, 0.0055]
    back = density.read_cube(path)
    assert np.allclose(back["rho"], rho, rtol=1e-5) and back["n"].tolist() == [2, 1, 3]
    assert np.allclose(back["origin"], [-4.0, 2.0, -8.0], atol=1e-6)
    # voxel vector k = column k of box%matrix over n_k
    assert np.allclose(back["vectors"], (SHEARED / np.array([2.0, 1.0, 3.0])[None, :]).T, atol=1e-6)
    assert [a[0] for a in back["atoms"]] == [14, 8, 0] and np.allclose([a[1:] for a in back["atoms"]], [a[1:] for a in atoms], atol=1e-6)
    assert density.cube_name(3, 1) == "density_g03_type02.cube"


def test_atomic_numbers_from_masses():
    assert [density.atomic_number(m) for m in (12.011, 15.9994, 1.008, 28.0855, 26.98, 65.38)] == [6, 8, 1, 14, 13, 30]
    assert density.atomic_number(1.0) == 1 and density.atomic_number(100.0) == 0 and density.atomic_number(0.0) == 0


def test_counts_file_has_equal_bytes_for_equal_counts(tmp_path):
    hist = np.arange(2 * 1 * 2 * 2 * 2, dtype=np.uint64).reshape(2, 1, 2, 2, 2)
    a, b = str(tmp_path / "a.npz"), str(tmp_path / "b.npz")
    for p in (a, b):
        density.write_counts(p, hist, [3, 3], [0, 1, 0, 1], [0, 1, 0, 1], [1], (2, 2, 2), 1, False)
    assert open(a, "rb").read() == open(b, "rb").read()
    with np.load(a, allow_pickle=False) as z:
        assert sorted(z.files) == ["every", "grid", "group", "group_of", "hist", "per_replica", "samples", "types"]
        assert z["hist"].dtype == np.uint64 and np.array_equal(z["hist"], hist) and z["samples"].tolist() == [3, 3]
        assert z["grid"].tolist() == [2, 2, 2] and z["types"].tolist() == [1] and int(z["per_replica"]) == 0


def test_command_line_refusals(capsys, tmp_path):
    base = ["-i", "x.maniac", "-d", "x.data", "-p", "x.inc", "-o", str(tmp_path)]
    for extra, text in ((["--density", "8,8,8"], "need --replicas"), (["--density-types", "1"], "need --replicas"),
                        (["--density-per-replica"], "need --replicas"),
                        (["--replicas", "2", "--density-types", "1"], "need --density"),
                        (["--replicas", "2", "--density-per-replica"], "need --density"),
                        (["--replicas", "2", "--density", "8,8"], "N0,N1,N2"),
                        (["--replicas", "2", "--density", "8,8,2000"], "outside [1, 1024]"),
                        (["--replicas", "2", "--density", "8,8,8", "--density-types", "1,1"], "twice")):
        with pytest.raises(SystemExit) as err:
            run.main(base + extra)
        assert err.value.code == 2
        msg = capsys.readouterr().err
        assert "--density" in msg and text in msg, (extra, msg)
