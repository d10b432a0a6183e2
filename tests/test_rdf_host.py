"""The host side of the radial distribution functions (maniac_mc_amd/rdf.py) without a device: the normalisation on hand-made
counts, the closed form of the eligible pairs against brute force, the half width of the triclinic cells, the option parsers
and the command line's refusals, and the rdf.dat writer's round trip."""
import itertools
import math

import numpy as np
import pytest

from maniac_mc_amd import rdf, run, synth
from tests import triclinic_cases
from tests.util import golden_system

SYSTEMS = {
    "spce216": lambda: golden_system("spce216")[1],
    "co2_20": lambda: golden_system("co2_20")[1],
    "mixture": lambda: golden_system("mixture")[1],
    "framework_small": lambda: golden_system("framework_small")[1],
    "triclinic_mild": lambda: triclinic_cases.cell("mild"),
    "triclinic_sheared": lambda: triclinic_cases.cell("sheared"),
    "adsorbate24": lambda: synth.rigid_adsorbate_box(),
    "adsorbate64": lambda: synth.large_adsorbate_box(n_sites=64, n_mol=4, L=34.0, seed=95),
}


def test_a_uniform_pair_density_gives_one_in_every_bin():
    # E eligible pairs spread uniformly over the volume V put E V_shell(b) / V into bin b: g = 1, as the formula states
    V, r_max, n_bins = 1000.0, 4.0, 8
    shell = rdf.shell_volumes(r_max, n_bins)
    assert np.allclose(shell.sum(), 4.0 * math.pi / 3.0 * r_max ** 3, rtol=1e-15)
    E = np.array([V * 7.0, V * 3.0])
    hist = E[:, None] * shell[None, :] / V                   # exact small multiples: 7 shell, 3 shell
    r_mid, g = rdf.normalise(hist, E, V, r_max)
    assert np.array_equal(r_mid, (np.arange(n_bins) + 0.5) * 0.5)
    assert np.allclose(g, 1.0, rtol=1e-15, atol=0.0)         # four roundings: the counts' quotient, two products, the quotient


def test_normalise_on_hand_made_counts():
    hist = np.array([[0, 2, 0, 5]], dtype=np.uint64)
    r_mid, g = rdf.normalise(hist, np.array([10], dtype=np.uint64), 64.0, 2.0)
    shell = 4.0 * math.pi / 3.0 * np.array([0.5 ** 3, 1.0 - 0.5 ** 3, 1.5 ** 3 - 1.0, 8.0 - 1.5 ** 3])
    assert np.array_equal(g[0], 64.0 * np.array([0.0, 2.0, 0.0, 5.0]) / (10.0 * shell))
    # pooling is the caller's: sums of counts, not means of g
    h2 = np.array([[1, 0, 0, 0], [0, 0, 0, 4]], dtype=np.uint64)
    _, gp = rdf.normalise(h2.sum(axis=0), np.uint64(6 + 2), 64.0, 2.0)
    assert np.array_equal(gp, 64.0 * np.array([1.0, 0.0, 0.0, 4.0]) / (8.0 * shell))
    # no eligible pairs: zero, not a division by zero
    assert not rdf.normalise(np.zeros((1, 4)), np.zeros(1), 64.0, 2.0)[1].any()


def test_bin_index_is_the_contracts_rule():
    r2 = np.array([0.0, 0.24, 0.25, 3.99, 4.0, 4.01, np.nextafter(4.0, 0.0)])
    b = rdf.bin_index(r2, 2.0, 4)
    assert b[:4].tolist() == [0, 0, 1, 3] and b[4] == -1 and b[5] == -1
    assert b[6] in (3, -1)                                   # the top edge: bin 3, or dropped where rounding gives 4


def _brute_force(s, n_mol, pairs, intra):
    topo = s.topo
    atoms = [(t, m, int(topo.atom_types[t, a]) - 1) for t in range(topo.n_res) for m in range(int(n_mol[t]))
             for a in range(int(topo.atoms_in_res[t]))]
    ty = np.array([a[2] for a in atoms])
    key = np.array([a[0] * (1 << 28) + a[1] for a in atoms])
    ii, jj = np.triu_indices(len(atoms), 1)
    out = []
    for a, b in pairs:
        sel = ((ty[ii] == a) & (ty[jj] == b)) | ((ty[ii] == b) & (ty[jj] == a))
        if not intra:
            sel &= key[ii] != key[jj]
        out.append(int(sel.sum()))
    return np.array(out, dtype=np.uint64)


@pytest.mark.parametrize("name", sorted(SYSTEMS))
@pytest.mark.parametrize("intra", [False, True])
def test_eligible_pairs_against_brute_force(name, intra):
    s = SYSTEMS[name]()
    nt = s.topo.n_atom_types
    pairs = list(itertools.combinations_with_replacement(range(nt), 2))
    if name == "framework_small":
        pairs = [(7, 0), (7, 7), (8, 9), (0, 0), (1, 2), (9, 6), (8, 8), (5, 5), (3, 3), (9, 9)]
    for n_mol in (s.n_mol, np.maximum(s.n_mol - 1, 0), np.where(s.topo.is_active == 1, 1, s.n_mol), np.zeros_like(s.n_mol)):
        got = rdf.eligible_pairs(s.topo, n_mol, pairs, intra)
        assert got.dtype == np.uint64 and np.array_equal(got, _brute_force(s, n_mol, pairs, intra)), (name, n_mol, intra)


def test_half_width():
    for name in ("mild", "sheared"):
        s = triclinic_cases.cell(name)
        m = np.asarray(s.box_matrix)
        a, b, c = m[:, 0], m[:, 1], m[:, 2]
        vol = abs(np.dot(a, np.cross(b, c)))
        want = 0.5 * min(vol / np.linalg.norm(np.cross(b, c)), vol / np.linalg.norm(np.cross(c, a)), vol / np.linalg.norm(np.cross(a, b)))
        got = rdf.half_width(m)
        print(name, got, want)
        assert abs(got - want) <= 4 * np.finfo(float).eps * want
        assert got < 0.5 * min(np.linalg.norm(a), np.linalg.norm(b), np.linalg.norm(c))
        assert abs(rdf.volume(m) - vol) <= 1e-12 * vol
    assert rdf.half_width(np.diag([30.0, 18.0, 24.5])) == 9.0
    assert rdf.half_width(np.diag([20.0, 20.0, 20.0])) == 10.0


def test_parse_spec_and_pairs():
    assert rdf.parse_spec("9.3,128") == dict(r_max=9.3, n_bins=128, every=1)
    assert rdf.parse_spec(" 12 , 1024 , 5 ") == dict(r_max=12.0, n_bins=1024, every=5)
    for bad in ("9.3", "9.3,128,1,2", "x,128", "9.3,12.5", "0,128", "-1,128", "9.3,0", "9.3,1025", "9.3,128,0", "nan,4"):
        with pytest.raises(ValueError, match="--rdf"):
            rdf.parse_spec(bad)
    assert rdf.parse_pairs("1-1,1-2, 3-2") == [(0, 0), (0, 1), (2, 1)]
    for bad in ("1", "1-2-3", "a-b", "0-1", "1-1,1-1", "1-2,2-1", ""):
        with pytest.raises(ValueError):
            rdf.parse_pairs(bad)
    nine = ",".join(f"{a}-{b}" for a, b in itertools.islice(itertools.combinations_with_replacement(range(1, 5), 2), 9))
    with pytest.raises(ValueError, match="limit is 8"):
        rdf.parse_pairs(nine)
    with pytest.raises(ValueError, match="outside"):
        rdf.check_pairs([(0, 4)], n_atom_types=4)


def test_default_pairs_are_the_active_types_atom_types():
    s = golden_system("framework_small")[1]
    assert rdf.default_pairs(s.topo) == [(7, 7), (7, 8), (7, 9), (8, 8), (8, 9), (9, 9)]
    s = golden_system("mixture")[1]
    d = rdf.default_pairs(s.topo)
    assert len(d) == 10
    with pytest.raises(ValueError, match="limit is 8"):
        rdf.check_pairs(d, s.topo.n_atom_types)


def test_command_line_refusals(capsys, tmp_path):
    base = ["-i", "x.maniac", "-d", "x.data", "-p", "x.inc", "-o", str(tmp_path)]
    for extra, text in ((["--rdf", "9,32"], "--rdf"), (["--rdf-pairs", "1-1"], "--rdf"), (["--rdf-intra"], "--rdf"),
                        (["--replicas", "2", "--rdf-pairs", "1-1"], "need --rdf"),
                        (["--replicas", "2", "--rdf", "9"], "R_MAX,N_BINS"),
                        (["--replicas", "2", "--rdf", "9,32", "--rdf-pairs", "1-1,1-1"], "twice"),
                        (["--replicas", "2", "--rdf", "9,2000"], "N_BINS")):
        with pytest.raises(SystemExit) as err:
            run.main(base + extra)
        assert err.value.code == 2
        msg = capsys.readouterr().err
        assert text in msg, (extra, msg)
    with pytest.raises(SystemExit):
        run.main(base + ["--rdf", "9,32"])
    assert "need --replicas" in capsys.readouterr().err


def test_rdf_dat_round_trip(tmp_path):
    rng = np.random.default_rng(3)
    Rn, pairs, n_bins, r_max, V = 5, [(0, 0), (2, 1)], 16, 6.5, 3000.0
    hist = rng.integers(0, 4000, (Rn, len(pairs), n_bins)).astype(np.uint64)
    elig = rng.integers(20000, 30000, (Rn, len(pairs))).astype(np.uint64)
    group = np.arange(Rn) % 2
    path = str(tmp_path / "rdf.dat")
    rdf.write_dat(path, hist, elig, group, pairs, V, r_max)
    with open(path) as f:
        lines = f.read().splitlines()
    assert lines[0].startswith("#") and all(k in lines[0] for k in ("group", "pair", "r_mid", "g(r)", "g_sem", "count"))
    assert len(lines) == 1 + 2 * len(pairs) * n_bins and len({len(ln) for ln in lines[1:]}) == 1, "fixed-width records"
    back = rdf.read_dat(path)
    assert sorted(back) == [(g, p) for g in (0, 1) for p in range(len(pairs))]
    for (g, p), d in back.items():
        sel = group == g
        r_mid, want = rdf.normalise(hist[sel, p].sum(axis=0), elig[sel, p].sum(), V, r_max)
        assert d["types"] == (pairs[p][0] + 1, pairs[p][1] + 1)
        assert np.array_equal(d["count"], hist[sel, p].sum(axis=0))
        assert np.allclose(d["r_mid"], r_mid, rtol=0, atol=5e-9) and np.allclose(d["g"], want, rtol=1e-8, atol=0)
        each = rdf.normalise(hist[sel, p], elig[sel, p], V, r_max)[1]
        assert np.allclose(d["sem"], np.std(each, axis=0, ddof=1) / math.sqrt(sel.sum()), rtol=1e-6, atol=0)
    # one replica in a group: no standard error to give
    rdf.write_dat(path, hist[:1], elig[:1], group[:1], pairs, V, r_max)
    assert not any(d["sem"].any() for d in rdf.read_dat(path).values())


def test_counts_file_is_reproducible(tmp_path):
    hist = np.arange(2 * 1 * 4, dtype=np.uint64).reshape(2, 1, 4)
    args = (hist, np.array([[9], [8]], dtype=np.uint64), np.array([3, 3], dtype=np.uint64), [0, 1], [(0, 1)], 5.0, 4, 1, False)
    rdf.write_counts(str(tmp_path / "a.npz"), *args)
    rdf.write_counts(str(tmp_path / "b.npz"), *args)
    assert open(tmp_path / "a.npz", "rb").read() == open(tmp_path / "b.npz", "rb").read()
    with np.load(tmp_path / "a.npz", allow_pickle=False) as z:
        assert sorted(z.files) == ["eligible", "every", "group", "hist", "include_intra", "n_bins", "pairs", "r_max", "samples"]
        assert np.array_equal(z["hist"], hist) and z["hist"].dtype == np.uint64 and z["pairs"].tolist() == [[0, 1]]
        assert float(z["r_max"]) == 5.0 and int(z["n_bins"]) == 4 and z["group"].tolist() == [0, 1]
