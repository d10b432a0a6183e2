"""run_replicas(rdf=...): the option changes nothing else -- every other output file, the energies and the counters are those
of the run without it, byte for byte -- rdf_counts.npz holds the sum of the per-block oracle histograms of the same run,
rdf.dat is rdf.normalise of the pooled counts, and a run cut back to its first checkpoint and resumed writes the two files of
the uninterrupted run, byte for byte.  A resume without the option, or with other bins, is refused by name.

The co2_gcmc fixture inputs at R = 4, two fugacity groups, 40 steps a block.  The per-block coordinates come from a further
identical run whose samples are followed by Engine.get_molecules (exact: the engine's own doubles); its counts must be the
unobserved run's.  The oracle comparison asserts its margin first (tests/test_gpu_rdf.py)."""
import os
import shutil

import numpy as np
import pytest

from maniac_mc_amd import checkpoint, io_maniac, rdf
from maniac_mc_amd.fortran_host import FortranFarm
from maniac_mc_amd.replicas import run_replicas
from tests.test_gpu_rdf import expected_counts, oracle_distances
from tests.util import GOLDEN

pytestmark = pytest.mark.gpu
D = os.path.join(GOLDEN, "runs", "co2_gcmc", "inputs")
INPUTS = (os.path.join(D, "system.maniac"), os.path.join(D, "system.data"), os.path.join(D, "system.inc"))
R, STEPS = 4, 40
KW = dict(replicas=R, seed=5, nb_step=STEPS, fugacities=[12.0, 30.0])
SPEC = dict(r_max=25.0, n_bins=32, pairs=[(0, 0), (0, 1), (1, 1)])
RDF_FILES = ("rdf.dat", "rdf_counts.npz")


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
    with np.load(os.path.join(out, "rdf_counts.npz"), allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("mode", ["windows", "host"])
def test_outputs_unchanged_and_counts_are_the_oracles(mode, tmp_path, monkeypatch, refcpu_mod):
    plain_dir, rdf_dir, seen_dir = (str(tmp_path / n) for n in ("plain", "rdf", "seen"))
    plain = run_replicas(*INPUTS, plain_dir, nb_block=3, mode=mode, **KW)
    with_rdf = run_replicas(*INPUTS, rdf_dir, nb_block=3, mode=mode, rdf=dict(SPEC), **KW)
    assert plain["mode"] == with_rdf["mode"] == mode
    # ---- every other output file is byte-identical, and so are the returned energies and counters
    ta, tb = _tree(plain_dir), _tree(rdf_dir)
    assert sorted(set(tb) - set(ta)) == sorted(RDF_FILES) and not set(ta) - set(tb)
    for name in sorted(ta):
        assert _without_dir(ta[name], tmp_path) == _without_dir(tb[name], tmp_path), name
    for key in ("energy", "counts", "chain_counters", "group"):
        assert np.array_equal(plain[key], with_rdf[key]), key
    assert plain["counters"] == with_rdf["counters"] and plain["accepted"] == with_rdf["accepted"]
    assert "rdf" not in plain["seconds"] and with_rdf["seconds"]["rdf"] > 0.0
    print(mode, "seconds", with_rdf["seconds"])
    # ---- rdf_counts.npz = the per-block oracle histograms of the same run
    sites = []                                            # [block][replica] -> (n, 3, 3)
    sample = FortranFarm.rdf_sample

    def watched(self, *a, **k):
        sample(self, *a, **k)
        sites.append([self.eng.get_molecules(r, 0) for r in range(R)])
    monkeypatch.setattr(FortranFarm, "rdf_sample", watched)
    run_replicas(*INPUTS, seen_dir, nb_block=3, mode=mode, rdf=dict(SPEC), **KW)
    monkeypatch.undo()
    z, z_seen = _counts(rdf_dir), _counts(seen_dir)
    assert all(np.array_equal(z[k], z_seen[k]) for k in z), "looking at the coordinates changed nothing"
    assert len(sites) == 3
    s = io_maniac.load_system(*INPUTS)[0]
    want_h = np.zeros((R, 3, SPEC["n_bins"]), dtype=np.uint64)
    want_e = np.zeros((R, 3), dtype=np.uint64)
    for block in range(3):
        for r in range(R):
            oracle = oracle_distances(refcpu_mod, s.topo, s.box_matrix, s.bounds_lo, s.real_space_cutoff, s.ewald_tolerance, [sites[block][r]])
            h, e = expected_counts(oracle, SPEC["pairs"], SPEC["n_bins"], SPEC["r_max"], False, f"{mode} block {block + 1} replica {r}")
            assert np.array_equal(e, rdf.eligible_pairs(s.topo, [len(sites[block][r])], SPEC["pairs"], False))
            want_h[r] += h
            want_e[r] += e
    n_last = [len(x) for x in sites[-1]]
    print(mode, "molecules in the last block", n_last, "pairs counted", want_h.sum(axis=(1, 2)).tolist())
    assert len(set(n_last)) > 1 or len({len(x) for b in sites for x in b}) > 1, "insertions and deletions happened"
    assert z["hist"].dtype == np.uint64 and np.array_equal(z["hist"], want_h) and np.array_equal(z["eligible"], want_e)
    assert np.array_equal(z["samples"], np.full(R, 3, dtype=np.uint64))
    assert z["group"].tolist() == [0, 1, 0, 1] and z["pairs"].tolist() == [list(p) for p in SPEC["pairs"]]
    assert float(z["r_max"]) == SPEC["r_max"] and int(z["n_bins"]) == SPEC["n_bins"] and int(z["every"]) == 1 and int(z["include_intra"]) == 0
    # ---- rdf.dat parses and is rdf.normalise of the pooled counts
    back = rdf.read_dat(os.path.join(rdf_dir, "rdf.dat"))
    assert sorted(back) == [(g, p) for g in (0, 1) for p in range(3)]
    V = rdf.volume(s.box_matrix)
    for (g, p), d in back.items():
        sel = z["group"] == g
        r_mid, g_want = rdf.normalise(z["hist"][sel, p].sum(axis=0), z["eligible"][sel, p].sum(), V, SPEC["r_max"])
        assert d["types"] == (SPEC["pairs"][p][0] + 1, SPEC["pairs"][p][1] + 1)
        assert np.array_equal(d["count"], z["hist"][sel, p].sum(axis=0))
        assert np.allclose(d["r_mid"], r_mid, rtol=0, atol=5e-9) and np.allclose(d["g"], g_want, rtol=1e-8, atol=0)
    assert sum(int(d["count"].sum()) for d in back.values()) == int(z["hist"].sum()) > 0


def test_every_and_default_pairs(tmp_path):
    out = str(tmp_path / "every")
    res = run_replicas(*INPUTS, out, nb_block=3, rdf=dict(r_max=20.0, n_bins=8, every=2, include_intra=True), **KW)
    z = _counts(out)
    assert np.array_equal(z["samples"], np.full(R, 1, dtype=np.uint64)), "blocks 2 of 3"
    assert z["pairs"].tolist() == [[0, 0], [0, 1], [1, 1]] and int(z["include_intra"]) == 1 and int(z["every"]) == 2
    # with intramolecular pairs every CO2 counts its own two C-O pairs and one O-O pair: N molecules were there at block 2
    n = np.rint(np.sqrt(z["eligible"][:, 1].astype(np.float64) / 2)).astype(np.int64)          # C-O pairs = N x 2 N
    s = io_maniac.load_system(*INPUTS)[0]
    for r in range(R):
        assert np.array_equal(z["eligible"][r], rdf.eligible_pairs(s.topo, [n[r]], [(0, 0), (0, 1), (1, 1)], True))
    assert res["mode"] == "windows"
    with pytest.raises(ValueError, match="half the smallest perpendicular width"):
        run_replicas(*INPUTS, out, nb_block=1, rdf=dict(r_max=25.5, n_bins=8), **KW)
    with pytest.raises(ValueError, match="rdf"):
        run_replicas(*INPUTS, out, nb_block=1, rdf=dict(r_max=20.0, n_bins=0), **KW)
    assert s.topo.n_atom_types == 2


def test_a_run_cut_back_to_its_first_checkpoint_resumes_to_the_same_files(tmp_path, monkeypatch):
    a_dir, b_dir = str(tmp_path / "A"), str(tmp_path / "B")
    run_replicas(*INPUTS, a_dir, nb_block=4, rdf=dict(SPEC), **KW)
    kept = {}
    save = checkpoint.save

    def keeping(outdir, ident, next_block, *a, **k):
        path = save(outdir, ident, next_block, *a, **k)
        kept[int(next_block)] = path + f".{int(next_block)}"
        shutil.copyfile(path, kept[int(next_block)])
        return path
    monkeypatch.setattr(checkpoint, "save", keeping)
    b = run_replicas(*INPUTS, b_dir, nb_block=4, checkpoint_every=2, rdf=dict(SPEC), **KW)
    monkeypatch.undo()
    assert sorted(kept) == [3, 5]
    for name in RDF_FILES:                                  # checkpointing changes nothing
        assert open(os.path.join(a_dir, name), "rb").read() == open(os.path.join(b_dir, name), "rb").read(), name
    # back to the first checkpoint (after block 2): it carries the accumulators of two samples
    os.replace(kept[3], checkpoint.path_of(b_dir))
    ck = checkpoint.load(b_dir)
    assert int(ck["next_block"]) == 3 and sorted(ck["extra"]) == ["rdf_eligible", "rdf_hist", "rdf_samples"]
    assert np.array_equal(ck["extra"]["rdf_samples"], np.full(R, 2, dtype=np.uint64)) and ck["extra"]["rdf_hist"].dtype == np.uint64
    for name in RDF_FILES:
        os.remove(os.path.join(b_dir, name))
    # refused by name, before anything is touched: no --rdf, other bins, other pairs
    for other in (None, dict(SPEC, n_bins=64), dict(SPEC, pairs=[(0, 0)])):
        with pytest.raises(ValueError, match="rdf"):
            run_replicas(*INPUTS, b_dir, nb_block=4, resume=True, rdf=other, **KW)
    c = run_replicas(*INPUTS, b_dir, nb_block=4, resume=True, rdf=dict(SPEC), **KW)
    for name in RDF_FILES:
        assert open(os.path.join(a_dir, name), "rb").read() == open(os.path.join(b_dir, name), "rb").read(), name
    for key in ("energy", "counts", "chain_counters"):
        assert np.array_equal(b[key], c[key]), key
    assert int(_counts(b_dir)["samples"][0]) == 4


def test_a_run_without_the_option_writes_todays_checkpoint_keys(tmp_path):
    out = str(tmp_path / "Z")
    run_replicas(*INPUTS, out, nb_block=1, checkpoint_every=1, **KW)
    with np.load(checkpoint.path_of(out), allow_pickle=False) as z:
        assert not any(k.startswith("x_") or k == "id_rdf" for k in z.files)
    assert not any(os.path.exists(os.path.join(out, n)) for n in RDF_FILES)
    # and a run with it cannot be resumed from there
    with pytest.raises(ValueError, match="rdf"):
        run_replicas(*INPUTS, out, nb_block=2, resume=True, rdf=dict(SPEC), **KW)
