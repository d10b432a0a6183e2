"""run_replicas(energy_pairs=...): the option changes nothing else -- every other output file, the energies and the counters
are those of the run without it, byte for byte -- every line of replica_NNNN/energy_pairs.dat is Engine.energy_pairs_replicas
at that block, the two default pairs' non-Coulomb entries add up to the running energy that energy.dat prints, and a run cut
back to its first checkpoint and resumed writes the files of the uninterrupted run, byte for byte.  A resume without the
option, with it after a run without, or with other pairs or another `every`, is refused by name.

The framework_water_gcmc fixture inputs (a 150-atom inactive FRAME + H2O) at R = 4, two fugacity groups, 40 steps a block.  The
values at each block come from a further identical run that watches FortranFarm.energy_pairs_sample; its files must be the
unobserved run's."""
import os
import shutil

import numpy as np
import pytest

from maniac_mc_amd import checkpoint, energy_pairs as ep
from maniac_mc_amd.fortran_host import FortranFarm
from maniac_mc_amd.replicas import run_replicas
from maniac_mc_amd.system import KB_KCALMOL
from tests.util import GOLDEN, farm_tol

pytestmark = pytest.mark.gpu
D = os.path.join(GOLDEN, "runs", "framework_water_gcmc", "inputs")
INPUTS = (os.path.join(D, "system.maniac"), os.path.join(D, "system.data"), os.path.join(D, "system.inc"))
R, STEPS = 4, 40
KW = dict(replicas=R, seed=5, nb_step=STEPS, fugacities=[40.0, 90.0])
DEFAULT = [(0, 1), (1, 1)]                      # FRAME:H2O, H2O:H2O
NEW_FILES = [ep.FILE_NAME] + [os.path.join(f"replica_{r:04d}", ep.FILE_NAME) for r in range(R)]


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


def _new_files(out):
    return {n: open(os.path.join(out, n), "rb").read() for n in NEW_FILES}


@pytest.mark.parametrize("mode", ["windows", "host"])
def test_outputs_unchanged_and_lines_are_the_engines_values(mode, tmp_path, monkeypatch):
    plain_dir, ep_dir, seen_dir = (str(tmp_path / n) for n in ("plain", "pairs", "seen"))
    plain = run_replicas(*INPUTS, plain_dir, nb_block=3, mode=mode, **KW)
    with_ep = run_replicas(*INPUTS, ep_dir, nb_block=3, mode=mode, energy_pairs=dict(), **KW)
    assert plain["mode"] == with_ep["mode"] == mode
    # ---- every other output file is byte-identical, and so are the returned energies and counters
    ta, tb = _tree(plain_dir), _tree(ep_dir)
    assert sorted(set(tb) - set(ta)) == sorted(NEW_FILES) and not set(ta) - set(tb)
    for name in sorted(ta):
        assert _without_dir(ta[name], tmp_path) == _without_dir(tb[name], tmp_path), name
    for key in ("energy", "counts", "chain_counters", "group"):
        assert np.array_equal(plain[key], with_ep[key]), key
    assert plain["counters"] == with_ep["counters"] and plain["accepted"] == with_ep["accepted"]
    assert "energy_pairs" not in plain["seconds"] and with_ep["seconds"]["energy_pairs"] > 0.0
    print(mode, "seconds", with_ep["seconds"])
    # ---- a further identical run, watched: the values, the three-pair matrix and the running energies at every sample
    seen = []                                             # [sample] -> (pairs, values (R, 2, 5), three (R, 3, 5), running (R, 5))
    sample = FortranFarm.energy_pairs_sample

    def watched(self, pairs, *a, **k):
        values = sample(self, pairs, *a, **k)
        three = self.eng.energy_pairs_replicas([(0, 0), (0, 1), (1, 1)])
        self._select()
        seen.append((list(pairs), values.copy(), three, np.array([self.energy(r) for r in range(R)])))
        return values
    monkeypatch.setattr(FortranFarm, "energy_pairs_sample", watched)
    run_replicas(*INPUTS, seen_dir, nb_block=3, mode=mode, energy_pairs=dict(), **KW)
    monkeypatch.undo()
    assert _new_files(seen_dir) == _new_files(ep_dir), "looking changed nothing"
    assert len(seen) == 3 and all(s[0] == DEFAULT for s in seen), "the default selection is FRAME:H2O, H2O:H2O"
    frame_frame = seen[0][2][0, 0]
    for r in range(R):
        labels, blocks, printed = ep.read_replica_file(os.path.join(ep_dir, f"replica_{r:04d}", ep.FILE_NAME))
        assert labels == ["FRAME:H2O", "H2O:H2O"] and blocks.tolist() == [1, 2, 3], "no block-0 line"
        lines = open(os.path.join(ep_dir, f"replica_{r:04d}", ep.FILE_NAME)).read().splitlines()
        energy_dat = np.loadtxt(os.path.join(ep_dir, f"replica_{r:04d}", "energy.dat"))
        for i, (pairs, values, three, running) in enumerate(seen):
            assert lines[1 + i] == ep.block_line(i + 1, values[r]).rstrip("\n")
            assert np.array_equal(three[r, 1:], values[r]), "a pair alone or among others: the same bits"
            assert np.array_equal(three[r, 0], frame_frame), "FRAME:FRAME is a constant"
            # energy.dat's line of that block prints these running energies (block, total, recip, non-coulomb, ...)
            row = energy_dat[energy_dat[:, 0] == i + 1][0]
            assert f"{row[3]:.6f}" == f"{running[r, 0] * KB_KCALMOL:.6f}"
            tol = farm_tol(running[r], (i + 1) * STEPS)
            assert abs(values[r, 0, 0] + values[r, 1, 0] - (running[r, 0] - frame_frame[0])) <= tol, (mode, r, i)
            assert abs(printed[i, 0, 0] + printed[i, 1, 0] - (row[3] - frame_frame[0] * KB_KCALMOL)) <= 1.6e-6, "three %.6f numbers"
    n_last = with_ep["counts"][:, 0].tolist()
    print(mode, "molecules at the end", n_last)
    # ---- the pooled file is built from the per-replica files
    rows = ep.read_pooled_file(os.path.join(ep_dir, ep.FILE_NAME))
    assert [(r[0], r[4]) for r in rows] == [(g, lab) for g in (0, 1) for lab in ("FRAME:H2O", "H2O:H2O")]
    per = np.array([ep.read_replica_file(os.path.join(ep_dir, f"replica_{r:04d}", ep.FILE_NAME))[2].mean(axis=0) for r in range(R)])
    for g, f_atm, n_rep, n_blocks, lab, mean, sem in rows:
        x = per[with_ep["group"] == g][:, ("FRAME:H2O", "H2O:H2O").index(lab), :]
        assert f_atm == KW["fugacities"][g] and n_rep == 2 and n_blocks == 3
        assert np.allclose(mean, x.mean(axis=0), rtol=0.0, atol=0.5000001e-6)
        assert np.allclose(sem, x.std(axis=0, ddof=1) / np.sqrt(2), rtol=0.0, atol=0.5000001e-6)


def test_every_and_a_selection(tmp_path):
    out = str(tmp_path / "every")
    res = run_replicas(*INPUTS, out, nb_block=3, energy_pairs=dict(every=2, pairs=[(1, 1), (1, 0), (0, 0)]), **KW)
    for r in range(R):
        labels, blocks, values = ep.read_replica_file(os.path.join(out, f"replica_{r:04d}", ep.FILE_NAME))
        assert labels == ["H2O:H2O", "FRAME:H2O", "FRAME:FRAME"] and blocks.tolist() == [2], "blocks 2 of 3: one line"
    assert res["mode"] == "windows"
    for bad in (dict(every=0), dict(pairs=[]), dict(pairs=[(0, 2)]), dict(pairs=[(0, 1), (1, 0)]), dict(each=2)):
        with pytest.raises(ValueError, match="energy_pairs"):
            run_replicas(*INPUTS, out, nb_block=1, energy_pairs=bad, **KW)


def test_a_run_cut_back_to_its_first_checkpoint_resumes_to_the_same_files(tmp_path, monkeypatch):
    a_dir, b_dir = str(tmp_path / "A"), str(tmp_path / "B")
    run_replicas(*INPUTS, a_dir, nb_block=4, energy_pairs=dict(), **KW)
    kept = {}
    save = checkpoint.save

    def keeping(outdir, ident, next_block, *a, **k):
        path = save(outdir, ident, next_block, *a, **k)
        kept[int(next_block)] = path + f".{int(next_block)}"
        shutil.copyfile(path, kept[int(next_block)])
        return path
    monkeypatch.setattr(checkpoint, "save", keeping)
    b = run_replicas(*INPUTS, b_dir, nb_block=4, checkpoint_every=2, energy_pairs=dict(), **KW)
    monkeypatch.undo()
    assert sorted(kept) == [3, 5]
    assert _new_files(a_dir) == _new_files(b_dir), "checkpointing changes nothing"
    # back to the first checkpoint (after block 2); the sampling is stateless: the checkpoint only records the option
    os.replace(kept[3], checkpoint.path_of(b_dir))
    ck = checkpoint.load(b_dir)
    assert int(ck["next_block"]) == 3 and not ck["extra"] and ck["id_energy_pairs"].tolist() == [1, 0, 1, 1, 1]
    os.remove(os.path.join(b_dir, ep.FILE_NAME))
    before = _tree(b_dir)
    # refused by name, before anything is touched: without the option, other pairs, another every
    for other in (None, dict(pairs=[(1, 1)]), dict(every=2)):
        with pytest.raises(ValueError, match="--energy-pairs"):
            run_replicas(*INPUTS, b_dir, nb_block=4, resume=True, energy_pairs=other, **KW)
    assert _tree(b_dir) == before
    c = run_replicas(*INPUTS, b_dir, nb_block=4, resume=True, energy_pairs=dict(), **KW)
    assert _new_files(a_dir) == _new_files(b_dir)
    for key in ("energy", "counts", "chain_counters"):
        assert np.array_equal(b[key], c[key]), key
    assert ep.read_replica_file(os.path.join(b_dir, "replica_0003", ep.FILE_NAME))[1].tolist() == [1, 2, 3, 4]


def test_a_run_without_the_option_writes_todays_checkpoint_keys(tmp_path):
    out = str(tmp_path / "Z")
    run_replicas(*INPUTS, out, nb_block=1, checkpoint_every=1, **KW)
    with np.load(checkpoint.path_of(out), allow_pickle=False) as z:
        assert not any(k.startswith("x_") or k in ("id_rdf", "id_energy_pairs") for k in z.files)
    assert not any(os.path.exists(os.path.join(out, n)) for n in NEW_FILES)
    before = _tree(out)
    # and a run with the option cannot be resumed from there
    with pytest.raises(ValueError, match="--energy-pairs"):
        run_replicas(*INPUTS, out, nb_block=2, resume=True, energy_pairs=dict(), **KW)
    assert _tree(out) == before
