"""run_replicas with rdf, density and energy_pairs in ONE run: the three analyses do not see each other.  Every analysis file
is byte-equal to the file of a run with that option alone, every other output file to a run with no option; the checkpoint
holds exactly the three analyses' keys; the run cut back to its first checkpoint and resumed reproduces every file, byte for
byte.

The co2_gcmc fixture inputs at R = 4, two fugacity groups, 40 steps a block, three blocks."""
import os
import shutil

import numpy as np
import pytest

from maniac_mc_amd import checkpoint, density
from maniac_mc_amd import energy_pairs as ep
from maniac_mc_amd.replicas import run_replicas
from tests.util import GOLDEN

pytestmark = pytest.mark.gpu
D = os.path.join(GOLDEN, "runs", "co2_gcmc", "inputs")
INPUTS = (os.path.join(D, "system.maniac"), os.path.join(D, "system.data"), os.path.join(D, "system.inc"))
R = 4
KW = dict(replicas=R, seed=5, nb_step=40, nb_block=3, fugacities=[12.0, 30.0])
OPTIONS = dict(rdf=dict(r_max=4.0, n_bins=8), density=dict(grid=(5, 4, 3), types=[0, 1]), energy_pairs=dict())
FILES = dict(rdf=["rdf.dat", "rdf_counts.npz"],
             density=["density_counts.npz", "density_profiles.dat"] + [density.cube_name(g, t) for g in (0, 1) for t in (0, 1)],
             energy_pairs=[ep.FILE_NAME] + [os.path.join(f"replica_{r:04d}", ep.FILE_NAME) for r in range(R)])


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


def _together_and_alone(mode, tmp_path, **kw):
    """The tree of the run with all three options (run with **kw besides), after asserting that it is the sum of the runs
    with one option each and of the run with none"""
    run_replicas(*INPUTS, str(tmp_path / "all"), mode=mode, **OPTIONS, **KW, **kw)
    together = _tree(str(tmp_path / "all"))
    run_replicas(*INPUTS, str(tmp_path / "plain"), mode=mode, **KW)
    plain = _tree(str(tmp_path / "plain"))
    analysis_files = sorted(n for names in FILES.values() for n in names)
    assert sorted(set(together) - set(plain)) == analysis_files and not set(plain) - set(together)
    for name in sorted(plain):
        assert _without_dir(plain[name], tmp_path) == _without_dir(together[name], tmp_path), name
    for key, names in FILES.items():
        run_replicas(*INPUTS, str(tmp_path / key), mode=mode, **{key: OPTIONS[key]}, **KW)
        alone = _tree(str(tmp_path / key))
        assert sorted(set(alone) - set(plain)) == sorted(names), key
        for name in names:
            assert alone[name] == together[name], (key, name)
    return together


def test_device_mode_files_checkpoint_keys_and_resume(tmp_path, monkeypatch):
    kept = {}
    save = checkpoint.save

    def keeping(outdir, ident, next_block, *a, **k):
        path = save(outdir, ident, next_block, *a, **k)
        kept[int(next_block)] = path + f".{int(next_block)}"
        shutil.copyfile(path, kept[int(next_block)])
        return path
    monkeypatch.setattr(checkpoint, "save", keeping)
    together = _together_and_alone("device", tmp_path, checkpoint_every=1)
    monkeypatch.undo()
    out = str(tmp_path / "all")
    assert sorted(kept) == [2, 3, 4]
    for path in [checkpoint.path_of(out)] + list(kept.values()):
        with np.load(path, allow_pickle=False) as z:
            keys = sorted(k for k in z.files if k.startswith("x_") or k in ("id_rdf", "id_density", "id_energy_pairs"))
        assert keys == sorted(["x_rdf_hist", "x_rdf_eligible", "x_rdf_samples", "x_density_hist", "x_density_samples",
                               "id_rdf", "id_density", "id_energy_pairs"]), path
    # back to the first checkpoint (after block 1); the final files go, the per-replica ones are cut back by the resume
    os.replace(kept[2], checkpoint.path_of(out))
    assert int(checkpoint.load(out)["next_block"]) == 2
    for name in FILES["rdf"] + FILES["density"] + [ep.FILE_NAME]:
        os.remove(os.path.join(out, name))
    run_replicas(*INPUTS, out, mode="device", resume=True, checkpoint_every=1, **OPTIONS, **KW)
    resumed = _tree(out)
    assert sorted(resumed) == sorted(together)
    for name in sorted(together):
        assert resumed[name] == together[name], name


def test_host_mode_files(tmp_path):
    _together_and_alone("host", tmp_path)
