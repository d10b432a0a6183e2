"""checkpoint.save(..., extra=...) / load: further arrays of a run (the histograms of --rdf) travel in the same archive as
x_<name>; an archive without extras has exactly the keys it always had; a run's `rdf` identity is compared by name."""
import os

import numpy as np
import pytest

from maniac_mc_amd import checkpoint, rdf

KEYS_TODAY = {"format", "next_block", "nb_block", "mode_ran", "n_engine", "driver", "size_names", "size_bytes", "engine_0", "engine_1"}


def _ident(tmp_path, **more):
    paths = []
    for name in ("a.maniac", "a.data", "a.inc"):
        p = tmp_path / name
        p.write_text(name)
        paths.append(str(p))
    ident = checkpoint.identity(2, 40, 5, "windows", 3, [1.0, 2.0], (0,), *paths, None)
    ident["recalibrate"] = 0
    ident.update(more)
    return ident


def _save(out, ident, extra=None):
    """extra = None: the call as today's callers make it, without the keyword"""
    blocks = [np.arange(16, dtype=np.uint8), np.arange(8, dtype=np.uint8)]
    args = (str(out), ident, 3, 4, "windows", blocks, np.arange(32, dtype=np.uint8).tobytes(), {"replicas.dat": 120, "replica_0000/energy.dat": 64})
    return checkpoint.save(*args) if extra is None else checkpoint.save(*args, extra=extra)


def test_an_archive_without_extras_has_exactly_todays_keys(tmp_path):
    ident = _ident(tmp_path)
    for out, extra in ((tmp_path / "A", None), (tmp_path / "B", {})):
        path = _save(out, ident, extra)
        with np.load(path, allow_pickle=False) as z:
            assert set(z.files) == KEYS_TODAY | {"id_" + k for k in ident}
            assert not any(k.startswith("x_") for k in z.files)
        ck = checkpoint.load(str(out))
        assert ck["extra"] == {}
        checkpoint.check(ck, ident, 4)
    # the positional call of the callers there are has not changed
    a = np.load(checkpoint.path_of(str(tmp_path / "A")))
    b = np.load(checkpoint.path_of(str(tmp_path / "B")))
    assert all(np.array_equal(a[k], b[k]) for k in a.files)


def test_extra_arrays_round_trip_in_the_same_file(tmp_path):
    ident = _ident(tmp_path)
    rng = np.random.default_rng(1)
    extra = dict(rdf_hist=rng.integers(0, 2 ** 62, (3, 2, 8)).astype(np.uint64), rdf_eligible=np.full((3, 2), 2 ** 40, dtype=np.uint64),
                 rdf_samples=np.array([4, 4, 4], dtype=np.uint64), anything=np.linspace(0.0, 1.0, 5))
    path = _save(tmp_path / "C", ident, extra)
    assert sorted(os.listdir(os.path.dirname(path))) == [checkpoint.FILE_NAME], "one atomic file, no temporary left"
    with np.load(path, allow_pickle=False) as z:
        assert set(z.files) == KEYS_TODAY | {"id_" + k for k in ident} | {"x_" + k for k in extra}
    ck = checkpoint.load(str(tmp_path / "C"))
    assert sorted(ck["extra"]) == sorted(extra)
    for k, v in extra.items():
        assert ck["extra"][k].dtype == v.dtype and np.array_equal(ck["extra"][k], v)
    assert not any(k.startswith("x_") for k in ck)
    assert len(ck["engine"]) == 2 and ck["sizes"] == {"replicas.dat": 120, "replica_0000/energy.dat": 64}
    checkpoint.check(ck, ident, 4)


def test_the_rdf_identity_is_compared_by_name(tmp_path):
    spec = dict(r_max=9.0, n_bins=32, every=1, include_intra=False, pairs=[(0, 0), (0, 1)])
    with_rdf = _ident(tmp_path, rdf=rdf.identity_array(spec))
    without = _ident(tmp_path)
    _save(tmp_path / "D", with_rdf, {"rdf_samples": np.zeros(3, dtype=np.uint64)})
    _save(tmp_path / "E", without)
    ck_with, ck_without = checkpoint.load(str(tmp_path / "D")), checkpoint.load(str(tmp_path / "E"))
    checkpoint.check(ck_with, with_rdf, 4)
    with pytest.raises(ValueError, match="rdf"):
        checkpoint.check(ck_with, without, 4)                  # resumed without --rdf
    with pytest.raises(ValueError, match="rdf"):
        checkpoint.check(ck_without, with_rdf, 4)              # --rdf on a run that had none
    for change in (dict(n_bins=64), dict(r_max=8.5), dict(every=2), dict(include_intra=True), dict(pairs=[(0, 0)]),
                   dict(pairs=[(0, 0), (1, 1)])):
        other = _ident(tmp_path, rdf=rdf.identity_array(dict(spec, **change)))
        with pytest.raises(ValueError, match="rdf"):
            checkpoint.check(ck_with, other, 4)
    assert "id_rdf" not in np.load(checkpoint.path_of(str(tmp_path / "E"))).files
