"""The checkpoint file of a replica farm (maniac_mc_amd/checkpoint.py), without the library or a device: it round-trips from
synthetic blocks, every named mismatch raises a ValueError that names it, the output files are cut back to the recorded
sizes, and a leftover temporary file is ignored."""
import os

import numpy as np
import pytest

from maniac_mc_amd import checkpoint


def _inputs(tmp_path, reservoir=True):
    paths = {}
    for name in ("system.maniac", "system.data", "system.inc") + (("reservoir.data",) if reservoir else ()):
        p = tmp_path / name
        p.write_bytes(("contents of " + name).encode())
        paths[name] = str(p)
    return paths


def _identity(paths, **over):
    kw = dict(abi_version=2, nb_step=40, seed=5, mode="auto", n_replicas=3, fugacities=[0.5, 1.0], frames=(2, 0),
              maniac=paths["system.maniac"], data=paths["system.data"], inc=paths["system.inc"],
              reservoir_path=paths.get("reservoir.data"))
    kw.update(over)
    return checkpoint.identity(**kw)


def _outputs(root, R=3):
    """a tree as run_replicas leaves it: replicas.dat and a few files per replica"""
    (root / "replicas.dat").write_bytes(b"# header\n1 2 3\n")
    for r in range(R):
        d = root / f"replica_{r:04d}"
        d.mkdir(parents=True)
        (d / "energy.dat").write_bytes(b"e" * (10 + r))
        (d / "log.maniac").write_bytes(b"l" * (20 + r))
        (d / "topology.data").write_bytes(b"t" * 30)


def _saved(tmp_path, paths):
    rng = np.random.default_rng(1)
    out = tmp_path / "out"
    out.mkdir()
    _outputs(out)
    engine = [rng.integers(0, 256, 4096, dtype=np.uint8), rng.integers(0, 256, 808, dtype=np.uint8)]
    driver = rng.integers(0, 256, 1000, dtype=np.uint8).tobytes()          # (any bytes-like)
    sizes = checkpoint.output_sizes(str(out), 3)
    path = checkpoint.save(str(out), _identity(paths), 3, 4, "windows", engine, driver, sizes)
    return out, engine, driver, sizes, path


def test_round_trip_and_atomic_name(tmp_path):
    paths = _inputs(tmp_path)
    out, engine, driver, sizes, path = _saved(tmp_path, paths)
    assert path == checkpoint.path_of(str(out)) == str(out / "checkpoint" / "farm.ckpt")
    assert sorted(os.listdir(out / "checkpoint")) == ["farm.ckpt"], "the temporary name is gone"
    assert sizes["replicas.dat"] == 15 and sizes["replica_0002/energy.dat"] == 12 and len(sizes) == 1 + 3 * 3
    ck = checkpoint.load(str(out))
    assert int(ck["format"]) == checkpoint.FORMAT_VERSION and int(ck["next_block"]) == 3 and int(ck["nb_block"]) == 4
    assert str(ck["mode_ran"]) == "windows" and int(ck["id_abi_version"]) == 2 and int(ck["id_replicas"]) == 3
    assert len(ck["engine"]) == 2 and all(np.array_equal(a, b) for a, b in zip(ck["engine"], engine))
    assert ck["driver"].tobytes() == driver and ck["sizes"] == sizes
    assert ck["id_frames"].tolist() == [0, 2] and ck["id_fugacities"].tolist() == [0.5, 1.0]
    checkpoint.check(ck, _identity(paths), 4)
    checkpoint.check(ck, _identity(paths), 9)                      # a larger nb_block extends the run
    checkpoint.check(ck, _identity(paths), 2)                      # the blocks done, no more
    # the file holds no pickled object
    with np.load(path, allow_pickle=False) as z:
        assert all(z[k].dtype != object for k in z.files)
    # a second save replaces the first
    checkpoint.save(str(out), _identity(paths), 4, 4, "windows", engine, driver, sizes)
    assert int(checkpoint.load(str(out))["next_block"]) == 4 and sorted(os.listdir(out / "checkpoint")) == ["farm.ckpt"]


@pytest.mark.parametrize("change,named", [
    (dict(abi_version=3), "ABI version"), (dict(nb_step=41), "nb_step"), (dict(seed=6), "seed"), (dict(mode="device"), "mode"),
    (dict(n_replicas=4), "R"), (dict(fugacities=[0.5, 1.5]), "fugacities"), (dict(fugacities=None), "fugacities"),
    (dict(frames=(0,)), "frames")])
def test_each_mismatch_is_named(tmp_path, change, named):
    paths = _inputs(tmp_path)
    out = _saved(tmp_path, paths)[0]
    ck = checkpoint.load(str(out))
    with pytest.raises(ValueError, match=named):
        checkpoint.check(ck, _identity(paths, **change), 4)


@pytest.mark.parametrize("name,named", [("system.maniac", "input file"), ("system.data", "data file"), ("system.inc", "parameter file"),
                                        ("reservoir.data", "reservoir")])
def test_a_changed_input_file_is_named(tmp_path, name, named):
    paths = _inputs(tmp_path)
    out = _saved(tmp_path, paths)[0]
    ck = checkpoint.load(str(out))
    with open(paths[name], "ab") as f:
        f.write(b" ")
    with pytest.raises(ValueError, match=named):
        checkpoint.check(ck, _identity(paths), 4)


def test_other_refusals(tmp_path):
    paths = _inputs(tmp_path)
    out = _saved(tmp_path, paths)[0]
    ck = checkpoint.load(str(out))
    with pytest.raises(ValueError, match="reservoir"):             # a run without the reservoir the checkpoint had
        checkpoint.check(ck, _identity(paths, reservoir_path=None), 4)
    with pytest.raises(ValueError, match="nb_block"):
        checkpoint.check(ck, _identity(paths), 1)
    with pytest.raises(ValueError, match="no checkpoint"):
        checkpoint.load(str(tmp_path / "elsewhere"))
    # another format version, and a file that is no archive
    with np.load(checkpoint.path_of(str(out)), allow_pickle=False) as z:
        arrays = {k: z[k] for k in z.files}
    arrays["format"] = np.int64(checkpoint.FORMAT_VERSION + 1)
    with open(checkpoint.path_of(str(out)), "wb") as f:
        np.savez(f, **arrays)
    with pytest.raises(ValueError, match="format"):
        checkpoint.load(str(out))
    with open(checkpoint.path_of(str(out)), "wb") as f:
        f.write(b"not an archive")
    with pytest.raises(ValueError, match="not a checkpoint"):
        checkpoint.load(str(out))


def test_truncation_and_a_leftover_temporary_file(tmp_path):
    paths = _inputs(tmp_path)
    out, engine, driver, sizes, path = _saved(tmp_path, paths)
    before = {n: open(out / n, "rb").read() for n in sizes}
    # what a killed run leaves behind: bytes appended, a topology.data written anew, a new file, a torn temporary checkpoint
    for n in ("replicas.dat", "replica_0001/energy.dat", "replica_0002/log.maniac"):
        with open(out / n, "ab") as f:
            f.write(b"garbage after the checkpoint\n")
    (out / "replica_0000" / "topology.data").write_bytes(b"short")
    (out / "replica_0001" / "trajectory.lammpstrj").write_bytes(b"new")
    (out / "checkpoint" / checkpoint.TMP_NAME).write_bytes(b"torn")
    ck = checkpoint.load(str(out))
    assert ck["sizes"] == sizes and np.array_equal(ck["engine"][0], engine[0])
    checkpoint.truncate_outputs(str(out), ck["sizes"])
    for n in sizes:
        if n == "replica_0000/topology.data":
            assert open(out / n, "rb").read() == b"short", "files written anew every time are left alone"
        else:
            assert open(out / n, "rb").read() == before[n], n
    assert (out / "replica_0001" / "trajectory.lammpstrj").read_bytes() == b"new"
    # a recorded file that is missing or shorter: not the checkpoint's run, and nothing is cut
    with open(out / "replica_0002" / "log.maniac", "ab") as f:
        f.write(b"more")
    (out / "replica_0001" / "energy.dat").write_bytes(b"e")
    with pytest.raises(ValueError, match="shorter"):
        checkpoint.truncate_outputs(str(out), ck["sizes"])
    assert (out / "replica_0002" / "log.maniac").read_bytes().endswith(b"more")
    os.remove(out / "replica_0001" / "energy.dat")
    with pytest.raises(ValueError, match="missing"):
        checkpoint.truncate_outputs(str(out), ck["sizes"])


def test_an_extended_run_restates_the_block_count_of_its_frames(tmp_path):
    """every trajectory frame states the run's block count (the reference prints input%nb_block in every frame): a resume
    with a larger nb_block rewrites that field of the frames kept, and nothing else, at the same file size"""
    d = tmp_path / "replica_0000"
    d.mkdir()
    frame = b"ITEM: TIMESTEP\n         2\nITEM: NUMBER OF ATOMS\n         2\nITEM: ATOMS id type x y z\n1 1          2 0 0\n2 1 0          2 0\n"
    (d / "trajectory.lammpstrj").write_bytes(frame * 3)
    (d / "energy.dat").write_bytes(b"ITEM: TIMESTEP\n         2\n")
    sizes = {"replica_0000/trajectory.lammpstrj": 3 * len(frame), "replica_0000/energy.dat": 26}
    checkpoint.restate_block_count(str(tmp_path), sizes, 2, 2)
    assert (d / "trajectory.lammpstrj").read_bytes() == frame * 3
    checkpoint.restate_block_count(str(tmp_path), sizes, 2, 4)
    assert (d / "trajectory.lammpstrj").read_bytes() == frame.replace(b"TIMESTEP\n         2", b"TIMESTEP\n         4") * 3
    assert (d / "energy.dat").read_bytes() == b"ITEM: TIMESTEP\n         2\n", "only the trajectory"
