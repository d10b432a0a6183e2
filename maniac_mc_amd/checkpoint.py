"""The checkpoint file of a replica farm: <outdir>/checkpoint/farm.ckpt (run_replicas(checkpoint_every=..., resume=...)).

One numpy.savez archive without pickle: the run's identity (format and ABI versions, block and step counts, seed, farm mode,
replicas, fugacities, frames, digests of the input files), the next block's index, the engine's state blocks
(Engine.state_export) and the Fortran driver's (mfarm_state_export), and the byte size of every output file of the run at that
moment.  It is written to a temporary name beside it, flushed and synced, and renamed over the old file: a killed run leaves
the previous checkpoint or the new one, never a torn one.  Nothing here needs the library or a device.

A checkpoint continues a run bit for bit on the same library build and the same GPU model only.
"""
from __future__ import annotations

import hashlib
import os

import numpy as np

FORMAT_VERSION = 1
DIR_NAME = "checkpoint"
FILE_NAME = "farm.ckpt"
TMP_NAME = FILE_NAME + ".tmp"
REWRITTEN = ("topology.data",)        # output files written anew every time (all others grow by appending)
ANALYSES = ("rdf", "energy_pairs", "density", "molecule_energy")     # the identity entries of the farm analyses, in the order check names them


def path_of(outdir):
    return os.path.join(outdir, DIR_NAME, FILE_NAME)


def digest(path):
    """sha256 of the file's bytes ('' for no file: a run without a reservoir)"""
    if not path:
        return ""
    h = hashlib.sha256()
    with open(path, "rb") as f:
        for part in iter(lambda: f.read(1 << 20), b""):
            h.update(part)
    return h.hexdigest()


def output_sizes(outdir, n_replicas):
    """{path relative to outdir: bytes} of the run's output files as they stand: replicas.dat and every file of every
    replica_NNNN directory"""
    sizes = {}
    stats = os.path.join(outdir, "replicas.dat")
    if os.path.isfile(stats):
        sizes["replicas.dat"] = os.path.getsize(stats)
    for r in range(n_replicas):
        d = f"replica_{r:04d}"
        full = os.path.join(outdir, d)
        if not os.path.isdir(full):
            continue
        for name in sorted(os.listdir(full)):
            p = os.path.join(full, name)
            if os.path.isfile(p):
                sizes[d + "/" + name] = os.path.getsize(p)
    return sizes


def identity(abi_version, nb_step, seed, mode, n_replicas, fugacities, frames, maniac, data, inc, reservoir_path):
    """What a resumed run must share with the run that wrote the checkpoint"""
    return dict(abi_version=int(abi_version), nb_step=int(nb_step), seed=int(seed), mode=str(mode), replicas=int(n_replicas),
                fugacities=np.asarray([] if fugacities is None else fugacities, dtype=np.float64),
                frames=np.asarray(sorted(frames), dtype=np.int64),
                digest_maniac=digest(maniac), digest_data=digest(data), digest_inc=digest(inc),
                digest_reservoir=digest(reservoir_path))


def save(outdir, ident, next_block, nb_block, mode_ran, engine_blocks, driver_block, sizes, extra=None):
    """Write <outdir>/checkpoint/farm.ckpt atomically (temporary name, flush, fsync, rename, fsync of the directory).
    ``extra``: {name: array} of further arrays a run carries (the histograms of --rdf), stored as x_<name> in the same archive;
    None or empty: the archive has exactly the keys it always had."""
    d = os.path.join(outdir, DIR_NAME)
    os.makedirs(d, exist_ok=True)
    names = sorted(sizes)
    arrays = dict(format=np.int64(FORMAT_VERSION), next_block=np.int64(next_block), nb_block=np.int64(nb_block),
                  mode_ran=np.str_(mode_ran), n_engine=np.int64(len(engine_blocks)),
                  driver=np.ascontiguousarray(np.frombuffer(driver_block, dtype=np.uint8)),
                  size_names=np.asarray(names, dtype=np.str_), size_bytes=np.asarray([sizes[n] for n in names], dtype=np.int64))
    for k, v in ident.items():
        arrays["id_" + k] = np.asarray(v)
    for i, b in enumerate(engine_blocks):
        arrays[f"engine_{i}"] = np.ascontiguousarray(np.frombuffer(b, dtype=np.uint8))
    for k, v in (extra or {}).items():
        arrays["x_" + str(k)] = np.ascontiguousarray(v)
    tmp, final = os.path.join(d, TMP_NAME), os.path.join(d, FILE_NAME)
    with open(tmp, "wb") as f:
        np.savez(f, **arrays)
        f.flush()
        os.fsync(f.fileno())
    os.replace(tmp, final)
    fd = os.open(d, os.O_RDONLY)
    try:
        os.fsync(fd)
    finally:
        os.close(fd)
    return final


def load(outdir):
    """The checkpoint of outdir as a dict (a leftover temporary file beside it is ignored); ValueError where there is none or
    it is of another format.  ck["extra"] = {name: array} of the arrays saved as ``extra`` (empty without any)."""
    p = path_of(outdir)
    if not os.path.isfile(p):
        raise ValueError(f"resume: no checkpoint at {p}")
    try:
        with np.load(p, allow_pickle=False) as z:
            ck = {k: z[k] for k in z.files}
    except Exception as err:
        raise ValueError(f"resume: {p} is not a checkpoint file ({err})") from None
    if "format" not in ck or int(ck["format"]) != FORMAT_VERSION:
        raise ValueError(f"resume: checkpoint format {int(ck['format']) if 'format' in ck else '?'}, this version reads format {FORMAT_VERSION}")
    ck["engine"] = [ck.pop(f"engine_{i}") for i in range(int(ck["n_engine"]))]
    ck["sizes"] = {str(n): int(b) for n, b in zip(ck.pop("size_names"), ck.pop("size_bytes"))}
    ck["extra"] = {k[2:]: ck.pop(k) for k in [k for k in ck if k.startswith("x_")]}
    return ck


_NAMES = dict(abi_version="ABI version", nb_step="nb_step", seed="seed", mode="mode", replicas="R (replicas)",
              fugacities="fugacities", frames="frames", digest_maniac="the input file's digest", digest_data="the data file's digest",
              digest_inc="the parameter file's digest", digest_reservoir="the reservoir (file's digest)",
              recalibrate="recalibrate_moves", rdf="rdf (--rdf, --rdf-pairs, --rdf-intra)",
              energy_pairs="energy_pairs (--energy-pairs, --energy-pairs-select)",
              density="density (--density, --density-types, --density-per-replica)",
              molecule_energy="molecule_energy (--molecule-energy, --molecule-energy-types)")


def check(ck, ident, nb_block):
    """ValueError naming the first thing in which the run asked for differs from the run that wrote the checkpoint.  A larger
    nb_block than recorded extends the run; one below the blocks already done is refused."""
    for k in ANALYSES:
        # (an entry only a run with the analysis has: the checkpointed run had it switched on and this one has not)
        if "id_" + k in ck and k not in ident:
            raise ValueError(f"resume: {_NAMES[k]} differs from the checkpoint's (checkpoint "
                             f"{np.asarray(ck['id_' + k]).tolist()!r}, this run without it)")
    for k, want in ident.items():
        got = ck.get("id_" + k)
        same = got is not None and np.asarray(got).shape == np.asarray(want).shape and np.array_equal(np.asarray(got), np.asarray(want))
        if not same:
            raise ValueError(f"resume: {_NAMES[k]} differs from the checkpoint's (checkpoint "
                             f"{None if got is None else np.asarray(got).tolist()!r}, this run {np.asarray(want).tolist()!r})")
    if int(nb_block) < int(ck["next_block"]) - 1:
        raise ValueError(f"resume: nb_block {int(nb_block)} is below the {int(ck['next_block']) - 1} blocks the checkpoint has done")


def truncate_outputs(outdir, sizes):
    """Every recorded output file back to its recorded size: what a killed run wrote after its last checkpoint goes away.
    ValueError where a recorded file is missing or shorter than recorded (the directory is not the checkpoint's run).  The
    files of REWRITTEN are left alone: the next block that writes them, or the end of the run, writes them whole."""
    sizes = {n: b for n, b in sizes.items() if n.split("/")[-1] not in REWRITTEN}
    for name, size in sizes.items():
        p = os.path.join(outdir, *name.split("/"))
        if not os.path.isfile(p):
            raise ValueError(f"resume: output file {p} of the checkpointed run is missing")
        if os.path.getsize(p) < size:
            raise ValueError(f"resume: output file {p} is shorter ({os.path.getsize(p)} bytes) than the checkpoint recorded ({size})")
    for name, size in sizes.items():
        p = os.path.join(outdir, *name.split("/"))
        if os.path.getsize(p) != size:
            with open(p, "r+b") as f:
                f.truncate(size)


def restate_block_count(outdir, sizes, old, new, name="trajectory.lammpstrj"):
    """A resumed run with another nb_block than the checkpointed one (an extended run): every frame already in a replica's
    trajectory states the run's block count -- the reference prints input%nb_block, I10, under ITEM: TIMESTEP in every
    frame -- so that field of the frames kept is rewritten in place (same width, same file size): the file is the one the
    run of `new` blocks would have written from the start."""
    if int(old) == int(new):
        return
    was, now = b"%10d" % int(old), b"%10d" % int(new)
    for rel in sizes:
        if rel.split("/")[-1] != name:
            continue
        p = os.path.join(outdir, *rel.split("/"))
        with open(p, "rb") as f:
            lines = f.read().split(b"\n")
        for i in range(1, len(lines)):
            if lines[i - 1] == b"ITEM: TIMESTEP" and lines[i] == was:
                lines[i] = now
        with open(p, "r+b") as f:
            f.write(b"\n".join(lines))
            f.flush()
            os.fsync(f.fileno())
