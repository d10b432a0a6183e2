"""Energies by residue-type pair of a replica farm (run_replicas(energy_pairs=...), --energy-pairs): the selection, the files
and the checkpoint identity.  Nothing here needs the library or a device.

The numbers come from Engine.energy_pairs_replicas: per replica and selected unordered pair (a, b) of residue types the five
components non_coulomb, coulomb, recip_coulomb, ewald_self, intra_coulomb in K.  A run writes

  <out>/replica_NNNN/energy_pairs.dat   a header naming the pairs by residue name, then one line per sampled block: the block
                                        index, then per pair the five components and their sum in kcal/mol, fixed-width %.6f;
  <out>/energy_pairs.dat                after the last block, built from those files: per fugacity group and pair the mean and
                                        the standard error over the group's replicas of every component and of the sum, each
                                        replica's value being its average over the sampled blocks.
"""
from __future__ import annotations

import os

import numpy as np

from .system import KB_KCALMOL

FILE_NAME = "energy_pairs.dat"
COMPONENTS = ("non_coulomb", "coulomb", "recip_coulomb", "ewald_self", "intra_coulomb")
COLUMNS = COMPONENTS + ("sum",)
MAX_PAIRS = 36
WIDTH = 18                      # of a number's column


def parse_spec(text):
    """--energy-pairs [EVERY] -> dict(every=EVERY) (default 1); ValueError naming the switch otherwise."""
    text = "" if text is None else str(text).strip()
    if text == "":
        return dict(every=1)
    try:
        every = int(text)
    except ValueError:
        raise ValueError(f"--energy-pairs: expected a number of blocks EVERY, got {text!r}") from None
    if every < 1:
        raise ValueError("--energy-pairs: EVERY must be at least 1")
    return dict(every=every)


def check_pairs(pairs, n_res):
    """[(a, b), ...] of 0-based residue types, each normalised to a <= b, in the caller's order; ValueError for an empty
    list, more than MAX_PAIRS, a type outside [0, n_res) or a duplicate."""
    out = []
    for p in pairs:
        a, b = int(p[0]), int(p[1])
        if not (0 <= a < n_res and 0 <= b < n_res):
            raise ValueError(f"energy_pairs: pair ({a}, {b}): residue types must lie in [0, {n_res - 1}]")
        ab = (min(a, b), max(a, b))
        if ab in out:
            raise ValueError(f"energy_pairs: pair ({a}, {b}) is a duplicate")
        out.append(ab)
    if not out:
        raise ValueError("energy_pairs: the selection is empty")
    if len(out) > MAX_PAIRS:
        raise ValueError(f"energy_pairs: at most {MAX_PAIRS} pairs")
    return out


def parse_select(text, names):
    """--energy-pairs-select NAME:NAME,... with the input's residue names -> [(a, b), ...] (0-based, a <= b, the order given);
    ValueError naming the switch for an unknown name, a duplicate or an empty list."""
    names = [str(n) for n in names]
    items = [x.strip() for x in str(text).split(",") if x.strip()]
    if not items:
        raise ValueError("--energy-pairs-select: expected NAME:NAME,..., got an empty list")
    out = []
    for item in items:
        parts = [x.strip() for x in item.split(":")]
        if len(parts) != 2 or not all(parts):
            raise ValueError(f"--energy-pairs-select: expected NAME:NAME, got {item!r}")
        for n in parts:
            if n not in names:
                raise ValueError(f"--energy-pairs-select: unknown residue name {n!r} (the input has {', '.join(names)})")
        a, b = names.index(parts[0]), names.index(parts[1])
        ab = (min(a, b), max(a, b))
        if ab in out:
            raise ValueError(f"--energy-pairs-select: pair {item!r} is a duplicate")
        out.append(ab)
    if len(out) > MAX_PAIRS:
        raise ValueError(f"--energy-pairs-select: at most {MAX_PAIRS} pairs")
    return out


def default_pairs(topo):
    """Every unordered pair of residue types with at least one ACTIVE type, ascending: what moves can change."""
    act = [int(x) == 1 for x in topo.is_active]
    return [(a, b) for a in range(topo.n_res) for b in range(a, topo.n_res) if act[a] or act[b]]


def pair_names(pairs, names):
    return [f"{names[a]}:{names[b]}" for a, b in pairs]


def check_spec(spec, topo):
    """run_replicas' ``energy_pairs`` dict -> dict(every, pairs), checked; ValueError naming what is wrong."""
    unknown = set(spec) - {"every", "pairs"}
    if unknown:
        raise ValueError(f"energy_pairs: takes every and pairs ({sorted(unknown)} unknown)")
    pairs = spec.get("pairs")
    out = dict(every=int(spec.get("every", 1)), pairs=check_pairs(default_pairs(topo) if pairs is None else pairs, topo.n_res))
    if out["every"] < 1:
        raise ValueError("energy_pairs: every must be at least 1")
    return out


def from_args(ap, a):
    """--energy-pairs, --energy-pairs-select of the parsed command line `a` -> run_replicas' ``energy_pairs`` dict, None
    without --energy-pairs; ap.error for the sub-option without it or an argument that does not parse.  The names of
    --energy-pairs-select are the input file's (a missing input file is reported by the caller)."""
    if a.energy_pairs is None and a.energy_pairs_select is not None:
        ap.error("--energy-pairs-select needs --energy-pairs [EVERY]")
    if a.energy_pairs is None:
        return None
    try:
        spec = parse_spec(a.energy_pairs)
        spec["pairs"] = None
        if a.energy_pairs_select is not None and os.path.isfile(a.maniac):
            from . import io_maniac
            names = [r.name for r in io_maniac.read_maniac_input(a.maniac).residues]
            spec["pairs"] = parse_select(a.energy_pairs_select, names)
    except ValueError as err:
        ap.error(str(err))
    return spec


def identity_array(spec):
    """What a resumed run must share: every, then the pairs, as int64"""
    return np.asarray([int(spec["every"])] + [int(v) for ab in spec["pairs"] for v in ab], dtype=np.int64)


# ---- per-replica file -------------------------------------------------------------------------------------------------------
def header_line(labels):
    """Line 1 of a per-replica file: the pairs by residue name, then what the columns hold"""
    return "# pairs: " + " ".join(labels) + " ; columns: block, then per pair " + " ".join(COLUMNS) + " (kcal/mol)\n"


def block_line(block, values_k):
    """One line of a per-replica file from (n_sel, 5) values in K: kcal/mol, the sum formed from the five in K first"""
    v = np.asarray(values_k, dtype=np.float64).reshape(-1, 5)
    out = f"{int(block):10d}"
    for row in v:
        total = (row[0] + row[1] + row[2] + row[3] + row[4]) * KB_KCALMOL
        out += "".join(f" {x * KB_KCALMOL:{WIDTH}.6f}" for x in row) + f" {total:{WIDTH}.6f}"
    return out + "\n"


def start_replica_file(path, labels):
    """A new file holding the header line"""
    with open(path, "w") as f:
        f.write(header_line(labels))


def append_replica_file(path, block, values_k):
    with open(path, "a") as f:
        f.write(block_line(block, values_k))


def read_replica_file(path):
    """(labels, blocks (n,), values (n, n_sel, 6) in kcal/mol as printed)"""
    with open(path) as f:
        lines = f.read().splitlines()
    if not lines or not lines[0].startswith("# pairs:"):
        raise ValueError(f"{path}: not an energy_pairs.dat file")
    labels = lines[0][len("# pairs:"):].split(";")[0].split()
    rows = [ln.split() for ln in lines[1:] if ln.strip() and not ln.startswith("#")]
    blocks = np.asarray([int(r[0]) for r in rows], dtype=np.int64)
    values = np.asarray([[float(x) for x in r[1:]] for r in rows], dtype=np.float64).reshape(len(rows), len(labels), len(COLUMNS))
    return labels, blocks, values


# ---- pooled file ------------------------------------------------------------------------------------------------------------
def _stats(x):
    x = np.asarray(x, dtype=np.float64)
    sem = float(np.std(x, ddof=1) / np.sqrt(x.size)) if x.size > 1 else 0.0
    return float(np.mean(x)), sem


def pooled(replica_paths, group):
    """(labels, n_blocks, {group: (n_replicas, mean (n_sel, 6), sem (n_sel, 6))}) from the per-replica files: a replica's value
    is its average over the sampled blocks, mean and standard error are taken over the group's replicas"""
    group = np.asarray(group, dtype=np.int64)
    labels, n_blocks, per = None, None, []
    for p in replica_paths:
        lab, blocks, values = read_replica_file(p)
        if labels is None:
            labels, n_blocks = lab, blocks.size
        elif lab != labels or blocks.size != n_blocks:
            raise ValueError(f"{p}: other pairs or another number of sampled blocks than the first replica's file")
        per.append(values.mean(axis=0) if blocks.size else np.zeros((len(lab), len(COLUMNS))))
    per = np.asarray(per).reshape(len(replica_paths), len(labels or []), len(COLUMNS))
    out = {}
    for g in sorted(set(group.tolist())):
        sel = group == g
        mean = np.zeros(per.shape[1:])
        sem = np.zeros(per.shape[1:])
        for p in range(per.shape[1]):
            for c in range(per.shape[2]):
                mean[p, c], sem[p, c] = _stats(per[sel, p, c])
        out[int(g)] = (int(sel.sum()), mean, sem)
    return labels, int(n_blocks or 0), out


def write_pooled_file(path, replica_paths, group, fugacities_atm=None):
    """<out>/energy_pairs.dat, whole: one line per (group, pair)"""
    labels, n_blocks, groups = pooled(replica_paths, group)
    with open(path, "w") as f:
        f.write(f"# energies by residue-type pair, kcal/mol: mean and standard error over a group's replicas of each replica's "
                f"average over {n_blocks} sampled blocks\n")
        f.write("# group   fugacity_atm  replicas  blocks " + f"{'pair':>16s}" +
                "".join(f" {(c + '_mean')[-WIDTH:]:>{WIDTH}s} {(c + '_sem')[-WIDTH:]:>{WIDTH}s}" for c in COLUMNS) + "\n")
        for g, (n_rep, mean, sem) in groups.items():
            f_atm = float(fugacities_atm[g]) if fugacities_atm is not None else 0.0
            for p, lab in enumerate(labels):
                f.write(f"{g:7d} {f_atm:14.6e} {n_rep:9d} {n_blocks:7d} {lab:>16s}" +
                        "".join(f" {mean[p, c]:{WIDTH}.6f} {sem[p, c]:{WIDTH}.6f}" for c in range(len(COLUMNS))) + "\n")


def read_pooled_file(path):
    """[(group, fugacity_atm, replicas, blocks, label, mean (6,), sem (6,)), ...] in the file's order"""
    out = []
    with open(path) as f:
        for ln in f:
            if ln.startswith("#") or not ln.strip():
                continue
            r = ln.split()
            nums = np.asarray([float(x) for x in r[5:]], dtype=np.float64).reshape(len(COLUMNS), 2)
            out.append((int(r[0]), float(r[1]), int(r[2]), int(r[3]), r[4], nums[:, 0].copy(), nums[:, 1].copy()))
    return out


class Sampler:
    """run_replicas' ``energy_pairs`` option as one of its farm analyses ("adding a farm analysis").  It keeps no
    state on the device: every sample goes to the replicas' files at once."""
    name = "energy_pairs"

    def __init__(self, option, ctx):
        self.ctx = ctx
        self.spec = check_spec(option, ctx.topo)
        self.every = self.spec["every"]

    def check_size(self):
        """(nothing of it depends on the groups)"""

    def identity_array(self):
        return identity_array(self.spec)

    def configure(self, farm, root, resumed):
        self.paths = [os.path.join(root, f"replica_{r:04d}", FILE_NAME) for r in range(self.ctx.R)]
        if not resumed:
            labels = pair_names(self.spec["pairs"], self.ctx.residue_names)
            for p in self.paths:
                start_replica_file(p, labels)

    def sample(self, farm, block):
        values = farm.energy_pairs_sample(self.spec["pairs"])
        for r, p in enumerate(self.paths):
            append_replica_file(p, block, values[r])

    def state(self, farm):
        return {}

    def load(self, farm, extra):
        pass

    def finish(self, farm, root, inp, dat):
        active = [t for t in range(self.ctx.topo.n_res) if self.ctx.topo.is_active[t] == 1]
        f_atm = self.ctx.fugacities if self.ctx.fugacities is not None else [inp.residues[active[0]].fugacity_atm if active else 0.0]
        write_pooled_file(os.path.join(root, FILE_NAME), self.paths, self.ctx.group, f_atm)
