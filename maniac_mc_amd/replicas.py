"""A MANIAC input run as a farm of R independent replicas on one GPU, each writing the files one MANIAC run writes.

    run_replicas("input.maniac", "topology.data", "parameters.inc", "outputs/", replicas=64)

loads the reference's three input files (io_maniac), builds one FortranFarm of R chains of that system and runs the input's
nb_block blocks of nb_step steps per replica.  After every block the farm's Fortran writer (mfarm_write_block, with the
single chain's writers of maniac_output.f90) adds the block's records to every replica's energy.dat, number_<res>.dat,
moves.dat and log.maniac under <outdir>/replica_NNNN/; the replicas of the `frames` set also get trajectory.lammpstrj and
topology.data every block, and every replica gets its final topology.data (a restartable MANIAC input).  Where the engine
holds the coordinates (device-built and window farms) they come back in one snapshot launch per chunk of replicas
(Engine.farm_snapshot_raw).  <outdir>/replicas.dat holds, per block and fugacity group, the mean and standard error over the
replicas of the total energy and of every active type's molecule count.

Step-size recalibration, where the input asks for it, is farm-wide: the pooled counters after every block.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import os
import types

import numpy as np

from . import _lib, checkpoint, fortran_host, io_maniac
from . import energy_pairs as epairs_mod
from . import density as density_mod
from . import molecule_energy as molen_mod
from . import rdf as rdf_mod
from .fortran_host import FortranFarm
from .run import header_text, set_chain_state
from .system import KB_KCALMOL, NB_MAX_MOLECULE

MODES = ("auto", "windows", "device", "device_accept", "host")
SNAPSHOT_BYTES = 256 << 20          # a snapshot chunk's size at the types' capacities


def parse_frames(text, n_replicas):
    """--frames: "0,3,7" | "all" | "none" -> the sorted replica indices; ValueError on anything else or out of range."""
    text = str(text).strip()
    if text == "all":
        return tuple(range(n_replicas))
    if text == "none":
        return ()
    try:
        out = sorted({int(v) for v in text.split(",")})
    except ValueError:
        raise ValueError(f"--frames: expected a list of replica indices, 'all' or 'none', got {text!r}") from None
    if out and (out[0] < 0 or out[-1] >= n_replicas):
        raise ValueError(f"--frames: replica indices must lie in [0, {n_replicas - 1}]")
    return tuple(out)


def parse_fugacities(text):
    """--fugacities: "f1,f2,..." (the input's units, atm) -> list of positive floats."""
    try:
        out = [float(v) for v in str(text).split(",")]
    except ValueError:
        raise ValueError(f"--fugacities: expected comma-separated numbers, got {text!r}") from None
    if not out or any(not (f > 0.0) for f in out):
        raise ValueError("--fugacities: every fugacity must be positive")
    return out


def _with_fugacity(inp, f_atm):
    """The input with every active residue's fugacity set to f_atm (atm)."""
    res = [dataclasses.replace(r, fugacity_atm=float(f_atm)) if r.is_active == 1 else r for r in inp.residues]
    return dataclasses.replace(inp, residues=res)


def _stats(x):
    x = np.asarray(x, dtype=np.float64)
    sem = float(np.std(x, ddof=1) / np.sqrt(x.size)) if x.size > 1 else 0.0
    return float(np.mean(x)), sem


def run_replicas(maniac, data, inc, outdir, replicas, seed=None, reservoir_path=None, fugacities=None, frames=(0,),
                 mode="auto", device=0, nb_block=None, nb_step=None, mol_capacity=None, n_lanes=2, n_threads=8,
                 chunk=None, wide_triclinic=False, restart_from=None, audit=False, checkpoint_every=0, resume=False,
                 recalibrate_moves=None, rdf=None, energy_pairs=None, density=None, molecule_energy=None):
    """Run `replicas` independent chains of the input; returns a dict with the final energies (R, 5) in K (non-Coulomb,
    Coulomb, reciprocal, self, intramolecular), counts (R, n_active), chain counters (R, 8), the farm's counters, the
    mode that ran and the block timings.

    ``seed``: None -> the input's seed, else 1; replica r's stream is seeded from it and r.
    ``fugacities``: [f1, ..., fk] in the input's units (atm): replica r runs at f[r % k] for every active type (GCMC inputs
    only).  ``frames``: the replicas that write trajectory.lammpstrj and topology.data every block.
    ``mode``: "auto" -> windows where the engine's one-launch path applies, else device-built batched steps, else (triclinic
    boxes) host-built ones; "windows" | "device" | "device_accept" | "host" force one.  A triclinic input runs an explicit
    "windows", "device" or "device_accept" with the engine's triclinic moves switched on (Engine.set_triclinic_moves);
    "auto" keeps choosing "host" there.
    ``wide_triclinic``: True -> mode "windows" also takes a triclinic input with rigid molecules of 6 to 63 sites
    (Engine.farm_set_wide_triclinic); off by default: "windows" then raises for such an input, as it always did.  "auto" is
    not changed by it.
    ``chunk``: replicas per snapshot launch (default: about SNAPSHOT_BYTES at the types' capacities).
    ``restart_from``: a directory an earlier run_replicas wrote: replica r starts from
    <restart_from>/replica_NNNN/topology.data (read with the same input and parameter files; `data` still supplies the
    topology).  A NEW run from those configurations -- blocks count from 0, streams are seeded from `seed` and r as always --
    not a bit-continuation: topology.data holds positions to seven decimals.  Not with a reservoir, whose contents
    topology.data does not hold.
    ``audit``: True -> after the last block every replica's energy and S(k) are recomputed from scratch (FortranFarm.audit,
    one batched call) and written to <outdir>/audit.dat, one line per replica in kcal/mol: replica, running total, recomputed
    total, largest component difference, max |A(k) - S(k)|; the result gains ``recomputed_energy`` (R, 6) in K and ``audit``.
    ``checkpoint_every``: N > 0 -> after every N-th block's files are written, and after the last block's, the farm's whole
    state goes to <outdir>/checkpoint/farm.ckpt (maniac_mc_amd.checkpoint): the engine's state blocks, the Fortran driver's,
    the run's identity and the size of every output file.  0 (default): no checkpoint/ directory.
    ``resume``: True -> continue the run whose checkpoint lies in `outdir`: the same inputs, replicas, seed, mode, fugacities,
    frames and nb_step (ValueError naming what differs), nb_block at least the blocks done (a larger one extends the run: the
    block count the trajectory frames already written state, as the reference prints it in every frame, is restated).  The
    output files are cut back to their recorded sizes, engine and farm are created as for a fresh run and take the carried
    state -- generator states, unrounded coordinates, A(k), reservoirs, running energies, step sizes, counters -- and the blocks
    go on from the recorded index, appending: the files are those of the uninterrupted run, byte for byte, on the same
    library build and GPU model.  Works with a reservoir; not together with ``restart_from``.
    ``recalibrate_moves``: None -> the input's choice; True / False override it.
    ``rdf``: dict(r_max=..., n_bins=..., pairs=[(a, b), ...] (0-based atom types; default: every pair of the active types' atom
    types, at most 8), every=1, include_intra=False) -> after every `every`-th block one sample of every replica goes into the
    engine's histograms (Engine.rdf_accumulate; its time in seconds["rdf"]); after the last block <outdir>/rdf_counts.npz
    (hist, eligible, samples per replica, the spec, every replica's group) and <outdir>/rdf.dat (per fugacity group and pair:
    r_mid, g(r) pooled over the group's replicas and samples, its standard error over the replicas, the pooled raw count) are
    written (maniac_mc_amd.rdf).  A checkpoint then carries the accumulators, and a resumed run must ask for the same rdf.
    None (default): nothing of this, and every file is what it always was.
    ``energy_pairs``: dict(every=1, pairs=None) -> after every `every`-th block the energy by residue-type pair of every replica
    (FortranFarm.energy_pairs_sample; its time in seconds["energy_pairs"]) adds one line to
    <outdir>/replica_NNNN/energy_pairs.dat: the block, then per pair the five components and their sum in kcal/mol.  ``pairs``:
    [(a, b), ...] of 0-based residue types (default: every pair with at least one active type, e.g. guest-framework and
    guest-guest).  After the last block <outdir>/energy_pairs.dat holds, per fugacity group and pair, mean and standard error
    over the replicas (maniac_mc_amd.energy_pairs).  The sampling keeps no state: a checkpoint only records the option, and a
    resumed run must ask for the same.  None (default): nothing of this, and every file is what it always was.
    ``density``: dict(grid=(n0, n1, n2), types=[...] (0-based atom types; default: the atom types of the active residue types, at
    most 8), every=1, per_replica=False) -> after every `every`-th block one sample of every replica goes into the engine's
    density maps (Engine.density_accumulate; its time in seconds["density"]), one map per fugacity group and type, or per
    replica and type with per_replica; after the last block <outdir>/density_counts.npz (hist, samples, the spec, every
    replica's map and group), <outdir>/density_profiles.dat (per map, type and cell axis the slab densities) and one Gaussian
    cube file <outdir>/density_gGG_typeTT.cube per map and type (sites per cubic Angstrom over the cell, with the atoms of the
    inactive residue types) are written (maniac_mc_amd.density).  A checkpoint then carries the accumulators, and a resumed
    run must ask for the same density.  None (default): nothing of this, and every file is what it always was.
    ``molecule_energy``: dict(e_min=..., e_max=..., n_bins=..., types=None, every=1) -> after every `every`-th block every
    molecule of the 0-based ACTIVE residue ``types`` (default: every active type) of every replica adds its removal energy
    E(X) - E(X without m) to the engine's histograms of n_bins bins over [e_min, e_max) kcal/mol and one slot below, one above
    (FortranFarm.molecule_energy_sample; its time in seconds["molecule_energy"]); after the last block
    <outdir>/molecule_energy_counts.npz (hist, samples per replica, the spec, every replica's group) and
    <outdir>/molecule_energy.dat (per fugacity group and type: the bin centre, the probability density pooled over the group's
    replicas, its standard error over the replicas, the pooled raw count) are written (maniac_mc_amd.molecule_energy).  A
    checkpoint then carries the accumulators, and a resumed run must ask for the same molecule_energy.  None (default): nothing
    of this, and every file is what it always was.
    """
    import time
    if mode not in MODES:
        raise ValueError(f"mode must be one of {MODES}, got {mode!r}")
    R = int(replicas)
    if R < 1:
        raise ValueError("replicas must be at least 1")
    if restart_from is not None and reservoir_path:
        raise ValueError("restart_from cannot be combined with a reservoir: topology.data does not hold a reservoir's contents")
    if resume and restart_from is not None:
        raise ValueError("resume cannot be combined with restart_from: a resumed run continues its own checkpoint")
    if int(checkpoint_every) < 0:
        raise ValueError("checkpoint_every must be 0 (off) or a positive number of blocks")
    system, inp, dat = io_maniac.load_system(maniac, data, inc, with_data=True)
    rdat = io_maniac.read_lammps_data(reservoir_path, inp) if reservoir_path else None
    topo = system.topo
    n_res = topo.n_res
    active = [t for t in range(n_res) if topo.is_active[t] == 1]
    gcmc = inp.insertion_deletion_proba > 0.0
    if inp.swap_proba > 0.0:
        raise ValueError("replica farms have no swap moves: the input asks for swap_proba > 0")
    if fugacities is not None and not gcmc:
        raise ValueError("--fugacities needs a grand-canonical input (insertion_deletion_proba > 0)")
    frames = tuple(sorted({int(r) for r in frames}))
    if frames and (frames[0] < 0 or frames[-1] >= R):
        raise ValueError(f"frames must lie in [0, {R - 1}]")
    triclinic = system.is_triclinic()
    triclinic_moves = triclinic and mode in ("windows", "device", "device_accept")
    if mol_capacity is None:
        mol_capacity = [NB_MAX_MOLECULE if topo.is_active[t] == 1 else max(1, int(system.n_mol[t])) for t in range(n_res)]
    nb_block = inp.nb_block if nb_block is None else int(nb_block)
    nb_step = inp.nb_step if nb_step is None else int(nb_step)
    if seed is None:
        seed = inp.seed if inp.has_seed and inp.seed > 0 else 1
    # the analyses asked for, in the order every later loop takes them; the groups reach ctx once they are known
    ctx = types.SimpleNamespace(topo=topo, system=system, R=R, residue_names=[res.name for res in inp.residues],
                                group=None, fugacities=None)
    analyses = [mod.Sampler(option, ctx) for mod, option in ((rdf_mod, rdf), (density_mod, density), (epairs_mod, energy_pairs),
                                                             (molen_mod, molecule_energy))
                if option is not None]
    group = np.zeros(R, dtype=np.int64)
    if fugacities is not None:
        fugacities = [float(f) for f in fugacities]
        group = np.arange(R) % len(fugacities)
        fug_grid = np.array([[_with_fugacity(inp, fugacities[g]).fugacity_per_A3()[t] for t in active] for g in group])
    else:
        fug_grid = np.tile(np.array([inp.fugacity_per_A3()[t] for t in active])[None, :], (R, 1)) if gcmc else None
    ctx.group, ctx.fugacities = group, fugacities
    for s in analyses:
        s.check_size()
    gcmc_arg = dict(p_translation=inp.translation_proba, p_rotation=inp.rotation_proba, fugacity=fug_grid) if gcmc else None
    reservoir = io_maniac.reservoir_offsets(reservoir_path, inp) if reservoir_path else None
    recalibrate = bool(inp.recalibrate_moves) if recalibrate_moves is None else bool(recalibrate_moves)
    ident = ck = None
    if checkpoint_every or resume:
        ident = checkpoint.identity(_lib.ABI_VERSION, nb_step, seed, mode, R, fugacities, frames, maniac, data, inc, reservoir_path)
        ident["recalibrate"] = int(recalibrate)
        for s in sorted(analyses, key=lambda s: checkpoint.ANALYSES.index(s.name)):      # (the order checkpoint.check names them in)
            ident[s.name] = s.identity_array()
    if resume:
        ck = checkpoint.load(outdir)
        checkpoint.check(ck, ident, nb_block)
    initial = None
    if restart_from is not None:
        initial = []
        for r in range(R):
            path = os.path.join(restart_from, f"replica_{r:04d}", "topology.data")
            if not os.path.isfile(path):
                raise ValueError(f"restart_from: {path} is missing")
            s_r, _ = io_maniac.load_system(maniac, path, inc)
            for t in range(n_res):
                if int(s_r.n_mol[t]) > int(mol_capacity[t]):
                    raise ValueError(f"restart_from: {path} holds {int(s_r.n_mol[t])} molecules of residue type {t}, "
                                     f"above the capacity {int(mol_capacity[t])}")
            initial.append(s_r)
    device_build = (not triclinic or triclinic_moves) and mode != "host"
    farm = FortranFarm(system, R, device=device, seed=int(seed), translation_step=inp.translation_step,
                       rotation_step=inp.rotation_step_angle, p_translation=inp.translation_proba, n_threads=n_threads,
                       mol_capacity=mol_capacity, gcmc=gcmc_arg, n_lanes=n_lanes, device_build=device_build,
                       device_accept=mode == "device_accept", window=mode in ("auto", "windows"), reservoir=reservoir,
                       triclinic_moves=triclinic_moves, wide_triclinic=bool(wide_triclinic) and triclinic_moves, initial=initial)
    try:
        ran = "host" if not farm.device_build else ("windows" if farm.window else
                                                     ("device_accept" if farm.device_accept else "device"))
        if mode == "windows" and ran != "windows":
            raise ValueError("mode 'windows': the engine's one-launch farm window does not apply to this system")
        if ck is not None and str(ck["mode_ran"]) != ran:
            raise ValueError(f"resume: the farm mode taken ({ran}) differs from the checkpoint's ({str(ck['mode_ran'])})")
        H = fortran_host.lib()
        farm._select()
        hold = set_chain_state(H, farm.eng.h, system, inp, dat, mol_capacity, rdat)
        H.mchain_export_template()
        del hold
        headers = {}
        for r in range(R):
            g = int(group[r])
            if g not in headers:
                inp_g = _with_fugacity(inp, fugacities[g]) if fugacities is not None else inp
                headers[g] = header_text(inp_g, dat, maniac, data, inc, farm.eng, reservoir_path, rdat)
            H.mfarm_set_log_header(C.c_int(r), headers[g], C.c_int(len(headers[g])))
        root = os.path.join(outdir, "")
        for r in range(R):
            os.makedirs(os.path.join(root, f"replica_{r:04d}"), exist_ok=True)
        if chunk is None:
            per = sum(3 * (1 + int(topo.atoms_in_res[t])) * int(mol_capacity[t]) * 8 for t in active)
            chunk = max(1, SNAPSHOT_BYTES // max(1, per))
        in_frames = np.zeros(R, dtype=bool)
        in_frames[list(frames)] = True
        n_groups = len(fugacities) if fugacities is not None else 1
        names = [inp.residues[t].name for t in active]
        stats_path = os.path.join(root, "replicas.dat")
        times = dict(run=0.0, write=0.0, snapshot=0.0)
        for s in analyses:
            s.configure(farm, root, ck is not None)
            times[s.name] = 0.0

        def write(block, final):
            t0 = time.perf_counter()
            for c0 in range(0, R, int(chunk)):
                reps = np.arange(c0, min(R, c0 + int(chunk)), dtype=np.int32)
                what = np.full(reps.size, 2, dtype=np.int32) if final else np.where(in_frames[reps], 3, 0).astype(np.int32)
                snap, n_dbl = None, 0
                if farm.device_build and what.any():
                    ts = time.perf_counter()
                    snap, n_dbl = farm.eng.farm_snapshot_raw(reps[what != 0])
                    times["snapshot"] += time.perf_counter() - ts
                    farm._select()
                rc = H.mfarm_write_block(C.c_int(block), C.c_int(nb_block), C.c_int(nb_step), C.c_int(1 if final else 0),
                                         C.c_int(reps.size), reps.ctypes.data_as(C.POINTER(C.c_int)),
                                         what.ctypes.data_as(C.POINTER(C.c_int)), snap, C.c_longlong(n_dbl),
                                         root.encode())
                if rc:
                    raise RuntimeError(f"mfarm_write_block: code {rc} (block {block})")
            if final:
                times["write"] += time.perf_counter() - t0
                return
            e = np.array([farm.energy(r) for r in range(R)])
            total = (e[:, 0] + e[:, 1] + e[:, 2] + e[:, 3] + e[:, 4]) * KB_KCALMOL
            cnt = farm.counts()
            with open(stats_path, "w" if block == 0 else "a") as f:
                if block == 0:
                    f.write("#     block  group   fugacity_atm  replicas      total_mean       total_sem"
                            + "".join(f"  {('N_' + n):>14s}_mean  {('N_' + n):>14s}_sem" for n in names) + "\n")
                for g in range(n_groups):
                    sel = group == g
                    f_atm = fugacities[g] if fugacities is not None else \
                        (inp.residues[active[0]].fugacity_atm if active else 0.0)
                    m, s = _stats(total[sel])
                    line = f"{block:10d} {g:6d} {f_atm:14.6e} {int(sel.sum()):9d} {m:15.6f} {s:15.6f}"
                    for k in range(len(active)):
                        m, s = _stats(cnt[sel, k])
                        line += f" {m:19.6f} {s:18.6f}"
                    f.write(line + "\n")
            times["write"] += time.perf_counter() - t0

        def save_checkpoint(next_block):
            t0 = time.perf_counter()
            state = farm.checkpoint_state()
            extra = {}
            for s in analyses:
                extra.update(s.state(farm))
            checkpoint.save(outdir, ident, next_block, nb_block, ran, state["engine"], state["driver"],
                            checkpoint.output_sizes(outdir, R), extra=extra or None)
            times["checkpoint"] = times.get("checkpoint", 0.0) + time.perf_counter() - t0

        first = 1
        if ck is not None:
            # the files back to where the checkpoint left them, the carried state into the fresh engine and farm: no block 0
            checkpoint.truncate_outputs(outdir, ck["sizes"])
            checkpoint.restate_block_count(outdir, ck["sizes"], int(ck["nb_block"]), nb_block)
            farm.restore_state(dict(engine=ck["engine"], driver=ck["driver"]))
            for s in analyses:
                s.load(farm, ck["extra"])
            first = int(ck["next_block"])
        else:
            write(0, False)
        for block in range(first, nb_block + 1):
            t0 = time.perf_counter()
            farm.run(nb_step)
            if recalibrate:
                farm.recalibrate()
            times["run"] += time.perf_counter() - t0
            for s in analyses:
                if block % s.every == 0:
                    t0 = time.perf_counter()
                    s.sample(farm, block)
                    times[s.name] += time.perf_counter() - t0
            write(block, False)
            if checkpoint_every and (block % int(checkpoint_every) == 0 or block == nb_block):
                save_checkpoint(block + 1)
        write(nb_block, True)
        for s in analyses:
            s.finish(farm, root, inp, dat)
        _lib.check(0)
        energies = np.array([farm.energy(r) for r in range(R)])
        res = dict(energy=energies, counts=farm.counts(), chain_counters=farm.chain_counters(), counters=farm.counters(),
                   accepted=farm.accepted, mode=ran, seconds=times, group=group)
        if audit:
            a = farm.audit()
            run_k, rec_k = a["running"], a["recomputed"]
            with open(os.path.join(root, "audit.dat"), "w") as f:
                f.write("#  replica    running_total  recomputed_total   max_component_diff        max_|A-S|\n")
                for r in range(R):
                    # (the totals as energy.dat forms its own: the five components added in K, then kcal/mol)
                    tot_run = (run_k[r, 0] + run_k[r, 1] + run_k[r, 2] + run_k[r, 3] + run_k[r, 4]) * KB_KCALMOL
                    tot_rec = (rec_k[r, 0] + rec_k[r, 1] + rec_k[r, 2] + rec_k[r, 3] + rec_k[r, 4]) * KB_KCALMOL
                    f.write(f"{r:10d} {tot_run:16.6f} {tot_rec:17.6f} {a['energy_deviation'][r] * KB_KCALMOL:20.6e} "
                            f"{a['a_deviation'][r]:16.6e}\n")
            res["recomputed_energy"] = a["recomputed"]
            res["audit"] = a
        return res
    finally:
        farm.close()
