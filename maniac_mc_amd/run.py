"""One MANIAC run on the GPU engine: the reference's program flow (main.f90:16-33) for ONE chain.

    run_simulation("input.maniac", "topology.data", "parameters.inc", "outputs/")

reads the reference's three input files (io_maniac), creates the engine for one replica and hands
the state to the Fortran chain driver (fortran/mc_chain.f90), which mirrors MonteCarloLoop move by
move -- same random-number order -- and writes the reference's output files (fortran/
maniac_output.f90): log.maniac (Monte Carlo part), energy.dat, number_<res>.dat, moves.dat,
trajectory.lammpstrj, topology.data, and reservoir.lammpstrj when a reservoir topology is given
(the reference's ``-r`` option, cli_utils.f90:60-63).  Python here is plumbing only.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import _lib, fortran_host, io_maniac
from .engine import Engine, box_prepare
from .system import NB_MAX_MOLECULE

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int)


def _f(a):
    """Fortran (column-major) view of a 2-D array as a flat double pointer."""
    arr = np.asfortranarray(np.asarray(a, dtype=np.float64))
    return arr, arr.ctypes.data_as(_dp)


def _box_args(dat):
    box_type, volume, reciprocal, _ = box_prepare(dat["matrix"])
    m, mp = _f(dat["matrix"])
    r, rp = _f(reciprocal)
    lo = np.ascontiguousarray(dat["lo"], dtype=np.float64)
    hi = np.ascontiguousarray(dat["hi"], dtype=np.float64)
    tilt = np.ascontiguousarray(dat["tilt"], dtype=np.float64)
    keep = (m, r, lo, hi, tilt)
    return keep, (mp, rp, lo.ctypes.data_as(_dp), hi.ctypes.data_as(_dp), tilt.ctypes.data_as(_dp),
                  C.c_int(1 if dat["triclinic"] else 0), C.c_int(box_type), C.c_double(volume))


def _mol_arrays(com, off, n1):
    """(n, 3) / (n, n1, 3) numpy -> the Fortran shapes com(3, n) / off(3, n1, n)."""
    com = np.ascontiguousarray(np.asarray(com, dtype=np.float64).reshape(-1, 3))
    off = np.ascontiguousarray(np.asarray(off, dtype=np.float64).reshape(-1, n1, 3))
    return com, off


def header_text(inp, dat, maniac_path, data_path, inc_path, eng_or_ewald, reservoir_path=None, rdat=None):
    """The messages above "Started Monte Carlo Loop" as one byte string (one message per line) for mchain_set_log_header.
    File names are echoed as given, like the reference does.  ``eng_or_ewald``: an Engine, or the dict ewald_setup returns."""
    present = sorted({int(t) for i, r in enumerate(inp.residues) for t in dat["atom_types"][i, : r.nb_atoms] if t > 0})
    _, _, eps_raw, sig_raw = io_maniac.read_parameters(inc_path, dat["n_atom_types"], present, with_raw=True)
    if isinstance(eng_or_ewald, dict):
        ew = eng_or_ewald
    else:
        from .engine import ewald_setup
        _, _, _, metrics = box_prepare(dat["matrix"])
        ew = ewald_setup(metrics, inp.real_space_cutoff, inp.ewald_tolerance)
        assert ew["nk"] == eng_or_ewald.nk and ew["alpha"] == eng_or_ewald.alpha      # what the engine itself set up
    lines = io_maniac.log_header_lines(inp, dat, maniac_path, data_path, inc_path, eps_raw, sig_raw, ew,
                                       reservoir=(reservoir_path, rdat) if reservoir_path else None)
    return "\n".join(lines).encode("utf-8")


def set_chain_state(H, engine_h, system, inp, dat, mol_capacity, rdat=None):
    """mc_chain's state from the loaded input: box, residues (templates, molecules, bonded lists), tables, move parameters
    and, with a reservoir data file (rdat), the reservoir.  Returns the arrays the Fortran side was handed (keep them alive
    while it runs)."""
    topo = system.topo
    n_res = topo.n_res
    H.mchain_reset(engine_h, C.c_int(n_res), C.c_int(topo.n_atom_types), C.c_double(system.temperature))
    keep, args = _box_args(dat)
    H.mchain_set_box(*args)
    fug = inp.fugacity_per_A3()
    hold = []
    for t in range(n_res):
        n1 = int(topo.atoms_in_res[t])
        com, off = _mol_arrays(system.com[t], system.offsets[t], n1)
        types = np.ascontiguousarray(topo.atom_types[t, :n1], dtype=np.int32)
        q = np.ascontiguousarray(topo.charges[t, :n1], dtype=np.float64)
        hold += [com, off, types, q]
        H.mchain_set_residue(C.c_int(t + 1), inp.residues[t].name.encode(), C.c_int(n1), C.c_int(int(topo.is_active[t])),
                             C.c_int(int(mol_capacity[t])), C.c_int(com.shape[0]), types.ctypes.data_as(_ip),
                             q.ctypes.data_as(_dp), com.ctypes.data_as(_dp), off.ctypes.data_as(_dp),
                             C.c_double(float(fug[t])))
        for kind, key in enumerate(("bonds", "angles", "dihedrals", "impropers"), start=1):
            rows = dat["bonded_per_residue"][key][t]
            tab = np.zeros((max(1, len(rows)), 5), dtype=np.int32)
            for k, row in enumerate(rows):
                tab[k, : len(row)] = row
            hold.append(tab)
            H.mchain_set_bonded(C.c_int(t + 1), C.c_int(kind), C.c_int(len(rows)), tab.ctypes.data_as(_ip))
    masses = np.ascontiguousarray(dat["masses"], dtype=np.float64)
    ntypes = np.array([dat["type_counts"][k] for k in ("bonds", "angles", "dihedrals", "impropers")], dtype=np.int32)
    H.mchain_set_tables(masses.ctypes.data_as(_dp), ntypes.ctypes.data_as(_ip))
    H.mchain_set_moves(C.c_double(inp.translation_step), C.c_double(inp.rotation_step_angle),
                       C.c_double(inp.translation_proba), C.c_double(inp.rotation_proba),
                       C.c_int(1 if inp.recalibrate_moves else 0))
    if rdat is not None:
        rkeep, rargs = _box_args(rdat)
        any_bonded = np.array([1 if rdat["bonded_counts"][k] > 0 else 0
                               for k in ("bonds", "angles", "dihedrals", "impropers")], dtype=np.int32)
        H.mchain_set_reservoir_box(*rargs, any_bonded.ctypes.data_as(_ip))
        for t in range(n_res):
            n1 = int(topo.atoms_in_res[t])
            com, off = _mol_arrays(rdat["com"][t], rdat["off"][t], n1)
            hold += [com, off]
            H.mchain_set_reservoir_residue(C.c_int(t + 1), C.c_int(n1), C.c_int(NB_MAX_MOLECULE), C.c_int(com.shape[0]),
                                           com.ctypes.data_as(_dp), off.ctypes.data_as(_dp))
    return hold + [keep] + ([rkeep] if rdat is not None else [])


# one-launch windows for molecules of 6 to 63 sites: the default of run_simulation and of the command line.  Off until the path
# has been timed against the batched windows (LABNOTES round 10): --wide-chain-windows / wide_chain_windows=True turn it on
WIDE_CHAIN_WINDOWS_DEFAULT = False


def run_simulation(maniac_path, data_path, inc_path, outdir, seed=None, reservoir_path=None, device=0,
                   mol_capacity=None, nb_block=None, nb_step=None, seams=False, as_written=False, speculate=4,
                   chain_windows=True, chain_margin=None, wide_chain_windows=WIDE_CHAIN_WINDOWS_DEFAULT, chain_run=None,
                   chain_run_triclinic=False, chain_run_gcmc=False, chain_run_wide=False, wide_triclinic=False):
    """Run the chain; returns a dict with the final energies (K), counters, molecule counts, step sizes.

    ``seed``: None -> the input file's ``seed`` if present, else the generator is left unseeded
    (as the reference leaves it when the input names a seed, input_parser.f90:597).
    ``mol_capacity``: molecule slots per residue type (default: NB_MAX_MOLECULE for active types).
    ``seams``: True -> one engine call per reference seam (ComputePairInteractionEnergy_singlemol, ...), the literal
    integration of INTEGRATION.md; False (default) -> one batched call per move, same energies, ~3x fewer waits.
    ``as_written``: True -> the reference's deletion update exactly as written (A(k) gains the swapped-in
    molecule's terms, monte_carlo_utils.f90:308), composed in the host loop from neutral engine primitives; for
    charged grand-canonical runs this reproduces the reference's files but not the intended physics (default False).
    ``speculate``: K > 1 (default 4 -- measured best with one launch per window, where a longer window costs more than the
    steps it saves; batched mode only) -> the next K steps are drawn in the reference's random-number
    order assuming every one is rejected and evaluated in ONE engine call; the first accepted one is applied, the
    generator is put back to its state after that step and the rest is redrawn.  Same states, same files, up to
    1 / acceptance fewer round trips.  1 -> one step per engine call.
    ``chain_windows``: True (default; batched mode only) -> a window is ONE kernel launch (mgpu_chain_window): the engine
    evaluates its steps, applies the acceptance rule to them in order with the loop's own draws and commits the first
    accepted one, leaving to the loop only the steps too close to call; where the engine cannot (triclinic box, molecules
    of more than five sites without ``wide_chain_windows``) the loop falls back to the batched calls by itself.  False -> the
    batched calls always.
    ``wide_chain_windows``: True -> one-launch windows also for rigid molecules of 6 to 63 sites (mgpu_chain_set_wide; an
    orthorhombic box, the row form or an untiled wide form of the reciprocal update).  The files do not depend on it.
    ``chain_margin``: relative width of the band around an acceptance probability inside which the engine leaves the step to
    this loop's own exp (default: the engine's 16 ulp; tests widen it to drive the loop's side of that hand-over).
    ``chain_run``: None (default) -> windows as above.  (k, depth) -> an input without insertions / deletions runs each block
    as a CHAIN RUN (mgpu_chain_run_*): the block's steps are drawn ahead as records, the engine runs them in launches of up
    to k steps queued back to back -- each continues from the step cursor it finds on the device -- and the loop keeps
    ``depth`` launches in flight and books the results in order.  Same files.  Where the engine does not take the system
    (Engine.chain_run_capacity) or the input is grand-canonical, the loop keeps its windows by itself; the result's
    ``chain_run`` says which: dict(on, k, depth, launches, steps, void_launches, undecided).
    ``chain_run_triclinic``: True (with ``chain_run``) -> a TRICLINIC input's blocks are chain runs too: the engine is created
    with device-built triclinic moves and takes runs (Engine.chain_run_set_triclinic).  False (default): a triclinic input
    keeps its windows whatever ``chain_run`` says.  An orthorhombic input does not look at it.  ValueError without ``chain_run``.
    ``chain_run_gcmc``: True (with ``chain_run``) -> a GRAND-CANONICAL input's blocks are chain runs too, of by-count records
    (Engine.chain_run_set_gc / chain_run_push_gc): the launch that takes a record picks the molecule and forms the prefactor
    from the count it finds.  The loop draws a record ahead of the outcomes before it only while no count can reach 0 or the
    capacity; where that rule fails it takes steps through its windows (``chain_run['fallback_steps']``).  Same files as the
    windows.  Runs with ``as_written`` or a reservoir keep their windows (``on`` False), and so does a TRICLINIC grand-canonical
    input unless ``chain_run_triclinic`` is given as well: it takes both switches, and either alone leaves it its windows.  False
    (default): a grand-canonical input keeps its windows whatever ``chain_run`` says.  ValueError without ``chain_run``.
    ``chain_run`` in the result gains ``gcmc`` and ``fallback_steps``.
    ``chain_run_wide``: True (with ``chain_run``) -> an input with rigid molecules of 6 to 63 sites runs its blocks as chain runs
    too (Engine.chain_run_set_wide), NVT or -- with ``chain_run_gcmc`` -- grand-canonical.  Same files as the windows.  Runs with
    ``as_written`` or a reservoir and triclinic inputs (unless ``wide_triclinic``) keep their windows (``on`` False).  False
    (default): such an input keeps its windows whatever ``chain_run`` says.  ValueError without ``chain_run``.
    ``wide_triclinic``: True -> a TRICLINIC input with rigid molecules of 6 to 63 sites is taken by the single-chain one-launch
    paths (Engine.chain_set_wide_triclinic): ``wide_chain_windows`` and ``chain_run_wide`` then apply to it as they do to an
    orthorhombic input (runs still need ``chain_run_triclinic``, which creates the engine with device-built moves).  Same files.
    False (default): such an input does what it always did -- batched windows, no runs.  Other inputs do not look at it.
    """
    system, inp, dat = io_maniac.load_system(maniac_path, data_path, inc_path, with_data=True)
    rdat = io_maniac.read_lammps_data(reservoir_path, inp) if reservoir_path else None
    topo = system.topo
    n_res = topo.n_res
    if mol_capacity is None:
        mol_capacity = [NB_MAX_MOLECULE if topo.is_active[t] == 1 else max(1, int(system.n_mol[t])) for t in range(n_res)]
    if chain_run_triclinic and chain_run is None:
        raise ValueError("chain_run_triclinic needs chain_run=(k, depth)")
    if chain_run_gcmc and chain_run is None:
        raise ValueError("chain_run_gcmc needs chain_run=(k, depth)")
    if chain_run_wide and chain_run is None:
        raise ValueError("chain_run_wide needs chain_run=(k, depth)")
    run_tri = bool(chain_run_triclinic) and not seams and system.is_triclinic()
    eng = Engine.from_system(system, n_replicas=1, device=device, mol_capacity=mol_capacity, triclinic_moves=run_tri)
    if run_tri:
        eng.chain_run_set_triclinic(True)
    tri_wide = bool(wide_triclinic) and not seams and system.is_triclinic()
    if tri_wide:
        eng.chain_set_wide_triclinic(True)
    if chain_run_wide and not seams and not as_written and rdat is None and (not system.is_triclinic() or tri_wide):
        eng.chain_run_set_wide(True)
    if chain_margin is not None:
        eng.chain_set_margin(float(chain_margin))
    H = fortran_host.lib()
    H.mchain_run.restype = C.c_int
    try:
        hold = set_chain_state(H, eng.h, system, inp, dat, mol_capacity, rdat)
        H.mchain_set_mode(C.c_int(1 if seams else 0))
        H.mchain_set_as_written(C.c_int(1 if as_written else 0))
        H.mchain_set_speculation(C.c_int(1 if seams else max(1, int(speculate))))
        H.mchain_set_chain_windows(C.c_int(1 if chain_windows else 0))
        H.mchain_set_wide_windows(C.c_int(1 if wide_chain_windows else 0))
        k_run, depth_run = (0, 3) if chain_run is None or seams else (int(chain_run[0]), int(chain_run[1]))
        fortran_host.set_chain_run(k_run, depth_run)
        fortran_host.set_chain_run_gcmc(bool(chain_run_gcmc) and not seams)
        H.mchain_get_loop_seconds.restype = C.c_double
        header = header_text(inp, dat, maniac_path, data_path, inc_path, eng, reservoir_path, rdat)
        H.mchain_set_log_header(header, C.c_int(len(header)))
        if seed is None:
            seed = inp.seed if inp.has_seed else 0
        outdir = os.path.join(outdir, "")
        os.makedirs(outdir, exist_ok=True)
        import time
        t_loop = time.perf_counter()
        rc = H.mchain_run(C.c_int(inp.nb_block if nb_block is None else nb_block),
                          C.c_int(inp.nb_step if nb_step is None else nb_step), C.c_int(int(seed)), outdir.encode())
        t_loop = time.perf_counter() - t_loop       # initial energy + Monte Carlo loop + files
        _lib.check(rc)
        e = np.zeros(6); cnt = np.zeros(8, dtype=np.int32); nm = np.zeros(n_res, dtype=np.int32); st = np.zeros(2)
        H.mchain_get_energy(e.ctypes.data_as(_dp))
        H.mchain_get_counters(cnt.ctypes.data_as(_ip))
        H.mchain_get_counts(nm.ctypes.data_as(_ip))
        H.mchain_get_steps(st.ctypes.data_as(_dp))
        mc_seconds = float(H.mchain_get_loop_seconds())
        times = np.zeros(3)
        H.mchain_get_times(times.ctypes.data_as(_dp))
        chain_stats = eng.chain_stats()
        run_mode = fortran_host.chain_run_mode()
        run_stats = dict(zip(("on", "k", "depth", "launches", "steps", "void_launches", "undecided"), run_mode + eng.chain_run_stats()))
        run_stats["gcmc"], run_stats["fallback_steps"] = fortran_host.chain_run_gcmc_mode()
        e_final = eng.system_energy(0)
    finally:
        eng.close()
    keys = ("non_coulomb", "coulomb", "recip_coulomb", "ewald_self", "intra_coulomb", "total")
    # loop_seconds: mchain_run as a whole (initial energy, Monte Carlo loop, every output file); mc_seconds: the Monte
    # Carlo steps alone; chain_windows: (one-launch windows, windows with a step left to the host's exp)
    return dict(energy=dict(zip(keys, e)), recomputed_energy=e_final, counters=cnt, n_mol=nm, loop_seconds=t_loop,
                mc_seconds=mc_seconds, init_seconds=float(times[0]), file_seconds=float(times[2]), chain_windows=chain_stats, translation_step=st[0], rotation_step=st[1],
                chain_run=run_stats)


def parse_chain_run(text):
    """--chain-run K[,DEPTH] -> (k, depth); depth defaults to 3."""
    parts = [p.strip() for p in str(text).split(",")]
    if len(parts) not in (1, 2) or not all(p.isdigit() for p in parts):
        raise ValueError(f"--chain-run takes K or K,DEPTH (positive integers), not {text!r}")
    k, depth = int(parts[0]), int(parts[1]) if len(parts) == 2 else 3
    if k < 1 or depth < 1:
        raise ValueError("--chain-run: K and DEPTH must be at least 1")
    return k, depth


def main(argv=None):
    """`python -m maniac_mc_amd.run -i input.maniac -d topology.data -p parameters.inc [-r reservoir.data] [-o outputs/]`
    -- the reference's command line (cli_utils.f90:36-83: -i, -d, -p mandatory, -r optional, -o defaults to
    outputs/), plus --seed and --device; --replicas R runs R independent replicas on one GPU (maniac_mc_amd.replicas)."""
    import argparse
    import sys
    ap = argparse.ArgumentParser(prog="python -m maniac_mc_amd.run", description=main.__doc__)
    ap.add_argument("-i", dest="maniac", required=True, help="MANIAC input file")
    ap.add_argument("-d", dest="data", required=True, help="LAMMPS data file (atom_style full)")
    ap.add_argument("-p", dest="inc", required=True, help="pair_coeff include file")
    ap.add_argument("-r", dest="reservoir", default=None, help="reservoir data file")
    ap.add_argument("-o", dest="out", default="outputs/", help="output directory")
    ap.add_argument("--seed", type=int, default=None)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--speculate", type=int, default=4,
                    help="speculative window: steps evaluated per engine call (same states and files; 1: one step per call)")
    ap.add_argument("--no-chain-windows", action="store_true",
                    help="evaluate windows through the batched submit / wait calls instead of the one-launch path")
    ap.add_argument("--wide-chain-windows", dest="wide_chain_windows", action="store_true", default=WIDE_CHAIN_WINDOWS_DEFAULT,
                    help="one-launch windows also for rigid molecules of 6 to 63 sites")
    ap.add_argument("--no-wide-chain-windows", dest="wide_chain_windows", action="store_false",
                    help="such molecules' windows through the batched calls")
    ap.add_argument("--chain-run", dest="chain_run", default=None, metavar="K[,DEPTH]",
                    help="NVT inputs: run each block as a chain run of K steps per launch, DEPTH (default 3) launches in flight")
    ap.add_argument("--chain-run-triclinic", dest="chain_run_triclinic", action="store_true",
                    help="with --chain-run: a triclinic input's blocks are chain runs too (off by default: such an input keeps its windows; "
                         "a triclinic grand-canonical input needs --chain-run-gcmc as well)")
    ap.add_argument("--chain-run-gcmc", dest="chain_run_gcmc", action="store_true",
                    help="with --chain-run: a grand-canonical input's blocks are chain runs too (off by default: such an input keeps its windows; "
                         "a triclinic grand-canonical input needs --chain-run-triclinic as well)")
    ap.add_argument("--chain-run-wide", dest="chain_run_wide", action="store_true",
                    help="with --chain-run: an input with rigid molecules of 6 to 63 sites runs its blocks as chain runs too (off by "
                         "default: such an input keeps its windows; not for reservoirs or --as-written, and for triclinic inputs "
                         "only with --wide-triclinic)")
    ap.add_argument("--wide-triclinic", dest="wide_triclinic", action="store_true",
                    help="a triclinic input with rigid molecules of 6 to 63 sites: --wide-chain-windows and --chain-run-wide apply to it "
                         "(off by default: such an input keeps its batched windows); with --replicas: --farm-mode windows applies to it "
                         "(off by default: that mode then stops for such an input)")
    ap.add_argument("--as-written", action="store_true",
                    help="the reference's deletion update exactly as written (SURVEY F3) instead of the intended physics")
    ap.add_argument("--replicas", type=int, default=None,
                    help="run R independent replicas of the input on one GPU, each writing its files to <out>/replica_NNNN/")
    ap.add_argument("--fugacities", default=None,
                    help="with --replicas, GCMC inputs: f1,f2,... (atm); replica r runs at f[r %% k] (an isotherm)")
    ap.add_argument("--frames", default="0",
                    help="with --replicas: replicas writing trajectory / topology every block: 0,3,7 | all | none (default 0)")
    ap.add_argument("--farm-mode", default="auto", choices=("auto", "windows", "device", "device_accept", "host"),
                    help="with --replicas: how the farm builds and decides its steps (default auto)")
    ap.add_argument("--restart-from", dest="restart_from", default=None, metavar="DIR",
                    help="with --replicas: replica r starts from DIR/replica_NNNN/topology.data (a new run from those "
                         "configurations; -d still supplies the topology)")
    ap.add_argument("--audit", action="store_true",
                    help="with --replicas: after the last block recompute every replica's energy and S(k) from scratch and "
                         "write <out>/audit.dat")
    ap.add_argument("--checkpoint-every", dest="checkpoint_every", type=int, default=0, metavar="N",
                    help="with --replicas: after every N-th block (and the last) write <out>/checkpoint/farm.ckpt, the farm's "
                         "whole state (default 0: none)")
    ap.add_argument("--resume", action="store_true",
                    help="with --replicas: continue the run whose checkpoint lies in <out>, bit for bit (same inputs, replicas, "
                         "seed, mode and nb_step; a larger nb_block extends it)")
    ap.add_argument("--rdf", default=None, metavar="R_MAX,N_BINS[,EVERY]",
                    help="with --replicas: pair distribution functions up to R_MAX (at most half the smallest cell width) in N_BINS "
                         "bins, one sample of every replica after every EVERY-th block (default 1); writes <out>/rdf.dat and "
                         "<out>/rdf_counts.npz")
    ap.add_argument("--rdf-pairs", dest="rdf_pairs", default=None, metavar="A-B,A-B,...",
                    help="with --rdf: the atom-type pairs, ids as in the data file (default: every pair of the active types' atom "
                         "types; at most 8)")
    ap.add_argument("--rdf-intra", dest="rdf_intra", action="store_true",
                    help="with --rdf: count pairs inside one molecule too")
    ap.add_argument("--energy-pairs", dest="energy_pairs", nargs="?", const="1", default=None, metavar="EVERY",
                    help="with --replicas: the energy by residue-type pair (guest-framework, guest-guest, ...; van der Waals, "
                         "Coulomb, reciprocal, self, intra) of every replica after every EVERY-th block (default 1); writes "
                         "<out>/replica_NNNN/energy_pairs.dat and <out>/energy_pairs.dat")
    ap.add_argument("--energy-pairs-select", dest="energy_pairs_select", default=None, metavar="NAME:NAME,...",
                    help="with --energy-pairs: the pairs, by the input's residue names (default: every pair with an active type)")
    ap.add_argument("--density", default=None, metavar="N0,N1,N2[,EVERY]",
                    help="with --replicas: density maps of N0 x N1 x N2 voxels along the cell vectors, one sample of every replica "
                         "after every EVERY-th block (default 1), pooled per fugacity group; writes <out>/density_counts.npz, "
                         "<out>/density_profiles.dat and <out>/density_gGG_typeTT.cube")
    ap.add_argument("--density-types", dest="density_types", default=None, metavar="T,T,...",
                    help="with --density: the atom types, ids as in the data file (default: the active types' atom types; at most 8)")
    ap.add_argument("--density-per-replica", dest="density_per_replica", action="store_true",
                    help="with --density: one map per replica instead of one per fugacity group")
    ap.add_argument("--molecule-energy", dest="molecule_energy", default=None, metavar="EMIN,EMAX,BINS[,EVERY]",
                    help="with --replicas: the distribution of the molecules' removal energies E(X) - E(X without m) in BINS bins "
                         "over [EMIN, EMAX) kcal/mol, one sample of every replica after every EVERY-th block (default 1); writes "
                         "<out>/molecule_energy.dat and <out>/molecule_energy_counts.npz")
    ap.add_argument("--molecule-energy-types", dest="molecule_energy_types", default=None, metavar="NAME,NAME",
                    help="with --molecule-energy: the residue types, by the input's names (default: every active type)")
    argv = list(sys.argv[1:] if argv is None else argv)
    for i in range(len(argv) - 1):
        # EMIN is usually negative: "--molecule-energy -12,2,64" would be read as a switch named -12,2,64
        if argv[i] == "--molecule-energy" and argv[i + 1][:1] == "-" and argv[i + 1][1:2] in tuple("0123456789."):
            argv[i:i + 2] = [argv[i] + "=" + argv[i + 1]]
            break
    a = ap.parse_args(argv)
    try:
        chain_run = parse_chain_run(a.chain_run) if a.chain_run is not None else None
    except ValueError as err:
        ap.error(str(err))
    if a.chain_run_triclinic and chain_run is None:
        ap.error("--chain-run-triclinic needs --chain-run K[,DEPTH]")
    if a.chain_run_gcmc and chain_run is None:
        ap.error("--chain-run-gcmc needs --chain-run K[,DEPTH]")
    if a.chain_run_wide and chain_run is None:
        ap.error("--chain-run-wide needs --chain-run K[,DEPTH]")
    if chain_run is not None and a.replicas is not None:
        ap.error("--chain-run is the single chain's mode: it cannot be combined with --replicas")
    if a.replicas is None:
        if a.fugacities is not None or a.frames != "0" or a.farm_mode != "auto":
            ap.error("--fugacities, --frames and --farm-mode need --replicas")
        if a.restart_from is not None or a.audit:
            ap.error("--restart-from and --audit need --replicas")
        if a.checkpoint_every or a.resume:
            ap.error("--checkpoint-every and --resume need --replicas")
        if a.rdf is not None or a.rdf_pairs is not None or a.rdf_intra:
            ap.error("--rdf, --rdf-pairs and --rdf-intra need --replicas: the single chain writes no distribution functions")
        if a.energy_pairs is not None or a.energy_pairs_select is not None:
            ap.error("--energy-pairs and --energy-pairs-select need --replicas: the single chain writes no energy decomposition")
        if a.density is not None or a.density_types is not None or a.density_per_replica:
            ap.error("--density, --density-types and --density-per-replica need --replicas: the single chain writes no density maps")
        if a.molecule_energy is not None or a.molecule_energy_types is not None:
            ap.error("--molecule-energy and --molecule-energy-types need --replicas: the single chain writes no molecule energies")
    else:
        from . import replicas as farm_run
        if a.as_written:
            ap.error("--as-written cannot be combined with --replicas: the replica farm implements the intended physics only")
        if a.replicas < 1:
            ap.error("--replicas must be at least 1")
        if a.checkpoint_every < 0:
            ap.error("--checkpoint-every must be a positive number of blocks")
        if a.resume and a.restart_from is not None:
            ap.error("--resume cannot be combined with --restart-from: a resumed run continues its own checkpoint")
        try:
            frames = farm_run.parse_frames(a.frames, a.replicas)
            fugacities = farm_run.parse_fugacities(a.fugacities) if a.fugacities is not None else None
        except ValueError as err:
            ap.error(str(err))
        from . import density as density_mod, energy_pairs as epairs_mod, molecule_energy as molen_mod, rdf as rdf_mod
        rdf = rdf_mod.from_args(ap, a)
        energy_pairs = epairs_mod.from_args(ap, a)
        density = density_mod.from_args(ap, a)
        molecule_energy = molen_mod.from_args(ap, a)
    for path, what in ((a.maniac, "Input"), (a.data, "Data"), (a.inc, "Parameter"), (a.reservoir, "Reservoir")):
        if path is not None and not os.path.isfile(path):
            print(f"{what} file not found: {path}", file=sys.stderr)
            return 1
    if a.replicas is not None:
        try:
            res = farm_run.run_replicas(a.maniac, a.data, a.inc, a.out, a.replicas, seed=a.seed, reservoir_path=a.reservoir,
                                        fugacities=fugacities, frames=frames, mode=a.farm_mode, device=a.device,
                                        wide_triclinic=a.wide_triclinic, restart_from=a.restart_from, audit=a.audit,
                                        checkpoint_every=a.checkpoint_every, resume=a.resume, rdf=rdf,
                                        energy_pairs=energy_pairs, density=density, molecule_energy=molecule_energy)
        except ValueError as err:
            print(f"error: {err}", file=sys.stderr)
            return 2
        print(f"{a.replicas} replicas ({res['mode']}): {res['accepted']} accepted moves;  output in "
              f"{os.path.join(a.out, '')}replica_NNNN/ and replicas.dat")
        return 0
    res = run_simulation(a.maniac, a.data, a.inc, a.out, seed=a.seed, reservoir_path=a.reservoir, device=a.device,
                         as_written=a.as_written, speculate=a.speculate, chain_windows=not a.no_chain_windows,
                         wide_chain_windows=a.wide_chain_windows, chain_run=chain_run,
                         chain_run_triclinic=a.chain_run_triclinic, chain_run_gcmc=a.chain_run_gcmc,
                         chain_run_wide=a.chain_run_wide, wide_triclinic=a.wide_triclinic)
    e = res["energy"]
    print(f"final energy (K): total {e['total']:.6f}  non_coulomb {e['non_coulomb']:.6f}  coulomb {e['coulomb']:.6f}  "
          f"recip {e['recip_coulomb']:.6f};  molecules {res['n_mol'].tolist()};  output in {os.path.join(a.out, '')}")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
