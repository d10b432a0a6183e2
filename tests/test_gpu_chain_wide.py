"""Single-chain windows for rigid molecules of 6 to 63 sites (chain_window_kernel<..., WIDE>, DESIGN section 4.3;
mgpu_chain_set_wide): capacity by the rule in include/maniac_gpu.h, then energies, decisions and committed state held bit for
bit to the batched path for these molecules -- mgpu_gcmc_trial_submit / wait, mgpu_commit_submit -- and to the oracle within
tests/util.tol_for; the undecided protocol; the reference's deletion as written; the vector wide form; and the chain driver,
whose files must be the reference's whichever way its windows run.  Reference: src/monte_carlo.f90:40-86,
src/monte_carlo_utils.f90:184-226, :275-395, src/create_molecule.f90:100-112, src/delete_molecule.f90:100-142."""
import json
import os

import numpy as np
import pytest

from maniac_mc_amd import synth
from maniac_mc_amd._lib import MGPU_CREATION, MGPU_DELETION, MGPU_MOVE
from maniac_mc_amd.engine import Engine
from tests.test_gpu_farm_window_wide import _env, _shell, _system, _water
from tests.util import GOLDEN, blank_output_path, tol_for

pytestmark = pytest.mark.gpu

RUNS = os.path.join(GOLDEN, "runs_wide")


def _box(name):
    """(system, active types, molecule slots per type)"""
    if name in ("6", "8", "24"):
        return synth.rigid_adsorbate_box(n_mol=6, n_sites=int(name), L=26.0, seed=17), [0], [8]
    if name == "3+24":       # tests/test_gpu_farm_window_wide.py's mixture: narrow and wide rows in one window
        return _system(np.diag([36.0, 36.0, 36.0]), [(*_water(), 10), (*_shell(24, seed=21), 3)], seed=21), [0, 1], [12, 5]
    raise KeyError(name)


def _twin(s, cap, env=None):
    """The window engine (wide windows on) and the batched engine on the same system."""
    out = []
    with _env(**(env or {})):
        for _ in range(2):
            e = Engine.from_system(s, n_replicas=1, mol_capacity=cap)
            e.init_structure_factor(0, True)
            out.append(e)
    out[0].chain_set_wide(True)
    return out


def _same_state(a, b, n_res):
    for t in range(n_res):
        assert a.num_molecules(0, t) == b.num_molecules(0, t)
        assert np.array_equal(a.get_molecules(0, t), b.get_molecules(0, t))
    assert np.array_equal(a.structure_factor(0), b.structure_factor(0))


def _free_spot(rng, eng, s, clearance=4.5):
    """a point of the cell at least `clearance` from every site"""
    atoms = np.concatenate([eng.get_molecules(0, t)[:eng.num_molecules(0, t)].reshape(-1, 3) for t in range(s.topo.n_res)])
    L = np.diag(s.box_matrix)
    while True:
        p = s.bounds_lo + rng.random(3) * L
        d = atoms - p
        d -= L * np.rint(d / L)
        if np.min(np.linalg.norm(d, axis=1)) > clearance:
            return p


def _window(rng, eng, s, act, kinds, wide_t):
    """rows of one window: kinds[c] of a type drawn from `act` (insertions / deletions: of the wide type)"""
    n = len(kinds)
    stride = max(int(x) for x in s.topo.atoms_in_res)
    t = np.array([wide_t if k != MGPU_MOVE else act[c % len(act)] for c, k in enumerate(kinds)], np.int32)
    m = np.full(n, -1, np.int32)
    sites = np.zeros((n, stride, 3))
    for c in range(n):
        n1 = int(s.topo.atoms_in_res[t[c]])
        nm = eng.num_molecules(0, int(t[c]))
        if kinds[c] != MGPU_CREATION:
            m[c] = (c + 1) % (nm - 1)                          # never the last slot
        if kinds[c] == MGPU_MOVE:
            sites[c, :n1] = eng.get_molecules(0, int(t[c]))[m[c]] + rng.uniform(-0.3, 0.3, 3)[None, :]
        elif kinds[c] == MGPU_CREATION:
            mol = eng.get_molecules(0, int(t[c]))[0]
            sites[c, :n1] = mol - mol.mean(0)[None, :] + _free_spot(rng, eng, s)[None, :]
    return t, m, sites


KINDS6 = np.array([MGPU_MOVE, MGPU_CREATION, MGPU_MOVE, MGPU_DELETION, MGPU_MOVE, MGPU_MOVE], np.int32)


def test_capacity_follows_the_switch_and_the_rule():
    """0 on a default engine (and the row refused), > 0 with wide windows on for 6, 8 and 24 sites and the 3 + 24 mixture;
    still 0 for a 300-site (site-major) type, a tilted box with a 24-site type and the per-k form."""
    for name in ("6", "8", "24", "3+24"):
        s, act, cap = _box(name)
        e = Engine.from_system(s, n_replicas=1, mol_capacity=cap)
        e.init_structure_factor(0, True)
        assert e.chain_window_capacity() == 0, name
        wide_t = act[-1]
        n1 = int(s.topo.atoms_in_res[wide_t])
        row = e.get_molecules(0, wide_t)[:1].copy()
        with pytest.raises(Exception, match="chain_window"):
            e.chain_window(0, [wide_t], [0], [MGPU_MOVE], row, [0.5], [1.0], 300.0, 0.0)
        e.chain_set_wide(True)
        assert e.chain_window_capacity() >= 8, name
        assert e.recip_form(n1)["form"] in ("rows", "wide-vector", "wide-mfma"), name
        e.chain_set_wide(False)
        assert e.chain_window_capacity() == 0, name
        e.close()
    tilted = synth.rigid_adsorbate_box(n_mol=6, n_sites=24, L=26.0, seed=17)
    tilted.box_matrix[1, 0], tilted.box_matrix[2, 0], tilted.box_matrix[2, 1] = 1.5, -0.8, 0.6
    for s in (synth.large_adsorbate_box(), tilted):
        e = Engine.from_system(s, n_replicas=1)
        e.chain_set_wide(True)
        assert e.chain_window_capacity() == 0, s.label
        e.close()
    with _env(MGPU_RECIP_PER_K="1"):
        e = Engine.from_system(_box("24")[0], n_replicas=1)
    e.chain_set_wide(True)
    assert e.recip_form(24)["form"] == "per-k" and e.chain_window_capacity() == 0
    e.close()


def _oracle_rows(P, s, t, m, kinds, sites):
    """old / new components of every row from the oracle, each a trial of the same state"""
    n = len(kinds)
    exp_old, exp_new = np.zeros((n, 5)), np.zeros((n, 5))
    for c in range(n):
        tt, n1 = int(t[c]), int(s.topo.atoms_in_res[t[c]])
        row = sites[c, :n1]
        A0 = P.amplitude()
        if kinds[c] == MGPU_MOVE:
            com, off = P.get_molecule(tt, int(m[c]))
            P.save_fourier(tt, int(m[c]))
            exp_old[c] = P.old_energy(tt, int(m[c]), 0)[:5]
            P.set_molecule(tt, int(m[c]), row[0], row - row[0][None, :])
            exp_new[c] = P.new_energy(tt, int(m[c]), 0)[:5]
            P.set_molecule(tt, int(m[c]), com, off)
            P.restore_fourier(tt, int(m[c]))
        elif kinds[c] == MGPU_CREATION:
            nm = P.num_residues(tt)
            exp_old[c] = P.old_energy(tt, nm, 1)[:5]
            P.set_num_residues(tt, nm + 1)
            P.save_fourier(tt, nm)
            P.set_molecule(tt, nm, row[0], row - row[0][None, :])
            exp_new[c] = P.new_energy(tt, nm, 1)[:5]
            P.set_num_residues(tt, nm)
            P.set_amplitude(A0)
        else:
            P.all_fourier_terms()
            exp_old[c] = P.old_energy(tt, int(m[c]), 2)[:5]
            P.save_fourier(tt, int(m[c]))
            exp_new[c, 2] = P.recip_singlemol(tt, int(m[c]), 2)
            P.set_amplitude(A0)
    return exp_old, exp_new


@pytest.mark.parametrize("name,form", [("6", "mfma"), ("8", "mfma"), ("24", "mfma"), ("3+24", "mfma"), ("24", "vector"), ("3+24", "vector")])
def test_window_energies_are_the_batched_trials_and_the_oracles(name, form, refcpu_mod):
    """K = 6: moves, an insertion and a deletion of the same state.  Energies array_equal to the batched trial of the same
    explicit sites on a twin engine, and equal to the oracle within tol_for.  MGPU_RECIP_NO_MFMA=1 (read at engine creation)
    gives the vector wide form, without it a 24-site type takes the matrix-unit form."""
    s, act, cap = _box(name)
    A, B = _twin(s, cap, env={"MGPU_RECIP_NO_MFMA": "1" if form == "vector" else None})
    wide_t = act[-1]
    f = A.recip_form(int(s.topo.atoms_in_res[wide_t]))["form"]
    if name in ("24", "3+24"):
        assert f == ("wide-vector" if form == "vector" else "wide-mfma"), f
    rng = np.random.default_rng(11)
    t, m, sites = _window(rng, B, s, act, KINDS6, wide_t)
    u, pref = np.full(6, 0.999999), np.full(6, 1e-200)               # every step rejected: the state stays
    e_recip = B.system_energy(0)["recip_coulomb"]
    T = float(s.temperature)
    old_b, new_b = B.gcmc_trial(np.zeros(6, np.int32), t, m, KINDS6, sites)
    old_a, new_a, first, und = A.chain_window(0, t, m, KINDS6, sites, u, pref, T, e_recip)
    assert (first, und) == (-1, -1)
    assert np.array_equal(old_a, old_b) and np.array_equal(new_a, new_b), (np.abs(old_a - old_b).max(), np.abs(new_a - new_b).max())
    P = refcpu_mod.RefCPU(s, mol_capacity=max(cap))
    e_sys = P.system_energy()
    P.init_amplitude(True)
    P.set_energy_recip(e_sys["recip_coulomb"])
    exp_old, exp_new = _oracle_rows(P, s, t, m, KINDS6, sites)
    for c in range(6):
        for got, ref, what in ((old_a[c], exp_old[c], "old"), (new_a[c], exp_new[c], "new")):
            err = np.max(np.abs(got - ref))
            print(name, form, c, what, err, tol_for(*ref, *got))
            assert err <= tol_for(*ref, *got), (c, what, err)
    _same_state(A, B, s.topo.n_res)
    assert A.chain_stats() == (1, 0)
    A.close(); B.close()


@pytest.mark.parametrize("name,form", [("6", "mfma"), ("24", "mfma"), ("3+24", "mfma"), ("24", "vector")])
def test_first_accepted_step_is_committed_as_the_batched_commit(name, form):
    """Draws that make step i the first accepted one -- a translation, an insertion, a deletion that is not the last slot,
    one window each: positions, counts and A(k) array_equal to a twin engine that committed the same step through
    mgpu_commit_submit.  Steps behind the accepted one are not applied."""
    s, act, cap = _box(name)
    A, B = _twin(s, cap, env={"MGPU_RECIP_NO_MFMA": "1" if form == "vector" else None})
    wide_t = act[-1]
    rng = np.random.default_rng(4)
    T = float(s.temperature)
    e_recip = B.system_energy(0)["recip_coulomb"]
    for i, kind in ((2, MGPU_MOVE), (1, MGPU_CREATION), (3, MGPU_DELETION)):
        assert KINDS6[i] == kind
        t, m, sites = _window(rng, B, s, act, KINDS6, wide_t)
        if kind == MGPU_MOVE and len(act) > 1:
            assert t[i] != wide_t or t[0] != wide_t                 # narrow and wide rows in the window
        u, pref = np.full(6, 0.999999), np.full(6, 1e-200)
        u[i:], pref[i:] = 0.0, 1.0                                   # step i and every step behind it would be accepted
        old_b, new_b = B.gcmc_trial(np.zeros(6, np.int32), t, m, KINDS6, sites)
        old_a, new_a, first, und = A.chain_window(0, t, m, KINDS6, sites, u, pref, T, e_recip)
        assert (first, und) == (i, -1)
        assert np.array_equal(old_a, old_b) and np.array_equal(new_a, new_b)
        acc = np.zeros(6, np.int32)
        acc[i] = 1
        B.commit_lane(0, np.zeros(6, np.int32), t, m, KINDS6, acc)
        _same_state(A, B, s.topo.n_res)
        e_recip = e_recip + (new_a[i][2] - old_a[i][2]) if kind == MGPU_MOVE else new_a[i][2]
    assert A.num_molecules(0, wide_t) == B.num_molecules(0, wide_t) == int(s.n_mol[wide_t])
    A.close(); B.close()


def test_wide_steps_too_close_to_call_are_left_to_the_host():
    """tests/test_gpu_chain.py's protocol on the 24-site box with the margin widened: the window stops at the undecided step
    and commits nothing at or behind it; a step accepted before it is committed as usual."""
    s, act, cap = _box("24")
    A, B = _twin(s, cap)
    rng = np.random.default_rng(3)
    kinds = np.full(6, MGPU_MOVE, np.int32)
    t, m, sites = _window(rng, B, s, act, kinds, 0)
    T = float(s.temperature)
    old, new = B.gcmc_trial(np.zeros(6, np.int32), t, m, kinds, sites)
    pref = np.full(6, 0.3)
    x = pref * np.exp(-(((new[:, 0] + new[:, 1]) + new[:, 2]) - ((old[:, 0] + old[:, 1]) + old[:, 2])) / T)
    assert np.all(x < 0.6)
    u = x * 1.5                                 # everything rejected ...
    u[3] = x[3] * (1.0 + 1e-7)                  # ... step 3 too, but from inside a margin of 1e-6
    before = (A.get_molecules(0, 0).copy(), A.structure_factor(0).copy())
    A.chain_set_margin(1e-6)
    u2 = u.copy()
    u2[4] = 0.0                                 # behind the undecided step nothing is decided
    for uu in (u, u2):
        _, _, first, und = A.chain_window(0, t, m, kinds, sites, uu, pref, T, 0.0)
        assert (first, und) == (-1, 3)
        assert np.array_equal(A.get_molecules(0, 0), before[0]) and np.array_equal(A.structure_factor(0), before[1])
    u3 = u.copy()
    u3[1] = 0.0
    _, _, first, und = A.chain_window(0, t, m, kinds, sites, u3, pref, T, 0.0)
    assert (first, und) == (1, -1)
    assert np.array_equal(A.get_molecules(0, 0)[m[1]], sites[1])
    assert A.chain_stats() == (3, 2)
    A.close(); B.close()
    # the default margin (16 ulp) decides the same window: step 3's draw lies 1e-7 above its probability
    A, B = _twin(s, cap)
    _, _, first, und = A.chain_window(0, t, m, kinds, sites, u, pref, T, 0.0)
    assert (first, und) == (-1, -1)
    A.close(); B.close()


def test_wide_deletion_as_written_window():
    """link >= 0 on the charged 24-site molecule: the new reciprocal energy is the creation-kind energy of the companion row
    (the molecule RemoveMolecule moves into the slot), and the commit adds THAT molecule's terms to A(k) while the
    coordinates lose slot m (monte_carlo_utils.f90:301-309) -- against the batched trial and the neutral primitives
    mc_chain.f90 composes the same update from."""
    s, act, cap = _box("24")
    A, B = _twin(s, cap)
    e_recip = B.system_energy(0)["recip_coulomb"]
    T = float(s.temperature)
    nm = 6
    last = B.get_molecules(0, 0)[nm - 1]
    kinds = np.array([MGPU_DELETION, MGPU_CREATION], dtype=np.int32)
    sites = np.stack([np.zeros((24, 3)), last])
    m = np.array([2, -1], dtype=np.int32)
    old_b, new_b = B.gcmc_trial(np.zeros(2, np.int32), [0, 0], m, kinds, sites)
    old_a, new_a, first, und = A.chain_window(0, [0, 0], m, kinds, sites, [1e-300, 0.0], [1.0, 0.0], T, e_recip, link=[1, -2])
    assert np.array_equal(old_a[0], old_b[0]) and new_a[1][2] == new_b[1][2]
    assert (first, und) == (0, -1)            # u = 1e-300: accepted whatever the energies
    B.replace_molecule(0, 0, 2, nm - 1)
    B.set_num_molecules(0, 0, nm - 1)
    B.structure_factor_add(0, 0, last)
    _same_state(A, B, 1)
    # ... and a rejected one (u = 1) changes nothing
    state = (A.get_molecules(0, 0).copy(), A.structure_factor(0).copy())
    last = A.get_molecules(0, 0)[nm - 2]
    sites = np.stack([np.zeros((24, 3)), last])
    _, _, first, und = A.chain_window(0, [0, 0], [1, -1], kinds, sites, [1.0, 0.0], [1e-6, 0.0], T, e_recip, link=[1, -2])
    assert (first, und) == (-1, -1)
    assert np.array_equal(A.get_molecules(0, 0), state[0]) and np.array_equal(A.structure_factor(0), state[1])
    A.close(); B.close()


@pytest.mark.parametrize("case", ["cage24_gcmc", "cage6_nvt"])
def test_chain_driver_writes_the_reference_files_either_way(case, tmp_path):
    """run_simulation on the whole-run fixtures of these molecules: one launch per window (K = 4), windows through the batched
    calls (K = 4) and one step per call (K = 1) write the reference's files, character for character (log.maniac with the
    output path blanked); only the first reports one-launch windows, and at the default margin none of its steps is left
    to the host."""
    from maniac_mc_amd import run
    summary = json.load(open(os.path.join(RUNS, "summary.json")))[case]
    inputs = os.path.join(RUNS, case, "inputs")
    expected = os.path.join(RUNS, case, "expected")
    cwd = os.getcwd()
    for k, cw, wide in ((4, True, True), (4, True, False), (1, False, False)):
        out = str(tmp_path / f"out_{k}_{int(cw)}_{int(wide)}") + "/"
        os.chdir(inputs)
        try:
            res = run.run_simulation("system.maniac", "system.data", "system.inc", out, seed=summary["seed"],
                                     as_written=bool(summary["as_written"]), speculate=k, chain_windows=cw, wide_chain_windows=wide)
        finally:
            os.chdir(cwd)
        windows, undecided = res["chain_windows"]
        print(case, k, cw, wide, windows, undecided, res["mc_seconds"])
        assert (windows > 0) == wide and undecided == 0
        for f in summary["files"]:
            want = open(os.path.join(expected, f)).read().split("\n")
            got = open(os.path.join(out, f)).read().split("\n")
            if f == "log.maniac":
                got = blank_output_path(got, out)
            assert got == want, (k, cw, wide, f)
