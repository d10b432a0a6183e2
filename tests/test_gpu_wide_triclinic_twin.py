"""The batched device-built path (mgpu_move_trial_submit under mgpu_set_triclinic_moves, the twin the chain runs of such boxes are
held to) on a 24-site type in a TRICLINIC cell, which nothing had run before: the trial geometry bit for bit against the oracle's
ApplyPBC, as tests/test_gpu_triclinic_moves.py holds it for molecules of up to five sites, and the energies of the candidates it
builds against the host-row path bit for bit and against the oracle's ComputeOldEnergy / ComputeNewEnergy within
tests/util.tol_for.  The two cells of tests/test_gpu_chain_wide_triclinic.py (the mild tilt; the sheared cell, where the full
27-image search runs).  Reference: src/geometry_utils.f90:167-220 (ApplyPBC), :397-411 (ComputeDistance),
src/create_molecule.f90:180-184."""
import numpy as np
import pytest

from maniac_mc_amd.engine import Engine
from tests import triclinic_cases as tc
from tests.test_gpu_chain_wide_triclinic import _images, print_redraws, tri_box  # noqa: F401  (print_redraws: autouse fixture)
from tests.test_gpu_triclinic_moves import _kinds
from tests.util import tol_for

pytestmark = pytest.mark.gpu

CELLS = ("mild", "sheared")


def _records(s, rng):
    """(m, move, u[5], com0): centres on the wrap's edges and far outside the cell, translations by nothing and by a draw,
    rotations about every axis, insertions at fractions on and next to the faces (tests/test_gpu_triclinic_moves.py's case)"""
    n = int(s.n_mol[0])
    edge = np.vstack([tc.edge_points(s, 8, 41, True), tc.edge_points(s, 4, 42)])
    far = rng.uniform(-200.0, 200.0, (4, 3))
    ins = np.array([0.0, 1e-17, 1e-16, 0.5, 1.0 - 1e-16, 0.25])
    recs, k = [], 0
    for p in edge:
        u = rng.random(5); u[:3] = 0.5
        recs.append((k % n, 1, u, p)); k += 1
    for p in np.vstack([edge[:4], far]):
        recs.append((k % n, 1, rng.random(5), p)); k += 1
    for i in range(4):
        recs.append((k % n, 1, rng.random(5), None)); k += 1
    for i in range(6):
        u = rng.random(5); u[4] = (0.05, 0.4, 0.7, 0.99, 0.5, 0.2)[i]
        recs.append((k % n, 2, u, far[i % 4] if i % 2 else None)); k += 1
    for i in range(8):
        u = rng.random(5); u[:3] = ins[rng.integers(0, len(ins), 3)] if i < 6 else rng.random(3)
        recs.append((0, 3, u, None)); k += 1
    return recs


@pytest.mark.parametrize("cell", CELLS)
def test_device_built_geometry_of_24_sites_is_the_oracles_bit_for_bit(cell, refcpu_mod):
    s, _, _ = tri_box("24", cell)
    cap = [int(s.n_mol[0]) + 2]
    P = refcpu_mod.RefCPU(s, mol_capacity=cap[0])
    rng = np.random.default_rng(17)
    recs = _records(s, rng)
    n = len(recs)
    eng = Engine.from_system(s, n_replicas=n, mol_capacity=cap, triclinic_moves=True)
    com0 = []
    for r, (m, mv, u, p) in enumerate(recs):
        if r:
            eng.replica_copy(r, 0)
        com = s.com[0].copy()
        if p is not None:
            com[m] = p
        eng.set_frames(r, 0, com, s.offsets[0])
        com0.append(com[m].copy())
        eng.init_structure_factor(r, True)
    t = np.zeros(n, np.int32)
    m = np.array([rc[0] for rc in recs], np.int32)
    move = np.array([rc[1] for rc in recs], np.int32)
    u = np.array([rc[2] for rc in recs])
    rep = np.arange(n, dtype=np.int32)
    t_step, r_step = 6.0, 0.6
    eng.move_trial(rep, t, m, move, u, t_step, r_step)
    eng.commit_lane(0, rep, t, m, _kinds(move), np.ones(n, np.int32))
    outside = 0
    for c in range(n):
        mm = int(m[c])
        off0 = s.offsets[0][mm]
        slot = mm
        if move[c] == 1:
            target = com0[c] + (u[c, :3] - 0.5) * t_step
            com_e, off_e = P.apply_pbc(target), off0
            outside += int(np.max(np.abs(target)) > 60.0)
        elif move[c] == 2:
            com_e, off_e = com0[c], off0 @ P.rotation_matrix(int(u[c, 4] * 3.0) + 1, (u[c, 3] - 0.5) * r_step).T
        else:
            slot = int(s.n_mol[0])
            com_e = tc.cart(s, u[c, :3])
            off_e = s.offsets[0][0] @ P.rotation_matrix(int(u[c, 4] * 3.0) + 1, u[c, 3] * 2 * np.pi).T
        com_d, off_d = eng.get_frames(c, 0)
        assert np.array_equal(com_d[slot], com_e), (cell, c, int(move[c]), com_d[slot] - com_e)
        if move[c] == 1:
            assert np.array_equal(off_d[slot], off_e), (c, move[c])
        else:
            assert np.max(np.abs(off_d[slot] - off_e)) <= 1e-12, (c, move[c])
        assert np.array_equal(eng.get_molecules(c, 0)[slot], com_d[slot][None, :] + off_d[slot])
        assert eng.num_molecules(c, 0) == s.n_mol[0] + (move[c] == 3)
    assert outside >= 4
    eng.close()


# Insertions that overlap a neighbour THROUGH A FAR IMAGE, chosen, not drawn: the centre lies this far (A) from the image of a
# molecule's centre under a lattice vector of the search (a sum of columns of the matrix, not zero), and more than 12 A from the
# centre as it is stored, so the overlap exists only for a search that tries that image.  Bounding spheres of 2.6 A: at 5.0 A the
# rings interleave, at 4.4 A sites come within an Angstrom or two of one another.
FAR_IMAGE_DIST = (5.0, 4.4)


def _far_image_insertions(s, dists):
    """fractions f (centre lo + M f, inside the cell) of one insertion per distance: the first molecule, lattice vector and axis,
    in order, that put the centre inside the cell and leave every OTHER molecule's images at least 7.5 A away"""
    M = np.asarray(s.box_matrix, dtype=np.float64)
    inv = np.linalg.inv(M)
    shifts = _images(M)
    out = []
    for dist in dists:
        found = None
        for k in range(int(s.n_mol[0])):
            others = np.delete(s.com[0], k, axis=0)
            for sh in shifts:
                if not np.any(sh):
                    continue
                for axis in np.vstack([np.eye(3), -np.eye(3)]):
                    p = s.com[0][k] + sh + dist * axis
                    f = inv @ (p - s.bounds_lo)
                    clear = np.min(np.linalg.norm((others - p)[:, None, :] + shifts[None, :, :], axis=2)) >= 7.5
                    if found is None and np.all(f > 0.02) and np.all(f < 0.98) and clear and np.linalg.norm(s.com[0][k] - p) > 12.0:
                        found = f
        assert found is not None, "no far image of a molecule lies inside the cell"
        # (the search sees it: the minimum over the 27 images of the stored difference is the chosen distance)
        seen = np.min(np.linalg.norm((s.com[0] - tc.cart(s, found))[:, None, :] + shifts[None, :, :], axis=2))
        assert abs(seen - dist) < 1e-9, (seen, dist)
        out.append(found)
    return np.array(out)


@pytest.mark.parametrize("cell", CELLS)
def test_device_built_energies_of_24_sites_are_the_host_row_paths_and_the_oracles(cell, refcpu_mod):
    """The candidates the device builds, read back after a forced commit on one engine, go to gcmc_trial as host rows on an
    untouched twin: five components of both states BIT FOR BIT; every move, insertion and deletion against the oracle within
    tol_for -- the records drawn once, whatever they land on, and two insertions placed on a neighbour's far image."""
    s, _, _ = tri_box("24", cell)
    N = int(s.n_mol[0])
    cap = [N + 2]
    rng = np.random.default_rng(23)
    move = np.array([1, 2, 3, 4] * 3 + [3] * len(FAR_IMAGE_DIST), np.int32)
    n = len(move)
    t = np.zeros(n, np.int32)
    eng = []
    for _ in range(2):
        e = Engine.from_system(s, n_replicas=n, mol_capacity=cap, triclinic_moves=True)
        e.set_frames(0, 0, s.com[0], s.offsets[0])
        e.init_structure_factor(0, True)
        for r in range(1, n):
            e.replica_copy(r, 0)
        eng.append(e)
    a, b = eng
    m = np.array([0 if mv == 3 else int(rng.integers(0, N)) for mv in move], np.int32)
    u = rng.random((n, 5))                     # drawn once: whatever an insertion lands on goes to the oracle
    far = _far_image_insertions(s, FAR_IMAGE_DIST)
    assert np.all(move[-len(far):] == 3)
    u[-len(far):, :3] = far
    rep = np.arange(n, dtype=np.int32)
    kinds = _kinds(move)
    old, new = a.move_trial(rep, t, m, move, u, 0.8, 0.6)
    a.commit_lane(0, rep, t, m, kinds, (move != 4).astype(np.int32))
    rows = np.zeros((n, 24, 3))
    for c in range(n):
        rows[c] = a.get_molecules(c, 0)[N if move[c] == 3 else int(m[c])]
    mh = np.where(move == 3, -1, m).astype(np.int32)
    oh, nh = b.gcmc_trial(rep, t, mh, kinds, rows)
    assert np.array_equal(old, oh), np.max(np.abs(old - oh))
    assert np.array_equal(new, nh), np.max(np.abs(new - nh))
    P = refcpu_mod.RefCPU(s, mol_capacity=cap[0])
    e_sys = P.system_energy()
    P.init_amplitude(True)
    P.set_energy_recip(e_sys["recip_coulomb"])
    worst = 0.0
    for c in range(n):
        mm = int(m[c])
        A0 = P.amplitude()
        eo, en = np.zeros(5), np.zeros(5)
        if move[c] <= 2:
            com0, off0 = P.get_molecule(0, mm)
            com_d, off_d = a.get_frames(c, 0)
            P.save_fourier(0, mm)
            eo = P.old_energy(0, mm, 0)[:5]
            P.set_molecule(0, mm, com_d[mm], off_d[mm])
            en = P.new_energy(0, mm, 0)[:5]
            P.set_molecule(0, mm, com0, off0)
            P.restore_fourier(0, mm)
        elif move[c] == 3:
            com_d, off_d = a.get_frames(c, 0)
            eo = P.old_energy(0, N, 1)[:5]
            P.set_num_residues(0, N + 1)
            P.save_fourier(0, N)
            P.set_molecule(0, N, com_d[N], off_d[N])
            en = P.new_energy(0, N, 1)[:5]
            P.set_num_residues(0, N)
            P.set_amplitude(A0)
        else:
            P.all_fourier_terms()
            eo = P.old_energy(0, mm, 2)[:5]
            P.save_fourier(0, mm)
            en[2] = P.recip_singlemol(0, mm, 2)
            P.set_amplitude(A0)
        for got, ref, what in ((old[c], eo, "old"), (new[c], en, "new")):
            err = float(np.max(np.abs(got - ref)))
            worst = max(worst, err)
            print(cell, c, int(move[c]), what, err, tol_for(*ref, *got))
            assert err <= tol_for(*ref, *got), (cell, c, int(move[c]), what, got, ref)
    print(f"{cell}: worst |batched - oracle| = {worst:.3e} K")
    a.close(); b.close()
