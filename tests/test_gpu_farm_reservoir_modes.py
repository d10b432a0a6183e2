"""Reservoirs in the Fortran farm (mc_farm.f90 mfarm_set_reservoir, FortranFarm(reservoir=...)) in every mode: host-built
(the driver's mirror), device-built, device-decided and windows (the engine's), and host-built in a triclinic cell.  After a
run: running energies = a from-scratch evaluation, A(k) = a fresh S(k), box count + reservoir count conserved, every molecule
one of the conformers it could have come from, host mirrors = the device; the device-decided farm is the host-decided farm bit
for bit; an empty reservoir inserts nothing.  Reference: src/create_molecule.f90:117-128, :185-193; delete_molecule.f90:146-166."""
import numpy as np
import pytest

from maniac_mc_amd import synth
from tests.test_gpu_farm_reservoir import _bent, _dists, _reservoir
from tests.util import farm_tol

pytestmark = pytest.mark.gpu

MODES = {"host_built": dict(), "device_built": dict(device_build=True), "device_decided": dict(device_build=True, device_accept=True),
         "window": dict(device_build=True, window=True)}
KEYS = ("non_coulomb", "coulomb", "recip_coulomb", "ewald_self", "intra_coulomb")


def _co2_farm(mode, n_rsv, phi_v=20.0, R=8, seed=17):
    from maniac_mc_amd.fortran_host import FortranFarm
    s = synth.co2_box(20, seed=13)
    rng = np.random.default_rng(4)
    res = _reservoir(rng, [s.offsets[0][0], _bent(s.offsets[0][0])], n_rsv)
    farm = FortranFarm(s, R, seed=seed, translation_step=1.0, rotation_step=0.6, n_threads=2, mol_capacity=[90],
                       gcmc=dict(p_translation=0.2, p_rotation=0.2, fugacity=phi_v / 50.0 ** 3), reservoir={0: res}, **MODES[mode])
    return s, res, farm


def _check_invariants(s, farm, res, steps, types=(0,)):
    eng = farm.eng
    counts = farm.counts()
    for r in range(farm.R):
        e = eng.system_energy(r)
        ref = np.array([e[k] for k in KEYS])
        assert np.max(np.abs(farm.energy(r) - ref)) < farm_tol(ref, steps), (r, farm.energy(r) - ref)
        A = eng.structure_factor(r)
        eng.init_structure_factor(r, True)
        assert np.max(np.abs(A - eng.structure_factor(r))) < 1e-9
        for ia in types:
            t = int(farm.active[ia])
            rsv = farm.reservoir(r, ia)
            assert counts[r, ia] + rsv.shape[0] == int(s.n_mol[t]) + res.shape[0], (r, ia)
            known = [_dists(o) for o in np.concatenate([s.offsets[t], res])]
            dev = eng.get_molecules(r, t)
            assert dev.shape[0] == counts[r, ia]
            for mol in list(dev) + list(rsv):
                assert min(np.max(np.abs(_dists(mol) - k)) for k in known) <= 1e-10
            for slot in range(counts[r, ia]):
                com, off = farm.molecule(r, ia, slot)
                assert np.array_equal(dev[slot], com[None, :] + off[: dev.shape[1]])


@pytest.mark.parametrize("mode", list(MODES))
def test_farm_with_a_reservoir_keeps_its_invariants(mode):
    s, res, farm = _co2_farm(mode, 30)
    assert farm.window == (mode == "window")
    farm.run(300)
    c = farm.counters()
    assert c["creations"] > 0 and c["deletions"] > 0, c
    _check_invariants(s, farm, res, 300)
    farm.close()


def test_device_decided_farm_is_the_host_decided_farm_with_a_reservoir():
    a = _co2_farm("device_built", 30)[2]
    b = _co2_farm("device_decided", 30)[2]
    for f in (a, b):
        f.run(150)
    assert a.trials == b.trials and a.accepted == b.accepted and a.skipped == b.skipped and a.accepted > 0
    assert a.counters() == b.counters()
    assert np.array_equal(a.counts(), b.counts())
    for r in range(a.R):
        assert np.array_equal(a.energy(r), b.energy(r)), r
        assert np.array_equal(a.eng.structure_factor(r), b.eng.structure_factor(r)), r
        assert np.array_equal(a.eng.get_molecules(r, 0), b.eng.get_molecules(r, 0)), r
        assert np.array_equal(a.reservoir(r, 0), b.reservoir(r, 0)), r
    a.close(); b.close()


@pytest.mark.parametrize("mode", list(MODES))
def test_an_empty_reservoir_inserts_nothing(mode):
    """two reservoir molecules and a fugacity that wants 200: the count never exceeds the conserved total, and the
    insertions that found the reservoir empty were skipped"""
    s, res, farm = _co2_farm(mode, 2, phi_v=200.0, R=4)
    for _ in range(6):
        farm.run(25)
        assert np.all(farm.counts()[:, 0] <= 20 + 2)
    assert farm.skipped > 0
    _check_invariants(s, farm, res, 150)
    farm.close()


def test_host_built_triclinic_farm_with_a_reservoir():
    from maniac_mc_amd.engine import box_prepare
    from maniac_mc_amd.fortran_host import FortranFarm
    s = synth.mixture_box(seed=8, tilt=(1.5, -0.8, 0.6))
    _, volume, _, _ = box_prepare(s.box_matrix)
    rng = np.random.default_rng(6)
    res = _reservoir(rng, [s.offsets[0][0], _bent(s.offsets[0][0])], 20)
    farm = FortranFarm(s, 6, seed=5, translation_step=0.8, rotation_step=0.5, n_threads=2, mol_capacity=[40, 40],
                       gcmc=dict(p_translation=0.3, p_rotation=0.3, fugacity=12.0 / volume), reservoir={0: res})
    assert not farm.device_build
    farm.run(300)
    c = farm.counters()
    assert c["creations"] > 0 and c["deletions"] > 0
    _check_invariants(s, farm, res, 300)
    farm.close()
