"""The molecule-energy histograms on the device (mgpu_molecule_energy_*, Engine.molecule_energy_*): after two samples of every
replica the histogram equals, EXACTLY, twice the numpy bin rule (maniac_mc_amd.molecule_energy.slot_index) applied to the
stateless call's totals -- the accumulate path runs the same kernels in the same order, so its totals are those bit for bit.

The limits are taken from the device's own totals so that every kind of slot is hit: e_min IS one molecule's total (slot 1), e_max
IS another's (the top slot), and molecules lie below and above the range; with 1, 16 and 4096 bins.  On the three-type box (all
three types selected; one uncharged) and co2_20 with capacity + 3, the variants and the never loaded replica of
tests/test_gpu_energy_pairs.py."""
import numpy as np
import pytest

from maniac_mc_amd import molecule_energy as me
from maniac_mc_amd._lib import MgpuError
from maniac_mc_amd.engine import Engine
from tests.test_gpu_energy_pairs import SYSTEMS
from tests.test_gpu_rdf import _capacity, _first_active, _load, _variants

pytestmark = pytest.mark.gpu

MGPU_ERR_INVALID_ARG, MGPU_ERR_STATE = 1, 5
R = 5
NAMES = ["three_types", "co2_20"]

_cases = {}


def _case(name):
    """(system, capacities, engine of R + 1 replicas, selected types, per (replica, selected type) the live totals)"""
    if name not in _cases:
        s = SYSTEMS[name]()
        cap = _capacity(name, s)
        eng = Engine(s.topo, s.box_matrix, s.bounds_lo, s.real_space_cutoff, s.ewald_tolerance, R + 1, 0, cap)
        _load(eng, _variants(name, s, cap), _first_active(s))
        types = [t for t in range(s.topo.n_res) if s.topo.is_active[t] == 1]
        full, counts = eng.molecule_energies_replicas(types)
        total = me.total_energy(full)
        row0 = np.concatenate([[0], np.cumsum([cap[t] for t in types])[:-1]]).astype(int)
        live = [[total[r, row0[k]:row0[k] + counts[r, k]] for k in range(len(types))] for r in range(R + 1)]
        _cases[name] = (s, cap, eng, types, live, counts)
    return _cases[name]


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    for c in _cases.values():
        c[2].close()
    _cases.clear()


def _expected(live, e_min, e_max, n_bins):
    return np.array([[me.histogram(u, e_min, e_max, n_bins) for u in per_type] for per_type in live], dtype=np.uint64)


def _limits(live):
    """two of replica 0's own totals with molecules below the lower and above the upper one"""
    u = np.unique(np.concatenate(live[0]))
    assert u.size >= 8
    return float(u[u.size // 4]), float(u[(3 * u.size) // 4])


@pytest.mark.parametrize("n_bins", [1, 16, 4096])
@pytest.mark.parametrize("name", NAMES)
def test_two_samples_are_twice_the_numpy_rule(name, n_bins):
    s, cap, eng, types, live, counts = _case(name)
    e_min, e_max = _limits(live)
    eng.molecule_energy_configure(n_bins, e_min, e_max, types)
    hist, samples = eng.molecule_energy_read()
    assert hist.shape == (R + 1, len(types), n_bins + 2) and hist.dtype == np.uint64 and not hist.any() and not samples.any()
    eng.molecule_energy_accumulate()
    eng.molecule_energy_accumulate(chunk=2)
    hist, samples = eng.molecule_energy_read()
    want = _expected(live, e_min, e_max, n_bins)
    assert np.array_equal(hist, 2 * want)
    assert np.array_equal(samples, np.full(R + 1, 2, dtype=np.uint64)), "a replica without molecules is a sample too"
    # every kind of slot is hit, the two limits where the rule says
    assert me.slot_index(e_min, e_min, e_max, n_bins) == 1 and me.slot_index(e_max, e_min, e_max, n_bins) == n_bins + 1
    assert want[0, :, 0].sum() > 0 and want[0, :, 1].sum() > 0 and want[0, :, n_bins + 1].sum() > 1 and want[0, :, 1:-1].sum() > 1
    # nothing is dropped: the slots of a replica add up to samples x its molecules
    assert np.array_equal(hist.sum(axis=2), 2 * counts.astype(np.uint64))
    assert not hist[R].any()


@pytest.mark.parametrize("name", NAMES)
def test_subsets_round_trip_and_reset(name):
    s, cap, eng, types, live, counts = _case(name)
    e_min, e_max = _limits(live)
    n_bins = 16
    want = _expected(live, e_min, e_max, n_bins)
    eng.molecule_energy_configure(n_bins, e_min, e_max, types)
    eng.molecule_energy_accumulate([4, 1])
    hist, samples = eng.molecule_energy_read()
    for r in range(R + 1):
        assert np.array_equal(hist[r], want[r] if r in (1, 4) else 0 * want[r]), "the others' words are untouched"
    assert samples.tolist() == [0, 1, 0, 0, 1, 0]
    h41, s41 = eng.molecule_energy_read([4, 1])
    assert np.array_equal(h41, want[[4, 1]]) and s41.tolist() == [1, 1]
    # read -> reset -> load -> read
    eng.molecule_energy_accumulate()
    hist, samples = eng.molecule_energy_read()
    eng.molecule_energy_reset()
    zh, zs = eng.molecule_energy_read()
    assert not zh.any() and not zs.any()
    eng.molecule_energy_load(hist, samples)
    bh, bs = eng.molecule_energy_read()
    assert np.array_equal(bh, hist) and np.array_equal(bs, samples)
    eng.molecule_energy_reset([1])
    eng.molecule_energy_load(hist[[3]] + np.uint64(5), samples[[3]], [0])
    bh, bs = eng.molecule_energy_read()
    assert not bh[1].any() and bs[1] == 0 and np.array_equal(bh[0], hist[3] + np.uint64(5)) and np.array_equal(bh[2:], hist[2:])
    # a configure with other bins starts from zero
    eng.molecule_energy_configure(4, e_min, e_max, types[:1])
    zh, zs = eng.molecule_energy_read()
    assert zh.shape == (R + 1, 1, 6) and not zh.any() and not zs.any()


def test_refusals_with_their_codes():
    s, cap, eng, types, live, counts = _case("co2_20")
    eng.molecule_energy_configure(0, 0.0, 0.0, [])                      # frees the accumulators
    for call in (eng.molecule_energy_accumulate, eng.molecule_energy_read, eng.molecule_energy_reset):
        with pytest.raises(MgpuError) as err:
            call()
        assert err.value.code == MGPU_ERR_STATE and "configure" in str(err.value), "before configure"
    for n_bins, lo, hi, ty, text in ((0, -1.0, 1.0, types, "n_bins 0 is outside [1, 4096]"),
                                     (4097, -1.0, 1.0, types, "n_bins 4097 is outside [1, 4096]"),
                                     (8, 1.0, 1.0, types, "e_min below e_max"),
                                     (8, 2.0, 1.0, types, "e_min below e_max"),
                                     (8, -np.inf, 1.0, types, "finite"),
                                     (8, 0.0, np.nan, types, "finite"),
                                     (8, -1.0, 1.0, [types[0], types[0]], "is a duplicate"),
                                     (8, -1.0, 1.0, [s.topo.n_res], "is out of range")):
        with pytest.raises(MgpuError) as err:
            eng.molecule_energy_configure(n_bins, lo, hi, ty)
        assert err.value.code == MGPU_ERR_INVALID_ARG and text in str(err.value), (text, str(err.value))
    with pytest.raises(MgpuError) as err:
        eng.molecule_energy_accumulate()
    assert err.value.code == MGPU_ERR_STATE, "a refused configure configures nothing"
    eng.molecule_energy_configure(8, -1.0, 1.0, types)
    hist, samples = eng.molecule_energy_read()
    with pytest.raises(ValueError, match="molecule_energy_load"):
        eng.molecule_energy_load(hist[:, :, :-1], samples)
    with pytest.raises(ValueError, match="molecule_energy_load"):
        eng.molecule_energy_load(hist, samples[:-1])
    with pytest.raises(MgpuError) as err:
        eng.molecule_energy_accumulate([1, 1])
    assert err.value.code == MGPU_ERR_INVALID_ARG and "listed twice" in str(err.value)
    eng.molecule_energy_accumulate([])                                   # nothing listed is nothing to do
    assert not eng.molecule_energy_read()[0].any()
