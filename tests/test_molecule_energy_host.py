"""maniac_mc_amd.molecule_energy without a device: the numpy restatement of the engine's bin rule on hand-made values, the
pooling over a fugacity group and its standard error on synthetic counts, the two files written and read back, every refusal of
check_spec and of the command line with its text, and run_replicas refusing a bad option before a farm exists."""
import math
import os
import types

import numpy as np
import pytest

from maniac_mc_amd import molecule_energy as me
from maniac_mc_amd import replicas, run
from maniac_mc_amd.system import KB_KCALMOL
from tests.util import GOLDEN, golden_system

D = os.path.join(GOLDEN, "runs", "co2_gcmc", "inputs")
INPUTS = (os.path.join(D, "system.maniac"), os.path.join(D, "system.data"), os.path.join(D, "system.inc"))


# ---- the bin rule -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_bins", [1, 7, 4096])
def test_bin_rule_on_hand_made_values(n_bins):
    e_min, e_max = -3.25e3, 1.75e2
    below_max = np.nextafter(e_max, -np.inf)
    u = np.array([e_min, e_max, below_max, np.nan, np.nextafter(e_min, -np.inf), -np.inf, np.inf, 1e300, -1e300])
    want = [1, n_bins + 1, n_bins, n_bins + 1, 0, 0, n_bins + 1, n_bins + 1, 0]
    assert me.slot_index(u, e_min, e_max, n_bins).tolist() == want
    # interior values: the floor of the rounded product of the rounded difference, clamped to the last bin
    rng = np.random.default_rng(n_bins)
    v = rng.uniform(e_min, e_max, 2000)
    inv_w = n_bins / (e_max - e_min)
    by_hand = [1 + min(n_bins - 1, int(math.floor((float(x) - e_min) * inv_w))) for x in v]
    got = me.slot_index(v, e_min, e_max, n_bins)
    assert got.tolist() == by_hand and got.min() >= 1 and got.max() <= n_bins
    h = me.histogram(np.concatenate([u, v]), e_min, e_max, n_bins)
    assert h.dtype == np.uint64 and h.shape == (n_bins + 2,) and int(h.sum()) == u.size + v.size, "nothing is dropped"
    assert int(h[0]) == 3 and int(h[-1]) == 4


def test_bin_edges_fall_into_the_upper_bin():
    # edges that are exact doubles: 4 bins of width 0.5 from -1.  0.5 - 2^-52 is the largest value whose distance from e_min
    # still rounds below 1.5 (the next double below 0.5 is nearer: its difference rounds TO 1.5, and the rule puts it in bin 4)
    assert me.slot_index([-1.0, -0.5, 0.0, 0.5, 0.5 - 2.0 ** -52, np.nextafter(0.5, 0.0), np.nextafter(1.0, 0.0), 1.0],
                         -1.0, 1.0, 4).tolist() == [1, 2, 3, 4, 3, 4, 4, 5]
    assert np.array_equal(me.bin_centres(-1.0, 1.0, 4), [-0.75, -0.25, 0.25, 0.75])


def test_total_is_the_serial_chain():
    c = np.array([[1e16, 1.0, -1e16, 1.0, 1.0], [0.1, 0.2, 0.3, 0.4, 0.5]])
    want = [((((r[0] + r[1]) + r[2]) + r[3]) + r[4]) for r in c.tolist()]
    assert me.total_energy(c).tolist() == want and want[0] == 2.0


def test_kelvin_limits_divide_once():
    lo, hi = me.kelvin_limits(dict(e_min=-12.5, e_max=0.75))
    assert lo == -12.5 / KB_KCALMOL and hi == 0.75 / KB_KCALMOL


# ---- pooling --------------------------------------------------------------------------------------------------------------------
def _synthetic(seed=4, Rn=5, n_sel=2, n_bins=6):
    rng = np.random.default_rng(seed)
    hist = rng.integers(0, 500, (Rn, n_sel, n_bins + 2)).astype(np.uint64)
    return hist, np.arange(Rn) % 2


def test_pooling_and_standard_error():
    hist, group = _synthetic()
    e_min, e_max = -8.0, 4.0
    w = (e_max - e_min) / 6
    out = me.pooled(hist, group, e_min, e_max)
    assert [(g, s) for g, s, *_ in out] == [(0, 0), (0, 1), (1, 0), (1, 1)]
    for g, s, p, sem, count in out:
        sel = group == g
        total = hist[sel, s].sum(axis=0)
        assert np.array_equal(count, total) and count.dtype == np.uint64
        inside = total[1:-1].astype(np.float64)
        assert np.allclose(p, inside / (inside.sum() * w), rtol=1e-15, atol=0)
        assert abs(p.sum() * w - 1.0) < 1e-14, "a density over the range"
        each = np.array([h[1:-1] / (h[1:-1].sum() * w) for h in hist[sel, s].astype(np.float64)])
        assert np.allclose(sem, np.std(each, axis=0, ddof=1) / math.sqrt(sel.sum()), rtol=1e-14, atol=0)
    # one replica in a group: no standard error to give; nothing inside the range: zeros, not a division by zero
    one = me.pooled(hist[:1], group[:1], e_min, e_max)
    assert not any(sem.any() for *_, sem, _c in one)
    empty = np.zeros((2, 1, 8), dtype=np.uint64)
    empty[:, 0, 0] = 3
    (g, s, p, sem, count), = me.pooled(empty, [0, 0], e_min, e_max)
    assert not p.any() and not sem.any() and count.tolist() == [6, 0, 0, 0, 0, 0, 0, 0]


# ---- the files ------------------------------------------------------------------------------------------------------------------
def test_dat_round_trip(tmp_path):
    hist, group = _synthetic()
    path = str(tmp_path / "molecule_energy.dat")
    me.write_dat(path, hist, group, [1, 0], ["frame", "co2"], -8.0, 4.0)
    with open(path) as f:
        lines = f.read().splitlines()
    assert lines[0].startswith("#") and sum("below" in ln and "above" in ln for ln in lines) == 4
    assert all(k in lines[2] for k in ("group", "type", "e_mid", "density", "density_sem", "count"))
    assert len({len(ln) for ln in lines if not ln.startswith("#")}) == 1, "fixed-width records"
    back = me.read_dat(path)
    assert sorted(back) == [(0, 0), (0, 1), (1, 0), (1, 1)]
    for g, s, p, sem, count in me.pooled(hist, group, -8.0, 4.0):
        d = back[(g, s)]
        assert d["type"] == [2, 1][s] and d["name"] == ["co2", "frame"][s]
        assert d["below"] == int(count[0]) and d["above"] == int(count[-1]) and np.array_equal(d["count"], count[1:-1])
        assert np.allclose(d["e_mid"], me.bin_centres(-8.0, 4.0, 6), rtol=0, atol=5e-9)
        assert np.allclose(d["density"], p, rtol=1e-8, atol=0) and np.allclose(d["sem"], sem, rtol=1e-8, atol=0)
    with open(path, "w") as f:
        f.write("# something else\n")
    with pytest.raises(ValueError, match="not a molecule_energy.dat"):
        me.read_dat(path)


def test_counts_file_round_trip_and_is_reproducible(tmp_path):
    hist, group = _synthetic()
    spec = dict(e_min=-8.0, e_max=4.0, n_bins=6, every=2, types=[1, 0])
    samples = np.full(5, 3, dtype=np.uint64)
    for n in ("a.npz", "b.npz"):
        me.write_counts(str(tmp_path / n), hist, samples, group, spec)
    assert open(tmp_path / "a.npz", "rb").read() == open(tmp_path / "b.npz", "rb").read()
    z = me.read_counts(str(tmp_path / "a.npz"))
    assert sorted(z) == ["e_max", "e_min", "every", "group", "hist", "n_bins", "samples", "types"]
    assert np.array_equal(z["hist"], hist) and z["hist"].dtype == np.uint64 and np.array_equal(z["samples"], samples)
    assert z["types"].tolist() == [1, 0] and z["group"].tolist() == [0, 1, 0, 1, 0]
    assert float(z["e_min"]) == -8.0 and float(z["e_max"]) == 4.0 and int(z["n_bins"]) == 6 and int(z["every"]) == 2


# ---- the option -----------------------------------------------------------------------------------------------------------------
def _topo():
    topo = golden_system("framework_small")[1].topo
    assert [int(v) for v in topo.is_active] == [0, 1], "a frozen framework and an active guest"
    return topo


def test_check_spec_accepts_and_fills_the_defaults():
    topo = _topo()
    assert me.check_spec(dict(e_min=-10, e_max=2.5, n_bins=64), topo) == dict(e_min=-10.0, e_max=2.5, n_bins=64, every=1, types=[1])
    assert me.check_spec(dict(e_min=-1.0, e_max=0.0, n_bins=1, every=3, types=(1,)), topo)["every"] == 3
    assert me.check_spec(dict(e_min=-1.0, e_max=0.0, n_bins=4096), topo)["n_bins"] == 4096
    both = types.SimpleNamespace(n_res=3, is_active=[1, 0, 1])
    assert me.check_spec(dict(e_min=-1.0, e_max=0.0, n_bins=2), both)["types"] == [0, 2]
    assert me.check_spec(dict(e_min=-1.0, e_max=0.0, n_bins=2, types=[2, 0]), both)["types"] == [2, 0]
    a = me.identity_array(me.check_spec(dict(e_min=-1.0, e_max=0.5, n_bins=2, types=[2, 0], every=4), both))
    assert a.dtype == np.float64 and a.tolist() == [-1.0, 0.5, 2.0, 4.0, 2.0, 0.0]


@pytest.mark.parametrize("spec, text", [
    (dict(e_min=-1.0, e_max=0.0, n_bins=4, bins=3), r"\['bins'\] unknown"),
    (dict(e_max=0.0, n_bins=4), "e_min is missing"),
    (dict(e_min=-1.0, n_bins=4), "e_max is missing"),
    (dict(e_min=-1.0, e_max=0.0), "n_bins is missing"),
    (dict(e_min=0.0, e_max=0.0, n_bins=4), "e_min must be below e_max"),
    (dict(e_min=1.0, e_max=0.0, n_bins=4), "e_min must be below e_max"),
    (dict(e_min=-math.inf, e_max=0.0, n_bins=4), "must be finite"),
    (dict(e_min=0.0, e_max=math.nan, n_bins=4), "must be finite"),
    (dict(e_min=-1.0, e_max=0.0, n_bins=0), r"n_bins must lie in \[1, 4096\]"),
    (dict(e_min=-1.0, e_max=0.0, n_bins=4097), r"n_bins must lie in \[1, 4096\]"),
    (dict(e_min=-1.0, e_max=0.0, n_bins=4, every=0), "every must be at least 1"),
    (dict(e_min=-1.0, e_max=0.0, n_bins=4, types=[2]), r"residue type 2 is outside the residue types \[0, 1\]"),
    (dict(e_min=-1.0, e_max=0.0, n_bins=4, types=[-1]), "residue type -1 is outside the residue types"),
    (dict(e_min=-1.0, e_max=0.0, n_bins=4, types=[0]), "residue type 0 is not an active type"),
    (dict(e_min=-1.0, e_max=0.0, n_bins=4, types=[1, 1]), "residue type 1 is given twice"),
    (dict(e_min=-1.0, e_max=0.0, n_bins=4, types=[]), "the selection is empty"),
])
def test_check_spec_refusals(spec, text):
    with pytest.raises(ValueError, match="molecule_energy: .*" + text):
        me.check_spec(spec, _topo())


def test_parse_spec_and_types():
    assert me.parse_spec("-12.5,2,64") == dict(e_min=-12.5, e_max=2.0, n_bins=64, every=1)
    assert me.parse_spec(" -3 , 0.5 , 4096 , 5 ") == dict(e_min=-3.0, e_max=0.5, n_bins=4096, every=5)
    for bad in ("-1,0", "-1,0,4,1,2", "x,0,4", "-1,0,4.5", "0,0,4", "1,0,4", "-1,0,0", "-1,0,4097", "-1,0,4,0", "nan,0,4", "-inf,0,4"):
        with pytest.raises(ValueError, match="--molecule-energy"):
            me.parse_spec(bad)
    assert me.parse_types("co2, frame", ["frame", "co2"]) == [1, 0]
    for bad, text in (("", "empty list"), ("water", "unknown residue name 'water'"), ("co2,co2", "given twice")):
        with pytest.raises(ValueError, match="--molecule-energy-types.*" + text):
            me.parse_types(bad, ["frame", "co2"])


def test_command_line_refusals(capsys, tmp_path):
    base = ["-i", "x.maniac", "-d", "x.data", "-p", "x.inc", "-o", str(tmp_path)]
    for extra, text in ((["--molecule-energy", "-10,0,32"], "--molecule-energy and --molecule-energy-types need --replicas"),
                        (["--molecule-energy-types", "co2"], "--molecule-energy and --molecule-energy-types need --replicas"),
                        (["--replicas", "2", "--molecule-energy-types", "co2"], "--molecule-energy-types needs --molecule-energy"),
                        (["--replicas", "2", "--molecule-energy", "-10,0"], "EMIN,EMAX,BINS"),
                        (["--replicas", "2", "--molecule-energy", "0,-10,32"], "EMIN must be below EMAX"),
                        (["--replicas", "2", "--molecule-energy", "-10,0,5000"], "BINS must lie in")):
        with pytest.raises(SystemExit) as err:
            run.main(base + extra)
        assert err.value.code == 2
        msg = capsys.readouterr().err
        assert text in msg, (extra, msg)
    # the names are the input file's
    with pytest.raises(SystemExit):
        run.main(["-i", INPUTS[0], "-d", INPUTS[1], "-p", INPUTS[2], "-o", str(tmp_path), "--replicas", "2",
                  "--molecule-energy", "-10,0,32", "--molecule-energy-types", "nothing"])
    assert "unknown residue name 'nothing'" in capsys.readouterr().err


def test_run_replicas_refuses_a_bad_option_before_a_farm_exists(tmp_path, monkeypatch):
    def no_farm(*a, **k):
        raise AssertionError("a farm was created")
    monkeypatch.setattr(replicas, "FortranFarm", no_farm)
    for bad, text in ((dict(e_min=0.0, e_max=-1.0, n_bins=8), "e_min must be below e_max"),
                      (dict(e_min=-1.0, e_max=0.0, n_bins=8, width=1), "unknown"),
                      (dict(e_min=-1.0, e_max=0.0, n_bins=8, types=[3]), "outside the residue types")):
        with pytest.raises(ValueError, match="molecule_energy: .*" + text):
            replicas.run_replicas(*INPUTS, str(tmp_path / "out"), replicas=2, molecule_energy=bad)
    assert not os.path.exists(tmp_path / "out")
