"""The energy decomposition's host side (maniac_mc_amd/energy_pairs.py, checkpoint.check), without the library or a device:
the switches' parsing and errors, the default selection, the per-replica file's round trip, the pooled file against NumPy,
the checkpoint identity and its refusals."""
import numpy as np
import pytest

from maniac_mc_amd import checkpoint, energy_pairs as ep
from maniac_mc_amd.system import KB_KCALMOL
from tests.util import golden_system


def test_spec_parsing():
    assert ep.parse_spec(None) == dict(every=1) and ep.parse_spec("") == dict(every=1)
    assert ep.parse_spec("3") == dict(every=3) and ep.parse_spec(" 1 ") == dict(every=1)
    for bad in ("0", "-2", "x", "1.5", "2,3"):
        with pytest.raises(ValueError, match="--energy-pairs"):
            ep.parse_spec(bad)


def test_select_parsing_and_its_errors():
    names = ["FRAME", "H2O", "CO2"]
    assert ep.parse_select("FRAME:H2O,H2O:H2O", names) == [(0, 1), (1, 1)]
    assert ep.parse_select(" CO2:FRAME , H2O:CO2 ", names) == [(0, 2), (1, 2)], "either order inside a pair, the order given"
    for bad, what in (("FRAME:XYZ", "unknown residue name 'XYZ'"), ("FRAME:H2O,H2O:FRAME", "duplicate"), ("", "empty list"),
                      (" , ", "empty list"), ("FRAME", "NAME:NAME"), ("FRAME:H2O:CO2", "NAME:NAME"), ("FRAME:", "NAME:NAME")):
        with pytest.raises(ValueError) as err:
            ep.parse_select(bad, names)
        assert "--energy-pairs-select" in str(err.value) and what in str(err.value), (bad, str(err.value))


def test_pair_checks():
    assert ep.check_pairs([(1, 0), (1, 1)], 2) == [(0, 1), (1, 1)]
    for bad, what in (([], "empty"), ([(0, 2)], r"\(0, 2\)"), ([(-1, 0)], r"\(-1, 0\)"), ([(0, 1), (1, 0)], "duplicate")):
        with pytest.raises(ValueError, match=what):
            ep.check_pairs(bad, 2)
    with pytest.raises(ValueError, match="at most 36"):
        ep.check_pairs([(a, b) for a in range(9) for b in range(a, 9)], 9)


def test_default_pairs_leave_out_inactive_inactive():
    mix = golden_system("mixture")[1].topo
    assert list(mix.is_active) == [1, 1]
    assert ep.default_pairs(mix) == [(0, 0), (0, 1), (1, 1)]
    fw = golden_system("framework_small")[1].topo
    assert list(fw.is_active) == [0, 1]
    assert ep.default_pairs(fw) == [(0, 1), (1, 1)], "framework-framework is a constant: not sampled by default"
    assert ep.pair_names(ep.default_pairs(fw), ["FRAME", "H2O"]) == ["FRAME:H2O", "H2O:H2O"]


def test_identity_array():
    a = ep.identity_array(dict(every=2, pairs=[(0, 1), (1, 1)]))
    assert a.dtype == np.int64 and a.tolist() == [2, 0, 1, 1, 1]
    assert not np.array_equal(a, ep.identity_array(dict(every=1, pairs=[(0, 1), (1, 1)])))
    assert ep.identity_array(dict(every=2, pairs=[(1, 1), (0, 1)])).tolist() == [2, 1, 1, 0, 1], "the order of the pairs counts"


def _values(rng, n_sel):
    return rng.normal(0.0, 3.0e4, (n_sel, 5))


def test_per_replica_file_round_trip(tmp_path):
    rng = np.random.default_rng(5)
    labels = ["FRAME:H2O", "H2O:H2O"]
    path = str(tmp_path / ep.FILE_NAME)
    ep.start_replica_file(path, labels)
    assert ep.read_replica_file(path)[1].size == 0, "no block-0 line"
    written = {}
    for block in (2, 4, 6):
        written[block] = _values(rng, 2)
        ep.append_replica_file(path, block, written[block])
    text = open(path).read().splitlines()
    assert len(text) == 4 and text[0].startswith("#") and "FRAME:H2O" in text[0] and "H2O:H2O" in text[0]
    assert all(len(ln) == 10 + 12 * (ep.WIDTH + 1) for ln in text[1:]), "fixed width"
    got_labels, blocks, values = ep.read_replica_file(path)
    assert got_labels == labels and blocks.tolist() == [2, 4, 6] and values.shape == (3, 2, 6)
    for i, block in enumerate((2, 4, 6)):
        v = written[block]
        want = np.concatenate([v * KB_KCALMOL, ((v[:, 0] + v[:, 1] + v[:, 2] + v[:, 3] + v[:, 4]) * KB_KCALMOL)[:, None]], axis=1)
        assert np.allclose(values[i], want, rtol=0.0, atol=0.5000001e-6), "what %.6f keeps"
        assert text[1 + i] == ep.block_line(block, v).rstrip("\n")
    with pytest.raises(ValueError, match="not an energy_pairs.dat"):
        other = tmp_path / "other.dat"
        other.write_text("1 2 3\n")
        ep.read_replica_file(str(other))


def test_pooled_file_against_numpy(tmp_path):
    rng = np.random.default_rng(8)
    labels = ["FRAME:H2O", "H2O:H2O", "CO2:CO2"]
    R, blocks = 6, (1, 2, 3, 4)
    group = np.arange(R) % 2
    paths = []
    for r in range(R):
        p = str(tmp_path / f"r{r}.dat")
        ep.start_replica_file(p, labels)
        for b in blocks:
            ep.append_replica_file(p, b, _values(rng, 3))
        paths.append(p)
    out = str(tmp_path / ep.FILE_NAME)
    ep.write_pooled_file(out, paths, group, [0.5, 2.0])
    rows = ep.read_pooled_file(out)
    assert [(r[0], r[4]) for r in rows] == [(g, lab) for g in (0, 1) for lab in labels]
    per = np.array([ep.read_replica_file(p)[2].mean(axis=0) for p in paths])          # (R, 3, 6) from the files as printed
    for g, f_atm, n_rep, n_blocks, lab, mean, sem in rows:
        assert f_atm == [0.5, 2.0][g] and n_rep == 3 and n_blocks == 4
        x = per[group == g][:, labels.index(lab), :]
        assert np.allclose(mean, x.mean(axis=0), rtol=0.0, atol=0.5000001e-6)
        assert np.allclose(sem, x.std(axis=0, ddof=1) / np.sqrt(3), rtol=0.0, atol=0.5000001e-6)
    # one replica per group: no spread to report; written twice: the same bytes
    ep.write_pooled_file(out, paths[:2], group[:2])
    assert all(r[2] == 1 and not r[6].any() for r in ep.read_pooled_file(out))
    first = open(out, "rb").read()
    ep.write_pooled_file(out, paths[:2], group[:2])
    assert open(out, "rb").read() == first
    # files that do not belong together are refused
    ep.append_replica_file(paths[1], 5, _values(rng, 3))
    with pytest.raises(ValueError, match="another number of sampled blocks"):
        ep.write_pooled_file(out, paths, group)


def _ident(**more):
    d = dict(abi_version=2, nb_step=40, seed=1, mode="windows", replicas=4, fugacities=np.array([1.0, 2.0]),
             frames=np.array([0], dtype=np.int64), digest_maniac="a", digest_data="b", digest_inc="c", digest_reservoir="",
             recalibrate=0)
    d.update(more)
    return d


def _ck(ident):
    ck = {"id_" + k: np.asarray(v) for k, v in ident.items()}
    ck["next_block"] = np.int64(3)
    return ck


def test_checkpoint_refusals_name_the_switch():
    spec = dict(every=1, pairs=[(0, 1), (1, 1)])
    with_it = _ident(energy_pairs=ep.identity_array(spec))
    without = _ident()
    checkpoint.check(_ck(with_it), with_it, 4)
    checkpoint.check(_ck(without), without, 4)
    assert "id_energy_pairs" not in _ck(without), "a run without the option writes no such key"
    for ck_ident, run_ident in ((with_it, without),                                              # resumed without the option
                                (without, with_it),                                              # resumed with it
                                (with_it, _ident(energy_pairs=ep.identity_array(dict(every=1, pairs=[(1, 1)])))),
                                (with_it, _ident(energy_pairs=ep.identity_array(dict(every=2, pairs=spec["pairs"]))))):
        with pytest.raises(ValueError) as err:
            checkpoint.check(_ck(ck_ident), run_ident, 4)
        assert "--energy-pairs" in str(err.value) and str(err.value).startswith("resume:"), str(err.value)
    # the histograms' refusal is still the first one a run with both options meets
    both = _ident(rdf=np.array([1.0]), energy_pairs=ep.identity_array(spec))
    with pytest.raises(ValueError, match="--rdf"):
        checkpoint.check(_ck(both), without, 4)
