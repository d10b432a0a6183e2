"""The shared far row of the Coulomb table (CPU test, through mgpu_coulomb_table_eval as tests/test_coulomb_table.py).

Where a box reaches distances at which one term of unit charge product is worth no more than 1e-12 K
(167101 K A * erfc(alpha r)/r <= 1e-12), the table ends in ONE row that starts at the first row start s_far of that kind
and holds the constant G(s_far): every lookup from there on reads the same LDS address.  G falls with s, so such a
lookup is wrong by less than G(s_far) itself, i.e. by at most 1e-12 K per unit charge product -- a tenth of the bar the
table is held to beyond alpha r = 1.  Rows below s_far, and the whole table of a box that does not reach s_far, are
what they were.
"""
import numpy as np
import pytest

from maniac_mc_amd import _lib
from tests.test_coulomb_table import table_G

mp = pytest.importorskip("mpmath")

KELVIN = 167101.0
BOUND_K = 1e-12
CASES = [(0.2346370178899813, 40.4), (0.16, 87.0), (0.30995665486983587, 40.4)]


def exact_G(alpha, s):
    a = mp.mpf(alpha)
    return [mp.erfc(a * mp.sqrt(mp.mpf(float(v)))) / mp.sqrt(mp.mpf(float(v))) for v in np.atleast_1d(s)]


def row_starts():
    """Every row start of the table from r^2 = 0.25 on: 64 rows per binary octave."""
    return np.array([2.0 ** e * (1.0 + q / 64.0) for e in range(-2, 16) for q in range(64)])


def far_row(alpha):
    """(s_far, start of the row before it), s_far derived from alpha alone in 50 digits."""
    mp.mp.dps = 50
    starts = row_starts()
    g = exact_G(alpha, starts)
    k = next(i for i, v in enumerate(g) if mp.mpf(KELVIN) * v <= mp.mpf(BOUND_K))
    return float(starts[k]), float(starts[k - 1])


def abs_err(alpha, s, got):
    return np.array([abs(float(mp.mpf(float(g)) - e)) for g, e in zip(got, exact_G(alpha, s))])


@pytest.mark.parametrize("alpha,half_diag", CASES)
def test_far_row_is_positive_and_within_its_bound(alpha, half_diag):
    _lib.build()
    s_far, s_prev = far_row(alpha)
    r2_max = half_diag ** 2
    assert s_far < r2_max
    if alpha == CASES[0][0]:
        assert 24.0 ** 2 < s_far < 25.5 ** 2              # about 24.7 A for the benchmark's alpha
    rng = np.random.default_rng(23)
    s = np.concatenate([[s_far, np.nextafter(s_far, 0.0), np.nextafter(s_far, np.inf), s_prev],
                        np.exp(rng.uniform(np.log(s_prev), np.log(r2_max), 1000)),
                        [np.nextafter(r2_max, 0.0)]])
    got = table_G(alpha, r2_max, s)
    assert np.all(got > 0.0)
    err = abs_err(alpha, s, got) * KELVIN
    print(f"alpha {alpha}: r_far {np.sqrt(s_far):.4f} A, max |dG| * 167101 = {err.max():.3e} K, shared value {got[0]:.3e}")
    assert err.max() <= BOUND_K, err.max()
    # one value from s_far on, whatever the lane's own row and t
    assert np.all(got[s >= s_far] == got[0])
    assert got[1] > got[0] and got[3] > got[1]            # the rows below it still fall with s


@pytest.mark.parametrize("alpha,half_diag", CASES)
def test_rows_below_the_far_row_are_bit_identical(alpha, half_diag):
    _lib.build()
    s_far, _ = far_row(alpha)
    rng = np.random.default_rng(5)
    starts = row_starts()
    starts = starts[starts < s_far]
    s = np.concatenate([np.exp(rng.uniform(np.log(0.25), np.log(s_far), 4000)), starts, np.nextafter(starts[1:], 0.0),
                        [np.nextafter(s_far, 0.0)]])
    s = s[s < s_far]
    with_rule = table_G(alpha, half_diag ** 2, s)
    without = table_G(alpha, np.nextafter(s_far, 0.0), s)          # a box that stops short of s_far: the table as it was
    assert np.array_equal(with_rule, without)


@pytest.mark.parametrize("alpha,half_diag", CASES)
def test_a_box_short_of_the_far_row_keeps_its_whole_table(alpha, half_diag):
    """The table of r2_max < s_far still runs to the end of r2_max's binary octave in REAL rows: beyond s_far it follows
    G itself.  (Bound: a row there spans alpha^2 ds ~ 0.5 in the exponent of G; the degree-6 interpolation leaves
    (0.27)^7 / (7! 2^6) ~ 3e-10 of G and the two fp32 coefficients ~2e-11, so 1e-8 relative holds with room, while the
    constant row would be off by tens of per cent.)"""
    _lib.build()
    mp.mp.dps = 50
    s_far, s_prev = far_row(alpha)
    r2_max = float(np.nextafter(s_far, 0.0))
    octave_end = 2.0 ** (np.floor(np.log2(s_far)) + 1)
    assert s_far > 0.5 * octave_end                       # (s_far does not open an octave for these alphas: rows follow it)
    s = np.linspace(s_far, np.nextafter(octave_end, 0.0), 200)
    got = table_G(alpha, r2_max, s)
    ref = np.array([float(e) for e in exact_G(alpha, s)])
    assert np.all(got > 0.0)
    assert np.max(np.abs(got - ref) / ref) <= 1e-8, np.max(np.abs(got - ref) / ref)
    assert np.all(np.diff(got) < 0.0)
    # and below s_far it is the table every larger box has
    lo = np.exp(np.random.default_rng(9).uniform(np.log(0.25), np.log(s_prev), 2000))
    assert np.array_equal(table_G(alpha, r2_max, lo), table_G(alpha, half_diag ** 2, lo))
