"""The arithmetic of the quantised box test as written, before a GPU sees it: tests/qbox_ref.py's float32 restatement of qlo / qhi,
quantised_axis and the quantised slab test against exact rational arithmetic, on the cases tests/test_gpu_qbox.py gives the
device.  Assertions (a) to (d) of qbox_ref.check_cases -- the packed words bound the box within three grid steps, a ray that
enters the grid box is never culled, a box box_pair admits is never culled, and a hit lies within the derived growth of the grid
box -- and in every regime at least a tenth of the cases enter the grid box and at least a tenth are answered "miss", so neither
implication is vacuous.  No GPU, no library."""
from fractions import Fraction

import numpy as np
import pytest

import qbox_ref as Q

N_PER_REGIME = 700


@pytest.mark.parametrize("regime", Q.REGIMES)
def test_the_restatement_keeps_the_claims(regime):
    cases = Q.make_cases(regime, N_PER_REGIME, seed=2024)
    want = Q.restate(cases)
    enters, misses = Q.check_cases(cases, want, want)
    print(f"{regime}: the ray enters the grid box in {enters:.0%} of the cases, the quantised test says miss in {misses:.0%}")
    assert enters >= 0.10 and misses >= 0.10, (regime, enters, misses)


def test_the_generator_is_seeded_and_covers_what_it_names():
    a, b = Q.make_cases("random", 50, seed=7), Q.make_cases("random", 50, seed=7)
    assert a.tobytes() == b.tobytes() and a.tobytes() != Q.make_cases("random", 50, seed=8).tobytes()
    for regime in Q.REGIMES:
        c = Q.make_cases(regime, 400, seed=1)
        assert np.all(c["smin"] <= c["lo"]) and np.all(c["lo"] <= c["hi"]) and np.all(c["hi"] <= c["smax"]), regime
        size = c["smax"] - c["smin"]
        assert np.all(np.maximum(np.abs(c["smin"]), np.abs(c["smax"])) <= 64 * size + (size == 0) * 1e30), regime      # grid_ok
    c = Q.make_cases("thin", 400, seed=1)
    assert np.any(np.all(c["lo"] == c["hi"], axis=1) | np.any(c["lo"] == c["hi"], axis=1))
    c = Q.make_cases("touching", 400, seed=1)
    assert np.any(c["lo"] == c["smin"]) and np.any(c["hi"] == c["smax"]) and np.any(np.all((c["lo"] == c["smin"]) & (c["hi"] == c["smax"]), axis=1))
    c = Q.make_cases("flat_scene", 400, seed=1)
    assert np.all(np.sum(c["smin"] == c["smax"], axis=1) == 1) and np.any(Q.restate(c)["step"] == 1.0)
    c = Q.make_cases("tiny_direction", 400, seed=1)
    for v in Q.TINY:
        assert np.any(c["d"].view(np.uint32) == np.float32(v).view(np.uint32)), v
    with np.errstate(over="ignore"):
        assert np.isinf(np.float32(1.0) / np.float32(-1e-39))
    c = Q.make_cases("on_plane", 400, seed=1)
    assert np.any(c["o"] == c["lo"]) and np.any(c["o"] == c["hi"]) and np.any(c["d"] == 0)
    c = Q.make_cases("finite_tbest", 400, seed=1)
    assert np.all(np.isfinite(c["tbest"]))
    far = Q.make_cases("far", 400, seed=1)
    reach = np.linalg.norm(far["o"].astype(np.float64) - 0.5 * (far["lo"] + far["hi"]), axis=1) / np.max(far["smax"] - far["smin"], axis=1)
    assert reach.max() > 5e4 and reach.min() > 500


def test_fma32_rounds_once():
    """The case a float64 sum rounded twice gets wrong: the product is a float32 midpoint, the addend far below it."""
    a, b, c = np.float32([1 + 2.0 ** -12]), np.float32([1 + 2.0 ** -12]), np.float32([2.0 ** -60])
    exact = Fraction(float(a[0])) * Fraction(float(b[0])) + Fraction(float(c[0]))
    lo, hi = np.float32(1 + 2.0 ** -11), np.nextafter(np.float32(1 + 2.0 ** -11), np.float32(2))
    want = lo if exact - Fraction(float(lo)) < Fraction(float(hi)) - exact else hi
    assert Q.fma32(a, b, c)[0] == want == hi
    assert np.float32(np.float64(a[0]) * np.float64(b[0]) + np.float64(c[0])) == lo      # (the double rounding)


def test_exact_enters_on_the_cases_it_defines():
    inf, tmin = np.float32(np.inf), Q.TMIN
    box = ([0, 0, 0], [1, 1, 1])
    assert Q.exact_enters(*box, [-1, 0.5, 0.5], [1, 0, 0], inf, tmin)
    assert not Q.exact_enters(*box, [-1, 1.0, 0.5], [1, 0, 0], inf, tmin)          # d == 0 and the origin on a plane: undecided
    assert Q.exact_enters(*box, [-1, 1.0, 0.5], [1, 0, 0], inf, tmin, strict=False)
    assert not Q.exact_enters(*box, [-1, 0.5, 0.5], [1, 0, 0], 1.0, tmin)          # t_enter == tbest
    assert Q.exact_enters(*box, [-1, 0.5, 0.5], [1, 0, 0], 1.0, tmin, strict=False)
    assert not Q.exact_enters(*box, [-1, 0.5, 0.5], [-1, 0, 0], inf, tmin)         # behind the origin
    assert not Q.exact_enters(*box, [-1, -1, 0.5], [1, 1, -0.0], 0.5, tmin)
    assert not Q.exact_enters([0, 0, 0], [1, 0, 1], [-1, -1, 0.5], [1, 1, 0], inf, tmin)      # a flat box: t_enter == t_exit
