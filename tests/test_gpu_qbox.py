"""The quantised box test on the device, case by case, against exact rational arithmetic (tests/qbox_ref.py).

mirt_probe_qbox runs the builder's qlo / qhi and the walk's quantised_axis, box_pair, box_pair_q (the packed box in the left slot,
then in the right one) and box_q on one case per thread.  Per case (qbox_ref.check_cases):
  (a) the six grid coordinates, the step and 2^60 / step equal the float32 restatement bit for bit, and -- independently of it --
      bound the box from outside by less than three grid steps (the form at q_hi == 65535: check_words);
  (b) a ray that enters the grid box, in exact arithmetic, is a hit in all three quantised forms (no tolerance);
  (c) a box that box_pair admits on the device is a hit in all three quantised forms;
  (d) where every |d_k| >= 2^-20, a quantised hit is a non-strict hit of the grid box grown by qbox_ref.growth;
  (e) the three quantised forms agree with each other and with the restatement, bit for bit, in the hit flag and in te
      (box_q returns no te).
In every regime at least a tenth of the cases have the antecedent of (b) true and at least a tenth are answered "miss".
2 000 cases per regime, 20 000 in all; the device time is nothing, the Fractions take about a second per regime."""
import numpy as np
import pytest

from cuda_ray_tracer_amd import api, layouts
import qbox_ref as Q

pytestmark = pytest.mark.gpu

N_PER_REGIME = 2000


def test_the_probes_rows_are_the_references():
    assert layouts.QBOX_CASE == Q.CASE and layouts.QBOX_RESULT == Q.RESULT


@pytest.mark.parametrize("regime", Q.REGIMES)
def test_the_device_keeps_the_claims(regime):
    cases = Q.make_cases(regime, N_PER_REGIME, seed=950)
    got = api.probe_qbox(cases)
    want = Q.restate(cases)
    # (e) the three copies of the arithmetic, before anything is compared with the restatement
    hit = got["hit"]
    assert np.array_equal(hit[:, 1], hit[:, 2]) and np.array_equal(hit[:, 1], hit[:, 3]), np.flatnonzero((hit[:, 1] != hit[:, 2]) | (hit[:, 1] != hit[:, 3]))[:5]
    assert Q.same_floats(got["te"][:, 1], got["te"][:, 2]).all()
    assert not got["pad"].any() and set(np.unique(hit)) <= {0, 1}
    enters, misses = Q.check_cases(cases, got, want)
    print(f"{regime}: the ray enters the grid box in {enters:.1%} of the cases, the quantised test says miss in {misses:.1%}")
    assert enters >= 0.10 and misses >= 0.10, (regime, enters, misses)


def test_bad_arguments_are_errors():
    import cuda_ray_tracer_amd as m
    c = Q.make_cases("random", 4, seed=1)
    out = np.zeros(4, layouts.QBOX_RESULT)
    for args in ((0, 0, c.ctypes.data, out.ctypes.data), (0, 4, None, out.ctypes.data), (0, 4, c.ctypes.data, None)):
        assert m.lib().mirt_probe_qbox(*args) == 3
