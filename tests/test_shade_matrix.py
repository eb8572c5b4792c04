"""The shading-branch scene matrix (tests/shade_scenes.py) on the CPU: the scenes reach the branches they were built for (the
oracle's branch counters), the oracle's mirror of the product gives the plain restatement's image on them, and the plain
restatement agrees with an independent float64 arbiter (tests/f64_arbiter.py) wherever no random numbers are involved."""
import numpy as np
import pytest

import oracle_lib as ol
import pyscene
import shade_scenes
from f64_arbiter import Arbiter, CLEAR

TOL = 1e-4


def _oracle(case):
    sc = pyscene.parse_lines(case.text.split("\n"))
    return sc, ol.OracleScene(sc, bounds_mode=0)


def _mirror(case, sc, o):
    return ol.product_flags(len(sc.triangles) > 0, skip_unlit=case.skip_unlit, nprims=len(sc.refs), grid_ok=o.grid_ok())


def test_the_matrix_has_the_scenes_the_gpu_tests_name():
    names = set(shade_scenes.ALL)
    assert {"lights_0", "lights_33_mixed", "lights_64_bulbs", "inf_colour", "nan_light_colour", "expose_zero", "tir_first_b1", "glass_in_glass_b5",
            "gi_chain_g3_b1", "closed_box_b16_g3", "planes_8", "plane_tie"} <= names
    for name, case in shade_scenes.ALL.items():
        sc = pyscene.parse_lines(case.text.split("\n"))
        assert len(sc.refs) <= 20 and case.w <= 64 and case.h <= 48, name
        assert case.skip_unlit == (len(sc.suns) + len(sc.bulbs) <= 32 and name not in ("inf_colour", "nan_light_colour")), name


@pytest.mark.parametrize("name", list(shade_scenes.ALL))
def test_every_scene_reaches_the_branches_it_was_built_for(name):
    """A condition on the test data, met by the oracle alone: at spp 0, under the flags that mirror the product's default mode,
    every branch counter the scene names is at least 10."""
    case = shade_scenes.ALL[name]
    sc, o = _oracle(case)
    br = o.render_branches(case.w, case.h, 0, flags=_mirror(case, sc, o), nthreads=8)["branches"]
    o.close()
    assert case.targets
    for k in case.targets:
        assert br[k] >= 10, (k, br[k])


def test_no_row_of_the_branch_table_is_zero_over_the_matrix():
    """The counters of refractionLight's rare paths (never taken by the edge scenes or redchair.txt; `refr_tir_first` by no scene
    that existed), and every other counter, summed over the matrix at spp 0."""
    total = dict.fromkeys(ol.BRANCH_FIELDS, 0)
    for case in shade_scenes.ALL.values():
        sc, o = _oracle(case)
        br = o.render_branches(case.w, case.h, 0, flags=_mirror(case, sc, o), nthreads=8)["branches"]
        o.close()
        for k, v in br.items():
            total[k] += v
    print(total)
    assert all(v >= 10 for v in total.values()), total


@pytest.mark.parametrize("spp", [0, 5])
@pytest.mark.parametrize("name", list(shade_scenes.ALL))
def test_the_mirror_equals_the_reference_walk_on_the_matrix(name, spp):
    """The oracle under the flags the GPU tests compare with (skip_unlit off exactly where the product switches it off) against its
    plain restatement of the reference (flags = 0): same float image bit for bit, same bytes, same rays."""
    case = shade_scenes.ALL[name]
    sc, o = _oracle(case)
    plain = o.render(case.w, case.h, spp, flags=0, nthreads=8)
    mirror = o.render(case.w, case.h, spp, flags=_mirror(case, sc, o), nthreads=8)
    o.close()
    both_nan = np.isnan(plain["f32"]) & np.isnan(mirror["f32"])
    assert np.array_equal(np.where(both_nan, 0, plain["f32"].view(np.uint32)), np.where(both_nan, 0, mirror["f32"].view(np.uint32)))
    assert np.array_equal(plain["u8"], mirror["u8"])
    assert plain["stats"]["rays"] == mirror["stats"]["rays"]


def test_skipping_unlit_lights_would_change_a_non_finite_scene():
    """Why the host switch exists (0 * inf is NaN): with ORC_FLAG_SKIP_UNLIT the NaN pattern of inf_colour differs from the
    reference's -- the mirror the GPU tests use for it must not set the flag."""
    case = shade_scenes.ALL["inf_colour"]
    sc, o = _oracle(case)
    plain = o.render(case.w, case.h, 0, flags=0, nthreads=8)
    skipping = o.render(case.w, case.h, 0, flags=ol.product_flags(False, skip_unlit=True), nthreads=8)
    o.close()
    assert not np.array_equal(np.isnan(plain["f32"]), np.isnan(skipping["f32"]))


# Scenes on which float32 legitimately differs from float64 by more than TOL on a clear pixel: the measured worst difference
# (oracle, flags = 0, against the arbiter); such a scene is bound at twice it.
#   closed_box_b8_g0: 1.51e-3 at pixel (21, 19), a sample of 211 rays through up to eight curved glass surfaces next to a point
#   light.  The pixel is that ill-conditioned in float64 alone: moving the camera by 1e-7 moves the arbiter's own value by 3.5e-3.
MEASURED_WORST = {"closed_box_b8_g0": 1.51e-3}

# Not put to the arbiter: closed_box_b16_g0.  A pixel of it takes some 1 900 rays and 50 000 decisions; 124 of its 768 pixels
# (16 %) have one with a margin below 1e-4 -- the 5 % cap cannot be met at that depth by moving the camera -- and the Python
# restatement needs 66 s for the frame.  (closed_box at bounces 1, 2 and 8 is.)
ARBITER_TOO_DEEP = ("closed_box_b16_g0",)

RNG_FREE = [n for n, c in shade_scenes.ALL.items() if c.rng_free and n not in ARBITER_TOO_DEEP]


@pytest.mark.parametrize("name", RNG_FREE)
def test_the_oracle_agrees_with_the_float64_arbiter_on_clear_pixels(name):
    """spp 0, no random numbers: on every pixel whose decisions all have a relative margin above 1e-4 in the float64
    restatement the oracle's float image (flags = 0) is within TOL of it, with the same NaN / infinity pattern; at most 5 % of
    the pixels that hit anything may be unclear (a property of the float64 restatement alone)."""
    case = shade_scenes.ALL[name]
    sc, o = _oracle(case)
    got = o.render(case.w, case.h, 0, flags=0, nthreads=8)["f32"].astype(np.float64)
    o.close()
    arb = Arbiter(sc)
    want = np.zeros((case.h, case.w, 4))
    margin = np.zeros((case.h, case.w))
    hit = np.zeros((case.h, case.w), bool)
    for y in range(case.h):
        for x in range(case.w):
            want[y, x], margin[y, x], hit[y, x] = arb.pixel(x, y, case.w, case.h)
    clear = margin > CLEAR
    unclear = int((hit & ~clear).sum())
    assert hit.sum() >= 100
    assert unclear <= 0.05 * hit.sum(), (unclear, int(hit.sum()))
    assert np.array_equal(np.isnan(got[clear]), np.isnan(want[clear]))
    same = (np.isnan(got) & np.isnan(want)) | (np.isinf(got) & (got == want))
    with np.errstate(invalid="ignore"):
        d = np.where(same | ~clear[..., None], 0.0, np.abs(got - want))
    worst = float(d.max())
    print(f"{name}: clear {int(clear.sum())} of {clear.size}, unclear among hits {unclear} of {int(hit.sum())}, worst |oracle - float64| {worst:.3g}")
    assert worst <= 2.0 * MEASURED_WORST.get(name, TOL / 2.0), (worst, np.unravel_index(np.argmax(d), d.shape))
