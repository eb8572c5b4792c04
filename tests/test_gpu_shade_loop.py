"""The trace kernel's shade loop (render.hip: batch_next / advance for the lanes that are not traversing) under the options that
move lanes between its arms.  One pass of the loop first ends the batches whose last ray has finished and then shades, in the same
pass, those lanes together with the ones that arrived without a batch; which lanes meet in a pass depends on refill_k, batch_k,
init_k and reps, on the kernel's specialisation and on whether the frame's queue is empty -- the pixels and the counters may not.

Every scene is rendered under each option set through gpu_case.run_case (float image within 1e-4 of the oracle's, 8-bit image
within one level, every ray / node / leaf / material counter equal to the oracle's), and the sets must agree with each other byte
for byte and counter for counter.  The scenes are a few dozen primitives at 64 x 48; each puts lanes at another edge of the loop."""
import math

import numpy as np
import pytest

from gpu_case import COUNTER_KEYS, run_case

pytestmark = pytest.mark.gpu

W, H = 64, 48

# defaults; every batch transition happens in the shade phase (a lane leaves the traversal loop as soon as it waits, and the loop's
# own batch_next never collects 64 lanes); every batch transition in the traversal loop's header, one lane at a time; a refill at
# every shade phase; one traversal step per pass through the header; the general kernels
OPTION_SETS = {"defaults": {}, "shade_phase_batches": dict(refill_k=1, batch_k=64), "batch_k_1": dict(batch_k=1), "init_k_1": dict(init_k=1),
               "reps_1": dict(reps=1), "general": dict(specialise=0)}


def _spheres(n, material, z0=-4.0, seed=0):
    """n spheres on a jittered grid in front of the camera, above the floor y = -1; `material(i)` returns the lines that precede
    sphere i."""
    out = []
    cols = int(math.ceil(math.sqrt(n * 1.5)))
    for i in range(n):
        cx, cy = i % cols, i // cols
        jx = 0.3 * math.sin(12.9898 * (i + 1 + seed))
        jy = 0.25 * math.cos(78.233 * (i + 1 + seed))
        jz = 0.8 * math.sin(37.719 * (i + 1 + seed))
        x = (cx - 0.5 * (cols - 1)) * 0.85 + jx
        y = -0.55 + cy * 0.8 + jy
        r = 0.28 + 0.1 * (i % 3)
        out.append(material(i))
        out.append("sphere %.4f %.4f %.4f %.3f\n" % (x, y, z0 + jz, r))
    return "".join(out)


def _rough_mirror(i):
    return "color %.2f %.2f %.2f\nshininess %.2f\nroughness %.2f\n" % (0.3 + 0.1 * (i % 7), 0.9 - 0.1 * (i % 5), 0.4 + 0.05 * (i % 11),
                                                                      0.3 + 0.1 * (i % 4), 0.05 * (i % 3))


_TWO_SUNS = "color 1 1 1\nsun 1 1 0.5\ncolor 0.5 0.5 0.9\nsun -1 0.6 0.3\n"
_FLOOR = "color 0.7 0.7 0.7\nshininess 0.3\nroughness 0.02\nplane 0 1 0 1\n"


def _scene(body, bounces=4):
    return f"png {W} {H} loop.png\nbounces {bounces}\n" + body


def two_suns():
    """The headline scene's kind (the NOTRI | NOBULB | NOPEND kernel): two suns, a floor, rough reflective spheres."""
    return _scene(_TWO_SUNS + _FLOOR + _spheres(30, _rough_mirror))


def shininess_0():
    """No reflection ray anywhere: every batch ends on a shadow ray."""
    mat = lambda i: "color %.2f %.2f %.2f\nshininess 0\nroughness %.2f\n" % (0.3 + 0.1 * (i % 7), 0.9 - 0.1 * (i % 5), 0.5, 0.04 * (i % 3))
    return _scene(_TWO_SUNS + "color 0.7 0.7 0.7\nshininess 0\nplane 0 1 0 1\n" + _spheres(30, mat))


def no_lights():
    """A batch is the reflection ray alone; on a node without one it is empty and advance() runs twice in a row."""
    mat = lambda i: _rough_mirror(i) if i % 4 else "color 0.8 0.2 0.2\nshininess 0\nroughness 0\n"
    return _scene(_FLOOR + _spheres(30, mat))


def suns_below_the_horizon():
    """Both suns shine from below the floor: the floor faces away from them (every light unlit: the batch goes straight to the
    reflection ray) and the shadow rays of the spheres' undersides are answered by the floor, so start_ray leaves the lane waiting."""
    return _scene("color 1 1 1\nsun 0.3 -1 0.2\ncolor 0.5 0.5 0.9\nsun -0.5 -0.7 0.3\n" + _FLOOR + _spheres(30, _rough_mirror))


def camera_under_the_plane():
    """The camera below the floor looks up through it: the floor is seen from behind, and every shadow ray from there is cut off by
    nothing while those of the spheres above still are traced."""
    return _scene("eye 0 -2.5 1\nforward 0 0.45 -1\n" + _TWO_SUNS + _FLOOR + _spheres(30, _rough_mirror))


def bounces_1():
    """Every reflection ray would have bounce 0: has_reflect is false on every node."""
    return _scene(_TWO_SUNS + _FLOOR + _spheres(30, _rough_mirror), bounces=1)


def point_lights():
    """Point lights: the general kernels, and shadow rays whose hits the shade phase vets before batch_next reads them (a sun
    first, so that a lane can be between the two kinds)."""
    return _scene("color 1 1 1\nsun 1 1 0.5\ncolor 6 5 4\nbulb 0.5 2.5 -2\ncolor 3 4 6\nbulb -2 1 -5\n" + _FLOOR + _spheres(30, _rough_mirror))


def glass_gi():
    """Glass and gi 2: refraction and gi children wait in the pending list, single rays (M_TRACE) start next to batches."""
    def mat(i):
        if i % 3 == 0:
            return "color 0.9 0.9 1\nshininess 0.2\ntransparency 0.7\nior 1.3\nroughness 0\n"
        return "transparency 0\n" + _rough_mirror(i)
    return _scene("gi 2\n" + _TWO_SUNS + _FLOOR + _spheres(24, mat), bounces=3)


def triangles():
    """Triangles among the spheres: the exact 64-byte records by default, the wide quantised ones with qnodes = 2."""
    out = [_TWO_SUNS, _FLOOR]
    nv = 0
    for i in range(20):
        x = (i % 5 - 2) * 1.1 + 0.2 * math.sin(3.1 * i)
        y = -0.8 + (i // 5) * 0.8
        z = -5.0 + 0.7 * math.cos(2.3 * i)
        out.append("xyz %.4f %.4f %.4f\nxyz %.4f %.4f %.4f\nxyz %.4f %.4f %.4f\n" % (x - 0.5, y, z, x + 0.5, y + 0.1, z + 0.3, x, y + 0.7, z - 0.2))
        out.append("color %.2f %.2f %.2f\nshininess %.2f\nroughness %.2f\ntri %d %d %d\n" % (0.4 + 0.1 * (i % 6), 0.8 - 0.1 * (i % 4), 0.5, 0.2 + 0.1 * (i % 3),
                                                                                  0.03 * (i % 2), nv + 1, nv + 2, nv + 3))
        nv += 3
    out.append(_spheres(16, _rough_mirror, z0=-3.2, seed=5))
    return _scene("".join(out))


# (spp: 16 = the headline's resolve and RNG tables; 4 and 5 elsewhere -- 5 is no power of two)
SCENES = {"two_suns": (two_suns, 16, {}), "shininess_0": (shininess_0, 4, {}), "no_lights": (no_lights, 4, {}),
          "suns_below_the_horizon": (suns_below_the_horizon, 4, {}), "camera_under_the_plane": (camera_under_the_plane, 4, {}),
          "bounces_1": (bounces_1, 5, {}), "point_lights": (point_lights, 4, {}), "glass_gi": (glass_gi, 4, {}),
          "triangles": (triangles, 4, {}), "triangles_qnodes2": (triangles, 4, dict(qnodes=2))}


def _same(a, b, what):
    (sa, ua), (sb, ub) = a, b
    assert np.array_equal(ua, ub), what
    for k in COUNTER_KEYS:
        assert sa[k] == sb[k], (what, k, sa[k], sb[k])


@pytest.mark.parametrize("name", list(SCENES))
def test_option_sets_that_move_lanes_between_the_arms_give_the_same_frame(name):
    make, spp, scene_opts = SCENES[name]
    text = make()
    got = {k: run_case(text, W, H, spp, **scene_opts, **opts) for k, opts in OPTION_SETS.items()}
    assert got["defaults"][0]["rays"] > W * H * max(spp, 1)      # (the scene is hit, and shaded)
    for k in OPTION_SETS:
        _same(got["defaults"], got[k], (name, k))


@pytest.mark.parametrize("name", ["two_suns", "point_lights", "glass_gi"])
def test_four_waves_render_the_frame_in_many_chunks_each(name):
    """trace_waves = 4: 49 152 samples in chunks of 64 for four waves -- each wave takes ~190 chunks, so nearly all of its shade phases
    run with the queue not yet empty (the steady state), where a 1 000-wave grid on this frame is draining from its first chunk."""
    make, _, scene_opts = SCENES[name]
    text = make()
    few = run_case(text, W, H, 16, trace_waves=4, **scene_opts)
    few_batches = run_case(text, W, H, 16, trace_waves=4, refill_k=1, batch_k=64, **scene_opts)
    full = run_case(text, W, H, 16, **scene_opts)
    _same(full, few, name)
    _same(full, few_batches, name)
