"""The shading-branch scene matrix (test data, generated not stored): small scenes, each aimed at named branches of the shading
state machine (shade_common.h advance_core / batch_next / unlit_mask, wavefront.hip's own emission of a node's batch, the host switches of
plan_call, render_plan.h) that the bundled scenes, edge_scenes.py and the fuzzer do not reach.

Every entry of ALL is a Case: the scene text, the frame size, the oracle branch counters (oracle_lib.BRANCH_FIELDS) the scene was
built to reach -- tests/test_shade_matrix.py requires each to be >= 10 at spp 0 -- and what the product's host switches make of it
(`skip_unlit`: False where plan_call turns the unlit-light shortcut off: more than 32 lights, a non-finite colour or exposure).
`rng_free`: at spp 0 the scene draws no random number (no roughness, depth of field or gi)."""
import math
from collections import namedtuple

Case = namedtuple("Case", "text w h targets skip_unlit rng_free")

# (an odd height: no row of pixels whose rays are exactly parallel to the floor -- the float64 arbiter calls such pixels unclear;
# the even width keeps a column of rays whose x component is exactly 0)
W, H = 48, 35


def _header(w, h):
    return f"png {w} {h} shade.png\n"


def _case(body, targets=(), w=W, h=H, skip_unlit=True, rng_free=None):
    text = _header(w, h) + body
    if rng_free is None:
        rng_free = not any(l.split()[0] in ("roughness", "dof", "gi") and any(float(x) != 0 for x in l.split()[1:])
                           for l in body.split("\n") if l.split())
    return Case(text, w, h, tuple(targets), skip_unlit, rng_free)


def _sphere_dir(i, n):
    """Direction i of n, spread over the whole sphere (golden spiral): about half of them point below the horizon."""
    z = 1.0 - 2.0 * (i + 0.5) / n
    r = math.sqrt(max(0.0, 1.0 - z * z))
    phi = i * 2.399963229728653
    return r * math.cos(phi), z, r * math.sin(phi)      # (x, y, z): y is up, the first directions point upwards


# ---------------------------------------------------------------------------------------------------------------------------
# 1. lights_N: 0, 1, 31, 32, 33 and 64 lights; suns only, point lights only, both
# ---------------------------------------------------------------------------------------------------------------------------
def lights(n, kind):
    """n lights from all around: the floor plane faces away from the lower half (unlit), and answers the shadow rays that the
    spheres send downwards without a walk; the spheres shadow each other and the floor.  One reflective sphere, one rough one,
    a triangle behind them.  kind: "suns", "bulbs" or "mixed" (even lights are suns -- all suns come first in the light index)."""
    out = ["bounces 3\n"]
    for i in range(n):
        x, y, z = _sphere_dir(i, max(n, 2))
        c = 2.5 / max(n, 1)
        out.append("color %.4f %.4f %.4f\n" % (c * (1.0 + 0.5 * math.sin(i)), c, c * (1.0 + 0.5 * math.cos(i))))
        sun = kind == "suns" or (kind == "mixed" and i % 2 == 0)
        if sun:
            out.append("sun %.5f %.5f %.5f\n" % (x, y, z))
        else:
            out.append("bulb %.5f %.5f %.5f\n" % (3.5 * x, 3.5 * y + 0.2, 3.5 * z - 3.0))
    out.append("""color 0.7 0.7 0.7
plane 0 1 0 1
color 1 0.3 0.2
shininess 0.5
sphere -0.9 0 -3 0.8
shininess 0
roughness 0.2
color 0.2 0.9 0.3
sphere 0.9 -0.2 -2.6 0.6
roughness 0
color 0.3 0.4 0.9
sphere 0 1.2 -3.5 0.5
xyz -3 -1 -6
xyz 3 -1 -6
xyz 0 3 -6
color 0.9 0.9 0.2
tri 1 2 3
""")
    if n == 0:
        targets = ["diffuse_no_lights"]
    else:
        targets = (["diffuse_over_32"] if n > 32 else ["unlit_skipped"]) + (["shadow_by_plane"] if n >= 31 else [])
    return _case("".join(out), targets, skip_unlit=n <= 32)


# ---------------------------------------------------------------------------------------------------------------------------
# 2. colours and exposures that are not ordinary numbers
# ---------------------------------------------------------------------------------------------------------------------------
def _colour_scene(sphere_colour="1 0.3 0.2", sun_colour="1 1 1", expose=None):
    return (("expose %s\n" % expose) if expose is not None else "") + f"""bounces 3
color {sun_colour}
sun 1 1 0.5
color 0.5 0.5 1
sun -1 0.5 -0.3
color 1 0.8 0.6
bulb 0.5 2 -1
color 0.7 0.7 0.7
shininess 0.2
plane 0 1 0 1
color {sphere_colour}
shininess 0.4
sphere -0.8 0 -3 0.8
color 0.9 0.9 0.9
shininess 0.1
transparency 0.7
sphere 0.9 -0.2 -2.4 0.6
transparency 0
shininess 0
color 0.3 0.4 0.9
sphere 0 1.2 -3.5 0.5
"""


def inf_colour():
    return _case(_colour_scene(sphere_colour="inf 0.5 0.2"), ["refr_entered"], skip_unlit=False)


def nan_light_colour():
    return _case(_colour_scene(sun_colour="nan 1 1"), ["refr_entered"], skip_unlit=False)


def negative_colour():
    return _case(_colour_scene(sphere_colour="-0.5 0.3 1", sun_colour="1 -0.2 1"), ["unlit_skipped"])


def expose(value):
    return _case(_colour_scene(expose=value), ["unlit_skipped"])


# ---------------------------------------------------------------------------------------------------------------------------
# 3. glass
# ---------------------------------------------------------------------------------------------------------------------------
_GLASS_LIGHTS = """color 1 1 1
sun 1 1 0.5
color 1 0.8 0.6
bulb 0.5 2 -1
color 0.6 0.6 0.6
plane 0 1 0 1
"""


def _bounce_targets(bounces, extra=()):
    # bounces 1: every refraction ends in a bounce-0 final ray and every reflection ray would have bounce 0 -- the M_POP side of
    # `micro = (S.bounce == 0) ? M_POP : M_TRACE`; deeper: the M_TRACE side, and M_POP only where a chain runs out of bounces
    return ["refr_entered"] + (["refr_final_bounce0", "refl_bounce0"] if bounces == 1 else []) + list(extra)


def tir_first(bounces):
    """Glass with ior 0.5 ... 0.9: 1 / ior > 1, the first interface totally reflects at grazing angles (the `k < 0` branch of
    refractionLight, draw.cu:471-474, which no ior >= 1 can reach)."""
    body = f"bounces {bounces}\n" + _GLASS_LIGHTS + """color 0.9 0.9 1
shininess 0.2
transparency 0.8
ior 0.5
sphere -1.3 0 -3 0.7
ior 0.7
sphere 0 0 -3 0.6
ior 0.9
sphere 1.3 0 -3 0.7
ior 0.6
sphere 0 1.3 -3.5 0.5
transparency 0
shininess 0
color 0.8 0.3 0.2
sphere 0 -0.5 -5 0.5
"""
    return _case(body, _bounce_targets(bounces, ["refr_tir_first"]))


def ior_one(bounces):
    """ior 1: the refracted direction is the incoming one, k = dn^2 (exactly 1 - (1 - dn^2))."""
    body = f"bounces {bounces}\n" + _GLASS_LIGHTS + """color 0.9 1 0.9
shininess 0.2
transparency 0.8
ior 1
sphere -0.8 0 -3 0.8
sphere 0.9 0.2 -2.5 0.6
transparency 0
shininess 0
color 0.8 0.3 0.2
sphere 0 -0.3 -5 0.7
"""
    return _case(body, _bounce_targets(bounces))


def glass_plane(bounces):
    """A transparent wall (a plane) in front of the scene: the inside ray of its refraction ends on a sphere, on the floor plane
    or -- upwards -- on nothing at all (the default ObjectInfo: normal 0, ior 1.458, point 0)."""
    body = f"bounces {bounces}\n" + _GLASS_LIGHTS + """color 0.9 0.9 1
shininess 0.2
transparency 0.7
ior 1.3
plane 0 0 1 2.1
transparency 0
shininess 0
color 0.8 0.3 0.2
sphere -0.8 0 -4 0.8
color 0.2 0.8 0.3
shininess 0.3
sphere 0.9 0.2 -3.5 0.6
"""
    return _case(body, _bounce_targets(bounces, ["refr_on_plane", "refr_inside_plane", "refr_inside_miss"]))


def glass_triangle(bounces):
    """Transparent triangles: a pane in front of two spheres and a tilted one at the side."""
    body = f"bounces {bounces}\n" + _GLASS_LIGHTS + """xyz -1.5 -0.9 -2
xyz 1.5 -0.9 -2
xyz 0 1.6 -2.4
xyz 1 -0.9 -1.5
xyz 2.5 -0.9 -3
xyz 1.8 1.5 -2.5
color 0.9 0.9 1
shininess 0.2
transparency 0.7
ior 1.2
tri 1 2 3
tri 4 5 6
transparency 0
shininess 0
color 0.8 0.3 0.2
sphere -0.5 0 -4 0.8
color 0.2 0.8 0.3
shininess 0.3
sphere 0.9 0.2 -3.5 0.6
"""
    return _case(body, _bounce_targets(bounces, ["refr_on_triangle", "refr_inside_plane", "refr_inside_miss"]))


def glass_in_glass(bounces):
    """The camera inside a glass sphere that also holds a smaller glass sphere and an opaque one: every primary ray starts inside
    glass (the sphere normal flipped, `inside`), inside rays leave through the outer sphere towards the floor or nothing; a
    second point light is inside with the camera (the lights outside are shadowed by the sphere itself).  (Radius
    1.5: an inside ray starts 1e-4 under the surface, a relative margin of 2e-4 / r for the `inside` test -- above the float64
    arbiter's 1e-4 only for r < 2.)"""
    body = f"bounces {bounces}\n" + _GLASS_LIGHTS + """color 2 2 1.5
bulb 0.3 0.9 -0.5
color 0.9 1 1
shininess 0.1
transparency 0.8
ior 1.5
sphere 0 0.2 -0.6 1.5
color 1 0.9 0.9
ior 1.3
shininess 0.3
sphere 0.2 0.1 -1.3 0.35
transparency 0
shininess 0
color 0.8 0.3 0.2
sphere -0.5 0 -1.4 0.25
color 0.3 0.3 0.9
sphere 1 0 -6 1
"""
    return _case(body, _bounce_targets(bounces, ["refr_inside_miss"]))


def rgb_weights(bounces):
    """Three-value shininess / transparency with channels at exactly 0 and exactly 1: (1 - Sh) (1 - T) is 0 in two channels."""
    body = f"bounces {bounces}\n" + _GLASS_LIGHTS + """color 0.9 0.8 1
shininess 0 0.5 1
transparency 1 0.3 0
ior 1.4
sphere -0.8 0 -3 0.8
shininess 1 0 0.25
transparency 0 1 1
sphere 0.9 0.2 -2.5 0.6
shininess 0 0 0.5
transparency 0 1 0
color 0.6 0.6 0.6
plane 0 0 1 7
transparency 0
shininess 0
color 0.8 0.3 0.2
sphere 0 -0.3 -5 0.7
"""
    return _case(body, _bounce_targets(bounces, ["refr_on_plane"]))


def rough_glass(bounces):
    body = f"bounces {bounces}\n" + _GLASS_LIGHTS + """color 0.9 0.9 1
shininess 0.3
transparency 0.6
roughness 0.15
ior 1.4
sphere -0.8 0 -3 0.8
roughness 0.05
ior 0.8
sphere 0.9 0.2 -2.5 0.6
transparency 0
shininess 0
color 0.8 0.3 0.2
sphere 0 -0.3 -5 0.7
"""
    return _case(body, _bounce_targets(bounces, ["refr_tir_first"]))


# ---------------------------------------------------------------------------------------------------------------------------
# 4. gi chains, also longer than the bounce budget
# ---------------------------------------------------------------------------------------------------------------------------
def gi_chain(gi, bounces):
    body = f"bounces {bounces}\ngi {gi}\n" + _GLASS_LIGHTS + """color 1 0.3 0.2
shininess 0.4
sphere -0.9 0 -3 0.8
shininess 0.1
transparency 0.6
color 0.9 0.9 1
sphere 0.9 -0.2 -2.6 0.6
transparency 0
shininess 0
color 0.3 0.4 0.9
sphere 0 1.2 -3.5 0.5
"""
    return _case(body, ["gi_bounce0", "refr_entered"] + (["refr_final_bounce0", "refl_bounce0"] if bounces == 1 else []))


# ---------------------------------------------------------------------------------------------------------------------------
# 5. closed_box: no ray tree ends early on a miss -- the scene built to fill the pending-children list
# ---------------------------------------------------------------------------------------------------------------------------
def closed_box(bounces, gi):
    """The camera inside a large sphere with a dozen spheres in it, every material shininess 0.5 / transparency 0.5, a sun and a
    point light inside: every node of the ray tree has a reflection and a refraction child (and gi children for `gi` levels).
    (The enclosing radius is 1.8 for the same reason as glass_in_glass's 1.5.)"""
    out = [f"bounces {bounces}\n", f"gi {gi}\n" if gi else "", """color 1 1 1
sun 1 1 0.5
color 4 3 2
bulb 0.1 0.4 -0.2
shininess 0.5
transparency 0.5
ior 1.3
color 0.8 0.8 0.8
sphere 0 0 -0.6 1.8
"""]
    for i in range(12):
        x, y, z = _sphere_dir(i, 12)
        out.append("color %.2f %.2f %.2f\n" % (0.4 + 0.05 * (i % 7), 0.9 - 0.06 * (i % 5), 0.5 + 0.04 * (i % 11)))
        out.append("ior %.2f\n" % (1.1 + 0.05 * (i % 6)))
        out.append("sphere %.4f %.4f %.4f %.2f\n" % (0.9 * x, 0.9 * y, 0.9 * z - 0.6, 0.2 + 0.03 * (i % 4)))
    return _case("".join(out), ["refr_entered", "refr_final_bounce0", "refl_bounce0"] + (["gi_bounce0"] if gi else []), w=32, h=24)


# ---------------------------------------------------------------------------------------------------------------------------
# 6. planes
# ---------------------------------------------------------------------------------------------------------------------------
_PLANE_PRIMS = """color 1 0.3 0.2
shininess 0.4
sphere -0.9 0 -3 0.8
shininess 0
color 0.2 0.9 0.3
sphere 0.9 -0.2 -2.6 0.6
xyz -3 -1 -6
xyz 3 -1 -6
xyz 0 3 -6
color 0.9 0.9 0.2
tri 1 2 3
"""


def planes(n):
    """0, 1 or 8 planes.  Of the eight: two coincident floors (the first one, red, must win), a side wall parallel to the view
    axis (x = -2: the middle column of pixels has a direction whose x is exactly 0 -- t = +-inf there), a ceiling, a back wall,
    a slanted one and two behind the camera."""
    body = "bounces 3\ncolor 1 1 1\nsun 1 1 0.5\ncolor 1 0.8 0.6\nbulb 0.5 1.5 -1\n"
    if n >= 1:
        body += "color 0.9 0.1 0.1\nshininess 0.3\nplane 0 1 0 1\n"
    if n >= 8:
        body += """color 0.1 0.1 0.9
plane 0 1 0 1
color 0.5 0.5 0.5
shininess 0
plane 1 0 0 2
color 0.4 0.6 0.4
plane 0 -1 0 4
color 0.6 0.4 0.6
plane 0 0 1 9
color 0.3 0.5 0.7
shininess 0.5
plane -1 0.2 0.3 4
shininess 0
plane 0 0 -1 5
plane 1 0 1 -40
"""
    assert body.count("plane ") == n
    return _case(body + _PLANE_PRIMS, ["unlit_skipped"] + (["shadow_by_plane"] if n >= 8 else []))


def plane_tie():
    """A plane exactly tying a sphere hit, on a whole row of pixels: a panorama camera at the centre of a sphere of radius 2 (every
    hit at t = sqrtf(2 * 2) = 2) under the plane y = 2.  In the top row of the frame (spp 0) phi = -pi / 2, the direction's y is
    exactly 1 and the plane's t is 2 / 1 = 2: hitNearest takes the plane (`b.distance < p.distance` is false, draw.cu:311)."""
    body = """panorama
bounces 2
color 1 1 1
sun 0.2 -1 0.3
color 2 2 2
bulb 0.5 0.5 0.5
color 0.1 0.9 0.1
plane 0 1 0 -2
color 0.9 0.1 0.1
shininess 0.3
sphere 0 0 0 2
color 0.2 0.2 0.9
sphere 1 0 -0.5 0.3
sphere -0.8 -0.5 0.6 0.4
"""
    return _case(body, ["plane_wins_tie"])


def axis_ray_grazes_box_face():
    """Found by this matrix (the reduced scene): the central pixel of an even frame has the direction (0, 0, -1); the sphere's
    leaf box [-1.6, 0] x [-0.8, 0.8] x ... has the face x = 0 through the camera, (0 - 0) * inf is NaN and the reference's box
    test fails although the ray touches the sphere at (0, 0, -3): sqrtf(r r - d2) = 0.  A walk over the larger quantised boxes
    reaches the sphere; the product's leaf test admits the hit (t_far >> t_min, sphere_leaf_box_admits) and its vetting then walks
    the ray again literally -- the oracle's mirror has to do the same for the visit counters to agree."""
    body = """bounces 2
color 1 1 1
sun 1 1 1
color 1 0.3 0.2
shininess 0.3
sphere -0.8 0 -3 0.8
color 0.2 0.9 0.3
sphere 0.9 0.2 -2.5 0.6
color 0.3 0.4 0.9
sphere 0 1.3 -3.5 0.5
"""
    return _case(body, ["unlit_skipped"], w=48, h=36)


def _build():
    all_ = {"lights_0": lights(0, "suns")}
    for n in (1, 31, 32, 33, 64):
        for kind in ("suns", "bulbs", "mixed"):
            all_[f"lights_{n}_{kind}"] = lights(n, kind)
    all_.update(inf_colour=inf_colour(), nan_light_colour=nan_light_colour(), negative_colour=negative_colour(),
                expose_negative=expose("-1.5"), expose_zero=expose("0"), expose_tiny=expose("1e-30"))
    for fn in (tir_first, ior_one, glass_plane, glass_triangle, glass_in_glass, rgb_weights, rough_glass):
        for b in (1, 2, 5):
            all_[f"{fn.__name__}_b{b}"] = fn(b)
    for gi in (1, 3):
        for b in (1, 4):
            all_[f"gi_chain_g{gi}_b{b}"] = gi_chain(gi, b)
    for b in (1, 2, 8, 16):
        for gi in (0, 1, 3):
            all_[f"closed_box_b{b}_g{gi}"] = closed_box(b, gi)
    for n in (0, 1, 8):
        all_[f"planes_{n}"] = planes(n)
    all_["plane_tie"] = plane_tie()
    all_["axis_ray_grazes_box_face"] = axis_ray_grazes_box_face()
    return all_


ALL = _build()
