"""Matte-white scenes for the direct-light query (test data, generated not stored): every material is colour 1, shininess 0,
transparency 0, roughness 0, with gi 0 and the default 4 bounces, so that a pixel of a render at spp 0 is diffuseLight of its
first hit and nothing else (include/mirt_light.h).  The lights keep colours of their own."""
import math

W, H = 40, 30      # 1200 rows: a tail in every wave and in every block of the query, whatever the number of lights

GEOMETRY = {
    "spheres": """sphere -0.9 0 -3 0.8
sphere 0.9 -0.2 -2.6 0.6
sphere 0 1.2 -3.5 0.5
sphere -0.2 -0.6 -2.1 0.25
sphere 1.7 0.9 -4 0.7
""",
    "mixed": """sphere -0.9 0 -3 0.8
sphere 0.9 -0.2 -2.6 0.6
sphere 0 1.2 -3.5 0.5
xyz -3 -1 -6
xyz 3 -1 -6
xyz 0 3 -6
tri 1 2 3
xyz -0.6 0.9 -2.2
xyz 0.5 1.0 -2.0
xyz 0.1 1.5 -2.6
tri 4 5 6
""",
}
FLOOR = "plane 0 1 0 1\nplane 0 0 1 9\n"
GEOMETRIES = ("spheres", "spheres_planes", "mixed", "mixed_planes")


def _sphere_dir(i, n):
    """Direction i of n, spread over the whole sphere (golden spiral): about half of them point below the horizon."""
    y = 1.0 - 2.0 * (i + 0.5) / n
    r = math.sqrt(max(0.0, 1.0 - y * y))
    phi = 0.7 + i * 2.399963229728653      # (the offset: no direction parallel to a coordinate plane)
    return r * math.cos(phi), y, r * math.sin(phi)


def lights(n, kind):
    """n lights from all around, each with a colour of its own.  kind: "suns", "bulbs" or "mixed" (even lights are suns; all suns
    come first in the light index)."""
    suns, bulbs = [], []
    for i in range(n):
        x, y, z = _sphere_dir(i, max(n, 2))
        c = 2.5 / max(n, 1)
        colour = "color %.4f %.4f %.4f\n" % (c * (1.0 + 0.5 * math.sin(i)), c, c * (1.0 + 0.5 * math.cos(i)))
        if kind == "suns" or (kind == "mixed" and i % 2 == 0):
            suns.append(colour + "sun %.5f %.5f %.5f\n" % (2.0 * x, 2.0 * y, 2.0 * z))      # (not of unit length: the query normalises)
        else:
            bulbs.append(colour + "bulb %.5f %.5f %.5f\n" % (3.5 * x, 3.5 * y + 0.2, 3.5 * z - 3.0))
    return "".join(suns + bulbs)


# (name, number, kind): G = 1 with nothing to do, G = 1, G = 4 with an idle lane, the sizes around 32, and the full word
LIGHT_SETS = [("none", 0, "mixed"), ("sun", 1, "suns"), ("bulb", 1, "bulbs"), ("mixed3", 3, "mixed"), ("mixed31", 31, "mixed"),
              ("mixed32", 32, "mixed"), ("mixed33", 33, "mixed"), ("mixed64", 64, "mixed"), ("suns64", 64, "suns"), ("bulbs64", 64, "bulbs")]


def scene(geometry, nlights, kind, expose=None, w=W, h=H):
    body = GEOMETRY[geometry.split("_")[0]]
    return "".join([f"png {w} {h} light.png\n", f"expose {expose}\n" if expose is not None else "", lights(nlights, kind), "color 1 1 1\n",
                    FLOOR if geometry.endswith("_planes") else "", body])
