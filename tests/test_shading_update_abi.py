"""Shading values of a built scene in place (mirt_scene_set_lights / set_planes / set_shading, the material updates, their
inverses, mirt_make_plane and the mirt_multi_* setters): the C ABI, the Python plumbing, the one copy of the material-flags
rule and the material kernels' code generation.  No compute calls are made here (no GPU needed)."""
import ctypes as C
import os
import re
import shutil
import subprocess
import tempfile
import types

import numpy as np
import pytest

import cuda_ray_tracer_amd as m
from cuda_ray_tracer_amd import api, layouts
from cuda_ray_tracer_amd import build as B
import codegen_lib

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
f32 = np.float32
ENTRY_POINTS = ("mirt_scene_get_lights", "mirt_scene_set_lights", "mirt_scene_get_planes", "mirt_scene_set_planes", "mirt_make_plane",
                "mirt_scene_get_shading", "mirt_scene_set_shading", "mirt_scene_update_sphere_materials",
                "mirt_scene_update_triangle_materials", "mirt_scene_get_sphere_materials", "mirt_scene_get_triangle_materials",
                "mirt_multi_set_lights", "mirt_multi_set_planes", "mirt_multi_set_shading")


def _header():
    return open(os.path.join(ROOT, "include", "mirt.h")).read()


def test_header_declares_and_library_exports_the_entry_points():
    L = m.lib()
    declared = set(re.findall(r"\b(mirt_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)))
    for s in ENTRY_POINTS:
        assert s in declared, s
        assert s in api.EXPORTS, s
        assert hasattr(L, s), s
    assert L.mirt_version() == 3
    assert "update_shading.hip" in B.LIB_SOURCES
    for name in ("Shading", "make_plane", "update_sphere_materials", "update_triangle_materials", "get_sphere_materials", "get_triangle_materials"):
        assert hasattr(m, name) and name in m.__all__, name
    for name in ("lights", "set_lights", "planes", "set_planes", "shading", "set_shading"):
        assert hasattr(api.RawConfig, name), name
    for name in ("set_lights", "set_planes", "set_shading"):
        assert hasattr(api.MultiGpu, name), name


def test_the_header_no_longer_says_these_values_stay_fixed():
    hdr = re.sub(r"\s+", " ", _header())
    assert "lights and planes are not part of it and stay fixed" not in hdr
    assert "planes and lights do not change" not in hdr
    assert "typedef struct MirtShading { int32_t bounces, gi; float expose; } MirtShading;" in hdr
    assert "typedef struct MirtLight { MirtVec3 v; MirtRGB color; } MirtLight;" in hdr
    assert C.sizeof(api.Shading) == 12 and layouts.LIGHT.itemsize == 24


def test_null_scene_is_an_argument_error():
    L = m.lib()
    sh = api.Shading()
    buf = (C.c_char * 256)()
    calls = [lambda: L.mirt_scene_get_lights(None, buf, buf), lambda: L.mirt_scene_set_lights(None, buf, buf, None),
             lambda: L.mirt_scene_get_planes(None, 0, 1, buf), lambda: L.mirt_scene_set_planes(None, buf, 0, 1, None),
             lambda: L.mirt_scene_get_planes(None, 0, 0, None), lambda: L.mirt_scene_set_planes(None, None, 0, 0, None),
             lambda: L.mirt_scene_get_shading(None, C.byref(sh)), lambda: L.mirt_scene_set_shading(None, C.byref(sh)),
             lambda: L.mirt_scene_update_sphere_materials(None, None, 0, 0, None), lambda: L.mirt_scene_update_sphere_materials(None, buf, 0, 4, None),
             lambda: L.mirt_scene_update_triangle_materials(None, None, 0, 0, None), lambda: L.mirt_scene_update_triangle_materials(None, buf, 0, 4, None),
             lambda: L.mirt_scene_get_sphere_materials(None, 0, 0, None, None), lambda: L.mirt_scene_get_sphere_materials(None, 0, 4, buf, None),
             lambda: L.mirt_scene_get_triangle_materials(None, 0, 0, None, None), lambda: L.mirt_scene_get_triangle_materials(None, 0, 4, buf, None)]
    for k, call in enumerate(calls):
        assert call() == 3, k
        assert "null scene" in L.mirt_last_error().decode(), k
    assert L.mirt_multi_set_lights(None, buf, buf) == 3
    assert L.mirt_multi_set_planes(None, buf, 0, 1) == 3
    assert L.mirt_multi_set_shading(None, C.byref(sh)) == 3
    assert L.mirt_make_plane(None, buf, buf) == 3 and L.mirt_make_plane(buf, None, buf) == 3 and L.mirt_make_plane(buf, buf, None) == 3


PLANES = [(0, 1, 0, 1), (0, 1, 0, 0), (0, 0, 1, 2.1), (-1, 0.2, 0.3, 4), (1, 0, 1, -40), (0.3, -0.7, 0.11, -2.5), (-3, -4, -12, -13),
          (1e-3, 2e-3, -1e-3, 5e-4), (1e-7, 0, 0, 1), (1e-20, 1e-20, 1e-20, 1e-20), (1e-4, 1e-4, 1e-4, 0.5), (1e18, -1e18, 3e17, 7),
          (0, 0, 0, 1), (0.1, 0.2, 0.3, 0)]


def test_make_plane_gives_the_parsers_bits():
    """`plane a b c d` lines under a material that is not the default, parsed; mirt_make_plane of the coefficients as the parser read
    them (the record's own a, b, c, d) and the record's material must give the record: tiny coefficients (normalize answers 0 below
    1e-6), a zero normal (0 / 0: NaN point in both places), negative ones, huge ones whose squares overflow."""
    text = "png 4 4 p.png\ncolor 0.25 0.5 0.75\nshininess 0.1 0.2 0.3\ntransparency 0.4\nior 1.3\nroughness 0.05\n"
    text += "".join("plane %r %r %r %r\n" % p for p in PLANES)
    stl = m.parseText(text)
    want = stl.array("planes")
    assert len(want) == len(PLANES)
    nonzero_nor = 0
    for k, rec in enumerate(want):
        got = m.make_plane(rec["abcd"], rec["mat"])
        assert got.dtype == layouts.PLANE and got.shape == (1,)
        assert got.tobytes() == rec.tobytes(), (k, PLANES[k], got, rec)
        nonzero_nor += bool(np.any(rec["nor"] != 0))
    assert nonzero_nor >= 10
    assert np.all(np.isnan(want["point"][PLANES.index((0, 0, 0, 1))]))
    with pytest.raises(ValueError, match="shape"):
        m.make_plane([0, 1, 0], want[0]["mat"])


def _fake_scene(**desc):
    d = types.SimpleNamespace(num_suns=2, num_bulbs=1, num_planes=3, num_spheres=8, num_triangles=8)
    d.__dict__.update(desc)
    return types.SimpleNamespace(device=0, _h=None, desc=d)


@pytest.mark.parametrize("fn", ["update_sphere_materials", "update_triangle_materials", "get_sphere_materials", "get_triangle_materials"])
def test_material_calls_check_their_tensor_before_calling_the_library(fn):
    import torch
    raw = _fake_scene()
    f = getattr(m, fn)
    with pytest.raises(ValueError, match="torch tensor"):
        f(raw, [[0.0] * 11])
    with pytest.raises(ValueError, match="torch tensor"):
        f(raw, np.zeros((4, 11), f32))
    with pytest.raises(ValueError, match="dtype"):
        f(raw, torch.zeros((4, 11), dtype=torch.float64))
    with pytest.raises(ValueError, match="dtype"):
        f(raw, torch.zeros((4, 11), dtype=torch.int32))
    with pytest.raises(ValueError, match="shape"):
        f(raw, torch.zeros((4, 12), dtype=torch.float32))
    with pytest.raises(ValueError, match="shape"):
        f(raw, torch.zeros(44, dtype=torch.float32))
    with pytest.raises(ValueError, match="contiguous"):
        f(raw, torch.zeros((11, 4), dtype=torch.float32).t())
    with pytest.raises(ValueError, match="contiguous"):
        f(raw, torch.zeros((4, 22), dtype=torch.float32)[:, ::2])
    with pytest.raises(ValueError, match="cuda"):            # right dtype and shape, but on the host
        f(raw, torch.zeros((4, 11), dtype=torch.float32))


def test_light_plane_and_shading_setters_check_their_arguments_before_calling_the_library():
    raw = _fake_scene()
    set_lights = lambda **kw: api.RawConfig.set_lights(raw, **kw)      # noqa: E731
    set_planes = lambda *a, **kw: api.RawConfig.set_planes(raw, *a, **kw)      # noqa: E731
    with pytest.raises(ValueError, match="numpy array"):
        set_lights(suns=[(0, 1, 0, 1, 1, 1)] * 2)
    with pytest.raises(ValueError, match="dtype"):
        set_lights(suns=np.zeros((2, 6), f32))
    with pytest.raises(ValueError, match="dtype"):
        set_lights(bulbs=np.zeros(1, layouts.PLANE))
    with pytest.raises(ValueError, match="shape"):
        set_lights(suns=np.zeros(3, layouts.LIGHT))                 # the counts are fixed
    with pytest.raises(ValueError, match="shape"):
        set_lights(bulbs=np.zeros((1, 1), layouts.LIGHT))
    with pytest.raises(ValueError, match="contiguous"):
        set_lights(suns=np.zeros(4, layouts.LIGHT)[::2])
    with pytest.raises(ValueError, match="numpy array"):
        set_planes([1, 2, 3])
    with pytest.raises(ValueError, match="dtype"):
        set_planes(np.zeros(2, layouts.LIGHT))
    with pytest.raises(ValueError, match="shape"):
        set_planes(np.zeros((2, 1), layouts.PLANE))
    with pytest.raises(ValueError, match="contiguous"):
        set_planes(np.zeros(4, layouts.PLANE)[::2], first=1)
    multi = types.SimpleNamespace(_h=None, _keep=types.SimpleNamespace(desc=raw.desc))
    with pytest.raises(ValueError, match="shape"):
        api.MultiGpu.set_lights(multi, suns=np.zeros(5, layouts.LIGHT))
    with pytest.raises(ValueError, match="dtype"):
        api.MultiGpu.set_planes(multi, np.zeros(2, layouts.LIGHT))
    sh = api.Shading(4, 0, float("inf"))
    new = api._shading_with(sh, dict(gi=2, expose=1.5))
    assert (new.bounces, new.gi, new.expose) == (4, 2, 1.5) and (sh.gi, sh.expose) == (0, float("inf"))      # a copy
    with pytest.raises(ValueError, match="shading field"):
        api._shading_with(sh, dict(eye=(0, 0, 0)))
    with pytest.raises(ValueError, match="shading field"):
        api.MultiGpu.set_shading(multi, sh, fisheye=1)


# ---- material_flags: one copy of the rule --------------------------------------------------------------------------------------
NAN, INF = float("nan"), float("inf")
#            colour        shininess  trans            ior   roughness
EDGE_ROWS = [
    ((0, 0, 0), (0, 0, 0), (0, 0, 0), 0, 0),                                   # all zero
    ((1, 1, 1), (0, 0, 0), (-0.0, -0.0, -0.0), 1.458, -0.0),                   # -0.0f trans and roughness: neither counts
    ((1, 1, 1), (0, 0, 0), (NAN, 0, 0), 1.458, 0),                             # NaN trans: transparent
    ((1, 1, 1), (0, 0, 0), (0, 0, NAN), 1.458, 0),
    ((1, 1, 1), (0, 0, 0), (0, 0, 0), 1.458, NAN),                             # NaN roughness: not rough
    ((1, 1, 1), (0, 0, 0), (0, 0, 0), 1.458, -0.5),                            # negative roughness: not rough
    ((1, 1, 1), (0, 0, 0), (0, 0, 0), 1.458, 1e-45),                           # the smallest denormal: rough
    ((INF, 0.5, 0.2), (0, 0, 0), (0, 0, 0), 1.458, 0),                         # inf colour
    ((0.5, -INF, 0.2), (0, 0, 0), (0, 0, 0), 1.458, 0),
    ((0.5, 0.2, NAN), (0, 0, 0), (0, 0, 0), 1.458, 0),                         # NaN colour
    ((3.4028234663852886e38, 1, 1), (0, 0, 0), (0, 0, 0), 1.458, 0),           # FLT_MAX is finite
    ((1, 1, 1), (INF, NAN, 0), (0, 0, 0), NAN, 0),                             # shininess and ior are not looked at
    ((1, 1, 1), (0, 0, 0), (9.9e-7, -9.9e-7, 0), 1.458, 0),                    # below the 1e-6 threshold
    ((1, 1, 1), (0, 0, 0), (0, -1.1e-6, 0), 1.458, 0),                         # above it, negative
    ((1, 1, 1), (0, 0, 0), (1e-6, 0, 0), 1.458, 0),                            # float32(1e-6) itself: not below
    ((1, 1, 1), (0, 0, 0), (INF, 0, 0), 1.458, INF),                           # inf trans, inf roughness
    ((NAN, NAN, NAN), (0, 0, 0), (0.7, 0.7, 0.7), 1.3, 0.15),                  # all three
]


def _rows():
    return np.array([list(c) + list(s) + list(t) + [ior, rough] for c, s, t, ior, rough in EDGE_ROWS], dtype=f32)


def expected_flags(rows):
    """The three rules, stated with numpy on float32: bit 0 trans not all below 1e-6 in magnitude, bit 1 roughness > 0, bit 2 a
    colour channel not finite."""
    with np.errstate(invalid="ignore"):
        trans = ~np.all(np.abs(rows[:, 6:9]) < f32(1e-6), axis=1)
        rough = rows[:, 10] > f32(0)
        nonfinite = ~np.all(np.isfinite(rows[:, 0:3]), axis=1)
    return trans.astype(np.uint32) | rough.astype(np.uint32) << 1 | nonfinite.astype(np.uint32) << 2


def test_material_flags_header_against_the_three_rules():
    """csrc/material_flags.h compiled into tests/material_flags_probe.cpp with the host compiler under the address and undefined
    sanitizers (as tests/plan_probe.cpp is: without them only where their runtimes do not link) and run directly."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    rows = _rows()
    want = expected_flags(rows)
    assert set(want) >= {0, 1, 2, 4, 7}                                          # the table reaches every bit alone
    with tempfile.TemporaryDirectory(prefix="mirt_flags_") as tmp:      # private: /tmp is shared between users
        exe = os.path.join(tmp, "material_flags_probe")
        base = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", os.path.join(HERE, "material_flags_probe.cpp"), "-o", exe]
        if subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True).returncode != 0:
            r = subprocess.run(base, capture_output=True, text=True)      # (a toolchain without the sanitizer runtimes)
            assert r.returncode == 0, r.stderr
        text = "".join(" ".join("%08x" % w for w in row.view(np.uint32)) + "\n" for row in rows)
        r = subprocess.run([exe], input=text, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
    got = np.array([int(x) for x in r.stdout.split()], dtype=np.uint32)
    assert got.tolist() == want.tolist(), [(k, EDGE_ROWS[k]) for k in np.nonzero(got != want)[0]] if len(got) == len(want) else r.stdout


def test_there_is_one_copy_of_the_flags_rule():
    """Host (mirt_scene_create, the setters) and device (the material kernels) call material_flags; nobody restates the 1e-6 test."""
    csrc = os.path.join(ROOT, "cuda_ray_tracer_amd", "csrc")
    users = [f for f in sorted(os.listdir(csrc)) if "material_flags(" in open(os.path.join(csrc, f)).read()]
    assert users == ["api.hip", "material_flags.h", "update_shading.hip"]
    for f in ("api.hip", "update_shading.hip"):
        txt = open(os.path.join(csrc, f)).read()
        assert '#include "material_flags.h"' in txt
        assert "nonzero(" not in txt and "isfinite" not in txt, f


def test_material_kernels_use_no_scratch():
    res, asm = codegen_lib._resource_usage("update_shading.hip")
    kernels = sorted(k for k in res if any(n in k for n in ("update_materials_kernel", "material_flags_kernel", "get_materials_kernel", "reduce_flags_kernel")))
    assert len(kernels) == 4, list(res)
    for k in kernels:
        r = res[k]
        assert r["ScratchSize [bytes/lane]"] == 0, (k, r)
        assert r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0, (k, r)
        assert r["LDS Size [bytes/block]"] == (4 if "reduce_flags_kernel" in k else 0), (k, r)
    assert not re.search(r"^\s*scratch_", asm, flags=re.M)
