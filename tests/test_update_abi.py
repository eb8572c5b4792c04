"""Updates of a built scene in place (mirt_scene_get_camera / set_camera, mirt_multi_set_camera, mirt_scene_update_spheres /
update_triangles): the C ABI, the Python plumbing and the update kernels' code generation.  No compute calls are made here (no
GPU needed)."""
import ctypes as C
import os
import re
import types

import pytest

import cuda_ray_tracer_amd as m
from cuda_ray_tracer_amd import api
from cuda_ray_tracer_amd import build as B
import codegen_lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("mirt_scene_get_camera", "mirt_scene_set_camera", "mirt_multi_set_camera", "mirt_scene_update_spheres",
                "mirt_scene_update_triangles")


def _declared():
    txt = open(os.path.join(ROOT, "include", "mirt.h")).read()
    return set(re.findall(r"\b(mirt_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", txt, flags=re.S)))


def test_header_declares_and_library_exports_the_update_entry_points():
    L = m.lib()
    for s in ENTRY_POINTS:
        assert s in _declared(), s
        assert s in api.EXPORTS, s
        assert hasattr(L, s), s
    assert L.mirt_version() == 3
    assert "update.hip" in B.LIB_SOURCES
    for name in ("Camera", "update_spheres", "update_triangles"):
        assert hasattr(m, name) and name in m.__all__, name


def test_camera_layout():
    assert C.sizeof(api.Camera) == 64
    assert [(n, getattr(api.Camera, n).offset) for n, _ in api.Camera._fields_] == [
        ("eye", 0), ("forward", 12), ("right", 24), ("up", 36), ("dof_focus", 48), ("dof_lens", 52), ("fisheye", 56), ("panorama", 60)]
    hdr = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "mirt.h")).read())
    assert "typedef struct MirtCamera { MirtVec3 eye, forward, right, up; float dof_focus, dof_lens; int32_t fisheye, panorama; } MirtCamera;" in hdr


def test_null_scene_is_an_argument_error():
    L = m.lib()
    cam = api.Camera()
    assert L.mirt_scene_get_camera(None, C.byref(cam)) == 3
    assert L.mirt_scene_set_camera(None, C.byref(cam)) == 3
    assert L.mirt_multi_set_camera(None, C.byref(cam)) == 3
    assert L.mirt_scene_update_spheres(None, None, 0, 0, None) == 3
    assert L.mirt_scene_update_spheres(None, None, 0, 4, None) == 3
    assert L.mirt_scene_update_triangles(None, None, 0, 0, None) == 3
    assert L.mirt_scene_update_triangles(None, None, 0, 4, None) == 3


def test_camera_keyword_fields_override_a_copy():
    cam = api.Camera()
    cam.eye = api.Vec3(1, 2, 3)
    cam.dof_focus = 2.5
    new = api._camera_with(cam, dict(eye=(4, 5, 6), fisheye=1, up=api.Vec3(0, 0, 1)))
    assert new.eye.tolist() == [4, 5, 6] and new.fisheye == 1 and new.up.tolist() == [0, 0, 1] and new.dof_focus == 2.5
    assert cam.eye.tolist() == [1, 2, 3] and cam.fisheye == 0          # the argument is not changed
    with pytest.raises(ValueError, match="camera field"):
        api._camera_with(cam, dict(expose=1.0))


def _fake_scene():
    return types.SimpleNamespace(device=0, _h=None)


@pytest.mark.parametrize("fn,cols", [("update_spheres", 4), ("update_triangles", 9)])
def test_updates_check_their_tensor_before_calling_the_library(fn, cols):
    import torch
    raw = _fake_scene()
    f = getattr(m, fn)
    with pytest.raises(ValueError, match="torch tensor"):
        f(raw, [[0.0] * cols])
    with pytest.raises(ValueError, match="dtype"):
        f(raw, torch.zeros((4, cols), dtype=torch.float64))
    with pytest.raises(ValueError, match="dtype"):
        f(raw, torch.zeros((4, cols), dtype=torch.int32))
    with pytest.raises(ValueError, match="shape"):
        f(raw, torch.zeros((4, cols + 1), dtype=torch.float32))
    with pytest.raises(ValueError, match="shape"):
        f(raw, torch.zeros(4 * cols, dtype=torch.float32))
    with pytest.raises(ValueError, match="contiguous"):
        f(raw, torch.zeros((cols, 4), dtype=torch.float32).t())
    with pytest.raises(ValueError, match="contiguous"):
        f(raw, torch.zeros((4, 2 * cols), dtype=torch.float32)[:, ::2])
    with pytest.raises(ValueError, match="cuda"):            # right dtype and shape, but on the host
        f(raw, torch.zeros((4, cols), dtype=torch.float32))


def test_update_kernels_use_no_scratch():
    """update.hip compiled for gfx950 with the project's flags: one kernel per primitive type, neither touches scratch (no
    spills, no private arrays).  Nothing is asserted about fused multiply-adds: the expansions the compiler emits for IEEE `/` and
    sqrtf contain them, and the assembly cannot tell those from a contraction of the source -- what pins the arithmetic is the
    bit-for-bit comparison of device-computed with host-computed triangle records in test_gpu_update.py."""
    res, asm = codegen_lib._resource_usage("update.hip")
    kernels = sorted(k for k in res if "update_spheres_kernel" in k or "update_triangles_kernel" in k)
    assert len(kernels) == 2, list(res)
    for k in kernels:
        r = res[k]
        assert r["ScratchSize [bytes/lane]"] == 0, r
        assert r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0, r
        assert r["LDS Size [bytes/block]"] == 0, r
    assert not re.search(r"^\s*scratch_", asm, flags=re.M)
