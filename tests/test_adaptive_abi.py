"""Adaptive sampling (mirt_render_accumulate_pixels / mirt_select_pixels / mirt_finalize_counts): the C ABI, the Python plumbing
and the command line's usage check.  No compute calls are made here (no GPU needed)."""
import ctypes as C
import os
import re
import subprocess
import types

import pytest

import cuda_ray_tracer_amd as m
from cuda_ray_tracer_amd import api
from conftest import scene_path

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "cuda_ray_tracer_amd", "_build", "raytracer")
SYMBOLS = ("mirt_render_accumulate_pixels", "mirt_select_pixels", "mirt_finalize_counts")


def _declared():
    txt = open(os.path.join(ROOT, "include", "mirt.h")).read()
    return set(re.findall(r"\b(mirt_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", txt, flags=re.S)))


def test_header_declares_and_library_exports_the_adaptive_entry_points():
    L = m.lib()
    for s in SYMBOLS:
        assert s in _declared(), s
        assert s in api.EXPORTS, s
        assert hasattr(L, s), s
    assert L.mirt_version() == 3
    for f in ("render_accumulate_pixels", "select_pixels", "finalize_counts", "render_adaptive"):
        assert f in m.__all__ and callable(getattr(m, f))


def test_null_and_out_of_range_arguments_are_argument_errors():
    """Everything the host can check without a device: null pointers, the bounds on min_samples / max_samples."""
    L = m.lib()
    p = api.render_params(8, 8, 4)
    one = (C.c_uint32 * 4)()
    assert L.mirt_render_accumulate_pixels(None, C.byref(p), None, 0, one, None, None, 0, 4, None) == 3
    assert L.mirt_select_pixels(None, one, one, one, 2, 8, 0.1, one, one, None) == 3
    assert L.mirt_select_pixels(C.byref(p), None, one, one, 2, 8, 0.1, one, one, None) == 3
    assert L.mirt_select_pixels(C.byref(p), one, one, one, 2, 8, 0.1, one, None, None) == 3
    assert L.mirt_select_pixels(C.byref(p), one, one, one, 1, 8, 0.1, one, one, None) == 3      # min_samples < 2
    assert L.mirt_select_pixels(C.byref(p), one, one, one, 4, 3, 0.1, one, one, None) == 3      # max_samples < min_samples
    assert b"min_samples" in L.mirt_last_error()
    assert L.mirt_finalize_counts(None, one, one, one, None) == 3
    assert L.mirt_finalize_counts(C.byref(p), one, None, one, None) == 3


def _fake_scene():
    return types.SimpleNamespace(device=0, _h=None)


def test_render_accumulate_pixels_checks_its_tensors_before_calling_the_library():
    import torch
    raw = _fake_scene()
    n = 8 * 8
    acc, cnt, lst = torch.zeros(4 * n), torch.zeros(n, dtype=torch.int32), torch.zeros(5, dtype=torch.int32)
    with pytest.raises(ValueError, match="dtype"):
        m.render_accumulate_pixels(raw, torch.zeros(4 * n, dtype=torch.float64), 8, 8, 0, 4, lst)
    with pytest.raises(ValueError, match="shape"):
        m.render_accumulate_pixels(raw, torch.zeros(4 * n - 4), 8, 8, 0, 4, lst)
    with pytest.raises(ValueError, match="contiguous"):
        m.render_accumulate_pixels(raw, torch.zeros(8 * n)[::2], 8, 8, 0, 4, lst)
    with pytest.raises(ValueError, match="cuda"):            # right dtype and shape, but on the host
        m.render_accumulate_pixels(raw, acc, 8, 8, 0, 4, lst)
    with pytest.raises(ValueError, match="torch tensor"):
        m.render_accumulate_pixels(raw, [0.0] * (4 * n), 8, 8, 0, 4, lst)
    if not torch.cuda.is_available():
        return
    dacc, dcnt, dlst = acc.cuda(), cnt.cuda(), lst.cuda()
    with pytest.raises(ValueError, match="dtype"):
        m.render_accumulate_pixels(raw, dacc, 8, 8, 0, 4, dlst.to(torch.int64))
    with pytest.raises(ValueError, match="shape"):
        m.render_accumulate_pixels(raw, dacc, 8, 8, 0, 4, dlst.reshape(5, 1))
    with pytest.raises(ValueError, match="contiguous"):
        m.render_accumulate_pixels(raw, dacc, 8, 8, 0, 4, torch.zeros(10, dtype=torch.int32, device="cuda")[::2])
    with pytest.raises(ValueError, match="cuda"):
        m.render_accumulate_pixels(raw, dacc, 8, 8, 0, 4, lst)
    with pytest.raises(ValueError, match="dtype"):
        m.render_accumulate_pixels(raw, dacc, 8, 8, 0, 4, dlst, d_accum_sq=dacc.double())
    with pytest.raises(ValueError, match="shape"):
        m.render_accumulate_pixels(raw, dacc, 8, 8, 0, 4, dlst, d_counts=dcnt[:-1])
    with pytest.raises(ValueError, match="dtype"):
        m.render_accumulate_pixels(raw, dacc, 8, 8, 0, 4, dlst, d_counts=dcnt.float())
    with pytest.raises(ValueError, match="cuda"):
        m.render_accumulate_pixels(raw, dacc, 8, 8, 0, 4, dlst, d_counts=cnt)


def test_select_pixels_and_finalize_counts_check_their_tensors_before_calling_the_library():
    import torch
    n = 8 * 8
    acc, cnt, out, num = torch.zeros(4 * n), torch.zeros(n, dtype=torch.int32), torch.zeros(n, dtype=torch.int32), torch.zeros(1, dtype=torch.int32)
    img = torch.zeros(4 * n, dtype=torch.uint8)
    with pytest.raises(ValueError, match="dtype"):
        m.select_pixels(acc.double(), acc, cnt, 8, 8, 2, 8, 0.1, out, num)
    with pytest.raises(ValueError, match="dtype"):
        m.select_pixels(acc, acc, cnt.to(torch.int64), 8, 8, 2, 8, 0.1, out, num)
    with pytest.raises(ValueError, match="shape"):
        m.select_pixels(acc, acc[:-4], cnt, 8, 8, 2, 8, 0.1, out, num)
    with pytest.raises(ValueError, match="shape"):
        m.select_pixels(acc, acc, cnt, 8, 8, 2, 8, 0.1, out[:-1], num)      # capacity: one entry per pixel
    with pytest.raises(ValueError, match="shape"):
        m.select_pixels(acc, acc, cnt, 8, 8, 2, 8, 0.1, out, torch.zeros(2, dtype=torch.int32))
    with pytest.raises(ValueError, match="contiguous"):
        m.select_pixels(acc, acc, torch.zeros(2 * n, dtype=torch.int32)[::2], 8, 8, 2, 8, 0.1, out, num)
    with pytest.raises(ValueError, match="cuda"):
        m.select_pixels(acc, acc, cnt, 8, 8, 2, 8, 0.1, out, num)
    with pytest.raises(ValueError, match="dtype"):
        m.finalize_counts(img.to(torch.int8), acc, cnt, 8, 8)
    with pytest.raises(ValueError, match="shape"):
        m.finalize_counts(img, acc, cnt[:-1], 8, 8)
    with pytest.raises(ValueError, match="contiguous"):
        m.finalize_counts(img, torch.zeros(8 * n)[::2], cnt, 8, 8)
    with pytest.raises(ValueError, match="cuda"):
        m.finalize_counts(img, acc, cnt, 8, 8)
    with pytest.raises(ValueError, match="min_spp"):
        m.render_adaptive(_fake_scene(), 8, 8, 1, 8, 4, 0.1)
    with pytest.raises(ValueError, match="min_spp"):
        m.render_adaptive(_fake_scene(), 8, 8, 4, 3, 4, 0.1)


def test_cli_refuses_adaptive_on_several_gpus_before_it_touches_a_device(tmp_path):
    r = subprocess.run([CLI, scene_path("tri"), "--adaptive", "0.001", "--gpus", "2"], cwd=tmp_path, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                       timeout=300)
    assert r.returncode == 2 and "--adaptive" in r.stderr and "--gpus" in r.stderr
    r = subprocess.run([CLI, scene_path("tri"), "--adaptive", "0.001", "--min-spp", "1"], cwd=tmp_path, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                       timeout=300)
    assert r.returncode == 2 and "--min-spp" in r.stderr
    assert not list(tmp_path.iterdir())
