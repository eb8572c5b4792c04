"""Ray queries (mirt_trace_rays / mirt_camera_rays): the C ABI, the Python plumbing and the query kernel's code generation.
No compute calls are made here (no GPU needed)."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest

import cuda_ray_tracer_amd as m
from cuda_ray_tracer_amd import api
from codegen_lib import _kernel_body, _resource_usage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    txt = open(os.path.join(ROOT, "include", "mirt.h")).read()
    return set(re.findall(r"\b(mirt_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", txt, flags=re.S)))


def test_header_declares_and_library_exports_the_query_entry_points():
    L = m.lib()
    for s in ("mirt_trace_rays", "mirt_camera_rays"):
        assert s in _declared(), s
        assert s in api.EXPORTS, s
        assert hasattr(L, s), s
    assert L.mirt_version() == 3


def test_ray_and_hit_layout():
    assert C.sizeof(api.Ray) == 32
    assert [(n, getattr(api.Ray, n).offset) for n, _ in api.Ray._fields_] == [("o", 0), ("tmax", 12), ("d", 16), ("pad", 28)]
    assert C.sizeof(api.Hit) == 24
    assert [(n, getattr(api.Hit, n).offset) for n, _ in api.Hit._fields_] == [("t", 0), ("kind", 4), ("id", 8), ("n", 12)]
    hdr = open(os.path.join(ROOT, "include", "mirt.h")).read()
    for name, v in (("MIRT_HIT_NONE", 0), ("MIRT_HIT_SPHERE", 1), ("MIRT_HIT_TRIANGLE", 2), ("MIRT_HIT_PLANE", 3)):
        assert re.search(r"#define %s %d\b" % (name, v), hdr), name
        assert getattr(api, name) == v
    assert re.search(r"#define MIRT_QUERY_ANY_HIT 1u\b", hdr) and api.MIRT_QUERY_ANY_HIT == 1


def test_hit_record_is_the_primary_hit_record_of_the_test_side():
    import oracle_lib
    dt = oracle_lib.HIT
    assert dt.itemsize == C.sizeof(api.Hit)
    assert dt.fields["t"][1] == api.Hit.t.offset
    assert dt.fields["kind"][1] == api.Hit.kind.offset
    assert dt.fields["id"][1] == api.Hit.id.offset
    assert dt.fields["n"][1] == api.Hit.n.offset


def test_null_scene_is_an_argument_error():
    L = m.lib()
    assert L.mirt_trace_rays(None, None, 0, None, 0, None) == 3
    assert L.mirt_trace_rays(None, None, 5, None, 1, None) == 3
    p = api.render_params(8, 8, 0)
    assert L.mirt_camera_rays(None, C.byref(p), None, None) == 3


def _fake_scene():
    return types.SimpleNamespace(device=0, _h=None)


def test_trace_rays_checks_its_tensors_before_calling_the_library():
    import torch
    raw = _fake_scene()
    good_r, good_h = torch.zeros((4, 8), dtype=torch.float32), torch.zeros((4, 6), dtype=torch.int32)
    with pytest.raises(ValueError, match="dtype"):
        m.trace_rays(raw, torch.zeros((4, 8), dtype=torch.float64), good_h)
    with pytest.raises(ValueError, match="dtype"):
        m.trace_rays(raw, good_r, torch.zeros((4, 6), dtype=torch.int16))
    with pytest.raises(ValueError, match="shape"):
        m.trace_rays(raw, torch.zeros((4, 7), dtype=torch.float32), good_h)
    with pytest.raises(ValueError, match="shape"):
        m.trace_rays(raw, good_r, torch.zeros((5, 6), dtype=torch.int32))
    with pytest.raises(ValueError, match="shape"):
        m.trace_rays(raw, torch.zeros(32, dtype=torch.float32), good_h)
    with pytest.raises(ValueError, match="contiguous"):
        m.trace_rays(raw, torch.zeros((8, 4), dtype=torch.float32).t(), good_h)
    with pytest.raises(ValueError, match="contiguous"):
        m.trace_rays(raw, good_r, torch.zeros((4, 12), dtype=torch.int32)[:, ::2])
    with pytest.raises(ValueError, match="cuda"):            # right dtype and shape, but on the host
        m.trace_rays(raw, good_r, good_h)
    with pytest.raises(ValueError, match="dtype"):
        m.camera_rays(raw, torch.zeros((64, 8), dtype=torch.float16), 8, 8, 0)
    with pytest.raises(ValueError, match="shape"):
        m.camera_rays(raw, torch.zeros((63, 8), dtype=torch.float32), 8, 8, 0)


def test_pack_rays_and_unpack_hits_round_trip():
    import torch
    g = torch.Generator().manual_seed(3)
    o = torch.rand((17, 3), generator=g)
    d = torch.rand((17, 3), generator=g) - 0.5
    tmax = torch.rand(17, generator=g) * 10
    r = m.pack_rays(o, d, tmax)
    assert r.shape == (17, 8) and r.dtype == torch.float32 and r.is_contiguous()
    assert torch.equal(r[:, 0:3], o) and torch.equal(r[:, 3], tmax) and torch.equal(r[:, 4:7], d) and torch.all(r[:, 7] == 0)
    # one origin for all rays, default tmax
    r1 = m.pack_rays(torch.tensor([1.0, 2.0, 3.0]), d)
    assert torch.all(r1[:, 0:3] == torch.tensor([1.0, 2.0, 3.0])) and torch.all(torch.isinf(r1[:, 3]))
    # the row layout is MirtRay's
    row = api.Ray.from_buffer_copy(r[5].numpy().tobytes())
    assert row.tmax == r[5, 3].item() and row.d.y == r[5, 5].item()

    rec = np.zeros(17, dtype=[("t", "<f4"), ("kind", "<u4"), ("id", "<u4"), ("n", "<f4", 3)])
    rec["t"] = np.arange(17, dtype=np.float32) * 0.5 - 1
    rec["kind"] = np.arange(17) % 4
    rec["id"] = np.arange(17) * 7
    rec["n"] = np.arange(51, dtype=np.float32).reshape(17, 3)
    hits = torch.from_numpy(rec.view(np.int32).reshape(17, 6).copy())
    t, kind, pid, n = m.unpack_hits(hits)
    assert np.array_equal(t.numpy(), rec["t"]) and np.array_equal(kind.numpy(), rec["kind"].astype(np.int32))
    assert np.array_equal(pid.numpy(), rec["id"].astype(np.int32)) and np.array_equal(n.numpy(), rec["n"])
    t[0] = 42.0                                               # views, not copies
    assert hits.view(torch.float32)[0, 0].item() == 42.0
    h = api.Hit.from_buffer_copy(hits[3].numpy().tobytes())
    assert (h.t, h.kind, h.id, h.n.z) == (rec["t"][3], rec["kind"][3], rec["id"][3], rec["n"][3][2])


def test_query_kernel_codegen_runs_8_waves_per_simd_with_scratch_only_on_the_spill_path():
    """query.hip compiled for gfx950: both trace kernels at <= 64 VGPRs (8 waves per SIMD), a 20-entry LDS stack per lane of a
    256-thread block, no register spills, and exactly one scratch store per kernel: the push of a stack entry beyond the LDS
    part (the designed spill path into the lane's private array)."""
    res, asm = _resource_usage("query.hip")
    kernels = [k for k in res if "trace_rays_kernel" in k]
    assert len(kernels) == 2, list(res)
    for k in kernels:
        r = res[k]
        assert r["Occupancy [waves/SIMD]"] == 8, r
        assert r["VGPRs"] <= 64, r
        assert r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0, r
        assert r["LDS Size [bytes/block]"] == 20 * 256 * 4, r
        body = _kernel_body(asm, k)
        stores = [t for t in body if t.startswith("scratch_store")]
        assert len(stores) == 1, stores
