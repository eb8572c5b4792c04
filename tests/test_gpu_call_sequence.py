"""State carried between render calls.  One call on a fresh scene is pinned by the parity tests; what the host side of a render
(render.hip: the steps of render_impl) can still get wrong is what a scene keeps from call to call -- the four contexts and their
argument slots, the grown workspaces, the chunk orders, the by-sample table.  So ONE scene object goes through a sequence of
differently shaped calls, and every result is compared byte for byte with the same call on a freshly built scene."""
import numpy as np
import pytest
import torch

import cuda_ray_tracer_amd as m
from cuda_ray_tracer_amd import api
from conftest import scene_path
from gpu_case import COUNTER_KEYS, gpu_render, options

pytestmark = pytest.mark.gpu

DEV = "cuda"
W, H = 48, 27


def dense(spp):
    def call(raw):
        img = torch.zeros(W * H * 4, dtype=torch.uint8, device=DEV)
        flt = torch.zeros(W * H * 4, dtype=torch.float32, device=DEV)
        m.render(img, W, H, spp, raw, d_float=flt)
        torch.cuda.synchronize()
        return [img.cpu().numpy(), flt.cpu().numpy().view(np.uint32)], None
    return call


def counted(spp):
    def call(raw):
        gu, gf, st = gpu_render(raw, W, H, spp)
        assert st["overflow_events"] == 0
        return [gu, gf.view(np.uint32)], {k: st[k] for k in COUNTER_KEYS + ("rays_traversed", "trace_launches", "node_record_bytes")}
    return call


def listed(count):
    """About 100 distinct pixels with the first and the last one, shuffled; sums, squares and counts."""
    n = W * H
    rng = np.random.default_rng(5)
    lst = np.concatenate([[0, n - 1], rng.choice(np.arange(1, n - 1), size=98, replace=False)]).astype(np.int32)
    rng.shuffle(lst)

    def call(raw):
        acc = torch.full((4 * n,), 0.25, dtype=torch.float32, device=DEV)
        asq = torch.full((4 * n,), 0.25, dtype=torch.float32, device=DEV)
        cn = torch.full((n,), 7, dtype=torch.int32, device=DEV)
        m.render_accumulate_pixels(raw, acc, W, H, 0, count, torch.as_tensor(lst, device=DEV), asq, cn, params=api.render_params(W, H, count))
        torch.cuda.synchronize()
        return [acc.cpu().numpy().view(np.uint32), asq.cpu().numpy().view(np.uint32), cn.cpu().numpy()], None
    return call


SEQUENCE = [
    ("spp 4", {}, dense(4)),
    ("spp 16 in 81 slabs", dict(slab_log2=8), dense(16)),      # 16 pixels a slab: the four argument slots come round twenty times
    ("100 listed pixels", {}, listed(4)),
    ("spp 4 with counters", {}, counted(4)),
    ("wavefront", dict(wavefront=1, wf_pool=4096), dense(4)),
    ("by chunk, measures", dict(sched=1), dense(4)),
    ("by chunk, uses", dict(sched=1), dense(4)),
] + [(f"spp 4 again {i}", {}, dense(4)) for i in range(1, 6)]      # round all four contexts; the by-sample table is measured again, then used


def build(name):
    raw = m.initRawConfigFromStl(m.parseInput(scene_path(name)), 0)
    m.build_lbvh_karas(raw)
    return raw


@pytest.mark.parametrize("name", ["spiral", "tri"])      # the quantised walk; exact records with triangles
def test_a_scene_that_has_rendered_other_shapes_renders_what_a_fresh_scene_does(name):
    shared = build(name)
    try:
        for step, opts, call in SEQUENCE:
            with options(shared, **opts):
                got, got_stats = call(shared)
            fresh = build(name)
            try:
                for k, v in opts.items():
                    fresh.set_option(k, v)
                want, want_stats = call(fresh)
                assert fresh.stats()["overflow_events"] == 0
            finally:
                fresh.close()
            assert len(got) == len(want)
            for g, w in zip(got, want):
                assert np.array_equal(g, w), (name, step, int(np.count_nonzero(g != w)))
            assert got_stats == want_stats, (name, step)
            if step == "spp 16 in 81 slabs":
                assert shared.stats()["trace_launches"] == 81
        assert shared.stats()["overflow_events"] == 0
    finally:
        shared.close()
