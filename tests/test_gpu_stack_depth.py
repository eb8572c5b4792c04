"""The trace kernel whose traversal stack never leaves LDS (render.hip, SPEC_LDS_STACK), at the edge of what it may be chosen for.

The plan (render_plan.h) picks it when D, the most internal nodes on a root-to-leaf path of the built tree, is within the capacity
of the register-plus-LDS stack: a two-child walk keeps at most D entries pending.  Three "comb" scenes of two dozen spheres put D
just below, exactly at and just above that capacity, and a ray through each of them really fills the stack to D entries, so the
scene at the capacity uses every slot the kernel has and the one above it must have been given the general kernel.

The comb: 30-bit Morton codes that share ever longer prefixes, so that every Karras split peels off one leaf.  With u one cell of
the 1023-cell code grid, a base sphere sits at (512.5, 512.5, 512.5) u and tooth k = 3 j + axis at the same point moved by 2^j u
along its axis: its code is the base's with bit k set.  A sphere G at (255.5, 255.5, 255.5) u with radius 255.5 u puts the scene
box's minimum at 0, the three j = 8 teeth (radius 254.5 u) its maximum at 1023 u; u = 2^-7, so every coordinate is exact.  The
tree is {G | {... {{base | tooth k0} | tooth k0+1} ... | tooth 26}}: D = number of spheres - 1.  The camera looks down the
diagonal from beyond the maximum corner: the ray enters every "rest" box (it holds the base sphere, nearly as large as the scene)
before the tooth's and G's box last, so the near-child-first walk descends the comb to its bottom with one sibling pending per
node: max_stack = D.  All of that is checked on the CPU, on the oracle's tree and counters, before anything is rendered."""
import os

import numpy as np
import pytest
import torch

import cuda_ray_tracer_amd as m
import oracle_lib as ol
import pyscene
from gpu_case import COUNTER_KEYS, check_against_oracle, gpu_render, mirror_flags

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, SPP = 64, 64, 4
U = 2.0 ** -7
REFERENCE_STACK = 64      # bvh_traversal.cu:8


def comb(depth):
    """The comb scene whose tree has `depth` internal nodes on its longest path: depth + 1 spheres, the teeth 27 - (depth - 1) .. 26."""
    teeth = depth - 1
    assert 3 <= teeth <= 24      # (teeth 24, 25, 26 set the scene box; tooth offsets of at least 2 cells)
    out = ["png %d %d comb.png\nbounces 3\n" % (W, H), "eye 14 14 14\nforward -1 -1 -1\nup 0 1 0\n",
           "color 1 1 1\nsun 1 2 3\ncolor 0.4 0.5 0.9\nsun 3 1 -1\n"]

    def sphere(c, r, i):
        out.append("color %.2f %.2f %.2f\nshininess %.2f\nroughness 0\n" % (0.3 + 0.1 * (i % 7), 0.9 - 0.1 * (i % 5), 0.4 + 0.05 * (i % 11), 0.2 + 0.1 * (i % 4)))
        out.append("sphere %.10g %.10g %.10g %.10g\n" % (c[0] * U, c[1] * U, c[2] * U, r * U))
    sphere((255.5, 255.5, 255.5), 255.5, 0)
    sphere((512.5, 512.5, 512.5), 508.0, 1)
    for k in range(27 - teeth, 27):
        c = [512.5, 512.5, 512.5]
        c[k % 3] += float(1 << (k // 3))
        sphere(c, 254.5 if k >= 24 else 200.0 + k, 2 + k)
    return "".join(out)


def tree_depth(nodes, n):
    """Most internal nodes on a root-to-leaf path: the reference's numbering, internal nodes [0, n - 2], leaves [n - 1, 2 n - 2]."""
    best, todo = 0, [(0, 1)]
    while todo:
        i, d = todo.pop()
        best = max(best, d)
        todo += [(int(c), d + 1) for c in (nodes["left"][i], nodes["right"][i]) if c < n - 1]
    return best


class Rendered:
    """A scene rendered with counters by the product, under `options`: bytes, float image, stats and the stack facts; and by the
    oracle under the flags that mirror the default options (computed once per scene text and kept)."""
    _oracle = {}

    def __init__(self, text, w, h, spp, **options):
        stl = m.parseText(text)
        raw = m.initRawConfigFromStl(stl, 0)
        for k, v in options.items():
            raw.set_option(k, v)
        m.build_lbvh_karas(raw)
        self.u8, self.f32, self.stats = gpu_render(raw, w, h, spp)
        self.info = raw.stack_info()
        self.tree = raw.tree()
        raw.close()
        key = (text, w, h, spp)
        if key not in Rendered._oracle:
            o = ol.OracleScene(pyscene.parse_lines(text.split("\n")), bounds_mode=0)
            nodes = o.nodes()
            ref = o.render(w, h, spp, flags=mirror_flags(stl, o), nthreads=8)
            Rendered._oracle[key] = (ref, nodes, tree_depth(nodes, o.n) if o.n > 1 else 0)
            o.close()
        self.ref, self.oracle_nodes, self.oracle_depth = Rendered._oracle[key]

    def check(self):
        for f in ("left", "right"):
            assert np.array_equal(self.tree[0][f], self.oracle_nodes[f]), f
        check_against_oracle(self.f32, self.u8, self.stats, self.ref)


def same(a, b, what):
    assert np.array_equal(a.u8, b.u8), what
    for k in COUNTER_KEYS:
        assert a.stats[k] == b.stats[k], (what, k, a.stats[k], b.stats[k])


def capacity():
    stl = m.parseText(comb(8))
    raw = m.initRawConfigFromStl(stl, 0)
    cap = raw.stack_info()["lds_capacity"]
    assert raw.stack_info()["tree_depth"] == -1      # (nothing built yet)
    raw.close()
    return cap


@pytest.mark.parametrize("over", [-1, 0, 1])
def test_comb_scenes_around_the_capacity(over):
    cap = capacity()
    depth = cap + over
    text = comb(depth)
    # on the CPU first: the oracle's tree is the comb, its walk fills the stack to D entries, within the reference's own stack
    o = ol.OracleScene(pyscene.parse_lines(text.split("\n")), bounds_mode=0)
    assert tree_depth(o.nodes(), o.n) == depth and depth < REFERENCE_STACK
    o.close()
    r = Rendered(text, W, H, SPP)
    assert r.ref["stats"]["max_stack"] == depth
    assert r.info["tree_depth"] == r.oracle_depth == depth
    assert r.info["lds_only"] == (depth <= cap)
    r.check()      # pixels, and every counter of COUNTER_KEYS -- max_stack among them -- equal to the oracle's


def test_the_spill_path_forced_on_the_first_comb_gives_the_same_frame():
    text = comb(capacity() - 1)
    default = Rendered(text, W, H, SPP)
    forced = Rendered(text, W, H, SPP, stack_lds_depth=2)
    assert default.info["lds_only"] and not forced.info["lds_only"]
    assert forced.stats["max_stack"] > 2 + 1      # (the forced frame did spill)
    forced.check()
    same(default, forced, "stack_lds_depth = 2")


def test_tenthousand_selects_the_lds_only_kernel_and_renders_what_the_general_one_does():
    with open(os.path.join(ROOT, "scenes", "tenthousand.txt")) as f:
        text = f.read()
    default = Rendered(text, 96, 54, 16)
    cap = default.info["lds_capacity"]
    general = Rendered(text, 96, 54, 16, stack_lds_depth=cap)      # the compiled size, said explicitly: the general kernel
    assert default.info["lds_only"] and not general.info["lds_only"]
    assert 0 < default.info["tree_depth"] <= cap and default.stats["max_stack"] <= default.info["tree_depth"]
    default.check()
    same(default, general, "stack_lds_depth = capacity")
    assert torch.cuda.is_available()
