"""The trace kernel the headline scene runs -- trace_kernel<false, 8, true, 15>: the sphere-only specialisation with the stack
that never leaves LDS (render.hip, SPEC_LDS_STACK) -- compiled to gfx950 assembly, no GPU needed (tools/hotloop.analyze).  Its
traversal loop (the loop header with its batch_next arm, and the step loop) must hold no scratch instruction, no SGPR-spill
instruction and no global store, and the kernel must keep its 128 VGPRs at 4 waves per SIMD.

The general kernel, ...Li7EE, has two global stores there (the spill arm of its two pushes) and 13 v_readlane_b32, all in the
header's batch_next arm.  Without the spill arm alone 12 of them stay: the light array's address, the root reference and four
loop-invariant conditions of start_ray that 106 scalar registers do not hold across the loop.  They went when the arm began to
read what it only looks at, and that address, through the shade phase's opaque pointer, and the step count was made opaque per
pass (DESIGN.md section 4 has the timings of each form)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

KERNEL = "trace_kernelILb0ELi8ELb1ELi15EE"
STORES = ("global_store", "flat_store", "buffer_store", "global_atomic", "flat_atomic", "buffer_atomic")


def _loop():
    import hotloop
    res, cnt, listed = hotloop.analyze(kernel=KERNEL, also=STORES)
    assert cnt.get("lds", 0) >= 4 and cnt.get("valu", 0) > 100, cnt      # (the loop was found: two pushes and two pops -- one step is peeled)
    return res, cnt, [t for _, t in listed]


def test_no_scratch_instruction_in_the_traversal_loop():
    _, cnt, listed = _loop()
    assert [t for t in listed if t.startswith("scratch_")] == [] and cnt.get("scratch", 0) == 0, (cnt, listed)


def test_no_sgpr_spill_instruction_in_the_traversal_loop():
    _, cnt, listed = _loop()
    assert [t for t in listed if t.startswith(("v_readlane", "v_writelane"))] == [] and cnt.get("sgpr-spill", 0) == 0, (cnt, listed)


def test_no_global_store_in_the_traversal_loop():
    _, _, listed = _loop()
    assert [t for t in listed if t.startswith(STORES)] == [], listed


def test_128_vgprs_at_four_waves_per_simd():
    res, _, _ = _loop()
    facts = dict(r.split(":", 1) for r in res)
    assert facts["VGPRs"].strip() == "128" and facts["Occupancy [waves/SIMD]"].strip() == "4", res
