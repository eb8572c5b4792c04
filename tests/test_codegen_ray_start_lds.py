"""The kernel the headline scene runs -- trace_kernel<false, 8, true, 31>: the LDS-only sphere-only kernel whose loop header
starts rays from values kept in LDS (render.hip, SPEC_START_LDS) -- compiled to gfx950 assembly, no GPU needed
(tools/hotloop.analyze).  What trace_kernel<false, 8, true, 15> promises (test_codegen_lds_stack.py) holds for it too: no scratch
instruction, no SGPR-spill instruction and no global store in the traversal loop, 128 VGPRs at 4 waves per SIMD.  On top of that:
at most 10 240 bytes of LDS (16 waves per compute unit), and the loop header's ray start -- from the read of its LDS block to the
plane loop's scalar loads -- issues no vector-memory load."""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

KERNEL = "trace_kernelILb0ELi8ELb1ELi31EE"
STORES = ("global_store", "flat_store", "buffer_store", "global_atomic", "flat_atomic", "buffer_atomic")
LOADS = ("global_load", "flat_load", "buffer_load", "ds_read", "s_load", "v_readfirstlane")


def _loop():
    import hotloop
    res, cnt, listed = hotloop.analyze(kernel=KERNEL, also=STORES + LOADS)
    assert cnt.get("lds", 0) >= 4 and cnt.get("valu", 0) > 100, cnt      # (the loop was found)
    return res, cnt, listed


def test_no_scratch_sgpr_spill_or_global_store_in_the_traversal_loop():
    _, cnt, listed = _loop()
    ops = [t for _, t in listed]
    assert [t for t in ops if t.startswith("scratch_")] == [] and cnt.get("scratch", 0) == 0, (cnt, ops)
    assert [t for t in ops if t.startswith(("v_readlane", "v_writelane"))] == [] and cnt.get("sgpr-spill", 0) == 0, (cnt, ops)
    assert [t for t in ops if t.startswith(STORES)] == [], ops


def test_128_vgprs_at_four_waves_per_simd():
    res, _, _ = _loop()
    facts = {k.strip(): v.strip() for k, v in (r.split(":", 1) for r in res)}
    assert 96 < int(facts["VGPRs"]) <= 128 and facts["Occupancy [waves/SIMD]"] == "4", res


def test_lds_within_a_sixteenth_of_the_compute_unit():
    import hotloop
    remarks, _ = hotloop._compile(())
    sizes = re.findall(r"Function Name: \S*" + KERNEL + r"\S*.*?LDS Size \[bytes/block\]: (\d+)", remarks, re.S)
    assert sizes and all(int(s) <= 10240 for s in sizes), sizes


def test_the_header_ray_start_issues_no_vector_memory_load():
    """In the loop, in program order: the ds_read_b128 of the LDS block's head -- the one whose words go to scalar registers right
    away (v_readfirstlane) -- opens the arm; the plane loop's scalar loads come after it.  Between the two there is no global,
    flat or buffer load: the sun record is an LDS read.  And the loop has no flat load at all: the node and sphere records are
    global loads."""
    _, _, listed = _loop()
    ops = [t for _, t in listed]
    head = [i for i in range(len(ops) - 1) if ops[i].startswith("ds_read_b128") and ops[i + 1].startswith("v_readfirstlane")]
    assert len(head) == 1, ops
    planes = [i for i, t in enumerate(ops) if t.startswith("s_load") and i > head[0]]
    assert planes, ops
    between = ops[head[0] + 1:planes[0]]
    assert [t for t in between if t.startswith(("global_load", "flat_load", "buffer_load"))] == [], between
    assert [t for t in between if t.startswith("ds_read")] != [], between      # (the lane's sun record)
    assert [t for t in ops if t.startswith("flat_load")] == [], ops
