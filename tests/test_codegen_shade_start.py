"""The kernel the headline scene runs -- trace_kernel<false, 8, true, 31> -- with one ray start per shade pass (render.hip,
ONE_START; shade_common.h, batch_setup / advance_setup), compiled to gfx950 assembly, no GPU needed (tools/hotloop).  The shade
phase lost two copies of start_ray; the traversal loop, whose source did not change, may not pay for that: no spill instruction
in it, and no more vector or branch instructions than on the commit before.

The commit before, measured with

    python tools/hotloop.py trace_kernelILb0ELi8ELb1ELi31EE        (the loop: 376 valu, 213 salu, 31 branch; 127 VGPRs, 4 waves)
    whole_body_valu(hotloop._compile(())[1], KERNEL)  (below)       (the kernel: 3843)

With the change: 371 / 211 / 31 in the loop, 3653 in the kernel."""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

KERNEL = "trace_kernelILb0ELi8ELb1ELi31EE"
PARENT_LOOP_VALU, PARENT_LOOP_BRANCHES = 376, 31
PARENT_BODY_VALU = 3843


def whole_body_valu(asm, kernel):
    """Instructions of `kernel`, label to s_endpgm, whose opcode starts with v_."""
    n, inside = 0, False
    for l in asm.splitlines():
        if re.match(r"^_ZN4mirt.*" + kernel + r".*:", l):
            inside = True
            continue
        if inside and "s_endpgm" in l:
            break
        if inside and l.strip().startswith("v_"):
            n += 1
    assert inside
    return n


def _loop():
    import hotloop
    return hotloop.analyze(kernel=KERNEL)


def test_no_spill_instruction_in_the_traversal_loop():
    _, cnt, listed = _loop()
    assert cnt.get("lds", 0) >= 4 and cnt.get("valu", 0) > 100, cnt      # (the loop was found)
    assert cnt.get("scratch", 0) == 0 and cnt.get("sgpr-spill", 0) == 0 and listed == [], (cnt, listed)


def test_the_traversal_loop_has_no_more_vector_and_branch_instructions_than_the_parents():
    _, cnt, _ = _loop()
    print("traversal loop:", cnt)
    assert cnt["valu"] <= PARENT_LOOP_VALU, cnt
    assert cnt["branch"] <= PARENT_LOOP_BRANCHES, cnt


def test_four_waves_per_simd_within_128_registers():
    res, _, _ = _loop()
    facts = {k.strip(): v.strip() for k, v in (r.split(":", 1) for r in res)}
    assert int(facts["VGPRs"]) <= 128 and facts["Occupancy [waves/SIMD]"] == "4", res


def test_the_kernel_has_fewer_vector_instructions_than_the_parents():
    import hotloop
    _, asm = hotloop._compile(())
    n = whole_body_valu(asm, KERNEL)
    print("whole kernel, v_*:", n)
    assert 1000 < n < PARENT_BODY_VALU, n
