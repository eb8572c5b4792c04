"""The step loop of the kernel the headline scene runs -- trace_kernel<false, 8, true, 31> -- compiled to gfx950 assembly, no GPU
needed (tools/hotloop).  The steps after the peeled first one are the innermost loop of the traversal loop, the one that pushes
onto the LDS stack.  With "not traversing" read off the current reference (render.hip, CUR_MARK) instead of the lane's flag, a
step has no byte to move, select, mask and compare, and one exec region -- "at an internal node" -- where the flag needed two
("traversing", then "not at a leaf").

PARENT_STEP_VALU: what step_loop() below counts on the commit before the change (56 vector-ALU instructions; 49 with it)."""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

KERNEL = "trace_kernelILb0ELi8ELb1ELi31EE"
PARENT_STEP_VALU = 56
STORES = ("global_store", "flat_store", "buffer_store", "global_atomic", "flat_atomic", "buffer_atomic")


def step_loop(asm, kernel):
    """The instructions of the depth-3 loop of `kernel` that holds a ds_write_b32, in program order."""
    body, inside = [], False
    for l in asm.splitlines():
        if re.match(r"^_ZN4mirt.*" + kernel + r".*:", l):
            inside = True
            continue
        if inside and "s_endpgm" in l:
            break
        if inside:
            body.append(l)
    loops, cur = {}, None
    for i, l in enumerate(body):
        m = re.match(r"^\.L(BB\d+_\d+):", l)
        if m:
            # the block's comment lines say which loop it belongs to
            j, text = i, l
            while j + 1 < len(body) and body[j + 1].strip().startswith(";"):
                j += 1
                text += "\n" + body[j]
            inner = re.search(r"Header=(BB\d+_\d+) Depth=3", text)
            cur = m.group(1) if "Inner Loop Header: Depth=3" in text else (inner.group(1) if inner else None)
            continue
        t = l.strip()
        if cur and t and not t.startswith((";", ".")):
            loops.setdefault(cur, []).append(t.split(";")[0].strip())
    found = [ins for ins in loops.values() if any(t.startswith("ds_write_b32") for t in ins)]
    assert len(found) == 1, sorted(loops)
    return found[0]


def _step():
    import hotloop
    _, asm = hotloop._compile(())
    return step_loop(asm, KERNEL)


def test_a_step_has_at_least_five_vector_instructions_fewer_than_the_parents():
    ins = _step()
    valu = [t for t in ins if t.startswith("v_")]
    assert 20 < len(valu) <= PARENT_STEP_VALU - 5, (len(valu), ins)


def test_one_exec_region_ahead_of_the_node_record_loads():
    ins = _step()
    loads = [i for i, t in enumerate(ins) if t.startswith("global_load_dwordx4")]
    assert len(loads) == 2, ins
    ahead = [t for t in ins[:loads[0]] if t.startswith("s_and_saveexec_b64")]
    assert len(ahead) == 1, ins[:loads[0]]


def test_the_traversal_loop_keeps_its_promises():
    """No scratch, no SGPR-spill instruction, no global store in the whole traversal loop; at most 128 VGPRs at 4 waves per SIMD;
    at most 10 240 bytes of LDS."""
    import hotloop
    res, cnt, listed = hotloop.analyze(kernel=KERNEL, also=STORES)
    assert cnt.get("lds", 0) >= 4 and cnt.get("valu", 0) > 100, cnt      # (the loop was found)
    assert cnt.get("scratch", 0) == 0 and cnt.get("sgpr-spill", 0) == 0 and listed == [], (cnt, listed)
    facts = {k.strip(): v.strip() for k, v in (r.split(":", 1) for r in res)}
    assert int(facts["VGPRs"]) <= 128 and facts["Occupancy [waves/SIMD]"] == "4", res
    remarks, _ = hotloop._compile(())
    sizes = re.findall(r"Function Name: \S*" + KERNEL + r"\S*.*?LDS Size \[bytes/block\]: (\d+)", remarks, re.S)
    assert sizes and all(int(s) <= 10240 for s in sizes), sizes
