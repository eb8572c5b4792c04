#!/usr/bin/env python3
"""Which kernels did a source change move?  Compiles HIP sources of two trees to gfx950 assembly (no GPU) and compares them.

    python tools/asmdiff.py PARENT_TREE [FILE.hip ...]

PARENT_TREE is a checkout of the commit to compare against (`git worktree add --detach DIR COMMIT`); the other tree is the one
this script lies in.  The named sources -- by default every .hip of build.LIB_SOURCES -- are compiled in both trees with
build.COMMON (`-S --cuda-device-only`, private temporary directories, at most 16 compiles at a time).  Per kernel the instruction
lines from its label to its `.Lfunc_end` are compared, comments and directives stripped.  Prints, per differing kernel, both
lengths, the number of differing lines and the resource figures that changed (registers, occupancy, scratch, spill counts), then
a summary per file; exit status 1 if any kernel differs.  Reads nothing but the two source trees.
"""
import concurrent.futures
import difflib
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from cuda_ray_tracer_amd import build as B

CSRC_REL = os.path.relpath(B.CSRC, os.path.abspath(ROOT))
RESOURCES = ("NumVgprs", "NumAgprs", "TotalNumSgprs", "ScratchSize", "Occupancy")


def compile_s(tree, src, out):
    cmd = [B._hipcc()] + B.COMMON + ["-x", "hip", "-S", "--cuda-device-only", os.path.join(tree, CSRC_REL, src), "-o", out]
    subprocess.check_call(cmd, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    return out


def kernels(path):
    """{name: (instruction lines, {resource: value})} of one assembly file."""
    with open(path) as fh:
        lines = fh.read().split("\n")
    names = {m.group(1) for m in (re.match(r"\s*\.amdhsa_kernel\s+(\S+)", l) for l in lines) if m}
    out, spills, name, body, meta_name = {}, {}, None, None, None
    for l in lines:
        m = re.match(r"(\w+):", l)
        if m and m.group(1) in names and body is None:
            name, body = m.group(1), []
            out[name] = (body, {})
            continue
        m = re.match(r";\s*(\w+):\s*(\d+)\s*$", l)
        if m and name and body is None and m.group(1) in RESOURCES:
            out[name][1].setdefault(m.group(1), int(m.group(2)))
        m = re.match(r"\s*\.name:\s*(\S+)", l)
        if m:
            meta_name = m.group(1)
        m = re.match(r"\s*\.(sgpr|vgpr)_spill_count:\s*(\d+)", l)
        if m:
            spills.setdefault(meta_name, {})[m.group(1) + "_spills"] = int(m.group(2))
        if body is None:
            continue
        if l.startswith(".Lfunc_end"):
            body = None      # (the resource comments of `name` follow)
            continue
        t = l.split(";")[0].strip()
        if not t or (t.startswith(".") and not t.endswith(":")):
            continue
        body.append(re.sub(r"\.LBB\d+_", ".LBB_", t))      # (the function's number in its file is not part of its code)
    # (the spill counts stand in the metadata at the end of the file, under the kernel's .name, which its keys' order puts first)
    for n, s in spills.items():
        if n in out:
            out[n][1].update(s)
    return out


def differing_lines(a, b):
    sm = difflib.SequenceMatcher(None, a, b, autojunk=False)
    return sum(max(i2 - i1, j2 - j1) for tag, i1, i2, j1, j2 in sm.get_opcodes() if tag != "equal")


def demangle(names):
    tool = shutil.which("llvm-cxxfilt", path=os.path.dirname(B._hipcc()) + os.pathsep + os.path.join(os.path.dirname(B._hipcc()), "..", "llvm", "bin")) or shutil.which("c++filt")
    if not tool or not names:
        return {n: n for n in names}
    res = subprocess.run([tool] + list(names), capture_output=True, text=True)
    got = res.stdout.split("\n")[:len(names)]
    return dict(zip(names, got)) if res.returncode == 0 and len(got) == len(names) else {n: n for n in names}


def main(argv):
    if len(argv) < 2 or argv[1].startswith("-"):
        print(__doc__)
        return 2
    parent = os.path.abspath(argv[1])
    sources = argv[2:] or [s for s in B.LIB_SOURCES if s.endswith(".hip")]
    sources = [os.path.basename(s) for s in sources]
    for s in [s for s in sources if not os.path.exists(os.path.join(parent, CSRC_REL, s))]:
        print(f"{s}: only in the new tree")      # (a new source moves no kernel of the parent's)
        sources.remove(s)
    moved = 0
    with tempfile.TemporaryDirectory() as tp, tempfile.TemporaryDirectory() as tn, concurrent.futures.ThreadPoolExecutor(max_workers=16) as pool:
        jobs = {s: (pool.submit(compile_s, parent, s, os.path.join(tp, s + ".s")), pool.submit(compile_s, os.path.abspath(ROOT), s, os.path.join(tn, s + ".s"))) for s in sources}
        for s in sources:
            old, new = kernels(jobs[s][0].result()), kernels(jobs[s][1].result())
            names = sorted(set(old) | set(new))
            pretty = demangle(names)
            diff = 0
            for n in names:
                if n not in old or n not in new:
                    print(f"{s}: {pretty[n]}: only in the {'parent' if n in old else 'new'} tree")
                    diff += 1
                    continue
                (a, ra), (b, rb) = old[n], new[n]
                if a == b:
                    continue
                diff += 1
                res = ", ".join(f"{k} {ra.get(k)} -> {rb.get(k)}" for k in sorted(set(ra) | set(rb)) if ra.get(k) != rb.get(k)) or "resources unchanged"
                print(f"{s}: {pretty[n]}: {len(a)} -> {len(b)} lines, {differing_lines(a, b)} differ; {res}")
            print(f"{s}: {len(names) - diff} of {len(names)} kernels identical")
            moved += diff
    return 1 if moved else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
