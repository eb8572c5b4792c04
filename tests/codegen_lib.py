"""What the ABI and code-generation tests of the query kernels share: a header without its comments, a source's resource usage
as the compiler reports it, and a kernel's instructions.  No GPU needed."""
import os
import re
import subprocess
import tempfile

from cuda_ray_tracer_amd import build as B


def _strip(path):
    """The header's text without its comments."""
    return re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)


def _resource_usage(src):
    """(kernel name -> {resource: value} of -Rpass-analysis=kernel-resource-usage, the assembly) of csrc/<src> for gfx950."""
    with tempfile.TemporaryDirectory(prefix="mirt_codegen_") as tmp:       # private: /tmp is shared between users
        out = os.path.join(tmp, "q.s")
        cmd = [B._hipcc()] + [c for c in B.COMMON if c != "-fPIC"] + ["-x", "hip", "-S", "--cuda-device-only", os.path.join(B.CSRC, src),
                                                                      "-o", out, "-Rpass-analysis=kernel-resource-usage"]
        r = subprocess.run(cmd, capture_output=True, text=True, check=True)
        asm = open(out).read()
    res, cur = {}, None
    for line in r.stderr.splitlines():
        mm = re.search(r"Function Name: (\S+)", line)
        if mm:
            cur = mm.group(1)
            res[cur] = {}
            continue
        mm = re.search(r"remark: \s*([^:]+):\s*(\d+)\s*\[-Rpass", line)
        if cur and mm:
            res[cur][mm.group(1).strip()] = int(mm.group(2))
    return res, asm


def _kernel_body(asm, name):
    """The instructions of kernel `name`, up to its s_endpgm."""
    body, inside = [], False
    for l in asm.splitlines():
        if l.startswith(name + ":"):
            inside = True
            continue
        if inside and "s_endpgm" in l:
            break
        if inside:
            t = l.split(";")[0].strip()
            if t and not t.startswith("."):
                body.append(t)
    assert body, name
    return body
