"""The extension headers (include/mirt_light.h, mirt_visibility.h, mirt_indirect.h, mirt_closest.h, mirt_multihit.h), each against
its module's signature table and the built library: what tests/test_binding_header.py holds for mirt.h, once for all of them.  A new
extension adds a row to EXTENSIONS.  What only one header says stays in that extension's own test file (test_light_abi.py, the
first of them, also still has its own older form of these six).  No GPU needed."""
import collections
import ctypes as C
import importlib
import os
import re
import subprocess
import sys

import pytest

import cuda_ray_tracer_amd as m
from cuda_ray_tracer_amd import api, binding
from cuda_ray_tracer_amd import build as B
from codegen_lib import _strip
from test_binding_header import compare_prototypes, constants, prototypes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PTR, I32, I64, U32, FLT = "pointer", (4, True, False), (8, True, False), (4, False, False), (4, True, True)
INF = float("inf")

# module: of cuda_ray_tracer_amd; table: its signature table; prototype: the header's, as test_binding_header.prototypes reads it;
# constants: the header's #defines, which the module restates (api_constants: and api re-exports); wrong: (a ctypes type of the
# table, the type put in its place, the mismatch compare_prototypes must report); names: what the package exports from the module;
# null_calls: argument lists after the scene, which is NULL.
Extension = collections.namedtuple("Extension", "module header table symbol prototype constants api_constants wrong names source null_calls")
_DIRS = (I32, [PTR, PTR, I64, PTR, I32, PTR, FLT, PTR, PTR, U32, PTR])
_FLOAT_AS_DOUBLE = (C.c_float, C.c_double, "parameter 6 is (4, True, True), the table says (8, True, True)")
_I64_AS_INT = (C.c_int64, C.c_int, "parameter 2 is (8, True, False), the table says (4, True, False)")
EXTENSIONS = [
    Extension("lighting", "mirt_light.h", "LIGHT_SIGNATURES", "mirt_direct_light", (I32, [PTR, PTR, I64, PTR, PTR, U32, PTR]),
              {"MIRT_LIGHT_RAW": 1}, ("MIRT_LIGHT_RAW",), _I64_AS_INT, ("direct_light", "pack_features", "direct_light_frame"), "light.hip",
              [(None, 0, None, None, 0, None), (None, 5, None, None, 1, None)]),
    Extension("visibility", "mirt_visibility.h", "VISIBILITY_SIGNATURES", "mirt_hemisphere_visibility", _DIRS, {}, (), _FLOAT_AS_DOUBLE,
              ("hemisphere_visibility", "cosine_directions", "rotations", "ambient_occlusion_frame"), "visibility.hip",
              [(None, 0, None, 1, None, 1.0, None, None, 0, None), (None, 5, None, 16, None, INF, None, None, 0, None)]),
    Extension("indirect", "mirt_indirect.h", "INDIRECT_SIGNATURES", "mirt_indirect_light", _DIRS, {}, (), _FLOAT_AS_DOUBLE,
              ("indirect_light", "indirect_light_frame"), "indirect.hip",
              [(None, 0, None, 1, None, 1.0, None, None, 0, None), (None, 5, None, 16, None, INF, None, None, 0, None)]),
    Extension("closest", "mirt_closest.h", "CLOSEST_SIGNATURES", "mirt_closest_points", (I32, [PTR, PTR, I64, PTR, PTR, U32, PTR]),
              {}, (), _I64_AS_INT, ("closest_points", "pack_points"), "closest.hip",
              [(None, 0, None, None, 0, None), (None, 5, None, None, 0, None)]),
    Extension("multihit", "mirt_multihit.h", "MULTIHIT_SIGNATURES", "mirt_trace_rays_multi", (I32, [PTR, PTR, I64, I32, PTR, PTR, U32, PTR]),
              {"MIRT_MULTIHIT_MAX_K": 8}, (), _I64_AS_INT, ("trace_rays_multi", "count_hits"), "multihit.hip",
              [(None, 0, 0, None, None, 0, None), (None, 5, 4, None, None, 0, None)]),
]
each = pytest.mark.parametrize("x", EXTENSIONS, ids=[x.module for x in EXTENSIONS])


def _module(x):
    return importlib.import_module("cuda_ray_tracer_amd." + x.module)


def _table(x):
    return getattr(_module(x), x.table)


def _header_path(x):
    return os.path.join(ROOT, "include", x.header)


@each
def test_the_extension_header_agrees_with_the_signature_table(x):
    header, table = _strip(_header_path(x)), _table(x)
    assert [name for name, _, _ in prototypes(header)] == list(table) == [x.symbol]
    assert sorted(set(re.findall(r"\b(mirt_[a-z0-9_]+)\s*\(", header))) == [x.symbol]
    assert compare_prototypes(header, table) == []
    assert prototypes(header)[0] == (x.symbol,) + x.prototype
    assert constants(header) == x.constants
    for name, value in x.constants.items():
        assert getattr(_module(x), name) == value, name
    for name in x.api_constants:
        assert getattr(api, name) == x.constants[name], name
    assert re.search(r'^#include "mirt.h"$', header, flags=re.M)
    # a table that disagrees is a mismatch: in a parameter's type, and in the number of parameters
    restype, argtypes = table[x.symbol]
    right, wrong, message = x.wrong
    assert right in argtypes
    assert compare_prototypes(header, {x.symbol: (restype, [wrong if t is right else t for t in argtypes])}) == [f"{x.symbol}: {message}"]
    n = len(argtypes)
    assert compare_prototypes(header, {x.symbol: (restype, argtypes[:-1])}) == [f"{x.symbol}: {n} parameters, the table has {n - 1}"]
    # an extension leaves the version of mirt.h alone
    assert re.search(r"#define MIRT_VERSION 3\b", open(os.path.join(ROOT, "include", "mirt.h")).read())


@each
def test_the_other_headers_and_tables_do_not_know_the_extension(x):
    assert x.symbol not in open(os.path.join(ROOT, "include", "mirt.h")).read() and x.symbol not in binding.SIGNATURES
    for name in x.constants:
        assert not hasattr(binding, name), name
    others = [y for y in EXTENSIONS if y is not x]
    assert len(others) == len(EXTENSIONS) - 1
    for y in others:
        # (EXTENSIONS is in the order the headers were written: an older header does not name x at all, a newer one may speak of
        # it in its comments -- mirt_indirect.h of mirt_direct_light -- and nowhere else)
        older = EXTENSIONS.index(y) < EXTENSIONS.index(x)
        assert x.symbol not in (open(_header_path(y)).read() if older else _strip(_header_path(y))), y.header
        assert x.symbol not in _table(y), y.table


def test_every_extension_header_has_its_row():
    headers = sorted(f for f in os.listdir(os.path.join(ROOT, "include")) if f != "mirt.h")
    assert headers == sorted(x.header for x in EXTENSIONS)


@each
def test_library_exports_the_symbol_and_the_signature_is_applied(x):
    out = subprocess.run(["nm", "-D", "--defined-only", B.LIB], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT %s$" % x.symbol, out, flags=re.M)
    f = getattr(_module(x).lib(), x.symbol)
    assert f.restype is C.c_int and list(f.argtypes) == _table(x)[x.symbol][1]
    for name in x.names:
        assert getattr(m, name) is getattr(_module(x), name) is getattr(api, name) and name in m.__all__, name


@each
def test_the_module_needs_neither_torch_nor_numpy(x):
    code = f"import sys; import cuda_ray_tracer_amd.{x.module}; assert 'torch' not in sys.modules and 'numpy' not in sys.modules, sorted(sys.modules)"
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


@each
def test_the_build_depends_on_the_extension_header_and_the_kernel(x):
    deps = [os.path.normpath(d) for d in B._all_deps()]
    assert _header_path(x) in deps and os.path.join(B.CSRC, x.source) in deps
    assert x.source in B.LIB_SOURCES


@each
def test_null_scene_is_an_argument_error(x):
    f = getattr(_module(x).lib(), x.symbol)
    for args in x.null_calls:
        # (another call's message first, so that the one read back is this call's)
        assert m.lib().mirt_build_lbvh(None, None, None) == 3 and x.symbol.encode() not in m.lib().mirt_last_error()
        assert f(None, *args) == 3
        assert m.lib().mirt_last_error() == x.symbol.encode() + b": null scene"
