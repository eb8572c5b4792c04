"""Every extension header (the five under include/ and the five under include_ext/), each against its module's signature table
and the built library: what tests/test_binding_header.py holds for mirt.h, once for all of them.  A new extension adds a row to
EXTENSIONS.  What only one header says stays in that extension's own test file.  No GPU needed."""
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

# A symbol: its name; prototype: the header's, as test_binding_header.prototypes reads it; null_calls: argument lists after the scene,
# which is NULL (None: the entry point takes no scene).
Symbol = collections.namedtuple("Symbol", "name prototype null_calls")
# module: of cuda_ray_tracer_amd; folder: the header's, from which its include line of mirt.h follows; table: the module's signature
# table; symbols: in the header's order; constants: the header's #defines, which the module restates (api_constants: and api
# re-exports); wrong: (the symbol doctored, a ctypes type of its row in the table, the type put in its place, the mismatches
# compare_prototypes must report for it); names: what the package exports from the module; source, csrc_headers: the kernel and the
# headers of csrc the build must depend on.
Extension = collections.namedtuple("Extension", "module folder header table symbols constants api_constants wrong names source csrc_headers")
INCLUDE_LINE = {"include": '#include "mirt.h"', "include_ext": '#include "../include/mirt.h"'}


def _float_as_double(symbol):
    return (symbol, C.c_float, C.c_double, ["parameter 6 is (4, True, True), the table says (8, True, True)"])


def _i64_as_int(symbol, *parameters):
    return (symbol, C.c_int64, C.c_int, [f"parameter {p} is (8, True, False), the table says (4, True, False)" for p in parameters])


_ROWS = (I32, [PTR, PTR, I64, PTR, PTR, U32, PTR])
_DIRS = (I32, [PTR, PTR, I64, PTR, I32, PTR, FLT, PTR, PTR, U32, PTR])
_DIRS_NULL = [(None, 0, None, 1, None, 1.0, None, None, 0, None), (None, 5, None, 16, None, INF, None, None, 0, None)]
_RECORDS = (I32, [PTR, PTR, I64, I32, PTR, PTR, PTR, U32, PTR])
_FILL = (I32, [PTR, PTR, I64, PTR, PTR, PTR, I64, U32, PTR])
_FILL_NULL = [(None, 0, None, None, None, 0, 0, None), (None, 5, None, None, None, 7, 0, None), (None, -1, None, None, None, -1, 9, None)]
# (in the order the headers were written: test_the_other_headers_and_tables_do_not_know_the_extension reads it)
EXTENSIONS = [
    Extension("lighting", "include", "mirt_light.h", "LIGHT_SIGNATURES",
              [Symbol("mirt_direct_light", _ROWS, [(None, 0, None, None, 0, None), (None, 5, None, None, 1, None)])],
              {"MIRT_LIGHT_RAW": 1}, ("MIRT_LIGHT_RAW",), _i64_as_int("mirt_direct_light", 2),
              ("direct_light", "pack_features", "direct_light_frame"), "light.hip", ()),
    Extension("visibility", "include", "mirt_visibility.h", "VISIBILITY_SIGNATURES", [Symbol("mirt_hemisphere_visibility", _DIRS, _DIRS_NULL)],
              {}, (), _float_as_double("mirt_hemisphere_visibility"),
              ("hemisphere_visibility", "cosine_directions", "rotations", "ambient_occlusion_frame"), "visibility.hip", ()),
    Extension("indirect", "include", "mirt_indirect.h", "INDIRECT_SIGNATURES", [Symbol("mirt_indirect_light", _DIRS, _DIRS_NULL)],
              {}, (), _float_as_double("mirt_indirect_light"), ("indirect_light", "indirect_light_frame"), "indirect.hip", ()),
    Extension("closest", "include", "mirt_closest.h", "CLOSEST_SIGNATURES",
              [Symbol("mirt_closest_points", _ROWS, [(None, 0, None, None, 0, None), (None, 5, None, None, 0, None)])],
              {}, (), _i64_as_int("mirt_closest_points", 2), ("closest_points", "pack_points"), "closest.hip", ()),
    Extension("multihit", "include", "mirt_multihit.h", "MULTIHIT_SIGNATURES",
              [Symbol("mirt_trace_rays_multi", (I32, [PTR, PTR, I64, I32, PTR, PTR, U32, PTR]),
                      [(None, 0, 0, None, None, 0, None), (None, 5, 4, None, None, 0, None)])],
              {"MIRT_MULTIHIT_MAX_K": 8}, (), _i64_as_int("mirt_trace_rays_multi", 2), ("trace_rays_multi", "count_hits"), "multihit.hip", ()),
    Extension("contacts", "include_ext", "mirt_contacts.h", "CONTACTS_SIGNATURES",
              [Symbol("mirt_closest_points_multi", _RECORDS, [(None, 0, 0, None, None, None, 0, None), (None, 5, 4, None, None, None, 0, None)])],
              {"MIRT_CONTACTS_MAX_K": 8}, (), _i64_as_int("mirt_closest_points_multi", 2), ("closest_points_multi", "count_within"),
              "closest_multi.hip", ("point_query.h", "key_list.h")),
    Extension("spherecast", "include_ext", "mirt_spherecast.h", "SPHERECAST_SIGNATURES",
              [Symbol("mirt_cast_spheres", _ROWS, [(None, 0, None, None, 0, None), (None, 5, None, None, 1, None)])],
              {"MIRT_CAST_ANY_HIT": 1}, (), _i64_as_int("mirt_cast_spheres", 2), ("cast_spheres", "pack_casts"),
              "spherecast.hip", ("point_query.h", "query_walk.h")),
    Extension("overlap", "include_ext", "mirt_overlap.h", "OVERLAP_SIGNATURES",
              [Symbol("mirt_overlap_boxes", _RECORDS, [(None, 0, 0, None, None, None, 0, None), (None, 5, 4, None, None, None, 1, None)])],
              {"MIRT_OVERLAP_MAX_K": 8, "MIRT_OVERLAP_ANY": 1}, (), _i64_as_int("mirt_overlap_boxes", 2),
              ("overlap_boxes", "count_overlaps", "pack_boxes", "voxel_rows", "occupancy_grid"), "overlap.hip", ("point_query.h", "key_list.h")),
    # (no record format and no constant of their own in the two list headers: a word and a value are 32 bits each)
    Extension("overlap_list", "include_ext", "mirt_overlap_list.h", "OVERLAP_LIST_SIGNATURES",
              [Symbol("mirt_list_offsets_work_bytes", (I64, [I64]), None),
               Symbol("mirt_list_offsets", (I32, [PTR, PTR, I64, PTR, PTR, PTR]), [(None, 0, None, None, None), (None, 5, None, None, None)]),
               Symbol("mirt_overlap_list", (I32, [PTR, PTR, I64, PTR, PTR, I64, PTR]), [(None, 0, None, None, 0, None), (None, 5, None, None, 7, None)])],
              {}, (), _i64_as_int("mirt_overlap_list", 2, 5),
              ("list_offsets", "list_offsets_work_bytes", "overlap_list", "overlap_lists", "unpack_words", "voxel_lists"),
              "overlap_list.hip", ("overlap_tests.h", "block_scan.h")),
    Extension("query_lists", "include_ext", "mirt_query_lists.h", "QUERY_LISTS_SIGNATURES",
              [Symbol("mirt_ray_list", _FILL, _FILL_NULL), Symbol("mirt_ball_list", _FILL, _FILL_NULL)],
              {}, (), _i64_as_int("mirt_ball_list", 2, 6), ("ray_list", "ball_list", "ray_lists", "ball_lists"), "query_lists.hip", ("list_cursor.h",)),
]
each = pytest.mark.parametrize("x", EXTENSIONS, ids=[x.module for x in EXTENSIONS])
ENTRY_POINTS = [s.name for x in EXTENSIONS for s in x.symbols]


def _module(x):
    # (by importlib: the package attribute overlap_list is the function, not the module)
    return importlib.import_module("cuda_ray_tracer_amd." + x.module)


def _table(x):
    return getattr(_module(x), x.table)


def _header_path(x):
    return os.path.join(ROOT, x.folder, x.header)


def other_entry_points(x):
    """The entry points of every extension but x."""
    return [s.name for y in EXTENSIONS if y is not x for s in y.symbols]


def mentions(text, symbol):
    """The identifiers of `text` that contain `symbol`, but for the other entry points whose names it begins (mirt_closest_points
    begins mirt_closest_points_multi, mirt_list_offsets begins mirt_list_offsets_work_bytes)."""
    return [w for w in re.findall(r"\w+", text) if symbol in w and (w == symbol or w not in ENTRY_POINTS)]


@each
def test_the_extension_header_agrees_with_the_signature_table(x):
    header, table, names = _strip(_header_path(x)), _table(x), [s.name for s in x.symbols]
    assert [name for name, _, _ in prototypes(header)] == list(table) == names
    assert sorted(set(re.findall(r"\b(mirt_[a-z0-9_]+)\s*\(", header))) == sorted(names)
    assert compare_prototypes(header, table) == []
    assert prototypes(header) == [(s.name,) + s.prototype for s in x.symbols]
    assert constants(header) == x.constants
    for name, value in x.constants.items():
        assert getattr(_module(x), name) == value, name
    for name in x.api_constants:
        assert getattr(api, name) == x.constants[name], name
    assert re.findall(r'^#include "[./a-z]*mirt\.h"$', header, flags=re.M) == [INCLUDE_LINE[x.folder]]
    # a table that disagrees is a mismatch: in a parameter's type, and in the number of parameters
    symbol, right, wrong, messages = x.wrong
    restype, argtypes = table[symbol]
    assert right in argtypes
    doctored = {**table, symbol: (restype, [wrong if t is right else t for t in argtypes])}
    assert compare_prototypes(header, doctored) == [f"{symbol}: {message}" for message in messages]
    for name, (restype, argtypes) in table.items():
        n = len(argtypes)
        assert compare_prototypes(header, {**table, name: (restype, argtypes[:-1])}) == [f"{name}: {n} parameters, the table has {n - 1}"]
    # an extension leaves the version of mirt.h alone
    assert re.search(r"#define MIRT_VERSION 3\b", open(os.path.join(ROOT, "include", "mirt.h")).read())


@each
def test_the_other_headers_and_tables_do_not_know_the_extension(x):
    for name in x.constants:
        assert not hasattr(binding, name), name
    others = [y for y in EXTENSIONS if y is not x]
    assert len(others) == len(EXTENSIONS) - 1
    for s in x.symbols:
        assert mentions(open(os.path.join(ROOT, "include", "mirt.h")).read(), s.name) == [] and s.name not in binding.SIGNATURES
        for y in others:
            # (EXTENSIONS is in the order the headers were written: an older header does not name x at all, a newer one may speak of
            # it in its comments -- mirt_indirect.h of mirt_direct_light, mirt_contacts.h of mirt_closest_points -- and nowhere else)
            older = EXTENSIONS.index(y) < EXTENSIONS.index(x)
            assert mentions(open(_header_path(y)).read() if older else _strip(_header_path(y)), s.name) == [], (s.name, y.header)
            assert s.name not in _table(y), (s.name, y.table)


def test_every_extension_header_has_its_row():
    found = sorted((folder, f) for folder in INCLUDE_LINE for f in os.listdir(os.path.join(ROOT, folder)) if (folder, f) != ("include", "mirt.h"))
    assert found == sorted((x.folder, x.header) for x in EXTENSIONS)


@each
def test_library_exports_the_symbol_and_the_signature_is_applied(x):
    out = subprocess.run(["nm", "-D", "--defined-only", B.LIB], capture_output=True, text=True, check=True).stdout
    for s in x.symbols:
        assert re.search(r"\bT %s$" % s.name, out, flags=re.M), s.name
        f = getattr(_module(x).lib(), s.name)
        restype, argtypes = _table(x)[s.name]
        assert f.restype is restype is {I32: C.c_int, I64: C.c_int64}[s.prototype[0]] and list(f.argtypes) == argtypes, s.name
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
    for path in (_header_path(x), os.path.join(B.CSRC, x.source), *(os.path.join(B.CSRC, h) for h in x.csrc_headers)):
        assert path in deps, path
    assert x.source in B.LIB_SOURCES


@each
def test_null_scene_is_an_argument_error(x):
    assert any(s.null_calls for s in x.symbols)
    for s in x.symbols:
        for args in s.null_calls or ():
            # (another call's message first, so that the one read back is this call's)
            assert m.lib().mirt_build_lbvh(None, None, None) == 3 and s.name.encode() not in m.lib().mirt_last_error()
            assert getattr(_module(x).lib(), s.name)(None, *args) == 3
            assert m.lib().mirt_last_error() == s.name.encode() + b": null scene"
