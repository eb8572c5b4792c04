"""cuda_ray_tracer_amd/binding.py against include/mirt.h: every prototype against the SIGNATURES table, every struct against its
ctypes class, layouts.py's numpy dtypes against their structs, every restated constant against its #define or enum value.
The header is parsed as text (comments stripped, two regular expressions); neither the built library nor a GPU is needed.
The comparers return a list of mismatches, and the last tests feed them doctored headers to show they can fail."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from cuda_ray_tracer_amd import binding, layouts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mirt.h")).read(), flags=re.S)

# C scalar type -> (bytes, signed, floating)
SCALARS = {"int": (C.sizeof(C.c_int), True, False), "int32_t": (4, True, False), "int64_t": (8, True, False), "uint8_t": (1, False, False),
           "uint32_t": (4, False, False), "uint64_t": (8, False, False), "size_t": (C.sizeof(C.c_size_t), False, False), "float": (4, True, True)}
# ctypes type code -> (signed, floating)
CODES = {"f": (True, True), "d": (True, True), **{c: (True, False) for c in "bhilq"}, **{c: (False, False) for c in "BHILQ"}}


def describe(ct):
    """A ctypes type the way the header's side is described: "void" for None, "pointer", ("struct", its name in the header),
    (element, length) for an array, (bytes, signed, floating) for a scalar."""
    if ct is None:
        return "void"
    if ct in (C.c_void_p, C.c_char_p) or issubclass(ct, C._Pointer):
        return "pointer"
    if issubclass(ct, C.Structure):
        return ("struct", {cls: name for name, cls in binding.STRUCTS.items()}[ct])
    if issubclass(ct, C.Array):
        return (describe(ct._type_), ct._length_)
    return (C.sizeof(ct),) + CODES[ct._type_]


def c_type(words):
    """The same description for a declaration's type, e.g. "const MirtSphere*", "uint32_t", "MirtVec3"."""
    if "*" in words:
        return "pointer"
    name = words.replace("const", "").replace("struct", "").split()
    assert len(name) == 1, words
    return "void" if name[0] == "void" else SCALARS[name[0]] if name[0] in SCALARS else ("struct", name[0])


def constants(header):
    """#define NAME number and enum NAME = number."""
    found = {}
    for name, value in re.findall(r"^\s*(?:#define\s+)?(MIRT_[A-Z0-9_]+)\s*=?\s*(-?[0-9][0-9.]*)[uf]?\s*,?\s*$", header, flags=re.M):
        found[name] = float(value) if "." in value else int(value)
    return found


def prototypes(header):
    """[(name, return type, [parameter, ...])] in the header's order; a parameter is "pointer" or a scalar's description."""
    out = []
    for ret, name, params in re.findall(r"^([A-Za-z_][\w \t\*]*?)\b(mirt_\w+)\s*\(([^)]*)\)\s*;", header, flags=re.M):
        params = [] if params.strip() == "void" else [p.strip() for p in params.split(",")]
        kinds = []
        for p in params:
            if "[" in p:
                kinds.append("pointer")
            else:
                words, arg = re.match(r"(.*?)(\w+)$", p).groups()      # (every parameter of the header is named)
                kinds.append(c_type(words))
        out.append((name, c_type(ret), kinds))
    return out


def structs(header):
    """{struct name: [(field, description)]} for every `typedef struct Name { ... } Name;`."""
    defines = constants(header)
    out = {}
    for name, body in re.findall(r"typedef\s+struct\s+(\w+)\s*\{(.*?)\}\s*\w+\s*;", header, flags=re.S):
        fields = []
        for decl in body.split(";"):
            if not decl.strip():
                continue
            words, names = re.match(r"\s*((?:const\s+)?\w+\s*\*?)\s*(.*)$", decl, flags=re.S).groups()
            for n in names.split(","):
                n = n.strip()
                array = re.match(r"(\w+)\[(\w+)\]$", n)
                if array:
                    length = array.group(2)
                    fields.append((array.group(1), (c_type(words), int(length) if length.isdigit() else defines[length])))
                else:
                    fields.append((n, c_type(words)))
        out[name] = fields
    return out


def compare_prototypes(header, table):
    """Mismatches between the header's prototypes and a SIGNATURES table, in both directions."""
    wrong = []
    protos = prototypes(header)
    for name, ret, params in protos:
        if name not in table:
            wrong.append(f"{name}: not in the table")
            continue
        restype, argtypes = table[name]
        if ret == "pointer":      # (the only pointer the ABI returns is a string)
            if restype is not C.c_char_p:
                wrong.append(f"{name}: returns a string, the table says {restype}")
        elif describe(restype) != ret:
            wrong.append(f"{name}: returns {ret}, the table says {describe(restype)}")
        if len(argtypes) != len(params):
            wrong.append(f"{name}: {len(params)} parameters, the table has {len(argtypes)}")
            continue
        for k, (want, have) in enumerate(zip(params, argtypes)):
            if describe(have) != want:
                wrong.append(f"{name}: parameter {k} is {want}, the table says {describe(have)}")
    declared = [name for name, _, _ in protos]
    wrong += [f"{name}: in the table, not in the header" for name in table if name not in declared]
    if not wrong and list(table) != declared:
        wrong.append("the table is not in the header's order")
    return wrong


def compare_structs(header, classes):
    wrong = []
    parsed = structs(header)
    for name, cls in classes.items():
        if name not in parsed:
            wrong.append(f"{name}: not in the header")
            continue
        have = [(f, describe(t)) for f, t in cls._fields_]
        if have != parsed[name]:
            wrong.append(f"{name}: the header has {parsed[name]}, the class {have}")
    return wrong


def flat_struct(parsed, name):
    """The scalars of a header struct, nested structs and arrays expanded."""
    out = []
    for _, kind in parsed[name]:
        reps = 1
        assert kind != "pointer", name
        if isinstance(kind[0], tuple):      # an array
            kind, reps = kind
        out += (flat_struct(parsed, kind[1]) if kind[0] == "struct" else [kind]) * reps
    return out


def flat_dtype(dt):
    if dt.subdtype:
        base, shape = dt.subdtype
        return flat_dtype(base) * int(np.prod(shape))
    if dt.names:
        offsets = [dt.fields[n][1] for n in dt.names]
        assert offsets == sorted(offsets), dt
        return [s for n in dt.names for s in flat_dtype(dt.fields[n][0])]
    return [(dt.itemsize, dt.kind in "if", dt.kind == "f")]


DTYPES = {"MirtMaterials": layouts.MAT, "MirtSphere": layouts.SPHERE, "MirtTriangle": layouts.TRIANGLE, "MirtPlane": layouts.PLANE,
          "MirtLight": layouts.LIGHT, "MirtPrimRef": layouts.PRIMREF, "MirtTreeNode": layouts.TREENODE}


def compare_dtypes(header, dtypes):
    wrong = []
    parsed = structs(header)
    for name, dt in dtypes.items():
        want = flat_struct(parsed, name)
        if flat_dtype(dt) != want:
            wrong.append(f"{name}: the header has {want}, the dtype {flat_dtype(dt)}")
        if dt.itemsize != sum(size for size, _, _ in want):
            wrong.append(f"{name}: {sum(size for size, _, _ in want)} bytes, the dtype has {dt.itemsize}")
    return wrong


# ---- the shipped binding agrees ----------------------------------------------------------------------------------------------
def test_the_parser_sees_the_whole_header():
    names = sorted(set(re.findall(r"\b(mirt_[a-z0-9_]+)\s*\(", HEADER)))
    assert sorted(name for name, _, _ in prototypes(HEADER)) == names and len(names) == 69
    parsed = structs(HEADER)
    assert set(parsed) >= set(binding.STRUCTS) | set(DTYPES) | {"MirtRGB", "MirtSun", "MirtBulb"}
    assert parsed["MirtVec3"] == [("x", (4, True, True)), ("y", (4, True, True)), ("z", (4, True, True))]
    assert parsed["MirtMultiStats"][2] == ("render_ms", ((4, True, True), 16))
    assert parsed["MirtSceneDesc"][-1] == ("bulbs", "pointer")
    assert ("mirt_render_num_pixels", (8, True, False), ["pointer"]) in prototypes(HEADER)
    assert ("mirt_make_plane", (4, True, False), ["pointer", "pointer", "pointer"]) in prototypes(HEADER)      # (float abcd[4])


def test_every_prototype_has_its_signature_and_every_signature_its_prototype():
    assert compare_prototypes(HEADER, binding.SIGNATURES) == []
    assert binding.EXPORTS == [name for name, _, _ in prototypes(HEADER)]


def test_every_struct_class_has_the_headers_fields():
    assert sorted(binding.STRUCTS) == sorted(["MirtVec3", "MirtRay", "MirtHit", "MirtCamera", "MirtShading", "MirtSceneDesc", "MirtRenderParams",
                                              "MirtStats", "MirtMultiStats", "MirtTreeNode", "MirtRecordInfo", "MirtSampleOrderInfo"])
    assert compare_structs(HEADER, binding.STRUCTS) == []
    assert (C.sizeof(binding.Ray), C.sizeof(binding.Hit), C.sizeof(binding.Camera), C.sizeof(binding.Shading)) == (32, 24, 64, 12)


def test_every_numpy_dtype_has_the_headers_scalars():
    assert compare_dtypes(HEADER, DTYPES) == []
    assert flat_struct(structs(HEADER), "MirtSun") == flat_struct(structs(HEADER), "MirtBulb") == flat_dtype(layouts.LIGHT)


def test_every_restated_constant_has_the_headers_value():
    want = constants(HEADER)
    assert want["MIRT_ERR_STATE"] == 6 and want["MIRT_DENOISE_SIGMA_N"] == 0.03 and want["MIRT_RENDER_COUNTERS"] == 1
    restated = {name: v for name, v in vars(binding).items() if name.startswith("MIRT_") and isinstance(v, (int, float))}
    assert len(restated) >= 17
    for name, v in restated.items():
        assert name in want and want[name] == v and type(want[name]) is type(v), name
    for name in ("MIRT_OK", "MIRT_ERR_IO", "MIRT_ERR_PARSE", "MIRT_ERR_ARG", "MIRT_ERR_HIP", "MIRT_ERR_NO_DEVICE", "MIRT_ERR_STATE"):
        assert name in restated, name


def test_the_binding_module_needs_neither_torch_nor_numpy():
    import subprocess
    import sys
    code = "import sys; import cuda_ray_tracer_amd.binding; assert 'torch' not in sys.modules and 'numpy' not in sys.modules, sorted(sys.modules)"
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


# ---- the comparers can fail --------------------------------------------------------------------------------------------------
def doctored(old, new):
    assert HEADER.count(old) == 1, old
    return HEADER.replace(old, new)


@pytest.mark.parametrize("old,new,symbol", [
    ("const uint32_t* d_pixels, int64_t num_listed,", "const uint32_t* d_pixels, int num_listed,", "mirt_render_accumulate_pixels"),      # narrower
    ("int64_t mirt_render_num_pixels", "int mirt_render_num_pixels", "mirt_render_num_pixels"),                                           # the return type
    ("int mirt_synthetic_scene(uint64_t seed,", "int mirt_synthetic_scene(int64_t seed,", "mirt_synthetic_scene"),                         # signedness
    ("int max_samples, float max_variance,", "int max_samples, int max_variance,", "mirt_select_pixels"),                                  # floatness
    ("int mirt_scene_get_planes(const MirtScene* sc, int first, int count,", "int mirt_scene_get_planes(const MirtScene* sc, int first,", "mirt_scene_get_planes"),
    ("int mirt_multi_num_parts(const MirtMulti* mm);", "int mirt_multi_num_parts(const MirtMulti* mm, int extra);", "mirt_multi_num_parts"),
    ("int mirt_trace_rays(MirtScene* sc, const void* d_rays, int64_t num_rays,", "int mirt_trace_rays(MirtScene* sc, int64_t num_rays, const void* d_rays,", "mirt_trace_rays"),
    ("void mirt_scene_destroy(", "int mirt_scene_destroy(", "mirt_scene_destroy"),
    ("int mirt_version(void);", "int mirt_version(void);\nint mirt_new_call(int x);", "mirt_new_call"),
    ("int mirt_version(void);", "", "mirt_version"),
])
def test_a_doctored_prototype_is_a_mismatch(old, new, symbol):
    wrong = compare_prototypes(doctored(old, new), binding.SIGNATURES)
    assert wrong and all(w.startswith(symbol + ":") for w in wrong), wrong


@pytest.mark.parametrize("old,new,struct", [
    ("float dof_focus, dof_lens; int32_t fisheye, panorama; } MirtCamera;", "float dof_lens, dof_focus; int32_t fisheye, panorama; } MirtCamera;", "MirtCamera"),
    ("typedef struct MirtHit { float t; uint32_t kind, id;", "typedef struct MirtHit { float t; int32_t kind, id;", "MirtHit"),
    ("float render_ms[MIRT_MULTI_MAX_GPUS];", "float render_ms[8];", "MirtMultiStats"),
    ("typedef struct MirtShading { int32_t bounces, gi; float expose; }", "typedef struct MirtShading { int32_t bounces, gi; }", "MirtShading"),
    ("  uint32_t flags;\n", "  uint64_t flags;\n", "MirtRenderParams"),
])
def test_a_doctored_struct_is_a_mismatch(old, new, struct):
    wrong = compare_structs(doctored(old, new), binding.STRUCTS)
    assert len(wrong) == 1 and wrong[0].startswith(struct + ":"), wrong


def test_a_doctored_struct_or_table_is_a_mismatch_for_the_dtypes_and_the_table():
    wrong = compare_dtypes(doctored("float ior, roughness;", "float ior;"), DTYPES)
    assert {w.split(":")[0] for w in wrong} == {"MirtMaterials", "MirtSphere", "MirtTriangle", "MirtPlane"}, wrong
    wrong = compare_dtypes(doctored("typedef struct MirtPrimRef { uint32_t type; uint32_t id; }", "typedef struct MirtPrimRef { uint32_t type; int32_t id; }"), DTYPES)
    assert len(wrong) == 1 and wrong[0].startswith("MirtPrimRef:"), wrong
    table = dict(binding.SIGNATURES)
    restype, argtypes = table["mirt_trace_rays"]
    table["mirt_trace_rays"] = (restype, [C.c_int if t is C.c_int64 else t for t in argtypes])      # the mistake the guard is for
    assert compare_prototypes(HEADER, table) == ["mirt_trace_rays: parameter 2 is (8, True, False), the table says (4, True, False)"]
