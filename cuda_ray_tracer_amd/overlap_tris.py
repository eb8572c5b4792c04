"""Triangle overlap queries on a built scene: include_ext2/mirt_overlap_tris.h restated for ctypes, and the calls over it.

mirt_overlap_tris.h is an extension header like mirt_overlap_list.h: binding.SIGNATURES stays the table of include/mirt.h, the other
modules' tables those of their headers, and the two entry points more live here.  tests/test_overlap_tris_abi.py holds the table to
the header the way tests/test_binding_header.py holds binding.py to mirt.h.

A row is a triangle, float32 [9]: a, b, c -- what get_triangles writes, so a scene's own mesh is a row array (scene_triangle_rows).
A list is count (overlap_triangles), exclusive scan (overlap_list.list_offsets), fill (triangle_list); triangle_lists does the three.
A word is kind << 30 | id (overlap_list.unpack_words reads it).

Needs ctypes only: torch and numpy are imported when a call needs them.
"""
from . import binding
from .binding import _check, _int, _i64, _u32, _vp

MIRT_TRIS_ANY = 1

# symbol -> (restype, argtypes): every entry point of include_ext2/mirt_overlap_tris.h, in the header's order
OVERLAP_TRIS_SIGNATURES = {
    "mirt_overlap_triangles": (_int, [_vp, _vp, _i64, _vp, _u32, _vp]),
    "mirt_triangle_list": (_int, [_vp, _vp, _i64, _vp, _vp, _i64, _vp]),
}
_I64 = ("int64",)


def lib():
    """binding.lib() with the signatures of mirt_overlap_tris.h applied."""
    return binding.extension_lib(OVERLAP_TRIS_SIGNATURES)


def pack_triangles(verts):
    """float32 [n, 9] rows (a, b, c) for overlap_triangles from the vertices `verts` ([n, 3, 3]: triangle, vertex, coordinate; or
    [n, 9] already), contiguous, on verts' device."""
    import torch
    v = torch.as_tensor(verts, dtype=torch.float32)
    if not ((v.dim() == 3 and tuple(v.shape[1:]) == (3, 3)) or (v.dim() == 2 and v.shape[1] == 9)):
        raise ValueError(f"verts has shape {list(v.shape)}; expected [n, 3, 3] or [n, 9]")
    return v.reshape(v.shape[0], 9).contiguous()


def overlap_triangles(raw, d_tris, d_counts=None, any=False, stream=None):
    """mirt_overlap_triangles: the number of planes, spheres and triangles of the scene every row of d_tris (float32 [n, 9];
    pack_triangles makes them) touches -- with any=True 1 or 0: whether it touches one, the walk ending at the first -- into
    d_counts (int32 [n]; a new tensor on the rows' device if None), which is returned.  A row without area, or with a coordinate
    that is not finite, counts 0.  Both tensors contiguous, distinct and on the scene's device.  Asynchronous on `stream` (default:
    torch's current stream)."""
    from . import api
    d_counts = api._count_tensor((d_tris, "d_tris", 9), d_counts)
    n = d_tris.shape[0]
    api._on_device(api._tensors((d_tris, "d_tris", api._F32, [None, 9]), (d_counts, "d_counts", api._INT, [n])), raw.device)
    _check(lib().mirt_overlap_triangles(raw._h, api._ptr(d_tris), n, api._ptr(d_counts), MIRT_TRIS_ANY if any else 0, api._stream_ptr(stream)))
    return d_counts


def triangle_list(raw, d_tris, d_offsets, d_words, stream=None):
    """mirt_triangle_list: for each row of d_tris (float32 [n, 9]) the words kind << 30 | id (overlap_list.unpack_words) of ALL the
    surfaces the triangle touches into its segment d_words[d_offsets[i] : d_offsets[i + 1]] (d_offsets int64 [n + 1], d_words int32
    [capacity]): the planes by index, then the spheres and triangles in the scene's leaf order.  A row writes no more words than
    its segment holds and none at or beyond d_words.numel().  All tensors contiguous, distinct and on the scene's device.
    Asynchronous on `stream` (default: torch's current stream)."""
    from . import api
    tensors = api._tensors((d_tris, "d_tris", api._F32, [None, 9]))
    n = d_tris.shape[0]
    tensors += api._tensors((d_offsets, "d_offsets", _I64, [n + 1]), (d_words, "d_words", api._INT, [None]))
    api._on_device(tensors, raw.device)
    _check(lib().mirt_triangle_list(raw._h, api._ptr(d_tris), n, api._ptr(d_offsets), api._ptr(d_words), d_words.numel(), api._stream_ptr(stream)))


def triangle_lists(raw, d_tris, sort=False, stream=None):
    """(offsets int64 [n + 1], words int32 [offsets[n]]): every surface every row of d_tris (float32 [n, 9]) touches, row i's in
    words[offsets[i] : offsets[i + 1]] -- overlap_triangles, list_offsets, one host read of the total (it waits for the stream), the
    allocation, triangle_list.  The order within a row is the scene's (planes, then leaf order); sort=True orders each segment
    ascending by unsigned word, i.e. by (kind, id), through one torch sort of row << 32 | word."""
    import torch
    from . import api
    from .overlap_list import list_offsets
    api._on_device(api._tensors((d_tris, "d_tris", api._F32, [None, 9])), raw.device)
    with api._device_and_stream(raw.device, stream) as (dev, s):
        counts = overlap_triangles(raw, d_tris, stream=s)
        offsets = list_offsets(raw, counts, stream=s)
        total = int(offsets[-1].item())
        words = torch.empty(total, dtype=torch.int32, device=dev)
        triangle_list(raw, d_tris, offsets, words, stream=s)
        if sort and total:
            row = torch.repeat_interleave(torch.arange(counts.shape[0], dtype=torch.int64, device=dev), offsets[1:] - offsets[:-1], output_size=total)
            key = torch.sort((row << 32) | (words.to(torch.int64) & 0xffffffff)).values
            words = (((key & 0xffffffff) ^ 0x80000000) - 0x80000000).to(torch.int32)      # (the low word as the int32 of the same bits)
    return offsets, words


def scene_triangle_rows(raw, first=0, count=None, stream=None):
    """float32 [count, 9] on the scene's device: triangles first .. first + count - 1 of the scene itself (file order; count None:
    all from `first` on) as rows, through get_triangles -- for a mesh against itself: row i's list then holds the word of triangle
    first + i and of every triangle that shares a vertex with it."""
    import torch
    from . import api
    total = raw.desc.num_triangles
    count = total - first if count is None else count
    if first < 0 or count < 0 or first + count > total:
        raise ValueError(f"first = {first}, count = {count}; the scene has {total} triangles")
    with api._device_and_stream(raw.device, stream) as (dev, s):
        rows = torch.empty((count, 9), dtype=torch.float32, device=dev)
        if count:
            api.get_triangles(raw, rows, first=first, stream=s)
    return rows
