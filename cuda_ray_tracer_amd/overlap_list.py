"""Overlap lists on a built scene: include_ext/mirt_overlap_list.h restated for ctypes, and the calls over it.

mirt_overlap_list.h is an extension header like mirt_overlap.h: binding.SIGNATURES stays the table of include/mirt.h, the other
modules' tables those of their headers, and the three entry points more live here.  tests/test_extension_abi.py holds the table
to the header the way tests/test_binding_header.py holds binding.py to mirt.h.

A list is count (overlap.count_overlaps), exclusive scan (list_offsets), fill (overlap_list); overlap_lists does the three.

Needs ctypes only: torch and numpy are imported when a call needs them.

The package exports this module's function overlap_list, so the attribute cuda_ray_tracer_amd.overlap_list is that function; the
module itself is importlib.import_module("cuda_ray_tracer_amd.overlap_list") (`from cuda_ray_tracer_amd.overlap_list import ...`
works as usual).
"""
from . import binding
from .binding import _check, _int, _i64, _vp

# symbol -> (restype, argtypes): every entry point of include_ext/mirt_overlap_list.h, in the header's order
OVERLAP_LIST_SIGNATURES = {
    "mirt_list_offsets_work_bytes": (_i64, [_i64]),
    "mirt_list_offsets": (_int, [_vp, _vp, _i64, _vp, _vp, _vp]),
    "mirt_overlap_list": (_int, [_vp, _vp, _i64, _vp, _vp, _i64, _vp]),
}
_I64 = ("int64",)


def lib():
    """binding.lib() with the signatures of mirt_overlap_list.h applied."""
    return binding.extension_lib(OVERLAP_LIST_SIGNATURES)


def list_offsets_work_bytes(n):
    """mirt_list_offsets_work_bytes: the bytes of workspace a mirt_list_offsets call of n counts needs (host arithmetic; 0 for a
    small n)."""
    return int(lib().mirt_list_offsets_work_bytes(int(n)))


def list_offsets(raw, d_counts, d_offsets=None, stream=None):
    """mirt_list_offsets: the exclusive prefix sums of d_counts (int32 [n], read as unsigned: what count_overlaps, count_within or
    count_hits wrote) and their total, into d_offsets (int64 [n + 1]; a new tensor on the counts' device if None), which is
    returned: d_offsets[0] = 0, d_offsets[i + 1] = d_offsets[i] + d_counts[i].  64-bit sums.  The call's workspace is allocated
    here.  Asynchronous on `stream` (default: torch's current stream)."""
    import torch
    from . import api
    tensors = api._tensors((d_counts, "d_counts", api._INT, [None]))
    n = d_counts.shape[0]
    if d_offsets is not None:
        tensors += api._tensors((d_offsets, "d_offsets", _I64, [n + 1]))
    api._on_device(tensors, raw.device)
    with api._device_and_stream(raw.device, stream) as (dev, s):
        if d_offsets is None:
            d_offsets = torch.empty(n + 1, dtype=torch.int64, device=dev)
        work = list_offsets_work_bytes(n)
        d_work = torch.empty(work // 8, dtype=torch.int64, device=dev) if work else None
        _check(lib().mirt_list_offsets(raw._h, api._ptr(d_counts), n, api._ptr(d_offsets), api._ptr(d_work), api._stream_ptr(s)))
    return d_offsets


def overlap_list(raw, d_boxes, d_offsets, d_words, stream=None):
    """mirt_overlap_list: for each row of d_boxes (float32 [n, 8]; overlap.pack_boxes makes them) the words kind << 30 | id
    (unpack_words) of ALL the surfaces the box touches into its segment d_words[d_offsets[i] : d_offsets[i + 1]] (d_offsets int64
    [n + 1], d_words int32 [capacity]): the planes by index, then the spheres and triangles in the scene's leaf order.  A row
    writes no more words than its segment holds and none at or beyond d_words.numel().  All tensors contiguous, distinct and on the
    scene's device.  Asynchronous on `stream` (default: torch's current stream)."""
    from . import api
    tensors = api._tensors((d_boxes, "d_boxes", api._F32, [None, 8]))
    n = d_boxes.shape[0]
    tensors += api._tensors((d_offsets, "d_offsets", _I64, [n + 1]), (d_words, "d_words", api._INT, [None]))
    api._on_device(tensors, raw.device)
    _check(lib().mirt_overlap_list(raw._h, api._ptr(d_boxes), n, api._ptr(d_offsets), api._ptr(d_words), d_words.numel(), api._stream_ptr(stream)))


def overlap_lists(raw, d_boxes, sort=False, stream=None):
    """(offsets int64 [n + 1], words int32 [offsets[n]]): every surface every row of d_boxes (float32 [n, 8]) touches, row i's in
    words[offsets[i] : offsets[i + 1]] -- count_overlaps, list_offsets, one host read of the total (it waits for the stream), the
    allocation, overlap_list.  The order within a row is the scene's (planes, then leaf order); sort=True orders each segment
    ascending by unsigned word, i.e. by (kind, id), through one torch sort of row << 32 | word."""
    import torch
    from . import api
    from .overlap import count_overlaps
    api._on_device(api._tensors((d_boxes, "d_boxes", api._F32, [None, 8])), raw.device)
    with api._device_and_stream(raw.device, stream) as (dev, s):
        counts = count_overlaps(raw, d_boxes, stream=s)
        offsets = list_offsets(raw, counts, stream=s)
        total = int(offsets[-1].item())
        words = torch.empty(total, dtype=torch.int32, device=dev)
        overlap_list(raw, d_boxes, offsets, words, stream=s)
        if sort and total:
            row = torch.repeat_interleave(torch.arange(counts.shape[0], dtype=torch.int64, device=dev), offsets[1:] - offsets[:-1], output_size=total)
            key = torch.sort((row << 32) | (words.to(torch.int64) & 0xffffffff)).values
            words = (((key & 0xffffffff) ^ 0x80000000) - 0x80000000).to(torch.int32)      # (the low word as the int32 of the same bits)
    return offsets, words


def unpack_words(words):
    """(kind, id), int32 each, of a tensor of list words kind << 30 | id: the kind (1 sphere, 2 triangle, 3 plane) and the
    file-order index a hit record of that surface carries."""
    import torch
    if words.dtype not in (torch.int32, getattr(torch, "uint32", torch.int32)):
        raise ValueError(f"words has dtype {words.dtype}; expected a 4-byte integer tensor")
    w = words.view(torch.int32)
    return (w >> 30) & 3, w & 0x3fffffff


def voxel_lists(raw, lo, hi, shape, sort=False, stream=None):
    """(offsets int64 [nx * ny * nz + 1], words): the surfaces in every voxel of the regular grid of shape = (nx, ny, nz) over
    [lo, hi], voxel (x, y, z) being row (z * ny + y) * nx + x (overlap.voxel_rows through overlap_lists)."""
    from . import api
    from .overlap import voxel_rows
    rows = voxel_rows(lo, hi, shape)      # (on the host: its checks come before anything touches the device)
    with api._device_and_stream(raw.device, stream) as (dev, s):
        return overlap_lists(raw, rows.to(dev), sort=sort, stream=s)
