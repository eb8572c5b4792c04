"""Cast lists on a built scene: include_ext3/mirt_cast_lists.h restated for ctypes, and the calls over it.

mirt_cast_lists.h is an extension header like mirt_query_lists.h: binding.SIGNATURES stays the table of include/mirt.h, the other
modules' tables those of their headers, and the two entry points more live here.  tests/test_cast_lists_abi.py holds the table to
the header the way tests/test_binding_header.py holds binding.py to mirt.h.

A list is count (count_casts), exclusive scan (overlap_list.list_offsets), fill (cast_list); cast_lists does the three.  A word is
kind << 30 | id (overlap_list.unpack_words reads it).  Rows are spherecast.pack_casts'.

Needs ctypes only: torch and numpy are imported when a call needs them.
"""
from . import binding
from .binding import _check, _int, _i64, _u32, _vp

# symbol -> (restype, argtypes): every entry point of include_ext3/mirt_cast_lists.h, in the header's order
CAST_LISTS_SIGNATURES = {
    "mirt_cast_counts": (_int, [_vp, _vp, _i64, _vp, _u32, _vp]),
    "mirt_cast_list": (_int, [_vp, _vp, _i64, _vp, _vp, _vp, _i64, _u32, _vp]),
}
_I64 = ("int64",)


def lib():
    """binding.lib() with the signatures of mirt_cast_lists.h applied."""
    return binding.extension_lib(CAST_LISTS_SIGNATURES)


def count_casts(raw, d_casts, counts=None, stream=None):
    """mirt_cast_counts: for each row (ox, oy, oz, tmax) (dx, dy, dz, r) of d_casts (float32 [n, 8]; pack_casts makes them) the
    number of planes, spheres and triangles the moving ball touches before tmax -- every one, not only the first cast_spheres
    reports -- into counts (int32 [n]; a new tensor on the rows' device if None), which is returned.  A row that is not live counts
    0.  Both tensors contiguous, distinct and on the scene's device.  Asynchronous on `stream` (default: torch's current stream)."""
    from . import api
    counts = api._count_tensor((d_casts, "d_casts", 8), counts)
    n = d_casts.shape[0]
    api._on_device(api._tensors((d_casts, "d_casts", api._F32, [None, 8]), (counts, "counts", api._INT, [n])), raw.device)
    _check(lib().mirt_cast_counts(raw._h, api._ptr(d_casts), n, api._ptr(counts), 0, api._stream_ptr(stream)))
    return counts


def cast_list(raw, d_casts, offsets, words, t=None, stream=None):
    """mirt_cast_list: for each row of d_casts (float32 [n, 8]) the words kind << 30 | id (unpack_words) of ALL the surfaces the
    moving ball touches before its tmax -- the set count_casts counts -- into its segment words[offsets[i] : offsets[i + 1]]
    (offsets int64 [n + 1], words int32 [capacity]), and, if t (float32 [capacity]) is given, the contact parameter of each at the
    word's index (0 where the ball overlaps the surface at the start): the planes by index, then the spheres and triangles in the
    scene's leaf order.  A surface appears once.  A row writes no more than its segment holds and nothing at or beyond
    words.numel().  All tensors contiguous, distinct and on the scene's device.  Asynchronous on `stream` (default: torch's current
    stream)."""
    from . import api
    tensors = api._tensors((d_casts, "d_casts", api._F32, [None, 8]))
    n = d_casts.shape[0]
    tensors += api._tensors((offsets, "offsets", _I64, [n + 1]), (words, "words", api._INT, [None]))
    if t is not None:
        tensors += api._tensors((t, "t", api._F32, [words.shape[0]]))
    api._on_device(tensors, raw.device)
    _check(lib().mirt_cast_list(raw._h, api._ptr(d_casts), n, api._ptr(offsets), api._ptr(words), api._ptr(t), words.numel(), 0, api._stream_ptr(stream)))


def cast_lists(raw, d_casts, values=True, sort=False, stream=None):
    """(offsets int64 [n + 1], words int32 [offsets[n]], t float32 [offsets[n]] or None without `values`): every surface the ball of
    every row of d_casts (float32 [n, 8]) touches before its tmax, row i's in words[offsets[i] : offsets[i + 1]] with its contact
    parameter at the same index -- count_casts, list_offsets, one host read of the total (it waits for the stream), the allocation,
    cast_list.  The order within a row is the scene's (planes, then leaf order); sort=True orders each segment by (t, kind, id),
    cast_spheres' order, through two torch sorts: the first entry of a sorted row is cast_spheres' answer."""
    import torch
    from . import api
    from .overlap_list import list_offsets
    api._on_device(api._tensors((d_casts, "d_casts", api._F32, [None, 8])), raw.device)
    with api._device_and_stream(raw.device, stream) as (dev, s):
        counts = count_casts(raw, d_casts, stream=s)
        offsets = list_offsets(raw, counts, stream=s)
        total = int(offsets[-1].item())
        words = torch.empty(total, dtype=torch.int32, device=dev)
        vals = torch.empty(total, dtype=torch.float32, device=dev) if (values or sort) else None
        cast_list(raw, d_casts, offsets, words, vals, stream=s)
        if sort and total:
            row = torch.repeat_interleave(torch.arange(counts.shape[0], dtype=torch.int64, device=dev), offsets[1:] - offsets[:-1], output_size=total)
            # by t's bits << 32 | word (t is non-negative: its bits order as it does), i.e. (t, kind, id), then stably by row
            bits = vals.view(torch.int32).to(torch.int64) & 0xffffffff
            first = torch.sort((bits << 32) | (words.to(torch.int64) & 0xffffffff)).indices
            at = first[torch.sort(row[first], stable=True).indices]
            words, vals = words[at], vals[at]
    return offsets, words, (vals if values else None)
