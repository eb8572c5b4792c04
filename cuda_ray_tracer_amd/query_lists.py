"""Ray and ball lists on a built scene: include_ext/mirt_query_lists.h restated for ctypes, and the calls over it.

mirt_query_lists.h is an extension header like mirt_overlap_list.h: binding.SIGNATURES stays the table of include/mirt.h, the other
modules' tables those of their headers, and the two entry points more live here.  tests/test_extension_abi.py holds the table to
the header the way tests/test_binding_header.py holds binding.py to mirt.h.

A list is count (multihit.count_hits / contacts.count_within), exclusive scan (overlap_list.list_offsets), fill (ray_list /
ball_list); ray_lists and ball_lists do the three.  A word is kind << 30 | id (overlap_list.unpack_words reads it).

Needs ctypes only: torch and numpy are imported when a call needs them.
"""
from . import binding
from .binding import _check, _int, _i64, _u32, _vp

# symbol -> (restype, argtypes): every entry point of include_ext/mirt_query_lists.h, in the header's order
QUERY_LISTS_SIGNATURES = {
    "mirt_ray_list": (_int, [_vp, _vp, _i64, _vp, _vp, _vp, _i64, _u32, _vp]),
    "mirt_ball_list": (_int, [_vp, _vp, _i64, _vp, _vp, _vp, _i64, _u32, _vp]),
}
_I64 = ("int64",)


def lib():
    """binding.lib() with the signatures of mirt_query_lists.h applied."""
    return binding.extension_lib(QUERY_LISTS_SIGNATURES)


def _fill(symbol, raw, d_rows, rows_name, width, d_offsets, d_words, d_values, values_name, stream):
    from . import api
    tensors = api._tensors((d_rows, rows_name, api._F32, [None, width]))
    n = d_rows.shape[0]
    tensors += api._tensors((d_offsets, "d_offsets", _I64, [n + 1]), (d_words, "d_words", api._INT, [None]))
    if d_values is not None:
        tensors += api._tensors((d_values, values_name, api._F32, [d_words.shape[0]]))
    api._on_device(tensors, raw.device)
    _check(getattr(lib(), symbol)(raw._h, api._ptr(d_rows), n, api._ptr(d_offsets), api._ptr(d_words), api._ptr(d_values), d_words.numel(), 0,
                                  api._stream_ptr(stream)))


def ray_list(raw, d_rays, d_offsets, d_words, d_t=None, stream=None):
    """mirt_ray_list: for each ray of d_rays (float32 [n, 8], MirtRay rows: pack_rays) the words kind << 30 | id (unpack_words) of
    ALL the surfaces it crosses before its tmax -- the set count_hits counts -- into its segment d_words[d_offsets[i] :
    d_offsets[i + 1]] (d_offsets int64 [n + 1], d_words int32 [capacity]), and, if d_t (float32 [capacity]) is given, the t of each
    at the word's index: the planes by index, then the spheres and triangles in the scene's leaf order.  A row writes no more than
    its segment holds and nothing at or beyond d_words.numel().  All tensors contiguous, distinct and on the scene's device.
    Asynchronous on `stream` (default: torch's current stream)."""
    _fill("mirt_ray_list", raw, d_rays, "d_rays", 8, d_offsets, d_words, d_t, "d_t", stream)


def ball_list(raw, d_points, d_offsets, d_words, d_dist=None, stream=None):
    """mirt_ball_list: for each row (qx, qy, qz, R) of d_points (float32 [n, 4]) the words kind << 30 | id (unpack_words) of ALL
    the surfaces nearer than R -- the set count_within counts -- into its segment d_words[d_offsets[i] : d_offsets[i + 1]]
    (d_offsets int64 [n + 1], d_words int32 [capacity]), and, if d_dist (float32 [capacity]) is given, the distance of each at the
    word's index: the planes by index, then the spheres and triangles in the scene's leaf order.  A row writes no more than its
    segment holds and nothing at or beyond d_words.numel().  All tensors contiguous, distinct and on the scene's device.
    Asynchronous on `stream` (default: torch's current stream)."""
    _fill("mirt_ball_list", raw, d_points, "d_points", 4, d_offsets, d_words, d_dist, "d_dist", stream)


def _bits(values):
    """The bits of non-negative float32 values as int64: they order as the values do."""
    import torch
    return values.view(torch.int32).to(torch.int64) & 0xffffffff


def _lists(raw, d_rows, rows_name, width, count, fill, values, sort, order, stream):
    import torch
    from . import api
    from .overlap_list import list_offsets
    api._on_device(api._tensors((d_rows, rows_name, api._F32, [None, width])), raw.device)
    with api._device_and_stream(raw.device, stream) as (dev, s):
        counts = count(raw, d_rows, stream=s)
        offsets = list_offsets(raw, counts, stream=s)
        total = int(offsets[-1].item())
        words = torch.empty(total, dtype=torch.int32, device=dev)
        vals = torch.empty(total, dtype=torch.float32, device=dev) if (values or sort) else None
        fill(raw, d_rows, offsets, words, vals, stream=s)
        if sort and total:
            row = torch.repeat_interleave(torch.arange(counts.shape[0], dtype=torch.int64, device=dev), offsets[1:] - offsets[:-1], output_size=total)
            at = order(row, words, vals)
            words, vals = words[at], vals[at]
    return offsets, words, (vals if values else None)


def _ray_order(row, words, t):
    # one stable sort of row << 32 | t's bits: within a t the emission order stays, which is the record call's (class, index)
    import torch
    return torch.sort((row << 32) | _bits(t), stable=True).indices


def _ball_order(row, words, dist):
    # by dist's bits << 32 | word, i.e. (dist, kind, id), then stably by row
    import torch
    first = torch.sort((_bits(dist) << 32) | (words.to(torch.int64) & 0xffffffff)).indices
    return first[torch.sort(row[first], stable=True).indices]


def ray_lists(raw, d_rays, values=True, sort=False, stream=None):
    """(offsets int64 [n + 1], words int32 [offsets[n]], t float32 [offsets[n]] or None without `values`): every surface every ray
    of d_rays (float32 [n, 8]) crosses before its tmax, row i's in words[offsets[i] : offsets[i + 1]] with its t at the same index
    -- count_hits, list_offsets, one host read of the total (it waits for the stream), the allocation, ray_list.  The order within
    a row is the scene's (planes, then leaf order); sort=True orders each segment as trace_rays_multi orders its records, by
    (t, class, index), through one stable torch sort."""
    from .multihit import count_hits
    return _lists(raw, d_rays, "d_rays", 8, count_hits, ray_list, values, sort, _ray_order, stream)


def ball_lists(raw, d_points, values=True, sort=False, stream=None):
    """(offsets int64 [n + 1], words int32 [offsets[n]], dist float32 [offsets[n]] or None without `values`): every surface nearer
    than R to every row (qx, qy, qz, R) of d_points (float32 [n, 4]), row i's in words[offsets[i] : offsets[i + 1]] with its distance
    at the same index -- count_within, list_offsets, one host read of the total (it waits for the stream), the allocation,
    ball_list.  The order within a row is the scene's (planes, then leaf order); sort=True orders each segment as
    closest_points_multi orders its records, by (dist, kind, id), through two torch sorts."""
    from .contacts import count_within
    return _lists(raw, d_points, "d_points", 4, count_within, ball_list, values, sort, _ball_order, stream)
