"""Box overlap queries on a built scene: include_ext/mirt_overlap.h restated for ctypes, and the calls over it.

mirt_overlap.h is an extension header like mirt_contacts.h and mirt_spherecast.h: binding.SIGNATURES stays the table of
include/mirt.h, the other modules' tables those of their headers, and the one entry point more lives here.
tests/test_extension_abi.py holds the table to the header the way tests/test_binding_header.py holds binding.py to mirt.h.

Needs ctypes only: torch and numpy are imported when a call needs them.  The records are read by api.unpack_hits
(d_hits.reshape(-1, 6)).
"""
from . import binding
from .binding import _check, _int, _i64, _u32, _vp

MIRT_OVERLAP_MAX_K = 8
MIRT_OVERLAP_ANY = 1

# symbol -> (restype, argtypes): every entry point of include_ext/mirt_overlap.h, in the header's order
OVERLAP_SIGNATURES = {
    "mirt_overlap_boxes": (_int, [_vp, _vp, _i64, _int, _vp, _vp, _vp, _u32, _vp]),
}


def lib():
    """binding.lib() with the signatures of mirt_overlap.h applied."""
    return binding.extension_lib(OVERLAP_SIGNATURES)


def overlap_boxes(raw, d_boxes, d_hits, d_counts=None, d_features=None, any_overlap=False, stream=None):
    """mirt_overlap_boxes: for each row (lox, loy, loz, _) (hix, hiy, hiz, _) of d_boxes (float32 [n, 8]; pack_boxes makes them)
    all the planes, spheres and triangles whose surface meets the box [lo, hi]: the k nearest to the box's centre, nearest first,
    into d_hits (int32 [n, k, 6], k read from the shape, at most 8; MirtHit records: unpack_hits reads d_hits.reshape(-1, 6)) --
    slots past a row's surfaces are misses (t = -1) -- and, if d_counts (int32 [n]) is given, the number of all of them, which may
    exceed k.  d_features (float32 [n, k, 8]), if given, receives each record's surface point nearest the centre (it may lie
    outside the box) and normal in hit_features' layout.  d_hits None: a count-only call; with any_overlap the count is 1 or 0
    (does the box touch anything) and the walk ends at the first surface found.  All tensors contiguous, distinct and on the
    scene's device.  Asynchronous on `stream` (default: torch's current stream)."""
    from . import api

    def count_only(k):
        if any_overlap and k != 0:
            raise ValueError("any_overlap is a count-only call: d_hits must be None (or k = 0)")

    tensors, n, k = api._record_tensors((d_boxes, "d_boxes", 8), d_hits, d_counts, d_features, max_k=MIRT_OVERLAP_MAX_K, check_k=count_only)
    api._on_device(tensors, raw.device)
    _check(lib().mirt_overlap_boxes(raw._h, api._ptr(d_boxes), n, k, api._ptr(d_hits), api._ptr(d_counts), api._ptr(d_features),
                                    MIRT_OVERLAP_ANY if any_overlap else 0, api._stream_ptr(stream)))


def count_overlaps(raw, d_boxes, d_counts=None, any_overlap=False, stream=None):
    """The number of surfaces every row of d_boxes (float32 [n, 8]) touches -- with any_overlap 1 or 0: whether it touches any --
    into d_counts (int32 [n]; a new tensor on the rows' device if None), which is returned: overlap_boxes with k = 0."""
    from . import api
    d_counts = api._count_tensor((d_boxes, "d_boxes", 8), d_counts)
    overlap_boxes(raw, d_boxes, None, d_counts, any_overlap=any_overlap, stream=stream)
    return d_counts


def pack_boxes(lo, hi):
    """float32 [n, 8] rows (lox, loy, loz, 0) (hix, hiy, hiz, 0) for overlap_boxes from the corners lo and hi ([n, 3] each, or one of
    them [3]), on hi's device."""
    import torch
    hi = torch.as_tensor(hi, dtype=torch.float32)
    lo = torch.as_tensor(lo, dtype=torch.float32, device=hi.device)
    if hi.dim() == 1 and lo.dim() == 2:
        hi = hi.expand(lo.shape[0], -1)
    if hi.dim() != 2 or hi.shape[1] != 3:
        raise ValueError(f"hi has shape {list(hi.shape)}; expected [n, 3]")
    n = hi.shape[0]
    if tuple(lo.shape) not in ((3,), (n, 3)):
        raise ValueError(f"lo has shape {list(lo.shape)}; expected [3] or [{n}, 3]")
    out = torch.zeros((n, 8), dtype=torch.float32, device=hi.device)
    out[:, 0:3] = lo
    out[:, 4:7] = hi
    return out


def voxel_edges(lo, hi, shape):
    """The float32 edge arrays (x [nx + 1], y [ny + 1], z [nz + 1]) of the regular grid of shape = (nx, ny, nz) voxels over the box
    [lo, hi]: edge j of an axis is lo + (hi - lo) * j / n in float64, rounded once, the last edge hi itself.  voxel_rows takes its
    voxels' faces from these, so that two neighbours share a face's one bit pattern."""
    import numpy as np
    lo = np.asarray(lo, np.float64).reshape(3)
    hi = np.asarray(hi, np.float64).reshape(3)
    if len(shape) != 3 or any(int(s) < 1 for s in shape):
        raise ValueError(f"shape is {shape!r}; expected three positive voxel counts (nx, ny, nz)")
    if not (np.all(np.isfinite(lo)) and np.all(np.isfinite(hi)) and np.all(lo <= hi)):
        raise ValueError("lo and hi must be finite with lo <= hi on every axis")
    edges = []
    for a in range(3):
        n = int(shape[a])
        e = (lo[a] + (hi[a] - lo[a]) * (np.arange(n + 1, dtype=np.float64) / n)).astype(np.float32)
        e[0], e[n] = np.float32(lo[a]), np.float32(hi[a])
        edges.append(e)
    return tuple(edges)


def voxel_rows(lo, hi, shape, device=None):
    """float32 [nx * ny * nz, 8] rows for overlap_boxes: the voxels of the regular grid of shape = (nx, ny, nz) over [lo, hi], x
    fastest, then y, then z (row (z * ny + y) * nx + x).  Per axis one float32 edge array (voxel_edges) is shared by neighbouring
    voxels, so a shared face has one bit pattern: a surface lying exactly on it touches both.  A torch tensor on `device` (None:
    the host)."""
    import numpy as np
    import torch
    ex, ey, ez = voxel_edges(lo, hi, shape)
    nx, ny, nz = (int(s) for s in shape)
    out = np.zeros((nz, ny, nx, 8), np.float32)
    out[..., 0], out[..., 4] = ex[None, None, :-1], ex[None, None, 1:]
    out[..., 1], out[..., 5] = ey[None, :-1, None], ey[None, 1:, None]
    out[..., 2], out[..., 6] = ez[:-1, None, None], ez[1:, None, None]
    rows = torch.from_numpy(out.reshape(-1, 8))
    return rows if device is None else rows.to(device)


def occupancy_grid(raw, lo, hi, shape, stream=None):
    """A bool tensor [nz, ny, nx] on the scene's device: which voxels of the regular grid of shape = (nx, ny, nz) over [lo, hi] a
    surface of the scene touches (voxel_rows through the any-overlap call)."""
    import torch
    nx, ny, nz = (int(s) for s in shape)
    rows = voxel_rows(lo, hi, shape, device=torch.device("cuda", raw.device))
    counts = count_overlaps(raw, rows, any_overlap=True, stream=stream)
    return (counts != 0).reshape(nz, ny, nx)
