"""Closest-point queries on a built scene: include/mirt_closest.h restated for ctypes, and the calls over it.

mirt_closest.h is an extension header like mirt_light.h, mirt_visibility.h and mirt_indirect.h: binding.SIGNATURES stays the table
of include/mirt.h, the other modules' tables those of their headers, and the one entry point more lives here.
tests/test_extension_abi.py holds the table to the header the way tests/test_binding_header.py holds binding.py to mirt.h.

Needs ctypes only: torch and numpy are imported when a call needs them.
"""
from . import binding
from .binding import _check, _int, _i64, _u32, _vp

# symbol -> (restype, argtypes): every entry point of include/mirt_closest.h, in the header's order
CLOSEST_SIGNATURES = {
    "mirt_closest_points": (_int, [_vp, _vp, _i64, _vp, _vp, _u32, _vp]),
}


def lib():
    """binding.lib() with the signatures of mirt_closest.h applied."""
    return binding.extension_lib(CLOSEST_SIGNATURES)


def closest_points(raw, d_points, d_hits, d_features=None, stream=None):
    """mirt_closest_points: for each row (qx, qy, qz, R) of d_points (float32 [n, 4]; pack_points makes them) the plane, sphere or
    triangle of the scene nearest to q and nearer than R, found on the device.  d_hits (int32 [n, 6], MirtHit records: unpack_hits
    reads them) receives the distance, the kind and index as trace_rays reports them, and the surface normal turned towards q --
    t = -1 and kind 0 for a row with nothing within R; d_features (float32 [n, 8]), if given, the closest point and that normal in
    hit_features' layout -- rows direct_light, hemisphere_visibility and indirect_light take as they are.  All tensors contiguous,
    distinct and on the scene's device.  Asynchronous on `stream` (default: torch's current stream)."""
    from . import api
    tensors = api._tensors((d_points, "d_points", api._F32, [None, 4]))
    n = d_points.shape[0]
    tensors += api._tensors((d_hits, "d_hits", api._HIT, [n, 6]))
    if d_features is not None:
        tensors += api._tensors((d_features, "d_features", api._F32, [n, 8]))
    api._on_device(tensors, raw.device)
    _check(lib().mirt_closest_points(raw._h, api._ptr(d_points), n, api._ptr(d_hits), api._ptr(d_features), 0, api._stream_ptr(stream)))


def pack_points(xyz, radius=float("inf"), device=None):
    """float32 [n, 4] rows (qx, qy, qz, R) for closest_points from points [n, 3] (a torch tensor, or anything torch.as_tensor
    takes) and a search radius: one number for all rows, or [n].  On `device` if given, else where xyz is."""
    import torch
    xyz = torch.as_tensor(xyz, dtype=torch.float32)
    if device is not None:
        xyz = xyz.to(device)
    if xyz.dim() != 2 or xyz.shape[1] != 3:
        raise ValueError(f"xyz has shape {list(xyz.shape)}; expected [n, 3]")
    n = xyz.shape[0]
    radius = torch.as_tensor(radius, dtype=torch.float32).to(xyz.device)
    if radius.dim() > 1 or (radius.dim() == 1 and radius.shape[0] != n):
        raise ValueError(f"radius has shape {list(radius.shape)}; expected a number or [n]")
    rows = torch.empty((n, 4), dtype=torch.float32, device=xyz.device)
    rows[:, 0:3] = xyz
    rows[:, 3] = radius
    return rows
