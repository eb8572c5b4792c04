"""Sphere casts on a built scene: include_ext/mirt_spherecast.h restated for ctypes, and the calls over it.

mirt_spherecast.h is an extension header like mirt_closest.h and mirt_contacts.h: binding.SIGNATURES stays the table of
include/mirt.h, the other modules' tables those of their headers, and the one entry point more lives here.
tests/test_extension_abi.py holds the table to the header the way tests/test_binding_header.py holds binding.py to mirt.h.

Needs ctypes only: torch and numpy are imported when a call needs them.  The records are read by api.unpack_hits.
"""
from . import binding
from .binding import _check, _int, _i64, _u32, _vp

MIRT_CAST_ANY_HIT = 1

# symbol -> (restype, argtypes): every entry point of include_ext/mirt_spherecast.h, in the header's order
SPHERECAST_SIGNATURES = {
    "mirt_cast_spheres": (_int, [_vp, _vp, _i64, _vp, _vp, _u32, _vp]),
}


def lib():
    """binding.lib() with the signatures of mirt_spherecast.h applied."""
    return binding.extension_lib(SPHERECAST_SIGNATURES)


def cast_spheres(raw, casts, hits, features=None, any_hit=False, stream=None):
    """mirt_cast_spheres: for each row (ox, oy, oz, tmax) (dx, dy, dz, r) of casts (float32 [n, 8]; pack_casts makes them) the first
    plane, sphere or triangle that a ball of radius r touches while its centre travels from o along d, nearer than tmax, found on
    the device.  hits (int32 [n, 6], MirtHit records: unpack_hits reads them) receives the distance the centre travels (0: the ball
    touches at the start), the kind and index as trace_rays reports them, and the contact normal, which points from the surface to
    the centre -- t = -1 and kind 0 for a row that touches nothing; features (float32 [n, 8]), if given, the contact point and
    that normal in hit_features' layout -- rows direct_light, hemisphere_visibility and indirect_light take as they are.  With
    any_hit the record is that of some contact before tmax, not necessarily the first.  All tensors contiguous, distinct and on
    the scene's device.  Asynchronous on `stream` (default: torch's current stream)."""
    from . import api
    tensors = api._tensors((casts, "casts", api._F32, [None, 8]))
    n = casts.shape[0]
    tensors += api._tensors((hits, "hits", api._HIT, [n, 6]))
    if features is not None:
        tensors += api._tensors((features, "features", api._F32, [n, 8]))
    api._on_device(tensors, raw.device)
    _check(lib().mirt_cast_spheres(raw._h, api._ptr(casts), n, api._ptr(hits), api._ptr(features), MIRT_CAST_ANY_HIT if any_hit else 0,
                                   api._stream_ptr(stream)))


def pack_casts(o, d, tmax=float("inf"), r=0.0):
    """float32 [n, 8] rows (ox, oy, oz, tmax) (dx, dy, dz, r) for cast_spheres from origins [n, 3] (or [3]), directions [n, 3] (any
    non-zero length), tmax and the radius r (each a number or [n]), on the directions' device."""
    import torch
    d = torch.as_tensor(d, dtype=torch.float32)
    if d.dim() != 2 or d.shape[1] != 3:
        raise ValueError(f"d has shape {list(d.shape)}; expected [n, 3]")
    n = d.shape[0]
    o = torch.as_tensor(o, dtype=torch.float32, device=d.device)
    if tuple(o.shape) not in ((3,), (n, 3)):
        raise ValueError(f"o has shape {list(o.shape)}; expected [3] or [{n}, 3]")
    columns = []
    for x, name in ((tmax, "tmax"), (r, "r")):
        x = torch.as_tensor(x, dtype=torch.float32, device=d.device)
        if x.dim() > 1 or (x.dim() == 1 and x.shape[0] != n):
            raise ValueError(f"{name} has shape {list(x.shape)}; expected a number or [{n}]")
        columns.append(x)
    out = torch.empty((n, 8), dtype=torch.float32, device=d.device)
    out[:, 0:3] = o
    out[:, 3] = columns[0]
    out[:, 4:7] = d
    out[:, 7] = columns[1]
    return out
