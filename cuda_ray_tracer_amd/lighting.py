"""Direct light at surface points: include/mirt_light.h restated for ctypes, and the calls over it.

mirt_light.h is an extension header: binding.SIGNATURES stays the table of include/mirt.h, and the one entry point more lives
here with its constant.  tests/test_extension_abi.py holds both to the header the way tests/test_binding_header.py holds binding.py
to mirt.h.

Needs ctypes only: torch is imported when a call needs it, numpy not at all.
"""
from . import binding
from .binding import _check, _int, _i64, _u32, _vp

MIRT_LIGHT_RAW = 1

# symbol -> (restype, argtypes): every entry point of include/mirt_light.h, in the header's order
LIGHT_SIGNATURES = {
    "mirt_direct_light": (_int, [_vp, _vp, _i64, _vp, _vp, _u32, _vp]),
}


def lib():
    """binding.lib() with the signatures of mirt_light.h applied."""
    return binding.extension_lib(LIGHT_SIGNATURES)


def direct_light(raw, d_features, d_out, d_lit_mask=None, raw_units=False, stream=None):
    """mirt_direct_light: the light of every sun and bulb of the scene that reaches each row of d_features (float32 [n, 8]:
    hit_features' rows, or pack_features' for points of the caller's own), shadow-tested on the device, into d_out (float32
    [n, 4]: r, g, b and 1, zeros for a row that is no hit) and, if given, d_lit_mask (int64 [n], read as uint64: bit li set when
    light li -- suns first, then bulbs -- reaches the point).  raw_units: MIRT_LIGHT_RAW, the terms before the scene's exposure.
    All tensors contiguous, distinct and on the scene's device.  Asynchronous on `stream` (default: torch's current stream)."""
    from . import api
    tensors = api._tensors((d_features, "d_features", api._F32, [None, 8]))
    n = d_features.shape[0]
    tensors += api._tensors((d_out, "d_out", api._F32, [n, 4]))
    if d_lit_mask is not None:
        tensors += api._tensors((d_lit_mask, "d_lit_mask", ("int64",), [n]))
    api._on_device(tensors, raw.device)
    _check(lib().mirt_direct_light(raw._h, api._ptr(d_features), n, api._ptr(d_out), api._ptr(d_lit_mask), MIRT_LIGHT_RAW if raw_units else 0,
                                   api._stream_ptr(stream)))


def pack_features(points, normals, hit=None):
    """float32 [n, 8] feature rows (Px, Py, Pz, hit) (nx, ny, nz, 0) from points [n, 3], normals [n, 3] (any length: the query
    normalises them, and offsets the shadow rays' origin by 0.001 of the normal as given) and hit (None: every row is a hit; or
    [n], non-zero = hit), on the points' device."""
    import torch
    points = torch.as_tensor(points, dtype=torch.float32)
    if points.dim() != 2 or points.shape[1] != 3:
        raise ValueError(f"points has shape {list(points.shape)}; expected [n, 3]")
    normals = torch.as_tensor(normals, dtype=torch.float32, device=points.device)
    if list(normals.shape) != list(points.shape):
        raise ValueError(f"normals has shape {list(normals.shape)}; expected {list(points.shape)}")
    n = points.shape[0]
    out = torch.zeros((n, 8), dtype=torch.float32, device=points.device)
    out[:, 0:3] = points
    out[:, 3] = 1.0 if hit is None else (torch.as_tensor(hit, device=points.device).reshape(n) != 0).to(torch.float32)
    out[:, 4:7] = normals
    return out


def direct_light_frame(raw, width, height, spp=0, want_mask=True, raw_units=False, params=None, stream=None):
    """The direct light at the first hit of every pixel's camera ray: camera_rays (sample 0 of every pixel of a width x height
    frame at `spp`, or of the part `params` selects) -> trace_rays -> hit_features -> direct_light.  Returns (out float32 [n, 4],
    lit_mask int64 [n] or None, features float32 [n, 8]).  On a matte-white scene with gi 0, out at spp 0 is render's d_float."""
    import torch
    from . import api
    p = api._frame(params, width, height, spp)
    n = api.num_pixels(p)
    with api._device_and_stream(raw.device, stream) as (dev, s):
        rays = torch.empty((n, 8), dtype=torch.float32, device=dev)
        hits = torch.empty((n, 6), dtype=torch.int32, device=dev)
        features = torch.empty((n, 8), dtype=torch.float32, device=dev)
        out = torch.empty((n, 4), dtype=torch.float32, device=dev)
        mask = torch.empty(n, dtype=torch.int64, device=dev) if want_mask else None
        api._primary_features(raw, p, rays, hits, features, s)
        direct_light(raw, features, out, mask, raw_units=raw_units, stream=s)
    return out, mask, features
