"""Indirect light at surface points: include/mirt_indirect.h restated for ctypes, and the calls over it.

mirt_indirect.h is an extension header like mirt_light.h and mirt_visibility.h: binding.SIGNATURES stays the table of
include/mirt.h, lighting.LIGHT_SIGNATURES and visibility.VISIBILITY_SIGNATURES the tables of the other two, and the one entry point
more lives here.  tests/test_extension_abi.py holds the table to the header the way tests/test_binding_header.py holds binding.py to
mirt.h.

Needs ctypes only: torch and numpy are imported when a call needs them.
"""
from . import binding
from .binding import _check, _int, _i64, _u32, _vp, _f

# symbol -> (restype, argtypes): every entry point of include/mirt_indirect.h, in the header's order
INDIRECT_SIGNATURES = {
    "mirt_indirect_light": (_int, [_vp, _vp, _i64, _vp, _int, _vp, _f, _vp, _vp, _u32, _vp]),
}


def lib():
    """binding.lib() with the signatures of mirt_indirect.h applied."""
    return binding.extension_lib(INDIRECT_SIGNATURES)


def indirect_light(raw, d_features, d_dirs, d_out, d_hit_mask=None, d_rot=None, radius=float("inf"), stream=None):
    """mirt_indirect_light: for each row of d_features (float32 [n, 8]: hit_features' rows, or pack_features' for points of the
    caller's own) the light that arrives by one diffuse bounce along the directions of d_dirs (float32 [K, 4], 1 <= K <= 64:
    (lx, ly, lz, w), z along the row's normal): every direction is traced to its closest hit within `radius`, the hit point
    receives direct_light's raw sum of the scene's lights times the diffuse weight of its material, and the terms are summed
    with the weights w.  d_out (float32 [n, 4]) receives (r, g, b) and, in its last channel, the weight of the directions that
    found nothing -- hemisphere_visibility's visible weight (zeros for a row that is no hit); d_hit_mask (int64 [n], read as
    uint64), if given, bit k set when direction k hit something; d_rot (float32 [n, 2]), if given, holds the cosine and sine of a
    rotation of the table about the normal for each row.  All tensors contiguous, distinct and on the scene's device.
    Asynchronous on `stream` (default: torch's current stream)."""
    from . import api
    tensors = api._tensors((d_features, "d_features", api._F32, [None, 8]), (d_dirs, "d_dirs", api._F32, [None, 4]))
    n, k = d_features.shape[0], d_dirs.shape[0]
    if not 1 <= k <= 64:
        raise ValueError(f"d_dirs has shape {list(d_dirs.shape)}; expected 1 to 64 rows")
    tensors += api._tensors((d_out, "d_out", api._F32, [n, 4]))
    if d_hit_mask is not None:
        tensors += api._tensors((d_hit_mask, "d_hit_mask", ("int64",), [n]))
    if d_rot is not None:
        tensors += api._tensors((d_rot, "d_rot", api._F32, [n, 2]))
    api._on_device(tensors, raw.device)
    _check(lib().mirt_indirect_light(raw._h, api._ptr(d_features), n, api._ptr(d_dirs), k, api._ptr(d_rot), float(radius),
                                     api._ptr(d_out), api._ptr(d_hit_mask), 0, api._stream_ptr(stream)))


def indirect_light_frame(raw, width, height, spp=0, directions=16, radius=float("inf"), rotate_seed=None, want_mask=False, params=None,
                         stream=None):
    """The one-bounce indirect light at the first hit of every pixel's camera ray: camera_rays (sample 0 of every pixel of a
    width x height frame at `spp`, or of the part `params` selects) -> trace_rays -> hit_features -> indirect_light with
    visibility.cosine_directions(directions) (or `directions` a float32 [K, 4] table of the caller's) and, with `rotate_seed`,
    visibility.rotations(n, rotate_seed).  Returns (out float32 [n, 4], mask int64 [n] or None, features float32 [n, 8]); with
    the cosine table out[:, :3] estimates the bounced irradiance over pi."""
    import torch
    from . import api
    from .visibility import _frame_directions
    p = api._frame(params, width, height, spp)
    n = api.num_pixels(p)
    with api._device_and_stream(raw.device, stream) as (dev, s):
        dirs, rot = _frame_directions(directions, n, rotate_seed, dev)
        rays = torch.empty((n, 8), dtype=torch.float32, device=dev)
        hits = torch.empty((n, 6), dtype=torch.int32, device=dev)
        features = torch.empty((n, 8), dtype=torch.float32, device=dev)
        out = torch.empty((n, 4), dtype=torch.float32, device=dev)
        mask = torch.empty(n, dtype=torch.int64, device=dev) if want_mask else None
        api._primary_features(raw, p, rays, hits, features, s)
        indirect_light(raw, features, dirs, out, mask, rot, radius, stream=s)
    return out, mask, features
