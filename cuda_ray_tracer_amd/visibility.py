"""Hemisphere visibility at surface points: include/mirt_visibility.h restated for ctypes, and the calls over it.

mirt_visibility.h is an extension header like mirt_light.h: binding.SIGNATURES stays the table of include/mirt.h,
lighting.LIGHT_SIGNATURES the table of mirt_light.h, and the one entry point more lives here.  tests/test_extension_abi.py holds
the table to the header the way tests/test_binding_header.py holds binding.py to mirt.h.

Needs ctypes only: torch and numpy are imported when a call needs them.
"""
from . import binding
from .binding import _check, _int, _i64, _u32, _vp, _f

# symbol -> (restype, argtypes): every entry point of include/mirt_visibility.h, in the header's order
VISIBILITY_SIGNATURES = {
    "mirt_hemisphere_visibility": (_int, [_vp, _vp, _i64, _vp, _int, _vp, _f, _vp, _vp, _u32, _vp]),
}

GOLDEN_ANGLE = 2.399963229728653


def lib():
    """binding.lib() with the signatures of mirt_visibility.h applied."""
    return binding.extension_lib(VISIBILITY_SIGNATURES)


def hemisphere_visibility(raw, d_features, d_dirs, d_out, d_vis_mask=None, d_rot=None, radius=float("inf"), stream=None):
    """mirt_hemisphere_visibility: for each row of d_features (float32 [n, 8]: hit_features' rows, or pack_features' for points of
    the caller's own) the directions of d_dirs (float32 [K, 4], 1 <= K <= 64: (lx, ly, lz, w), z along the row's normal) that no
    geometry blocks within `radius`, traced on the device.  d_out (float32 [n, 4]) receives the sum over the visible directions
    of w times the unit direction, and of w: the unnormalised bent normal and the visible weight (zeros for a row that is no
    hit); d_vis_mask (int64 [n], read as uint64), if given, bit k set when direction k is visible; d_rot (float32 [n, 2]), if
    given, holds the cosine and sine of a rotation of the table about the normal for each row.  All tensors contiguous, distinct
    and on the scene's device.  Asynchronous on `stream` (default: torch's current stream)."""
    from . import api
    tensors = api._tensors((d_features, "d_features", api._F32, [None, 8]), (d_dirs, "d_dirs", api._F32, [None, 4]))
    n, k = d_features.shape[0], d_dirs.shape[0]
    if not 1 <= k <= 64:
        raise ValueError(f"d_dirs has shape {list(d_dirs.shape)}; expected 1 to 64 rows")
    tensors += api._tensors((d_out, "d_out", api._F32, [n, 4]))
    if d_vis_mask is not None:
        tensors += api._tensors((d_vis_mask, "d_vis_mask", ("int64",), [n]))
    if d_rot is not None:
        tensors += api._tensors((d_rot, "d_rot", api._F32, [n, 2]))
    api._on_device(tensors, raw.device)
    _check(lib().mirt_hemisphere_visibility(raw._h, api._ptr(d_features), n, api._ptr(d_dirs), k, api._ptr(d_rot), float(radius),
                                            api._ptr(d_out), api._ptr(d_vis_mask), 0, api._stream_ptr(stream)))


def _placed(a, device):
    """The numpy array itself without a device, else a torch tensor of it there."""
    if device is None:
        return a
    import torch
    return torch.from_numpy(a).to(device)


def cosine_directions(k, device=None):
    """float32 [k, 4]: k directions over the hemisphere about +z with a density proportional to the cosine (a golden spiral on
    the unit disc, lifted), each with the weight 1 / k, so that the visible weight estimates the cosine-weighted visible
    fraction.  Computed in float64 and cast; the same table for the same k.  A numpy array, or with `device` a torch tensor
    there."""
    import numpy as np
    if not 1 <= int(k) <= 64:
        raise ValueError(f"k is {k}; expected 1 to 64")
    i = np.arange(int(k), dtype=np.float64)
    u = (i + 0.5) / k
    r = np.sqrt(u)
    phi = 0.3 + i * GOLDEN_ANGLE
    rows = np.stack([r * np.cos(phi), r * np.sin(phi), np.sqrt(1.0 - u), np.full(int(k), 1.0 / k)], axis=1)
    return _placed(np.ascontiguousarray(rows, dtype=np.float32), device)


def rotations(n, seed, device=None):
    """float32 [n, 2]: (cos, sin) of n angles drawn uniformly from [0, 2 pi) by numpy.random.default_rng(seed) -- d_rot for
    hemisphere_visibility, one turn of the direction table per row.  A numpy array, or with `device` a torch tensor there."""
    import numpy as np
    angle = np.random.default_rng(seed).random(int(n)) * (2.0 * np.pi)
    return _placed(np.ascontiguousarray(np.stack([np.cos(angle), np.sin(angle)], axis=1), dtype=np.float32), device)


def _frame_directions(directions, n, rotate_seed, device):
    """The direction table and the rotations of a frame call, on `device`: cosine_directions(directions) for an int, else the
    caller's float32 [K, 4] table; rotations(n, rotate_seed), or None without a seed."""
    import torch
    if isinstance(directions, int):
        dirs = cosine_directions(directions, device)
    else:
        dirs = torch.as_tensor(directions, dtype=torch.float32).to(device).contiguous()
    return dirs, (rotations(n, rotate_seed, device) if rotate_seed is not None else None)


def ambient_occlusion_frame(raw, width, height, spp=0, directions=16, radius=float("inf"), rotate_seed=None, want_mask=False, params=None,
                            stream=None):
    """The hemisphere visibility at the first hit of every pixel's camera ray: camera_rays (sample 0 of every pixel of a
    width x height frame at `spp`, or of the part `params` selects) -> trace_rays -> hit_features -> hemisphere_visibility with
    cosine_directions(directions) (or `directions` a float32 [K, 4] table of the caller's) and, with `rotate_seed`,
    rotations(n, rotate_seed).  Returns (out float32 [n, 4], mask int64 [n] or None, features float32 [n, 8]); out[:, 3] of a
    hit row is one minus its ambient occlusion."""
    import torch
    from . import api
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
        hemisphere_visibility(raw, features, dirs, out, mask, rot, radius, stream=s)
    return out, mask, features
