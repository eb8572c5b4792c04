"""Multi-hit ray queries on a built scene: include/mirt_multihit.h restated for ctypes, and the calls over it.

mirt_multihit.h is an extension header like mirt_light.h, mirt_visibility.h, mirt_indirect.h and mirt_closest.h: binding.SIGNATURES
stays the table of include/mirt.h, the other modules' tables those of their headers, and the one entry point more lives here.
tests/test_extension_abi.py holds the table to the header the way tests/test_binding_header.py holds binding.py to mirt.h.

Needs ctypes only: torch and numpy are imported when a call needs them.
"""
from . import binding
from .binding import _check, _int, _i64, _u32, _vp

MIRT_MULTIHIT_MAX_K = 8

# symbol -> (restype, argtypes): every entry point of include/mirt_multihit.h, in the header's order
MULTIHIT_SIGNATURES = {
    "mirt_trace_rays_multi": (_int, [_vp, _vp, _i64, _int, _vp, _vp, _u32, _vp]),
}


def lib():
    """binding.lib() with the signatures of mirt_multihit.h applied."""
    return binding.extension_lib(MULTIHIT_SIGNATURES)


def trace_rays_multi(raw, d_rays, d_hits, d_counts=None, stream=None):
    """mirt_trace_rays_multi: for every ray of d_rays (float32 [n, 8], MirtRay rows: pack_rays) the k nearest of all the planes,
    spheres and triangles it meets before its tmax, nearest first, into d_hits (a 4-byte dtype, [n, k, 6], k read from the shape, at
    most 8; MirtHit records: unpack_hits reads d_hits.reshape(-1, 6)) -- slots past a ray's hits are misses (t = -1) -- and, if
    d_counts (int32 or uint32 [n]) is given, the number of all its hits, which may exceed k.  d_hits None: a count-only call.  All
    tensors contiguous, distinct and on the scene's device.  Asynchronous on `stream` (default: torch's current stream)."""
    from . import api
    tensors, n, k = api._record_tensors((d_rays, "d_rays", 8), d_hits, d_counts, max_k=MIRT_MULTIHIT_MAX_K)
    api._on_device(tensors, raw.device)
    _check(lib().mirt_trace_rays_multi(raw._h, api._ptr(d_rays), n, k, api._ptr(d_hits), api._ptr(d_counts), 0, api._stream_ptr(stream)))


def count_hits(raw, d_rays, stream=None):
    """The number of hits of every ray of d_rays (float32 [n, 8]) before its tmax, as a new int32 [n] tensor on the rays' device:
    trace_rays_multi with k = 0."""
    from . import api
    counts = api._count_tensor((d_rays, "d_rays", 8))
    trace_rays_multi(raw, d_rays, None, counts, stream=stream)
    return counts
