"""Contact queries on a built scene: include_ext/mirt_contacts.h restated for ctypes, and the calls over it.

mirt_contacts.h is an extension header like mirt_closest.h and mirt_multihit.h: binding.SIGNATURES stays the table of
include/mirt.h, the other modules' tables those of their headers, and the one entry point more lives here.
tests/test_extension_abi.py holds the table to the header the way tests/test_binding_header.py holds binding.py to mirt.h.

Needs ctypes only: torch and numpy are imported when a call needs them.  The rows are closest.pack_points', the records are read
by api.unpack_hits (d_hits.reshape(-1, 6)).
"""
from . import binding
from .binding import _check, _int, _i64, _u32, _vp

MIRT_CONTACTS_MAX_K = 8

# symbol -> (restype, argtypes): every entry point of include_ext/mirt_contacts.h, in the header's order
CONTACTS_SIGNATURES = {
    "mirt_closest_points_multi": (_int, [_vp, _vp, _i64, _int, _vp, _vp, _vp, _u32, _vp]),
}


def lib():
    """binding.lib() with the signatures of mirt_contacts.h applied."""
    return binding.extension_lib(CONTACTS_SIGNATURES)


def closest_points_multi(raw, d_points, d_hits, d_counts=None, d_features=None, stream=None):
    """mirt_closest_points_multi: for each row (qx, qy, qz, R) of d_points (float32 [n, 4]; pack_points makes them) the k nearest of
    all the planes, spheres and triangles nearer than R, nearest first, into d_hits (int32 [n, k, 6], k read from the shape, at most
    8; MirtHit records: unpack_hits reads d_hits.reshape(-1, 6)) -- slots past a row's surfaces are misses (t = -1) -- and, if
    d_counts (int32 [n]) is given, the number of all of them, which may exceed k.  d_features (float32 [n, k, 8]), if given,
    receives each record's closest point and normal in hit_features' layout.  d_hits None: a count-only call.  All tensors
    contiguous, distinct and on the scene's device.  Asynchronous on `stream` (default: torch's current stream)."""
    from . import api
    tensors, n, k = api._record_tensors((d_points, "d_points", 4), d_hits, d_counts, d_features, max_k=MIRT_CONTACTS_MAX_K)
    api._on_device(tensors, raw.device)
    _check(lib().mirt_closest_points_multi(raw._h, api._ptr(d_points), n, k, api._ptr(d_hits), api._ptr(d_counts), api._ptr(d_features), 0,
                                           api._stream_ptr(stream)))


def count_within(raw, d_points, d_counts=None, stream=None):
    """The number of surfaces nearer than R to every row (qx, qy, qz, R) of d_points (float32 [n, 4]), into d_counts (int32 [n]; a new
    tensor on the rows' device if None), which is returned: closest_points_multi with k = 0.  A count with R = inf visits the
    whole scene."""
    from . import api
    d_counts = api._count_tensor((d_points, "d_points", 4), d_counts)
    closest_points_multi(raw, d_points, None, d_counts, stream=stream)
    return d_counts
