"""include_ext2/mirt_overlap_tris.h restated in numpy float32, one operation per line: for every row (a caller's triangle) the test of
every plane, sphere and triangle of the scene -- a brute force over the scene's arrays, never over a tree --, the counts, and the
lists in the header's order: the planes by index, then the spheres and triangles in the scene's leaf order, which is the oracle
tree's refs (overlap_list_ref.column_order).  Offsets and the bounded fill are overlap_list_ref's.

Scenes are pyscene.PyScene.arrays() dictionaries (spheres, triangles, planes in file order).  Rows are float32 [n, 9]: a, b, c."""
import numpy as np

import closest_ref as cr
import overlap_list_ref as olr

f32 = np.float32
u32 = np.uint32
ZERO = f32(0.0)
AXES = 17
_dot = cr._dot


def _cross(u, v):
    x1 = u[..., 1] * v[..., 2]
    x2 = u[..., 2] * v[..., 1]
    y1 = u[..., 2] * v[..., 0]
    y2 = u[..., 0] * v[..., 2]
    z1 = u[..., 0] * v[..., 1]
    z2 = u[..., 1] * v[..., 0]
    return np.stack([x1 - x2, y1 - y2, z1 - z2], axis=-1)


def _min3(x, y, z):
    return np.fmin(np.fmin(x, y), z)


def _max3(x, y, z):
    return np.fmax(np.fmax(x, y), z)


def _finite(x):
    return (x - x) == 0      # (x - x is 0 for a finite x and NaN for an infinity or a NaN)


# ---- the row ----------------------------------------------------------------------------------------------------------------------
def row_quantities(rows):
    """(a, b, c, ub, uc, lo, hi), float32 [n, 3] each: the vertices as given, the edges from a, the exact bounds."""
    rows = np.ascontiguousarray(rows, f32).reshape(-1, 9)
    a, b, c = (np.ascontiguousarray(rows[:, k:k + 3]) for k in (0, 3, 6))
    with np.errstate(all="ignore"):
        ub = b - a
        uc = c - a
        lo = _min3(a, b, c)
        hi = _max3(a, b, c)
    cr._assert_f32(ub, uc, lo, hi)
    return a, b, c, ub, uc, lo, hi


def live_rows(rows):
    a, b, c, ub, uc, _, _ = row_quantities(rows)
    with np.errstate(all="ignore"):
        n1 = _cross(ub, uc)
        m1 = _dot(n1, n1)
        return np.all(_finite(a), axis=1) & np.all(_finite(b), axis=1) & np.all(_finite(c), axis=1) & _finite(m1) & (m1 > 0)


# ---- the three tests, each broadcast over [..., 3] ------------------------------------------------------------------------------------
def plane_passes(a, b, c, nor, point):
    N = cr._normalize(nor)
    sa = _dot(N, a - point)
    sb = _dot(N, b - point)
    sc = _dot(N, c - point)
    cr._assert_f32(sa, sb, sc)
    return (_min3(sa, sb, sc) <= 0) & (_max3(sa, sb, sc) >= 0) & (sa == sa) & (sb == sb) & (sc == sc)


def sphere_box_meets(lo, hi, ctr, rs):
    """Clause (0): the builder's box of the sphere against the row's bounds."""
    r = rs[..., None]
    lower = ctr - r
    upper = ctr + r
    ordered = lower <= upper
    smin = np.where(ordered, lower, upper)
    smax = np.where(ordered, upper, lower)
    return np.all((smin <= hi) & (smax >= lo), axis=-1)


def sphere_distances(a, ub, uc, ctr):
    """(dn, df) of clauses (1) and (2)."""
    C = ctr - a
    zero = np.zeros_like(ub)
    P = cr.triangle_point(C, zero, ub, uc)
    dn = cr._length(C - P)
    df = _max3(cr._length(zero - C), cr._length(ub - C), cr._length(uc - C))
    cr._assert_f32(dn, df)
    return dn, df


def sphere_passes(lo, hi, a, ub, uc, ctr, rs):
    dn, df = sphere_distances(a, ub, uc, ctr)
    return sphere_box_meets(lo, hi, ctr, rs) & (dn <= rs) & (df >= rs)


def triangle_axes(ub, uc, P, Q, R):
    """The seventeen axes in the header's order (a list of arrays [..., 3])."""
    f0 = Q - P
    f1 = R - Q
    f2 = R - P
    e = (ub, uc - ub, uc)
    f = (f0, f1, f2)
    n1 = _cross(ub, uc)
    n2 = _cross(f0, f2)
    return [n1, n2] + [_cross(e[i], f[j]) for i in range(3) for j in range(3)] + [_cross(n1, e[i]) for i in range(3)] + [_cross(n2, f[j]) for j in range(3)]


def axis_separates(L, ub, uc, P, Q, R):
    r1 = _dot(L, ub)
    r2 = _dot(L, uc)
    s0 = _dot(L, P)
    s1 = _dot(L, Q)
    s2 = _dot(L, R)
    cr._assert_f32(r1, s0)
    return (_max3(ZERO, r1, r2) < _min3(s0, s1, s2)) | (_max3(s0, s1, s2) < _min3(ZERO, r1, r2))


def triangle_clauses(lo, hi, a, ub, uc, p, q, r):
    """(bounds meet, the scene triangle has area, separates [17, ...]) of the header's clauses (i), (ii), (iii)."""
    near = np.all((_min3(p, q, r) <= hi) & (_max3(p, q, r) >= lo), axis=-1)
    P = p - a
    Q = q - a
    R = r - a
    n2 = _cross(Q - P, R - P)
    m2 = _dot(n2, n2)
    area = _finite(m2) & (m2 > 0)
    axes = triangle_axes(ub, uc, P, Q, R)
    assert len(axes) == AXES
    sep = np.stack([np.broadcast_to(axis_separates(L, ub, uc, P, Q, R), near.shape) for L in axes])
    return near, area, sep


def triangle_passes(lo, hi, a, ub, uc, p, q, r, axes=AXES):
    """The header's test; axes < 17: with the first `axes` axes alone (the negative control of the coplanar case)."""
    near, area, sep = triangle_clauses(lo, hi, a, ub, uc, p, q, r)
    return near & area & ~np.any(sep[:axes], axis=0)


# ---- all candidates of a scene --------------------------------------------------------------------------------------------------------
def passes(arrays, rows, axes=AXES, chunk=256):
    """(spheres [n, Ns], triangles [n, Nt], planes [n, Np]), bool: the admitted candidates of every row (a dead row: none)."""
    a, b, c, ub, uc, lo, hi = row_quantities(rows)
    live = live_rows(rows)
    n = len(a)
    S, T, Pl = arrays["spheres"], arrays["triangles"], arrays["planes"]
    ps, pt, pp = np.zeros((n, len(S)), bool), np.zeros((n, len(T)), bool), np.zeros((n, len(Pl)), bool)
    with np.errstate(all="ignore"):
        for s in range(0, n, chunk):
            k = slice(s, s + chunk)
            A, B, Cc, UB, UC, LO, HI = (x[k, None] for x in (a, b, c, ub, uc, lo, hi))
            if len(S):
                ps[k] = sphere_passes(LO, HI, A, UB, UC, S["c"][None].astype(f32), S["r"][None].astype(f32))
            if len(T):
                pt[k] = triangle_passes(LO, HI, A, UB, UC, T["p0"][None].astype(f32), T["p1"][None].astype(f32), T["p2"][None].astype(f32), axes=axes)
            if len(Pl):
                pp[k] = plane_passes(A, B, Cc, Pl["nor"][None].astype(f32), Pl["point"][None].astype(f32))
    return ps & live[:, None], pt & live[:, None], pp & live[:, None]


def admitted(arrays, rows):
    """bool [n, Ns + Nt + Np]: the columns are the spheres, the triangles, the planes, each in file order."""
    return np.concatenate(passes(arrays, rows), axis=1)


def counts(arrays, rows, adm=None):
    adm = admitted(arrays, rows) if adm is None else adm
    return adm.sum(axis=1).astype(u32)


def lists(arrays, rows, refs, adm=None):
    """(offsets int64 [n + 1], words uint32 [offsets[n]]): every row's admitted set in the header's order, the segments exact."""
    adm = admitted(arrays, rows) if adm is None else adm
    cols, words = olr.column_order(arrays, refs)
    adm = adm[:, cols]
    return olr.offsets_of(adm.sum(axis=1)), np.ascontiguousarray(np.broadcast_to(words[None, :], adm.shape)[adm], u32)


def scene_rows(arrays):
    """The scene's own triangles as rows: what mirt_scene_get_triangles writes."""
    T = arrays["triangles"]
    return np.ascontiguousarray(np.concatenate([T["p0"], T["p1"], T["p2"]], axis=1), f32).reshape(-1, 9)
