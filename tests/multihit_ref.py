"""include/mirt_multihit.h restated in numpy float32, one rounding per operation, vectorised over rays x nodes: the three primitive
tests, the box test and its reachability from the root, the admitted set S, its (t, class, index) order, the records, the counts
and the per-ray `regular` flag.  Then the same set by a brute force over the scene's arrays, with no tree.

Scenes are dictionaries of structured arrays `spheres` (c, r), `triangles` (p0, nor, e1, e2), `planes` (nor, point) in file order:
pyscene.PyScene.arrays(), or StlConfig.array() of each.  The tree is oracle_lib.NODE records (node 0 the root; a leaf has count 1
and its prim_offset is its sorted position) and the sorted (type, id) pairs: OracleScene.nodes() / refs(), or RawConfig.tree().
Rays are float32 [n, 8]: (o, tmax), (d, pad)."""
import numpy as np

f32 = np.float32
u32 = np.uint32
KIND_SPHERE, KIND_TRIANGLE, KIND_PLANE = 1, 2, 3
MISS = np.array([f32(-1.0).view(u32), 0, 0, 0, 0, 0], u32)
EPSILON = f32(0.001)


def _dot(a, b):
    x = a[..., 0] * b[..., 0]
    y = a[..., 1] * b[..., 1]
    z = a[..., 2] * b[..., 2]
    s = x + y
    return s + z


def _normalize(v):
    """vec3::normalize: (0, 0, 0) when the length is below 1e-6, else each component times 1 / length."""
    mag = np.sqrt(_dot(v, v))
    inv = f32(1.0) / mag
    out = v * inv[..., None]
    return np.where((np.abs(mag) < f32(1e-6))[..., None], f32(0.0), out)


def _f32(*arrays):
    for a in arrays:
        assert a.dtype == f32, a.dtype


def split(rays):
    """(o [n, 3], d [n, 3] normalised, tmax [n], live [n]) of ray rows."""
    rays = np.ascontiguousarray(rays, f32)
    o, tmax = rays[:, 0:3], rays[:, 3]
    with np.errstate(all="ignore"):
        d = _normalize(rays[:, 4:7])
        live = (tmax > 0) & (((np.abs(d[:, 0]) + np.abs(d[:, 1])) + np.abs(d[:, 2])) > 0)
    _f32(o, d, tmax)
    return o, d, tmax, live


# ---- the three primitive tests: t [n, count] and the test's verdict, before the bounds 1e-6 < t < tmax --------------------------
def plane_test(o, d, planes):
    nor, point = planes["nor"][None], planes["point"][None]
    t = _dot(point - o[:, None], nor) / _dot(d[:, None], nor)
    ok = ~(t <= f32(1e-6)) & (t > EPSILON) & (t < f32(2147483648.0))
    _f32(t)
    return t, ok


def sphere_test(o, d, spheres):
    c, r = spheres["c"][None], spheres["r"][None]
    cr0 = c - o[:, None]
    rr = r * r
    inside = _dot(cr0, cr0) < rr
    tc = _dot(cr0, d[:, None])
    dv = (o[:, None] + tc[..., None] * d[:, None]) - c
    d2 = _dot(dv, dv)
    toff = np.sqrt(rr - d2)
    t = np.where(inside, tc + toff, tc - toff)
    hit = ~(~inside & (tc < 0)) & ~(~inside & (rr < d2))
    _f32(t)
    return t, hit


def triangle_test(o, d, triangles):
    p0, nor, e1, e2 = (triangles[k][None] for k in ("p0", "nor", "e1", "e2"))
    denom = _dot(d[:, None], nor)
    t = _dot(p0 - o[:, None], nor) / denom
    ip = t[..., None] * d[:, None] + o[:, None]
    w = ip - p0
    b1 = _dot(e1, w)
    b2 = _dot(e2, w)
    b0 = (f32(1.0) - b1) - b2
    hit = ~(np.abs(denom) < f32(1e-9)) & ~(t <= EPSILON) & (b0 >= -EPSILON) & (b1 >= -EPSILON) & (b2 >= -EPSILON)
    _f32(t)
    return t, hit


def leaf_tests(arrays, o, d, tmax, refs):
    """(t [n, leaves], accepted [n, leaves]) of the primitives in sorted-leaf order: the leaf test with 1e-6 < t < tmax."""
    n = len(o)
    S, T = arrays["spheres"], arrays["triangles"]
    ts, hs = sphere_test(o, d, S) if len(S) else (np.zeros((n, 0), f32), np.zeros((n, 0), bool))
    tt, ht = triangle_test(o, d, T) if len(T) else (np.zeros((n, 0), f32), np.zeros((n, 0), bool))
    col = np.where(refs["type"] != 0, len(S) + refs["id"].astype(np.int64), refs["id"].astype(np.int64))
    t = np.concatenate([ts, tt], axis=1)[:, col]
    hit = np.concatenate([hs, ht], axis=1)[:, col]
    return t, hit & (t > f32(1e-6)) & (t < tmax[:, None])


# ---- the boxes -----------------------------------------------------------------------------------------------------------------------
def box_test(nodes, o, d, tmax):
    """hit_aabb_adapted for every (ray, node): (te [n, nodes], entered-if-reached [n, nodes])."""
    inv = f32(1.0) / d
    lo, hi = [], []
    for k, (a, b) in enumerate((("xmin", "xmax"), ("ymin", "ymax"), ("zmin", "zmax"))):
        ta = (nodes[a][None, :] - o[:, k:k + 1]) * inv[:, k:k + 1]
        tb = (nodes[b][None, :] - o[:, k:k + 1]) * inv[:, k:k + 1]
        lo.append(np.fmin(ta, tb))
        hi.append(np.fmax(ta, tb))
    te = np.fmax(np.fmax(lo[0], lo[1]), lo[2])
    tx = np.fmin(np.fmin(hi[0], hi[1]), hi[2])
    _f32(te, tx)
    return te, (te < tx) & (te < tmax[:, None]) & (tx > f32(1e-4))


def reachability(nodes, te, enter):
    """From the root, which is entered untested: reach[child] = reach[parent] & enter[child], and the largest te of the boxes on
    the way (the root's own excluded).  Returns both at the leaves, in sorted-leaf order: ([n, leaves], [n, leaves])."""
    n = len(te)
    nleaves = int(np.count_nonzero(nodes["count"] > 0))
    reach = np.zeros(enter.shape, bool)
    path_te = np.full(te.shape, -np.inf, f32)
    reach[:, 0] = True
    level = np.array([0])
    while len(level):
        inner = level[nodes["count"][level] == 0]
        nxt = []
        for side in ("left", "right"):
            child = nodes[side][inner].astype(np.int64)
            reach[:, child] = reach[:, inner] & enter[:, child]
            path_te[:, child] = np.maximum(path_te[:, inner], te[:, child])      # (a NaN te stays: nothing is greater than it)
            nxt.append(child)
        level = np.concatenate(nxt) if nxt else np.array([], np.int64)
    leaves = np.flatnonzero(nodes["count"] > 0)
    assert np.all(nodes["count"][leaves] == 1) and sorted(nodes["prim_offset"][leaves].tolist()) == list(range(nleaves))
    by_sorted = leaves[np.argsort(nodes["prim_offset"][leaves])]
    return reach[:, by_sorted], path_te[:, by_sorted]


# ---- the admitted sets ----------------------------------------------------------------------------------------------------------------
def _planes(arrays, o, d, tmax, live):
    P = arrays["planes"]
    if not len(P):
        return np.zeros((len(o), 0), f32), np.zeros((len(o), 0), bool)
    t, ok = plane_test(o, d, P)
    return t, ok & (t < tmax[:, None]) & live[:, None]


def admitted(arrays, rays, nodes, refs):
    """The header's set S over the tree: dict(tp, in_p [n, planes]; tl, in_l [n, leaves] (sorted-leaf order); regular [n];
    brute_l [n, leaves]: the leaf tests' verdicts with no tree)."""
    o, d, tmax, live = split(rays)
    n = len(o)
    with np.errstate(all="ignore"):
        tp, in_p = _planes(arrays, o, d, tmax, live)
        if len(nodes):
            tl, ok = leaf_tests(arrays, o, d, tmax, refs)
            ok &= live[:, None]
            te, enter = box_test(nodes, o, d, tmax)
            reach, path_te = reachability(nodes, te, enter)
            in_l = ok & reach
            regular = np.all(~ok | (reach & (tl > path_te)), axis=1)
        else:
            tl, ok, in_l, regular = np.zeros((n, 0), f32), np.zeros((n, 0), bool), np.zeros((n, 0), bool), np.ones(n, bool)
    return dict(tp=tp, in_p=in_p, tl=tl, in_l=in_l, regular=regular, brute_l=ok, o=o, d=d)


def brute_force(arrays, rays, refs):
    """The admitted primitives by the leaf tests alone, over the arrays: (in_p [n, planes], in_l [n, leaves in sorted order])."""
    o, d, tmax, live = split(rays)
    with np.errstate(all="ignore"):
        _, in_p = _planes(arrays, o, d, tmax, live)
        if len(refs):
            _, ok = leaf_tests(arrays, o, d, tmax, refs)
            ok &= live[:, None]
        else:
            ok = np.zeros((len(o), 0), bool)
    return in_p, ok


# ---- order, records, counts -------------------------------------------------------------------------------------------------------------
def records(arrays, refs, S, k):
    """(hits uint32 [n, k, 6], counts uint32 [n]) of an admitted() result: the first min(k, |S|) hits by (t, class, index), then
    misses.  The columns are the planes by index, then the leaves by sorted position, so a stable sort by t is the whole order."""
    o, d = S["o"], S["d"]
    n = len(o)
    T = np.concatenate([np.where(S["in_p"], S["tp"], f32(np.inf)), np.where(S["in_l"], S["tl"], f32(np.inf))], axis=1)
    counts = (np.count_nonzero(S["in_p"], axis=1) + np.count_nonzero(S["in_l"], axis=1)).astype(u32)
    hits = np.tile(MISS, (n, k, 1))
    if not T.shape[1] or not k:
        return hits, counts
    order = np.argsort(T, axis=1, kind="stable")[:, :k]
    npl = S["tp"].shape[1]
    sph, tri, pl = arrays["spheres"], arrays["triangles"], arrays["planes"]
    rows = np.arange(n)
    with np.errstate(all="ignore"):
        for j in range(order.shape[1]):
            col = order[:, j]
            t = T[rows, col]
            has = np.isfinite(t)
            is_plane = has & (col < npl)
            leaf = np.clip(col - npl, 0, max(len(refs) - 1, 0))
            is_tri = has & ~is_plane & (refs["type"][leaf] != 0 if len(refs) else False)
            is_sph = has & ~is_plane & ~is_tri
            pid = refs["id"][leaf] if len(refs) else np.zeros(n, u32)
            for sel, kind in ((is_plane, KIND_PLANE), (is_sph, KIND_SPHERE), (is_tri, KIND_TRIANGLE)):
                i = np.flatnonzero(sel)
                if not len(i):
                    continue
                if kind == KIND_PLANE:
                    ids = col[i]
                    nor = pl["nor"][ids]
                    nn = np.where((_dot(nor, d[i]) < 0)[:, None], nor, -nor)
                elif kind == KIND_TRIANGLE:
                    ids = pid[i]
                    nor = tri["nor"][ids]
                    nn = np.where((_dot(d[i], nor) < 0)[:, None], nor, -nor)
                else:
                    ids = pid[i]
                    c, r = sph["c"][ids], sph["r"][ids]
                    p = t[i, None] * d[i] + o[i]
                    cr0 = c - o[i]
                    inside = _dot(cr0, cr0) < r * r
                    nn = _normalize(np.where(inside[:, None], c - p, p - c))
                _f32(nn)
                hits[i, j, 0] = t[i].view(u32)
                hits[i, j, 1] = kind
                hits[i, j, 2] = ids
                hits[i, j, 3:6] = np.ascontiguousarray(nn, f32).view(u32)
    return hits, counts


def multihit(arrays, rays, nodes, refs, k):
    """(hits uint32 [n, k, 6], counts uint32 [n], regular bool [n]): mirt_trace_rays_multi's answer."""
    S = admitted(arrays, rays, nodes, refs)
    hits, counts = records(arrays, refs, S, k)
    return hits, counts, S["regular"]
