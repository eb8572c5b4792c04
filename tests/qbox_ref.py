"""References for the quantised box test (csrc/scene_dev.h qlo / qhi, csrc/shade_common.h quantised_axis, box_pair_q, box_q) and
for box_pair, in plain Python and numpy; nothing here touches the GPU or the library.

  exact_enters    the slab test in exact rational arithmetic (fractions.Fraction) on float32 inputs
  grid_planes     the planes smin + q * step of a packed box, exact
  restate         the float32 restatement of what one thread of mirt_probe_qbox computes.  The library is built with
                  -ffp-contract=off -fno-fast-math, so numpy float32 is the same arithmetic; a fused multiply-add is the exact
                  product and sum rounded once (fma32), fminf / fmaxf are np.fmin / np.fmax (NaN from 0 * inf loses)
  make_cases      the seeded case generator, one regime at a time (REGIMES)
  check_cases     assertions (a) to (e) of tests/test_qbox_ref.py and tests/test_gpu_qbox.py on a result table
"""
from fractions import Fraction

import numpy as np

F = np.float32
QGRID = F(65535.0)
QINV_STEPS = F(2.0 ** 60)
TMIN = F(0.0001)

CASE = np.dtype([("smin", "<f4", 3), ("smax", "<f4", 3), ("lo", "<f4", 3), ("hi", "<f4", 3), ("o", "<f4", 3), ("d", "<f4", 3),
                 ("tbest", "<f4"), ("pad", "<f4")])
RESULT = np.dtype([("qlo", "<u4", 3), ("qhi", "<u4", 3), ("hit", "<u4", 4), ("te", "<f4", 3), ("pad", "<u4"),
                   ("step", "<f4", 3), ("lim", "<f4", 3)])


# ---- exact arithmetic ----------------------------------------------------------------------------------------------------------
def exact_enters(planes_lo, planes_hi, o, d, tbest, tmin, strict=True):
    """Does the ray o + t d enter the box [planes_lo, planes_hi] (three planes each: Fractions or floats) within (tmin, tbest)?
    Per axis with d != 0 the near and far parameters; an axis with d == +-0 is "surely inside" only for lo < o < hi (an origin
    exactly on a plane is undecided and counts as not entering).  t_enter < t_exit and t_enter < tbest and t_exit > tmin, all
    strict -- or, strict=False, none of them strict (the form the tightness check uses)."""
    t_enter = t_exit = None
    for k in range(3):
        lo, hi, ok, dk = Fraction(planes_lo[k]), Fraction(planes_hi[k]), Fraction(float(o[k])), Fraction(float(d[k]))
        if dk == 0:
            if not ((lo < ok < hi) if strict else (lo <= ok <= hi)):
                return False
            continue
        t1, t2 = (lo - ok) / dk, (hi - ok) / dk
        near, far = (t1, t2) if t1 <= t2 else (t2, t1)
        t_enter = near if t_enter is None or near > t_enter else t_enter
        t_exit = far if t_exit is None or far < t_exit else t_exit
    if t_enter is None:      # no axis moves: the origin is inside for every t
        return True
    tb = float(tbest)
    tb = tb if np.isinf(tb) else Fraction(tb)
    tm = Fraction(float(tmin))
    if strict:
        return t_enter < t_exit and t_enter < tb and t_exit > tm
    return t_enter <= t_exit and t_enter <= tb and t_exit >= tm


def grid_planes(smin, step, q, grow=None):
    """smin + (q + grow) * step per axis, exact (grow: Fractions, default 0)."""
    return [Fraction(float(smin[k])) + (int(q[k]) + (grow[k] if grow is not None else 0)) * Fraction(float(step[k])) for k in range(3)]


# ---- the float32 restatement ---------------------------------------------------------------------------------------------------
def fma32(a, b, c):
    """fmaf on float32 arrays: the product of two float32 is exact in float64; the sum is rounded to odd in float64 (TwoSum tells
    whether it was inexact and which way), so that the final rounding to float32 is the only one that counts."""
    p = a.astype(np.float64) * b.astype(np.float64)
    c = np.broadcast_to(c, p.shape).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)
        fix = np.isfinite(s) & np.isfinite(err) & (err != 0) & ((s.view(np.int64) & 1) == 0)
        s = np.where(fix, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
        return s.astype(F)


def grid_of(smin, smax):
    """step and 2^60 / step as pack_qnodes_kernel computes them."""
    rng = smax - smin
    with np.errstate(divide="ignore", invalid="ignore"):
        step = np.where(rng > 0, rng / QGRID, F(1.0)).astype(F)
    return step, (QINV_STEPS / step).astype(F)


def q_lo(x, smin, step):
    q = np.floor((x - smin) / step) - F(1.0)
    return np.fmin(np.fmax(q, F(0.0)), QGRID).astype(np.uint32)


def q_hi(x, smin, step):
    q = np.ceil((x - smin) / step) + F(1.0)
    return np.fmin(np.fmax(q, F(0.0)), QGRID).astype(np.uint32)


def quantised_axis(gmin, gstep, lim, o, inv):
    """A, Cn, Cf and whether the near plane is the high half-word."""
    ic = np.fmin(np.fmax(inv, -lim), lim)
    B = (gmin - o) * ic
    A = gstep * ic
    E = fma32(np.abs(B), F(9.5367431640625e-07), F(1.0625) * np.abs(A))
    C0 = fma32(np.full_like(A, -8388608.0), A, B)
    return A, C0 - E, C0 + E, ~(A >= 0)


def slab3(near, far, tbest):
    with np.errstate(invalid="ignore"):
        te = np.fmax(np.fmax(near[:, 0], near[:, 1]), near[:, 2])
        tx = np.fmin(np.fmin(far[:, 0], far[:, 1]), far[:, 2])
        return (te < tx) & (te < tbest) & (tx > TMIN), te


def restate(cases):
    """What mirt_probe_qbox returns for `cases` (CASE records), as RESULT records: one quantised form stands for the three the
    device has (hit[1..3] and te[1], te[2] are copies of it)."""
    c = cases
    out = np.zeros(len(c), dtype=RESULT)
    step, lim = grid_of(c["smin"], c["smax"])
    out["step"], out["lim"] = step, lim
    out["qlo"], out["qhi"] = q_lo(c["lo"], c["smin"], step), q_hi(c["hi"], c["smin"], step)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        inv = (F(1.0) / c["d"]).astype(F)
        # box_pair: (plane - o) * inv per plane, min / max per axis
        t1, t2 = (c["lo"] - c["o"]) * inv, (c["hi"] - c["o"]) * inv
        hit, te = slab3(np.fmin(t1, t2), np.fmax(t1, t2), c["tbest"])
        out["hit"][:, 0], out["te"][:, 0] = hit, te
        # the quantised form: 2^23 + q as a float, one fused multiply-add per plane
        A, Cn, Cf, high = quantised_axis(c["smin"], step, lim, c["o"], inv)
        qn = np.where(high, out["qhi"], out["qlo"]).astype(F) + F(8388608.0)
        qf = np.where(high, out["qlo"], out["qhi"]).astype(F) + F(8388608.0)
        hit, te = slab3(fma32(qn, A, Cn), fma32(qf, A, Cf), c["tbest"])
    for k in (1, 2, 3):
        out["hit"][:, k] = hit
    out["te"][:, 1], out["te"][:, 2] = te, te
    return out


# ---- the case generator --------------------------------------------------------------------------------------------------------
REGIMES = ("random", "thin", "touching", "flat_scene", "near", "far", "grazing", "tiny_direction", "on_plane", "finite_tbest")
OFFSETS = (0.0, 1.0, 10.0, 60.0)                 # scene offset from the world origin, in extents (grid_ok allows 64)
DISTANCES = (0.0, 1.0, 10.0, 1e3, 3e4, 1e5)       # ray origin from its target, in extents (0: somewhere inside the scene)
TINY = (0.0, -0.0, 1e-25, -1e-25, -1e-39, 3e-23, -3e-23)      # +-0; 1 / 1e-39 is infinite; 3e-23 is near the clamp 2^60 / step


def make_cases(regime, n, seed):
    """n CASE records of one regime.  Every regime draws what it does not fix from the common distributions: extents 1e-2..1e2
    per axis, an offset from OFFSETS, a random box, an origin at one of DISTANCES, a target in or around the box, tbest = inf."""
    assert regime in REGIMES, regime
    rng = np.random.default_rng([seed, REGIMES.index(regime)])
    c = np.zeros(n, dtype=CASE)
    pick = lambda values, size: np.asarray(values)[rng.integers(0, len(values), size)]      # noqa: E731

    # scene bounds
    extent = 10.0 ** rng.uniform(-2, 2, (n, 3))
    off = pick(OFFSETS, n)[:, None] * rng.choice([-1.0, 1.0], (n, 3))
    smin = np.where(off == 0, -0.5 * extent, np.where(off > 0, off * extent, (off - 1.0) * extent)).astype(F)
    smax = (smin + extent.astype(F)).astype(F)
    if regime == "flat_scene":
        ax = rng.integers(0, 3, n)
        smax[np.arange(n), ax] = smin[np.arange(n), ax]
    c["smin"], c["smax"] = smin, smax
    rge = (smax - smin).astype(F)
    step, _ = grid_of(smin, smax)

    # the box, inside the scene bounds
    u0, u1 = rng.uniform(0, 1, (n, 3)), rng.uniform(0, 1, (n, 3))
    ulo, uhi = np.minimum(u0, u1), np.maximum(u0, u1)
    lo = (smin + (ulo * rge).astype(F)).astype(F)
    hi = (smin + (uhi * rge).astype(F)).astype(F)
    if regime == "thin":      # 0 to 3 grid steps thick on one to three axes, lo == hi included
        thin = rng.random((n, 3)) < 0.6
        thin[np.arange(n), rng.integers(0, 3, n)] = True
        thick = np.where(rng.random((n, 3)) < 0.3, 0.0, rng.uniform(0, 3, (n, 3)))
        hi = np.where(thin, (lo + (thick * step).astype(F)).astype(F), hi)
    if regime == "touching":      # the scene's own planes: smin, smax, or the whole scene box
        kind = rng.integers(0, 3, n)[:, None]
        which = rng.random((n, 3)) < 0.6
        which[np.arange(n), rng.integers(0, 3, n)] = True
        lo = np.where((kind == 2) | ((kind == 0) & which), smin, lo)
        hi = np.where((kind == 2) | ((kind == 1) & which), smax, hi)
    lo = np.clip(lo, smin, smax)
    hi = np.clip(np.maximum(hi, lo), smin, smax)
    c["lo"], c["hi"] = lo, hi

    # the target: in the box, or around it by up to 0.6 of its half-size plus a few grid steps
    ctr = 0.5 * (lo.astype(np.float64) + hi.astype(np.float64))
    half = 0.5 * (hi.astype(np.float64) - lo.astype(np.float64))
    s = rng.uniform(-1.6, 1.6, (n, 3))
    reach = half + np.where(rge > 0, 4.0, 0.5) * step      # (an axis of zero extent has step 1.0 and a grid box [0, 1])
    if regime == "grazing":      # on a face, an edge or a corner, within a few grid steps (from nearby: a far origin cannot aim that finely)
        on = rng.random((n, 3)) < 0.5
        on[np.arange(n), rng.integers(0, 3, n)] = True
        s = np.where(on, rng.choice([-1.0, 1.0], (n, 3)), rng.uniform(-1, 1, (n, 3)))
        target = ctr + s * half + np.where(on, rng.uniform(-12, 12, (n, 3)) * step, 0.0)
    else:
        target = ctr + s * reach

    # the origin
    ext = np.max(extent, axis=1)[:, None]
    dist = pick({"near": DISTANCES[:3], "grazing": DISTANCES[:3], "far": DISTANCES[3:]}.get(regime, DISTANCES), n)[:, None]
    way = rng.normal(size=(n, 3))
    way /= np.linalg.norm(way, axis=1)[:, None]
    inside = smin + rng.uniform(0, 1, (n, 3)) * rge
    o = np.where(dist == 0, inside, target + dist * ext * way).astype(F)
    if regime == "on_plane":      # exactly on a plane of the box, or on a grid plane next to it, on one axis
        ax = rng.integers(0, 3, n)
        rows = np.arange(n)
        kind = rng.integers(0, 4, n)
        q = np.where(kind == 2, q_lo(lo, smin, step)[rows, ax], q_hi(hi, smin, step)[rows, ax]).astype(np.int64) + rng.integers(-2, 3, n)
        gridp = (smin[rows, ax] + (np.clip(q, 0, 65535).astype(F) * step[rows, ax]).astype(F)).astype(F)
        o[rows, ax] = np.where(kind == 0, lo[rows, ax], np.where(kind == 1, hi[rows, ax], gridp))
        # (the other two coordinates: half of the cases start within the box's slabs, so that a ray along the plane can enter)
        within = (rng.random(n) < 0.5)[:, None] & (np.arange(3)[None, :] != ax[:, None])
        o = np.where(within, (ctr + rng.uniform(-1, 1, (n, 3)) * half).astype(F), o)
    d = target - o.astype(np.float64)
    norm = np.linalg.norm(d, axis=1)[:, None]
    d = np.where(norm > 0, d / np.where(norm > 0, norm, 1.0), way).astype(F)
    if regime == "on_plane":      # a third of them run along the plane (d == +-0 there: undecided, not entering)
        along = rng.random(n) < 0.33
        d[np.arange(n)[along], ax[along]] = rng.choice([0.0, -0.0], int(along.sum()))
    if regime == "tiny_direction":      # one or two components replaced; the origin then in or near the box's slab on those axes
        keep = rng.integers(0, 3, n)
        rep = rng.random((n, 3)) < 0.4
        rep[np.arange(n), (keep + rng.integers(1, 3, n)) % 3] = True
        rep[np.arange(n), keep] = False
        d = np.where(rep, pick(TINY, (n, 3)).astype(F), d)
        o = np.where(rep, (ctr + rng.uniform(-1.5, 1.5, (n, 3)) * (half + 2.0 * step)).astype(F), o)
        # (the kept component must move the ray)
        d[np.arange(n), keep] = np.where(np.abs(d[np.arange(n), keep]) < 0.05, F(0.7), d[np.arange(n), keep])
    c["o"], c["d"] = o, d

    c["tbest"] = F(np.inf)
    if regime == "finite_tbest":      # around the distance at which the ray meets the box (float64 is enough to place it)
        with np.errstate(divide="ignore", invalid="ignore"):
            t1 = (lo.astype(np.float64) - o) / d.astype(np.float64)
            t2 = (hi.astype(np.float64) - o) / d.astype(np.float64)
        te = np.nanmax(np.fmin(t1, t2), axis=1)
        te = np.where(np.isfinite(te) & (te > 0), te, norm[:, 0])
        c["tbest"] = (te * pick((0.5, 0.99, 1.0 - 1e-5, 1.0 - 1e-6, 1.0, 1.0 + 1e-6, 1.0 + 1e-5, 1.01, 2.0), n)).astype(F)
    return c


# ---- the assertions ------------------------------------------------------------------------------------------------------------
def check_words(c, r):
    """(a) independent of the restatement: with u = (x - smin) / step exact, q_lo <= u and u - q_lo < 3 unless q_lo == 0;
    q_hi >= u and q_hi - u < 3 unless q_hi == 65535, where u - 65535 < 1/16 must hold instead (step is a rounded quotient: the top
    grid plane may fall a hair below smax, which the walker's margin of more than a step covers)."""
    for k in range(3):
        smin, step = Fraction(float(c["smin"][k])), Fraction(float(r["step"][k]))
        u = (Fraction(float(c["lo"][k])) - smin) / step
        q = int(r["qlo"][k])
        assert q <= u and (q == 0 or u - q < 3), ("q_lo", k, q, float(u))
        u = (Fraction(float(c["hi"][k])) - smin) / step
        q = int(r["qhi"][k])
        if q == 65535:
            assert u - 65535 < Fraction(1, 16), ("q_hi at the top", k, float(u))
        else:
            assert q >= u and q - u < 3, ("q_hi", k, q, float(u))


def growth(c, r):
    """(d) how far, in grid steps per axis, the tested box may exceed the grid box.  quantised_axis moves the near offset down and
    the far offset up by E = 2^-20 |B| + 1.0625 |A|, a bound on every rounding on the way, so a computed plane parameter lies
    within 2 E of the grid plane's: 2 E / |A| = 2.125 + 2^-19 |B| / |A| grid steps, and |B| / |A| is |smin - o| / step but for the
    roundings of B and A themselves (a few 2^-24).  One more step and the eighth that rounds 3.125 up to 3.25 cover those, the
    rounding of 1 / d against the exact d the reference divides by (65535 * 2^-23 of a step at most), and E's own rounding."""
    return [Fraction(13, 4) + Fraction(1, 2 ** 19) * abs(Fraction(float(c["smin"][k])) - Fraction(float(c["o"][k]))) / Fraction(float(r["step"][k]))
            for k in range(3)]


def same_floats(a, b):
    """Bit for bit -- but for what C leaves open: which NaN a NaN is, and the sign of fmaxf(-0, +0)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b)) | ((a == 0) & (b == 0))


def check_cases(cases, got, want, tight=True):
    """Assertions (a) to (e) on `got` (RESULT records: the device's, or the restatement's own) against `want` = restate(cases).
    Returns (fraction of cases whose grid box the ray enters, fraction the quantised test answers "miss" for)."""
    assert len(cases) == len(got) == len(want)
    enters = misses = 0
    for i in range(len(cases)):
        c, r = cases[i], got[i]
        check_words(c, r)
        q_hit = [bool(h) for h in r["hit"][1:]]
        glo, ghi = grid_planes(c["smin"], r["step"], r["qlo"]), grid_planes(c["smin"], r["step"], r["qhi"])
        # (b) the walker is sound: a ray that enters the grid box is a hit in all three quantised forms
        if exact_enters(glo, ghi, c["o"], c["d"], c["tbest"], TMIN):
            enters += 1
            assert all(q_hit), ("(b)", i, q_hit)
        # (c) the pair is sound: where box_pair admits the exact box, so do the quantised forms
        if r["hit"][0]:
            assert all(q_hit), ("(c)", i, q_hit)
        misses += not any(q_hit)
        # (d) tightness, where no direction component is tiny: a quantised hit is a (non-strict) hit of the grown grid box
        if tight and any(q_hit) and np.all(np.abs(c["d"]) >= F(2.0 ** -20)):
            g = growth(c, r)
            glo_g = grid_planes(c["smin"], r["step"], r["qlo"], [-x for x in g])
            ghi_g = grid_planes(c["smin"], r["step"], r["qhi"], g)
            assert exact_enters(glo_g, ghi_g, c["o"], c["d"], c["tbest"], TMIN, strict=False), ("(d)", i)
    # (a) the words, the grid's step and 2^60 / step, bit for bit; (e) the three copies agree with each other and the restatement
    # (after the exact checks, which do not depend on the restatement: a failure there is reported as what it is)
    for name in ("qlo", "qhi", "hit"):
        assert np.array_equal(got[name], want[name]), (name, np.flatnonzero((got[name] != want[name]).any(axis=1))[:5])
    for name in ("step", "lim", "te"):
        same = same_floats(got[name], want[name])
        assert same.all(), (name, np.flatnonzero(~same.all(axis=1))[:5])
    return enters / len(cases), misses / len(cases)
