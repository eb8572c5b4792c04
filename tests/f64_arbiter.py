"""An independent float64 arbiter for the part of the renderer that draws no random numbers (test code).

A plain recursive restatement, in Python floats (IEEE double), of the reference's hitNearest, diffuseLight, reflectionLight and
refractionLight (draw.cu:260-527, 581-659) and of its sphere / triangle / plane intersections (struct.cu:16-163), brute force
over the primitives: no BVH, no float32, no state machine.  The oracle and the HIP path come from one reading of the reference;
this is a second one, and it shares no code with either.

While it recurses it records the smallest relative margin of every decision it takes -- hit or miss, which of two hits is nearer,
a shadow hit against the light's distance, the sign of k, inside or outside a sphere, the sign of a denominator, the epsilon
tests.  A pixel whose margin exceeds CLEAR is one on which float32 and float64 take the same decisions, so the two images may
differ by rounding only.

Scope: spp 0, the regular / fisheye-free / panorama cameras without depth of field, no roughness, no gi."""
import math

import numpy as np

CLEAR = 1e-4
INF = float("inf")
NAN = float("nan")
EPSILON = 0.001


def _rel(a, b):
    """Relative distance of a from b: the margin of the comparison a < b."""
    s = max(abs(a), abs(b))
    if s == 0.0 or s == INF:
        return 0.0 if a == b else 1.0
    return abs(a - b) / s


def _add(a, b): return (a[0] + b[0], a[1] + b[1], a[2] + b[2])
def _sub(a, b): return (a[0] - b[0], a[1] - b[1], a[2] - b[2])
def _mul(a, s): return (a[0] * s, a[1] * s, a[2] * s)
def _dot(a, b): return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]
def _neg(a): return (-a[0], -a[1], -a[2])
def _cmul(a, b): return (a[0] * b[0], a[1] * b[1], a[2] * b[2])


def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def _sqrt(x):
    return math.sqrt(x) if x >= 0.0 else NAN      # (x NaN: the comparison is false as well)


def _length(a):
    return _sqrt(_dot(a, a))


def _normalize(a):
    """vec3::normalize: the zero vector for a (nearly) zero length."""
    mag = _length(a)
    if mag != mag:
        return (NAN, NAN, NAN)
    if mag < 1e-6:
        return (0.0, 0.0, 0.0)
    return _mul(a, 1.0 / mag)


def _black(c):
    """RGB == RGB(0, 0, 0) (fequal: every channel below 1e-6)."""
    return all(abs(x) < 1e-6 for x in c)


class Hit:
    __slots__ = ("is_hit", "t", "p", "n", "mat")

    def __init__(self, t=-1.0, p=(0.0, 0.0, 0.0), n=(0.0, 0.0, 0.0), mat=None, is_hit=False):
        self.is_hit, self.t, self.p, self.n, self.mat = is_hit, t, p, n, mat


class Arbiter:
    def __init__(self, sc):
        """sc: a tests.pyscene.PyScene.  Derived quantities (unit normals, the triangles' edge vectors, a plane's point) are
        recomputed in float64 from what the scene file gives."""
        f = lambda v: tuple(float(x) for x in v)
        mat = lambda m: dict(color=f(m["color"]), shine=f(m["shininess"]), trans=f(m["trans"]), ior=float(m["ior"]))
        self.default_mat = dict(color=(0.0, 0.0, 0.0), shine=(0.0, 0.0, 0.0), trans=(0.0, 0.0, 0.0), ior=float(np.float32(1.458)))
        self.spheres = [(f(s["c"]), float(s["r"]), mat(s["mat"])) for s in sc.spheres]
        self.tris = []
        for t in sc.triangles:
            p0, p1, p2 = f(t["p0"]), f(t["p1"]), f(t["p2"])
            nor = _normalize(_cross(_sub(p1, p0), _sub(p2, p0)))
            a1, a2 = _cross(_sub(p2, p0), nor), _cross(_sub(p1, p0), nor)
            self.tris.append((p0, nor, _mul(a1, 1.0 / _dot(a1, _sub(p1, p0))), _mul(a2, 1.0 / _dot(a2, _sub(p2, p0))), mat(t["mat"])))
        self.planes = []
        for p in sc.planes:
            a, b, c, d = (float(x) for x in p["abcd"])
            den = a * a + b * b + c * c
            self.planes.append((_normalize((a, b, c)), (-a * d / den, -b * d / den, -c * d / den), mat(p["mat"])))
        self.suns = [(f(l["v"]), f(l["color"])) for l in sc.suns]
        self.bulbs = [(f(l["v"]), f(l["color"])) for l in sc.bulbs]
        self.expose = float(sc.expose)
        self.sc = sc
        self.forward, self.right, self.up, self.eye = f(sc.forward), f(sc.right), f(sc.up), f(sc.eye)
        assert float(sc.dof_focus) == 0.0 and not sc.fisheye and sc.gi == 0
        self.margin, self.what = INF, None      # the smallest margin of the current pixel, and the decision that has it

    def _decide(self, m, what):
        if m < self.margin:
            self.margin, self.what = m, what

    # ---- intersections (struct.cu:64-163, draw.cu:581-615) ----
    def _sphere(self, eye, d, s):
        c, r, mat = s
        cr0 = _sub(c, eye)
        cc = _dot(cr0, cr0)
        inside = cc < r * r
        self._decide(_rel(cc, r * r), "inside sphere")
        tc = _dot(cr0, d)
        dv = _sub(_add(eye, _mul(d, tc)), c)
        d2 = _dot(dv, dv)
        if not inside:
            # two tests, one outcome: a sphere behind the origin (tc < 0) is also missed by the line (r r < d2) unless the origin
            # is all but on it -- the miss is as clear as the clearer of the two
            behind = abs(tc) / max(math.sqrt(cc), 1e-300)
            if tc < 0.0:
                self._decide(max(behind, _rel(r * r, d2)) if r * r < d2 else behind, "sphere behind")
                return None
            if r * r < d2:
                self._decide(_rel(r * r, d2), "sphere missed")
                return None
            self._decide(min(behind, _rel(r * r, d2)), "sphere hit")
        t = tc + _sqrt(r * r - d2) if inside else tc - _sqrt(r * r - d2)
        p = _add(_mul(d, t), eye)
        n = _normalize(_sub(c, p) if inside else _sub(p, c))
        return Hit(t, p, n, mat, True)

    def _triangle(self, eye, d, tr):
        p0, nor, e1, e2, mat = tr
        den = _dot(d, nor)
        if den != den:
            return None
        self._decide(abs(den), "triangle denominator")      # its sign, and |den| against 1e-9 (both vectors have unit length)
        if abs(den) < 1e-9:
            return None
        t = _dot(_sub(p0, eye), nor) / den
        self._decide(_rel(t, EPSILON), "triangle t > epsilon")
        if t <= EPSILON:
            return None
        p = _add(_mul(d, t), eye)
        b1, b2 = _dot(e1, _sub(p, p0)), _dot(e2, _sub(p, p0))
        b0 = 1.0 - b1 - b2
        self._decide(min(abs(b0 + EPSILON), abs(b1 + EPSILON), abs(b2 + EPSILON)), "barycentric")
        if not (b0 >= -EPSILON and b1 >= -EPSILON and b2 >= -EPSILON):
            return None
        if min(b0, b1, b2) < 0.0:
            # up to 0.001 outside the triangle proper, possibly outside its box: whether the reference's walk finds this hit
            # depends on the boxes on the way (the oracle restates that walk; a brute-force loop cannot)
            self._decide(0.0, "hit outside the triangle proper")
        return Hit(t, p, nor if den < 0.0 else _neg(nor), mat, True)

    def _plane(self, eye, d):
        best, best_plane = None, None
        for nor, point, mat in self.planes:
            den = _dot(d, nor)
            if den != den:
                continue
            self._decide(abs(den), "plane denominator")
            if den == 0.0:
                continue      # t is +-inf or NaN: `t <= 1e-6` or `t < t_sol` fails
            t = _dot(_sub(point, eye), nor) / den
            self._decide(min(_rel(t, 1e-6), _rel(t, EPSILON)), "plane t > epsilon")
            if t <= 1e-6 or not t > EPSILON:
                continue
            if best is not None and (nor, point) != best_plane:      # (of two identical planes the first wins in any arithmetic)
                self._decide(_rel(t, best.t), "nearer plane")
            if best is None or t < best.t:
                best, best_plane = Hit(t, _add(_mul(d, t), eye), nor if den < 0.0 else _neg(nor), mat, True), (nor, point)
        if best is not None:
            self._decide(_rel(best.t, 2147483637.0), "plane t < INT_MAX")
            if best.t >= 2147483637.0:      # t_sol >= INT_MAX - 10
                return None
        return best

    def hit_nearest(self, eye, d, bounce):
        """hitNearest, draw.cu:292-318: the nearest primitive hit beyond 1e-6 (traverse_lbvh's acceptance, bvh_traversal.cu:62-80)
        against the nearest plane; the plane wins a tie."""
        if bounce == 0:
            return Hit()
        if d[0] != d[0] or d[1] != d[1] or d[2] != d[2]:
            return Hit()      # a NaN direction fails every comparison of every test
        hits = []
        for s in self.spheres:
            h = self._sphere(eye, d, s)
            if h is not None and h.t == h.t:
                self._decide(_rel(h.t, 1e-6), "sphere t > 1e-6")
                if h.t > 1e-6:
                    hits.append(h)
        for tr in self.tris:
            h = self._triangle(eye, d, tr)
            if h is not None:
                hits.append(h)
        pl = self._plane(eye, d)
        if pl is not None:
            hits.append(pl)
        if not hits:
            return Hit()
        best = min(hits, key=lambda h: h.t)
        for h in hits:
            if h is not best:
                self._decide(_rel(h.t, best.t), "nearer hit")
        if pl is not None and pl is not best and pl.t == best.t:
            best = pl
        return best

    # ---- shading (draw.cu:260-527) ----
    def _expose(self, c):
        return c if self.expose == INF else 1.0 - math.exp(-self.expose * c)

    def diffuse(self, obj):
        n = _normalize(obj.n)
        o = _add(obj.p, _mul(obj.n, EPSILON))
        col = (0.0, 0.0, 0.0)
        oc = obj.mat["color"]
        for ldir, lc in self.suns:
            ld = _normalize(ldir)
            if self.hit_nearest(o, ld, 1).is_hit:
                continue
            lam = max(_dot(n, ld), 0.0)
            col = _add(col, tuple(self._expose(oc[k] * (lc[k] * lam)) for k in range(3)))
        for lp, lc in self.bulbs:
            bd = _sub(lp, obj.p)
            dist = _length(bd)
            sh = self.hit_nearest(o, _normalize(bd), 1)
            if sh.is_hit:
                self._decide(_rel(sh.t, dist), "shadow hit before the light")
                if sh.t < dist:
                    continue
            lam = max(_dot(n, _normalize(bd)), 0.0)
            i = 1.0 / (dist * dist)
            col = _add(col, tuple(self._expose(oc[k] * (lc[k] * lam)) * i for k in range(3)))
        return col + (0.0,)

    @staticmethod
    def _mix(shine, trans, reflect, refract, diffuse):
        out = []
        for k in range(3):
            out.append(shine[k] * reflect[k] + (1.0 - shine[k]) * trans[k] * refract[k] + (1.0 - shine[k]) * (1.0 - trans[k]) * diffuse[k])
        # (rgb * RGBA keeps the RGBA's alpha, struct.cuh:52-55)
        return tuple(out) + (reflect[3] + refract[3] + diffuse[3],)

    def reflection(self, d, bounce, obj):
        if _black(obj.mat["shine"]) or bounce <= 0:
            return (0.0, 0.0, 0.0, 0.0)
        n = _normalize(obj.n)
        rd = _normalize(_sub(d, _mul(n, 2.0 * _dot(n, d))))
        o = _add(obj.p, _mul(obj.n, EPSILON))
        so = self.hit_nearest(o, rd, bounce - 1)
        if not so.is_hit:
            return (0.0, 0.0, 0.0, 1.0)
        shine, trans = ((0.0,) * 3, (0.0,) * 3) if bounce == 1 else (so.mat["shine"], so.mat["trans"])
        return self._mix(shine, trans, self.reflection(rd, bounce - 1, so), self.refraction(d, bounce, obj), self.diffuse(so))

    def refraction(self, d, bounce, obj):
        if _black(obj.mat["trans"]) or bounce <= 0:
            return (0.0, 0.0, 0.0, 0.0)
        ior = 1.0 / obj.mat["ior"]
        n = _normalize(obj.n)
        dn = _dot(n, d)
        k = 1.0 - ior * ior * (1.0 - dn * dn)
        self._decide(abs(k) / max(1.0, ior * ior), "sign of k")
        if k < 0:
            fd = _normalize(_sub(d, _mul(n, 2.0 * dn)))
            fo = _add(obj.p, _mul(n, EPSILON))
        else:
            ind = _normalize(_sub(_mul(d, ior), _mul(n, ior * dn + math.sqrt(k))))
            other = self.hit_nearest(_sub(obj.p, _mul(n, 0.0001)), ind, bounce)      # no miss check: the default ObjectInfo
            n2 = _normalize(other.n)
            ior2 = other.mat["ior"] if other.is_hit else self.default_mat["ior"]
            dn2 = _dot(n2, ind)
            k2 = 1.0 - ior2 * ior2 * (1.0 - dn2 * dn2)
            self._decide(abs(k2) / max(1.0, ior2 * ior2), "sign of k (second interface)")
            s = _sqrt(k2)
            fd = _normalize(_sub(_mul(ind, ior2), tuple((ior2 * dn2 + s) * c for c in n2)))      # (NaN * 0 is NaN)
            fo = _sub(other.p, _mul(n2, 0.0001))
        bounce -= 1
        fobj = self.hit_nearest(fo, fd, bounce)
        if not fobj.is_hit:
            return (0.0, 0.0, 0.0, 1.0)
        shine, trans = ((0.0,) * 3, (0.0,) * 3) if bounce == 0 else (fobj.mat["shine"], fobj.mat["trans"])
        return self._mix(shine, trans, self.reflection(fd, bounce, fobj), self.refraction(fd, bounce, fobj), self.diffuse(fobj))

    # ---- camera (struct.cu:16-62) and shootPrimaryRay ----
    def primary_dir(self, x, y, w, h):
        if self.sc.panorama:
            theta = (x / w - 0.5) * 2.0 * math.pi
            phi = (y / h - 0.5) * math.pi
            fr = _add(_mul(self.forward, math.cos(theta)), _mul(self.right, math.sin(theta)))
            return _normalize(_normalize(_sub(_mul(fr, math.cos(phi)), _mul(self.up, math.sin(phi)))))
        md = float(max(w, h))
        sx, sy = (2.0 * x - w) / md, (h - 2.0 * y) / md
        return _normalize(_add(self.forward, _add(_mul(self.right, sx), _mul(self.up, sy))))

    def pixel(self, x, y, w, h):
        """(rgba, margin, hit) of pixel (x, y) of a w x h frame at spp 0 (self.what: the decision with that margin)."""
        self.margin, self.what = INF, None
        d = self.primary_dir(float(x), float(y), w, h)
        obj = self.hit_nearest(self.eye, d, self.sc.bounces)
        if not obj.is_hit:
            return (0.0, 0.0, 0.0, 0.0), self.margin, False
        b = self.sc.bounces
        # gi 0: globalIllumination returns RGBA(), and mat.color * RGBA() is still added to the diffuse term (draw.cu:274-280):
        # 0 for a finite colour, NaN for an infinite one
        diffuse = tuple(dc + oc * 0.0 for dc, oc in zip(self.diffuse(obj), obj.mat["color"] + (0.0,)))
        c = self._mix(obj.mat["shine"], obj.mat["trans"], self.reflection(d, b, obj), self.refraction(d, b, obj), diffuse)
        return c[:3] + (1.0,), self.margin, True
