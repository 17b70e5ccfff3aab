"""Contour integrals (CPU): a literal numpy restatement of the reference's
ElectrostaticsPostProcessor::lineIntegral (epproc.cpp:489-724) and
HPProc::lineIntegral (hpproc.cpp:648-800) on top of tests/postproc.Post, with
the reference's element walk -- stay in the last sample's element, else the
lists of that element's three corners in order, else InTriangle with its
static index (PostProcessor.cpp:300-355) -- and of bendContour
(PostProcessor.cpp:772-820).

No reference program records a line integral, so parity of the device rests
on this restatement and on the closed forms of tests/test_contour_cpu.py.

The contours the device tests integrate are defined here (contours(), cases)
so that tests/test_contour_cpu.py can assert on the CPU what the device
comparison presumes: that the walk's element is the lowest-numbered containing
element at every sample."""
from __future__ import annotations

import math

import numpy as np

from postproc import PI, Post, cabs, cdiv

LINE_INTEGRAL_POINTS = 400   # d_LineIntegralPoints (PostProcessor.cpp:76)


def bend(points, angle, step=1.0):
    """bendContour on a list of (x, y): the new list."""
    c = [(float(x), float(y)) for x, y in points]
    if angle == 0:
        return c
    if step == 0:
        step = 1
    k = len(c) - 1
    if k < 1:
        return c
    if angle < -180. or angle > 180.:
        return c
    n = int(math.ceil(math.fabs(angle / step)))
    tta = angle * PI / 180.
    dtta = tta / float(n)
    a1 = c[k]
    del c[k]
    a0 = c[k - 1]
    d = cabs(a1[0] - a0[0], a1[1] - a0[1])
    R = d / (2. * math.sin(math.fabs(tta / 2.)))
    dr, di = a1[0] - a0[0], a1[1] - a0[1]
    if tta > 0:
        ph = (1. * (PI - tta)) / 2.          # exp(I*(PI-tta)/2.)
    else:
        ph = ((-1.) * (PI + tta)) / 2.       # exp(-I*(PI+tta)/2.)
    er, ei = math.cos(ph), math.sin(ph)
    sr, si = (R / d) * dr, (R / d) * di
    cr, ci = a0[0] + (sr * er - si * ei), a0[1] + (sr * ei + si * er)
    vr, vi = a0[0] - cr, a0[1] - ci
    for m in range(1, n + 1):
        er, ei = math.cos(float(m) * dtta), math.sin(float(m) * dtta)
        c.append((cr + (vr * er - vi * ei), ci + (vr * ei + vi * er)))
    return c


class Lines:
    """lineIntegral over the post-processor state R (a postproc.Post)."""

    def __init__(self, R: Post):
        self.R = R
        self.k = 0   # InTriangle's static index
        cx = np.array([c[0] for c in R.ctr])
        cy = np.array([c[1] for c in R.ctr])
        rs = np.zeros(R.NE)
        for i in range(R.NE):   # epproc.cpp:106-120
            for j in range(3):
                b = (R.X[R.p[i][j]] - R.ctr[i][0]) * (R.X[R.p[i][j]] - R.ctr[i][0]) + \
                    (R.Y[R.p[i][j]] - R.ctr[i][1]) * (R.Y[R.p[i][j]] - R.ctr[i][1])
                if b > rs[i]:
                    rs[i] = b
        self.cx, self.cy, self.rsqr = cx, cy, rs

    # -- the search ----------------------------------------------------------
    def in_triangle_literal(self, x, y):
        """InTriangle as written, element by element."""
        R, sz = self.R, self.R.NE
        if self.k < 0 or self.k >= sz:
            self.k = 0
        if R.in_triangle_test(x, y, self.k):
            return self.k
        hi = lo = self.k
        for _ in range(0, sz, 2):
            hi += 1
            if hi >= sz:
                hi = 0
            lo -= 1
            if lo < 0:
                lo = sz - 1
            for e in (hi, lo):
                z = (self.cx[e] - x) * (self.cx[e] - x) + (self.cy[e] - y) * (self.cy[e] - y)
                if z <= self.rsqr[e]:
                    if R.in_triangle_test(x, y, e):
                        self.k = e
                        return e
        return -1

    def in_triangle(self, x, y, hits=None):
        """InTriangle: the same visiting order (hi, lo alternating outwards from
        the static index) and the same tests, the circle test over all elements
        at once."""
        R, sz = self.R, self.R.NE
        if self.k < 0 or self.k >= sz:
            self.k = 0
        if R.in_triangle_test(x, y, self.k):
            return self.k
        if hits is None:
            hits = R.containing(x, y)
        best, rank = -1, None
        for e in hits:
            z = (self.cx[e] - x) * (self.cx[e] - x) + (self.cy[e] - y) * (self.cy[e] - y)
            if not z <= self.rsqr[e]:
                continue
            up, dn = (e - self.k) % sz, (self.k - e) % sz   # steps of hi, of lo, to reach e
            cand = []
            if 1 <= up <= (sz + 1) // 2:
                cand.append(2 * (up - 1))
            if 1 <= dn <= (sz + 1) // 2:
                cand.append(2 * (dn - 1) + 1)
            if cand and (rank is None or min(cand) < rank):
                best, rank = e, min(cand)
        if best >= 0:
            self.k = best
        return best

    def walk(self, elm, x, y, hits=None):
        R = self.R
        if elm < 0:
            return self.in_triangle(x, y, hits)
        if not R.in_triangle_test(x, y, elm):
            flag = False
            j = 0
            while j < 3:
                m = 0
                # (after a hit the reference sets m = 100 and j = 3 and leaves
                # both loops at their next test; the inner test would read
                # p[3], so it is not evaluated here)
                while m < len(R.con[R.p[elm][j]]):
                    elm = R.con[R.p[elm][j]][m]
                    if R.in_triangle_test(x, y, elm):
                        flag = True
                        j = 3
                        break
                    m += 1
                j += 1
            if not flag:
                elm = self.in_triangle(x, y, hits)
        return elm

    # -- the integrals ---------------------------------------------------------
    def point_v(self, x, y):
        k = self.in_triangle(x, y)
        if k < 0:
            return float("nan"), k
        return self.R.point_values(x, y, k, True)[0], k

    def line_integral(self, contour, kind, smooth=True, npts=LINE_INTEGRAL_POINTS, record=True):
        """dict(value: the two results; scale: the sums of the absolute terms
        of the two running sums; sums: the running sums before the averages are
        formed; missed; elems, containing, pts: per sample the element the walk
        chose, every containing element (record=True) and the point)."""
        R = self.R
        c = [(float(x), float(y)) for x, y in contour]
        if kind == 0:
            v0, k0 = self.point_v(*c[0])
            v1, k1 = self.point_v(*c[-1])
            r = v0
            r -= v1
            return dict(value=[r, 0.], scale=[abs(v0) + abs(v1), 0.], missed=int(k0 < 0) + int(k1 < 0))
        if kind == 2:
            r0 = r1 = 0.
            for i in range(len(c) - 1):
                r0 += cabs(c[i + 1][0] - c[i][0], c[i + 1][1] - c[i][1])
            r0 *= R.lc
            if R.axi:
                for i in range(len(c) - 1):
                    r1 += (PI * (c[i][0] + c[i + 1][0]) * cabs(c[i + 1][0] - c[i][0], c[i + 1][1] - c[i][1]))
                r1 *= pow(R.lc, 2.) if R.heat else R.lc * R.lc
            else:
                r1 = r0 * R.depth
            return dict(value=[r0, r1], scale=[abs(r0), abs(r1)], missed=0)
        assert kind in ((1, 3) if R.heat else (1, 3, 4)), kind
        no_shift = R.heat and kind == 3
        s, a = [0., 0.], [0., 0.]
        missed = 0
        elems, cont, pts = [], [], []
        with np.errstate(all="ignore"):
            for k in range(1, len(c)):
                dx, dy = c[k][0] - c[k - 1][0], c[k][1] - c[k - 1][1]
                dz = cabs(dx, dy) / float(npts)
                elm = -1
                for i in range(npts):
                    u = (float(i) + 0.5) / float(npts)
                    px, py = c[k - 1][0] + u * dx, c[k - 1][1] + u * dy
                    ab = cabs(dx, dy)
                    tr, ti = dx / ab, dy / ab
                    nr, ni = 0. * tr - 1. * ti, 0. * ti + 1. * tr
                    if not no_shift:
                        px += nr * 1.e-06
                        py += ni * 1.e-06
                    hits = R.containing(px, py) if record else None
                    elm = self.walk(elm, px, py, hits)
                    elems.append(elm)
                    pts.append((px, py))
                    if record:
                        cont.append(hits)
                    if elm < 0:
                        missed += 1
                        continue
                    v = R.point_values(px, py, elm, smooth)
                    t = [0., 0.]
                    if kind == 1 or no_shift:
                        if R.axi:
                            d = 2. * PI * px * (R.lc * R.lc)
                        else:
                            d = R.depth * R.lc
                        if kind == 1:
                            Dn = cdiv(v[1], v[2], nr, ni)[0]
                            t[0] = (Dn * dz * d)
                        else:
                            t[0] = (v[0] * dz * d)
                        t[1] = dz * d
                    else:
                        Dr, Di, Er, Ei = v[1], v[2], v[3], v[4]
                        Hn = cdiv(Er, Ei, nr, ni)[0]
                        Bn = cdiv(Dr, Di, nr, ni)[0]
                        BH = Dr * Er - Di * (-Ei)
                        dF1 = Er * Bn + Dr * Hn - nr * BH
                        dF2 = Ei * Bn + Di * Hn - ni * BH
                        if kind == 3:
                            dza = dz * R.lc
                            if R.axi:
                                dza *= 2. * PI * px * R.lc
                                dF1 = 0
                            else:
                                dza *= R.depth
                            t[0] = (dF1 * dza / 2.)
                            t[1] = (dF2 * dza / 2.)
                        elif not R.axi:
                            # (type 4; on an axisymmetric problem the reference
                            # multiplies by a Depth that means nothing there:
                            # the project returns 0, as for block integral 6)
                            dT = px * dF2 - dF1 * py
                            dza = dz * (R.lc * R.lc)
                            t[0] = (dT * dza * R.depth / 2.)
                    for q in range(2):
                        s[q] += t[q]
                        a[q] += abs(t[q])
            value = list(s)
            if kind == 1:
                value[1] = float(np.float64(s[0]) / np.float64(s[1]))
            elif no_shift:
                value[0] = float(np.float64(s[0]) / np.float64(s[1]))
        return dict(value=value, scale=a, sums=s, missed=missed, elems=elems, containing=cont, pts=pts)


# --- the contours of the device tests -----------------------------------------

def at(R: Post, fx, fy):
    """The point at the fractions (fx, fy) of the mesh's bounding box."""
    xa, xb, ya, yb = min(R.X), max(R.X), min(R.Y), max(R.Y)
    return xa + fx * (xb - xa), ya + fy * (yb - ya)


def contours(R: Post) -> dict:
    """Oblique contours off the mesh lines, by name: one segment, two
    segments, and 181 segments (a straight piece, then its last segment bent by
    180 degrees in steps of 1), one that leaves the mesh and one wholly outside."""
    w = max(R.X) - min(R.X)
    return dict(
        one=[at(R, 0.131, 0.217), at(R, 0.829, 0.673)],
        two=[at(R, 0.207, 0.811), at(R, 0.553, 0.307), at(R, 0.901, 0.719)],
        arc=bend([at(R, 0.171, 0.263), at(R, 0.307, 0.349), at(R, 0.693, 0.607)], 180., 1.),
        partly=[at(R, 0.377, 0.419), at(R, 1.283, 0.887)],
        outside=[at(R, 1.1, 0.1), at(R, 1.4, 0.3), (max(R.X) + 2. * w, max(R.Y))],
    )


TYPES = {False: (1, 3, 4), True: (1, 3)}   # the sampled types, by R.heat
CONDITION_NPTS = (7,)                        # samples per segment of the device-against-restatement cases
Q_BLOCK = 256                                # kPotQBlock: the workgroup of the sums
SWEEP_NPTS = (1, 7, Q_BLOCK - 1, Q_BLOCK, Q_BLOCK + 1, LINE_INTEGRAL_POINTS)
SWEEP_MESH = (False, "es")                   # synthetic(6, 5, axi, physics) of the samples-per-segment sweep
SWEEP_CONTOURS = ("one", "two", "arc")
