"""A plain-Python restatement of the reference's magnetostatic point values and
contour integrals at Frequency 0, planar and axisymmetric, in IEEE double
without fused multiply-adds:

    GetNodalB        fpproc.cpp:2704-2967
    GetPointValues   fpproc.cpp:2257-2498 with GetPointB (2669-2702),
                     FPProc::GetMu (5322-5328) over CMMaterialProp::GetMu
                     (CMaterialProp.cpp:775-844)
    LineIntegral     fpproc.cpp:4094-4515
    InTriangle       fpproc.cpp:2180-2235, InTriangleTest 3387-3424

on top of tests/magpostref.py (element B, energies, the label's circuit
columns).  The element search has two modes: "reference" (InTriangle's walk
from its static k; LineIntegral's walk over the neighbours of the previous
sample's element) and "lowest" (the lowest-numbered containing element, what
the device returns).  They differ only for a point exactly on an edge or node.

Where oracle/pointvalues.py -- the planar restatement the recorded field values
of the reference were checked with -- associates differently from fpproc.cpp,
its order is followed (as the device does): an interface's tangential and
normal parts are added to each other first, and a corner value is multiplied by
its weight already divided by da.
"""
import math

import numpy as np

import magpostref
from magpostref import MUO, PI, cabs

POINT_NAMES = ("A", "B1", "B2", "mu1", "mu2", "H1", "H2", "Js", "c", "E", "Hc_re", "Hc_im", "ff")

# branches of GetNodalB, as nodal_b records them
PATCH, INTERFACE, PUNT, SHARP = "patch", "interface", "punt", "sharp"


def get_mu(bp, b1, b2):
    """CMMaterialProp::GetMu(double ...), CMaterialProp.cpp:775-844 (MuMax == 0)"""
    muo = MUO
    LamFill = bp["LamFill"]
    mu1 = mu2 = muo
    if len(bp["B"]) == 0:
        if bp["LamType"] == 0:
            mu1 = ((1. + LamFill * (bp["mu_x"] - 1.)) * muo)
            mu2 = ((1. + LamFill * (bp["mu_y"] - 1.)) * muo)
        if bp["LamType"] == 1:
            mu1 = ((1. + LamFill * (bp["mu_x"] - 1.)) * muo)
            mu2 = 1. / (LamFill / (bp["mu_y"] * muo) + (1. - LamFill) / muo)
        if bp["LamType"] == 2:
            mu2 = ((1. + LamFill * (bp["mu_y"] - 1.)) * muo)
            mu1 = 1. / (LamFill / (bp["mu_x"] * muo) + (1. - LamFill) / muo)
    else:
        s0 = bp["slope"][0]
        if bp["LamType"] == 0:
            biron = math.sqrt(b1 * b1 + b2 * b2)
            mu1 = 1. / s0 if biron < 1.e-08 else biron / magpostref.get_h(bp, biron)
            mu2 = mu1
        if bp["LamType"] == 1:
            biron = math.sqrt((b1 / LamFill) * (b1 / LamFill) + b2 * b2)
            muiron = 1. / s0 if biron < 1.e-08 else biron / magpostref.get_h(bp, biron)
            mu1 = muiron * LamFill
            mu2 = 1. / (LamFill / muiron + (1. - LamFill) / muo)
        if bp["LamType"] == 2:
            biron = math.sqrt((b2 / LamFill) * (b2 / LamFill) + b1 * b1)
            muiron = 1. / s0 if biron < 1.e-08 else biron / magpostref.get_h(bp, biron)
            mu2 = muiron * LamFill
            mu1 = 1. / (LamFill / muiron + (1. - LamFill) / muo)
    return mu1 / muo, mu2 / muo


class MagPoint:
    """Point values and contour integrals of one opened solution (a
    magpostref.MagPost).  point_j: per node, non-zero where the node's point
    property carries a current."""

    def __init__(self, post, point_j=None):
        self.post = post
        self.X = [float(v) for v in post.X]
        self.Y = [float(v) for v in post.Y]
        self.A = [float(v) for v in post.A]
        self.p = [[int(v) for v in row] for row in post.p]
        self.lbl = [int(v) for v in post.lbl]
        self.blk = [int(post.labels[l]["block"]) for l in self.lbl]
        self.magdir = [float(v) for v in post.magdir]
        self.lc, self.axi, self.depth = post.lc, post.axi, post.depth
        self.point_j = np.zeros(len(self.X), bool) if point_j is None else np.asarray(point_j) != 0
        B = post.element_b_all()
        self.B1 = [float(v) for v in B[:, 0]]
        self.B2 = [float(v) for v in B[:, 1]]
        ne = len(self.p)
        # Ctr (fpproc.cpp:3426-3438) and rsqr (:1622-1630)
        self.cx, self.cy = [0.] * ne, [0.] * ne
        for e in range(ne):
            cx = cy = 0.
            for j in range(3):
                cx += self.X[self.p[e][j]] / 3.
                cy += self.Y[self.p[e][j]] / 3.
            self.cx[e], self.cy[e] = cx, cy
        self.rsqr = [max((self.X[n] - self.cx[e]) ** 2 + (self.Y[n] - self.cy[e]) ** 2 for n in self.p[e])
                     for e in range(ne)]
        # ConList: the elements around each node, ascending (:1766-1786)
        self.con = [[] for _ in self.X]
        for e in range(ne):
            for n in self.p[e]:
                self.con[n].append(e)
        self.k = 0                # InTriangle's static start element
        self.branches = set()     # the GetNodalB branches taken so far
        self._nodal = {}

    # -- the element search --------------------------------------------------

    def in_triangle_test(self, x, y, i):   # :3387-3424
        X, Y, p = self.X, self.Y, self.p[i]
        for j in range(3):
            k = (j + 1) % 3
            if p[k] > p[j]:
                z = (X[p[k]] - X[p[j]]) * (y - Y[p[j]]) - (Y[p[k]] - Y[p[j]]) * (x - X[p[j]])
                if z < 0:
                    return False
            else:
                z = (X[p[j]] - X[p[k]]) * (y - Y[p[k]]) - (Y[p[j]] - Y[p[k]]) * (x - X[p[k]])
                if z > 0:
                    return False
        return True

    def _buckets(self):
        """cells over the bounding box -> the elements whose (slightly widened)
        bounding box touches them, ascending"""
        X, Y = np.array(self.X), np.array(self.Y)
        p = np.array(self.p)
        x0, x1, y0, y1 = X.min(), X.max(), Y.min(), Y.max()
        n = max(1, int(math.sqrt(len(p) / 2.)))
        hx, hy = max(x1 - x0, 1e-300) / n, max(y1 - y0, 1e-300) / n
        pad = 1e-9 * max(x1 - x0, y1 - y0, abs(x0), abs(x1), abs(y0), abs(y1))
        cell = lambda v, v0, h: min(n - 1, max(0, int(math.floor((v - v0) / h))))
        grid = {}
        for e in range(len(p)):
            ex, ey = X[p[e]], Y[p[e]]
            for cy in range(cell(ey.min() - pad, y0, hy), cell(ey.max() + pad, y0, hy) + 1):
                for cx in range(cell(ex.min() - pad, x0, hx), cell(ex.max() + pad, x0, hx) + 1):
                    grid.setdefault((cx, cy), []).append(e)
        self._grid = (grid, x0, y0, hx, hy, cell)

    def find_lowest(self, x, y):
        """the lowest-numbered element containing (x, y), or -1"""
        if not hasattr(self, "_grid"):
            self._buckets()
        grid, x0, y0, hx, hy, cell = self._grid
        if x != x or y != y:
            return -1
        for e in grid.get((cell(x, x0, hx), cell(y, y0, hy)), ()):
            if self.in_triangle_test(x, y, e):
                return e
        return -1

    def in_triangle(self, x, y):   # :2180-2235
        sz = len(self.p)
        if self.k < 0 or self.k >= sz:
            self.k = 0
        if self.in_triangle_test(x, y, self.k):
            return self.k
        hi = lo = self.k
        for _ in range(0, sz, 2):
            hi += 1
            if hi >= sz:
                hi = 0
            lo -= 1
            if lo < 0:
                lo = sz - 1
            for c in (hi, lo):
                z = (self.cx[c] - x) * (self.cx[c] - x) + (self.cy[c] - y) * (self.cy[c] - y)
                if z <= self.rsqr[c] and self.in_triangle_test(x, y, c):
                    self.k = c
                    return c
        return -1

    def find(self, x, y, mode="lowest"):
        return self.find_lowest(x, y) if mode == "lowest" else self.in_triangle(x, y)

    # -- GetNodalB -------------------------------------------------------------

    def _same_material(self, e, m):   # the m++ test of :2725-2738 (Frequency 0)
        if self.lbl[e] == self.lbl[m]:
            return True
        be, bm = self.post.blocks[self.blk[e]], self.post.blocks[self.blk[m]]
        if (be["mu_x"] == bm["mu_x"] and be["mu_y"] == bm["mu_y"] and be["H_c"] == bm["H_c"] and
                self.magdir[e] == self.magdir[m]):
            return True
        return self.blk[e] == self.blk[m] and self.magdir[e] == self.magdir[m]

    def _interface(self, e, k, pt):
        """the interface side k-pt seen from element e (:2799-2823)"""
        X, Y = self.X, self.Y
        tnx, tny = X[pt] - X[k], Y[pt] - Y[k]
        r = (X[pt] + X[k]) * self.lc / 2.
        atn = cabs(tnx, tny)
        bn = (self.A[pt] - self.A[k]) / (atn * self.lc)
        if self.axi:
            bn /= (-2. * PI * r)
        z = 0.5 / atn
        tnx, tny = tnx / atn, tny / atn
        bt = self.B1[e] * tnx + self.B2[e] * tny
        return z, z * tnx * bt + z * tny * bn, z * tny * bt - z * tnx * bn, (tnx, tny)

    def _next(self, e, k, ccw):
        pe = self.p[e]
        pt = 0
        for j in range(3):
            if pe[j] == k:
                pt = j
        pt = pe[(pt - 1) % 3 if ccw else (pt + 1) % 3]
        nxt = -1
        for m in self.con[k]:
            if m != e and pt in self.p[m]:
                nxt = m
        return pt, nxt

    def nodal_b(self, elm):
        """GetNodalB for the three corners of element elm: [(b1, b2)] * 3"""
        if elm in self._nodal:
            return self._nodal[elm]
        X, Y = self.X, self.Y
        out = []
        for i in range(3):
            k = self.p[elm][i]
            con = self.con[k]
            m = sum(1 for e in con if self._same_material(elm, e))
            if m == len(con):
                self.branches.add(PATCH)
                R = b1 = b2 = 0.0
                for e in con:
                    z = 1. / cabs(X[k] - self.cx[e], Y[k] - self.cy[e])
                    R += z
                    b1 += z * self.B1[e]
                    b2 += z * self.B2[e]
                b1, b2 = b1 / R, b2 / R
            else:
                R = b1 = b2 = 0.0
                v1 = v2 = (0.0, 0.0)
                punt = False
                e = elm
                for _ in range(len(con)):
                    pt, nxt = self._next(e, k, True)
                    if nxt == -1:
                        b1, b2 = self.B1[e], self.B2[e]
                        v1 = v2 = (1.0, 0.0)
                        punt = True
                        break
                    if self.lbl[elm] != self.lbl[nxt]:
                        z, d1, d2, v1 = self._interface(e, k, pt)
                        R += z
                        b1 += d1
                        b2 += d2
                        break
                    e = nxt
                if v2 == (0.0, 0.0):
                    e = elm
                    for _ in range(len(con)):
                        pt, nxt = self._next(e, k, False)
                        if nxt == -1:
                            b1, b2 = self.B1[e], self.B2[e]
                            v1 = v2 = (1.0, 0.0)
                            punt = True
                            break
                        if self.lbl[elm] != self.lbl[nxt]:
                            z, d1, d2, v2 = self._interface(e, k, pt)
                            R += z
                            b1 += d1
                            b2 += d2
                            break
                        e = nxt
                    b1, b2 = b1 / R, b2 / R
                self.branches.add(PUNT if punt else INTERFACE)
                flag = (cabs(*v1) < 0.9 or cabs(*v2) < 0.9) or (-v1[0] * v2[0] - v1[1] * v2[1]) > 0.985
                if not flag:
                    self.branches.add(SHARP)
                    bn = 0.0
                    for e in con:
                        if self.lbl[elm] == self.lbl[e]:
                            bt = math.sqrt(self.B1[e] * self.B1[e] + self.B2[e] * self.B2[e])
                            if bt > bn:
                                bn = bt
                    R = math.sqrt(self.B1[elm] * self.B1[elm] + self.B2[elm] * self.B2[elm])
                    if R != 0:
                        b1, b2 = bn / R * self.B1[elm], bn / R * self.B2[elm]
                    else:
                        b1 = b2 = 0.0
            if self.point_j[k]:
                b1, b2 = self.B1[elm], self.B2[elm]
            if self.axi and abs(X[k]) < 1.e-06:
                b1 = 0.
            out.append((b1, b2))
        self._nodal[elm] = out
        return out

    def corner_b(self):
        """(n_elems, 3, 2): nodal_b of every element"""
        return np.array([self.nodal_b(e) for e in range(len(self.p))]).reshape(-1, 3, 2)

    # -- GetPointValues ----------------------------------------------------------

    def point_values_at(self, x, y, k, smooth=True):
        """the 13 values of POINT_NAMES at (x, y) of element k"""
        post = self.post
        n = self.p[k]
        X = [self.X[j] for j in n]
        Y = [self.Y[j] for j in n]
        An = [self.A[j] for j in n]
        lab = post.labels[self.lbl[k]]
        bp = post.blocks[self.blk[k]]
        lc = self.lc
        a = [X[1] * Y[2] - X[2] * Y[1], X[2] * Y[0] - X[0] * Y[2], X[0] * Y[1] - X[1] * Y[0]]
        b = [Y[1] - Y[2], Y[2] - Y[0], Y[0] - Y[1]]
        c = [X[2] - X[1], X[0] - X[2], X[1] - X[0]]
        da = (b[0] * c[1] - b[1] * c[0])
        ravg = lc * (X[0] + X[1] + X[2]) / 3.
        if not smooth:
            B1, B2 = self.B1[k], self.B2[k]
        else:
            nb = self.nodal_b(k)
            B1 = B2 = 0.
            for i in range(3):
                w = (a[i] + b[i] * x + c[i] * y) / da
                B1 += nb[i][0] * w
                B2 += nb[i][1] * w
        A = 0.
        if not self.axi:
            for i in range(3):
                A += An[i] * (a[i] + b[i] * x + c[i] * y) / (da)
        else:
            R = X
            v = [0.] * 6
            v[0], v[2], v[4] = An[0], An[1], An[2]
            if R[0] < 1.e-06 and R[1] < 1.e-06:
                v[1] = (v[0] + v[2]) / 2.
            else:
                v[1] = (R[1] * (3. * v[0] + v[2]) + R[0] * (v[0] + 3. * v[2])) / (4. * (R[0] + R[1]))
            if R[1] < 1.e-06 and R[2] < 1.e-06:
                v[3] = (v[2] + v[4]) / 2.
            else:
                v[3] = (R[2] * (3. * v[2] + v[4]) + R[1] * (v[2] + 3. * v[4])) / (4. * (R[1] + R[2]))
            if R[2] < 1.e-06 and R[0] < 1.e-06:
                v[5] = (v[4] + v[0]) / 2.
            else:
                v[5] = (R[0] * (3. * v[4] + v[0]) + R[2] * (v[4] + 3. * v[0])) / (4. * (R[2] + R[0]))
            pp = (b[1] * x + c[1] * y + a[1]) / da
            q = (b[2] * x + c[2] * y + a[2]) / da
            A = (v[0] - pp * (3. * v[0] - 4. * v[1] + v[2]) + 2. * pp * pp * (v[0] - 2. * v[1] + v[2]) -
                 q * (3. * v[0] + v[4] - 4. * v[5]) + 2. * q * q * (v[0] + v[4] - 2. * v[5]) +
                 4. * pp * q * (v[0] - v[1] + v[3] - v[5]))
        mu1, mu2 = get_mu(bp, B1, B2)
        aecf = 1.
        if self.axi and lab.get("is_external", 0):     # AECF(k), fpproc.cpp:5286-5304
            ro, ri, zo = post.ext
            qq = cabs(self.cx[k], self.cy[k] - zo)
            aecf = (qq * qq * ri) / (ro * ro * ro)
        mu1 /= aecf
        mu2 /= aecf
        H1 = B1 / (mu1 * MUO)
        H2 = B2 / (mu2 * MUO)
        Js = bp["J_re"]
        l = self.lbl[k]
        if post.lab_case[l] >= 0:
            if post.lab_case[l] == 0:
                if not self.axi:
                    Js -= bp["Cduct"] * post.lab_dV[l]
                else:
                    R = [0.] * 3
                    for tn in range(3):
                        R[tn] = X[tn]
                        if R[tn] < 1.e-6:
                            R[tn] = ravg
                        else:
                            R[tn] *= lc
                    ravg = 0.
                    for tn in range(3):
                        ravg += (1. / R[tn]) * (a[tn] + b[tn] * x + c[tn] * y) / (da)
                    Js -= bp["Cduct"] * post.lab_dV[l] * ravg
            else:
                Js += post.lab_J[l]
        E = magpostref.do_energy(bp, B1, B2)
        Hcr = Hci = 0.
        if bp["H_c"] != 0:
            t = self.magdir[k] * PI / 180.
            Hcr = bp["H_c"] * math.cos(t)
            Hci = bp["H_c"] * math.sin(t)
            H1 = H1 - Hcr
            H2 = H2 - Hci
            E = 0.5 * MUO * (mu1 * H1 * H1 + mu2 * H2 * H2)
        ff = 1. if lab.get("is_wound", 0) else -1.
        return [A, B1, B2, mu1, mu2, H1, H2, Js, bp["Cduct"], E, Hcr, Hci, ff]

    def point_values(self, x, y, smooth=True, mode="lowest"):
        """(elem, values (n, 13)) of the points; NaN where no element holds one"""
        x, y = np.atleast_1d(x), np.atleast_1d(y)
        el = np.zeros(len(x), np.int64)
        out = np.full((len(x), len(POINT_NAMES)), np.nan)
        for t in range(len(x)):
            el[t] = self.find(float(x[t]), float(y[t]), mode)
            if el[t] >= 0:
                out[t] = self.point_values_at(float(x[t]), float(y[t]), int(el[t]), smooth)
        return el, out

    # -- LineIntegral -------------------------------------------------------------

    def contour_samples(self, contour, npts=400, mode="lowest"):
        """the sample points of types 1 3 4 5 and the element of each:
        (xy (ns, 2), elem (ns,), per sample (tr, ti, nr, ni, dz))"""
        pts = [(float(q[0]), float(q[1])) for q in contour]
        xy, el, geo = [], [], []
        for k in range(1, len(pts)):
            (x0, y0), (x1, y1) = pts[k - 1], pts[k]
            dx, dy = x1 - x0, y1 - y0
            ln = cabs(dx, dy)
            dz = ln / float(npts)
            elm = -1
            for i in range(npts):
                u = (float(i) + 0.5) / float(npts)
                ptx, pty = x0 + u * dx, y0 + u * dy
                tr, ti = dx / ln, dy / ln
                nr, ni = 0. * tr - 1. * ti, 0. * ti + 1. * tr
                ptx += nr * 1.e-06
                pty += ni * 1.e-06
                if mode == "lowest":
                    elm = self.find_lowest(ptx, pty)
                elif elm < 0:
                    elm = self.in_triangle(ptx, pty)
                elif not self.in_triangle_test(ptx, pty, elm):
                    flag = False
                    j = 0
                    while j < 3 and not flag:
                        m = 0
                        # (elm changes inside the loop, as in the reference)
                        while m < len(self.con[self.p[elm][j]]):
                            elm = self.con[self.p[elm][j]][m]
                            if self.in_triangle_test(ptx, pty, elm):
                                flag = True
                                break
                            m += 1
                        j += 1
                    if not flag:
                        elm = self.in_triangle(ptx, pty)
                xy.append((ptx, pty))
                el.append(elm)
                geo.append((tr, ti, nr, ni, dz))
        return np.array(xy).reshape(-1, 2), np.array(el, np.int64), geo

    def contour_length(self, contour):
        pts = [(float(q[0]), float(q[1])) for q in contour]
        l = 0.
        for i in range(len(pts) - 1):
            l += cabs(pts[i + 1][0] - pts[i][0], pts[i + 1][1] - pts[i][1])
        l *= self.lc
        area = 0.
        if self.axi:
            for i in range(len(pts) - 1):
                area += (PI * (pts[i][0] + pts[i + 1][0]) * cabs(pts[i + 1][0] - pts[i][0], pts[i + 1][1] - pts[i][1]))
            area *= math.pow(self.lc, 2.)
        return l, area

    def line_integral(self, contour, kind, smooth=True, npts=400, mode="lowest"):
        """LineIntegral of one contour: dict(z=(z0, z1), scale=(s0, s1) the sums
        of the absolute terms, missed, elem)"""
        pts = [(float(q[0]), float(q[1])) for q in contour]
        lc, Depth = self.lc, self.depth
        l, area = self.contour_length(pts)
        if kind == 0:
            e0 = self.find(pts[0][0], pts[0][1], mode)
            e1 = self.find(pts[-1][0], pts[-1][1], mode)
            a0 = self.point_values_at(pts[0][0], pts[0][1], e0, False)[0] if e0 >= 0 else math.nan
            a1 = self.point_values_at(pts[-1][0], pts[-1][1], e1, False)[0] if e1 >= 0 else math.nan
            if not self.axi:
                z0 = (a0 - a1) * Depth
                z1 = z0 / (l * Depth) if l != 0 else 0.
                sc = (abs(a0) + abs(a1)) * Depth
            else:
                z0 = a1 - a0
                z1 = z0 / area if area != 0 else 0.
                sc = abs(a0) + abs(a1)
            return dict(z=(z0, z1), scale=(sc, sc), missed=(e0 < 0) + (e1 < 0), elem=np.array([e0, e1]))
        if kind == 2:
            return dict(z=(l, area if self.axi else l * Depth), scale=(l, l), missed=0, elem=np.zeros(0, np.int64))
        xy, el, geo = self.contour_samples(pts, npts, mode)
        z0 = z1 = s0 = s1 = 0.
        missed = 0
        for (ptx, pty), k, (tr, ti, nr, ni, dz) in zip(xy, el, geo):
            if k < 0:
                missed += 1
                continue
            o = self.point_values_at(float(ptx), float(pty), int(k), smooth)
            B1, B2, H1, H2 = o[1], o[2], o[5], o[6]
            t0 = t1 = 0.
            if kind == 1:
                Ht = tr * H1 + ti * H2
                t0 = (Ht * dz * lc)
            elif kind == 5:
                Bn = nr * B1 + ni * B2
                t0 = (Bn * Bn * dz * lc)
            else:
                Hn = nr * H1 + ni * H2
                Bn = nr * B1 + ni * B2
                BH = B1 * H1 + B2 * H2
                dF1 = H1 * Bn + B1 * Hn - nr * BH
                dF2 = H2 * Bn + B2 * Hn - ni * BH
                if kind == 3:
                    dza = dz * lc
                    if self.axi:
                        dza *= 2. * PI * float(ptx) * lc
                        dF1 = 0.
                    else:
                        dza *= Depth
                    t0 = (dF1 * dza / 2.)
                    t1 = (dF2 * dza / 2.)
                elif not self.axi:      # type 4; 0 on an axisymmetric problem
                    dT = float(ptx) * dF2 - dF1 * float(pty)
                    dza = dz * lc * lc
                    t0 = (dT * dza * Depth / 2.)
            z0 += t0
            z1 += t1
            s0 += abs(t0)
            s1 += abs(t1)
        if kind in (1, 5):
            z1 = z0 / l if l != 0 else 0.
            s1 = s0 / l if l != 0 else 0.
        return dict(z=(z0, z1), scale=(s0, s1), missed=missed, elem=el, xy=xy)
