"""Post-processing test helpers (CPU): a literal numpy restatement of what the
reference's epproc and hpproc compute from a solved electrostatic or heat-flow
problem -- getElementD, E(elem) and AECF (epproc.cpp:726-763,
hpproc.cpp:368-395, 851-863, PostProcessor.cpp:865-891), the counter-clockwise
node lists (epproc.cpp:140-182), getNodalD (PostProcessor.cpp:894-1092),
blockIntegral types 0-4 (epproc.cpp:268-397, hpproc.cpp:584-646),
InTriangleTest by brute force (PostProcessor.cpp:359-398), getPointD and
getPointValues (PostProcessor.cpp:1153-1188, epproc.cpp:434-469,
hpproc.cpp:332-366).

A problem is the keyword dictionary of kernels.ElectrostaticProblem or
kernels.HeatFlowProblem (tests/electro.py, tests/heat.py): coordinates in the
solver's unit (mm, m).  The post-processors work in the problem's own length
units, so the coordinates are divided back by the solver's unit first, as the
device does."""
from __future__ import annotations

import math
import re

import numpy as np

import electro
import heat

EO = 8.85418781762e-12
PI = 3.141592653589793238462643383
LENGTH_CONV = (0.0254, 0.001, 0.01, 1., 2.54e-5, 1.e-6)   # PostProcessor: user units -> m


def cabs(re_, im_):
    """abs(CComplex) (femmcomplex.cpp:749-757)."""
    if re_ == 0 and im_ == 0:
        return 0.
    if abs(re_) > abs(im_):
        return abs(re_) * math.sqrt(1. + (im_ / re_) * (im_ / re_))
    return abs(im_) * math.sqrt(1. + (re_ / im_) * (re_ / im_))


def carg(re_, im_):
    if re_ == 0 and im_ == 0:
        return 0.
    return math.atan2(im_, re_)


def cdiv(xr, xi, zr, zi):
    """operator/(CComplex, CComplex) (femmcomplex.cpp:456-474)."""
    with np.errstate(all="ignore"):
        zr, zi = np.float64(zr), np.float64(zi)
        if abs(zr) > abs(zi):
            c = zi / zr
            yr = 1. / (zr * (1. + c * c))
            yi = (-c) * yr
        else:
            c = zr / zi
            yi = (-1.) / (zi * (1. + c * c))
            yr = (-c) * yi
        return float(xr * yr - xi * yi), float(xr * yi + xi * yr)


class Post:
    """The post-processor's state after OpenDocument for the problem kw
    (physics "es" or "hf") with the nodal solution V."""

    def __init__(self, kw: dict, V, physics: str):
        assert physics in ("es", "hf")
        self.kw, self.heat = kw, physics == "hf"
        units = heat.UNITS if self.heat else electro.UNITS
        lu = kw.get("length_units", 0)
        u = units[lu]
        self.X = [float(v) for v in np.asarray(kw["x"], float) / u]
        self.Y = [float(v) for v in np.asarray(kw["y"], float) / u]
        self.V = [float(v) for v in np.asarray(V, float)]
        self.N = len(self.X)
        self.NE = len(kw["lbl"])
        self.p = [[int(v) for v in r] for r in np.asarray(kw["p"], np.int64).reshape(self.NE, 3)]
        self.lbl = [int(v) for v in kw["lbl"]]
        self.labels, self.blocks = kw["labels"], kw["blocks"]
        self.blk = [self.labels[l]["block"] for l in self.lbl]
        self.axi = kw.get("problem_type", 0) == 1
        self.lc = LENGTH_CONV[lu]
        d = kw.get("depth", 1.0)
        self.depth = 1 if d == -1 else d * self.lc
        self.extRo, self.extRi, self.extZo = kw.get("ext_ro", 0.), kw.get("ext_ri", 0.), kw.get("ext_zo", 0.)
        self.Q = qmarks(kw)
        self.ctr = [self._ctr(i) for i in range(self.NE)]
        self.D, self.E = [], []
        for i in range(self.NE):
            self.D.append(self.get_element_d(i))
        for i in range(self.NE):
            self.E.append(self.e_of(i))
        self.con = self._conlist()
        self.branch = [[0, 0, 0] for _ in range(self.NE)]
        self.d = [self.get_nodal_d(i) for i in range(self.NE)]

    # -- geometry ------------------------------------------------------------
    def _ctr(self, i):
        cx = cy = 0.
        for j in range(3):
            cx += self.X[self.p[i][j]] / 3.
            cy += self.Y[self.p[i][j]] / 3.
        return cx, cy

    def external(self, i):
        return bool(self.labels[self.lbl[i]].get("is_external", 0))

    def aecf(self, i, pt=None):
        if not self.axi:
            return 1.
        if not self.external(i):
            return 1.
        if pt is not None:
            r = cabs(pt[0] - 0., pt[1] - self.extZo)
            if r == 0:
                return self.aecf(i)
            return (r * r) / (self.extRo * self.extRi)
        r = cabs(self.ctr[i][0] - 0., self.ctr[i][1] - self.extZo)
        return (r * r) / (self.extRo * self.extRi)

    def getk(self, i, t):
        return heat.getk(self.blocks[self.blk[i]], t)

    def mean_k(self, i):
        knx = kny = 0.
        for k in range(3):
            kx, ky = self.getk(i, self.V[self.p[i][k]])
            knx += kx / 3.
            kny += ky / 3.
        return knx, kny

    # -- element fields --------------------------------------------------------
    def get_element_d(self, k):
        n, X, Y = self.p[k], self.X, self.Y
        b = [Y[n[1]] - Y[n[2]], Y[n[2]] - Y[n[0]], Y[n[0]] - Y[n[1]]]
        c = [X[n[2]] - X[n[1]], X[n[0]] - X[n[2]], X[n[1]] - X[n[0]]]
        da = (b[0] * c[1] - b[1] * c[0])
        Er = Ei = 0.
        with np.errstate(all="ignore"):
            den = np.float64(da * self.lc)
            for i in range(3):
                Er -= float((self.V[n[i]] * b[i]) / den)
                Ei -= float((self.V[n[i]] * c[i]) / den)
        a = self.aecf(k)
        if self.heat:
            knx, kny = self.mean_k(k)
            return (Er * knx) / a, (Ei * kny) / a
        m = self.blocks[self.blk[k]]
        return (EO * (Er * m.get("ex", 1.0))) / a, (EO * (Ei * m.get("ey", 1.0))) / a

    def e_of(self, k):
        Dr, Di = self.D[k]
        a = self.aecf(k)
        with np.errstate(all="ignore"):
            if self.heat:
                knx, kny = self.mean_k(k)
                return float(np.float64(Dr) / knx * a), float(np.float64(Di) / kny * a)
            m = self.blocks[self.blk[k]]
            return (float(np.float64(Dr) / m.get("ex", 1.0) / EO * a),
                    float(np.float64(Di) / m.get("ey", 1.0) / EO * a))

    # -- the counter-clockwise lists ---------------------------------------------
    def _conlist(self):
        con = [[] for _ in range(self.N)]
        for i in range(self.NE):
            for j in range(3):
                con[self.p[i][j]].append(i)
        for i in range(self.N):
            L = con[i]
            num = len(L)
            j = 0
            while j < num:   # the reference's bubble sort, swap for swap
                swapped = False
                for k in range(num - j - 1):
                    u0 = carg(self.ctr[L[k]][0] - self.X[i], self.ctr[L[k]][1] - self.Y[i])
                    u1 = carg(self.ctr[L[k + 1]][0] - self.X[i], self.ctr[L[k + 1]][1] - self.Y[i])
                    if u0 > u1:
                        L[k], L[k + 1] = L[k + 1], L[k]
                        swapped = True
                if not swapped:
                    j = num
                j += 1
        return con

    def same_material(self, e1, e2):
        b1, b2 = self.blk[e1], self.blk[e2]
        if b1 == b2:
            return True
        m1, m2 = self.blocks[b1], self.blocks[b2]
        if not self.heat:
            return m1.get("ex", 1.0) == m2.get("ex", 1.0) and m1.get("ey", 1.0) == m2.get("ey", 1.0)
        n1 = 0 if m1.get("T") is None else len(m1["T"])
        n2 = 0 if m2.get("T") is None else len(m2["T"])
        if m1.get("kx", 1.0) == m2.get("kx", 1.0) and m1.get("ky", 1.0) == m2.get("ky", 1.0) and n1 == 0 and n2 == 0:
            return True
        if n1 > 0 and n1 == n2:
            for k in range(n1):
                if m1["T"][k] != m2["T"][k] or m1["K"][k] != m2["K"][k]:
                    return False
            return True
        return False

    # -- getNodalD -------------------------------------------------------------
    def get_nodal_d(self, N):
        X, Y, V, Q, p = self.X, self.Y, self.V, self.Q, self.p
        out = []
        for i in range(3):
            j = p[N][i]
            con = self.con[j]
            num = len(con)
            lf = rt = -1
            q = []
            eos = con.index(N)
            m = eos
            for _ in range(num):   # scan ccw
                n = con[m]
                if not self.same_material(N, n):
                    break
                nos = p[n].index(j) - 1
                if nos < 0:
                    nos = 2
                pn = p[n][nos]
                if len(q) < 20:
                    q.append(pn)
                if Q[j] != -2 and Q[pn] != -2:
                    rt = pn
                    break
                m += 1
                if m == num:
                    m = 0
            m = eos
            for _ in range(num):   # scan cw
                n = con[m]
                if not self.same_material(N, n):
                    break
                nos = p[n].index(j) + 1
                if nos > 2:
                    nos = 0
                pn = p[n][nos]
                if len(q) < 20:
                    q.append(pn)
                if Q[j] != -2 and Q[pn] != -2:
                    lf = pn
                    break
                m -= 1
                if m < 0:
                    m = num - 1
            br = 0
            if lf == rt and rt != -1 and Q[j] != -2:
                br = 1
            elif rt != -1 and Q[j] != -2 and lf == -1:
                br = 2
            elif lf != -1 and Q[j] != -2 and rt == -1:
                br = 3
            elif lf == -1 and rt == -1 and Q[j] != -2:
                br = 4
            elif lf != -1 and rt != -1 and Q[j] != -2:
                xr, xi_ = X[lf] - X[j], Y[lf] - Y[j]
                ab = cabs(xr, xi_)
                xr, xi_ = xr / ab, xi_ / ab
                yr, yi_ = X[j] - X[rt], Y[j] - Y[rt]
                ab = cabs(yr, yi_)
                yr, yi_ = yr / ab, yi_ / ab
                zr, zi = cdiv(xr, xi_, yr, yi_)
                if abs(carg(zr, zi)) > 10.0001 * PI / 180.:
                    br = 5
            val = self.D[N]
            if br == 0:
                xi = yi = ii = xx = xy = yy = iv = xv = yv = 0.
                q.append(j)
                for k in q:
                    dx = X[k] - X[j]
                    dy = Y[k] - Y[j]
                    dv = V[j] - V[k]
                    ii += 1.
                    xi += dx
                    yi += dy
                    xx += dx * dx
                    xy += dx * dy
                    yy += dy * dy
                    iv += dv
                    xv += dx * dv
                    yv += dy * dv
                det = (-(ii * xy * xy) + 2 * xi * xy * yi - xx * yi * yi - xi * xi * yy + ii * xx * yy) * self.lc
                if det == 0:
                    br = 6
                else:
                    Ex = (iv * xy * yi - xv * yi * yi - ii * xy * yv + xi * yi * yv - iv * xi * yy + ii * xv * yy) / det
                    Ey = (iv * xi * xy - ii * xv * xy + xi * xv * yi - iv * xx * yi - xi * xi * yv + ii * xx * yv) / det
                    if self.heat:
                        kx, ky = self.getk(N, V[j])
                        val = (kx * Ex, ky * Ey)
                    else:
                        mt = self.blocks[self.blk[N]]
                        a = self.aecf(N, (X[j], Y[j]))
                        val = ((mt.get("ex", 1.0) * Ex * EO) / a, (mt.get("ey", 1.0) * Ey * EO) / a)
            self.branch[N][i] = br
            out.append(val)
        return out

    # -- block integrals ---------------------------------------------------------
    def block_terms(self, selected):
        """Per selected element the seven terms the device sums: (NE_sel, 7)."""
        sel = set(int(s) for s in selected)
        lc2 = pow(self.lc, 2.) if self.heat else self.lc * self.lc
        rows = []
        for i in range(self.NE):
            if self.lbl[i] not in sel:
                continue
            n, X, Y = self.p[i], self.X, self.Y
            b0, b1 = Y[n[1]] - Y[n[2]], Y[n[2]] - Y[n[0]]
            c0, c1 = X[n[2]] - X[n[1]], X[n[0]] - X[n[2]]
            a = ((b0 * c1 - b1 * c0) / 2.) * lc2
            av = a
            if self.axi:
                r = [X[n[k]] * self.lc for k in range(3)]
                R = (r[0] + r[1] + r[2]) / 3.
                av *= (2. * PI * R)
            else:
                av *= self.depth
            Dr, Di = self.D[i]
            Er, Ei = self.E[i]
            if self.heat:
                T = 0.
                for k in range(3):
                    T += self.V[n[k]] / 3.
                t0 = av * T
            else:
                t0 = av * (Dr * Er - Di * (-Ei)) / 2.
            rows.append([t0, a, av, av * Dr, av * Di, av * Er, av * Ei])
        return np.array(rows, float).reshape(-1, 7)

    def block_integrals(self, selected):
        """(the seven results in the device's order, the sum of the absolute terms)."""
        t = self.block_terms(selected)
        s = [0.] * 7
        for row in t:   # the reference's running sums, in element order
            for c in range(7):
                s[c] += row[c]
        vol = s[2]
        out = list(s)
        if self.heat:
            out[0] = cdiv(s[0], 0., vol, 0.)[0]
        out[3], out[4] = cdiv(s[3], s[4], vol, 0.)
        out[5], out[6] = cdiv(s[5], s[6], vol, 0.)
        return np.array(out), np.abs(t).sum(axis=0)

    # -- points ------------------------------------------------------------------
    def in_triangle_test(self, x, y, i):
        X, Y = self.X, self.Y
        for j in range(3):
            k = (j + 1) % 3
            pk, pj = self.p[i][k], self.p[i][j]
            if pk > pj:
                z = (X[pk] - X[pj]) * (y - Y[pj]) - (Y[pk] - Y[pj]) * (x - X[pj])
                if z < 0:
                    return False
            else:
                z = (X[pj] - X[pk]) * (y - Y[pk]) - (Y[pj] - Y[pk]) * (x - X[pk])
                if z > 0:
                    return False
        return True

    def containing(self, x, y):
        """Every element containing (x, y), ascending (brute force, vectorised
        over the elements with the same arithmetic)."""
        if not hasattr(self, "_np"):
            p = np.array(self.p, np.int64)
            self._np = (p, np.array(self.X), np.array(self.Y))
        p, X, Y = self._np
        ok = np.ones(self.NE, bool)
        for j in range(3):
            k = (j + 1) % 3
            pj, pk = p[:, j], p[:, k]
            lo, hi = np.minimum(pj, pk), np.maximum(pj, pk)
            z = (X[hi] - X[lo]) * (y - Y[lo]) - (Y[hi] - Y[lo]) * (x - X[lo])
            ok &= np.where(pk > pj, ~(z < 0), ~(z > 0))
        hits = [int(i) for i in np.nonzero(ok)[0]]
        assert all(self.in_triangle_test(x, y, i) for i in hits)
        return hits

    def point_values(self, x, y, k, smooth):
        """getPointValues(x, y, k): the 8 values in the device's order."""
        n, X, Y = self.p[k], self.X, self.Y
        a = [X[n[1]] * Y[n[2]] - X[n[2]] * Y[n[1]], X[n[2]] * Y[n[0]] - X[n[0]] * Y[n[2]],
             X[n[0]] * Y[n[1]] - X[n[1]] * Y[n[0]]]
        b = [Y[n[1]] - Y[n[2]], Y[n[2]] - Y[n[0]], Y[n[0]] - Y[n[1]]]
        c = [X[n[2]] - X[n[1]], X[n[0]] - X[n[2]], X[n[1]] - X[n[0]]]
        da = (b[0] * c[1] - b[1] * c[0])
        with np.errstate(all="ignore"):
            da = np.float64(da)
            if not smooth:
                Dr, Di = self.D[k]
            else:
                Dr = Di = 0.
                for i in range(3):
                    w = (a[i] + b[i] * x + c[i] * y)
                    Dr += float((self.d[k][i][0] * w) / da)
                    Di += float((self.d[k][i][1] * w) / da)
            T = 0.
            for i in range(3):
                T += float(self.V[n[i]] * (a[i] + b[i] * x + c[i] * y) / da)
            ae = self.aecf(k, (x, y))
            if self.heat:
                kx, ky = self.getk(k, T)
                kx, ky = kx / ae, ky / ae
                return [T, Dr, Di, kx, ky, float(np.float64(Dr) / kx), float(np.float64(Di) / ky), 0.]
            m = self.blocks[self.blk[k]]
            ex, ey = m.get("ex", 1.0) / ae, m.get("ey", 1.0) / ae
            Er, Ei = float(np.float64(Dr) / (ex * EO)), float(np.float64(Di) / (ey * EO))
            return [T, Dr, Di, Er, Ei, ex, ey, (Dr * Er - Di * (-Ei)) / 2.]

    def points(self, xs, ys, smooth):
        """(elem, values) as the device returns them: the lowest-numbered
        containing element or -1, its 8 values or NaN."""
        el = np.full(len(xs), -1, np.int32)
        out = np.full((len(xs), 8), np.nan)
        for t, (x, y) in enumerate(zip(xs, ys)):
            hits = self.containing(float(x), float(y))
            if hits:
                el[t] = hits[0]
                out[t] = self.point_values(float(x), float(y), hits[0], smooth)
        return el, out


def qmarks(kw: dict) -> np.ndarray:
    """L.Q as the solvers leave it in the solution file (esolver.cpp:412-440,
    592-600; hsolver.cpp:501-529, 766-774)."""
    N = len(kw["x"])
    NE = len(kw["lbl"])
    p = np.asarray(kw["p"], np.int64).reshape(NE, 3)
    e = kw.get("e")
    marker, cond = kw.get("marker"), kw.get("conductor")
    points, circ, lines = list(kw.get("points", ())), list(kw.get("conductors", ())), list(kw.get("lines", ()))
    Q = np.full(N, -2, np.int64)
    for i in range(N):
        if marker is not None and marker[i] >= 0 and points[marker[i]].get("qp", 0.0) == 0:
            Q[i] = -1
        if cond is not None and cond[i] >= 0 and circ[cond[i]].get("type", 1) == 1:
            Q[i] = cond[i]
    if e is not None:
        e = np.asarray(e, np.int64).reshape(NE, 3)
        for i in range(NE):
            for j in range(3):
                if e[i, j] >= 0 and lines[e[i, j]].get("format", 0) == 0:
                    Q[p[i, j]] = -1
                    Q[p[i, (j + 1) % 3]] = -1
    for i in range(N):
        if marker is not None and marker[i] >= 0 and Q[i] == -2:
            Q[i] = -1
        if cond is not None and cond[i] >= 0:
            Q[i] = cond[i]
    return Q


def read_check(path: str) -> dict:
    """A recorded .out.check: the integral lines in order, and per smoothing
    setting the points with their named values."""
    integrals, points = [], {False: [], True: []}
    smooth = False
    cur = None
    num = r"[-+]?\d+\.\d+"
    for ln in open(path).read().splitlines():
        if ln.startswith("Field Smoothing"):
            smooth = ln.strip().endswith("ON")
        elif ln.startswith("Point vals"):
            m = re.search(r"x = (%s), y = (%s)" % (num, num), ln)
            cur = (float(m.group(1)), float(m.group(2)))
        elif cur is not None and ":" in ln and not ln.startswith("Block") and "Integral" not in ln:
            vals = {k: float(v) for k, v in re.findall(r"(\w+):\s*(%s)" % num, ln)}
            points[smooth].append((cur[0], cur[1], vals))
            cur = None
        elif "Integral" in ln:
            integrals.append((ln, [float(v) for v in re.findall(num, ln)]))
    return dict(integrals=integrals, points=points)


def synthetic(nx, ny, axi, physics):
    """A small structured problem that takes every case of the smoothing.
    Two materials meeting along x = mid, an external region on top
    (axisymmetric), fixed edges along the bottom and the left side meeting at
    90 degrees, a prescribed-value conductor along y = mid ending on the material
    line, another inside the right material, and an isolated fixed node."""
    w, h, x0, y0 = 6.0, 5.0, (1.0 if axi else 0.0), -1.0
    x, y, p = electro.grid(nx, ny, w, h, x0, y0)
    cx, cy = x[p].mean(axis=1), y[p].mean(axis=1)
    xm, ytop = x[nx // 2], y[(ny - 2) * nx]
    lbl = np.where(cy > ytop, 2, np.where(cx < xm, 0, 1)).astype(np.int32)
    labels = [dict(block=0), dict(block=1), dict(block=0, is_external=1)]
    vname = "Tset" if physics == "hf" else "V"
    cname = "T" if physics == "hf" else "V"
    e = electro.tag_edges(x, y, p, [(lambda xa, ya, xb, yb: ya == y0 and yb == y0, 0),
                                    (lambda xa, ya, xb, yb: xa == x0 and xb == x0, 0)])
    jm = ny // 2
    cond = -np.ones(len(x), np.int32)
    cond[jm * nx + 1: jm * nx + nx // 2 + 1] = 0                          # ends on the material line
    cond[[j * nx + (nx - 3) for j in range(2, jm)]] = 1                   # ends inside the right material
    marker = -np.ones(len(x), np.int32)
    marker[(jm + 2) * nx + 2] = 0                                          # an isolated fixed node
    if physics == "hf":
        blocks = [dict(kx=5.0, ky=2.0, kt=3.0, qv=0.0),
                  dict(kx=0.02, ky=0.02, kt=1.0, qv=0.0, T=np.array([0., 50., 100.]), K=np.array([0.02, 0.03, 0.05]))]
    else:
        blocks = [dict(ex=4.0, ey=2.0, qv=0.0), dict(ex=1.0, ey=1.0, qv=0.0)]
    kw = dict(x=x, y=y, p=p, lbl=lbl, e=e, blocks=blocks, labels=labels,
              lines=[{"format": 0, vname: 10.0}], points=[{cname: 3.0, "qp": 0.0}],
              conductors=[{"type": 1, cname: 5.0, "q": 0.0}, {"type": 1, cname: 7.0, "q": 0.0}],
              conductor=cond, marker=marker, length_units=2, problem_type=1 if axi else 0, depth=2.5,
              ext_ro=9.0, ext_ri=7.0, ext_zo=0.5, precision=1e-8)
    V = 20. + 3. * x - 2. * y + 0.5 * x * y + 4. * np.sin(0.9 * x) * np.cos(0.7 * y)
    return kw, V


SYNTH = [(7, 7, False, "es"), (13, 11, True, "es"), (7, 7, True, "hf"), (13, 11, False, "hf")]
