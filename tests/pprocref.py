"""Restatements for the post-processor tests (CPU, numpy): the reference's
addContourPointFromNode (PostProcessor.cpp:173-298) on complex numbers, with
the one deliberate difference of the project's version -- the last step of an
arc is the input point itself -- and d_PlotBounds of OpenDocument
(epproc.cpp:184-225) with the reference's starting elements."""
import math

import numpy as np

PI = 3.141592653589793238462643383


def geometry(points, segments=(), arcs=()):
    """arcs: (n0, n1, ArcLength, MaxSideLength), degrees."""
    a = np.asarray(arcs, float).reshape(-1, 4)
    return dict(points=np.asarray(points, float).reshape(-1, 2), segments=np.asarray(segments, np.int32).reshape(-1, 2),
                arcs=a[:, :2].astype(np.int32), arc_length=a[:, 2].copy(), arc_maxside=a[:, 3].copy())


def fee_geometry_lines(g):
    """The geometry sections of a .fee / .feh for g."""
    out = ["[NumPoints] = %d" % len(g["points"])]
    out += ["%.17g\t%.17g\t0\t0\t0" % (x, y) for x, y in g["points"]]
    out += ["[NumSegments] = %d" % len(g["segments"])]
    out += ["%d\t%d\t-1\t0\t0\t0\t0" % (a, b) for a, b in g["segments"]]
    out += ["[NumArcSegments] = %d" % len(g["arcs"])]
    out += ["%d\t%d\t%.17g\t%.17g\t0\t0\t0\t0" % (a, b, l, m)
            for (a, b), l, m in zip(g["arcs"], g["arc_length"], g["arc_maxside"])]
    out += ["[NumHoles] = 0"]
    return out


def solution_text(kind, kw, V, Q=None, cond=(), geom=None, label_xy=None, unit=1.0):
    """A .res / .anh as the solvers write it: the header of kw (x, y in the
    solver's unit; the file carries x / unit), then [Solution]."""
    from xfemm_amd import synth
    head = synth.potential_text(kind, kw)
    if geom is not None:
        old = "[NumPoints] = 0\n[NumSegments] = 0\n[NumArcSegments] = 0\n[NumHoles] = 0\n"
        assert old in head
        head = head.replace(old, "\n".join(fee_geometry_lines(geom)) + "\n")
    if label_xy is not None:
        lines = head.splitlines()
        k = max(i for i, l in enumerate(lines) if l.startswith("[NumBlockLabels]"))
        for j, (lx, ly) in enumerate(label_xy):
            f = lines[k + 1 + j].split("\t")
            lines[k + 1 + j] = "\t".join(["%.17g" % lx, "%.17g" % ly] + f[2:])
        head = "\n".join(lines) + "\n"
    x, y = np.asarray(kw["x"], float) / unit, np.asarray(kw["y"], float) / unit
    p = np.asarray(kw["p"]).reshape(-1, 3)
    Q = -2 * np.ones(len(x), int) if Q is None else Q
    out = [head + "[Solution]", "%d" % len(x)]
    out += ["%.17g\t%.17g\t%.17g\t%d" % (a, b, v, q) for a, b, v, q in zip(x, y, V, Q)]
    out += ["%d" % len(p)] + ["%d\t%d\t%d\t%d" % (a, b, c, l) for (a, b, c), l in zip(p, kw["lbl"])]
    out += ["%d" % len(cond)] + ["%.17g\t%.17g" % (a, b) for a, b in cond]
    return "\n".join(out) + "\n"


def circle(g, k):
    P = g["points"][:, 0] + 1j * g["points"][:, 1]
    a0, a1 = P[g["arcs"][k][0]], P[g["arcs"][k][1]]
    d = abs(a1 - a0)
    tta = g["arc_length"][k] * PI / 180.
    R = d / (2. * math.sin(tta / 2.))
    return a0 + (d / 2. + 1j * math.sqrt(R * R - d * d / 4.)) * ((a1 - a0) / d), R


def add_from_node(g, contour, mx, my):
    """contour: a list of complex, extended in place."""
    P = g["points"][:, 0] + 1j * g["points"][:, 1]
    if len(P) == 0:
        return contour
    m = complex(mx, my)
    n0 = int(np.argmin(np.abs(P - m)))
    z = P[n0]
    if not contour:
        contour.append(z)
        return contour
    y = contour[-1]
    if y == z:
        return contour
    n1 = int(np.argmin(np.abs(P - y)))
    best, d1 = None, 1.e08
    if abs(P[n1] - y) < 1.e-08:
        for k, (a, b) in enumerate(g["segments"]):
            if {int(a), int(b)} == {n0, n1} and a != b:
                p0, p1 = P[a], P[b]
                t = ((m - p0) * (p1 - p0).conjugate()).real / abs(p1 - p0) ** 2
                d2 = abs(m - (p0 + min(1., max(0., t)) * (p1 - p0)))
                if d2 < d1:
                    best, d1 = ("line", k, False), d2
        for k, (a, b) in enumerate(g["arcs"]):
            for rev in (True, False):
                if (int(a), int(b)) == ((n1, n0) if rev else (n0, n1)):
                    c, R = circle(g, k)
                    d = abs(m - c)
                    if d == 0:
                        d2 = R
                    else:
                        t = (m - c) / d
                        ang = np.angle(t / (P[a] - c)) * 180 / PI
                        d2 = abs(m - c - R * t) if 0 < ang < g["arc_length"][k] else min(abs(m - P[a]), abs(m - P[b]))
                    if d2 < d1:
                        best, d1 = ("arc", k, rev), d2

    def behind(q):
        return len(contour) > 1 and abs(contour[-2] - q) < 1.e-08

    if best is None:
        contour.append(z)
    elif best[0] == "line":
        if not behind(z):
            contour.append(z)
    else:
        _, k, rev = best
        c, _ = circle(g, k)
        n = int(math.ceil(g["arc_length"][k] / g["arc_maxside"][k]))
        rot = np.exp((1j if rev else -1j) * g["arc_length"][k] * PI / (180. * n))
        for i in range(n):
            y = (y - c) * rot + c
            if i == n - 1:
                y = z
            if behind(y):
                break
            contour.append(y)
    return contour


def cabs(re, im):
    """abs(CComplex) (femmcomplex.cpp:749-757), elementwise."""
    re, im = np.asarray(re, float), np.asarray(im, float)
    out = np.zeros(re.shape)
    a = np.abs(re) > np.abs(im)
    nz = ~((re == 0) & (im == 0))
    with np.errstate(divide="ignore", invalid="ignore"):
        out = np.where(a, np.abs(re) * np.sqrt(1. + (im / re) * (im / re)), np.abs(im) * np.sqrt(1. + (re / im) * (re / im)))
    return np.where(nz, out, 0.)


def plot_bounds(V, D, E, external):
    """V per node; D, E (n, 2) per element; external: bool per element."""
    d, e = cabs(D[:, 0], D[:, 1]), cabs(E[:, 0], E[:, 1])
    ext = int(np.count_nonzero(external))
    dlo = dhi = d[ext if ext < len(d) else 0]
    elo = ehi = e[0]
    inner = ~np.asarray(external, bool)
    if inner.any():
        dhi, dlo = max(dhi, d[inner].max()), min(dlo, d[inner].min())
        ehi, elo = max(ehi, e[inner].max()), min(elo, e[inner].min())
    return np.array([[V.min(), V.max()], [dlo, dhi], [elo, ehi]])


class Walk:
    """PostProcessor::InTriangle (PostProcessor.cpp:300-355): the search from
    the element found last, outwards in both directions, over the elements
    whose circle about the centroid holds the point."""

    def __init__(self, X, Y, p):
        self.X, self.Y, self.p = np.asarray(X, float), np.asarray(Y, float), np.asarray(p).reshape(-1, 3)
        X, Y, p = self.X, self.Y, self.p
        self.cx = X[p[:, 0]] / 3. + X[p[:, 1]] / 3. + X[p[:, 2]] / 3.
        self.cy = Y[p[:, 0]] / 3. + Y[p[:, 1]] / 3. + Y[p[:, 2]] / 3.
        self.rs = np.max((X[p] - self.cx[:, None]) ** 2 + (Y[p] - self.cy[:, None]) ** 2, axis=1)
        self.k = 0

    def holds(self, x, y, i):
        X, Y, p = self.X, self.Y, self.p
        for j in range(3):
            a, b = p[i, j], p[i, (j + 1) % 3]
            if b > a:
                if (X[b] - X[a]) * (y - Y[a]) - (Y[b] - Y[a]) * (x - X[a]) < 0:
                    return False
            elif (X[a] - X[b]) * (y - Y[b]) - (Y[a] - Y[b]) * (x - X[b]) > 0:
                return False
        return True

    def find(self, x, y):
        sz = len(self.p)
        k = self.k if 0 <= self.k < sz else 0
        self.k = k
        if self.holds(x, y, k):
            return k
        hi = lo = k
        for _ in range(0, sz, 2):
            hi = hi + 1 if hi + 1 < sz else 0
            lo = lo - 1 if lo > 0 else sz - 1
            for e in (hi, lo):
                if (self.cx[e] - x) ** 2 + (self.cy[e] - y) ** 2 <= self.rs[e] and self.holds(x, y, e):
                    self.k = e
                    return e
        return -1
