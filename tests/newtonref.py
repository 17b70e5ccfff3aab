"""A plain restatement of one Newton pass of the static element assembly
(FSolver::Static2D, static2d.cpp:352-805, and FSolver::StaticAxisymmetric,
staticaxi.cpp:172-636; CMaterialProp::GetBHProps, CMaterialProp.cpp:997-1057)
in numpy.longdouble, with an a-priori rounding bound beside every value.
Host only: no device, no oracle.

It takes the keyword arguments of kernels.Static2DProblem, so it reads the
B / H / slope tables exactly as they are uploaded.  Every formula is written
once, for one element, on arrays that hold all elements (branches by mask):
a Python loop over elements would cost seconds per pass and the device test
evaluates some fifty of them.

newton_pass(prep, V, state, first) returns the full matrix K and the right
side b before the Dirichlet and periodic treatment (the reference's sign:
AddTo(-Me), b -= be; point currents added), the new state (mu1, mu2), and per
element B, dv and the branch GetBHProps took.

The rounding bound
------------------
Every quantity is a pair (value, bound): the value in longdouble, the bound an
upper limit on |f64 evaluation - exact| of the same formula under the standard
model fl(a op b) = (a op b)(1 + d), |d| <= u = 2^-53, for inputs that are f64
numbers (bound 0).  It is carried operation by operation:

    a + b:  e_a + e_b + u |a + b|
    a * b:  |a| e_b + |b| e_a + e_a e_b + u |a b|
    a / b:  (e_a + |a / b| e_b) / (|b| - e_b) + u |a / b|
    sqrt a: e_a / (sqrt a + sqrt max(a - e_a, 0)) + u sqrt a
    log a:  e_a / (a - e_a) + 2 u |log a|;  cos, sin: 2 u (one ulp: the
            library functions are not correctly rounded)
    a sum of k terms in any order: sum e_i + (k - 1) u sum |t_i|

so a result that is the end of a chain of c roundings carries c u sum |terms|,
with the absolute sums taken through every cancelling step -- the p q
differences of the area, B1^2 + B2^2, the Hermite sums, dh / b^2 - h / b^3,
the logarithmic mean radius, the sum over a row's incident elements.  The
depth c is thereby counted by the arithmetic itself instead of by hand; for
the planar element it comes to: area 4, Mx / My 7, B 14, h and dh 12 + B's
share through z, dv 6 more, Kn 6 more, an Mn entry 4 more, an Me entry 3 more
(the two-reciprocal form Mx (1 / m2) + My (1 / m1) is restated as the device
evaluates it, so it carries its extra rounding), a matrix entry (k - 1) more
for its k incident elements.  A fused multiply-add rounds once where the
model rounds twice, so contraction stays inside the bound.  The longdouble
value's own error (2^-64 per operation) is 2^-11 of the bound.  Nothing in it
is fitted to a result.

What the bound does not cover: an iterate whose B lies within its own bound of
a knot of the B-H table may be evaluated on the neighbouring interval by an
f64 run; the Hermite interpolant is C1, so h and dh agree there to O(e) but
dh's derivative jumps.  No test iterate sits on a knot other than B = 0.
"""
import numpy as np

LD = np.longdouble
U = LD(2.0) ** -53
KC = 3.141592653589793238462643383 * 4.0e-5     # c (static2d.cpp:66)
MUO = 1.2566370614359173e-6
UNITS = (2.54, 0.1, 1.0, 100.0, 0.00254, 1.0e-04)


class Bv:
    """value and rounding bound (see the module docstring)."""
    __slots__ = ("v", "e")
    __array_ufunc__ = None      # ndarray op Bv goes to Bv's reflected operator

    def __init__(self, v, e=None):
        self.v = np.asarray(v, LD)
        self.e = np.zeros_like(self.v) if e is None else np.asarray(e, LD)

    @staticmethod
    def of(a):
        return a if isinstance(a, Bv) else Bv(a)

    def __add__(self, o):
        o = Bv.of(o)
        v = self.v + o.v
        return Bv(v, self.e + o.e + U * np.abs(v))

    __radd__ = __add__

    def __neg__(self):
        return Bv(-self.v, self.e)

    def __sub__(self, o):
        return self + (-Bv.of(o))

    def __rsub__(self, o):
        return Bv.of(o) + (-self)

    def __mul__(self, o):
        o = Bv.of(o)
        v = self.v * o.v
        return Bv(v, np.abs(self.v) * o.e + np.abs(o.v) * self.e + self.e * o.e + U * np.abs(v))

    __rmul__ = __mul__

    def __truediv__(self, o):
        o = Bv.of(o)
        with np.errstate(all="ignore"):
            v = self.v / o.v
            e = (self.e + np.abs(v) * o.e) / (np.abs(o.v) - o.e) + U * np.abs(v)
        return Bv(v, e)

    def __rtruediv__(self, o):
        return Bv.of(o) / self

    def sqrt(self):
        with np.errstate(all="ignore"):
            r = np.sqrt(self.v)
            den = r + np.sqrt(np.maximum(self.v - self.e, 0))
            e = np.where(self.e > 0, self.e / den, 0) + U * r
        return Bv(r, e)

    def abs(self):
        return Bv(np.abs(self.v), self.e)

    def log(self):
        with np.errstate(all="ignore"):
            r = np.log(self.v)
            return Bv(r, self.e / (self.v - self.e) + 2 * U * np.abs(r))

    def __getitem__(self, k):
        return Bv(self.v[k], self.e[k])

    def exact(self, c):
        """times a power of two (or -1): no rounding."""
        return Bv(self.v * c, self.e * abs(c))


def where(m, a, b):
    a, b = Bv.of(a), Bv.of(b)
    return Bv(np.where(m, a.v, b.v), np.where(m, a.e, b.e))


def put(dst, m, src):
    """dst with src's values where m."""
    return where(m, src, dst)


def total(terms):
    """A sum of len(terms) values in any order."""
    v = sum(t.v for t in terms)
    return Bv(v, sum(t.e for t in terms) + (len(terms) - 1) * U * sum(np.abs(t.v) for t in terms))


def trig(t_deg):
    """cos, sin of an angle in degrees as the host forms them (cos(t pi / 180))."""
    a = Bv(t_deg) * np.pi / 180.0
    c, s = np.cos(a.v), np.sin(a.v)
    return (Bv(c, np.abs(s) * a.e + 2 * U * np.abs(c)), Bv(s, np.abs(c) * a.e + 2 * U * np.abs(s)))


# ---- the problem as the solver holds it ----------------------------------------

class Prep:
    pass


def fixed_nodes(kw):
    """node -> prescribed V (the solver's unit), in the reference's SetValue
    order, last value kept (static2d.cpp:826-926, staticaxi.cpp:652-731)."""
    x, y = np.asarray(kw["x"], float), np.asarray(kw["y"], float)
    p, e = np.asarray(kw["p"]), kw.get("e")
    lines, points, marker = kw.get("lines", ()), kw.get("points", ()), kw.get("marker")
    unit = UNITS[kw.get("length_units", 0)]
    axi = kw.get("problem_type", 0) == 1
    out = {}
    for i in range(len(x)):
        m = -1 if marker is None else marker[i]
        if axi and abs(x[i]) < unit * 1.0e-06:
            out[i] = 0.0
        elif m >= 0 and points[m].get("J_re", 0.0) == 0 and points[m].get("J_im", 0.0) == 0:
            out[i] = points[m].get("A_re", 0.0) / KC
    if e is not None:
        e = np.asarray(e)
        for i in np.nonzero((e >= 0).any(axis=1))[0]:
            for j in range(3):
                if e[i, j] < 0 or lines[e[i, j]].get("format", 0) != 0:
                    continue
                ln = lines[e[i, j]]
                for nd in (p[i, j], p[i, (j + 1) % 3]):
                    if kw.get("coords", 0) == 0:
                        a = ln.get("A0", 0.0) + x[nd] / unit * ln.get("A1", 0.0) + y[nd] / unit * ln.get("A2", 0.0)
                    else:
                        r = np.hypot(x[nd], y[nd]) / unit
                        t = 0.0 if (x[nd] == 0 and y[nd] == 0) else np.degrees(np.arctan2(y[nd], x[nd]))
                        a = ln.get("A0", 0.0) + r * ln.get("A1", 0.0) + t * ln.get("A2", 0.0)
                    a *= np.cos(np.radians(ln.get("phi", 0.0)))
                    if not axi or x[nd] != 0:
                        out[int(nd)] = a / KC
    return out


def prepare(kw):
    """Per-element arrays of everything a pass reads; the circuit values
    (static2d.cpp:84-167, staticaxi.cpp:78-160) with their bounds."""
    if kw.get("ages") or any(lb.get("mag_dir_fctn") for lb in kw["labels"]):
        raise NotImplementedError("air-gap elements and MagDirFctn are not restated here")
    P = Prep()
    P.axi = kw.get("problem_type", 0) == 1
    P.x, P.y = np.asarray(kw["x"], float), np.asarray(kw["y"], float)
    P.p = np.asarray(kw["p"], np.int64).reshape(-1, 3)
    P.N, P.NE = len(P.x), len(P.p)
    lbl = np.asarray(kw["lbl"])
    labels, blocks = kw["labels"], kw["blocks"]
    P.blk = np.array([labels[l]["block"] for l in lbl])
    P.blocks = blocks

    def per_block(key, default):
        return np.array([b.get(key, default) for b in blocks], float)[P.blk]

    P.mu_x, P.mu_y = per_block("mu_x", 1.0), per_block("mu_y", 1.0)
    P.H_c, P.J_re, P.Cduct = per_block("H_c", 0.0), per_block("J_re", 0.0), per_block("Cduct", 0.0)
    P.fill = per_block("LamFill", 1.0)
    P.lam = np.array([b.get("LamType", 0) for b in blocks])[P.blk]
    P.bhn = np.array([len(b.get("B", ())) for b in blocks])[P.blk]
    P.external = np.array([int(lb.get("is_external", 0)) for lb in labels])[lbl] != 0
    cs = [trig(lb.get("mag_dir", 0.0)) for lb in labels]
    P.cos_m = Bv([c.v for c, _ in cs], [c.e for c, _ in cs])[lbl]
    P.sin_m = Bv([s.v for _, s in cs], [s.e for _, s in cs])[lbl]
    unit = UNITS[kw.get("length_units", 0)]
    P.ext_ro, P.ext_ri, P.ext_zo = (Bv(kw.get(k, 0.0)) * unit for k in ("ext_ro", "ext_ri", "ext_zo"))
    # mixed-condition edges: c0, c1 per (element, edge), 0 elsewhere
    P.c0, P.c1 = np.zeros((P.NE, 3)), np.zeros((P.NE, 3))
    P.mixed = np.zeros((P.NE, 3), bool)
    if kw.get("e") is not None:
        e = np.asarray(kw["e"]).reshape(-1, 3)
        for i, j in zip(*np.nonzero(e >= 0)):
            ln = kw["lines"][e[i, j]]
            if ln.get("format", 0) == 2:
                P.mixed[i, j], P.c0[i, j], P.c1[i, j] = True, ln.get("c0", 0.0), ln.get("c1", 0.0)
    # circuits: the source term t of every element
    P.circ = []
    P.t = Bv(np.zeros(P.NE))
    circ = np.array([lb.get("in_circuit", -1) for lb in labels])[lbl]
    wound = np.array([int(lb.get("is_wound", 0)) for lb in labels])[lbl] != 0
    X, Y = P.x[P.p], P.y[P.p]
    a = area(Bv(X), Bv(Y))
    R = total([Bv(X[:, 0]), Bv(X[:, 1]), Bv(X[:, 2])]) / 3.0
    for k, c in enumerate(kw.get("circuits", ())):
        m = circ == k
        cd = np.where(wound, 0.0, P.Cduct)
        n = int(m.sum())

        def tot(q):
            return Bv(q.v[m].sum(), q.e[m].sum() + max(n - 1, 0) * U * np.abs(q.v[m]).sum())

        I1 = tot(a)
        I2 = tot(a * 100.0 * cd / R) if P.axi else tot(a * cd)
        I3 = tot(Bv(P.J_re) * a * 100.0)
        ccase, J, dV = 0, Bv(0.0), Bv(0.0)
        if c.get("type", 0) == 0:
            if I2.v == 0:
                ccase = 1
                J = Bv(0.0) if I1.v == 0 else 0.01 * (c.get("amps_re", 0.0) - I3) / I1
            else:
                dV = -0.01 * (c.get("amps_re", 0.0) - I3) / I2
        else:
            dV = Bv(c.get("dvolts_re", 0.0))
        P.circ.append((ccase, J, dV))
        # static2d.cpp:482-507 / staticaxi.cpp:322-337
        if ccase == 1:
            P.t = put(P.t, m, J)
        elif P.axi:
            P.t = put(P.t, m, -100.0 * dV * P.Cduct / R)
        else:
            P.t = put(P.t, m, (-dV) * P.Cduct)
    # point currents (static2d.cpp:818-825, staticaxi.cpp:644-650)
    P.pt = np.zeros(P.N, LD)
    marker = kw.get("marker")
    if marker is not None:
        for i in np.nonzero(np.asarray(marker) >= 0)[0]:
            J = kw["points"][marker[i]].get("J_re", 0.0)
            if J != 0.0:
                P.pt[i] = LD(0.01) * J * 2.0 * P.x[i] if P.axi else LD(0.01 * J)
    P.fixed = fixed_nodes(kw)
    P.pbc = np.zeros(0, int) if kw.get("pbc") is None else np.asarray(kw["pbc"])[:, :2].reshape(-1)
    return P


def area(X, Y):
    p0, p1 = Y[:, 1] - Y[:, 2], Y[:, 2] - Y[:, 0]
    q0, q1 = X[:, 2] - X[:, 1], X[:, 0] - X[:, 2]
    return (p0 * q1 - p1 * q0).exact(0.5)


# ---- GetBHProps ------------------------------------------------------------------

def bh_props(block, B):
    """v = H / B and dv = d(v) / d(B^2) of the block's curve at B (cubic
    Hermite between knots, the last slope beyond them), with the branch:
    -1 for B == 0, the knot interval, len(B) - 1 beyond the last knot."""
    Bd, Hd, sl = (np.asarray(block[k], float) for k in ("B", "H", "slope"))
    n = len(Bd)
    b = B.abs()
    zero, past = b.v == 0, b.v > Bd[n - 1]
    i = np.clip(np.searchsorted(Bd[1:], np.asarray(b.v, float), side="left"), 0, n - 2)
    if not (np.diff(Bd) >= 0).all():    # the reference's scan on an unsorted table
        i = np.array([next((k for k in range(n - 1) if Bd[k] <= bb <= Bd[k + 1]), 0) for bb in b.v])
    assert (zero | past | (b.v >= Bd[i])).all(), "B below the first knot: GetBHProps returns nothing"
    with np.errstate(all="ignore"):
        # beyond the last knot (CMaterialProp.cpp:1012-1019)
        h_p = Hd[n - 1] + sl[n - 1] * (b - Bd[n - 1])
        dh_p = Bv(np.full(b.v.shape, sl[n - 1]))
        # between knots (CMaterialProp.cpp:1021-1054)
        l = Bv(Bd[i + 1]) - Bd[i]
        z = (b - Bd[i]) / l
        z2 = z * z
        h_i = total([(1.0 - 3.0 * z2 + 2.0 * z2 * z) * Hd[i], z * (1.0 - 2.0 * z + z2) * l * sl[i],
                     z2 * (3.0 - 2.0 * z) * Hd[i + 1], z2 * (z - 1.0) * l * sl[i + 1]])
        dh_i = total([6.0 * z * (z - 1.0) * Hd[i] / l, (1.0 - 4.0 * z + 3.0 * z * z) * sl[i],
                      6.0 * z * (1.0 - z) * Hd[i + 1] / l, z * (3.0 * z - 2.0) * sl[i + 1]])
        h, dh = where(past, h_p, h_i), where(past, dh_p, dh_i)
        v = h / b
        dv = (dh / (b * b) - h / (b * b * b)).exact(0.5)
    v = where(zero, Bv(np.full(b.v.shape, sl[0])), v)
    dv = where(zero, Bv(np.zeros(b.v.shape)), dv)
    branch = np.where(zero, -1, np.where(past, n - 1, i))
    return v, dv, branch


# ---- geometry --------------------------------------------------------------------

def planar_geometry(X, Y):
    p = [Y[:, 1] - Y[:, 2], Y[:, 2] - Y[:, 0], Y[:, 0] - Y[:, 1]]
    q = [X[:, 2] - X[:, 1], X[:, 0] - X[:, 2], X[:, 1] - X[:, 0]]
    a = (p[0] * q[1] - p[1] * q[0]).exact(0.5)
    K = -1.0 / a.exact(4.0)
    Mx = [[K * p[j] * p[k] for k in range(3)] for j in range(3)]
    My = [[K * q[j] * q[k] for k in range(3)] for j in range(3)]
    return p, q, a, Mx, My


def axi_geometry(X, Y):
    """staticaxi.cpp:215-276: Mr, Mz with the logarithmic mean radius, the
    diagonal kept on axis nodes; -> Mx, My, a, R, vol."""
    p = [Y[:, 1] - Y[:, 2], Y[:, 2] - Y[:, 0], Y[:, 0] - Y[:, 1]]
    q = [X[:, 2] - X[:, 1], X[:, 0] - X[:, 2], X[:, 1] - X[:, 0]]
    g = [(X[:, 2] + X[:, 1]).exact(0.5), (X[:, 0] + X[:, 2]).exact(0.5), (X[:, 1] + X[:, 0]).exact(0.5)]
    rn = [X[:, 0], X[:, 1], X[:, 2]]
    a = (p[0] * q[1] - p[1] * q[0]).exact(0.5)
    R = total(rn) / 3.0
    a_hat = total([rn[j] * rn[j] * p[j] / R.exact(4.0) for j in range(3)])
    vol = R.exact(2.0) * a_hat
    on = [r.v < 1.0e-06 for r in rn]
    flag = sum(o.astype(int) for o in on)
    with np.errstate(all="ignore"):
        lg = [r.log() for r in rn]
        # no node on the axis
        gen = -(q[0] * q[1] * q[2]) / total([q[j] * rn[j] * lg[j] for j in range(3)]).exact(2.0)
        for j in (2, 1, 0):    # an edge along z: q[j] == 0 (the first such j wins)
            k, m = (j + 1) % 3, (j + 2) % 3      # q[j] = rn[m] - rn[k]; q[k] = rn[j] - rn[m]
            alt = (q[k] * q[k]) / (-q[k] + rn[j] * (rn[j] / rn[m]).log()).exact(2.0)
            gen = where(np.abs(q[j].v) < 1.0e-06, alt, gen)
        # one node on the axis: from the other two
        one = gen
        for j in (0, 1, 2):
            k, m = (j + 1) % 3, (j + 2) % 3
            alt = where(np.abs((rn[k] - rn[m]).v) < 1.0e-06, rn[m].exact(0.5),
                        (rn[k] - rn[m]) / (lg[k].exact(2.0) - lg[m].exact(2.0)))
            one = where(on[j], alt, one)
        R_hat = where(flag == 2, R, where(flag == 1, one, gen))
    K = -1.0 / (a_hat.exact(2.0) * R)
    Mx = [[K * p[j] * rn[j] * p[k] * rn[k] for k in range(3)] for j in range(3)]
    for j in range(3):      # (in turn: a second axis node sees the first one's new diagonal)
        Mx[j][j] = where(on[j], Mx[j][j] + total([Mx[0][0], Mx[1][1], Mx[2][2]]), Mx[j][j])
    K = -1.0 / (a_hat.exact(2.0) * R_hat)
    My = [[K * (q[j] * rn[j]) * (q[k] * rn[k]) * (g[j] / R) * (g[k] / R) for k in range(3)] for j in range(3)]
    return p, q, a, Mx, My, R, vol


# ---- one pass --------------------------------------------------------------------

def initial_state(P, X, Y, R):
    """Iter == 0: the blocks' linear permeabilities (static2d.cpp:603-631,
    staticaxi.cpp:428-452), the exterior warp (staticaxi.cpp:611-617)."""
    f, mx, my = Bv(P.fill), Bv(P.mu_x), Bv(P.mu_y)
    air = 1.0 - f
    one = Bv(np.ones(P.NE))
    if P.axi:
        m1, m2 = mx * f, my * f
    else:
        m1, m2 = mx * f + air, my * f + air
    m1 = put(m1, P.lam == 1, mx * f + air)
    m2 = put(m2, P.lam == 1, mx / (f + mx * air))
    if P.axi:
        m1 = put(m1, P.lam == 2, my * f + air)
        m2 = put(m2, P.lam == 2, my / (f + my * air))
    else:
        m2 = put(m2, P.lam == 2, my * f + air)
        m1 = put(m1, P.lam == 2, my / (f + my * air))
    m1, m2 = put(m1, P.lam > 2, one), put(m2, P.lam > 2, one)
    if P.axi and P.external.any():
        Z = total([Y[:, 0], Y[:, 1], Y[:, 2]]) / 3.0 - P.ext_zo
        kludge = (R * R + Z * Z) * P.ext_ri / (P.ext_ro * P.ext_ro * P.ext_ro)
        m1, m2 = put(m1, P.external, m1 / kludge), put(m2, P.external, m2 / kludge)
    return m1, m2


def matvec(M, V):
    return [total([M[j][w] * V[w] for w in range(3)]) for j in range(3)]


def newton_pass(P, V=None, state=None, first=False, newton_terms=True):
    """One assembly pass at the iterate V (the solver's unit; ignored by the
    first pass, which assembles from the blocks' linear permeabilities).
    state: (mu1, mu2) of the pass before, as returned.  newton_terms=False
    leaves Mn out (the secant matrix: K V = b is then the fixed-point form).
    -> dict(K, Kb, b, bb: dense values and bounds before the Dirichlet /
    periodic treatment; mu1, mu2: the new state (Bv); B, dv (Bv), branch, kind
    per element: 'linear' (no table, or lamination type > 2), 'off' (a table,
    type 0, mu1 != mu2: Newton off, state kept), 'on'; Mn, V: per element)."""
    NE = P.NE
    X, Y = Bv(P.x[P.p]), Bv(P.y[P.p])
    if P.axi:
        p, q, a, Mx, My, R, vol = axi_geometry(X, Y)
    else:
        p, q, a, Mx, My = planar_geometry(X, Y)
        R, vol = None, a
    zero = Bv(np.zeros(NE))
    Me = [[zero for _ in range(3)] for _ in range(3)]
    be = [zero, zero, zero]
    Vn = [Bv(np.zeros(NE) if first else np.asarray(V, float)[P.p[:, j]]) for j in range(3)]

    # mixed boundary conditions (static2d.cpp:459-480, staticaxi.cpp:298-320)
    if P.mixed.any():
        for j in range(3):
            k = (j + 1) % 3
            dx, dy = X[:, k] - X[:, j], Y[:, k] - Y[:, j]
            sx, sy = dx * dx, dy * dy
            if P.axi:    # pow(., 2.), one ulp each; the planar element squares by a product
                sx.e, sy.e = sx.e + U * np.abs(sx.v), sy.e + U * np.abs(sy.v)
            lj = (sx + sy).sqrt()
            m = P.mixed[:, j]
            if P.axi:
                r = (X[:, j] + X[:, k]).exact(0.5)
                Kb = Bv(-0.0001) * KC * 2.0 * r * P.c0[:, j] * lj / 6.0
                Kc = (Bv(P.c1[:, j]) * lj).exact(0.5) * 0.0001 * 2.0 * r
            else:
                Kb = Bv(-0.0001) * KC * P.c0[:, j] * lj / 6.0
                Kc = (Bv(P.c1[:, j]) * lj).exact(0.5) * 0.0001
            Kb, Kc = where(m, Kb, zero), where(m, Kc, zero)
            Me[j][j] = Me[j][j] + Kb.exact(2.0)
            Me[k][k] = Me[k][k] + Kb.exact(2.0)
            Me[j][k] = Me[j][k] + Kb
            Me[k][j] = Me[k][j] + Kb
            be[j], be[k] = be[j] + Kc, be[k] + Kc

    # source current density (static2d.cpp:482-507, staticaxi.cpp:322-337)
    Jt = P.J_re + P.t
    Ks = (-2.0 * R * Jt * a / 3.0) if P.axi else (-Jt * a / 3.0)
    be = [be[j] + Ks for j in range(3)]

    # magnetisation (static2d.cpp:584-598, staticaxi.cpp:396-407)
    if (P.H_c != 0).any():
        for j in range(3):
            k = (j + 1) % 3
            dirn = P.cos_m * (X[:, k] - X[:, j]) + P.sin_m * (Y[:, k] - Y[:, j])
            if P.axi:
                Km = Bv(-0.0001) * (X[:, j] + X[:, k]).exact(0.5) * P.H_c * dirn
            else:
                Km = (Bv(0.0001) * P.H_c * dirn).exact(0.5)
            Km = where(P.H_c != 0, Km, zero)
            be[j], be[k] = be[j] + Km, be[k] + Km

    # permeability (static2d.cpp:600-797, staticaxi.cpp:409-632)
    Mn = [[zero for _ in range(3)] for _ in range(3)]
    B, dv = zero, zero
    branch = np.full(NE, -2)
    kind = np.where((P.bhn > 0) & (P.lam <= 2), "on", "linear").astype(object)
    if first:
        m1, m2 = initial_state(P, X, Y, R)
    else:
        m1, m2 = state
        kind[(kind == "on") & (P.lam == 0) & (m1.v != m2.v)] = "off"
        on = kind == "on"
        f = Bv(P.fill)
        l0, l1, l2 = P.lam == 0, P.lam == 1, P.lam == 2
        if on.any():
            with np.errstate(all="ignore"):
                if P.axi:     # B from the element's energy (staticaxi.cpp:511-520)
                    ff = f * f
                    sx, sy = where(l2, 1.0 / ff, 1.0), where(l1, 1.0 / ff, 1.0)
                    Ms = [[Mx[j][w] * sx + My[j][w] * sy for w in range(3)] for j in range(3)]
                    v = matvec(Ms, Vn)
                    en = total([Vn[j] * v[j] for j in range(3)]) * (Bv(10000.0) * KC * KC / vol)
                    B = en.abs().sqrt()
                else:         # B from the gradient of A (static2d.cpp:691-696)
                    B1 = total([where(l2, (Vn[j] * q[j]) / f, Vn[j] * q[j]) for j in range(3)])
                    B2 = total([where(l1, Vn[j] * p[j] / f, Vn[j] * p[j]) for j in range(3)])
                    B = KC * (B1 * B1 + B2 * B2).sqrt() / (0.02 * a)
                B = where(on, B, zero)
                mu, dv = Bv(np.zeros(NE)), Bv(np.zeros(NE))
                for k, blk in enumerate(P.blocks):
                    m = on & (P.blk == k)
                    if m.any():
                        vk, dvk, brk = bh_props(blk, B[m])
                        muk = 1.0 / (MUO * vk)
                        for dst, src in ((mu, muk), (dv, dvk)):
                            dst.v[m], dst.e[m] = src.v, src.e
                        branch[m] = brk
                lam_par, lam_ser = mu * f, mu / (f + mu * (1.0 - f))
                m1 = put(put(put(m1, on & l0, mu), on & l1, lam_par), on & l2, lam_ser)
                m2 = put(put(put(m2, on & l0, mu), on & l1, lam_ser), on & l2, lam_par)
                if newton_terms:
                    # type 0: Kn v v'; laminated: Kn / 2 (v u' + u v')
                    Mv = [[where(l0, Mx[j][w] + My[j][w],
                                 where(l1, My[j][w] / f + Mx[j][w], Mx[j][w] / f + My[j][w])) for w in range(3)]
                          for j in range(3)]
                    Mu = [[where(l1, My[j][w] / f + f * Mx[j][w], Mx[j][w] / f + f * My[j][w]) for w in range(3)]
                          for j in range(3)]
                    v, u = matvec(Mv, Vn), matvec(Mu, Vn)
                    K0 = Bv(-200.0) * KC * KC * KC * dv / vol
                    K1 = Bv(-100.0) * KC * KC * KC * dv / vol
                    for j in range(3):
                        for w in range(3):
                            t = where(l0, K0 * v[j] * v[w], K1 * (v[j] * u[w] + v[w] * u[j]))
                            Mn[j][w] = where(on, t, zero)

    # the element matrix (static2d.cpp:799-805), the device's two reciprocals
    im1, im2 = 1.0 / m1, 1.0 / m2
    for j in range(3):
        for k in range(3):
            Me[j][k] = Me[j][k] + (Mx[j][k] * im2 + My[j][k] * im1 + Mn[j][k])
            be[j] = be[j] + Mn[j][k] * Vn[k]

    # the rows: every entry the sum of its incident elements' terms
    N = P.N
    K, Ka, Ke, cnt = (np.zeros((N, N), LD) for _ in range(4))
    b, ba, bE, bc = (np.zeros(N, LD) for _ in range(4))
    for j in range(3):
        nj = P.p[:, j]
        np.add.at(b, nj, -be[j].v)
        np.add.at(ba, nj, np.abs(be[j].v))
        np.add.at(bE, nj, be[j].e)
        np.add.at(bc, nj, 1)
        for k in range(3):
            # (the upper triangle's value on both sides, as AddTo stores it)
            t = Me[min(j, k)][max(j, k)]
            np.add.at(K, (nj, P.p[:, k]), -t.v)
            np.add.at(Ka, (nj, P.p[:, k]), np.abs(t.v))
            np.add.at(Ke, (nj, P.p[:, k]), t.e)
            np.add.at(cnt, (nj, P.p[:, k]), 1)
    Kb = Ke + np.maximum(cnt - 1, 0) * U * Ka
    bb = bE + np.maximum(bc - 1, 0) * U * ba + np.where(P.pt != 0, U * np.abs(b + P.pt), 0)
    return dict(K=K, Kb=Kb, b=b + P.pt, bb=bb, mu1=m1, mu2=m2, B=B, dv=dv, branch=branch, kind=kind,
                Mn=Mn, Vn=Vn, be=be, incident=bc)


def chain(P, Vs, newton_terms=True):
    """The first pass, then one pass per iterate: the list of their results."""
    out = [newton_pass(P, first=True)]
    for V in Vs:
        out.append(newton_pass(P, V, (out[-1]["mu1"], out[-1]["mu2"]), newton_terms=newton_terms))
    return out


def free_nodes(P):
    """Rows neither fixed nor periodic: the Dirichlet and periodic steps
    leave their free-free entries and (fixed values all 0) their b alone."""
    m = np.ones(P.N, bool)
    m[list(P.fixed)] = False
    m[P.pbc] = False
    return m
