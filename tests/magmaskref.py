"""Weighted stress tensor test helpers for magnetostatic problems (CPU): a
literal numpy restatement of what the reference's fpproc does for block
integrals 18-23 at Frequency 0.

    MakeMask            makemask.cpp:48-379 (WeightingScheme 0, the non-SIMPLE
                        branch), its Laplace system solved directly
    IsKosher            makemask.cpp:383-414
    FindBoundaryEdges   fpproc.cpp:5356-5415
    HenrotteVector      fpproc.cpp:3614-3640
    BlockIntegral       fpproc.cpp:3966-4079, cases 18-23

Built on magpostref.MagPost (coordinates in the problem's length units, the
element B).  B1 and B2 are real at Frequency 0, so the reference's complex
products are the real ones written here, operation by operation.

As the device does: the system is returned with the sign turned (the
reference stores the negative definite matrix; the solution is the same), and
a node carries a point property when its marker is >= 0 (the reference matches
the geometry's points to the mesh nodes by their coordinates).
"""
from __future__ import annotations

import math

import numpy as np

import magpostref as M
from magpostref import MUO, PI

INVALID = "The selected region is invalid. A valid selection\ncannot abut a region which is not free space."
TYPES = (18, 19, 20, 21, 22, 23)


class InvalidSelection(Exception):
    pass


def block_is_not_air(b: dict) -> bool:
    """matflag, makemask.cpp:111-125 (a block dictionary as kernels takes it)"""
    k = 0
    if b.get("mu_x", 1.0) != 1 or b.get("mu_y", 1.0) != 1:
        k = 1
    if len(b.get("B", ())) != 0:
        k = 1
    if b.get("LamType", 0) != 0:
        k = 1
    if b.get("H_c", 0.0) != 0:
        k = 1
    if b.get("J_re", 0.0) != 0:
        k = 1
    if b.get("Cduct", 0.0) != 0:
        k = 1
    return bool(k)


class MagMask:
    """MakeMask on the opened solution R (magpostref.MagPost) for the selected
    labels; max_area per label (None: all 0); block_not_air per block (None:
    no hysteresis angle anywhere)."""

    def __init__(self, R: M.MagPost, selected_labels, max_area=None, block_not_air=None):
        self.R = R
        self.N, self.NE = len(R.X), len(R.p)
        self.p = [[int(v) for v in row] for row in R.p]
        self.lbl = [int(v) for v in R.lbl]
        self.X, self.Y = [float(v) for v in R.X], [float(v) for v in R.Y]
        self.lsel = [False] * len(R.labels)
        for l in selected_labels:
            self.lsel[int(l)] = True
        self.max_area = [0.] * len(R.labels) if max_area is None else [float(v) for v in max_area]
        na = [0] * len(R.kw["blocks"]) if block_not_air is None else [int(v) for v in block_not_air]
        marker = R.kw.get("marker")
        self.marker = [-1] * self.N if marker is None else [int(v) for v in marker]
        self.con = [[] for _ in range(self.N)]
        for e in range(self.NE):
            for j in range(3):
                self.con[self.p[e][j]].append(e)
        matflag = [1 if (block_is_not_air(b) or na[k]) else 0 for k, b in enumerate(R.kw["blocks"])]
        self.lblflag = []
        for lb in R.labels:
            f = matflag[lb["block"]]
            if lb.get("in_circuit", -1) >= 0:
                f = 1
            self.lblflag.append(f)
        self.edge = self.find_boundary_edges()
        self.on_axis = self.selection_on_axis()
        self.LV = self.fixed_values()
        self.A, self.b = self.system()
        self.W = np.linalg.solve(self.A, self.b)
        self.msk = np.where(self.W > 0.5, 1., 0.)

    def find_boundary_edges(self):
        nb = [[0, 0, 0] for _ in range(self.NE)]
        for i in range(self.NE):
            for j in range(3):
                org, dest = self.p[i][(j + 1) % 3], self.p[i][(j + 2) % 3]
                done = False
                for ei in self.con[org]:
                    if ei == i:
                        continue
                    if dest in self.p[ei]:
                        done = True
                        break
                if not done:
                    nb[i][j] = 1
        return nb

    def is_kosher(self, k):
        if not self.R.axi or self.X[k] > 1.e-6:
            return True
        score = 0
        for e in self.con[k]:
            for j in range(3):
                n = self.p[e][j]
                if n != k and self.X[n] < 1.e-6:
                    score += 1
                    if score > 1:
                        return False
        return True

    def selection_on_axis(self):
        if not self.R.axi:
            return False
        for i in range(self.NE):
            if self.lsel[self.lbl[i]]:
                for j in range(3):
                    if self.X[self.p[i][j]] < 1.e-6:
                        return True
        return False

    def fixed_values(self):
        LV = [-1.] * self.N
        for i in range(self.NE):
            for j in range(3):
                if self.edge[i][j] == 1:
                    for k in (self.p[i][(j + 1) % 3], self.p[i][(j + 2) % 3]):
                        if (not self.on_axis) or self.is_kosher(k):
                            LV[k] = 0.
        for i in range(self.NE):
            if self.lsel[self.lbl[i]]:
                for j in range(3):
                    LV[self.p[i][j]] = 1.
            elif self.lblflag[self.lbl[i]] != 0:
                for j in range(3):
                    LV[self.p[i][j]] = 0.
        for i in range(self.N):
            if self.marker[i] >= 0 and LV[i] < 0:
                LV[i] = 0.
        return LV

    def system(self):
        LV, X, Y = self.LV, self.X, self.Y
        A = np.zeros((self.N, self.N))
        b = np.zeros(self.N)
        for i in range(self.NE):
            n = self.p[i]
            p = [Y[n[1]] - Y[n[2]], Y[n[2]] - Y[n[0]], Y[n[0]] - Y[n[1]]]
            q = [X[n[2]] - X[n[1]], X[n[0]] - X[n[2]], X[n[1]] - X[n[0]]]
            a = (p[0] * q[1] - p[1] * q[0]) / 2.
            if (not self.lsel[self.lbl[i]]) and self.lblflag[self.lbl[i]]:
                k = 0
                for j in range(3):
                    if LV[n[j]] == 0:
                        k += 1
                if k < 3:
                    raise InvalidSelection(INVALID)
            v = self.max_area[self.lbl[i]]
            v = math.sqrt(a) if v <= 0 else math.sqrt(v)
            Me = [[0. + v * (p[j] * p[k] + q[j] * q[k]) / a for k in range(3)] for j in range(3)]
            be = [0., 0., 0.]
            for j in range(3):
                if LV[n[j]] >= 0:
                    for k in range(3):
                        if j != k:
                            be[k] -= Me[k][j] * LV[n[j]]
                            Me[k][j] = 0.
                            Me[j][k] = 0.
                    be[j] = LV[n[j]] * Me[j][j]
            # L.Put(L.Get - Me), L.b -= be on symmetric storage; kept with the sign turned
            for j in range(3):
                for k in range(j, 3):
                    if Me[j][k] != 0:
                        A[n[j], n[k]] += Me[j][k]
                        if j != k:
                            A[n[k], n[j]] += Me[j][k]
                b[n[j]] += be[j]
        return A, b

    def henrotte(self, k, msk):
        n, X, Y, lc = self.p[k], self.X, self.Y, self.R.lc
        b = [Y[n[1]] - Y[n[2]], Y[n[2]] - Y[n[0]], Y[n[0]] - Y[n[1]]]
        c = [X[n[2]] - X[n[1]], X[n[0]] - X[n[2]], X[n[1]] - X[n[0]]]
        da = (b[0] * c[1] - b[1] * c[0])
        vr = vi = 0.
        for i in range(3):
            vr -= (float(msk[n[i]]) * b[i]) / (da * lc)
            vi -= (float(msk[n[i]]) * c[i]) / (da * lc)
        return vr, vi

    def stress_terms(self, msk=None):
        """Per element the six terms cases 18-23 add to z: (NE, 6)."""
        R = self.R
        lc, axi = R.lc, R.axi
        msk = self.msk if msk is None else msk
        rows = []
        for i in range(self.NE):
            Xc, Yc, An = R.corners(i)
            b0, b1 = Yc[1] - Yc[2], Yc[2] - Yc[0]
            c0, c1 = Xc[2] - Xc[1], Xc[0] - Xc[2]
            a = ((b0 * c1 - b1 * c0) / 2.) * math.pow(lc, 2.)
            if axi:
                r = [Xc[k] * lc for k in range(3)]
                Rm = (r[0] + r[1] + r[2]) / 3.
                a *= (2. * PI * Rm)
            else:
                a *= R.depth
            B1, B2 = M.element_b(axi, lc, Xc, Yc, An)
            cr, ci = self.henrotte(i, msk)
            ae = 1.
            if axi and R.labels[self.lbl[i]].get("is_external", 0):
                cx = cy = 0.
                for j in range(3):
                    cx += Xc[j] / 3.
                    cy += Yc[j] / 3.
                ro, ri, zo = R.ext
                q = M.cabs(cx, cy - zo)
                ae = (q * q * ri) / (ro * ro * ro)
            F1 = (((B1 * B1) - (B2 * B2)) * cr + 2. * (B1 * B2) * ci) / (2. * MUO)
            F2 = (((B2 * B2) - (B1 * B1)) * ci + 2. * (B1 * B2) * cr) / (2. * MUO)
            G1 = (((B1 * B1) - (B2 * B2)) * cr + 2. * B1 * B2 * ci) / (4. * MUO)
            G2 = (((B2 * B2) - (B1 * B1)) * ci + 2. * B1 * B2 * cr) / (4. * MUO)
            t = [0.] * 6
            y = F2
            y *= ae
            t[1] = a * y
            t[3] = a * G2 * ae
            if not axi:
                y = F1
                y *= ae
                t[0] = a * y
                t[2] = a * G1 * ae
                tr = ti = 0.
                for k in range(3):
                    tr += Xc[k] * lc / 3.
                    ti += Yc[k] * lc / 3.
                y = tr * F2 - ti * F1
                y *= ae
                t[4] = a * y
                t[5] = a * (tr * G2 - ti * G1) * ae
            rows.append(t)
        return np.array(rows, float).reshape(-1, 6)

    def integrals(self, msk=None):
        """(z, scale): types 18-23 as running sums in element order, and the
        sums of the absolute terms (the scale of a rounding bound)."""
        t = self.stress_terms(msk)
        s = [0.] * 6
        for row in t:
            for c in range(6):
                s[c] += row[c]
        return np.array(s), np.abs(t).sum(axis=0)


# --- meshes and problems ---------------------------------------------------------

def graded(n, a, b, ratio=1.35):
    """n + 1 lines from a to b, each gap `ratio` times the one before"""
    g = ratio ** np.arange(n)
    return a + (b - a) * np.concatenate([[0.], np.cumsum(g) / g.sum()])


def crisscross(xs, ys):
    """Every cell of the grid cut into four triangles round a centre node: the
    mesh maps onto itself under a reflection about any of its grid lines.
    Returns x, y, p (counter-clockwise) and the cell column of each element."""
    xs, ys = np.asarray(xs, float), np.asarray(ys, float)
    nx, ny = len(xs), len(ys)
    x = list(np.tile(xs, ny))
    y = list(np.repeat(ys, nx))
    p, col, row = [], [], []
    for j in range(ny - 1):
        for i in range(nx - 1):
            n00, n10 = j * nx + i, j * nx + i + 1
            n01, n11 = n00 + nx, n10 + nx
            c = len(x)
            x.append((xs[i] + xs[i + 1]) / 2.)
            y.append((ys[j] + ys[j + 1]) / 2.)
            p += [[n00, n10, c], [n10, n11, c], [n11, n01, c], [n01, n00, c]]
            col += [i] * 4
            row += [j] * 4
    return np.array(x), np.array(y), np.array(p, np.int32), np.array(col), np.array(row)


def grid(xs, ys):
    """Two triangles per cell (one diagonal direction); cell column and row per element."""
    xs, ys = np.asarray(xs, float), np.asarray(ys, float)
    nx, ny = len(xs), len(ys)
    p, col, row = [], [], []
    for j in range(ny - 1):
        for i in range(nx - 1):
            n00, n10 = j * nx + i, j * nx + i + 1
            n01, n11 = n00 + nx, n10 + nx
            p += [[n00, n10, n11], [n00, n11, n01]]
            col += [i, i]
            row += [j, j]
    return np.tile(xs, ny), np.repeat(ys, nx), np.array(p, np.int32), np.array(col), np.array(row)


def tag_edges(x, y, p, rules):
    """e (NE, 3): the line property of the edge from p[j] to p[j + 1] by the first rule that holds, else -1"""
    e = -np.ones((len(p), 3), np.int32)
    for i in range(len(p)):
        for j in range(3):
            a, b = p[i][j], p[i][(j + 1) % 3]
            for f, k in rules:
                if f(x[a], y[a], x[b], y[b]):
                    e[i, j] = k
                    break
    return e


def solve_planar(kw):
    """The first-order discretisation of a linear planar problem without
    circuits (static2d.cpp: K = (b b + c c) / (4 a mu mu0), f = J a / 3, the
    ends of BdryFormat 0 edges fixed at A0), assembled in SI units and solved
    directly, then refined against a long-double residual: A in Wb/m."""
    lc = M.LENGTH_CONV[kw.get("length_units", 0)]
    X, Y = M.user_xy(kw)
    X, Y = X * lc, Y * lc
    p = np.asarray(kw["p"], np.int64)
    N = len(X)
    K = np.zeros((N, N), np.longdouble)
    f = np.zeros(N, np.longdouble)
    for i in range(len(p)):
        n = p[i]
        blk = kw["blocks"][kw["labels"][int(kw["lbl"][i])]["block"]]
        assert len(blk.get("B", ())) == 0 and blk.get("H_c", 0.0) == 0
        b = np.array([Y[n[1]] - Y[n[2]], Y[n[2]] - Y[n[0]], Y[n[0]] - Y[n[1]]], np.longdouble)
        c = np.array([X[n[2]] - X[n[1]], X[n[0]] - X[n[2]], X[n[1]] - X[n[0]]], np.longdouble)
        a = (b[0] * c[1] - b[1] * c[0]) / 2
        mu = np.longdouble(MUO)
        K[np.ix_(n, n)] += (np.outer(b, b) / blk.get("mu_y", 1.0) + np.outer(c, c) / blk.get("mu_x", 1.0)) / (4 * a * mu)
        f[n] += np.longdouble(blk.get("J_re", 0.0)) * 1e6 * a / 3
    fixed = {}
    e = np.asarray(kw["e"])
    for i in range(len(p)):
        for j in range(3):
            if e[i, j] >= 0 and kw["lines"][e[i, j]].get("format", 0) == 0:
                for v in (p[i][j], p[i][(j + 1) % 3]):
                    fixed[int(v)] = kw["lines"][e[i, j]].get("A0", 0.0)
    fn = np.array(sorted(fixed))
    fv = np.array([fixed[k] for k in fn], np.longdouble)
    free = np.setdiff1d(np.arange(N), fn)
    A = np.zeros(N, np.longdouble)
    A[fn] = fv
    Kff = K[np.ix_(free, free)]
    rhs = f[free] - K[np.ix_(free, fn)] @ fv
    Kd = Kff.astype(float)
    u = np.linalg.solve(Kd, rhs.astype(float)).astype(np.longdouble)
    for _ in range(3):
        u = u + np.linalg.solve(Kd, (rhs - Kff @ u).astype(float))
    A[free] = u
    return A.astype(float)


def layered_strip(length_units=1, nair=3, nslab=4, ny=4, J=2.0, A_left=0.0, A_right=3e-3, depth=25.0,
                  wa=6.0, ws=8.0, h=10.0):
    """Air, a slab with uniform J (label 1, the selection), air, side by side in
    x; A fixed on the two x ends, natural on top and bottom.  The crisscross
    mesh with uniform rows, uniform slab columns and air columns graded away
    from the slab maps onto itself under the reflections about its rows, so the
    discrete A does not depend on y, is linear in x in both air layers and B is
    uniform there.  y = 0 is the slab's centre line.  Sizes in the problem's
    length units.  Returns kw and A (solve_planar)."""
    u = M.UNIT_CM[length_units]
    left = -(ws / 2. + wa) + (graded(nair, 0., wa, 1. / 1.35))
    right = ws / 2. + graded(nair, 0., wa, 1.35)
    xs = np.concatenate([left, np.linspace(-ws / 2., ws / 2., nslab + 1)[1:-1], right])
    ys = np.linspace(-h / 2., h / 2., ny + 1)
    x, y, p, col, _ = crisscross(xs, ys)
    lbl = np.where((col >= nair) & (col < nair + nslab), 1, 0).astype(np.int32)
    x0, x1 = xs[0], xs[-1]
    e = tag_edges(x, y, p, [(lambda xa, ya, xb, yb: xa == x0 and xb == x0, 0),
                            (lambda xa, ya, xb, yb: xa == x1 and xb == x1, 1)])
    kw = dict(x=x * u, y=y * u, p=p, lbl=lbl, e=e, marker=None, pbc=None,
              blocks=[dict(mu_x=1.0, mu_y=1.0), dict(mu_x=1.0, mu_y=1.0, J_re=J)],
              labels=[dict(block=0), dict(block=1)],
              lines=[dict(format=0, A0=A_left), dict(format=0, A0=A_right)], points=[], circuits=[],
              precision=1e-8, length_units=length_units, coords=0, relax=1.0, problem_type=0)
    info = dict(depth=depth, h=h, left_elem=0, right_elem=int(np.flatnonzero(col == len(xs) - 2)[0]), sel=[1])
    return kw, solve_planar(kw), info


def strip_closed_form(R: M.MagPost, info):
    """F_x = depth h (B_L^2 - B_R^2) / (2 mu0) from the uniform B of the two air
    layers (the Maxwell stress -B_y^2 / (2 mu0) on the slab's two faces, outward
    normals -x and +x): the Lorentz force of type 11."""
    BL = M.element_b(False, R.lc, *R.corners(info["left_elem"]))[1]
    BR = M.element_b(False, R.lc, *R.corners(info["right_elem"]))[1]
    return R.depth * (info["h"] * R.lc) * (BL * BL - BR * BR) / (2. * MUO), BL, BR


def rules_problem(axi=False):
    """A grid whose labels take every rule of MakeMask.  Planar: air (0), the
    body (1), a label that is air by its material but sits in a circuit (2), a
    block that only block_not_air marks (3), iron next to the body (4: its
    elements are numbered after the body's, so the nodes they share end at 0 and
    the selection stays valid) and iron whose elements come before its air
    neighbours' (5: selecting the air, label 0, is refused); a point property on
    a free air node, on a body node (already 1) and on a boundary node (already
    0).  Axisymmetric: the body touches r = 0, so the axis's end nodes are
    kosher and its inner ones are not.  A is random (no solve)."""
    rng = np.random.default_rng(7 + axi)
    xs = (0.0 if axi else -4.0) + np.concatenate([[0.], np.cumsum(0.8 + 0.1 * np.arange(9))])
    ys = -3.0 + np.concatenate([[0.], np.cumsum(0.7 + 0.07 * np.arange(8))])
    x, y, p, col, row = grid(xs, ys)
    nx = len(xs)
    lbl = np.zeros(len(p), np.int32)
    b0 = 0 if axi else 3
    body = (col >= b0) & (col < b0 + 2) & (row >= 3) & (row < 5)
    lbl[body] = 1
    lbl[(col == 7) & (row == 1)] = 2
    lbl[(col == 7) & (row == 6)] = 3
    lbl[(col >= b0 + 2) & (col < b0 + 4) & (row >= 3) & (row < 5)] = 4
    lbl[(col == 1) & (row == 0)] = 5 if not axi else 0
    # the iron next to the body last
    order = np.concatenate([np.flatnonzero(lbl != 4), np.flatnonzero(lbl == 4)])
    p, lbl = p[order], lbl[order]
    marker = -np.ones(len(x), np.int32)
    marker[6 * nx + 2 if not axi else 6 * nx + 6] = 0      # free, in the air
    marker[4 * nx + b0 + 1] = 0                            # in the body
    marker[0 * nx + 5] = 0                                 # on the outer boundary
    blocks = [dict(mu_x=1.0, mu_y=1.0), dict(mu_x=1.0, mu_y=1.0, J_re=1.5), dict(mu_x=1.0, mu_y=1.0),
              dict(mu_x=200.0, mu_y=200.0)]
    labels = [dict(block=0), dict(block=1), dict(block=0, in_circuit=0), dict(block=2), dict(block=3),
              dict(block=3)]
    u = M.UNIT_CM[1]
    kw = dict(x=x * u, y=y * u, p=p, lbl=lbl, e=-np.ones((len(p), 3), np.int32), marker=marker, pbc=None,
              blocks=blocks, labels=labels, lines=[], points=[dict(J_re=0.5)], circuits=[dict(type=0, amps_re=0.0)],
              precision=1e-8, length_units=1, coords=0, relax=1.0, problem_type=1 if axi else 0)
    A = rng.uniform(-1, 1, len(x)) * 1e-3
    if axi:
        A = A * x
    extra = dict(sel=[1], max_area=np.array([0.3, -1.0, 0.0, 0.5, 0.2, 0.0]), block_not_air=np.array([0, 0, 1, 0]),
                 invalid_sel=[0])
    return kw, A, extra


def strip_case(ne, axi=False):
    """magpostref.strip_problem's mesh and A with every block air, so that a
    label can be selected: every node ends an exterior edge, the mask is 1 on
    the nodes of the selected elements and 0 elsewhere, by hand."""
    kw, A = M.strip_problem(ne, axi)
    kw["blocks"] = [dict(mu_x=1.0, mu_y=1.0) for _ in range(4)]
    kw["labels"] = [dict(block=k, is_external=lb.get("is_external", 0)) for k, lb in enumerate(kw["labels"])]
    kw["circuits"] = []
    sel = [2] if ne > 2 else [0]
    msk = np.zeros(ne + 2)
    for e in range(ne):
        if kw["lbl"][e] in sel:
            msk[kw["p"][e]] = 1.
    return kw, A, sel, msk


def free_body(n):
    """Two conductors carrying opposite J in air inside a square with A = 0 on
    its boundary, 2 n cells a side; the selection is the first (label 1)."""
    xs = np.linspace(-6., 6., 2 * n + 1)
    x, y, p, col, row = crisscross(xs, xs)
    cx, cy = (xs[col] + xs[col + 1]) / 2., (xs[row] + xs[row + 1]) / 2.
    lbl = np.zeros(len(p), np.int32)
    lbl[(cx > -3.) & (cx < -1.5) & (abs(cy) < 1.5)] = 1
    lbl[(cx > 1.5) & (cx < 3.) & (cy > 0.) & (cy < 3.)] = 2
    lo, hi = xs[0], xs[-1]
    box = lambda xa, ya, xb, yb: ((xa == lo and xb == lo) or (xa == hi and xb == hi) or
                                  (ya == lo and yb == lo) or (ya == hi and yb == hi))
    e = tag_edges(x, y, p, [(box, 0)])
    u = M.UNIT_CM[2]
    kw = dict(x=x * u, y=y * u, p=p, lbl=lbl, e=e, marker=None, pbc=None,
              blocks=[dict(mu_x=1.0, mu_y=1.0), dict(mu_x=1.0, mu_y=1.0, J_re=3.0),
                      dict(mu_x=1.0, mu_y=1.0, J_re=-2.0)],
              labels=[dict(block=0), dict(block=1), dict(block=2)], lines=[dict(format=0, A0=0.0)], points=[],
              circuits=[], precision=1e-8, length_units=2, coords=0, relax=1.0, problem_type=0)
    return kw, solve_planar(kw)
