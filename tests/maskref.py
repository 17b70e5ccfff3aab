"""Weighted stress tensor test helpers (CPU): a literal numpy restatement of
what the reference's post-processor does for block integrals 5 and 6 of an
electrostatic problem -- FindBoundaryEdges (PostProcessor.cpp:1097-1150),
isKosher (400-430), isSelectionOnAxis (479-494, epproc.cpp:471-487), makeMask
(497-725) with its Laplace system solved directly, HenrotteVector (742-768)
and cases 5 and 6 of blockIntegral (epproc.cpp:329-389).

Built on postproc.Post (coordinates in the problem's length units, the
element D, AECF, the node -> element lists) and electro's tables.

Two things differ from the reference on purpose, as the device does:
 - the system is returned with the sign turned (A = -L, b = -L.b): the
   reference stores the negative definite matrix, the solution is the same;
 - the planar case 5 returns (Fx, Fy).  The reference's adds the x term to the
   imaginary part too (epproc.cpp:353-360: FEMM's separate y-force integral
   was lost when its three integrals became two); Fy here is a F2 AECF with F2
   as case 6 writes it."""
from __future__ import annotations

import math
import re

import numpy as np

import electro
import postproc
from postproc import EO, PI

INVALID = "The selected region is invalid. A valid selection cannot abut a region which is not free space."


class InvalidSelection(Exception):
    pass


def read_max_area(path: str) -> np.ndarray:
    """The labels' MaxArea from a .res header (electro.read_res drops the
    column): the file holds a mesh size d, MaxArea = d (PI d / 4), 0 when
    d <= 0 (CBlockLabel.cpp:130-134)."""
    lines = open(path).read().splitlines()
    for i, ln in enumerate(lines):
        m = re.match(r"\[NumBlockLabels\]\s*=\s*(\d+)", ln.strip())
        if m:
            out = []
            for k in range(int(m.group(1))):
                v = float(lines[i + 1 + k].split()[3])
                if v <= 0:
                    v = 0.
                else:
                    v *= PI * v / 4.
                out.append(v)
            return np.array(out)
    raise ValueError("no [NumBlockLabels] in " + path)


def is_air(blk: dict) -> bool:
    """CSMaterialProp::isAir (CMaterialProp.cpp:1603-1609)."""
    return blk.get("ex", 1.0) == 1 and blk.get("ey", 1.0) == 1 and blk.get("qv", 0.0) == 0


class Mask:
    """makeMask on the post-processor state R (postproc.Post, electrostatic)
    for the selected labels and nodes; max_area per label (None: all 0)."""

    def __init__(self, R: postproc.Post, selected_labels, selected_nodes=(), max_area=None):
        assert not R.heat
        self.R = R
        self.lsel = [False] * len(R.labels)
        for l in selected_labels:
            self.lsel[int(l)] = True
        self.nsel = [False] * R.N
        for n in selected_nodes:
            self.nsel[int(n)] = True
        self.max_area = [0.] * len(R.labels) if max_area is None else [float(v) for v in max_area]
        marker = R.kw.get("marker")
        self.marker = [-1] * R.N if marker is None else [int(v) for v in marker]
        self.edge = self.find_boundary_edges()
        self.on_axis = self.is_selection_on_axis()
        self.LV = self.fixed_values()
        self.A, self.b = self.system()
        self.W = np.linalg.solve(self.A, self.b)
        self.msk = np.where(self.W > 0.5, 1., 0.)

    # -- FindBoundaryEdges -------------------------------------------------------
    def find_boundary_edges(self):
        R = self.R
        nb = [[0, 0, 0] for _ in range(R.NE)]
        for i in range(R.NE):
            for j in range(3):
                org, dest = R.p[i][(j + 1) % 3], R.p[i][(j + 2) % 3]
                done = False
                for ei in R.con[org]:
                    if ei == i:
                        continue
                    if dest in R.p[ei]:
                        done = True
                        break
                if not done:
                    nb[i][j] = 1
        return nb

    def is_kosher(self, k):
        R = self.R
        if not R.axi or R.X[k] > 1.e-6:
            return True
        score = 0
        for e in R.con[k]:
            for j in range(3):
                n = R.p[e][j]
                if n != k and R.X[n] < 1.e-6:
                    score += 1
                    if score > 1:
                        return False
        return True

    def is_selection_on_axis(self):
        R = self.R
        if not R.axi:
            return False
        for i in range(R.NE):
            if self.lsel[R.lbl[i]]:
                for j in range(3):
                    if R.X[R.p[i][j]] < 1.e-6:
                        return True
        for i in range(R.N):
            if self.nsel[i] and R.X[i] < 1.e-6:
                return True
        return False

    # -- the fixed values, rule by rule ---------------------------------------------
    def fixed_values(self):
        R = self.R
        lblflag = [0 if is_air(R.blocks[l["block"]]) else 1 for l in R.labels]
        LV = [0. if R.Q[i] != -2 else -1. for i in range(R.N)]
        for i in range(R.NE):
            for j in range(3):
                if self.edge[i][j] == 1:
                    for k in (R.p[i][(j + 1) % 3], R.p[i][(j + 2) % 3]):
                        if (not self.on_axis) or self.is_kosher(k):
                            LV[k] = 0.
        for i in range(R.NE):
            if self.lsel[R.lbl[i]]:
                for j in range(3):
                    LV[R.p[i][j]] = 1.
            elif lblflag[R.lbl[i]] != 0:
                for j in range(3):
                    LV[R.p[i][j]] = 0.
        # (the reference matches the geometry's points that carry a property
        # against the mesh nodes within 1e-8: on the mesher's meshes, the nodes
        # whose marker is a point property)
        for i in range(R.N):
            if self.marker[i] >= 0 and LV[i] < 0:
                LV[i] = 0.
        for i in range(R.N):
            if self.nsel[i]:
                LV[i] = 1.
        self.lblflag = lblflag
        return LV

    # -- the Laplace system ------------------------------------------------------------
    def system(self):
        R, LV = self.R, self.LV
        A = np.zeros((R.N, R.N))
        b = np.zeros(R.N)
        for i in range(R.NE):
            n = R.p[i]
            X, Y = R.X, R.Y
            p = [Y[n[1]] - Y[n[2]], Y[n[2]] - Y[n[0]], Y[n[0]] - Y[n[1]]]
            q = [X[n[2]] - X[n[1]], X[n[0]] - X[n[2]], X[n[1]] - X[n[0]]]
            area = (p[0] * q[1] - p[1] * q[0]) / 2.
            if (not self.lsel[R.lbl[i]]) and self.lblflag[R.lbl[i]]:
                k = 0
                for j in range(3):
                    if LV[n[j]] == 0:
                        k += 1
                if k < 3:
                    raise InvalidSelection(INVALID)
            v = self.max_area[R.lbl[i]]
            v = math.sqrt(area) if v <= 0 else math.sqrt(v)
            Me = [[0. + v * (p[j] * p[k] + q[j] * q[k]) / area for k in range(3)] for j in range(3)]
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

    # -- HenrotteVector and the integrals ----------------------------------------------------
    def henrotte(self, k, msk):
        R = self.R
        n, X, Y = R.p[k], R.X, R.Y
        b = [Y[n[1]] - Y[n[2]], Y[n[2]] - Y[n[0]], Y[n[0]] - Y[n[1]]]
        c = [X[n[2]] - X[n[1]], X[n[0]] - X[n[2]], X[n[1]] - X[n[0]]]
        da = (b[0] * c[1] - b[1] * c[0])
        vr = vi = 0.
        for i in range(3):
            vr -= (msk[n[i]] * b[i]) / (da * R.lc)
            vi -= (msk[n[i]] * c[i]) / (da * R.lc)
        return vr, vi

    def stress_terms(self, msk=None):
        """Per element the three terms the integrals sum: a Fx AECF (planar),
        a Fy AECF (Fz), a (x Fy - y Fx) AECF (planar): (NE, 3)."""
        R = self.R
        msk = self.msk if msk is None else msk
        rows = []
        for i in range(R.NE):
            n, X, Y = R.p[i], R.X, R.Y
            b0, b1 = Y[n[1]] - Y[n[2]], Y[n[2]] - Y[n[0]]
            c0, c1 = X[n[2]] - X[n[1]], X[n[0]] - X[n[2]]
            a = ((b0 * c1 - b1 * c0) / 2.) * (R.lc * R.lc)
            if R.axi:
                r = [X[n[k]] * R.lc for k in range(3)]
                Rm = (r[0] + r[1] + r[2]) / 3.
                a *= (2. * PI * Rm)
            else:
                a *= R.depth
            B1, B2 = R.D[i]
            cr, ci = self.henrotte(i, msk)
            ae = R.aecf(i)
            F1 = (((B1 * B1) - (B2 * B2)) * cr + 2. * (B1 * B2) * ci) / (2. * EO)
            F2 = (((B2 * B2) - (B1 * B1)) * ci + 2. * (B1 * B2) * cr) / (2. * EO)
            t = [0., a * (F2 * ae), 0.]
            if not R.axi:
                t[0] = a * (F1 * ae)
                tr = ti = 0.
                for k in range(3):
                    tr += (X[n[k]] * R.lc) / 3.
                    ti += (Y[n[k]] * R.lc) / 3.
                y = tr * F2 - ti * F1
                y *= ae
                t[2] = a * y
            rows.append(t)
        return np.array(rows, float).reshape(-1, 3)

    def integrals(self, msk=None):
        """((Fx, Fy), torque, the sums of the absolute terms (3)): the running
        sums in element order, as the reference."""
        t = self.stress_terms(msk)
        s = [0., 0., 0.]
        for row in t:
            for c in range(3):
                s[c] += row[c]
        return np.array(s[:2]), s[2], np.abs(t).sum(axis=0)


# --- small structured problems ----------------------------------------------------------

def ygrid(xs, ys):
    """electro.grid's triangulation on the given grid lines."""
    xs, ys = np.asarray(xs, float), np.asarray(ys, float)
    nx, ny = len(xs), len(ys)
    _, _, p = electro.grid(nx, ny, 1.0, 1.0)
    return np.tile(xs, ny), np.repeat(ys, nx), p


def graded(n, a, b, ratio=1.35):
    """n + 1 lines from a to b, each gap `ratio` times the one before: no line
    falls on the middle of a layer."""
    g = ratio ** np.arange(n)
    return a + (b - a) * np.concatenate([[0.], np.cumsum(g) / g.sum()])


def capacitor(nx=7, nair=3, ndiel=4, axi=False, w=3.0, g=1.0, h=2.5, er=4.0, V0=100.0, depth=2.0, x0=None,
              length_units=2):
    """The layered capacitor of the closed forms: [x0, x0 + w] x [0, h] (user
    units: cm), air below y = g, a dielectric er (label 1, the selection)
    above; V = 0 on y = 0 and V0 on y = h through fixed edges; the exact,
    piecewise linear V.  nair (odd) graded layers of cells in the air, so no
    node's W comes near 0.5.  Returns kw, V, the closed forms (E_air in V/m)."""
    x0 = (1.0 if axi else 0.0) if x0 is None else x0
    u = electro.UNITS[length_units]
    lc = postproc.LENGTH_CONV[length_units]
    xs = x0 + w * np.arange(nx) / (nx - 1)
    ys = np.concatenate([graded(nair, 0., g), graded(ndiel, g, h, 1.2)[1:]])
    x, y, p = ygrid(xs, ys)
    cy = y[p].mean(axis=1)
    lbl = np.where(cy < g, 0, 1).astype(np.int32)
    e = electro.tag_edges(x, y, p, [(lambda xa, ya, xb, yb: ya == 0 and yb == 0, 0),
                                    (lambda xa, ya, xb, yb: ya == h and yb == h, 1)])
    kw = dict(x=x * u, y=y * u, p=p, lbl=lbl, e=e, blocks=[dict(ex=1.0, ey=1.0, qv=0.0), dict(ex=er, ey=er, qv=0.0)],
              labels=[dict(block=0), dict(block=1)], lines=[dict(format=0, V=0.0), dict(format=0, V=V0)],
              length_units=length_units, problem_type=1 if axi else 0, depth=depth, precision=1e-8)
    Eair = V0 / ((g + (h - g) / er) * lc)
    V = np.where(y <= g, Eair * lc * y, Eair * lc * g + (Eair / er) * lc * (y - g))
    P0 = 0.5 * EO * Eair * Eair
    if axi:
        ri, ro = x0 * lc, (x0 + w) * lc
        closed = dict(force=np.array([0., -P0 * PI * (ro * ro - ri * ri)]), torque=0.,
                      scale=P0 * PI * (ro * ro - ri * ri))
    else:
        W, D = w * lc, depth * lc
        closed = dict(force=np.array([0., -P0 * W * D]), torque=-P0 * (W * W / 2.) * D, scale=P0 * W * D)
    return kw, V, closed


def free_body(n=12, lo=4, hi=7):
    """A square dielectric body (label 1, cells lo..hi of n in each direction,
    graded lines) in air inside a grounded box, a prescribed-voltage conductor
    node line on one side of the air: the mask is truly two-dimensional."""
    xs = graded(n, 0., 6., 1.06)
    ys = graded(n + 1, 0., 7., 1.04)
    x, y, p = ygrid(xs, ys)
    nx = len(xs)
    ci, cj = [], []
    for j in range(len(ys) - 1):
        for i in range(nx - 1):
            ci += [i, i]
            cj += [j, j]
    ci, cj = np.array(ci), np.array(cj)
    lbl = ((ci >= lo) & (ci < hi) & (cj >= lo) & (cj < hi + 1)).astype(np.int32)
    box = lambda xa, ya, xb, yb: ((xa == xs[0] and xb == xs[0]) or (xa == xs[-1] and xb == xs[-1]) or
                                  (ya == ys[0] and yb == ys[0]) or (ya == ys[-1] and yb == ys[-1]))
    e = electro.tag_edges(x, y, p, [(box, 0)])
    cond = -np.ones(len(x), np.int32)
    cond[[j * nx + 1 for j in range(2, len(ys) - 2)]] = 0
    u = electro.UNITS[1]
    kw = dict(x=x * u, y=y * u, p=p, lbl=lbl, e=e, blocks=[dict(ex=1.0, ey=1.0, qv=0.0), dict(ex=3.0, ey=5.0, qv=0.0)],
              labels=[dict(block=0), dict(block=1)], lines=[dict(format=0, V=0.0)],
              conductors=[dict(type=1, V=50.0, q=0.0)], conductor=cond, length_units=1, depth=3.0, precision=1e-8)
    return kw


def rules_problem():
    """The planar capacitor with what the rules of makeMask look at, all in
    the air: a node with a point charge, two nodes of a prescribed-voltage
    conductor, MaxArea > 0 on the air's label and <= 0 on the dielectric's, and
    a selected node."""
    kw, _, _ = capacitor(nx=8, nair=5, ndiel=3)
    nx = 8
    marker = -np.ones(len(kw["x"]), np.int32)
    marker[2 * nx + 2] = 0
    cond = -np.ones(len(kw["x"]), np.int32)
    cond[[1 * nx + 4, 1 * nx + 5]] = 0
    kw.update(marker=marker, points=[dict(V=0.0, qp=2e-9)], conductor=cond,
              conductors=[dict(type=1, V=30.0, q=0.0)])
    return kw, dict(sel=[1], nsel=[3 * nx + 6], max_area=np.array([0.02, -1.0]))


CASES = ("cap_planar", "cap_axi", "cap_on_axis", "rules", "free_body", "fixture")


def case(name):
    """One mesh of the device tests, built once: kw, V (exact where a closed
    form exists, else the direct solve of the restated problem), the selection,
    the post-processor state R and the restated mask M."""
    if name in case.cache:
        return case.cache[name]
    c = dict(nsel=None, max_area=None, closed=None, sel=[1])
    if name == "cap_planar":
        c["kw"], c["V"], c["closed"] = capacitor(nx=7, nair=3, ndiel=4)
    elif name == "cap_axi":
        c["kw"], c["V"], c["closed"] = capacitor(nx=8, nair=5, ndiel=4, axi=True)
    elif name == "cap_on_axis":
        c["kw"], c["V"], c["closed"] = capacitor(nx=7, nair=3, ndiel=5, axi=True, x0=0.0)
    elif name == "rules":
        c["kw"], extra = rules_problem()
        c.update(extra)
    elif name == "free_body":
        c["kw"] = free_body()
    elif name == "fixture":
        import os
        from test_postproc_cpu import GOLD, load
        R, _, r = load("test")
        c.update(kw=r["kw"], V=r["V"], sel=[0], R=R,
                 max_area=read_max_area(os.path.join(GOLD, "esolver", "test.res.check")))
    else:
        raise KeyError(name)
    if "V" not in c:
        c["V"] = electro.restate(c["kw"])["V"][:len(c["kw"]["x"])]
    if "R" not in c:
        c["R"] = postproc.Post(c["kw"], c["V"], "es")
    c["M"] = Mask(c["R"], c["sel"], c["nsel"] or (), c["max_area"])
    case.cache[name] = c
    return c


case.cache = {}
