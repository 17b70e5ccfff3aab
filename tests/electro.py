"""Electrostatics test helpers (CPU): a reader of the reference's .res files,
a literal numpy restatement of ESolver::AnalyzeProblem
(cfemm/esolver/esolver.cpp:389-646) solved directly, a restatement of
ESolver::ChargeOnConductor (esolver.cpp:797-844) with the coefficient vector
of the charge functional, and small structured meshes.

A problem is the keyword dictionary of kernels.ElectrostaticProblem: the
device and the restatement read the same arrays."""
from __future__ import annotations

import re

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

EO = 8.85418781762e-12                             # femmconstants.h:24
PI = 3.141592653589793238462643383
UNITS = (25.4, 1., 10., 1000., 0.0254, 0.001)      # esolver.cpp:65, user units -> mm
UNIT_NAMES = {"inches": 0, "millimeters": 1, "centimeters": 2, "meters": 3, "mils": 4, "microns": 5,
              "micrometers": 5}


def read_res(path: str) -> dict:
    """A .res file (the echoed .fee header, then [Solution]) -> the problem's
    keyword dictionary plus the recorded V (per node), Q (per node: the
    conductor index, or -1 / -2) and conductor lines (V, q)."""
    lines = open(path).read().splitlines()
    sol = lines.index("[Solution]")
    head = lines[:sol]
    hdr, blocks, conductors, points, bdrys, labels = {}, [], [], [], [], []
    cur = None
    i = 0
    while i < len(head):
        ln = head[i].strip()
        m = re.match(r"\[(\w+)\]\s*=\s*(.*)", ln)
        if m:
            hdr[m.group(1)] = m.group(2).strip().strip('"')
            if m.group(1) == "NumBlockLabels":
                for k in range(int(m.group(2))):
                    f = head[i + 1 + k].split()
                    labels.append(dict(block=int(f[2]) - 1, is_external=int(f[5]) & 1 if len(f) > 5 else 0))
        elif ln.startswith("<Begin"):
            cur = {}
        elif ln.startswith("<End"):
            {"<EndBlock>": blocks, "<EndConductor>": conductors, "<EndPoint>": points,
             "<EndBdry>": bdrys}[ln].append(cur)
            cur = None
        elif cur is not None:
            m = re.match(r"<(\w+)>\s*=\s*(.*)", ln)
            if m:
                cur[m.group(1)] = m.group(2).strip()
        i += 1
    n = int(lines[sol + 1])
    nod = np.array([l.split() for l in lines[sol + 2:sol + 2 + n]], dtype=float)
    ne = int(lines[sol + 2 + n])
    el = np.array([l.split() for l in lines[sol + 3 + n:sol + 3 + n + ne]], dtype=np.int64)
    nc = int(lines[sol + 3 + n + ne])
    cl = np.array([l.split() for l in lines[sol + 4 + n + ne:sol + 4 + n + ne + nc]], dtype=float).reshape(nc, 2)
    lu = UNIT_NAMES[hdr.get("LengthUnits", "inches")]
    Q = nod[:, 3].astype(np.int64)
    kw = dict(
        x=nod[:, 0] * UNITS[lu], y=nod[:, 1] * UNITS[lu], p=el[:, :3].astype(np.int32), lbl=el[:, 3].astype(np.int32),
        blocks=[dict(ex=float(b["ex"]), ey=float(b["ey"]), qv=float(b["qv"])) for b in blocks],
        labels=labels,
        lines=[dict(format=int(b.get("BdryType", 0)), V=float(b.get("Vs", 0)), qs=float(b.get("qs", 0)),
                    c0=float(b.get("c0", 0)), c1=float(b.get("c1", 0))) for b in bdrys],
        points=[dict(V=float(q.get("Vp", 0)), qp=float(q.get("qp", 0))) for q in points],
        conductors=[dict(type=int(c["ConductorType"]), V=float(c["Vc"]), q=float(c["qc"])) for c in conductors],
        conductor=np.where(Q >= 0, Q, -1).astype(np.int32),
        precision=float(hdr["Precision"]), length_units=lu,
        problem_type=1 if hdr.get("ProblemType", "planar") == "axisymmetric" else 0,
        depth=float(hdr.get("Depth", 1)), ext_zo=float(hdr.get("extZo", 0)), ext_ro=float(hdr.get("extRo", 0)),
        ext_ri=float(hdr.get("extRi", 0)))
    return dict(kw=kw, V=nod[:, 2].copy(), Q=Q, conductors=cl)


def _tables(kw):
    N = len(kw["x"])
    NE = len(kw["lbl"])
    p = np.asarray(kw["p"], np.int64).reshape(NE, 3)
    e = kw.get("e")
    e = -np.ones((NE, 3), np.int64) if e is None else np.asarray(e, np.int64).reshape(NE, 3)
    marker = kw.get("marker")
    marker = -np.ones(N, np.int64) if marker is None else np.asarray(marker, np.int64)
    cond = kw.get("conductor")
    cond = -np.ones(N, np.int64) if cond is None else np.asarray(cond, np.int64)
    return N, NE, p, e, marker, cond


def restate(kw: dict) -> dict:
    """ESolver::AnalyzeProblem, literally: the N + NumCircProps system with the
    per-element elimination of prescribed values, the bordered conductor rows
    with the reference's diagonal rule, Periodicity / AntiPeriodicity as
    spars.cpp:366-474 (full range), solved directly.  Returns A (dense, both
    triangles), b, V (N + NumCircProps) and Q."""
    N, NE, p, e, marker, cond = _tables(kw)
    X = np.asarray(kw["x"], float)
    Y = np.asarray(kw["y"], float)
    blocks, labels = kw["blocks"], kw["labels"]
    lines, points, circ = list(kw.get("lines", ())), list(kw.get("points", ())), list(kw.get("conductors", ()))
    NC = len(circ)
    axi = kw.get("problem_type", 0) == 1
    u = UNITS[kw.get("length_units", 0)]
    c = (1.e-6) / EO
    Depth = kw.get("depth", 1.0) * u
    extRo, extRi, extZo = kw.get("ext_ro", 0.) * u, kw.get("ext_ri", 0.) * u, kw.get("ext_zo", 0.) * u
    kludge = 1
    n_tot = N + NC
    A = np.zeros((n_tot, n_tot))
    b = np.zeros(n_tot)
    LV = np.zeros(n_tot)
    LQ = np.full(n_tot, -2, np.int64)

    def add(r, cc, v):   # Put(Get(r, cc) + v, r, cc) on symmetric storage
        A[r, cc] += v
        if r != cc:
            A[cc, r] += v

    for i in range(N):
        if marker[i] >= 0 and points[marker[i]].get("qp", 0.0) == 0:
            LV[i] = points[marker[i]].get("V", 0.0)
            LQ[i] = -1
        if cond[i] >= 0 and circ[cond[i]].get("type", 1) == 1:
            LV[i] = circ[cond[i]].get("V", 0.0)
            LQ[i] = cond[i]
    for i in range(NE):
        for j in range(3):
            k = (j + 1) % 3
            if e[i, j] >= 0 and lines[e[i, j]].get("format", 0) == 0:
                LV[p[i, j]] = lines[e[i, j]].get("V", 0.0)
                LV[p[i, k]] = lines[e[i, j]].get("V", 0.0)
                LQ[p[i, j]] = -1
                LQ[p[i, k]] = -1

    for i in range(NE):
        Me = np.zeros((3, 3))
        be = np.zeros(3)
        n = p[i]
        blk = blocks[labels[kw["lbl"][i]]["block"]]
        pp = [Y[n[1]] - Y[n[2]], Y[n[2]] - Y[n[0]], Y[n[0]] - Y[n[1]]]
        qq = [X[n[2]] - X[n[1]], X[n[0]] - X[n[2]], X[n[1]] - X[n[0]]]
        l = [np.sqrt((X[n[(j + 1) % 3]] - X[n[j]]) ** 2 + (Y[n[(j + 1) % 3]] - Y[n[j]]) ** 2) for j in range(3)]
        a = (pp[0] * qq[1] - pp[1] * qq[0]) / 2.
        r = (X[n[0]] + X[n[1]] + X[n[2]]) / 3.
        if axi:
            Depth = 2. * PI * r
            if labels[kw["lbl"][i]].get("is_external", 0):
                z = (Y[n[0]] + Y[n[1]] + Y[n[2]]) / 3. - extZo
                kludge = (r * r + z * z) / (extRi * extRo)
            else:
                kludge = 1
        K = -Depth * blk.get("ex", 1.0) / (4. * a) / kludge
        for j in range(3):
            for k in range(j, 3):
                Me[j][k] += K * pp[j] * pp[k]
                if j != k:
                    Me[k][j] += K * pp[j] * pp[k]
        K = -Depth * blk.get("ey", 1.0) / (4. * a) / kludge
        for j in range(3):
            for k in range(j, 3):
                Me[j][k] += K * qq[j] * qq[k]
                if j != k:
                    Me[k][j] += K * qq[j] * qq[k]
        for j in range(3):
            K = -Depth * c * blk.get("qv", 0.0) * a / 3.
            be[j] += K
        for j in range(3):
            if e[i, j] >= 0:
                k = (j + 1) % 3
                ln = lines[e[i, j]]
                if axi:
                    Depth = PI * (X[n[j]] + X[n[k]])
                if ln.get("format", 0) == 1:
                    K = -1000. * Depth * c * ln.get("c0", 0.0) * l[j] / 6.
                    Me[j][j] += K * 2.
                    Me[k][k] += K * 2.
                    Me[j][k] += K
                    Me[k][j] += K
                    K = 1000. * Depth * c * ln.get("c1", 0.0) * l[j] / 2.
                    be[j] += K
                    be[k] += K
                if ln.get("format", 0) == 2:
                    K = -1000. * Depth * c * ln.get("qs", 0.0) * l[j] / 2.
                    be[j] += K
                    be[k] += K
        for j in range(3):
            if LQ[n[j]] != -2:
                for k in range(3):
                    if j != k:
                        be[k] -= Me[k][j] * LV[n[j]]
                        Me[k][j] = 0
                        Me[j][k] = 0
                be[j] = LV[n[j]] * Me[j][j]
        ne_ = [int(v) for v in n]
        for j in range(3):
            if cond[n[j]] >= 0 and circ[cond[n[j]]].get("type", 1) == 0:
                ne_[j] = int(cond[n[j]]) + N
        for j in range(3):
            for k in range(j, 3):
                add(ne_[j], ne_[k], -Me[j][k])
            b[ne_[j]] -= be[j]
            if ne_[j] != n[j]:
                add(n[j], n[j], -Me[j][j])
                add(n[j], ne_[j], Me[j][j])

    for i in range(N):
        if marker[i] >= 0 and LQ[i] == -2:
            if axi:
                Depth = 2. * PI * X[i]
            b[i] += ((1.e6) * Depth * c * points[marker[i]].get("qp", 0.0))
            LQ[i] = -1
        if cond[i] >= 0:
            LQ[i] = cond[i]

    pbc = kw.get("pbc")
    for i, j, t in (np.asarray(pbc, np.int64).reshape(-1, 3) if pbc is not None and len(pbc) else ()):
        if j < i:
            i, j = j, i
        sg = 1.0 if t == 0 else -1.0
        for k in range(n_tot):
            if k != i and k != j:
                v1, v2 = A[k, i], A[k, j]
                if v1 != 0 or v2 != 0:
                    cc = (v1 + sg * v2) / 2.
                    A[k, i] = A[i, k] = cc
                    A[k, j] = A[j, k] = sg * cc
        cc = 0.5 * (A[i, i] + A[j, j])
        A[i, i] = cc
        A[j, j] = cc
        cc = 0.5 * (b[i] + sg * b[j])
        b[i] = cc
        b[j] = sg * cc

    for i in range(NC):
        k = N + i
        if circ[i].get("type", 1) == 1:
            K = A[0, 0]
            A[k, k] = K
            b[k] = K * circ[i].get("V", 0.0)
        else:
            K = A[k].sum() - A[k, k]
            if K != 0:
                A[k, k] = -K
                b[k] = (1.e9) * c * circ[i].get("q", 0.0)
            else:
                A[k, k] = A[0, 0]
    V = spla.spsolve(sp.csc_matrix(A), b)
    return dict(A=A, b=b, V=V, Q=LQ[:N].copy(), N=N)


def charge_functional(kw: dict, conductor: int) -> np.ndarray:
    """g with ChargeOnConductor(conductor) = g . V (esolver.cpp:797-844: the
    integral is linear in the nodal potentials)."""
    N, NE, p, e, marker, cond = _tables(kw)
    X = np.asarray(kw["x"], float)
    Y = np.asarray(kw["y"], float)
    axi = kw.get("problem_type", 0) == 1
    Depth = kw.get("depth", 1.0) * UNITS[kw.get("length_units", 0)]
    LC = 0.001
    P = (cond == conductor).astype(float)
    g = np.zeros(N)
    for i in range(NE):
        n = p[i]
        if not P[n].any():
            continue
        blk = kw["blocks"][kw["labels"][kw["lbl"][i]]["block"]]
        bb = [Y[n[1]] - Y[n[2]], Y[n[2]] - Y[n[0]], Y[n[0]] - Y[n[1]]]
        cc = [X[n[2]] - X[n[1]], X[n[0]] - X[n[2]], X[n[1]] - X[n[0]]]
        da = (bb[0] * cc[1] - bb[1] * cc[0])
        a = da * LC * LC / 2.
        if axi:
            a *= (2. * PI * LC * (X[n[0]] + X[n[1]] + X[n[2]]) / 3.)
        else:
            a *= (Depth * LC)
        vx = vy = 0.0
        for k in range(3):
            vx -= (P[n[k]] * bb[k]) / (da * LC)
            vy -= (P[n[k]] * cc[k]) / (da * LC)
        for k in range(3):
            g[n[k]] += a * (-(bb[k] / (da * LC)) * (EO * blk.get("ex", 1.0)) * vx
                            - (cc[k] / (da * LC)) * (EO * blk.get("ey", 1.0)) * vy)
    return g


def charge(kw: dict, V, conductor: int) -> float:
    """ESolver::ChargeOnConductor on the nodal potentials V, literally."""
    N, NE, p, e, marker, cond = _tables(kw)
    X = np.asarray(kw["x"], float)
    Y = np.asarray(kw["y"], float)
    axi = kw.get("problem_type", 0) == 1
    Depth = kw.get("depth", 1.0) * UNITS[kw.get("length_units", 0)]
    LC = 0.001
    P = (cond == conductor).astype(float)
    Z = 0.0
    for i in range(NE):
        n = p[i]
        if P[n[0]] != 0 or P[n[1]] != 0 or P[n[2]] != 0:
            blk = kw["blocks"][kw["labels"][kw["lbl"][i]]["block"]]
            bb = [Y[n[1]] - Y[n[2]], Y[n[2]] - Y[n[0]], Y[n[0]] - Y[n[1]]]
            cc = [X[n[2]] - X[n[1]], X[n[0]] - X[n[2]], X[n[1]] - X[n[0]]]
            da = (bb[0] * cc[1] - bb[1] * cc[0])
            a = da * LC * LC / 2.
            if axi:
                a *= (2. * PI * LC * (X[n[0]] + X[n[1]] + X[n[2]]) / 3.)
            else:
                a *= (Depth * LC)
            vx = vy = Dx = Dy = 0.0
            for k in range(3):
                vx -= (P[n[k]] * bb[k]) / (da * LC)
                vy -= (P[n[k]] * cc[k]) / (da * LC)
                Dx -= (V[n[k]] * bb[k]) / (da * LC)
                Dy -= (V[n[k]] * cc[k]) / (da * LC)
            Dx *= (EO * blk.get("ex", 1.0))
            Dy *= (EO * blk.get("ey", 1.0))
            Z += a * (Dx * vx + Dy * vy)
    return Z


def grid(nx: int, ny: int, w: float, h: float, x0: float = 0.0, y0: float = 0.0):
    """nx x ny nodes on [x0, x0 + w] x [y0, y0 + h] (row-major, x fastest), each
    cell cut into two counter-clockwise triangles, the diagonal alternating."""
    xs = x0 + w * np.arange(nx) / (nx - 1)
    ys = y0 + h * np.arange(ny) / (ny - 1)
    x = np.tile(xs, ny)
    y = np.repeat(ys, nx)
    p = []
    for j in range(ny - 1):
        for i in range(nx - 1):
            a, b, c, d = j * nx + i, j * nx + i + 1, (j + 1) * nx + i + 1, (j + 1) * nx + i
            p += [[a, b, c], [a, c, d]] if (i + j) % 2 == 0 else [[a, b, d], [b, c, d]]
    return x, y, np.array(p, np.int32)


def tag_edges(x, y, p, rules):
    """e[i, j] = the property of the first rule (pred(xa, ya, xb, yb) -> bool,
    property) that edge j of element i (p[i, j] -> p[i, (j + 1) % 3]) meets."""
    e = -np.ones(p.shape, np.int32)
    for i in range(len(p)):
        for j in range(3):
            a, b = p[i, j], p[i, (j + 1) % 3]
            for pred, prop in rules:
                if pred(x[a], y[a], x[b], y[b]):
                    e[i, j] = prop
                    break
    return e
