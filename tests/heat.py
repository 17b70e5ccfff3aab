"""Heat-flow test helpers (CPU): a reader of the reference's .anh files, a
literal numpy restatement of one pass of HSolver::AnalyzeProblem
(cfemm/hsolver/hsolver.cpp:458-852) solved directly, its outer loop with the
reference's stopping rule, and HSolver::ChargeOnConductor (hsolver.cpp:987-1035).

A problem is the keyword dictionary of kernels.HeatFlowProblem: the device and
the restatement read the same arrays (coordinates in metres)."""
from __future__ import annotations

import gzip
import re

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from electro import grid, tag_edges  # noqa: F401  (the structured meshes)

PI = 3.141592653589793238462643383
KSB = 5.67032e-8                                       # femmconstants.h
UNITS = (0.0254, 0.001, 0.01, 1, 2.54e-5, 1.e-6)       # hsolver.cpp:65, user units -> m
UNIT_NAMES = {"inches": 0, "millimeters": 1, "centimeters": 2, "meters": 3, "mils": 4, "microns": 5,
              "micrometers": 5}


def read_anh(path: str) -> dict:
    """An .anh file, plain or gzip-compressed (the echoed .feh header, then
    [Solution]) -> the problem's keyword dictionary plus the recorded V and Q (per node).  The file does not
    carry the mesh's .edge data; the fixtures' convection edges are recovered
    from geometry: an element edge with both nodes on y == 2 or both on x == 2
    (file units, exact in the file) carries boundary property 0."""
    opener = gzip.open if path.endswith(".gz") else open
    lines = opener(path, "rt").read().splitlines()
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
            if m and m.group(1) == "TKPoints":
                n = int(m.group(2))
                tk = np.array([head[i + 1 + k].split() for k in range(n)], dtype=float).reshape(n, 2)
                cur["T"], cur["K"] = tk[:, 0].copy(), tk[:, 1].copy()
                i += n
            elif m:
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
    p = el[:, :3].astype(np.int32)
    xf, yf = nod[:, 0], nod[:, 1]
    e = -np.ones(p.shape, np.int32)
    for j in range(3):
        a, b = p[:, j], p[:, (j + 1) % 3]
        e[((yf[a] == 2) & (yf[b] == 2)) | ((xf[a] == 2) & (xf[b] == 2)), j] = 0

    def block(b):
        d = dict(kx=float(b["Kx"]), ky=float(b["Ky"]), kt=float(b["Kt"]), qv=float(b["qv"]))
        if "T" in b:
            d.update(T=b["T"], K=b["K"])
        return d

    kw = dict(
        x=xf * UNITS[lu], y=yf * UNITS[lu], p=p, e=e, lbl=el[:, 3].astype(np.int32),
        blocks=[block(b) for b in blocks], labels=labels,
        lines=[dict(format=int(b.get("BdryType", 0)), Tset=float(b.get("Tset", 0)), qs=float(b.get("qs", 0)),
                    beta=float(b.get("beta", 0)), h=float(b.get("h", 0)), Tinf=float(b.get("Tinf", 0)))
               for b in bdrys],
        points=[dict(T=float(q.get("Tp", 0)), qp=float(q.get("qp", 0))) for q in points],
        conductors=[dict(type=int(c["ConductorType"]), T=float(c["Tc"]), q=float(c["qc"])) for c in conductors],
        conductor=np.where(Q >= 0, Q, -1).astype(np.int32),
        precision=float(hdr["Precision"]), length_units=lu,
        problem_type=1 if hdr.get("ProblemType", "planar") == "axisymmetric" else 0,
        depth=float(hdr.get("Depth", 1)), ext_zo=float(hdr.get("extZo", 0)), ext_ro=float(hdr.get("extRo", 0)),
        ext_ri=float(hdr.get("extRi", 0)), dt=float(hdr.get("dT", 0)))
    return dict(kw=kw, V=nod[:, 2].copy(), Q=Q, conductors=cl)


def getk(blk: dict, t: float):
    """CHMaterialProp::GetK (CMaterialProp.cpp:1388-1409), literally: (Kx, Ky)."""
    T, K = blk.get("T"), blk.get("K")
    npts = 0 if T is None else len(T)
    if npts == 0:
        return blk.get("kx", 1.0), blk.get("ky", 1.0)
    if npts == 1:
        return K[0], K[0]
    if t <= T[0]:
        return K[0], K[0]
    if t >= T[npts - 1]:
        return K[npts - 1], K[npts - 1]
    for i in range(npts - 1):
        j = i + 1
        if t >= T[i] and t <= T[j]:
            v = K[i] + (K[j] - K[i]) * (t - T[i]) / (T[j] - T[i])
            return v, v
    return blk.get("kx", 1.0), blk.get("ky", 1.0)


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


def is_nonlinear(kw: dict) -> bool:
    """A K(T) table on the block of any element, or a radiation edge on any
    element (the reference scans the blocks of its first NumNodes elements
    only; the project scans every element)."""
    N, NE, p, e, marker, cond = _tables(kw)
    for i in range(NE):
        T = kw["blocks"][kw["labels"][kw["lbl"][i]]["block"]].get("T")
        if T is not None and len(T) > 0:
            return True
    lines = list(kw.get("lines", ()))
    return any(lines[v].get("format", 0) == 3 for v in e.reshape(-1) if v >= 0)


def restate(kw: dict, Vo=None, merged: bool = False, dense: bool = True) -> dict:
    """One pass of HSolver::AnalyzeProblem from the nodal temperatures Vo
    (None: zeros), literally: the N + NumCircProps system with the per-element
    elimination of prescribed values, the bordered conductor rows with the
    reference's diagonal rule, Periodicity / AntiPeriodicity as
    spars.cpp:366-474, solved directly.  Returns A (dense, both triangles;
    sparse `As` always), b, V (N + NumCircProps) and Q.

    merged=True gives the project's documented form of a CircType 0 conductor
    instead of the bordered one: the conductor's nodes merged onto its
    lowest-numbered node, whose row carries q on its right-hand side; the other
    nodes are identity rows with a zero right-hand side (their value is copied
    after the solve: V returns it copied)."""
    N, NE, p, e, marker, cond = _tables(kw)
    X = np.asarray(kw["x"], float)
    Y = np.asarray(kw["y"], float)
    blocks, labels = kw["blocks"], kw["labels"]
    lines, points, circ = list(kw.get("lines", ())), list(kw.get("points", ())), list(kw.get("conductors", ()))
    NC = len(circ)
    axi = kw.get("problem_type", 0) == 1
    u = UNITS[kw.get("length_units", 0)]
    Depth = kw.get("depth", 1.0) * u
    extRo, extRi, extZo = kw.get("ext_ro", 0.) * u, kw.get("ext_ri", 0.) * u, kw.get("ext_zo", 0.) * u
    dT = kw.get("dt", 0.0)
    Tprev = kw.get("t_prev")
    Tprev = np.zeros(N) if Tprev is None else np.asarray(Tprev, float)
    Vo = np.zeros(N) if Vo is None else np.asarray(Vo, float)
    kludge = 1
    n_tot = N + NC
    rows, cols, vals = [], [], []
    b = np.zeros(n_tot)
    LV = np.zeros(n_tot)
    LQ = np.full(n_tot, -2, np.int64)
    rep = {}
    if merged:
        for i in range(N):
            if cond[i] >= 0 and circ[cond[i]].get("type", 1) == 0 and cond[i] not in rep:
                rep[int(cond[i])] = i

    def add(r, cc, v):   # Put(Get(r, cc) + v, r, cc) on symmetric storage
        rows.append(r)
        cols.append(cc)
        vals.append(v)
        if r != cc:
            rows.append(cc)
            cols.append(r)
            vals.append(v)

    for i in range(N):
        if marker[i] >= 0 and points[marker[i]].get("qp", 0.0) == 0:
            LV[i] = points[marker[i]].get("T", 0.0)
            LQ[i] = -1
        if cond[i] >= 0 and circ[cond[i]].get("type", 1) == 1:
            LV[i] = circ[cond[i]].get("T", 0.0)
            LQ[i] = cond[i]
    for i in range(NE):
        for j in range(3):
            k = (j + 1) % 3
            if e[i, j] >= 0 and lines[e[i, j]].get("format", 0) == 0:
                LV[p[i, j]] = lines[e[i, j]].get("Tset", 0.0)
                LV[p[i, k]] = lines[e[i, j]].get("Tset", 0.0)
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
        k0, k1, k2 = getk(blk, Vo[n[0]]), getk(blk, Vo[n[1]]), getk(blk, Vo[n[2]])
        knx, kny = (k0[0] + k1[0] + k2[0]) / 3., (k0[1] + k1[1] + k2[1]) / 3.
        if axi:
            Depth = 2. * PI * r
            if labels[kw["lbl"][i]].get("is_external", 0):
                z = (Y[n[0]] + Y[n[1]] + Y[n[2]]) / 3. - extZo
                kludge = (r * r + z * z) / (extRi * extRo)
            else:
                kludge = 1
        K = -Depth * knx / (4. * a) / kludge
        for j in range(3):
            for k in range(j, 3):
                Me[j][k] += K * pp[j] * pp[k]
                if j != k:
                    Me[k][j] += K * pp[j] * pp[k]
        K = -Depth * kny / (4. * a) / kludge
        for j in range(3):
            for k in range(j, 3):
                Me[j][k] += K * qq[j] * qq[k]
                if j != k:
                    Me[k][j] += K * qq[j] * qq[k]
        if dT != 0:
            K = -Depth * blk.get("kt", 0.0) * a / (3. * dT)
            for j in range(3):
                Me[j][j] += K
                be[j] += K * Tprev[n[j]]
        for j in range(3):
            K = -Depth * blk.get("qv", 0.0) * a / 3.
            be[j] += K
        for j in range(3):
            if e[i, j] >= 0:
                k = (j + 1) % 3
                ln = lines[e[i, j]]
                if axi:
                    Depth = PI * (X[n[j]] + X[n[k]])
                bf = ln.get("format", 0)
                if bf in (1, 2, 3):
                    if bf == 1:
                        c1 = ln.get("qs", 0.0)
                        c0 = 0
                    elif bf == 2:
                        c0 = ln.get("h", 0.0)
                        c1 = -c0 * ln.get("Tinf", 0.0)
                    else:
                        bta = ln.get("beta", 0.0)
                        Tinf = ln.get("Tinf", 0.0)
                        Tlast = (Vo[n[j]] + Vo[n[k]]) / 2.
                        c0 = 4. * bta * KSB * Tlast ** 3.
                        c1 = -(bta * KSB * (Tinf ** 4. + 3. * Tlast ** 4.))
                    if axi:
                        K = -2. * PI * c0 * l[j] / 6.
                        Me[j][j] += K * 2. * (3. * X[n[j]] + X[n[k]]) / 4.
                        Me[k][k] += K * 2. * (X[n[j]] + 3. * X[n[k]]) / 4.
                        Me[j][k] += K * (X[n[j]] + X[n[k]]) / 2.
                        Me[k][j] += K * (X[n[j]] + X[n[k]]) / 2.
                        K = 2. * PI * c1 * l[j] / 2.
                        be[j] += K * (2. * X[n[j]] + X[n[k]]) / 3.
                        be[k] += K * (X[n[j]] + 2. * X[n[k]]) / 3.
                    else:
                        K = -Depth * c0 * l[j] / 6.
                        Me[j][j] += K * 2.
                        Me[k][k] += K * 2.
                        Me[j][k] += K
                        Me[k][j] += K
                        K = Depth * c1 * l[j] / 2.
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
                ne_[j] = rep[int(cond[n[j]])] if merged else int(cond[n[j]]) + N
        for j in range(3):
            if merged:
                # (the Galerkin projection onto one value per conductor: every
                # entry of Me, both triangles, lands on the merged indices)
                for k in range(3):
                    rows.append(ne_[j])
                    cols.append(ne_[k])
                    vals.append(-Me[j][k])
                b[ne_[j]] -= be[j]
                continue
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
            b[i] += (Depth * points[marker[i]].get("qp", 0.0))
            LQ[i] = -1
        if cond[i] >= 0:
            LQ[i] = cond[i]

    As = sp.coo_matrix((vals, (rows, cols)), shape=(n_tot, n_tot)).tocsr()
    pbc = kw.get("pbc")
    if pbc is not None and len(pbc):
        A = As.toarray()
        for i, j, t in np.asarray(pbc, np.int64).reshape(-1, 3):
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
        As = sp.csr_matrix(A)

    As = As.tolil()
    slaves = []
    for i in range(NC):
        k = N + i
        if circ[i].get("type", 1) == 1 or merged:
            K = As[0, 0]
            As[k, k] = K
            b[k] = K * (circ[i].get("T", 0.0) if circ[i].get("type", 1) == 1 else 0.0)
            if merged and circ[i].get("type", 1) == 0 and i in rep:
                b[rep[i]] += circ[i].get("q", 0.0)
                for m in np.flatnonzero(cond == i):
                    if m != rep[i]:
                        As[m, m] = 1.0
                        b[m] = 0.0
                        slaves.append((int(m), rep[i]))
        else:
            K = As[k].sum() - As[k, k]
            if K != 0:
                As[k, k] = -K
                b[k] = circ[i].get("q", 0.0)
            else:
                As[k, k] = As[0, 0]
    As = As.tocsr()
    V = spla.spsolve(As.tocsc(), b)
    for m, r_ in slaves:
        V[m] = V[r_]
    if merged:
        for i in range(NC):
            if circ[i].get("type", 1) == 0 and i in rep:
                V[N + i] = V[rep[i]]
    out = dict(As=As, b=b, V=V, Q=LQ[:N].copy(), N=N)
    if dense:
        out["A"] = As.toarray()
    return out


def change(V, Vo):
    """The two sums of hsolver.cpp:827-830."""
    V, Vo = np.asarray(V, float), np.asarray(Vo, float)
    return float(((V - Vo) * (V - Vo)).sum()), float((Vo * Vo).sum())


def restate_solve(kw: dict, max_passes: int = 100) -> dict:
    """The outer loop of HSolver::AnalyzeProblem with the reference's stopping
    rule (a linear problem: one pass; no test while sum Vo^2 == 0).  Returns V
    (N + NumCircProps), the pass count and the change sqrt(e1 / e2) of every
    tested pass."""
    N = len(kw["x"])
    nonlinear = is_nonlinear(kw)
    V = np.zeros(N + len(kw.get("conductors", ())))
    passes, hist = 0, []
    while True:
        Vo = V[:N].copy()
        V = restate(kw, Vo, dense=False)["V"]
        passes += 1
        if not nonlinear:
            break
        e1, e2 = change(V[:N], Vo)
        if e2 != 0:
            hist.append(np.sqrt(e1 / e2))
            if hist[-1] < kw.get("precision", 1e-8) * 100.:
                break
        elif e1 == 0:
            break
        if passes >= max_passes:
            raise RuntimeError("restatement did not converge in %d passes" % passes)
    return dict(V=V, passes=passes, changes=hist)


def flow(kw: dict, V, conductor: int) -> float:
    """HSolver::ChargeOnConductor on the nodal temperatures V, literally."""
    N, NE, p, e, marker, cond = _tables(kw)
    X = np.asarray(kw["x"], float)
    Y = np.asarray(kw["y"], float)
    axi = kw.get("problem_type", 0) == 1
    Depth = kw.get("depth", 1.0) * UNITS[kw.get("length_units", 0)]
    P = (cond == conductor).astype(float)
    Z = 0.0
    for i in range(NE):
        n = p[i]
        if P[n[0]] != 0 or P[n[1]] != 0 or P[n[2]] != 0:
            blk = kw["blocks"][kw["labels"][kw["lbl"][i]]["block"]]
            bb = [Y[n[1]] - Y[n[2]], Y[n[2]] - Y[n[0]], Y[n[0]] - Y[n[1]]]
            cc = [X[n[2]] - X[n[1]], X[n[0]] - X[n[2]], X[n[1]] - X[n[0]]]
            da = (bb[0] * cc[1] - bb[1] * cc[0])
            a = da / 2.
            if axi:
                a *= (2. * PI * (X[n[0]] + X[n[1]] + X[n[2]]) / 3.)
            else:
                a *= Depth
            vx = vy = Dx = Dy = knx = kny = 0.0
            for k in range(3):
                vx -= (P[n[k]] * bb[k]) / da
                vy -= (P[n[k]] * cc[k]) / da
                Dx -= (V[n[k]] * bb[k]) / da
                Dy -= (V[n[k]] * cc[k]) / da
                kk = getk(blk, V[n[k]])
                knx += kk[0] / 3.
                kny += kk[1] / 3.
            Dx *= knx
            Dy *= kny
            Z += a * (Dx * vx + Dy * vy)
    return Z
