"""Helpers of the ESolver / HSolver tests (CPU): the input files of the
reference's solved fixtures, a literal numpy restatement of ESolver::LoadMesh
(cfemm/esolver/esolver.cpp:127-374; HSolver::LoadMesh, hsolver.cpp:187-431, is
the same code with metres), readers of the written .res / .anh text, and small
synthetic problems written to files."""
from __future__ import annotations

import gzip
import os

import numpy as np

import electro
import heat
from util import GOLDEN
from xfemm_amd import synth

FIXTURES = {"test": ("e", os.path.join(GOLDEN, "esolver", "test.res.check")),
            "Temp0": ("h", os.path.join(GOLDEN, "hsolver", "Temp0.anh.check.gz")),
            "Temp1": ("h", os.path.join(GOLDEN, "hsolver", "Temp1.anh.check.gz"))}
EXT = {"e": (".fee", ".res"), "h": (".feh", ".anh")}
UNITS = {"e": electro.UNITS, "h": heat.UNITS}


def fixture_text(name: str) -> str:
    kind, path = FIXTURES[name]
    return (gzip.open(path, "rt") if path.endswith(".gz") else open(path)).read()


def fixture_input(name: str) -> str:
    """The echoed .fee / .feh: the part of the fixture before [Solution]."""
    t = fixture_text(name)
    return t[:t.index("[Solution]\n")]


def read_fixture(name: str) -> dict:
    kind, path = FIXTURES[name]
    return electro.read_res(path) if kind == "e" else heat.read_anh(path)


def write_fixture_case(name: str, base: str) -> dict:
    """<base>.fee/.feh and the four mesh files from the fixture's own nodes
    (file units, as recorded), elements, conductor marks and -- heat flow --
    the convection edges read_anh recovers.  Returns the fixture."""
    kind, _ = FIXTURES[name]
    f = read_fixture(name)
    with open(base + EXT[kind][0], "w") as fh:
        fh.write(fixture_input(name))
    lines = fixture_text(name).splitlines()
    sol = lines.index("[Solution]")
    n = int(lines[sol + 1])
    xy = np.array([l.split()[:2] for l in lines[sol + 2:sol + 2 + n]], dtype=float)
    kw = f["kw"]
    marks = synth.side_edge_marks(kw["p"], kw["e"]) if kw.get("e") is not None else ()
    synth.write_potential_mesh(base, xy[:, 0], xy[:, 1], kw["p"], kw["lbl"], conductor=kw["conductor"],
                               edge_marks=marks)
    f["xy_file"] = xy
    return f


def read_output(path: str) -> dict:
    """A written .res / .anh: the header bytes, and the [Solution] section as
    text fields (x, y kept as written) and arrays."""
    t = open(path).read()
    k = t.index("[Solution]\n")
    lines = t[k:].splitlines()
    n = int(lines[1])
    nod = [l.split("\t") for l in lines[2:2 + n]]
    ne = int(lines[2 + n])
    el = np.array([l.split("\t") for l in lines[3 + n:3 + n + ne]], dtype=np.int64).reshape(ne, 4)
    nc = int(lines[3 + n + ne])
    cl = np.array([l.split("\t") for l in lines[4 + n + ne:4 + n + ne + nc]], dtype=float).reshape(nc, 2)
    assert len(lines) == 4 + n + ne + nc
    return dict(header=t[:k], xt=[r[0] for r in nod], yt=[r[1] for r in nod],
                x=np.array([float(r[0]) for r in nod]), y=np.array([float(r[1]) for r in nod]),
                V=np.array([float(r[2]) for r in nod]), Q=np.array([int(r[3]) for r in nod], dtype=np.int64),
                p=el[:, :3], lbl=el[:, 3], conductors=cl)


def match_nodes(xo, yo, xi, yi) -> np.ndarray:
    """perm with (xo[k], yo[k]) == (xi[perm[k]], yi[perm[k]]) exactly; the points are distinct."""
    where = {(a, b): i for i, (a, b) in enumerate(zip(xi.tolist(), yi.tolist()))}
    assert len(where) == len(xi)
    return np.array([where[(a, b)] for a, b in zip(xo.tolist(), yo.tolist())], dtype=np.int64)


class MissingMaterial(Exception):
    pass


def load_mesh_ref(base: str, labels, line_formats, unit: float) -> dict:
    """ESolver::LoadMesh, literally, on the files at <base>: labels carry
    block and is_default, line_formats the BdryFormat of each boundary
    property, unit the length conversion."""
    tok = open(base + ".node").read().split("\n", 1)
    n = int(tok[0].split()[0])
    v = tok[1].split()
    x, y = np.zeros(n), np.zeros(n)
    marker, cond = np.zeros(n, np.int64), np.zeros(n, np.int64)
    for i in range(n):
        x[i], y[i], m = float(v[4 * i + 1]) * unit, float(v[4 * i + 2]) * unit, int(v[4 * i + 3])
        if m > 1:
            j = (m & 0xffff) - 2
            marker[i] = -1 if j < 0 else j
            cond[i] = (m - (m & 0xffff)) // 0x10000 - 1
        else:
            marker[i] = cond[i] = -1
    tok = open(base + ".pbc").read().split("\n", 1)
    k = int(tok[0].split()[0])
    v = tok[1].split()
    pbc = np.array([[int(v[4 * i + 1]), int(v[4 * i + 2]), int(v[4 * i + 3])] for i in range(k)],
                   dtype=np.int64).reshape(k, 3)
    tok = open(base + ".ele").read().split("\n", 1)
    ne = int(tok[0].split()[0])
    v = tok[1].split()
    default = -1
    for i, lb in enumerate(labels):
        if lb.get("is_default"):
            default = i
    p = np.zeros((ne, 3), np.int64)
    lbl, blk = np.zeros(ne, np.int64), np.zeros(ne, np.int64)
    for i in range(ne):
        p[i] = [int(v[5 * i + 1]), int(v[5 * i + 2]), int(v[5 * i + 3])]
        l = int(v[5 * i + 4]) - 1
        if l < 0:
            l = default
        if l < 0:
            raise MissingMaterial(i)
        lbl[i], blk[i] = l, labels[l]["block"]
    e = -np.ones((ne, 3), np.int64)
    mbr = [[] for _ in range(n)]
    for i in range(ne):
        for j in range(3):
            mbr[p[i, j]].append(i)
    v = open(base + ".edge").read().split()
    k = int(v[0])
    v = v[2:]
    for i in range(k):
        n0, n1, m = int(v[4 * i + 1]), int(v[4 * i + 2]), int(v[4 * i + 3])
        if m < 0:
            m = -m
            j = (m & 0xffff) - 2
            if j < 0:
                j = -1
            c = (m - (m & 0xffff)) // 0x10000 - 1
            if c >= 0:
                cond[n0] = cond[n1] = c
        else:
            j = -1
        if j >= 0:
            hit = False
            for q in mbr[n0]:
                for s in range(3):
                    a, b = p[q, s], p[q, (s + 1) % 3]
                    if (a == n0 and b == n1) or (a == n1 and b == n0):
                        e[q, s] = j
                        hit = True
                if line_formats[j] == 2 and hit:
                    break
    return dict(x=x, y=y, marker=marker, conductor=cond, pbc=pbc, p=p, lbl=lbl, blk=blk, e=e)


def write_case(kind: str, base: str, kw: dict, marker=None, conductor=None, edge_marks=None, unit_scale=None):
    """<base>.fee/.feh and mesh files of a keyword dictionary whose x, y are in
    the solver's unit: the files carry them in the problem's length units."""
    u = UNITS[kind][kw.get("length_units", 0)] if unit_scale is None else unit_scale
    with open(base + EXT[kind][0], "w") as fh:
        fh.write(synth.potential_text(kind, kw))
    if edge_marks is None:
        edge_marks = synth.side_edge_marks(kw["p"], kw["e"]) if kw.get("e") is not None else ()
    synth.write_potential_mesh(base, np.asarray(kw["x"]) / u, np.asarray(kw["y"]) / u, kw["p"], kw["lbl"],
                               marker=kw.get("marker") if marker is None else marker,
                               conductor=kw.get("conductor") if conductor is None else conductor,
                               edge_marks=edge_marks, pbc=kw.get("pbc"))
