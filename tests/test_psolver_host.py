"""Host side of ESolver / HSolver (CPU only): C-ABI exports, the .fee / .feh
parser against the fixtures' own readers, LoadMesh against a numpy restatement
of esolver.cpp:127-374 on a mesh whose markers take every branch, the shared
renumbering against FSolver's on the same mesh files, and the refused time
step."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import electro
import psolverref as R
from util import ROOT
from xfemm_amd import fsolver, psolver, synth


def test_c_abi_library_exports_every_declared_symbol():
    txt = open(os.path.join(ROOT, "include", "xfemm_psolver.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    names = sorted(set(re.findall(r"\b(xfemm_\w+)\s*\(", txt)))
    assert len(names) == 74
    lib = C.CDLL(fsolver.FSOLVER_SO)
    for nm in names:
        assert hasattr(lib, nm), nm
    assert sorted(psolver.EXPORTED) == names


# ---- the parser ----------------------------------------------------------------

def _same(a, b):
    if isinstance(a, dict):
        return set(a) == set(b) and all(_same(a[k], b[k]) for k in a)
    return np.array_equal(np.asarray(a, dtype=float), np.asarray(b, dtype=float))


@pytest.mark.parametrize("name", ["test", "Temp0", "Temp1"])
def test_parser_reads_what_the_fixture_readers_read(tmp_path, name):
    kind = R.FIXTURES[name][0]
    base = str(tmp_path / name)
    with open(base + R.EXT[kind][0], "w") as fh:
        fh.write(R.fixture_input(name))
    want = R.read_fixture(name)["kw"]
    s = psolver.ESolver() if kind == "e" else psolver.HSolver()
    s.PathName = base
    assert s.LoadProblemFile(), s.last_error()
    got = s.kw()
    for key in ("blocks", "lines", "points", "conductors"):
        assert len(got[key]) == len(want[key]), key
        for a, b in zip(got[key], want[key]):
            assert _same(a, b), (key, a, b)
    assert [(l["block"], l["is_external"]) for l in s.labels()] == [(l["block"], l["is_external"])
                                                                    for l in want["labels"]]
    for key in ("precision", "length_units", "problem_type", "depth", "ext_zo", "ext_ro", "ext_ri"):
        assert got[key] == want[key], key
    if kind == "h":
        assert s.header()["dt"] == want["dt"]
        assert s.previousSolutionFile == ("Temp0.anh" if name == "Temp1" else "")
        assert len(got["blocks"][1]["T"]) == 18 and got["blocks"][1]["K"][17] == 0.1032   # <TKPoints>


def test_parser_reads_default_labels_inches_and_exterior(tmp_path):
    kw = dict(blocks=[dict(ex=2.0)], labels=[dict(block=0), dict(block=0, is_default=True, is_external=1)],
              length_units=0, problem_type=1, ext_zo=1.5, ext_ro=2.5, ext_ri=3.5, depth=0.75, precision=1e-9)
    (tmp_path / "a.fee").write_text(synth.potential_text("e", kw))
    s = psolver.ESolver()
    s.PathName = str(tmp_path / "a")
    assert s.LoadProblemFile(), s.last_error()
    assert s.labels() == [dict(block=0, is_external=0, is_default=0), dict(block=0, is_external=1, is_default=1)]
    h = s.header()
    assert (h["length_units"], h["problem_type"], h["ext_zo"], h["ext_ro"], h["ext_ri"], h["depth"],
            h["precision"]) == (0, 1, 1.5, 2.5, 3.5, 0.75, 1e-9)


@pytest.mark.parametrize("text,what", [
    ("[Format] = 1\n[Bogus] = 3\n", "Unknown token"),
    ("[Format] = 1\n[Precision] = abc\n", "Parse error"),
    ("[Format] = 1\n[BlockProps] = 1\n  <BeginBlock>\n    <Kx> = 1\n", "unterminated block"),
    ("[Format] = 1\n[BlockProps] = 1\n  <BeginBlock>\n    <TKPoints> = 3\n  1 2\n  <EndBlock>\n", "Parse error"),
    ("[Format] = 1\n[NumBlockLabels] = 2\n0 0 1 -1 0 0\n", "block label"),
    ("[Format] = 1\n[NumBlockLabels] = 1\n0 0 4 -1 0 0\n", "undefined block property"),
])
def test_malformed_files_fail_with_a_message(tmp_path, text, what):
    (tmp_path / "bad.feh").write_text(text)
    s = psolver.HSolver()
    s.PathName = str(tmp_path / "bad")
    assert not s.LoadProblemFile()
    assert what in s.last_error(), s.last_error()
    s.PathName = str(tmp_path / "absent")
    assert not s.LoadProblemFile() and "Couldn't read" in s.last_error()


# ---- LoadMesh --------------------------------------------------------------------

def _branch_mesh():
    """12 x 9 cells in inches.  Point property only (node 5), conductor only
    (node 20), both (node 40); an edge marker with a conductor and no property
    (bottom row), with a property and a conductor (top row), a BdryFormat 2
    edge inside the mesh (two elements hold it), a BdryFormat 0 edge on the
    left side; label 0 in the file for the right half (the default label)."""
    nx, ny = 13, 10
    x, y, p = electro.grid(nx, ny, 6.0, 4.5)
    lbl = np.where(x[p].mean(axis=1) > 3.0, -1, 0)
    marker = -np.ones(nx * ny, np.int64)
    cond = -np.ones(nx * ny, np.int64)
    marker[5], cond[20], marker[40], cond[40] = 1, 0, 0, 1
    marks = [(i, i + 1, -1, 1) for i in range(0, 4)]                               # conductor only
    marks += [((ny - 1) * nx + i + 1, (ny - 1) * nx + i, 0, 0) for i in range(3)]  # property 0 and conductor 0
    marks += [(j * nx, (j + 1) * nx, 1, -1) for j in range(3)]                     # BdryFormat 0
    a, b = p[30][0], p[30][1]
    shared = [i for i in range(len(p)) if a in p[i] and b in p[i]]
    assert len(shared) == 2
    marks.append((int(a), int(b), 2, -1))                                          # BdryFormat 2, two elements
    kw = dict(blocks=[dict(ex=1.0), dict(ex=3.0)], labels=[dict(block=0), dict(block=1, is_default=True)],
              lines=[dict(format=1, c0=1.0), dict(format=0, V=2.0), dict(format=2, qs=1e-9)],
              points=[dict(V=1.0), dict(qp=1e-12)], conductors=[dict(type=1, V=5.0), dict(type=0, q=1e-11)],
              length_units=0, depth=1.0)
    return kw, x, y, p, lbl, marker, cond, marks, shared


def _write_branch(base, default=True):
    kw, x, y, p, lbl, marker, cond, marks, shared = _branch_mesh()
    if not default:
        kw = dict(kw, labels=[dict(block=0), dict(block=1)])
    with open(base + ".fee", "w") as fh:
        fh.write(synth.potential_text("e", kw))
    synth.write_potential_mesh(base, x, y, p, lbl, marker=marker, conductor=cond, edge_marks=marks,
                               pbc=[[0, 12, 0], [13, 25, 1]])
    open(base + ".poly", "w").write("\n")
    return kw, shared


@pytest.mark.parametrize("cls,kind", [(psolver.ESolver, "e"), (psolver.HSolver, "h")])
def test_load_mesh_decodes_like_the_reference(tmp_path, cls, kind):
    base = str(tmp_path / "m")
    kw, shared = _write_branch(base)
    if kind == "h":
        os.rename(base + ".fee", base + ".feh")
        txt = open(base + ".feh").read().replace("<ex>", "<Kx>").replace("<ey>", "<Ky>")
        open(base + ".feh", "w").write(txt)
    s = cls(delete_mesh_files=False)
    s.PathName = base
    assert s.LoadProblemFile() and s.LoadMesh(), s.last_error()
    ref = R.load_mesh_ref(base, kw["labels"], [l["format"] for l in kw["lines"]], R.UNITS[kind][0])
    x, y, m, c = s.nodes()
    p, lbl, e = s.elements()
    assert np.array_equal(x, ref["x"]) and np.array_equal(y, ref["y"])
    assert np.array_equal(m, ref["marker"]) and np.array_equal(c, ref["conductor"])
    assert np.array_equal(p, ref["p"]) and np.array_equal(lbl, ref["lbl"]) and np.array_equal(e, ref["e"])
    assert np.array_equal(s.pbcs(), ref["pbc"])
    # the branches are there: the three node kinds, the edge conductor on both
    # ends, the default label, and the BdryFormat 2 edge on the first element only
    assert (m[5], c[5], m[20], c[20], m[40], c[40]) == (1, -1, -1, 0, 0, 1)
    assert c[0] == c[4] == 1 and c[9 * 13] == 0 and (lbl == 1).any()
    assert (e[shared[0]] == 2).sum() == 1 and (e[shared[1]] == 2).sum() == 0
    assert x[1] == 0.5 * R.UNITS[kind][0]
    for ext in (".node", ".ele", ".pbc", ".poly", ".edge"):
        assert os.path.exists(base + ext)


def test_load_mesh_removals(tmp_path):
    base = str(tmp_path / "m")
    _write_branch(base)
    s = psolver.ESolver()      # deleteFiles = true, as runSolver's LoadMesh()
    s.PathName = base
    assert s.LoadProblemFile() and s.LoadMesh(), s.last_error()
    for ext in (".node", ".ele", ".pbc", ".poly"):
        assert not os.path.exists(base + ext), ext
    assert os.path.exists(base + ".edge") and os.path.exists(base + ".fee")
    assert s.Cuthill() and not os.path.exists(base + ".edge")


def test_missing_material_properties(tmp_path, capfd):
    base = str(tmp_path / "m")
    kw, _ = _write_branch(base, default=False)
    with pytest.raises(R.MissingMaterial):
        R.load_mesh_ref(base, kw["labels"], [0, 0, 2], 25.4)
    s = psolver.ESolver()
    s.PathName = base
    assert s.LoadProblemFile() and not s.LoadMesh()
    assert s.last_error() == ("problem loading mesh:\nMaterial properties have not been defined for all regions.\n")
    assert ("Material properties have not been defined for\nall regions. Press the \"Run Mesh Generator\"\n"
            "button to highlight the problem regions.") in capfd.readouterr().err
    for ext in (".node", ".ele", ".pbc", ".poly", ".edge"):
        assert not os.path.exists(base + ext), ext
    assert os.path.exists(base + ".fee")


def test_missing_mesh_files_are_reported(tmp_path):
    (tmp_path / "a.fee").write_text(synth.potential_text("e", dict(blocks=[dict()], labels=[dict(block=0)])))
    s = psolver.ESolver()
    s.PathName = str(tmp_path / "a")
    assert s.LoadProblemFile() and not s.LoadMesh()
    assert ".ele" in s.last_error()      # (the reference reports a missing .node as BADELEMENTFILE)


# ---- the shared renumbering --------------------------------------------------------

def _renumber_both(tmp_path, x, y, p, lbl, n_labels, marker=None, cond=None, marks=(), pbc=None):
    base = str(tmp_path / "r")
    kw = dict(blocks=[dict()], labels=[dict(block=0)] * n_labels, length_units=2)
    fem = synth.fem_text([dict(mu_x=1.0, mu_y=1.0)], [], 1e-8)
    fem += "[NumPoints] = 0\n[NumSegments] = 0\n[NumArcSegments] = 0\n[NumHoles] = 0\n"
    fem += "[NumBlockLabels] = %d\n" % n_labels + "0\t0\t1\t-1\t0\t0\t0\t1\t0\n" * n_labels
    open(base + ".fem", "w").write(fem)
    open(base + ".fee", "w").write(synth.potential_text("e", kw))
    open(base + ".feh", "w").write(synth.potential_text("h", kw))
    synth.write_potential_mesh(base, x, y, p, lbl, marker=marker, conductor=cond, edge_marks=marks, pbc=pbc)
    out = []
    for s in (fsolver.FSolver(delete_mesh_files=False), psolver.ESolver(delete_mesh_files=False),
              psolver.HSolver(delete_mesh_files=False)):
        s.PathName = base
        assert s.LoadProblemFile() and s.LoadMesh() and s.Cuthill(), s.last_error()
        xs, ys = s.nodes()[:2]
        ps, ls, _ = s.elements()
        out.append((xs, ys, ps, ls, s.BandWidth, s.pbcs()))
    return out


def _assert_same_order(out):
    f, e, h = out
    # (the three scale the same file coordinates by their own unit: compare the order through exact ratios)
    for o, unit in ((e, 10.0), (h, 0.01)):
        assert np.array_equal(o[0], f[0] * unit) and np.array_equal(o[1], f[1] * unit)
        assert np.array_equal(o[2], f[2]) and np.array_equal(o[3], f[3])
        assert o[4] == f[4] and np.array_equal(o[5], f[5])


def test_renumbering_equals_fsolvers_on_the_small_mesh(tmp_path):
    kw, x, y, p, lbl, marker, cond, marks, _ = _branch_mesh()
    _assert_same_order(_renumber_both(tmp_path, np.round(x * 4), np.round(y * 4), p, np.maximum(lbl, 0), 2, marker,
                                      cond, marks, pbc=[[0, 12, 0], [13, 25, 1]]))


def test_renumbering_equals_fsolvers_on_a_large_scrambled_mesh(tmp_path):
    """80k elements, scrambled node and element numbering: large enough for
    the parallel comb-sort passes and neighbour ordering (FSolver's own order
    on such a mesh is pinned to the reference's cuthill.cpp)."""
    kw = synth.magnetostatic(200)
    rng = np.random.default_rng(11)
    nn, ne = len(kw["x"]), len(kw["p"])
    perm = rng.permutation(nn)
    inv = np.argsort(perm)
    eperm = rng.permutation(ne)
    # integer coordinates: the three unit conversions are exact
    x, y = np.round(kw["x"][inv] * 20), np.round(kw["y"][inv] * 20)
    out = _renumber_both(tmp_path, x, y, perm[kw["p"]][eperm].astype(np.int32), kw["lbl"][eperm],
                         int(kw["lbl"].max()) + 1, pbc=[[int(perm[0]), int(perm[200]), 0]])
    assert len(out[0][2]) >= 80000
    _assert_same_order(out)


# ---- the time step ---------------------------------------------------------------

def _heat_case(tmp_path, **extra):
    x, y, p = electro.grid(4, 3, 0.03, 0.02)
    kw = dict(x=x, y=y, p=p, lbl=np.zeros(len(p), np.int32), blocks=[dict(kx=1.0, ky=1.0, kt=2.0)],
              labels=[dict(block=0)], length_units=3, depth=1.0, **extra)
    base = str(tmp_path / "h")
    R.write_case("h", base, kw)
    s = psolver.HSolver(delete_mesh_files=False)
    s.PathName = base
    assert s.LoadProblemFile(), s.last_error()
    return s, base


def test_previous_solution_file_with_a_time_step_is_refused(tmp_path, capfd):
    s, base = _heat_case(tmp_path, dt=10.0, prev_soln="earlier.anh")
    assert s.header()["dt"] == 10.0 and s.previousSolutionFile == "earlier.anh"
    assert not s.runSolver()
    assert "[PrevSoln] = \"earlier.anh\"" in s.last_error() and "refused" in s.last_error()
    assert "earlier.anh" in capfd.readouterr().err
    assert not os.path.exists(base + ".anh")
    # temperatures of the wrong length are refused too, before any device work
    assert s.set_previous_solution(np.zeros(5))
    assert not s.runSolver() and "5 values" in s.last_error()


def test_time_step_without_a_previous_solution_is_reset(tmp_path, capfd):
    s, base = _heat_case(tmp_path, dt=10.0)
    s.runSolver()      # (goes on to the device solve: its outcome is the GPU tests' matter)
    assert "Warning: no previous solution set even though dT is non-zero. Resetting dT...\n" in capfd.readouterr().err
    assert s.header()["dt"] == 0.0
