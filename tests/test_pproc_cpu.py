"""The host side of the file-based post-processors (xfemm_amd/csrc/fsolver/
pproc.cpp through include/xfemm_pproc.h): the .res / .anh reader against the
Python readers of the tests bit for bit, its refusals of bad files, a
sanitizer run of the reader as a stand-alone program, and
addContourPointFromNode against the restatement of tests/pprocref.py.  No GPU."""
import gzip
import os
import shutil
import subprocess

import numpy as np
import pytest

import electro
import heat
import pprocref
from xfemm_amd import kernels, pproc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
RES = os.path.join(GOLD, "esolver", "test.res.check")


def unpack(name, tmp_path):
    dst = str(tmp_path / (name + ".anh"))
    with gzip.open(os.path.join(GOLD, "hpproc", name + ".anh.gz"), "rb") as f, open(dst, "wb") as o:
        shutil.copyfileobj(f, o)
    return dst


def section_count(text, token):
    for ln in text.splitlines():
        if ln.startswith(token):
            return int(ln.split("=")[1])
    raise AssertionError(token)


@pytest.mark.parametrize("name", ["test", "Temp0", "Temp1"])
def test_reader_equals_python_reader(name, tmp_path):
    if name == "test":
        path, cls, r, units = RES, pproc.EPProc, electro.read_res(RES), electro.UNITS
    else:
        path = unpack(name, tmp_path)
        cls, r, units = pproc.HPProc, heat.read_anh(path), heat.UNITS
    P = cls()
    assert P.read(path), P.last_error()
    kw = r["kw"]
    x, y, V, Q = P.nodes()
    p, lbl = P.elements()
    u = units[kw["length_units"]]
    # the Python readers keep x * unit; the file's own x gives the same bits when multiplied the same way
    assert np.array_equal(x * u, kw["x"]) and np.array_equal(y * u, kw["y"])
    assert np.array_equal(V, r["V"]) and np.array_equal(Q, r["Q"])
    assert np.array_equal(p, kw["p"]) and np.array_equal(lbl, kw["lbl"])
    Vc, qc = P.conductors()
    cl = np.asarray(r.get("conductors", np.zeros((0, 2)))).reshape(-1, 2)
    assert np.array_equal(Vc, cl[:, 0]) and np.array_equal(qc, cl[:, 1])
    h = P.header()
    assert h["precision"] == kw["precision"] and h["length_units"] == kw["length_units"]
    assert h["problem_type"] == kw["problem_type"] and h["depth"] == kw["depth"]
    assert (h["ext_zo"], h["ext_ro"], h["ext_ri"]) == (kw["ext_zo"], kw["ext_ro"], kw["ext_ri"])
    assert h["n_block_props"] == len(kw["blocks"]) and h["n_line_props"] == len(kw["lines"])
    assert h["n_node_props"] == len(kw["points"]) and h["n_block_labels"] == len(kw["labels"])
    key = ("ex", "ey") if name == "test" else ("kx", "ky")
    for b, want in zip(P.blocks(), kw["blocks"]):
        assert (b["kx"], b["ky"], b["qv"]) == (want[key[0]], want[key[1]], want["qv"])
    text = open(path).read()
    head = text[:text.index("[Solution]")].splitlines()
    k = [i for i, l in enumerate(head) if l.startswith("[NumBlockLabels]")][0]
    for j, lb in enumerate(P.labels()):
        f = head[k + 1 + j].split()
        assert (lb["x"], lb["y"], lb["block"]) == (float(f[0]), float(f[1]), int(f[2]) - 1)
        assert lb["block"] == kw["labels"][j]["block"] and lb["is_external"] == kw["labels"][j]["is_external"]
    g = P.geometry()
    assert len(g["points"]) == section_count(text, "[NumPoints]")
    assert len(g["segments"]) == section_count(text, "[NumSegments]")
    assert len(g["arcs"]) == section_count(text, "[NumArcSegments]")
    assert g["n_holes"] == section_count(text, "[NumHoles]")
    P.close()


def bad_files():
    lines = open(RES).read().splitlines()
    sol = lines.index("[Solution]")
    n = int(lines[sol + 1])
    ne = int(lines[sol + 2 + n])
    nlab = 1
    first_el = sol + 3 + n

    def join(ls):
        return "\n".join(ls) + "\n"

    def with_line(k, new):
        return join(lines[:k] + [new] + lines[k + 1:])

    el = lines[first_el + 5].split()
    text = join(lines)
    cut = text.index(lines[sol + 2 + n // 2]) + len(lines[sol + 2 + n // 2]) // 2
    return ne, {
        "no-solution": (join(lines[:sol]), "[Solution]"),
        "node-count-plus-one": (with_line(sol + 1, str(n + 1)), "node"),
        "node-index-N": (with_line(first_el + 5, "\t".join([el[0], str(n), el[2], el[3]])), "node index"),
        "label-equal-nlabels": (with_line(first_el + 5, "\t".join(el[:3] + [str(nlab)])), "label"),
        "cut-in-a-node-line": (text[:cut], "truncated"),
        "empty": ("", "empty"),
    }


@pytest.mark.parametrize("case", ["no-solution", "node-count-plus-one", "node-index-N", "label-equal-nlabels",
                                  "cut-in-a-node-line", "empty"])
def test_bad_file_is_refused_with_a_message(case, tmp_path):
    ne, cases = bad_files()
    text, word = cases[case]
    bad = tmp_path / "bad.res"
    bad.write_text(text)
    P = pproc.EPProc()
    assert not P.read(str(bad))
    print(case, "->", P.last_error())
    assert word in P.last_error()
    assert P.NumNodes == 0 and P.NumEls == 0
    # the next good file still opens
    assert P.read(RES), P.last_error()
    assert P.NumEls == ne
    P.close()


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_reader_under_sanitizers(tmp_path):
    """The reader as a stand-alone program under AddressSanitizer and
    UndefinedBehaviorSanitizer: the three fixtures, each also cut at 64 evenly
    spaced byte offsets."""
    exe = str(tmp_path / "pproc_read_check")
    src = os.path.join(ROOT, "xfemm_amd", "csrc", "fsolver")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-pthread", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                    os.path.join(ROOT, "tests", "native", "pproc_read_check.cpp"), os.path.join(src, "pproc.cpp"),
                    os.path.join(src, "femm_problem.cpp")], check=True)
    r = subprocess.run([exe, str(tmp_path / "cut.tmp"), "e:" + RES, "h:" + unpack("Temp0", tmp_path),
                        "h:" + unpack("Temp1", tmp_path)], capture_output=True, text=True, timeout=300)
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0
    assert "all clean" in r.stdout and r.stdout.count("64 refused") == 3


# --- addContourPointFromNode ---------------------------------------------------

# a straight segment 0-1, a 90 degree arc 1-2 and a 180 degree arc 2-3
GEOM = pprocref.geometry(points=[(0., 0.), (2., 0.), (2., 2.), (-1.5, 2.), (7., 7.)],
                         segments=[(0, 1)], arcs=[(1, 2, 90., 7.), (2, 3, 180., 11.)])


def arc_file(tmp_path):
    x, y, p = electro.grid(3, 3, 1.0, 1.0)
    kw = dict(x=x, y=y, p=p, lbl=np.zeros(len(p), np.int32), blocks=[dict(ex=1.0, ey=1.0, qv=0.0)],
              labels=[dict(block=0)], length_units=1, depth=1.0)
    path = tmp_path / "arcs.res"
    path.write_text(pprocref.solution_text("e", kw, np.zeros(len(x)), geom=GEOM, label_xy=[(0.4, 0.3)]))
    return str(path)


@pytest.mark.parametrize("walk", [[0, 1], [1, 0], [1, 2], [2, 1], [2, 3], [3, 2], [0, 1, 2, 3], [3, 2, 1, 0], [0, 4, 2]])
def test_contour_from_node(walk, tmp_path):
    P = pproc.EPProc()
    assert P.read(arc_file(tmp_path)), P.last_error()
    g = P.geometry()
    assert np.array_equal(g["points"], GEOM["points"]) and np.array_equal(g["arcs"], GEOM["arcs"])
    assert np.array_equal(g["arc_length"], GEOM["arc_length"]) and np.array_equal(g["arc_maxside"], GEOM["arc_maxside"])
    want, C = [], kernels.Contour()
    for k in walk:
        # (a click near the point, not on it)
        mx, my = GEOM["points"][k] + np.array([0.01, -0.02])
        P.add_contour_point_from_node(mx, my)
        C.add_point_from_node(g, mx, my)
        pprocref.add_from_node(GEOM, want, mx, my)
    got = P.contour()
    got = got[:, 0] + 1j * got[:, 1]
    want = np.array(want)
    print(walk, len(got), "points")
    assert len(got) == len(want) == len(C)
    assert np.abs(got - want).max() <= 1e-12 * 4 and np.abs(np.array([complex(*q) for q in C.points]) - want).max() <= 4e-12
    # the walk's ends are the input points themselves
    hit = [np.flatnonzero(got == complex(*GEOM["points"][k])) for k in walk]
    assert all(len(h) >= 1 for h in hit)
    assert got[0] == complex(*GEOM["points"][walk[0]]) and got[-1] == complex(*GEOM["points"][walk[-1]])
    # every point between two ends of an arc lies on its circle
    for a, b in zip(walk[:-1], walk[1:]):
        for k, (n0, n1) in enumerate(GEOM["arcs"]):
            if {a, b} == {int(n0), int(n1)}:
                c, R = pprocref.circle(GEOM, k)
                i0, i1 = sorted((int(np.flatnonzero(got == complex(*GEOM["points"][a]))[0]),
                                 int(np.flatnonzero(got == complex(*GEOM["points"][b]))[0])))
                n = int(np.ceil(GEOM["arc_length"][k] / GEOM["arc_maxside"][k]))
                assert i1 - i0 == n
                assert np.abs(np.abs(got[i0:i1 + 1] - c) - R).max() <= 1e-12 * R
    P.close()


def test_selection_and_closest_label(tmp_path):
    P = pproc.EPProc()
    assert P.read(RES)
    assert P.selection().tolist() == [0]
    assert P.select_block_label(5.0, 5.0) and P.selection().tolist() == [1]
    assert P.toggle_group(3) and P.selection().tolist() == [0]
    assert not P.toggle_label(1)
    P.toggle_label(0)
    P.clear_selection()
    assert P.selection().tolist() == [0]
    P.close()
