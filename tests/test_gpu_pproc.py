"""The file-based post-processors on the device (bin/epproc, bin/hpproc,
pproc.EPProc / HPProc over include/xfemm_pproc.h): the reference's recorded
output, the same bits as a problem built in memory from the Python readers'
arrays, files written by ESolver / HSolver read back, the plot bounds against
a numpy restatement, multiply-defined labels, the refusal to solve an opened
file, and edge shapes."""
import os
import re
import subprocess

import numpy as np
import pytest

import electro
import heat
import pprocref
import test_gpu_psolver as tgp
from test_postproc_cpu import load
from test_pproc_cpu import GOLD, RES, ROOT, unpack
from xfemm_amd import kernels, pproc

pytestmark = pytest.mark.gpu

BIN = os.path.join(ROOT, "xfemm_amd", "bin")
TOL = 5.1e-7   # the bound tests/test_postproc_cpu.py holds the recorded %f output to
XFK_ERR_UNSUPPORTED = -5
NUM = re.compile(r"^[-+]?(\d+\.?\d*|\.\d+)([eE][-+]?\d+)?,?$")


def fixture(name, tmp_path):
    """(path, post-processor class, Python reader's result, problem class)"""
    if name == "test":
        return RES, pproc.EPProc, electro.read_res(RES), kernels.ElectrostaticProblem
    path = unpack(name, tmp_path)
    return path, pproc.HPProc, heat.read_anh(path), kernels.HeatFlowProblem


def memory_twin(cls, r, Q=None):
    """The problem as tests/test_gpu_postproc.py builds it from a reader's arrays."""
    kw = dict(r["kw"])
    if kw.get("dt", 0) != 0 and kw.get("t_prev") is None:
        kw["t_prev"] = np.zeros(len(kw["x"]))
    M = cls(**kw)
    if Q is not None:
        M.set_qmarks(Q)
    M.set_solution(r["V"])
    return M


# --- the recorded output --------------------------------------------------------

@pytest.mark.parametrize("name,prog,check", [("test", "epproc", "epproc/test.out.check"),
                                             ("Temp0", "hpproc", "hpproc/Temp0.out.check"),
                                             ("Temp1", "hpproc", "hpproc/Temp1.out.check")])
def test_program_prints_the_recorded_output(name, prog, check, tmp_path):
    """Line count, every word, and every number within 5.1e-7.  Two lines
    need the reference's own ways: the cross-section area of the heat-flow
    fixtures is 3.375e-4 m^2, a tie of "%f" that only the element-by-element
    sum leaves on the recorded side (0.000337), and the recorded 'smoothing
    on' line at the mesh node (0.01, 0.01), which five elements of two
    materials share, was taken in the element the reference's walk reaches
    from the point looked up before, not in the lowest-numbered one."""
    path = fixture(name, tmp_path)[0]
    r = subprocess.run([os.path.join(BIN, prog), path], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    got = r.stdout.splitlines()
    want = open(os.path.join(GOLD, check)).read().splitlines()
    assert len(got) == len(want), r.stdout
    worst = 0.0
    for g, w in zip(got, want):
        gt, wt = g.split(), w.split()
        assert len(gt) == len(wt), (g, w)
        for a, b in zip(gt, wt):
            if NUM.match(b):
                err = abs(float(a.rstrip(",")) - float(b.rstrip(",")))
                worst = max(worst, err)
                print("%-28s got %s recorded %s err %.3g" % (" ".join(wt[:2]), a, b, err))
                assert err <= TOL, (g, w)
            else:
                assert a == b, (g, w)
    print(name, "worst", worst)


def test_program_exit_status_on_a_bad_file(tmp_path):
    bad = tmp_path / "bad.res"
    bad.write_text("[Format] = 1\n")
    for prog in ("epproc", "hpproc"):
        r = subprocess.run([os.path.join(BIN, prog), str(bad)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 1 and "Solution" in r.stderr


# --- the same bits as the in-memory path ---------------------------------------

def compare_all(P, M, es, xs, ys, contour):
    a, b = P.element_fields(), M.element_fields()
    assert all(np.array_equal(a[k], b[k]) for k in a)
    assert np.array_equal(P.corner_fields(), M.corner_fields())
    assert np.array_equal(P.block_integrals([0])["raw"], M.block_integrals([0])["raw"])
    for smooth in (False, True):
        a, b = P.point_values(xs, ys, smooth=smooth), M.point_values(xs, ys, smooth=smooth)
        assert np.array_equal(a["elem"], b["elem"]) and np.array_equal(a["raw"], b["raw"], equal_nan=True)
        for k in (0, len(xs) // 2, len(xs) - 1):   # and one at a time
            one = P.point_values([xs[k]], [ys[k]], smooth=smooth)
            assert np.array_equal(one["raw"][0], a["raw"][k], equal_nan=True)
    for kind in range(5 if es else 4):
        assert np.array_equal(P.line_integrals([contour], kind)["raw"], M.line_integrals([contour], kind)["raw"],
                              equal_nan=True), kind
    assert np.array_equal(P.plot_bounds(), M.plot_bounds())


@pytest.mark.parametrize("name", ["test", "Temp0", "Temp1"])
def test_opened_file_equals_memory_problem(name, tmp_path):
    path, cls, r, pcls = fixture(name, tmp_path)
    F = cls()
    assert F.open(path), F.last_error()
    assert not F.has_multiply_defined_labels() and not F.selection().any()
    P, M = F.problem(), memory_twin(pcls, r)
    assert np.array_equal(P.qmarks(), r["Q"]) and np.array_equal(M.qmarks(), r["Q"])
    x, y, _, _ = F.nodes()
    gx, gy = np.meshgrid(np.linspace(x.min(), x.max(), 7), np.linspace(y.min(), y.max(), 7))
    contour = [(x.min() * 0.8 + x.max() * 0.2, y.min() * 0.7 + y.max() * 0.3),
               (x.min() * 0.3 + x.max() * 0.7, y.min() * 0.4 + y.max() * 0.6)]
    compare_all(P, M, name == "test", gx.ravel(), gy.ravel(), contour)
    # the post-processor's own calls are the problem's
    F.toggle_label(0)
    # ... its block integrals in the reference's order of summation: the area
    # and the volume (plain products of the coordinates) have the bits of the
    # literal restatement's element-by-element sums, all seven lie within the
    # bound tests/test_gpu_postproc.py holds the tree sums to
    o = M.block_integrals_ordered([0])
    for kind in range(5):
        want = complex(o[kind], 0.) if kind < 3 else complex(o[3 + 2 * (kind - 3)], o[4 + 2 * (kind - 3)])
        assert F.block_integral(kind) == want
    R = load(name)[0]
    want, scale = R.block_integrals([0])
    assert o[1] == want[1] and o[2] == want[2]
    vol = want[2]
    div = np.array([vol if R.heat else 1., 1., 1., vol, vol, vol, vol])
    for k in range(7):
        assert abs(o[k] - want[k]) <= 1e-12 * scale[k] / abs(div[k]), k
    # ... and its single points are located by the reference's walk: here from
    # the element of the last label, then from each point's to the next
    W = pprocref.Walk(R.X, R.Y, R.p)
    for lb in F.labels():
        W.find(lb["x"], lb["y"])
    shared = [(0.25, 0.0), (0.1, 0.8)] if name == "test" else [(0.01, 0.01), (0.005, 0.005), (0.01, 0.01)]
    for smooth in (False, True):
        F.set_smoothing(smooth)
        for px, py in shared:
            e = W.find(px, py)
            assert e in R.containing(px, py)
            assert np.array_equal(F.point_values(px, py), M.point_values_at([px], [py], [e], smooth=smooth)[0])
            assert np.array_equal(M.point_values_at([px], [py], [R.containing(px, py)[0]], smooth=smooth),
                                  M.point_values([px], [py], smooth=smooth)["raw"])
    F.set_smoothing(False)
    b = F.point_values_batch(gx.ravel(), gy.ravel())
    assert np.array_equal(b["raw"], M.point_values(gx.ravel(), gy.ravel(), smooth=False)["raw"], equal_nan=True)
    for px, py in contour:
        F.add_contour_point(px, py)
    F.set_smoothing(True)
    assert F.line_integral(1) == M.line_integral(contour, 1)
    if name == "test":
        a, b = P.make_mask([0]), M.make_mask([0])
        for kind in (5, 6):
            assert P.block_integral([0], kind) == M.block_integral([0], kind)
        Vc, qc = P.conductors()
        Vm, qm = M.conductors()
        assert np.array_equal(Vc, Vm) and np.array_equal(qc, qm)
    M.close()
    F.close()


# --- files written by the solvers, read back ------------------------------------

@pytest.mark.parametrize("make", [tgp._planar_electro, tgp._axi_electro, tgp._nonlinear_heat],
                         ids=["planar-periodic-point", "axi-floating", "heat-nonlinear"])
def test_round_trip_through_the_solver(make, tmp_path):
    kind, kw = make()
    base = str(tmp_path / "c")
    tgp.R.write_case(kind, base, kw)
    s = tgp._solver(kind, base)
    assert s.runSolver(), s.last_error()
    out = base + tgp.R.EXT[kind][1]
    cls, pcls, reader = ((pproc.EPProc, kernels.ElectrostaticProblem, electro.read_res) if kind == "e" else
                         (pproc.HPProc, kernels.HeatFlowProblem, heat.read_anh))
    F = cls()
    assert F.open(out), F.last_error()
    r = reader(out)
    if kind == "h":
        r["kw"]["e"] = None   # (heat.read_anh's edge recovery is for its fixtures)
    x, y, V, Q = F.nodes()
    assert np.array_equal(V, r["V"]) and np.array_equal(Q, r["Q"])
    # the marks come with the file: the reader's arrays carry no edges to derive them from
    M = memory_twin(pcls, r, Q=r["Q"])
    P = F.problem()
    assert np.array_equal(P.qmarks(), r["Q"])
    xs = np.linspace(x.min(), x.max(), 7).repeat(7)
    ys = np.tile(np.linspace(y.min(), y.max(), 7), 7)
    contour = [(x.min() * 0.75 + x.max() * 0.25, y.min() * 0.8 + y.max() * 0.2),
               (x.min() * 0.2 + x.max() * 0.8, y.min() * 0.3 + y.max() * 0.7)]
    compare_all(P, M, kind == "e", xs, ys, contour)
    Vc, qc = F.conductors()
    Vs, qs = s.conductors()
    assert np.array_equal(Vc, Vs) and np.array_equal(qc, qs)
    M.close()
    F.close()


# --- plot bounds -------------------------------------------------------------------

def bounds_block():
    src = open(os.path.join(ROOT, "xfemm_amd", "csrc", "xfk_postproc.hip")).read()
    return int(re.search(r"constexpr int kPpBoundsBlock = (\d+);", src).group(1))


def strip(ne, externals, big_first):
    """ne triangles in a strip; label 1 is external."""
    n = ne + 2
    x = np.concatenate([np.arange((n + 1) // 2), np.arange(n // 2) + 0.5]).astype(float)
    y = np.concatenate([np.zeros((n + 1) // 2), np.ones(n // 2)])
    order = np.empty(n, int)
    order[0::2], order[1::2] = np.arange((n + 1) // 2), (n + 1) // 2 + np.arange(n // 2)
    p = np.array([[order[k], order[k + 1], order[k + 2]] if k % 2 == 1 else [order[k + 1], order[k], order[k + 2]]
                  for k in range(ne)], np.int32)
    lbl = np.zeros(ne, np.int32)
    lbl[list(externals)] = 1
    V = np.sin(0.37 * x) + 0.5 * y * np.cos(0.11 * x)
    if big_first:
        V[order[0]] += 100.   # (the strip's first node belongs to element 0 alone)
    kw = dict(x=x + 1.0, y=y, p=p, lbl=lbl, blocks=[dict(ex=2.0, ey=3.0, qv=0.0)],
              labels=[dict(block=0), dict(block=0, is_external=1)], length_units=1, problem_type=1, ext_ro=3.0,
              ext_ri=2.0, ext_zo=0.5)
    return kw, V


@pytest.mark.parametrize("which", ["none-external", "all-but-last-external", "first-external-largest"])
def test_plot_bounds(which):
    c = bounds_block()
    for ne in (1, c - 1, c, c + 1, 2 * c + 3):
        ext = {"none-external": [], "all-but-last-external": range(ne - 1), "first-external-largest": [0]}[which]
        kw, V = strip(ne, ext, which == "first-external-largest")
        P = kernels.ElectrostaticProblem(**kw)
        P.set_solution(V)
        f = P.element_fields()
        want = pprocref.plot_bounds(V, f["D"], f["E"], kw["lbl"] == 1)
        got = P.plot_bounds()
        print(which, ne, got.ravel(), want.ravel())
        assert np.array_equal(got, want)
        assert np.array_equal(P.plot_bounds(), got)
        if which == "first-external-largest" and ne > 1:
            e = pprocref.cabs(f["E"][:, 0], f["E"][:, 1])
            assert got[2, 1] == e[0] > e[1:].max()   # the reference's starting value shows
        P.close()


# --- multiply-defined labels, refusals, edge shapes ------------------------------------

def square_file(tmp_path, label_xy, nlabels=2, cond=(), Q=None, grid=(3, 3), geom=None):
    x, y, p = electro.grid(grid[0], grid[1], 1.0, 1.0)
    kw = dict(x=x, y=y, p=p, lbl=np.zeros(len(p), np.int32), blocks=[dict(ex=1.0, ey=1.0, qv=0.0)],
              labels=[dict(block=0)] * nlabels, length_units=1, depth=1.0)
    path = tmp_path / "square.res"
    path.write_text(pprocref.solution_text("e", kw, 3.0 * x + y, Q=Q, cond=cond, geom=geom, label_xy=label_xy))
    return str(path), kw


def test_two_labels_in_one_region_are_flagged(tmp_path):
    path, _ = square_file(tmp_path, [(0.3, 0.3), (0.7, 0.6)])
    F = pproc.EPProc()
    assert F.open(path), F.last_error()
    assert F.has_multiply_defined_labels()
    assert F.selection().tolist() == [1, 0]   # the element's label, not the stray one
    F.close()


def test_opened_problem_refuses_to_solve(tmp_path):
    L = kernels.load_library()
    path, kw = square_file(tmp_path, [(0.3, 0.3)], nlabels=1)
    F = pproc.EPProc()
    assert F.open(path), F.last_error()
    r = kernels.Result()
    import ctypes as C
    assert L.xfk_electrostatic(F.problem()._h, 0, C.byref(r)) == XFK_ERR_UNSUPPORTED
    assert b"solution file" in L.xfk_last_error()
    hp, _, _, _ = fixture("Temp0", tmp_path)
    H = pproc.HPProc()
    assert H.open(hp), H.last_error()
    assert L.xfk_heatflow(H.problem()._h, 0, C.byref(r)) == XFK_ERR_UNSUPPORTED
    assert L.xfk_heatflow_assemble(H.problem()._h, None) == XFK_ERR_UNSUPPORTED
    assert b"solution file" in L.xfk_last_error()
    # a fresh in-memory problem still solves
    x, y, p = electro.grid(9, 9, 1.0, 1.0)
    e = electro.tag_edges(x, y, p, [(lambda xa, ya, xb, yb: xa == 0 and xb == 0, 0),
                                    (lambda xa, ya, xb, yb: xa == 1 and xb == 1, 1)])
    Q = kernels.ElectrostaticProblem(x=x * 10, y=y * 10, p=p, lbl=np.zeros(len(p), np.int32), e=e,
                                     blocks=[dict(ex=1.0, ey=1.0, qv=0.0)], labels=[dict(block=0)],
                                     lines=[dict(format=0, V=0.0), dict(format=0, V=10.0)], length_units=2, depth=1.0)
    Q.solve()
    assert np.allclose(Q.element_fields()["E"][:, 0], -10.0 / 0.01, rtol=1e-6)   # as tests/test_gpu_postproc.py
    Q.close()
    F.close()
    H.close()


def test_single_triangle_without_conductors(tmp_path):
    kw = dict(x=np.array([0., 1., 0.]), y=np.array([0., 0., 1.]), p=np.array([[0, 1, 2]], np.int32),
              lbl=np.zeros(1, np.int32), blocks=[dict(ex=2.0, ey=2.0, qv=0.0)], labels=[dict(block=0)],
              length_units=1, depth=1.0)
    path = tmp_path / "one.res"
    path.write_text(pprocref.solution_text("e", kw, np.array([1., 3., 2.]), label_xy=[(0.2, 0.2)]))
    F = pproc.EPProc()
    assert F.open(str(path)), F.last_error()
    assert len(F.conductors()[0]) == 0 and not F.has_multiply_defined_labels()
    F.toggle_label(0)
    assert abs(F.block_integral(1).real - 0.5e-6) <= 1e-18   # half a square millimetre
    v = F.point_values(0.25, 0.25)
    assert v is not None and abs(v[0] - 1.75) <= 1e-14
    assert F.point_values(2.0, 2.0) is None
    b = F.plot_bounds()
    assert b[0].tolist() == [1., 3.] and b[1, 0] == b[1, 1] and b[2, 0] == b[2, 1]
    F.close()


def test_contour_from_node_along_an_arc_integrates_as_by_coordinates(tmp_path):
    """The plate-capacitor fixture's own geometry: a contour built from its
    input points along an arc segment gives what the same points give when
    passed by coordinates."""
    F = pproc.EPProc()
    assert F.open(RES), F.last_error()
    g = F.geometry()
    a = g["arcs"][0]
    for k in a:
        F.add_contour_point_from_node(*g["points"][k])
    pts = F.contour()
    assert len(pts) == 1 + int(np.ceil(g["arc_length"][0] / g["arc_maxside"][0])) > 2
    got = np.array([F.line_integral(kind) for kind in range(5)])
    F.clear_contour()
    for px, py in pts:
        F.add_contour_point(px, py)
    assert np.array_equal(np.array([F.line_integral(kind) for kind in range(5)]), got, equal_nan=True)
    P = F.problem()
    assert np.array_equal(np.array([P.line_integral(kernels.Contour(pts), kind) for kind in range(5)]), got,
                          equal_nan=True)
    print("along the arc:", got)
    assert np.isfinite(got[2].real) and got[2].real > 0   # (the arc bounds a conductor: its length, at least)
    F.close()
