"""Post-processing of potential problems on the device (xfk_postproc.hip)
against the literal restatement of the reference's epproc / hpproc
(tests/postproc.py) and against the reference's recorded output.

Solutions are loaded with set_solution, so no solver tolerance enters.  Bounds:
1e-12 of the largest magnitude of the quantity (the bound the project holds
assembled systems to: a few dozen roundings of ~1.1e-16 each, the only
differences being library atan2 / pow and the order of the integrals' sums);
for the integrals 1e-12 of the sum of the absolute terms; 5.1e-7 absolute
against the %f-printed recorded numbers; element indices exactly."""

import numpy as np
import pytest

import electro
import postproc
from test_postproc_cpu import check_integrals, check_points, load
from util import precision_bound, rel_err, synth_to_oracle
from xfemm_amd import kernels, synth

pytestmark = pytest.mark.gpu

TOL = 1e-12
XFK_ERR_ARG = -1   # include/xfemm_kernels.h


def close(got, want, what):
    got, want = np.asarray(got, float), np.asarray(want, float)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(np.isnan(got), np.isnan(want)), what
    scale = np.nanmax(np.abs(want)) if np.isfinite(want).any() else 0.0
    err = np.nanmax(np.abs(got - want)) if np.isfinite(want).any() else 0.0
    print("%s: err %.3e of max %.3e" % (what, err, scale))
    assert err <= TOL * scale, (what, err, scale)


def device(R, cls=None):
    """The device problem of restatement R with R's solution loaded."""
    cls = cls or (kernels.HeatFlowProblem if R.heat else kernels.ElectrostaticProblem)
    kw = dict(R.kw)
    if kw.get("dt", 0) != 0 and kw.get("t_prev") is None:
        kw["t_prev"] = np.zeros(R.N)   # (a time step's previous solution: the post-processor does not read it)
    P = cls(**kw)
    P.set_solution(R.V)
    return P


def compare_fields(P, R):
    f = P.element_fields()
    D, E = (f["F"], f["G"]) if R.heat else (f["D"], f["E"])
    close(D, R.D, "element D")
    close(E, R.E, "element E")
    close(P.corner_fields(), R.d, "corner d")
    assert np.array_equal(P.corner_branches(), np.array(R.branch, np.uint8))


def compare_integrals(P, R, sel):
    got = P.block_integrals(sel)["raw"]
    want, scale = R.block_integrals(sel)
    vol = want[2]
    # the averaged types are divided by the volume after the sum
    div = np.array([vol if R.heat else 1., 1., 1., vol, vol, vol, vol])
    for k in range(7):
        print("integral %d: got %.15g want %.15g (sum |terms| %.3e)" % (k, got[k], want[k], scale[k]))
        assert abs(got[k] - want[k]) <= TOL * scale[k] / abs(div[k]), k
    return got


def compare_points(P, R, xs, ys):
    for smooth in (False, True):
        r = P.point_values(xs, ys, smooth=smooth)
        el, out = R.points(xs, ys, smooth)
        assert np.array_equal(r["elem"], el), (smooth, r["elem"], el)
        for c in range(8):
            close(r["raw"][:, c], out[:, c], "point value %d smooth %d" % (c, smooth))
    return r


# --- the three fixtures -------------------------------------------------------

@pytest.mark.parametrize("name", ["test", "Temp0", "Temp1"])
def test_fixture(name):
    R, chk, _ = load(name)
    P = device(R)
    compare_fields(P, R)
    got = compare_integrals(P, R, [0])
    check_integrals(R, chk, got)
    pts = sorted({(x, y) for s in (False, True) for x, y, _ in chk["points"][s]})
    xs, ys = np.array([q[0] for q in pts]), np.array([q[1] for q in pts])
    compare_points(P, R, xs, ys)

    # the recorded lines directly: the device's element, or for the node shared
    # by several elements one of the containing ones (the reference's search is
    # stateful; the device's value there is the lowest-numbered element's)
    def values_at(x, y, smooth):
        r = P.point_values([x], [y], smooth=smooth)
        hits = R.containing(x, y)
        assert r["elem"][0] == hits[0]
        cands = {int(r["elem"][0]): r["raw"][0]}
        for k in hits[1:]:
            cands[k] = R.point_values(x, y, k, smooth)
        return cands

    check_points(R, chk, values_at)
    P.close()


def test_loaded_solution_conductors():
    """set_solution integrates the conductors' charges from the loaded V, as a solve does."""
    R, _, r = load("test")
    P = device(R)
    Vc, q = P.conductors()
    for c in range(2):
        want = electro.charge(r["kw"], r["V"], c)
        print("conductor %d: q %.12e, restated %.12e" % (c, q[c], want))
        assert abs(q[c] - want) <= 1e-10 * abs(want)
    P.close()


def test_end_to_end_solve_then_postprocess():
    """The electrostatic fixture solved by xfk_electrostatic itself, then
    post-processed: the stored energy and the average E over label 0 against
    the restatement on the recorded V, within the bound
    tests/test_gpu_electro.py holds the solved potential to against the
    recorded one -- util.precision_bound(recorded V, direct solve, 1e-6) --
    relative to the energy, and to the larger component of the average E."""
    R, _, r = load("test")
    Vdirect = electro.restate(r["kw"])["V"][:R.N]
    bound = precision_bound(r["V"], Vdirect, 1e-6)
    P = kernels.ElectrostaticProblem(**r["kw"])
    P.solve()
    print("solved V vs recorded: %.3e (bound %.3e)" % (rel_err(P.solution(), r["V"]), bound))
    got = P.block_integrals([0])
    want, _ = R.block_integrals([0])
    e_nrg = abs(got["energy"] - want[0]) / abs(want[0])
    e_E = rel_err(got["E"], want[5:7])
    print("stored energy %.12e vs %.12e: %.3e; average E %s vs %s: %.3e"
          % (got["energy"], want[0], e_nrg, got["E"], want[5:7], e_E))
    assert e_nrg <= bound and e_E <= bound
    P.close()


# --- small synthetic meshes: every branch of the smoothing -----------------------

@pytest.mark.parametrize("nx,ny,axi,physics", postproc.SYNTH)
def test_synthetic(nx, ny, axi, physics):
    kw, V = postproc.synthetic(nx, ny, axi, physics)
    R = postproc.Post(kw, V, physics)
    P = device(R)
    compare_fields(P, R)
    compare_integrals(P, R, [0, 2])
    compare_integrals(P, R, [1])
    # points: inside, on interior edges, on nodes, on the grid's cell
    # boundaries, on the mesh boundary, outside
    X, Y = np.array(R.X), np.array(R.Y)
    p = np.array(R.p)
    W, H = X.max() - X.min(), Y.max() - Y.min()
    g = P.grid_info()   # the device's own cells: the boundary points below stay on them if the sizing changes
    gx, gy = g["nx"], g["ny"]
    assert gx > 1 and gy > 1 and g["x0"] == X.min() and g["y0"] == Y.min()
    assert g["cells_per_x"] == gx / W and g["cells_per_y"] == gy / H
    xs = list(X[p].mean(axis=1)) + list((X[p[:, 0]] + X[p[:, 1]]) / 2) + list(X)
    ys = list(Y[p].mean(axis=1)) + list((Y[p[:, 0]] + Y[p[:, 1]]) / 2) + list(Y)
    for k in range(gx + 1):
        for m in range(gy + 1):
            xs.append(X.min() + k * W / gx)
            ys.append(Y.min() + (m + 0.37) * H / gy if m < gy else Y.max())
            xs.append(X.min() + (k + 0.21) * W / gx if k < gx else X.max())
            ys.append(Y.min() + m * H / gy)
    xs += [X.min() - 1., X.max() + 1e-9, X.mean(), X.min() - 1e-9]
    ys += [Y.mean(), Y.mean(), Y.max() + 2., Y.min() - 1e-9]
    r = compare_points(P, R, np.array(xs), np.array(ys))
    assert (r["elem"] == -1).sum() >= 4 and (r["elem"] >= 0).sum() >= len(X)
    print("branches taken:", np.bincount(np.array(R.branch).ravel(), minlength=7))
    P.close()


# --- shapes chosen to break the kernels ---------------------------------------------

def plain(x, y, p, V=None, lbl=None, **kw):
    d = dict(x=np.asarray(x, float), y=np.asarray(y, float), p=np.asarray(p, np.int32),
             lbl=np.zeros(len(p), np.int32) if lbl is None else lbl, blocks=[dict(ex=2.0, ey=3.0, qv=0.0)],
             labels=[dict(block=0)], length_units=1, depth=1.0)
    d.update(kw)
    x, y = d["x"], d["y"]
    return d, (1. + x * 0 + 2. * x / max(np.abs(x).max(), 1e-300) - y / max(np.abs(y).max(), 1e-300)
               + (x / max(np.abs(x).max(), 1e-300)) ** 2) if V is None else V


def test_fan_hits_the_list_cap():
    """One interior node with 24 incident triangles: both scans go round, the
    list stops at 20 entries."""
    n = 24
    a = 2 * np.pi * np.arange(n) / n
    x = np.concatenate([[0.3], 0.3 + (2 + 0.3 * np.cos(3 * a)) * np.cos(a)])
    y = np.concatenate([[-0.2], -0.2 + (2 + 0.3 * np.cos(3 * a)) * np.sin(a)])
    p = [[0, 1 + k, 1 + (k + 1) % n] for k in range(n)]
    kw, V = plain(x, y, p)
    R = postproc.Post(kw, V + 0.3 * np.sin(5 * x), "es")
    assert len(R.con[0]) == 24
    P = device(R)
    compare_fields(P, R)
    compare_points(P, R, np.array([0.3, 0.3 + 1.0, 5.0]), np.array([-0.2, -0.2 + 0.1, 5.0]))
    P.close()


def test_strip_singular_fit():
    """A strip one element wide.  The neighbour list of a corner always holds
    the element's own two other corners, so the fit's determinant vanishes only
    through the arithmetic: at 1e-100 length units the products of three sums
    underflow to zero, and every corner falls back to the element's value."""
    n = 9
    x = np.concatenate([np.arange(n), np.arange(n) + 0.5]) * 1e-100
    y = np.concatenate([np.zeros(n), np.ones(n)]) * 1e-100
    p = []
    for k in range(n - 1):
        p += [[k, k + 1, n + k], [k + 1, n + k + 1, n + k]]
    kw, V = plain(x, y, p)
    R = postproc.Post(kw, V, "es")
    assert (np.array(R.branch) == 6).all()
    P = device(R)
    compare_fields(P, R)
    compare_points(P, R, np.array([2.2e-100, 0.0, 1e-99]), np.array([0.4e-100, 0.0, 1e-99]))
    P.close()


def test_oversize_element():
    """One triangle over more than half the bounding box beside 288 small
    ones: the cells are sized by the mean element (13 per axis here), the big
    triangle's box covers all 169 > 64 of them and goes on the oversize list."""
    xg, yg, pg = electro.grid(13, 13, 1.0, 1.0, 0.0, 0.0)
    x = np.concatenate([xg, [1.0, 20.0, 1.0]])
    y = np.concatenate([yg, [1.5, 1.5, 20.0]])
    nb = len(xg)
    p = np.concatenate([pg, [[nb, nb + 1, nb + 2]]])
    kw, V = plain(x, y, p)
    R = postproc.Post(kw, V, "es")
    P = device(R)
    compare_fields(P, R)
    xs = np.array([5.0, 1.0, 10.5, 19.0, 0.5, 0.25, 1.0, 15.0, 3.0])
    ys = np.array([5.0, 1.5, 10.75, 1.6, 0.5, 1.0, 20.0, 15.0, 1.5])
    r = compare_points(P, R, xs, ys)
    assert r["elem"][0] == len(pg) and r["elem"][7] == -1
    P.close()


def test_no_points():
    kw, V = plain(*electro.grid(3, 3, 1.0, 1.0))
    P = device(postproc.Post(kw, V, "es"))
    r = P.point_values(np.zeros(0), np.zeros(0))
    assert r["elem"].shape == (0,) and r["raw"].shape == (0, 8)
    P.close()


# --- determinism -----------------------------------------------------------------------

def test_bit_equal_runs():
    kw, V = postproc.synthetic(13, 11, True, "es")
    R = postproc.Post(kw, V, "es")
    xs = np.linspace(min(R.X) - 0.1, max(R.X) + 0.1, 41).repeat(37)
    ys = np.tile(np.linspace(min(R.Y) - 0.1, max(R.Y) + 0.1, 37), 41)
    runs = []
    for _ in range(2):          # a second problem: the grid built again
        P = device(R)
        for _ in range(2):      # and every call twice on each
            f = P.element_fields()
            pts = [P.point_values(xs, ys, smooth=s) for s in (False, True)]
            runs.append((f["D"], f["E"], P.corner_fields(), P.block_integrals([0, 1, 2])["raw"],
                         pts[0]["elem"], pts[0]["raw"], pts[1]["elem"], pts[1]["raw"]))
        P.close()
    for r in runs[1:]:
        for a, b in zip(runs[0], r):
            assert a.tobytes() == b.tobytes()


# --- lifecycle ---------------------------------------------------------------------------

def test_new_solve_invalidates_and_memory_grows():
    x, y, p = electro.grid(9, 9, 1.0, 1.0)
    e = electro.tag_edges(x, y, p, [(lambda xa, ya, xb, yb: xa == 0 and xb == 0, 0),
                                    (lambda xa, ya, xb, yb: xa == 1 and xb == 1, 1)])

    def problem(v1):
        return kernels.ElectrostaticProblem(x=x * 10, y=y * 10, p=p, lbl=np.zeros(len(p), np.int32), e=e,
                                            blocks=[dict(ex=1.0, ey=1.0, qv=0.0)], labels=[dict(block=0)],
                                            lines=[dict(format=0, V=0.0), dict(format=0, V=v1)], length_units=2,
                                            depth=1.0)

    P = problem(10.0)
    P.solve()
    m0 = P.memory()
    E1 = P.element_fields()["E"]
    P.corner_fields()
    P.point_values([0.5], [0.5])
    m1 = P.memory()
    ne, n = len(p), len(x)
    cached = 8 * (2 * n + 4 * ne + 6 * ne) + 4 * (n + n + 1 + 3 * ne)   # coordinates, fields, marks and lists
    print("memory live before %d after %d (cached arrays >= %d)" % (m0["live_bytes"], m1["live_bytes"], cached))
    assert m1["live_bytes"] - m0["live_bytes"] >= cached
    assert np.allclose(E1[:, 0], -10.0 / 0.01, rtol=1e-6) and np.abs(E1[:, 1]).max() <= 1e-3   # 10 V over 1 cm
    # scratch retired by the entry points becomes reusable: repeated calls do not grow the arena
    for _ in range(2):   # (the first rounds grow the point buffers and retire the small ones)
        P.corner_branches()
        P.point_values(np.linspace(0, 1, 50), np.linspace(0, 1, 50))
    m2 = P.memory()
    for _ in range(3):
        P.corner_branches()
        P.point_values(np.linspace(0, 1, 50), np.linspace(0, 1, 50))
    m3 = P.memory()
    assert m3["live_bytes"] + m3["reuse_bytes"] == m2["live_bytes"] + m2["reuse_bytes"], (m2, m3)
    P.close()
    Q = problem(30.0)
    Q.solve()
    assert np.allclose(Q.element_fields()["E"][:, 0], -30.0 / 0.01, rtol=1e-6)
    # the same problem solved again after its fields were cached: a loaded
    # solution, then a solve, each replace them
    Q.set_solution(np.zeros(n))
    assert np.abs(Q.element_fields()["E"]).max() == 0
    Q.solve()
    assert np.allclose(Q.element_fields()["E"][:, 0], -30.0 / 0.01, rtol=1e-6)
    Q.close()


def test_refusals():
    kw, V = plain(*electro.grid(3, 3, 1.0, 1.0))
    P = kernels.ElectrostaticProblem(**kw)
    for call in (P.element_fields, P.corner_fields, lambda: P.block_integrals([0]),
                 lambda: P.point_values([0.5], [0.5])):
        with pytest.raises(kernels.XfkError, match="no solution yet"):
            call()
    P.set_solution(V)
    with pytest.raises(kernels.XfkError, match="types 5 and 6"):
        P.block_integral([0], 5)
    with pytest.raises(kernels.XfkError, match="null selection mask"):
        P.block_integrals(None)
    assert abs(P.block_integral([0], 1).real - 1e-6) <= 1e-18   # 1 mm^2
    L = kernels.load_library()
    import ctypes as C
    el = np.zeros(1, np.int32)
    o = np.zeros(8)
    rc = L.xfk_pot_point_values(P._h, -1, o.ctypes.data_as(kernels.dptr), o.ctypes.data_as(kernels.dptr), 0,
                                el.ctypes.data_as(kernels.iptr), o.ctypes.data_as(kernels.dptr))
    assert rc == XFK_ERR_ARG and b"negative number of points" in L.xfk_last_error()
    P.close()
    M = kernels.Static2DProblem(device=0, **synth_to_oracle(synth.bc_showcase(8))[2])
    D = np.zeros(2 * M.n_elems)
    for rc in (L.xfk_pot_element_fields(M._h, D.ctypes.data_as(kernels.dptr), None),
               L.xfk_pot_set_solution(M._h, D.ctypes.data_as(kernels.dptr)),
               L.xfk_pot_corner_fields(M._h, None),
               L.xfk_pot_block_integrals(M._h, C.cast(D.ctypes.data, C.POINTER(C.c_ubyte)), o.ctypes.data_as(kernels.dptr)),
               L.xfk_pot_point_values(M._h, 0, None, None, 0, None, None)):
        assert rc == XFK_ERR_ARG and b"not a scalar-potential problem" in L.xfk_last_error()
    M.close()
