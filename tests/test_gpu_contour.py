"""Contour integrals on the device (k_pp_contour of xfk_postproc.hip) against
the literal restatement of the reference's lineIntegral (tests/contourref.py).
No recorded reference output of a line integral exists; the restatement is
held to closed forms by tests/test_contour_cpu.py, which also asserts that on
the contours used here the reference's walk takes the lowest-numbered
containing element at every sample, the device's rule.

Solutions are loaded with set_solution, so no solver tolerance enters.  Bound:
1e-12 of the restatement's sum of the absolute terms (the bound
tests/test_gpu_postproc.py holds the block integrals to: the summation order
and a few dozen roundings); an averaged output is divided by the weight sum
after the bound is formed.  Sample points and elements are compared exactly."""
import numpy as np
import pytest

import contourref
import electro
import postproc
from contourref import Lines
from test_contour_cpu import MESHES, mesh
from util import precision_bound, rel_err, synth_to_oracle
from xfemm_amd import kernels, synth

pytestmark = pytest.mark.gpu

TOL = 1e-12
XFK_ERR_ARG = -1   # include/xfemm_kernels.h
NPTS = contourref.CONDITION_NPTS[0]


def device(R):
    """The device problem of restatement R with R's solution loaded."""
    cls = kernels.HeatFlowProblem if R.heat else kernels.ElectrostaticProblem
    kw = dict(R.kw)
    if kw.get("dt", 0) != 0 and kw.get("t_prev") is None:
        kw["t_prev"] = np.zeros(R.N)
    P = cls(**kw)
    P.set_solution(R.V)
    return P


@pytest.fixture(scope="module", params=MESHES, ids=str)
def case(request):
    """(restatement, its lines, device problem, the contours) of one mesh, shared by the tests below."""
    R = mesh(request.param)
    P = device(R)
    yield R, Lines(R), P, contourref.contours(R)
    P.close()


def check(got, want, kind, heat, what):
    """The two results against the restatement's, the averages divided after the bound."""
    v, s, sums = want["value"], want["scale"], want["sums"]
    bound = [TOL * s[0], TOL * s[1]]
    if kind == 1:
        bound[1] = TOL * s[0] / abs(sums[1]) if sums[1] != 0 else 0.
    elif heat and kind == 3:
        bound[0] = TOL * s[0] / abs(sums[1]) if sums[1] != 0 else 0.
    for q in range(2):
        print("%s [%d]: got %.15g want %.15g (bound %.3e)" % (what, q, got[q], v[q], bound[q]))
        if np.isnan(v[q]):
            assert np.isnan(got[q]), what
        else:
            assert abs(got[q] - v[q]) <= bound[q], (what, q, got[q], v[q], bound[q])


@pytest.mark.parametrize("smooth", [False, True])
def test_device_against_restatement(case, smooth):
    """Every type, every contour: the sampled types with their samples and
    elements one for one, type 0 through the point path, type 2 on the host."""
    R, L, P, cs = case
    for cname, c in cs.items():
        for kind in contourref.TYPES[R.heat]:
            want = L.line_integral(c, kind, smooth, NPTS, record=False)
            r = P.line_integrals([c], kind, smooth=smooth, points=NPTS)
            s = P.contour_samples(c, kind, points=NPTS)
            assert s["xy"].tobytes() == np.array(want["pts"]).tobytes(), (cname, kind)
            assert np.array_equal(s["elem"], np.array(want["elems"], np.int32)), (cname, kind)
            assert r["missed"][0] == want["missed"]
            check(r["raw"][0], want, kind, R.heat, "%s type %d smooth %d" % (cname, kind, smooth))
            z = P.line_integral(c, kind, smooth=smooth, points=NPTS)
            assert np.array([z.real, z.imag]).tobytes() == r["raw"][0].tobytes()
        if R.axi and not R.heat:
            assert P.line_integral(c, 4, smooth=smooth, points=NPTS) == 0   # as block integral 6
        for kind in (0, 2):
            want = L.line_integral(c, kind)
            r = P.line_integrals([c], kind, smooth=smooth)
            assert r["missed"][0] == want["missed"]
            for q in range(2):
                if np.isnan(want["value"][q]):
                    assert np.isnan(r["raw"][0, q])
                else:
                    assert abs(r["raw"][0, q] - want["value"][q]) <= TOL * want["scale"][q], (cname, kind, q)
    n = len(cs["outside"]) - 1
    out = P.line_integrals([cs["outside"]], 1, points=NPTS)
    assert out["missed"][0] == n * NPTS and out["raw"][0, 0] == 0 and np.isnan(out["raw"][0, 1])   # 0/0
    part = P.line_integrals([cs["partly"]], 1, points=NPTS)["missed"][0]
    assert 0 < part < NPTS
    assert np.isnan(P.line_integral(cs["partly"], 0).real)   # an end outside the mesh


def test_default_points_and_smoothing(case):
    """points <= 0 is the reference's 400; smooth defaults to on."""
    R, L, P, cs = case
    a = P.line_integrals([cs["one"]], 1)["raw"]
    assert a.tobytes() == P.line_integrals([cs["one"]], 1, smooth=True, points=0)["raw"].tobytes()
    assert a.tobytes() == P.line_integrals([cs["one"]], 1, smooth=True, points=400)["raw"].tobytes()
    assert len(P.contour_samples(cs["one"], 1, points=-3)["elem"]) == 400


@pytest.fixture(scope="module")
def sweep():
    R = mesh(contourref.SWEEP_MESH)
    P = device(R)
    yield R, Lines(R), P, contourref.contours(R)
    P.close()


@pytest.mark.parametrize("npts", contourref.SWEEP_NPTS)
def test_points_per_segment_around_the_workgroup(sweep, npts):
    """1, 2 and 181 segments at samples per segment below, at and above the
    summing workgroup: workgroups that end inside a segment, on its end, and
    contours of one partial and of many."""
    R, L, P, cs = sweep
    for cname in contourref.SWEEP_CONTOURS:
        want = L.line_integral(cs[cname], 3, False, npts, record=False)
        r = P.line_integrals([cs[cname]], 3, smooth=False, points=npts)
        assert r["missed"][0] == want["missed"] == 0
        check(r["raw"][0], want, 3, False, "%s npts %d" % (cname, npts))
        s = P.contour_samples(cs[cname], 3, points=npts)
        assert np.array_equal(s["elem"], np.array(want["elems"], np.int32))


@pytest.mark.parametrize("nbatch", [1, 2, 33])
def test_batches_are_bit_equal_to_single_contours(sweep, nbatch):
    R, L, P, cs = sweep
    rng = np.random.default_rng(5)
    batch = []
    for k in range(nbatch):   # unequal lengths: 1 to 5 segments, some leaving the mesh, and the arc
        n = 2 + k % 5
        batch.append([contourref.at(R, *rng.uniform(0.02, 0.98, 2)) for _ in range(n)])
        if k % 4 == 3:
            batch[k].append(contourref.at(R, 1.3, 0.4 + 0.01 * k))
    if nbatch > 2:
        batch[7] = cs["arc"]
    for kind, npts in ((1, 37), (3, contourref.Q_BLOCK + 1), (4, 400)):
        a = P.line_integrals(batch, kind, points=npts)
        b = P.line_integrals(batch, kind, points=npts)
        assert a["raw"].tobytes() == b["raw"].tobytes() and np.array_equal(a["missed"], b["missed"])
        for k, c in enumerate(batch):
            one = P.line_integrals([c], kind, points=npts)
            assert one["raw"][0].tobytes() == a["raw"][k].tobytes(), (kind, k)
            assert one["missed"][0] == a["missed"][k]
        if nbatch > 2:
            assert (a["missed"] > 0).any() and (a["missed"] == 0).any()


def test_average_temperature_along_a_mesh_line():
    """Heat-flow type 3 does not shift its samples: along a mesh line they sit
    exactly on edges, where the walk's element and the lowest-numbered one may
    differ.  T is continuous, so the result still agrees: the element rule does
    not leak into a continuous quantity."""
    R = mesh((False, "hf"))
    L, P = Lines(R), device(R)
    ys = sorted(set(R.Y))
    c = [(min(R.X), ys[2]), (max(R.X), ys[2])]
    want = L.line_integral(c, 3, True, 50)
    s = P.contour_samples(c, 3, points=50)
    assert s["xy"].tobytes() == np.array(want["pts"]).tobytes()
    assert all(len(h) >= 2 for h in want["containing"])          # every sample on an edge or a node
    assert all(e in h for e, h in zip(s["elem"], want["containing"]))
    print("samples whose element differs from the walk's: %d of %d"
          % (int((s["elem"] != np.array(want["elems"])).sum()), len(s["elem"])))
    for smooth in (False, True):
        r = P.line_integrals([c], 3, smooth=smooth, points=50)
        check(r["raw"][0], want, 3, True, "average T on a mesh line")
    P.close()


def close_to(got, want, what):
    got, want = np.asarray(got, float), np.asarray(want, float)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(np.isnan(got), np.isnan(want)), what
    scale = np.nanmax(np.abs(want)) if np.isfinite(want).any() else 0.0
    err = np.nanmax(np.abs(got - want)) if np.isfinite(want).any() else 0.0
    assert err <= TOL * scale, (what, err, scale)


@pytest.mark.parametrize("name", ["test", "Temp0", "Temp1"])
def test_point_values_unchanged(name):
    """k_pp_points shares its search and its values with the contour kernel:
    on the fixtures' recorded points it gives what it gave, element and value."""
    from test_postproc_cpu import load
    R, chk, _ = load(name)
    P = device(R)
    pts = sorted({(x, y) for s in (False, True) for x, y, _ in chk["points"][s]})
    xs, ys = np.array([q[0] for q in pts]), np.array([q[1] for q in pts])
    for smooth in (False, True):
        r = P.point_values(xs, ys, smooth=smooth)
        el, out = R.points(xs, ys, smooth)
        assert np.array_equal(r["elem"], el), (smooth, r["elem"], el)
        for c in range(8):
            close_to(r["raw"][:, c], out[:, c], "point value %d smooth %d" % (c, smooth))
        assert r["raw"].tobytes() == P.point_values(xs, ys, smooth=smooth)["raw"].tobytes()
    P.close()


def test_solved_plates_charge():
    """The plate capacitor solved on the device: the flux of D through a
    contour between the plates is the conductor's integrated charge, within the
    bound the solved potential keeps (the field is uniform)."""
    w, h, depth, V0 = 4.0, 2.5, 0.7, 12.0
    x, y, p = electro.grid(9, 6, w, h)
    e = electro.tag_edges(x, y, p, [(lambda xa, ya, xb, yb: xa == 0 and xb == 0, 0)])
    cond = np.where(x == x.max(), 0, -1).astype(np.int32)
    kw = dict(x=x, y=y, p=p, e=e, lbl=np.zeros(len(p), np.int32), blocks=[dict(ex=3.0, ey=7.0)],
              labels=[dict(block=0)], lines=[dict(format=0, V=0.0)], conductors=[dict(type=1, V=V0)],
              conductor=cond, depth=depth, length_units=1, precision=1e-12)
    P = kernels.ElectrostaticProblem(**kw)
    P.solve()
    V = P.solution()
    bound = precision_bound(V0 * x / w, electro.restate(kw)["V"][:len(x)], 1e-6)
    _, q = P.conductors()
    flux = P.line_integral(kernels.Contour().add(1.3, 0.0).add(1.3, h), 1)
    print("solved V vs exact %.3e (bound %.3e); flux %.12e, charge %.12e" % (rel_err(V, V0 * x / w), bound, flux.real, q[0]))
    assert abs(flux.real - q[0]) <= bound * abs(q[0])
    assert abs(flux.imag - q[0] / (h * 1e-3 * depth * 1e-3)) <= bound * abs(flux.imag)
    P.close()


def test_refusals():
    kw, V = postproc.synthetic(6, 5, False, "es")
    P = kernels.ElectrostaticProblem(**kw)
    line = [(1.0, 0.5), (3.0, 2.0)]
    with pytest.raises(kernels.XfkError, match="no solution yet"):
        P.line_integral(line, 1)
    P.set_solution(V)
    with pytest.raises(kernels.XfkError, match="electrostatic problem has types 0-4"):
        P.line_integral(line, 5)
    with pytest.raises(kernels.XfkError, match="type out of range"):
        P.line_integral(line, -1)
    with pytest.raises(kernels.XfkError, match="at least 2 points"):
        P.line_integral([(1.0, 0.5)], 1)
    with pytest.raises(kernels.XfkError, match="at least 2 points"):
        P.line_integrals([line, []], 2)
    with pytest.raises(kernels.XfkError, match="zero-length segment"):
        P.line_integral([(1.0, 0.5), (3.0, 2.0), (3.0, 2.0)], 3)
    with pytest.raises(kernels.XfkError, match="vertex is NaN"):
        P.line_integral([(1.0, 0.5), (float("nan"), 2.0)], 1)
    with pytest.raises(kernels.XfkError, match="vertex is infinite"):
        P.line_integral([(1.0, 0.5), (float("inf"), 2.0)], 1)
    assert P.line_integrals([], 1)["raw"].shape == (0, 2)
    L = kernels.load_library()
    d, i = kernels.dptr, kernels.iptr
    xs, ys, o = np.array([1.0, 3.0]), np.array([0.5, 2.0]), np.zeros(2)
    ptr = np.array([0, 2], np.int32)
    xp, yp, op, pp = xs.ctypes.data_as(d), ys.ctypes.data_as(d), o.ctypes.data_as(d), ptr.ctypes.data_as(i)
    for call, msg in (
            (lambda: L.xfk_pot_line_integrals(P._h, -1, pp, xp, yp, 1, 1, 0, op, None), b"negative number of contours"),
            (lambda: L.xfk_pot_line_integral(P._h, -2, xp, yp, 1, 1, 0, op, None), b"negative number of contour points"),
            (lambda: L.xfk_pot_line_integrals(P._h, 1, None, xp, yp, 1, 1, 0, op, None), b"null contour arrays"),
            (lambda: L.xfk_pot_line_integrals(P._h, 1, pp, None, yp, 1, 1, 0, op, None), b"null contour arrays"),
            (lambda: L.xfk_pot_line_integral(P._h, 2, xp, None, 1, 1, 0, op, None), b"null contour arrays"),
            (lambda: L.xfk_pot_line_integral(P._h, 2, xp, yp, 1, 1, 0, None, None), b"null output"),
            (lambda: L.xfk_pot_contour_samples(P._h, 2, xp, yp, 1, 0, None, None), b"null output"),
            (lambda: L.xfk_pot_contour_time(P._h, 1, pp, xp, yp, 1, 1, 0, 0, op), b"repeats > 0")):
        rc = call()
        assert rc == XFK_ERR_ARG and msg in L.xfk_last_error(), (rc, msg, L.xfk_last_error())
    ms = P.time_contours([line], 1, repeats=2)
    assert ms > 0
    P.close()
    kw, V = postproc.synthetic(6, 5, False, "hf")
    H = kernels.HeatFlowProblem(**kw)
    H.set_solution(V)
    with pytest.raises(kernels.XfkError, match="heat-flow problem has types 0-3"):
        H.line_integral(line, 4)
    H.close()
    M = kernels.Static2DProblem(device=0, **synth_to_oracle(synth.bc_showcase(8))[2])
    for call in (lambda: L.xfk_pot_line_integrals(M._h, 1, pp, xp, yp, 1, 1, 0, op, None),
                 lambda: L.xfk_pot_line_integral(M._h, 2, xp, yp, 1, 1, 0, op, None)):
        assert call() == XFK_ERR_ARG and b"not a scalar-potential problem" in L.xfk_last_error()
    M.close()
