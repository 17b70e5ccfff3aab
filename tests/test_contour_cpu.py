"""The restatement of the reference's lineIntegral and bendContour
(tests/contourref.py) against closed forms, to 1e-12 of the sum of the absolute
terms (the midpoint rule is exact for the constant and linear integrands used
here, so only rounding separates the two), and the condition the device
comparison of tests/test_gpu_contour.py presumes about its contours."""
import math

import numpy as np
import pytest

import contourref
import electro
import postproc
from contourref import Lines, bend
from postproc import EO, PI
from test_postproc_cpu import load

TOL = 1e-12


def near(got, want, scale, what):
    print("%s: got %.15g want %.15g (scale %.3e)" % (what, got, want, scale))
    assert abs(got - want) <= TOL * scale, (what, got, want, scale)


def plates():
    """Planar plate capacitor, V = V0 x / w, ex != ey (cm, depth 0.7 cm)."""
    w, h, depth, V0 = 4.0, 2.5, 0.7, 12.0
    u = electro.UNITS[2]
    x, y, p = electro.grid(9, 6, w * u, h * u)
    kw = dict(x=x, y=y, p=p, lbl=np.zeros(len(p), np.int32), blocks=[dict(ex=3.0, ey=7.0)], labels=[dict(block=0)],
              depth=depth, length_units=2)
    return postproc.Post(kw, V0 * x / x.max(), "es"), w, h, depth, V0


@pytest.mark.parametrize("smooth", [False, True])
@pytest.mark.parametrize("contour", [[(1.3, 0.2), (1.3, 2.3)], [(0.35, 0.4), (3.1, 2.2)]], ids=["across", "oblique"])
def test_planar_plates(contour, smooth):
    R, w, h, depth, V0 = plates()
    L = Lines(R)
    lc = R.lc
    Ex = -V0 / (w * lc)
    Dx = EO * 3.0 * Ex
    (xa, ya), (xb, yb) = contour
    ln = math.hypot(xb - xa, yb - ya)
    nr, ni = -(yb - ya) / ln, (xb - xa) / ln
    area = ln * lc * depth * lc
    r = L.line_integral(contour, 1, smooth, 40)
    assert r["missed"] == 0
    near(r["value"][0], Dx * nr * area, r["scale"][0], "D.n")
    near(r["value"][1], Dx * nr, r["scale"][0] / area, "average D.n")
    r = L.line_integral(contour, 3, smooth, 40)
    # 1/2 eps E^2 area along n for a contour across the field; in general
    # 1/2 D E (n_x, -n_y) area for a field along x
    near(r["value"][0], 0.5 * Dx * Ex * nr * area, max(r["scale"]), "Fx")
    near(r["value"][1], -0.5 * Dx * Ex * ni * area, max(r["scale"]), "Fy")
    F1, F2 = 0.5 * Dx * Ex * nr * area, -0.5 * Dx * Ex * ni * area
    mx, my = (0.5 * (xa + xb) + nr * 1e-6) * lc, (0.5 * (ya + yb) + ni * 1e-6) * lc
    r = L.line_integral(contour, 4, smooth, 40)
    near(r["value"][0], mx * F2 - F1 * my, r["scale"][0] + abs(mx * F2) + abs(F1 * my), "torque")
    r = L.line_integral(contour, 0)
    near(r["value"][0], V0 * (xa - xb) / w, V0, "V difference")
    r = L.line_integral(contour, 2)
    near(r["value"][0], ln * lc, ln * lc, "length")
    near(r["value"][1], ln * lc * depth * lc, area, "area")


def test_axisymmetric_axial_field():
    """V = V0 z / h on a disc 0 <= r <= R (mm): through the radial contour
    0 -> R the flux is pi R^2 D_z and the force 1/2 eps E^2 pi R^2."""
    Rr, h, V0 = 30.0, 8.0, 5.0
    x, y, p = electro.grid(8, 5, Rr, h)
    kw = dict(x=x, y=y, p=p, lbl=np.zeros(len(p), np.int32), blocks=[dict(ex=2.0, ey=5.0)], labels=[dict(block=0)],
              length_units=1, problem_type=1)
    R = postproc.Post(kw, V0 * y / h, "es")
    L = Lines(R)
    Ez = -V0 / (h * R.lc)
    Dz = EO * 5.0 * Ez
    A = PI * (Rr * R.lc) ** 2
    c = [(0.0, 3.1), (Rr, 3.1)]
    for smooth in (False, True):
        r = L.line_integral(c, 1, smooth, 25)
        assert r["missed"] == 0
        near(r["value"][0], Dz * A, r["scale"][0], "flux")
        near(r["value"][1], Dz, r["scale"][0] / A, "average D.n")
        r = L.line_integral(c, 3, smooth, 25)
        assert r["value"][0] == 0
        near(r["value"][1], 0.5 * Dz * Ez * A, r["scale"][1], "Fz")
        assert L.line_integral(c, 4, smooth, 25)["value"] == [0., 0.]
    r = L.line_integral(c, 2)
    near(r["value"][0], Rr * R.lc, Rr * R.lc, "length")
    near(r["value"][1], A, A, "swept area")


def test_heat_strip_linear_temperature():
    """T = T0 + a x + b y in a strip of constant k (m): F = -k grad T, and the
    average T along an oblique line is T at its midpoint."""
    w, h, depth, k = 0.5, 0.2, 0.3, 4.0
    T0, a, b = 300.0, 40.0, -25.0
    x, y, p = electro.grid(8, 5, w, h)
    kw = dict(x=x, y=y, p=p, lbl=np.zeros(len(p), np.int32), blocks=[dict(kx=k, ky=k, kt=0.0, qv=0.0)],
              labels=[dict(block=0)], length_units=3, depth=depth)
    R = postproc.Post(kw, T0 + a * x + b * y, "hf")
    L = Lines(R)
    (xa, ya), (xb, yb) = c = [(0.03, 0.021), (0.44, 0.173)]
    ln = math.hypot(xb - xa, yb - ya)
    nr, ni = -(yb - ya) / ln, (xb - xa) / ln
    for smooth in (False, True):
        r = L.line_integral(c, 1, smooth, 30)
        assert r["missed"] == 0
        Fn = -k * a * nr - k * b * ni
        near(r["value"][0], Fn * ln * depth, r["scale"][0], "F.n")
        near(r["value"][1], Fn, r["scale"][0] / (ln * depth), "average F.n")
        r = L.line_integral(c, 3, smooth, 30)
        Tm = T0 + a * 0.5 * (xa + xb) + b * 0.5 * (ya + yb)
        near(r["value"][0], Tm, r["scale"][0] / (ln * depth), "average T")
        near(r["value"][1], ln * depth, ln * depth, "weight")
    near(L.line_integral(c, 0)["value"][0], a * (xa - xb) + b * (ya - yb), T0, "T difference")
    r = L.line_integral(c + [(0.44, 0.01)], 2)
    near(r["value"][0], ln + 0.163, ln + 0.163, "length")
    near(r["value"][1], (ln + 0.163) * depth, ln, "area")


def test_bend():
    c = bend([(1.0, 2.0), (4.0, 3.0)], 90., 1.)
    assert len(c) == 1 + 90 and c[0] == (1.0, 2.0)
    assert math.hypot(c[-1][0] - 4.0, c[-1][1] - 3.0) <= 1e-14 * 5
    # the circle through both ends on which the chord subtends 90 degrees
    d = math.hypot(3.0, 1.0)
    Rr = d / (2. * math.sin(math.pi / 4))
    pts = np.array(c)
    # its centre: equidistant from every point
    A = 2 * (pts[1:] - pts[0])
    ctr = np.linalg.lstsq(A, (pts[1:] ** 2).sum(axis=1) - (pts[0] ** 2).sum(), rcond=None)[0]
    rad = np.hypot(pts[:, 0] - ctr[0], pts[:, 1] - ctr[1])
    assert np.abs(rad - Rr).max() <= 1e-13 * Rr
    # counts: ceil(|angle / step|) points replace the last one
    assert len(bend([(0., 0.), (1., 0.), (2., 1.)], -100., 7.)) == 2 + math.ceil(100. / 7.)
    assert len(bend([(0., 0.), (1., 0.)], 45., 0.)) == 1 + 45          # a step of 0 is taken as 1
    assert len(bend([(0., 0.), (1., 0.)], 180., 1.)) == 181
    # the refusals
    two = [(0., 0.), (1., 0.5)]
    assert bend(two, 0., 1.) == two and bend(two, 181., 1.) == two and bend(two, -180.5, 1.) == two
    assert bend([(3., 4.)], 90., 1.) == [(3., 4.)] and bend([], 90., 1.) == []
    # a negative angle bends to the other side
    up, dn = bend(two, 90., 10.), bend(two, -90., 10.)
    side = lambda q: (two[1][0] - two[0][0]) * (q[1] - two[0][1]) - (two[1][1] - two[0][1]) * (q[0] - two[0][0])
    assert side(up[4]) * side(dn[4]) < 0


def test_package_contour_helper_is_the_restatement():
    """kernels.Contour (host only) builds what the restatement builds."""
    from xfemm_amd.kernels import Contour
    c = Contour().add(1.0, 2.0).add(1.0, 2.0).add(4.0, 3.0)
    assert c.points == [(1.0, 2.0), (4.0, 3.0)]           # a point equal to the last is dropped
    for angle, step in ((90., 1.), (-100., 7.), (180., 1.), (45., 0.), (0., 1.), (200., 1.)):
        q = Contour([(1.0, 2.0), (4.0, 3.0)]).bend(angle, step)
        assert q.points == bend([(1.0, 2.0), (4.0, 3.0)], angle, step), (angle, step)
    assert Contour([(1., 1.)]).bend(90., 1.).points == [(1., 1.)]
    assert Contour([(1., 1.), (2., 2.)]).clear().points == []


def test_search_is_the_literal_search():
    """The restatement's InTriangle (circle test over all elements at once)
    visits and returns what the element-by-element loop does, static index
    included."""
    kw, V = postproc.synthetic(6, 5, True, "es")
    L = Lines(postproc.Post(kw, V, "es"))
    rng = np.random.default_rng(7)
    for _ in range(300):
        x, y = contourref.at(L.R, rng.uniform(-0.1, 1.1), rng.uniform(-0.1, 1.1))
        k0 = L.k
        a, k1 = L.in_triangle(x, y), L.k
        L.k = k0
        assert L.in_triangle_literal(x, y) == a and L.k == k1


def mesh(name):
    if isinstance(name, str):
        return load(name)[0]
    kw, V = postproc.synthetic(6, 5, name[0], name[1])
    return postproc.Post(kw, V, name[1])


MESHES = ["test", "Temp0", "Temp1", (False, "es"), (True, "es"), (False, "hf"), (True, "hf")]


@pytest.mark.parametrize("name", MESHES, ids=str)
def test_walk_takes_the_lowest_containing_element(name):
    """The condition of the device comparison: on every contour the device
    tests compare with an unsmoothed or cross-material field, the reference's
    walk chooses the lowest-numbered containing element at every sample (the
    device's rule), so the 1e-12 comparison cannot hide an element mismatch.
    The share of disagreeing samples must be exactly 0."""
    R = mesh(name)
    L = Lines(R)
    for cname, c in contourref.contours(R).items():
        for npts in contourref.CONDITION_NPTS:
            r = L.line_integral(c, 1, False, npts)
            bad = sum(1 for e, h in zip(r["elems"], r["containing"]) if e != (h[0] if h else -1))
            print("%s %s npts %d: %d samples, %d disagree, %d outside" % (name, cname, npts, len(r["elems"]), bad,
                                                                          r["missed"]))
            assert bad == 0
            assert r["missed"] == sum(1 for h in r["containing"] if not h)
        n = len(c) - 1
        if cname == "outside":
            assert r["missed"] == n * npts
        elif cname == "partly":
            assert 0 < r["missed"] < n * npts


@pytest.mark.parametrize("npts", contourref.SWEEP_NPTS)
def test_walk_takes_the_lowest_containing_element_in_the_sweep(npts):
    """The same condition for the samples-per-segment sweep of the device tests."""
    R = mesh(contourref.SWEEP_MESH)
    L = Lines(R)
    C = contourref.contours(R)
    for cname in contourref.SWEEP_CONTOURS:
        r = L.line_integral(C[cname], 3, False, npts)
        bad = sum(1 for e, h in zip(r["elems"], r["containing"]) if e != (h[0] if h else -1))
        print("%s npts %d: %d samples, %d disagree" % (cname, npts, len(r["elems"]), bad))
        assert bad == 0 and len(r["elems"]) == (len(C[cname]) - 1) * npts
