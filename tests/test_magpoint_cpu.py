"""The restatement of fpproc's point values and contour integrals
(tests/magpointref.py) pinned on the CPU: against oracle/pointvalues.py, the
planar restatement the project already trusts, bit for bit; against a uniform
field; and against the closed forms of the layered strip.

A condition, not a tolerance: interior test points are barycentric
combinations with every weight >= 0.05 and contour coordinates lie off every
mesh line, and the tests assert that the reference's search and the
lowest-numbered search choose the same element for every test point and every
contour sample, and that no sample is missed -- so the device comparison
(tests/test_gpu_magpoint.py, lowest-numbered mode) leaves nothing out.
"""
import os

import numpy as np
import pytest

import magmaskref as MM
import magpointref as MP
import magpostref as M
from oracle import ansmesh, femfile, pointvalues
from util import GOLDEN, kernel_kwargs

BOUND = 1e-12


def bary_points(R, rng, elems, n_per=1):
    """interior points of the elements: every barycentric weight >= 0.05"""
    xs, ys = [], []
    for e in elems:
        X, Y, _ = R.corners(e)
        for _ in range(n_per):
            w = 0.05 + 0.85 * rng.dirichlet([1., 1., 1.])
            xs.append(w[0] * X[0] + w[1] * X[1] + w[2] * X[2])
            ys.append(w[0] * Y[0] + w[1] * Y[1] + w[2] * Y[2])
    return np.array(xs), np.array(ys)


def two_material(n=6, corner=False, seed=0, length_units=1):
    """A planar n x n grid of two labels with different permeabilities and a
    random A: label 1 the right half, or (corner) the upper right quadrant --
    a node away from interfaces, interface nodes, boundary nodes on the
    interface (the special-case punt) and the quadrant's corner (too sharp)."""
    rng = np.random.default_rng(seed)
    xs = np.linspace(-1.5, 2.1, n + 1) + np.concatenate([[0.], 0.05 * rng.uniform(-1, 1, n - 1), [0.]])
    ys = np.linspace(-1.0, 1.7, n + 1)
    x, y, p, col, row = MM.grid(xs, ys)
    lbl = ((col >= n // 2) & ((row >= n // 2) | (not corner))).astype(np.int32)
    u = M.UNIT_CM[length_units]
    kw = dict(x=x * u, y=y * u, p=p, lbl=lbl, e=-np.ones((len(p), 3), np.int32), marker=None, pbc=None,
              blocks=[dict(mu_x=1.0, mu_y=1.0), dict(mu_x=300.0, mu_y=200.0)], labels=[dict(block=0), dict(block=1)],
              lines=[], points=[], circuits=[], precision=1e-8, length_units=length_units, coords=0, relax=1.0,
              problem_type=0)
    return kw, rng.uniform(-1, 1, len(x)) * 1e-3


@pytest.mark.parametrize("corner", [False, True], ids=["halves", "quadrant"])
def test_planar_b_equals_pointvalues_bit_for_bit(corner):
    kw, A = two_material(corner=corner)
    R = M.MagPost(kw, A)
    Q = MP.MagPoint(R)
    F = pointvalues.FluxPost(R.X, R.Y, A, R.p, R.lbl, [0, 1], [0., 0.], [(1.0, 1.0, 0.0), (300.0, 200.0, 0.0)],
                             kw["length_units"])
    for e in range(len(R.p)):
        assert Q.nodal_b(e) == [tuple(float(v) for v in b) for b in F.nodal_b(e)]
    px, py = bary_points(R, np.random.default_rng(1), range(len(R.p)), 2)
    for x, y in zip(px, py):
        k = Q.find(float(x), float(y), "reference")
        assert k == F.in_triangle(float(x), float(y)) == Q.find_lowest(float(x), float(y)) and k >= 0
        o = Q.point_values_at(float(x), float(y), k, True)
        assert (o[1], o[2]) == tuple(float(v) for v in F.point_b(float(x), float(y)))
    want = {MP.PATCH, MP.INTERFACE, MP.PUNT, MP.SHARP}
    print("branches", sorted(Q.branches))
    assert Q.branches == want


def uniform_problem(axi, n=5, B0=0.7, length_units=1):
    """A uniform field B0 along y (z) in a linear medium of two labels (mu_r 5
    left, 1 right): planar A = -B0 x, axisymmetric 2 pi r A = pi r^2 B0."""
    xs = (np.linspace(0., 3.0, n + 1) if axi else np.linspace(-1.3, 1.7, n + 1))
    ys = np.linspace(-1.1, 1.4, n + 1)
    x, y, p, col, _ = MM.grid(xs, ys)
    lbl = (col >= n // 2).astype(np.int32)
    u = M.UNIT_CM[length_units]
    lc = M.LENGTH_CONV[length_units]
    kw = dict(x=x * u, y=y * u, p=p, lbl=lbl, e=-np.ones((len(p), 3), np.int32), marker=None, pbc=None,
              blocks=[dict(mu_x=5.0, mu_y=5.0), dict(mu_x=1.0, mu_y=1.0)], labels=[dict(block=0), dict(block=1)],
              lines=[], points=[], circuits=[], precision=1e-8, length_units=length_units, coords=0, relax=1.0,
              problem_type=1 if axi else 0)
    X = M.user_xy(kw)[0]
    A = (M.PI * (X * lc) * (X * lc) * B0) if axi else -B0 * (X * lc)
    return kw, A, B0


def uniform_points(R, rng):
    """interior points, every node, and the midpoints of every element's first edge"""
    px, py = bary_points(R, rng, range(len(R.p)))
    mx = (R.X[R.p[:, 0]] + R.X[R.p[:, 1]]) / 2.
    my = (R.Y[R.p[:, 0]] + R.Y[R.p[:, 1]]) / 2.
    return np.concatenate([px, R.X, mx]), np.concatenate([py, R.Y, my]), len(px)


@pytest.mark.parametrize("axi", [False, True], ids=["planar", "axi"])
@pytest.mark.parametrize("smooth", [False, True], ids=["element", "smooth"])
def test_uniform_field(axi, smooth):
    kw, A, B0 = uniform_problem(axi)
    R = M.MagPost(kw, A)
    Q = MP.MagPoint(R)
    x, y, n_in = uniform_points(R, np.random.default_rng(2))
    el, o = Q.point_values(x, y, smooth)
    el_ref = np.array([Q.find(float(a), float(b), "reference") for a, b in zip(x, y)])
    assert np.all(el >= 0) and np.all(el[:n_in] == el_ref[:n_in])
    lc = R.lc
    Aex = (M.PI * (x * lc) * (x * lc) * B0) if axi else -B0 * (x * lc)
    mu = np.array([R.blocks[R.labels[R.lbl[k]]["block"]]["mu_x"] for k in el])
    assert np.abs(o[:, 0] - Aex).max() <= BOUND * np.abs(A).max()
    assert np.abs(o[:, 1]).max() <= BOUND * B0 and np.abs(o[:, 2] - B0).max() <= BOUND * B0
    H = B0 / (mu * M.MUO)
    assert np.all(np.abs(o[:, 6] - H) <= BOUND * H) and np.all(np.abs(o[:, 5]) <= BOUND * H)
    E = B0 * B0 / (2. * mu * M.MUO)
    assert np.all(np.abs(o[:, 9] - E) <= BOUND * E)
    assert np.all(o[:, 3] == mu) and np.all(o[:, 4] == mu)


STRIP_NY = 6   # rows of the strip: the middle four have no boundary node, so smoothing leaves them alike


def strip_contours(h=10.0):
    """The layered strip's contours (length units; off every mesh line).  The
    horizontal sides lie in interior rows at one offset from their rows' lower
    lines, where element and smoothed fields repeat from row to row: their
    contributions to H.t and to the force cancel.  Each sample is shifted by
    1e-6 along n = I t, outwards on the clockwise contour: its lower side is
    drawn 2e-6 higher, so that both sides sample their rows at one offset (the
    smoothed field varies with y inside a row)."""
    d = h / STRIP_NY
    xl, xr, yb, yt = -8.1, 8.15, -d + 0.6, d + 0.6
    ccw = [(xl, yb), (xr, yb), (xr, yt), (xl, yt), (xl, yb)]
    yc = yb + 2e-6
    cw = [(xl, yc), (xl, yt), (xr, yt), (xr, yc), (xl, yc)]
    ta, tb = d - 0.6, d + 0.6
    torque = [(xl, ta), (xl, tb), (xr, tb), (xr, ta), (xl, ta)]
    return dict(ccw=ccw, cw=cw, hcw=yt - yc, xl=xl, xr=xr, yb=yb, yt=yt, torque=torque, arm=d,
                flux=[(-9.3, 0.4), (-6.2, -1.1)], bn=[(-9.1, 0.8), (-5.9, 0.8)])


@pytest.mark.parametrize("length_units", [1, 0], ids=["mm", "inch"])
def test_layered_strip_contours(length_units):
    kw, A, info = MM.layered_strip(length_units=length_units, ny=STRIP_NY)
    R = M.MagPost(kw, A, depth=info["depth"])
    Q = MP.MagPoint(R)
    C = strip_contours(info["h"])
    lc, depth = R.lc, R.depth
    F, BL, BR = MM.strip_closed_form(R, info)
    hc = (C["yt"] - C["yb"]) * lc
    J = kw["blocks"][1]["J_re"] * 1.e6
    current = J * (8.0 * lc) * hc

    def both(contour, kind, smooth):
        a = Q.line_integral(contour, kind, smooth, 400, "lowest")
        b = Q.line_integral(contour, kind, smooth, 400, "reference")
        assert np.array_equal(a["elem"], b["elem"]) and a["missed"] == 0 and b["missed"] == 0
        assert a["z"] == b["z"]
        return a

    for smooth in (False, True):
        r = both(C["ccw"], 1, smooth)
        print("H.t %.17g current %.17g scale %.3g" % (r["z"][0], current, r["scale"][0]))
        assert abs(r["z"][0] - current) <= BOUND * r["scale"][0]
        # the stress tensor force on what the contour encloses: n = I t points
        # out of a clockwise contour
        r = both(C["cw"], 3, smooth)
        part = C["hcw"] / info["h"]      # the part of the slab's height the contour encloses
        Fc = F * part
        lorentz = R.block_integrals(info["sel"])[0][11].real * part
        w18 = MM.MagMask(R, info["sel"]).integrals()[0][0] * part
        print("Fx %.17g closed %.17g lorentz %.17g weighted %.17g scale %.3g; Fy %.3g" %
              (r["z"][0], Fc, lorentz, w18, r["scale"][0], r["z"][1]))
        assert abs(r["z"][0] - Fc) <= BOUND * r["scale"][0]
        assert abs(r["z"][0] - lorentz) <= BOUND * r["scale"][0]
        assert abs(r["z"][0] - w18) <= BOUND * r["scale"][0]
        assert abs(r["z"][1]) <= BOUND * r["scale"][1]
        # The torque about the origin is the lever arm times that force where the
        # stress is mirror-symmetric about the force's line of action.  Inside
        # the slab the discrete A is quadratic in x, so the crisscross cells'
        # upper and lower triangles carry a B_x of opposite sign, and the
        # horizontal sides of a contour add a couple unless they mirror each
        # other about a row line of the mesh (which maps the mesh onto itself):
        # such a contour about an interior row line y = d has the torque -d x
        # its own type-3 force.
        tq = C["torque"]
        t = both(tq, 4, smooth)
        f3 = both(tq, 3, smooth)
        arm = C["arm"] * lc
        print("T %.17g arm x F %.17g scale %.3g" % (t["z"][0], -arm * f3["z"][0], t["scale"][0]))
        assert f3["z"][0] != 0 and abs(t["z"][0] - (-arm * f3["z"][0])) <= BOUND * t["scale"][0]
        # ... and that force is tied to the closed form: its two vertical sides
        # alone give F for the enclosed height (and the Lorentz force); the
        # mirrored horizontal sides add the same x-force each (they do not
        # cancel as on the force contour above), and the four sides add up
        side = [both([tq[k], tq[k + 1]], 3, smooth) for k in range(4)]
        part_t = (tq[1][1] - tq[0][1]) / info["h"]
        fv = side[0]["z"][0] + side[2]["z"][0]
        sv = side[0]["scale"][0] + side[2]["scale"][0]
        assert abs(fv - F * part_t) <= BOUND * sv and abs(fv - lorentz / part * part_t) <= BOUND * sv
        assert abs(side[1]["z"][0] - side[3]["z"][0]) <= BOUND * f3["scale"][0]
        assert abs(f3["z"][0] - sum(q["z"][0] for q in side)) <= BOUND * f3["scale"][0]
        # (B.n)^2 along a horizontal line in the left air
        r = both(C["bn"], 5, smooth)
        ln = (C["bn"][1][0] - C["bn"][0][0]) * lc
        assert abs(r["z"][0] - BL * BL * ln) <= BOUND * r["scale"][0]
        assert abs(r["z"][1] - BL * BL) <= BOUND * BL * BL
    # B.n between two points of the left air: (A0 - A1) depth, the flux of B_L through the span in x
    r = both(C["flux"], 0, False)
    flux = BL * (C["flux"][1][0] - C["flux"][0][0]) * lc * depth
    print("flux %.17g closed %.17g" % (r["z"][0], flux))
    assert abs(r["z"][0] - flux) <= BOUND * r["scale"][0]
    # the length and the swept area
    r = Q.line_integral(C["ccw"], 2)
    per = 2. * ((C["xr"] - C["xl"]) + (C["yt"] - C["yb"])) * lc
    assert abs(r["z"][0] - per) <= BOUND * per and abs(r["z"][1] - per * depth) <= BOUND * per * depth


# Contours on the reference's own .ans.check meshes (unstructured; metres): a
# closed one round two coil sides and an open one across the core and the gap,
# their coordinates off every mesh line
GOLDEN_CONTOURS = dict(
    closed=[(0.0113, 0.0671), (0.0713, 0.0699), (0.0731, 0.1371), (0.0117, 0.1343), (0.0113, 0.0671)],
    open=[(0.0031, 0.2117), (0.1513, 0.2433), (0.1391, 0.3017)])


def golden_case(name):
    """The reference's .fem and .ans.check as a problem dictionary, A and Depth.
    The files' coil blocks are wound regions with proximity effects
    (LamType > 2), which the point values refuse: wound is True and they are
    taken as solid (LamType 0)."""
    pr = femfile.prepare_problem(femfile.parse_fem(os.path.join(GOLDEN, name + ".fem")))
    femfile.get_fill_factor(pr)
    mesh, sol = ansmesh.mesh_from_ans(os.path.join(GOLDEN, name + ".fem"), os.path.join(GOLDEN, name + ".ans.check"), pr)
    kw = kernel_kwargs(pr, mesh)
    wound = False
    for b in kw["blocks"]:
        if b.get("LamType", 0) > 2:
            b["LamType"] = 0
            wound = True
    return kw, sol.A, pr.Depth, wound


@pytest.mark.parametrize("name", ["Temp", "Temp1"])
def test_reference_mesh_contours_condition(name):
    """on the unstructured fixture meshes too, both searches take the same
    element for every sample of the contours the device tests use, none missed"""
    kw, A, depth, _ = golden_case(name)
    nc = len(kw["circuits"])
    Q = MP.MagPoint(M.MagPost(kw, A, depth=depth, circuits=([1] * nc, [0.] * nc, [0.] * nc)))
    for c in GOLDEN_CONTOURS.values():
        for points in (257, 400):
            _, lo, _ = Q.contour_samples(c, points, "lowest")
            _, rf, _ = Q.contour_samples(c, points, "reference")
            assert np.array_equal(lo, rf) and np.all(lo >= 0)
            assert len(set(Q.lbl[k] for k in lo)) > 1 and len(set(lo.tolist())) > 20
        for q in (c[0], c[-1]):
            assert Q.find(q[0], q[1], "reference") == Q.find_lowest(q[0], q[1]) >= 0
