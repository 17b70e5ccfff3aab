"""The restatement of the weighted stress tensor integrals (tests/maskref.py)
against the reference's recorded output, against closed forms, and rule by
rule; and the margin that lets the device tests demand the mask exactly."""

import numpy as np
import pytest

import maskref
import postproc
from maskref import Mask
from test_postproc_cpu import TOL, load


def test_fixture_lines_6_and_7():
    """Label 0 selected on the electrostatic fixture: integrals 5 and 6 print as
    lines 6 and 7 of test.out.check, within 5.1e-7 absolute (%f).  The fixture
    has one label, so every node is 1, the mask's gradient vanishes and the
    recorded values are 0.000000: this pins the plumbing (the file's MaxArea
    column, a mask of ones) and little else."""
    c = maskref.case("fixture")
    _, chk, _ = load("test")
    assert c["max_area"].shape == (1,) and c["max_area"][0] > 0
    F, T, _ = c["M"].integrals()
    l6, l7 = chk["integrals"][5], chk["integrals"][6]
    assert "Force" in l6[0] and "Torque" in l7[0]
    print("force %r torque %r; recorded %r %r" % (F, T, l6[1], l7[1]))
    assert abs(F[0] - l6[1][0]) <= TOL and abs(F[1] - l6[1][1]) <= TOL
    assert abs(T - l7[1][0]) <= TOL and abs(0. - l7[1][1]) <= TOL
    assert (c["M"].msk == 1).all()


def check_closed(c):
    F, T, _ = c["M"].integrals()
    cl = c["closed"]
    print("force %r (closed %r) torque %.15g (closed %.15g), scale %.6g"
          % (F, cl["force"], T, cl["torque"], cl["scale"]))
    assert np.abs(F - cl["force"]).max() <= 1e-12 * cl["scale"]
    # (the torque's own scale: the force times the lever arm w, <= 1 m here)
    assert abs(T - cl["torque"]) <= 1e-12 * cl["scale"]


def test_planar_capacitor_closed_form():
    """[0, w] x [0, h], air below y = g, a dielectric er above (selected),
    V = 0 on y = 0 and V0 on y = h, the same y-lines on both side walls.  The
    potential is piecewise linear in y, so in the air D = (0, D2) is uniform,
    D2 = -eo E_air, E_air = V0 / (g + (h - g) / er), and in the dielectric every
    node is 1, so grad msk = 0 there.  In an air element the integrand is, with
    c = -grad msk,  a F1 = a D2^2 msk_x / (2 eo),  a F2 = -a D2^2 msk_y / (2 eo).
    msk is linear per element, so a msk_y is the exact integral of msk_y over
    the element, and the sum over the air is, by the divergence theorem, the
    boundary integral of msk n_y: msk is 1 on the whole interface (n_y = 1,
    length w) and 0 on the plate, the side walls have n_y = 0.  Hence
    Fy = -(eo E_air^2 / 2) w Depth whatever 0 / 1 values the interior air nodes
    take.  Likewise Fx is the integral of msk n_x over the two side walls, whose
    values agree node by node (0 below y = g, 1 at it) on equal y-lines: 0.  The
    torque sums a (xc F2 - yc F1) with the element's centroid: for linear msk
    that is the exact integral of x msk_y - y msk_x, i.e. the boundary integral
    of x msk n_y - y msk n_x = w^2 / 2 from the interface, the walls cancelling
    again: T = -(eo E_air^2 / 2) (w^2 / 2) Depth.  Bound: 1e-12 of
    (eo E_air^2 / 2) w Depth."""
    check_closed(maskref.case("cap_planar"))


def test_axisymmetric_capacitor_closed_form():
    """The same layers on an annulus R_i <= r <= R_o, R_i > 0: a carries
    2 pi R of the centroid, exact for the linear r, so the sum telescopes to
    2 pi int r dr over the interface: Fz = -(eo E_air^2 / 2) pi (R_o^2 - R_i^2),
    Fr reported 0, no torque."""
    c = maskref.case("cap_axi")
    check_closed(c)
    F, T, _ = c["M"].integrals()
    assert F[0] == 0 and T == 0


# --- the rules, one mesh each ----------------------------------------------------------

def air_base(**extra):
    kw, V, _ = maskref.capacitor(nx=7, nair=5, ndiel=3)
    kw.update(extra)
    return kw, V


NX = 7


def test_rule_point_property_node_in_the_air():
    i = 2 * NX + 3
    kw, V = air_base()
    free = Mask(postproc.Post(kw, V, "es"), [1])
    assert free.LV[i] == -1 and 0.01 < free.W[i] < 0.99
    marker = -np.ones(len(V), np.int32)
    marker[i] = 0
    kw, V = air_base(marker=marker, points=[dict(V=0.0, qp=1e-9)])
    M = Mask(postproc.Post(kw, V, "es"), [1])
    assert M.LV[i] == 0 and abs(M.W[i]) <= 1e-14
    # the rule itself, where the Q mark does not already fix the node
    M.R.Q = np.full(M.R.N, -2)
    assert M.fixed_values()[i] == 0
    M.marker[i] = -1
    assert M.fixed_values()[i] == -1


def test_rule_conductor_node_in_the_air():
    i = 3 * NX + 2
    kw, V = air_base()
    cond = -np.ones(len(V), np.int32)
    cond[i] = 0
    kw, V = air_base(conductor=cond, conductors=[dict(type=0, V=0.0, q=1e-12)])
    M = Mask(postproc.Post(kw, V, "es"), [1])
    assert M.R.Q[i] == 0 and M.LV[i] == 0 and abs(M.W[i]) <= 1e-14


def test_rule_max_area_per_label():
    kw, V = air_base()
    R = postproc.Post(kw, V, "es")
    M0 = Mask(R, [1])
    M = Mask(R, [1], max_area=[0.04, -3.0])
    # an element of the air with three free nodes: its entries scale by sqrt(MaxArea) / sqrt(area)
    e = next(k for k in range(R.NE) if R.lbl[k] == 0 and all(M.LV[n] < 0 for n in R.p[k]))
    n = R.p[e]
    X, Y = R.X, R.Y
    area = ((Y[n[1]] - Y[n[2]]) * (X[n[0]] - X[n[2]]) - (Y[n[2]] - Y[n[0]]) * (X[n[2]] - X[n[1]])) / 2.
    assert area > 0 and abs(np.sqrt(0.04) - np.sqrt(area)) > 0.01
    free = [k for k in range(R.N) if M.LV[k] < 0]
    assert not np.allclose(M.A[np.ix_(free, free)], M0.A[np.ix_(free, free)])
    # the dielectric's label (<= 0) keeps the element areas: its rows are fixed nodes' diagonals, unchanged
    top = [k for k in range(R.N) if all(R.lbl[el] == 1 for el in R.con[k])]
    assert top and np.array_equal(M.A[top], M0.A[top])
    # one label throughout: the weight is a common factor and the solution the same
    Mu = Mask(R, [1], max_area=[0.04, 0.04])
    rows = [k for k in free if all(R.lbl[el] == 0 for el in R.con[k])]
    assert rows and (Mu.A[rows] != M0.A[rows]).any()


def test_rule_selected_node():
    kw, V = air_base()
    R = postproc.Post(kw, V, "es")
    inner, wall = 2 * NX + 3, 2 * NX
    M = Mask(R, [1], selected_nodes=[inner, wall])
    assert M.LV[inner] == 1 and M.LV[wall] == 1   # (the wall node: after the exterior-edge rule)
    assert Mask(R, [1]).LV[wall] == 0


def test_rule_selection_on_the_axis():
    kw, V, _ = maskref.capacitor(nx=7, nair=5, ndiel=3, axi=True, x0=0.0)
    R = postproc.Post(kw, V, "es")
    M = Mask(R, [1])
    assert M.on_axis
    axis_air = [j * NX for j in range(1, 5)]
    assert all(not M.is_kosher(k) for k in axis_air) and all(M.LV[k] == -1 for k in axis_air)
    assert M.LV[6] == 0 and M.LV[2 * NX + 6] == 0      # the outer wall, off the axis: kosher
    # the same mesh moved off the axis: its inner wall is an exterior edge like any other
    kw, V, _ = maskref.capacitor(nx=7, nair=5, ndiel=3, axi=True, x0=1.0)
    M1 = Mask(postproc.Post(kw, V, "es"), [1])
    assert not M1.on_axis and all(M1.LV[k] == 0 for k in axis_air)
    # a selected node on the axis alone turns the rule on
    kw, V, _ = maskref.capacitor(nx=7, nair=5, ndiel=3, axi=True, x0=0.0)
    kw["blocks"][1] = dict(ex=1.0, ey=1.0, qv=0.0)
    M2 = Mask(postproc.Post(kw, V, "es"), [], selected_nodes=[3 * NX])
    assert M2.on_axis and M2.LV[3 * NX] == 1 and M2.LV[2 * NX] == -1


def test_invalid_selection_raises():
    kw, V = air_base()
    R = postproc.Post(kw, V, "es")
    # nothing selected but a node inside the dielectric, which is not air
    with pytest.raises(maskref.InvalidSelection, match="cannot abut a region which is not free space"):
        Mask(R, [], selected_nodes=[7 * NX + 3])
    # two dielectric labels that touch, the higher-numbered elements selected
    lbl = np.array(kw["lbl"]).copy()
    cy = np.asarray(kw["y"])[np.asarray(kw["p"])].mean(axis=1)
    lbl[cy > np.unique(kw["y"])[-2]] = 2
    kw2 = dict(kw, lbl=lbl, labels=[dict(block=0), dict(block=1), dict(block=1)])
    R2 = postproc.Post(kw2, V, "es")
    with pytest.raises(maskref.InvalidSelection):
        Mask(R2, [2])
    assert Mask(R2, [1, 2]).LV[-1] == 1


# --- the margin of the threshold -----------------------------------------------------------

@pytest.mark.parametrize("name", maskref.CASES)
def test_no_node_near_the_threshold(name):
    """The device's W carries the PCG's error (1e-6 of max |W| = 1 is what the
    device tests allow), so its mask can be demanded exactly only where the
    converged W stays clear of 0.5: by 1e-3 on every mesh the device tests use."""
    M = maskref.case(name)["M"]
    gap = np.abs(M.W - 0.5).min()
    print("%s: %d nodes, %d free, min |W - 0.5| = %.4g, msk ones %d"
          % (name, len(M.W), sum(v < 0 for v in M.LV), gap, int(M.msk.sum())))
    assert gap >= 1e-3
    assert M.W.min() >= -1e-12 and M.W.max() <= 1 + 1e-12
