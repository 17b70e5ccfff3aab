"""The restatement of fpproc's weighted stress tensor integrals 18-23
(tests/magmaskref.py) held to closed forms (CPU only).  No reference program
records a value of these types (fpproc's main computes one and prints nothing),
so the device tests' parity rests on what is asserted here.

The bound of the identities is 1e-12 of the sum of the absolute terms of the
integral: the terms are sums of a few hundred products of O(1) factors in
double, and the potential they start from is solved directly and refined
against a long-double residual (magmaskref.solve_planar).
"""
import numpy as np
import pytest

import magmaskref as MM
import magpostref as M

BOUND = 1e-12
NO_CIRC = ((1,), (0.,), (0.,))    # the circuit columns of rules_problem's one circuit (not read by 18-23)


@pytest.mark.parametrize("length_units", [1, 0], ids=["mm", "inch"])
@pytest.mark.parametrize("max_area", [None, (0.5, 2.0)], ids=["elem_area", "max_area"])
def test_layered_strip_closed_form(length_units, max_area):
    """F_x = depth h (B_L^2 - B_R^2) / (2 mu0): the Maxwell stress -B_y^2 / (2 mu0)
    on the slab's faces with outward normals -x and +x, which is type 11's
    Lorentz force -J B_y (mu0 J = dB_y/dx), whatever the mask's shape; F_y and
    the torque about the slab's centre line vanish; 20 / 21 / 23 are half of
    18 / 19 / 22."""
    kw, A, info = MM.layered_strip(length_units=length_units)
    R = M.MagPost(kw, A, depth=info["depth"])
    K = MM.MagMask(R, info["sel"], max_area)
    z, sc = K.integrals()
    F, BL, BR = MM.strip_closed_form(R, info)
    lorentz = R.block_integrals(info["sel"])[0][11].real
    print("Fx %.17g closed %.17g lorentz %.17g scale %.3g; Fy %.3g T %.3g; B_L %.6g B_R %.6g" %
          (z[0], F, lorentz, sc[0], z[1], z[4], BL, BR))
    assert abs(BL) != abs(BR) and F != 0
    # B is uniform in each air layer
    B = R.element_b_all()
    air = np.flatnonzero(np.asarray(kw["lbl"]) == 0)
    cx = R.X[R.p[air]].mean(axis=1)
    for side, b in ((cx < 0, BL), (cx > 0, BR)):
        assert np.abs(B[air[side], 1] - b).max() <= 1e-12 * abs(b) and np.abs(B[air[side], 0]).max() <= 1e-12 * abs(b)
    assert abs(z[0] - F) <= BOUND * sc[0]
    assert abs(z[0] - lorentz) <= BOUND * sc[0]
    assert abs(z[1]) <= BOUND * sc[1]
    assert abs(z[4]) <= BOUND * sc[4]
    assert np.all(np.abs(z[[2, 3, 5]] - z[[0, 1, 4]] / 2.) <= BOUND * sc[[0, 1, 4]])
    # the mask is not the slab's indicator: the identity did not hold trivially
    assert 0 < K.msk.sum() and np.any((K.msk == 1) & (np.array(K.LV) < 0))


def test_axisymmetric_types_are_zero():
    kw, A, ex = MM.rules_problem(axi=True)
    R = M.MagPost(kw, A, circuits=NO_CIRC)
    z, sc = MM.MagMask(R, ex["sel"], ex["max_area"], ex["block_not_air"]).integrals()
    assert z[0] == 0 and z[2] == 0 and z[4] == 0 and z[5] == 0
    assert z[1] != 0 and abs(z[3] - z[1] / 2.) <= BOUND * sc[1]


def _rules(axi):
    kw, A, ex = MM.rules_problem(axi)
    R = M.MagPost(kw, A, depth=12.0, circuits=NO_CIRC)
    return kw, R, ex, MM.MagMask(R, ex["sel"], ex["max_area"], ex["block_not_air"])


def test_rules_planar():
    kw, R, ex, K = _rules(False)
    LV = np.array(K.LV)
    lbl, p, mk = np.asarray(kw["lbl"]), np.asarray(kw["p"]), np.asarray(kw["marker"])
    # a circuit label that is air by its material, and the block only block_not_air marks: not air
    assert K.lblflag == [0, 1, 1, 1, 1, 1]
    assert np.all(LV[p[lbl == 2]] == 0) and np.all(LV[p[lbl == 3]] == 0)
    without = MM.MagMask(R, ex["sel"], ex["max_area"], None)
    assert np.any(np.array(without.LV)[p[lbl == 3]] < 0)
    # the point properties: a free node becomes 0, a body node stays 1, a boundary node stays 0
    pts = np.flatnonzero(mk >= 0)
    assert sorted(LV[pts]) == [0., 0., 1.]
    nomark = dict(kw, marker=None)
    LV0 = np.array(MM.MagMask(M.MagPost(nomark, R.A, circuits=NO_CIRC), ex["sel"], ex["max_area"],
                              ex["block_not_air"]).LV)
    assert sorted(LV0[pts]) == [-1., 0., 1.]
    # a node shared by the body and the higher-numbered iron ends at 0
    shared = np.intersect1d(p[lbl == 1], p[lbl == 4])
    assert len(shared) == 3 and np.all(LV[shared] == 0)
    assert np.flatnonzero(lbl == 4).min() > np.flatnonzero(lbl == 1).max()
    # free nodes remain, none near the threshold
    free = LV < 0
    assert free.sum() > 10 and np.abs(K.W - 0.5)[free].min() > 1e-4
    # the invalid selection
    with pytest.raises(MM.InvalidSelection) as ei:
        MM.MagMask(R, ex["invalid_sel"], ex["max_area"], ex["block_not_air"])
    assert str(ei.value) == MM.INVALID


def test_rules_on_axis():
    kw, R, ex, K = _rules(True)
    assert K.on_axis
    LV = np.array(K.LV)
    axis = np.flatnonzero(R.X < 1e-6)
    kosher = [k for k in axis if K.is_kosher(k)]
    assert len(kosher) == 2 and len(axis) > 4            # the two ends of the axis
    assert np.all(LV[kosher] == 0)
    body = np.unique(np.asarray(kw["p"])[np.asarray(kw["lbl"]) == 1])
    inner = [k for k in axis if k not in kosher and k not in body]
    assert len(inner) > 0 and np.all(LV[inner] == -1)     # exterior-edge ends that stay free
    assert np.all(LV[np.intersect1d(axis, body)] == 1)
    # with the selection off the axis the same nodes are zeroed
    K2 = MM.MagMask(R, [3], ex["max_area"], ex["block_not_air"])
    assert not K2.on_axis and np.all(np.array(K2.LV)[inner] == 0)
    free = LV < 0
    assert np.abs(K.W - 0.5)[free].min() > 1e-4


def test_free_body_gap_shrinks():
    """Weighted stress force against the Lorentz force (types 11 / 12) on one of
    two conductors in air: a discretisation-level check.  Measured,
    |F_ws - F_lorentz| / |F_lorentz|: 3.52e-2 at 8 cells a side (n = 4),
    8.08e-3 at 16 (n = 8); the torques 1.91e-3 against 1.94e-3 N m and 1.956e-3
    against 1.968e-3.  Asserted: the gap shrinks."""
    gap = []
    for n in (4, 8):
        kw, A = MM.free_body(n)
        R = M.MagPost(kw, A, depth=10.0)
        z, _ = MM.MagMask(R, [1]).integrals()
        zz, _ = R.block_integrals([1])
        F = np.array([zz[11].real, zz[12].real])
        gap.append(np.linalg.norm(z[:2] - F) / np.linalg.norm(F))
        print("n %d weighted stress %s lorentz %s gap %.3e torque %.4e / %.4e" % (n, z[:2], F, gap[-1], z[4],
                                                                                  zz[15].real))
    assert gap[1] < gap[0]
