"""The two callers of the shared mask rules (xfk_mask.hip) held to each other:
xfk_mag_make_mask on the meshes of magmaskref.rules_problem -- the smallest in
the tree at which every rule fires: an exterior edge, an on-axis node whose
score exceeds 1, a node shared by a selected and an unselected non-air element,
a point property -- and xfk_pot_make_mask on an electrostatic problem over the
same nodes, triangles, labels, length units and Precision, whose blocks are air
(ex = ey = 1, qv = 0) exactly where the magnetic label is and ex = 2 where it
is not; the same point-property nodes, no conductors, no selected nodes.

The magnetic lists are ascending and the potential's angle-sorted, the
magnetic flags come from the host's per-block loop and the potential's from
the block table's air test, so the comparison holds the rules' one copy to
both of its inputs.

Bounds: the 0 / 1 mask node by node; W to 1e-6, the tolerance
tests/test_gpu_magmask.py holds W to against its restatement (the two paths
derive the user-unit coordinates by different expressions, x / 0.1 and
x / 1., so W need not agree to the bit).  On the CPU first: both restatements
(maskref, magmaskref) accept the selection and refuse the invalid one, agree on
the mask, and the mask is neither all 0 nor all 1, no free node within 1e-4 of
the threshold.
"""
import numpy as np
import pytest

import electro
import magmaskref as MM
import magpostref as M
import maskref
import postproc
from xfemm_amd import kernels

pytestmark = pytest.mark.gpu

TOL_W = 1e-6      # tests/test_gpu_magmask.py
DEPTH = 12.0


def pair(axi):
    """The magnetic problem, the electrostatic one on the same mesh, and the restated masks, built once"""
    if axi in pair.cache:
        return pair.cache[axi]
    kw, A, ex = MM.rules_problem(axi=axi)
    R = M.MagPost(kw, A, depth=DEPTH, circuits=((1,), (0.,), (0.,)))
    K = MM.MagMask(R, ex["sel"], ex["max_area"], ex["block_not_air"])
    X, Y = M.user_xy(kw)
    u = electro.UNITS[kw["length_units"]]
    # one electrostatic block per magnetic label: air where MakeMask's lblflag is 0
    blocks = [dict(ex=2.0, ey=2.0, qv=0.0) if f else dict(ex=1.0, ey=1.0, qv=0.0) for f in K.lblflag]
    ekw = dict(x=X * u, y=Y * u, p=kw["p"], lbl=kw["lbl"], e=kw["e"], marker=kw["marker"], blocks=blocks,
               labels=[dict(block=k) for k in range(len(blocks))], points=[dict(V=0.0, qp=1e-9)],
               length_units=kw["length_units"], problem_type=kw["problem_type"], depth=DEPTH,
               precision=kw["precision"])
    V = np.random.default_rng(3).uniform(-1, 1, len(X))
    E = maskref.Mask(postproc.Post(ekw, V, "es"), ex["sel"], (), ex["max_area"])
    c = dict(kw=kw, A=A, ekw=ekw, V=V, K=K, E=E, **ex)
    pair.cache[axi] = c
    return c


pair.cache = {}


def check_on_the_cpu(c):
    K, E = c["K"], c["E"]
    assert np.array_equal(K.LV, E.LV) and np.array_equal(K.msk, E.msk)
    assert 0 < K.msk.sum() < len(K.msk)
    free = np.array(K.LV) < 0
    assert free.any() and np.abs(K.W - 0.5)[free].min() > 1e-4 and np.abs(E.W - 0.5)[free].min() > 1e-4
    with pytest.raises(MM.InvalidSelection):
        MM.MagMask(K.R, c["invalid_sel"], c["max_area"], c["block_not_air"])
    with pytest.raises(maskref.InvalidSelection):
        maskref.Mask(E.R, c["invalid_sel"], (), c["max_area"])


def devices(c):
    P = kernels.Static2DProblem(**c["kw"])
    P.set_solution(c["A"])
    P.set_depth(DEPTH)
    Q = kernels.ElectrostaticProblem(**c["ekw"])
    Q.set_solution(c["V"])
    return P, Q


def make_both(P, Q, c):
    m = P.make_mask(c["sel"], max_area=c["max_area"], block_not_air=c["block_not_air"])
    e = Q.make_mask(c["sel"], max_area=c["max_area"])
    return m, e


@pytest.mark.parametrize("axi", [False, True], ids=["planar", "axi"])
def test_the_two_callers_agree(axi):
    c = pair(axi)
    check_on_the_cpu(c)
    P, Q = devices(c)
    m, e = make_both(P, Q, c)
    print("W: magnetic vs potential %.3e; vs restated %.3e, %.3e; ones %d of %d" %
          (np.abs(m["W"] - e["W"]).max(), np.abs(m["W"] - c["K"].W).max(), np.abs(e["W"] - c["E"].W).max(),
           int(m["msk"].sum()), len(m["msk"])))
    assert np.array_equal(m["msk"], e["msk"])
    assert np.array_equal(m["msk"], c["K"].msk)
    assert np.abs(m["W"] - e["W"]).max() <= TOL_W
    P.close()
    Q.close()


@pytest.mark.parametrize("axi", [False, True], ids=["planar", "axi"])
def test_both_refuse_a_selection_abutting_a_non_air_label(axi):
    c = pair(axi)
    check_on_the_cpu(c)
    P, Q = devices(c)
    with pytest.raises(kernels.XfkError) as ei:
        P.make_mask(c["invalid_sel"], max_area=c["max_area"], block_not_air=c["block_not_air"])
    assert MM.INVALID in str(ei.value)
    with pytest.raises(kernels.XfkError) as ei:
        Q.make_mask(c["invalid_sel"], max_area=c["max_area"])
    assert maskref.INVALID in str(ei.value) and MM.INVALID not in str(ei.value)
    assert not P.mask_info()["ready"] and not Q.mask_info()["ready"]
    m, e = make_both(P, Q, c)
    assert P.mask_info()["ready"] and Q.mask_info()["ready"]
    assert np.array_equal(m["msk"], e["msk"]) and np.array_equal(m["msk"], c["K"].msk)
    assert np.abs(m["W"] - e["W"]).max() <= TOL_W
    P.close()
    Q.close()
