"""The weighted stress tensor mask and block integrals 5 and 6 on the device
(xfk_postproc.hip: xfk_pot_make_mask, xfk_pot_block_integral) against the
literal restatement of the reference (tests/maskref.py), its closed forms and
the reference's recorded output.

Bounds: the assembled mask system 1e-12 of its largest entry (the bound the
project holds assembled systems to); W 1e-6 of max |W| = 1 against the direct
solve (the bound it holds solved potentials to); the mask itself exactly, on
every node -- tests/test_mask_cpu.py shows that no node of these meshes comes
within 1e-3 of the threshold; the integrals 1e-12 of the sum of the absolute
terms against the restatement on the same mask, and 1e-12 of the closed form's
scale where one exists and the exact V is loaded; 5.1e-7 absolute against the
%f-printed recorded numbers."""

import numpy as np
import pytest
import scipy.sparse as sp

import electro
import maskref
import postproc
from test_postproc_cpu import TOL as TOL_PRINTED, load
from util import precision_bound, rel_err
from xfemm_amd import kernels

pytestmark = pytest.mark.gpu

TOL = 1e-12
TOL_W = 1e-6


def device(c, solved=False):
    P = kernels.ElectrostaticProblem(**c["kw"])
    if solved:
        P.solve()
    else:
        P.set_solution(c["V"])
    return P


def mask_args(c):
    return dict(selected_labels=c["sel"], selected_nodes=c["nsel"], max_area=c["max_area"])


def check_integrals(P, c, msk):
    """Types 5 and 6 against the restatement evaluated on the same mask."""
    F, T, scale = c["M"].integrals(msk)
    f = P.block_integral(c["sel"], 5)
    t = P.block_integral(c["sel"], 6)
    got = (f.real, f.imag, t.real)
    want = (F[0], F[1], T)
    for k in range(3):
        print("stress term %d: got %.15g want %.15g (sum |terms| %.3e)" % (k, got[k], want[k], scale[k]))
        assert abs(got[k] - want[k]) <= TOL * scale[k], k
    assert t.imag == 0
    return np.array(got)


@pytest.mark.parametrize("name", maskref.CASES)
def test_mask_and_integrals(name):
    c = maskref.case(name)
    M = c["M"]
    P = device(c)
    r = P.make_mask(**mask_args(c))
    # the assembled system
    rp, col, val, b = P.mask_csr()
    n = len(rp) - 1
    G = sp.csr_matrix((val, col, rp), shape=(n, n)).toarray()
    ea, eb = np.abs(G - M.A).max() / np.abs(M.A).max(), np.abs(b - M.b).max() / max(np.abs(M.b).max(), 1e-300)
    print("%s: mask system A %.3e b %.3e; PCG %d iterations; times %s" % (name, ea, eb, r["cg_iters"], r["times"]))
    assert ea <= TOL and eb <= TOL
    # W, and the mask on every node
    ew = np.abs(r["W"] - M.W).max()
    print("W: err %.3e of max |W| = 1; min |W - 0.5| %.4g" % (ew, np.abs(M.W - 0.5).min()))
    assert ew <= TOL_W
    assert r["msk"].shape == (n,) and np.array_equal(r["msk"], M.msk)
    got = check_integrals(P, c, r["msk"])
    if c["closed"] is not None:
        cl = c["closed"]
        print("closed form: force %r torque %.15g" % (cl["force"], cl["torque"]))
        assert np.abs(got[:2] - cl["force"]).max() <= TOL * cl["scale"]
        assert abs(got[2] - cl["torque"]) <= TOL * cl["scale"]
    if c["R"].axi:
        assert got[0] == 0 and got[2] == 0
    P.close()


def test_fixture_recorded_lines():
    """Lines 6 and 7 of the reference's recorded epproc output."""
    c = maskref.case("fixture")
    _, chk, _ = load("test")
    P = device(c)
    w = P.weighted_stress(**mask_args(c))
    l6, l7 = chk["integrals"][5][1], chk["integrals"][6][1]
    print("force %r torque %r; recorded %r %r" % (w["force"], w["torque"], l6, l7))
    assert abs(w["force"][0] - l6[0]) <= TOL_PRINTED and abs(w["force"][1] - l6[1]) <= TOL_PRINTED
    assert abs(w["torque"] - l7[0]) <= TOL_PRINTED and abs(0. - l7[1]) <= TOL_PRINTED
    P.close()


@pytest.mark.parametrize("name", ["cap_planar", "cap_axi"])
def test_solved_capacitor(name):
    """The capacitor solved on the device, not loaded: the force within the
    bound the project holds a solved potential to against the exact one
    (util.precision_bound of the exact V and the direct solve, 1e-6), relative
    to the closed form."""
    c = maskref.case(name)
    Vd = electro.restate(c["kw"])["V"][:len(c["V"])]
    bound = precision_bound(c["V"], Vd, TOL_W)
    P = device(c, solved=True)
    print("solved V vs exact: %.3e (bound %.3e)" % (rel_err(P.solution(), c["V"]), bound))
    w = P.weighted_stress(**mask_args(c))
    cl = c["closed"]
    err = np.abs(w["force"] - cl["force"]).max() / cl["scale"]
    print("force %r closed %r: %.3e" % (w["force"], cl["force"], err))
    assert err <= bound
    assert np.array_equal(P.make_mask(**mask_args(c))["msk"], c["M"].msk)
    P.close()


def test_refusals_and_state():
    c = maskref.case("free_body")
    sel = c["sel"]
    P = device(c)
    with pytest.raises(kernels.XfkError, match="types 5 and 6"):
        P.block_integral(sel, 5)
    with pytest.raises(kernels.XfkError, match="no mask"):
        kernels._check(kernels._lib.xfk_pot_get_mask(P._h, None, None))
    before = P.block_integrals([0, 1])["raw"].copy()
    P.make_mask(sel)
    w = P.weighted_stress(sel)
    f, t = P.block_integral(sel, 5), P.block_integral(sel, 6)
    assert np.array([f.real, f.imag]).tobytes() == w["force"].tobytes()
    assert np.float64(t.real).tobytes() == np.float64(w["torque"]).tobytes()
    # a mixed call: integrals 0-4 keep their bits, and types 5 and 6 theirs
    assert P.block_integrals([0, 1])["raw"].tobytes() == before.tobytes()
    assert P.block_integral(sel, 5) == f
    # another selection: refused until its own mask is made
    with pytest.raises(kernels.XfkError, match="types 5 and 6"):
        P.block_integral([0, 1], 5)
    with pytest.raises(kernels.XfkError, match="xfk_pot_make_mask"):
        P.block_integral([0], 6)
    # a new solution drops the mask
    P.set_solution(c["V"])
    assert not P.mask_info()["ready"]
    with pytest.raises(kernels.XfkError, match="types 5 and 6"):
        P.block_integral(sel, 5)
    assert P.weighted_stress(sel)["force"].tobytes() == w["force"].tobytes()
    # an invalid selection: the reference's message, and the problem stays usable
    with pytest.raises(kernels.XfkError, match="The selected region is invalid. A valid selection cannot abut a "
                                               "region which is not free space."):
        P.make_mask([0])
    assert not P.mask_info()["ready"]
    with pytest.raises(kernels.XfkError, match="types 5 and 6"):
        P.block_integral([0], 5)
    assert P.weighted_stress(sel)["force"].tobytes() == w["force"].tobytes()
    assert P.block_integrals([0, 1])["raw"].tobytes() == before.tobytes()
    with pytest.raises(ValueError):
        P.make_mask(sel, max_area=[1.0])
    P.close()


def test_two_runs_give_the_same_bits():
    c = maskref.case("rules")
    runs = []
    for _ in range(2):          # a second problem: the auxiliary problem built again
        P = device(c)
        for _ in range(2):      # and the mask made twice on each
            r = P.make_mask(**mask_args(c))
            runs.append((r["W"], r["msk"], P.mask_csr()[2], np.array([P.block_integral(c["sel"], 5)]),
                         np.array([P.block_integral(c["sel"], 6)])))
        P.close()
    for r in runs[1:]:
        for a, b in zip(runs[0], r):
            assert a.tobytes() == b.tobytes()


def test_heat_flow_refuses():
    kw, V = postproc.synthetic(7, 7, False, "hf")
    P = kernels.HeatFlowProblem(**kw)
    P.set_solution(V)
    assert not hasattr(P, "make_mask") and not hasattr(P, "weighted_stress")
    with pytest.raises(kernels.XfkError, match="types 5 and 6"):
        P.block_integral([0], 5)
    sel = np.ones(len(kw["labels"]), np.uint8)
    import ctypes as C
    rc = kernels._lib.xfk_pot_make_mask(P._h, sel.ctypes.data_as(C.POINTER(C.c_ubyte)), None, None)
    assert rc == -1 and b"electrostatic problems" in kernels._lib.xfk_last_error()
    P.close()
