"""The device's Newton-pass element assembly (xfk_device.hip: get_bh_props,
planar_newton_state / planar_newton_terms / k_planar_state, the PRE arm of
assemble_rows, the !FIRST half of axi_element, the mu1 / mu2 double buffer of
assemble()) against the longdouble restatement tests/newtonref.py, evaluated
at the same chosen iterates (tests/newtonzoo.py) through
Static2DProblem.assemble_at: every free-free matrix entry, every free row of
b and every element's new state within the restatement's per-entry rounding
bound.  The converged solution cannot see these terms: Mn enters Me and be
consistently, so the fixed point does not depend on it.

Largest |device - reference| / bound measured (MI355X), over every problem
and chain: matrix 0.203, b 0.072, state 0.608 -- each case prints its own;
the bound is derived in newtonref, not fitted to these."""
import ctypes as C

import numpy as np
import pytest

import electro
import newtonref as nr
import newtonzoo as zoo
from util import synth_to_oracle
from xfemm_amd import kernels, synth

pytestmark = pytest.mark.gpu

PROBLEMS = zoo.problems()


def _ratio(err, bound):
    """max err / bound; an entry with bound 0 must be exact."""
    err, bound = np.asarray(err, float), np.asarray(bound, float)
    assert (err[bound == 0] == 0).all()
    m = bound > 0
    return float((err[m] / bound[m]).max()) if m.any() else 0.0


def _compare(P, ref, r, first_state, label):
    """One assembled pass on the device against the reference's pass r."""
    rp, col, val, b = P.csr()
    free = nr.free_nodes(ref)
    rows = np.repeat(np.arange(ref.N), np.diff(rp))
    ff = free[rows] & free[col]
    # the device's pattern holds every entry the reference fills
    pat = np.zeros((ref.N, ref.N), bool)
    pat[rows, col] = True
    assert not ((r["K"] != 0) & ~pat).any()
    eK = np.abs(val.astype(nr.LD) - r["K"][rows, col])[ff]
    eb = np.abs(b.astype(nr.LD) - r["b"])[free]
    qK, qb = _ratio(eK, r["Kb"][rows, col][ff]), _ratio(eb, r["bb"][free])
    mu1, mu2 = P.element_state()
    on = r["kind"] == "on"
    e1, e2 = np.abs(mu1.astype(nr.LD) - r["mu1"].v), np.abs(mu2.astype(nr.LD) - r["mu2"].v)
    qs = max(_ratio(e1, r["mu1"].e), _ratio(e2, r["mu2"].e))
    print("%s: error / bound: matrix %.3f b %.3f state %.3f" % (label, qK, qb, qs))
    assert qK <= 1 and qb <= 1 and qs <= 1, label
    if first_state is not None:      # linear and Newton-off elements: carried to the bit
        assert np.array_equal(mu1[~on], first_state[0][~on]) and np.array_equal(mu2[~on], first_state[1][~on])
    return val, b, mu1, mu2


@pytest.mark.parametrize("name, kw", PROBLEMS, ids=[n for n, _ in PROBLEMS])
def test_newton_pass_matches_the_reference(name, kw, monkeypatch):
    ref = nr.prepare(kw)
    assert all(v == 0 for v in ref.fixed.values())    # the Dirichlet step leaves free rows alone
    P = kernels.Static2DProblem(**kw)
    P.assemble_at([])
    first = nr.newton_pass(ref, first=True)
    _, _, m1, m2 = _compare(P, ref, first, None, name + " pass 0")
    got = []
    chains = zoo.chains(kw, ref)
    for c, chain in enumerate(chains):
        r = nr.chain(ref, chain)[-1]
        P.assemble_at(chain)
        got.append(_compare(P, ref, r, (m1, m2), "%s chain %d (%d)" % (name, c, len(chain))))
        assert (r["kind"] == "on").any()
    P.close()
    # the scan arm of the table lookup: the same systems and states to the bit
    monkeypatch.setenv("XFK_BH_SCAN", "1")
    Q = kernels.Static2DProblem(**kw)
    for chain, g in zip(chains, got):
        Q.assemble_at(chain)
        for a, bb in zip(Q.csr()[2:] + Q.element_state(), g):
            assert np.array_equal(a.view(np.int64), bb.view(np.int64))
    Q.close()


PLANAR = [(n, kw) for n, kw in PROBLEMS if kw.get("problem_type", 0) == 0]


@pytest.mark.parametrize("name, kw", PLANAR, ids=[n for n, _ in PLANAR])
def test_state_arms_give_the_same_bits(name, kw, monkeypatch):
    """The Newton state evaluated once per element (k_planar_state, the
    default) and once per row (XFK_ASM_STATE=0): the same system and state to
    the bit.

    This test found a difference: before planar_element wrote the sum of two
    products Mx / m2 + My / m1 as an explicit fma, 5 of these 12 problems gave
    matrices 1-4 ulp apart in 1-15 entries (b and the state to the bit), also
    at B == 0 where Mn == 0: k_assemble_rows_pre and k_assemble_rows<false,
    false> are separate compilations of planar_element, and which of the two
    products the backend fused differed between them."""
    ref = nr.prepare(kw)
    chains = zoo.chains(kw, ref)
    out = []
    for arm in ("1", "0"):
        monkeypatch.setenv("XFK_ASM_STATE", arm)
        P = kernels.Static2DProblem(**kw)
        got = []
        for chain in chains:
            P.assemble_at(chain)
            got.append(P.csr()[2:] + P.element_state())
        P.close()
        out.append(got)
    bad = [0, 0, 0, 0]
    for c, (g1, g0) in enumerate(zip(*out)):
        for q, (a, b) in enumerate(zip(g1, g0)):
            d = np.abs(a.view(np.int64) - b.view(np.int64))
            bad[q] += int((d != 0).sum())
            if d.any():
                print("%s chain %d %s: %d of %d differ, %d ulp at most" %
                      (name, c, ("matrix", "b", "mu1", "mu2")[q], (d != 0).sum(), d.size, d.max()))
    assert bad == [0, 0, 0, 0]


@pytest.mark.parametrize("maker", ["planar", "axi"])
def test_probe_leaves_the_solve_alone(maker):
    """solve() after assemble_at gives the bits of a solve without it, and
    assemble_at after a solve the bits of one before it."""
    kw = (synth.magnetostatic(12, nonlinear=True) if maker == "planar" else synth.axisymmetric(10, nonlinear=True))
    pr, mesh, kw = synth_to_oracle(kw)
    ref = nr.prepare(kw)
    chain = zoo.chains(kw, ref)[7]
    P = kernels.Static2DProblem(**kw)
    r0 = P.solve()
    A0 = P.solution()
    P.close()
    P = kernels.Static2DProblem(**kw)
    P.assemble_at(chain)
    sys0 = P.csr()[2:] + P.element_state()
    r1 = P.solve()
    A1 = P.solution()
    assert (r0["newton_iters"], r0["cg_iters"]) == (r1["newton_iters"], r1["cg_iters"]) and r0["newton_iters"] > 1
    assert np.array_equal(A0.view(np.int64), A1.view(np.int64))
    P.assemble_at(chain)
    for a, b in zip(sys0, P.csr()[2:] + P.element_state()):
        assert np.array_equal(a.view(np.int64), b.view(np.int64))
    P.close()


def test_refusals():
    L = kernels.load_library()
    V = np.zeros(4096)
    vp, dp = V.ctypes.data_as(kernels.dptr), V.ctypes.data_as(kernels.dptr)

    def refused(h, code, word):
        assert L.xfk_static2d_assemble_at(h, 1, vp) == code
        assert word in L.xfk_last_error().decode()
        assert L.xfk_get_element_state(h, dp, dp) == code
        assert word in L.xfk_last_error().decode()

    refused(None, -1, "null")
    x, y, p = electro.grid(5, 4, 4.0, 3.0)
    e = electro.tag_edges(x, y, p, [(lambda xa, ya, xb, yb: xa == 0 and xb == 0, 0)])
    base = dict(x=x, y=y, p=p, e=e, lbl=np.zeros(len(p), np.int32), labels=[dict(block=0)], length_units=3)
    E = kernels.ElectrostaticProblem(**base, blocks=[dict(ex=3.0, ey=7.0)], lines=[dict(format=0, V=1.0)], depth=1.0)
    refused(E._h, -1, "electrostatic")
    E.close()
    H = kernels.HeatFlowProblem(**base, blocks=[dict(kx=2.0, ky=2.0)], lines=[dict(format=0, Tset=300.0)], depth=1.0)
    refused(H._h, -1, "heat-flow")
    H.close()
    A = kernels.Harmonic2DProblem(**synth_to_oracle(synth.harmonic(8))[2])
    refused(A._h, -1, "harmonic")
    A.close()
    kw = synth.magnetostatic(8)
    (comm,) = kernels.Comm.local_group(1)
    S = kernels.Static2DProblem(**kw, comm=comm)
    refused(S._h, -5, "sharded")
    S.close()
    M = kernels.Static2DProblem(**kw)
    M.solve()
    M.make_mask([4])
    h = C.c_void_p()
    assert L.xfk_mag_mask_problem(M._h, C.byref(h)) == 0
    refused(h, -1, "mask")
    # a linear problem assembles, and keeps no state
    M.assemble_at([np.zeros(M.n_nodes)])
    with pytest.raises(kernels.XfkError, match="linear"):
        M.element_state()
    with pytest.raises(kernels.XfkError, match="n_nodes"):
        M.assemble_at([np.zeros(3)])
    assert L.xfk_static2d_assemble_at(M._h, -1, vp) == -1 and L.xfk_static2d_assemble_at(M._h, 1, None) == -1
    M.close()
