"""The restated Newton pass (tests/newtonref.py) checked on the host: against
the oracle at iteration 0, against a difference quotient of its own secant
system, against the oracle's converged solution, and the branches the device
test's problems reach (tests/newtonzoo.py).  No device."""
import os
import re

import numpy as np
import pytest

import newtonref as nr
import newtonzoo as zoo
from oracle import oracle
from util import C_ANS, ROOT, rel_err, synth_to_oracle
from xfemm_amd import synth

LD = np.longdouble
CSRC = os.path.join(ROOT, "xfemm_amd", "csrc")


def constant(name):
    m = re.search(r"constexpr int %s = (\d+);" % name, open(os.path.join(CSRC, "xfk_device.hip")).read())
    assert m, "%s not found in xfk_device.hip" % name
    return int(m.group(1))


MAKERS = {"magnetostatic": lambda nl=False: synth.magnetostatic(12, nonlinear=nl),
          "bc_showcase": lambda nl=False: synth.bc_showcase(12, nonlinear=nl),
          "axisymmetric": lambda nl=False: synth.axisymmetric(12, nonlinear=nl)}


@pytest.mark.parametrize("maker", sorted(MAKERS))
def test_iteration_0_matches_the_oracle(maker):
    """The first pass's free-free entries and free rows of b (the prescribed
    values moved to the right side) equal oracle.system, which is pinned bit
    for bit to the reference's goldens, within 1e-12 max|K|."""
    pr, mesh, kw = synth_to_oracle(MAKERS[maker]())
    P = nr.prepare(kw)
    r = nr.newton_pass(P, first=True)
    O, bo = oracle.system(pr, mesh)
    O = O.toarray()
    free = nr.free_nodes(P)
    assert free.sum() > 50
    fx = np.array(sorted(P.fixed), int)
    xv = np.array([P.fixed[i] for i in fx])
    K = np.asarray(r["K"], float)
    b = np.asarray(r["b"] - r["K"][:, fx] @ xv.astype(LD), float)
    assert abs(K - O)[np.ix_(free, free)].max() <= 1e-12 * abs(O).max()
    assert abs(b - bo)[free].max() <= 1e-12 * abs(bo).max()
    # and the bound the device is held to is no looser than that tolerance
    assert r["Kb"][np.ix_(free, free)].max() <= 1e-12 * abs(O).max()


def _first(kw):
    P = nr.prepare(kw)
    r = nr.newton_pass(P, first=True)
    return P, (r["mu1"], r["mu2"])


def _iterate(kw, P):
    """A seeded smooth field with 1.6 T at most in the steel, and a direction."""
    V = zoo.chains(kw, P)[5][0]
    w = np.random.default_rng(3).normal(size=P.N) * np.abs(V).max()
    return V, (w * P.x if P.axi else w)


def _quotient(P, state, V, w):
    """-> (max |K w - D|, the quotient's own error margin, max |Mn w|) with D
    the central difference of V -> K_secant(V) V along w at h / 2, h = 1e-5."""
    def f(X):
        return nr.newton_pass(P, X, state, newton_terms=False)["K"] @ np.asarray(X, LD)

    def D(h):
        return (f(V + h * w) - f(V - h * w)) / (2 * h)

    h = LD(1e-5)
    full = nr.newton_pass(P, V, state)
    sec = nr.newton_pass(P, V, state, newton_terms=False)
    Jw = full["K"] @ np.asarray(w, LD)
    mn = np.abs((full["K"] - sec["K"]) @ np.asarray(w, LD)).max()
    d1, d2 = D(h), D(h / 2)
    margin = np.abs(d1 - d2).max() + 2 * (full["Kb"] @ np.abs(V).astype(LD)).max() * LD(2.0) ** -11 / (h / 2)
    return np.abs(Jw - d2).max(), margin, mn


@pytest.mark.parametrize("fill", [0.98, 0.5])
@pytest.mark.parametrize("maker", ["magnetostatic", "axisymmetric"])
def test_newton_terms_are_the_derivative_lam_type_0(maker, fill):
    """K (the pass's full matrix, Mn included) times w equals the central
    difference of V -> K_secant(V) V along w, K_secant being the same pass with
    Mn left out: Mn is the derivative of the secant matrix.  The margin is the
    quotient's own error: D(h) - D(h / 2) is 3/4 of D(h)'s truncation error
    h^2 f''' / 6, i.e. three times that of D(h / 2), which is what is compared
    (B-H knots crossed inside the stencil enlarge both alike); the rounding of
    the quotient is 2 fb 2^-11 / h with fb the f64 bound of K V, the longdouble
    evaluation being 2^-11 of it."""
    kw = zoo.variant(MAKERS[maker](True), 0, fill, extras=False)
    P, state = _first(kw)
    V, w = _iterate(kw, P)
    err, margin, mn = _quotient(P, state, V, w)
    print("lam 0 fill %g %s: |K w - D| %.3e, margin %.3e, Mn's share %.3e" % (fill, maker, err, margin, mn))
    assert margin < 1e-4 * mn      # the quotient resolves Mn to four digits
    assert err <= margin


@pytest.mark.parametrize("lam_type, fill", [(1, 0.98), (1, 0.5), (2, 0.98), (2, 0.5)])
@pytest.mark.parametrize("maker", ["magnetostatic", "axisymmetric"])
def test_newton_terms_laminated(maker, lam_type, fill):
    """The reference's laminated Newton terms Kn (v u' + u v') are NOT the
    derivative of the secant matrix: measured with the quotient of the test
    above (its own error below 3e-5 of Mn w) on the makers of this file
    (n = 12) at the 1.6 T random iterate, max |K w - D| / max |Mn w| is 0.009
    to 0.054 at fill 0.98 and 0.74 to 6.7 at fill 0.5; each case prints its
    own and asserts that the quotient resolves it.  The symmetrised product is a
    Newton-like term that keeps the matrix symmetric; it is the reference's
    formula and the device's, so what is asserted is what the formula
    promises: Mn symmetric to the bit and be - be_0 = Mn V, so that the fixed
    point does not depend on Mn."""
    kw = zoo.variant(MAKERS[maker](True), lam_type, fill, extras=False)
    P, state = _first(kw)
    V, w = _iterate(kw, P)
    err, margin, mn = _quotient(P, state, V, w)
    print("lam %d fill %g %s: |K w - D| / |Mn w| %.4f (the quotient's own error %.1e of |Mn w|)"
          % (lam_type, fill, maker, err / mn, margin / mn))
    assert margin < 1e-4 * mn and err > 100 * margin      # a gap the quotient resolves
    full = nr.newton_pass(P, V, state)
    sec = nr.newton_pass(P, V, state, newton_terms=False)
    steel = P.blk == zoo.STEEL
    Mn = full["Mn"]
    assert max(np.abs(Mn[j][k].v[steel]).max() for j in range(3) for k in range(3)) > 0
    for j in range(3):
        for k in range(3):
            assert np.array_equal(Mn[j][k].v, Mn[k][j].v)
    KMn, dbe = full["K"] - sec["K"], full["b"] - sec["b"]
    # (both sides are sums of the same products: equal up to longdouble rounding)
    assert np.abs(dbe - KMn @ np.asarray(V, LD)).max() <= 1e-15 * (np.abs(KMn) @ np.abs(V).astype(LD)).max()


@pytest.mark.parametrize("maker", ["magnetostatic", "axisymmetric"])
def test_converged_solution_matches_the_oracle(maker):
    """Reference passes with a direct solve of the free rows, relaxed as
    static2d_run and the oracle relax (static2d.cpp:960-1010), reach
    oracle.solve's A within the suite's 1e-5 max|A|."""
    pr, mesh, kw = synth_to_oracle(MAKERS[maker](True))
    P = nr.prepare(kw)
    assert all(v == 0 for v in P.fixed.values()) and not len(P.pbc)
    free = nr.free_nodes(P)
    r = nr.newton_pass(P, first=True)
    V, relax, res, it = np.zeros(P.N), 1.0, 0.0, 0
    while True:
        Vold = V
        V = np.zeros(P.N)
        V[free] = np.linalg.solve(np.asarray(r["K"], float)[np.ix_(free, free)], np.asarray(r["b"], float)[free])
        last, res = res, np.sqrt(((V - Vold) ** 2).sum() / (V ** 2).sum())
        if it > 5:
            relax = relax / 2 if (res > last and relax > 0.125) else relax + 0.1 * (1 - relax)
            V = relax * V + (1 - relax) * Vold
        it += 1
        if res < 100 * kw["precision"] and it > 1:
            break
        assert it < 60
        r = nr.newton_pass(P, V, (r["mu1"], r["mu2"]))
    A = V * C_ANS
    if P.axi:
        A = A * P.x * 0.01 * 2 * np.pi
    Ao = oracle.solve(pr, mesh)[0]
    print("%s: %d passes, distance to the oracle %.3e" % (maker, it, rel_err(A, Ao)))
    assert rel_err(A, Ao) <= 1e-5


def test_zoo_reaches_every_branch():
    """The device test's problems and iterates reach every arm of the Newton
    pass; asserted on the reference's per-element record so that a change of
    the problems cannot quietly stop reaching one."""
    row_acc, row_block = constant("kRowAcc"), constant("kRowBlock")
    seen = set()
    for name, kw in zoo.problems():
        P = nr.prepare(kw)
        assert all(v == 0 for v in P.fixed.values()), name
        axi = "axi" if P.axi else "planar"
        n_tab = len(kw["blocks"][zoo.STEEL]["B"])
        steel = P.blk == zoo.STEEL
        lam = int(kw["blocks"][zoo.STEEL]["LamType"])
        if P.N > row_block:
            free = np.nonzero(nr.free_nodes(P))[0]
            if (free < row_block).any() and (free >= row_block).any():
                seen.add("rows on both sides of a kRowBlock boundary")
        if P.external.any():
            seen.add("external")
        if any(c[0] == 1 for c in P.circ):
            seen.add("circuit case 1")
        if P.mixed.any():
            seen.add("mixed " + axi)
        for chain in zoo.chains(kw, P):
            passes = nr.chain(P, chain)
            for k, r in enumerate(passes[1:]):
                br, kind = r["branch"], r["kind"]
                on = kind == "on"
                assert on[steel].all()
                seen.add(("table", axi, lam))
                if (r["B"].v[on] == 0).any():
                    assert (r["dv"].v[on & (r["B"].v == 0)] == 0).all()
                    seen.add("B == 0")
                if (br[on] == n_tab - 1).any():
                    seen.add(("past the last knot", axi))
                if (br[on] == 0).any():
                    seen.add("first interval")
                if ((br[on] > 0) & (br[on] < n_tab - 2)).any():
                    seen.add("middle interval")
                if (br[on] == n_tab - 2).any():
                    seen.add("last interval")
                off = kind == "off"
                if off.any():
                    assert (P.lam[off] == 0).all() and (P.mu_x[off] != P.mu_y[off]).all()
                    assert np.array_equal(r["mu1"].v[off], passes[0]["mu1"].v[off])
                    seen.add("Newton off, state kept")
                lin = kind == "linear"
                assert np.array_equal(r["mu1"].v[lin], passes[0]["mu1"].v[lin])
                assert np.array_equal(r["mu2"].v[lin], passes[0]["mu2"].v[lin])
                if (P.bhn[lin] == 0).any():
                    seen.add("linear block")
                if (lin & (P.lam > 2) & (P.bhn > 0)).any():
                    seen.add("type > 2 with a table")
                if k > 0:
                    seen.add("a pass that reads a Newton pass's state")
                # a nonlinear element on a row the device accumulates in place
                rows = np.count_nonzero(r["K"], axis=1)
                long_rows = np.nonzero(rows > row_acc)[0]
                if np.isin(P.p[on], long_rows).any() and (r["B"].v[on & np.isin(P.p, long_rows).any(axis=1)] > 0).any():
                    seen.add("nonlinear element on a row longer than kRowAcc")
    want = {"B == 0", "first interval", "middle interval", "last interval", "Newton off, state kept", "linear block",
            "type > 2 with a table", "a pass that reads a Newton pass's state", "external", "circuit case 1",
            "mixed planar", "mixed axi", "rows on both sides of a kRowBlock boundary",
            "nonlinear element on a row longer than kRowAcc", ("past the last knot", "planar"),
            ("past the last knot", "axi")}
    want |= {("table", a, t) for a in ("planar", "axi") for t in (0, 1, 2)}
    assert not (want - seen), "not reached: %r" % sorted(map(str, want - seen))
