"""The restated AMG reference (tests/amgref.py) checked against itself: no
device.  Hierarchies come from the restated setup rules with greedy
distance-2 aggregates and the exact inverse on the coarsest level."""
import numpy as np
import pytest

import amgref
from util import _laplace_random

# a cycle is ~10 sparse products per level, each entry a sum of <= 16 terms:
# a few hundred roundings of 2^-53 relative to the largest entry
TOL = 2048 * 2.0 ** -53


@pytest.fixture(scope="module")
def hier():
    A = _laplace_random(20, 3)                 # 400 rows
    return A, amgref.build_reference_hierarchy(A, coarse=16)


def _plain(levels):
    return [dict(L, fold=False) for L in levels]


def test_hierarchy_is_deep(hier):
    A, levels = hier
    assert len(levels) >= 4 and levels[-1]["A"].shape[0] <= 16


@pytest.mark.parametrize("nu", [1, 2, 3])
def test_plain_cycle_is_symmetric(hier, nu):
    A, levels = hier
    U = amgref.cycle(_plain(levels), np.eye(A.shape[0]), nu=nu)
    assert np.abs(U - U.T).max() <= TOL * np.abs(U).max()


def test_folded_cycle_equals_plain_cycle(hier):
    A, levels = hier
    I = np.eye(A.shape[0])
    Up = amgref.cycle(_plain(levels), I)
    Uf = amgref.cycle(levels, I)
    assert np.abs(Up - Uf).max() <= TOL * np.abs(Up).max()
    # the W-cycle's second visit adds onto the first: also symmetric
    W = [dict(L) for L in levels]
    assert len(W) >= 4                          # (level 1 has a non-coarsest child)
    W[1]["w_at"] = True
    Uw = amgref.cycle(W, I)
    assert np.abs(Uw - Uw.T).max() <= TOL * np.abs(Uw).max()


def test_galerkin_equals_dense_triple_product(hier):
    A, levels = hier
    for L in levels[:-1]:
        C, mag, cnt = amgref.galerkin(L["R"], L["A"], L["P"])
        D = L["R"].toarray() @ L["A"].toarray() @ L["P"].toarray()
        k = cnt.data.max()
        assert np.all(np.abs(C.toarray() - D) <= 2 * (k + 4) * 2.0 ** -53 * mag.toarray())
        assert np.array_equal(C.toarray() != 0, (C.toarray() != 0) & (cnt.toarray() > 0))


def test_cycle_is_positive_definite(hier):
    A, levels = hier
    B = amgref.cycle(_plain(levels), np.eye(A.shape[0]))
    assert np.linalg.eigvalsh(0.5 * (B + B.T)).min() > 0


def test_longdouble_cycle_is_close_to_float64(hier):
    A, levels = hier
    I = np.eye(A.shape[0])[:, ::8]             # (50 columns: the longdouble products are slow)
    U = amgref.cycle(levels, I)
    Ul = amgref.cycle(levels, I, dtype=np.longdouble)
    d = float(np.abs(U - Ul).max() / np.abs(Ul).max())
    assert 0 < d <= TOL


def test_strength_follows_the_diagonals_sign(hier):
    A, _ = hier
    s, t = amgref.strength(A, 0.08), amgref.strength(-A, 0.08)
    assert np.array_equal(s["flags"], t["flags"]) and s["near_ties"] == 0
    assert np.array_equal(s["wF"], t["wF"]) and s["rho_A"] == t["rho_A"]
