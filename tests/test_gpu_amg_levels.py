"""The AMG hierarchy and cycle, level by level, against the restated reference
(tests/amgref.py) through the diagnostics probe (kernels.AmgProbe).

Setup checks compare every level's traced scratch and operators with the
restated rules; cycle checks apply the device cycle to unit vectors and compare
with the restated cycle built from the operators the probe returned, within
8 delta, delta = max |U_64 - U_ld| / max |U_ld| measured on the reference alone
(printed per configuration; see DESIGN.md for the figures of one run).

Deep hierarchies come from amg_dense = 16.  Grids: 40 x 40 (M1-M4), 24 x 96
(M5), synth.magnetostatic(30) (M6), 270 x 270 with the first 70000 rows
permuted (M7: a permuted half would span fewer than 65536 columns), 72 x 72
for the W-cycle (applied to 64 random columns, not the full identity).

Measured on an MI355X (delta, device error in units of delta; bound 8):
  plain 1.1e-16 (0.92)   folded 7.3e-17 (1.03)   sweeps 2 2.1e-16 (0.61)
  sweeps 3 1.8e-16 (1.26)   default f32 9.2e-17 (1.00)   dense level 1 9.6e-17 (1.89)
  diagonal 7.3e-16 (1.06)   M2 8.9e-17 (1.00)   M3 9.1e-17 (1.16)
  W 72 x 72 9.3e-16 (0.93)   M7 6.3e-16 (0.94)   refresh folded 4.7e-17 (1.00)
  refresh unfolded 5.6e-17 (0.54)
Level rows: M1, M3 1600/427/66/11; M2 1600/416/90/20 (smoother-only coarsest);
M4 1600/429/76/13; M5 2304/648/180/57/19/4; M6 961/139/16;
72 x 72 5184/1323/216/28/5; M7 72900/18460/2952/372/45/7.
The default cycle's reference asymmetry (f32 R and P~): 1.2e-8.

Lumped diagonals that cancel (test_strength_flags_and_weights), measured: of
the 40 x 40 grid's 1600 rows 27 have kappa > 2 (largest 7.8), 2 of them cancel
altogether (Neumann rows with weak couplings only) and those 2 break the plain
(len + 2) 2^-52 bound; 25 / 2 rows on its levels 1 / 2, none breaking it; M5
one row per coarse level (kappa 70.8 on level 3 breaks it); M6 61 of 961 rows
(5 cancel altogether) and 20 of 139 on level 1, all cancelling altogether.
Every other row of every level meets the plain bound.
"""
import numpy as np
import pytest
import scipy.sparse as sp

import amgref
from util import _laplace_random
from xfemm_amd import kernels, synth

pytestmark = pytest.mark.gpu
E52, E53 = 2.0 ** -52, 2.0 ** -53
DENSE = 16


def _grid(ny, nx, cx, cy, shift=1.0):
    idx = np.arange(ny * nx).reshape(ny, nx)
    r, c, v = [], [], []
    d = np.zeros(ny * nx)
    for a, b, w in ((idx[:, :-1].ravel(), idx[:, 1:].ravel(), cx), (idx[:-1, :].ravel(), idx[1:, :].ravel(), cy)):
        r += [a, b]
        c += [b, a]
        v += [-w, -w]
        np.add.at(d, a, w)
        np.add.at(d, b, w)
    d[idx[0]] += shift
    r.append(idx.ravel()), c.append(idx.ravel()), v.append(d)
    M = sp.csr_matrix((np.concatenate(v), (np.concatenate(r), np.concatenate(c))), shape=(ny * nx,) * 2)
    M.sort_indices()
    return M


def _m2(M1):
    A = M1.tolil(copy=True)
    for i in range(0, M1.shape[0], 17):
        A[i, :] = 0
        A[:, i] = 0
        A[i, i] = 1.0
    A = A.tocsr()
    A.eliminate_zeros()
    A.sort_indices()
    return A


def _m4(M1, n=40, line=20):
    A = M1.tolil(copy=True)
    for j in range(n):
        a, b = line * n + j, (line + 1) * n + j
        c = abs(A[a, b])
        A[a, b] = A[b, a] = c
        A[a, a] += 2 * c
        A[b, b] += 2 * c
    A = A.tocsr()
    A.sort_indices()
    return A


def _m6():
    P = kernels.Static2DProblem(**synth.magnetostatic(30), precond="amg")
    P.solve()
    rp, col, val, _ = P.csr()
    P.close()
    A = sp.csr_matrix((val, col, rp), shape=(len(rp) - 1,) * 2)
    A.sort_indices()
    return A


def _m7():
    M = _laplace_random(270, 3)
    N = M.shape[0]
    perm = np.arange(N)
    # (half of 72900 rows spans fewer than 65536 columns: the permuted part
    # has to be wider than that for a tile to fall back to int columns)
    perm[:70000] = np.random.default_rng(5).permutation(70000)
    A = M[perm][:, perm].tocsr()
    A.sort_indices()
    return A


_cache = {}


def matrix(name):
    if name not in _cache:
        M1 = _laplace_random(40, 3)
        rng = np.random.default_rng(9)
        make = {"M1": lambda: M1, "M2": lambda: _m2(M1), "M3": lambda: (-M1).tocsr(), "M4": lambda: _m4(M1),
                "M5": lambda: _grid(24, 96, np.exp(rng.uniform(-1, 1, 24 * 95)),
                                    1e-4 * np.exp(rng.uniform(-1, 1, 23 * 96))),
                "M6": _m6, "M7": _m7, "M72": lambda: _laplace_random(72, 3),
                "DIAG": lambda: sp.diags(np.linspace(1.0, 3.0, 700)).tocsr()}
        _cache[name] = make[name]()
    return _cache[name]


def probe(A, **kw):
    kw.setdefault("dense_max", DENSE)
    return kernels.AmgProbe(A.indptr, A.indices, A.data, **kw)


def op(pr, l, sel):
    sh, rp, cl, v = pr.csr(l, sel)
    return amgref.csr(sh, rp, cl, v)


def operators(pr):
    """The levels as the cycle reads them, for amgref.cycle."""
    I = pr.info()
    out = []
    for l, lv in enumerate(I["level"]):
        L = {"A": op(pr, l, pr.A), "dinv": pr.dinv(l), "w": lv["weight"]}
        if l < I["levels"] - 1:
            L.update(P=op(pr, l, pr.P), R=op(pr, l, pr.R), fold=bool(lv["fold"]), w_at=bool(lv["w_at"]))
            if lv["fnnz"] > 0:
                L["PF"] = op(pr, l, pr.PF)
                if l > 0:
                    L["RF"] = op(pr, l, pr.RF)
        elif I["dense_coarse"]:
            L["dense"] = pr.dense()
        out.append(L)
    return out


def same_pattern(X, Y):
    return np.array_equal(X.indptr, Y.indptr) and np.array_equal(X.indices, Y.indices)


def sorted_unique(X):
    for i in range(X.shape[0]):
        c = X.indices[X.indptr[i]:X.indptr[i + 1]]
        if np.any(np.diff(c) <= 0):
            return False
    return True


SETUP = ["M1", "M2", "M3", "M4", "M5", "M6"]
_setup = {}


def setup_of(name, omega=1.75):
    """One traced hierarchy per matrix (fold, col16, f32 on), shared by the setup checks."""
    key = (name, omega)
    if key not in _setup:
        pr = probe(matrix(name), trace=True, omega=omega)
        I = pr.info()
        lv = []
        for l in range(I["levels"]):
            L = {"A": op(pr, l, pr.A | pr.PLAIN_COLS), "info": I["level"][l]}
            if l < I["levels"] - 1:
                for k in ("sflag", "sdeg", "agg", "agg_pre", "root", "dfinv", "wF"):
                    L[k] = pr.trace(l, k)
                L["P"] = op(pr, l, pr.P)
                L["R"] = op(pr, l, pr.R | pr.PLAIN_COLS | pr.F64_VALS)
                L["PF"] = op(pr, l, pr.PF | pr.PLAIN_COLS | pr.F64_VALS)
                if l > 0:
                    L["RF"] = op(pr, l, pr.RF)
            lv.append(L)
        _setup[key] = (pr, I, lv)
        print("%s omega %g levels n/nnz: %s" % (name, omega, [(x["n"], x["nnz"]) for x in I["level"]]))
    return _setup[key]


@pytest.mark.parametrize("name", SETUP)
def test_depth(name):
    pr, I, lv = setup_of(name)
    assert I["levels"] >= 3
    assert all(x["fold"] for x in I["level"][:-1])


def test_depth_72_has_a_folded_w_level():
    pr = probe(matrix("M72"), wlevel=-2)
    I = pr.info()
    print("M72 levels:", [(x["n"], x["nnz"]) for x in I["level"]])
    assert I["levels"] >= 4
    assert any(x["fold"] and x["w_at"] for x in I["level"][1:-1])
    pr.close()


@pytest.mark.parametrize("name", SETUP)
def test_strength_flags_and_weights(name):
    """sflag, strong degree, dfinv, wF and rho_A equal the restated rule on every level."""
    pr, I, lv = setup_of(name)
    for l, L in enumerate(lv[:-1]):
        s = amgref.strength(L["A"], 0.08)
        assert s["near_ties"] == 0, (name, l)
        assert np.array_equal(L["sflag"], s["flags"]), (name, l)
        assert np.array_equal(L["sdeg"], s["deg"]), (name, l)
        # The bound (len + 2) 2^-52 relative holds for a sum without
        # cancellation.  The lumped diagonal d_F = a_ii + sum(weak) does cancel
        # in a few rows (weak couplings of the sign opposite to the diagonal's:
        # kappa = (|a_ii| + sum |weak|) / |d_F| > 1), fully in a Neumann row
        # whose couplings are all weak.  So: every row's d_F (1 / dfinv, or 0
        # as the kernel documents for d_F == 0) within the bound of the sum,
        # absolute; the plain relative bound on dfinv and wF wherever
        # kappa <= 2 (the bound counts 2^-52 per term, twice the unit
        # roundoff); the bound times kappa on the other rows, which are
        # counted and printed.
        A = L["A"]
        rows = np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))
        lumped = np.bincount(rows[s["flags"] != 1], np.abs(A.data[s["flags"] != 1]), A.shape[0])
        U = (s["row_len"] + 2) * E52
        dev = L["dfinv"]
        dF_dev = np.where(dev != 0, 1 / np.where(dev != 0, dev, 1), 0)
        assert np.all(np.abs(dF_dev - s["dF"]) <= U * (lumped + np.abs(s["dF"]))), (name, l)
        assert np.all(L["wF"][dev == 0] == 0) and np.all((L["wF"] >= 0) & (L["wF"] <= 2 / 3)), (name, l)
        kappa = lumped / np.maximum(np.abs(s["dF"]), 1e-300)
        plain = kappa <= 2
        wide = ~plain & (U * kappa < 0.25)
        broke = 0
        for k in ("dfinv", "wF"):
            err, ref = np.abs(L[k] - s[k]), np.abs(s[k])
            assert np.all(err[plain] <= (U * ref)[plain]), (name, l, k, (err[plain] / np.maximum(ref[plain], 1e-300)).max())
            assert np.all(err[wide] <= (U * kappa * ref)[wide]), (name, l, k)
            broke += int((err[~plain] > (U * ref)[~plain]).sum())
        print("%s L%d rows %d: kappa > 2 in %d (largest %.3g among the checked, %d cancel beyond 0.25 / bound), "
              "%d values there break the plain bound" % (name, l, A.shape[0], int((~plain).sum()),
                                                          kappa[wide].max() if wide.any() else 0.0,
                                                          int((~plain & ~wide).sum()), broke))
        # rho[0] = rho_A / omega and the weight 1 / rho[0]: len + 2 roundings from the row's terms
        w = np.longdouble(L["info"]["weight"])
        ref = np.longdouble(s["rho_A"]) / np.longdouble(1.75)
        assert abs(1 / w - ref) <= (s["row_len"].max() + 2) * E52 * ref, (name, l, float(1 / w), float(ref))


@pytest.mark.parametrize("name", SETUP)
def test_aggregates_are_a_maximal_distance2_set(name):
    pr, I, lv = setup_of(name)
    for l, L in enumerate(lv[:-1]):
        A, n, nc = L["A"], L["info"]["n"], L["info"]["nc"]
        S = amgref.csr(A.shape, A.indptr.copy(), A.indices.copy(), (L["sflag"] == 1).astype(float))
        S.eliminate_zeros()
        S2 = (S + S @ S + sp.identity(n)).tocsr()
        roots = np.flatnonzero(L["root"])
        agg, pre, deg = L["agg"], L["agg_pre"], L["sdeg"]
        assert roots.size == nc
        near = S2[roots][:, roots]
        assert near.nnz == roots.size, (name, l)                    # only the diagonal: no two roots within 2
        assert np.array_equal(np.sort(agg[roots]), np.arange(nc))   # every id seeded once
        root_of = np.empty(nc, np.int64)
        root_of[agg[roots]] = roots
        strong = np.flatnonzero(deg > 0)
        assert np.all((agg[strong] >= 0) & (agg[strong] < nc)), (name, l)
        assert np.all(np.asarray(S2[strong, root_of[agg[strong]]]).ravel() != 0), (name, l)
        assert np.array_equal(np.unique(agg[agg >= 0]), np.arange(nc))
        # rows the strong joins left out (k_agg_join3): the aggregate of the
        # largest |a_ij| among aggregated neighbours (ties: larger j), else -1
        assert np.all(pre[deg == 0] == -1)
        assert np.array_equal(agg[pre >= 0], pre[pre >= 0])
        for i in np.flatnonzero(pre < 0):
            c = A.indices[A.indptr[i]:A.indptr[i + 1]]
            v = np.abs(A.data[A.indptr[i]:A.indptr[i + 1]])
            ok = (c != i) & (pre[c] >= 0) & (v > 0)
            want = -1
            if ok.any():
                best = v[ok].max()
                want = pre[c[ok & (v == best)].max()]
            assert agg[i] == want, (name, l, i)
        if name == "M2" and l == 0:
            assert np.all(agg[::17] == -1) and np.all(deg[::17] == 0)


@pytest.mark.parametrize("name", SETUP)
def test_prolongator_and_transposes(name):
    """P equals the restated prolongator; R = P^T and R~ = P~^T bit for bit."""
    pr, I, lv = setup_of(name)
    for l, L in enumerate(lv[:-1]):
        P, mag, cnt = amgref.prolongator(L["A"], L["sflag"], L["agg"], L["info"]["nc"])
        D = L["P"]
        assert same_pattern(D, P) and sorted_unique(D), (name, l)
        assert np.all(np.abs(D.data - P.data) <= (cnt.data + 2) * E52 * mag.data), (name, l)
        for X, Xt in ((L["P"], L["R"]),) + (((L["PF"], L["RF"]),) if l > 0 else ()):
            T = X.T.tocsr()
            T.sort_indices()
            assert sorted_unique(Xt) and same_pattern(Xt, T), (name, l)
            assert np.array_equal(Xt.data.view(np.int64), T.data.view(np.int64)), (name, l)


@pytest.mark.parametrize("name", SETUP)
def test_galerkin_product(name):
    """A_{l+1} = R A P: the structural pattern, each value within
    2 (k + 4) 2^-53 (|R| |A| |P|)_ij, symmetric within the same bound."""
    pr, I, lv = setup_of(name)
    for l, L in enumerate(lv[:-1]):
        C, mag, cnt = amgref.galerkin(L["R"], L["A"], L["P"])
        D = lv[l + 1]["A"]
        assert same_pattern(D, cnt) and sorted_unique(D), (name, l)
        assert np.all(D.diagonal() != 0) and np.all(cnt.diagonal() > 0)
        bound = 2 * (cnt.data.max() + 4) * E53 * amgref.sample(mag, cnt)
        err = np.abs(D.data - amgref.sample(C, cnt))
        print("%s L%d galerkin max err/bound %.3g" % (name, l, (err[bound > 0] / bound[bound > 0]).max()))
        assert np.all(err <= bound), (name, l)
        assert np.all(np.abs(D.data - amgref.sample(D.T.tocsr(), cnt)) <= bound), (name, l)


@pytest.mark.parametrize("name,omega", [(m, 1.75) for m in SETUP] + [("M1", 1.0)])
def test_folded_transfer(name, omega):
    """P~ = P - w D^-1 (A P) with the reported weight, which is omega / rho_A."""
    pr, I, lv = setup_of(name, omega)
    for l, L in enumerate(lv[:-1]):
        s = amgref.strength(L["A"], 0.08)
        w = L["info"]["weight"]
        assert abs(1 / np.longdouble(w) - np.longdouble(s["rho_A"]) / np.longdouble(omega)) <= \
            (s["row_len"].max() + 2) * E52 * s["rho_A"] / omega, (name, l)
        F, mag, cnt = amgref.fold(L["A"], L["P"], w)
        D = L["PF"]
        assert same_pattern(D, F), (name, l)
        assert np.all(np.abs(D.data - F.data) <= (cnt.data + 2) * E52 * mag.data), (name, l)


@pytest.mark.parametrize("name", ["M1", "M7"])
def test_16bit_columns_and_f32_values(name):
    pr = setup_of(name)[0] if name == "M1" else probe(matrix(name))
    I = pr.info()
    assert I["level"][0]["has16"] and I["level"][0]["has32"]
    for sel in (pr.A, pr.PF, pr.R):
        a, b = op(pr, 0, sel), op(pr, 0, sel | pr.PLAIN_COLS)
        assert same_pattern(a, b)
        t, w = pr.tiles(sel)
        if name == "M7" and sel != pr.PF:       # (P~'s columns are coarse ids: fewer than 65536)
            assert 0 < w < t, (sel, t, w)
    for sel in (pr.PF, pr.R):
        a, b = op(pr, 0, sel), op(pr, 0, sel | pr.F64_VALS)
        assert np.array_equal(a.data, b.data.astype(np.float32).astype(np.float64))
    if name == "M7":
        rng = np.random.default_rng(1)
        B = rng.standard_normal((pr.n, 8))
        lv = operators(pr)
        check_cycle(pr, lv, B, "M7 default")
        pr.close()


@pytest.mark.parametrize("f32", [False, True])
def test_coarsest_inverse(f32):
    pr = probe(matrix("M1"), f32=int(f32))
    I = pr.info()
    Ac = op(pr, I["levels"] - 1, pr.A).toarray()
    D = pr.dense()
    n = Ac.shape[0]
    assert I["cinv_f64"] == (not f32)
    tol = n * (2.0 ** -23 if f32 else E52) * np.linalg.cond(Ac, 1)
    err = np.abs(D @ Ac - np.eye(n)).max()
    print("coarsest n %d f32 %d |D A - I| %.3g tol %.3g" % (n, f32, err, tol))
    assert err <= tol
    pr.close()


def test_dense_only_with_and_without_nested_dissection(monkeypatch):
    A = _laplace_random(30, 7)
    out = []
    for nd in (True, False):
        if not nd:
            monkeypatch.setenv("XFK_NO_ND", "1")
        pr = probe(A, dense_max=2048, f32=0)
        assert pr.info()["levels"] == 1
        out.append(pr.dense())
        pr.close()
    Ad = A.toarray()
    tol = 900 * E52 * np.linalg.cond(Ad, 1)
    for D in out:
        assert np.abs(D @ Ad - np.eye(900)).max() <= tol
    assert np.abs(out[0] - out[1]).max() <= tol * np.abs(out[0]).max()


def test_dense_null_direction_is_a_generalised_inverse():
    A = _laplace_random(30, 11, shift=0.0)
    pr = probe(A, dense_max=2048, f32=0)
    D = pr.dense()
    pr.close()
    Ad = A.toarray()
    assert np.all(np.abs(D - D.T) <= 4 * E52 * np.abs(D))      # S_i (M_ij S_j): symmetric M, two roundings a side
    # the bound of the regular case with the condition number of the range
    ev = np.linalg.eigvalsh(Ad)
    tol = 900 * E52 * (ev[-1] / ev[1]) * np.abs(Ad).sum(0).max()
    err = np.abs(Ad @ D @ Ad - Ad).max()
    print("null direction |A D A - A| %.3g tol %.3g" % (err, tol))
    assert err <= tol


_delta = {}


def check_cycle(pr, lv, B, tag, nu=1, factor=8):
    """Device cycle on the columns of B against the restated cycle in
    longdouble, within factor * delta (delta: float64 vs longdouble reference)."""
    U = pr.apply(B)
    Ul = amgref.cycle(lv, B, nu=nu, dtype=np.longdouble)
    U64 = amgref.cycle(lv, B, nu=nu)
    scale = float(np.abs(Ul).max())
    delta = float(np.abs(U64 - Ul).max()) / scale
    err = float(np.abs(U - Ul).max()) / scale
    _delta[tag] = delta
    print("cycle %-14s delta %.3g device err %.3g (%.2f delta) levels %s" % (
        tag, delta, err, err / delta, [x["A"].shape[0] for x in lv]))
    assert np.isfinite(U).all() and delta > 0
    assert err <= factor * delta, (tag, err, delta)
    return U, Ul.astype(np.float64), delta


CYCLES = {
    "plain": ("M1", dict(fold=0, wlevel=-1, f32=0)),
    "folded": ("M1", dict(fold=1, wlevel=-1, f32=0)),
    "sweeps2": ("M1", dict(sweeps=2, f32=0)),
    "sweeps3": ("M1", dict(sweeps=3, f32=0)),
    "default": ("M1", dict()),
    "dense_level1": ("M1", dict(dense_max=1024)),
    "diagonal": ("DIAG", dict(sweeps=2)),
    "M2": ("M2", dict()),
    "M3": ("M3", dict()),
}
_cyc = {}


def cycle_of(tag):
    if tag not in _cyc:
        name, kw = CYCLES[tag]
        pr = probe(matrix(name), **kw)
        lv = operators(pr)
        n = pr.n
        U, Ur, delta = check_cycle(pr, lv, np.eye(n), tag, nu=kw.get("sweeps", 1))
        pr.close()
        _cyc[tag] = (U, Ur, delta, lv)
    return _cyc[tag]


@pytest.mark.parametrize("tag", list(CYCLES))
def test_cycle_equals_restated_cycle(tag):
    U, Ur, delta, lv = cycle_of(tag)
    if tag in ("sweeps2", "sweeps3"):
        assert not any(L.get("fold") for L in lv[:-1])      # the code's own rule
    if tag == "dense_level1":
        assert len(lv) == 2 and lv[1].get("dense") is not None
    if tag == "diagonal":
        assert len(lv) == 1 and lv[0].get("dense") is None
    if tag == "default":
        print("default f32 cycle: reference asymmetry %.3g" % (np.abs(Ur - Ur.T).max() / np.abs(Ur).max()))


@pytest.mark.parametrize("tag", ["plain", "folded"])
def test_f64_cycle_is_symmetric_positive_definite(tag):
    U, Ur, delta, lv = cycle_of(tag)
    assert np.abs(U - U.T).max() <= 8 * delta * np.abs(U).max()
    assert np.linalg.eigvalsh(0.5 * (U + U.T)).min() > 0


def test_folded_and_plain_device_cycles_agree():
    Up, _, dp, _ = cycle_of("plain")
    Uf, _, df, _ = cycle_of("folded")
    assert np.abs(Up - Uf).max() <= 16 * max(dp, df) * np.abs(Up).max()


def test_w_cycle_equals_restated_cycle():
    """72 x 72, folded with the default W level: 64 random columns."""
    pr = probe(matrix("M72"), wlevel=-2, f32=0)
    lv = operators(pr)
    assert any(L["fold"] and L["w_at"] for L in lv[1:-1])
    B = np.random.default_rng(2).standard_normal((pr.n, 64))
    check_cycle(pr, lv, B, "W 72x72")
    pr.close()


@pytest.mark.parametrize("fold", [True, False])
def test_refresh(fold, monkeypatch):
    A = matrix("M1")
    n = A.shape[0]
    x = np.arange(n) / n
    s = sp.diags(np.sqrt(0.5 + 1.5 * (0.5 + 0.5 * np.sin(5 * x))))
    An = (s @ A @ s).tocsr()
    An.sort_indices()
    assert same_pattern(A, An)
    pr = probe(A, f32=0)
    w_old = pr.info()["level"][0]["weight"]
    P_old = op(pr, 0, pr.P)
    before = operators(pr)
    pr.refresh(An.data, fold)
    I = pr.info()
    w = I["level"][0]["weight"]
    sn = amgref.strength(An, 0.08)
    assert w != w_old
    assert abs(1 / np.longdouble(w) - np.longdouble(sn["rho_A"]) / np.longdouble(1.75)) <= \
        (sn["row_len"].max() + 2) * E52 * sn["rho_A"] / 1.75
    assert np.array_equal(pr.dinv(0), 1.0 / An.diagonal())
    assert bool(I["level"][0]["fold"]) == fold
    lv = operators(pr)
    assert np.array_equal(lv[0]["A"].data, An.data)
    # the refresh keeps P, R and every coarse level, bit for bit
    bits = lambda x: x.view(np.int64) if isinstance(x, np.ndarray) else np.concatenate(
        [x.indptr, x.indices, x.data.view(np.int64)])
    for k in ("P", "R"):
        assert np.array_equal(bits(before[0][k]), bits(lv[0][k]))
    for Lb, La in zip(before[1:], lv[1:]):
        assert Lb.keys() == La.keys()
        for k in Lb:
            if k in ("fold", "w_at", "w"):
                assert Lb[k] == La[k]
            else:
                assert np.array_equal(bits(Lb[k]), bits(La[k])), k
    if fold:
        F, mag, cnt = amgref.fold(An, P_old, w)
        D = op(pr, 0, pr.PF)
        assert same_pattern(D, F)
        assert np.all(np.abs(D.data - F.data) <= (cnt.data + 2) * E52 * mag.data)
        monkeypatch.setenv("XFK_REFOLD_STAGE", "0")
        pr.refresh(An.data, True)
        assert np.array_equal(op(pr, 0, pr.PF).data.view(np.int64), D.data.view(np.int64))
    check_cycle(pr, lv, np.eye(n)[:, ::5], "refresh fold=%d" % fold)
    pr.close()
