"""The AMG setup rules and cycle of xfemm_amd/csrc/xfk_amg*.hip restated in
plain numpy / scipy, as the reference of tests/test_gpu_amg_levels.py.

Nothing here runs on a device.  The setup rules (strength, prolongator,
galerkin, fold) follow the comments and code of the kernels; `cycle` restates
vcycle_level branch by branch and only ever multiplies operators handed to it
(the tests hand it the operators copied out of the device hierarchy, so a
setup error and a cycle error fail different tests).  Every function takes a
dtype; np.longdouble measures the float64 cycle's own rounding.
"""
import numpy as np
import scipy.sparse as sp

EPS = 2.0 ** -52


def csr(shape, rowptr, col, val):
    """scipy CSR that keeps explicit zeros and the stored order."""
    return sp.csr_matrix((np.asarray(val), np.asarray(col), np.asarray(rowptr)), shape=shape)


def _rows(A):
    return np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))


def _rowsum(rows, w, n, dtype):
    out = np.zeros(n, dtype)
    np.add.at(out, rows, w)
    return out


def diagonal(A, dtype=np.float64):
    rows = _rows(A)
    d = np.zeros(A.shape[0], dtype)
    m = A.indices == rows
    d[rows[m]] = A.data[m].astype(dtype)
    return d


def strength(A, theta, dtype=np.float64):
    """k_amg_strength: flags (0 weak, 1 strong, 2 diagonal), strong degree,
    lumped diagonal d_F, its inverse, rho_i, w_i, rho_A; `near_ties` counts
    off-diagonal entries whose test lies within 4 ulp of equality."""
    A = sp.csr_matrix(A)
    n = A.shape[0]
    rows, cols = _rows(A), A.indices
    v = A.data.astype(dtype)
    d = diagonal(A, dtype)
    ad = np.abs(d)
    sg = np.where(d < 0, -1.0, 1.0).astype(dtype)
    isd = cols == rows
    lhs = -sg[rows] * v
    rhs = dtype(theta) * np.sqrt(ad[rows] * ad[cols])
    strong = ~isd & (v != 0) & (lhs > rhs)
    weak = ~isd & ~strong
    near = ~isd & (v != 0) & (np.abs(lhs - rhs) <= 4 * np.spacing(np.abs(rhs).astype(np.float64)))
    flags = np.where(isd, 2, np.where(strong, 1, 0)).astype(np.uint8)
    deg = np.bincount(rows[strong], minlength=n).astype(np.int32)
    dF = d + _rowsum(rows[weak], v[weak], n, dtype)
    sumS = _rowsum(rows[strong], np.abs(v[strong]), n, dtype)
    sumA = _rowsum(rows[~isd], np.abs(v[~isd]), n, dtype)
    ok = dF != 0
    safe = np.where(ok, dF, 1)
    rho_i = np.where(ok, (np.abs(dF) + sumS) / np.abs(safe), 0)
    dfinv = np.where(ok, 1 / safe, 0)
    wF = np.where(ok & (deg > 0), (dtype(4) / dtype(3)) / np.maximum(rho_i, 2), 0)
    rA = np.where(d != 0, (ad + sumA) / np.where(d != 0, ad, 1), 0)
    return {"flags": flags, "deg": deg, "dF": dF, "dfinv": dfinv, "rho_i": rho_i, "wF": wF,
            "rho_A": rA.max() if n else dtype(0), "near_ties": int(near.sum()),
            "row_len": np.diff(A.indptr)}


def _coo_sum(r, c, v, shape, dtype):
    """CSR (sorted, unique columns, zeros kept) of the summed triplets, with
    the number of terms and the sum of |terms| per entry."""
    key = r.astype(np.int64) * shape[1] + c
    uk, inv = np.unique(key, return_inverse=True)
    val = np.zeros(uk.size, dtype)
    mag = np.zeros(uk.size, dtype)
    np.add.at(val, inv, v)
    np.add.at(mag, inv, np.abs(v))
    cnt = np.bincount(inv, minlength=uk.size)
    rr, cc = uk // shape[1], uk % shape[1]
    rp = np.zeros(shape[0] + 1, np.int64)
    np.add.at(rp, rr + 1, 1)
    rp = np.cumsum(rp)
    return (csr(shape, rp, cc, val), csr(shape, rp, cc, mag), csr(shape, rp, cc, cnt.astype(np.float64)))


def prolongator(A, flags, agg, nc=None, dtype=np.float64):
    """P = (I - W D_F^-1 A_F) P_tent from the flags and the aggregate map: a
    row's kept entries (strong, diagonal) with an aggregated column j add to
    column agg[j] -- 1 - w_i for the diagonal, -(w_i / d_F,i) a_ij for a strong
    entry.  Returns (P, sum |terms|, terms) on one pattern."""
    A = sp.csr_matrix(A)
    n = A.shape[0]
    agg = np.asarray(agg)
    nc = int(agg.max()) + 1 if nc is None else nc
    rows, cols = _rows(A), A.indices
    v = A.data.astype(dtype)
    isd, strong, weak = flags == 2, flags == 1, flags == 0
    d = diagonal(A, dtype)
    dF = d + _rowsum(rows[weak], v[weak], n, dtype)
    sumS = _rowsum(rows[strong], np.abs(v[strong]), n, dtype)
    deg = np.bincount(rows[strong], minlength=n)
    ok = dF != 0
    safe = np.where(ok, dF, 1)
    dfinv = np.where(ok, 1 / safe, 0)
    rho_i = np.where(ok, (np.abs(dF) + sumS) / np.abs(safe), 0)
    w = np.where(ok & (deg > 0), (dtype(4) / dtype(3)) / np.maximum(rho_i, 2), 0)
    keep = (flags != 0) & (agg[cols] >= 0)
    val = np.where(isd, 1 - w[rows], (-w[rows] * dfinv[rows]) * v)
    return _coo_sum(rows[keep], agg[cols[keep]], val[keep], (n, nc), dtype)


def galerkin(R, A, P):
    """R A P in float64 with its entrywise magnitude |R| |A| |P|, its
    structural pattern (all-ones product: the products feeding each entry)."""
    R, A, P = (sp.csr_matrix(M) for M in (R, A, P))
    ones = lambda M: csr(M.shape, M.indptr, M.indices, np.ones(M.nnz))
    C = (R @ A @ P).tocsr()
    mag = (abs(R) @ abs(A) @ abs(P)).tocsr()
    cnt = (ones(R) @ ones(A) @ ones(P)).tocsr()
    for M in (C, mag, cnt):
        M.sort_indices()
    return C, mag, cnt


def sample(M, pat):
    """The values of M at the entries of pattern `pat` (zeros where M has none)."""
    r = _rows(pat)
    return np.asarray(sp.csr_matrix(M)[r, pat.indices]).ravel() if pat.nnz else np.zeros(0)


def fold(A, P, w, dtype=np.float64):
    """P~ = P - w D^-1 (A P) on the pattern of A P.  Returns (P~, sum |terms|,
    terms) on that pattern; the terms of an entry are P_ic and the products of
    (A P)_ic."""
    A, P = sp.csr_matrix(A), sp.csr_matrix(P)
    ones = lambda M: csr(M.shape, M.indptr, M.indices, np.ones(M.nnz))
    pat = (ones(A) @ ones(P)).tocsr()
    pat.sort_indices()
    d = diagonal(A, dtype)
    wd = dtype(w) * np.where(d != 0, 1 / np.where(d != 0, d, 1), 0)
    r = _rows(pat)
    ap = sample(A @ P, pat).astype(dtype)
    apm = sample(abs(A) @ abs(P), pat).astype(dtype)
    p = sample(P, pat).astype(dtype)
    val = p - wd[r] * ap
    mag = np.abs(p) + np.abs(wd[r]) * apm
    mk = lambda x: csr(pat.shape, pat.indptr, pat.indices, x)
    return mk(val), mk(mag), mk(pat.data + 1)


def spmm(M, X, dtype):
    """M X for a scipy CSR and a dense block, products and sums in dtype."""
    M = sp.csr_matrix(M)
    out = np.zeros((M.shape[0], X.shape[1]), dtype)
    if M.nnz == 0:
        return out
    v = M.data.astype(dtype)
    nonempty = np.flatnonzero(np.diff(M.indptr) > 0)
    for c0 in range(0, X.shape[1], 256):
        prod = v[:, None] * X[M.indices, c0:c0 + 256]
        out[nonempty, c0:c0 + 256] = np.add.reduceat(prod, M.indptr[nonempty], axis=0)
    return out


def cycle(levels, b, nu=1, dtype=np.float64, l=0, yadd=None):
    """vcycle_level restated.  levels[l] is a dict with A, dinv, w (the
    smoother weight 1 / rho[0]) and, above the coarsest, R, P, fold, w_at and
    (folded) PF, RF; the coarsest may carry `dense`, the operator applied."""
    L = levels[l]
    b = np.asarray(b, dtype)
    if b.ndim == 1:
        return cycle(levels, b[:, None], nu, dtype, l, yadd)[:, 0]
    wd = (dtype(L["w"]) * L["dinv"].astype(dtype))[:, None]
    A = L["A"]
    sweep = lambda x: x + wd * (b - spmm(A, x, dtype))
    if l == len(levels) - 1:
        if L.get("dense") is not None:
            return L["dense"].astype(dtype) @ b
        x = sweep(wd * b)                      # smoother only: 2 nu sweeps from zero
        for _ in range(2, 2 * nu):
            x = sweep(x)
        return x
    if L["fold"] and l > 0:
        y = sweep(wd * b)
        if yadd is not None:
            y = yadd + y
        bc = spmm(L["RF"], b, dtype)
        if L["w_at"]:
            x1 = cycle(levels, bc, nu, dtype, l + 1)
            rc = bc - spmm(levels[l + 1]["A"], x1, dtype)
            xc = cycle(levels, rc, nu, dtype, l + 1, yadd=x1)
        else:
            xc = cycle(levels, bc, nu, dtype, l + 1)
        return y + spmm(L["PF"], xc, dtype)
    cur = wd * b
    for _ in range(1, nu):
        cur = sweep(cur)
    r = b - spmm(A, cur, dtype)
    xc = cycle(levels, spmm(L["R"], r, dtype), nu, dtype, l + 1)
    if L["fold"] and l == 0 and nu == 1:
        return (wd * b + wd * r) + spmm(L["PF"], xc, dtype)
    cur = cur + spmm(L["P"], xc, dtype)
    for _ in range(nu):
        cur = sweep(cur)
    return cur


def greedy_aggregates(A, flags):
    """A simple greedy distance-2 aggregation of the strong graph (the CPU
    tests' stand-in for MIS-2): rows without strong couplings get -1."""
    A = sp.csr_matrix(A)
    n = A.shape[0]
    S = csr(A.shape, A.indptr.copy(), A.indices.copy(), (flags == 1).astype(np.float64))
    S.eliminate_zeros()
    S2 = (S + S @ S).tocsr()
    agg = np.full(n, -1)
    deg = np.diff(S.indptr)
    covered = np.zeros(n, bool)                 # within distance 2 of a root
    nc = 0
    for i in range(n):
        if deg[i] == 0 or covered[i]:
            continue
        nb = S.indices[S.indptr[i]:S.indptr[i + 1]]
        agg[i] = nc
        agg[nb[agg[nb] < 0]] = nc
        covered[S2.indices[S2.indptr[i]:S2.indptr[i + 1]]] = True
        covered[i] = True
        nc += 1
    for _ in range(n):                          # leftovers join a strong neighbour's aggregate
        left = np.flatnonzero((agg < 0) & (deg > 0))
        if left.size == 0:
            break
        for i in left:
            a = agg[S.indices[S.indptr[i]:S.indptr[i + 1]]]
            if (a >= 0).any():
                agg[i] = a[a >= 0][0]
    return agg, nc


def build_reference_hierarchy(A, theta=0.08, omega=1.75, coarse=16, fold_levels=True):
    """A whole hierarchy by the restated rules and greedy aggregates, with the
    exact dense inverse on the coarsest level (CPU tests only)."""
    levels = []
    A = sp.csr_matrix(A)
    while True:
        s = strength(A, theta)
        d = diagonal(A)
        L = {"A": A, "dinv": np.where(d != 0, 1 / np.where(d != 0, d, 1), 0), "w": omega / s["rho_A"]}
        levels.append(L)
        if A.shape[0] <= coarse:
            L["dense"] = np.linalg.inv(A.toarray())
            return levels
        agg, nc = greedy_aggregates(A, s["flags"])
        P = prolongator(A, s["flags"], agg, nc)[0]
        L.update(P=P, R=P.T.tocsr(), fold=fold_levels, w_at=False)
        PF = fold(A, P, L["w"])[0]
        L.update(PF=PF, RF=PF.T.tocsr())
        A = galerkin(L["R"], A, P)[0]
