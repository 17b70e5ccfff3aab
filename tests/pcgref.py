"""A plain restatement of the device PCG (xfk_pcg.hip's header comment,
CBigLinProb::PCGSolve of the reference, spars.cpp:238-316) and the matrices
the PCG kernels are tested on.  Host only.

The restatement is the Chronopoulos-Gear arrangement of preconditioned CG,
    u = M^-1 r, w = A u, gamma = r.u, delta = w.u,
    beta = gamma_k / gamma_k-1, alpha = gamma_k / (delta_k - beta gamma_k / alpha_k-1),
    z = w + beta z, p = u + beta p, x += alpha p, r -= alpha z,
with res_o = (M^-1 b).b, er_k = sqrt(gamma_k / res_o) and a stop at the first
k >= 1 with er_k <= precision (res_o == 0 returns at once).  It runs in
numpy.longdouble; a float64 run with sequential sums exists only to size the
tolerance of the whole-solve er comparison.

rounding_bound is the a-priori bound of a float64 evaluation of one step, from
absolute-value sums with gamma_k = k u / (1 - k u), u = 2^-53, k the longest
addition chain (row length for an SpMV entry, vector length for a dot
product; valid for any summation order).  No constant in it is fitted.
"""
import numpy as np
import scipy.sparse as sp

LD = np.longdouble
U = 2.0 ** -53


def gam(k):
    k = np.asarray(k, np.float64)
    return k * U / (1.0 - k * U)


# ---- the restated PCG --------------------------------------------------------

def spmv(rp, col, val, x, dt=LD):
    """A x; products in dt, summed per row (every row has a diagonal: none is empty)."""
    prod = np.asarray(val, dt) * np.asarray(x, dt)[col]
    return np.add.reduceat(prod, rp[:-1])


def dot(a, b, dt=LD):
    if dt is LD:
        return np.sum(np.asarray(a, LD) * np.asarray(b, LD))
    s = np.cumsum(np.asarray(a, dt) * np.asarray(b, dt))      # sequential
    return s[-1]


def csr(rp, col, val):
    """scipy's CSR on copies: scipy may sort a row's entries in place, and the
    order of an unsorted case's entries is what that case is there for."""
    n = len(rp) - 1
    return sp.csr_matrix((np.array(val, np.float64), np.array(col), np.array(rp)), shape=(n, n))


def diag_of(rp, col, val):
    rows = np.repeat(np.arange(len(rp) - 1), np.diff(rp))
    d = np.zeros(len(rp) - 1)
    d[rows[col == rows]] = np.asarray(val)[col == rows]
    return d


def jacobi(rp, col, val, dt=LD):
    d = np.asarray(diag_of(rp, col, val), dt)
    return lambda r: np.asarray(r, dt) / d


def pcg(rp, col, val, b, x0, flag, precision, minv, dt=LD, keep=False, max_it=100000):
    """-> dict(x, er (the whole sequence), k (the stopping index), xs (the
    iterates when keep), drift (see true_residual_drift))."""
    n = len(rp) - 1
    b = np.asarray(b, dt)
    x = np.asarray(x0, dt).copy() if flag else np.zeros(n, dt)
    r = b - spmv(rp, col, val, x, dt) if flag else b.copy()
    u = np.asarray(minv(r), dt)
    res_o = dot(minv(b), b, dt) if flag else dot(u, b, dt)
    out = {"x": x, "er": [], "k": 0, "xs": [x.copy()] if keep else None, "res_o": res_o, "drift": None}
    if res_o == 0:
        out["er"] = [dt(0)]
        return out
    absA = csr(rp, col, np.abs(np.asarray(val, np.float64)))
    L = int(np.diff(rp).max())
    w = spmv(rp, col, val, u, dt)
    g, d = dot(r, u, dt), dot(w, u, dt)
    z, p = np.zeros(n, dt), np.zeros(n, dt)
    phat, drift = np.zeros(n), np.zeros(n)
    gp = ap = None
    k = 0
    er = [np.sqrt(g / res_o)]
    while k < max_it:
        if k >= 1 and er[k] <= precision:
            break
        if k == 0:
            beta, alpha = dt(0), g / d
        else:
            beta = g / gp
            alpha = g / (d - beta * g / ap)
        z = w + beta * z
        p = u + beta * p
        x = x + alpha * p
        r = r - alpha * z
        # the recursive residual's distance from b - A x (true_residual_drift)
        phat = np.abs(np.asarray(u, np.float64)) + abs(float(beta)) * phat
        drift += gam(L + k + 3) * (abs(float(alpha)) * (absA @ phat) + np.abs(np.asarray(r, np.float64))) \
            + U * (absA @ np.abs(np.asarray(x, np.float64)))
        u = np.asarray(minv(r), dt)
        w = spmv(rp, col, val, u, dt)
        gp, ap = g, alpha
        g, d = dot(r, u, dt), dot(w, u, dt)
        k += 1
        er.append(np.sqrt(g / res_o))
        if keep:
            out["xs"].append(x.copy())
    out.update(x=x, er=er, k=k, drift=drift)
    return out


def one_step(rp, col, val, b, x0, flag, minv):
    """x1 = x0 + alpha0 u0, r1 and er_1, written without the loop; every
    intermediate is returned for rounding_bound."""
    n = len(rp) - 1
    b = np.asarray(b, LD)
    xs = np.asarray(x0, LD) if flag else np.zeros(n, LD)
    ax = spmv(rp, col, val, xs) if flag else np.zeros(n, LD)
    r0 = b - ax
    u0 = np.asarray(minv(r0), LD)
    mb = np.asarray(minv(b), LD) if flag else u0
    res_o = np.sum(mb * b)
    w0 = spmv(rp, col, val, u0)
    g0, d0 = np.sum(r0 * u0), np.sum(w0 * u0)
    a0 = g0 / d0
    x1 = xs + a0 * u0
    r1 = r0 - a0 * w0
    u1 = np.asarray(minv(r1), LD)
    g1 = np.sum(r1 * u1)
    return dict(x0=xs, ax=ax, r0=r0, u0=u0, mb=mb, res_o=res_o, w0=w0, g0=g0, d0=d0, a0=a0, x1=x1, r1=r1, u1=u1,
                g1=g1, er1=np.sqrt(g1 / res_o))


def rounding_bound(rp, col, val, b, flag, s, mnorm=None, kv=0):
    """Bounds of |x1 - one_step's x1| (element-wise) and |er - er_1| for a
    float64 evaluation of one step, s = one_step(...).

    Jacobi (mnorm None): u = fl(fl(1 / d) r), two roundings on top of r's error.
    AMG (mnorm = an estimate of ||M^-1||_2, kv = the cycle's addition-chain
    count): the cycle is an input, a fixed symmetric linear operator that the
    device and the reference apply with the same code; applied to an input
    that differs by e it returns M^-1 e more, and its own rounding is taken as
    a backward error of gam(kv) ||r||_2 on each of the two inputs compared.
    Where the device's input is the reference's bit for bit (r0 = b at
    flag == 0, M^-1 b) the cycle adds nothing.  Its effect on gamma = r.M^-1 r
    is 2 u.e to first order (symmetry), on delta = u.A u it is 2 w.(M^-1 e).
    """
    f = lambda a: np.abs(np.asarray(a, np.float64))
    n = len(rp) - 1
    N = float(n)
    ln = np.diff(rp).astype(np.float64)
    absA = csr(rp, col, f(val))
    d = diag_of(rp, col, val)
    b_, r0, u0, w0, x1, r1, u1 = f(b), f(s["r0"]), f(s["u0"]), f(s["w0"]), f(s["x1"]), f(s["r1"]), f(s["u1"])
    g0, d0, a0, g1, res_o = (abs(float(s[k])) for k in ("g0", "d0", "a0", "g1", "res_o"))
    n2 = lambda v: float(np.sqrt(np.sum(v * v)))
    amg = mnorm is not None

    # r0 = b - A x0
    if flag:
        e_ax = gam(ln) * (absA @ f(s["x0"]))
        e_r0 = e_ax + U * (r0 + e_ax)
    else:
        e_r0 = np.zeros(n)
    # u0 = M^-1 r0 (element-wise e_u0; AMG: the same figure for every element)
    if amg:
        E0 = mnorm * (n2(e_r0) + n2(r0) * (U + 2 * gam(kv))) if flag else 0.0
        e_u0 = np.full(n, E0)
    else:
        e_u0 = gam(2) * u0 + (1 + gam(2)) * e_r0 / np.abs(d)
    # w0 = A u0.  AMG: what A makes of the cycle's uniform figure is carried as a
    # 2-norm (||A||_2 <= the largest absolute row sum), not spread over the elements
    rowmax = float((absA @ np.ones(n)).max())
    if amg:
        e_w0, Nw0 = gam(ln) * (absA @ (u0 + e_u0)), rowmax * float(e_u0[0])
    else:
        e_w0, Nw0 = gam(ln) * (absA @ (u0 + e_u0)) + absA @ e_u0, 0.0
    # res_o = (M^-1 b).b: AMG reads the cycle's output bit for bit
    e_res = gam(N) * float(np.sum(b_ * f(s["mb"]))) if amg else gam(N + 2) * float(np.sum(b_ * b_ / np.abs(d)))

    def e_gamma(r, u, e_r, e_u, E, Nr=0.0):      # r's error: e_r element-wise plus Nr in the 2-norm
        summed = gam(N) * (float(np.sum((r + e_r) * (u + e_u))) + Nr * n2(u + e_u))
        if amg:      # 2 u.e + the cycle's rounding + second order
            return summed + float(np.sum(u * (2 * e_r + U * r))) + 2 * n2(u) * Nr \
                + n2(r) ** 2 * mnorm * 2 * gam(kv) + (n2(e_r) + Nr) * E
        return summed + float(np.sum(r * e_u + u * e_r + e_r * e_u))

    def e_delta(u, w, e_u, e_w, E):
        summed = gam(N) * (float(np.sum((u + e_u) * (w + e_w))) + Nw0 * n2(u + e_u))
        if amg:      # the SpMV's rounding on u as given, then 2 w.(M^-1 e) and second order
            return summed + float(np.sum(u * gam(ln) * (absA @ u))) + 2 * n2(w) * E + rowmax * E * E \
                + gam(ln.max()) * rowmax * E * float(np.sum(u))
        return summed + float(np.sum(u * e_w + w * e_u + e_u * e_w))

    E0 = float(e_u0[0]) if amg else 0.0
    e_g0 = e_gamma(r0, u0, e_r0, e_u0, E0) if (flag or not amg) else gam(N) * float(np.sum(r0 * u0))
    e_d0 = e_delta(u0, w0, e_u0, e_w0, E0)
    assert e_d0 < d0, "delta_0's bound swallows delta_0: the case is too ill-conditioned to pin"
    e_a0 = (e_g0 + a0 * e_d0) / (d0 - e_d0) + U * a0
    # x1 = x0 + alpha0 p0 (p0 = u0), r1 = r0 - alpha0 z0 (z0 = w0); fused or not
    e_x1 = a0 * e_u0 + e_a0 * (u0 + e_u0) + gam(2) * (a0 * u0 + x1)
    e_r1 = e_r0 + a0 * e_w0 + e_a0 * (w0 + e_w0) + gam(2) * (a0 * w0 + r1)
    Nr1 = (a0 + e_a0) * Nw0
    if amg:
        E1 = mnorm * (n2(e_r1) + Nr1 + n2(r1) * (U + 2 * gam(kv)))
        e_u1 = np.full(n, E1)
    else:
        E1 = 0.0
        e_u1 = gam(2) * u1 + (1 + gam(2)) * e_r1 / np.abs(d)
    e_g1 = e_gamma(r1, u1, e_r1, e_u1, E1, Nr1)
    # er_1 = sqrt(gamma_1 / res_o): sqrt(1 + t) <= 1 + t / 2, one division, one root.
    # gamma_1 is a sum of non-negative terms whose true value may be far below its
    # bound (an exactly solved system): the bound is absolute, through sqrt(a + e) <= sqrt(a) + sqrt(e)
    rr = e_res / res_o
    er1 = float(s["er1"])
    e_er = er1 * (0.5 * rr / (1 - rr) + 3 * U) + np.sqrt(e_g1 / (res_o * (1 - rr))) \
        if e_g1 >= g1 else er1 * (0.5 * (e_g1 / g1 + rr) / (1 - e_g1 / g1 - rr) + 3 * U)
    return {"x1": e_x1, "er": float(e_er)}


def true_residual(rp, col, val, b, x, minv):
    """sqrt(r.M^-1 r / b.M^-1 b) of r = b - A x, in longdouble."""
    b = np.asarray(b, LD)
    r = b - spmv(rp, col, val, x)
    return float(np.sqrt(np.sum(r * np.asarray(minv(r), LD)) / np.sum(b * np.asarray(minv(b), LD))))


def true_residual_drift(rp, col, val, b, ref, minv_abs):
    """How far sqrt(r.M^-1 r / res_o) of the true residual may lie above that
    of the recursive one after ref["k"] float64 steps: the triangle inequality
    in the M^-1 norm on the vector pcg() accumulated.  Per step the recursive
    r moves away from b - A x by the rounding of z (= A p up to the SpMV's
    gam(L) |A| |u_j| of every w_j it was built from, carried by the betas:
    phat = |u| + beta phat, one more rounding per recurrence step), of the two
    updates (gam(3) (|alpha z| + |r|), within the first term's constant) and
    of x (u |x|, seen through A).  minv_abs(v) bounds v.M^-1 v."""
    return float(np.sqrt(minv_abs(ref["drift"]) / float(ref["res_o"])))


def error_reach(rp, col, val, res_o, er, mu=None):
    """The a-priori 2-norm distance from the solution of an iterate whose true
    residual has sqrt(r.M^-1 r / res_o) <= er.  With e the error, A e = r:
    |e|_2^2 <= e.A e / lmin(A) = r.A^-1 r / lmin(A) <= r.M^-1 r / (mu lmin(A)),
    mu the smallest eigenvalue of M^-1 A.  lmin(A) is Gershgorin's bound where
    that is well above zero, the dense eigenvalue otherwise; mu is given for the
    AMG and is that of D^-1/2 A D^-1/2 for Jacobi, found the same way."""
    n = len(rp) - 1
    A = csr(rp, col, val)
    d = A.diagonal()
    off = np.asarray(abs(A).sum(axis=1)).ravel() - d
    lam = float((d - off).min())
    if lam <= 1e-3 * d.min():
        lam = float(np.linalg.eigvalsh(A.toarray())[0])
    if mu is None:
        mu = float((1 - off / d).min())
        if mu <= 1e-3:
            S = sp.diags(1 / np.sqrt(d))
            mu = float(np.linalg.eigvalsh((S @ A @ S).toarray())[0])
    return float(er) * float(np.sqrt(float(res_o) / (mu * lam)))


def direct_solve(rp, col, val, b):
    """Sparse LU, refined once in longdouble."""
    import scipy.sparse.linalg as sla
    n = len(rp) - 1
    lu = sla.splu(csr(rp, col, val).tocsc())
    x = np.asarray(lu.solve(np.asarray(b, np.float64)), LD)
    r = np.asarray(b, LD) - spmv(rp, col, val, x)
    return x + np.asarray(lu.solve(np.asarray(r, np.float64)), LD)


# ---- the zoo -----------------------------------------------------------------

DOM = 30.0      # diagonal = DOM x the row's off-diagonal sum: Jacobi-PCG gains > 16x per step


def _finish(n, i, j, v, dom):
    """Symmetric CSR from the strict upper triangle (i < j), a dominant diagonal added."""
    A = sp.coo_matrix((np.r_[v, v], (np.r_[i, j], np.r_[j, i])), shape=(n, n)).tocsr()
    off = np.asarray(abs(A).sum(axis=1)).ravel()
    A = (A + sp.diags(dom * np.maximum(off, 1.0))).tocsr()
    A.sort_indices()
    return A.indptr.astype(np.int32), A.indices.astype(np.int32), A.data.astype(np.float64)


def _offdiag(rng, m):
    return rng.uniform(0.1, 1.0, m) * rng.choice([-1.0, 1.0], m)


def banded(n, per_row, seed, dom=DOM):
    """Tridiagonal plus random long-range entries, about per_row entries per row."""
    rng = np.random.default_rng(seed)
    i = np.arange(n - 1)
    j = i + 1
    extra = max(0, per_row - 3) // 2
    if n > 3 and extra:
        a = np.repeat(np.arange(n), extra)
        c = rng.integers(0, n, a.size)
        lo, hi = np.minimum(a, c), np.maximum(a, c)
        keep = hi - lo > 1
        pair = np.unique(lo[keep].astype(np.int64) * n + hi[keep])
        i, j = np.r_[i, pair // n], np.r_[j, pair % n]
    return _finish(n, i, j, _offdiag(rng, i.size), dom)


def arrow(n, hub, seed, dom=DOM):
    """Row and column `hub` dense, the other rows a diagonal and the arrow entry."""
    rng = np.random.default_rng(seed)
    o = np.delete(np.arange(n), hub)
    return _finish(n, np.minimum(o, hub), np.maximum(o, hub), _offdiag(rng, n - 1), dom)


def diagonal(n, seed, dom=None):
    rng = np.random.default_rng(seed)
    return np.arange(n + 1, dtype=np.int32), np.arange(n, dtype=np.int32), rng.uniform(0.5, 1.5, n)


def grid5(m, seed, dom=None):
    """5-point grid, conductances in [0.5, 2], a unit shift on the first grid line."""
    rng = np.random.default_rng(seed)
    idx = np.arange(m * m).reshape(m, m)
    i = np.r_[idx[:, :-1].ravel(), idx[:-1, :].ravel()]
    j = np.r_[idx[:, 1:].ravel(), idx[1:, :].ravel()]
    g = rng.uniform(0.5, 2.0, i.size)
    n = m * m
    A = sp.coo_matrix((np.r_[-g, -g], (np.r_[i, j], np.r_[j, i])), shape=(n, n)).tocsr()
    dg = -np.asarray(A.sum(axis=1)).ravel()
    dg[idx[0]] += 1.0
    A = (A + sp.diags(dg)).tocsr()
    A.sort_indices()
    return A.indptr.astype(np.int32), A.indices.astype(np.int32), A.data.astype(np.float64)


def shuffled(csr, seed):
    """The same matrix, the entries of every row permuted."""
    rp, col, val = csr
    rng = np.random.default_rng(seed)
    rows = np.repeat(np.arange(len(rp) - 1), np.diff(rp))
    o = np.lexsort((rng.random(col.size), rows))
    return rp, col[o], val[o]


# name -> (builder, arguments); SEEDS below holds the seed of each
CASES = {}
for _n in (1, 2, 3, 63, 64, 65, 511, 512, 513, 1023, 1025):
    CASES["band%d" % _n] = (banded, (_n, 9))
CASES["pass2"] = (banded, (1025, 12))            # 512 rows x ~12: 2 passes per tile
CASES["pass5"] = (banded, (1025, 40))            # 512 rows x ~40: 5 or more
CASES["arrow_first"] = (arrow, (4609, 0))        # a row longer than a pass, first ...
CASES["arrow_last"] = (arrow, (4609, 4608))      # ... last ...
CASES["arrow_mid"] = (arrow, (4609, 768))        # ... and in the middle of the second tile
CASES["diag1000"] = (diagonal, (1000,))
CASES["unsorted"] = (lambda s, dom: shuffled(banded(1025, 12, s, dom), s + 1), ())
SMALL = list(CASES)                               # Jacobi, one step and whole solve
LARGE = {"grid725": (grid5, (725,)), "grid1025": (grid5, (1025,))}      # one step, both preconditioners
AMG_SMALL = {"grid45": (grid5, (45,)), "grid150": (grid5, (150,)),
             "grid150_unsorted": (lambda s, dom: shuffled(grid5(150, s), s + 1), ())}
CASES.update(LARGE)
CASES.update(AMG_SMALL)

# (matrix seed, diagonal dominance): chosen so that the reference alone stops
# clear-cut at both flags and the pass cases' rows and residues fall as
# tests/test_pcgref_cpu.py asserts
SEEDS = {"band1": (0, 30.0), "band2": (0, 30.0), "band3": (0, 30.0), "band63": (0, 55.0), "band64": (0, 50.0),
         "band65": (0, 55.0), "band511": (0, 55.0), "band512": (0, 55.0), "band513": (0, 55.0),
         "band1023": (0, 55.0), "band1025": (0, 55.0), "pass2": (1, 50.0), "pass5": (0, 35.0),
         "arrow_first": (0, 30.0), "arrow_last": (0, 30.0), "arrow_mid": (0, 30.0), "diag1000": (0, 30.0),
         "unsorted": (0, 50.0)}

PRECISION = 1e-10


def matrix(name):
    fn, args = CASES[name]
    seed, dom = SEEDS.get(name, (0, DOM))
    return fn(*args, seed, dom)


def rhs(name, flag, n):
    """b and x0 with magnitudes in [0.5, 1.5], random signs."""
    rng = np.random.default_rng([n, 1 if flag else 0, 77])
    mk = lambda: rng.uniform(0.5, 1.5, n) * rng.choice([-1.0, 1.0], n)
    return mk(), mk()


def tile_layout(rp, block, cap):
    """Per tile of `block` rows: (passes, first nonzero % 4, last-end % 4, a row
    lies across a pass boundary, longest row), as tile_spmv_impl walks it: the
    passes start at the tile's first nonzero rounded down to 4."""
    rp = np.asarray(rp, np.int64)
    n = len(rp) - 1
    out = []
    for r0 in range(0, n, block):
        r1 = min(n, r0 + block)
        s, e = rp[r0], rp[r1]
        c0 = s & ~3
        bounds = np.arange(c0 + cap, e, cap)
        across = any(((rp[r0:r1] < B) & (rp[r0 + 1:r1 + 1] > B)).any() for B in bounds)
        out.append((len(bounds) + 1, int(s % 4), int(e % 4), bool(across), int(np.diff(rp[r0:r1 + 1]).max())))
    return out
