"""The Galerkin products with packed sort words (xfk_amg_spgemm.hip:
k_spgemm_sort<..., PACK>) against the generic (column, value) network that
stays in the tree (the prolongator and sharded levels keep using it).

XFK_SPGEMM_PACK=0 sends A P and R (A P) through the generic network; it is read
per setup, so both hierarchies are built in this process, each from a fresh
AmgProbe (no capacity hints carried over), and every operator of every level
is compared byte for byte: rowptr, col and val of A, P, R, P~ (A P's
pattern) and R~.  A_1 = R (A P) carries A P's values, and everything below
carries A_1's.  There is no tolerance anywhere in this file.

Matrices: synth.magnetostatic(n) for n = 8 (level 0 below one workgroup), 33
and 70 (1156 and 5041 rows: partial last wavefront and slab for every W);
the 12-cell mesh with k dense weak couplings added to a few rows, which moves
level 0's products up the capacity classes (the classes reached are printed
and checked: both call sites sit in different classes, and the long rows share
their wavefronts with the mesh's short ones); and a block matrix with
degenerate rows: Dirichlet (identity) rows whose products are empty, an
isolated pair and a star whose rows of A P fall on one column (one summation
chain of 2 and of 7 products), an isolated node.
"""
import hashlib
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

from xfemm_amd import kernels, synth

pytestmark = pytest.mark.gpu
DENSE = 16


class _env:
    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        for k, v in self.kv.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


_mesh = {}


def mesh_matrix(n):
    if n not in _mesh:
        P = kernels.Static2DProblem(**synth.magnetostatic(n), precond="amg")
        P.solve()
        rp, col, val, _ = P.csr()
        P.close()
        A = sp.csr_matrix((val, col, rp), shape=(len(rp) - 1,) * 2)
        A.sort_indices()
        _mesh[n] = A
    return _mesh[n]


def with_dense_rows(A, k, rows=(5, 40, 41, 90)):
    """k weak symmetric couplings from each of a few rows to spread-out columns
    (1e-3 of the row's diagonal, the diagonals raised by as much: still SPD)."""
    N = A.shape[0]
    B = A.tolil(copy=True)
    for q, i in enumerate(rows):
        d = A[i, i]
        for j in np.unique((i + 7 + 11 * np.arange(k) + q) % N):
            if j == i or B[i, j] != 0:
                continue
            w = 1e-3 * abs(d)
            B[i, j] = B[j, i] = -w
            B[i, i] += w
            B[j, j] += w
    B = B.tocsr()
    B.sort_indices()
    return B


def degenerate_matrix():
    M = mesh_matrix(12).tolil(copy=True)
    for i in range(0, M.shape[0], 13):   # identity rows: no strong coupling, empty P rows
        M[i, :] = 0
        M[:, i] = 0
        M[i, i] = 1.0
    pair = sp.csr_matrix(np.array([[2.0, -1.0], [-1.0, 2.5]]))
    m = 6
    star = np.zeros((m + 1, m + 1))
    w = 1.0 + 0.1 * np.arange(1, m + 1) / 3.0
    star[0, 1:] = star[1:, 0] = -w
    star[0, 0] = w.sum() + 0.3
    star[np.arange(1, m + 1), np.arange(1, m + 1)] = w + 0.7
    lone = sp.csr_matrix(np.array([[3.0]]))
    A = sp.block_diag([M.tocsr(), pair, sp.csr_matrix(star), lone], format="csr")
    A.eliminate_zeros()
    A.sort_indices()
    return A


def hierarchy(A, pack, capfd=None, **kw):
    """Every operator of a fresh hierarchy as bytes, and the capacity classes it measured."""
    kw.setdefault("dense_max", DENSE)
    kernels.forget_amg_hints()
    with _env(XFK_SPGEMM_PACK=None if pack else "0", XFK_AMG_HINTS_PRINT="1"):
        if capfd is not None:
            capfd.readouterr()
        pr = kernels.AmgProbe(A.indptr, A.indices, A.data, **kw)
        err = capfd.readouterr().err if capfd is not None else ""
    I = pr.info()
    ops = {}
    for l in range(I["levels"]):
        sels = {"A": pr.A | pr.PLAIN_COLS}
        if l < I["levels"] - 1:
            sels.update(P=pr.P, R=pr.R | pr.PLAIN_COLS | pr.F64_VALS)
            if I["level"][l]["fnnz"] > 0:
                sels["PF"] = pr.PF | pr.PLAIN_COLS | pr.F64_VALS
                if l > 0:
                    sels["RF"] = pr.RF
        for name, sel in sels.items():
            sh, rp, cl, v = pr.csr(l, sel)
            ops[(l, name)] = (sh, rp.tobytes(), cl.tobytes(), v.tobytes())
    pr.close()
    kernels.forget_amg_hints()
    caps = {(int(a), int(b)): int(c) for a, b, c in re.findall(r"cap\[(\d+)\.(\d+)\]=(\d+)", err)}
    return ops, caps, I


def assert_same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert a[k][0] == b[k][0], ("shape", k)
        for what, x, y in zip(("rowptr", "col", "val"), a[k][1:], b[k][1:]):
            assert x == y, (what, k)


@pytest.mark.parametrize("n", [8, 33, 70])
@pytest.mark.parametrize("f32", [1, 0])
def test_mesh_hierarchy_keeps_every_bit(n, f32, capfd):
    A = mesh_matrix(n)
    new, caps, I = hierarchy(A, True, capfd, f32=f32)
    old, caps0, _ = hierarchy(A, False, capfd, f32=f32)
    print("n", n, "rows", A.shape[0], "levels", [(x["n"], x["nnz"]) for x in I["level"]], "caps", caps)
    assert I["levels"] >= 2 and (0, "PF") in new and (1, "A") in new
    assert caps == caps0 and (0, 1) in caps and (0, 2) in caps
    assert_same(new, old)


_dense_caps = {}


@pytest.mark.parametrize("k", [4, 12, 30])
def test_dense_couplings_move_level0_up_the_classes(k, capfd):
    A = with_dense_rows(mesh_matrix(12), k)
    new, caps, I = hierarchy(A, True, capfd, f32=0)
    old, caps0, _ = hierarchy(A, False, capfd, f32=0)
    print("k", k, "levels", [(x["n"], x["nnz"]) for x in I["level"]], "caps", caps)
    assert caps == caps0
    _dense_caps[k] = (caps[(0, 1)], caps[(0, 2)])
    assert_same(new, old)


def test_dense_cases_reach_the_wider_classes():
    """The three cases above run level 0's A P and R (A P) in more than the
    mesh's own classes: the 16-lane and the 32-lane instance are among them."""
    assert len(_dense_caps) == 3, "runs after the dense cases"
    reached = {c for pair in _dense_caps.values() for c in pair}
    print("level-0 classes:", _dense_caps)
    assert reached >= {128, 256}, reached
    assert len(reached) >= 3, reached


def test_degenerate_rows(capfd):
    A = degenerate_matrix()
    new, caps, I = hierarchy(A, True, capfd, f32=0)
    old, _, _ = hierarchy(A, False, capfd, f32=0)
    assert_same(new, old)
    # the rows the case is there for, read from P~ (A P's pattern) of level 0
    sh, rp, cl, v = new[(0, "PF")]
    rp = np.frombuffer(rp, np.int32)
    cl = np.frombuffer(cl, np.int32)
    ln = np.diff(rp)
    N = A.shape[0]
    print("P~ row lengths: min", ln.min(), "tail", ln[-10:], "empty rows", int((ln == 0).sum()))
    assert (ln == 0).sum() >= 1                       # empty product rows
    star = slice(N - 8, N - 1)                        # the star's 7 rows: one column each, the same one
    assert (ln[star] == 1).all() and len(set(cl[rp[N - 8]:rp[N - 1]])) == 1
    assert (ln[N - 10:N - 8] == 1).all()              # the pair


def test_two_fresh_setups_give_identical_bytes():
    A = mesh_matrix(33)
    a, _, _ = hierarchy(A, True)
    b, _, _ = hierarchy(A, True)
    assert_same(a, b)


def _solve_reports(kw, small_hint):
    out = []
    kernels.forget_amg_hints()
    P = kernels.Static2DProblem(**kw, precond="amg", amg_dense=DENSE)
    with _env(XFK_AMG_TEST_SMALL_HINT="1" if small_hint else None):
        for q in range(3):   # measured (stores the hint), then two hinted setups
            r = P.solve(rebuild_symbolic=q > 0)
            out.append((hashlib.sha256(P.solution().tobytes()).hexdigest(), int(r["cg_iters"]),
                        int(r["amg_levels"]), float(r["amg_op_complexity"]).hex()))
    P.close()
    kernels.forget_amg_hints()
    return out


def test_overflow_redo_keeps_every_bit():
    """A too-small stored capacity (16 slots): level 0's packed instance
    overflows, the hierarchy is rebuilt with measured capacities."""
    kw = synth.magnetostatic(49)
    with _env(XFK_SPGEMM_PACK=None):
        ovf = _solve_reports(kw, True)
        plain = _solve_reports(kw, False)
    with _env(XFK_SPGEMM_PACK="0"):
        ovf0 = _solve_reports(kw, True)
    print(ovf, plain, ovf0)
    assert ovf[0] == ovf[1] == ovf[2]
    assert ovf == plain and ovf == ovf0
