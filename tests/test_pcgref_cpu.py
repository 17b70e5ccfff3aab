"""The restated PCG and the matrix zoo of tests/pcgref.py on the CPU: the
reference solves its own cases, the zoo sits on both sides of every threshold
of the PCG kernels (read from the sources, so a retuned constant fails here
instead of the coverage silently moving off its edge), the reference alone
decides every whole-solve iteration count clear-cut, and the stand-alone
entries refuse a malformed CSR before any device work."""
import os
import re

import numpy as np
import pytest

import pcgref as pr
from util import ROOT
from xfemm_amd import kernels

CSRC = os.path.join(ROOT, "xfemm_amd", "csrc")
CONSTANTS = {
    "kCgBlock": ("xfk_spmv.h", r"constexpr int kCgBlock = (\d+);", 512),
    "kCgCapSlots": ("xfk_spmv.h", r"constexpr int kCgCap = (\d+) \* kCgBlock;", 8),
    "kAxBlock": ("xfk_pcg.hip", r"constexpr int kAxBlock = (\d+);", 256),
    "kAxGrid": ("xfk_pcg.hip", r"constexpr int kAxGrid = (\d+);", 1024),
}


def constant(name):
    fn, rx, _ = CONSTANTS[name]
    m = re.search(rx, open(os.path.join(CSRC, fn)).read(), re.S)
    assert m, "%s: %r no longer matches %s" % (name, rx, fn)
    return int(m.group(1))


@pytest.fixture(scope="module")
def solved():
    """Every small case at both flags: the reference's whole solve, once."""
    out = {}
    for name in pr.SMALL:
        rp, col, val = pr.matrix(name)
        for flag in (0, 1):
            b, x0 = pr.rhs(name, flag, len(rp) - 1)
            out[name, flag] = (rp, col, val, b, x0,
                               pr.pcg(rp, col, val, b, x0, flag, pr.PRECISION, pr.jacobi(rp, col, val), keep=True))
    return out


def test_constants_are_what_the_zoo_was_laid_out_for():
    for name, (_, _, want) in CONSTANTS.items():
        assert constant(name) == want, name


def test_zoo_is_spd_dominant_and_in_range():
    for name in pr.SMALL + list(pr.AMG_SMALL):
        rp, col, val = pr.matrix(name)
        n = len(rp) - 1
        rows = np.repeat(np.arange(n), np.diff(rp))
        A = pr.csr(rp, col, val)
        assert abs(A - A.T).max() == 0, name
        d = pr.diag_of(rp, col, val)
        off = np.asarray(abs(A).sum(axis=1)).ravel() - d
        assert (d > 0).all() and (d >= off * (1 - 1e-12)).all() and (d > off * 1.1).any(), name
        if name in pr.SMALL:
            assert (d >= 29 * off).all(), name
            o = np.abs(val[rows != col])
            assert o.size == 0 or (o.min() >= 0.1 and o.max() <= 1.0), name
        for k in range(n):           # no column twice in a row
            c = col[rp[k]:rp[k + 1]]
            assert len(set(c.tolist())) == c.size
        for flag in (0, 1):
            for v in pr.rhs(name, flag, n):
                assert np.abs(v).min() >= 0.5 and np.abs(v).max() <= 1.5


def test_reference_solves_every_case_up_to_5000(solved):
    """Every zoo case with N <= 5000 (grid45 with Jacobi too) against a direct
    solve, within what the stopping rule alone allows (pcgref.error_reach)."""
    cases = dict(solved)
    rp, col, val = pr.matrix("grid45")
    for flag in (0, 1):
        b, x0 = pr.rhs("grid45", flag, len(rp) - 1)
        cases["grid45", flag] = (rp, col, val, b, x0,
                                 pr.pcg(rp, col, val, b, x0, flag, pr.PRECISION, pr.jacobi(rp, col, val)))
    assert all(len(pr.matrix(n)[0]) - 1 > 5000 for n in pr.CASES if (n, 0) not in cases)
    for (name, flag), (rp, col, val, b, x0, ref) in cases.items():
        xd = pr.direct_solve(rp, col, val, b)
        err = float(np.sqrt(np.sum((ref["x"] - xd) ** 2)))
        assert ref["er"][ref["k"]] <= pr.PRECISION
        assert err <= pr.error_reach(rp, col, val, ref["res_o"], pr.PRECISION), (name, flag, err)
        assert pr.true_residual(rp, col, val, b, ref["x"], pr.jacobi(rp, col, val)) <= pr.PRECISION


def test_one_step_is_the_first_iterate(solved):
    for (name, flag), (rp, col, val, b, x0, ref) in solved.items():
        s = pr.one_step(rp, col, val, b, x0, flag, pr.jacobi(rp, col, val))
        x1 = ref["xs"][1]
        assert np.abs(s["x1"] - x1).max() <= 64 * np.finfo(pr.LD).eps * np.abs(x1).max(), (name, flag)
        assert abs(s["er1"] - ref["er"][1]) <= 1e-6 * pr.U * max(1.0, float(ref["er"][1])) \
            or abs(s["er1"] - ref["er"][1]) <= 64 * np.finfo(pr.LD).eps * float(ref["er"][0]), (name, flag)
        bd = pr.rounding_bound(rp, col, val, b, flag, s)
        assert np.isfinite(bd["x1"]).all() and np.isfinite(bd["er"])
        # the bound leaves the teeth in: a dropped or doubled entry moves x1 by >= 1e-4 relative
        assert bd["x1"].max() <= 1e-10 * np.abs(np.asarray(s["x1"], np.float64)).max(), (name, flag)


def test_stop_is_clear_cut(solved):
    """er[k-1] >= 4 precision and er[k] <= precision / 4: no rounding of a
    float64 evaluation can move the stopping index."""
    for (name, flag), (*_, ref) in solved.items():
        k, er = ref["k"], ref["er"]
        assert k >= 1 and er[k] <= pr.PRECISION / 4, (name, flag, k, float(er[k]))
        assert all(e >= 4 * pr.PRECISION for e in er[1:k]), (name, flag)
        assert k == 1 or er[k - 1] >= 4 * pr.PRECISION, (name, flag, float(er[k - 1]))


def test_float64_reference_stops_at_the_same_index(solved):
    for (name, flag), (rp, col, val, b, x0, ref) in solved.items():
        r64 = pr.pcg(rp, col, val, b, x0, flag, pr.PRECISION, pr.jacobi(rp, col, val, np.float64), dt=np.float64)
        assert r64["k"] == ref["k"], (name, flag)


def test_zoo_straddles_the_tile_spmv():
    block, cap = constant("kCgBlock"), constant("kCgCapSlots") * constant("kCgBlock")
    lay = {name: pr.tile_layout(pr.matrix(name)[0], block, cap) for name in pr.SMALL}
    tiles = [t for v in lay.values() for t in v]
    assert any(t[0] == 1 for t in tiles) and any(t[0] == 2 for t in tiles) and any(t[0] >= 5 for t in tiles)
    assert [t[0] for t in lay["pass2"][:2]] == [2, 2] and all(t[0] >= 5 for t in lay["pass5"][:2])
    # a row across a pass boundary in every multi-pass tile of the pass cases
    for name in ("pass2", "pass5", "unsorted"):
        assert all(t[3] for t in lay[name] if t[0] > 1), name
    # a row longer than a whole pass: first, last, and inside the second tile
    for name, where in (("arrow_first", 0), ("arrow_last", -1), ("arrow_mid", 1)):
        assert lay[name][where][4] > cap and sum(t[4] > cap for t in lay[name]) == 1, name
    assert 768 // block == 1 and 768 % block not in (0, block - 1)
    # the quad path and the per-entry path meet at every residue, at both ends
    assert {t[1] for t in tiles} == {0, 1, 2, 3} and {t[2] for t in tiles} == {0, 1, 2, 3}
    # sizes on both sides of one tile and of one wave
    ns = {len(pr.matrix(n)[0]) - 1 for n in pr.SMALL}
    assert {1, 2, 3, 63, 64, 65, block - 1, block, block + 1, 2 * block - 1, 2 * block + 1} <= ns


def test_zoo_straddles_the_streaming_update():
    full = 2 * constant("kAxBlock") * constant("kAxGrid")        # rows one full grid covers, two per thread
    large = sorted(fn_args[1][0] ** 2 for fn_args in pr.LARGE.values())
    small = max(len(pr.matrix(n)[0]) - 1 for n in pr.SMALL)
    assert small < full < large[0] < 2 * full < large[1]
    assert all(n % 2 == 1 for n in large)                            # the scalar tail
    ns = {len(pr.matrix(n)[0]) - 1 for n in pr.SMALL}
    assert 1 in ns and any(n % 2 == 0 for n in ns)                   # npair == 0; no tail


# ---- what the stand-alone entries refuse (host checks: no device needed) -----

XFK_ERR_ARG, XFK_ERR_SINGULAR = -1, -3      # include/xfemm_kernels.h


def _solve(precond):
    return lambda rp, col, val: kernels.pcg_solve_csr(np.array(rp), np.array(col), np.array(val, float),
                                                      np.ones(len(rp) - 1), precond=precond)


def _probe(rp, col, val):
    return kernels.AmgProbe(np.array(rp), np.array(col), np.array(val, float))


@pytest.mark.parametrize("entry", [_solve("jacobi"), _solve("amg"), _probe], ids=["jacobi", "amg", "probe"])
@pytest.mark.parametrize("what,rp,col,val", [
    ("same column twice", [0, 3, 5], [0, 1, 1, 0, 1], [4, -1, -1, -2, 4]),
    ("same column twice", [0, 2, 5], [0, 1, 1, 0, 1], [4, -1, 2, -1, 2]),           # the diagonal itself
    ("column index out of range", [0, 2, 4], [0, 2, 0, 1], [4, -1, -1, 4]),
    ("column index out of range", [0, 2, 4], [0, -1, 0, 1], [4, -1, -1, 4]),
    ("row pointers descend", [0, 2, 1, 3], [0, 1, 2], [4, -1, 4]),
    ("rowptr\\[0\\] is not 0", [1, 2, 3], [0, 0, 1], [0, 4, 4]),
])
def test_malformed_csr_is_refused(entry, what, rp, col, val):
    with pytest.raises(kernels.XfkError, match="xfk error %d: CSR: .*%s" % (XFK_ERR_ARG, what)):
        entry(rp, col, val)


@pytest.mark.parametrize("entry", [_solve("jacobi"), _solve("amg"), _probe], ids=["jacobi", "amg", "probe"])
def test_row_without_a_diagonal_is_refused(entry):
    with pytest.raises(kernels.XfkError, match="xfk error %d: row without a diagonal entry" % XFK_ERR_SINGULAR):
        entry([0, 2, 3], [0, 1, 0], [4, -1, -1])
