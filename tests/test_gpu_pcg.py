"""The PCG kernels (xfk_pcg.hip: k_cg_init_r, k_cg_spmv, k_cg_axpy, k_cg_dot,
the tile SpMV of xfk_spmv.h, the host loop of xfk_api.hip) against the
restated PCG of tests/pcgref.py, through kernels.pcg_solve_csr and
kernels.AmgProbe only.

One step, exactly: precision = 1e300 stops at the first test that may stop
(it >= 1), so the device returns x1, iters == 1 and er_1; both are held to
pcgref.rounding_bound, an a-priori bound with no fitted constant, at both
flags, with Jacobi on every zoo case and with the AMG on its grids.  Under the
AMG the V-cycle is an input (AmgProbe.apply on a probe built with the solver's
options; the cycle itself is held to tests/amgref.py elsewhere).

The whole solve at 1e-10: iters is the reference's stopping index (decided
clear-cut by the reference alone, tests/test_pcgref_cpu.py), er its er[k]
within 16 x the float64-versus-longdouble difference of the reference itself
(where the reference's step ends in exact termination its er[k] is its own
rounding, and er is held to the recursion's a-priori reach), the true residual
within precision + the recursion's drift, the solution within the stopping
rule's a-priori reach (pcgref.error_reach) of a direct solve.

Measured error / bound figures are printed by every test (pytest -s).
"""
import functools
import inspect
import os
import re

import numpy as np
import pytest

import pcgref as pr
from util import ROOT
from xfemm_amd import kernels

pytestmark = pytest.mark.gpu

LD = pr.LD
JACOBI_ONE = pr.SMALL + list(pr.LARGE)
AMG_ONE = list(pr.AMG_SMALL) + list(pr.LARGE)
# the two runs whose er_1 bound is above 1e-5 of er's scale (see one_step_case)
ER_BOUND_LOOSE = {("grid725", "amg", 1), ("grid1025", "amg", 1)}


@functools.lru_cache(maxsize=2)
def matrix(name):
    return pr.matrix(name)


def solver_amg_options():
    """The options xfk_pcg_solve_csr's hierarchy is built with: xfk_problem's defaults."""
    src = open(os.path.join(ROOT, "xfemm_amd", "csrc", "xfk_internal.h")).read()
    get = lambda nm: float(re.search(r"\b(?:int|double) %s = ([-0-9.e]+);" % nm, src).group(1))
    return dict(sweeps=int(get("amg_sweeps")), theta=get("amg_theta"), omega=get("amg_omega"),
                dense_max=int(get("amg_dense")), fold=int(get("amg_fold")), col16=int(get("amg_col16")),
                f32=int(get("amg_f32")), wlevel=int(get("amg_wlevel")))


class Cycle:
    """The solver's V-cycle of one matrix as the reference's M^-1, an estimate
    of its 2-norm (power iteration: it is symmetric positive definite) and
    the addition-chain count of one application (per level: the smoother's and
    the residual's rows of A, the rows of R and P; the dense coarsest product)."""

    def __init__(self, name):
        rp, col, val = matrix(name)
        self.probe = kernels.AmgProbe(rp, col, val, **solver_amg_options())
        I = self.probe.info()
        sw = solver_amg_options()["sweeps"]
        self.kv = sum((2 * sw + 1) * -(-lv["nnz"] // lv["n"]) + 2 * -(-lv["pnnz"] // max(1, lv["n"]))
                      for lv in I["level"]) + (I["level"][-1]["n"] if I["dense_coarse"] else 0)
        v = np.random.default_rng(3).standard_normal(len(rp) - 1)
        for _ in range(30):
            v /= np.linalg.norm(v)
            v = self.probe.apply(v)
        self.mnorm = float(np.linalg.norm(v))

    def __call__(self, r):
        return self.probe.apply(np.asarray(r, np.float64))


@functools.lru_cache(maxsize=1)
def cycle(name):
    return Cycle(name)


def test_probe_defaults_are_the_solvers_options():
    """The stand-alone solve builds its hierarchy with xfk_problem's defaults;
    AmgProbe's defaults are the same but for wlevel, where the solver takes
    the default W level (-2) and the probe none: Cycle passes the solver's."""
    o = solver_amg_options()
    dflt = {k: p.default for k, p in inspect.signature(kernels.AmgProbe.__init__).parameters.items() if k in o}
    assert {k: v for k, v in o.items() if k != "wlevel"} == {k: v for k, v in dflt.items() if k != "wlevel"}
    assert (o["wlevel"], dflt["wlevel"]) == (-2, -1)


# ---- one step, exactly --------------------------------------------------------

def one_step_case(name, precond, flag):
    rp, col, val = matrix(name)
    n = len(rp) - 1
    b, x0 = pr.rhs(name, flag, n)
    if precond == "amg":
        M = cycle(name)
        minv, kw = M, dict(mnorm=M.mnorm, kv=M.kv)
    else:
        minv, kw = pr.jacobi(rp, col, val), {}
    V, it, er = kernels.pcg_solve_csr(rp, col, val, b, x0, flag=flag, precision=1e300, precond=precond)
    s = pr.one_step(rp, col, val, b, x0, flag, minv)
    bd = pr.rounding_bound(rp, col, val, b, flag, s, **kw)
    ex = np.abs(np.asarray(V, LD) - s["x1"]).astype(np.float64)
    rx = float((ex / bd["x1"]).max())
    re_ = abs(er - float(s["er1"])) / bd["er"] if bd["er"] > 0 else (0.0 if er == float(s["er1"]) else np.inf)
    scale = float(np.abs(s["x1"]).max())
    print("one step %-16s %-6s flag=%d: x1 err/bound %.3f (bound <= %.1e of max|x1|), er err/bound %.3f "
          "(er_1 %.3e, bound %.1e)" % (name, precond, flag, rx, bd["x1"].max() / scale, re_, float(s["er1"]),
                                       bd["er"]))
    assert it == 1
    # a dropped entry moves x1 by >= 1e-4 of its scale, and r1 = r0 - alpha0 w0 by
    # as much of r0's, so er_1 by 1e-4 of er_0: neither can hide in its bound
    er0 = float(np.sqrt(s["g0"] / s["res_o"]))
    assert bd["x1"].max() <= 1e-5 * scale
    if (name, precond, flag) in ER_BOUND_LOOSE:
        # the cycle model's norm-wise terms at N > 500,000: 3.4e-4 and 2.5e-3 of er_1
        # measured; er_1 is pinned to that only, x1 as everywhere
        assert bd["er"] < float(s["er1"])
    else:
        assert bd["er"] <= 1e-5 * max(er0, float(s["er1"])), (bd["er"], er0, float(s["er1"]))
    assert rx <= 1.0 and re_ <= 1.0, (rx, re_)


@pytest.mark.parametrize("flag", [0, 1])
@pytest.mark.parametrize("name", JACOBI_ONE)
def test_one_step_jacobi(name, flag):
    one_step_case(name, "jacobi", flag)


@pytest.mark.parametrize("flag", [0, 1])
@pytest.mark.parametrize("name", AMG_ONE)
def test_one_step_amg(name, flag):
    one_step_case(name, "amg", flag)


def test_grid45_is_the_dense_coarsest_level():
    I = cycle("grid45").probe.info()
    assert I["levels"] == 1 and I["dense_coarse"]
    assert cycle("grid150").probe.info()["levels"] > 1


def test_cycle_of_unsorted_rows_is_the_cycle_of_sorted_rows():
    """The AMG setup takes rows in any column order: the same operator up to
    the order of its float64 sums and the f32 roundings of transfer entries
    that this moves across a rounding boundary (2^-24 relative on an entry); a
    hierarchy that lost an entry differs at 1e-2."""
    R = np.random.default_rng(11).standard_normal(150 * 150)
    a = cycle("grid150")(R)
    b = cycle("grid150_unsorted")(R)
    d = float(np.abs(a - b).max() / np.abs(a).max())
    print("unsorted vs sorted cycle: %.2e" % d)
    assert d <= 1e-6


# ---- the whole solve ----------------------------------------------------------

def whole_solve_case(name, precond, flag):
    rp, col, val = matrix(name)
    n = len(rp) - 1
    P = pr.PRECISION
    b, x0 = pr.rhs(name, flag, n)
    if precond == "amg":
        M = cycle(name)
        minv, minv64, mabs = M, M, lambda v: M.mnorm * float(v @ v)
    else:
        d = pr.diag_of(rp, col, val)
        minv, minv64, mabs = pr.jacobi(rp, col, val), pr.jacobi(rp, col, val, np.float64), lambda v: float(v @ (v / d))
    V, it, er = kernels.pcg_solve_csr(rp, col, val, b, x0, flag=flag, precision=P, precond=precond)
    ref = pr.pcg(rp, col, val, b, x0, flag, P, minv)
    r64 = pr.pcg(rp, col, val, b, x0, flag, P, minv64, dt=np.float64)
    k, e = ref["k"], [float(v) for v in ref["er"]]
    clear = e[k] <= P / 4 and all(v >= 4 * P for v in e[1:k])
    assert r64["k"] >= k
    self_diff = abs(float(r64["er"][k]) - e[k])
    tr = pr.true_residual(rp, col, val, b, V, minv)
    drift = pr.true_residual_drift(rp, col, val, b, ref, mabs)
    print("solve %-16s %-6s flag=%d: iters %d (ref %d, %s), er %.6e (ref %.6e, |f64 - ld| %.2e, err / (16 x that) "
          "%.3f), true residual %.3e (drift bound %.1e)"
          % (name, precond, flag, it, k, "clear-cut" if clear else "near tie: +-1", er, e[k], self_diff,
             abs(er - e[k]) / (16 * self_diff) if self_diff > 0 else (0 if er == e[k] else np.inf), tr, drift))
    assert np.isfinite(V).all()
    if precond == "jacobi":
        assert clear            # (test_pcgref_cpu.py holds the zoo to it)
    # a step that annihilates the residual to float64's last bit (exact
    # termination: N steps, a diagonal matrix) leaves the longdouble er[k] with
    # no digit that float64 could share: there er is held to the recursion's
    # a-priori reach instead
    exact = k >= 1 and e[k] <= pr.U * e[k - 1]
    if clear:
        assert it == k
        assert (er <= drift) if exact else (abs(er - e[k]) <= 16 * self_diff)
    else:
        assert abs(it - k) <= 1 and er <= P
    assert tr <= P + drift
    if n <= 5000:
        # the distance from a direct solve, bounded from the stopping rule alone
        # (pcgref.error_reach), not from V's own residual
        mu = None
        if precond == "amg":
            # the smallest eigenvalue of M^-1 A, M^-1 the cycle's matrix (its
            # asymmetry, 1e-8 of its largest entry, is averaged out)
            Minv = M(np.eye(n))
            Lc = np.linalg.cholesky(pr.csr(rp, col, val).toarray())
            mu = float(np.linalg.eigvalsh(Lc.T @ (0.5 * (Minv + Minv.T)) @ Lc)[0])
        reach = pr.error_reach(rp, col, val, ref["res_o"], P + drift, mu)
        xd = pr.direct_solve(rp, col, val, b)
        dist = lambda v: float(np.sqrt(np.sum((np.asarray(v, LD) - xd) ** 2)))
        big = float(np.abs(xd).max())
        print("      |V - direct|_2 %.3e, reach %.3e (%.1e of max|x|)" % (dist(V), reach, reach / big))
        assert dist(V) <= reach
        # the check has teeth: one entry off by 1e-6 of the solution's scale is out of reach
        Vbad = V.copy()
        Vbad[n // 2] += 1e-6 * big
        assert reach <= 1e-7 * big and dist(Vbad) > reach


@pytest.mark.parametrize("flag", [0, 1])
@pytest.mark.parametrize("name", pr.SMALL)
def test_whole_solve_jacobi(name, flag):
    whole_solve_case(name, "jacobi", flag)


@pytest.mark.parametrize("flag", [0, 1])
@pytest.mark.parametrize("name", list(pr.AMG_SMALL))
def test_whole_solve_amg(name, flag):
    whole_solve_case(name, "amg", flag)


# ---- edges of the contract -----------------------------------------------------

@pytest.mark.parametrize("precond,name", [("jacobi", "band513"), ("amg", "grid45"), ("amg", "grid150")])
def test_zero_right_hand_side(precond, name):
    rp, col, val = matrix(name)
    n = len(rp) - 1
    _, x0 = pr.rhs(name, 1, n)
    V, it, er = kernels.pcg_solve_csr(rp, col, val, np.zeros(n), x0, flag=0, precision=1e-10, precond=precond)
    assert it == 0 and er == 0 and not V.any()
    V, it, er = kernels.pcg_solve_csr(rp, col, val, np.zeros(n), x0, flag=1, precision=1e-10, precond=precond)
    assert it == 0 and er == 0 and V.tobytes() == x0.tobytes()       # spars.cpp:259


@pytest.mark.parametrize("precond,name", [("jacobi", "pass5"), ("amg", "grid150")])
def test_two_solves_are_bit_identical(precond, name):
    rp, col, val = matrix(name)
    b, x0 = pr.rhs(name, 1, len(rp) - 1)
    a = kernels.pcg_solve_csr(rp, col, val, b, x0, flag=1, precision=1e-10, precond=precond)
    c = kernels.pcg_solve_csr(rp, col, val, b, x0, flag=1, precision=1e-10, precond=precond)
    assert a[0].tobytes() == c[0].tobytes() and a[1:] == c[1:]


def test_exact_initial_guess_is_returned():
    """r0 == 0 exactly with b != 0: gamma_0 = delta_0 = 0 would make alpha
    0 / 0 and a NaN er that never stops; gamma_0 == 0 at iteration 0 is a
    stop, and the guess comes back untouched."""
    rp, col, val = matrix("diag1000")
    n = len(rp) - 1
    x0 = np.random.default_rng(5).choice([-1.0, 1.0], n)
    b = val * x0                    # exact: x0 = +-1
    V, it, er = kernels.pcg_solve_csr(rp, col, val, b, x0, flag=1, precision=1e-10)
    assert it == 0 and er == 0 and V.tobytes() == x0.tobytes()
