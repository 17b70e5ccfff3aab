"""Sharded time-harmonic solve (xfk_problem_create_harmonic_dist): the
Harmonic2D COCG with the AMG surrogate preconditioner over row blocks, as the
static sharded path -- each rank assembles its rows, exchanges the halo of
x / u before each SpMV, all-reduces the COCG partials after it, runs the
sharded AMG setup / V-cycle, and sums the successive-approximation change
over the ranks.  The Newton AC solver and Case-2 circuits run sharded too.

Driven through the in-process transport (one host thread per rank, all ranks
on cuda:0), every communicator recording its calls so that
kernels.check_comm_logs proves the issue order (same sequence on every rank,
matched sends / receives, the wait on every stream switch).

Tolerances: against the single-device solve 1e-6 of max|A| (linear) and 1e-5
(nonlinear successive approximation) -- the partial sums are grouped per rank,
so iterates differ in the last bits and both stop at the same COCG
criterion; one rank reproduces the single-device solve bit for bit.
"""
import threading

import numpy as np
import pytest

from util import rel_err
from xfemm_amd import kernels, synth

pytestmark = pytest.mark.gpu

TOL_LINEAR = 1e-6
TOL_NONLINEAR = 1e-5


def run_sharded(kw, nranks, solves=1, **opt):
    comms = kernels.Comm.local_group(nranks)
    for c in comms:
        c.record(1)
    probs = [kernels.Harmonic2DProblem(**kw, comm=comms[q], **opt) for q in range(nranks)]
    out = [None] * nranks
    err = [None] * nranks

    def work(q):
        try:
            for _ in range(solves):
                out[q] = (probs[q].solve(), probs[q].solution(), probs[q].dist_info())
        except Exception as ex:   # surfaced below
            err[q] = ex

    th = [threading.Thread(target=work, args=(q,)) for q in range(nranks)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    for p in probs:
        p.close()
    logs = [c.log() for c in comms]
    for c in comms:
        c.close()
    for e in err:
        if e is not None:
            raise e
    return out, logs


def single(kw, **opt):
    P = kernels.Harmonic2DProblem(**kw, **opt)
    r = P.solve()
    A = P.solution()
    P.close()
    return r, A


def test_one_rank_is_bit_identical_to_single_device():
    kw = synth.harmonic(30)
    r1, A1 = single(kw)
    ((rs, As, info),), _ = run_sharded(kw, 1)
    assert info["n_halo"] == 0 and info["n_own"] == len(kw["x"])
    assert rs["cg_iters"] == r1["cg_iters"]
    assert np.array_equal(As, A1)


@pytest.mark.parametrize("nranks", [2, 4])
@pytest.mark.parametrize("periodic", [None, "per", "anti"])
def test_sharded_linear_matches_single_device(nranks, periodic):
    kw = synth.harmonic(48, periodic=periodic is not None, anti=periodic == "anti")
    r1, A1 = single(kw)
    out, logs = run_sharded(kw, nranks)
    for rs, As, info in out:
        assert rs["precond"] == r1["precond"] == kernels.XFK_PRECOND_AMG
        assert rel_err(As, A1) <= TOL_LINEAR, (nranks, periodic, rel_err(As, A1))
        # the sharded V-cycle is the single-device one up to rounding
        assert abs(rs["cg_iters"] - r1["cg_iters"]) <= max(2, r1["cg_iters"] // 10)
    assert sum(o[2]["n_own"] for o in out) == len(kw["x"])
    kernels.check_comm_logs(logs)


@pytest.mark.parametrize("nranks", [2, 4])
def test_sharded_jacobi_matches_single_device(nranks):
    kw = synth.harmonic(32, circuits=False)
    r1, A1 = single(kw, precond="jacobi")
    out, logs = run_sharded(kw, nranks, precond="jacobi")
    for rs, As, _ in out:
        assert rs["precond"] == kernels.XFK_PRECOND_JACOBI
        assert rel_err(As, A1) <= TOL_LINEAR
    kernels.check_comm_logs(logs)


@pytest.mark.parametrize("nranks", [2, 4])
def test_sharded_nonlinear_matches_single_device(nranks):
    """Successive approximation: the elements read V at their halo nodes (one
    exchange per pass), the change |dV| / |V| is summed over the ranks, so
    every rank takes the same number of passes."""
    kw = synth.harmonic(36, nonlinear=True)
    r1, A1 = single(kw)
    out, logs = run_sharded(kw, nranks, solves=2)
    assert r1["newton_iters"] > 1
    for rs, As, _ in out:
        assert rel_err(As, A1) <= TOL_NONLINEAR
        assert abs(rs["newton_iters"] - r1["newton_iters"]) <= 2
        assert rs["newton_iters"] == out[0][0]["newton_iters"]
    kernels.check_comm_logs(logs)


def _oracle(kw):
    from oracle import harmonic as oh
    from util import synth_to_oracle
    pr, mesh, kk = synth_to_oracle(kw)
    Ao, _, circ_o = oh.solve(pr, mesh)
    return pr, mesh, kk, Ao, circ_o


@pytest.mark.parametrize("nranks", [2, 4])
@pytest.mark.parametrize("kind,n", [("planar", 14), ("planar", 20), ("periodic", 14), ("anti", 16), ("axi", 12)])
def test_sharded_newton_ac_matches_oracle(nranks, kind, n):
    """The Newton AC solver ([ACSolver] = 1, KludgeSolve, cspars.cpp:1000-1060)
    over row blocks: the auxiliary matrices are assembled per rank (their
    periodic map keeps the entries of the rows a rank assembles), the
    products read V and the step at the halo (one exchange each), the line
    search's dot products are summed over the ranks.  Against the oracle's
    converged answer with the single-device test's tolerance
    (tests/test_gpu_newton_ac.py).

    Not periodic 16: there the path decides the answer.  The first Newton
    pass starts from the same V and the same matrices (auxiliary, M, b equal
    to 1e-9 on 2 ranks, compared entry by entry from a temporary dump), but the row-block AMG is
    another preconditioner, so the inner COCG stops at lprec after other
    iterations (4 vs 1); on 2 ranks pass 10 then finds KludgeSolve's start
    residual below lprec, takes no step, and the loop stops on a zero change
    with |A - Ac| 3.9e-2 -- the reference's own early exit (harmonic2d.cpp
    loop, cspars.cpp:1000-1060), on which the single device passes only
    narrowly (1.62e-5 against 1.70e-5).  The same exit takes the single
    device on antiperiodic 16 (4.2e-2, 12 passes) while the row blocks pass
    there (1.1e-5): luck of the path both ways, measured round 5."""
    import copy
    from oracle import harmonic as oh
    from test_gpu_newton_ac import _case, _tol
    from util import CONVERGED_PRECISION
    kw = _case(kind, n)
    pr, mesh, kk, Ao, circ_o = _oracle(kw)
    pr2 = copy.deepcopy(pr)
    pr2.Precision = CONVERGED_PRECISION
    Ac, _, _ = oh.solve(pr2, mesh)
    r1, A1 = single(kk)
    out, logs = run_sharded(kk, nranks)
    for rs, As, _ in out:
        assert rs["newton_iters"] >= 2 and rs["newton_iters"] == out[0][0]["newton_iters"]
        assert rel_err(As, Ac) <= _tol(Ao, Ac), (kind, n, nranks, rel_err(As, Ac), _tol(Ao, Ac))
        assert np.array_equal(As, out[0][1])
    print("sharded newton AC %s %d x%d: |A - Ac| %.3e (one device %.3e), %d / %d passes" % (
        kind, n, nranks, rel_err(out[0][1], Ac), rel_err(A1, Ac), out[0][0]["newton_iters"], r1["newton_iters"]))
    kernels.check_comm_logs(logs)


@pytest.mark.parametrize("nranks", [2, 4])
@pytest.mark.parametrize("cells,nonlinear,periodic,ac", [(20, False, False, 0), (30, False, "anti", 0),
                                                         (16, True, True, 0), (14, True, False, 1),
                                                         (14, True, True, 1)])
def test_sharded_case2_circuit_matches_oracle(nranks, cells, nonlinear, periodic, ac):
    """Case-2 circuits (a specified current in a conducting region: the
    bordered system [A C; C^T D], solved through the Schur complement) over row
    blocks: each rank holds the border columns of its owned rows, C . y is
    summed over the ranks, the small dense solve for the circuit unknowns runs
    on every rank on the same sums.  A and the voltage gradient against the
    oracle (tests/test_gpu_harmonic.py::test_harmonic_case2_circuit_matches_oracle,
    tests/test_gpu_newton_ac.py::test_newton_ac_case2_matches_oracle)."""
    kw = synth.harmonic(cells, nonlinear=nonlinear, periodic=bool(periodic), anti=periodic == "anti")
    kw["circuits"][1] = dict(type=0, amps_re=2.0, amps_im=0.5)
    kw["ac_solver"] = ac
    pr, mesh, kk, Ao, circ_o = _oracle(kw)
    assert circ_o[1][0] == 2
    if ac:
        import copy
        from oracle import harmonic as oh
        from test_gpu_newton_ac import _tol
        from util import CONVERGED_PRECISION
        pr2 = copy.deepcopy(pr)
        pr2.Precision = CONVERGED_PRECISION
        Ac, _, circ_c = oh.solve(pr2, mesh)
        tol, dv_tol, ref, circ_ref = _tol(Ao, Ac), 1e-4, Ac, circ_c
    else:
        tol = 1e-5 if nonlinear else 1e-6
        dv_tol, ref, circ_ref = tol, Ao, circ_o
    comms = kernels.Comm.local_group(nranks)
    for c in comms:
        c.record(1)
    probs = [kernels.Harmonic2DProblem(**kk, comm=comms[q]) for q in range(nranks)]
    out = [None] * nranks
    err = [None] * nranks

    def work(q):
        try:
            probs[q].solve()
            out[q] = (probs[q].solution(), probs[q].circuits())
        except Exception as ex:   # surfaced below
            err[q] = ex

    th = [threading.Thread(target=work, args=(q,)) for q in range(nranks)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    for p in probs:
        p.close()
    logs = [c.log() for c in comms]
    for c in comms:
        c.close()
    for e in err:
        if e is not None:
            raise e
    for A, (cc, J, dV) in out:
        assert rel_err(A, ref) <= tol, (rel_err(A, ref), tol)
        assert cc[1] == 2
        assert abs(dV[1] - circ_ref[1][2]) <= dv_tol * abs(circ_ref[1][2]), (dV[1], circ_ref[1][2])
        assert dV[1] == out[0][1][2][1]
    kernels.check_comm_logs(logs)
