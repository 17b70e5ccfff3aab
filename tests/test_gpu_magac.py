"""Time-harmonic post-processing on the device (xfk_magpost_ac.hip, the
xfk_mag_ac_ entry points) against the restatement of fpproc at Frequency != 0
(tests/magacref.py, pinned by tests/test_magac_cpu.py).

Bounds: element B to 1e-12 of max |B|; every integral type to 1e-12 of the sum
of the absolute terms.  With nothing selected every type is 0 and type 25, the
centroid, is NaN + NaN j.  The identities on the device's own solve hold within
the harmonic solve's parity bound, 1e-5.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import magacref as R
import magpostref as M
import postproc
from oracle import femfile
from oracle import harmonic as oh
from util import ROOT, kernel_kwargs, synth_to_oracle
from xfemm_amd import fsolver, kernels, synth

pytestmark = pytest.mark.gpu

TOL = 1e-12
SOLVE_TOL = 1e-5
XFK_ERR_ARG, XFK_ERR_UNSUPPORTED = -1, -5


def _workgroup():
    txt = open(os.path.join(ROOT, "xfemm_amd", "csrc", "xfk_potential.h")).read()
    return int(re.search(r"constexpr int kPotQBlock = (\d+);", txt).group(1))


def _check_integrals(P, Rf, sel):
    z, s = Rf.block_integrals(sel)
    raw = P.block_integrals_complex(sel)["raw"]
    for t in range(26):
        if t == 25 and not np.isfinite(z[25]):
            assert np.isnan(raw[25].real) and np.isnan(raw[25].imag)
            continue
        assert abs(raw[t] - z[t]) <= TOL * s[t], "type %d: device %r, restated %r, scale %.3e" % (t, raw[t], z[t], s[t])
    for t in range(18, 24):
        assert raw[t] == 0
    return raw


def _check_all(P, kw, A, depth, selections):
    Rf = R.MagAcPost(kw, A, depth=depth, circuits=P.circuits())
    B = P.element_b_complex()
    Br = Rf.element_b_all()
    assert np.abs(B - Br).max() <= TOL * np.abs(Br).max()
    for sel in selections:
        _check_integrals(P, Rf, sel)


CASES = {
    "planar": lambda: synth.harmonic(8),
    "planar_no_circuits": lambda: synth.harmonic(8, circuits=False),
    "planar_nonlinear": lambda: synth.harmonic(8, nonlinear=True),
    "planar_periodic": lambda: synth.harmonic(8, periodic=True),
    "axi": lambda: synth.harmonic_axisymmetric(8),
    "axi_external": lambda: synth.harmonic_axisymmetric(8, external=True),
    "axi_nonlinear": lambda: synth.harmonic_axisymmetric(8, nonlinear=True),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_device_against_restatement(name):
    pr, mesh, kw = synth_to_oracle(CASES[name]())
    nl = len(kw["labels"])
    sels = [np.ones(nl, bool), np.zeros(nl, bool), [1], [2, nl - 1], list(range(1, nl))]
    P = kernels.Harmonic2DProblem(**kw)
    P.set_depth(37.0)
    P.solve()
    _check_all(P, kw, P.solution(), 37.0, sels)
    # ... and with A set from the oracle's solution (the circuit results stay the device's)
    Ao, _, _ = oh.solve(pr, mesh)
    P.set_solution_complex(Ao)
    _check_all(P, kw, Ao, 37.0, sels)
    P.solve()                                       # a solve replaces the given solution again
    _check_all(P, kw, P.solution(), 37.0, sels[:1])
    P.close()


def _strip(ne, axi):
    """tests/magpostref.py's strip as a harmonic problem: air, a lossy
    lamination, a hysteretic anisotropic block, a conducting coil in a Case-0
    circuit; a random complex A"""
    kw, A = M.strip_problem(ne, axi=axi)
    kw["blocks"] = [dict(mu_x=1.0, mu_y=1.0), dict(mu_x=900.0, mu_y=400.0, LamFill=0.9, Lam_d=0.35, Cduct=2.0,
                                                    Theta_hx=9.0, Theta_hy=4.0),
                    dict(mu_x=1.05, mu_y=1.1, Theta_hx=20.0, Theta_hy=20.0, J_re=0.3, J_im=-0.2),
                    dict(mu_x=1.0, mu_y=1.0, J_re=1.25, J_im=0.5, Cduct=58.0)]
    kw["circuits"] = [dict(type=1, dvolts_re=0.02, dvolts_im=-0.01)]
    kw["frequency"] = 400.0
    rng = np.random.default_rng(ne)
    A = A * np.exp(1j * rng.uniform(0, 2 * np.pi, len(A)))
    return kw, A


@pytest.mark.parametrize("axi", [False, True])
def test_reduction_shapes(axi):
    c = _workgroup()
    for ne in (1, c - 1, c, c + 1, 2 * c + 3):
        kw, A = _strip(ne, axi)
        if axi:            # nodes on the axis: the first element has two, the second one
            assert kw["x"][0] == 0.0 and kw["x"][1] == 0.0 and kw["x"][2] > 0.0
        P = kernels.Harmonic2DProblem(**kw)
        P.set_solution_complex(A)
        P.set_depth(12.5)
        nl = len(kw["labels"])
        present = np.unique(kw["lbl"])
        _check_all(P, kw, A, 12.5, [np.ones(nl, bool), [int(present[-1])], np.zeros(nl, bool)])
        P.close()


def test_repeatability_single_and_batch():
    pr, mesh, kw = synth_to_oracle(synth.harmonic(8))
    nl = len(kw["labels"])
    sel = [1, 2, 4]
    P = kernels.Harmonic2DProblem(**kw)
    P.solve()
    A = P.solution()
    a = P.block_integrals_complex(sel)["raw"]
    b = P.block_integrals_complex(sel)["raw"]
    assert a.tobytes() == b.tobytes()
    B = P.element_b_complex()
    for k in range(26):
        assert P.block_integral_complex(sel, k) == a[k] or (k == 25 and np.isnan(a[k]))
    assert a[6] == a[3] + a[4]
    assert a[17] == a[2]
    cc = P.circuits()
    P.close()
    Q = kernels.Harmonic2DProblem(**kw)      # a fresh problem, the same A
    Q.set_solution_complex(A)                # (k_mag_ac_a makes A in the operation order of solution())
    assert Q.block_integrals_complex(sel)["raw"].tobytes() == a.tobytes()
    assert Q.element_b_complex().tobytes() == B.tobytes()
    Q.close()


def test_identities_on_the_device_solve():
    w = 2. * np.pi * 60.0
    for theta in (0.0, 12.0):
        pr, mesh, kw = synth_to_oracle(R.identity_problem(20, theta, precision=1e-8))
        P = kernels.Harmonic2DProblem(**kw)
        P.solve()
        P.set_depth(30.0)
        z = P.block_integrals_complex(np.ones(4, bool))["raw"]
        zs = P.block_integrals_complex([2])["raw"]
        P.close()
        if theta == 0.0:
            gap = abs(z[0] - 4. * z[2]) / abs(4. * z[2])
            print("type-0 identity on the device's solve: %.3e" % gap)
        else:
            want = -(w / 2.) * zs[0].imag
            gap = abs(z[6].real - want) / abs(want)
            print("power balance on the device's solve: %.3e" % gap)
        assert gap <= SOLVE_TOL


def _refused(call, code, word):
    with pytest.raises(kernels.XfkError) as ei:
        call()
    assert ("xfk error %d" % code) in str(ei.value) and word in str(ei.value), str(ei.value)


def test_refusals():
    sel = [0]
    # a static problem, a potential problem
    S = kernels.Static2DProblem(**synth.magnetostatic(8))
    for f in (lambda: S.block_integrals_complex(sel), S.element_b_complex, lambda: S.block_integral_complex(sel, 2),
              lambda: S.set_solution_complex(np.zeros(S.n_nodes, complex)), lambda: S.time_postproc_complex(1)):
        _refused(f, XFK_ERR_ARG, "use xfk_mag_*")
    assert S.solve()["cg_iters"] > 0
    S.close()
    kwp, V = postproc.synthetic(6, 5, False, "es")
    E = kernels.ElectrostaticProblem(**kwp)
    L = kernels.load_library()
    o = np.zeros(52)
    m = np.ones(8, np.uint8)
    rc = L.xfk_mag_ac_block_integrals(E._h, m.ctypes.data_as(C.POINTER(C.c_ubyte)), o.ctypes.data_as(kernels.dptr))
    assert rc == XFK_ERR_ARG and b"not a magnetics problem" in L.xfk_last_error()
    E.close()
    # sharded
    pr, mesh, kw = synth_to_oracle(synth.harmonic(8, circuits=False))
    (comm,) = kernels.Comm.local_group(1)
    H = kernels.Harmonic2DProblem(**kw, comm=comm)
    _refused(lambda: H.block_integrals_complex(sel), XFK_ERR_UNSUPPORTED, "sharded")
    _refused(H.element_b_complex, XFK_ERR_UNSUPPORTED, "sharded")
    assert H.solve()["cg_iters"] > 0
    H.close()
    comm.close()
    # no solution yet; an unknown type; PrevType != 0
    H = kernels.Harmonic2DProblem(**kw)
    _refused(lambda: H.block_integrals_complex(sel), XFK_ERR_ARG, "no solution yet")
    _refused(H.element_b_complex, XFK_ERR_ARG, "no solution yet")
    _refused(lambda: H.time_postproc_complex(1), XFK_ERR_ARG, "no solution yet")
    assert H.solve()["cg_iters"] > 0
    _refused(lambda: H.block_integral_complex(sel, 26), XFK_ERR_ARG, "out of range")
    _refused(lambda: H.block_integral_complex(sel, -1), XFK_ERR_ARG, "out of range")
    assert np.isfinite(H.block_integrals_complex(sel)["raw"][:25]).all()
    H.close()
    H = kernels.Harmonic2DProblem(**kw, prev_type=1)
    assert H.solve()["cg_iters"] > 0
    _refused(lambda: H.block_integrals_complex(sel), XFK_ERR_UNSUPPORTED, "PrevType")
    _refused(H.element_b_complex, XFK_ERR_UNSUPPORTED, "PrevType")
    assert H.solve()["cg_iters"] > 0
    H.close()


def test_refusal_proximity_winding():
    pr, mesh, kw = synth_to_oracle(synth.harmonic(8, prox=0))
    nl = len(kw["labels"])
    H = kernels.Harmonic2DProblem(**kw)
    H.solve()
    for k in (0, 2, 4, 6, 13):
        _refused(lambda: H.block_integral_complex([3], k), XFK_ERR_UNSUPPORTED, "LamType > 2")
    _refused(lambda: H.block_integrals_complex(np.ones(nl, bool)), XFK_ERR_UNSUPPORTED, "LamType > 2")
    assert H.solve()["cg_iters"] > 0
    A = H.solution()
    others = [k for k in range(nl) if k != 3]
    Rf = R.MagAcPost(kw, A, depth=-1, circuits=H.circuits())
    _check_integrals(H, Rf, others)
    B = H.element_b_complex()                      # answered for the whole problem
    assert np.abs(B - Rf.element_b_all()).max() <= TOL * np.abs(B).max()
    assert H.time_postproc_complex(1)["block_integrals"] > 0
    H.close()


def test_fsolver_kept_problem(tmp_path):
    """a harmonic .fem through fsolver.FSolver: its kept problem answers the
    same calls with the file's [Depth], within the solve bound of the in-memory one"""
    kw = synth.harmonic(12, circuits=False)
    kw["marker"] = None
    kw["points"] = []
    base = str(tmp_path / "h")
    synth.write_problem(base, kw)
    pr, mesh = femfile.load_problem(base)
    fs = fsolver.FSolver()
    fs.keep_problem(True)
    fs.PathName = base
    assert fs.LoadProblemFile() and fs.runSolver(False), fs.last_error()
    V = fs.problem()
    assert V is not None
    kk = kernel_kwargs(pr, mesh)
    nl = len(kk["labels"])
    P = kernels.Harmonic2DProblem(**kk)
    P.solve()
    P.set_depth(pr.Depth)
    a = V.block_integrals_complex(np.ones(nl, bool))["raw"]
    b = P.block_integrals_complex(np.ones(nl, bool))["raw"]
    Rf = R.MagAcPost(kk, P.solution(), depth=pr.Depth, circuits=P.circuits())
    z, s = Rf.block_integrals(np.ones(nl, bool))
    for t in range(25):
        assert abs(a[t] - b[t]) <= SOLVE_TOL * s[t], (t, a[t], b[t])
    Bv, Bp = V.element_b_complex(), P.element_b_complex()
    assert np.abs(Bv - Bp).max() <= SOLVE_TOL * np.abs(Bp).max()
    with pytest.raises(kernels.XfkError, match="harmonic"):
        V.block_integrals(np.ones(nl, bool))
    P.close()
