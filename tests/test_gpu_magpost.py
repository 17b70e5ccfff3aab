"""Magnetostatic post-processing on the device (xfk_magpost.hip, the xfk_mag_
entry points) against the restatement of fpproc (tests/magpostref.py, pinned
by tests/test_magpost_cpu.py).

Bounds: element B to 1e-12 of max |B|; every integral type to 1e-12 of the sum
of the absolute terms (the device sums per workgroup and then over the
workgroups, the restatement element by element).  With nothing selected every
type is 0 and type 25, the centroid, is NaN + NaN j: the reference divides 0
by BlockIntegral(5) = 0.
"""
import os
import re
import shutil

import numpy as np
import pytest

import magpostref as M
from oracle import ansmesh, femfile
from torque import write_case
from util import GOLDEN, ROOT, kernel_kwargs, synth_to_oracle
from xfemm_amd import fsolver, kernels, synth

pytestmark = pytest.mark.gpu

TOL = 1e-12
SOLVE_TOL = 1e-6      # the project's solve tolerance (tests/test_gpu_static2d.py)


def _workgroup():
    """the reduction's workgroup size, from the source"""
    txt = open(os.path.join(ROOT, "xfemm_amd", "csrc", "xfk_potential.h")).read()
    return int(re.search(r"constexpr int kPotQBlock = (\d+);", txt).group(1))


def _magdir(kw):
    labels = kw["labels"]
    if not any(lb.get("mag_dir_fctn") for lb in labels):
        return None
    return kernels.magdir_eval_labels([lb.get("mag_dir_fctn") or "" for lb in labels],
                                      [lb.get("mag_dir", 0.0) for lb in labels], kw["p"], kw["lbl"], kw["x"],
                                      kw["y"], kw.get("length_units", 0), bool(kw.get("problem_type", 0)))


def _ref(kw, P, A, depth):
    return M.MagPost(kw, A, depth=depth, circuits=P.circuits(), magdir=_magdir(kw))


def _check_integrals(P, R, sel):
    z, s = R.block_integrals(sel)
    raw = P.block_integrals(sel)["raw"]
    for t in range(26):
        if t == 25 and not np.isfinite(z[25]):
            assert np.isnan(raw[25].real) and np.isnan(raw[25].imag)
            continue
        assert abs(raw[t] - z[t]) <= TOL * s[t], "type %d: device %r, restated %r, scale %.3e" % (t, raw[t], z[t], s[t])
    return raw


def _check_all(P, kw, A, depth, selections=None):
    R = _ref(kw, P, A, depth)
    B = P.element_b()
    Br = R.element_b_all()
    assert np.abs(B - Br).max() <= TOL * np.abs(Br).max()
    nl = len(kw["labels"])
    for sel in (selections if selections is not None else [np.ones(nl, bool)]):
        _check_integrals(P, R, sel)
    return R


def _answered(kw):
    """the labels whose block the block integrals answer (LamType <= 2, no nonlinear magnet)"""
    def ok(b):
        return b.get("LamType", 0) <= 2 and not (b.get("H_c", 0.0) != 0 and len(b.get("B", ())))
    return np.array([ok(kw["blocks"][lb["block"]]) for lb in kw["labels"]])


def _golden(name):
    pr = femfile.prepare_problem(femfile.parse_fem(os.path.join(GOLDEN, name + ".fem")))
    femfile.get_fill_factor(pr)
    mesh, sol = ansmesh.mesh_from_ans(os.path.join(GOLDEN, name + ".fem"),
                                      os.path.join(GOLDEN, name + ".ans.check"), pr)
    return pr, mesh, sol


@pytest.mark.parametrize("name", ["Temp", "Temp1"])
def test_reference_solution_files_through_set_solution(name):
    """the reference's own .ans.check: no device solve is involved"""
    pr, mesh, sol = _golden(name)
    kw = kernel_kwargs(pr, mesh)
    P = kernels.Static2DProblem(**kw)
    P.set_solution(sol.A)
    P.set_depth(pr.Depth)
    nl = len(kw["labels"])
    ok = _answered(kw)
    assert ok.any()
    if not ok.all():     # (the files' coil is a wound region with proximity effects)
        _refused(P, np.ones(nl, bool), "LamType > 2")
    _check_all(P, kw, sol.A, pr.Depth, [ok, [int(np.nonzero(ok)[0][0])], np.zeros(nl, bool)])
    P.close()


def test_torque_benchmark_mesh(tmp_path):
    """magnets (two of the four labels), an air gap; solved on the device"""
    base = write_case(tmp_path, 30)
    pr, mesh = femfile.load_problem(base)
    kw = kernel_kwargs(pr, mesh)
    P = kernels.Static2DProblem(**kw)
    P.solve()
    P.set_depth(pr.Depth)
    nl = len(kw["labels"])
    magnets = [k for k, lb in enumerate(kw["labels"]) if kw["blocks"][lb["block"]].get("H_c", 0.0) != 0]
    assert magnets and nl >= 4
    _check_all(P, kw, P.solution(), pr.Depth, [np.ones(nl, bool), magnets] + [[k] for k in range(nl)])
    P.close()


def test_axisymmetric_column_with_axis_and_external_region():
    pr, mesh, kw = synth_to_oracle(synth.axisymmetric(16, circuit=True, external=True))
    P = kernels.Static2DProblem(**kw)
    P.solve()
    x = np.asarray(kw["x"])
    assert (x[np.asarray(kw["p"])] == 0).any() and any(lb.get("is_external") for lb in kw["labels"])
    nl = len(kw["labels"])
    _check_all(P, kw, P.solution(), -1, [np.ones(nl, bool), [nl - 1], [2]])
    P.close()


def _shapes():
    c = _workgroup()
    return [1, c - 1, c, c + 1, 2 * c + 3]


@pytest.mark.parametrize("axi", [False, True], ids=["planar", "axisymmetric"])
@pytest.mark.parametrize("which", range(5))
def test_reduction_shapes(which, axi):
    ne = _shapes()[which]
    kw, A = M.strip_problem(ne, axi=axi)
    P = kernels.Static2DProblem(**kw)
    P.set_solution(A)
    P.set_depth(12.5)
    nl = len(kw["labels"])
    _check_all(P, kw, A, 12.5, [np.ones(nl, bool)] + [[k] for k in range(nl)])
    P.close()


@pytest.fixture(scope="module")
def strip():
    kw, A = M.strip_problem(2 * _workgroup() + 3)
    P = kernels.Static2DProblem(**kw)
    P.set_solution(A)
    P.set_depth(12.5)
    yield kw, A, P
    P.close()


def test_selections(strip):
    kw, A, P = strip
    R = _ref(kw, P, A, 12.5)
    nl = len(kw["labels"])
    none = _check_integrals(P, R, np.zeros(nl, bool))
    assert np.all(none[:25] == 0) and np.isnan(none[25].real) and np.isnan(none[25].imag)
    parts = [_check_integrals(P, R, [k]) for k in range(nl)]
    union = _check_integrals(P, R, np.ones(nl, bool))
    _, s = R.block_integrals(np.ones(nl, bool))
    for t in range(25):          # (the centroid is a quotient, not a sum)
        assert abs(sum(q[t] for q in parts) - union[t]) <= TOL * s[t], t
    for t in M.TYPES:
        assert P.block_integral(np.ones(nl, bool), t) == union[t]
    for t in (3, 4, 6, 13, 14, 16):
        assert P.block_integral(np.ones(nl, bool), t) == 0


def test_two_calls_and_a_fresh_problem_give_the_same_bits(strip):
    kw, A, P = strip
    nl = len(kw["labels"])
    sel = np.ones(nl, bool)
    a = P.block_integrals(sel)["raw"]
    b = P.block_integrals(sel)["raw"]
    assert a.tobytes() == b.tobytes()
    Ba = P.element_b()
    Q = kernels.Static2DProblem(**kw)
    Q.set_solution(A)
    Q.set_depth(12.5)
    assert Q.block_integrals(sel)["raw"].tobytes() == a.tobytes()
    assert Q.element_b().tobytes() == Ba.tobytes()
    Q.close()


def test_identity_a_on_the_device():
    """int A.J = 2 int energy on the 20 x 20 square, solved on the device: the
    CPU-measured bound plus the solve tolerance (both relative to the energy)"""
    pr, mesh, kw = synth_to_oracle(M.square_problem(20))
    P = kernels.Static2DProblem(**kw)
    P.solve()
    P.set_depth(3.0)
    r = P.block_integrals(np.ones(len(kw["labels"]), bool))
    d = abs(r["AJ"] - 2 * r["energy"]) / (2 * r["energy"])
    print("identity (a) on the device: %.3e" % d)
    assert d <= M.IDENTITY_A_PLANAR_BOUND + SOLVE_TOL
    P.close()


def test_identity_b_on_the_device():
    pr, mesh, kw = synth_to_oracle(M.winding_problem(20))
    P = kernels.Static2DProblem(**kw)
    P.solve()
    P.set_depth(3.0)
    R = _ref(kw, P, P.solution(), 3.0)
    for k, amps in enumerate(M.WINDING_AMPS):
        sel = [i for i, lb in enumerate(kw["labels"]) if lb.get("in_circuit", -1) == k]
        _, s = R.block_integrals(sel)
        z = P.block_integral(sel, 7)
        assert abs(z - amps) <= TOL * s[7], (k, z, amps)
    P.close()


def _refused(P, sel, word):
    with pytest.raises(kernels.XfkError) as ei:
        P.block_integrals(sel)
    assert word in str(ei.value), str(ei.value)


def test_refusal_harmonic():
    pr, mesh, kw = synth_to_oracle(synth.harmonic(8))
    H = kernels.Harmonic2DProblem(**kw)
    _refused(H, [0], "harmonic")
    with pytest.raises(kernels.XfkError):
        H.element_b()
    assert H.solve()["cg_iters"] > 0
    H.close()


def test_refusal_proximity_winding_label():
    kw, A = M.strip_problem(40)
    kw["blocks"][1] = dict(mu_x=1.0, mu_y=1.0, LamType=3, Cduct=58.0)
    P = kernels.Static2DProblem(**kw)
    P.set_solution(A)
    _refused(P, [1], "LamType > 2")
    _refused(P, np.ones(4, bool), "LamType > 2")
    _check_all(P, kw, A, -1, [[0, 2, 3]])
    P.solve()
    _check_all(P, kw, P.solution(), -1, [[0, 2, 3]])
    P.close()


def test_refusal_nonlinear_permanent_magnet():
    kw = synth.magnetostatic(8, nonlinear=True)
    kw["blocks"][1]["H_c"] = 1000.0            # the steel's curve with a coercivity
    pr, mesh, kw = synth_to_oracle(kw)
    P = kernels.Static2DProblem(**kw)
    P.set_solution(np.zeros(P.n_nodes))
    _refused(P, [1], "nonlinear permanent magnet")
    P.solve()
    _refused(P, [1], "nonlinear permanent magnet")
    _check_all(P, kw, P.solution(), -1, [[0, 2, 3, 4]])
    P.close()


def test_refusal_sharded():
    kw = synth.magnetostatic(8)
    (comm,) = kernels.Comm.local_group(1)
    P = kernels.Static2DProblem(**kw, comm=comm)
    _refused(P, [0], "sharded")
    assert P.solve()["cg_iters"] > 0
    _refused(P, [0], "sharded")
    P.close()
    Q = kernels.Static2DProblem(**kw)
    Q.solve()
    _check_all(Q, kw, Q.solution(), -1)
    Q.close()


def test_file_solved_problem_gives_the_in_memory_bits(tmp_path):
    for ext in (".fem", ".node", ".ele", ".edge", ".pbc"):
        shutil.copy(os.path.join(GOLDEN, "Temp" + ext), tmp_path / ("Temp" + ext))
    base = str(tmp_path / "Temp")
    pr, mesh = femfile.load_problem(base)
    kw = kernel_kwargs(pr, mesh)
    fs = fsolver.FSolver(delete_mesh_files=False)
    fs.keep_problem()
    fs.PathName = base
    assert fs.LoadProblemFile() and fs.runSolver(False), fs.last_error()
    F = fs.problem()
    assert F is not None
    P = kernels.Static2DProblem(**kw)
    P.solve()
    P.set_depth(pr.Depth)
    nl = len(kw["labels"])
    ok = _answered(kw)
    for sel in (ok, [int(np.nonzero(ok)[0][0])]):
        assert F.block_integrals(sel)["raw"].tobytes() == P.block_integrals(sel)["raw"].tobytes()
    assert F.element_b().tobytes() == P.element_b().tobytes()
    # ... and the file's Depth and circuit table are in them
    _, _, A = fs.solution()
    R = M.MagPost(kw, A, depth=pr.Depth, circuits=P.circuits())
    _check_integrals(F, R, ok)
    P.close()
