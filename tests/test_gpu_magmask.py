"""The weighted stress tensor mask and block integrals 18-23 of a magnetostatic
problem on the device (xfk_magpost.hip: xfk_mag_make_mask, k_mag_stress)
against the restatement of fpproc (tests/magmaskref.py, held to closed forms
by tests/test_magmask_cpu.py).

Bounds: the fixed values and the 0 / 1 mask node by node; the assembled mask
system 1e-12 of its largest entry; W 1e-6 (the project's solve tolerance, W
lies in [0, 1]); each of types 18-23 to 1e-12 of the sum of its absolute terms
on the restatement's mask.  The mask comparison means something only away
from the threshold: every case asserts |W - 0.5| > 1e-4 on the restatement's
free nodes first.
"""
import math
import os
import re

import numpy as np
import pytest

import magmaskref as MM
import magpostref as M
from oracle import femfile
from util import ROOT, kernel_kwargs, synth_to_oracle
from xfemm_amd import fsolver, kernels, synth

pytestmark = pytest.mark.gpu

TOL = 1e-12
TOL_W = 1e-6
SOLVE_TOL = 1e-6
NO_CIRC = ((1,), (0.,), (0.,))


def _workgroup():
    txt = open(os.path.join(ROOT, "xfemm_amd", "csrc", "xfk_potential.h")).read()
    return int(re.search(r"constexpr int kPotQBlock = (\d+);", txt).group(1))


def case(name):
    """kw, A, the restated mask and its arguments, built once"""
    if name in case.cache:
        return case.cache[name]
    c = dict(max_area=None, block_not_air=None, depth=-1, circuits=None)
    if name in ("strip_mm", "strip_inch"):
        c["kw"], c["A"], info = MM.layered_strip(length_units=1 if name == "strip_mm" else 0)
        c.update(sel=info["sel"], depth=info["depth"], info=info)
        if name == "strip_inch":
            c["max_area"] = np.array([0.5, 2.0])
    elif name in ("rules", "rules_axi"):
        c["kw"], c["A"], ex = MM.rules_problem(axi=name == "rules_axi")
        c.update(sel=ex["sel"], max_area=ex["max_area"], block_not_air=ex["block_not_air"], depth=12.0,
                 circuits=NO_CIRC, invalid_sel=ex["invalid_sel"])
    elif name == "free_body":      # a body floating in a full domain: most nodes free, no boundary touched
        c["kw"], c["A"] = MM.free_body(8)
        c.update(sel=[1], depth=10.0)
    else:
        raise KeyError(name)
    c["R"] = M.MagPost(c["kw"], c["A"], depth=c["depth"], circuits=c["circuits"])
    c["K"] = MM.MagMask(c["R"], c["sel"], c["max_area"], c["block_not_air"])
    case.cache[name] = c
    return c


case.cache = {}


def device(c, solved=False):
    P = kernels.Static2DProblem(**c["kw"])
    if solved:
        P.solve()
    else:
        P.set_solution(c["A"])
    P.set_depth(c["depth"])
    return P


def mask_args(c):
    return dict(selected_labels=c["sel"], max_area=c["max_area"], block_not_air=c["block_not_air"])


def dense(csr, n):
    rp, col, val, b = csr
    A = np.zeros((n, n))
    for i in range(n):
        A[i, col[rp[i]:rp[i + 1]]] = val[rp[i]:rp[i + 1]]
    return A, b


def check_against_restatement(P, c, K=None):
    K = c["K"] if K is None else K
    LV = np.array(K.LV)
    free = LV < 0
    if free.any():
        assert np.abs(K.W - 0.5)[free].min() > 1e-4
    m = P.make_mask(**mask_args(c))
    n = len(LV)
    A, b = dense(P.mask_csr(), n)
    # the fixed values: a fixed node's row is its diagonal alone and b = value x diagonal, bit for bit
    fx = np.flatnonzero(~free)
    off = A - np.diag(np.diag(A))
    assert np.all(off[fx] == 0) and np.all(off[:, fx] == 0)
    assert np.array_equal(b[fx] / np.diag(A)[fx], LV[fx])
    assert np.abs(A - K.A).max() <= TOL * np.abs(K.A).max()
    assert np.abs(b - K.b).max() <= TOL * np.abs(K.b).max()
    print("W: %.3e of 1; cg %d" % (np.abs(m["W"] - K.W).max(), m["cg_iters"]))
    assert np.abs(m["W"] - K.W).max() <= TOL_W
    assert np.array_equal(m["msk"], K.msk)
    z, sc = K.integrals()
    raw = P.block_integrals(c["sel"])["raw"]
    for k, t in enumerate(MM.TYPES):
        print("type %d: device %.17g restated %.17g scale %.3e" % (t, raw[t].real, z[k], sc[k]))
        assert raw[t].imag == 0
        assert abs(raw[t].real - z[k]) <= TOL * sc[k], t
        assert abs(P.block_integral(c["sel"], t).real - raw[t].real) == 0
    w = P.weighted_stress(**mask_args(c))
    assert np.array_equal(w["force"], [raw[18].real, raw[19].real]) and w["torque"] == raw[22].real
    assert np.array_equal(w["force_2x"], [raw[20].real, raw[21].real]) and w["torque_2x"] == raw[23].real
    return m, raw


@pytest.mark.parametrize("name", ["strip_mm", "strip_inch", "rules", "rules_axi", "free_body"])
def test_against_restatement(name):
    c = case(name)
    P = device(c)
    m, raw = check_against_restatement(P, c)
    if name.startswith("strip"):
        F = MM.strip_closed_form(c["R"], c["info"])[0]
        sc = c["K"].integrals()[1]
        assert abs(raw[18].real - F) <= 2 * TOL * sc[0] and abs(raw[18].real - raw[11].real) <= 2 * TOL * sc[0]
    if name == "rules_axi":
        assert raw[18] == 0 and raw[20] == 0 and raw[22] == 0 and raw[23] == 0 and raw[19] != 0
    P.close()


@pytest.mark.parametrize("axi", [False, True], ids=["planar", "axi"])
@pytest.mark.parametrize("which", ["1", "c-1", "c", "c+1", "2c+3"])
def test_reduction_shapes(which, axi):
    """Element counts round the workgroup size of the two-stage sum, a hand-set
    solution and a mask known by hand: every node of a strip of triangles ends
    an exterior edge, so the mask is 1 on the selected elements' nodes and 0
    elsewhere."""
    c0 = _workgroup()
    ne = {"1": 1, "c-1": c0 - 1, "c": c0, "c+1": c0 + 1, "2c+3": 2 * c0 + 3}[which]
    kw, A, sel, msk = MM.strip_case(ne, axi)
    R = M.MagPost(kw, A, depth=7.0)
    K = MM.MagMask(R, sel)
    assert np.all(np.array(K.LV) >= 0) and np.array_equal(K.msk, msk)
    c = dict(kw=kw, A=A, sel=sel, max_area=None, block_not_air=None, depth=7.0, K=K, R=R)
    P = device(c)
    m, raw = check_against_restatement(P, c)
    assert np.array_equal(m["msk"], msk)
    if ne == 1:      # one element: a constant mask, no gradient
        assert all(raw[t] == 0 for t in MM.TYPES)
    else:
        assert any(raw[t] != 0 for t in MM.TYPES)
    P.close()


def test_two_calls_give_identical_bits():
    c = case("rules")
    P = device(c)
    a = P.weighted_stress(**mask_args(c))
    r1 = P.block_integrals(c["sel"])["raw"].tobytes()
    r2 = P.block_integrals(c["sel"])["raw"].tobytes()
    assert r1 == r2
    m1 = P.make_mask(**mask_args(c))
    b = P.weighted_stress(**mask_args(c))
    assert np.array_equal(m1["msk"], P.make_mask(**mask_args(c))["msk"])
    for k in a:
        assert np.array_equal(a[k], b[k])
    P.close()


def test_without_a_mask_and_mask_lifetime():
    c = case("rules")
    sel = c["sel"]
    P = device(c)
    assert not P.mask_info()["ready"]
    raw = P.block_integrals(sel)["raw"]
    assert np.all(raw[18:24] == 0) and raw[11] != 0
    for t in MM.TYPES:
        with pytest.raises(kernels.XfkError, match="make_mask"):
            P.block_integral(sel, t)
    with pytest.raises(kernels.XfkError, match="no mask"):
        P.time_stress(1)
    P.make_mask(**mask_args(c))
    assert P.mask_info()["ready"] and P.block_integral(sel, 19).real != 0
    assert P.time_stress(2) > 0
    # a mask for another selection is refused, and block_integrals leaves 18-23 at 0
    other = [3]
    with pytest.raises(kernels.XfkError, match="make_mask"):
        P.block_integral(other, 19)
    assert np.all(P.block_integrals(other)["raw"][18:24] == 0)
    assert P.block_integral(sel, 19).real != 0
    # set_solution and a solve drop the mask
    P.set_solution(c["A"])
    assert not P.mask_info()["ready"]
    with pytest.raises(kernels.XfkError, match="make_mask"):
        P.block_integral(sel, 19)
    P.make_mask(**mask_args(c))
    assert P.mask_info()["ready"]
    P.solve()
    assert not P.mask_info()["ready"]
    assert np.all(P.block_integrals(sel)["raw"][18:24] == 0)
    w = P.weighted_stress(**mask_args(c))      # makes the mask again
    assert P.mask_info()["ready"] and w["force"][1] == P.block_integral(sel, 19).real
    P.close()


def test_invalid_selection_leaves_the_problem_usable():
    c = case("rules")
    P = device(c)
    with pytest.raises(kernels.XfkError) as ei:
        P.make_mask(c["invalid_sel"], c["max_area"], c["block_not_air"])
    assert MM.INVALID in str(ei.value)
    assert not P.mask_info()["ready"]
    assert P.solve()["cg_iters"] > 0
    P.set_solution(c["A"])
    check_against_restatement(P, c)
    P.close()


@pytest.mark.parametrize("block", [dict(mu_x=1.0, mu_y=1.0, LamType=3, Cduct=58.0), "nonlinear_magnet"],
                         ids=["LamType3", "nonlinear_magnet"])
def test_selection_whose_energy_is_not_built(block):
    """Types 18-23 read B and the mask alone: a selected label the energy
    integrals refuse (LamType > 2, a magnet with a B-H curve) still gets its
    force and torque, while block_integrals stays refused."""
    kw, A, sel, msk = MM.strip_case(40)
    if block == "nonlinear_magnet":
        Bc, Hc, Sc, mu = fsolver.bh_get_slopes(*synth.m19_curve())
        block = dict(mu_x=mu, mu_y=mu, H_c=1000.0, B=Bc, H=Hc, slope=Sc)
    kw["blocks"][sel[0]] = block
    R = M.MagPost(kw, A, depth=7.0)
    K = MM.MagMask(R, sel)
    z, sc = K.integrals()
    P = kernels.Static2DProblem(**kw)
    P.set_solution(A)
    P.set_depth(7.0)
    with pytest.raises(kernels.XfkError, match="energy"):
        P.block_integrals(sel)
    w = P.weighted_stress(sel)
    got = [w["force"][0], w["force"][1], w["force_2x"][0], w["force_2x"][1], w["torque"], w["torque_2x"]]
    assert np.array_equal(P.make_mask(sel)["msk"], msk)
    assert np.all(np.abs(np.array(got) - z) <= TOL * sc) and np.any(z != 0)
    assert P.time_stress(1) > 0
    with pytest.raises(kernels.XfkError, match="energy"):
        P.block_integral(sel, 2)
    P.close()


def test_harmonic_and_sharded_are_refused():
    pr, mesh, kw = synth_to_oracle(synth.harmonic(8))
    H = kernels.Harmonic2DProblem(**kw)
    for f in (lambda: H.make_mask([0]), lambda: H.mask_info(), lambda: H.weighted_stress([0]), lambda: H.mask_csr(),
              lambda: H.time_stress(1)):
        with pytest.raises(kernels.XfkError, match="harmonic"):
            f()
    H.close()
    kw = synth.magnetostatic(8)
    (comm,) = kernels.Comm.local_group(1)
    P = kernels.Static2DProblem(**kw, comm=comm)
    for f in (lambda: P.make_mask([0]), lambda: P.weighted_stress([0]), lambda: P.time_stress(1)):
        with pytest.raises(kernels.XfkError, match="sharded"):
            f()
    P.close()


@pytest.mark.parametrize("name", ["strip_mm", "strip_inch"])
def test_strip_solved_on_the_device(name):
    """The layered strip solved on the device, not loaded: F_x within the bound
    the project holds a solved potential to (1e-6), relative to the closed
    form's scale depth h (B_L^2 + B_R^2) / (2 mu0); the mask is the restated one."""
    c = case(name)
    P = device(c, solved=True)
    A = P.solution()
    print("solved A vs direct: %.3e of max |A|" % (np.abs(A - c["A"]).max() / np.abs(c["A"]).max()))
    assert np.abs(A - c["A"]).max() <= SOLVE_TOL * np.abs(c["A"]).max()
    w = P.weighted_stress(**mask_args(c))
    R, info = c["R"], c["info"]
    F, BL, BR = MM.strip_closed_form(R, info)
    scale = R.depth * (info["h"] * R.lc) * (BL * BL + BR * BR) / (2. * M.MUO)
    print("F_x %.12e closed %.12e: %.3e of the scale; F_y %.3e torque %.3e" %
          (w["force"][0], F, abs(w["force"][0] - F) / scale, w["force"][1], w["torque"]))
    assert abs(w["force"][0] - F) <= SOLVE_TOL * scale
    assert abs(w["force"][1]) <= SOLVE_TOL * scale
    assert abs(w["torque"]) <= SOLVE_TOL * scale * (abs(R.X).max() * R.lc)
    assert np.array_equal(P.make_mask(**mask_args(c))["msk"], c["K"].msk)
    P.close()


def test_file_solved_problem_takes_its_mask_inputs_from_the_fem(tmp_path):
    """FSolver on a .fem with a mesh size on its labels and a hysteresis angle
    on an otherwise-air block: its kept problem's weighted_stress() equals the
    in-memory problem's given the same MaxArea and block_not_air."""
    kw, _, info = MM.layered_strip(length_units=2)
    # the hysteretic "air": the outermost column of the left air layer, away from the slab
    kw["blocks"].append(dict(mu_x=1.0, mu_y=1.0, Theta_hn=12.0))
    kw["labels"].append(dict(block=2))
    X = M.user_xy(kw)[0]
    cx = X[kw["p"]].mean(axis=1)
    kw["lbl"][cx < np.sort(np.unique(X))[2]] = 2      # (grid line, centre line, grid line)
    size = [0.9, -1, 0.4]
    for lb, d in zip(kw["labels"], size):
        lb["mesh_size"] = d
    base = str(tmp_path / "ws")
    synth.write_problem(base, kw)
    pr, mesh = femfile.load_problem(base)
    kwf = kernel_kwargs(pr, mesh)
    fs = fsolver.FSolver(delete_mesh_files=False)
    fs.keep_problem()
    fs.PathName = base
    assert fs.LoadProblemFile() and fs.runSolver(False), fs.last_error()
    F = fs.problem()
    assert F is not None
    area, notair = fs.mask_inputs()
    want = np.array([0. if d <= 0 else math.pi * d * d / 4. for d in size])
    assert np.allclose(area, want, rtol=1e-15, atol=0) and list(notair) == [0, 0, 1]
    sel = info["sel"]
    wf = F.weighted_stress(sel)
    P = kernels.Static2DProblem(**kwf)
    P.solve()
    P.set_depth(pr.Depth)
    wp = P.weighted_stress(sel, max_area=area, block_not_air=notair)
    # an argument given replaces its default alone: the other is still the .fem's
    for one in (dict(max_area=area), dict(block_not_air=notair)):
        wo = F.weighted_stress(sel, **one)
        assert all(np.array_equal(wo[k], wf[k]) for k in wf)
    half = F.make_mask(sel, max_area=np.zeros(len(area)))
    assert np.array_equal(half["W"], P.make_mask(sel, max_area=np.zeros(len(area)), block_not_air=notair)["W"])
    print("file %r in-memory %r" % (wf, wp))
    for k in wf:
        assert np.array_equal(wf[k], wp[k]), k
    assert wf["force"][0] != 0
    # ... and they matter: without them the hysteretic patch is air and its nodes are free
    m0 = P.make_mask(sel)
    m1 = P.make_mask(sel, max_area=area, block_not_air=notair)
    patch = np.unique(np.asarray(kwf["p"])[np.asarray(kwf["lbl"]) == 2])
    assert np.abs(m1["W"][patch]).max() <= 1e-12 and np.abs(m0["W"][patch]).max() > 1e-3
    P.close()
