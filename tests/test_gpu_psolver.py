"""ESolver / HSolver end to end on the device: the reference's solved fixtures
from files (.fee / .feh and mesh files in, .res / .anh out), the file path
against the in-memory path on the same arrays (bit for bit), post-processing
on a file-solved problem, repeated runs, and the command-line programs.

Bounds are those of tests/test_gpu_electro.py and tests/test_gpu_heat.py for
the same fixtures through the in-memory path: V within
precision_bound(recorded, direct, 1e-6) of the recorded potentials, the
conductor potentials equal and the charges within the charge functional's
1e-6 bound; T within 1e-6 of max |T| of the recorded temperatures in 3 passes."""
import os
import subprocess

import numpy as np
import pytest

import electro
import heat
import psolverref as R
import test_gpu_electro as tge
import test_gpu_heat as tgh
from util import precision_bound, rel_err
from xfemm_amd import kernels, psolver

pytestmark = pytest.mark.gpu

BIN = os.path.join(os.path.dirname(kernels.LIB_DIR), "bin")


def _solver(kind, base, **kw):
    s = (psolver.ESolver if kind == "e" else psolver.HSolver)(delete_mesh_files=False, **kw)
    s.PathName = base
    assert s.LoadProblemFile(), s.last_error()
    return s


def _check_text_and_mesh(name, base, f, out):
    """Header bytes, counts, coordinate text, Q and the elements of a written
    fixture solution; returns the matching perm (output node -> fixture node)."""
    kind = R.FIXTURES[name][0]
    assert out["header"] == R.fixture_input(name)
    n, ne = len(f["V"]), len(f["kw"]["lbl"])
    assert len(out["V"]) == n and len(out["lbl"]) == ne and len(out["conductors"]) == len(f["conductors"])
    cf = R.UNITS[kind][f["kw"]["length_units"]]
    xi, yi = f["xy_file"][:, 0] * cf / cf, f["xy_file"][:, 1] * cf / cf     # the reference's arithmetic
    perm = R.match_nodes(out["x"], out["y"], xi, yi)
    assert sorted(perm.tolist()) == list(range(n))
    assert out["xt"] == ["%.17g" % v for v in xi[perm]] and out["yt"] == ["%.17g" % v for v in yi[perm]]
    assert np.array_equal(out["Q"], f["Q"][perm])
    got = {(tuple(perm[t].tolist()), int(l)) for t, l in zip(out["p"], out["lbl"])}
    want = {(tuple(int(v) for v in t), int(l)) for t, l in zip(f["kw"]["p"], f["kw"]["lbl"])}
    assert got == want
    return perm


def test_esolver_fixture_end_to_end(tmp_path):
    base = str(tmp_path / "test")
    f = R.write_fixture_case("test", base)
    assert not (f["kw"].get("lines") or [])          # no boundary properties: no marked edge
    s = _solver("e", base)
    assert s.runSolver(), s.last_error()
    out = R.read_output(base + ".res")
    perm = _check_text_and_mesh("test", base, f, out)
    N = len(f["V"])
    Vc = electro.restate(f["kw"])["V"][:N]
    V = out["V"]
    print("file path V: vs direct %.3e, vs recorded %.3e (bound %.3e)"
          % (rel_err(V, Vc[perm]), rel_err(V, f["V"][perm]), precision_bound(f["V"], Vc, tge.TOL_V)))
    assert rel_err(V, Vc[perm]) <= tge.TOL_V
    assert rel_err(V, f["V"][perm]) <= precision_bound(f["V"], Vc, tge.TOL_V)
    # the conductor lines: the prescribed potentials exactly, as the in-memory path gives them (the
    # recorded ones are the reference's bordered unknowns, solved to its Precision)
    assert (out["conductors"][:, 0] == [50., 0.]).all()
    assert np.abs(out["conductors"][:, 0] - f["conductors"][:, 0]).max() <= tge.TOL_V * np.abs(f["V"]).max()
    for c in range(2):
        g = electro.charge_functional(f["kw"], c)
        bound = np.abs(g).sum() * 1e-6 * np.abs(Vc).max()
        print("conductor %d: q %.10e recorded %.10e (bound %.3e)" % (c, out["conductors"][c, 1], f["conductors"][c, 1],
                                                                     bound))
        assert abs(out["conductors"][c, 1] - f["conductors"][c, 1]) <= bound
    st = s.stats()
    assert st["precond"] == kernels.XFK_PRECOND_AMG and st["newton_iters"] == 1
    x, y, Vg, Q = s.solution()
    assert np.array_equal(Vg, V) and np.array_equal(Q, out["Q"])


@pytest.mark.parametrize("name", ["Temp0", "Temp1"])
def test_hsolver_fixture_end_to_end(tmp_path, name):
    base = str(tmp_path / name)
    f = R.write_fixture_case(name, base)
    s = _solver("h", base)
    if name == "Temp1":
        # [PrevSoln] = "Temp0.anh" with [dT] = 10: the file is never read, the
        # previous temperatures come in the order of the .node file
        assert not s.runSolver() and "Temp0.anh" in s.last_error()
        assert s.set_previous_solution(R.read_fixture("Temp0")["V"])
    assert s.runSolver(), s.last_error()
    out = R.read_output(base + ".anh")
    perm = _check_text_and_mesh(name, base, f, out)
    print("%s file path: vs recorded %.3e, passes %d" % (name, rel_err(out["V"], f["V"][perm]),
                                                       s.stats()["newton_iters"]))
    assert rel_err(out["V"], f["V"][perm]) <= tgh.TOL_V
    assert s.stats()["newton_iters"] == 3
    assert s.stats()["precond"] == kernels.XFK_PRECOND_AMG


# ---- the file path is the memory path ------------------------------------------------

def _planar_electro():
    """Periodic left / right sides, a point charge inside, fixed V below and above."""
    nx, ny = 9, 7
    x, y, p = electro.grid(nx, ny, 8.0, 6.0)
    e = electro.tag_edges(x, y, p, [(lambda xa, ya, xb, yb: ya == 0 and yb == 0, 0),
                                    (lambda xa, ya, xb, yb: ya == 6 and yb == 6, 1)])
    marker = -np.ones(nx * ny, np.int32)
    marker[3 * nx + 4] = 0
    return "e", dict(x=x, y=y, p=p, e=e, lbl=np.zeros(len(p), np.int32), marker=marker,
                     pbc=[[j * nx, j * nx + nx - 1, 0] for j in range(1, ny - 1)],
                     blocks=[dict(ex=2.0, ey=3.0, qv=1e-6)], labels=[dict(block=0)],
                     lines=[dict(format=0, V=0.0), dict(format=0, V=10.0)], points=[dict(qp=1e-12)],
                     length_units=1, depth=2.5, precision=1e-10)


def _axi_electro():
    """An electrode on the inner radius, a floating conductor inside, V = 0 outside."""
    nx, ny = 9, 9
    x, y, p = electro.grid(nx, ny, 4.0, 4.0, x0=1.0)
    e = electro.tag_edges(x, y, p, [(lambda xa, ya, xb, yb: xa == 5 and xb == 5, 0)])
    cond = -np.ones(nx * ny, np.int32)
    cond[x == 1] = 0
    cond[4 * nx + 3:4 * nx + 6] = 1
    return "e", dict(x=x, y=y, p=p, e=e, lbl=np.zeros(len(p), np.int32), conductor=cond,
                     blocks=[dict(ex=1.0, ey=1.0)], labels=[dict(block=0)], lines=[dict(format=0, V=0.0)],
                     conductors=[dict(type=1, V=5.0), dict(type=0, q=1e-11)], length_units=1, problem_type=1,
                     precision=1e-10)


def _nonlinear_heat():
    """A K(T) table, a fixed temperature on the left, convection on the right."""
    nx, ny = 9, 6
    x, y, p = electro.grid(nx, ny, 0.08, 0.05)
    e = heat.tag_edges(x, y, p, [(lambda xa, ya, xb, yb: xa == 0 and xb == 0, 0),
                                 (lambda xa, ya, xb, yb: xa == 0.08 and xb == 0.08, 1)])
    return "h", dict(x=x, y=y, p=p, e=e, lbl=np.zeros(len(p), np.int32),
                     blocks=[dict(kx=1.0, ky=1.0, kt=0.0, qv=2e4, T=np.array([300., 400., 600.]),
                                  K=np.array([1.0, 1.6, 2.9]))],
                     labels=[dict(block=0)], lines=[dict(format=0, Tset=500.0), dict(format=2, h=20.0, Tinf=300.0)],
                     length_units=3, depth=1.0, precision=1e-8)


@pytest.mark.parametrize("make", [_planar_electro, _axi_electro, _nonlinear_heat],
                         ids=["planar-periodic-point", "axi-floating", "heat-nonlinear"])
def test_file_path_equals_memory_path(tmp_path, make):
    kind, kw = make()
    base = str(tmp_path / "c")
    R.write_case(kind, base, kw)
    s = _solver(kind, base)
    assert s.runSolver(), s.last_error()
    x, y, V, Q = s.solution()
    twin_kw = s.kw()
    # the file path decoded what the test wrote (up to the renumbering)
    assert len(twin_kw["pbc"]) == len(kw.get("pbc", ()))
    assert (twin_kw["marker"] >= 0).sum() == (np.asarray(kw.get("marker", [-1])) >= 0).sum()
    assert (twin_kw["conductor"] >= 0).sum() == (np.asarray(kw.get("conductor", [-1])) >= 0).sum()
    assert (twin_kw["e"] >= 0).sum() == (np.asarray(kw["e"]) >= 0).sum()
    cls = kernels.ElectrostaticProblem if kind == "e" else kernels.HeatFlowProblem
    M = cls(**twin_kw)
    r = M.solve()
    Vm = M.solution()
    assert np.array_equal(V, Vm), np.abs(V - Vm).max()
    Vc, qc = s.conductors()
    Vcm, qcm = M.conductors()
    assert np.array_equal(Vc, Vcm) and np.array_equal(qc, qcm)
    assert s.stats()["newton_iters"] == r["newton_iters"] and s.stats()["cg_iters"] == r["cg_iters"]
    if kind == "h":
        assert r["newton_iters"] >= 2
    if "conductors" in kw:
        # the floating conductor: a merged row, its line's V the representative node's value
        ring = twin_kw["conductor"] == 1
        assert len(set(V[ring].tolist())) == 1 and Vc[1] == V[ring][0] and qc[1] == kw["conductors"][1]["q"]
        assert (Q[ring] == 1).all()
    # post-processing through problem() is the in-memory twin's
    P = s.problem()
    a, b = P.block_integrals([0]), M.block_integrals([0])
    assert set(a) == set(b) and all(np.array_equal(a[k], b[k]) for k in a)
    u = R.UNITS[kind][kw["length_units"]]
    xs, ys = np.asarray(kw["x"]) / u, np.asarray(kw["y"]) / u
    contour = [(xs.min() * 0.75 + xs.max() * 0.25, ys.min() * 0.8 + ys.max() * 0.2),
               (xs.min() * 0.2 + xs.max() * 0.8, ys.min() * 0.3 + ys.max() * 0.7)]
    assert P.line_integral(contour, 0) == M.line_integral(contour, 0)
    pv, pm = P.point_values(xs[5:9] * 0.999 + 1e-3 * xs.mean(), ys[5:9] * 0.999 + 1e-3 * ys.mean()), \
        M.point_values(xs[5:9] * 0.999 + 1e-3 * xs.mean(), ys[5:9] * 0.999 + 1e-3 * ys.mean())
    assert all(np.array_equal(pv[k], pm[k]) for k in pv)
    M.close()
    P.close()
    assert s.problem().n_nodes == len(V)      # the view's close leaves the solver's problem alive


def test_second_run_and_second_object_write_the_same_bytes(tmp_path):
    kind, kw = _planar_electro()
    base = str(tmp_path / "c")
    R.write_case(kind, base, kw)
    s = _solver(kind, base)
    assert s.runSolver(), s.last_error()
    first = open(base + ".res", "rb").read()
    os.remove(base + ".res")
    assert s.runSolver(), s.last_error()
    assert open(base + ".res", "rb").read() == first
    os.remove(base + ".res")
    s2 = _solver(kind, base)
    assert s2.runSolver(), s2.last_error()
    assert open(base + ".res", "rb").read() == first
    t = s2.times()
    assert all(t[k] > 0 for k in ("ms_load_mesh", "ms_cuthill", "ms_create", "ms_solve", "ms_write"))


@pytest.mark.parametrize("name,prog", [("test", "esolver"), ("Temp0", "hsolver")])
def test_command_line_program(tmp_path, name, prog):
    kind = R.FIXTURES[name][0]
    os.mkdir(tmp_path / "lib")
    os.mkdir(tmp_path / "cli")
    lib_base, cli_base = str(tmp_path / "lib" / name), str(tmp_path / "cli" / name)
    R.write_fixture_case(name, lib_base)
    R.write_fixture_case(name, cli_base)
    s = _solver(kind, lib_base)
    assert s.runSolver(), s.last_error()
    r = subprocess.run([os.path.join(BIN, prog), cli_base], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    for msg in ("renumbering nodes\n", "solving...Problem Statistics:\n", "Problem solved\n",
                "results written to disk\n"):
        assert msg in r.stderr
    ext = R.EXT[kind][1]
    assert open(cli_base + ext, "rb").read() == open(lib_base + ext, "rb").read()
    for e in (".node", ".ele", ".pbc", ".edge"):      # the program deletes the mesh files, as the reference's does
        assert not os.path.exists(cli_base + e)
    # the reference's exits: 1 without a problem file, 2 when the solver fails (no mesh files left)
    r = subprocess.run([os.path.join(BIN, prog), str(tmp_path / "absent")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "problem loading %s file" % R.EXT[kind][0] in r.stderr
    r = subprocess.run([os.path.join(BIN, prog), cli_base], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "problem loading mesh:\n" in r.stderr
    r = subprocess.run([os.path.join(BIN, prog)], input=str(tmp_path / "absent") + "\n", capture_output=True,
                       text=True, timeout=60)
    assert r.returncode == 1 and "Enter %s file name without extension:\n" % R.EXT[kind][0][1:] in r.stdout
