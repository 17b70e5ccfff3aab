"""Electrostatic problems on the device (xfk_electrostatic) against the
reference's solved fixture, exact solutions, and the literal restatement of
ESolver::AnalyzeProblem solved directly (tests/electro.py).

Bounds: the assembled system within 1e-12 of the restatement's (matrix by
max-entry norm, right-hand side after the boundary conditions); V within 1e-6
of max |V| of the direct solve; the charge kernel within 1e-10 of the restated
ChargeOnConductor on the V the device returned; a charge against the direct
solve's within |g|_1 1e-6 max |V| (q = g . V is linear in V)."""
import ctypes as C
import os

import numpy as np
import pytest
import scipy.sparse as sp

import electro
from util import GOLDEN, precision_bound, rel_err
from xfemm_amd import kernels, synth

pytestmark = pytest.mark.gpu

TOL_SYSTEM = 1e-12
TOL_V = 1e-6
EO = electro.EO


def _system_err(P, sol):
    rp, col, val, b = P.csr()
    n = len(rp) - 1
    G = sp.csr_matrix((val, col, rp), shape=(n, n)).toarray()
    Go, bo = sol["A"][:n, :n], sol["b"][:n]
    return np.abs(G - Go).max() / np.abs(Go).max(), np.abs(b - bo).max() / max(np.abs(bo).max(), 1e-300)


def _solve(kw, **opt):
    P = kernels.ElectrostaticProblem(**kw, **opt)
    r = P.solve()
    return P, r, P.solution()


@pytest.fixture(scope="module")
def fixture():
    res = electro.read_res(os.path.join(GOLDEN, "esolver", "test.res.check"))
    res["sol"] = electro.restate(res["kw"])
    P, r, V = _solve(res["kw"])
    res.update(r=r, Vd=V, sys=_system_err(P, res["sol"]), cond=P.conductors(),
               qc=[P.conductor_charge(c) for c in range(2)])
    P.close()
    return res


def test_fixture_system(fixture):
    es, eb = fixture["sys"]
    print("fixture system: matrix %.3e rhs %.3e" % (es, eb))
    assert es <= TOL_SYSTEM and eb <= TOL_SYSTEM


def test_fixture_potential(fixture):
    N = len(fixture["V"])
    Vc, Vo, V = fixture["sol"]["V"][:N], fixture["V"], fixture["Vd"]
    print("fixture V: vs direct %.3e, vs recorded %.3e (bound %.3e)"
          % (rel_err(V, Vc), rel_err(V, Vo), precision_bound(Vo, Vc, TOL_V)))
    assert rel_err(V, Vc) <= TOL_V
    assert rel_err(V, Vo) <= precision_bound(Vo, Vc, TOL_V)
    assert fixture["r"]["precond"] == kernels.XFK_PRECOND_AMG
    assert fixture["r"]["newton_iters"] == 1


def test_fixture_charges(fixture):
    kw, N = fixture["kw"], len(fixture["V"])
    Vcond, q = fixture["cond"]
    assert (Vcond == [50.0, 0.0]).all()
    for c in range(2):
        q_kernel = electro.charge(kw, fixture["Vd"], c)
        q_direct = electro.charge(kw, fixture["sol"]["V"][:N], c)
        g = electro.charge_functional(kw, c)
        bound = np.abs(g).sum() * 1e-6 * np.abs(fixture["sol"]["V"][:N]).max()
        print("conductor %d: q %.10e, vs restated on device V %.3e rel, vs direct %.3e (bound %.3e), recorded %.10e"
              % (c, q[c], abs(q[c] - q_kernel) / abs(q_kernel), abs(q[c] - q_direct), bound,
                 fixture["conductors"][c, 1]))
        assert abs(q[c] - q_kernel) <= 1e-10 * abs(q_kernel)
        assert abs(q[c] - q_direct) <= bound
        assert fixture["qc"][c] == q[c]   # the entry point serves any conductor: the same kernel, the same bits


@pytest.mark.parametrize("units", [1, 0], ids=["mm", "inches"])
def test_planar_plates_exact(units):
    """A BdryFormat 0 edge at 0 V on the left, a prescribed-voltage conductor
    on the right, ex != ey: V = V0 x / w at the nodes and
    q = eo ex V0 h Depth / w, both exact for linear elements."""
    u = electro.UNITS[units]
    w, h, depth, V0 = 4.0, 2.5, 0.7, 12.0          # user units
    x, y, p = electro.grid(9, 6, w * u, h * u)
    e = electro.tag_edges(x, y, p, [(lambda xa, ya, xb, yb: xa == 0 and xb == 0, 0)])
    cond = np.where(x == x.max(), 0, -1).astype(np.int32)
    kw = dict(x=x, y=y, p=p, e=e, lbl=np.zeros(len(p), np.int32), blocks=[dict(ex=3.0, ey=7.0)],
              labels=[dict(block=0)], lines=[dict(format=0, V=0.0)], conductors=[dict(type=1, V=V0)],
              conductor=cond, depth=depth, length_units=units, precision=1e-12)
    P, r, V = _solve(kw)
    _, q = P.conductors()
    P.close()
    m = 0.001 * u                                   # user unit in metres
    q_exact = EO * 3.0 * V0 * (h * m) * (depth * m) / (w * m)
    print("plates: V %.3e of V0, q %.3e rel" % (np.abs(V - V0 * x / x.max()).max() / V0, abs(q[0] / q_exact - 1)))
    assert np.abs(V - V0 * x / x.max()).max() <= 1e-9 * V0
    assert abs(q[0] - q_exact) <= 1e-9 * q_exact


def test_axisymmetric_plates_exact():
    """A disc 0 <= r <= R with its axis nodes, V linear in z:
    q = eo ey V0 pi R^2 / h (centroid radii integrate r exactly)."""
    R, h, V0 = 30.0, 8.0, 5.0                       # mm
    x, y, p = electro.grid(8, 5, R, h)
    e = electro.tag_edges(x, y, p, [(lambda xa, ya, xb, yb: ya == 0 and yb == 0, 0)])
    cond = np.where(y == y.max(), 0, -1).astype(np.int32)
    kw = dict(x=x, y=y, p=p, e=e, lbl=np.zeros(len(p), np.int32), blocks=[dict(ex=2.0, ey=5.0)],
              labels=[dict(block=0)], lines=[dict(format=0, V=0.0)], conductors=[dict(type=1, V=V0)],
              conductor=cond, length_units=1, problem_type=1, precision=1e-12)
    P, r, V = _solve(kw)
    _, q = P.conductors()
    P.close()
    q_exact = EO * 5.0 * V0 * np.pi * (R * 1e-3) ** 2 / (h * 1e-3)
    assert np.abs(V - V0 * y / h).max() <= 1e-9 * V0
    assert abs(q[0] - q_exact) <= 1e-9 * q_exact


def _planar_everything(nx, ny):
    x, y, p = electro.grid(nx, ny, 30.0, 20.0)
    cx = x[p].mean(axis=1)
    lbl = (cx > 15.0).astype(np.int32)
    e = electro.tag_edges(x, y, p, [
        (lambda xa, ya, xb, yb: xa == 0 and xb == 0, 0),          # fixed V
        (lambda xa, ya, xb, yb: ya == 20.0 and yb == 20.0, 1),    # mixed
        (lambda xa, ya, xb, yb: ya == 0 and yb == 0, 2)])         # surface charge
    marker = -np.ones(len(x), np.int32)
    marker[(ny // 2) * nx + nx // 3] = 0                          # point charge
    marker[(ny // 3) * nx + 2 * nx // 3] = 1                      # fixed-potential point
    cond = np.where(x == x.max(), 0, -1).astype(np.int32)
    return dict(x=x, y=y, p=p, e=e, lbl=lbl, marker=marker, conductor=cond,
                blocks=[dict(ex=2.0, ey=3.0), dict(ex=5.0, ey=1.5, qv=4e-6)],
                labels=[dict(block=0), dict(block=1)],
                lines=[dict(format=0, V=3.0), dict(format=1, c0=4e-8, c1=2e-8), dict(format=2, qs=3e-8)],
                points=[dict(qp=5e-11), dict(V=-1.5)], conductors=[dict(type=1, V=7.0)],
                depth=0.5, length_units=2)


def _axi_external(nx, ny):
    x, y, p = electro.grid(nx, ny, 40.0, 50.0, x0=5.0, y0=-25.0)
    cx, cy = x[p].mean(axis=1), y[p].mean(axis=1)
    lbl = (cx * cx + cy * cy > 30.0 ** 2).astype(np.int32)
    e = electro.tag_edges(x, y, p, [(lambda xa, ya, xb, yb: xa == 5.0 and xb == 5.0, 0),
                                    (lambda xa, ya, xb, yb: xa == 45.0 and xb == 45.0, 1)])
    return dict(x=x, y=y, p=p, e=e, lbl=lbl, blocks=[dict(ex=1.0, ey=1.0, qv=1e-6)],
                labels=[dict(block=0), dict(block=0, is_external=1)],
                lines=[dict(format=0, V=10.0), dict(format=0, V=0.0)], length_units=1, problem_type=1,
                ext_ro=30.0, ext_ri=20.0, ext_zo=1.0)


def _periodic(nx, ny, anti):
    x, y, p = electro.grid(nx, ny, 24.0, 16.0)
    e = electro.tag_edges(x, y, p, [(lambda xa, ya, xb, yb: xa == 0 and xb == 0, 0),
                                    (lambda xa, ya, xb, yb: xa == 24.0 and xb == 24.0, 1)])
    lbl = (x[p].mean(axis=1) > 10.0).astype(np.int32)
    # bottom and top rows, without the fixed corners
    pbc = [[i, (ny - 1) * nx + i, 1 if anti else 0] for i in range(1, nx - 1)]
    return dict(x=x, y=y, p=p, e=e, lbl=lbl, pbc=pbc, blocks=[dict(ex=1.0, ey=2.0), dict(ex=3.0, ey=1.0, qv=2e-6)],
                labels=[dict(block=0), dict(block=1)],
                lines=[dict(format=0, V=0.0 if anti else 4.0), dict(format=0, V=0.0)], depth=2.0, length_units=1)


CASES = {"planar": _planar_everything, "axi_external": _axi_external,
         "periodic": lambda nx, ny: _periodic(nx, ny, False), "antiperiodic": lambda nx, ny: _periodic(nx, ny, True)}


@pytest.mark.parametrize("size", [(7, 7), (13, 11)], ids=["7x7", "13x11"])
@pytest.mark.parametrize("case", list(CASES))
def test_matches_direct_solve(case, size):
    """7 x 7 nodes: one partial row-gather workgroup; 13 x 11 = 143 rows: two
    workgroups, the second partial."""
    kw = CASES[case](*size)
    sol = electro.restate(kw)
    N = len(kw["x"])
    P, r, V = _solve(kw)
    es, eb = _system_err(P, sol)
    Vc, q = P.conductors()
    P.close()
    print("%s %s: matrix %.3e rhs %.3e V %.3e" % (case, size, es, eb, rel_err(V, sol["V"][:N])))
    assert es <= TOL_SYSTEM and eb <= TOL_SYSTEM
    assert rel_err(V, sol["V"][:N]) <= TOL_V
    for c in range(len(kw.get("conductors", ()))):
        g = electro.charge_functional(kw, c)
        assert abs(q[c] - electro.charge(kw, V, c)) <= 1e-10 * abs(q[c])
        assert abs(q[c] - g @ sol["V"][:N]) <= np.abs(g).sum() * 1e-6 * np.abs(sol["V"][:N]).max()


def _floating_ring():
    nx = ny = 25
    x, y, p = electro.grid(nx, ny, 48.0, 48.0)
    ix, iy = np.arange(nx * ny) % nx, np.arange(nx * ny) // nx
    cond = -np.ones(nx * ny, np.int32)
    cond[ix == 0] = 0
    cond[ix == nx - 1] = 1
    ring = (np.maximum(abs(ix - 12), abs(iy - 12)) == 3)           # 24 nodes, free layers around it
    cond[ring] = 2
    return dict(x=x, y=y, p=p, lbl=np.zeros(len(p), np.int32), blocks=[dict(ex=2.0, ey=2.0)],
                labels=[dict(block=0)], conductor=cond,
                conductors=[dict(type=1, V=10.0), dict(type=1, V=0.0), dict(type=0, q=3e-11)], depth=1.5,
                length_units=1), ring


def test_floating_conductor():
    """A ring of 24 nodes with a prescribed charge between two fixed-voltage
    conductors: its merged row (longer than the 12-entry LDS rows, in a
    workgroup with LDS rows) gives one potential, bit-equal on all its nodes."""
    kw, ring = _floating_ring()
    assert ring.sum() >= 16
    sol = electro.restate(kw)
    N = len(kw["x"])
    P, r, V = _solve(kw)
    rp = P.csr()[0]
    Vc, q = P.conductors()
    qi = P.conductor_charge(2)
    P.close()
    rep = int(np.flatnonzero(ring)[0])
    assert rp[rep + 1] - rp[rep] > 12
    assert len(set(V[ring].tolist())) == 1 and Vc[2] == V[rep]
    g = electro.charge_functional(kw, 2)
    bound = np.abs(g).sum() * 1e-6 * np.abs(sol["V"][:N]).max()
    print("floating: V %.3e, V_c %.9g (direct %.9g), q %.6e of %.6e (bound %.3e), precond %d"
          % (rel_err(V, sol["V"][:N]), Vc[2], sol["V"][N + 2], qi, 3e-11, bound, r["precond"]))
    assert rel_err(V, sol["V"][:N]) <= TOL_V
    assert abs(Vc[2] - sol["V"][N + 2]) <= TOL_V * np.abs(sol["V"][:N]).max()
    assert abs(qi - 3e-11) <= bound
    assert q[2] == 3e-11


def test_repeat_and_jacobi():
    kw, ring = _floating_ring()
    P, r, V = _solve(kw)
    c1 = P.conductors()
    P.solve()
    V2, c2 = P.solution(), P.conductors()
    assert (V == V2).all() and (c1[0] == c2[0]).all() and (c1[1] == c2[1]).all()
    P.set_option(kernels.XFK_OPT_PRECOND, kernels.XFK_PRECOND_JACOBI)
    r3 = P.solve()
    V3 = P.solution()
    assert r3["precond"] == kernels.XFK_PRECOND_JACOBI
    assert rel_err(V3, V) <= TOL_V
    assert P.memory()["chunk_bytes"] > 0
    P.close()


def test_wrong_solver_is_refused():
    kw, _ = _floating_ring()
    P = kernels.ElectrostaticProblem(**kw)
    L = kernels.load_library()
    res = kernels.Result()
    assert L.xfk_static2d(P._h, 0, C.byref(res)) == -1
    assert "electrostatic" in L.xfk_last_error().decode()
    assert L.xfk_harmonic2d(P._h, 0, C.byref(res)) == -1
    P.close()
    M = kernels.Static2DProblem(**synth.magnetostatic(8))
    assert L.xfk_electrostatic(M._h, 0, C.byref(res)) == -1
    M.close()
