"""Heat-flow problems on the device (xfk_heatflow) against the reference's
solved fixtures, closed forms, and the literal restatement of
HSolver::AnalyzeProblem solved directly (tests/heat.py).

Bounds: an assembled system within 1e-12 of the restatement's (matrix by
max-entry norm, right-hand side after the boundary conditions: the project's
bound for assembled systems); T within 1e-6 of max |T| of the restatement's
outer loop, with the same number of passes; the flow kernel within 1e-9 of the
restated ChargeOnConductor on the T the device returned (only the summation
order differs).  Every nonlinear input below was run through the restatement
alone first: its last change and the one before are at least a factor 10 away
from 100 Precision on either side (each case's Precision is chosen for that;
test_matches_restated_loop asserts it again), so a borderline stop cannot
decide a pass count."""
import ctypes as C
import os

import numpy as np
import pytest
import scipy.sparse as sp

import heat
from util import GOLDEN, rel_err
from xfemm_amd import kernels, synth

pytestmark = pytest.mark.gpu

TOL_SYSTEM = 1e-12
TOL_V = 1e-6
TOL_FLOW = 1e-9


def _system_err(P, sol):
    """test_gpu_electro's measure on sparse storage (the fixtures' dense
    matrices would be 155 MB each): max |G - Go| / max |Go| over the N x N
    block, max |b - bo| / max |bo|."""
    rp, col, val, b = P.csr()
    n = len(rp) - 1
    G = sp.csr_matrix((val, col, rp), shape=(n, n))
    Go, bo = sol["As"][:n, :n], sol["b"][:n]
    D = (G - Go).tocoo()
    return (np.abs(D.data).max() if D.nnz else 0.0) / np.abs(Go.data).max(), \
        np.abs(b - bo).max() / max(np.abs(bo).max(), 1e-300)


def _field(kw, lo, hi):
    """A smooth non-constant field over [lo, hi]."""
    x, y = np.asarray(kw["x"]), np.asarray(kw["y"])
    s = (x - x.min()) / (x.max() - x.min())
    t = (y - y.min()) / (y.max() - y.min())
    return lo + (hi - lo) * (0.8 * s + 0.2 * t * t)


# ---- the reference's fixtures ------------------------------------------------

@pytest.fixture(scope="module")
def fixtures():
    f0 = heat.read_anh(os.path.join(GOLDEN, "hsolver", "Temp0.anh.check.gz"))
    f1 = heat.read_anh(os.path.join(GOLDEN, "hsolver", "Temp1.anh.check.gz"))
    f1["kw"]["t_prev"] = f0["V"].copy()
    for f in (f0, f1):
        f["sol"] = heat.restate_solve(f["kw"])
    return f0, f1


@pytest.mark.parametrize("which,at", [(0, "zero"), (0, "recorded"), (1, "recorded")],
                         ids=["Temp0-T0", "Temp0-Tsolved", "Temp1-Tsolved"])
def test_fixture_system(fixtures, which, at):
    f = fixtures[which]
    T = None if at == "zero" else f["V"]
    sol = heat.restate(f["kw"], T, dense=False)
    P = kernels.HeatFlowProblem(**f["kw"])
    P.assemble(T)
    es, eb = _system_err(P, sol)
    P.close()
    print("fixture %d at %s: matrix %.3e rhs %.3e" % (which, at, es, eb))
    assert es <= TOL_SYSTEM and eb <= TOL_SYSTEM


@pytest.mark.parametrize("which", [0, 1], ids=["Temp0", "Temp1"])
def test_fixture_solution(fixtures, which):
    f = fixtures[which]
    P = kernels.HeatFlowProblem(**f["kw"])
    r = P.solve()
    V = P.solution()
    P.close()
    ref = f["sol"]
    print("fixture %d: vs restatement %.3e, vs recorded %.3e, passes %d (restatement %d, changes %s), last change %.3e"
          % (which, rel_err(V, ref["V"]), rel_err(V, f["V"]), r["newton_iters"], ref["passes"], ref["changes"],
             r["last_res"]))
    assert rel_err(V, ref["V"]) <= TOL_V
    assert rel_err(V, f["V"]) <= TOL_V        # the recorded solution is within 2e-8 of the restatement's
    assert r["newton_iters"] == ref["passes"] == 3
    assert r["precond"] == kernels.XFK_PRECOND_AMG


# ---- synthetic grids ---------------------------------------------------------

def _planar_everything(nx, ny):
    """Two blocks (one with a 3-point table), fixed / flux / convection /
    radiation edges, a fixed point, a point source, a prescribed-temperature
    conductor and a time step."""
    w, h = 0.30, 0.20
    x, y, p = heat.grid(nx, ny, w, h)
    lbl = (x[p].mean(axis=1) > w / 2).astype(np.int32)
    e = heat.tag_edges(x, y, p, [
        (lambda xa, ya, xb, yb: xa == 0 and xb == 0, 0),          # fixed T
        (lambda xa, ya, xb, yb: ya == h and yb == h, 1),          # convection
        (lambda xa, ya, xb, yb: ya == 0 and yb == 0, 2),          # flux
        (lambda xa, ya, xb, yb: xa == w and xb == w, 3)])         # radiation
    marker = -np.ones(len(x), np.int32)
    marker[(ny // 2) * nx + nx // 3] = 0                          # point source
    marker[(ny // 3) * nx + 2 * nx // 3] = 1                      # fixed-temperature point
    cond = -np.ones(len(x), np.int32)
    cond[(2 * ny // 3) * nx + nx // 2] = 0
    cond[(2 * ny // 3) * nx + nx // 2 + 1] = 0
    kw = dict(x=x, y=y, p=p, e=e, lbl=lbl, marker=marker, conductor=cond,
              blocks=[dict(kx=2.0, ky=3.0, kt=4e4, qv=5e3),
                      dict(kx=9.0, ky=9.0, kt=6e4, T=[300.0, 350.0, 420.0], K=[1.0, 1.8, 1.4])],
              labels=[dict(block=0), dict(block=1)],
              lines=[dict(format=0, Tset=400.0), dict(format=2, h=15.0, Tinf=290.0), dict(format=1, qs=-200.0),
                     dict(format=3, beta=0.8, Tinf=280.0)],
              points=[dict(qp=30.0), dict(T=380.0)], conductors=[dict(type=1, T=360.0)],
              depth=50.0, length_units=2, dt=50.0, precision=6e-10)
    kw["t_prev"] = _field(kw, 330.0, 390.0)
    return kw


def _axi_external(nx, ny):
    """Axisymmetric with an exterior region, a table on every element,
    convection and radiation edges in their axisymmetric form, and a floating
    conductor: a ring of 8 nodes around the grid's centre with free,
    source-free nodes around it (where the merged and the bordered form agree),
    whose merged row is longer than the 12 LDS entries."""
    x, y, p = heat.grid(nx, ny, 0.040, 0.050, x0=0.005, y0=-0.025)
    cx, cy = x[p].mean(axis=1), y[p].mean(axis=1)
    lbl = (cx * cx + cy * cy > 0.030 ** 2).astype(np.int32)
    e = heat.tag_edges(x, y, p, [(lambda xa, ya, xb, yb: xa == 0.005 and xb == 0.005, 0),
                                 (lambda xa, ya, xb, yb: xa == x.max() and xb == x.max(), 1),
                                 (lambda xa, ya, xb, yb: ya == y.max() and yb == y.max(), 2)])
    assert (e == 1).sum() == ny - 1 and (e == 2).sum() == nx - 1
    ix, iy = np.arange(nx * ny) % nx, np.arange(nx * ny) // nx
    cond = np.where(np.maximum(abs(ix - nx // 2), abs(iy - ny // 2)) == 1, 0, -1).astype(np.int32)
    return dict(x=x, y=y, p=p, e=e, lbl=lbl, conductor=cond,
                blocks=[dict(kx=1.0, ky=1.0, T=[300.0, 400.0, 520.0], K=[0.79, 0.8, 0.81])],
                labels=[dict(block=0), dict(block=0, is_external=1)],
                lines=[dict(format=0, Tset=500.0), dict(format=2, h=40.0, Tinf=300.0),
                       dict(format=3, beta=0.9, Tinf=310.0)],
                conductors=[dict(type=0, q=2.0)], length_units=3, problem_type=1,
                ext_ro=0.030, ext_ri=0.020, ext_zo=0.001, precision=2.3e-9)


def _periodic(nx, ny, anti):
    """Bottom and top rows paired; a table whose knots straddle the answer."""
    x, y, p = heat.grid(nx, ny, 0.24, 0.16)
    e = heat.tag_edges(x, y, p, [(lambda xa, ya, xb, yb: xa == 0 and xb == 0, 0),
                                 (lambda xa, ya, xb, yb: xa == 0.24 and xb == 0.24, 1)])
    lbl = (x[p].mean(axis=1) > 0.10).astype(np.int32)
    pbc = [[i, (ny - 1) * nx + i, 1 if anti else 0] for i in range(1, nx - 1)]
    lo, hi = (-40.0, 60.0) if anti else (300.0, 400.0)
    K = [1.0, 2.0, 4.0] if anti else [1.0, 1.05, 1.1]
    return dict(x=x, y=y, p=p, e=e, lbl=lbl, pbc=pbc, precision=4.3e-8 if anti else 4.3e-9,
                blocks=[dict(kx=1.0, ky=2.0), dict(kx=1.0, ky=1.0, qv=2e3, T=[lo, (lo + hi) / 2, hi], K=K)],
                labels=[dict(block=0), dict(block=1)],
                lines=[dict(format=0, Tset=0.0 if anti else 380.0), dict(format=0, Tset=0.0 if anti else 320.0)],
                depth=2.0, length_units=3)


CASES = {"planar": _planar_everything, "axi_external": _axi_external,
         "periodic": lambda nx, ny: _periodic(nx, ny, False), "antiperiodic": lambda nx, ny: _periodic(nx, ny, True)}
SIZES = [(9, 7), (65, 49)]      # one partial row-gather workgroup; 3185 rows: 25 workgroups and a coarse AMG level


def _assembly_field(kw):
    """Smooth and non-constant, with values below the first knot, above the
    last and exactly on knots of the table (two nodes of the table's block)."""
    tab = [b for b in kw["blocks"] if b.get("T") is not None][0]["T"]
    T = _field(kw, tab[0] - 25.0, tab[-1] + 40.0)
    blk = np.array([kw["labels"][l]["block"] for l in kw["lbl"]])
    tb = [k for k, b in enumerate(kw["blocks"]) if b.get("T") is not None][0]
    nodes = np.unique(np.asarray(kw["p"])[blk == tb])
    T[nodes[len(nodes) // 2]] = tab[1]
    T[nodes[len(nodes) // 3]] = tab[0]
    assert T.min() < tab[0] and T.max() > tab[-1]
    return T


@pytest.mark.parametrize("size", SIZES, ids=["9x7", "65x49"])
@pytest.mark.parametrize("case", ["planar", "axi_external"])
def test_assembled_system(case, size):
    kw = CASES[case](*size)
    for b in kw["blocks"]:      # (a steep table here: no loop has to converge on it)
        if b.get("T") is not None:
            b["K"] = [0.5, 0.8, 1.3]
    T = _assembly_field(kw)
    sol = heat.restate(kw, T, merged=True, dense=False)
    P = kernels.HeatFlowProblem(**kw)
    P.assemble(T)
    es, eb = _system_err(P, sol)
    rp = P.csr()[0]
    P.assemble()
    es0, eb0 = _system_err(P, heat.restate(kw, None, merged=True, dense=False))
    P.close()
    print("%s %s: at T matrix %.3e rhs %.3e; at 0 matrix %.3e rhs %.3e" % (case, size, es, eb, es0, eb0))
    assert es <= TOL_SYSTEM and eb <= TOL_SYSTEM
    assert es0 <= TOL_SYSTEM and eb0 <= TOL_SYSTEM
    if case == "axi_external":      # the merged conductor's row took the in-place path
        rep = int(np.flatnonzero(kw["conductor"] == 0)[0])
        assert rp[rep + 1] - rp[rep] > 12


@pytest.mark.parametrize("size", SIZES, ids=["9x7", "65x49"])
@pytest.mark.parametrize("case", list(CASES))
def test_matches_restated_loop(case, size):
    kw = CASES[case](*size)
    ref = heat.restate_solve(kw)
    N = len(kw["x"])
    ch = ref["changes"]
    # (the inputs' margin, checked where the test runs too)
    stop = 100. * kw["precision"]
    assert ch[-1] < stop / 10 and all(c > 10 * stop for c in ch[:-1]), ch
    P = kernels.HeatFlowProblem(**kw)
    r = P.solve()
    V = P.solution()
    Tc, q = P.conductors()
    qi = [P.conductor_flow(c) for c in range(len(q))]
    P.close()
    print("%s %s: T %.3e, passes %d (restatement %d, changes %s), levels %d"
          % (case, size, rel_err(V, ref["V"][:N]), r["newton_iters"], ref["passes"], ch, r["amg_levels"]))
    assert rel_err(V, ref["V"][:N]) <= TOL_V
    assert r["newton_iters"] == ref["passes"]
    if size == SIZES[1]:
        assert r["precond"] == kernels.XFK_PRECOND_AMG and r["amg_levels"] >= 2
    for c, cd in enumerate(kw.get("conductors", ())):
        qr = heat.flow(kw, V, c)
        assert abs(qi[c] - qr) <= TOL_FLOW * abs(qr)
        if cd["type"] == 1:
            assert q[c] == qi[c] and Tc[c] == cd["T"]       # the same kernel, the same bits
        else:
            ring = np.flatnonzero(kw["conductor"] == c)
            assert q[c] == cd["q"] and len(set(V[ring].tolist())) == 1 and Tc[c] == V[ring[0]]
            assert abs(Tc[c] - ref["V"][N + c]) <= TOL_V * np.abs(ref["V"][:N]).max()


# ---- closed forms on a strip -------------------------------------------------

L_STRIP, H_STRIP, K_STRIP, T0_STRIP, DEPTH_STRIP = 0.10, 0.02, 2.0, 400.0, 0.5


def _strip(right, conductor=False, **over):
    x, y, p = heat.grid(9, 3, L_STRIP, H_STRIP)
    rules = [(lambda xa, ya, xb, yb: xa == L_STRIP and xb == L_STRIP, 1)]
    if not conductor:
        rules.append((lambda xa, ya, xb, yb: xa == 0 and xb == 0, 0))
    kw = dict(x=x, y=y, p=p, e=heat.tag_edges(x, y, p, rules), lbl=np.zeros(len(p), np.int32),
              blocks=[dict(kx=K_STRIP, ky=K_STRIP)], labels=[dict(block=0)],
              lines=[dict(format=0, Tset=T0_STRIP), right], depth=DEPTH_STRIP, length_units=3)
    if conductor:
        kw.update(conductors=[dict(type=1, T=T0_STRIP)], conductor=np.where(x == 0, 0, -1).astype(np.int32))
    kw.update(over)
    return kw


def test_strip_convection_exact():
    """k (T0 - T1) / L = h (T1 - Tinf): T is linear in x, which linear elements
    hold exactly, so the answer is exact to the PCG's precision (1e-12 asked;
    1e-9 of T0 allowed, as the exact plate capacitors of test_gpu_electro).
    The left side as a CircType 1 conductor: its flow is
    h (T1 - Tinf) Depth height; T's error 1e-9 T0 is amplified by
    T0 / (T0 - T1) < 10 in the gradient, so 1e-8 relative."""
    h, Tinf = 50.0, 300.0
    T1 = (K_STRIP / L_STRIP * T0_STRIP + h * Tinf) / (K_STRIP / L_STRIP + h)
    exact = T0_STRIP + (T1 - T0_STRIP) * heat.grid(9, 3, L_STRIP, H_STRIP)[0] / L_STRIP
    for conductor in (False, True):
        kw = _strip(dict(format=2, h=h, Tinf=Tinf), conductor=conductor, precision=1e-12)
        P = kernels.HeatFlowProblem(**kw)
        r = P.solve()
        V = P.solution()
        q = P.conductors()[1] if conductor else None
        P.close()
        print("convection strip (conductor %s): T %.3e of T0, T1 %.12g (exact %.12g)"
              % (conductor, np.abs(V - exact).max() / T0_STRIP, V[8], T1))
        assert r["newton_iters"] == 1
        assert np.abs(V - exact).max() <= 1e-9 * T0_STRIP
        if conductor:
            q_exact = h * (T1 - Tinf) * DEPTH_STRIP * H_STRIP
            print("  flow %.12g (exact %.12g)" % (q[0], q_exact))
            assert abs(q[0] - q_exact) <= 1e-8 * q_exact


def test_strip_radiation():
    """k (T0 - T1) / L = beta ksb (T1^4 - Tinf^4), T1 by bisection.  The
    stopping rule bounds the last change by 1e-6 in the 2-norm; the factor 10
    covers the conversion to one node on this mesh: 1e-5 relative.  (The
    restatement's T1 is within 1e-9 of the bisection's on the CPU.)  The fixed
    left edge keeps pass 0, where Tlast = 0 gives c0 = 0, regular."""
    beta, Tinf = 0.9, 300.0
    f = lambda t: K_STRIP * (T0_STRIP - t) / L_STRIP - beta * heat.KSB * (t ** 4 - Tinf ** 4)
    lo, hi = Tinf, T0_STRIP
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if f(mid) > 0 else (lo, mid)
    T1 = 0.5 * (lo + hi)
    kw = _strip(dict(format=3, beta=beta, Tinf=Tinf))
    ref = heat.restate_solve(kw)
    P = kernels.HeatFlowProblem(**kw)
    r = P.solve()
    V = P.solution()
    P.close()
    right = np.asarray(kw["x"]) == L_STRIP
    print("radiation strip: T1 %.10g (bisection %.10g, restatement %.10g), passes %d (restatement %d, changes %s)"
          % (V[8], T1, ref["V"][8], r["newton_iters"], ref["passes"], ref["changes"]))
    assert np.abs(ref["V"][right] - T1).max() <= 1e-5 * T1
    assert np.abs(V[right] - T1).max() <= 1e-5 * T1
    assert r["newton_iters"] == ref["passes"] >= 2


# ---- time stepping -----------------------------------------------------------

def _body(**over):
    x, y, p = heat.grid(9, 7, 0.3, 0.2)
    kw = dict(x=x, y=y, p=p, lbl=np.zeros(len(p), np.int32), blocks=[dict(kx=3.0, ky=2.0, kt=2e5, qv=4e4)],
              labels=[dict(block=0)], depth=1.0, length_units=3, precision=1e-12)
    kw.update(over)
    return kw


def test_time_steps_uniform_body():
    """No boundary condition, uniform heating and a uniform previous
    temperature: T = Tprev + dt qv / Kt at every node (the stiffness rows sum to
    zero; the capacity term is the whole equation), to the PCG's 1e-12 -- 1e-9
    allowed.  Three advance(dt) steps on the device equal three steps fed from
    the host bit for bit."""
    dt, T = 25.0, 300.0
    N = 63
    A = kernels.HeatFlowProblem(**_body(dt=dt, t_prev=np.full(N, T)))
    B = kernels.HeatFlowProblem(**_body())
    Vb = np.full(N, T)
    for step in range(3):
        ra = A.solve()
        Va = A.solution()
        B.set_step(dt, Vb)
        B.solve()
        Vb = B.solution()
        T += dt * 4e4 / 2e5
        print("step %d: T %.12g (exact %.12g), passes %d" % (step, Va[0], T, ra["newton_iters"]))
        assert ra["newton_iters"] == 1
        assert np.abs(Va - T).max() <= 1e-9 * T
        assert (Va == Vb).all()
        A.advance(dt)
    A.close()
    B.close()


# ---- conductor flow, pass counts, the cap, the wrong solver ---------------------

def test_flow_is_deterministic():
    kw = _axi_external(*SIZES[1])
    kw["conductors"] = [dict(type=1, T=450.0)]       # 8 nodes, their elements in one workgroup chunk ...
    kw["conductor"] = np.where(kw["x"] == kw["x"].max(), 1, kw["conductor"]).astype(np.int32)
    kw["conductors"].append(dict(type=1, T=320.0))   # ... and a side of 49 nodes
    kw["e"] = np.where(kw["e"] == 1, -1, kw["e"]).astype(np.int32)
    out = []
    for run in range(2):
        P = kernels.HeatFlowProblem(**kw)
        P.solve()
        V = P.solution()
        out.append((V, P.conductors()[1], [P.conductor_flow(c) for c in range(2)]))
        P.close()
    (V, q, qi), (V2, q2, qi2) = out
    assert (V == V2).all() and (q == q2).all() and qi == qi2 and list(q) == qi
    for c in range(2):
        qr = heat.flow(kw, V, c)
        print("conductor %d: flow %.12g, restated %.12g" % (c, q[c], qr))
        assert abs(q[c] - qr) <= TOL_FLOW * abs(qr)


def test_pass_counts():
    """A linear problem takes one pass; a table alone or a radiation edge alone
    makes it nonlinear: at least two (no test is made from T = 0)."""
    lin = kernels.HeatFlowProblem(**_strip(dict(format=2, h=50.0, Tinf=300.0)))
    assert lin.solve()["newton_iters"] == 1
    lin.close()
    tab = kernels.HeatFlowProblem(**_strip(dict(format=2, h=50.0, Tinf=300.0),
                                           blocks=[dict(kx=1.0, ky=1.0, T=[300.0, 400.0], K=[1.0, 2.0])]))
    rad = kernels.HeatFlowProblem(**_strip(dict(format=3, beta=0.9, Tinf=300.0)))
    nt, nr = tab.solve()["newton_iters"], rad.solve()["newton_iters"]
    tab.close()
    rad.close()
    print("passes: table %d, radiation %d" % (nt, nr))
    assert nt >= 2 and nr >= 2


def test_table_beyond_the_first_elements_is_seen():
    """The nonlinearity scan reads every element: a table on the block of the
    LAST element only (beyond the first NumNodes = 27 of 32) still makes the
    loop iterate."""
    kw = _strip(dict(format=2, h=50.0, Tinf=300.0),
                blocks=[dict(kx=2.0, ky=2.0), dict(kx=1.0, ky=1.0, T=[300.0, 400.0], K=[1.0, 2.0])],
                labels=[dict(block=0), dict(block=1)], precision=1.2e-9)
    assert len(kw["lbl"]) == 32 and len(kw["x"]) == 27
    kw["lbl"][-1] = 1
    P = kernels.HeatFlowProblem(**kw)
    n = P.solve()["newton_iters"]
    P.close()
    assert n >= 2 and n == heat.restate_solve(kw)["passes"]


def test_pass_cap():
    P = kernels.HeatFlowProblem(**_strip(dict(format=3, beta=0.9, Tinf=300.0)))
    P.set_option(kernels.XFK_OPT_HEAT_MAX_PASSES, 1)
    with pytest.raises(kernels.XfkError) as ei:
        P.solve()
    assert str(ei.value) == "xfk error -4: heat-flow iteration did not converge in 1 passes"
    P.set_option(kernels.XFK_OPT_HEAT_MAX_PASSES, 100)
    assert P.solve()["newton_iters"] >= 2      # the problem is usable afterwards
    P.close()


def test_wrong_solver_is_refused():
    P = kernels.HeatFlowProblem(**_strip(dict(format=2, h=50.0, Tinf=300.0)))
    L = kernels.load_library()
    res = kernels.Result()
    assert L.xfk_static2d(P._h, 0, C.byref(res)) == -1
    assert "heat-flow" in L.xfk_last_error().decode()
    assert L.xfk_electrostatic(P._h, 0, C.byref(res)) == -1
    assert L.xfk_harmonic2d(P._h, 0, C.byref(res)) == -1
    P.close()
    M = kernels.Static2DProblem(**synth.magnetostatic(8))
    assert L.xfk_heatflow(M._h, 0, C.byref(res)) == -1
    assert "not a heat-flow problem" in L.xfk_last_error().decode()
    assert L.xfk_heatflow_assemble(M._h, None) == -1
    M.close()
