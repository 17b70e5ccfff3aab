"""The problems and iterates of the Newton-pass tests: shared by the device
test (tests/test_gpu_newton_pass.py) and the host test that asserts which
branches they reach (tests/test_newtonref_cpu.py).  Host only.

A case is (name, kwargs of kernels.Static2DProblem, chains): every chain a
list of iterates V_1 .. V_k for Newton passes 1 .. k after the first pass.
The iterates are chosen, not solved for: gradient fields scaled so that the
largest B in the steel is 0 T, 1e-6 T (first knot interval), 0.8 T, the middle
of the last knot interval and twice the last knot, a seeded smooth field for a
spread of B, and a two- and a three-pass chain of different fields, so that a
pass reads the state another one wrote."""
import numpy as np

import irregular
import newtonref as nr
from xfemm_amd import synth
from xfemm_amd.fsolver import bh_get_slopes

STEEL = 1      # the steel block of every synth problem


def variant(kw, lam_type, fill, extras=True):
    """The steel block as lamination type lam_type, fill factor fill, its
    table from GetSlopes as synth builds it; extras: two air elements become
    a type-0 block with a table and mu_x != mu_y (Newton off: the state is
    kept), two more a type-3 block with a table (treated as linear, mu = 1)."""
    kw = {k: v for k, v in kw.items() if k not in ("hubs", "orig", "sign")}
    blocks = [dict(b) for b in kw["blocks"]]
    labels = [dict(lb) for lb in kw["labels"]]
    B, H, S, mu = bh_get_slopes(*synth.m19_curve(), lam_type=lam_type, lam_fill=fill)
    blocks[STEEL] = dict(mu_x=mu, mu_y=mu, LamFill=fill, LamType=lam_type, B=B, H=H, slope=S)
    lbl = np.array(kw["lbl"], np.int32)
    if extras:
        B0, H0, S0, mu0 = bh_get_slopes(*synth.m19_curve(), lam_type=0, lam_fill=1.0)
        blocks.append(dict(mu_x=0.5 * mu0, mu_y=mu0, LamFill=1.0, LamType=0, B=B0, H=H0, slope=S0))
        blocks.append(dict(mu_x=mu0, mu_y=mu0, LamFill=0.9, LamType=3, B=B0, H=H0, slope=S0))
        labels += [dict(block=len(blocks) - 2), dict(block=len(blocks) - 1)]
        air = np.nonzero(np.array([labels[l]["block"] for l in lbl]) == 0)[0]
        lbl[air[[3, 4]]] = len(labels) - 2
        lbl[air[[10, 11]]] = len(labels) - 1
    return dict(kw, blocks=blocks, labels=labels, lbl=lbl)


def zero_dirichlet(kw):
    """bc_showcase with every prescribed value 0: the Dirichlet step then
    leaves the free rows of the matrix and of b alone."""
    lines = [dict(ln, A0=0.0, A1=0.0, A2=0.0) if ln.get("format", 0) == 0 else ln for ln in kw["lines"]]
    points = [dict(q, A_re=0.0) for q in kw["points"]]
    return dict(kw, lines=lines, points=points)


def problems():
    """(name, kwargs): every mesh with some of the lamination variants, each
    variant on a planar, a showcase, an axisymmetric and (types 0 and 2) the
    wheel mesh."""
    out = []

    def add(name, kw, variants):
        for t, f in variants:
            out.append(("%s-lam%d-%g" % (name, t, f), variant(kw, t, f)))

    add("ms8", synth.magnetostatic(8, nonlinear=True), [(0, 0.98), (1, 0.5), (2, 0.98)])
    add("ms12", synth.magnetostatic(12, nonlinear=True), [(0, 0.5), (1, 0.98), (2, 0.5)])
    add("sc8", zero_dirichlet(synth.bc_showcase(8, nonlinear=True)), [(0, 0.98), (1, 0.98)])
    add("sc12", zero_dirichlet(synth.bc_showcase(12, nonlinear=True)), [(0, 0.98), (2, 0.98)])
    add("ax10", synth.axisymmetric(10, nonlinear=True), [(0, 0.98), (0, 0.5), (1, 0.98), (1, 0.5), (2, 0.98), (2, 0.5)])
    add("axext10", synth.axisymmetric(10, nonlinear=True, circuit=True, external=True), [(0, 0.98)])
    add("wheel16", irregular.wheel(16, 3, nonlinear=True), [(0, 0.98), (2, 0.5)])
    return out


def fields(kw):
    """Three unit fields: planar g x, g y, g (x + 0.3 y); axisymmetric (V = 0
    on the axis) g r^2, g r z, g (r^2 + 0.3 r z)."""
    x, y = np.asarray(kw["x"], float), np.asarray(kw["y"], float)
    if kw.get("problem_type", 0) == 1:
        return [x * x, x * y, x * x + 0.3 * x * y]
    return [x, y, x + 0.3 * y]


def smooth_random(kw, seed):
    x, y = np.asarray(kw["x"], float), np.asarray(kw["y"], float)
    L = max(np.ptp(x), np.ptp(y))
    rng = np.random.default_rng(seed)
    V = np.zeros(len(x))
    for _ in range(4):
        kx, ky = rng.uniform(0.5, 2.5, 2) * np.pi / L
        V += rng.normal() * np.sin(kx * x + rng.uniform(0, np.pi)) * np.cos(ky * y + rng.uniform(0, np.pi))
    return V * x if kw.get("problem_type", 0) == 1 else V


def chains(kw, P=None):
    """The chains of iterates of one problem (see the module docstring)."""
    P = P or nr.prepare(kw)
    first = nr.newton_pass(P, first=True)
    state = (first["mu1"], first["mu2"])
    Bd = np.asarray(kw["blocks"][STEEL]["B"], float)
    steel = P.blk == STEEL

    def scaled(F, target):
        r = nr.newton_pass(P, F, state, newton_terms=False)
        return F * (target / float(r["B"].v[steel].max()))

    F = fields(kw)
    last, twice = 0.5 * (Bd[-2] + Bd[-1]), 2.0 * Bd[-1]
    single = [np.zeros(P.N), scaled(F[0], 1.0e-6), scaled(F[1], 0.8), scaled(F[2], last), scaled(F[0], twice),
              scaled(smooth_random(kw, 7), 1.6)]
    out = [[V] for V in single]
    out.append([scaled(F[0], 0.8), scaled(F[1], last)])
    out.append([scaled(smooth_random(kw, 11), 1.2), scaled(F[2], 1.0e-6), scaled(F[1], twice)])
    return out
