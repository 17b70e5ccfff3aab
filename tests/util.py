"""Shared test helpers: feed identical inputs to the oracle and to the HIP path."""
from __future__ import annotations

import os

import numpy as np
import scipy.sparse as sp

from oracle import femfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def kernel_kwargs(pr: femfile.FemProblem, mesh: femfile.Mesh) -> dict:
    """Oracle-parsed problem -> keyword arguments of kernels.Static2DProblem."""
    blocks = []
    for m in pr.blocks:
        b = dict(mu_x=m.mu_x, mu_y=m.mu_y, H_c=m.H_c, J_re=m.J_re, Cduct=m.Cduct, LamFill=m.LamFill,
                 LamType=m.LamType, J_im=m.J_im, Theta_hx=m.Theta_hx, Theta_hy=m.Theta_hy, Lam_d=m.Lam_d)
        if m.BHpoints:
            b.update(B=np.array(m.Bdata), H=np.array(m.Hdata), slope=np.array(m.slope))
        blocks.append(b)
    labels = [dict(block=max(lb.BlockType, 0), in_circuit=lb.InCircuit, mag_dir=lb.MagDir,
                   is_wound=int(lb.bIsWound), is_external=int(lb.IsExternal),
                   prox_mu=complex(lb.ProximityMu), mag_dir_fctn=lb.MagDirFctn) for lb in pr.labels]
    lines = [dict(format=b.BdryFormat, A0=b.A0, A1=b.A1, A2=b.A2, phi=b.phi, c0=b.c0, c1=b.c1, c0_im=b.c0i,
                  c1_im=b.c1i, Mu=b.Mu, Sig=b.Sig) for b in pr.bdrys]
    points = [dict(A_re=q.A_re, A_im=q.A_im, J_re=q.J_re, J_im=q.J_im) for q in pr.points]
    circuits = [dict(type=c.CircType, amps_re=c.Amps_re, dvolts_re=c.dVolts_re, amps_im=c.Amps_im,
                     dvolts_im=c.dVolts_im) for c in pr.circuits]
    return dict(x=mesh.x, y=mesh.y, p=mesh.p, lbl=mesh.lbl, marker=mesh.marker, e=mesh.e,
                pbc=mesh.pbc if len(mesh.pbc) else None, blocks=blocks, labels=labels, lines=lines,
                points=points, circuits=circuits, precision=pr.Precision, length_units=pr.LengthUnits,
                coords=pr.Coords, relax=pr.Relax, frequency=pr.Frequency, problem_type=pr.ProblemType,
                ext_zo=pr.extZo, ext_ro=pr.extRo, ext_ri=pr.extRi, ages=list(mesh.ages), ac_solver=pr.ACSolver)


def synth_to_oracle(kw: dict):
    """xfemm_amd.synth problem -> (FemProblem, Mesh) for the oracle (slopes via
    the oracle's GetSlopes restatement), and kernel kwargs with those slopes."""
    from xfemm_amd import synth
    pr = femfile.FemProblem()
    pr.Precision = kw["precision"]
    pr.LengthUnits = kw["length_units"]
    pr.Relax = 1.0
    pr.Frequency = kw.get("frequency", 0.0)
    pr.ProblemType = kw.get("problem_type", 0)
    pr.ACSolver = kw.get("ac_solver", 0)
    pr.extZo, pr.extRo, pr.extRi = kw.get("ext_zo", 0.0), kw.get("ext_ro", 0.0), kw.get("ext_ri", 0.0)
    for b in kw["blocks"]:
        m = femfile.BlockProp(mu_x=b.get("mu_x", 1.0), mu_y=b.get("mu_y", 1.0), H_c=b.get("H_c", 0.0),
                              J_re=b.get("J_re", 0.0), Cduct=b.get("Cduct", 0.0),
                              LamFill=b.get("LamFill", 1.0), LamType=b.get("LamType", 0),
                              J_im=b.get("J_im", 0.0), Theta_hx=b.get("Theta_hx", 0.0),
                              Theta_hy=b.get("Theta_hy", 0.0), Lam_d=b.get("Lam_d", 0.0),
                              WireD=b.get("WireD", 0.0), NStrands=b.get("NStrands", 0))
        if len(b.get("B", ())) and np.iscomplexobj(b["H"]):
            # harmonic: the GetSlopes(omega) curve (host restatement, pinned
            # against the reference by tests/test_oracle_acslopes.py)
            m.BHpoints, m.Bdata, m.Hdata, m.slope = len(b["B"]), list(b["B"]), list(b["H"]), list(b["slope"])
        elif b.get("bh") == "M19":
            B, H = synth.m19_curve()
            m.BHpoints, m.Bdata, m.Hdata = len(B), list(B), list(H)
            femfile.get_slopes(m)
        pr.blocks.append(m)
    for lb in kw["labels"]:
        pr.labels.append(femfile.BlockLabel(BlockType=lb["block"], InCircuit=lb.get("in_circuit", -1),
                                            MagDir=lb.get("mag_dir", 0.0),
                                            MagDirFctn=lb.get("mag_dir_fctn", ""),
                                            Turns=lb.get("turns", 2 if lb.get("is_wound", 0) else 1),
                                            IsExternal=bool(lb.get("is_external", 0))))
    for ln in kw["lines"]:
        pr.bdrys.append(femfile.BdryProp(BdryFormat=ln.get("format", 0), A0=ln.get("A0", 0.0),
                                         A1=ln.get("A1", 0.0), A2=ln.get("A2", 0.0), phi=ln.get("phi", 0.0),
                                         c0=ln.get("c0", 0.0), c1=ln.get("c1", 0.0), c0i=ln.get("c0_im", 0.0),
                                         c1i=ln.get("c1_im", 0.0), Mu=ln.get("Mu", 0.0), Sig=ln.get("Sig", 0.0)))
    for c in kw.get("circuits", []):
        pr.circuits.append(femfile.Circuit(CircType=c.get("type", 0), Amps_re=c.get("amps_re", 0.0),
                                           Amps_im=c.get("amps_im", 0.0), dVolts_re=c.get("dvolts_re", 0.0),
                                           dVolts_im=c.get("dvolts_im", 0.0)))
    for q in kw.get("points", []):
        pr.points.append(femfile.PointProp(A_re=q.get("A_re", 0.0), A_im=q.get("A_im", 0.0),
                                           J_re=q.get("J_re", 0.0), J_im=q.get("J_im", 0.0)))
    nn = len(kw["x"])
    marker = kw.get("marker")
    pbc = kw.get("pbc")
    mesh = femfile.Mesh(x=np.asarray(kw["x"], float), y=np.asarray(kw["y"], float),
                        marker=-np.ones(nn, np.int32) if marker is None else np.asarray(marker, np.int32),
                        p=np.asarray(kw["p"], np.int32),
                        e=np.asarray(kw["e"], np.int32), lbl=np.asarray(kw["lbl"], np.int32),
                        blk=np.array([kw["labels"][l]["block"] for l in kw["lbl"]], np.int32),
                        pbc=np.zeros((0, 3), np.int32) if pbc is None else np.asarray(pbc, np.int32),
                        ages=list(kw.get("ages", [])))
    femfile.get_fill_factor(pr, mesh)
    return pr, mesh, kernel_kwargs(pr, mesh)


def rel_err(a, b):
    a = np.asarray(a)
    b = np.asarray(b)
    scale = max(np.abs(b).max(), 1e-300)
    return float(np.abs(a - b).max() / scale)


C_ANS = 3.141592653589793238462643383 * 4.0e-5   # A = V * c (static2d.cpp:66, 1018-1021)


CONVERGED_PRECISION = 1e-13


def converged(pr, mesh, solve=None):
    """The oracle run to convergence: the reference's own algorithm (restated
    Static2D / Harmonic2D with SSOR-PCG / COCG) at Precision 1e-13 instead of
    the problem's.  The parity contract of the AMG path is

        max|A_gpu - A_converged| <= tol * max|A_converged|   (tol fixed per test)

    The reference stops its SSOR-PCG at sqrt(z.r / z0.b) <= Precision
    (spars.cpp:259/313); on ill-conditioned steel problems that leaves slow-mode
    error (2.6e-5 of max|A| on bc_showcase(24, nonlinear) at Precision 1e-8)
    which the AMG-PCG, stopping on the same test, resolves.  The target is built
    from the oracle alone, so it cannot move with the device's result; the
    plain distance to the oracle at the problem's Precision is reported next to
    it (``parity_message``).  Measured: the oracle at 1e-13 is within 7e-14 of a
    direct solve of its own system (linear) and within 2e-12 of its 1e-15 run
    (nonlinear)."""
    import copy
    from oracle import oracle
    pr2 = copy.deepcopy(pr)
    pr2.Precision = CONVERGED_PRECISION
    return (solve or oracle.solve)(pr2, mesh)[0]


def precision_bound(Ao, Ac, tol):
    """The bound the device answer keeps to the reference's own output at the
    problem's Precision (the oracle, bit-identical to the reference, stopped
    where the reference stops): max(tol, 2 x the reference's own distance to
    its converged answer).  The reference's SSOR-PCG leaves slow-mode error
    e_ref = |Ao - Ac| (up to 2.6e-5 of max|A| on the steel systems); the device
    answer is within tol of Ac -- in practice 1e-7 or closer -- so its distance
    to Ao is e_ref plus that, below 2 e_ref whenever e_ref is the larger, and
    below tol otherwise."""
    return max(tol, 2.0 * rel_err(Ao, Ac))


def parity_message(A, Ao, Ac, tol):
    return ("max|dA|/max|A|: vs converged oracle %.3e (tol %.1e), vs oracle at the problem Precision %.3e "
            "(bound %.3e; the oracle's own distance %.3e)"
            % (rel_err(A, Ac), tol, rel_err(A, Ao), precision_bound(Ao, Ac, tol), rel_err(Ao, Ac)))


def assert_parity(A, Ao, Ac, tol, extra=""):
    """The parity contract (DESIGN.md "Parity contract", INTEGRATION.md "What
    the answer is compared with"): within tol of the converged oracle Ac, and
    within precision_bound of the oracle at the problem's Precision Ao."""
    msg = parity_message(A, Ao, Ac, tol) + extra
    assert rel_err(A, Ac) <= tol, msg
    assert rel_err(A, Ao) <= precision_bound(Ao, Ac, tol), msg


def _laplace_random(n, seed, shift=1.0):
    """5-point operator with random positive conductances and a Dirichlet-like
    diagonal shift on the first row of nodes (SPD; shift = 0: pure Neumann,
    constants are the null space)."""
    rng = np.random.default_rng(seed)
    N = n * n
    idx = np.arange(N).reshape(n, n)
    rows, cols, vals = [], [], []
    diag = np.zeros(N)
    for a, b in [(idx[:, :-1], idx[:, 1:]), (idx[:-1, :], idx[1:, :])]:
        a = a.ravel()
        b = b.ravel()
        c = np.exp(rng.uniform(-3, 3, len(a)))
        rows += [a, b]
        cols += [b, a]
        vals += [-c, -c]
        np.add.at(diag, a, c)
        np.add.at(diag, b, c)
    diag[idx[0]] += shift
    rows.append(np.arange(N))
    cols.append(np.arange(N))
    vals.append(diag)
    M = sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(N, N))
    M.sort_indices()
    return M
