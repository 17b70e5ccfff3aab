"""The restatement of fpproc's harmonic block integrals (tests/magacref.py) held
to what it cannot get right by accident: closed forms on a uniform field, two
discrete identities of the solved problem, the circuits' prescribed currents,
and a time-domain average for the double-frequency types.  No GPU.

Measured by this file (oracle/harmonic.py at Precision 1e-12, printed by the
tests): the relative gaps of the type-0 identity and of the power balance at
10 x 10 and 20 x 20 cells are recorded in magacref.IDENTITY_*; the asserted
bounds are 10 x the larger of each pair.
"""
import numpy as np
import pytest

import magacref as R
import magpostref as M
from oracle import harmonic as oh
from util import synth_to_oracle
from xfemm_amd import synth

TOL = 1e-12
F = 60.0


@pytest.mark.parametrize("axi", [False, True])
def test_uniform_field_element_b_and_energy(axi):
    B0, phi = 0.8, 0.7
    kw, A = (R.uniform_axi if axi else R.uniform_planar)(B0=B0, phi=phi, mu_x=40.0, mu_y=40.0)
    P = R.MagAcPost(kw, A, depth=25.0)
    B = P.element_b_all()
    want = B0 * np.exp(1j * phi) * (1 if axi else -1)
    assert np.abs(B[:, 0]).max() <= TOL * B0
    assert np.abs(B[:, 1] - want).max() <= TOL * B0
    z, s = P.block_integrals([0])
    V = z[10].real
    assert abs(z[2] - B0 * B0 * V / (4. * M.MUO * 40.0)) <= 1e-12 * s[2]
    assert z[17] == z[2]
    # the geometry-only types: the static restatement's bits
    zs, _ = M.MagPost(kw, np.zeros(len(A)), depth=25.0).block_integrals([0])
    for t in (5, 10, 24, 25):
        assert z[t] == zs[t]


@pytest.mark.parametrize("axi", [False, True])
@pytest.mark.parametrize("block", [dict(Theta_hx=15.0, Theta_hy=15.0),
                                   dict(Theta_hx=8.0, Theta_hy=8.0, Lam_d=0.35, LamFill=0.95, Cduct=2.0),
                                   dict(Lam_d=0.5, LamFill=0.9)])
def test_uniform_field_hysteresis_and_lamination_loss(axi, block):
    B0 = 0.8
    blk = dict(mu_x=300.0, mu_y=300.0, **block)
    kw, A = (R.uniform_axi if axi else R.uniform_planar)(B0=B0, **blk)
    z, s = R.MagAcPost(kw, A, depth=25.0).block_integrals([0])
    w = 2. * np.pi * F
    mu = R.mu_fd(300.0, blk["Theta_hx"] if "Theta_hx" in blk else 0.0, blk.get("Lam_d", 0.0), blk.get("Cduct", 0.0),
                 blk.get("LamFill", 1.0), w)
    want = np.pi * F * B0 * B0 * z[10].real * (1. / (M.MUO * mu)).imag
    # (the scale of a rounding bound: the products the imaginary part is taken of)
    scale = np.pi * F * B0 * B0 * z[10].real / (M.MUO * abs(mu))
    assert abs(z[3] - want) <= 1e-12 * scale, (z[3], want)
    if "Theta_hx" in blk:
        assert z[3].real > 0
    assert z[4] == 0          # a lamination carries no bulk current
    assert z[6] == z[3] + z[4]


def _solved(kw):
    pr, mesh, kk = synth_to_oracle(kw)
    A, _, circs = oh.solve(pr, mesh)
    cc = (np.array([c[0] for c in circs]), np.array([c[1] for c in circs]), np.array([c[2] for c in circs]))
    return kk, A, cc


def _gaps(theta):
    out = []
    for n in (10, 20):
        kk, A, cc = _solved(R.identity_problem(n, theta))
        P = R.MagAcPost(kk, A, depth=30.0, circuits=cc)
        z, _ = P.block_integrals(np.ones(4, bool))
        zs, _ = P.block_integrals([2])
        out.append((z, zs))
    return out


def test_type0_identity():
    """type 0 over all labels is real and equals 4 x type 2 over all labels
    (real permeabilities): the eddy term's consistent mass matrix is PlnInt's"""
    g = []
    for z, _ in _gaps(0.0):
        g.append(abs(z[0] - 4. * z[2]) / abs(4. * z[2]))
    print("type-0 identity gaps (10 x 10, 20 x 20): %.3e %.3e" % tuple(g))
    assert max(g) <= R.IDENTITY_TYPE0_BOUND


def test_power_balance():
    """type 6 over all labels = -(omega / 2) Im(type 0 over the source label),
    with a hysteresis angle in the steel"""
    w = 2. * np.pi * F
    g = []
    for z, zs in _gaps(12.0):
        assert z[3].real > 0 and z[4].real > 0
        want = -(w / 2.) * zs[0].imag
        g.append(abs(z[6].real - want) / abs(want))
    print("power-balance gaps (10 x 10, 20 x 20): %.3e %.3e" % tuple(g))
    assert max(g) <= R.POWER_BALANCE_BOUND


def test_type7_is_the_circuits_current():
    kw = synth.harmonic(8)
    kk, A, cc = _solved(kw)
    P = R.MagAcPost(kk, A, depth=30.0, circuits=cc)
    T = P.terms()[7]
    for q, circ in enumerate(kw["circuits"]):
        if circ["type"] != 0:        # (a voltage-driven plate prescribes no current)
            continue
        labs = [k for k, lb in enumerate(kk["labels"]) if lb.get("in_circuit", -1) == q]
        m = np.isin(P.lbl, labs)
        amps = complex(circ.get("amps_re", 0.0), circ.get("amps_im", 0.0))
        assert abs(T[m].sum() - amps) <= 1e-12 * np.abs(T[m]).sum(), (T[m].sum(), amps)


def test_type7_case0_plate_matches_its_elements():
    """the Case-0 plate of synth.harmonic(8): type 7 is the sum of a x Javg with
    J = -I w c A - c dV (no source): independent of GetJA's restatement"""
    kw = synth.harmonic(8)
    kk, A, cc = _solved(kw)
    P = R.MagAcPost(kk, A, depth=30.0, circuits=cc)
    z, s = P.block_integrals([4])
    m = P.lbl == 4
    w = 2. * np.pi * F
    a = P.terms()[5].real[m]
    Abar = P.A[m].mean(axis=1)
    want = (a * 1e6 * (-1j * w * 35.0 * Abar - 35.0 * cc[2][1])).sum()
    assert abs(z[7] - want) <= 1e-12 * s[7]


def test_double_frequency_types_against_a_time_average():
    """j(t) x b(t) of every element at 8 phases, fitted by its constant and its
    e^{2 i w t} part: types 11 / 12 / 15 and 13 / 14 / 16 (planar)"""
    kw = synth.harmonic(8)
    kk, A, cc = _solved(kw)
    depth = 30.0
    P = R.MagAcPost(kk, A, depth=depth, circuits=cc)
    P.terms()
    fld = P._fields
    sel = np.ones(len(kk["labels"]), bool)
    z, s = P.block_integrals(sel)
    th = 2. * np.pi * np.arange(8) / 8.
    vol = fld["a"] * P.depth
    fx = np.zeros(8)
    fy = np.zeros(8)
    tq = np.zeros(8)
    sa = np.zeros(3)
    for k, t in enumerate(th):
        j = (fld["J"] * np.exp(1j * t)).real
        b1 = (fld["B1"] * np.exp(1j * t)).real
        b2 = (fld["B2"] * np.exp(1j * t)).real
        fx[k] = (-(j * b2) * vol).sum()
        fy[k] = ((j * b1) * vol).sum()
        tq[k] = ((fld["cx"] * (j * b1) + fld["cy"] * (j * b2)) * vol).sum()
        sa = np.maximum(sa, [np.abs(j * b2 * vol).sum(), np.abs(j * b1 * vol).sum(),
                             np.abs((fld["cx"] * (j * b1) + fld["cy"] * (j * b2)) * vol).sum()])
    for q, (f, t0, t2) in enumerate(((fx, 11, 13), (fy, 12, 14), (tq, 15, 16))):
        c0 = f.mean()
        c2 = 2. * (f * np.exp(-2j * th)).mean()        # f = c0 + Re(c2 e^{2 i theta})
        assert abs(z[t0] - c0) <= 1e-12 * sa[q], (t0, z[t0], c0)
        assert abs(z[t2] - c2) <= 1e-12 * sa[q], (t2, z[t2], c2)
