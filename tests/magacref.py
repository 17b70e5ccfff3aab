"""A restatement of the time-harmonic part of the reference's fpproc that needs
no mask, in complex double with numpy, all elements at once:

    GetElementB      fpproc.cpp:2970-3082 (complex A)
    GetJA            fpproc.cpp:3495-3578 (the eddy term, complex Case / J / dVolts)
    PlnInt, AxiInt   fpproc.cpp:3580-3612 (complex arguments)
    BlockIntegral    fpproc.cpp:3642-3963 at Frequency != 0
    mu_fdx, mu_fdy   OpenDocument, fpproc.cpp:1703-1758
    FPProc::GetMu    fpproc.cpp:5308-5320
    GetMu(CComplex), GetH(CComplex), DoEnergy(CComplex, CComplex)
                     CMaterialProp.cpp:722-772, 493-519, 680-696

The problem is the keyword dictionary of kernels.Harmonic2DProblem (coordinates
in cm, divided back to the problem's length units here), A the .ans value (A,
or the flux 2 pi r A when axisymmetric), circuits the solve's circuit results
(ccase, J, dV: Harmonic2DProblem.circuits()).  The geometry is
tests/magpostref.py's; the types that read no field (5, 10, 24, 25) are its
values, bit for bit.  LamType 0 blocks (the reference's harmonic solver
rejects 1 and 2; a LamType > 2 label is refused by the device).

Where a label's conductivity is 0 the reference's sig = 1e6 / Re(1 / o) of
type 4 is 0 / 0; no loss is added there, as on the device.
"""
import numpy as np

import magpostref as M

PI = M.PI
MUO = M.MUO

# The two discrete identities of identity_problem, relative gaps of the
# oracle's solution at Precision 1e-12, measured by tests/test_magac_cpu.py at
# 10 x 10 and 20 x 20 cells; the asserted bounds are 10 x the larger of each
IDENTITY_TYPE0_MEASURED = (1.75e-15, 2.26e-15)
IDENTITY_TYPE0_BOUND = 10 * max(IDENTITY_TYPE0_MEASURED)
POWER_BALANCE_MEASURED = (4.55e-14, 2.71e-13)    # (the solve's residual at 1e-12 enters Im(type 0) directly)
POWER_BALANCE_BOUND = 10 * max(POWER_BALANCE_MEASURED)

# inttype -> complex sums answered (6 = 3 + 4, 17 = 2)
TYPES = (0, 1, 2, 3, 4, 5, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 24)


def cdiv(x, z):
    """x / z as CComplex forms it (femmcomplex.cpp:456-474), elementwise"""
    x = np.asarray(x, complex)
    z = np.asarray(z, complex) + np.zeros(np.shape(x), complex)
    big = np.abs(z.real) > np.abs(z.imag)
    with np.errstate(all="ignore"):
        c1 = z.imag / z.real
        yr1 = 1. / (z.real * (1. + c1 * c1))
        yi1 = (-c1) * yr1
        c2 = z.real / z.imag
        yi2 = (-1.) / (z.imag * (1. + c2 * c2))
        yr2 = (-c2) * yi2
    y = np.where(big, yr1 + 1j * yi1, yr2 + 1j * yi2)
    return x * y


def mu_fd(mu, theta, Lam_d, Cduct, LamFill, w):
    """mu_fdx or mu_fdy of OpenDocument, fpproc.cpp:1716-1753"""
    m = mu * np.exp(-1j * theta * PI / 180.)
    if Lam_d != 0:
        if Cduct != 0:
            halflag = np.exp(-1j * theta * PI / 360.)
            ds = np.sqrt(2. / (0.4 * PI * w * Cduct * mu))
            K = halflag * (1 + 1j) * Lam_d * 0.001 / (2. * ds)
            m = (m * np.tanh(K) / K) * LamFill + (1. - LamFill)
        else:
            m = m * LamFill + (1. - LamFill)
    return complex(m)


def element_b(axi, lc, X, Y, A):
    """GetElementB on (n, 3) arrays; A real or complex"""
    b = [Y[:, 1] - Y[:, 2], Y[:, 2] - Y[:, 0], Y[:, 0] - Y[:, 1]]
    c = [X[:, 2] - X[:, 1], X[:, 0] - X[:, 2], X[:, 1] - X[:, 0]]
    da = (b[0] * c[1] - b[1] * c[0])
    if not axi:
        B1 = 0.
        B2 = 0.
        for i in range(3):
            B1 = B1 + A[:, i] * c[i] / (da * lc)
            B2 = B2 - A[:, i] * b[i] / (da * lc)
        return B1, B2
    R = [X[:, 0], X[:, 1], X[:, 2]]
    r = 0.
    for i in range(3):
        r = r + R[i] / 3.
    v = [None] * 6
    v[0], v[2], v[4] = A[:, 0], A[:, 1], A[:, 2]

    def mid(i, j, vi, vj):
        on = (R[i] < 1.e-06) & (R[j] < 1.e-06)
        with np.errstate(all="ignore"):
            off = (R[j] * (3. * vi + vj) + R[i] * (vi + 3. * vj)) / (4. * (R[i] + R[j]))
        return np.where(on, (vi + vj) / 2., off)
    v[1] = mid(0, 1, v[0], v[2])
    v[3] = mid(1, 2, v[2], v[4])
    v[5] = mid(2, 0, v[4], v[0])
    dp = (-v[0] + v[2] + 4. * v[3] - 4. * v[5]) / 3.
    dq = (-v[0] - 4. * v[1] + 4. * v[3] + v[4]) / 3.
    da = da * (2. * PI * r * lc * lc)
    return -(c[1] * dp + c[2] * dq) / da, (b[1] * dp + b[2] * dq) / da


def pln_int(a, u, v):
    z = [2. * u[0] + u[1] + u[2], u[0] + 2. * u[1] + u[2], u[0] + u[1] + 2. * u[2]]
    x = 0.
    for i in range(3):
        x = x + v[i] * z[i]
    return a * x / 12.


def axi_int(a, u, v, r):
    Mx = [[None] * 3 for _ in range(3)]
    Mx[0][0] = 6. * r[0] + 2. * r[1] + 2. * r[2]
    Mx[0][1] = 2. * r[0] + 2. * r[1] + 1. * r[2]
    Mx[0][2] = 2. * r[0] + 1. * r[1] + 2. * r[2]
    Mx[1][1] = 2. * r[0] + 6. * r[1] + 2. * r[2]
    Mx[1][2] = 1. * r[0] + 2. * r[1] + 2. * r[2]
    Mx[2][2] = 2. * r[0] + 2. * r[1] + 6. * r[2]
    Mx[1][0], Mx[2][0], Mx[2][1] = Mx[0][1], Mx[0][2], Mx[1][2]
    z = [Mx[i][0] * u[0] + Mx[i][1] * u[1] + Mx[i][2] * u[2] for i in range(3)]
    x = 0.
    for i in range(3):
        x = x + v[i] * z[i]
    return PI * a * x / 30.


def identity_problem(n, theta=0.0, precision=1e-12, L=10.0, frequency=60.0):
    """The problem of the type-0 identity and of the power balance: linear,
    planar, n x n cells; A = 0 on three sides, the side x = L natural; a steel
    core of real mu_r 50 (hysteresis angle theta), a source coil with a complex
    J in a non-conducting label (2), a solid conducting plate without a source
    (3).  Labels: 0 air, 1 steel, 2 coil, 3 plate."""
    kw = M.square_problem(n, False, precision, L)
    kw["blocks"] = [dict(mu_x=1.0, mu_y=1.0), dict(mu_x=50.0, mu_y=50.0, Theta_hx=theta, Theta_hy=theta),
                    dict(mu_x=1.0, mu_y=1.0, J_re=1.5, J_im=0.4), dict(mu_x=1.0, mu_y=1.0, Cduct=35.0)]
    x, p = np.asarray(kw["x"]), np.asarray(kw["p"])
    e = np.array(kw["e"], np.int32).reshape(-1, 3).copy()
    for j in range(3):
        a, b = p[:, j], p[:, (j + 1) % 3]
        e[(np.abs(x[a] - L) < 1e-9 * L) & (np.abs(x[b] - L) < 1e-9 * L), j] = -1
    kw["e"] = e
    kw["frequency"] = frequency
    return kw


def uniform_planar(ne_side=5, B0=0.8, phi=0.7, seed=3, **block):
    """A scrambled planar mesh (mm) of one block carrying the uniform complex
    field A = B0 e^{i phi} x (Wb/m with x in m): B = (0, -B0 e^{i phi})."""
    from xfemm_amd import synth
    rng = np.random.default_rng(seed)
    x, y, p = synth.square_mesh(ne_side, 10.0)
    m = ne_side + 1
    inner = ((np.arange(len(x)) % m) % ne_side != 0) & ((np.arange(len(x)) // m) % ne_side != 0)
    x = x + inner * rng.uniform(-0.3, 0.3, len(x))
    y = y + inner * rng.uniform(-0.3, 0.3, len(x))
    perm = rng.permutation(len(p))
    p = np.asarray(p)[perm]
    blk = dict(mu_x=1.0, mu_y=1.0)
    blk.update(block)
    kw = dict(x=x * 0.1, y=y * 0.1, p=p.astype(np.int32), lbl=np.zeros(len(p), np.int32),
              e=-np.ones((len(p), 3), np.int32), marker=None, pbc=None, blocks=[blk], labels=[dict(block=0)],
              lines=[], points=[], circuits=[], precision=1e-8, length_units=1, coords=0, relax=1.0, problem_type=0,
              frequency=60.0)
    A = B0 * np.exp(1j * phi) * (x * 1e-3)
    return kw, A


def uniform_axi(ne_side=5, B0=0.8, phi=0.7, seed=4, **block):
    """The same with the axisymmetric flux pi r^2 B0 e^{i phi} (r in m):
    B = (0, B0 e^{i phi}); the mesh touches the axis."""
    kw, _ = uniform_planar(ne_side, B0, phi, seed, **block)
    kw["problem_type"] = 1
    r = np.asarray(kw["x"]) / 0.1 * 1e-3
    return kw, PI * r * r * B0 * np.exp(1j * phi)


class MagAcPost:
    """One opened harmonic solution."""

    def __init__(self, kw, A, depth=-1, circuits=None):
        self.kw = kw
        lu = kw.get("length_units", 0)
        self.lc = M.LENGTH_CONV[lu]
        self.axi = bool(kw.get("problem_type", 0))
        self.f = float(kw["frequency"])
        X, Y = M.user_xy(kw)
        self.p = np.asarray(kw["p"], np.int64).reshape(-1, 3)
        self.lbl = np.asarray(kw["lbl"], np.int64)
        self.X, self.Y = X[self.p], Y[self.p]
        self.A = np.asarray(A, complex)[self.p]
        self.labels = kw["labels"]
        self.blocks = kw["blocks"]
        self.depth = 1. if depth == -1 else depth * self.lc
        self.ext = (kw.get("ext_ro", 0.), kw.get("ext_ri", 0.), kw.get("ext_zo", 0.))
        cc, J, dV = circuits if circuits is not None else ((), (), ())
        # the label's Case / J / dVolts as the .ans label lines carry them
        # (harmonic2d.cpp:968-992: Case 2 is written as Case 0 with the solved gradient)
        nl = len(self.labels)
        self.lab_case = np.full(nl, -1)
        self.lab_J = np.zeros(nl, complex)
        self.lab_dV = np.zeros(nl, complex)
        for k, lb in enumerate(self.labels):
            q = lb.get("in_circuit", -1)
            if q < 0:
                continue
            if cc[q] == 1:
                self.lab_case[k], self.lab_J[k] = 1, J[q]
            else:
                self.lab_case[k], self.lab_dV[k] = 0, dV[q]
        # the static restatement of the same mesh: geometry-only types
        skw = dict(kw)
        skw["blocks"] = [dict(mu_x=1.0, mu_y=1.0) for _ in kw["blocks"]]
        skw["labels"] = [dict(block=lb["block"], is_external=lb.get("is_external", 0)) for lb in kw["labels"]]
        self.static = M.MagPost(skw, np.zeros(len(X)), depth=depth)

    def element_b_all(self):
        B1, B2 = element_b(self.axi, self.lc, self.X, self.Y, self.A)
        return np.stack([B1, B2], axis=1)

    def _per_element(self, name, default=0.0, of="blocks"):
        if of == "blocks":
            tab = np.array([b.get(name, default) for b in self.blocks])
            return tab[np.array([lb["block"] for lb in self.labels])][self.lbl]
        return np.array([lb.get(name, default) for lb in self.labels])[self.lbl]

    def block_mu(self, B1, B2):
        """CMMaterialProp::GetMu(CComplex ...) per element: (mu1, mu2), relative"""
        w = 2. * PI * self.f
        ne = len(self.p)
        mu1 = np.zeros(ne, complex)
        mu2 = np.zeros(ne, complex)
        blk = np.array([lb["block"] for lb in self.labels])[self.lbl]
        for k, b in enumerate(self.blocks):
            m = blk == k
            if not m.any():
                continue
            if len(b.get("B", ())) == 0 or b.get("LamType", 0) != 0:
                if b.get("LamType", 0) == 0:
                    args = (b.get("Lam_d", 0.0), b.get("Cduct", 0.0), b.get("LamFill", 1.0), w)
                    mu1[m] = mu_fd(b.get("mu_x", 1.0), b.get("Theta_hx", 0.0), *args)
                    mu2[m] = mu_fd(b.get("mu_y", 1.0), b.get("Theta_hy", 0.0), *args)
                else:
                    mu1[m] = mu2[m] = 1.0
                continue
            Bk = np.asarray(b["B"], float)
            Hk = np.asarray(b["H"], complex)
            Sk = np.asarray(b["slope"], complex)
            biron = np.sqrt((B1[m] * np.conj(B1[m]) + B2[m] * np.conj(B2[m])).real)
            mu = np.zeros(len(biron), complex)
            for q, bb in enumerate(biron):
                if abs(bb) < 1.e-08:
                    mu[q] = 1. / Sk[0]
                else:
                    mu[q] = bb / self.get_h(Bk, Hk, Sk, bb)
            mu1[m] = mu / MUO
            mu2[m] = mu / MUO
        return mu1, mu2

    @staticmethod
    def get_h(B, H, S, x):
        """CMMaterialProp::GetH(CComplex), CMaterialProp.cpp:493-519, real x >= 0"""
        n = len(B)
        b = abs(x)
        if n == 0 or b == 0:
            return 0.
        p = x / b
        if b > B[n - 1]:
            return p * (H[n - 1] + S[n - 1] * (b - B[n - 1]))
        for i in range(n - 1):
            if b >= B[i] and b <= B[i + 1]:
                l = B[i + 1] - B[i]
                z = (b - B[i]) / l
                z2 = z * z
                h = ((1. - 3. * z2 + 2. * z2 * z) * H[i] + z * (1. - 2. * z + z2) * l * S[i] +
                     z2 * (3. - 2. * z) * H[i + 1] + z2 * (z - 1.) * l * S[i + 1])
                return p * h
        return 0.

    def get_ja(self):
        """GetJA of every element: (Javg, J[3], A[3]) in A/m^2 and Wb/m"""
        lc, axi = self.lc, self.axi
        X = self.X
        A = [None] * 3
        for i in range(3):
            if not axi:
                A[i] = self.A[:, i]
            else:
                rn = X[:, i] * lc
                with np.errstate(all="ignore"):
                    A[i] = np.where(np.abs(rn / lc) < 1.e-06, 0., self.A[:, i] / (2. * PI * rn))
        r = 0.
        if axi:
            cx = 0.
            for j in range(3):
                cx = cx + X[:, j] / 3.
            r = cx * lc
        Jb = self._per_element("J_re") + 1j * self._per_element("J_im")
        J = [Jb.copy() for _ in range(3)]
        Javg = Jb.copy()
        c = self._per_element("Cduct").astype(float)
        lam = (self._per_element("Lam_d") != 0) & (self._per_element("LamType", 0) == 0)
        c = np.where(lam, 0., c)
        c = np.where(self._per_element("is_wound", 0, "labels") != 0, 0., c)
        for i in range(3):
            t = 1j * self.f * 2. * PI * c * A[i]
            J[i] = J[i] - t
            Javg = Javg - t / 3.
        case = self.lab_case[self.lbl]
        dV = self.lab_dV[self.lbl]
        Jc = self.lab_J[self.lbl]
        v0 = case == 0
        if not axi:
            for i in range(3):
                J[i] = np.where(v0, J[i] - c * dV, J[i])
            Javg = np.where(v0, Javg - c * dV, Javg)
        else:
            with np.errstate(all="ignore"):
                for i in range(3):
                    rn = X[:, i]
                    d = np.where(np.abs(rn / lc) < 1.e-06, c * dV / r, c * dV / (rn * lc))
                    J[i] = np.where(v0, J[i] - d, J[i])
                Javg = np.where(v0, Javg - c * dV / r, Javg)
        v1 = case > 0
        for i in range(3):
            J[i] = np.where(v1, J[i] + Jc, J[i])
        Javg = np.where(v1, Javg + Jc, Javg)
        return Javg * 1.e06, [j * 1.e06 for j in J], A

    def terms(self):
        """{inttype: (n_elems,) complex}: every element's term of the types in
        TYPES, and "cx", "cy" of type 25"""
        if hasattr(self, "_terms"):
            return self._terms
        lc, axi, Depth, f = self.lc, self.axi, self.depth, self.f
        X, Y = self.X, self.Y
        B1, B2 = element_b(axi, lc, X, Y, self.A)
        cx = cy = 0.
        for j in range(3):
            cx = cx + X[:, j] / 3.
            cy = cy + Y[:, j] / 3.
        J, Jn, A = self.get_ja()
        b0, b1 = Y[:, 1] - Y[:, 2], Y[:, 2] - Y[:, 0]
        c0, c1 = X[:, 2] - X[:, 1], X[:, 0] - X[:, 2]
        a = ((b0 * c1 - b1 * c0) / 2.) * np.power(lc, 2.)
        r = [np.zeros(len(a))] * 3
        R = 0.
        if axi:
            r = [X[:, k] * lc for k in range(3)]
            R = (r[0] + r[1] + r[2]) / 3.
        av = a * (2. * PI * R) if axi else a * Depth
        U = [1., 1., 1.]
        aecf = np.ones(len(a))
        if axi:
            ro, ri, zo = self.ext
            ext = self._per_element("is_external", 0, "labels") != 0
            if ext.any():
                q = np.abs(cx + 1j * (cy - zo))
                aecf = np.where(ext, (q * q * ri) / (ro * ro * ro), 1.)
        o = {}
        V = [np.conj(j) for j in Jn]
        o[0] = axi_int(a, A, V, r) if axi else pln_int(a, A, V) * Depth
        if axi:
            o[1] = axi_int(a, U, A, r)
        else:
            y = 0.
            for k in range(3):
                y = y + a * Depth * A[k] / 3.
            o[1] = y
        mu1, mu2 = self.block_mu(B1, B2)
        h1 = cdiv(B1, mu1 * MUO)
        h2 = cdiv(B2, mu2 * MUO)
        o[2] = av * ((h1 * np.conj(B1) + h2 * np.conj(B2)).real / 4.) * aecf
        H1 = cdiv(B1, (mu1 / aecf) * MUO)
        H2 = cdiv(B2, (mu2 / aecf) * MUO)
        o[3] = av * PI * f * (H1 * np.conj(B1) + H2 * np.conj(B2)).imag
        cd = self._per_element("Cduct").astype(float)
        lam = (self._per_element("Lam_d") != 0) & (self._per_element("LamType", 0) == 0)
        with np.errstate(all="ignore"):
            sig = np.where((cd != 0) & ~lam, 1.e06 / (1. / cd), 0.)
            if not axi:
                y = pln_int(a, Jn, [np.conj(j) / sig for j in Jn]) * Depth
            else:
                y = 2. * PI * R * a * J * np.conj(J) / sig
            o[4] = np.where(sig != 0, y / 2., 0.)
        o[5] = a
        o[7] = a * J
        o[8] = av * B1
        o[9] = av * B2
        o[10] = av
        o[11] = a * (np.zeros(len(a)) if axi else -(B2.real * J.real + B2.imag * J.imag) * Depth * 0.5)
        V = [(B1 * np.conj(j)).real for j in Jn]
        o[12] = (axi_int(-a, U, V, r) if axi else pln_int(a, U, V) * Depth) * 0.5
        if axi:
            o[13] = np.zeros(len(a), complex)
        else:
            o[13] = 0.5 * (a * (-(B2.real * J.real - B2.imag * J.imag) - 1j * (B2.real * J.imag + B2.imag * J.real)) * Depth)
        y = (B1.real * J.real - B1.imag * J.imag) + 1j * (B1.real * J.imag + B1.imag * J.real)
        y = (-y * 2. * PI * R) if axi else y * Depth
        o[14] = (a * y) / 2.
        if axi:
            o[15] = np.zeros(len(a))
            o[16] = np.zeros(len(a), complex)
        else:
            ccx, ccy = cx * lc, cy * lc
            o[15] = a * ((ccy * (B2.real * J.real + B2.imag * J.imag) + ccx * (B1.real * J.real + B1.imag * J.imag)) * 0.5) * Depth
            y = (ccx * ((B1.real * J.real - B1.imag * J.imag) + 1j * (B1.real * J.imag + B1.imag * J.real)) +
                 ccy * ((B2.real * J.real - B2.imag * J.imag) + 1j * (B2.real * J.imag + B2.imag * J.real)))
            o[16] = 0.5 * (a * y * Depth)
        # The types that keep one part of a complex product (2, 3, 11, 12, 15):
        # the part can cancel inside an element (no loss where mu is real, no
        # steady force where J lags B by a quarter period), so their rounding
        # scale is taken from the products' magnitudes, not from the part kept
        aB1, aB2, aJ = np.abs(B1), np.abs(B2), np.abs(J)
        sc = {}
        sc[2] = av * (np.abs(h1) * aB1 + np.abs(h2) * aB2) / 4. * aecf
        sc[3] = av * PI * f * (np.abs(H1) * aB1 + np.abs(H2) * aB2)
        sc[11] = np.zeros(len(a)) if axi else np.abs(a) * Depth * 0.5 * aB2 * aJ
        Vm = [aB1 * np.abs(j) for j in Jn]
        sc[12] = np.abs(axi_int(a, U, Vm, r) if axi else pln_int(a, U, Vm) * Depth) * 0.5
        sc[15] = (np.zeros(len(a)) if axi else
                  np.abs(a) * Depth * 0.5 * (np.abs(cy * lc) * aB2 * aJ + np.abs(cx * lc) * aB1 * aJ))
        self._scales = sc
        self._terms = {k: np.asarray(v, complex) for k, v in o.items()}
        self._fields = dict(B1=B1, B2=B2, J=J, a=a, cx=cx * lc, cy=cy * lc)
        return self._terms

    def selected(self, selected):
        s = np.asarray(selected)
        m = np.zeros(len(self.labels), bool)
        if s.dtype == np.bool_:
            m[:len(s)] = s
        elif s.size:
            m[s.astype(np.int64)] = True
        return m

    def block_integrals(self, selected):
        """(z, scale) indexed by inttype: the sums over the selected labels'
        elements and the sums of the absolute terms"""
        m = self.selected(selected)[self.lbl]
        T = self.terms()
        z = np.zeros(26, complex)
        scale = np.zeros(26)
        for t in TYPES:
            if t in (5, 10, 24):
                continue
            z[t] = T[t][m].sum()
            scale[t] = (self._scales[t][m] if t in self._scales else np.abs(T[t][m])).sum()
        zs, ss = self.static.block_integrals(selected)
        for t in (5, 10, 24, 25):
            z[t], scale[t] = zs[t], ss[t]
        z[6], scale[6] = z[3] + z[4], scale[3] + scale[4]
        z[17], scale[17] = z[2], scale[2]
        return z, scale
