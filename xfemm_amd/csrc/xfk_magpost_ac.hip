// Post-processing of a time-harmonic magnetics problem on the device: the
// complex element flux density and the block integrals of the reference's
// fpproc at Frequency != 0, for MI355X (gfx950).  Planar and axisymmetric.
// The counterpart of xfk_magpost.hip, which stays Frequency 0 only.
//
//   element B         FPProc::GetElementB (fpproc.cpp:2970-3082) on complex A
//   J and A           FPProc::GetJA (3495-3578) with the eddy term, PlnInt /
//                     AxiInt (3580-3612) on complex arguments
//   permeability      OpenDocument's mu_fdx, mu_fdy (1703-1758), FPProc::GetMu
//                     (5308-5320), CMMaterialProp::GetMu(CComplex ...)
//                     (CMaterialProp.cpp:722-772), GetH(CComplex) (493-519),
//                     DoEnergy(CComplex, CComplex) (680-696)
//   block integrals   FPProc::BlockIntegral (3642-3963) types 0 1 2 3 4 5 7 8 9
//                     10 11 12 13 14 15 16 17 24 25; 6 = 3 + 4 on the host
//
// A is the value the .ans carries, interleaved (re, im): V c, times 2 pi r on an
// axisymmetric problem (harmonic2d.cpp:783, harmonicaxi.cpp:790).  CComplex's
// operators are restated one by one (femmcomplex.cpp), in double, without
// contraction into fused multiply-adds.
//
// One pass over the elements gives every type: a thread per element evaluates
// B, J, A and the 28 real sums of all types (zero where the element's label is
// not selected); block_sums and k_pot_sum add them in a fixed order.  No
// atomics: two calls give the same bits.
#include "xfk_potential.h"

#pragma clang fp contract(off)

#include "xfk_magpost.h"
#include "xfk_post.h"

#include <cmath>

namespace xfk {

// CComplex (femmcomplex.cpp), the operators the restated functions use
struct cd {
    double re, im;
};
__host__ __device__ __forceinline__ cd cd_of(double re, double im) { return cd{re, im}; }
__host__ __device__ __forceinline__ cd cd_of(double2 z) { return cd{z.x, z.y}; }
__host__ __device__ __forceinline__ cd operator+(cd a, cd b) { return cd{a.re + b.re, a.im + b.im}; }
__host__ __device__ __forceinline__ cd operator-(cd a, cd b) { return cd{a.re - b.re, a.im - b.im}; }
__host__ __device__ __forceinline__ cd operator-(cd a) { return cd{-a.re, -a.im}; }
__host__ __device__ __forceinline__ cd operator*(cd a, cd b)   // :355-358
{
    return cd{a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re};
}
__host__ __device__ __forceinline__ cd operator*(double x, cd y) { return cd{x * y.re, x * y.im}; }   // :350-353
__host__ __device__ __forceinline__ cd operator*(cd y, double x) { return cd{y.re * x, y.im * x}; }   // :323-326
__host__ __device__ __forceinline__ cd operator/(cd y, double x) { return cd{y.re / x, y.im / x}; }   // :388-391
__host__ __device__ __forceinline__ cd cd_conj(cd a) { return cd{a.re, -a.im}; }
// 1 / z as every quotient forms it (:362-380, 433-474)
__host__ __device__ __forceinline__ cd cd_inv(cd z)
{
    cd y;
    if (fabs(z.re) > fabs(z.im)) {
        const double c = z.im / z.re;
        y.re = 1. / (z.re * (1. + c * c));
        y.im = (-c) * y.re;
    } else {
        const double c = z.re / z.im;
        y.im = (-1.) / (z.im * (1. + c * c));
        y.re = (-c) * y.im;
    }
    return y;
}
__host__ __device__ __forceinline__ cd operator/(cd x, cd z) { return x * cd_inv(z); }
__host__ __device__ __forceinline__ cd operator/(double x, cd z)
{
    cd y = cd_inv(z);
    y.re *= x;
    y.im *= x;
    return y;
}
// abs (:749-757)
__host__ __device__ __forceinline__ double cd_abs(cd x)
{
    if ((x.re == 0) && (x.im == 0)) return 0.;
    if (fabs(x.re) > fabs(x.im)) return fabs(x.re) * sqrt(1. + (x.im / x.re) * (x.im / x.re));
    return fabs(x.im) * sqrt(1. + (x.re / x.im) * (x.re / x.im));
}
// sqrt (:636-673)
__host__ __device__ __forceinline__ cd cd_sqrt(cd x)
{
    double w, z;
    if ((x.re == 0) && (x.im == 0)) w = 0;
    else if (fabs(x.re) > fabs(x.im)) {
        z = x.im / x.re;
        w = sqrt(fabs(x.re)) * sqrt((1. + sqrt(1. + z * z)) / 2.);
    } else {
        z = x.re / x.im;
        w = sqrt(fabs(x.im)) * sqrt((fabs(z) + sqrt(1. + z * z)) / 2.);
    }
    if (w == 0) return cd{0, 0};
    if (x.re >= 0) return cd{w, x.im / (2. * w)};
    if (x.im >= 0) return cd{fabs(x.im) / (2. * w), w};
    return cd{fabs(x.im) / (2. * w), -w};
}
// exp (:622-634), tanh (:675-687): the host's block table
static inline cd cd_exp(cd x)
{
    const double e = std::exp(x.re);
    return cd{std::cos(x.im) * e, std::sin(x.im) * e};
}
static inline cd cd_tanh(cd x)
{
    const cd one = {1., 0.};
    if (x.re > 0) {
        const cd e = cd_exp(-2. * x);
        return (one - e) / (one + e);
    }
    const cd e = cd_exp(2. * x);
    return (e - one) / (e + one);
}

// the label table's complex twin: Case / J / dVolts of the label's circuit
struct MagAcLabel {
    double2 J, dV;          // blocklist[lbl].J (Case 1), dVolts (Case 0)
    int blk;
    int ccase;              // blocklist[lbl].Case; -1: InCircuit < 0
    int wound;              // FillFactor > 0: no bulk conductivity
    int external;
    int sel;
    int pad;
};

struct MagAcArgs {
    const MagAcLabel *labels;
    const MagAcBlock *blocks;
    const double *bhB;             // the complex curves of GetSlopes(omega)
    const double2 *bhH, *bhS;
    double freq;                   // Hz
};

// the sums one pass makes, in this order
enum {
    AS_AJ_R, AS_AJ_I, AS_A_R, AS_A_I, AS_ENERGY, AS_HYST, AS_RES_R, AS_RES_I, AS_AREA, AS_CUR_R, AS_CUR_I, AS_B1_R,
    AS_B1_I, AS_B2_R, AS_B2_I, AS_VOLUME, AS_FX, AS_FY, AS_FX2_R, AS_FX2_I, AS_FY2_R, AS_FY2_I, AS_TORQUE, AS_T2_R,
    AS_T2_I, AS_INERTIA, AS_CX, AS_CY, kMagAcSums
};

struct MagAcElem {
    double X[3], Y[3];
    cd A[3];
    int lbl;
};

__device__ __forceinline__ void mag_ac_load(const MagArgs &M, int e, MagAcElem &E)
{
    const double2 *A = reinterpret_cast<const double2 *>(M.A);
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const int n = M.p[3 * e + j];
        E.X[j] = M.x[n];
        E.Y[j] = M.y[n];
        E.A[j] = cd_of(A[n]);
    }
    E.lbl = M.lbl[e];
}

// GetElementB on complex A: the real and the imaginary part in turn (mag_element_b)
template <bool AXI>
__device__ __forceinline__ void mag_ac_b(double lc, const MagAcElem &E, cd &B1, cd &B2)
{
    const double Ar[3] = {E.A[0].re, E.A[1].re, E.A[2].re}, Ai[3] = {E.A[0].im, E.A[1].im, E.A[2].im};
    mag_element_b<AXI>(lc, E.X, E.Y, Ar, B1.re, B2.re);
    mag_element_b<AXI>(lc, E.X, E.Y, Ai, B1.im, B2.im);
}

// A as xfk_get_solution_complex gives it (harmonic2d.cpp:783, harmonicaxi.cpp:790)
static __global__ void k_mag_ac_a(int N, int axi, const double2 *__restrict__ V, const double *__restrict__ xcm,
                                  double2 *__restrict__ A)
{
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= N) return;
    double2 a = V[i];
    if (axi) {
        a.x = a.x * kC * 2. * kPI * xcm[i] * 0.01;
        a.y = a.y * kC * 2. * kPI * xcm[i] * 0.01;
    } else {
        a.x *= kC;
        a.y *= kC;
    }
    A[i] = a;
}

template <bool AXI>
__global__ void __launch_bounds__(kBlock) k_mag_ac_element_b(int NE, MagArgs M, double2 *__restrict__ B1,
                                                             double2 *__restrict__ B2)
{
    const int e = blockIdx.x * kBlock + threadIdx.x;
    if (e >= NE) return;
    MagAcElem E;
    mag_ac_load(M, e, E);
    cd b1, b2;
    mag_ac_b<AXI>(M.lc, E, b1, b2);
    B1[e] = make_double2(b1.re, b1.im);
    B2[e] = make_double2(b2.re, b2.im);
}

// CMMaterialProp::GetH(CComplex) (CMaterialProp.cpp:493-519) over the block's complex curve
__device__ __forceinline__ cd mag_ac_get_h(const MagAcArgs &C, const MagAcBlock &bp, cd x)
{
    const double b = cd_abs(x);
    const int n = bp.bh_n;
    if ((n == 0) || (b == 0)) return cd{0, 0};
    const double *B = C.bhB + bp.bh_off;
    const double2 *H = C.bhH + bp.bh_off, *S = C.bhS + bp.bh_off;
    const cd p = x / b;
    if (b > B[n - 1]) return p * (cd_of(H[n - 1]) + cd_of(S[n - 1]) * (b - B[n - 1]));
    for (int i = 0; i < n - 1; ++i)
        if ((b >= B[i]) && (b <= B[i + 1])) {
            const double l = B[i + 1] - B[i];
            const double z = (b - B[i]) / l;
            const double z2 = z * z;
            const cd h = (1. - 3. * z2 + 2. * z2 * z) * cd_of(H[i]) + z * (1. - 2. * z + z2) * l * cd_of(S[i]) +
                         z2 * (3. - 2. * z) * cd_of(H[i + 1]) + z2 * (z - 1.) * l * cd_of(S[i + 1]);
            return p * h;
        }
    return cd{0, 0};
}

// CMMaterialProp::GetMu(CComplex ...) (CMaterialProp.cpp:722-772), LamType 0
// (the reference's harmonic solver rejects 1 and 2; a LamType > 2 label is
// refused on the host)
__device__ __forceinline__ void mag_ac_get_mu(const MagAcArgs &C, const MagAcBlock &bp, cd b1, cd b2, cd &mu1,
                                              cd &mu2)
{
    if (bp.bh_n == 0) {
        mu1 = cd_of(bp.mu_fdx);
        mu2 = cd_of(bp.mu_fdy);
        return;
    }
    const cd biron = cd_sqrt(b1 * cd_conj(b1) + b2 * cd_conj(b2));
    if (cd_abs(biron) < 1.e-08) mu1 = 1. / cd_of(C.bhS[bp.bh_off]);   // catch degenerate case
    else mu1 = biron / mag_ac_get_h(C, bp, biron);
    mu2 = mu1;
    mu1 = mu1 / kMUO;
    mu2 = mu2 / kMUO;
}

// PlnInt / AxiInt (fpproc.cpp:3580-3612) on complex arguments
__device__ __forceinline__ cd mag_ac_pln_int(double a, const cd (&u)[3], const cd (&v)[3])
{
    cd z[3], x = {0, 0};
    z[0] = 2. * u[0] + u[1] + u[2];
    z[1] = u[0] + 2. * u[1] + u[2];
    z[2] = u[0] + u[1] + 2. * u[2];
#pragma unroll
    for (int i = 0; i < 3; ++i) x = x + v[i] * z[i];
    return a * x / 12.;
}

// (M[][] is real: its products with u are the reference's complex ones with a zero imaginary factor)
__device__ __forceinline__ cd mag_ac_axi_int(double a, const cd (&u)[3], const cd (&v)[3], const double (&r)[3])
{
    double Mx[3][3];
    cd z[3], x = {0, 0};
    Mx[0][0] = 6. * r[0] + 2. * r[1] + 2. * r[2];
    Mx[0][1] = 2. * r[0] + 2. * r[1] + 1. * r[2];
    Mx[0][2] = 2. * r[0] + 1. * r[1] + 2. * r[2];
    Mx[1][1] = 2. * r[0] + 6. * r[1] + 2. * r[2];
    Mx[1][2] = 1. * r[0] + 2. * r[1] + 2. * r[2];
    Mx[2][2] = 2. * r[0] + 2. * r[1] + 6. * r[2];
    Mx[1][0] = Mx[0][1];
    Mx[2][0] = Mx[0][2];
    Mx[2][1] = Mx[1][2];
#pragma unroll
    for (int i = 0; i < 3; ++i) z[i] = Mx[i][0] * u[0] + Mx[i][1] * u[1] + Mx[i][2] * u[2];
#pragma unroll
    for (int i = 0; i < 3; ++i) x = x + v[i] * z[i];
    return kPI * a * x / 30.;
}

// The integrands of one element of a selected label: one case of
// FPProc::BlockIntegral's switch per sum, at Frequency != 0
template <bool AXI>
__device__ __forceinline__ void mag_ac_integrands(const MagArgs &M, const MagAcArgs &C, const MagAcElem &E,
                                                  const MagAcLabel &lab, double (&v)[kMagAcSums])
{
    const MagAcBlock bp = C.blocks[lab.blk];
    const double lc = M.lc, Depth = M.depth, Frequency = C.freq;
    cd B1, B2;
    mag_ac_b<AXI>(lc, E, B1, B2);
    double cx, cy;
    mag_ctr(E.X, E.Y, cx, cy);

    // GetJA (fpproc.cpp:3495-3578)
    cd A[3], Jn[3], J;
    double rn = 0, r = 0;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        if (!AXI) A[i] = E.A[i];
        else {
            rn = E.X[i] * lc;
            if (fabs(rn / lc) < 1.e-06) A[i] = cd{0, 0};
            else A[i] = E.A[i] / (2. * kPI * rn);
        }
    }
    if (AXI) r = cx * lc;
#pragma unroll
    for (int i = 0; i < 3; ++i) Jn[i] = cd_of(bp.J);
    J = cd_of(bp.J);
    double c = bp.Cduct;
    if (bp.lam) c = 0;
    if (lab.wound) c = 0;
    {   // the eddy currents: I * Frequency * 2. * PI * c * A[i]
        const cd iw = cd{0., 1.} * Frequency * 2. * kPI * c;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const cd t = iw * A[i];
            Jn[i] = Jn[i] - t;
            J = J - t / 3.;
        }
    }
    if (lab.ccase == 0) {
        const cd dV = cd_of(lab.dV);
        if (!AXI) {
#pragma unroll
            for (int i = 0; i < 3; ++i) Jn[i] = Jn[i] - c * dV;
            J = J - c * dV;
        } else {
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                rn = E.X[i];
                if (fabs(rn / lc) < 1.e-06) Jn[i] = Jn[i] - c * dV / r;
                else Jn[i] = Jn[i] - c * dV / (rn * lc);
            }
            J = J - c * dV / r;
        }
    } else if (lab.ccase > 0) {
#pragma unroll
        for (int i = 0; i < 3; ++i) Jn[i] = Jn[i] + cd_of(lab.J);
        J = J + cd_of(lab.J);
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) Jn[i] = Jn[i] * 1.e06;
    J = J * 1.e06;

    const double a = mag_area(E.X, E.Y, M.lc2);
    double rr[3] = {0, 0, 0}, R = 0;
    if (AXI) {
#pragma unroll
        for (int k = 0; k < 3; ++k) rr[k] = E.X[k] * lc;
        R = (rr[0] + rr[1] + rr[2]) / 3.;
    }
    const double av = AXI ? a * (2. * kPI * R) : a * Depth;   // the element's volume
    const cd ones[3] = {{1., 0.}, {1., 0.}, {1., 0.}};
    const double aecf = mag_aecf_of<AXI>(M.ext_ro, M.ext_ri, M.ext_zo, lab.external, cx, cy);

    // 0: A.J
    {
        cd V[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) V[k] = cd_conj(Jn[k]);
        const cd y = AXI ? mag_ac_axi_int(a, A, V, rr) : mag_ac_pln_int(a, A, V) * Depth;
        v[AS_AJ_R] = y.re;
        v[AS_AJ_I] = y.im;
    }
    // 1: A
    {
        cd y = {0, 0};
        if (AXI) y = mag_ac_axi_int(a, ones, A, rr);
        else {
#pragma unroll
            for (int k = 0; k < 3; ++k) y = y + a * Depth * A[k] / 3.;
        }
        v[AS_A_R] = y.re;
        v[AS_A_I] = y.im;
    }
    // 2 (and 17): DoEnergy(CComplex, CComplex), with the block's own GetMu
    cd mu1, mu2;
    mag_ac_get_mu(C, bp, B1, B2, mu1, mu2);
    {
        const cd h1 = B1 / (mu1 * kMUO), h2 = B2 / (mu2 * kMUO);
        const cd s = h1 * cd_conj(B1) + h2 * cd_conj(B2);
        double y = av * (s.re / 4.);
        y *= aecf;
        v[AS_ENERGY] = y;
    }
    // 3: hysteresis and lamination loss, through FPProc::GetMu (the AECF division)
    {
        const cd m1 = mu1 / aecf, m2 = mu2 / aecf;
        const cd H1 = B1 / (m1 * kMUO), H2 = B2 / (m2 * kMUO);
        const cd s = H1 * cd_conj(B1) + H2 * cd_conj(B2);
        v[AS_HYST] = av * kPI * Frequency * s.im;
    }
    // 4: resistive loss.  sig = 1e6 / Re(1. / o) with o the block's
    // conductivity; 1. / 0 is 0 / 0 there: taken as no loss
    {
        cd y = {0, 0};
        double sig = 0;
        if (bp.Cduct != 0) sig = 1.e06 / cd_inv(cd{bp.Cduct, 0.}).re;
        if (bp.lam) sig = 0;
        if (sig != 0) {
            if (!AXI) {
                cd V[3];
#pragma unroll
                for (int k = 0; k < 3; ++k) V[k] = cd_conj(Jn[k]) / sig;
                y = mag_ac_pln_int(a, Jn, V) * Depth;
            } else y = 2. * kPI * R * a * J * cd_conj(J) / sig;
            y = y / 2.;
        }
        v[AS_RES_R] = y.re;
        v[AS_RES_I] = y.im;
    }
    // 5, 10: area, volume
    v[AS_AREA] = a;
    v[AS_VOLUME] = av;
    // 7: total current
    v[AS_CUR_R] = a * J.re;
    v[AS_CUR_I] = a * J.im;
    // 8, 9: B over the volume
    v[AS_B1_R] = av * B1.re;
    v[AS_B1_I] = av * B1.im;
    v[AS_B2_R] = av * B2.re;
    v[AS_B2_I] = av * B2.im;
    // 11, 12: the steady Lorentz force
    {
        double y = -(B2.re * J.re + B2.im * J.im);
        if (AXI) y = 0;
        else y *= Depth;
        y *= 0.5;
        v[AS_FX] = a * y;
    }
    {
        cd V[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) V[k] = cd{(B1 * cd_conj(Jn[k])).re, 0.};
        cd y = AXI ? mag_ac_axi_int(-a, ones, V, rr) : mag_ac_pln_int(a, ones, V) * Depth;
        y = y * 0.5;
        v[AS_FY] = y.re;
    }
    // 13, 14: its double-frequency part
    if (AXI) v[AS_FX2_R] = v[AS_FX2_I] = 0.;
    else {
        const cd y = {-(B2.re * J.re - B2.im * J.im), -(B2.re * J.im + B2.im * J.re)};
        const cd t = 0.5 * (a * y * Depth);
        v[AS_FX2_R] = t.re;
        v[AS_FX2_I] = t.im;
    }
    {
        cd y = {(B1.re * J.re - B1.im * J.im), (B1.re * J.im + B1.im * J.re)};
        if (AXI) y = (-y * 2. * kPI * R);
        else y = y * Depth;
        const cd t = (a * y) / 2.;
        v[AS_FY2_R] = t.re;
        v[AS_FY2_I] = t.im;
    }
    // 15, 16: the Lorentz torque (planar), steady and double-frequency
    if (AXI) v[AS_TORQUE] = v[AS_T2_R] = v[AS_T2_I] = 0.;
    else {
        const double ccx = cx * lc, ccy = cy * lc;
        double y = ccy * (B2.re * J.re + B2.im * J.im) + ccx * (B1.re * J.re + B1.im * J.im);
        y *= 0.5;
        v[AS_TORQUE] = a * y * Depth;
        const cd y2 = ccx * cd{(B1.re * J.re - B1.im * J.im), (B1.re * J.im + B1.im * J.re)} +
                      ccy * cd{(B2.re * J.re - B2.im * J.im), (B2.re * J.im + B2.im * J.re)};
        const cd t = 0.5 * (a * y2 * Depth);
        v[AS_T2_R] = t.re;
        v[AS_T2_I] = t.im;
    }
    // 24: moment of inertia
    if (AXI) {
        const cd rc[3] = {{rr[0], 0.}, {rr[1], 0.}, {rr[2], 0.}};
        v[AS_INERTIA] = mag_ac_axi_int(a, rc, rc, rr).re;
    } else {
        double U[3], V[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            U[k] = E.X[k] * lc;
            V[k] = E.Y[k] * lc;
        }
        double y = U[0] * U[0] + U[1] * U[1] + U[2] * U[2];
        y += U[0] * U[1] + U[0] * U[2] + U[1] * U[2];
        y += V[0] * V[0] + V[1] * V[1] + V[2] * V[2];
        y += V[0] * V[1] + V[0] * V[2] + V[1] * V[2];
        y *= (a * Depth / 6.);
        v[AS_INERTIA] = y;
    }
    // 25: the centroid's two area-weighted sums
    v[AS_CX] = cx * a;
    v[AS_CY] = cy * a;
}

template <bool AXI>
__global__ void __launch_bounds__(kPotQBlock) k_mag_ac_integrands(int NE, MagArgs M, MagAcArgs C,
                                                                  double *__restrict__ part)
{
    const int e = blockIdx.x * kPotQBlock + threadIdx.x;
    double v[kMagAcSums];
#pragma unroll
    for (int c = 0; c < kMagAcSums; ++c) v[c] = 0.;
    if (e < NE) {
        MagAcElem E;
        mag_ac_load(M, e, E);
        const MagAcLabel lab = C.labels[E.lbl];
        if (lab.sel) mag_ac_integrands<AXI>(M, C, E, lab, v);
    }
    block_sums<kMagAcSums>(v, part);
}

// --- host side ------------------------------------------------------------------

// mu_fdx or mu_fdy of OpenDocument (fpproc.cpp:1716-1753)
static cd mag_ac_mu_fd(double mu, double theta, double Lam_d, double Cduct, double LamFill, double w)
{
    const cd I = {0., 1.};
    cd m = mu * cd_exp(-I * theta * kPI / 180.);
    if (Lam_d != 0) {
        const cd deg45 = {1., 1.};
        const cd halflag = cd_exp(-I * theta * kPI / 360.);
        const double ds = sqrt(2. / (0.4 * kPI * w * Cduct * mu));
        const cd K = halflag * deg45 * Lam_d * 0.001 / (2. * ds);
        if (Cduct != 0) m = (m * cd_tanh(K) / K) * LamFill + cd{(1. - LamFill), 0.};
        else m = (m)*LamFill + cd{(1. - LamFill), 0.};
    }
    return m;
}

void mag_ac_host_tables(xfk_problem *P, const xfk_problem_desc *d, const xfk_harmonic_desc *ac, const GlobalPrep &G,
                        const std::vector<DevBlockAC> &blk)
{
    const double w = 2. * kPI * ac->frequency;
    P->mag_hblk = G.blk;
    P->mag_hlab = G.lab;
    P->mag_nlabels = d->n_labels;
    P->mag_lab_orig.resize(G.lab.size());
    for (size_t k = 0; k < G.lab.size(); ++k) P->mag_lab_orig[k] = (int)std::min<size_t>(k, d->n_labels - 1);
    P->mag_ext_user[0] = d->ext_ro;
    P->mag_ext_user[1] = d->ext_ri;
    P->mag_ext_user[2] = d->ext_zo;
    P->mag_prev_type = ac->prev_type;
    P->mag_ac_hblk.assign(std::max(1, d->n_blocks), MagAcBlock{});
    for (int k = 0; k < d->n_blocks; ++k) {
        const xfk_block_desc &b = d->blocks[k];
        const xfk_block_ac_desc &a = ac->blocks[k];
        MagAcBlock &o = P->mag_ac_hblk[k];
        o.mu_fdx = o.mu_fdy = make_double2(1., 0.);
        if (b.LamType == 0) {
            const cd mx = mag_ac_mu_fd(b.mu_x, a.Theta_hx, a.Lam_d, b.Cduct, b.LamFill, w);
            const cd my = mag_ac_mu_fd(b.mu_y, a.Theta_hy, a.Lam_d, b.Cduct, b.LamFill, w);
            o.mu_fdx = make_double2(mx.re, mx.im);
            o.mu_fdy = make_double2(my.re, my.im);
        }
        o.J = make_double2(b.J_re, a.J_im);
        o.Cduct = b.Cduct;
        o.lam = ((a.Lam_d != 0) && (b.LamType == 0)) ? 1 : 0;
        o.LamType = b.LamType;
        o.bh_n = blk[k].bh_n;
        o.bh_off = blk[k].bh_off;
    }
}

// The problem kinds this post-processor answers; every other is refused with
// its name (post_entry: xfk_post.h)
template <class F>
static int mag_ac_entry(xfk_problem *P, F &&body)
{
    return post_entry(P, [&]() -> int {
        XFK_REQUIRE(P, XFK_ERR_ARG, "null problem");
        XFK_REQUIRE(!P->electro && !P->heat, XFK_ERR_ARG,
                    "not a magnetics problem: xfk_mag_ac_* post-processes time-harmonic magnetics problems (xfk_pot_* "
                    "is for electrostatic and heat-flow problems)");
        XFK_REQUIRE(P->harmonic, XFK_ERR_ARG,
                    "magnetostatic problem (Frequency 0): use xfk_mag_*; xfk_mag_ac_* post-processes time-harmonic "
                    "problems");
        XFK_REQUIRE(!P->comm, XFK_ERR_UNSUPPORTED,
                    "sharded problem: magnetics post-processing needs the whole mesh on one device");
        XFK_REQUIRE(P->mag_prev_type == 0, XFK_ERR_UNSUPPORTED,
                    "the problem was loaded with PrevType != 0 (incremental permeability about a previous solution): "
                    "its post-processing is not built");
        return XFK_OK;
    }, body);
}

// coordinates in user units, A of the solution, the block table on the device
static int mag_ac_prepare(xfk_problem *P)
{
    hipStream_t s = P->stream;
    const int N = P->N, G = (N + kBlock - 1) / kBlock;
    if (!P->mag_A_ready)
        XFK_REQUIRE(P->symbolic_ready && P->hc_vec.p && P->last.newton_iters > 0, XFK_ERR_ARG,
                    "no solution yet (solve the problem or xfk_mag_ac_set_solution)");
    int rc = mag_prepare_xy(P);
    if (rc != XFK_OK) return rc;
    if (!P->mag_ac_blk.p) {
        XFK_CHECK(upload(P->mag_ac_blk, P->mag_ac_hblk.data(), P->mag_ac_hblk.size(), s));
        XFK_CHECK(hipStreamSynchronize(s));
    }
    if (!P->mag_A_ready) {
        XFK_CHECK(P->mag_A.alloc(2 * (size_t)N));
        k_mag_ac_a<<<G, kBlock, 0, s>>>(N, P->axi ? 1 : 0, P->hc_vec.p, P->x.p, reinterpret_cast<double2 *>(P->mag_A.p));
        XFK_CHECK(hipGetLastError());
        P->mag_A_ready = true;
    }
    return XFK_OK;
}

static MagAcArgs mag_ac_args(const xfk_problem *P)
{
    MagAcArgs C = {};
    C.labels = reinterpret_cast<const MagAcLabel *>(P->mag_lab.p);
    C.blocks = P->mag_ac_blk.p;
    C.bhB = P->hbh_B.p;
    C.bhH = P->hbh_H.p;
    C.bhS = P->hbh_S.p;
    C.freq = P->omega / (2. * kPI);
    return C;
}

// The per-label table of a selection: block and flags from the problem's
// tables, Case / J / dVolts from the solve's circuit results as the .ans label
// lines carry them (harmonic2d.cpp:968-992: Case 2 is written as Case 0 with
// the solved gradient).  Refuses a selected LamType > 2 label.  answerable:
// select every label that is not one (xfk_mag_ac_time).
static int mag_ac_labels(xfk_problem *P, const unsigned char *sel, bool answerable = false)
{
    hipStream_t s = P->stream;
    const size_t nlab = P->mag_hlab.size();
    std::vector<MagAcLabel> t(std::max<size_t>(1, nlab), MagAcLabel{});
    for (size_t k = 0; k < nlab; ++k) {
        const DevLabel &L = P->mag_hlab[k];
        const MagAcBlock &B = P->mag_ac_hblk[L.blk];
        MagAcLabel &o = t[k];
        o.blk = L.blk;
        o.wound = L.is_wound ? 1 : 0;
        o.external = L.external ? 1 : 0;
        o.sel = answerable ? (B.LamType <= 2) : (sel[P->mag_lab_orig[k]] ? 1 : 0);
        o.ccase = -1;
        o.J = o.dV = make_double2(0., 0.);
        if (L.in_circuit >= 0 && L.in_circuit < P->ncircs) {
            const DevCircAC &Q = P->hcircs[L.in_circuit];
            o.ccase = Q.ccase == 1 ? 1 : 0;
            if (o.ccase == 0) o.dV = Q.dV;
            else o.J = Q.J;
        }
        XFK_REQUIRE(!o.sel || B.LamType <= 2, XFK_ERR_UNSUPPORTED,
                    "a selected label's block has LamType > 2 (a wound region with proximity effects): its current "
                    "density, conductivity and permeability need FPProc::GetFillFactor (wire diameter, strands, "
                    "turns), which the problem does not carry");
    }
    XFK_CHECK(P->mag_lab.alloc(sizeof(MagAcLabel) * t.size()));
    XFK_CHECK(hipMemcpyAsync(P->mag_lab.p, t.data(), sizeof(MagAcLabel) * t.size(), hipMemcpyHostToDevice, s));
    XFK_CHECK(hipStreamSynchronize(s));   // (t leaves scope)
    return XFK_OK;
}

static int mag_ac_launch_element_b(xfk_problem *P, const MagArgs &M)
{
    const int NE = P->NE, G = (NE + kBlock - 1) / kBlock;
    double2 *B = reinterpret_cast<double2 *>(P->mag_B.p);
    if (P->axi) k_mag_ac_element_b<true><<<G, kBlock, 0, P->stream>>>(NE, M, B, B + NE);
    else k_mag_ac_element_b<false><<<G, kBlock, 0, P->stream>>>(NE, M, B, B + NE);
    return hipGetLastError() == hipSuccess ? XFK_OK : XFK_ERR_HIP;
}

static int mag_ac_launch_integrals(xfk_problem *P, const MagArgs &M, const MagAcArgs &C)
{
    hipStream_t s = P->stream;
    const int NE = P->NE, G = (NE + kPotQBlock - 1) / kPotQBlock;
    double *part = P->mag_part.p, *sums = part + kMagAcSums * (size_t)G;
    if (P->axi) k_mag_ac_integrands<true><<<G, kPotQBlock, 0, s>>>(NE, M, C, part);
    else k_mag_ac_integrands<false><<<G, kPotQBlock, 0, s>>>(NE, M, C, part);
    k_pot_sum<kMagAcSums><<<1, kPotQBlock, 0, s>>>(G, part, sums);
    return hipGetLastError() == hipSuccess ? XFK_OK : XFK_ERR_HIP;
}

// every type as (re, im) pairs indexed by inttype
static int mag_ac_block_integrals(xfk_problem *P, const unsigned char *sel, double *out)
{
    XFK_REQUIRE(sel, XFK_ERR_ARG, "null selection mask (one byte per block label)");
    XFK_REQUIRE(out, XFK_ERR_ARG, "null output");
    int rc = mag_ac_labels(P, sel);
    if (rc == XFK_OK) rc = mag_ac_prepare(P);
    if (rc != XFK_OK) return rc;
    const int G = (P->NE + kPotQBlock - 1) / kPotQBlock;
    XFK_CHECK(P->mag_part.alloc(kMagAcSums * ((size_t)G + 1)));
    if ((rc = mag_ac_launch_integrals(P, mag_mesh_args(P), mag_ac_args(P))) != XFK_OK) {
        set_error("block integral launch failed");
        return rc;
    }
    double h[kMagAcSums];
    XFK_CHECK(d2h(h, P->mag_part.p + kMagAcSums * (size_t)G, sizeof(h), P->stream));
    for (int k = 0; k < 2 * kMagTypes; ++k) out[k] = 0.;
    auto put = [&](int type, double re, double im) {
        out[2 * type] = re;
        out[2 * type + 1] = im;
    };
    put(0, h[AS_AJ_R], h[AS_AJ_I]);
    put(1, h[AS_A_R], h[AS_A_I]);
    put(2, h[AS_ENERGY], 0.);
    put(3, h[AS_HYST], 0.);
    put(4, h[AS_RES_R], h[AS_RES_I]);
    put(5, h[AS_AREA], 0.);
    put(6, h[AS_HYST] + h[AS_RES_R], 0. + h[AS_RES_I]);   // BlockIntegral(3) + BlockIntegral(4)
    put(7, h[AS_CUR_R], h[AS_CUR_I]);
    put(8, h[AS_B1_R], h[AS_B1_I]);
    put(9, h[AS_B2_R], h[AS_B2_I]);
    put(10, h[AS_VOLUME], 0.);
    put(11, h[AS_FX], 0.);
    put(12, h[AS_FY], 0.);
    put(13, h[AS_FX2_R], h[AS_FX2_I]);
    put(14, h[AS_FY2_R], h[AS_FY2_I]);
    put(15, h[AS_TORQUE], 0.);
    put(16, h[AS_T2_R], h[AS_T2_I]);
    put(17, h[AS_ENERGY], 0.);   // DoCoEnergy(CComplex, CComplex) is DoEnergy
    put(24, h[AS_INERTIA], 0.);
    // the centroid: the two sums over BlockIntegral(5) (0 / 0 with nothing selected)
    put(25, h[AS_CX] / h[AS_AREA], h[AS_CY] / h[AS_AREA]);
    return XFK_OK;
}

}  // namespace xfk

using namespace xfk;

extern "C" {

int xfk_mag_ac_set_solution(xfk_problem *P, const double *A)
{
    return mag_ac_entry(P, [&]() -> int {
        XFK_REQUIRE(A, XFK_ERR_ARG, "null solution");
        P->mag_A_ready = false;
        XFK_CHECK(P->mag_A.alloc(2 * (size_t)P->N));
        XFK_CHECK(hipMemcpyAsync(P->mag_A.p, A, sizeof(double) * 2 * (size_t)P->N, hipMemcpyHostToDevice, P->stream));
        XFK_CHECK(hipStreamSynchronize(P->stream));
        P->mag_A_ready = true;
        return XFK_OK;
    });
}

int xfk_mag_ac_element_b(xfk_problem *P, double *B1, double *B2)
{
    return mag_ac_entry(P, [&]() -> int {
        int rc = mag_ac_prepare(P);
        if (rc != XFK_OK) return rc;
        const size_t NE = (size_t)P->NE;
        XFK_CHECK(P->mag_B.alloc(4 * NE));
        if ((rc = mag_ac_launch_element_b(P, mag_mesh_args(P))) != XFK_OK) {
            set_error("element B launch failed");
            return rc;
        }
        if (B1) XFK_CHECK(d2h(B1, P->mag_B.p, sizeof(double) * 2 * NE, P->stream));
        if (B2) XFK_CHECK(d2h(B2, P->mag_B.p + 2 * NE, sizeof(double) * 2 * NE, P->stream));
        XFK_CHECK(hipStreamSynchronize(P->stream));
        return XFK_OK;
    });
}

int xfk_mag_ac_block_integrals(xfk_problem *P, const unsigned char *label_selected, double *out)
{
    return mag_ac_entry(P, [&]() -> int { return mag_ac_block_integrals(P, label_selected, out); });
}

int xfk_mag_ac_block_integral(xfk_problem *P, const unsigned char *label_selected, int type, double *out2)
{
    return mag_ac_entry(P, [&]() -> int {
        XFK_REQUIRE(type >= 0 && type < kMagTypes, XFK_ERR_ARG, "block integral type out of range (0-25)");
        XFK_REQUIRE(out2, XFK_ERR_ARG, "null output");
        double o[2 * kMagTypes];
        const int rc = mag_ac_block_integrals(P, label_selected, o);
        if (rc != XFK_OK) return rc;
        out2[0] = o[2 * type];
        out2[1] = o[2 * type + 1];
        return XFK_OK;
    });
}

int xfk_mag_ac_time(xfk_problem *P, int repeats, double *ms)
{
    return mag_ac_entry(P, [&]() -> int {
        XFK_REQUIRE(repeats > 0 && ms, XFK_ERR_ARG, "xfk_mag_ac_time needs repeats > 0 and its output");
        int rc = mag_ac_labels(P, nullptr, true);
        if (rc == XFK_OK) rc = mag_ac_prepare(P);
        if (rc != XFK_OK) return rc;
        hipStream_t s = P->stream;
        const size_t NE = (size_t)P->NE;
        const int G = (P->NE + kPotQBlock - 1) / kPotQBlock;
        XFK_CHECK(P->mag_part.alloc(kMagAcSums * ((size_t)G + 1)));
        XFK_CHECK(P->mag_B.alloc(4 * NE));
        const MagArgs M = mag_mesh_args(P);
        const MagAcArgs C = mag_ac_args(P);
        auto timed = [&](auto f, double &out) { return timed_median(s, repeats, f, out); };
        rc = timed([&] { return mag_ac_launch_element_b(P, M); }, ms[0]);
        if (rc != XFK_OK) return rc;
        return timed([&] { return mag_ac_launch_integrals(P, M, C); }, ms[1]);
    });
}

}  // extern "C"
