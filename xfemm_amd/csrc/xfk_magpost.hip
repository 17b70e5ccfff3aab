// Post-processing of a magnetostatic problem on the device: the element flux
// density, the volume integrals of the reference's fpproc that need no mask,
// the weighted stress tensor force and torque over its mask, and its point
// values and contour integrals, for MI355X (gfx950).  Frequency 0 only, planar and axisymmetric.
//
//   element B         FPProc::GetElementB (fpproc.cpp:2970-3082)
//   J and A           FPProc::GetJA (3495-3578), PlnInt / AxiInt (3580-3612),
//                     Ctr (3426-3438), ElmArea (3440-3468), AECF (5286-5304)
//   energy            CMMaterialProp::GetH, GetEnergy, GetCoEnergy, DoEnergy,
//                     DoCoEnergy (CMaterialProp.cpp:488-519, 537-677)
//   block integrals   FPProc::BlockIntegral types 0 1 2 5 7 8 9 10 11 12 15 17
//                     24 25 (3642-4092)
//   the mask          FPProc::MakeMask (makemask.cpp:48-414): the air test
//                     here (108-132), the rest in xfk_mask.hip
//   force and torque  HenrotteVector (3614-3640), BlockIntegral types 18-23
//                     (3966-4079)
//   point values      GetNodalB (2704-2967), GetPointB (2669-2702),
//                     GetPointValues (2257-2498), InTriangleTest (3387-3424)
//   contour integrals LineIntegral (4094-4515)
//
// fpproc works in the problem's own length units with LengthConv[] to metres;
// the solver in cm.  The coordinates are divided back by the solver's unit once
// (mag_x, mag_y) and everything below reads those.  A is the value the .ans
// carries: V c, times 2 pi r on an axisymmetric problem (static2d.cpp:1018-1021,
// staticaxi.cpp:774-779).  All arithmetic is the reference's, operation by
// operation, in double, without contraction into fused multiply-adds.
//
// One pass over the elements gives every integral type: a thread per element
// evaluates the element's B, J, A and the integrands of all types (zero where
// the element's label is not selected), and the workgroup's sums go to partials
// in a fixed order (block_sums); one workgroup then sums the partials in a
// fixed order (k_pot_sum).  No atomics: two calls give the same bits.
#include "xfk_potential.h"

#pragma clang fp contract(off)

// (what the time-harmonic post-processor, xfk_magpost_ac.hip, reads too: the
// unit tables, MagLabel, MagArgs, GetElementB, Ctr, ElmArea, AECF, k_mag_xy)
#include "xfk_magpost.h"
#include "xfk_ppsearch.h"

#include <array>
#include <cstring>
#include <map>

namespace xfk {

// the sums one pass makes, in this order
enum {
    MS_AJ, MS_A, MS_ENERGY, MS_AREA, MS_CURRENT, MS_B1, MS_B2, MS_VOLUME, MS_FX, MS_FY, MS_TORQUE, MS_COENERGY,
    MS_INERTIA, MS_CX, MS_CY, kMagSums
};

// CMMaterialProp::GetH(double) on B >= 0 (CMaterialProp.cpp:488-519): the
// section search is a loop over the block's BHpoints knots
__device__ __forceinline__ double mag_get_h(const MagArgs &M, const DevBlock &bp, double x)
{
    const double b = fabs(x);
    const int n = bp.BHpoints;
    if ((n == 0) || (b == 0)) return 0;
    const double *B = M.bhB + bp.bh_off, *H = M.bhH + bp.bh_off, *S = M.bhS + bp.bh_off;
    const double p = x / b;
    if (b > B[n - 1]) return p * (H[n - 1] + S[n - 1] * (b - B[n - 1]));
    for (int i = 0; i < n - 1; ++i)
        if ((b >= B[i]) && (b <= B[i + 1])) {
            const double l = B[i + 1] - B[i];
            const double z = (b - B[i]) / l;
            const double z2 = z * z;
            const double h = (1. - 3. * z2 + 2. * z2 * z) * H[i] + z * (1. - 2. * z + z2) * l * S[i] +
                             z2 * (3. - 2. * z) * H[i + 1] + z2 * (z - 1.) * l * S[i + 1];
            return p * h;
        }
    return 0;
}

// CMMaterialProp::GetEnergy (CMaterialProp.cpp:537-588)
__device__ __forceinline__ double mag_get_energy(const MagArgs &M, const DevBlock &bp, double x)
{
    const double b = fabs(x);
    double nrg = 0.;
    const int n = bp.BHpoints;
    if (n == 0) return 0;
    const double *B = M.bhB + bp.bh_off, *H = M.bhH + bp.bh_off, *S = M.bhS + bp.bh_off;
    for (int i = 0; i < n - 1; ++i) {
        const double b0 = B[i], h0 = H[i], b1 = B[i + 1], h1 = H[i + 1];
        const double dh0 = S[i], dh1 = S[i + 1];
        if ((b >= b0) && (b <= b1)) {
            const double l = b1 - b0;
            const double z = (b - b0) / l;
            const double z2 = z * z;
            nrg += (dh0 * l * l * (6. + z * (-8. + 3. * z)) * z2) / 12. + (h0 * l * z * (2. + (-2. + z) * z2)) / 2. -
                   (h1 * l * (-2. + z) * z2 * z) / 2. + (dh1 * l * l * (-4. + 3. * z) * z2 * z) / 12;
            return nrg;
        }
        nrg += ((b0 - b1) * ((b0 - b1) * (dh0 - dh1) - 6. * (h0 + h1))) / 12.;
    }
    // off the scale: extrapolate the rest of the way
    const double h0 = H[n - 1], dh0 = S[n - 1], b0 = B[n - 1];
    nrg += ((b - b0) * (b * dh0 - b0 * dh0 + 2 * h0)) / 2.;
    return nrg;
}

// GetCoEnergy (CMaterialProp.cpp:590-593)
__device__ __forceinline__ double mag_get_coenergy(const MagArgs &M, const DevBlock &bp, double b)
{
    return (fabs(b) * mag_get_h(M, bp, b) - mag_get_energy(M, bp, b));
}

// DoEnergy / DoCoEnergy (CMaterialProp.cpp:595-677), LamType 0 1 2 (a
// LamType > 2 label is refused on the host).  The linear LamType 1 and 2
// cases multiply b1 where one would expect b2: kept as written.
template <bool CO>
__device__ __forceinline__ double mag_do_energy(const MagArgs &M, const DevBlock &bp, double b1, double b2)
{
    const double muo = kMUO;
    const double LamFill = bp.LamFill;
    if (bp.BHpoints == 0) {
        double h1 = 0, h2 = 0;
        if (bp.LamType == 0) {
            h1 = b1 / ((1. + LamFill * (bp.mu_x - 1.)) * muo);
            h2 = b2 / ((1. + LamFill * (bp.mu_y - 1.)) * muo);
        }
        if (bp.LamType == 1) {
            h1 = b1 / ((1. + LamFill * (bp.mu_x - 1.)) * muo);
            h2 = b1 * (LamFill / (bp.mu_y * muo) + (1. - LamFill) / muo);
        }
        if (bp.LamType == 2) {
            h2 = b1 / ((1. + LamFill * (bp.mu_y - 1.)) * muo);
            h1 = b1 * (LamFill / (bp.mu_x * muo) + (1. - LamFill) / muo);
        }
        return ((h1 * b1 + h2 * b2) / 2.);
    }
    auto raw = [&](double b) { return CO ? mag_get_coenergy(M, bp, b) : mag_get_energy(M, bp, b); };
    double nrg = 0;
    if (bp.LamType == 0) nrg = raw(sqrt(b1 * b1 + b2 * b2));
    if (bp.LamType == 1) {
        const double biron = sqrt((b1 / LamFill) * (b1 / LamFill) + b2 * b2);
        const double bair = b2;
        nrg = LamFill * raw(biron) + (1 - LamFill) * bair * bair / (2. * muo);
    }
    if (bp.LamType == 2) {
        const double biron = sqrt((b2 / LamFill) * (b2 / LamFill) + b1 * b1);
        const double bair = b1;
        nrg = LamFill * raw(biron) + (1 - LamFill) * bair * bair / (2. * muo);
    }
    return nrg;
}

// PlnInt / AxiInt (fpproc.cpp:3580-3612) on real arguments
__device__ __forceinline__ double mag_pln_int(double a, const double (&u)[3], const double (&v)[3])
{
    double z[3], x = 0;
    z[0] = 2. * u[0] + u[1] + u[2];
    z[1] = u[0] + 2. * u[1] + u[2];
    z[2] = u[0] + u[1] + 2. * u[2];
#pragma unroll
    for (int i = 0; i < 3; ++i) x += v[i] * z[i];
    return a * x / 12.;
}

__device__ __forceinline__ double mag_axi_int(double a, const double (&u)[3], const double (&v)[3],
                                              const double (&r)[3])
{
    double Mx[3][3], z[3], x = 0;
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
    for (int i = 0; i < 3; ++i) x += v[i] * z[i];
    return kPI * a * x / 30.;
}

struct MagElem {
    double X[3], Y[3], A[3];
    int lbl;
};

// AECF (fpproc.cpp:5286-5304) of an element with centroid (cx, cy)
template <bool AXI>
__device__ __forceinline__ double mag_aecf(const MagArgs &M, const MagLabel &lab, double cx, double cy)
{
    return mag_aecf_of<AXI>(M.ext_ro, M.ext_ri, M.ext_zo, lab.external, cx, cy);
}

__device__ __forceinline__ void mag_load(const MagArgs &M, int e, MagElem &E)
{
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const int n = M.p[3 * e + j];
        E.X[j] = M.x[n];
        E.Y[j] = M.y[n];
        E.A[j] = M.A[n];
    }
    E.lbl = M.lbl[e];
}

template <bool AXI>
__global__ void __launch_bounds__(kBlock) k_mag_element_b(int NE, MagArgs M, double *__restrict__ B1,
                                                          double *__restrict__ B2)
{
    const int e = blockIdx.x * kBlock + threadIdx.x;
    if (e >= NE) return;
    MagElem E;
    mag_load(M, e, E);
    double b1, b2;
    mag_element_b<AXI>(M.lc, E.X, E.Y, E.A, b1, b2);
    B1[e] = b1;
    B2[e] = b2;
}

// The integrands of one element of a selected label: one case of
// FPProc::BlockIntegral's switch per sum, in the reference's operation order
template <bool AXI>
__device__ __forceinline__ void mag_integrands(const MagArgs &M, const MagElem &E, const MagLabel &lab,
                                               double (&v)[kMagSums])
{
    const DevBlock bp = M.blocks[lab.blk];
    const double lc = M.lc, Depth = M.depth;
    double B1, B2;
    mag_element_b<AXI>(lc, E.X, E.Y, E.A, B1, B2);
    // Ctr (kept inline, as is ElmArea below: mag_ctr and mag_area of
    // xfk_magpost.h are the same operations, but this kernel's instruction
    // stream is held to what it was before the header existed)
    double cx = 0., cy = 0.;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        cx += E.X[j] / 3.;
        cy += E.Y[j] / 3.;
    }
    // GetJA (fpproc.cpp:3495-3578) at Frequency 0
    double A[3], Jn[3], J;
    double rn = 0, r = 0;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        if (!AXI) A[i] = E.A[i];
        else {
            rn = E.X[i] * lc;
            if (fabs(rn / lc) < 1.e-06) A[i] = 0;
            else A[i] = E.A[i] / (2. * kPI * rn);
        }
    }
    if (AXI) r = cx * lc;
#pragma unroll
    for (int i = 0; i < 3; ++i) Jn[i] = bp.J_re;
    J = bp.J_re;
    double c = bp.Cduct;
    if (lab.wound) c = 0;
    if (lab.ccase == 0) {
        if (!AXI) {
#pragma unroll
            for (int i = 0; i < 3; ++i) Jn[i] -= c * lab.dV;
            J -= c * lab.dV;
        } else {
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                rn = E.X[i];
                if (fabs(rn / lc) < 1.e-06) Jn[i] -= c * lab.dV / r;
                else Jn[i] -= c * lab.dV / (rn * lc);
            }
            J -= c * lab.dV / r;
        }
    } else if (lab.ccase > 0) {
#pragma unroll
        for (int i = 0; i < 3; ++i) Jn[i] += lab.J;
        J += lab.J;
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) Jn[i] *= 1.e06;
    J = J * 1.e06;

    // ElmArea, r[], R
    const double b0 = E.Y[1] - E.Y[2], b1 = E.Y[2] - E.Y[0];
    const double c0 = E.X[2] - E.X[1], c1 = E.X[0] - E.X[2];
    const double a = ((b0 * c1 - b1 * c0) / 2.) * M.lc2;
    double rr[3] = {0, 0, 0}, R = 0;
    if (AXI) {
#pragma unroll
        for (int k = 0; k < 3; ++k) rr[k] = E.X[k] * lc;
        R = (rr[0] + rr[1] + rr[2]) / 3.;
    }
    const double av = AXI ? a * (2. * kPI * R) : a * Depth;   // the element's volume
    const double ones[3] = {1., 1., 1.};
    const double aecf = mag_aecf<AXI>(M, lab, cx, cy);

    // 0: A.J
    v[MS_AJ] = AXI ? mag_axi_int(a, A, Jn, rr) : mag_pln_int(a, A, Jn) * Depth;
    // 1: A
    if (AXI) v[MS_A] = mag_axi_int(a, ones, A, rr);
    else {
        double y = 0;
#pragma unroll
        for (int k = 0; k < 3; ++k) y += a * Depth * A[k] / 3.;
        v[MS_A] = y;
    }
    // 2: stored energy, with the second-quadrant correction of a linear magnet
    {
        double y;
        if (bp.H_c != 0 && bp.BHpoints == 0) {
            const double mu1 = bp.mu_x, mu2 = bp.mu_y;
            double H1 = B1 / (mu1 * kMUO), H2 = B2 / (mu2 * kMUO);
            H1 = H1 - bp.H_c * lab.cos_m;
            H2 = H2 - bp.H_c * lab.sin_m;
            y = av * 0.5 * kMUO * (mu1 * H1 * H1 + mu2 * H2 * H2);
        } else y = av * mag_do_energy<false>(M, bp, B1, B2);
        v[MS_ENERGY] = y * aecf;
    }
    // 5, 10: area, volume
    v[MS_AREA] = a;
    v[MS_VOLUME] = av;
    // 7: total current
    v[MS_CURRENT] = a * J;
    // 8, 9: B over the volume
    v[MS_B1] = av * B1;
    v[MS_B2] = av * B2;
    // 11, 12: Lorentz force
    if (AXI) v[MS_FX] = a * 0.;
    else {
        double y = -(B2 * J);
        y *= Depth;
        v[MS_FX] = a * y;
    }
    {
        double V[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) V[k] = B1 * Jn[k];
        v[MS_FY] = AXI ? mag_axi_int(-a, ones, V, rr) : mag_pln_int(a, ones, V) * Depth;
    }
    // 15: Lorentz torque (planar)
    if (AXI) v[MS_TORQUE] = 0.;
    else {
        const double ccx = cx * lc, ccy = cy * lc;
        const double y = ccy * (B2 * J) + ccx * (B1 * J);
        v[MS_TORQUE] = a * y * Depth;
    }
    // 17: coenergy
    v[MS_COENERGY] = av * mag_do_energy<true>(M, bp, B1, B2) * aecf;
    // 24: moment of inertia
    if (AXI) v[MS_INERTIA] = mag_axi_int(a, rr, rr, rr);
    else {
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
        v[MS_INERTIA] = y;
    }
    // 25: the centroid's two area-weighted sums
    v[MS_CX] = cx * a;
    v[MS_CY] = cy * a;
}

template <bool AXI>
__global__ void __launch_bounds__(kPotQBlock) k_mag_integrands(int NE, MagArgs M, double *__restrict__ part)
{
    const int e = blockIdx.x * kPotQBlock + threadIdx.x;
    double v[kMagSums];
#pragma unroll
    for (int c = 0; c < kMagSums; ++c) v[c] = 0.;
    if (e < NE) {
        MagElem E;
        mag_load(M, e, E);
        const MagLabel lab = M.labels[E.lbl];
        if (lab.sel) mag_integrands<AXI>(M, E, lab, v);
    }
    block_sums<kMagSums>(v, part);
}

// BlockIntegral types 18-23 (fpproc.cpp:3966-4079) with HenrotteVector
// (3614-3640) at Frequency 0: one thread per element over ALL elements,
// whatever the selection; per workgroup the six sums in the order 18 .. 23
// into part.  B1 and B2 are real, so the reference's complex products reduce
// to the real ones written here, operation by operation.
enum { MW_FX, MW_FY, MW_FX2, MW_FY2, MW_T, MW_T2, kMagStressSums };

template <bool AXI>
__global__ void __launch_bounds__(kPotQBlock) k_mag_stress(int NE, MagArgs M, const double *__restrict__ msk,
                                                           double *__restrict__ part)
{
    const int e = blockIdx.x * kPotQBlock + threadIdx.x;
    double v[kMagStressSums];
#pragma unroll
    for (int c = 0; c < kMagStressSums; ++c) v[c] = 0.;
    if (e < NE) {
        MagElem E;
        mag_load(M, e, E);
        const MagLabel lab = M.labels[E.lbl];
        const double lc = M.lc, muo = kMUO;
        double B1, B2;
        mag_element_b<AXI>(lc, E.X, E.Y, E.A, B1, B2);
        double b[3], c[3], m[3];
        b[0] = E.Y[1] - E.Y[2]; b[1] = E.Y[2] - E.Y[0]; b[2] = E.Y[0] - E.Y[1];
        c[0] = E.X[2] - E.X[1]; c[1] = E.X[0] - E.X[2]; c[2] = E.X[1] - E.X[0];
#pragma unroll
        for (int j = 0; j < 3; ++j) m[j] = msk[M.p[3 * e + j]];
        const double da = (b[0] * c[1] - b[1] * c[0]);
        // HenrotteVector
        double hr = 0., hi = 0.;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            hr -= (m[j] * b[j]) / (da * lc);
            hi -= (m[j] * c[j]) / (da * lc);
        }
        double a = (da / 2.) * M.lc2;
        double cx = 0., cy = 0.;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            cx += E.X[j] / 3.;
            cy += E.Y[j] / 3.;
        }
        if (AXI) {
            const double r0 = E.X[0] * lc, r1 = E.X[1] * lc, r2 = E.X[2] * lc;
            const double R = (r0 + r1 + r2) / 3.;
            a *= (2. * kPI * R);
        } else a *= M.depth;
        const double aecf = mag_aecf<AXI>(M, lab, cx, cy);
        // (cases 18 19 22 write 2. * Re(B1 * conj(B2)), cases 20 21 23 2. * B1 * B2)
        const double d12 = (B1 * B1) - (B2 * B2), d21 = (B2 * B2) - (B1 * B1);
        const double bb = 2. * (B1 * B2), b2 = 2. * B1 * B2;
        const double F1 = (d12 * hr + bb * hi) / (2. * muo), F2 = (d21 * hi + bb * hr) / (2. * muo);
        const double G1 = (d12 * hr + b2 * hi) / (4. * muo), G2 = (d21 * hi + b2 * hr) / (4. * muo);
        if (!AXI) {
            v[MW_FX] = a * (F1 * aecf);
            v[MW_FX2] = (a * G1) * aecf;
            // the torque about the origin: the centroid in metres
            double tr = 0., ti = 0.;
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                tr += (E.X[j] * lc) / 3.;
                ti += (E.Y[j] * lc) / 3.;
            }
            v[MW_T] = a * ((tr * F2 - ti * F1) * aecf);
            v[MW_T2] = (a * (tr * G2 - ti * G1)) * aecf;
        }
        v[MW_FY] = a * (F2 * aecf);
        v[MW_FY2] = (a * G2) * aecf;
    }
    block_sums<kMagStressSums>(v, part);
}

// --- point values and contour integrals ----------------------------------------
//
//   GetNodalB        fpproc.cpp:2704-2967      k_mag_corner
//   GetPointValues   2257-2498, GetPointB 2669-2702, FPProc::GetMu 5322-5328,
//                    CMMaterialProp::GetMu CMaterialProp.cpp:775-844   k_mag_points
//   LineIntegral     4094-4515                 k_mag_contour
//
// The element of a point is the lowest-numbered one containing it (pp_find),
// not the one InTriangle's walk from its static k reaches.  Where
// oracle/pointvalues.py, the restatement the recorded field values were
// checked with, associates differently from fpproc.cpp, its order is taken:
// an interface's tangential and normal parts are added to each other before
// they are added to the nodal value (fpproc.cpp:2818-2821 adds them in turn),
// and a corner value is multiplied by its weight already divided by da
// (fpproc.cpp:2699 divides the product).

constexpr int kMagPointVals = 13;   // A B1 B2 mu1 mu2 H1 H2 Js c E Hc.re Hc.im ff

struct MagCornerArgs {
    const int *n2e_ptr, *n2e;   // ConList: node -> elements, ascending
    const int *clab;            // per entry of the label table: the descriptor's label, its "same material" class
    const unsigned char *pj;    // the node carries a point current
    const double *B1, *B2;      // the element flux density
};

// The interface side k-pt seen from an element with flux density (eB1, eB2)
// (fpproc.cpp:2799-2823): tangential B from the element, normal B from the A
// difference along the side
template <bool AXI>
__device__ __forceinline__ void mag_interface(const MagArgs &M, int k, int pt, double eB1, double eB2, double &R,
                                              double &b1, double &b2, double &vx, double &vy)
{
    double tnx = M.x[pt] - M.x[k], tny = M.y[pt] - M.y[k];
    const double r = (M.x[pt] + M.x[k]) * M.lc / 2.;
    const double atn = mag_cabs(tnx, tny);
    double bn = (M.A[pt] - M.A[k]) / (atn * M.lc);
    if (AXI) bn /= (-2. * kPI * r);
    const double z = 0.5 / atn;
    tnx /= atn;
    tny /= atn;
    const double bt = eB1 * tnx + eB2 * tny;
    R += z;
    b1 += (z * tnx * bt + z * tny * bn);
    b2 += (z * tny * bt - z * tnx * bn);
    vx = tnx;
    vy = tny;
}

// The walk around node k from element e to an interface, counter-clockwise or
// clockwise (fpproc.cpp:2767-2826, 2832-2889); true: a side without a
// neighbour, the "special-case punt" (b1, b2 are then that element's)
template <bool AXI, bool CCW>
__device__ __forceinline__ bool mag_walk(const MagArgs &M, const MagCornerArgs &C, int e, int k, int l0, int num,
                                         int mylabel, double &R, double &b1, double &b2, double &vx, double &vy)
{
    int ec = e;
    for (int q = 0; q < num; ++q) {
        int pt = 0;
        for (int j = 0; j < 3; ++j)
            if (M.p[3 * ec + j] == k) pt = j;
        if (CCW) {
            pt--;
            if (pt < 0) pt = 2;
        } else {
            pt++;
            if (pt > 2) pt = 0;
        }
        pt = M.p[3 * ec + pt];
        // the element adjacent to this side: the last matching entry of ConList
        int nxt = -1;
        for (int j = 0; j < num; ++j) {
            const int c = C.n2e[l0 + j];
            if (c != ec)
                for (int l = 0; l < 3; ++l)
                    if (M.p[3 * c + l] == pt) nxt = c;
        }
        if (nxt == -1) {
            b1 = C.B1[ec];
            b2 = C.B2[ec];
            return true;
        }
        if (mylabel != C.clab[2 * M.lbl[nxt]]) {
            mag_interface<AXI>(M, k, pt, C.B1[ec], C.B2[ec], R, b1, b2, vx, vy);
            return false;
        }
        ec = nxt;
    }
    return false;
}

// GetNodalB: one thread per (element, corner); bc[6 e + 2 i], [.. + 1] = b1, b2
// of corner i.  branch (may be null): 0 the patch, 1 an interface, 2 the
// special-case punt, + 4 the sharp-corner punt
template <bool AXI>
__global__ void __launch_bounds__(kBlock) k_mag_corner(int NE, MagArgs M, MagCornerArgs C, double *__restrict__ bc,
                                                       unsigned char *__restrict__ branch)
{
    const int t = blockIdx.x * kBlock + threadIdx.x;
    if (t >= 3 * NE) return;
    const int e = t / 3, i = t - 3 * e;
    const int k = M.p[3 * e + i];
    const double px = M.x[k], py = M.y[k];
    const int l0 = C.n2e_ptr[k], num = C.n2e_ptr[k + 1] - l0;
    const int mylabel = C.clab[2 * M.lbl[e]], myclass = C.clab[2 * M.lbl[e] + 1];
    double b1 = 0., b2 = 0.;
    int br = 0;
    int m = 0;
    for (int j = 0; j < num; ++j) {
        const int l = M.lbl[C.n2e[l0 + j]];
        if (mylabel == C.clab[2 * l]) m++;
        else if (myclass == C.clab[2 * l + 1]) m++;
    }
    if (m == num) {
        // normal smoothing method for points away from any boundaries
        double R = 0;
        for (int j = 0; j < num; ++j) {
            const int c = C.n2e[l0 + j];
            double cx = 0., cy = 0.;
            for (int q = 0; q < 3; ++q) {
                cx += M.x[M.p[3 * c + q]] / 3.;
                cy += M.y[M.p[3 * c + q]] / 3.;
            }
            const double z = 1. / mag_cabs(px - cx, py - cy);
            R += z;
            b1 += (z * C.B1[c]);
            b2 += (z * C.B2[c]);
        }
        b1 /= R;
        b2 /= R;
    } else {
        double R = 0, v1x = 0, v1y = 0, v2x = 0, v2y = 0;
        br = 1;
        if (mag_walk<AXI, true>(M, C, e, k, l0, num, mylabel, R, b1, b2, v1x, v1y)) {
            v1x = 1; v1y = 0; v2x = 1; v2y = 0;
            br = 2;
        }
        if ((v2x == 0) && (v2y == 0)) {   // (not after the punt, which has set the values)
            if (mag_walk<AXI, false>(M, C, e, k, l0, num, mylabel, R, b1, b2, v2x, v2y)) {
                v1x = 1; v1y = 0; v2x = 1; v2y = 0;
                br = 2;
            }
            b1 /= R;
            b2 /= R;
        }
        // too sharp a corner for the interface rule?
        bool flag = false;
        if ((mag_cabs(v1x, v1y) < 0.9) || (mag_cabs(v2x, v2y) < 0.9)) flag = true;
        if ((-v1x * v2x - v1y * v2y) > 0.985) flag = true;
        if (!flag) {
            br += 4;
            double bn = 0;
            for (int j = 0; j < num; ++j) {
                const int c = C.n2e[l0 + j];
                if (mylabel == C.clab[2 * M.lbl[c]]) {
                    const double bt = sqrt(C.B1[c] * C.B1[c] + C.B2[c] * C.B2[c]);
                    if (bt > bn) bn = bt;
                }
            }
            const double R2 = sqrt(C.B1[e] * C.B1[e] + C.B2[e] * C.B2[e]);
            if (R2 != 0) {
                b1 = bn / R2 * C.B1[e];
                b2 = bn / R2 * C.B2[e];
            } else {
                b1 = 0;
                b2 = 0;
            }
        }
    }
    // a point current at the node: the element's own values
    if (C.pj[k]) {
        b1 = C.B1[e];
        b2 = C.B2[e];
    }
    // a node on the axis: Br = 0
    if (AXI && (fabs(px) < 1.e-06)) b1 = 0.;
    bc[6 * (size_t)e + 2 * i] = b1;
    bc[6 * (size_t)e + 2 * i + 1] = b2;
    if (branch) branch[t] = (unsigned char)br;
}

// CMMaterialProp::GetMu(double ...) (CMaterialProp.cpp:775-844) at MuMax == 0
__device__ __forceinline__ void mag_get_mu(const MagArgs &M, const DevBlock &bp, double b1, double b2, double &mu1,
                                           double &mu2)
{
    const double muo = kMUO, LamFill = bp.LamFill;
    mu1 = mu2 = muo;
    if (bp.BHpoints == 0) {
        if (bp.LamType == 0) {
            mu1 = ((1. + LamFill * (bp.mu_x - 1.)) * muo);
            mu2 = ((1. + LamFill * (bp.mu_y - 1.)) * muo);
        }
        if (bp.LamType == 1) {
            mu1 = ((1. + LamFill * (bp.mu_x - 1.)) * muo);
            mu2 = 1. / (LamFill / (bp.mu_y * muo) + (1. - LamFill) / muo);
        }
        if (bp.LamType == 2) {
            mu2 = ((1. + LamFill * (bp.mu_y - 1.)) * muo);
            mu1 = 1. / (LamFill / (bp.mu_x * muo) + (1. - LamFill) / muo);
        }
    } else {
        const double s0 = M.bhS[bp.bh_off];
        double muiron;
        if (bp.LamType == 0) {
            const double biron = sqrt(b1 * b1 + b2 * b2);
            if (biron < 1.e-08) mu1 = 1. / s0;
            else mu1 = biron / mag_get_h(M, bp, biron);
            mu2 = mu1;
        }
        if (bp.LamType == 1) {
            const double biron = sqrt((b1 / LamFill) * (b1 / LamFill) + b2 * b2);
            if (biron < 1.e-08) muiron = 1. / s0;
            else muiron = biron / mag_get_h(M, bp, biron);
            mu1 = muiron * LamFill;
            mu2 = 1. / (LamFill / muiron + (1. - LamFill) / muo);
        }
        if (bp.LamType == 2) {
            const double biron = sqrt((b2 / LamFill) * (b2 / LamFill) + b1 * b1);
            if (biron < 1.e-08) muiron = 1. / s0;
            else muiron = biron / mag_get_h(M, bp, biron);
            mu2 = muiron * LamFill;
            mu1 = 1. / (LamFill / muiron + (1. - LamFill) / muo);
        }
    }
    mu1 /= muo;
    mu2 /= muo;
}

// GetPointValues(x, y, k, u) at Frequency 0 with d_ShiftH: the kMagPointVals
// values of a point of element k.  B: the element flux density (B1 then B2),
// bc: the corner values (read when smooth)
template <bool AXI>
__device__ __forceinline__ void mag_values_at(const MagArgs &M, int NE, int k, double x, double y, int smooth,
                                              const double *__restrict__ B, const double *__restrict__ bc,
                                              double (&o)[kMagPointVals])
{
    MagElem E;
    mag_load(M, k, E);
    const MagLabel lab = M.labels[E.lbl];
    const DevBlock bp = M.blocks[lab.blk];
    const double muo = kMUO;
    double a[3], b[3], c[3];
    a[0] = E.X[1] * E.Y[2] - E.X[2] * E.Y[1];
    a[1] = E.X[2] * E.Y[0] - E.X[0] * E.Y[2];
    a[2] = E.X[0] * E.Y[1] - E.X[1] * E.Y[0];
    b[0] = E.Y[1] - E.Y[2]; b[1] = E.Y[2] - E.Y[0]; b[2] = E.Y[0] - E.Y[1];
    c[0] = E.X[2] - E.X[1]; c[1] = E.X[0] - E.X[2]; c[2] = E.X[1] - E.X[0];
    const double da = (b[0] * c[1] - b[1] * c[0]);
    double ravg = M.lc * (E.X[0] + E.X[1] + E.X[2]) / 3.;
    // GetPointB
    double B1, B2;
    if (!smooth) {
        B1 = B[k];
        B2 = B[NE + k];
    } else {
        B1 = 0;
        B2 = 0;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const double w = (a[i] + b[i] * x + c[i] * y) / da;
            B1 += bc[6 * (size_t)k + 2 * i] * w;
            B2 += bc[6 * (size_t)k + 2 * i + 1] * w;
        }
    }
    double A = 0;
    if (!AXI) {
#pragma unroll
        for (int i = 0; i < 3; ++i) A += E.A[i] * (a[i] + b[i] * x + c[i] * y) / (da);
    } else {
        double v[6];
        const double (&R)[3] = E.X;
        v[0] = E.A[0];
        v[2] = E.A[1];
        v[4] = E.A[2];
        if ((R[0] < 1.e-06) && (R[1] < 1.e-06)) v[1] = (v[0] + v[2]) / 2.;
        else v[1] = (R[1] * (3. * v[0] + v[2]) + R[0] * (v[0] + 3. * v[2])) / (4. * (R[0] + R[1]));
        if ((R[1] < 1.e-06) && (R[2] < 1.e-06)) v[3] = (v[2] + v[4]) / 2.;
        else v[3] = (R[2] * (3. * v[2] + v[4]) + R[1] * (v[2] + 3. * v[4])) / (4. * (R[1] + R[2]));
        if ((R[2] < 1.e-06) && (R[0] < 1.e-06)) v[5] = (v[4] + v[0]) / 2.;
        else v[5] = (R[0] * (3. * v[4] + v[0]) + R[2] * (v[4] + 3. * v[0])) / (4. * (R[2] + R[0]));
        const double p = (b[1] * x + c[1] * y + a[1]) / da;
        const double q = (b[2] * x + c[2] * y + a[2]) / da;
        A = v[0] - p * (3. * v[0] - 4. * v[1] + v[2]) + 2. * p * p * (v[0] - 2. * v[1] + v[2]) -
            q * (3. * v[0] + v[4] - 4. * v[5]) + 2. * q * q * (v[0] + v[4] - 2. * v[5]) +
            4. * p * q * (v[0] - v[1] + v[3] - v[5]);
    }
    // FPProc::GetMu: the block's, divided by the element's AECF
    double cx = 0., cy = 0.;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        cx += E.X[j] / 3.;
        cy += E.Y[j] / 3.;
    }
    double mu1, mu2;
    mag_get_mu(M, bp, B1, B2, mu1, mu2);
    const double aecf = mag_aecf<AXI>(M, lab, cx, cy);
    mu1 /= aecf;
    mu2 /= aecf;
    double H1 = B1 / (mu1 * muo), H2 = B2 / (mu2 * muo);
    // the source current density
    double Js = bp.J_re;
    if (lab.ccase >= 0) {
        if (lab.ccase == 0) {
            if (!AXI) Js -= bp.Cduct * lab.dV;
            else {
                double R[3];
#pragma unroll
                for (int tn = 0; tn < 3; ++tn) {
                    R[tn] = E.X[tn];
                    if (R[tn] < 1.e-6) R[tn] = ravg;
                    else R[tn] *= M.lc;
                }
                ravg = 0.;
#pragma unroll
                for (int tn = 0; tn < 3; ++tn) ravg += (1. / R[tn]) * (a[tn] + b[tn] * x + c[tn] * y) / (da);
                Js -= bp.Cduct * lab.dV * ravg;
            }
        } else Js += lab.J;
    }
    double En = mag_do_energy<false>(M, bp, B1, B2);
    double Hcr = 0, Hci = 0;
    // the second-quadrant representation of a (linear) permanent magnet
    if (bp.H_c != 0) {
        Hcr = bp.H_c * lab.cos_m;
        Hci = bp.H_c * lab.sin_m;
        H1 = H1 - Hcr;
        H2 = H2 - Hci;
        En = 0.5 * muo * (mu1 * H1 * H1 + mu2 * H2 * H2);
    }
    o[0] = A;
    o[1] = B1;
    o[2] = B2;
    o[3] = mu1;
    o[4] = mu2;
    o[5] = H1;
    o[6] = H2;
    o[7] = Js;
    o[8] = bp.Cduct;
    o[9] = En;
    o[10] = Hcr;
    o[11] = Hci;
    o[12] = lab.wound ? 1. : -1.;
}

// GetPointValues of n points: the lowest-numbered element containing each
// (-1: none, its values NaN; given: elem[t] names it on entry), then
// kMagPointVals values per point
template <bool AXI>
__global__ void __launch_bounds__(kBlock) k_mag_points(int n, int NE, MagArgs M, PpGrid G, PpLists L,
                                                       const double *__restrict__ px, const double *__restrict__ py,
                                                       int smooth, const double *__restrict__ B,
                                                       const double *__restrict__ bc, int *__restrict__ elem,
                                                       double *__restrict__ out, int given)
{
    const int t = blockIdx.x * kBlock + threadIdx.x;
    if (t >= n) return;
    const double x = px[t], y = py[t];
    int nt = 0;
    const int k = given ? elem[t] : pp_find(M.x, M.y, M.p, G, L, x, y, nt);
    elem[t] = k;
    double v[kMagPointVals];
    if (k < 0) {
        const double nan = __longlong_as_double(0x7ff8000000000000LL);
#pragma unroll
        for (int c = 0; c < kMagPointVals; ++c) v[c] = nan;
    } else {
        mag_values_at<AXI>(M, NE, k, x, y, smooth, B, bc, v);
    }
    double *o = out + kMagPointVals * (size_t)t;
#pragma unroll
    for (int c = 0; c < kMagPointVals; ++c) o[c] = v[c];
}

// LineIntegral types 1, 3, 4 and 5: one thread per sample of a batch of
// contours, laid out as k_pp_contour's (xfk_postproc.hip): contour c holds the
// vertices cptr[c] .. cptr[c + 1) and owns the workgroups bptr[c] ..
// bptr[c + 1).  Per workgroup three sums into part: the integral's two, and
// the samples no element holds, which add nothing to the other two.
// dbg_xy, dbg_el (may be null; one contour only): every sample's point and element.
template <bool AXI>
__global__ void __launch_bounds__(kPotQBlock) k_mag_contour(int nc, int NE, MagArgs M, PpGrid G, PpLists L,
                                                            const int *__restrict__ cptr,
                                                            const int *__restrict__ bptr,
                                                            const double *__restrict__ cx,
                                                            const double *__restrict__ cy, int npts, int type,
                                                            int smooth, const double *__restrict__ B,
                                                            const double *__restrict__ bc,
                                                            double *__restrict__ part, double *__restrict__ dbg_xy,
                                                            int *__restrict__ dbg_el)
{
    // the contour of this workgroup: bptr[c] <= blockIdx.x < bptr[c + 1]
    int c = 0, hi = nc;
    while (hi - c > 1) {
        const int mid = (c + hi) >> 1;
        if (bptr[mid] <= (int)blockIdx.x) c = mid;
        else hi = mid;
    }
    const int v0 = cptr[c], nseg = cptr[c + 1] - v0 - 1;
    const int j = ((int)blockIdx.x - bptr[c]) * kPotQBlock + threadIdx.x;
    double v[3] = {0., 0., 0.};
    if (j < nseg * npts) {
        const int k = j / npts, i = j - k * npts;
        const double x0 = cx[v0 + k], y0 = cy[v0 + k], x1 = cx[v0 + k + 1], y1 = cy[v0 + k + 1];
        const double dx = x1 - x0, dy = y1 - y0;
        const double len = mag_cabs(dx, dy);
        const double dz = len / ((double)npts);
        const double u = (((double)i) + 0.5) / ((double)npts);
        double ptx = x0 + u * dx, pty = y0 + u * dy;
        const double tr = dx / len, ti = dy / len;
        // n = I * t, the complex product as the reference forms it
        const double nr = 0. * tr - 1. * ti, ni = 0. * ti + 1. * tr;
        ptx += nr * 1.e-06;
        pty += ni * 1.e-06;
        int nt;
        const int el = pp_find(M.x, M.y, M.p, G, L, ptx, pty, nt);
        if (dbg_xy) {
            dbg_xy[2 * (size_t)j] = ptx;
            dbg_xy[2 * (size_t)j + 1] = pty;
        }
        if (dbg_el) dbg_el[j] = el;
        if (el < 0) {
            v[2] = 1.;
        } else {
            double o[kMagPointVals];
            mag_values_at<AXI>(M, NE, el, ptx, pty, smooth, B, bc, o);
            const double B1 = o[1], B2 = o[2], H1 = o[5], H2 = o[6];
            if (type == 1) {
                const double Ht = tr * H1 + ti * H2;
                v[0] = (Ht * dz * M.lc);
            } else if (type == 5) {
                const double Bn = nr * B1 + ni * B2;
                // Ht * Ht.Conj() of a real number: its square less (0 * -0)
                v[0] = ((Bn * Bn - 0. * (-0.)) * dz * M.lc);
            } else {
                const double Hn = nr * H1 + ni * H2;
                const double Bn = nr * B1 + ni * B2;
                const double BH = B1 * H1 + B2 * H2;
                double dF1 = H1 * Bn + B1 * Hn - nr * BH;
                const double dF2 = H2 * Bn + B2 * Hn - ni * BH;
                if (type == 3) {
                    double dza = dz * M.lc;
                    if (AXI) {
                        dza *= 2. * kPI * ptx * M.lc;
                        dF1 = 0;
                    } else dza *= M.depth;
                    v[0] = (dF1 * dza / 2.);
                    v[1] = (dF2 * dza / 2.);
                } else if (!AXI) {   // (type 4; on an axisymmetric problem 0)
                    const double dT = ptx * dF2 - dF1 * pty;
                    const double dza = dz * M.lc * M.lc;
                    v[0] = (dT * dza * M.depth / 2.);
                }
            }
        }
    }
    block_sums<3>(v, part);
}

// A as xfk_get_solution gives it: V c, then (x 0.01 2 PI) on an axisymmetric problem
static __global__ void k_mag_a(int N, int axi, const double *__restrict__ V, const double *__restrict__ xcm,
                               double *__restrict__ A)
{
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= N) return;
    double a = V[i] * kC;
    if (axi) a *= (xcm[i] * 0.01 * 2 * kPI);
    A[i] = a;
}

// The problem kinds this post-processor answers; every other is refused with
// its name (post_entry: xfk_post.h)
template <class F>
static int mag_entry(xfk_problem *P, F &&body)
{
    return post_entry(P, [&]() -> int {
        XFK_REQUIRE(P, XFK_ERR_ARG, "null problem");
        XFK_REQUIRE(!P->electro && !P->heat, XFK_ERR_ARG,
                    "not a magnetics problem: xfk_mag_* post-processes magnetostatic problems (xfk_pot_* is for "
                    "electrostatic and heat-flow problems)");
        XFK_REQUIRE(!P->harmonic, XFK_ERR_UNSUPPORTED,
                    "harmonic problem: magnetics post-processing is built for magnetostatic problems only "
                    "(Frequency 0)");
        XFK_REQUIRE(!P->comm, XFK_ERR_UNSUPPORTED,
                    "sharded problem: magnetics post-processing needs the whole mesh on one device");
        return XFK_OK;
    }, body);
}

// (coordinates in user units, once: mag_prepare_xy of xfk_magpost.h)
// ... and A of the solution in V (after a solve)
static int mag_prepare(xfk_problem *P)
{
    hipStream_t s = P->stream;
    const int N = P->N, G = (N + kBlock - 1) / kBlock;
    const int rc = mag_prepare_xy(P);
    if (rc != XFK_OK) return rc;
    if (!P->mag_A_ready) {
        XFK_REQUIRE(P->symbolic_ready && P->V.p, XFK_ERR_ARG,
                    "no solution yet (solve the problem or xfk_mag_set_solution)");
        XFK_CHECK(P->mag_A.alloc((size_t)N));
        k_mag_a<<<G, kBlock, 0, s>>>(N, P->axi ? 1 : 0, P->V.p, P->x.p, P->mag_A.p);
        XFK_CHECK(hipGetLastError());
        P->mag_A_ready = true;
        P->mag_B_ready = P->mag_corner_ready = false;
    }
    return XFK_OK;
}

static MagArgs mag_args(const xfk_problem *P)
{
    MagArgs M = mag_mesh_args(P);
    M.labels = reinterpret_cast<const MagLabel *>(P->mag_lab.p);
    M.blocks = P->blocks.p;
    M.bhB = P->bhB.p;
    M.bhH = P->bhH.p;
    M.bhS = P->bhS.p;
    return M;
}

// The per-label table of a selection: the label's block, direction and flags
// from the problem's tables, its circuit's Case / J / dVolts from the solve's
// circuit results -- the columns FSolver writes to the .ans label lines
// (WriteStatic2D) and fpproc reads back (fpproc.cpp:1289-1308).  With energy
// set, refuses a selected label whose energy this post-processor does not
// compute (types 18-23 read B and the mask alone: their callers clear it).
// whole: every label counts as selected and the refusals name the problem
// (point values and contour integrals: sel is not read).
static int mag_labels(xfk_problem *P, const unsigned char *sel, bool energy = true, bool whole = false)
{
    hipStream_t s = P->stream;
    const size_t nlab = P->mag_hlab.size();
    std::vector<DevCirc> circ(std::max(1, P->ncircs));
    if (P->ncircs > 0) XFK_CHECK(d2h(circ.data(), P->circs.p, sizeof(DevCirc) * P->ncircs, s));
    std::vector<MagLabel> t(std::max<size_t>(1, nlab), MagLabel{});
    for (size_t k = 0; k < nlab; ++k) {
        const DevLabel &L = P->mag_hlab[k];
        const DevBlock &B = P->mag_hblk[L.blk];
        MagLabel &o = t[k];
        o.blk = L.blk;
        o.cos_m = L.cos_m;
        o.sin_m = L.sin_m;
        o.wound = L.is_wound ? 1 : 0;
        o.external = L.external ? 1 : 0;
        o.sel = (whole || sel[P->mag_lab_orig[k]]) ? 1 : 0;
        o.ccase = -1;
        if (L.in_circuit >= 0 && L.in_circuit < P->ncircs) {
            const DevCirc &C = circ[L.in_circuit];
            o.ccase = C.ccase;
            if (C.ccase == 0) o.dV = C.dV;
            else o.J = C.J;
        }
        if (!o.sel || !energy) continue;
        XFK_REQUIRE(B.LamType <= 2, XFK_ERR_UNSUPPORTED,
                    whole ? "the problem holds a label whose block has LamType > 2 (a wound region with proximity "
                            "effects): its fill factor, conductivity and energy at a point need GetFillFactor, which "
                            "is not built"
                          : "a selected label's block has LamType > 2 (a wound region with proximity effects): its "
                            "energy needs the label's effective conductivity and fill factor (GetFillFactor), which "
                            "are not built");
        XFK_REQUIRE(!(B.H_c != 0 && B.BHpoints > 0), XFK_ERR_UNSUPPORTED,
                    whole ? "the problem holds a nonlinear permanent magnet (H_c != 0 with a B-H curve): its energy "
                            "at a point needs fpproc's shifted curve and Nrg, which are not built"
                          : "a selected label's block is a nonlinear permanent magnet (H_c != 0 with a B-H curve): "
                            "its energy needs fpproc's shifted curve and Nrg, which are not built");
    }
    XFK_CHECK(P->mag_lab.alloc(sizeof(MagLabel) * t.size()));
    XFK_CHECK(hipMemcpyAsync(P->mag_lab.p, t.data(), sizeof(MagLabel) * t.size(), hipMemcpyHostToDevice, s));
    XFK_CHECK(hipStreamSynchronize(s));   // (t leaves scope)
    return XFK_OK;
}

static int mag_launch_integrals(xfk_problem *P, const MagArgs &M)
{
    hipStream_t s = P->stream;
    const int NE = P->NE, G = (NE + kPotQBlock - 1) / kPotQBlock;
    double *part = P->mag_part.p, *sums = part + kMagSums * (size_t)G;
    if (P->axi) k_mag_integrands<true><<<G, kPotQBlock, 0, s>>>(NE, M, part);
    else k_mag_integrands<false><<<G, kPotQBlock, 0, s>>>(NE, M, part);
    k_pot_sum<kMagSums><<<1, kPotQBlock, 0, s>>>(G, part, sums);
    return hipGetLastError() == hipSuccess ? XFK_OK : XFK_ERR_HIP;
}

// --- the weighted stress tensor mask: host side --------------------------------

static const char *const kMagMaskInvalid =
    "The selected region is invalid. A valid selection\ncannot abut a region which is not free space.";

// The node -> element lists over the caller's numbering p (host), ascending:
// the reference's element order, fpproc's ConList -- once
static int mag_conlist(xfk_problem *P, const std::vector<int> &p)
{
    if (P->mag_n2e_ready) return XFK_OK;
    hipStream_t s = P->stream;
    std::vector<int> ptr, lst;
    node_elements(p.data(), P->N, P->NE, ptr, lst);
    XFK_CHECK(upload(P->mag_n2e_ptr, ptr.data(), ptr.size(), s));
    XFK_CHECK(upload(P->mag_n2e, lst.data(), lst.size(), s));
    XFK_CHECK(hipStreamSynchronize(s));   // (ptr and lst leave scope)
    P->mag_n2e_ready = true;
    return XFK_OK;
}

// What the mask reads of the mesh, once: the node -> element lists over the
// caller's numbering (ascending: the reference's element order), the exterior
// edges, the point marks, and the auxiliary problem over the same connectivity
// in user units
static int mag_mask_mesh(xfk_problem *P, double &ms_create)
{
    ms_create = 0.;
    if (P->mask_ext_ready && P->mask_aux) return XFK_OK;
    hipStream_t s = P->stream;
    const int N = P->N, NE = P->NE;
    std::vector<double> x(N), y(N);
    std::vector<int> p(3 * (size_t)NE), lbl(NE);
    XFK_CHECK(d2h(x.data(), P->mag_x.p, sizeof(double) * N, s));
    XFK_CHECK(d2h(y.data(), P->mag_y.p, sizeof(double) * N, s));
    XFK_CHECK(d2h(p.data(), P->p_raw.p, sizeof(int) * 3 * (size_t)NE, s));
    XFK_CHECK(d2h(lbl.data(), P->lbl_raw.p, sizeof(int) * NE, s));
    int rc = mag_conlist(P, p);
    if (rc == XFK_OK)
        rc = mask_mesh_marks(P, P->p_raw.p, P->mag_n2e_ptr.p, P->mag_n2e.p, P->mag_has_point.data());
    if (rc != XFK_OK) return rc;
    const auto t0 = std::chrono::steady_clock::now();
    const std::vector<PotLabel> lab(std::max<size_t>(1, P->mag_hlab.size()), PotLabel{0, 0});
    if ((rc = mask_aux_create(P, x, y, p, lbl, lab, P->length_units)) != XFK_OK) return rc;
    ms_create = wall_ms(t0);
    return XFK_OK;
}

// FPProc::MakeMask for the selection (one byte per label); max_area, one double
// per label, and not_air, one byte per block, may be null
static int mag_make_mask(xfk_problem *P, const unsigned char *sel, const double *max_area,
                         const unsigned char *not_air)
{
    XFK_REQUIRE(sel, XFK_ERR_ARG, "null selection mask (one byte per block label)");
    P->mask_ready = false;
    MaskInputs I = {};
    I.t_all = std::chrono::steady_clock::now();
    int rc = mag_prepare_xy(P);
    if (rc != XFK_OK) return rc;
    const size_t nlab = P->mag_hlab.size();
    if ((rc = mag_mask_mesh(P, I.ms_create)) != XFK_OK) return rc;

    // the air test per block and per label (makemask.cpp:108-132), the labels' MaxArea
    I.t_rules = std::chrono::steady_clock::now();
    std::vector<unsigned char> mlab(2 * std::max<size_t>(1, nlab), 0);
    std::vector<double> area(std::max<size_t>(1, nlab), 0.);
    for (size_t k = 0; k < nlab; ++k) {
        const DevLabel &L = P->mag_hlab[k];
        const DevBlock &B = P->mag_hblk[L.blk];
        int f = 0;
        if ((B.mu_x != 1) || (B.mu_y != 1)) f = 1;
        if (B.BHpoints != 0) f = 1;
        if (B.LamType != 0) f = 1;
        if (B.H_c != 0) f = 1;
        if (B.J_re != 0) f = 1;
        if (B.Cduct != 0) f = 1;
        if (not_air && not_air[L.blk]) f = 1;
        if (L.in_circuit >= 0) f = 1;
        mlab[2 * k] = sel[P->mag_lab_orig[k]] ? 1 : 0;
        mlab[2 * k + 1] = (unsigned char)f;
        if (max_area) area[k] = max_area[P->mag_lab_orig[k]];
    }
    I.x = P->mag_x.p;
    I.p = P->p_raw.p;
    I.lbl = P->lbl_raw.p;
    I.n2e_ptr = P->mag_n2e_ptr.p;
    I.n2e = P->mag_n2e.p;
    I.lflag = mlab.data();
    I.area = area.data();
    I.nentries = area.size();
    I.point = P->mag_has_point.data();
    I.sel = sel;
    I.nsel_labels = (size_t)P->mag_nlabels;
    I.invalid = kMagMaskInvalid;
    return mask_make(P, I);
}

// mag_part: the partials and sums of the mask-free integrals, then those of
// the weighted stress tensor ones
static size_t mag_part_size(int G) { return (kMagSums + kMagStressSums) * ((size_t)G + 1); }
static double *mag_stress_part(xfk_problem *P, int G) { return P->mag_part.p + kMagSums * ((size_t)G + 1); }

// the six sums of k_mag_stress over all elements, in a fixed order
static int mag_launch_stress(xfk_problem *P, const MagArgs &M)
{
    hipStream_t s = P->stream;
    const int NE = P->NE, G = (NE + kPotQBlock - 1) / kPotQBlock;
    double *part = mag_stress_part(P, G), *sums = part + kMagStressSums * (size_t)G;
    if (P->axi) k_mag_stress<true><<<G, kPotQBlock, 0, s>>>(NE, M, P->mask_msk.p, part);
    else k_mag_stress<false><<<G, kPotQBlock, 0, s>>>(NE, M, P->mask_msk.p, part);
    k_pot_sum<kMagStressSums><<<1, kPotQBlock, 0, s>>>(G, part, sums);
    return hipGetLastError() == hipSuccess ? XFK_OK : XFK_ERR_HIP;
}

// types 18-23 alone into w[6], of the selection whose mask P holds: whatever
// the selected labels' blocks are
static int mag_stress_integrals(xfk_problem *P, const unsigned char *sel, double *w)
{
    int rc = mag_labels(P, sel, false);
    if (rc == XFK_OK) rc = mag_prepare(P);
    if (rc != XFK_OK) return rc;
    const int G = (P->NE + kPotQBlock - 1) / kPotQBlock;
    XFK_CHECK(P->mag_part.alloc(mag_part_size(G)));
    if ((rc = mag_launch_stress(P, mag_args(P))) != XFK_OK) {
        set_error("block integral launch failed");
        return rc;
    }
    XFK_CHECK(d2h(w, mag_stress_part(P, G) + kMagStressSums * (size_t)G, sizeof(double) * kMagStressSums, P->stream));
    return XFK_OK;
}

// every type as (re, im) pairs indexed by inttype
static int mag_block_integrals(xfk_problem *P, const unsigned char *sel, double *out)
{
    XFK_REQUIRE(sel, XFK_ERR_ARG, "null selection mask (one byte per block label)");
    XFK_REQUIRE(out, XFK_ERR_ARG, "null output");
    int rc = mag_labels(P, sel);
    if (rc == XFK_OK) rc = mag_prepare(P);
    if (rc != XFK_OK) return rc;
    const int G = (P->NE + kPotQBlock - 1) / kPotQBlock;
    XFK_CHECK(P->mag_part.alloc(mag_part_size(G)));
    const bool stress = mask_matches(P, sel, (size_t)P->mag_nlabels);   // types 18-23: with the mask of this very selection
    const MagArgs M = mag_args(P);
    if ((rc = mag_launch_integrals(P, M)) != XFK_OK || (stress && (rc = mag_launch_stress(P, M)) != XFK_OK)) {
        set_error("block integral launch failed");
        return rc;
    }
    double h[kMagSums], w[kMagStressSums];
    XFK_CHECK(d2h(h, P->mag_part.p + kMagSums * (size_t)G, sizeof(h), P->stream));
    if (stress) XFK_CHECK(d2h(w, mag_stress_part(P, G) + kMagStressSums * (size_t)G, sizeof(w), P->stream));
    for (int k = 0; k < 2 * kMagTypes; ++k) out[k] = 0.;
    out[2 * 0] = h[MS_AJ];
    out[2 * 1] = h[MS_A];
    out[2 * 2] = h[MS_ENERGY];
    out[2 * 5] = h[MS_AREA];
    out[2 * 7] = h[MS_CURRENT];
    out[2 * 8] = h[MS_B1];
    out[2 * 9] = h[MS_B2];
    out[2 * 10] = h[MS_VOLUME];
    out[2 * 11] = h[MS_FX];
    out[2 * 12] = h[MS_FY];
    out[2 * 15] = h[MS_TORQUE];
    out[2 * 17] = h[MS_COENERGY];
    out[2 * 24] = h[MS_INERTIA];
    // the centroid: the two sums over BlockIntegral(5) (0 / 0 with nothing selected)
    out[2 * 25] = h[MS_CX] / h[MS_AREA];
    out[2 * 25 + 1] = h[MS_CY] / h[MS_AREA];
    for (int k = 0; stress && k < kMagStressSums; ++k) out[2 * (18 + k)] = w[k];
    return XFK_OK;
}

// --- point values and contour integrals: host side ------------------------------

// What the corner kernel and the search read of the mesh and the tables, once:
// ConList, the grid's dimensions, the labels' "same material" classes and the
// point currents
static int mag_point_tables(xfk_problem *P)
{
    int rc = mag_prepare_xy(P);
    if (rc != XFK_OK || P->mag_ctab_ready) return rc;
    hipStream_t s = P->stream;
    const int N = P->N, NE = P->NE;
    std::vector<double> x(N), y(N);
    std::vector<int> p(3 * (size_t)NE);
    XFK_CHECK(d2h(x.data(), P->mag_x.p, sizeof(double) * N, s));
    XFK_CHECK(d2h(y.data(), P->mag_y.p, sizeof(double) * N, s));
    XFK_CHECK(d2h(p.data(), P->p_raw.p, sizeof(int) * 3 * (size_t)NE, s));
    if ((rc = mag_conlist(P, p)) != XFK_OK) return rc;
    pp_grid_dims(P, x.data(), y.data(), N, NE);
    // the m++ test of fpproc.cpp:2725-2738 at Frequency 0: the same label, or
    // equal mu_x, mu_y, H_c and direction (the same block and direction is a
    // case of that).  A class is the first entry of the label table with these.
    const size_t nlab = P->mag_hlab.size();
    std::vector<int> clab(2 * std::max<size_t>(1, nlab), 0);
    // (keyed on the values' bits with -0 folded into 0, which == does; an entry
    // holding a NaN equals nothing, itself included, and is a class of its own)
    std::map<std::array<unsigned long long, 5>, int> first;
    for (size_t k = 0; k < nlab; ++k) {
        const DevLabel &L = P->mag_hlab[k];
        const DevBlock &B = P->mag_hblk[L.blk];
        const double v[5] = {B.mu_x, B.mu_y, B.H_c, L.cos_m, L.sin_m};
        std::array<unsigned long long, 5> key;
        bool nan = false;
        for (int j = 0; j < 5; ++j) {
            const double d = v[j] == 0 ? 0. : v[j];
            nan |= d != d;
            std::memcpy(&key[j], &d, sizeof(d));
        }
        clab[2 * k] = P->mag_lab_orig[k];
        clab[2 * k + 1] = nan ? (int)k : first.emplace(key, (int)k).first->second;
    }
    XFK_CHECK(upload(P->mag_clab, clab.data(), clab.size(), s));
    XFK_CHECK(upload(P->mag_pj, P->mag_point_j.data(), (size_t)N, s));
    XFK_CHECK(hipStreamSynchronize(s));   // (clab leaves scope)
    P->mag_ctab_ready = true;
    return XFK_OK;
}

static int mag_grid(xfk_problem *P)
{
    const int rc = mag_point_tables(P);
    return rc != XFK_OK ? rc : pp_grid_build(P, P->mag_x.p, P->mag_y.p, P->p_raw.p);
}

static int mag_launch_element_b(xfk_problem *P)
{
    const int NE = P->NE, G = (NE + kBlock - 1) / kBlock;
    const MagArgs M = mag_args(P);
    if (P->axi) k_mag_element_b<true><<<G, kBlock, 0, P->stream>>>(NE, M, P->mag_B.p, P->mag_B.p + NE);
    else k_mag_element_b<false><<<G, kBlock, 0, P->stream>>>(NE, M, P->mag_B.p, P->mag_B.p + NE);
    return hipGetLastError() == hipSuccess ? XFK_OK : XFK_ERR_HIP;
}

// the element flux density of the solution, kept with it
static int mag_fields(xfk_problem *P)
{
    int rc = mag_prepare(P);
    if (rc != XFK_OK || P->mag_B_ready) return rc;
    XFK_CHECK(P->mag_B.alloc(2 * (size_t)P->NE));
    if ((rc = mag_launch_element_b(P)) != XFK_OK) return rc;
    P->mag_B_ready = true;
    return XFK_OK;
}

static int mag_launch_corners(xfk_problem *P, unsigned char *branch)
{
    const int NE = P->NE, G = (int)((3 * (long long)NE + kBlock - 1) / kBlock);
    const MagArgs M = mag_args(P);
    const MagCornerArgs C = {P->mag_n2e_ptr.p, P->mag_n2e.p, P->mag_clab.p, P->mag_pj.p, P->mag_B.p, P->mag_B.p + NE};
    if (P->axi) k_mag_corner<true><<<G, kBlock, 0, P->stream>>>(NE, M, C, P->mag_bc.p, branch);
    else k_mag_corner<false><<<G, kBlock, 0, P->stream>>>(NE, M, C, P->mag_bc.p, branch);
    return hipGetLastError() == hipSuccess ? XFK_OK : XFK_ERR_HIP;
}

// ... and the smoothed corner values, made at the first smoothed request
static int mag_corners(xfk_problem *P)
{
    int rc = mag_fields(P);
    if (rc == XFK_OK) rc = mag_point_tables(P);
    if (rc != XFK_OK || P->mag_corner_ready) return rc;
    // (one thread per corner: 3 NE must fit the kernel's int index)
    XFK_REQUIRE(P->NE <= 0x7fffffff / 3, XFK_ERR_ARG, "too many elements for the corner kernel (3 x elements >= 2^31)");
    XFK_CHECK(P->mag_bc.alloc(6 * (size_t)P->NE));
    if ((rc = mag_launch_corners(P, nullptr)) != XFK_OK) return rc;
    P->mag_corner_ready = true;
    return XFK_OK;
}

// what every point or contour request starts with: the refusals for the whole
// problem and the per-label table (before any launch), then the fields
static int mag_point_ready(xfk_problem *P, int smooth, bool grid)
{
    int rc = mag_labels(P, nullptr, true, true);
    if (rc == XFK_OK) rc = smooth ? mag_corners(P) : mag_fields(P);
    if (rc == XFK_OK && grid) rc = mag_grid(P);
    return rc;
}

static int mag_launch_points(xfk_problem *P, int n, int smooth, int given)
{
    const MagArgs M = mag_args(P);
    const PpGrid G = pp_grid_args(P);
    const PpLists L = pp_lists(P);
    const int g = (n + kBlock - 1) / kBlock;
    const double *px = P->pp_pts.p;
    double *o = P->pp_pts.p + 2 * (size_t)n;
    if (P->axi)
        k_mag_points<true><<<g, kBlock, 0, P->stream>>>(n, P->NE, M, G, L, px, px + n, smooth ? 1 : 0, P->mag_B.p,
                                                        P->mag_bc.p, P->pp_pel.p, o, given);
    else
        k_mag_points<false><<<g, kBlock, 0, P->stream>>>(n, P->NE, M, G, L, px, px + n, smooth ? 1 : 0, P->mag_B.p,
                                                         P->mag_bc.p, P->pp_pel.p, o, given);
    return hipGetLastError() == hipSuccess ? XFK_OK : XFK_ERR_HIP;
}

static int mag_contour_check(const xfk_problem *, int nc, const int *ptr, const double *x, const double *y, int type)
{
    XFK_REQUIRE(type >= 0 && type <= 5, XFK_ERR_ARG, "line integral type out of range: a magnetostatic problem has types 0-5");
    return pp_contour_check(nc, ptr, x, y);
}

// types 1, 3, 4, 5: the batch on the device, the fields and the grid ready
static int mag_contour_prepare(xfk_problem *P, int nc, const int *ptr, const double *x, const double *y, int type,
                               int smooth, int npts, PpContours &J)
{
    int rc = mag_point_ready(P, smooth, true);
    if (rc == XFK_OK) rc = pp_contour_layout(P, nc, ptr, x, y, type, smooth, npts, J);
    return rc;
}

static int mag_contour_launch(xfk_problem *P, PpContours &J, double *dbg_xy, int *dbg_el)
{
    const MagArgs M = mag_args(P);
    const PpGrid G = pp_grid_args(P);
    const PpLists L = pp_lists(P);
    hipStream_t s = P->stream;
    const double *cx = J.d_xy.p, *cy = cx + J.cptr[J.nc];
    if (P->axi)
        k_mag_contour<true><<<J.groups(), kPotQBlock, 0, s>>>(J.nc, P->NE, M, G, L, J.d_cptr.p, J.d_bptr.p, cx, cy,
                                                              J.npts, J.type, J.smooth, P->mag_B.p, P->mag_bc.p,
                                                              J.part.p, dbg_xy, dbg_el);
    else
        k_mag_contour<false><<<J.groups(), kPotQBlock, 0, s>>>(J.nc, P->NE, M, G, L, J.d_cptr.p, J.d_bptr.p, cx, cy,
                                                               J.npts, J.type, J.smooth, P->mag_B.p, P->mag_bc.p,
                                                               J.part.p, dbg_xy, dbg_el);
    launch_contour_sum(s, J);
    XFK_CHECK(hipGetLastError());
    return XFK_OK;
}

// the contour's length in metres, and on an axisymmetric problem its swept area (fpproc.cpp:4119-4130, 4200-4213)
static void mag_contour_length(const xfk_problem *P, int n, const double *x, const double *y, double &len, double &area)
{
    const double lc = kMagLengthConv[P->length_units];
    polyline_sums(n, x, y, P->axi, len, area);
    len *= lc;
    if (P->axi) area *= std::pow(lc, 2.);
}

// LineIntegral type 0: A at the two end points through the point kernel, then the reference's arithmetic
static int mag_contour_ends(xfk_problem *P, int nc, const int *ptr, const double *x, const double *y, double *out,
                            int *missed)
{
    int rc = mag_point_ready(P, 0, true);
    if (rc != XFK_OK) return rc;
    const int n = 2 * nc;
    std::vector<double> ex, ey, val(kMagPointVals * (size_t)n);
    contour_end_points(nc, ptr, x, y, ex, ey);
    if ((rc = upload_points(P, n, ex.data(), ey.data(), kMagPointVals)) != XFK_OK) return rc;
    if ((rc = mag_launch_points(P, n, 0, 0)) != XFK_OK) return rc;
    std::vector<int> el(n);
    XFK_CHECK(d2h(el.data(), P->pp_pel.p, sizeof(int) * (size_t)n, P->stream));
    XFK_CHECK(d2h(val.data(), P->pp_pts.p + 2 * (size_t)n, sizeof(double) * val.size(), P->stream));
    for (int c = 0; c < nc; ++c) {
        const double a0 = val[kMagPointVals * (size_t)(2 * c)], a1 = val[kMagPointVals * (size_t)(2 * c + 1)];
        double l, area;
        mag_contour_length(P, ptr[c + 1] - ptr[c], x + ptr[c], y + ptr[c], l, area);
        double z0, z1 = 0.;
        if (!P->axi) {
            z0 = (a0 - a1) * P->mag_depth;
            if (l != 0) z1 = z0 / (l * P->mag_depth);
        } else {
            z0 = a1 - a0;
            if (area != 0) z1 = z0 / area;
        }
        out[2 * c] = z0;
        out[2 * c + 1] = z1;
        if (missed) missed[c] = (el[2 * c] < 0) + (el[2 * c + 1] < 0);
    }
    return XFK_OK;
}

static int mag_line_integrals(xfk_problem *P, int nc, const int *ptr, const double *x, const double *y, int type,
                              int smooth, int npts, double *out, int *missed)
{
    int rc = mag_contour_check(P, nc, ptr, x, y, type);
    if (rc != XFK_OK || nc == 0) return rc;
    XFK_REQUIRE(out, XFK_ERR_ARG, "null output");
    if (type == 0) return mag_contour_ends(P, nc, ptr, x, y, out, missed);
    if (type == 2) {
        for (int c = 0; c < nc; ++c) {
            double l, area;
            mag_contour_length(P, ptr[c + 1] - ptr[c], x + ptr[c], y + ptr[c], l, area);
            out[2 * c] = l;
            out[2 * c + 1] = P->axi ? area : l * P->mag_depth;
            if (missed) missed[c] = 0;
        }
        return XFK_OK;
    }
    PpContours J;
    if ((rc = mag_contour_prepare(P, nc, ptr, x, y, type, smooth, npts, J)) != XFK_OK) return rc;
    if ((rc = mag_contour_launch(P, J, nullptr, nullptr)) != XFK_OK) return rc;
    std::vector<double> sums(3 * (size_t)nc);
    XFK_CHECK(d2h(sums.data(), J.sums(), sizeof(double) * sums.size(), P->stream));
    for (int c = 0; c < nc; ++c) {
        double r0 = sums[3 * (size_t)c], r1 = sums[3 * (size_t)c + 1];
        // the averages of types 1 and 5, divided after the loop as the reference does
        if (type == 1 || type == 5) {
            double l, area;
            mag_contour_length(P, ptr[c + 1] - ptr[c], x + ptr[c], y + ptr[c], l, area);
            r1 = 0.;
            if (l != 0) r1 = r0 / l;
        }
        out[2 * c] = r0;
        out[2 * c + 1] = r1;
        if (missed) missed[c] = (int)sums[3 * (size_t)c + 2];
    }
    return XFK_OK;
}

}  // namespace xfk

using namespace xfk;

extern "C" {

int xfk_mag_set_solution(xfk_problem *P, const double *A)
{
    return mag_entry(P, [&]() -> int {
        XFK_REQUIRE(A, XFK_ERR_ARG, "null solution");
        P->mag_A_ready = false;
        P->mag_B_ready = P->mag_corner_ready = false;
        P->mask_ready = false;   // (the reference clears bHasMask with a new solution)
        XFK_CHECK(P->mag_A.alloc((size_t)P->N));
        XFK_CHECK(hipMemcpyAsync(P->mag_A.p, A, sizeof(double) * P->N, hipMemcpyHostToDevice, P->stream));
        XFK_CHECK(hipStreamSynchronize(P->stream));
        P->mag_A_ready = true;
        return XFK_OK;
    });
}

int xfk_mag_set_depth(xfk_problem *P, double depth)
{
    // (a time-harmonic problem too: xfk_mag_ac_* reads the same Depth; nothing is launched)
    XFK_REQUIRE(P, XFK_ERR_ARG, "null problem");
    XFK_REQUIRE(!P->electro && !P->heat, XFK_ERR_ARG,
                "not a magnetics problem: xfk_mag_set_depth sets the depth of a magnetics problem");
    XFK_REQUIRE(!P->comm, XFK_ERR_UNSUPPORTED,
                "sharded problem: magnetics post-processing needs the whole mesh on one device");
    XFK_REQUIRE(depth > 0 || depth == -1, XFK_ERR_ARG,
                "depth must be positive (length units), or -1 for the reference's default of 1 m");
    // fpproc.cpp:1618-1619
    P->mag_depth = depth == -1 ? 1. : depth * kMagLengthConv[P->length_units];
    return XFK_OK;
}

int xfk_mag_element_b(xfk_problem *P, double *B1, double *B2)
{
    return mag_entry(P, [&]() -> int {
        int rc = mag_prepare(P);
        if (rc != XFK_OK) return rc;
        const int NE = P->NE;
        XFK_CHECK(P->mag_B.alloc(2 * (size_t)NE));
        const MagArgs M = mag_args(P);
        const int G = (NE + kBlock - 1) / kBlock;
        if (P->axi) k_mag_element_b<true><<<G, kBlock, 0, P->stream>>>(NE, M, P->mag_B.p, P->mag_B.p + NE);
        else k_mag_element_b<false><<<G, kBlock, 0, P->stream>>>(NE, M, P->mag_B.p, P->mag_B.p + NE);
        XFK_CHECK(hipGetLastError());
        P->mag_B_ready = true;
        if (B1) XFK_CHECK(d2h(B1, P->mag_B.p, sizeof(double) * (size_t)NE, P->stream));
        if (B2) XFK_CHECK(d2h(B2, P->mag_B.p + NE, sizeof(double) * (size_t)NE, P->stream));
        XFK_CHECK(hipStreamSynchronize(P->stream));
        return XFK_OK;
    });
}

int xfk_mag_block_integrals(xfk_problem *P, const unsigned char *label_selected, double *out)
{
    return mag_entry(P, [&]() -> int { return mag_block_integrals(P, label_selected, out); });
}

int xfk_mag_block_integral(xfk_problem *P, const unsigned char *label_selected, int type, double *out2)
{
    return mag_entry(P, [&]() -> int {
        XFK_REQUIRE(type >= 0 && type < kMagTypes, XFK_ERR_ARG, "block integral type out of range (0-25)");
        XFK_REQUIRE(type < 18 || type > 23 || mask_matches(P, label_selected, (size_t)P->mag_nlabels), XFK_ERR_ARG,
                    "block integral types 18-23 (weighted stress tensor force and torque) need the mask of this "
                    "very selection: xfk_mag_make_mask");
        XFK_REQUIRE(out2, XFK_ERR_ARG, "null output");
        if (type >= 18 && type <= 23) {
            double w[kMagStressSums];
            const int rc = mag_stress_integrals(P, label_selected, w);
            if (rc != XFK_OK) return rc;
            out2[0] = w[type - 18];
            out2[1] = 0.;
            return XFK_OK;
        }
        double o[2 * kMagTypes];
        const int rc = mag_block_integrals(P, label_selected, o);
        if (rc != XFK_OK) return rc;
        out2[0] = o[2 * type];
        out2[1] = o[2 * type + 1];
        return XFK_OK;
    });
}

int xfk_mag_time(xfk_problem *P, int repeats, double *ms)
{
    return mag_entry(P, [&]() -> int {
        XFK_REQUIRE(repeats > 0 && ms, XFK_ERR_ARG, "xfk_mag_time needs repeats > 0 and its output");
        std::vector<unsigned char> sel(std::max(1, P->mag_nlabels), 1);
        int rc = mag_labels(P, sel.data());
        if (rc == XFK_OK) rc = mag_prepare(P);
        if (rc != XFK_OK) return rc;
        hipStream_t s = P->stream;
        const int NE = P->NE, G = (NE + kPotQBlock - 1) / kPotQBlock, GB = (NE + kBlock - 1) / kBlock;
        XFK_CHECK(P->mag_part.alloc(mag_part_size(G)));
        XFK_CHECK(P->mag_B.alloc(2 * (size_t)NE));
        const MagArgs M = mag_args(P);
        auto timed = [&](auto f, double &out) { return timed_median(s, repeats, f, out); };
        rc = timed([&] {
            if (P->axi) k_mag_element_b<true><<<GB, kBlock, 0, s>>>(NE, M, P->mag_B.p, P->mag_B.p + NE);
            else k_mag_element_b<false><<<GB, kBlock, 0, s>>>(NE, M, P->mag_B.p, P->mag_B.p + NE);
            return hipGetLastError() == hipSuccess ? XFK_OK : XFK_ERR_HIP;
        }, ms[0]);
        if (rc != XFK_OK) return rc;
        return timed([&] { return mag_launch_integrals(P, M); }, ms[1]);
    });
}

int xfk_mag_make_mask(xfk_problem *P, const unsigned char *label_selected, const double *label_max_area,
                      const unsigned char *block_not_air)
{
    return mag_entry(P, [&]() -> int { return mag_make_mask(P, label_selected, label_max_area, block_not_air); });
}

int xfk_mag_get_mask(xfk_problem *P, double *W, double *msk)
{
    return mag_entry(P, [&]() -> int {
        XFK_REQUIRE(P->mask_ready && P->mask_aux, XFK_ERR_ARG,
                    "no mask (xfk_mag_make_mask; a new solution drops the mask)");
        const size_t bytes = sizeof(double) * (size_t)P->N;
        if (W) XFK_CHECK(d2h(W, P->mask_aux->V.p, bytes, P->stream));
        if (msk) XFK_CHECK(d2h(msk, P->mask_msk.p, bytes, P->stream));
        return XFK_OK;
    });
}

int xfk_mag_mask_info(xfk_problem *P, double *out9)
{
    return mag_entry(P, [&]() -> int {
        XFK_REQUIRE(out9, XFK_ERR_ARG, "null output");
        out9[0] = P->mask_ready ? 1. : 0.;
        for (int k = 0; k < 8; ++k) out9[1 + k] = P->mask_info[k];
        return XFK_OK;
    });
}

int xfk_mag_mask_problem(xfk_problem *P, xfk_problem **aux)
{
    return mag_entry(P, [&]() -> int {
        XFK_REQUIRE(aux, XFK_ERR_ARG, "null output");
        XFK_REQUIRE(P->mask_aux && P->mask_aux->symbolic_ready, XFK_ERR_ARG, "no mask problem yet (xfk_mag_make_mask)");
        *aux = P->mask_aux;
        return XFK_OK;
    });
}

int xfk_mag_stress_time(xfk_problem *P, int repeats, double *ms)
{
    return mag_entry(P, [&]() -> int {
        XFK_REQUIRE(repeats > 0 && ms, XFK_ERR_ARG, "xfk_mag_stress_time needs repeats > 0 and its output");
        XFK_REQUIRE(P->mask_ready, XFK_ERR_ARG, "no mask (xfk_mag_make_mask; a new solution drops the mask)");
        int rc = mag_labels(P, P->mask_sel.data(), false);
        if (rc == XFK_OK) rc = mag_prepare(P);
        if (rc != XFK_OK) return rc;
        const int G = (P->NE + kPotQBlock - 1) / kPotQBlock;
        XFK_CHECK(P->mag_part.alloc(mag_part_size(G)));
        const MagArgs M = mag_args(P);
        return timed_median(P->stream, repeats, [&] { return mag_launch_stress(P, M); }, *ms);
    });
}

int xfk_mag_corner_b(xfk_problem *P, double *b)
{
    return mag_entry(P, [&]() -> int {
        XFK_REQUIRE(b, XFK_ERR_ARG, "null output");
        const int rc = mag_point_ready(P, 1, false);
        if (rc != XFK_OK) return rc;
        XFK_CHECK(d2h(b, P->mag_bc.p, sizeof(double) * 6 * (size_t)P->NE, P->stream));
        return XFK_OK;
    });
}

int xfk_mag_point_values(xfk_problem *P, int n, const double *x, const double *y, int smooth, int *elem, double *out)
{
    return mag_entry(P, [&]() -> int {
        XFK_REQUIRE(n >= 0, XFK_ERR_ARG, "negative number of points");
        if (n == 0) return XFK_OK;
        XFK_REQUIRE(x && y && elem && out, XFK_ERR_ARG, "null point arrays");
        int rc = mag_point_ready(P, smooth, true);
        if (rc == XFK_OK) rc = upload_points(P, n, x, y, kMagPointVals);
        if (rc == XFK_OK) rc = mag_launch_points(P, n, smooth, 0);
        if (rc != XFK_OK) return rc;
        XFK_CHECK(d2h(elem, P->pp_pel.p, sizeof(int) * (size_t)n, P->stream));
        XFK_CHECK(d2h(out, P->pp_pts.p + 2 * (size_t)n, sizeof(double) * kMagPointVals * (size_t)n, P->stream));
        return XFK_OK;
    });
}

int xfk_mag_point_values_at(xfk_problem *P, int n, const double *x, const double *y, const int *elem, int smooth,
                            double *out)
{
    return mag_entry(P, [&]() -> int {
        XFK_REQUIRE(n >= 0, XFK_ERR_ARG, "negative number of points");
        if (n == 0) return XFK_OK;
        XFK_REQUIRE(x && y && elem && out, XFK_ERR_ARG, "null point arrays");
        for (int i = 0; i < n; ++i)
            XFK_REQUIRE(elem[i] >= -1 && elem[i] < P->NE, XFK_ERR_ARG, "a point's element is outside the element range");
        int rc = mag_point_ready(P, smooth, false);
        if (rc == XFK_OK) rc = upload_points(P, n, x, y, kMagPointVals);
        if (rc != XFK_OK) return rc;
        XFK_CHECK(hipMemcpyAsync(P->pp_pel.p, elem, sizeof(int) * (size_t)n, hipMemcpyHostToDevice, P->stream));
        if ((rc = mag_launch_points(P, n, smooth, 1)) != XFK_OK) return rc;
        XFK_CHECK(d2h(out, P->pp_pts.p + 2 * (size_t)n, sizeof(double) * kMagPointVals * (size_t)n, P->stream));
        return XFK_OK;
    });
}

int xfk_mag_line_integrals(xfk_problem *P, int n_contours, const int *ptr, const double *x, const double *y, int type,
                           int smooth, int npts, double *out, int *missed)
{
    return mag_entry(P, [&]() -> int {
        return mag_line_integrals(P, n_contours, ptr, x, y, type, smooth, npts, out, missed);
    });
}

int xfk_mag_line_integral(xfk_problem *P, int n, const double *x, const double *y, int type, int smooth, int npts,
                          double *out2, int *missed)
{
    return mag_entry(P, [&]() -> int {
        XFK_REQUIRE(n >= 0, XFK_ERR_ARG, "negative number of contour points");
        const int ptr[2] = {0, n};
        return mag_line_integrals(P, 1, ptr, x, y, type, smooth, npts, out2, missed);
    });
}

int xfk_mag_contour_samples(xfk_problem *P, int n, const double *x, const double *y, int type, int npts, double *xy,
                            int *elem)
{
    return mag_entry(P, [&]() -> int {
        return contour_samples(P, n, x, y, type, npts, xy, elem, mag_contour_check, mag_contour_prepare,
                               mag_contour_launch);
    });
}

int xfk_mag_point_time(xfk_problem *P, int n, const double *x, const double *y, int repeats, double *ms4)
{
    return mag_entry(P, [&]() -> int {
        XFK_REQUIRE(n > 0 && x && y && repeats > 0 && ms4, XFK_ERR_ARG,
                    "xfk_mag_point_time needs points, repeats > 0 and its output");
        int rc = mag_point_ready(P, 1, true);
        if (rc != XFK_OK) return rc;
        if ((rc = timed_median(P->stream, repeats, [&] { return mag_launch_corners(P, nullptr); }, ms4[0])) != XFK_OK) return rc;
        rc = timed_median(P->stream, repeats, [&] {
            P->pp_grid_ready = false;
            return pp_grid_build(P, P->mag_x.p, P->mag_y.p, P->p_raw.p);
        }, ms4[1]);
        if (rc != XFK_OK) return rc;
        if ((rc = upload_points(P, n, x, y, kMagPointVals)) != XFK_OK) return rc;
        for (int smooth = 0; smooth < 2; ++smooth)
            if ((rc = timed_median(P->stream, repeats, [&] { return mag_launch_points(P, n, smooth, 0); }, ms4[2 + smooth])) != XFK_OK)
                return rc;
        return XFK_OK;
    });
}

int xfk_mag_contour_time(xfk_problem *P, int n_contours, const int *ptr, const double *x, const double *y, int type,
                         int smooth, int npts, int repeats, double *ms)
{
    return mag_entry(P, [&]() -> int {
        XFK_REQUIRE(repeats > 0 && ms && n_contours > 0, XFK_ERR_ARG,
                    "xfk_mag_contour_time needs contours, repeats > 0 and its output");
        return contour_time(P, n_contours, ptr, x, y, type, smooth, npts, repeats, ms, mag_contour_check,
                            mag_contour_prepare, mag_contour_launch);
    });
}

}  // extern "C"
