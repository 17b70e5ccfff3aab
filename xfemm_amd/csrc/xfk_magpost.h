// What the magnetics post-processors share: the magnetostatic one
// (xfk_magpost.hip) and the time-harmonic one (xfk_magpost_ac.hip) work on the
// same mesh in the problem's length units, with the same element geometry and
// the same fixed-order sums (block_sums, k_pot_sum: xfk_potential.h).
//
// Include after `#pragma clang fp contract(off)`: everything here is the
// reference's arithmetic, operation by operation, in double.
#pragma once

#include "xfk_potential.h"

namespace xfk {

// FPProc's LengthConv[]: user length units -> m; and the solver's: -> cm
static const double kMagLengthConv[] = {0.0254, 0.001, 0.01, 1., 2.54e-5, 1.e-6};
static const double kMagUnitCm[] = {2.54, 0.1, 1., 100., 0.00254, 1.e-04};

constexpr int kMagTypes = 26;   // inttype 0 .. 25

// What GetJA and the energy read of a block label: the circuit columns are
// the ones the .ans label lines carry (fpproc.cpp:1289-1308)
struct MagLabel {
    double J, dV;           // blocklist[lbl].J (Case 1), dVolts (Case 0)
    double cos_m, sin_m;    // exp(I PI magdir / 180)
    int blk;
    int ccase;              // blocklist[lbl].Case; -1: InCircuit < 0
    int wound;              // FillFactor > 0: no bulk conductivity
    int external;
    int sel;
    int pad;
};

struct MagArgs {
    const double *x, *y, *A;       // user length units; the .ans solution (harmonic: interleaved re, im)
    const int *p, *lbl;
    const MagLabel *labels;
    const DevBlock *blocks;
    const double *bhB, *bhH, *bhS;
    double lc, lc2;                // LengthConv[LengthUnits] and its pow(., 2.)
    double depth;                  // Depth in m
    double ext_ro, ext_ri, ext_zo; // user units
};

// abs(CComplex) (femmcomplex.cpp:749-757)
__device__ __forceinline__ double mag_cabs(double re, double im)
{
    if ((re == 0) && (im == 0)) return 0.;
    if (fabs(re) > fabs(im)) return fabs(re) * sqrt(1. + (im / re) * (im / re));
    return fabs(im) * sqrt(1. + (re / im) * (re / im));
}

// FPProc::GetElementB (fpproc.cpp:2970-3082), without the incremental columns.
// Every operation on A is a sum or a product with a real number, so a complex
// A goes through it one part at a time with the reference's bits.
template <bool AXI>
__device__ __forceinline__ void mag_element_b(double lc, const double (&X)[3], const double (&Y)[3],
                                              const double (&A)[3], double &B1, double &B2)
{
    double b[3], c[3];
    b[0] = Y[1] - Y[2];
    b[1] = Y[2] - Y[0];
    b[2] = Y[0] - Y[1];
    c[0] = X[2] - X[1];
    c[1] = X[0] - X[2];
    c[2] = X[1] - X[0];
    double da = (b[0] * c[1] - b[1] * c[0]);
    if (!AXI) {
        B1 = 0;
        B2 = 0;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            B1 += A[i] * c[i] / (da * lc);
            B2 -= A[i] * b[i] / (da * lc);
        }
        return;
    }
    double v[6], r = 0;
#pragma unroll
    for (int i = 0; i < 3; ++i) r += X[i] / 3.;
    v[0] = A[0];
    v[2] = A[1];
    v[4] = A[2];
    // mid-side values
    if ((X[0] < 1.e-06) && (X[1] < 1.e-06)) v[1] = (v[0] + v[2]) / 2.;
    else v[1] = (X[1] * (3. * v[0] + v[2]) + X[0] * (v[0] + 3. * v[2])) / (4. * (X[0] + X[1]));
    if ((X[1] < 1.e-06) && (X[2] < 1.e-06)) v[3] = (v[2] + v[4]) / 2.;
    else v[3] = (X[2] * (3. * v[2] + v[4]) + X[1] * (v[2] + 3. * v[4])) / (4. * (X[1] + X[2]));
    if ((X[2] < 1.e-06) && (X[0] < 1.e-06)) v[5] = (v[4] + v[0]) / 2.;
    else v[5] = (X[0] * (3. * v[4] + v[0]) + X[2] * (v[4] + 3. * v[0])) / (4. * (X[2] + X[0]));
    const double dp = (-v[0] + v[2] + 4. * v[3] - 4. * v[5]) / 3.;
    const double dq = (-v[0] - 4. * v[1] + 4. * v[3] + v[4]) / 3.;
    da *= 2. * kPI * r * lc * lc;
    B1 = -(c[1] * dp + c[2] * dq) / da;
    B2 = (b[1] * dp + b[2] * dq) / da;
}

// Ctr (fpproc.cpp:3426-3438): the centroid in user units
__device__ __forceinline__ void mag_ctr(const double (&X)[3], const double (&Y)[3], double &cx, double &cy)
{
    cx = 0.;
    cy = 0.;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        cx += X[j] / 3.;
        cy += Y[j] / 3.;
    }
}

// ElmArea (fpproc.cpp:3440-3468) times pow(LengthConv, 2.): the area in m^2
__device__ __forceinline__ double mag_area(const double (&X)[3], const double (&Y)[3], double lc2)
{
    const double b0 = Y[1] - Y[2], b1 = Y[2] - Y[0];
    const double c0 = X[2] - X[1], c1 = X[0] - X[2];
    return ((b0 * c1 - b1 * c0) / 2.) * lc2;
}

// AECF (fpproc.cpp:5286-5304) of an element with centroid (cx, cy)
template <bool AXI>
__device__ __forceinline__ double mag_aecf_of(double ext_ro, double ext_ri, double ext_zo, int external, double cx,
                                              double cy)
{
    if (!(AXI && external)) return 1.;
    const double q = mag_cabs(cx, cy - ext_zo);
    return (q * q * ext_ri) / (ext_ro * ext_ro * ext_ro);
}

// user-unit coordinates
// (static: a copy per translation unit that includes this header)
static __global__ void k_mag_xy(int N, const double *__restrict__ x, const double *__restrict__ y, double u,
                                double *__restrict__ mx, double *__restrict__ my)
{
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= N) return;
    mx[i] = x[i] / u;
    my[i] = y[i] / u;
}

// coordinates in user units (once)
static inline int mag_prepare_xy(xfk_problem *P)
{
    const int N = P->N, G = (N + kBlock - 1) / kBlock;
    if (P->mag_xy_ready) return XFK_OK;
    XFK_CHECK(P->mag_x.alloc((size_t)N));
    XFK_CHECK(P->mag_y.alloc((size_t)N));
    k_mag_xy<<<G, kBlock, 0, P->stream>>>(N, P->x.p, P->y.p, kMagUnitCm[P->length_units], P->mag_x.p, P->mag_y.p);
    XFK_CHECK(hipGetLastError());
    P->mag_xy_ready = true;
    return XFK_OK;
}

// what the kernels read of the mesh, the units and the exterior region
// (labels, blocks and the curves are the caller's)
static inline MagArgs mag_mesh_args(const xfk_problem *P)
{
    MagArgs M = {};
    M.x = P->mag_x.p;
    M.y = P->mag_y.p;
    M.A = P->mag_A.p;
    M.p = P->p_raw.p;
    M.lbl = P->lbl_raw.p;
    M.lc = kMagLengthConv[P->length_units];
    M.lc2 = std::pow(M.lc, 2.);
    M.depth = P->mag_depth;
    M.ext_ro = P->mag_ext_user[0];
    M.ext_ri = P->mag_ext_user[1];
    M.ext_zo = P->mag_ext_user[2];
    return M;
}

}  // namespace xfk
