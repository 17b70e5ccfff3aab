// Post-processing of the scalar-potential problems on the device: what the
// reference's epproc and hpproc compute from a solved electrostatic or
// heat-flow problem, for MI355X (gfx950).
//
//   element fields    getElementD (epproc.cpp:735-763, hpproc.cpp:368-395) and
//                     E(elem) (epproc.cpp:726, hpproc.cpp:851)
//   corner fields     getNodalD (PostProcessor.cpp:894-1092)
//   block integrals   blockIntegral types 0-4 (epproc.cpp:268-397,
//                     hpproc.cpp:584-646)
//   force and torque  HenrotteVector (PostProcessor.cpp:742-768) and
//                     blockIntegral types 5 and 6 (epproc.cpp:329-389) over the
//                     mask of makeMask (xfk_mask.hip; the air test is
//                     CSMaterialProp::isAir): electrostatics only
//   point values      InTriangleTest (PostProcessor.cpp:359-398), getPointD
//                     (1153-1188), getPointValues (epproc.cpp:434-469,
//                     hpproc.cpp:332-366) over a uniform cell grid
//   contour integrals lineIntegral (epproc.cpp:489-724, hpproc.cpp:648-800)
//                     over batches of contours, a thread per sample
//
// The post-processors work in the problem's own length units with
// LengthConv[] to metres; the solvers in mm (esolver) or m (hsolver).  The
// coordinates are therefore divided back by the solver's unit once (pp_x,
// pp_y) and everything below reads those.  All arithmetic is the reference's,
// operation by operation, in double, without contraction into fused
// multiply-adds.
#include "xfk_potential.h"

#include <chrono>
#include <cstring>

#pragma clang fp contract(off)

#include "xfk_ppsearch.h"

namespace xfk {

constexpr double kPpEo = 8.85418781762e-12;   // femmconstants.h:24
// PostProcessor's LengthConv[]: user length units -> m
static const double kPpLengthConv[] = {0.0254, 0.001, 0.01, 1., 2.54e-5, 1.e-6};
constexpr int kPpMaxList = 20;    // getNodalD's cap on the neighbour list (q[21] with the node itself)
// An element whose bounding box covers more cells than this goes on the
// oversize list every point tests: the fill then writes at most this many
// entries per element, whatever the mesh grading.  The cells are sized so
// that the mean element's box spans about 2 x 2 of them; 64 is a box of 8 x 8.
constexpr int kPpBigCells = 64;
constexpr int kPpMaxCellsPerAxis = 4096;
constexpr int kPpScanBlock = 1024;

struct PpArgs {
    const double *x, *y, *V;       // user length units; the solution
    const int *p, *lbl;
    const PotLabel *labels;
    const EsBlock *es;             // electrostatics
    const HfBlock *hf;             // heat flow
    const double *tkT, *tkK;
    int axi;
    double lc;                     // LengthConv[LengthUnits]
    double depth;                  // Depth in m
    double ext_ro, ext_ri, ext_zo; // user units
};

// PostProcessor::Ctr: the thirds summed in corner order
__device__ __forceinline__ void pp_ctr(const double (&X)[3], const double (&Y)[3], double &cx, double &cy)
{
    cx = 0.;
    cy = 0.;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        cx += X[j] / 3.;
        cy += Y[j] / 3.;
    }
}

// AECF(elem) (PostProcessor.cpp:865-878)
__device__ __forceinline__ double pp_aecf(const PpArgs &A, int external, double cx, double cy)
{
    if (!A.axi) return 1.;
    if (!external) return 1;
    const double r = pp_cabs(cx - 0., cy - A.ext_zo);
    return (r * r) / (A.ext_ro * A.ext_ri);
}

// AECF(elem, p) (PostProcessor.cpp:881-891)
__device__ __forceinline__ double pp_aecf_at(const PpArgs &A, int external, double cx, double cy, double px,
                                             double py)
{
    if (!A.axi) return 1.;
    if (!external) return 1;
    const double r = pp_cabs(px - 0., py - A.ext_zo);
    if (r == 0) return pp_aecf(A, external, cx, cy);
    return (r * r) / (A.ext_ro * A.ext_ri);
}

struct PpElem {
    int n[3];
    double X[3], Y[3], V[3];
    int lbl, blk, external;
};

__device__ __forceinline__ void pp_load(const PpArgs &A, int e, PpElem &E)
{
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        E.n[j] = A.p[3 * e + j];
        E.X[j] = A.x[E.n[j]];
        E.Y[j] = A.y[E.n[j]];
        E.V[j] = A.V[E.n[j]];
    }
    E.lbl = A.lbl[e];
    const PotLabel lab = A.labels[E.lbl];
    E.blk = lab.blk;
    E.external = lab.external;
}

// the element's mean conductivities: kn += GetK(T_node) / 3. in corner order
template <bool HEAT>
__device__ __forceinline__ void pp_mean_k(const PpArgs &A, const PpElem &E, double &knx, double &kny)
{
    knx = 0.;
    kny = 0.;
    if (HEAT) {
        const HfBlock bp = A.hf[E.blk];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            double kx, ky;
            hf_getk(bp, A.tkT, A.tkK, E.V[i], kx, ky);
            knx += kx / 3.;
            kny += ky / 3.;
        }
    }
}

// getElementD and E(elem) of one element
template <bool HEAT>
__device__ __forceinline__ void pp_element_fields(const PpArgs &A, const PpElem &E, double (&D)[2], double (&F)[2])
{
    double b[3], c[3];
    b[0] = E.Y[1] - E.Y[2]; b[1] = E.Y[2] - E.Y[0]; b[2] = E.Y[0] - E.Y[1];
    c[0] = E.X[2] - E.X[1]; c[1] = E.X[0] - E.X[2]; c[2] = E.X[1] - E.X[0];
    const double da = (b[0] * c[1] - b[1] * c[0]);
    double Ere = 0., Eim = 0.;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        Ere -= (E.V[i] * b[i]) / (da * A.lc);
        Eim -= (E.V[i] * c[i]) / (da * A.lc);
    }
    double cx, cy;
    pp_ctr(E.X, E.Y, cx, cy);
    const double aecf = pp_aecf(A, E.external, cx, cy);
    if (HEAT) {
        double knx, kny;
        pp_mean_k<true>(A, E, knx, kny);
        D[0] = (Ere * knx) / aecf;
        D[1] = (Eim * kny) / aecf;
        F[0] = (D[0] / knx) * aecf;
        F[1] = (D[1] / kny) * aecf;
    } else {
        const EsBlock bp = A.es[E.blk];
        D[0] = (kPpEo * (Ere * bp.ex)) / aecf;
        D[1] = (kPpEo * (Eim * bp.ey)) / aecf;
        F[0] = ((D[0] / bp.ex) / kPpEo) * aecf;
        F[1] = ((D[1] / bp.ey) / kPpEo) * aecf;
    }
}

template <bool HEAT>
__global__ void __launch_bounds__(kBlock) k_pp_element(int NE, PpArgs A, double *__restrict__ D,
                                                       double *__restrict__ Ef)
{
    const int e = blockIdx.x * kBlock + threadIdx.x;
    if (e >= NE) return;
    PpElem E;
    pp_load(A, e, E);
    double d[2], f[2];
    pp_element_fields<HEAT>(A, E, d, f);
    D[2 * e] = d[0];
    D[2 * e + 1] = d[1];
    Ef[2 * e] = f[0];
    Ef[2 * e + 1] = f[1];
}

// getNodalD: one thread per (element, corner).  branch (may be null): which
// case the corner took -- 0 nominal, 1-5 the punts in the reference's order,
// 6 det == 0.
template <bool HEAT>
__global__ void __launch_bounds__(kBlock) k_pp_corner(int NE, PpArgs A, const int *__restrict__ Q,
                                                      const int *__restrict__ n2e_ptr,
                                                      const int *__restrict__ n2e, const int *__restrict__ cls,
                                                      const double *__restrict__ D, double *__restrict__ d,
                                                      unsigned char *__restrict__ branch)
{
    const int t = blockIdx.x * kBlock + threadIdx.x;
    if (t >= 3 * NE) return;
    const int N = t / 3, i = t - 3 * N;
    const int j = A.p[3 * N + i];
    const int lblN = A.lbl[N];
    const PotLabel labN = A.labels[lblN];
    const int clsN = cls[labN.blk];
    const int l0 = n2e_ptr[j], num = n2e_ptr[j + 1] - l0;
    const int *con = n2e + l0;
    const int Qj = Q[j];
    int q[kPpMaxList + 1];
    int lf = -1, rt = -1, qn = 0, eos;
    for (eos = 0; eos < num; eos++)
        if (con[eos] == N) break;
    // (the element is in its own corner's list: eos < num)
    // scan ccw
    for (int k = 0, m = eos; k < num; k++) {
        const int n = con[m];
        if (cls[A.labels[A.lbl[n]].blk] != clsN) break;
        int nos;
        for (nos = 0; nos < 3; nos++)
            if (A.p[3 * n + nos] == j) break;
        if (nos == 3) break;
        nos--;
        if (nos < 0) nos = 2;
        const int pn = A.p[3 * n + nos];
        if (qn < kPpMaxList) q[qn++] = pn;
        if ((Qj != -2) && (Q[pn] != -2)) {
            rt = pn;
            break;
        }
        m++;
        if (m == num) m = 0;
    }
    // scan cw
    for (int k = 0, m = eos; k < num; k++) {
        const int n = con[m];
        if (cls[A.labels[A.lbl[n]].blk] != clsN) break;
        int nos;
        for (nos = 0; nos < 3; nos++)
            if (A.p[3 * n + nos] == j) break;
        if (nos == 3) break;
        nos++;
        if (nos > 2) nos = 0;
        const int pn = A.p[3 * n + nos];
        if (qn < kPpMaxList) q[qn++] = pn;
        if ((Qj != -2) && (Q[pn] != -2)) {
            lf = pn;
            break;
        }
        m--;
        if (m < 0) m = num - 1;
    }
    const double xj = A.x[j], yj = A.y[j];
    int br = 0;
    if ((lf == rt) && (rt != -1) && (Qj != -2)) br = 1;
    else if ((rt != -1) && (Qj != -2) && (lf == -1)) br = 2;
    else if ((lf != -1) && (Qj != -2) && (rt == -1)) br = 3;
    else if ((lf == -1) && (rt == -1) && (Qj != -2)) br = 4;
    else if ((lf != -1) && (rt != -1) && (Qj != -2)) {
        double xr = A.x[lf] - xj, xi_ = A.y[lf] - yj;
        double ab = pp_cabs(xr, xi_);
        xr /= ab;
        xi_ /= ab;
        double yr = xj - A.x[rt], yi_ = yj - A.y[rt];
        ab = pp_cabs(yr, yi_);
        yr /= ab;
        yi_ /= ab;
        // x / y (femmcomplex.cpp:456-474)
        double c, ir, ii_;
        if (fabs(yr) > fabs(yi_)) {
            c = yi_ / yr;
            ir = 1. / (yr * (1. + c * c));
            ii_ = (-c) * ir;
        } else {
            c = yr / yi_;
            ii_ = (-1.) / (yi_ * (1. + c * c));
            ir = (-c) * ii_;
        }
        const double zr = xr * ir - xi_ * ii_, zi = xr * ii_ + xi_ * ir;
        const double ang = ((zr == 0) && (zi == 0)) ? 0. : atan2(zi, zr);
        if (fabs(ang) > 10.0001 * kPI / 180.) br = 5;
    }
    double dr = D[2 * N], di = D[2 * N + 1];
    if (br == 0) {
        double xi = 0, yi = 0, ii = 0, xx = 0, xy = 0, yy = 0, iv = 0, xv = 0, yv = 0;
        q[qn++] = j;
        const double Vj = A.V[j];
        for (int k = 0; k < qn; k++) {
            const double dx = A.x[q[k]] - xj;
            const double dy = A.y[q[k]] - yj;
            const double dv = Vj - A.V[q[k]];
            ii += 1.;
            xi += dx;
            yi += dy;
            xx += dx * dx;
            xy += dx * dy;
            yy += dy * dy;
            iv += dv;
            xv += dx * dv;
            yv += dy * dv;
        }
        const double det = (-(ii * xy * xy) + 2 * xi * xy * yi - xx * yi * yi - xi * xi * yy + ii * xx * yy) * A.lc;
        if (det == 0) br = 6;
        else {
            const double Ex = (iv * xy * yi - xv * yi * yi - ii * xy * yv + xi * yi * yv - iv * xi * yy + ii * xv * yy) / det;
            const double Ey = (iv * xi * xy - ii * xv * xy + xi * xv * yi - iv * xx * yi - xi * xi * yv + ii * xx * yv) / det;
            if (HEAT) {
                double kx, ky;
                hf_getk(A.hf[labN.blk], A.tkT, A.tkK, Vj, kx, ky);
                dr = kx * Ex;
                di = ky * Ey;
            } else {
                const EsBlock bp = A.es[labN.blk];
                double X[3], Y[3], cx, cy;
#pragma unroll
                for (int v = 0; v < 3; ++v) {
                    X[v] = A.x[A.p[3 * N + v]];
                    Y[v] = A.y[A.p[3 * N + v]];
                }
                pp_ctr(X, Y, cx, cy);
                const double aecf = pp_aecf_at(A, labN.external, cx, cy, xj, yj);
                dr = (bp.ex * Ex * kPpEo) / aecf;
                di = (bp.ey * Ey * kPpEo) / aecf;
            }
        }
    }
    d[2 * t] = dr;
    d[2 * t + 1] = di;
    if (branch) branch[t] = (unsigned char)br;
}

// blockIntegral types 0-4 at once: per selected element area, volume, the
// energy (electrostatics) or volume-weighted T (heat flow), a D and a E(elem);
// the workgroup's seven sums into part
// the seven terms of element e (zeros when it is not selected or past the end)
template <bool HEAT>
__device__ __forceinline__ void pp_integral_terms(int e, int NE, const PpArgs &A, const unsigned char *__restrict__ sel,
                                                  const double *__restrict__ D, const double *__restrict__ Ef,
                                                  double lc2, double (&v)[7])
{
#pragma unroll
    for (int c = 0; c < 7; ++c) v[c] = 0.;
    if (e < NE && sel[A.lbl[e]]) {
        const int n[3] = {A.p[3 * e], A.p[3 * e + 1], A.p[3 * e + 2]};
        const double X[3] = {A.x[n[0]], A.x[n[1]], A.x[n[2]]}, Y[3] = {A.y[n[0]], A.y[n[1]], A.y[n[2]]};
        const double b0 = Y[1] - Y[2], b1 = Y[2] - Y[0], c0 = X[2] - X[1], c1 = X[0] - X[2];
        const double a = ((b0 * c1 - b1 * c0) / 2.) * lc2;
        double av = a;
        if (A.axi) {
            const double r0 = X[0] * A.lc, r1 = X[1] * A.lc, r2 = X[2] * A.lc;
            const double R = (r0 + r1 + r2) / 3.;
            av *= (2. * kPI * R);
        } else {
            av *= A.depth;
        }
        const double Dr = D[2 * e], Di = D[2 * e + 1], Er = Ef[2 * e], Ei = Ef[2 * e + 1];
        if (HEAT) {
            double T = 0;
#pragma unroll
            for (int k = 0; k < 3; ++k) T += A.V[n[k]] / 3.;
            v[0] = av * T;
        } else {
            v[0] = av * (Dr * Er - Di * (-Ei)) / 2.;
        }
        v[1] = a;
        v[2] = av;
        v[3] = av * Dr;
        v[4] = av * Di;
        v[5] = av * Er;
        v[6] = av * Ei;
    }
}

template <bool HEAT>
__global__ void __launch_bounds__(kPotQBlock) k_pp_integrals(int NE, PpArgs A, const unsigned char *__restrict__ sel,
                                                             const double *__restrict__ D,
                                                             const double *__restrict__ Ef, double lc2,
                                                             double *__restrict__ part)
{
    const int e = blockIdx.x * kPotQBlock + threadIdx.x;
    double v[7];
    pp_integral_terms<HEAT>(e, NE, A, sel, D, Ef, lc2, v);
    block_sums<7>(v, part);
}

// The same seven sums in the reference's order: element by element, one
// rounding per selected element (epproc.cpp:268-397, hpproc.cpp:584-646), so
// that a value on a tie of the reference's "%f" prints as the reference
// prints it.  One workgroup: tiles of kPotQBlock elements, each thread its
// element's terms into LDS, then seven threads add their column in element
// order (an unselected element adds an exact 0).  About 3 ns per element;
// for the file-based post-processors, not the hot path.
template <bool HEAT>
__global__ void __launch_bounds__(kPotQBlock) k_pp_integrals_seq(int NE, PpArgs A,
                                                                 const unsigned char *__restrict__ sel,
                                                                 const double *__restrict__ D,
                                                                 const double *__restrict__ Ef, double lc2,
                                                                 double *__restrict__ out)
{
    __shared__ double term[7][kPotQBlock];
    double s = 0.;
    for (int e0 = 0; e0 < NE; e0 += kPotQBlock) {
        double v[7];
        pp_integral_terms<HEAT>(e0 + (int)threadIdx.x, NE, A, sel, D, Ef, lc2, v);
#pragma unroll
        for (int c = 0; c < 7; ++c) term[c][threadIdx.x] = v[c];
        __syncthreads();
        if (threadIdx.x < 7) {
            const int n = min(kPotQBlock, NE - e0);
            for (int i = 0; i < n; ++i) s += term[threadIdx.x][i];
        }
        __syncthreads();
    }
    if (threadIdx.x < 7) out[threadIdx.x] = s;
}

// blockIntegral types 5 and 6 (epproc.cpp:329-389) with HenrotteVector
// (PostProcessor.cpp:742-768): one thread per element over all elements; per
// workgroup the sums of the x (planar) and y (z) force terms and of the torque
// term (planar) into part.  The reference's planar case 5 adds its x term to
// the imaginary part as well -- the y term of FEMM's own integral was lost
// when its three integrals were merged into two -- which is not restated: the
// y force is a F2 AECF, F2 as case 6 writes it.
__global__ void __launch_bounds__(kPotQBlock) k_pp_stress(int NE, PpArgs A, const double *__restrict__ msk,
                                                          const double *__restrict__ D, double lc2,
                                                          double *__restrict__ part)
{
    const int e = blockIdx.x * kPotQBlock + threadIdx.x;
    double v[3] = {0., 0., 0.};
    if (e < NE) {
        PpElem E;
        pp_load(A, e, E);
        double b[3], c[3];
        b[0] = E.Y[1] - E.Y[2]; b[1] = E.Y[2] - E.Y[0]; b[2] = E.Y[0] - E.Y[1];
        c[0] = E.X[2] - E.X[1]; c[1] = E.X[0] - E.X[2]; c[2] = E.X[1] - E.X[0];
        double a = ((b[0] * c[1] - b[1] * c[0]) / 2.) * lc2;
        if (A.axi) {
            const double r0 = E.X[0] * A.lc, r1 = E.X[1] * A.lc, r2 = E.X[2] * A.lc;
            const double R = (r0 + r1 + r2) / 3.;
            a *= (2. * kPI * R);
        } else {
            a *= A.depth;
        }
        const double B1 = D[2 * e], B2 = D[2 * e + 1];
        const double da = (b[0] * c[1] - b[1] * c[0]);
        double cr = 0., ci = 0.;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const double m = msk[E.n[i]];
            cr -= (m * b[i]) / (da * A.lc);
            ci -= (m * c[i]) / (da * A.lc);
        }
        double cx, cy;
        pp_ctr(E.X, E.Y, cx, cy);
        const double aecf = pp_aecf(A, E.external, cx, cy);
        const double F1 = (((B1 * B1) - (B2 * B2)) * cr + 2. * (B1 * B2) * ci) / (2. * kPpEo);
        const double F2 = (((B2 * B2) - (B1 * B1)) * ci + 2. * (B1 * B2) * cr) / (2. * kPpEo);
        if (!A.axi) v[0] = a * (F1 * aecf);
        v[1] = a * (F2 * aecf);
        if (!A.axi) {
            double tr = 0., ti = 0.;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                tr += (E.X[k] * A.lc) / 3.;
                ti += (E.Y[k] * A.lc) / 3.;
            }
            double y = tr * F2 - ti * F1;
            y *= aecf;
            v[2] = a * y;
        }
    }
    block_sums<3>(v, part);
}

// --- the cell grid ----------------------------------------------------------

// the cells an element's bounding box touches (the box widened by a hair, so
// a point the edge tests accept through rounding finds the element too)
__device__ __forceinline__ void pp_cells_of(const PpGrid &G, const double *__restrict__ x,
                                            const double *__restrict__ y, const int *__restrict__ p, int e,
                                            int &cx0, int &cx1, int &cy0, int &cy1)
{
    const double X[3] = {x[p[3 * e]], x[p[3 * e + 1]], x[p[3 * e + 2]]};
    const double Y[3] = {y[p[3 * e]], y[p[3 * e + 1]], y[p[3 * e + 2]]};
    const double xa = fmin(X[0], fmin(X[1], X[2])), xb = fmax(X[0], fmax(X[1], X[2]));
    const double ya = fmin(Y[0], fmin(Y[1], Y[2])), yb = fmax(Y[0], fmax(Y[1], Y[2]));
    const double ex = 1e-12 * fmax(fabs(xa), fabs(xb)), ey = 1e-12 * fmax(fabs(ya), fabs(yb));
    cx0 = pp_cell1(xa - ex, G.x0, G.ihx, G.nx);
    cx1 = pp_cell1(xb + ex, G.x0, G.ihx, G.nx);
    cy0 = pp_cell1(ya - ey, G.y0, G.ihy, G.ny);
    cy1 = pp_cell1(yb + ey, G.y0, G.ihy, G.ny);
}

// pass 0: count the elements per cell (and the oversize ones); pass 1: fill
// (cnt then counts up again from zero).  The order inside a list is whatever
// the atomics give: the search takes the lowest index, not the first hit.
template <int PASS>
__global__ void __launch_bounds__(kBlock) k_pp_grid(int NE, PpGrid G, const double *__restrict__ x,
                                                    const double *__restrict__ y, const int *__restrict__ p,
                                                    int *__restrict__ cnt, const int *__restrict__ ptr,
                                                    int *__restrict__ cell_el, int *__restrict__ nbig,
                                                    int *__restrict__ big)
{
    const int e = blockIdx.x * kBlock + threadIdx.x;
    if (e >= NE) return;
    int cx0, cx1, cy0, cy1;
    pp_cells_of(G, x, y, p, e, cx0, cx1, cy0, cy1);
    if ((long long)(cx1 - cx0 + 1) * (cy1 - cy0 + 1) > kPpBigCells) {
        const int k = atomicAdd(nbig, 1);
        if (PASS == 1) big[k] = e;
        return;
    }
    for (int cy = cy0; cy <= cy1; ++cy)
        for (int cx = cx0; cx <= cx1; ++cx) {
            const int c = cy * G.nx + cx;
            const int k = atomicAdd(&cnt[c], 1);
            if (PASS == 1) cell_el[ptr[c] + k] = e;
        }
}

// exclusive scan of cnt[0 .. n) into ptr[0 .. n], one workgroup: a contiguous
// run per thread, the runs' totals scanned in LDS
__global__ void __launch_bounds__(kPpScanBlock) k_pp_scan(int n, const int *__restrict__ cnt, int *__restrict__ ptr)
{
    __shared__ int tot[kPpScanBlock];
    const int per = (n + kPpScanBlock - 1) / kPpScanBlock;
    const int a = min(n, (int)threadIdx.x * per), b = min(n, a + per);
    int s = 0;
    for (int i = a; i < b; ++i) s += cnt[i];
    tot[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        int run = 0;
        for (int k = 0; k < kPpScanBlock; ++k) {
            const int v = tot[k];
            tot[k] = run;
            run += v;
        }
        ptr[n] = run;
    }
    __syncthreads();
    s = tot[threadIdx.x];
    for (int i = a; i < b; ++i) {
        ptr[i] = s;
        s += cnt[i];
    }
}

// getPointValues(x, y, k) (epproc.cpp:434-469, hpproc.cpp:332-366) with
// getPointD (PostProcessor.cpp:1153-1188): the 8 values of k_pp_points
template <bool HEAT>
__device__ __forceinline__ void pp_values_at(const PpArgs &A, int k, double x, double y, int smooth,
                                             const double *__restrict__ D, const double *__restrict__ dc,
                                             double (&o)[8])
{
    PpElem E;
    pp_load(A, k, E);
    double a[3], b[3], c[3];
    a[0] = E.X[1] * E.Y[2] - E.X[2] * E.Y[1];
    a[1] = E.X[2] * E.Y[0] - E.X[0] * E.Y[2];
    a[2] = E.X[0] * E.Y[1] - E.X[1] * E.Y[0];
    b[0] = E.Y[1] - E.Y[2]; b[1] = E.Y[2] - E.Y[0]; b[2] = E.Y[0] - E.Y[1];
    c[0] = E.X[2] - E.X[1]; c[1] = E.X[0] - E.X[2]; c[2] = E.X[1] - E.X[0];
    const double da = (b[0] * c[1] - b[1] * c[0]);
    double Dr, Di;
    if (!smooth) {
        Dr = D[2 * k];
        Di = D[2 * k + 1];
    } else {
        Dr = 0;
        Di = 0;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const double w = (a[i] + b[i] * x + c[i] * y);
            Dr += (dc[6 * k + 2 * i] * w) / da;
            Di += (dc[6 * k + 2 * i + 1] * w) / da;
        }
    }
    double V = 0;
#pragma unroll
    for (int i = 0; i < 3; ++i) V += E.V[i] * (a[i] + b[i] * x + c[i] * y) / (da);
    double cx, cy;
    pp_ctr(E.X, E.Y, cx, cy);
    const double aecf = pp_aecf_at(A, E.external, cx, cy, x, y);
    o[0] = V;
    o[1] = Dr;
    o[2] = Di;
    if (HEAT) {
        double kx, ky;
        hf_getk(A.hf[E.blk], A.tkT, A.tkK, V, kx, ky);
        kx /= aecf;
        ky /= aecf;
        o[3] = kx;
        o[4] = ky;
        o[5] = Dr / (kx);
        o[6] = Di / (ky);
        o[7] = 0.;
    } else {
        const EsBlock bp = A.es[E.blk];
        const double ex = bp.ex / aecf, ey = bp.ey / aecf;
        const double Er = Dr / (ex * kPpEo), Ei = Di / (ey * kPpEo);
        o[3] = Er;
        o[4] = Ei;
        o[5] = ex;
        o[6] = ey;
        o[7] = (Dr * Er - Di * (-Ei)) / 2.;
    }
}

// getPointValues of n points: the lowest-numbered element containing each
// (-1: none, its values NaN), then 8 values per point --
//   electrostatics: V, Dx, Dy, Ex, Ey, ex, ey, nrg
//   heat flow:      T, Fx, Fy, Kx, Ky, Gx, Gy, 0
template <bool HEAT>
__global__ void __launch_bounds__(kBlock) k_pp_points(int n, PpArgs A, PpGrid G, PpLists L,
                                                      const double *__restrict__ px,
                                                      const double *__restrict__ py, int smooth,
                                                      const double *__restrict__ D, const double *__restrict__ dc,
                                                      int *__restrict__ elem, double *__restrict__ out,
                                                      int *__restrict__ ntests, int given)
{
    const int t = blockIdx.x * kBlock + threadIdx.x;
    if (t >= n) return;
    const double x = px[t], y = py[t];
    int nt = 0;
    // given: elem[t] names the element on entry (checked by the host; -1: none)
    const int k = given ? elem[t] : pp_find(A.x, A.y, A.p, G, L, x, y, nt);
    // (diagnostics: the elements this point is tested against)
    if (ntests) ntests[t] = nt;
    double *o = out + 8 * (size_t)t;
    elem[t] = k;
    double v[8];
    if (k < 0) {
        const double nan = __longlong_as_double(0x7ff8000000000000LL);
#pragma unroll
        for (int c = 0; c < 8; ++c) v[c] = nan;
    } else {
        pp_values_at<HEAT>(A, k, x, y, smooth, D, dc, v);
    }
#pragma unroll
    for (int c = 0; c < 8; ++c) o[c] = v[c];
}

// lineIntegral types 1, 3 and 4 (epproc.cpp:508-572, 597-723) and 1 and 3
// of heat flow (hpproc.cpp:668-725, 746-797): one thread per sample of a batch
// of contours, the samples made here from the contours' vertices.  Contour c
// holds the vertices cptr[c] .. cptr[c + 1) of (cx, cy) and owns the workgroups
// bptr[c] .. bptr[c + 1), so a workgroup never straddles two contours and a
// contour's partials do not depend on its place in the batch.  Per workgroup
// three sums into part: the integral's two, and the samples no element holds
// (which add nothing to the other two, the reference's flag == false).  The
// element of a sample is the lowest-numbered containing one, as k_pp_points
// takes it; the reference walks from the previous sample's element.
// dbg_xy, dbg_el (may be null; one contour only): every sample's point and
// element.
template <bool HEAT>
__global__ void __launch_bounds__(kPotQBlock) k_pp_contour(int nc, PpArgs A, PpGrid G, PpLists L,
                                                           const int *__restrict__ cptr,
                                                           const int *__restrict__ bptr,
                                                           const double *__restrict__ cx,
                                                           const double *__restrict__ cy, int npts, int type,
                                                           int smooth, const double *__restrict__ D,
                                                           const double *__restrict__ dc,
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
        const double len = pp_cabs(dx, dy);
        const double dz = len / ((double)npts);
        const double u = (((double)i) + 0.5) / ((double)npts);
        double ptx = x0 + u * dx, pty = y0 + u * dy;
        const double tr = dx / len, ti = dy / len;
        // n = I * t, the complex product as the reference forms it
        const double nr = 0. * tr - 1. * ti, ni = 0. * ti + 1. * tr;
        if (!(HEAT && type == 3)) {
            ptx += nr * 1.e-06;
            pty += ni * 1.e-06;
        }
        int nt;
        const int el = pp_find(A.x, A.y, A.p, G, L, ptx, pty, nt);
        if (dbg_xy) {
            dbg_xy[2 * (size_t)j] = ptx;
            dbg_xy[2 * (size_t)j + 1] = pty;
        }
        if (dbg_el) dbg_el[j] = el;
        if (el < 0) {
            v[2] = 1.;
        } else {
            double o[8];
            pp_values_at<HEAT>(A, el, ptx, pty, smooth, D, dc, o);
            // 1 / n (femmcomplex.cpp:362-380)
            double q, yr, yi;
            if (fabs(nr) > fabs(ni)) {
                q = ni / nr;
                yr = 1. / (nr * (1. + q * q));
                yi = (-q) * yr;
            } else {
                q = nr / ni;
                yi = (-1.) / (ni * (1. + q * q));
                yr = (-q) * yi;
            }
            if (type == 1 || (HEAT && type == 3)) {
                double d;
                if (A.axi) d = 2. * kPI * ptx * (A.lc * A.lc);
                else d = A.depth * A.lc;
                if (type == 1) {
                    const double Dn = o[1] * yr - o[2] * yi;
                    v[0] = (Dn * dz * d);
                } else {
                    v[0] = (o[0] * dz * d);
                }
                v[1] = dz * d;
            } else if (!HEAT) {
                const double Dr = o[1], Di = o[2], Er = o[3], Ei = o[4];
                const double Hn = Er * yr - Ei * yi;
                const double Bn = Dr * yr - Di * yi;
                const double BH = Dr * Er - Di * (-Ei);
                double dF1 = Er * Bn + Dr * Hn - nr * BH;
                const double dF2 = Ei * Bn + Di * Hn - ni * BH;
                if (type == 3) {
                    double dza = dz * A.lc;
                    if (A.axi) {
                        dza *= 2. * kPI * ptx * A.lc;
                        dF1 = 0;
                    } else {
                        dza *= A.depth;
                    }
                    v[0] = (dF1 * dza / 2.);
                    v[1] = (dF2 * dza / 2.);
                } else if (!A.axi) {   // (type 4; on an axisymmetric problem 0, as block integral 6)
                    const double dT = ptx * dF2 - dF1 * pty;
                    const double dza = dz * (A.lc * A.lc);
                    v[0] = (dT * dza * A.depth / 2.);
                }
            }
        }
    }
    block_sums<3>(v, part);
}

// one workgroup per contour: its workgroups' partials strided per thread in a
// fixed order, then the workgroup's sums, into out[3 c .. 3 c + 3)
__global__ void __launch_bounds__(kPotQBlock) k_pp_contour_sum(const int *__restrict__ bptr,
                                                               const double *__restrict__ part,
                                                               double *__restrict__ out)
{
    const int b0 = bptr[blockIdx.x], g = bptr[blockIdx.x + 1] - b0;
    double s[3] = {0., 0., 0.};
    for (int i = threadIdx.x; i < g; i += kPotQBlock) {
#pragma unroll
        for (int c = 0; c < 3; ++c) s[c] += part[3 * (size_t)(b0 + i) + c];
    }
    block_sums<3>(s, out);
}

// --- plot bounds (OpenDocument, epproc.cpp:184-225, hpproc.cpp: its twin) -----
//
// Extremes of the potential over the nodes and of |D| and |E| (|F|, |G|) over
// the elements outside the external region, and the number of external
// elements, which names the reference's starting element.  Seven values per
// workgroup: min V, max V, min |D|, max |D|, min |E|, max |E|, the count.
// fmin / fmax drop a NaN as the reference's comparisons do, and neither
// depends on the order, so the shuffles and the fold give the same bits
// whatever the launch shape; the count is an exact sum of small integers.
constexpr int kPpBoundsBlock = 256;
constexpr int kPpBoundsK = 7;

// the workgroup's extremes and count (wave shuffles, then the waves in
// order) into out[7 wg .. 7 wg + 7); workgroups of kPpBoundsBlock threads
__device__ __forceinline__ void block_bounds(double (&v)[kPpBoundsK], double *__restrict__ out)
{
    __shared__ double red[kPpBoundsK * (kPpBoundsBlock / 64)];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
        for (int c = 0; c < 6; c += 2) {
            v[c] = fmin(v[c], __shfl_xor(v[c], off, 64));
            v[c + 1] = fmax(v[c + 1], __shfl_xor(v[c + 1], off, 64));
        }
        v[6] += __shfl_xor(v[6], off, 64);
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int c = 0; c < kPpBoundsK; ++c) red[kPpBoundsK * (threadIdx.x >> 6) + c] = v[c];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double s[kPpBoundsK];
#pragma unroll
        for (int c = 0; c < kPpBoundsK; ++c) s[c] = red[c];
        for (int w = 1; w < kPpBoundsBlock / 64; ++w) {
#pragma unroll
            for (int c = 0; c < 6; c += 2) {
                s[c] = fmin(s[c], red[kPpBoundsK * w + c]);
                s[c + 1] = fmax(s[c + 1], red[kPpBoundsK * w + c + 1]);
            }
            s[6] += red[kPpBoundsK * w + 6];
        }
#pragma unroll
        for (int c = 0; c < kPpBoundsK; ++c) out[kPpBoundsK * (size_t)blockIdx.x + c] = s[c];
    }
}

__device__ __forceinline__ void pp_bounds_neutral(double (&v)[kPpBoundsK])
{
    const double inf = __longlong_as_double(0x7ff0000000000000LL);
#pragma unroll
    for (int c = 0; c < 6; c += 2) {
        v[c] = inf;
        v[c + 1] = -inf;
    }
    v[6] = 0.;
}

// thread t: node t and element t, where they exist
__global__ void __launch_bounds__(kPpBoundsBlock) k_pp_bounds(int N, int NE, const double *__restrict__ V,
                                                              const int *__restrict__ lbl,
                                                              const PotLabel *__restrict__ labels,
                                                              const double *__restrict__ D,
                                                              const double *__restrict__ Ef,
                                                              double *__restrict__ part)
{
    const size_t t = (size_t)blockIdx.x * kPpBoundsBlock + threadIdx.x;
    double v[kPpBoundsK];
    pp_bounds_neutral(v);
    if (t < (size_t)N) {
        const double a = V[t];
        v[0] = fmin(v[0], a);
        v[1] = fmax(v[1], a);
    }
    if (t < (size_t)NE) {
        if (labels[lbl[t]].external) {
            v[6] = 1.;
        } else {
            const double d = pp_cabs(D[2 * t], D[2 * t + 1]), e = pp_cabs(Ef[2 * t], Ef[2 * t + 1]);
            v[2] = fmin(v[2], d);
            v[3] = fmax(v[3], d);
            v[4] = fmin(v[4], e);
            v[5] = fmax(v[5], e);
        }
    }
    block_bounds(v, part);
}

// G workgroups' partials, strided per thread, then the workgroup's; one workgroup
__global__ void __launch_bounds__(kPpBoundsBlock) k_pp_bounds_fold(int G, const double *__restrict__ part,
                                                                   double *__restrict__ out)
{
    double v[kPpBoundsK];
    pp_bounds_neutral(v);
    for (int i = threadIdx.x; i < G; i += kPpBoundsBlock) {
        const double *q = part + kPpBoundsK * (size_t)i;
#pragma unroll
        for (int c = 0; c < 6; c += 2) {
            v[c] = fmin(v[c], q[c]);
            v[c + 1] = fmax(v[c + 1], q[c + 1]);
        }
        v[6] += q[6];
    }
    block_bounds(v, out);
}

// --- host side ---------------------------------------------------------------

static PpArgs pp_args(xfk_problem *P)
{
    PpArgs A = {};
    A.x = P->pp_x.p;
    A.y = P->pp_y.p;
    A.V = P->V.p;
    A.p = P->pot_p.p;
    A.lbl = P->lbl_raw.p;
    A.labels = P->pot_labels.p;
    A.es = P->es_blocks.p;
    A.hf = P->hf_blocks.p;
    A.tkT = P->hf_tk_T.p;
    A.tkK = P->hf_tk_K.p;
    A.axi = P->axi ? 1 : 0;
    A.lc = kPpLengthConv[P->pot_length_units];
    // (epproc.cpp:104, hpproc.cpp:160: a depth of -1 means 1 m)
    A.depth = P->pot_depth_user == -1 ? 1 : P->pot_depth_user * A.lc;
    A.ext_ro = P->pot_ext_user[0];
    A.ext_ri = P->pot_ext_user[1];
    A.ext_zo = P->pot_ext_user[2];
    return A;
}

// The tables that depend on the mesh alone, built at the first
// post-processing call on the host and uploaded: coordinates in user units,
// the Q marks, the "same material" class of each block, and the node ->
// element lists of the mesh's own connectivity in the reference's order (a
// stable sort by arg(centroid - node) of lists built in element order: what
// the bubble sort of epproc.cpp:165-182 leaves).
static int pp_mesh(xfk_problem *P)
{
    if (P->pp_mesh_ready) return XFK_OK;
    hipStream_t s = P->stream;
    const int N = P->N, NE = P->NE;
    std::vector<double> x(N), y(N);
    std::vector<int> p(3 * (size_t)NE), lbl(NE);
    XFK_CHECK(d2h(x.data(), P->x.p, sizeof(double) * N, s));
    XFK_CHECK(d2h(y.data(), P->y.p, sizeof(double) * N, s));
    XFK_CHECK(d2h(p.data(), P->pot_p.p, sizeof(int) * 3 * (size_t)NE, s));
    XFK_CHECK(d2h(lbl.data(), P->lbl_raw.p, sizeof(int) * NE, s));
    const double u = P->pot_unit;
    for (int i = 0; i < N; ++i) {
        x[i] = x[i] / u;
        y[i] = y[i] / u;
    }
    std::vector<int> ptr, lst;
    node_elements(p.data(), N, NE, ptr, lst);
    std::atomic<bool> failed{false};   // (an exception must not leave a worker thread)
    host_par_for(N, 1 << 14, [&](long long a, long long b) {
      try {
        std::vector<std::pair<double, int>> tmp;
        for (long long i = a; i < b; ++i) {
            const int l0 = ptr[i], num = ptr[i + 1] - l0;
            tmp.resize(num);
            for (int k = 0; k < num; ++k) {
                const int e = lst[l0 + k];
                double cx = 0., cy = 0.;
                for (int j = 0; j < 3; ++j) {
                    cx += x[p[3 * (size_t)e + j]] / 3.;
                    cy += y[p[3 * (size_t)e + j]] / 3.;
                }
                const double ur = cx - x[i], ui = cy - y[i];
                tmp[k] = {((ur == 0) && (ui == 0)) ? 0. : std::atan2(ui, ur), e};
            }
            std::stable_sort(tmp.begin(), tmp.end(),
                             [](const std::pair<double, int> &l, const std::pair<double, int> &r) { return l.first < r.first; });
            for (int k = 0; k < num; ++k) lst[l0 + k] = tmp[k].second;
        }
      } catch (...) {
        failed = true;
      }
    });
    XFK_REQUIRE(!failed, XFK_ERR_ARG, "post-processing failed: out of host memory while sorting the node lists");
    // isSameMaterialAs (CMaterialProp.cpp:1490-1520, 1611-1618) is an
    // equivalence: a block's class is the first block it equals
    std::vector<int> cls;
    if (P->electro) {
        std::vector<EsBlock> blk(P->es_blocks.n);
        XFK_CHECK(d2h(blk.data(), P->es_blocks.p, sizeof(EsBlock) * blk.size(), s));
        cls.resize(blk.size());
        for (size_t a = 0; a < blk.size(); ++a) {
            cls[a] = (int)a;
            for (size_t b = 0; b < a; ++b)
                if (blk[a].ex == blk[b].ex && blk[a].ey == blk[b].ey) {
                    cls[a] = cls[b];
                    break;
                }
        }
    } else {
        std::vector<HfBlock> blk(P->hf_blocks.n);
        std::vector<double> tT(P->hf_tk_T.n), tK(P->hf_tk_K.n);
        XFK_CHECK(d2h(blk.data(), P->hf_blocks.p, sizeof(HfBlock) * blk.size(), s));
        XFK_CHECK(d2h(tT.data(), P->hf_tk_T.p, sizeof(double) * tT.size(), s));
        XFK_CHECK(d2h(tK.data(), P->hf_tk_K.p, sizeof(double) * tK.size(), s));
        auto same = [&](const HfBlock &m1, const HfBlock &m2) {
            if ((m1.kx == m2.kx) && (m1.ky == m2.ky) && (m1.npts == 0) && (m2.npts == 0)) return true;
            if (m1.npts > 0 && m1.npts == m2.npts) {
                for (int k = 0; k < m1.npts; ++k)
                    if ((tT[m1.off + k] != tT[m2.off + k]) || (tK[m1.off + k] != tK[m2.off + k])) return false;
                return true;
            }
            return false;
        };
        cls.resize(blk.size());
        for (size_t a = 0; a < blk.size(); ++a) {
            cls[a] = (int)a;
            for (size_t b = 0; b < a; ++b)
                if (same(blk[a], blk[b])) {
                    cls[a] = cls[b];
                    break;
                }
        }
    }
    pp_grid_dims(P, x.data(), y.data(), N, NE);
    hipError_t e = upload(P->pp_x, x.data(), x.size(), s);
    if (e == hipSuccess) e = upload(P->pp_y, y.data(), y.size(), s);
    if (e == hipSuccess) e = upload(P->pp_q, P->pot_qmark.data(), P->pot_qmark.size(), s);
    if (e == hipSuccess) e = upload(P->pp_n2e_ptr, ptr.data(), ptr.size(), s);
    if (e == hipSuccess) e = upload(P->pp_n2e, lst.data(), lst.size(), s);
    if (e == hipSuccess) e = upload(P->pp_class, cls.data(), cls.size(), s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);   // (the host vectors go out of scope)
    XFK_CHECK(e);
    P->pp_mesh_ready = true;
    return XFK_OK;
}

}  // namespace xfk

// the grid over the bounding box: cells of twice the mean element area
void xfk::pp_grid_dims(xfk_problem *P, const double *x, const double *y, int N, int NE)
{
    double xa = x[0], xb = x[0], ya = y[0], yb = y[0];
    for (int i = 1; i < N; ++i) {
        xa = std::min(xa, x[i]);
        xb = std::max(xb, x[i]);
        ya = std::min(ya, y[i]);
        yb = std::max(yb, y[i]);
    }
    const double W = xb - xa, H = yb - ya;
    int nx = 1, ny = 1;
    if (W > 0 && H > 0) {
        const double h = std::sqrt(W * H / std::max(1., NE / 2.));
        nx = (int)std::min<double>(kPpMaxCellsPerAxis, std::max(1., std::ceil(W / h)));
        ny = (int)std::min<double>(kPpMaxCellsPerAxis, std::max(1., std::ceil(H / h)));
    } else if (W > 0) {
        nx = std::min(kPpMaxCellsPerAxis, std::max(1, NE));
    } else if (H > 0) {
        ny = std::min(kPpMaxCellsPerAxis, std::max(1, NE));
    }
    P->pp_nx = nx;
    P->pp_ny = ny;
    P->pp_x0 = xa;
    P->pp_y0 = ya;
    P->pp_ihx = W > 0 ? nx / W : 0.;
    P->pp_ihy = H > 0 ? ny / H : 0.;
}

// count, exclusive scan, fill -- once per problem
int xfk::pp_grid_build(xfk_problem *P, const double *x, const double *y, const int *p)
{
    if (P->pp_grid_ready) return XFK_OK;
    hipStream_t s = P->stream;
    const int NE = P->NE, nc = P->pp_nx * P->pp_ny;
    const PpGrid G = pp_grid_args(P);
    DBuf<int> cnt;   // nc counts, then the oversize count
    XFK_CHECK(cnt.alloc((size_t)nc + 1));
    XFK_CHECK(P->pp_cell_ptr.alloc((size_t)nc + 1));
    XFK_CHECK(hipMemsetAsync(cnt.p, 0, sizeof(int) * ((size_t)nc + 1), s));
    const int g = (NE + kBlock - 1) / kBlock;
    k_pp_grid<0><<<g, kBlock, 0, s>>>(NE, G, x, y, p, cnt.p, nullptr, nullptr, cnt.p + nc, nullptr);
    k_pp_scan<<<1, kPpScanBlock, 0, s>>>(nc, cnt.p, P->pp_cell_ptr.p);
    XFK_CHECK(hipGetLastError());
    int total = 0, nbig = 0;
    XFK_CHECK(d2h(&total, P->pp_cell_ptr.p + nc, sizeof(int), s));
    XFK_CHECK(d2h(&nbig, cnt.p + nc, sizeof(int), s));
    XFK_CHECK(P->pp_cell_el.alloc((size_t)std::max(1, total)));
    XFK_CHECK(P->pp_big.alloc((size_t)std::max(1, nbig)));
    XFK_CHECK(hipMemsetAsync(cnt.p, 0, sizeof(int) * ((size_t)nc + 1), s));
    k_pp_grid<1><<<g, kBlock, 0, s>>>(NE, G, x, y, p, cnt.p, P->pp_cell_ptr.p, P->pp_cell_el.p, cnt.p + nc,
                                      P->pp_big.p);
    XFK_CHECK(hipGetLastError());
    XFK_CHECK(hipStreamSynchronize(s));
    P->pp_nbig = nbig;
    P->pp_grid_ready = true;
    return XFK_OK;
}

namespace xfk {

static int pp_grid(xfk_problem *P) { return pp_grid_build(P, P->pp_x.p, P->pp_y.p, P->pot_p.p); }

static int pp_fields(xfk_problem *P)
{
    int rc = pp_mesh(P);
    if (rc != XFK_OK || P->pp_fields_ready) return rc;
    const int NE = P->NE;
    XFK_CHECK(P->pp_D.alloc(2 * (size_t)NE));
    XFK_CHECK(P->pp_E.alloc(2 * (size_t)NE));
    const PpArgs A = pp_args(P);
    const int g = (NE + kBlock - 1) / kBlock;
    if (P->heat) k_pp_element<true><<<g, kBlock, 0, P->stream>>>(NE, A, P->pp_D.p, P->pp_E.p);
    else k_pp_element<false><<<g, kBlock, 0, P->stream>>>(NE, A, P->pp_D.p, P->pp_E.p);
    XFK_CHECK(hipGetLastError());
    P->pp_fields_ready = true;
    return XFK_OK;
}

static int pp_corners(xfk_problem *P, unsigned char *branch_dev)
{
    int rc = pp_fields(P);
    if (rc != XFK_OK || (P->pp_corner_ready && !branch_dev)) return rc;
    const int NE = P->NE;
    XFK_CHECK(P->pp_d.alloc(6 * (size_t)NE));
    const PpArgs A = pp_args(P);
    const int g = (3 * NE + kBlock - 1) / kBlock;
    if (P->heat)
        k_pp_corner<true><<<g, kBlock, 0, P->stream>>>(NE, A, P->pp_q.p, P->pp_n2e_ptr.p, P->pp_n2e.p, P->pp_class.p,
                                                       P->pp_D.p, P->pp_d.p, branch_dev);
    else
        k_pp_corner<false><<<g, kBlock, 0, P->stream>>>(NE, A, P->pp_q.p, P->pp_n2e_ptr.p, P->pp_n2e.p, P->pp_class.p,
                                                        P->pp_D.p, P->pp_d.p, branch_dev);
    XFK_CHECK(hipGetLastError());
    P->pp_corner_ready = true;
    return XFK_OK;
}

// result /= CComplex(vol, 0) (femmcomplex.cpp:393, 456-474)
static void pp_div_volume(double &re, double &im, double vol)
{
    const double zr = vol, zi = 0.;
    double c, yr, yi;
    if (std::fabs(zr) > std::fabs(zi)) {
        c = zi / zr;
        yr = 1. / (zr * (1. + c * c));
        yi = (-c) * yr;
    } else {
        c = zr / zi;
        yi = (-1.) / (zi * (1. + c * c));
        yr = (-c) * yi;
    }
    const double r = re * yr - im * yi, i = re * yi + im * yr;
    re = r;
    im = i;
}

static int pp_block_integrals(xfk_problem *P, const unsigned char *sel, double *out, bool ordered = false)
{
    XFK_REQUIRE(sel, XFK_ERR_ARG, "null selection mask (one byte per block label)");
    XFK_REQUIRE(out, XFK_ERR_ARG, "null output");
    int rc = pp_fields(P);
    if (rc != XFK_OK) return rc;
    hipStream_t s = P->stream;
    const int NE = P->NE, G = (NE + kPotQBlock - 1) / kPotQBlock;
    const size_t nlab = P->pot_labels.n;
    XFK_CHECK(P->pp_sel.alloc(nlab));
    XFK_CHECK(hipMemcpyAsync(P->pp_sel.p, sel, nlab, hipMemcpyHostToDevice, s));
    XFK_CHECK(P->pp_part.alloc(7 * ((size_t)G + 1)));
    const PpArgs A = pp_args(P);
    // (epproc squares LengthConv, hpproc takes pow(., 2.))
    const double lc2 = P->heat ? std::pow(A.lc, 2.) : A.lc * A.lc;
    double *sums = P->pp_part.p + 7 * (size_t)G;
    if (ordered) {
        if (P->heat) k_pp_integrals_seq<true><<<1, kPotQBlock, 0, s>>>(NE, A, P->pp_sel.p, P->pp_D.p, P->pp_E.p, lc2, sums);
        else k_pp_integrals_seq<false><<<1, kPotQBlock, 0, s>>>(NE, A, P->pp_sel.p, P->pp_D.p, P->pp_E.p, lc2, sums);
    } else {
        if (P->heat) k_pp_integrals<true><<<G, kPotQBlock, 0, s>>>(NE, A, P->pp_sel.p, P->pp_D.p, P->pp_E.p, lc2, P->pp_part.p);
        else k_pp_integrals<false><<<G, kPotQBlock, 0, s>>>(NE, A, P->pp_sel.p, P->pp_D.p, P->pp_E.p, lc2, P->pp_part.p);
        k_pot_sum<7><<<1, kPotQBlock, 0, s>>>(G, P->pp_part.p, sums);
    }
    XFK_CHECK(hipGetLastError());
    XFK_CHECK(d2h(out, sums, 7 * sizeof(double), s));
    // the averaged types, divided after the loop as the reference does
    const double vol = out[2];
    double zero = 0.;
    if (P->heat) pp_div_volume(out[0], zero, vol);
    pp_div_volume(out[3], out[4], vol);
    pp_div_volume(out[5], out[6], vol);
    return XFK_OK;
}

}  // namespace xfk

using namespace xfk;

hipError_t xfk::warm_module_postproc()
{
    hipFuncAttributes a;
    return hipFuncGetAttributes(&a, reinterpret_cast<const void *>(&k_pp_scan));
}

// The problem kinds this post-processor answers (post_entry: xfk_post.h)
template <class F>
static int pp_entry(xfk_problem *P, bool need_solution, F &&body)
{
    return post_entry(P, [&]() -> int {
        XFK_REQUIRE(P, XFK_ERR_ARG, "null problem");
        XFK_REQUIRE(P->electro || P->heat, XFK_ERR_ARG,
                    "not a scalar-potential problem: post-processing is for electrostatic and heat-flow problems");
        XFK_REQUIRE(!need_solution || P->pot_solved, XFK_ERR_ARG,
                    "no solution yet (solve the problem or xfk_pot_set_solution)");
        return XFK_OK;
    }, body);
}

static int pp_launch_points(xfk_problem *P, int n, const double *px, const double *py, int smooth, double *o,
                            int *ntests, int given = 0)
{
    const PpArgs A = pp_args(P);
    const PpGrid G = pp_grid_args(P);
    const PpLists L = pp_lists(P);
    const int g = (n + kBlock - 1) / kBlock;
    hipStream_t s = P->stream;
    if (P->heat)
        k_pp_points<true><<<g, kBlock, 0, s>>>(n, A, G, L, px, py, smooth ? 1 : 0, P->pp_D.p, P->pp_d.p, P->pp_pel.p, o,
                                               ntests, given);
    else
        k_pp_points<false><<<g, kBlock, 0, s>>>(n, A, G, L, px, py, smooth ? 1 : 0, P->pp_D.p, P->pp_d.p, P->pp_pel.p, o,
                                                ntests, given);
    XFK_CHECK(hipGetLastError());
    return XFK_OK;
}

// --- the weighted stress tensor mask: host side (the rest is xfk_mask.hip) -------

// the mask's auxiliary problem of a scalar-potential problem: from its post-processing mesh tables
static int pot_mask_aux_create(xfk_problem *P)
{
    if (P->mask_aux) return XFK_OK;
    hipStream_t s = P->stream;
    const int N = P->N, NE = P->NE;
    std::vector<double> x(N), y(N);
    std::vector<int> p(3 * (size_t)NE), lbl(NE);
    std::vector<PotLabel> lab(P->pot_labels.n);
    XFK_CHECK(d2h(x.data(), P->pp_x.p, sizeof(double) * N, s));
    XFK_CHECK(d2h(y.data(), P->pp_y.p, sizeof(double) * N, s));
    XFK_CHECK(d2h(p.data(), P->pot_p.p, sizeof(int) * 3 * (size_t)NE, s));
    XFK_CHECK(d2h(lbl.data(), P->lbl_raw.p, sizeof(int) * NE, s));
    XFK_CHECK(d2h(lab.data(), P->pot_labels.p, sizeof(PotLabel) * lab.size(), s));
    return mask_aux_create(P, x, y, p, lbl, lab, P->pot_length_units);
}

static const char *const kMaskInvalid =
    "The selected region is invalid. A valid selection cannot abut a region which is not free space.";

// CSMaterialProp::isAir (CMaterialProp.cpp:1603-1609)
static bool pp_is_air(const EsBlock &b) { return (b.ex == 1) && (b.ey == 1) && (b.qv == 0); }

// PostProcessor::makeMask for the selection (one byte per label; nsel, one
// byte per node, may be null; max_area, one double per label, may be null: the
// element areas weight the Laplacian)
static int pot_make_mask(xfk_problem *P, const unsigned char *sel, const unsigned char *nsel, const double *max_area)
{
    XFK_REQUIRE(P->electro, XFK_ERR_ARG,
                "the weighted stress tensor mask is for electrostatic problems: heat-flow problems have no "
                "integrals 5 and 6");
    XFK_REQUIRE(sel, XFK_ERR_ARG, "null selection mask (one byte per block label)");
    P->mask_ready = false;
    MaskInputs I = {};
    I.t_all = std::chrono::steady_clock::now();
    int rc = pp_mesh(P);
    if (rc != XFK_OK) return rc;
    const size_t nlab = P->pot_labels.n;
    const auto t0 = std::chrono::steady_clock::now();
    const bool fresh = !P->mask_aux;
    if ((rc = pot_mask_aux_create(P)) != XFK_OK) return rc;
    I.ms_create = fresh ? wall_ms(t0) : 0.;
    // the rules begin: selected, and not air by the label's block
    I.t_rules = std::chrono::steady_clock::now();
    std::vector<PotLabel> lab(nlab);
    std::vector<EsBlock> blk(P->es_blocks.n);
    XFK_CHECK(d2h(lab.data(), P->pot_labels.p, sizeof(PotLabel) * nlab, P->stream));
    XFK_CHECK(d2h(blk.data(), P->es_blocks.p, sizeof(EsBlock) * blk.size(), P->stream));
    std::vector<unsigned char> lflag(2 * nlab);
    for (size_t k = 0; k < nlab; ++k) {
        lflag[2 * k] = sel[k] ? 1 : 0;
        lflag[2 * k + 1] = pp_is_air(blk[lab[k].blk]) ? 0 : 1;
    }
    std::vector<double> area(nlab, 0.);
    if (max_area) area.assign(max_area, max_area + nlab);
    I.x = P->pp_x.p;
    I.p = P->pot_p.p;
    I.lbl = P->lbl_raw.p;
    I.n2e_ptr = P->pp_n2e_ptr.p;
    I.n2e = P->pp_n2e.p;
    I.lflag = lflag.data();
    I.area = area.data();
    I.nentries = nlab;
    I.q = P->pp_q.p;
    I.nsel = nsel;
    I.point = P->pot_has_point.data();
    I.sel = sel;
    I.nsel_labels = nlab;
    I.invalid = kMaskInvalid;
    return mask_make(P, I);
}

// the three sums of k_pp_stress over all elements, in a fixed order: the x and
// y (z) force, the torque about the origin
static int pp_launch_stress(xfk_problem *P)
{
    const int NE = P->NE, G = (NE + kPotQBlock - 1) / kPotQBlock;
    const PpArgs A = pp_args(P);
    k_pp_stress<<<G, kPotQBlock, 0, P->stream>>>(NE, A, P->mask_msk.p, P->pp_D.p, A.lc * A.lc, P->pp_part.p);
    k_pot_sum<3><<<1, kPotQBlock, 0, P->stream>>>(G, P->pp_part.p, P->pp_part.p + 7 * (size_t)G);
    XFK_CHECK(hipGetLastError());
    return XFK_OK;
}

static int pp_stress_integrals(xfk_problem *P, double *out3)
{
    int rc = pp_fields(P);
    if (rc != XFK_OK) return rc;
    const int G = (P->NE + kPotQBlock - 1) / kPotQBlock;
    XFK_CHECK(P->pp_part.alloc(7 * ((size_t)G + 1)));
    if ((rc = pp_launch_stress(P)) != XFK_OK) return rc;
    XFK_CHECK(d2h(out3, P->pp_part.p + 7 * (size_t)G, 3 * sizeof(double), P->stream));
    return XFK_OK;
}

// --- contour integrals: host side ---------------------------------------------

static int pot_contour_check(const xfk_problem *P, int nc, const int *ptr, const double *x, const double *y,
                             int type)
{
    XFK_REQUIRE(nc >= 0, XFK_ERR_ARG, "negative number of contours");
    XFK_REQUIRE(type >= 0, XFK_ERR_ARG, "line integral type out of range (negative)");
    XFK_REQUIRE(!P->heat || type <= 3, XFK_ERR_ARG,
                "line integral type out of range: a heat-flow problem has types 0-3 (the stress tensor force and "
                "torque, 3 and 4, are electrostatic)");
    XFK_REQUIRE(!P->electro || type <= 4, XFK_ERR_ARG, "line integral type out of range: an electrostatic problem has types 0-4");
    return pp_contour_check(nc, ptr, x, y);
}

int xfk::pp_contour_check(int nc, const int *ptr, const double *x, const double *y)
{
    XFK_REQUIRE(nc >= 0, XFK_ERR_ARG, "negative number of contours");
    if (nc == 0) return XFK_OK;
    XFK_REQUIRE(ptr && x && y, XFK_ERR_ARG, "null contour arrays");
    XFK_REQUIRE(ptr[0] >= 0, XFK_ERR_ARG, "contour offsets must start at 0 or above and not decrease");
    for (int c = 0; c < nc; ++c) {
        XFK_REQUIRE(ptr[c + 1] >= ptr[c], XFK_ERR_ARG, "contour offsets must start at 0 or above and not decrease");
        XFK_REQUIRE(ptr[c + 1] - ptr[c] >= 2, XFK_ERR_ARG, "a contour needs at least 2 points");
        for (int k = ptr[c]; k < ptr[c + 1]; ++k) {
            XFK_REQUIRE(x[k] == x[k] && y[k] == y[k], XFK_ERR_ARG, "a contour vertex is NaN");
            XFK_REQUIRE(std::isfinite(x[k]) && std::isfinite(y[k]), XFK_ERR_ARG, "a contour vertex is infinite");
            if (k > ptr[c]) {
                const double len = pp_cabs(x[k] - x[k - 1], y[k] - y[k - 1]);
                XFK_REQUIRE(len > 0, XFK_ERR_ARG, "a contour has a zero-length segment (two equal consecutive points)");
                XFK_REQUIRE(std::isfinite(len), XFK_ERR_ARG, "a contour segment's length overflows");
            }
        }
    }
    return XFK_OK;
}

int xfk::pp_contour_layout(xfk_problem *P, int nc, const int *ptr, const double *x, const double *y, int type,
                           int smooth, int npts, PpContours &J)
{
    hipStream_t s = P->stream;
    J.nc = nc;
    J.type = type;
    J.smooth = smooth ? 1 : 0;
    J.npts = npts <= 0 ? kPpLineIntegralPoints : npts;
    J.cptr.assign(nc + 1, 0);
    J.bptr.assign(nc + 1, 0);
    long long groups = 0;
    for (int c = 0; c < nc; ++c) {
        const long long samples = (long long)(ptr[c + 1] - ptr[c] - 1) * J.npts;
        XFK_REQUIRE(samples < (1LL << 31) - kPotQBlock, XFK_ERR_ARG, "a contour has too many samples (segments x points >= 2^31)");
        groups += (samples + kPotQBlock - 1) / kPotQBlock;
        XFK_REQUIRE(groups < (1LL << 31), XFK_ERR_ARG, "the batch has too many samples (2^31 workgroups)");
        J.cptr[c + 1] = ptr[c + 1] - ptr[0];
        J.bptr[c + 1] = (int)groups;
    }
    const size_t nv = (size_t)J.cptr[nc];
    XFK_CHECK(J.d_xy.alloc(2 * nv));
    XFK_CHECK(hipMemcpyAsync(J.d_xy.p, x + ptr[0], sizeof(double) * nv, hipMemcpyHostToDevice, s));
    XFK_CHECK(hipMemcpyAsync(J.d_xy.p + nv, y + ptr[0], sizeof(double) * nv, hipMemcpyHostToDevice, s));
    XFK_CHECK(upload(J.d_cptr, J.cptr.data(), J.cptr.size(), s));
    XFK_CHECK(upload(J.d_bptr, J.bptr.data(), J.bptr.size(), s));
    XFK_CHECK(J.part.alloc(3 * ((size_t)groups + nc)));
    return XFK_OK;
}

void xfk::launch_contour_sum(hipStream_t s, PpContours &J)
{
    k_pp_contour_sum<<<J.nc, kPotQBlock, 0, s>>>(J.d_bptr.p, J.part.p, J.sums());
}

// types 1, 3, 4 (heat flow: 1, 3): the batch on the device, the fields and the grid ready
static int pp_contour_prepare(xfk_problem *P, int nc, const int *ptr, const double *x, const double *y, int type,
                              int smooth, int npts, PpContours &J)
{
    int rc = pp_contour_layout(P, nc, ptr, x, y, type, smooth, npts, J);
    if (rc == XFK_OK) rc = J.smooth ? pp_corners(P, nullptr) : pp_fields(P);
    if (rc == XFK_OK) rc = pp_grid(P);
    return rc;
}

// the sample kernel and the per-contour sums; dbg_xy, dbg_el: one contour's samples (may be null)
static int pp_contour_launch(xfk_problem *P, PpContours &J, double *dbg_xy, int *dbg_el)
{
    const PpArgs A = pp_args(P);
    const PpGrid G = pp_grid_args(P);
    const PpLists L = pp_lists(P);
    hipStream_t s = P->stream;
    const double *cx = J.d_xy.p, *cy = cx + J.cptr[J.nc];
    if (P->heat)
        k_pp_contour<true><<<J.groups(), kPotQBlock, 0, s>>>(J.nc, A, G, L, J.d_cptr.p, J.d_bptr.p, cx, cy, J.npts,
                                                             J.type, J.smooth, P->pp_D.p, P->pp_d.p, J.part.p, dbg_xy,
                                                             dbg_el);
    else
        k_pp_contour<false><<<J.groups(), kPotQBlock, 0, s>>>(J.nc, A, G, L, J.d_cptr.p, J.d_bptr.p, cx, cy, J.npts,
                                                              J.type, J.smooth, P->pp_D.p, P->pp_d.p, J.part.p, dbg_xy,
                                                              dbg_el);
    launch_contour_sum(s, J);
    XFK_CHECK(hipGetLastError());
    return XFK_OK;
}

// lineIntegral type 0: V (T) at the first point minus at the last, through the point kernel
static int pp_contour_ends(xfk_problem *P, int nc, const int *ptr, const double *x, const double *y, double *out,
                           int *missed)
{
    int rc = pp_fields(P);
    if (rc == XFK_OK) rc = pp_grid(P);
    if (rc != XFK_OK) return rc;
    const int n = 2 * nc;
    std::vector<double> ex, ey, val(8 * (size_t)n);
    contour_end_points(nc, ptr, x, y, ex, ey);
    if ((rc = upload_points(P, n, ex.data(), ey.data(), 8)) != XFK_OK) return rc;
    double *px = P->pp_pts.p, *o = px + 2 * (size_t)n;
    if ((rc = pp_launch_points(P, n, px, px + n, 0, o, nullptr)) != XFK_OK) return rc;
    std::vector<int> el(n);
    XFK_CHECK(d2h(el.data(), P->pp_pel.p, sizeof(int) * (size_t)n, P->stream));
    XFK_CHECK(d2h(val.data(), o, sizeof(double) * 8 * (size_t)n, P->stream));
    for (int c = 0; c < nc; ++c) {
        double r = val[8 * (size_t)(2 * c)];
        r -= val[8 * (size_t)(2 * c + 1)];
        out[2 * c] = r;
        out[2 * c + 1] = 0.;
        if (missed) missed[c] = (el[2 * c] < 0) + (el[2 * c + 1] < 0);
    }
    return XFK_OK;
}

// lineIntegral type 2 (epproc.cpp:574-595, hpproc.cpp:727-744): length and swept area, on the host
static void pp_contour_length(const xfk_problem *P, int n, const double *x, const double *y, double *out2)
{
    const double lc = kPpLengthConv[P->pot_length_units];
    const double depth = P->pot_depth_user == -1 ? 1 : P->pot_depth_user * lc;
    double len, area;
    polyline_sums(n, x, y, P->axi, len, area);
    out2[0] = len * lc;
    out2[1] = P->axi ? area * (P->heat ? std::pow(lc, 2.) : lc * lc) : out2[0] * depth;
}

static int pp_line_integrals(xfk_problem *P, int nc, const int *ptr, const double *x, const double *y, int type,
                             int smooth, int npts, double *out, int *missed)
{
    int rc = pot_contour_check(P, nc, ptr, x, y, type);
    if (rc != XFK_OK || nc == 0) return rc;
    XFK_REQUIRE(out, XFK_ERR_ARG, "null output");
    if (type == 0) return pp_contour_ends(P, nc, ptr, x, y, out, missed);
    if (type == 2) {
        for (int c = 0; c < nc; ++c) {
            pp_contour_length(P, ptr[c + 1] - ptr[c], x + ptr[c], y + ptr[c], out + 2 * c);
            if (missed) missed[c] = 0;
        }
        return XFK_OK;
    }
    PpContours J;
    if ((rc = pp_contour_prepare(P, nc, ptr, x, y, type, smooth, npts, J)) != XFK_OK) return rc;
    if ((rc = pp_contour_launch(P, J, nullptr, nullptr)) != XFK_OK) return rc;
    std::vector<double> sums(3 * (size_t)nc);
    XFK_CHECK(d2h(sums.data(), J.sums(), sizeof(double) * sums.size(), P->stream));
    for (int c = 0; c < nc; ++c) {
        double r0 = sums[3 * (size_t)c], r1 = sums[3 * (size_t)c + 1];
        // the averages, divided after the loop as the reference does
        if (type == 1) r1 = r0 / r1;
        else if (P->heat) r0 = r0 / r1;   // (type 3: the weight sum stays in r1)
        out[2 * c] = r0;
        out[2 * c + 1] = r1;
        if (missed) missed[c] = (int)sums[3 * (size_t)c + 2];
    }
    return XFK_OK;
}

extern "C" {

int xfk_pot_line_integrals(xfk_problem *P, int n_contours, const int *ptr, const double *x, const double *y,
                           int type, int smooth, int npts, double *out, int *missed)
{
    return pp_entry(P, true, [&]() -> int {
        return pp_line_integrals(P, n_contours, ptr, x, y, type, smooth, npts, out, missed);
    });
}

int xfk_pot_line_integral(xfk_problem *P, int n, const double *x, const double *y, int type, int smooth, int npts,
                          double *out2, int *missed)
{
    return pp_entry(P, true, [&]() -> int {
        XFK_REQUIRE(n >= 0, XFK_ERR_ARG, "negative number of contour points");
        const int ptr[2] = {0, n};
        return pp_line_integrals(P, 1, ptr, x, y, type, smooth, npts, out2, missed);
    });
}

int xfk_pot_contour_samples(xfk_problem *P, int n, const double *x, const double *y, int type, int npts, double *xy,
                            int *elem)
{
    return pp_entry(P, true, [&]() -> int {
        return contour_samples(P, n, x, y, type, npts, xy, elem, pot_contour_check, pp_contour_prepare,
                               pp_contour_launch);
    });
}

int xfk_pot_contour_time(xfk_problem *P, int n_contours, const int *ptr, const double *x, const double *y, int type,
                         int smooth, int npts, int repeats, double *ms)
{
    return pp_entry(P, true, [&]() -> int {
        XFK_REQUIRE(repeats > 0 && ms && n_contours > 0, XFK_ERR_ARG,
                    "xfk_pot_contour_time needs contours, repeats > 0 and its output");
        return contour_time(P, n_contours, ptr, x, y, type, smooth, npts, repeats, ms, pot_contour_check,
                            pp_contour_prepare, pp_contour_launch);
    });
}

int xfk_pot_set_solution(xfk_problem *P, const double *V)
{
    return pp_entry(P, false, [&]() -> int {
        XFK_REQUIRE(V, XFK_ERR_ARG, "null solution");
        P->pot_solved = false;
        pp_invalidate(P);
        XFK_CHECK(P->V.alloc((size_t)std::max(P->N, P->NL)));
        XFK_CHECK(hipMemcpyAsync(P->V.p, V, sizeof(double) * P->N, hipMemcpyHostToDevice, P->stream));
        XFK_CHECK(hipStreamSynchronize(P->stream));
        // the integrals of the prescribed-value conductors belong to the solution
        int rc = P->heat ? heat_conductor_integrals(P) : electro_conductor_integrals(P);
        if (rc != XFK_OK) return rc;
        XFK_CHECK(hipStreamSynchronize(P->stream));
        P->pot_solved = true;
        return XFK_OK;
    });
}

int xfk_pot_element_fields(xfk_problem *P, double *D, double *E)
{
    return pp_entry(P, true, [&]() -> int {
        int rc = pp_fields(P);
        if (rc != XFK_OK) return rc;
        const size_t bytes = sizeof(double) * 2 * (size_t)P->NE;
        if (D) XFK_CHECK(d2h(D, P->pp_D.p, bytes, P->stream));
        if (E) XFK_CHECK(d2h(E, P->pp_E.p, bytes, P->stream));
        XFK_CHECK(hipStreamSynchronize(P->stream));
        return XFK_OK;
    });
}

int xfk_pot_corner_fields(xfk_problem *P, double *d)
{
    return pp_entry(P, true, [&]() -> int {
        int rc = pp_corners(P, nullptr);
        if (rc != XFK_OK) return rc;
        if (d) XFK_CHECK(d2h(d, P->pp_d.p, sizeof(double) * 6 * (size_t)P->NE, P->stream));
        XFK_CHECK(hipStreamSynchronize(P->stream));
        return XFK_OK;
    });
}

int xfk_pot_corner_branches(xfk_problem *P, unsigned char *branch)
{
    return pp_entry(P, true, [&]() -> int {
        XFK_REQUIRE(branch, XFK_ERR_ARG, "null output");
        DBuf<unsigned char> br;
        XFK_CHECK(br.alloc(3 * (size_t)P->NE));
        int rc = pp_corners(P, br.p);
        if (rc != XFK_OK) return rc;
        XFK_CHECK(d2h(branch, br.p, 3 * (size_t)P->NE, P->stream));
        XFK_CHECK(hipStreamSynchronize(P->stream));
        return XFK_OK;
    });
}

int xfk_pot_block_integrals(xfk_problem *P, const unsigned char *label_selected, double *out7)
{
    return pp_entry(P, true, [&]() -> int { return pp_block_integrals(P, label_selected, out7); });
}

int xfk_pot_block_integral(xfk_problem *P, const unsigned char *label_selected, int type, double *out2)
{
    return pp_entry(P, true, [&]() -> int {
        XFK_REQUIRE(type >= 0 && type <= 6, XFK_ERR_ARG, "block integral type out of range (0-6)");
        XFK_REQUIRE(type <= 4 || P->electro, XFK_ERR_ARG,
                    "block integral types 5 and 6 (weighted stress tensor force and torque) are not supported "
                    "on a heat-flow problem: the reference's hpproc has none");
        XFK_REQUIRE(type <= 4 || mask_matches(P, label_selected, P->pot_labels.n), XFK_ERR_ARG,
                    "block integral types 5 and 6 (weighted stress tensor force and torque) need the mask of a "
                    "Laplace solve of their own, made for this label selection and this solution: call "
                    "xfk_pot_make_mask");
        XFK_REQUIRE(out2, XFK_ERR_ARG, "null output");
        if (type >= 5) {
            double o[3];
            const int rc = pp_stress_integrals(P, o);
            if (rc != XFK_OK) return rc;
            out2[0] = type == 5 ? o[0] : o[2];
            out2[1] = type == 5 ? o[1] : 0.;
            return XFK_OK;
        }
        double o[7];
        const int rc = pp_block_integrals(P, label_selected, o);
        if (rc != XFK_OK) return rc;
        out2[1] = 0.;
        if (type <= 2) out2[0] = o[type];
        else {
            out2[0] = o[type == 3 ? 3 : 5];
            out2[1] = o[type == 3 ? 4 : 6];
        }
        return XFK_OK;
    });
}

int xfk_pot_make_mask(xfk_problem *P, const unsigned char *label_selected, const unsigned char *node_selected,
                      const double *label_max_area)
{
    return pp_entry(P, true, [&]() -> int { return pot_make_mask(P, label_selected, node_selected, label_max_area); });
}

int xfk_pot_get_mask(xfk_problem *P, double *W, double *msk)
{
    return pp_entry(P, true, [&]() -> int {
        XFK_REQUIRE(P->mask_ready && P->mask_aux, XFK_ERR_ARG,
                    "no mask (xfk_pot_make_mask; a new solution drops the mask)");
        const size_t bytes = sizeof(double) * (size_t)P->N;
        if (W) XFK_CHECK(d2h(W, P->mask_aux->V.p, bytes, P->stream));
        if (msk) XFK_CHECK(d2h(msk, P->mask_msk.p, bytes, P->stream));
        return XFK_OK;
    });
}

int xfk_pot_get_qmarks(xfk_problem *P, int *Q)
{
    return pp_entry(P, false, [&]() -> int {
        XFK_REQUIRE(Q, XFK_ERR_ARG, "null output");
        std::copy(P->pot_qmark.begin(), P->pot_qmark.end(), Q);
        return XFK_OK;
    });
}

int xfk_pot_set_qmarks(xfk_problem *P, const int *Q)
{
    return pp_entry(P, false, [&]() -> int {
        XFK_REQUIRE(Q, XFK_ERR_ARG, "null marks");
        const int nc = (int)P->pot_cel_ptr.size() - 1;
        for (int i = 0; i < P->N; ++i)
            XFK_REQUIRE(Q[i] >= -2 && Q[i] < std::max(0, nc), XFK_ERR_ARG,
                        "a node mark is neither -2, -1 nor the index of a conductor");
        P->pot_qmark.assign(Q, Q + P->N);
        P->pot_from_file = true;
        // the corner fields and the mask read the marks
        pp_invalidate(P);
        if (P->pp_mesh_ready) {
            XFK_CHECK(upload(P->pp_q, P->pot_qmark.data(), P->pot_qmark.size(), P->stream));
            XFK_CHECK(hipStreamSynchronize(P->stream));
        }
        return XFK_OK;
    });
}

int xfk_pot_plot_bounds(xfk_problem *P, double *out6)
{
    return pp_entry(P, true, [&]() -> int {
        XFK_REQUIRE(out6, XFK_ERR_ARG, "null output");
        int rc = pp_fields(P);
        if (rc != XFK_OK) return rc;
        hipStream_t s = P->stream;
        const int N = P->N, NE = P->NE;
        XFK_REQUIRE(N > 0 && NE > 0, XFK_ERR_ARG, "plot bounds need a node and an element");
        const int G = (std::max(N, NE) + kPpBoundsBlock - 1) / kPpBoundsBlock;
        DBuf<double> part;
        XFK_CHECK(part.alloc(kPpBoundsK * ((size_t)G + 1)));
        double *sums = part.p + kPpBoundsK * (size_t)G;
        k_pp_bounds<<<G, kPpBoundsBlock, 0, s>>>(N, NE, P->V.p, P->lbl_raw.p, P->pot_labels.p, P->pp_D.p, P->pp_E.p,
                                                 part.p);
        k_pp_bounds_fold<<<1, kPpBoundsBlock, 0, s>>>(G, part.p, sums);
        XFK_CHECK(hipGetLastError());
        double h[kPpBoundsK];
        XFK_CHECK(d2h(h, sums, sizeof(h), s));
        XFK_CHECK(hipStreamSynchronize(s));
        // The reference's starting values: |D| of the element whose index is
        // the count of external elements, |E| of element 0, external or not
        // (epproc.cpp:205-208).  With every element external that index is
        // past the end in the reference; element 0 stands in here.
        const int ext = (int)h[6], d0 = ext < NE ? ext : 0;
        double Ds[2], Es[2];
        XFK_CHECK(d2h(Ds, P->pp_D.p + 2 * (size_t)d0, sizeof(Ds), s));
        XFK_CHECK(d2h(Es, P->pp_E.p, sizeof(Es), s));
        XFK_CHECK(hipStreamSynchronize(s));
        out6[0] = h[0];
        out6[1] = h[1];
        const double start[2] = {pp_cabs(Ds[0], Ds[1]), pp_cabs(Es[0], Es[1])};
        for (int k = 0; k < 2; ++k) {
            double lo = start[k], hi = start[k];
            if (h[3 + 2 * k] > hi) hi = h[3 + 2 * k];
            if (h[2 + 2 * k] < lo) lo = h[2 + 2 * k];
            out6[2 + 2 * k] = lo;
            out6[3 + 2 * k] = hi;
        }
        return XFK_OK;
    });
}

int xfk_pot_mask_info(xfk_problem *P, double *out9)
{
    return pp_entry(P, false, [&]() -> int {
        XFK_REQUIRE(out9, XFK_ERR_ARG, "null output");
        out9[0] = P->mask_ready ? 1. : 0.;
        for (int k = 0; k < 8; ++k) out9[1 + k] = P->mask_info[k];
        return XFK_OK;
    });
}

int xfk_pot_mask_problem(xfk_problem *P, xfk_problem **aux)
{
    return pp_entry(P, false, [&]() -> int {
        XFK_REQUIRE(aux, XFK_ERR_ARG, "null output");
        XFK_REQUIRE(P->mask_aux && P->mask_aux->symbolic_ready, XFK_ERR_ARG, "no mask problem yet (xfk_pot_make_mask)");
        *aux = P->mask_aux;
        return XFK_OK;
    });
}

int xfk_pot_stress_time(xfk_problem *P, int repeats, double *ms)
{
    return pp_entry(P, true, [&]() -> int {
        XFK_REQUIRE(repeats > 0 && ms, XFK_ERR_ARG, "xfk_pot_stress_time needs repeats > 0 and its output");
        XFK_REQUIRE(P->mask_ready, XFK_ERR_ARG, "no mask (xfk_pot_make_mask; a new solution drops the mask)");
        int rc = pp_fields(P);
        if (rc != XFK_OK) return rc;
        XFK_CHECK(P->pp_part.alloc(7 * ((size_t)(P->NE + kPotQBlock - 1) / kPotQBlock + 1)));
        return timed_median(P->stream, repeats, [&] { return pp_launch_stress(P); }, *ms);
    });
}

int xfk_pot_point_values(xfk_problem *P, int n, const double *x, const double *y, int smooth, int *elem, double *out)
{
    return pp_entry(P, true, [&]() -> int {
        XFK_REQUIRE(n >= 0, XFK_ERR_ARG, "negative number of points");
        if (n == 0) return XFK_OK;
        XFK_REQUIRE(x && y && elem && out, XFK_ERR_ARG, "null point arrays");
        int rc = smooth ? pp_corners(P, nullptr) : pp_fields(P);
        if (rc == XFK_OK) rc = pp_grid(P);
        if (rc == XFK_OK) rc = upload_points(P, n, x, y, 8);
        if (rc != XFK_OK) return rc;
        double *px = P->pp_pts.p, *o = px + 2 * (size_t)n;
        rc = pp_launch_points(P, n, px, px + n, smooth, o, nullptr);
        if (rc != XFK_OK) return rc;
        XFK_CHECK(d2h(elem, P->pp_pel.p, sizeof(int) * (size_t)n, P->stream));
        XFK_CHECK(d2h(out, o, sizeof(double) * 8 * (size_t)n, P->stream));
        return XFK_OK;
    });
}

int xfk_pot_point_values_at(xfk_problem *P, int n, const double *x, const double *y, const int *elem, int smooth,
                            double *out)
{
    return pp_entry(P, true, [&]() -> int {
        XFK_REQUIRE(n >= 0, XFK_ERR_ARG, "negative number of points");
        if (n == 0) return XFK_OK;
        XFK_REQUIRE(x && y && elem && out, XFK_ERR_ARG, "null point arrays");
        for (int i = 0; i < n; ++i)
            XFK_REQUIRE(elem[i] >= -1 && elem[i] < P->NE, XFK_ERR_ARG, "a point's element is outside the element range");
        int rc = smooth ? pp_corners(P, nullptr) : pp_fields(P);
        if (rc == XFK_OK) rc = upload_points(P, n, x, y, 8);
        if (rc != XFK_OK) return rc;
        XFK_CHECK(hipMemcpyAsync(P->pp_pel.p, elem, sizeof(int) * (size_t)n, hipMemcpyHostToDevice, P->stream));
        double *px = P->pp_pts.p, *o = px + 2 * (size_t)n;
        rc = pp_launch_points(P, n, px, px + n, smooth, o, nullptr, 1);
        if (rc != XFK_OK) return rc;
        XFK_CHECK(d2h(out, o, sizeof(double) * 8 * (size_t)n, P->stream));
        return XFK_OK;
    });
}

int xfk_pot_block_integrals_ordered(xfk_problem *P, const unsigned char *label_selected, double *out7)
{
    return pp_entry(P, true, [&]() -> int { return pp_block_integrals(P, label_selected, out7, true); });
}

int xfk_pot_grid_info(xfk_problem *P, double *out8)
{
    return pp_entry(P, false, [&]() -> int {
        XFK_REQUIRE(out8, XFK_ERR_ARG, "null output");
        int rc = pp_mesh(P);
        if (rc == XFK_OK) rc = pp_grid(P);
        if (rc != XFK_OK) return rc;
        int total = 0;
        XFK_CHECK(d2h(&total, P->pp_cell_ptr.p + (size_t)P->pp_nx * P->pp_ny, sizeof(int), P->stream));
        out8[0] = P->pp_x0;
        out8[1] = P->pp_y0;
        out8[2] = P->pp_ihx;
        out8[3] = P->pp_ihy;
        out8[4] = P->pp_nx;
        out8[5] = P->pp_ny;
        out8[6] = P->pp_nbig;
        out8[7] = total;
        return XFK_OK;
    });
}

int xfk_pot_time(xfk_problem *P, int n, const double *x, const double *y, int repeats, double *ms7,
                 double *tests_per_point)
{
    return pp_entry(P, true, [&]() -> int {
        XFK_REQUIRE(n > 0 && x && y && repeats > 0 && ms7 && tests_per_point, XFK_ERR_ARG,
                    "xfk_pot_time needs points, repeats > 0 and its outputs");
        hipStream_t s = P->stream;
        auto timed = [&](auto f, double &out) { return timed_median(s, repeats, f, out); };
        int rc;
        // the host build of the mesh tables (wall clock: downloads, the sort, uploads)
        std::vector<double> t;
        for (int k = 0; k <= repeats; ++k) {
            P->pp_mesh_ready = false;
            const auto t0 = std::chrono::steady_clock::now();
            if ((rc = pp_mesh(P)) != XFK_OK) return rc;
            if (k) t.push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
        }
        std::sort(t.begin(), t.end());
        ms7[0] = t[t.size() / 2];
        if ((rc = timed([&] { P->pp_grid_ready = false; return pp_grid(P); }, ms7[1])) != XFK_OK) return rc;
        if ((rc = timed([&] { P->pp_fields_ready = false; return pp_fields(P); }, ms7[2])) != XFK_OK) return rc;
        if ((rc = timed([&] { P->pp_corner_ready = false; return pp_corners(P, nullptr); }, ms7[3])) != XFK_OK) return rc;
        // the integral launch and its sum, every label selected
        const int NE = P->NE, G = (NE + kPotQBlock - 1) / kPotQBlock;
        const size_t nlab = P->pot_labels.n;
        std::vector<unsigned char> sel(nlab, 1);
        XFK_CHECK(P->pp_sel.alloc(nlab));
        XFK_CHECK(hipMemcpyAsync(P->pp_sel.p, sel.data(), nlab, hipMemcpyHostToDevice, s));
        XFK_CHECK(hipStreamSynchronize(s));
        XFK_CHECK(P->pp_part.alloc(7 * ((size_t)G + 1)));
        const PpArgs A = pp_args(P);
        const double lc2 = P->heat ? std::pow(A.lc, 2.) : A.lc * A.lc;
        rc = timed([&] {
            if (P->heat) k_pp_integrals<true><<<G, kPotQBlock, 0, s>>>(NE, A, P->pp_sel.p, P->pp_D.p, P->pp_E.p, lc2, P->pp_part.p);
            else k_pp_integrals<false><<<G, kPotQBlock, 0, s>>>(NE, A, P->pp_sel.p, P->pp_D.p, P->pp_E.p, lc2, P->pp_part.p);
            k_pot_sum<7><<<1, kPotQBlock, 0, s>>>(G, P->pp_part.p, P->pp_part.p + 7 * (size_t)G);
            return hipGetLastError() == hipSuccess ? XFK_OK : XFK_ERR_HIP;
        }, ms7[4]);
        if (rc != XFK_OK) return rc;
        if ((rc = upload_points(P, n, x, y, 8)) != XFK_OK) return rc;
        double *px = P->pp_pts.p, *o = px + 2 * (size_t)n;
        for (int smooth = 0; smooth < 2; ++smooth)
            if ((rc = timed([&] { return pp_launch_points(P, n, px, px + n, smooth, o, nullptr); }, ms7[5 + smooth])) != XFK_OK)
                return rc;
        // the counted run: the elements each point was tested against
        DBuf<int> cnt;
        XFK_CHECK(cnt.alloc((size_t)n));
        if ((rc = pp_launch_points(P, n, px, px + n, 0, o, cnt.p)) != XFK_OK) return rc;
        std::vector<int> h(n);
        XFK_CHECK(d2h(h.data(), cnt.p, sizeof(int) * (size_t)n, s));
        double sum = 0;
        for (int v : h) sum += v;
        *tests_per_point = sum / n;
        return XFK_OK;
    });
}

}  // extern "C"
