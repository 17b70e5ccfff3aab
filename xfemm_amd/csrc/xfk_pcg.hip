// Preconditioned conjugate gradient of the fsolver hot path: two launches per
// iteration with the Jacobi preconditioner, update + V-cycle + SpMV with the
// default smoothed-aggregation AMG (xfk_amg*.hip).
//
// Reference: CBigLinProb::PCGSolve (cfemm/libfemm/spars.cpp:238-316) -- same
// PCG, same stopping test sqrt(z.r / z0.b) <= Precision, same initial guess
// semantics (flag); the preconditioner M is the AMG V-cycle (default) or
// diag(A) (Jacobi) instead of the reference's sequential SSOR sweep.
//
// Formulation: the Chronopoulos-Gear arrangement of PCG, in which both inner
// products of an iteration (gamma = r.u, delta = w.u with u = M^-1 r, w = A u)
// come from ONE reduction phase.  With z = A p kept as a recurrence,
// iteration i is
//     beta  = gamma_i / gamma_{i-1},   alpha = gamma_i / (delta_i - beta gamma_i / alpha_{i-1})
//     z_i   = w_i + beta z_{i-1}        p_i   = u_i + beta p_{i-1}
//     x    += alpha p_i                 r_i+1 = r_i - alpha z_i
//     u_i+1 = M^-1 r_i+1,  w_i+1 = A u_i+1,  partials of gamma_i+1, delta_i+1
// The launch boundary between the streaming update (k_cg_axpy) and the SpMV
// (k_cg_spmv) is the only grid-wide synchronisation.  Every workgroup of
// k_cg_axpy first reduces the previous launches' per-block partials itself
// (identical order in every block -> bit-identical alpha/beta everywhere, no
// atomics, no fan-in tail).
#include <cstdlib>
#include "xfk_kernels.h"
#include "xfk_spmv.h"

namespace xfk {

// Launch structure per iteration i (two launches, one reduction phase):
//   k_cg_axpy(i): reduce the gamma_i (own previous launch) and delta_i (SpMV)
//                 partials -> alpha, beta, convergence test; stream the own
//                 rows: z, p, x, r updated in place, u = M^-1 r written;
//                 partials gamma_i+1 = r.u.      88 B/row, vectorised 2 rows/lane
//   k_cg_spmv(i): w = A u (CSR-stream, LDS row tiles), partials delta_i+1 = u.w
constexpr int kAxBlock = 256;
constexpr int kAxGrid = 1024;             // fixed grid of the streaming kernel

// r0 = b - A x0 (x0 = 0 when flag == 0), u0 = M^-1 r0, z_{-1} = p_{-1} = 0;
// partials of (M^-1 b).b and gamma_0 = r0.u0
__global__ void __launch_bounds__(kCgBlock) k_cg_init_r(int N, int flag, const int *__restrict__ rowptr,
                                                        const int *__restrict__ col, const double *__restrict__ val,
                                                        const double *__restrict__ b, double *__restrict__ V,
                                                        double *__restrict__ R, double *__restrict__ U,
                                                        double *__restrict__ Z, double *__restrict__ P,
                                                        const double *__restrict__ dinv, double *__restrict__ part_reso,
                                                        double *__restrict__ part_gam0)
{
    __shared__ __attribute__((aligned(16))) double lds[kCgCap];
    __shared__ double red[2 * (kCgBlock / 64)];
    const int r0 = blockIdx.x * kCgBlock;
    double ax = 0.0;
    if (flag) ax = cg_tile_spmv(r0, N, rowptr, col, val, [&](int j) { return V[j]; }, lds);
    const int r = r0 + threadIdx.x;
    double ro = 0.0, g = 0.0;
    if (r < N) {
        const double br = b[r], di = dinv[r];
        const double rr = br - ax;
        const double u = di * rr;
        R[r] = rr;
        U[r] = u;
        Z[r] = 0.0;
        P[r] = 0.0;
        if (!flag) V[r] = 0.0;
        ro = (br * di) * br;
        g = rr * u;
    }
    cg_block_sum2(ro, g, red);
    if (threadIdx.x == 0) {
        part_reso[blockIdx.x] = ro;
        part_gam0[blockIdx.x] = g;
    }
}

// w = A u; partials delta = u.w and, when the preconditioner is applied
// outside the update kernel (AMG: R != nullptr), gamma = r.u as well
__global__ void __launch_bounds__(kCgBlock) k_cg_spmv(int N, const int *__restrict__ rowptr,
                                                      const int *__restrict__ col, const double *__restrict__ val,
                                                      const double *__restrict__ U, double *__restrict__ W,
                                                      double *__restrict__ part_del, const CgState *S,
                                                      const double *__restrict__ R, double *__restrict__ part_gam,
                                                      const int *__restrict__ tl, const unsigned short *__restrict__ c16,
                                                      const int *__restrict__ cbase)
{
    // the convergence flag, the tile's row range and this row's u, r are
    // loaded together before the first branch (one memory latency, not two)
    const int dn = load_flag_v(S ? &S->done : nullptr);
    __shared__ __attribute__((aligned(16))) double lds[kCgCap];
    __shared__ double red[2 * (kCgBlock / 64)];
    const int t = tl ? tl[xcd_tile(blockIdx.x, gridDim.x)] : xcd_tile(blockIdx.x, gridDim.x);
    const int r0 = t * kCgBlock;
    const int r = r0 + threadIdx.x;
    const TileRows tr = tile_rows(r0, N, rowptr);
    const int cb = load_col_base(cbase, t);
    const double u = r < N ? U[r] : 0.0, rr = (R && r < N) ? R[r] : 0.0;
    if (dn) return;
    const double w = cg_tile_spmv16(tr, c16, cb, col, val, [&](int j) { return U[j]; }, lds);
    double d = 0.0, g = 0.0;
    if (r < N) {
        W[r] = w;
        d = w * u;
        if (R) g = rr * u;
    }
    cg_block_sum2(d, g, red);
    if (threadIdx.x == 0) {
        part_del[t] = d;
        if (R) part_gam[t] = g;
    }
}

// one pair of deterministic sums over two partial arrays of different lengths
__device__ __forceinline__ void cg_reduce2(const double *__restrict__ pa, int Ga, const double *__restrict__ pb,
                                           int Gb, double &a, double &b, double *red)
{
    // four independent accumulators per array so the loads overlap (a fixed
    // order: every block, every run gets the same bits)
    double sa[4] = {0.0, 0.0, 0.0, 0.0}, sb[4] = {0.0, 0.0, 0.0, 0.0};
    const int st = blockDim.x;
    int i = threadIdx.x;
    for (; i + 3 * st < Ga; i += 4 * st)
#pragma unroll
        for (int m = 0; m < 4; ++m) sa[m] += pa[i + m * st];
    for (; i < Ga; i += st) sa[0] += pa[i];
    i = threadIdx.x;
    for (; i + 3 * st < Gb; i += 4 * st)
#pragma unroll
        for (int m = 0; m < 4; ++m) sb[m] += pb[i + m * st];
    for (; i < Gb; i += st) sb[0] += pb[i];
    double ra = (sa[0] + sa[1]) + (sa[2] + sa[3]), rb = (sb[0] + sb[1]) + (sb[2] + sb[3]);
    cg_block_sum2(ra, rb, red);
    a = ra;
    b = rb;
}

// CgAxpyArgs: xfk_kernels.h
__global__ void __launch_bounds__(kAxBlock) k_cg_axpy(CgAxpyArgs A)
{
    __shared__ double red[2 * (kAxBlock / 64)];
    CgState *S = A.S;
    const int dn = load_flag_v(&S->done);
    // AMG form: the first two row pairs of this thread are loaded before the
    // partial reduction (they do not depend on alpha, beta), so the stream is
    // in flight while the partials are summed (and while the flag arrives)
    const int npair = A.N >> 1;
    const int k0 = blockIdx.x * kAxBlock + threadIdx.x, kst = gridDim.x * kAxBlock;
    double2 pf[2][6];
    if (A.amg) {
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int k = k0 + q * kst;
            if (k < npair) {
                pf[q][0] = reinterpret_cast<const double2 *>(A.W)[k];
                pf[q][1] = reinterpret_cast<const double2 *>(A.Z)[k];
                pf[q][2] = reinterpret_cast<const double2 *>(A.P)[k];
                pf[q][3] = reinterpret_cast<const double2 *>(A.V)[k];
                pf[q][4] = reinterpret_cast<const double2 *>(A.R)[k];
                pf[q][5] = reinterpret_cast<const double2 *>(A.U)[k];
            }
        }
    }
    if (dn) return;
    double gam, del;
    cg_reduce2(A.gam_in, A.Ggam, A.del_in, A.Gdel, gam, del, red);
    double res_o;
    if (A.it == 0) {
        double unused;
        cg_reduce2(A.reso, A.Gdel, A.reso, 0, res_o, unused, red);
    } else {
        res_o = S->res_o;
    }
    double beta = 0.0, alpha;
    if (A.it == 0) {
        alpha = gam / del;
    } else {
        const double gp = S->gam[(A.it - 1) & 1], ap = S->alp[(A.it - 1) & 1];
        beta = gam / gp;
        alpha = gam / (del - beta * gam / ap);
    }
    const double er = (res_o == 0.0) ? 0.0 : sqrt(gam / res_o);
    // spars.cpp:259, 313; an inexact Newton pass also stops once the residual
    // ratio fell by tol_rel from its iteration-0 value.  gamma_0 == 0 is an
    // initial guess whose residual is exactly zero: alpha would be 0 / 0 and
    // its NaN er would never meet the test, so the guess is the answer
    const bool stop = (res_o == 0.0) || (A.it == 0 && gam == 0.0) ||
                      (A.it >= 1 && (er <= S->tol || er <= S->tol_rel * S->er0));
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        if (A.it == 0) {
            S->res_o = res_o;
            S->er0 = er;
        }
        S->er = er;
        S->iters = A.it;
        if (stop) S->done = 1;
        S->gam[A.it & 1] = gam;
        S->alp[A.it & 1] = alpha;
    }
    if (stop) return;
    const int N = A.N;
    if (A.amg) {
        // u_i is the V-cycle output already in U; r.u partials come from the SpMV
        const double2 *U2c = reinterpret_cast<const double2 *>(A.U);
        double2 *Z2 = reinterpret_cast<double2 *>(A.Z);
        double2 *P2 = reinterpret_cast<double2 *>(A.P);
        double2 *V2 = reinterpret_cast<double2 *>(A.V);
        double2 *R2 = reinterpret_cast<double2 *>(A.R);
        const double2 *W2 = reinterpret_cast<const double2 *>(A.W);
        auto upd = [&](int k, double2 w, double2 zo, double2 po, double2 x, double2 ri, double2 u) {
            double2 z, p, rn, xn;
            z.x = w.x + beta * zo.x;          z.y = w.y + beta * zo.y;
            p.x = u.x + beta * po.x;          p.y = u.y + beta * po.y;
            rn.x = ri.x - alpha * z.x;        rn.y = ri.y - alpha * z.y;
            xn.x = x.x + alpha * p.x;         xn.y = x.y + alpha * p.y;
            Z2[k] = z; P2[k] = p; V2[k] = xn; R2[k] = rn;
        };
        if (k0 < npair) upd(k0, pf[0][0], pf[0][1], pf[0][2], pf[0][3], pf[0][4], pf[0][5]);
        if (k0 + kst < npair) upd(k0 + kst, pf[1][0], pf[1][1], pf[1][2], pf[1][3], pf[1][4], pf[1][5]);
        for (int k = k0 + 2 * kst; k < npair; k += kst) upd(k, W2[k], Z2[k], P2[k], V2[k], R2[k], U2c[k]);
        if ((N & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
            const int r = N - 1;
            const double z = A.W[r] + beta * A.Z[r];
            const double p = A.U[r] + beta * A.P[r];
            A.V[r] = A.V[r] + alpha * p;
            A.R[r] = A.R[r] - alpha * z;
            A.Z[r] = z; A.P[r] = p;
        }
        return;
    }
    double g = 0.0;
    const double2 *W2 = reinterpret_cast<const double2 *>(A.W);
    double2 *Z2 = reinterpret_cast<double2 *>(A.Z);
    double2 *P2 = reinterpret_cast<double2 *>(A.P);
    double2 *V2 = reinterpret_cast<double2 *>(A.V);
    double2 *R2 = reinterpret_cast<double2 *>(A.R);
    double2 *U2 = reinterpret_cast<double2 *>(A.U);
    const double2 *D2 = reinterpret_cast<const double2 *>(A.dinv);
    for (int k = blockIdx.x * kAxBlock + threadIdx.x; k < npair; k += gridDim.x * kAxBlock) {
        const double2 w = W2[k], zo = Z2[k], po = P2[k], x = V2[k], ri = R2[k], di = D2[k];
        double2 z, p, rn, u;
        z.x = w.x + beta * zo.x;          z.y = w.y + beta * zo.y;
        p.x = di.x * ri.x + beta * po.x;  p.y = di.y * ri.y + beta * po.y;
        rn.x = ri.x - alpha * z.x;        rn.y = ri.y - alpha * z.y;
        u.x = di.x * rn.x;                u.y = di.y * rn.y;
        double2 xn;
        xn.x = x.x + alpha * p.x;         xn.y = x.y + alpha * p.y;
        Z2[k] = z; P2[k] = p; V2[k] = xn; R2[k] = rn; U2[k] = u;
        g += rn.x * u.x + rn.y * u.y;
    }
    if ((N & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
        const int r = N - 1;
        const double z = A.W[r] + beta * A.Z[r];
        const double p = A.dinv[r] * A.R[r] + beta * A.P[r];
        const double rn = A.R[r] - alpha * z;
        const double u = A.dinv[r] * rn;
        A.V[r] = A.V[r] + alpha * p;
        A.Z[r] = z; A.P[r] = p; A.R[r] = rn; A.U[r] = u;
        g += rn * u;
    }
    double zero = 0.0;
    cg_block_sum2(g, zero, red);
    if (threadIdx.x == 0) A.gam_out[blockIdx.x] = g;
}

// the PCG state of a new solve (one launch instead of a host -> device copy)
__global__ void k_cg_state_init(CgState *S, double tol, double tol_rel)
{
    if (threadIdx.x == 0) {
        CgState z{};
        z.tol = tol;
        z.tol_rel = tol_rel;
        *S = z;
    }
}

void launch_cg_state_init(hipStream_t s, CgState *S, double tol, double tol_rel)
{
    k_cg_state_init<<<1, 64, 0, s>>>(S, tol, tol_rel);
}

int cg_grid(int N) { return (N + kCgBlock - 1) / kCgBlock; }
int cg_axpy_grid(int N)
{
    int g = (N / 2 + kAxBlock - 1) / kAxBlock;
    return g < 1 ? 1 : (g < kAxGrid ? g : kAxGrid);
}

void launch_cg_init_r(hipStream_t s, int N, int flag, const int *rowptr, const int *col, const double *val,
                      const double *b, double *V, double *R, double *U, double *Z, double *P, const double *dinv,
                      double *part_reso, double *part_gam0)
{
    k_cg_init_r<<<cg_grid(N), kCgBlock, 0, s>>>(N, flag, rowptr, col, val, b, V, R, U, Z, P, dinv, part_reso,
                                                part_gam0);
}

void launch_cg_axpy(hipStream_t s, const CgAxpyArgs &A)
{
    k_cg_axpy<<<cg_axpy_grid(A.N), kAxBlock, 0, s>>>(A);
}

void launch_cg_spmv(hipStream_t s, int N, const int *rowptr, const int *col, const double *val, const double *U,
                    double *W, double *part_del, const CgState *S, const double *R, double *part_gam,
                    const int *tiles, int ntiles, const unsigned short *c16, const int *cbase)
{
    if (tiles && ntiles == 0) return;
    k_cg_spmv<<<tiles ? ntiles : cg_grid(N), kCgBlock, 0, s>>>(N, rowptr, col, val, U, W, part_del, S, R, part_gam,
                                                               tiles, c16, cbase);
}

// partials of a.b over the cg_grid(N) layout (the AMG start: (M^-1 b).b)
__global__ void __launch_bounds__(kCgBlock) k_cg_dot(int N, const double *__restrict__ a, const double *__restrict__ b,
                                                     double *__restrict__ part)
{
    __shared__ double red[2 * (kCgBlock / 64)];
    const int r = blockIdx.x * kCgBlock + threadIdx.x;
    double d = (r < N) ? a[r] * b[r] : 0.0, zero = 0.0;
    cg_block_sum2(d, zero, red);
    if (threadIdx.x == 0) part[blockIdx.x] = d;
}

void launch_cg_dot(hipStream_t s, int N, const double *a, const double *b, double *part)
{
    k_cg_dot<<<cg_grid(N), kCgBlock, 0, s>>>(N, a, b, part);
}

}  // namespace xfk

// xfk_device_init: loads this translation unit's code object onto the device
// (the first use of any of its kernels would otherwise do it inside a solve)
hipError_t xfk::warm_module_pcg()
{
    hipFuncAttributes a;
    return hipFuncGetAttributes(&a, reinterpret_cast<const void *>(&k_cg_init_r));
}
