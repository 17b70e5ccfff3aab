// The AMG cycle (xfk_amg.h): smoothers, SpMV, the folded pre- and post-steps,
// the dense coarsest product, their launchers and the V/W-cycle hosts.
#include <algorithm>
#include <string>

#include "xfk_amg_impl.h"
#include "xfk_comm.h"

namespace xfk {

namespace {

// --------------------------------------------------------------------------
// V-cycle kernels
// --------------------------------------------------------------------------

enum SmoothMode {
    kSweepFromZero = 0,   // x1 = w D^-1 b implicit, out = x1 + w D^-1 (b - A x1)
    kSweep = 1,           // out = x + w D^-1 (b - A x)
    kResid = 2,           // r = b - A x
    kResidFromZero = 3    // x1 = w D^-1 b (written to out), r = b - A x1
};

template <int MODE>
__device__ __forceinline__ void smooth_finish(int i, double ax, double w, const double *__restrict__ dinv,
                                              const double *__restrict__ b, const double *__restrict__ x,
                                              double *__restrict__ out, double *__restrict__ rout)
{
    constexpr bool implicit = (MODE == kSweepFromZero || MODE == kResidFromZero);
    const double bi = b[i], di = dinv[i];
    const double xi = implicit ? w * di * bi : x[i];
    const double res = bi - ax;
    if constexpr (MODE == kSweepFromZero || MODE == kSweep) out[i] = xi + w * di * res;
    if constexpr (MODE == kResid || MODE == kResidFromZero) rout[i] = res;
    if constexpr (MODE == kResidFromZero)
        if (out) out[i] = xi;   // (a folded level-0 post-step recomputes x_pre: not written)
}

// smooth_finish with the row's b, D^-1 and x already loaded; returns out[i]
template <int MODE>
__device__ __forceinline__ double smooth_finish_v(int i, double ax, double w, double di, double bi, double xv,
                                                  double *__restrict__ out, double *__restrict__ rout)
{
    constexpr bool implicit = (MODE == kSweepFromZero || MODE == kResidFromZero);
    const double xi = implicit ? w * di * bi : xv;
    const double res = bi - ax;
    double o = xi;
    if constexpr (MODE == kSweepFromZero || MODE == kSweep) {
        o = xi + w * di * res;
        out[i] = o;
    }
    if constexpr (MODE == kResid || MODE == kResidFromZero) rout[i] = res;
    if constexpr (MODE == kResidFromZero)
        if (out) out[i] = xi;   // (a folded level-0 post-step recomputes x_pre: not written)
    return o;
}

// CSR-stream tile SpMV (the PCG's kernel shape): B = 1024 on level 0, 256 on
// large coarse levels (more workgroups than CUs)
// part_gam (the PCG's last level-0 sweep only): per-tile partials of
// b . out, i.e. gamma = r . u of the CG, in the layout and summation order of
// k_cg_spmv's (same tiles, same workgroup sum), so the SpMV need not read r
template <int MODE, int B, int SLOTS = 2, class V = double>
__global__ void __launch_bounds__(B) k_amg_smooth(int n, int ncl, const int *__restrict__ rowptr,
                                                         const int *__restrict__ col, const V *__restrict__ val,
                                                         const double *__restrict__ dinv,
                                                         const unsigned long long *rho, const double *__restrict__ b,
                                                         const double *__restrict__ x, double *__restrict__ out,
                                                         double *__restrict__ rout, const int *done,
                                                         double *__restrict__ part_gam, const int *__restrict__ tl,
                                                         const unsigned short *__restrict__ c16 = nullptr,
                                                         const int *__restrict__ cbase = nullptr)
{
    // the convergence flag, rho, the tile's row range and this row's b,
    // D^-1, x are loaded together before the first branch
    const int dn = load_flag_v(done);
    __shared__ __attribute__((aligned(16))) double lds[4 * SLOTS * B];
    const double ra = rho_of(rho);
    const int t = tl ? tl[xcd_tile(blockIdx.x, gridDim.x)] : xcd_tile(blockIdx.x, gridDim.x);
    const int r0 = t * B;
    const int i = r0 + threadIdx.x;
    constexpr bool implicit = (MODE == kSweepFromZero || MODE == kResidFromZero);
    const TileRows tr = tile_rows<B>(r0, n, rowptr);
    const int cb = load_col_base(cbase, t);
    const double bi = i < n ? b[i] : 0.0, di = i < n ? dinv[i] : 0.0;
    const double xv = (!implicit && i < n) ? x[i] : 0.0;
    if (dn) return;
    const double w = ra > 0.0 ? 1.0 / ra : 0.0;
    double ax;
    if constexpr (implicit)
        ax = cg_tile_spmv16<B, SLOTS>(tr, c16, cb, col, val,
                                      [&](int j) { return j < ncl ? w * dinv[j] * b[j] : 0.0; }, lds);
    else
        ax = cg_tile_spmv16<B, SLOTS>(tr, c16, cb, col, val, [&](int j) { return j < ncl ? x[j] : 0.0; }, lds);
    double oi = 0.0;
    if (i < n) oi = smooth_finish_v<MODE>(i, ax, w, di, bi, xv, out, rout);
    if constexpr (MODE == kSweep) {
        if (part_gam) {   // uniform per launch
            __shared__ double red[2 * (B / 64)];
            double g = 0.0, zero = 0.0;
            if (i < n) g = bi * oi;
            cg_block_sum2(zero, g, red);
            if (threadIdx.x == 0) part_gam[t] = g;
        }
    }
}

// G lanes per row, strided over the row, butterfly sum inside the group
template <int G, class XF>
__device__ __forceinline__ double group_row_dot(int i, int n, const int *__restrict__ rowptr,
                                                const int *__restrict__ col, const double *__restrict__ val, XF X)
{
    const int g = threadIdx.x & (G - 1);
    double s = 0.0;
    if (i < n)
        for (int k = rowptr[i] + g; k < rowptr[i + 1]; k += G) s += val[k] * X(col[k]);
#pragma unroll
    for (int off = G >> 1; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
    return s;
}

// coarse levels: G lanes per row
template <int MODE, int G>
__global__ void __launch_bounds__(256) k_amg_smooth_g(int n, int ncl, const int *__restrict__ rowptr,
                                                      const int *__restrict__ col, const double *__restrict__ val,
                                                      const double *__restrict__ dinv, const unsigned long long *rho,
                                                      const double *__restrict__ b, const double *__restrict__ x,
                                                      double *__restrict__ out, double *__restrict__ rout,
                                                      const int *done)
{
    if (done && *done) return;
    const double ra = rho_of(rho);
    const double w = ra > 0.0 ? 1.0 / ra : 0.0;
    const int i = (xcd_tile(blockIdx.x, gridDim.x) * blockDim.x + threadIdx.x) / G;
    constexpr bool implicit = (MODE == kSweepFromZero || MODE == kResidFromZero);
    double ax;
    if constexpr (implicit)
        ax = group_row_dot<G>(i, n, rowptr, col, val, [&](int j) { return j < ncl ? w * dinv[j] * b[j] : 0.0; });
    else
        ax = group_row_dot<G>(i, n, rowptr, col, val, [&](int j) { return j < ncl ? x[j] : 0.0; });
    if (i < n && (threadIdx.x & (G - 1)) == 0) smooth_finish<MODE>(i, ax, w, dinv, b, x, out, rout);
}

// y = M x (ACC: y += M x), tile form (large transfer operators)
template <int B, bool ACC, int SLOTS = 2, class V = double>
__global__ void __launch_bounds__(B) k_csr_mv_tile(int n, const int *__restrict__ rowptr, const int *__restrict__ col,
                                                   const V *__restrict__ val, const double *__restrict__ x,
                                                   double *__restrict__ y, const int *done,
                                                   const unsigned short *__restrict__ c16 = nullptr,
                                                   const int *__restrict__ cbase = nullptr)
{
    const int dn = load_flag_v(done);
    __shared__ __attribute__((aligned(16))) double lds[4 * SLOTS * B];
    const int t = xcd_tile(blockIdx.x, gridDim.x);
    const int r0 = t * B;
    const int i = r0 + threadIdx.x;
    const TileRows tr = tile_rows<B>(r0, n, rowptr);
    const int cb = load_col_base(cbase, t);
    const double y0 = (ACC && i < n) ? y[i] : 0.0;
    if (dn) return;
    const double s = cg_tile_spmv16<B, SLOTS>(tr, c16, cb, col, val, [&](int j) { return x[j]; }, lds);
    if (i < n) y[i] = ACC ? y0 + s : s;
}

// y = M x (ACC: y += M x), G lanes per row (restriction R r, prolongation x += P xc)
template <int G, bool ACC>
__global__ void __launch_bounds__(256) k_csr_mv_g(int n, const int *__restrict__ rowptr, const int *__restrict__ col,
                                                  const double *__restrict__ val, const double *__restrict__ x,
                                                  double *__restrict__ y, const int *done)
{
    if (done && *done) return;
    const int i = (xcd_tile(blockIdx.x, gridDim.x) * blockDim.x + threadIdx.x) / G;
    const double s = group_row_dot<G>(i, n, rowptr, col, val, [&](int j) { return x[j]; });
    if (i < n && (threadIdx.x & (G - 1)) == 0) y[i] = ACC ? y[i] + s : s;
}

// level 0, folded post-step (the pre-step stays sweep-from-0 + residual and
// R r'): u = x_pre + w D^-1 r' + P~ x_c, i.e. the prolongation and the
// post-sweep in one pass over P~ instead of P and A.  Tile shape and r.u
// partials as k_amg_smooth's last sweep (the SpMV's tiles and summation order).
template <int B, int SLOTS, class V>
__global__ void __launch_bounds__(B) k_fold_post0(int n, const int *__restrict__ frow, const int *__restrict__ fcol,
                                                  const V *__restrict__ fval, const double *__restrict__ xc,
                                                  const double *__restrict__ dinv, const unsigned long long *rho,
                                                  const double *__restrict__ rres,
                                                  const double *__restrict__ b, double *__restrict__ out,
                                                  const int *done, double *__restrict__ part_gam,
                                                  const unsigned short *__restrict__ c16,
                                                  const int *__restrict__ cbase)
{
    const int dn = load_flag_v(done);
    __shared__ __attribute__((aligned(16))) double lds[4 * SLOTS * B];
    const double ra = rho_of(rho);
    const int t = xcd_tile(blockIdx.x, gridDim.x);
    const int r0 = t * B;
    const int i = r0 + threadIdx.x;
    const TileRows tr = tile_rows<B>(r0, n, frow);
    const int cb = load_col_base(cbase, t);
    const double di = i < n ? dinv[i] : 0.0, bi = i < n ? b[i] : 0.0, ri = i < n ? rres[i] : 0.0;
    if (dn) return;
    const double w = ra > 0.0 ? 1.0 / ra : 0.0;
    const double pc = cg_tile_spmv16<B, SLOTS>(tr, c16, cb, fcol, fval, [&](int j) { return xc[j]; }, lds);
    double u = 0.0;
    if (i < n) {
        u = (w * di * bi + w * di * ri) + pc;
        out[i] = u;
    }
    if (part_gam) {   // uniform per launch
        __shared__ double red[2 * (B / 64)];
        double g = 0.0, zero = 0.0;
        if (i < n) g = bi * u;
        cg_block_sum2(zero, g, red);
        if (threadIdx.x == 0) part_gam[t] = g;
    }
}

// the folded pre-step: workgroups [0, blocks_a) form y (GA lanes per fine
// row), the rest b_c = P~^T b (GB lanes per coarse row)
template <int GA, int GB>
__global__ void __launch_bounds__(256) k_fold_pre(int n, int ncl, const int *__restrict__ rowptr,
                                                  const int *__restrict__ col, const double *__restrict__ val,
                                                  const double *__restrict__ dinv, const unsigned long long *rho,
                                                  const double *__restrict__ b, double *__restrict__ y, int nc,
                                                  const int *__restrict__ rrow, const int *__restrict__ rcol,
                                                  const double *__restrict__ rval, double *__restrict__ bc,
                                                  int blocks_a, const int *done, const double *__restrict__ yadd)
{
    if (done && *done) return;
    // XCD-contiguous row blocks in each range (blocks_a is a multiple of 8):
    // an XCD's L2 serves the vector entries its neighbouring rows share
    if ((int)blockIdx.x < blocks_a) {
        const double ra = rho_of(rho);
        const double w = ra > 0.0 ? 1.0 / ra : 0.0;
        const int i = (xcd_tile(blockIdx.x, blocks_a) * blockDim.x + threadIdx.x) / GA;
        const double ax =
            group_row_dot<GA>(i, n, rowptr, col, val, [&](int j) { return j < ncl ? w * dinv[j] * b[j] : 0.0; });
        if (i < n && (threadIdx.x & (GA - 1)) == 0) {
            const double di = dinv[i], bi = b[i], xi = w * di * bi;
            const double yi = xi + w * di * (bi - ax);
            y[i] = yadd ? yadd[i] + yi : yi;   // (a W-cycle's second correction adds onto the first)
        }
    } else {
        const int c = (xcd_tile(blockIdx.x - blocks_a, gridDim.x - blocks_a) * blockDim.x + threadIdx.x) / GB;
        const double sc = group_row_dot<GB>(c, nc, rrow, rcol, rval, [&](int j) { return b[j]; });
        if (c < nc && (threadIdx.x & (GB - 1)) == 0) bc[c] = sc;
    }
}

// x = M b, one 256-thread workgroup per row of the f32 inverse (ld a multiple
// of 64, padding columns zero): every thread issues its 16-B loads (4 floats)
// of the row at once, so the whole inverse is in flight (one wave per row
// left a 1.6k-row inverse at 2.3 TB/s: 6 waves per CU, each walking its row
// in dependent batches); products and sums in f64
constexpr int kDmvLoads = 2;
template <class V>
struct DmvVec;
template <>
struct DmvVec<float> {
    using T = float4;
};
template <>
struct DmvVec<double> {
    struct T {
        double x, y, z, w;
    };
};
// x = S M S b: row i of the symmetrised scaled inverse M (f32 or f64), the
// scale osc in f64, products and sums in f64
template <class V>
__global__ void __launch_bounds__(256) k_dense_mv(int n, int ld, const V *__restrict__ M,
                                                  const double *__restrict__ osc, const double *__restrict__ b,
                                                  double *__restrict__ x, const int *done)
{
    if (done && *done) return;
    using V4 = typename DmvVec<V>::T;
    __shared__ double red[4];
    const int i = blockIdx.x;
    const V4 *Mi = reinterpret_cast<const V4 *>(M + (size_t)i * ld);
    const int n4 = ld >> 2;
    double s0 = 0.0, s1 = 0.0;
    for (int j0 = 0; j0 < n4; j0 += 256 * kDmvLoads) {
        V4 m[kDmvLoads];
#pragma unroll
        for (int q = 0; q < kDmvLoads; ++q) {
            const int j = j0 + threadIdx.x + 256 * q;
            if (j < n4) m[q] = Mi[j];
            else m[q] = V4{0, 0, 0, 0};
        }
#pragma unroll
        for (int q = 0; q < kDmvLoads; ++q) {
            const int c = 4 * (j0 + threadIdx.x + 256 * q);
            if (c + 3 < n) {
                const double2 b0 = *reinterpret_cast<const double2 *>(b + c);
                const double2 b1 = *reinterpret_cast<const double2 *>(b + c + 2);
                const double2 c0 = *reinterpret_cast<const double2 *>(osc + c);
                const double2 c1 = *reinterpret_cast<const double2 *>(osc + c + 2);
                s0 += (double)m[q].x * (c0.x * b0.x) + (double)m[q].z * (c1.x * b1.x);
                s1 += (double)m[q].y * (c0.y * b0.y) + (double)m[q].w * (c1.y * b1.y);
            } else {
                if (c < n) s0 += (double)m[q].x * (osc[c] * b[c]);
                if (c + 1 < n) s1 += (double)m[q].y * (osc[c + 1] * b[c + 1]);
                if (c + 2 < n) s0 += (double)m[q].z * (osc[c + 2] * b[c + 2]);
            }
        }
    }
    const double w = cg_wave_sum(s0 + s1);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = w;
    __syncthreads();
    if (threadIdx.x == 0) x[i] = osc[i] * ((red[0] + red[1]) + (red[2] + red[3]));
}

// sharded levels
// x = w D^-1 b: the first Jacobi sweep from zero, written out (its halo is
// exchanged before the residual)
__global__ void k_jacobi_first(int n, const unsigned long long *rho, const double *__restrict__ dinv,
                               const double *__restrict__ b, double *__restrict__ x, const int *done)
{
    if (done && *done) return;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double ra = rho_of(rho);
    x[i] = (ra > 0.0 ? 1.0 / ra : 0.0) * dinv[i] * b[i];
}
// global coarse vector from the padded all-gather (stride ld per rank)
__global__ void k_unpad(int NC, int nranks, const int *__restrict__ c0, const double *__restrict__ all, int ld,
                        double *__restrict__ out, const int *done)
{
    if (done && *done) return;
    const int I = blockIdx.x * blockDim.x + threadIdx.x;
    if (I >= NC) return;
    int q = 0;
    while (c0[q + 1] <= I) ++q;
    out[I] = all[(size_t)q * ld + (I - c0[q])];
}

// levels / transfer operators with at least this many rows use the tile kernels
constexpr int kTileMinRows = 16384;

// lanes per row for a CSR with this many nonzeros per row on average
int lanes_for(double per_row)
{
    return per_row <= 6.0 ? 4 : (per_row <= 20.0 ? 8 : 16);
}

// The 256-row tile kernels, for f64 values (launch_mv: levels of >= kTileMinRows
// rows) and level 0's f32 values (level 0 always has that many rows).
// G <= 4: 2 staging slots per lane; G = 8: 7..20 entries per row -> 6 slots
// per lane, one staging pass per tile
// (128- and 64-row tiles for R's ~25-entry rows were measured slower: 14.4 -> 15.0 / 15.6 us,
// profiles/r04_experiments/r04h_XFK_R0_TILE_*.json)
// staging slots per lane for the long rows: 6 = 6144 products per pass (R's
// ~27-entry rows fill 256-row tiles with ~6900); 8 / 7 (one pass, 64 / 56 KiB
// of LDS) measured 20.3 / 20.2 us vs 14.7 us
// c16 / cbase: 16-bit column offsets in 256-row tiles (null: the int columns)
template <class V>
void launch_mv_tile(hipStream_t s, int n, const int *rowptr, const int *col, const V *val, const double *x, double *y,
                    bool acc, int G, const int *done, const unsigned short *c16, const int *cbase)
{
    if (n <= 0) return;
    const int g = (n + 255) / 256;
    if (G <= 4) {
        if (acc) k_csr_mv_tile<256, true, 2><<<g, 256, 0, s>>>(n, rowptr, col, val, x, y, done, c16, cbase);
        else k_csr_mv_tile<256, false, 2><<<g, 256, 0, s>>>(n, rowptr, col, val, x, y, done, c16, cbase);
    } else {
        if (acc) k_csr_mv_tile<256, true, 6><<<g, 256, 0, s>>>(n, rowptr, col, val, x, y, done, c16, cbase);
        else k_csr_mv_tile<256, false, 6><<<g, 256, 0, s>>>(n, rowptr, col, val, x, y, done, c16, cbase);
    }
}

// c16 / cbase: used by the tile kernels only
void launch_mv(hipStream_t s, int n, const int *rowptr, const int *col, const double *val, const double *x, double *y,
               bool acc, int G, const int *done, const unsigned short *c16 = nullptr, const int *cbase = nullptr)
{
    if (n <= 0) return;
    if (n >= kTileMinRows && G <= 8) return launch_mv_tile(s, n, rowptr, col, val, x, y, acc, G, done, c16, cbase);
    const int g = (int)(((long long)n * G + 255) / 256);
#define XFK_MV(GG)                                                                                        \
    if (acc) k_csr_mv_g<GG, true><<<g, 256, 0, s>>>(n, rowptr, col, val, x, y, done);                    \
    else k_csr_mv_g<GG, false><<<g, 256, 0, s>>>(n, rowptr, col, val, x, y, done);
    if (G == 4) { XFK_MV(4) } else if (G == 8) { XFK_MV(8) } else { XFK_MV(16) }
#undef XFK_MV
}

// which: 0 every row; 1 / 2 the interior / boundary tiles of A.ts (tile levels)
template <int MODE>
void launch_smooth_t(hipStream_t s, int l, const AmgLevel &A, const unsigned long long *rho, const double *b,
                     const double *x, double *out, double *rout, const int *done, double *part_gam, int which)
{
    const int *tl = nullptr;
    int nt = 0;
    if (which) {
        tl = A.ts.tiles.p + (which == 2 ? A.ts.n_in : 0);
        nt = which == 1 ? A.ts.n_in : A.ts.n_bd;
        if (nt == 0) return;
    }
    if (l == 0) {
        const int g = tl ? nt : (A.n + kCgBlock - 1) / kCgBlock;
        k_amg_smooth<MODE, kCgBlock><<<g, kCgBlock, 0, s>>>(A.n, A.ncol_smooth, A.rowptr, A.col, A.val, A.dinv.p, rho,
                                                            b, x, out, rout, done, part_gam, tl,
                                                            A.has16 ? A.a16.p : nullptr, A.has16 ? A.a16b.p : nullptr);
        return;
    }
    if (A.n >= kTileMinRows) {
        // coarse levels carry 10-16 entries per row: 4 slots per lane, one pass per tile
        const int g = tl ? nt : (A.n + 255) / 256;
        if ((double)A.nnz <= 8.0 * A.n)
            k_amg_smooth<MODE, 256, 2><<<g, 256, 0, s>>>(A.n, A.ncol_smooth, A.rowptr, A.col, A.val, A.dinv.p, rho, b,
                                                         x, out, rout, done, nullptr, tl);
        else
            k_amg_smooth<MODE, 256, 4><<<g, 256, 0, s>>>(A.n, A.ncol_smooth, A.rowptr, A.col, A.val, A.dinv.p, rho, b,
                                                         x, out, rout, done, nullptr, tl);
        return;
    }
    const int G = lanes_for(A.n > 0 ? (double)A.nnz / A.n : 1.0);
    const int g = (int)(((long long)A.n * G + 255) / 256);
    if (G == 4)
        k_amg_smooth_g<MODE, 4><<<g, 256, 0, s>>>(A.n, A.ncol_smooth, A.rowptr, A.col, A.val, A.dinv.p, rho, b, x, out,
                                                 rout, done);
    else if (G == 8)
        k_amg_smooth_g<MODE, 8><<<g, 256, 0, s>>>(A.n, A.ncol_smooth, A.rowptr, A.col, A.val, A.dinv.p, rho, b, x, out,
                                                 rout, done);
    else
        k_amg_smooth_g<MODE, 16><<<g, 256, 0, s>>>(A.n, A.ncol_smooth, A.rowptr, A.col, A.val, A.dinv.p, rho, b, x,
                                                  out, rout, done);
}

void launch_smooth(hipStream_t s, int mode, int l, const AmgLevel &A, const unsigned long long *rho, const double *b,
                   const double *x, double *out, double *rout, const int *done, double *part_gam = nullptr,
                   int which = 0)
{
    switch (mode) {
    case kSweepFromZero: launch_smooth_t<kSweepFromZero>(s, l, A, rho, b, x, out, rout, done, nullptr, which); break;
    case kSweep: launch_smooth_t<kSweep>(s, l, A, rho, b, x, out, rout, done, part_gam, which); break;
    case kResid: launch_smooth_t<kResid>(s, l, A, rho, b, x, out, rout, done, nullptr, which); break;
    default: launch_smooth_t<kResidFromZero>(s, l, A, rho, b, x, out, rout, done, nullptr, which); break;
    }
}

// lanes per row of the long R~ rows (up to one wavefront)
int lanes_wide(double per_row)
{
    return per_row <= 6.0 ? 4 : (per_row <= 20.0 ? 8 : (per_row <= 40.0 ? 16 : (per_row <= 80.0 ? 32 : 64)));
}

template <int GA>
void launch_fold_pre_a(hipStream_t s, const AmgLevel &A, const unsigned long long *rho, const double *b, double *y,
                       double *bc, const int *done, const double *yadd)
{
    const int GB = lanes_wide(A.nc > 0 ? (double)A.fnnz / A.nc : 1.0);
    // (the first range padded to whole rounds of the 8 XCDs, so both ranges
    // take the XCD-contiguous block order)
    const int ga = (int)(((((long long)A.n * GA + 255) / 256) + 7) & ~7LL);
    const int gb = (int)(((long long)A.nc * GB + 255) / 256);
#define XFK_FOLD(GG)                                                                                               \
    k_fold_pre<GA, GG><<<ga + gb, 256, 0, s>>>(A.n, A.ncol_smooth, A.rowptr, A.col, A.val, A.dinv.p, rho, b, y,   \
                                               A.nc, A.frrow.p, A.frcol.p, A.frval.p, bc, ga, done, yadd)
    switch (GB) {
    case 4: XFK_FOLD(4); break;
    case 8: XFK_FOLD(8); break;
    case 16: XFK_FOLD(16); break;
    case 32: XFK_FOLD(32); break;
    default: XFK_FOLD(64); break;
    }
#undef XFK_FOLD
}

void launch_fold_pre(hipStream_t s, const AmgLevel &A, const unsigned long long *rho, const double *b, double *y,
                     double *bc, const int *done, const double *yadd = nullptr)
{
    if (A.n <= 0) return;
    const int GA = lanes_for((double)A.nnz / A.n);
    if (GA == 4) launch_fold_pre_a<4>(s, A, rho, b, y, bc, done, yadd);
    else if (GA == 8) launch_fold_pre_a<8>(s, A, rho, b, y, bc, done, yadd);
    else launch_fold_pre_a<16>(s, A, rho, b, y, bc, done, yadd);
}

// tile size of the level's smoother launches (0: sub-wave kernels, no split)
int smooth_tile(int l, const AmgLevel &A) { return l == 0 ? kCgBlock : (A.n >= kTileMinRows ? 256 : 0); }

}  // namespace

// algorithmic bytes of one smoother launch (mode as launch_smooth): the
// matrix stream, the gathered operand once, b / D^-1, the written vectors
static double smooth_bytes(const AmgLevel &A, int mode)
{
    const double n = A.n, base = ((A.has16 ? 2.0 : 4.0) + 8.0) * (double)A.nnz + 4.0 * (n + 1);
    const bool implicit = mode == kSweepFromZero || mode == kResidFromZero;
    const double rd = (implicit ? 2.0 : 3.0) * 8.0 * n;
    const double wr = (mode == kResidFromZero && !A.fold ? 2.0 : 1.0) * 8.0 * n;
    return base + rd + wr;
}

static const char *smooth_name(int mode)
{
    switch (mode) {
    case kResidFromZero: return "sweep from 0 + residual";
    case kSweepFromZero: return "sweep from 0";
    case kResid: return "residual";
    default: return "sweep";
    }
}

static void smooth_ph(hipStream_t s, int mode, int l, const AmgLevel &A, const unsigned long long *rho,
                      const double *b, const double *x, double *out, double *rout, const int *done,
                      double *part_gam = nullptr)
{
    if (g_prof)
        XFK_PHASE("L" + std::to_string(l) + " " + smooth_name(mode) + (part_gam ? " (+ r.u partials)" : ""),
                  smooth_bytes(A, mode), launch_smooth(s, mode, l, A, rho, b, x, out, rout, done, part_gam));
    else
        launch_smooth(s, mode, l, A, rho, b, x, out, rout, done, part_gam);
}

// Symmetric V-cycle; returns the buffer holding the level's result.  Level 0
// writes its result to `out0`.
// (coarse folded / dense levels: yout = the result buffer instead of xa,
// yadd = a vector the result is added onto -- the W-cycle's second correction)
static double *vcycle_level(Amg &M, hipStream_t s, int l, const double *b, double *out0, const int *done,
                            double *part_gam = nullptr, double *yout = nullptr, const double *yadd = nullptr)
{
    AmgLevel &A = *M.L[l];
    const unsigned long long *rho = M.rho.p + 2 * l;
    const int nu = M.sweeps;
    auto other = [&](double *c) { return c == A.xa.p ? A.xb.p : A.xa.p; };
    const std::string lv = g_prof ? "L" + std::to_string(l) + " " : std::string();
    if (l == M.nlev - 1) {
        double *dst = (l == 0) ? out0 : (yout ? yout : A.xa.p);
        if (M.dense_coarse) {
            if (M.cinv_f64)
                XFK_PHASE(lv + "dense inverse x b", 8.0 * A.n * M.cinv_ld + 8.0 * (2 * M.cinv_ld + A.n),
                          (k_dense_mv<double><<<A.n, 256, 0, s>>>(A.n, M.cinv_ld, M.cinv_o64.p, M.cinv_sc.p, b, dst,
                                                                  done)));
            else
                XFK_PHASE(lv + "dense inverse x b", 4.0 * A.n * M.cinv_ld + 8.0 * (2 * M.cinv_ld + A.n),
                          (k_dense_mv<float><<<A.n, 256, 0, s>>>(A.n, M.cinv_ld, M.cinv_apply, M.cinv_sc.p, b, dst,
                                                                 done)));
            return dst;
        }
        // smoother-only coarsest level: 2 nu sweeps from zero
        double *cur = A.xa.p;
        smooth_ph(s, kSweepFromZero, l, A, rho, b, nullptr, cur, nullptr, done);
        for (int k = 2; k < 2 * nu; ++k) {
            double *nx = (k == 2 * nu - 1 && l == 0) ? out0 : other(cur);
            smooth_ph(s, kSweep, l, A, rho, b, cur, nx, nullptr, done);
            cur = nx;
        }
        if (l == 0 && cur != out0)
            (void)hipMemcpyAsync(out0, cur, sizeof(double) * A.n, hipMemcpyDeviceToDevice, s);
        return cur;
    }
    if (A.fold && l > 0) {
        // two launches: y and the coarse right-hand side, then x = y + P~ x_c
        AmgLevel &C = *M.L[l + 1];
        double *y = yout ? yout : A.xa.p;
        const double n = A.n, nc = A.nc, f = (double)A.fnnz;
        XFK_PHASE(lv + "folded pre: y, R~ r", 12.0 * A.nnz + 4.0 * (n + 1) + 24.0 * n + 12.0 * f + 4.0 * (nc + 1) +
                                                   8.0 * nc + (yadd ? 8.0 * n : 0.0),
                  launch_fold_pre(s, A, rho, b, y, C.b.p, done, yadd));
        const double *xc;
        if (M.w_at(l)) {
            // W-cycle at this level: a second coarse correction from the
            // coarse residual after the first, b_c' = b_c - A_c x_c (Galerkin:
            // R (b - A (x_pre + P x_c)) = b_c - A_c x_c), x_c += V(b_c'); the
            // second visit adds its result onto the first (its folded
            // pre-step starts from x_c), so the post-step prolongs the sum.
            // Symmetric like the V-cycle; three launches more than it.
            const double *x1 = vcycle_level(M, s, l + 1, C.b.p, nullptr, done, nullptr, C.xb.p);
            smooth_ph(s, kResid, l + 1, C, M.rho.p + 2 * (l + 1), C.b.p, x1, nullptr, C.r.p, done);
            xc = vcycle_level(M, s, l + 1, C.r.p, nullptr, done, nullptr, C.xa.p, x1);
        } else {
            xc = vcycle_level(M, s, l + 1, C.b.p, nullptr, done);
        }
        XFK_PHASE(lv + "folded post: x = y + P~ xc", 12.0 * f + 4.0 * (n + 1) + 8.0 * nc + 16.0 * n,
                  launch_mv(s, A.n, A.ftrow.p, A.ftcol.p, A.ftval.p, xc, y, true, lanes_for(f / n), done));
        return y;
    }
    // pre-smoothing (nu sweeps from zero) and residual
    double *cur = A.xa.p;
    if (nu == 1) {
        // (a folded level 0 recomputes x_pre = w D^-1 b in its post-step)
        smooth_ph(s, kResidFromZero, l, A, rho, b, nullptr, (A.fold && l == 0) ? nullptr : cur, A.r.p, done);
    } else {
        smooth_ph(s, kSweepFromZero, l, A, rho, b, nullptr, cur, nullptr, done);
        for (int k = 2; k < nu; ++k) {
            double *nx = other(cur);
            smooth_ph(s, kSweep, l, A, rho, b, cur, nx, nullptr, done);
            cur = nx;
        }
        smooth_ph(s, kResid, l, A, rho, b, cur, nullptr, A.r.p, done);
    }
    AmgLevel &C = *M.L[l + 1];
    const long long rnnz = A.pnnz;
    XFK_PHASE(lv + "restriction R r", A.nz_bytes() * rnnz + 4.0 * (A.nc + 1) + 8.0 * A.n + 8.0 * A.nc,
              (A.has32 ? launch_mv_tile(s, A.nc, A.rrow.p, A.rcol.p, A.r32.p, A.r.p, C.b.p, false,
                                     lanes_for((double)rnnz / A.nc), done, A.r16.p, A.r16b.p)
                       : launch_mv(s, A.nc, A.rrow.p, A.rcol.p, A.rval.p, A.r.p, C.b.p, false,
                                   lanes_for((double)rnnz / A.nc), done, A.has16 ? A.r16.p : nullptr,
                                   A.has16 ? A.r16b.p : nullptr)));
    const double *xc = vcycle_level(M, s, l + 1, C.b.p, nullptr, done);
    if (A.fold && l == 0 && nu == 1) {
        const double n = A.n, f = (double)A.fnnz;
        XFK_PHASE(lv + "folded post: u = x + w D^-1 r + P~ xc" + (part_gam ? " (+ r.u partials)" : ""),
                  A.nz_bytes() * f + 4.0 * (n + 1) + 8.0 * A.nc + 32.0 * n,
                  (A.has32 ? k_fold_post0<kCgBlock, 2><<<(A.n + kCgBlock - 1) / kCgBlock, kCgBlock, 0, s>>>(
                                 A.n, A.ftrow.p, A.ftcol.p, A.f32v.p, xc, A.dinv.p, rho, A.r.p, b, out0, done,
                                 part_gam, A.f16.p, A.f16b.p)
                           : k_fold_post0<kCgBlock, 2><<<(A.n + kCgBlock - 1) / kCgBlock, kCgBlock, 0, s>>>(
                                 A.n, A.ftrow.p, A.ftcol.p, A.ftval.p, xc, A.dinv.p, rho, A.r.p, b, out0, done,
                                 part_gam, A.has16 ? A.f16.p : nullptr, A.has16 ? A.f16b.p : nullptr)));
        if (part_gam) M.gamma_done = true;
        return out0;
    }
    XFK_PHASE(lv + "prolongation x += P xc", 12.0 * rnnz + 4.0 * (A.n + 1) + 8.0 * A.nc + 16.0 * A.n,
              launch_mv(s, A.n, A.prow.p, A.pcol.p, A.pval.p, xc, cur, true, lanes_for((double)rnnz / A.n), done));
    for (int k = 0; k < nu; ++k) {
        const bool last0 = k == nu - 1 && l == 0;
        double *nx = last0 ? out0 : other(cur);
        smooth_ph(s, kSweep, l, A, rho, b, cur, nx, nullptr, done, last0 ? part_gam : nullptr);
        if (last0 && part_gam) M.gamma_done = true;
        cur = nx;
    }
    return cur;
}

// sharded level l: every sweep reads the peers' halo values of the iterate;
// the restriction / prolongation stay rank-local (P rows reference the own
// aggregates only).  Returns the buffer holding the result (`out` if given).
double *Amg::vc_dist(hipStream_t s, int l, const double *b, double *out, const int *done, int &rc)
{
    AmgLevel &A = *L[l];
    const unsigned long long *rh = rho.p + 2 * l;
    double *cur = A.xa.p, *oth = A.xb.p;
    rc = XFK_OK;
    // tile levels: the halo exchange of the iterate overlaps the interior tiles
    const int B = smooth_tile(l, A);
    const bool ov = B > 0 && overlap;
    if (ov && !A.ts.ready()) {
        if ((rc = side.init()) != XFK_OK) return nullptr;
        if ((rc = build_tile_split(s, A.n, B, A.rowptr, A.col, A.ts)) != XFK_OK) return nullptr;
    }
    // halo of x, then mode over the level's rows (interior tiles during the exchange)
    auto smooth_after_exchange = [&](int mode, double *x, double *o, double *ro, double *pg) -> int {
        if (!ov) {
            const int r = comm->exchange(A.plan, x, s);
            if (r != XFK_OK) return r;
            launch_smooth(s, mode, l, A, rh, b, x, o, ro, done, pg);
            return XFK_OK;
        }
        return exchange_overlapped(
            s, side, [&](hipStream_t cs) { return comm->exchange(A.plan, x, cs); },
            [&] { launch_smooth(s, mode, l, A, rh, b, x, o, ro, done, pg, 1); },
            [&] { launch_smooth(s, mode, l, A, rh, b, x, o, ro, done, pg, 2); });
    };
    if (A.n > 0) k_jacobi_first<<<nb(A.n), kB, 0, s>>>(A.n, rh, A.dinv.p, b, cur, done);
    for (int k = 1; k < sweeps; ++k) {
        if ((rc = smooth_after_exchange(kSweep, cur, oth, nullptr, nullptr)) != XFK_OK) return nullptr;
        std::swap(cur, oth);
    }
    if ((rc = smooth_after_exchange(kResid, cur, nullptr, A.r.p, nullptr)) != XFK_OK) return nullptr;
    AmgLevel &C = *L[l + 1];
    const int GR = lanes_for(A.nc > 0 ? (double)A.pnnz / A.nc : 1.0);
    const double *xc;
    // level 0 with f32 transfers: R and P in f32 with 16-bit tile columns
    auto restrict_to = [&](double *dst) {
        if (A.has32)
            launch_mv_tile(s, A.nc, A.rrow.p, A.rcol.p, A.r32.p, A.r.p, dst, false, GR, done, A.r16.p, A.r16b.p);
        else
            launch_mv(s, A.nc, A.rrow.p, A.rcol.p, A.rval.p, A.r.p, dst, false, GR, done);
    };
    const bool fold = A.fold && sweeps == 1;
    const double *xfull = nullptr;   // folded: x_c with the columns P~ reads (coarse halo / global)
    if (C.dist) {
        restrict_to(C.b.p);
        xc = vc_dist(s, l + 1, C.b.p, nullptr, done, rc);
        if (rc != XFK_OK) return nullptr;
        if (fold) {   // the coarse halo P~ reads (the next level's plan covers P~'s columns)
            double *xh = const_cast<double *>(xc);
            if ((rc = comm->exchange(C.plan, xh, s)) != XFK_OK) return nullptr;
            xfull = xh;
        }
    } else {
        // the replicated levels: gather the global right-hand side, solve the
        // same coarse problem on every rank, read the own aggregates back
        restrict_to(cb_loc.p);
        const int te = tail_begin(s, 0);
        if ((rc = comm->allgather(cb_loc.p, cb_all.p, (size_t)ncmax, s)) != XFK_OK) return nullptr;
        k_unpad<<<nb(C.n), kB, 0, s>>>(C.n, nranks, c0_dev.p, cb_all.p, ncmax, C.b.p, done);
        xfull = vcycle_level(*this, s, l + 1, C.b.p, nullptr, done);
        xc = xfull + c0[rank];
        tail_end(s, te);
    }
    if (fold) {
        // u = w D^-1 b + w D^-1 r' + P~ x_c over the own rows: the prolongation
        // and the post-sweep (whose halo exchange it replaces) in one pass
        double *o = out ? out : oth;
        if (A.n > 0) {
            double *pg = (l == 0 && out) ? part_gam_ : nullptr;
            if (l == 0) {
                const int g = (A.n + kCgBlock - 1) / kCgBlock;
                if (A.has32)
                    k_fold_post0<kCgBlock, 2><<<g, kCgBlock, 0, s>>>(A.n, A.ftrow.p, A.ftcol.p, A.f32v.p, xfull,
                                                                     A.dinv.p, rh, A.r.p, b, o, done, pg,
                                                                     A.has16 ? A.f16.p : nullptr,
                                                                     A.has16 ? A.f16b.p : nullptr);
                else
                    k_fold_post0<kCgBlock, 2><<<g, kCgBlock, 0, s>>>(A.n, A.ftrow.p, A.ftcol.p, A.ftval.p, xfull,
                                                                     A.dinv.p, rh, A.r.p, b, o, done, pg,
                                                                     A.has16 ? A.f16.p : nullptr,
                                                                     A.has16 ? A.f16b.p : nullptr);
            } else {
                const int g = (A.n + 255) / 256;
                const unsigned short *no16 = nullptr;
                const int *nob = nullptr;
                if ((double)A.fnnz <= 8.0 * A.n)
                    k_fold_post0<256, 2><<<g, 256, 0, s>>>(A.n, A.ftrow.p, A.ftcol.p, A.ftval.p, xfull, A.dinv.p, rh,
                                                           A.r.p, b, o, done, pg, no16, nob);
                else
                    k_fold_post0<256, 4><<<g, 256, 0, s>>>(A.n, A.ftrow.p, A.ftcol.p, A.ftval.p, xfull, A.dinv.p, rh,
                                                           A.r.p, b, o, done, pg, no16, nob);
            }
        }
        if (l == 0 && out && part_gam_) gamma_done = true;
        return o;
    }
    if (A.n > 0) {
        const int GP = lanes_for((double)A.pnnz / A.n);
        if (A.has32)
            launch_mv_tile(s, A.n, A.prow.p, A.pcol.p, A.p32.p, xc, cur, true, GP, done, A.p16.p, A.p16b.p);
        else
            launch_mv(s, A.n, A.prow.p, A.pcol.p, A.pval.p, xc, cur, true, GP, done);
    }
    for (int k = 0; k < sweeps; ++k) {
        const bool last0 = k == sweeps - 1 && out && l == 0;
        double *nx = (k == sweeps - 1 && out) ? out : oth;
        if ((rc = smooth_after_exchange(kSweep, cur, nx, nullptr, last0 ? part_gam_ : nullptr)) != XFK_OK)
            return nullptr;
        if (last0 && part_gam_) gamma_done = true;
        oth = cur;
        cur = nx;
    }
    return cur;
}

int Amg::tail_begin(hipStream_t s, int kind)
{
    if (!time_tail) return -1;
    const int at = tail_used;
    while ((int)tail_ev.size() < at + 2) {
        hipEvent_t e = nullptr;
        if (hipEventCreate(&e) != hipSuccess) return -1;
        tail_ev.push_back(e);
    }
    if (hipEventRecord(tail_ev[at], s) != hipSuccess) return -1;
    tail_kind.resize(at / 2 + 1);
    tail_kind[at / 2] = (char)kind;
    tail_used = at + 2;
    return at;
}

void Amg::tail_end(hipStream_t s, int at)
{
    if (at >= 0) (void)hipEventRecord(tail_ev[at + 1], s);
}

int Amg::tail_read(double &ms_cycle, int &cycles, double &ms_setup)
{
    ms_cycle = ms_setup = 0;
    cycles = 0;
    for (int k = 0; k + 1 < tail_used; k += 2) {
        float m = 0;
        AMG_CHECK(hipEventElapsedTime(&m, tail_ev[k], tail_ev[k + 1]));
        if (tail_kind[k / 2] == 0) {
            ms_cycle += m;
            ++cycles;
        } else {
            ms_setup += m;
        }
    }
    tail_used = 0;
    return XFK_OK;
}

int Amg::vcycle(hipStream_t s, const double *r, double *u, const int *done, double *part_gam)
{
    gamma_done = false;
    if (!dist) {
        vcycle_level(*this, s, 0, r, u, done, part_gam);
        return XFK_OK;
    }
    int rc = XFK_OK;
    part_gam_ = part_gam;
    vc_dist(s, 0, r, u, done, rc);
    part_gam_ = nullptr;
    if (rc != XFK_OK) return rc;
    AMG_CHECK(hipGetLastError());
    return XFK_OK;
}

}  // namespace xfk

// xfk_device_init: loads this translation unit's code object onto the device
hipError_t xfk::warm_module_amg_cycle()
{
    hipFuncAttributes a;
    return hipFuncGetAttributes(&a, reinterpret_cast<const void *>(&k_jacobi_first));
}
