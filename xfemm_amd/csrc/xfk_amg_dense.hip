// The AMG's dense coarsest inverse (xfk_amg.h): blocked Gauss-Jordan kernels,
// the nested-dissection order and the host chain that launches them.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>

#include "xfk_amg_impl.h"

namespace xfk {

namespace {

// --------------------------------------------------------------------------
// setup: coarsest level, dense inverse
// --------------------------------------------------------------------------

// The coarsest level (<= kAmgDenseMax rows) becomes a dense matrix padded to
// a multiple of kBj with an identity tail (ld = padded size), inverted in
// place by blocked Gauss-Jordan without pivoting (the level operators are
// symmetric positive semi-definite).  Step k of kBj-wide block columns
// (k_bgj_step, one launch):
//     D  = inv(M_kk)                      k_bgj_diag for k = 0, else workgroup 0
//                                         of step k-1 (once its tile is final)
//     M_kj = D M_kj          (j != k),    M_kk = D
//     M_ij -= M_ik (D M_kj)  (i, j != k)
//     M_ik = -M_ik D         (i != k)     (old values of row k / column k)
// The matrix is first scaled symmetrically to unit diagonal and the inverse
// unscaled at the end.  A pivot below 1e-11 of the (unit) scaled diagonal
// marks a null direction -- roundoff leaves the exact null pivot of a
// pure-Neumann operator near 1e-13 (tools/lab/gj_emul.py) -- and its row and
// column are zeroed (generalised inverse on the range).

// the matrix has been zeroed (hipMemsetAsync); entries of row i, identity tail
// symmetric diagonal scaling sc_q = 1 / sqrt(a_qq) (1 for a zero diagonal
// and the padding rows): the scaled matrix has unit diagonal, so every
// Gauss-Jordan pivot (a Schur-complement diagonal) lies in (0, 1].
// perm / iperm (nested-dissection order, nullptr: identity): dense index of
// coarse row r is perm[r]; iperm[q] the coarse row of dense index q (-1: padding)
// kDsG lanes per dense row (consecutive entries on consecutive lanes): the
// row's column, permutation and scale loads of 16 entries in flight at once
// instead of one dependent chain per row (one thread per row took 11 + 26 us
// for the 1.6k-row coarsest level of configs[2]).  The coarse operator's rows
// hold distinct columns (SpGEMM output), so every entry is written once:
// 0 + v, the value the former accumulation into the zeroed matrix produced.
constexpr int kDsG = 16;
__global__ void k_dense_dscale(int n, int ld, const int *__restrict__ rowptr, const int *__restrict__ col,
                               const double *__restrict__ val, const int *__restrict__ iperm, double *__restrict__ sc)
{
    const int q = (blockIdx.x * blockDim.x + threadIdx.x) / kDsG, l = threadIdx.x % kDsG;
    if (q >= ld) return;   // (whole groups: ld * kDsG threads exactly cover the rows)
    const int i = iperm ? iperm[q] : (q < n ? q : -1);
    int kd = -1;
    if (i >= 0)
        for (int k = rowptr[i] + l; k < rowptr[i + 1]; k += kDsG)
            if (col[k] == i) kd = k;
#pragma unroll
    for (int off = 1; off < kDsG; off <<= 1) kd = max(kd, __shfl_xor(kd, off, kDsG));
    if (l != 0) return;
    const double d = kd >= 0 ? 0.0 + val[kd] : 0.0;
    sc[q] = d > 0.0 ? 1.0 / sqrt(d) : 1.0;
}
__global__ void k_dense_scatter(int n, int ld, const int *__restrict__ rowptr, const int *__restrict__ col,
                                const double *__restrict__ val, const int *__restrict__ perm,
                                const int *__restrict__ iperm, const double *__restrict__ sc, double *__restrict__ M)
{
    const int q = (blockIdx.x * blockDim.x + threadIdx.x) / kDsG, l = threadIdx.x % kDsG;
    if (q >= ld) return;
    const int i = iperm ? iperm[q] : (q < n ? q : -1);
    if (i < 0) {
        if (l == 0) M[(size_t)q * ld + q] = 1.0;
        return;
    }
    const double sq = sc[q];
    for (int k = rowptr[i] + l; k < rowptr[i + 1]; k += kDsG) {
        const int cj = col[k];
        if (cj >= n) continue;
        const int c = perm ? perm[cj] : cj;
        M[(size_t)q * ld + c] = 0.0 + val[k] * sq * sc[c];
    }
}

// The coarsest inverse the V-cycle applies, unpermuted: M is the inverse of
// the unit-diagonal scaled level (S A_c S)^-1, so A_c^-1 = S M S; the apply
// keeps S in f64 (osc, original order) and stores M symmetrised -- entries
// (i, j) and (j, i) both from the one value (M_qr + M_rq) / 2, rounded once --
// in f32 (V = float, the default: half the bytes of the per-iteration coarse
// solve) or f64.  Rounding the scaled, symmetrised inverse keeps the coarse
// correction exactly symmetric; the f32 perturbation is relative to the entries
// of a unit-diagonal matrix's inverse (not of A_c^-1 itself, whose entries span
// the coefficient contrast).  One 64 x 64 output tile per block, its mirror
// tile read through LDS.
template <class V>
__global__ void __launch_bounds__(256) k_dense_unperm(int n, int ld, int ldo, const double *__restrict__ M,
                                                      const double *__restrict__ sc, const int *__restrict__ iperm,
                                                      V *__restrict__ out, double *__restrict__ osc)
{
    __shared__ double t[64][65];
    const int bq = blockIdx.y * 64, br = blockIdx.x * 64;
    for (int k = threadIdx.x; k < 64 * 64; k += 256) {   // t[a][b] = M[br + b][bq + a]
        const int a = k & 63, b = k >> 6;
        t[a][b] = M[(size_t)(br + b) * ld + bq + a];
    }
    __syncthreads();
    for (int k = threadIdx.x; k < 64 * 64; k += 256) {
        const int a = k >> 6, b = k & 63, q = bq + a, r = br + b;
        const int i = iperm ? iperm[q] : (q < n ? q : -1), j = iperm ? iperm[r] : (r < n ? r : -1);
        if (i >= 0 && j >= 0) out[(size_t)i * ldo + j] = (V)(0.5 * (M[(size_t)q * ld + r] + t[a][b]));
    }
    if (blockIdx.x == 0)
        for (int a = threadIdx.x; a < 64; a += 256) {
            const int q = bq + a, i = iperm ? iperm[q] : (q < n ? q : -1);
            if (i >= 0) osc[i] = sc[q];
        }
}

__global__ void __launch_bounds__(1024) k_dense_maxdiag(int n, int ld, const double *__restrict__ M,
                                                        double *__restrict__ maxd)
{
    __shared__ double red[16];
    double m = 0.0;
    for (int i = threadIdx.x; i < n; i += blockDim.x) m = fmax(m, fabs(M[(size_t)i * ld + i]));
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) m = fmax(m, __shfl_xor(m, off, 64));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < (int)(blockDim.x >> 6); ++w) m = fmax(m, red[w]);
        *maxd = m;
    }
}

// D = inv(M_kk) by in-place Gauss-Jordan: 256 threads, thread t keeps the 16
// entries (rows 16 (t >> 6) + m, column t & 63) in registers for the whole
// inversion.  Pivots are taken four at a time: with P = {p0 .. p0+3},
// Dinv = inv(A_PP) (every thread inverts the 4 x 4 block in registers) and
//     c_i = A_iP,  r_j = Dinv A_Pj (j not in P),  r_j = e_t + Dinv[:, t] (j = p0 + t),
// one uniform rank-4 update a_ij -= c_i . r_j followed by a_sj += r_j[s] on
// the rows of P leaves Dinv A_Pj in rows P, -A_iP Dinv in columns P and Dinv
// in the pivot block; the scaled pivots lie in (0, 1], so no step cancels
// more than a few bits.  A pivot block with a vanishing pivot is eliminated
// by four scalar steps instead, which zero the row and column of a null
// direction.  Rows P and columns P go through LDS, double-buffered: one
// barrier per step.
__device__ __forceinline__ void gj_scalar_step(int p, double (&a)[16], double thr, double *slab, double *colk)
{
    const int j = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (w == (p >> 4))   // the wave holding row p publishes its slab
#pragma unroll
        for (int m = 0; m < 16; ++m) slab[m * kBj + j] = a[m];
    if (j == p)
#pragma unroll
        for (int m = 0; m < 16; ++m) colk[16 * w + m] = a[m];
    __syncthreads();
    const double *rowp = slab + (p & 15) * kBj;
    const double piv = rowp[p];
    if (!(fabs(piv) > thr)) {   // null direction: zero row p and column p
#pragma unroll
        for (int m = 0; m < 16; ++m)
            if (16 * w + m == p || j == p) a[m] = 0.0;
        return;
    }
    const double ip = 1.0 / piv;
    const double r = j == p ? 1.0 + ip : rowp[j] * ip;
#pragma unroll
    for (int m = 0; m < 16; ++m) a[m] -= (colk[16 * w + m] - (16 * w + m == p ? 1.0 : 0.0)) * r;
}

// lds: 2 * 16 * kBj + 2 * 4 * kBj doubles (16-byte aligned): the double-
// buffered 16-row slab holding P ([m][j]) and columns P ([i][t])
constexpr int kBjDiagLds = 2 * 16 * kBj + 2 * 4 * kBj;
__device__ __forceinline__ void bgj_diag_inv(double (&a)[16], double thr, double *lds)
{
    const int tid = threadIdx.x;
    const int j = tid & 63, w = tid >> 6;
    // (buffer pointers by arithmetic on lds: a runtime-indexed pointer array
    // would hide the LDS address space and turn every access into a flat op)
    int phase = 0;
    for (int p0 = 0; p0 < kBj; p0 += 4) {
        const int buf = phase & 1;
        const int mb = p0 & 15, wp = p0 >> 4;
        double *R4 = lds + buf * 16 * kBj, *C4 = lds + 32 * kBj + buf * 4 * kBj;
        if (w == wp)   // this wave holds rows P: publish its whole slab (no dynamic register index)
#pragma unroll
            for (int m = 0; m < 16; ++m) R4[m * kBj + j] = a[m];
        R4 += mb * kBj;   // rows P = slab rows mb .. mb+3
        if (j >= p0 && j < p0 + 4)   // these lanes hold columns P
#pragma unroll
            for (int m = 0; m < 16; ++m) C4[(16 * w + m) * 4 + (j - p0)] = a[m];
        __syncthreads();
        ++phase;
        // Dinv = inv(A_PP), in-place Gauss-Jordan in registers
        double Dv[4][4];
#pragma unroll
        for (int s2 = 0; s2 < 4; ++s2)
#pragma unroll
            for (int t = 0; t < 4; ++t) Dv[s2][t] = R4[s2 * kBj + p0 + t];
        bool ok = true;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const double piv = Dv[q][q];
            ok = ok && (fabs(piv) > thr);
            const double ip = 1.0 / piv;
            Dv[q][q] = 1.0;
#pragma unroll
            for (int t = 0; t < 4; ++t) Dv[q][t] *= ip;
#pragma unroll
            for (int s2 = 0; s2 < 4; ++s2) {
                if (s2 == q) continue;
                const double f = Dv[s2][q];
                Dv[s2][q] = 0.0;
#pragma unroll
                for (int t = 0; t < 4; ++t) Dv[s2][t] -= f * Dv[q][t];
            }
        }
        if (!ok) {   // a (near) null direction inside the block: scalar steps
            for (int p = p0; p < p0 + 4; ++p) {
                const int b2 = phase & 1;
                gj_scalar_step(p, a, thr, lds + b2 * 16 * kBj, lds + 32 * kBj + b2 * 4 * kBj);
                ++phase;
            }
            continue;
        }
        double r[4];
        if (j >= p0 && j < p0 + 4) {
            const int t = j - p0;
#pragma unroll
            for (int s2 = 0; s2 < 4; ++s2) {
                double d = Dv[s2][0];
#pragma unroll
                for (int tt = 1; tt < 4; ++tt)
                    if (tt == t) d = Dv[s2][tt];
                r[s2] = (s2 == t ? 1.0 : 0.0) + d;
            }
        } else {
            const double x0 = R4[j], x1 = R4[kBj + j], x2 = R4[2 * kBj + j], x3 = R4[3 * kBj + j];
#pragma unroll
            for (int s2 = 0; s2 < 4; ++s2) r[s2] = Dv[s2][0] * x0 + Dv[s2][1] * x1 + Dv[s2][2] * x2 + Dv[s2][3] * x3;
        }
        const double4 *cr = reinterpret_cast<const double4 *>(&C4[16 * w * 4]);
#pragma unroll
        for (int m = 0; m < 16; ++m) {
            const double4 c = cr[m];
            a[m] -= c.x * r[0] + c.y * r[1] + c.z * r[2] + c.w * r[3];
        }
        if (w == wp)
#pragma unroll
            for (int m = 0; m < 16; ++m) {
                const int s2 = m - mb;
                a[m] += (s2 == 0 ? r[0] : 0.0) + (s2 == 1 ? r[1] : 0.0) + (s2 == 2 ? r[2] : 0.0) +
                        (s2 == 3 ? r[3] : 0.0);
            }
    }
}

__global__ void __launch_bounds__(256) k_bgj_diag(int k, int ld, const double *__restrict__ M,
                                                  const double *__restrict__ maxd, double *__restrict__ D)
{
    __shared__ __attribute__((aligned(16))) double lds[kBjDiagLds];
    const int j = threadIdx.x & 63, w = threadIdx.x >> 6;
    const size_t base = (size_t)k * kBj * ld + (size_t)k * kBj;
    double a[16];
#pragma unroll
    for (int m = 0; m < 16; ++m) a[m] = M[base + (size_t)(16 * w + m) * ld + j];
    bgj_diag_inv(a, 1e-11 * (*maxd), lds);
#pragma unroll
    for (int m = 0; m < 16; ++m) D[(16 * w + m) * kBj + j] = a[m];
}

// C = X Y for 64 x 64 blocks staged in LDS on the f64 matrix cores: 4 waves,
// wave w computes the 32 x 32 quadrant (w >> 1, w & 1) as 2 x 2 tiles of
// v_mfma_f64_16x16x4_f64 (A[l & 15][k = l >> 4], B[k = l >> 4][l & 15];
// C/D col = l & 15, row = (l >> 4) + 4 r).  c[ti][tj][r] is element
// (32 (w >> 1) + 16 ti + (l >> 4) + 4 r, 32 (w & 1) + 16 tj + (l & 15)).
// LDS row strides (doubles) that make the operand reads conflict-free: a
// 32-lane half reads 16 rows x 2 k of X (stride 66 -> banks 4 li + 2 lk) and
// 2 k-rows x 16 columns of Y (stride 80 -> the two rows 32 banks apart).
typedef double dbl4 __attribute__((ext_vector_type(4)));
constexpr int kXs = 66, kYs = 80;

template <bool ZERO = true>
__device__ __forceinline__ void bgj_mm(const double *__restrict__ Xs, const double *__restrict__ Ys, dbl4 (&c)[2][2])
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int r0 = 32 * (w >> 1), c0 = 32 * (w & 1);
    const int li = lane & 15, lk = lane >> 4;
    if (ZERO)
#pragma unroll
        for (int ti = 0; ti < 2; ++ti)
#pragma unroll
            for (int tj = 0; tj < 2; ++tj) c[ti][tj] = dbl4{0.0, 0.0, 0.0, 0.0};
#pragma unroll 4
    for (int s = 0; s < kBj / 4; ++s) {
        double a[2], b[2];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            a[t] = Xs[(r0 + 16 * t + li) * kXs + 4 * s + lk];
            b[t] = Ys[(4 * s + lk) * kYs + c0 + 16 * t + li];
        }
#pragma unroll
        for (int ti = 0; ti < 2; ++ti)
#pragma unroll
            for (int tj = 0; tj < 2; ++tj)
                c[ti][tj] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[ti], b[tj], c[ti][tj], 0, 0, 0);
    }
}

// (row, col) of element r of tile (ti, tj) of this thread
__device__ __forceinline__ int bgj_row(int ti, int r) { return 32 * ((threadIdx.x >> 6) >> 1) + 16 * ti + ((threadIdx.x & 63) >> 4) + 4 * r; }
__device__ __forceinline__ int bgj_col(int tj) { return 32 * ((threadIdx.x >> 6) & 1) + 16 * tj + (threadIdx.x & 15); }

// inv(A) of a 64 x 64 block held in bgj_mm's accumulator layout
// (c[ti][tj][r] = element (bgj_row(ti, r), bgj_col(tj))), in place: 16
// rank-4 Gauss-Jordan steps whose updates run on the f64 matrix cores.  Step
// s publishes rows and columns P = 4s .. 4s+3 to LDS; every lane forms
// D = inv(A_PP) in registers and its B operand r = D A_Pj (r = I + D on the
// pivot columns); then c -= A_iP r on the MFMA, and rows P += r -- the update
// of bgj_diag_inv without its 64 FMAs and 32 LDS reads per lane and step.
// A (near) null pivot (|piv| <= thr) zeroes its row and column, as there.
// lds: kBjInvLds doubles (two buffers of a 4 x 64 row slab and a 64 x 4 column slab).
constexpr int kBjInvLds = 2 * 8 * kBj;
static_assert(kBjInvLds <= kBjDiagLds && kBjInvLds <= kBj * kYs, "bgj_inv_mfma's LDS exceeds its callers' buffers");
__device__ __forceinline__ void bgj_inv_mfma(dbl4 (&c)[2][2], double thr, double *lds)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int li = lane & 15, lk = lane >> 4;
    const int R0 = 32 * (w >> 1), C0 = 32 * (w & 1);
#pragma unroll
    for (int s = 0; s < 16; ++s) {
        const int p0 = 4 * s;
        const int tp = (p0 >> 4) & 1, rp = (p0 & 15) >> 2;   // tile / element index of rows (columns) P
        double *RS = lds + (s & 1) * 8 * kBj;   // RS[t][j] = A(p0 + t, j)
        double *CS = RS + 4 * kBj;              // CS[i][t] = A(i, p0 + t)
        const bool rowhold = (w >> 1) == (p0 >> 5);
        if (rowhold)   // this lane holds row p0 + lk
#pragma unroll
            for (int tj = 0; tj < 2; ++tj) RS[lk * kBj + C0 + 16 * tj + li] = c[tp][tj][rp];
        if ((w & 1) == (p0 >> 5) && li >= (p0 & 15) && li < (p0 & 15) + 4)   // ... column p0 + li - (p0 & 15)
#pragma unroll
            for (int ti = 0; ti < 2; ++ti)
#pragma unroll
                for (int r = 0; r < 4; ++r) CS[(R0 + 16 * ti + lk + 4 * r) * 4 + li - (p0 & 15)] = c[ti][tp][r];
        __syncthreads();
        double W[4][4];
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int t = 0; t < 4; ++t) W[q][t] = RS[q * kBj + p0 + t];
        // a null pivot takes ip = 0: its row of D becomes 0 and the
        // elimination leaves the other rows alone, i.e. D is the inverse on
        // the other directions; the update then zeroes column p0 + q of the
        // block by itself (r = e_q there), and row p0 + q is zeroed below
        unsigned nul = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const double piv = W[q][q];
            const bool ok = fabs(piv) > thr;
            nul |= ok ? 0u : 1u << q;
            double ip = __builtin_amdgcn_rcp(piv);   // 1 / piv: v_rcp_f64 + two Newton steps
            ip = fma(fma(-piv, ip, 1.0), ip, ip);
            ip = fma(fma(-piv, ip, 1.0), ip, ip);
            ip = ok ? ip : 0.0;
            W[q][q] = 1.0;
#pragma unroll
            for (int t = 0; t < 4; ++t) W[q][t] *= ip;
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                if (t == q) continue;
                const double f = W[t][q];
                W[t][q] = 0.0;
#pragma unroll
                for (int u = 0; u < 4; ++u) W[t][u] -= f * W[q][u];
            }
        }
        // row lk of D: this lane's B operand row
        double Dk[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) Dk[t] = lk == 0 ? W[0][t] : lk == 1 ? W[1][t] : lk == 2 ? W[2][t] : W[3][t];
        double bop[2], aop[2];
#pragma unroll
        for (int tj = 0; tj < 2; ++tj) {
            const int jj = C0 + 16 * tj + li, tc = jj - p0;
            if (tc >= 0 && tc < 4) {
                const double d = tc == 0 ? Dk[0] : tc == 1 ? Dk[1] : tc == 2 ? Dk[2] : Dk[3];
                bop[tj] = (lk == tc ? 1.0 : 0.0) + d;
            } else {
                bop[tj] = Dk[0] * RS[jj] + Dk[1] * RS[kBj + jj] + Dk[2] * RS[2 * kBj + jj] + Dk[3] * RS[3 * kBj + jj];
            }
        }
#pragma unroll
        for (int ti = 0; ti < 2; ++ti) aop[ti] = -CS[(R0 + 16 * ti + li) * 4 + lk];
#pragma unroll
        for (int ti = 0; ti < 2; ++ti)
#pragma unroll
            for (int tj = 0; tj < 2; ++tj) c[ti][tj] = __builtin_amdgcn_mfma_f64_16x16x4f64(aop[ti], bop[tj], c[ti][tj], 0, 0, 0);
        if (rowhold) {
            const bool zr = (nul >> lk) & 1u;   // row p0 + lk of a null pivot
#pragma unroll
            for (int tj = 0; tj < 2; ++tj) c[tp][tj][rp] = zr ? 0.0 : c[tp][tj][rp] + bop[tj];
        }
    }
}

template <int S>
__device__ __forceinline__ void bgj_load(double *__restrict__ dst, const double *__restrict__ src, size_t ld)
{
    // 2048 double2 per tile, 8 per thread, all issued before the first use
    double2 v[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const int e = threadIdx.x + 256 * q, r = e >> 5, c = 2 * (e & 31);
        v[q] = *reinterpret_cast<const double2 *>(src + (size_t)r * ld + c);
    }
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const int e = threadIdx.x + 256 * q, r = e >> 5, c = 2 * (e & 31);
        dst[r * S + c] = v[q].x;
        dst[r * S + c + 1] = v[q].y;
    }
}

// One launch per block step k.
// Step k reads only snapshots written by step k-1 (or the prologue), so every
// tile is finalised in the same launch with no ordering between workgroups:
//     D    = inv(M_kk)                               Dk
//     R[j] = M_kj after step k-1 (row k, unscaled)    Rk + j T2
//     C[i] = M_ik after step k-1 (column k)           Ck + i T2
// tile (i, j):  i == k:  M_kj = D R[j]          (j == k: M_kk = D)
//               j == k:  M_ik = -C[i] D
//               else:    M_ij -= C[i] (D R[j])  (T_kj = D R[j] recomputed per
//                                                tile: no row launch, no wait)
// Row k+1 of the result goes to Rn, column k+1 to Cn; workgroup 0 takes tile
// (k+1, k+1) -- the next pivot block -- and inverts it into Dn once written.
// The chain per step is one launch: the pivot workgroup's two tile GEMMs and
// the 64 x 64 inversion.
// snapshots of row k (R[j] = M_kj) and column k (C[i] = M_ik) before step k
__global__ void __launch_bounds__(256) k_bgj_snap(int k, int nbk, int ld, const double *__restrict__ M,
                                                  double *__restrict__ R, double *__restrict__ C)
{
    const int t = blockIdx.x % nbk;
    const bool row = blockIdx.x < nbk;
    const double *src = row ? M + (size_t)k * kBj * ld + (size_t)t * kBj : M + (size_t)t * kBj * ld + (size_t)k * kBj;
    double *dst = (row ? R : C) + (size_t)t * kBj * kBj;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const int e = threadIdx.x + 256 * q, r = e >> 5, c = 2 * (e & 31);
        *reinterpret_cast<double2 *>(dst + r * kBj + c) = *reinterpret_cast<const double2 *>(src + (size_t)r * ld + c);
    }
}

__global__ void __launch_bounds__(256) k_bgj_step(int k, int nbk, int ld, double *__restrict__ M,
                                                  const double *__restrict__ Dk, const double *__restrict__ Rk,
                                                  const double *__restrict__ Ck, double *__restrict__ Dn,
                                                  double *__restrict__ Rn, double *__restrict__ Cn,
                                                  const double *__restrict__ maxd)
{
    const int nt = nbk * nbk, kn = k + 1 < nbk ? k + 1 : 0;
    const int b = (int)((blockIdx.x + (unsigned)(kn * nbk + kn)) % (unsigned)nt);
    const int i = b / nbk, j = b % nbk;
    const bool piv = k + 1 < nbk && blockIdx.x == 0;
    const size_t T2 = (size_t)kBj * kBj;
    __shared__ __attribute__((aligned(16))) double Xs[kBj * kXs];
    __shared__ __attribute__((aligned(16))) double Ys[kBj * kYs];
    double *Mij = M + (size_t)i * kBj * ld + (size_t)j * kBj;
    if (i == k && j == k) {
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int e = threadIdx.x + 256 * q, r = e >> 5, c = 2 * (e & 31);
            *reinterpret_cast<double2 *>(Mij + (size_t)r * ld + c) = *reinterpret_cast<const double2 *>(Dk + r * kBj + c);
        }
        return;
    }
    dbl4 c[2][2];
    double sgn = 1.0;
    bool rmw = false;
    if (i == k) {   // T = D R[j]
        bgj_load<kXs>(Xs, Dk, kBj);
        bgj_load<kYs>(Ys, Rk + j * T2, kBj);
        __syncthreads();
        bgj_mm(Xs, Ys, c);
    } else if (j == k) {   // -C[i] D
        bgj_load<kXs>(Xs, Ck + i * T2, kBj);
        bgj_load<kYs>(Ys, Dk, kBj);
        __syncthreads();
        bgj_mm(Xs, Ys, c);
        sgn = -1.0;
    } else {   // M_ij - C[i] (D R[j])
        double2 pre[8];   // C[i], in flight during the first product
        const double *Ci = Ck + i * T2;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int e = threadIdx.x + 256 * q, r = e >> 5, cc = 2 * (e & 31);
            pre[q] = *reinterpret_cast<const double2 *>(Ci + r * kBj + cc);
        }
        bgj_load<kXs>(Xs, Dk, kBj);
        bgj_load<kYs>(Ys, Rk + j * T2, kBj);
        __syncthreads();
        bgj_mm(Xs, Ys, c);
        __syncthreads();
#pragma unroll
        for (int ti = 0; ti < 2; ++ti)
#pragma unroll
            for (int tj = 0; tj < 2; ++tj)
#pragma unroll
                for (int r = 0; r < 4; ++r) Ys[bgj_row(ti, r) * kYs + bgj_col(tj)] = c[ti][tj][r];
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int e = threadIdx.x + 256 * q, r = e >> 5, cc = 2 * (e & 31);
            Xs[r * kXs + cc] = pre[q].x;
            Xs[r * kXs + cc + 1] = pre[q].y;
        }
        __syncthreads();
        bgj_mm(Xs, Ys, c);
        sgn = -1.0;
        rmw = true;
    }
    double *rn = (i == k + 1) ? Rn + j * T2 : nullptr;
    double *cn = (j == k + 1) ? Cn + i * T2 : nullptr;
    if (piv) __syncthreads();   // Ys is reused below
#pragma unroll
    for (int ti = 0; ti < 2; ++ti)
#pragma unroll
        for (int tj = 0; tj < 2; ++tj)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = bgj_row(ti, r), col = bgj_col(tj);
                double *e = &Mij[(size_t)row * ld + col];
                const double v = rmw ? *e - c[ti][tj][r] : sgn * c[ti][tj][r];
                *e = v;
                if (rn) rn[row * kBj + col] = v;
                if (cn) cn[row * kBj + col] = v;
                if (piv) c[ti][tj][r] = v;
            }
    if (!piv) return;
    bgj_inv_mfma(c, 1e-11 * (*maxd), Ys);
#pragma unroll
    for (int ti = 0; ti < 2; ++ti)
#pragma unroll
        for (int tj = 0; tj < 2; ++tj)
#pragma unroll
            for (int r = 0; r < 4; ++r) Dn[bgj_row(ti, r) * kBj + bgj_col(tj)] = c[ti][tj][r];
}

// Nested-dissection steps.  The coarsest operator is reordered by a
// recursive bisection: leaves (parts that share no entry), then their
// separators, the top separator last.  Gauss-Jordan keeps distinct leaves
// decoupled: eliminating a block column of a leaf touches only the tiles of
// its region -- the leaf plus its ancestor separators -- and the updates of
// different leaves commute.  So the leaves' block columns are eliminated side
// by side, one pivot chain per leaf in each launch (up to four), then the
// separators of the next tree level the same way (region: their subtree plus
// ancestors), the top separator last.  Each tile applies the update of every
// chain whose region holds it (separator tiles: several, summed on the MFMA
// in chain order); per block, bit c of `mask` marks chain c's region.
constexpr int kNdChains = 8;
struct BgjStep {
    int n;                                             // chains of this step
    int k[kNdChains];                                  // their pivot blocks
    const double *D[kNdChains], *R[kNdChains], *C[kNdChains];   // inv(M_kk), row / column snapshots
    int nn;                                            // distinct next pivot blocks
    int nx[kNdChains];
    double *Dn[kNdChains], *Rn[kNdChains], *Cn[kNdChains];
};

// (chain fields are selected by unrolled comparisons: a dynamically indexed
// by-value kernel argument would be placed in scratch memory)
__global__ void __launch_bounds__(256, 2) k_bgj_multi(int nbk, int ld, double *__restrict__ M, BgjStep st,
                                                      const unsigned char *__restrict__ mask,
                                                      const int *__restrict__ tiles, const double *maxd)
{
    const size_t T2 = (size_t)kBj * kBj;
    int i, j;
    double *Dpiv = nullptr;
    if ((int)blockIdx.x < st.nn) {   // workgroups 0 .. nn-1 finalise and invert the next pivot blocks
#pragma unroll
        for (int t = 0; t < kNdChains; ++t)
            if (t == (int)blockIdx.x) {
                i = j = st.nx[t];
                Dpiv = st.Dn[t];
            }
    } else {
        const int t = tiles[blockIdx.x - st.nn];
        i = t / nbk;
        j = t % nbk;
        if (i == j)
#pragma unroll
            for (int u = 0; u < kNdChains; ++u)
                if (u < st.nn && st.nx[u] == i) return;   // taken by a pivot workgroup
    }
    const unsigned act = (unsigned)mask[i] & (unsigned)mask[j];
    int pc = -1;
    const double *pD = nullptr, *pR = nullptr, *pC = nullptr;
    int pk = -1;
#pragma unroll
    for (int c = 0; c < kNdChains; ++c)
        if (c < st.n && ((act >> c) & 1u) && (i == st.k[c] || j == st.k[c])) {
            pc = c;
            pk = st.k[c];
            pD = st.D[c];
            pR = st.R[c];
            pC = st.C[c];
        }
    __shared__ __attribute__((aligned(16))) double Xs[kBj * kXs];
    __shared__ __attribute__((aligned(16))) double Ys[kBj * kYs];
    double *Mij = M + (size_t)i * kBj * ld + (size_t)j * kBj;
    if (pc >= 0 && i == pk && j == pk) {
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int e = threadIdx.x + 256 * q, r = e >> 5, c = 2 * (e & 31);
            *reinterpret_cast<double2 *>(Mij + (size_t)r * ld + c) = *reinterpret_cast<const double2 *>(pD + r * kBj + c);
        }
        return;
    }
    dbl4 acc[2][2];
    double sgn = 1.0;
    bool rmw = false;
    if (pc >= 0 && i == pk) {   // row of a pivot: D R[j]
        bgj_load<kXs>(Xs, pD, kBj);
        bgj_load<kYs>(Ys, pR + j * T2, kBj);
        __syncthreads();
        bgj_mm(Xs, Ys, acc);
    } else if (pc >= 0) {       // column of a pivot: -C[i] D
        bgj_load<kXs>(Xs, pC + i * T2, kBj);
        bgj_load<kYs>(Ys, pD, kBj);
        __syncthreads();
        bgj_mm(Xs, Ys, acc);
        sgn = -1.0;
    } else {                    // M_ij - sum over the chains holding the tile of C[i] (D R[j])
#pragma unroll
        for (int ti = 0; ti < 2; ++ti)
#pragma unroll
            for (int tj = 0; tj < 2; ++tj) acc[ti][tj] = dbl4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int c = 0; c < kNdChains; ++c) {
            if (!(c < st.n && ((act >> c) & 1u))) continue;
            double2 pre[8];
            const double *Ci = st.C[c] + i * T2;
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int e = threadIdx.x + 256 * u, r = e >> 5, cc = 2 * (e & 31);
                pre[u] = *reinterpret_cast<const double2 *>(Ci + r * kBj + cc);
            }
            __syncthreads();   // the LDS of the previous chain's product is free
            bgj_load<kXs>(Xs, st.D[c], kBj);
            bgj_load<kYs>(Ys, st.R[c] + j * T2, kBj);
            __syncthreads();
            dbl4 t[2][2];
            bgj_mm(Xs, Ys, t);
            __syncthreads();
#pragma unroll
            for (int ti = 0; ti < 2; ++ti)
#pragma unroll
                for (int tj = 0; tj < 2; ++tj)
#pragma unroll
                    for (int r = 0; r < 4; ++r) Ys[bgj_row(ti, r) * kYs + bgj_col(tj)] = t[ti][tj][r];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int e = threadIdx.x + 256 * u, r = e >> 5, cc = 2 * (e & 31);
                Xs[r * kXs + cc] = pre[u].x;
                Xs[r * kXs + cc + 1] = pre[u].y;
            }
            __syncthreads();
            bgj_mm<false>(Xs, Ys, acc);
        }
        rmw = true;
    }
    // row / column snapshots of the next pivot blocks this tile belongs to
    double *rs[kNdChains], *cs[kNdChains];
#pragma unroll
    for (int t = 0; t < kNdChains; ++t) {
        rs[t] = (t < st.nn && i == st.nx[t]) ? st.Rn[t] + j * T2 : nullptr;
        cs[t] = (t < st.nn && j == st.nx[t]) ? st.Cn[t] + i * T2 : nullptr;
    }
    if (Dpiv) __syncthreads();   // Ys is reused below
#pragma unroll
    for (int ti = 0; ti < 2; ++ti)
#pragma unroll
        for (int tj = 0; tj < 2; ++tj)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = bgj_row(ti, r), col = bgj_col(tj);
                double *e = &Mij[(size_t)row * ld + col];
                const double v = rmw ? *e - acc[ti][tj][r] : sgn * acc[ti][tj][r];
                *e = v;
#pragma unroll
                for (int t = 0; t < kNdChains; ++t) {
                    if (rs[t]) rs[t][row * kBj + col] = v;
                    if (cs[t]) cs[t][row * kBj + col] = v;
                }
                if (Dpiv) acc[ti][tj][r] = v;
            }
    if (!Dpiv) return;
    bgj_inv_mfma(acc, 1e-11 * (*maxd), Ys);
#pragma unroll
    for (int ti = 0; ti < 2; ++ti)
#pragma unroll
        for (int tj = 0; tj < 2; ++tj)
#pragma unroll
            for (int r = 0; r < 4; ++r) Dpiv[bgj_row(ti, r) * kBj + bgj_col(tj)] = acc[ti][tj][r];
}

// first step of the first phase: pivot-block inverses (workgroups 0 .. n-1)
// and row / column snapshots of the chains' first pivot blocks
__global__ void __launch_bounds__(256) k_bgj_init(int nbk, int ld, const double *__restrict__ M, BgjStep st,
                                                  const double *__restrict__ maxd)
{
    const int b = blockIdx.x;
    if (b < st.nn) {
        __shared__ __attribute__((aligned(16))) double lds[kBjInvLds];
        int k = 0;
        double *D = nullptr;
#pragma unroll
        for (int t = 0; t < kNdChains; ++t)
            if (t == b) {
                k = st.nx[t];
                D = st.Dn[t];
            }
        const size_t base = (size_t)k * kBj * ld + (size_t)k * kBj;
        dbl4 c[2][2];
#pragma unroll
        for (int ti = 0; ti < 2; ++ti)
#pragma unroll
            for (int tj = 0; tj < 2; ++tj)
#pragma unroll
                for (int r = 0; r < 4; ++r) c[ti][tj][r] = M[base + (size_t)bgj_row(ti, r) * ld + bgj_col(tj)];
        bgj_inv_mfma(c, 1e-11 * (*maxd), lds);
#pragma unroll
        for (int ti = 0; ti < 2; ++ti)
#pragma unroll
            for (int tj = 0; tj < 2; ++tj)
#pragma unroll
                for (int r = 0; r < 4; ++r) D[bgj_row(ti, r) * kBj + bgj_col(tj)] = c[ti][tj][r];
        return;
    }
    const int e0 = b - st.nn, ch = e0 / (2 * nbk), rem = e0 % (2 * nbk);
    const int t = rem % nbk;
    const bool row = rem < nbk;
    int k = 0;
    double *dst = nullptr;
#pragma unroll
    for (int u = 0; u < kNdChains; ++u)
        if (u == ch) {
            k = st.nx[u];
            dst = (row ? st.Rn[u] : st.Cn[u]) + (size_t)t * kBj * kBj;
        }
    const double *src = row ? M + (size_t)k * kBj * ld + (size_t)t * kBj : M + (size_t)t * kBj * ld + (size_t)k * kBj;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const int e = threadIdx.x + 256 * q, r = e >> 5, c = 2 * (e & 31);
        *reinterpret_cast<double2 *>(dst + r * kBj + c) = *reinterpret_cast<const double2 *>(src + (size_t)r * ld + c);
    }
}

}  // namespace

// Nested-dissection order of the coarsest level for the dense inverse: a
// recursive bisection -- left = the first half of the rows (the levels are
// numbered along the fine level's Cuthill-McKee order, so the halves are
// banded slabs), right = the other rows without an entry in the left half,
// separator = those with one (about one grid line).  Two tree levels give
// four leaves (four pivot chains per launch), then their two separators,
// then the top separator; one level two leaves.  Groups are padded with
// identity rows to whole blocks, the groups of one phase to equal block
// counts.  Falls back to one level, then to the plain order, when a
// separator would be empty or hold more than a quarter of the rows.
// Host-synchronising (the coarsest level has <= dense_max rows).
namespace {
void nd_split_at(const std::vector<int> &rp, const std::vector<int> &cl, const std::vector<int> &rows, size_t h,
                 std::vector<char> &inl, std::vector<int> &L, std::vector<int> &R, std::vector<int> &S)
{
    L.assign(rows.begin(), rows.begin() + h);
    R.clear();
    S.clear();
    for (int r : L) inl[r] = 1;
    for (size_t t = h; t < rows.size(); ++t) {
        const int r = rows[t];
        bool cross = false;
        for (int k = rp[r]; k < rp[r + 1] && !cross; ++k) cross = inl[cl[k]] != 0;
        (cross ? S : R).push_back(r);
    }
    for (int r : L) inl[r] = 0;
}
// split position chosen so that the two parts (not counting the separator)
// come out about equal: the chain length of a phase is its largest part
void nd_bisect(const std::vector<int> &rp, const std::vector<int> &cl, const std::vector<int> &rows,
               std::vector<char> &inl, std::vector<int> &L, std::vector<int> &R, std::vector<int> &S)
{
    nd_split_at(rp, cl, rows, rows.size() / 2, inl, L, R, S);
    const size_t h = (rows.size() - S.size()) / 2;
    if (h > 0 && h != rows.size() / 2) nd_split_at(rp, cl, rows, h, inl, L, R, S);
}
}  // namespace

int Amg::nd_order(hipStream_t s, const AmgLevel &C, int &ld)
{
    const int n = C.n;
    nd_phases.clear();
    ld = ((n + kBj - 1) / kBj) * kBj;
    if (n < 8 * kBj || env_set("XFK_NO_ND")) {
        nd_key_n = -1;
        return XFK_OK;
    }
    // the pattern through pinned memory; an unchanged pattern (the next setup
    // of the same matrix family) keeps the plan and its device arrays
    const size_t npat = (size_t)n + 1 + (size_t)C.nnz;
    {
        int rc = host_ints((int)npat);
        if (rc != XFK_OK) return rc;
        AMG_CHECK(hipMemcpyAsync(host_big, C.rowptr, sizeof(int) * (n + 1), hipMemcpyDeviceToHost, s));
        AMG_CHECK(hipMemcpyAsync(host_big + n + 1, C.col, sizeof(int) * C.nnz, hipMemcpyDeviceToHost, s));
        AMG_CHECK(hipStreamSynchronize(s));
    }
    if (nd_key.size() == npat && std::equal(nd_key.begin(), nd_key.end(), host_big)) {
        nd_phases = nd_phases_key;
        ld = nd_ld;
        return XFK_OK;
    }
    nd_key.assign(host_big, host_big + npat);
    // the device copy of the key: the next setup compares its coarsest
    // pattern on the device and applies this plan without a host read
    AMG_CHECK(nd_key_dev.alloc(npat));
    AMG_CHECK(hipMemcpyAsync(nd_key_dev.p, C.rowptr, sizeof(int) * (n + 1), hipMemcpyDeviceToDevice, s));
    AMG_CHECK(hipMemcpyAsync(nd_key_dev.p + n + 1, C.col, sizeof(int) * C.nnz, hipMemcpyDeviceToDevice, s));
    nd_key_n = n;
    nd_key_nnz = C.nnz;
    nd_phases_key.clear();
    nd_ld = ld;
    std::vector<int> rp(host_big, host_big + n + 1), cl(host_big + n + 1, host_big + npat);
    for (int r = 0; r < n; ++r)   // columns >= n (none on a level built here) are dropped by the scatter
        for (int k = rp[r]; k < rp[r + 1]; ++k) cl[k] = std::min(cl[k], n);
    std::vector<char> inl(n + 1, 0);
    std::vector<int> all(n);
    for (int r = 0; r < n; ++r) all[r] = r;
    // groups: rows, phase, slot in the phase, parent separator group, subtree groups
    struct G {
        std::vector<int> rows;
        int phase, slot, parent;
        std::vector<int> sub;
    };
    std::vector<G> g;
    // the deepest bisection (3, 2, then 1 level) whose groups are all non-empty,
    // whose separators hold at most a quarter of the rows, and whose leaves
    // keep >= 1 block; leaves are phase 0 (slots = leaf index), the
    // separators of bisection level lev are phase D - lev
    // The bisection levels are computed once: nd_bisect is a function of its
    // set, so the first D levels of a deeper bisection are the D-level one and
    // every depth reads the same splits (no recomputation per depth tried)
    const int Dmax = n >= 24 * kBj ? 3 : (n >= 16 * kBj ? 2 : 1);
    std::vector<std::vector<std::vector<int>>> lev_sets(Dmax + 1), lev_seps(Dmax);
    std::vector<size_t> lev_nsep(Dmax, 0);
    int lev_done = 0;   // levels computed, each with all its groups non-empty
    lev_sets[0].push_back(all);
    for (int lev = 0; lev < Dmax; ++lev) {
        bool okl = true;
        for (const auto &x : lev_sets[lev]) {
            std::vector<int> L, R, S;
            nd_bisect(rp, cl, x, inl, L, R, S);
            okl = okl && !L.empty() && !R.empty() && !S.empty();
            lev_nsep[lev] += S.size();
            lev_sets[lev + 1].push_back(std::move(L));
            lev_sets[lev + 1].push_back(std::move(R));
            lev_seps[lev].push_back(std::move(S));
        }
        if (!okl) break;
        lev_done = lev + 1;
    }
    for (int D = Dmax; D >= 1 && g.empty(); --D) {
        bool ok = lev_done >= D;
        size_t nsep = 0;
        for (int lev = 0; lev < D && lev < Dmax; ++lev) nsep += lev_nsep[lev];
        const std::vector<std::vector<int>> &sets = lev_sets[std::min(D, lev_done + 1)];
        const std::vector<std::vector<std::vector<int>>> &seps = lev_seps;
        if (env_set("XFK_AMG_DEBUG")) {
            std::fprintf(stderr, "[amg] nested dissection depth %d: ok %d separators %zu, sets", D, (int)ok, nsep);
            for (const auto &x : sets) std::fprintf(stderr, " %zu", x.size());
            std::fprintf(stderr, "\n");
        }
        if (!ok || 3 * nsep > (size_t)n) continue;
        if (D > 1)
            for (const auto &x : sets) ok = ok && x.size() >= (size_t)kBj;
        if (!ok) continue;
        // group indices: leaves 0 .. 2^D - 1, then separators by level, deepest first
        const int nl = 1 << D;
        std::vector<int> sep_at(D);   // first group index of level lev's separators
        int q = nl;
        for (int lev = D - 1; lev >= 0; --lev) {
            sep_at[lev] = q;
            q += 1 << lev;
        }
        g.resize(q);
        for (int k = 0; k < nl; ++k)
            g[k] = {sets[k], 0, k, sep_at[D - 1] + (k >> 1), {k}};
        for (int lev = D - 1; lev >= 0; --lev)
            for (int m = 0; m < (1 << lev); ++m) {
                G &x = g[sep_at[lev] + m];
                x.rows = seps[lev][m];
                x.phase = D - lev;
                x.slot = m;
                x.parent = lev > 0 ? sep_at[lev - 1] + (m >> 1) : -1;
                // subtree: leaves and deeper separators under this one, and itself
                for (int k = 0; k < nl; ++k)
                    if ((k >> (D - lev)) == m) x.sub.push_back(k);
                for (int l2 = lev + 1; l2 < D; ++l2)
                    for (int m2 = 0; m2 < (1 << l2); ++m2)
                        if ((m2 >> (l2 - lev)) == m) x.sub.push_back(sep_at[l2] + m2);
                x.sub.push_back(sep_at[lev] + m);
            }
    }
    if (g.empty()) return XFK_OK;
    if (env_set("XFK_AMG_DEBUG")) {
        std::fprintf(stderr, "[amg] coarsest %d rows: nested dissection, %d groups:", n, (int)g.size());
        for (const G &x : g) std::fprintf(stderr, " %d/%d", (int)x.rows.size(), x.phase);
        std::fprintf(stderr, "\n");
    }
    const int nph = g.back().phase + 1;
    // blocks: each phase's groups padded to the phase's largest group
    std::vector<int> pblk(nph, 0), b0(g.size());
    for (const G &x : g) pblk[x.phase] = std::max(pblk[x.phase], (int)((x.rows.size() + kBj - 1) / kBj));
    int nbk = 0;
    for (size_t q = 0; q < g.size(); ++q) {
        b0[q] = nbk;
        nbk += pblk[g[q].phase];
    }
    ld = nbk * kBj;
    std::vector<int> perm(n), iperm(ld, -1);
    for (size_t q = 0; q < g.size(); ++q)
        for (size_t t = 0; t < g[q].rows.size(); ++t) {
            perm[g[q].rows[t]] = b0[q] * kBj + (int)t;
            iperm[b0[q] * kBj + (int)t] = g[q].rows[t];
        }
    // per phase: region masks (bit = slot) and the tiles some chain holds
    std::vector<unsigned char> mask((size_t)nph * nbk, 0);
    std::vector<int> tl;
    for (int ph = 0; ph < nph; ++ph) {
        unsigned char *m = mask.data() + (size_t)ph * nbk;
        NdPhase P{};
        P.steps = pblk[ph];
        for (size_t q = 0; q < g.size(); ++q) {
            if (g[q].phase != ph) continue;
            P.base[g[q].slot] = b0[q];
            P.nch = std::max(P.nch, g[q].slot + 1);
            P.next_slot[g[q].slot] = g[q].parent >= 0 ? g[g[q].parent].slot : -1;
            std::vector<int> reg = g[q].sub;
            for (int a = g[q].parent; a >= 0; a = g[a].parent) reg.push_back(a);
            for (int x : reg)
                for (int bb = 0; bb < pblk[g[x].phase]; ++bb) m[b0[x] + bb] |= (unsigned char)(1u << g[q].slot);
        }
        P.tiles_off = (int)tl.size();
        for (int i = 0; i < nbk; ++i)
            for (int j = 0; j < nbk; ++j)
                if (m[i] & m[j]) tl.push_back(i * nbk + j);
        P.ntiles = (int)tl.size() - P.tiles_off;
        nd_phases.push_back(P);
    }
    AMG_CHECK(cinv_perm.alloc(n));
    AMG_CHECK(cinv_iperm.alloc(ld));
    AMG_CHECK(nd_mask.alloc(mask.size()));
    AMG_CHECK(nd_tiles.alloc(tl.size()));
    // uploads from a pinned staging copy (no host check: the staging buffer
    // is rewritten only after the next setup's synchronising pattern read)
    const size_t bytes = sizeof(int) * ((size_t)n + ld + tl.size()) + mask.size();
    if (nd_stage_n < bytes) {
        pinned_free(nd_stage);   // (outside a destroy: hipHostFree)
        nd_stage = nullptr;
        nd_stage_n = 0;
        AMG_CHECK(pinned_malloc((void **)&nd_stage, bytes));
        nd_stage_n = bytes;
    }
    char *h = nd_stage;
    std::memcpy(h, perm.data(), sizeof(int) * n);
    std::memcpy(h + sizeof(int) * n, iperm.data(), sizeof(int) * ld);
    std::memcpy(h + sizeof(int) * ((size_t)n + ld), tl.data(), sizeof(int) * tl.size());
    std::memcpy(h + sizeof(int) * ((size_t)n + ld + tl.size()), mask.data(), mask.size());
    if (foreign_on()) {   // (the plan's device arrays for the next fresh problem of this size)
        nd_plan.assign(h, h + bytes);
        nd_tl_n = tl.size();
        nd_mask_n = mask.size();
    }
    AMG_CHECK(hipMemcpyAsync(cinv_perm.p, h, sizeof(int) * n, hipMemcpyHostToDevice, s));
    AMG_CHECK(hipMemcpyAsync(cinv_iperm.p, h + sizeof(int) * n, sizeof(int) * ld, hipMemcpyHostToDevice, s));
    AMG_CHECK(hipMemcpyAsync(nd_tiles.p, h + sizeof(int) * ((size_t)n + ld), sizeof(int) * tl.size(),
                             hipMemcpyHostToDevice, s));
    AMG_CHECK(hipMemcpyAsync(nd_mask.p, h + sizeof(int) * ((size_t)n + ld + tl.size()), mask.size(),
                             hipMemcpyHostToDevice, s));
    nd_phases_key = nd_phases;
    nd_ld = ld;
    return XFK_OK;
}

// the dense coarsest inverse of C in the order nd_phases / cinv_perm give
// (ld: the padded size of that order)
int Amg::dense_inverse(hipStream_t s, const AmgLevel &C, int ld)
{
    const bool nd = !nd_phases.empty();
    const int nbk = ld / kBj;
    cinv_ld = ld;
    AMG_CHECK(cinv.alloc((size_t)ld * ld));
    const size_t T2 = (size_t)kBj * kBj;
    // per chain slot and parity: row / column snapshots and the pivot inverse
    const size_t per = 2 * (size_t)nbk * T2 + T2;
    AMG_CHECK(bgj_tmp.alloc(2 * kNdChains * per + 1 + ld));
    auto Rb = [&](int c, int q) { return bgj_tmp.p + (size_t)(2 * c + q) * per; };
    auto Cb = [&](int c, int q) { return Rb(c, q) + (size_t)nbk * T2; };
    auto Db = [&](int c, int q) { return Rb(c, q) + 2 * (size_t)nbk * T2; };
    double *maxd = bgj_tmp.p + 2 * kNdChains * per, *sc = maxd + 1;
    const int *pm = nd ? cinv_perm.p : nullptr, *ipm = nd ? cinv_iperm.p : nullptr;
    AMG_CHECK(hipMemsetAsync(cinv.p, 0, sizeof(double) * (size_t)ld * ld, s));
    k_dense_dscale<<<nb((long long)ld * kDsG), kB, 0, s>>>(C.n, ld, C.rowptr, C.col, C.val, ipm, sc);
    k_dense_scatter<<<nb((long long)ld * kDsG), kB, 0, s>>>(C.n, ld, C.rowptr, C.col, C.val, pm, ipm, sc, cinv.p);
    k_dense_maxdiag<<<1, 1024, 0, s>>>(ld, ld, cinv.p, maxd);
    // (a lookahead variant -- block column k+1 first, its pivot block
    // inverted on a second stream during the rest of the update -- was
    // measured slower: the two cross-stream waits cost ~15 us per step,
    // more than the 25 us pivot-block inversion it hides)
    if (nd) {
        int par = 0;
        BgjStep st{};
        st.nn = nd_phases[0].nch;
        for (int c = 0; c < st.nn; ++c) {
            st.nx[c] = nd_phases[0].base[c];
            st.Dn[c] = Db(c, 0);
            st.Rn[c] = Rb(c, 0);
            st.Cn[c] = Cb(c, 0);
        }
        k_bgj_init<<<st.nn * (1 + 2 * nbk), 256, 0, s>>>(nbk, ld, cinv.p, st, maxd);
        for (size_t ph = 0; ph < nd_phases.size(); ++ph) {
            const NdPhase &P = nd_phases[ph];
            for (int t = 0; t < P.steps; ++t) {
                const int pp = par, qq = par ^ 1;
                BgjStep x{};
                x.n = P.nch;
                for (int c = 0; c < P.nch; ++c) {
                    x.k[c] = P.base[c] + t;
                    x.D[c] = Db(c, pp);
                    x.R[c] = Rb(c, pp);
                    x.C[c] = Cb(c, pp);
                }
                if (t + 1 < P.steps) {
                    x.nn = P.nch;
                    for (int c = 0; c < P.nch; ++c) x.nx[c] = P.base[c] + t + 1;
                } else if (ph + 1 < nd_phases.size()) {
                    const NdPhase &Q = nd_phases[ph + 1];
                    x.nn = Q.nch;
                    for (int c = 0; c < Q.nch; ++c) x.nx[c] = Q.base[c];
                }
                for (int c = 0; c < x.nn; ++c) {
                    x.Dn[c] = Db(c, qq);
                    x.Rn[c] = Rb(c, qq);
                    x.Cn[c] = Cb(c, qq);
                }
                k_bgj_multi<<<P.ntiles + x.nn, 256, 0, s>>>(nbk, ld, cinv.p, x, nd_mask.p + ph * (size_t)nbk,
                                                            nd_tiles.p + P.tiles_off, maxd);
                par = qq;
            }
        }
    } else {
        BgjStep st{};
        st.nn = 1;
        st.nx[0] = 0;
        st.Dn[0] = Db(0, 0);
        st.Rn[0] = Rb(0, 0);
        st.Cn[0] = Cb(0, 0);
        k_bgj_init<<<1 + 2 * nbk, 256, 0, s>>>(nbk, ld, cinv.p, st, maxd);
        for (int k = 0; k < nbk; ++k) {
            const int p = k & 1, q = (k + 1) & 1;
            k_bgj_step<<<nbk * nbk, 256, 0, s>>>(k, nbk, ld, cinv.p, Db(0, p), Rb(0, p), Cb(0, p), Db(0, q),
                                                 Rb(0, q), Cb(0, q), maxd);
        }
    }
    {
        const int ldo = ((C.n + kBj - 1) / kBj) * kBj;
        const dim3 g(ld / 64, ld / 64);
        AMG_CHECK(cinv_sc.alloc((size_t)ldo));
        cinv_f64 = prec32 == 0;   // (f64 transfers: the f64 inverse too)
        if (cinv_f64) {
            AMG_CHECK(cinv_o64.alloc((size_t)ldo * ldo));
            AMG_CHECK(hipMemsetAsync(cinv_o64.p, 0, sizeof(double) * (size_t)ldo * ldo, s));   // (padding columns)
            k_dense_unperm<double><<<g, 256, 0, s>>>(C.n, ld, ldo, cinv.p, sc, nd ? cinv_iperm.p : nullptr,
                                                     cinv_o64.p, cinv_sc.p);
        } else {
            AMG_CHECK(cinv_o.alloc((size_t)ldo * ldo));
            AMG_CHECK(hipMemsetAsync(cinv_o.p, 0, sizeof(float) * (size_t)ldo * ldo, s));
            k_dense_unperm<float><<<g, 256, 0, s>>>(C.n, ld, ldo, cinv.p, sc, nd ? cinv_iperm.p : nullptr, cinv_o.p,
                                                    cinv_sc.p);
        }
        cinv_apply = cinv_o.p;
        cinv_ld = ldo;
    }
    return XFK_OK;
}

}  // namespace xfk

// xfk_device_init: loads this translation unit's code object onto the device
hipError_t xfk::warm_module_amg_dense()
{
    hipFuncAttributes a;
    return hipFuncGetAttributes(&a, reinterpret_cast<const void *>(&k_dense_maxdiag));
}
