// Smoothed-aggregation AMG preconditioner for the fsolver PCG on MI355X
// (gfx950).  Design and parameters: xfk_amg.h.  Replaces the reference's SSOR
// preconditioner (cfemm/libfemm/spars.cpp:186-236, CBigLinProb::MultPC) on the
// device; the PCG itself (and its stopping test, spars.cpp:259/313) is
// unchanged.
//
// Every setup kernel is deterministic: decisions read only the previous
// launch's state, floating-point sums run in a fixed order (the SpGEMM
// accumulates each output entry in product-enumeration order), and atomics
// are used only where the result does not depend on their order (set
// membership, counts, max of non-negative values, positions that are sorted
// afterwards).
//
// This file: strength, MIS-2 aggregation and joins, R = P^T, the folded
// transfer's setup, the hierarchy's host side (scans, stream pool, hints,
// build, the sharded Galerkin path) and the probes.  The SpGEMM, the dense
// coarsest inverse and the cycle have files of their own (xfk_amg_impl.h).
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <vector>

#include "xfk_amg_impl.h"
#include "xfk_comm.h"

namespace xfk {

namespace {

// --------------------------------------------------------------------------
// small helpers
// --------------------------------------------------------------------------


// MIS key: (state:2 | perm(i):30), perm a bijection of [0, 2^30) (odd
// multipliers and xor-shifts): unique per node, so the max over a
// neighbourhood picks an IN node first, then the undecided node of the
// largest pseudo-random priority -- 4-byte keys halve the gathers of the two
// max sweeps of every round
using MisKey = unsigned;
constexpr MisKey kStIn = 2u, kStUnd = 1u;   // OUT = 0
constexpr MisKey kKeyMask = 0x3FFFFFFFu;

__device__ __forceinline__ MisKey perm30(unsigned x)
{
    x &= kKeyMask;
    x = (x * 0x2C1B3C6Du) & kKeyMask;
    x ^= x >> 15;
    x = (x * 0x297A2D39u) & kKeyMask;
    x ^= x >> 12;
    x = (x * 0x7FEB352Du) & kKeyMask;
    x ^= x >> 15;
    return x;
}
__device__ __forceinline__ MisKey mis_key(MisKey st, int i) { return (st << 30) | perm30((unsigned)i); }
__device__ __forceinline__ MisKey key_st(MisKey k) { return k >> 30; }
__device__ __forceinline__ MisKey key_low(MisKey k) { return k & kKeyMask; }

// entries of a row whose loads are issued together in the aggregation sweeps
// (per row; G lanes take kMisChunk / G each)
constexpr int kMisChunk = 8;

// max of two values over the workgroup (kB threads), result in thread 0
__device__ __forceinline__ void block_max2(double &a, double &b, double *red)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        a = fmax(a, __shfl_xor(a, off, 64));
        b = fmax(b, __shfl_xor(b, off, 64));
    }
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    if (lane == 0) {
        red[2 * wid] = a;
        red[2 * wid + 1] = b;
    }
    __syncthreads();
    if (threadIdx.x == 0)
        for (int w = 1; w < kB / 64; ++w) {
            a = fmax(a, red[2 * w]);
            b = fmax(b, red[2 * w + 1]);
        }
}

constexpr int kMaxReduceT = 256;

// per-block maxima (2 arrays of nblk) -> rho[0..1] as ordered bit patterns;
// rho[0] (read only by the smoothers, weight 1 / rho[0]) is divided by the
// Jacobi weight factor omega
__global__ void __launch_bounds__(kMaxReduceT) k_max_reduce(int nblk, const double *__restrict__ part, double omega,
                                                     unsigned long long *rho)
{
    __shared__ double red[2 * 16];
    double a = 0.0, b = 0.0;
    // kMaxU partials per array per thread loaded before the first fmax: one
    // load latency per kMaxU * blockDim partials (level 0 has ~2e4 blocks).
    // Launched with 256 threads (kMaxReduceT), not 1024: a 16-wave workgroup
    // waits for 16 free wave slots on one CU, which the side stream's
    // k_fold_p (31k 4-wave blocks) did not leave until it drained -- up to
    // 50 us of the setup's critical path at level 1
    constexpr int kMaxU = 16;
    for (int i0 = threadIdx.x; i0 < nblk; i0 += kMaxU * blockDim.x) {
        double pa[kMaxU], pb[kMaxU];
#pragma unroll
        for (int q = 0; q < kMaxU; ++q) {
            const int i = i0 + q * (int)blockDim.x;
            pa[q] = i < nblk ? part[i] : 0.0;
            pb[q] = i < nblk ? part[nblk + i] : 0.0;
        }
#pragma unroll
        for (int q = 0; q < kMaxU; ++q) {   // (fmax of non-negative bounds: any order, the same bits)
            a = fmax(a, pa[q]);
            b = fmax(b, pb[q]);
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        a = fmax(a, __shfl_xor(a, off, 64));
        b = fmax(b, __shfl_xor(b, off, 64));
    }
    if ((threadIdx.x & 63) == 0) {
        red[2 * (threadIdx.x >> 6)] = a;
        red[2 * (threadIdx.x >> 6) + 1] = b;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < (int)(blockDim.x >> 6); ++w) {
            a = fmax(a, red[2 * w]);
            b = fmax(b, red[2 * w + 1]);
        }
        rho[0] = (unsigned long long)__double_as_longlong(a / omega);
        rho[1] = (unsigned long long)__double_as_longlong(b);
    }
}

// --------------------------------------------------------------------------
// setup: diagonal, strength, Gershgorin bounds
// --------------------------------------------------------------------------

__global__ void k_amg_diag(int n, const int *__restrict__ rowptr, const int *__restrict__ col,
                           const double *__restrict__ val, double *__restrict__ absd, double *__restrict__ dinv)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    // the row's columns a chunk at a time, loads issued together; the first
    // match is the diagonal
    const int s = rowptr[i], e = rowptr[i + 1];
    int kd = -1;
    for (int k0 = s; k0 < e && kd < 0; k0 += kMisChunk) {
        int c[kMisChunk];
#pragma unroll
        for (int q = 0; q < kMisChunk; ++q) c[q] = k0 + q < e ? col[k0 + q] : -1;
#pragma unroll
        for (int q = kMisChunk - 1; q >= 0; --q)
            if (c[q] == i) kd = k0 + q;
    }
    const double d = kd >= 0 ? val[kd] : 0.0;
    absd[i] = fabs(d);
    dinv[i] = (d != 0.0) ? 1.0 / d : 0.0;
}

// strong flags per nonzero (1 strong off-diagonal, 2 diagonal, 0 weak or
// outside the block), strong degree per row, lumped filtered diagonal,
// Gershgorin bounds of D^-1 A (rho[0]) and D_F^-1 A_F (rho[1])
// kStrG lanes per row (consecutive entries of a row on consecutive lanes:
// coalesced col / val reads and flag writes, the row's sums by shuffles)
constexpr int kStrG = 4;
inline int nb_str(long long n) { return nb(n * kStrG); }

__global__ void __launch_bounds__(kB) k_amg_strength(int n, int ncl, double theta, const int *__restrict__ rowptr,
                                                     ColView cv, const double *__restrict__ val,
                                                     const double *__restrict__ absd,
                                                     const double *__restrict__ dinv,
                                                     unsigned char *__restrict__ sflag, int *__restrict__ sdeg,
                                                     double *__restrict__ dfinv, double *__restrict__ wF,
                                                     double *__restrict__ rho_part)
{
    __shared__ double red[2 * (kB / 64)];
    const int i = (blockIdx.x * blockDim.x + threadIdx.x) / kStrG;
    const int g = threadIdx.x % kStrG;
    double rA = 0.0, rF = 0.0;
    double aii = 0.0, lump = 0.0, sumS = 0.0, sumA = 0.0;
    int deg = 0, hdeg = 0;
    if (i < n) {
        const double ai = absd[i];
        const int cb = cv.base(i);
        // signed strength: only couplings of the sign opposite to the
        // diagonal's are strong (-a_ij for a positive diagonal).  Couplings of
        // the diagonal's own sign -- the reference's AntiPeriodicity averaging
        // gives each seam node such couplings to its partner's neighbours, an
        // air-gap element gives a few -- are weak and lumped, so no aggregate
        // spans an antiperiodic seam with a constant tentative value.
        // The test follows the diagonal's sign: the static operators are SPD,
        // the harmonic surrogate (Re A + s Im A of FEMM's sign convention) is
        // negative definite -- the diagonal negative, the couplings positive.
        const double sg = dinv[i] < 0.0 ? -1.0 : 1.0;
        const int s = rowptr[i] + g, e = rowptr[i + 1];
        // a chunk of this lane's entries at a time: columns and values, then
        // their diagonals, loaded before the first use; the entries are then
        // taken in the same order as one at a time (same sums, same bits)
        constexpr int C = kMisChunk / kStrG;
        for (int k0 = s; k0 < e; k0 += C * kStrG) {
        int jc[C];
        double ac[C], dj[C];
#pragma unroll
        for (int q = 0; q < C; ++q) {
            const int k = k0 + q * kStrG;
            const bool ok = k < e;
            jc[q] = ok ? cv.at(cb, k) : i;
            ac[q] = ok ? val[k] : 0.0;
        }
#pragma unroll
        for (int q = 0; q < C; ++q) dj[q] = absd[jc[q] < ncl ? jc[q] : i];
#pragma unroll
        for (int q = 0; q < C; ++q) {
            const int k = k0 + q * kStrG;
            if (k >= e) break;
            const int j = jc[q];
            const double a = ac[q];
            unsigned char f = 0;
            if (j == i) {
                aii = a;
                f = 2;   // the diagonal: not a neighbour, but kept by the prolongator smoothing
            } else if (j >= ncl) {
                // halo column: read by the smoother; for the rank-local P it is
                // lumped like a weak entry, so P keeps reproducing constants
                // (strong by the one-sided test -a_ij > theta |a_ii|: the
                // peer's diagonal is not known here)
                sumA += fabs(a);
                lump += a;
                hdeg += (-sg * a > theta * ai);
            } else {
                sumA += fabs(a);
                if (a != 0.0 && -sg * a > theta * sqrt(ai * dj[q])) {
                    f = 1;
                    ++deg;
                    sumS += fabs(a);
                } else {
                    lump += a;
                }
            }
            sflag[k] = f;
        }
        }
    }
#pragma unroll
    for (int off = 1; off < kStrG; off <<= 1) {   // fixed butterfly: the same bits on every run
        aii += __shfl_xor(aii, off, kStrG);
        lump += __shfl_xor(lump, off, kStrG);
        sumS += __shfl_xor(sumS, off, kStrG);
        sumA += __shfl_xor(sumA, off, kStrG);
        deg += __shfl_xor(deg, off, kStrG);
        hdeg += __shfl_xor(hdeg, off, kStrG);
    }
    if (i < n && g == 0) {
        const double dF = aii + lump;
        // -1: every strong coupling crosses to a peer -> a singleton aggregate
        sdeg[i] = (deg == 0 && hdeg > 0) ? -1 : deg;
        if (aii != 0.0) rA = (fabs(aii) + sumA) / fabs(aii);
        if (dF != 0.0) rF = (fabs(dF) + sumS) / fabs(dF);
        // prolongator smoothing weight per row, 4 / (3 max(rho_i, 2)) with
        // rho_i the row's Gershgorin bound of D_F^-1 A_F: one row whose
        // filtered diagonal nearly cancels no longer shrinks the weight of
        // every row of the level (a global Gershgorin maximum of 100-200 was
        // measured on coarse levels of the steel / air problem)
        // rows without strong couplings keep the tentative (injection) row
        dfinv[i] = (dF != 0.0) ? 1.0 / dF : 0.0;
        wF[i] = (dF != 0.0 && deg > 0) ? (4.0 / 3.0) / fmax(rF, 2.0) : 0.0;
    }
    block_max2(rA, rF, red);
    if (threadIdx.x == 0) {
        rho_part[blockIdx.x] = rA;
        rho_part[gridDim.x + blockIdx.x] = rF;
    }
}

// a Newton refresh (same aggregates, P and weights; new values): only the
// Gershgorin bound of D^-1 A, summed as k_amg_strength sums it (each lane's
// entries in order, the same butterfly: the same bits); rho[1] is not used
// after a setup and is left 0.  The row's diagonal found here also gives
// |a_ii| and D^-1 (k_amg_diag's values: the other lanes add 0.0 to it), so the
// refresh reads the matrix once
__global__ void __launch_bounds__(kB) k_amg_rho(int n, const int *__restrict__ rowptr, ColView cv,
                                                const double *__restrict__ val, double *__restrict__ rho_part,
                                                double *__restrict__ absd, double *__restrict__ dinv)
{
    __shared__ double red[2 * (kB / 64)];
    const int i = (blockIdx.x * blockDim.x + threadIdx.x) / kStrG;
    const int g = threadIdx.x % kStrG;
    double rA = 0.0, rF = 0.0, aii = 0.0, sumA = 0.0;
    if (i < n) {
        const int cb = cv.base(i);
        const int e = rowptr[i + 1];
        for (int k = rowptr[i] + g; k < e; k += kStrG) {
            const int j = cv.at(cb, k);
            const double a = val[k];
            if (j == i) aii = a;
            else sumA += fabs(a);
        }
    }
#pragma unroll
    for (int off = 1; off < kStrG; off <<= 1) {
        aii += __shfl_xor(aii, off, kStrG);
        sumA += __shfl_xor(sumA, off, kStrG);
    }
    if (i < n && g == 0) {
        if (aii != 0.0) rA = (fabs(aii) + sumA) / fabs(aii);
        absd[i] = fabs(aii);
        dinv[i] = (aii != 0.0) ? 1.0 / aii : 0.0;
    }
    block_max2(rA, rF, red);
    if (threadIdx.x == 0) {
        rho_part[blockIdx.x] = rA;
        rho_part[gridDim.x + blockIdx.x] = rF;
    }
}

// --------------------------------------------------------------------------
// setup: MIS-2 aggregation
// --------------------------------------------------------------------------

// also arms the round bookkeeping: "undecided" for the round before the
// first, no round run yet
__global__ void k_mis_init(int n, const int *__restrict__ sdeg, MisKey *__restrict__ key, int *und_prev,
                           int *run, unsigned char *__restrict__ act)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0) {
        *und_prev = 1;
        *run = 0;
    }
    if (i < n) {
        key[i] = mis_key(sdeg[i] > 0 ? kStUnd : (sdeg[i] < 0 ? kStIn : 0u), i);
        act[i] = 1;
    }
}

// Rounds are launched in batches without a host check in between: the
// undecided flag is double-buffered by round parity (prev = the last round's
// result, cur = this round's), and once a round leaves nothing undecided the
// later rounds of the batch exit at once (passing the 0 on).
// G lanes per row (coarse levels, 10-16 entries per row; 1 on the fine level):
// consecutive strong entries on consecutive lanes, the maximum by a butterfly.
// A row whose strong neighbourhood holds no undecided row any more keeps its
// maximum for good (decided rows never change): act[i] = 0 then, and later
// rounds skip the row -- after the first rounds most of the level.
template <int G>
__global__ void k_mis_max(int n, const int *__restrict__ rowptr, ColView cv,
                          const unsigned char *__restrict__ sflag, const MisKey *__restrict__ in,
                          MisKey *__restrict__ out, const int *prev, int *cur, int *run,
                          unsigned char *__restrict__ act)
{
    // consecutive blocks on one XCD (xcd_tile): a block's neighbour rows
    // a mesh row away stay in that XCD's L2
    const int bx = xcd_tile(blockIdx.x, gridDim.x);
    const int t = bx * blockDim.x + threadIdx.x;
    const int i = t / G, g = t % G;
    if (blockIdx.x == 0 && threadIdx.x == 0) {   // k_mis_update of this round runs after this launch
        if (*prev != 0) *run += 1;   // rounds that did work (the next setup's batch size)
        *cur = 0;
    }
    if (i >= n || *prev == 0 || act[i] == 0) return;
    MisKey m = in[i];
    int any = key_st(m) == kStUnd;
    const int cb = cv.base(i);
    for (int k = rowptr[i] + g; k < rowptr[i + 1]; k += G)
        if (sflag[k] == 1) {
            const MisKey v = in[cv.at(cb, k)];
            m = max(m, v);
            any |= key_st(v) == kStUnd;
        }
#pragma unroll
    for (int off = 1; off < G; off <<= 1) {
        m = max(m, (MisKey)__shfl_xor((int)m, off, G));
        any |= __shfl_xor(any, off, G);
    }
    if (g == 0) {
        out[i] = m;
        if (!any) act[i] = 0;
    }
}

// second max sweep fused with the state update: an undecided node whose
// distance-2 maximum is itself joins the set; one that sees a set member
// within distance 2 leaves
// ROOTS (the last round of a batch): every row also writes its root flag
// (k_agg_roots folded in: one launch less per level)
template <int G, bool ROOTS = false>
__global__ void k_mis_update(int n, const int *__restrict__ rowptr, ColView cv,
                             const unsigned char *__restrict__ sflag, const MisKey *__restrict__ t1,
                             MisKey *__restrict__ key, const int *prev, int *undecided, int *__restrict__ flag)
{
    const int bx = xcd_tile(blockIdx.x, gridDim.x);
    const int t = bx * blockDim.x + threadIdx.x;
    const int i = t / G, g = t % G;
    if (i >= n) return;
    const MisKey k = key[i];
    if (*prev == 0 || key_st(k) != kStUnd) {   // uniform over the row's lanes
        if (ROOTS && g == 0) flag[i] = key_st(k) == kStIn;
        return;
    }
    MisKey m = t1[i];
    const int cb = cv.base(i);
    for (int q = rowptr[i] + g; q < rowptr[i + 1]; q += G)
        if (sflag[q] == 1) m = max(m, t1[cv.at(cb, q)]);
#pragma unroll
    for (int off = 1; off < G; off <<= 1) m = max(m, (MisKey)__shfl_xor((int)m, off, G));
    if (g != 0) return;
    int root = 0;
    if (key_low(m) == perm30((unsigned)i)) {
        key[i] = (kStIn << 30) | key_low(k);
        root = 1;
    } else if (key_st(m) == kStIn) {
        key[i] = key_low(k);
    } else {
        *undecided = 1;   // benign race: every writer stores 1
    }
    if (ROOTS) flag[i] = root;
}


// the aggregation's host check in one read: {roots, undecided flag, rounds that did work}
__global__ void k_mis_pack(const int *__restrict__ roots, const int *__restrict__ und, const int *__restrict__ run,
                           int *__restrict__ out)
{
    if (threadIdx.x == 0) {
        out[0] = *roots;
        out[1] = *und;
        out[2] = *run;
    }
}

// out = 1 when the pattern (rowptr[0..n], col[0..key_nnz)) differs from the
// key (rowptr, then col); equal row pointers make the lengths equal, so the
// first key_nnz columns decide (columns read only below the buffer capacity,
// checked by the caller)
__global__ void k_pattern_diff(int n, const int *__restrict__ rowptr, const int *__restrict__ col,
                               const int *__restrict__ key, int key_nnz, int *__restrict__ out)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    bool d = false;
    if (t <= n) d = rowptr[t] != key[t];
    if (t < key_nnz) d = d || col[t] != key[n + 1 + t];
    if (d) out[0] = 1;
}

// The joins take G lanes per row (consecutive entries on consecutive lanes,
// G = 1 on the fine level): each lane keeps its best candidate in its own
// (increasing) entry order and the lanes' candidates are combined by the
// same total order the one-thread loop applies -- the largest key, on a tie
// the earlier entry (joins 1, 2), the largest |a_ij| and then the larger j
// (join 3) -- so every G selects the same neighbour.  The coarse levels'
// rows hold 10-40 entries: one thread walking them took 30-40 us per level.
template <int G>
__device__ __forceinline__ void join_best_key(MisKey &best, int &bk, int &bj)
{
#pragma unroll
    for (int off = 1; off < G; off <<= 1) {
        const MisKey ob = __shfl_xor(best, off, G);
        const int obk = __shfl_xor(bk, off, G), obj = __shfl_xor(bj, off, G);
        if (obj >= 0 && (bj < 0 || ob > best || (ob == best && obk < bk))) {
            best = ob;
            bk = obk;
            bj = obj;
        }
    }
}

// distance 1: roots keep their aggregate, neighbours of roots join the root
// with the largest key
// rows left out that have (weak) couplings to aggregated owned rows join the
// aggregate of the largest |a_ij| (ties: larger j); their P row is the
// tentative injection (no strong couplings -> smoothing weight 0)
template <int G>
__global__ void __launch_bounds__(kB) k_agg_join3(int n, int ncl, const int *__restrict__ rowptr, ColView cv,
                                                  const double *__restrict__ val, const int *__restrict__ agg2,
                                                  int *__restrict__ agg)
{
    const int i = (blockIdx.x * blockDim.x + threadIdx.x) / G, l = threadIdx.x % G;
    if (i >= n) return;   // (whole groups)
    int a = agg2[i];
    if (a < 0) {
        double best = 0.0;
        int bj = -1;
        const int cb = cv.base(i);
        for (int k = rowptr[i] + l; k < rowptr[i + 1]; k += G) {
            const int j = cv.at(cb, k);
            if (j == i || j >= ncl || agg2[j] < 0) continue;
            const double v = fabs(val[k]);
            if (v > best || (v == best && v > 0.0 && j > bj)) {
                best = v;
                bj = j;
            }
        }
#pragma unroll
        for (int off = 1; off < G; off <<= 1) {
            const double ob = __shfl_xor(best, off, G);
            const int obj = __shfl_xor(bj, off, G);
            if (obj >= 0 && (ob > best || (ob == best && ob > 0.0 && obj > bj))) {
                best = ob;
                bj = obj;
            }
        }
        if (bj >= 0) a = agg2[bj];
    }
    if (l == 0) agg[i] = a;
}

template <int G>
__global__ void __launch_bounds__(kB) k_agg_join1(int n, const int *__restrict__ rowptr, ColView cv,
                                                  const unsigned char *__restrict__ sflag,
                                                  const MisKey *__restrict__ key, const int *__restrict__ rootid,
                                                  int *__restrict__ agg1)
{
    const int i = (blockIdx.x * blockDim.x + threadIdx.x) / G, l = threadIdx.x % G;
    if (i >= n) return;
    if (key_st(key[i]) == kStIn) {
        if (l == 0) agg1[i] = rootid[i];
        return;
    }
    int bj = -1, bk = INT_MAX;
    MisKey best = 0;
    const int cb = cv.base(i);
    for (int k = rowptr[i] + l; k < rowptr[i + 1]; k += G) {
        if (sflag[k] != 1) continue;
        const int j = cv.at(cb, k);
        const MisKey kj = key[j];
        if (key_st(kj) == kStIn && (bj < 0 || key_low(kj) > best)) {
            best = key_low(kj);
            bj = j;
            bk = k;
        }
    }
    join_best_key<G>(best, bk, bj);
    if (l == 0) agg1[i] = (bj >= 0) ? rootid[bj] : -1;
}

// distance 2: the rest join the aggregate of their largest-key neighbour
// that joined at distance 1
template <int G>
__global__ void __launch_bounds__(kB) k_agg_join2(int n, const int *__restrict__ rowptr, ColView cv,
                                                  const unsigned char *__restrict__ sflag,
                                                  const MisKey *__restrict__ key, const int *__restrict__ agg1,
                                                  int *__restrict__ agg)
{
    const int i = (blockIdx.x * blockDim.x + threadIdx.x) / G, l = threadIdx.x % G;
    if (i >= n) return;
    const int a = agg1[i];
    if (a >= 0) {
        if (l == 0) agg[i] = a;
        return;
    }
    int bj = -1, bk = INT_MAX;
    MisKey best = 0;
    const int cb = cv.base(i);
    for (int k = rowptr[i] + l; k < rowptr[i + 1]; k += G) {
        if (sflag[k] != 1) continue;
        const int j = cv.at(cb, k);
        if (agg1[j] < 0) continue;
        const MisKey kl = key_low(key[j]);
        if (bj < 0 || kl > best) {
            best = kl;
            bj = j;
            bk = k;
        }
    }
    join_best_key<G>(best, bk, bj);
    if (l == 0) agg[i] = (bj >= 0) ? agg1[bj] : -1;   // -1: isolated (or unreachable) -> no coarse dof
}

// lanes per row of the aggregation joins for rows of this average length
static int join_lanes(double per_row)
{
    const int v = (int)env_int("XFK_JOIN_LANES", 0);   // (read per level: tests toggle it)
    if (v == 1 || v == 4 || v == 8) return v;
    return per_row <= 8.0 ? 1 : (per_row <= 16.0 ? 4 : 8);
}

// --------------------------------------------------------------------------
// setup: R = P^T
// --------------------------------------------------------------------------

// Tiled transpose: a workgroup of 256 rows holds its entries' columns in a
// window [lo, hi] (a banded numbering: a few hundred columns), counts them in
// LDS and touches the global counts once per (workgroup, column) instead of
// once per entry.
// The fill reserves one chunk of each target row per workgroup (returning
// atomic on the count-down counter), places its entries there through LDS
// cursors and writes the values with the columns; the row sort restores the
// order.  A window wider than kRtWin falls back to per-entry atomics.
constexpr int kRtWin = 4096;
template <bool FILL>
__global__ void __launch_bounds__(256) k_rt_tile(int n, const int *__restrict__ mrow, const int *__restrict__ mcol,
                                                 const double *__restrict__ mval, const int *__restrict__ trow,
                                                 int *__restrict__ cnt, int *__restrict__ tcol,
                                                 double *__restrict__ tval)
{
    __shared__ int h[kRtWin];
    __shared__ int cur[FILL ? kRtWin : 1];
    __shared__ int red[8];
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int s = i < n ? mrow[i] : 0, e = i < n ? mrow[i + 1] : 0;
    int lo = INT_MAX, hi = INT_MIN;   // (every entry: the rows need not be sorted)
    for (int k = s; k < e; ++k) {
        const int c = mcol[k];
        lo = min(lo, c);
        hi = max(hi, c);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        lo = min(lo, __shfl_xor(lo, off, 64));
        hi = max(hi, __shfl_xor(hi, off, 64));
    }
    if ((threadIdx.x & 63) == 0) {
        red[threadIdx.x >> 6] = lo;
        red[4 + (threadIdx.x >> 6)] = hi;
    }
    __syncthreads();
    lo = min(min(red[0], red[1]), min(red[2], red[3]));
    hi = max(max(red[4], red[5]), max(red[6], red[7]));
    if (hi < lo) return;   // no entries in this tile
    if ((long long)hi - lo >= kRtWin) {   // wide window: one global atomic per entry
        for (int k = s; k < e; ++k) {
            const int J = mcol[k];
            if (!FILL) {
                atomicAdd(&cnt[J], 1);
            } else {
                const int pos = trow[J] + atomicSub(&cnt[J], 1) - 1;
                tcol[pos] = i;
                tval[pos] = mval[k];
            }
        }
        return;
    }
    const int w = hi - lo + 1;
    for (int c = threadIdx.x; c < w; c += 256) {
        h[c] = 0;
        if (FILL) cur[c] = 0;
    }
    __syncthreads();
    for (int k = s; k < e; ++k) atomicAdd(&h[mcol[k] - lo], 1);
    __syncthreads();
    if (!FILL) {
        for (int c = threadIdx.x; c < w; c += 256)
            if (h[c]) atomicAdd(&cnt[lo + c], h[c]);
        return;
    }
    for (int c = threadIdx.x; c < w; c += 256) {
        const int m = h[c];
        if (m) h[c] = trow[lo + c] + atomicSub(&cnt[lo + c], m) - m;   // this tile's chunk of row lo + c
    }
    __syncthreads();
    for (int k = s; k < e; ++k) {
        const int c = mcol[k] - lo;
        const int pos = h[c] + atomicAdd(&cur[c], 1);
        tcol[pos] = i;
        tval[pos] = mval[k];
    }
}

// sort each row's (column, value) pairs by column (the rows' entries are
// distinct).  A wavefront takes 4 consecutive rows: when all hold <= 64
// entries (the usual case) each 16-lane group ranks its row's columns in
// wave-private LDS (rank = number of smaller columns, <= 64 broadcast reads
// per entry) and writes every pair straight to its rank -- no compare-exchange
// network, values never shuffled; longer rows are taken one at a time by the
// whole wavefront (<= kRtLdsRow entries in LDS, else lane 0's insertion sort).
constexpr int kRtLdsRow = 1024;
__global__ void __launch_bounds__(256) k_rt_sort_pairs(int nc, const int *__restrict__ rrow, int *__restrict__ rcol,
                                                       double *__restrict__ rval)
{
    __shared__ int buf[4][kRtLdsRow];
    __shared__ double bufv[4][kRtLdsRow];
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int J0 = ((blockIdx.x * blockDim.x + threadIdx.x) >> 6) * 4;
    if (J0 >= nc) return;
    int *b = buf[wv];
    double *bv = bufv[wv];
    auto wsync = [] {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    };
    // this group's row (groups past nc get an empty one)
    const int g = lane >> 4, gl = lane & 15, J = J0 + g;
    const int s = J < nc ? rrow[J] : 0, len = J < nc ? rrow[J + 1] - s : 0;
    int mx = len;
#pragma unroll
    for (int off = 16; off < 64; off <<= 1) mx = max(mx, __shfl_xor(mx, off, 64));
    if (mx <= 64) {
        int *gb = b + 64 * g;
        int kk[4];
        double vv[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int a = gl + 16 * q;
            kk[q] = a < len ? rcol[s + a] : 0;
            vv[q] = a < len ? rval[s + a] : 0.0;
            if (a < len) gb[a] = kk[q];
        }
        wsync();
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int a = gl + 16 * q;
            if (a < len) {
                int rk = 0;
                for (int t = 0; t < len; ++t) rk += gb[t] < kk[q];
                rcol[s + rk] = kk[q];
                rval[s + rk] = vv[q];
            }
        }
        return;
    }
    for (int r = 0; r < 4 && J0 + r < nc; ++r) {
        const int Jr = J0 + r;
        const int sr = rrow[Jr], er = rrow[Jr + 1], lr = er - sr;
        if (lr <= 1) continue;
        if (lr <= kRtLdsRow) {
            wsync();   // the previous row's reads of b are done
            for (int a = lane; a < lr; a += 64) {
                b[a] = rcol[sr + a];
                bv[a] = rval[sr + a];
            }
            wsync();
            for (int a = lane; a < lr; a += 64) {
                const int v = b[a];
                int rk = 0;
                for (int q = 0; q < lr; ++q) rk += b[q] < v;
                rcol[sr + rk] = v;
                rval[sr + rk] = bv[a];
            }
        } else if (lane == 0) {
            for (int a = sr + 1; a < er; ++a) {
                const int key = rcol[a];
                const double kv = rval[a];
                int q = a - 1;
                while (q >= sr && rcol[q] > key) {
                    rcol[q + 1] = rcol[q];
                    rval[q + 1] = rval[q];
                    --q;
                }
                rcol[q + 1] = key;
                rval[q + 1] = kv;
            }
        }
    }
}

// --------------------------------------------------------------------------
// setup: the folded transfer P~
// --------------------------------------------------------------------------

// Folded coarse level (V(1,1) with one Jacobi sweep, x_pre = w D^-1 b):
//   pre   y  = x_pre + w D^-1 (b - A x_pre),  b_c = P~^T b
//   post  x  = y + P~ x_c,                     P~ = (I - w D^-1 A) P
// equal in exact arithmetic to sweep-from-0 + residual, R r, x += P x_c and
// the post-sweep (R r' = P^T (I - w A D^-1) b = P~^T b for symmetric A), in
// two launches instead of four.  P~ is formed over the pattern of A P (which
// holds P's, the diagonal of A being nonzero).
// kFoldLanes lanes per row of A P, each entry's P_ij found by a scan of the
// (short: 2-3 entries) P row
constexpr int kFoldLanes = 8;
__global__ void __launch_bounds__(256) k_fold_p(int n, const unsigned long long *rho, const double *__restrict__ dinv,
                                                const int *__restrict__ aprow, const int *__restrict__ apcol,
                                                const double *__restrict__ apval, const int *__restrict__ prow,
                                                const int *__restrict__ pcol, const double *__restrict__ pval,
                                                int *__restrict__ fcol, double *__restrict__ fval)
{
    const int i = (int)(((long long)blockIdx.x * blockDim.x + threadIdx.x) / kFoldLanes);
    if (i >= n) return;
    const int g = threadIdx.x & (kFoldLanes - 1);
    const double ra = rho_of(rho);
    const double wd = (ra > 0.0 ? 1.0 / ra : 0.0) * dinv[i];
    const int pb = prow[i], pe = prow[i + 1];
    for (int k = aprow[i] + g; k < aprow[i + 1]; k += kFoldLanes) {
        const int c = apcol[k];
        double pij = 0.0;
        for (int q = pb; q < pe; ++q)
            if (pcol[q] == c) pij = pval[q];
        fcol[k] = c;
        fval[k] = pij - wd * apval[k];
    }
}

// A Newton refresh (new level-0 values, same pattern, same P): P~ re-formed
// numerically over its own pattern, P~_ic = P_ic - w d_i sum_j a_ij P_jc, no
// SpGEMM (the pattern of A P is the pattern of P~, which the setup formed).
// kFoldLanes lanes per row: the row's products a_ij x (c, P_jc) -- A's row in
// column order, each P row j in its stored order -- are staged in LDS once
// (the lanes' P-row lengths prefix-summed by shuffles); then one lane per P~
// entry c sums the products of column c in that order (P rows hold a column
// once, so the sum is the one over j in A's column order).  Rows of more than
// kRfA entries or kRfP products read A and P from memory in the same order.
// f32 (optional): the f32 copy of P~ written alongside.  stage = 0 reads
// every row from memory (XFK_REFOLD_STAGE=0: the test of the staged order).
constexpr int kRfA = 16, kRfP = 64, kRfRows = 256 / kFoldLanes;
static_assert(kRfA == 2 * kFoldLanes, "k_refold_p stages two A entries per lane");
__global__ void __launch_bounds__(256) k_refold_p(int n, const unsigned long long *rho, const double *__restrict__ dinv,
                                                  const int *__restrict__ rowptr, const int *__restrict__ col,
                                                  const double *__restrict__ val, const int *__restrict__ prow,
                                                  const int *__restrict__ pcol, const double *__restrict__ pval,
                                                  const int *__restrict__ frow, const int *__restrict__ fcol,
                                                  double *__restrict__ fval, float *__restrict__ f32, int stage)
{
    // (rows padded by one element: the 8 rows of a wave read one e at a time)
    __shared__ int s_pc[kRfRows][kRfP + 1];
    __shared__ double s_av[kRfRows][kRfP + 1], s_pv[kRfRows][kRfP + 1];
    const int lr = threadIdx.x / kFoldLanes, g = threadIdx.x & (kFoldLanes - 1);
    const int i = (int)blockIdx.x * kRfRows + lr;
    const bool live = i < n;   // (every thread reaches the barrier)
    const int ab = live ? rowptr[i] : 0, na = live ? rowptr[i + 1] - ab : 0;
    // lane g: A entries u = g and u = g + kFoldLanes, their P rows
    int pb[2] = {0, 0}, len[2] = {0, 0};
    double av[2] = {0.0, 0.0};
    if (na <= kRfA)
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int u = g + h * kFoldLanes;
            if (u < na) {
                const int j = col[ab + u];
                pb[h] = prow[j];
                len[h] = prow[j + 1] - pb[h];
                av[h] = val[ab + u];
            }
        }
    int off[2], tot = 0;
#pragma unroll
    for (int h = 0; h < 2; ++h) {   // exclusive prefix over u = 0 .. 15
        int inc = len[h];
#pragma unroll
        for (int d = 1; d < kFoldLanes; d <<= 1) {
            const int v = __shfl_up(inc, d, kFoldLanes);
            if (g >= d) inc += v;
        }
        off[h] = tot + inc - len[h];
        tot += __shfl(inc, kFoldLanes - 1, kFoldLanes);
    }
    const bool staged = stage && na <= kRfA && tot <= kRfP;
    if (staged)
#pragma unroll
        for (int h = 0; h < 2; ++h)
            for (int q = 0; q < len[h]; ++q) {
                s_pc[lr][off[h] + q] = pcol[pb[h] + q];
                s_pv[lr][off[h] + q] = pval[pb[h] + q];
                s_av[lr][off[h] + q] = av[h];
            }
    __syncthreads();
    if (!live) return;
    const double ra = rho_of(rho);
    const double wd = (ra > 0.0 ? 1.0 / ra : 0.0) * dinv[i];
    const int qb = prow[i], qe = prow[i + 1];
    for (int k = frow[i] + g; k < frow[i + 1]; k += kFoldLanes) {
        const int c = fcol[k];
        double ap = 0.0, pic = 0.0;
        for (int q = qb; q < qe; ++q)
            if (pcol[q] == c) pic = pval[q];
        if (staged) {
            for (int e = 0; e < tot; ++e)
                if (s_pc[lr][e] == c) ap = fma(s_av[lr][e], s_pv[lr][e], ap);
        } else {
            for (int t = ab; t < ab + na; ++t) {
                const int j = col[t];
                for (int q = prow[j]; q < prow[j + 1]; ++q)
                    if (pcol[q] == c) ap = fma(val[t], pval[q], ap);
            }
        }
        const double v = pic - wd * ap;
        fval[k] = v;
        if (f32) f32[k] = (float)v;
    }
}

// diagnostics (XFK_AMG_DEBUG): rows left without an aggregate, split by
// whether they have strong (owned) couplings / any off-diagonal coupling
__global__ void k_setup_zero(int *__restrict__ a, int na, unsigned long long *__restrict__ b, int nb_)
{
    for (int k = threadIdx.x; k < na; k += blockDim.x) a[k] = 0;
    for (int k = threadIdx.x; k < nb_; k += blockDim.x) b[k] = 0ull;
}

__global__ void k_debug_unagg(int n, const int *__restrict__ rowptr, const int *__restrict__ col,
                              const int *__restrict__ sdeg, const int *__restrict__ agg, int *out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || agg[i] >= 0) return;
    int offd = 0;
    for (int k = rowptr[i]; k < rowptr[i + 1]; ++k) offd += (col[k] != i);
    atomicAdd(&out[sdeg[i] > 0 ? 0 : (offd > 0 ? 1 : 2)], 1);
}

// --------------------------------------------------------------------------
// sharded level 0: helpers of the distributed Galerkin product and V-cycle
// --------------------------------------------------------------------------

__global__ void k_row_len_d(int n, const int *__restrict__ rowptr, double *__restrict__ len)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) len[i] = (double)(rowptr[i + 1] - rowptr[i]);
}
__global__ void k_dbl2int(long long n, const double *__restrict__ a, int *__restrict__ b)
{
    const long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    if (i < n) b[i] = (int)a[i];
}
__global__ void k_int2dbl(long long n, const int *__restrict__ a, double *__restrict__ b)
{
    const long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    if (i < n) b[i] = (double)a[i];
}
// b = (float) a over the rowptr[n] entries of a CSR (the length read on the
// device: the host may only hold an upper bound); fixed grid, grid-stride
__global__ void k_d2f(int n, const int *__restrict__ rowptr, const double *__restrict__ a, float *__restrict__ b)
{
    const long long m = rowptr[n];
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < m; i += (long long)gridDim.x * blockDim.x)
        b[i] = (float)a[i];
}

__global__ void k_add_int(long long n, int *__restrict__ a, int v)
{
    const long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    if (i < n) a[i] += v;
}
// row pointer of P extended by the halo rows: owned rows, then pnnz + hrow
__global__ void k_pe_row(int n, int nh, long long pnnz, const int *__restrict__ prow, const int *__restrict__ hrow,
                         int *__restrict__ out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i <= n) out[i] = prow[i];
    else if (i <= n + nh) out[i] = (int)pnnz + hrow[i - n];
}
// global coarse row pointer from the all-gathered per-rank row pointers
// (stride ld per rank); c0 / e0: first row / entry of each rank (nranks + 1)
__global__ void k_concat_rowptr(int NC, int nranks, const int *__restrict__ c0, const int *__restrict__ e0,
                                const int *__restrict__ grow, int ld, int *__restrict__ out)
{
    const int I = blockIdx.x * blockDim.x + threadIdx.x;
    if (I > NC) return;
    if (I == NC) {
        out[I] = e0[nranks];
        return;
    }
    int q = 0;
    while (c0[q + 1] <= I) ++q;
    out[I] = e0[q] + grow[(size_t)q * ld + (I - c0[q])];
}

}  // namespace

// --------------------------------------------------------------------------
// host side
// --------------------------------------------------------------------------

Amg::~Amg()
{
    pinned_free(nd_stage);   // (to the process cache when the problem is destroyed)
    pinned_free(def_host);
    pinned_free(host_int);
    pinned_free(host_big);
    if (ev_host) (void)hipEventDestroy(ev_host);
    for (hipEvent_t e : tail_ev) (void)hipEventDestroy(e);
    delete trace;
}

namespace {

// out[0..n] = exclusive scan of in[0..n-1], out[n] = total; returns total
// Short scans (coarse levels: <= kScanLds entries) in one workgroup, one
// launch instead of hipcub's memset + state init + scan: each of 1024 threads
// loads 16 consecutive entries at once (four 16-B loads), scans them in
// registers, a workgroup scan of the thread sums gives the offsets, and the
// prefixes are stored -- one memory round trip each way.
constexpr int kScanLds = 16384;

__global__ void __launch_bounds__(1024) k_scan_lds(int n, const int *__restrict__ in, int *__restrict__ out)
{
    __shared__ int wsum[16];
    const int b = 16 * threadIdx.x;
    int v[16];
    if (b + 16 <= n && (reinterpret_cast<uintptr_t>(in) & 15) == 0) {
        const int4 *p = reinterpret_cast<const int4 *>(in + b);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int4 x = p[q];
            v[4 * q] = x.x;
            v[4 * q + 1] = x.y;
            v[4 * q + 2] = x.z;
            v[4 * q + 3] = x.w;
        }
    } else {
#pragma unroll
        for (int q = 0; q < 16; ++q) v[q] = b + q < n ? in[b + q] : 0;
    }
#pragma unroll
    for (int q = 1; q < 16; ++q) v[q] += v[q - 1];
    const int loc = v[15];
    // exclusive scan of the thread sums over the workgroup
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    int x = loc;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int t = __shfl_up(x, off, 64);
        if (lane >= off) x += t;
    }
    if (lane == 63) wsum[wid] = x;
    __syncthreads();
    int before = x - loc;
#pragma unroll
    for (int w = 0; w < 16; ++w)
        if (w < wid) before += wsum[w];
#pragma unroll
    for (int q = 0; q < 16; ++q)
        if (b + q < n) out[b + q + 1] = before + v[q];
    if (threadIdx.x == 0) out[0] = 0;
}

}  // namespace

// (declared in xfk_amg_impl.h: the SpGEMM driver scans its row lengths too)
int scan_total(Amg &A, hipStream_t s, const int *in, int *out, int n, long long &total)
{
    if (n <= kScanLds) {
        k_scan_lds<<<1, 1024, 0, s>>>(n, in, out);
        AMG_CHECK(hipGetLastError());
    } else {
        size_t bytes = 0;
        AMG_CHECK(hipcub::DeviceScan::InclusiveSum(nullptr, bytes, in, out + 1, n, s));
        AMG_CHECK(A.cub_tmp.alloc(bytes ? bytes : 1));
        AMG_CHECK(hipMemsetAsync(out, 0, sizeof(int), s));
        if (n > 0) AMG_CHECK(hipcub::DeviceScan::InclusiveSum(A.cub_tmp.p, bytes, in, out + 1, n, s));
    }
    AMG_CHECK(hipMemcpyAsync(A.host_int, out + n, sizeof(int), hipMemcpyDeviceToHost, s));
    AMG_CHECK(hipStreamSynchronize(s));
    total = A.host_int[0];
    return XFK_OK;
}

// the same without reading the total back (no host synchronisation), with
// the given temporary storage.  `in` must hold n + 1 readable entries: the
// long scans are exclusive over n + 1 (out[0] = 0 without a memset; in[n]
// only fills the unused last slot)
int scan_only(DBuf<char> &tmp, hipStream_t s, const int *in, int *out, int n)
{
    if (n <= kScanLds) {
        k_scan_lds<<<1, 1024, 0, s>>>(n, in, out);
        AMG_CHECK(hipGetLastError());
        return XFK_OK;
    }
    size_t bytes = 0;
    AMG_CHECK(hipcub::DeviceScan::ExclusiveSum(nullptr, bytes, in, out, n + 1, s));
    AMG_CHECK(tmp.alloc(bytes ? bytes : 1));
    AMG_CHECK(hipcub::DeviceScan::ExclusiveSum(tmp.p, bytes, in, out, n + 1, s));
    return XFK_OK;
}
int scan_only(Amg &A, hipStream_t s, const int *in, int *out, int n) { return scan_only(A.cub_tmp, s, in, out, n); }

int read_flag(Amg &A, hipStream_t s, int idx, int &v)
{
    AMG_CHECK(hipMemcpyAsync(A.host_int + 1, A.dev_int.p + idx, sizeof(int), hipMemcpyDeviceToHost, s));
    AMG_CHECK(hipStreamSynchronize(s));
    v = A.host_int[1];
    return XFK_OK;
}

// XFK_SPGEMM_PACK=0: the Galerkin products sort (column, value) pairs like the
// prolongator's (read per setup: tests toggle it)
static bool spgemm_pack_on()
{
    return env_int("XFK_SPGEMM_PACK", 1) != 0;
}

// tile t reads a halo column (>= n) in one of its rows
__global__ void k_tile_halo_flags(int n, int B, const int *__restrict__ rowptr, const int *__restrict__ col,
                                  int *__restrict__ flag)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    bool h = false;
    for (int k = rowptr[i]; k < rowptr[i + 1]; ++k) h = h || col[k] >= n;
    if (h) flag[i / B] = 1;   // benign race: every writer stores 1
}

int build_tile_split(hipStream_t s, int n, int B, const int *rowptr, const int *col, TileSplit &ts)
{
    const int nt = (n + B - 1) / B;
    ts.B = 0;
    ts.n_in = ts.n_bd = 0;
    if (nt == 0) {
        ts.B = B;
        return XFK_OK;
    }
    DBuf<int> flag;
    AMG_CHECK(flag.alloc(nt));
    AMG_CHECK(hipMemsetAsync(flag.p, 0, sizeof(int) * nt, s));
    k_tile_halo_flags<<<nb(n), kB, 0, s>>>(n, B, rowptr, col, flag.p);
    std::vector<int> h(nt), list;
    list.reserve(nt);
    AMG_CHECK(hipMemcpyAsync(h.data(), flag.p, sizeof(int) * nt, hipMemcpyDeviceToHost, s));
    AMG_CHECK(hipStreamSynchronize(s));
    for (int t = 0; t < nt; ++t)
        if (!h[t]) list.push_back(t);
    ts.n_in = (int)list.size();
    for (int t = 0; t < nt; ++t)
        if (h[t]) list.push_back(t);
    ts.n_bd = nt - ts.n_in;
    AMG_CHECK(ts.tiles.alloc(nt));
    AMG_CHECK(hipMemcpyAsync(ts.tiles.p, list.data(), sizeof(int) * nt, hipMemcpyHostToDevice, s));
    AMG_CHECK(hipStreamSynchronize(s));   // `list` is a host temporary
    ts.B = B;
    return XFK_OK;
}

namespace {
std::mutex g_pool_mu;
std::map<hipStream_t, int> g_pool_dev;                 // every pooled stream -> its device
std::map<int, std::vector<hipStream_t>> g_pool_free;   // idle streams per device
}  // namespace

hipError_t stream_acquire(hipStream_t *s)
{
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    {
        std::lock_guard<std::mutex> lk(g_pool_mu);
        auto &f = g_pool_free[dev];
        if (!f.empty()) {
            *s = f.back();
            f.pop_back();
            return hipSuccess;
        }
    }
    e = hipStreamCreateWithFlags(s, hipStreamNonBlocking);
    if (e == hipSuccess) {
        std::lock_guard<std::mutex> lk(g_pool_mu);
        g_pool_dev[*s] = dev;
    }
    return e;
}

void stream_release(hipStream_t s)
{
    if (!s) return;
    std::lock_guard<std::mutex> lk(g_pool_mu);
    auto it = g_pool_dev.find(s);
    if (it == g_pool_dev.end()) {
        (void)hipStreamDestroy(s);
        return;
    }
    g_pool_free[it->second].push_back(s);
}

void stream_pool_drain()
{
    std::vector<hipStream_t> idle;
    {
        std::lock_guard<std::mutex> lk(g_pool_mu);
        for (auto &kv : g_pool_free)
            for (hipStream_t q : kv.second) {
                idle.push_back(q);
                g_pool_dev.erase(q);
            }
        g_pool_free.clear();
    }
    for (hipStream_t q : idle) (void)hipStreamDestroy(q);
}

long long stream_pool_idle()
{
    std::lock_guard<std::mutex> lk(g_pool_mu);
    long long n = 0;
    for (auto &kv : g_pool_free) n += (long long)kv.second.size();
    return n;
}

int SideStream::init()
{
    if (cs) return XFK_OK;
    AMG_CHECK(stream_acquire(&cs));
    AMG_CHECK(hipEventCreateWithFlags(&a, hipEventDisableTiming));
    AMG_CHECK(hipEventCreateWithFlags(&b, hipEventDisableTiming));
    AMG_CHECK(hipEventCreateWithFlags(&c, hipEventDisableTiming));
    return XFK_OK;
}

SideStream::~SideStream()
{
    if (a) (void)hipEventDestroy(a);
    if (b) (void)hipEventDestroy(b);
    if (c) (void)hipEventDestroy(c);
    if (cs) {
        (void)hipStreamSynchronize(cs);
        stream_release(cs);
    }
}

// The folded coarse level that runs a W-cycle (two coarse corrections): by
// default the level above the last V-cycle level (nlev - 3: on configs[2]
// level 1, whose coarse level of 14k rows costs a few launches per visit;
// 21 -> 18 PCG iterations), in single-device and replicated hierarchies
// alike.  wlevel when set (-1: none).
int Amg::wcycle_level() const
{
    if (wlevel != -2) return wlevel;
    return nlev >= 4 ? nlev - 3 : -1;
}

// W-cycle at level l: l is the W level
bool Amg::w_at(int l) const
{
    const int w = wcycle_level();
    return w >= 0 && l == w && l + 1 < nlev - 1;
}

// f32 copy of a CSR's values (cap: an upper bound of its length, for the allocation)
static int to_f32(hipStream_t s, int n, const int *rowptr, long long cap, const double *a, DBuf<float> &b)
{
    if (b.alloc((size_t)std::max(1LL, cap)) != hipSuccess) return XFK_ERR_HIP;
    if (n > 0) k_d2f<<<2048, 256, 0, s>>>(n, rowptr, a, b.p);
    return XFK_OK;
}

// Off by default: on MI355X each cross-stream hop (side stream waits for the
// main stream, main waits for the exchange) costs more than the interior
// tiles it overlaps -- configs[4] rank 0 of 8, compute only, 469 vs 304 us
// per PCG iteration (profiles/r04c_rank0_overlap.txt).  XFK_OVERLAP=1 turns
// it on.
bool overlap_enabled() { return env_int("XFK_OVERLAP", 0) != 0; }

int Amg::resolve_deferred(hipStream_t s, bool &overflow)
{
    int rc = fetch_deferred(s);
    if (rc != XFK_OK) return rc;
    return wait_deferred(s, overflow);
}

// the deferred slots' read, enqueued (the host waits for it in wait_deferred;
// work enqueued in between runs meanwhile)
int Amg::fetch_deferred(hipStream_t s)
{
    if (def_n == 0) return XFK_OK;
    AMG_CHECK(hipMemcpyAsync(def_host, def_dev.p, sizeof(int) * kAmgDeferTotal, hipMemcpyDeviceToHost, s));
    AMG_CHECK(hipEventRecord(ev_host, s));
    return XFK_OK;
}

int Amg::wait_deferred(hipStream_t s, bool &overflow)
{
    overflow = false;
    if (def_n == 0) return XFK_OK;
    AMG_CHECK(hipEventSynchronize(ev_host));
    for (int q = 0; q < def_n / 2; ++q) {
        if (def_host[2 * q]) overflow = true;
        else if (def_verify[q] && !def_host[kAmgDeferSlots + q]) overflow = true;   // another class measured
        else *def_target[q] = def_host[2 * q + 1];
        def_verify[q] = 0;
    }
    def_n = 0;
    AMG_CHECK(hipMemsetAsync(def_dev.p, 0, sizeof(int) * kAmgDeferTotal, s));
    return XFK_OK;
}

int Amg::host_ints(int count)
{
    if (host_big_n >= count) return XFK_OK;
    pinned_free(host_big);   // (outside a destroy: hipHostFree)
    host_big = nullptr;
    host_big_n = 0;
    AMG_CHECK(pinned_malloc((void **)&host_big, sizeof(int) * std::max(count, 1)));
    host_big_n = count;
    return XFK_OK;
}

int Amg::reserve_host()
{
    if (!host_int) AMG_CHECK(pinned_malloc((void **)&host_int, 16 * sizeof(int)));
    if (!def_host) AMG_CHECK(pinned_malloc((void **)&def_host, kAmgDeferTotal * sizeof(int)));
    if (!ev_host) AMG_CHECK(hipEventCreateWithFlags(&ev_host, hipEventDisableTiming));
    constexpr int kHostBig = 64 << 10;   // ints: a coarsest pattern of ~1600 rows x 40
    if (host_big_n < kHostBig) {
        const int rc = host_ints(kHostBig);
        if (rc != XFK_OK) return rc;
    }
    constexpr size_t kStage = 64 << 10;  // bytes: a nested-dissection plan of ~1600 rows
    if (nd_stage_n < kStage) {
        pinned_free(nd_stage);
        nd_stage = nullptr;
        nd_stage_n = 0;
        AMG_CHECK(pinned_malloc((void **)&nd_stage, kStage));
        nd_stage_n = kStage;
    }
    return XFK_OK;
}

int Amg::init(hipStream_t s)
{
    if (!host_int) AMG_CHECK(pinned_malloc((void **)&host_int, 16 * sizeof(int)));
    if (!ev_host) AMG_CHECK(hipEventCreateWithFlags(&ev_host, hipEventDisableTiming));
    if (!def_host) AMG_CHECK(pinned_malloc((void **)&def_host, kAmgDeferTotal * sizeof(int)));
    AMG_CHECK(dev_int.alloc(8));
    AMG_CHECK(def_dev.alloc(kAmgDeferTotal));
    def_n = 0;
    for (int &v : def_verify) v = 0;
    AMG_CHECK(rho.alloc(2 * kAmgMaxLevels));
    k_setup_zero<<<1, 64, 0, s>>>(def_dev.p, kAmgDeferTotal, rho.p, 2 * kAmgMaxLevels);   // (one launch, not two fills)
    if (L.empty()) L.emplace_back(new AmgLevel());
    for (auto &lv : L) {   // levels are rebuilt: none sharded until setup_dist says so
        lv->dist = false;
        lv->has16 = false;
        lv->has32 = false;
        lv->plan = HaloPlan();
        lv->ts.B = 0;
    }
    stats = AmgStats();
    dense_coarse = false;
    return XFK_OK;
}

// Hints of a fresh hierarchy, a priori from the longest fine row m (one int
// read with the pattern's length, no host check):
//   P = (I - W D^-1 A_F) P_tent on level 0: one product per entry of A's row,
//     at most m -- exact, so it is the capacity a measurement would choose;
//   MIS-2: 12 rounds per level (11-12 measured on configs[1] / configs[2]).
// The other products are measured in the first setup (a host check each):
// an a priori bound for them is 2x oversized, and a capacity carried over
// from an oversized first setup would stay so (the sort kernels over twice
// the padded rows: round 4 measured the warm setup 2.24 -> 2.64 ms with
// seeded A P and R (A P) capacities), while a capacity that changes between
// setups changes the Galerkin products' summation order, so repeated solves
// would no longer be bit-identical.

// Hints across problems.  A fresh problem has no hints of its own; the last
// single-device setup of the process leaves its SpGEMM capacities, MIS-2
// round counts and the coarsest nested-dissection plan here, keyed by the
// fine level's size (the next rotor angle, the next analysis of a session:
// the same mesh family).  A fresh hierarchy of the same size takes them as
// speculation, checked on the device, never trusted: a capacity must show no
// overflow AND some row needing more than half of it (else a measurement
// would have chosen a smaller class, with another sort order: the setup is
// redone with measured capacities, so the bits are always those of the
// measured class); the round counts only size the MIS-2 batches; the plan is
// used only if the coarsest pattern equals its key (k_pattern_diff).
// XFK_AMG_NO_FOREIGN=1: fresh problems measure everything.
namespace {
struct HintStore {
    std::mutex mu;
    bool valid = false;
    int n0 = 0;
    long long nnz0 = 0;
    std::map<int, int> cap, mis;
    std::vector<int> nd_key;
    std::vector<Amg::NdPhase> nd_phases;
    int nd_ld = 0, nd_key_n = -1;
    long long nd_key_nnz = 0;
    std::vector<char> nd_plan;   // perm, iperm, tiles, masks as nd_order uploads them
    size_t nd_tl_n = 0, nd_mask_n = 0;
};
HintStore &hint_store()
{
    static HintStore *h = new HintStore();   // (never destroyed, like the device caches)
    return *h;
}
}  // namespace

}  // namespace xfk

extern "C" int xfk_amg_forget_hints(void)
{
    xfk::HintStore &h = xfk::hint_store();
    std::lock_guard<std::mutex> g(h.mu);
    h.valid = false;
    h.cap.clear();
    h.mis.clear();
    h.nd_key.clear();
    h.nd_phases.clear();
    h.nd_plan.clear();
    h.nd_key_n = -1;
    return XFK_OK;
}

namespace xfk {

void Amg::save_hints(int n0, long long nnz0)
{
    if (!foreign_on() || cap_hint.empty()) return;
    HintStore &h = hint_store();
    std::lock_guard<std::mutex> g(h.mu);
    h.valid = true;
    h.n0 = n0;
    h.nnz0 = nnz0;
    h.cap = cap_hint;
    // XFK_AMG_TEST_FOREIGN_BIG=1 (tests only): store one class too large, so
    // the next problem's device check must refuse it and rebuild
    if (env_set("XFK_AMG_TEST_FOREIGN_BIG"))
        for (auto &c : h.cap) c.second = std::min(2 * c.second, (int)kSortCap);
    h.mis = mis_hint;
    h.nd_key = nd_key;
    h.nd_phases = nd_phases_key;
    h.nd_ld = nd_ld;
    h.nd_key_n = nd_key_n;
    h.nd_key_nnz = nd_key_nnz;
    h.nd_plan = nd_plan;
    h.nd_tl_n = nd_tl_n;
    h.nd_mask_n = nd_mask_n;
}

int Amg::load_hints(hipStream_t s, int n0, long long nnz0)
{
    foreign = false;
    if (!foreign_on() || !cap_hint.empty() || !mis_hint.empty()) return XFK_OK;
    HintStore &h = hint_store();
    std::lock_guard<std::mutex> g(h.mu);
    if (!h.valid || h.n0 != n0 || h.nnz0 != nnz0) return XFK_OK;
    cap_hint = h.cap;
    mis_hint = h.mis;
    foreign = true;
    const size_t plan_bytes = sizeof(int) * ((size_t)h.nd_key_n + h.nd_ld + h.nd_tl_n) + h.nd_mask_n;
    if (h.nd_key_n > 0 && !h.nd_key.empty() && !h.nd_phases.empty() && h.nd_plan.size() == plan_bytes) {
        const int n = h.nd_key_n, ld = h.nd_ld;
        AMG_CHECK(cinv_perm.alloc(n));
        AMG_CHECK(cinv_iperm.alloc(ld));
        AMG_CHECK(nd_mask.alloc(h.nd_mask_n));
        AMG_CHECK(nd_tiles.alloc(h.nd_tl_n));
        const char *q = h.nd_plan.data();
        AMG_CHECK(hipMemcpyAsync(cinv_perm.p, q, sizeof(int) * n, hipMemcpyHostToDevice, s));
        AMG_CHECK(hipMemcpyAsync(cinv_iperm.p, q + sizeof(int) * n, sizeof(int) * ld, hipMemcpyHostToDevice, s));
        AMG_CHECK(hipMemcpyAsync(nd_tiles.p, q + sizeof(int) * ((size_t)n + ld), sizeof(int) * h.nd_tl_n,
                                 hipMemcpyHostToDevice, s));
        AMG_CHECK(hipMemcpyAsync(nd_mask.p, q + sizeof(int) * ((size_t)n + ld + h.nd_tl_n), h.nd_mask_n,
                                 hipMemcpyHostToDevice, s));
        nd_plan = h.nd_plan;
        nd_tl_n = h.nd_tl_n;
        nd_mask_n = h.nd_mask_n;
        nd_key = h.nd_key;
        nd_phases_key = h.nd_phases;
        nd_ld = h.nd_ld;
        nd_key_n = h.nd_key_n;
        nd_key_nnz = h.nd_key_nnz;
        AMG_CHECK(nd_key_dev.alloc(nd_key.size()));
        AMG_CHECK(hipMemcpyAsync(nd_key_dev.p, nd_key.data(), sizeof(int) * nd_key.size(), hipMemcpyHostToDevice, s));
        AMG_CHECK(hipStreamSynchronize(s));   // (the host vector is the staging buffer; a first setup only)
    }
    return XFK_OK;
}

void Amg::seed_hints()
{
    if (row_max0 <= 0 || !cap_hint.empty() || !mis_hint.empty()) return;
    auto cap = [](long long v) { return v <= 16 ? 16 : v <= 32 ? 32 : v <= 64 ? 64 : v <= 128 ? 128 : 256; };
    if (row_max0 <= kSortCap) cap_hint[0] = cap(row_max0);
    for (int l = 0; l < kAmgMaxLevels; ++l) mis_hint[l] = 12;
}

double Amg::theta_at(int l) const
{
    if (l == 0) return theta;
    return theta_coarse >= 0.0 ? theta_coarse : theta;
}

int Amg::setup(hipStream_t s, int n0, int ncl0, const int *rowptr0, const int *col0, const double *val0,
               long long nnz0)
{
    dist = false;
    comm = nullptr;
    lrep = 0;
    int rc = load_hints(s, n0, nnz0);
    if (rc != XFK_OK) return rc;
    seed_hints();
    rc = init(s);
    if (rc != XFK_OK) return rc;
    AmgLevel &F = *L[0];
    F.n = n0;
    F.nnz = nnz0;
    F.ncol_lim = ncl0;
    F.ncol_smooth = ncl0;
    F.rowptr = rowptr0;
    F.col = col0;
    F.val = val0;
    rc = build(s, 0);
    if (rc == XFK_OK) {
        foreign = false;   // (verified, or rebuilt with measured capacities)
        save_hints(n0, nnz0);
    }
    return rc;
}

// MIS-2 aggregation of level l, P = (I - omega D_F^-1 A_F) P_tent and R = P^T
// (strength flags and rho_F already computed).  nc = 0 when the level does
// not coarsen usefully (allow_stop) or has no aggregate.
// T = M^T of an n x nc CSR whose rows are sorted by column (T's rows come
// out sorted by row): counting transpose, the fill counting the row counts
// back down and carrying the values, then each row's pairs sorted by rank.
// T's arrays hold as many entries as M (no read-back of the scan).
// cnt / tmp: scratch of the stream it runs on (the setup's side stream has its own)
static int transpose_csr(DBuf<int> &cnt, DBuf<char> &tmp, hipStream_t s, int n, int nc, const int *mrow,
                         const int *mcol, const double *mval, int *trow, int *tcol, double *tval)
{
    AMG_CHECK(cnt.alloc((size_t)std::max(n, nc) + 1));
    AMG_CHECK(hipMemsetAsync(cnt.p, 0, sizeof(int) * ((size_t)nc + 1), s));
    if (n > 0) k_rt_tile<false><<<nb(n), 256, 0, s>>>(n, mrow, mcol, mval, trow, cnt.p, tcol, tval);
    int rc = scan_only(tmp, s, cnt.p, trow, nc);
    if (rc != XFK_OK) return rc;
    if (n > 0) k_rt_tile<true><<<nb(n), 256, 0, s>>>(n, mrow, mcol, mval, trow, cnt.p, tcol, tval);
    if (nc > 0) k_rt_sort_pairs<<<(int)((((long long)nc + 3) / 4 * 64 + 255) / 256), 256, 0, s>>>(nc, trow, tcol, tval);
    AMG_CHECK(hipGetLastError());
    return XFK_OK;
}

// 16-bit tile columns (xfk_spmv.h) of an n-row CSR in tiles of B rows, on st
template <int B>
static int build_col16(hipStream_t st, int n, const int *rowptr, const int *col, long long nnz,
                       DBuf<unsigned short> &c16, DBuf<int> &base)
{
    const int nt = (n + B - 1) / B;
    AMG_CHECK(c16.alloc((size_t)std::max(1LL, nnz)));
    AMG_CHECK(base.alloc((size_t)std::max(1, nt)));
    if (nt > 0) k_tile_col16<B><<<nt, 256, 0, st>>>(n, rowptr, col, c16.p, base.p);
    AMG_CHECK(hipGetLastError());
    return XFK_OK;
}

int Amg::aggregate(hipStream_t s, int l, long long &nc, bool allow_stop)
{
    AmgLevel &A = *L[l];
    const int n = A.n;
    const ColView cv{A.col, A.has16 ? A.a16.p : nullptr, A.has16 ? A.a16b.p : nullptr};
    nc = 0;
    A.nc = 0;
    AMG_CHECK(key.alloc(n));
    AMG_CHECK(t1.alloc(n));
    const std::string lv = g_prof ? "setup L" + std::to_string(l) + " " : std::string();
    if (g_prof) g_prof->begin(lv + "MIS-2 aggregation", 0.0);
    int rounds = 0;
    int *und2 = dev_int.p + 4;   // undecided flag of rounds of parity 0 / 1
    int *run = dev_int.p + 7;    // rounds that did work
    AMG_CHECK(act.alloc(n));
    k_mis_init<<<std::max(1, nb(n)), kB, 0, s>>>(n, cnt.p, key.p, und2 + 1, run, act.p);
    AMG_CHECK(flag.alloc((size_t)n + 1));
    AMG_CHECK(cursor.alloc((size_t)n + 1));
    // Batches of rounds without a host check; the first batch is the round
    // count this level needed in the last setup (the same matrix family
    // needs the same count: one host check in the usual case, no idle
    // rounds), 12 without one.  Roots and their numbering are formed
    // speculatively after each batch and read back in the same host check.
    auto hint = mis_hint.find(l);
    // speculative joins and P need a round hint and a hinted (non-synchronising) P
    // (levels of a sharded hierarchy replicated on every rank speculate like a
    // single device's: every rank holds the same level and hints, so every
    // rank takes the same decisions; sharded levels keep their host checks)
    const bool spec = !g_prof && !A.dist && hint != mis_hint.end() && cap_hint.count(4 * l) &&
                      def_n + 4 <= kAmgDeferSlots && !env_set("XFK_AMG_DEBUG");
    bool joined = false;
    auto joins_and_p = [&]() { return joins_and_p_impl(s, l); };
    AMG_CHECK(mis_out.alloc(4));
    for (int batch = hint != mis_hint.end() ? std::max(1, hint->second) : 12;; batch = 2) {
        for (int b = 0; b < batch; ++b, ++rounds) {
            int *cur = und2 + (rounds & 1), *prev = und2 + ((rounds + 1) & 1);
            const bool last = b + 1 == batch;   // its update also writes the root flags
            if (A.nnz > 9LL * n) {
                k_mis_max<4><<<nb(4LL * n), kB, 0, s>>>(n, A.rowptr, cv, sflag.p, key.p, t1.p, prev, cur, run, act.p);
                if (last)
                    k_mis_update<4, true><<<nb(4LL * n), kB, 0, s>>>(n, A.rowptr, cv, sflag.p, t1.p, key.p, prev, cur,
                                                                      flag.p);
                else
                    k_mis_update<4><<<nb(4LL * n), kB, 0, s>>>(n, A.rowptr, cv, sflag.p, t1.p, key.p, prev, cur,
                                                                nullptr);
            } else {
                k_mis_max<1><<<nb(n), kB, 0, s>>>(n, A.rowptr, cv, sflag.p, key.p, t1.p, prev, cur, run, act.p);
                if (last)
                    k_mis_update<1, true><<<nb(n), kB, 0, s>>>(n, A.rowptr, cv, sflag.p, t1.p, key.p, prev, cur,
                                                                flag.p);
                else
                    k_mis_update<1><<<nb(n), kB, 0, s>>>(n, A.rowptr, cv, sflag.p, t1.p, key.p, prev, cur, nullptr);
            }
        }
        int rc = scan_only(*this, s, flag.p, cursor.p, n);   // cursor = root ids
        if (rc != XFK_OK) return rc;
        k_mis_pack<<<1, 64, 0, s>>>(cursor.p + n, und2 + ((rounds - 1) & 1), run, mis_out.p);
        AMG_CHECK(hipMemcpyAsync(host_int + 8, mis_out.p, 3 * sizeof(int), hipMemcpyDeviceToHost, s));
        AMG_CHECK(hipEventRecord(ev_host, s));
        // while the host waits for the check, the device goes on with the
        // joins and P (correct when the check finds the MIS complete -- the
        // usual case with a round hint; otherwise redone after more rounds)
        joined = spec;
        if (spec && (rc = joins_and_p()) != XFK_OK) return rc;
        AMG_CHECK(hipEventSynchronize(ev_host));
        if (!host_int[9]) break;
        joined = false;
        if (rounds > 4096) {
            set_error("AMG: MIS-2 aggregation did not terminate");
            return XFK_ERR_NOCONV;
        }
    }
    mis_hint[l] = host_int[10];
    nc = host_int[8];
    stats.mis_rounds[l] = host_int[10];
    int rc = XFK_OK;
    if (allow_stop && (nc == 0 || nc > (long long)(0.9 * n))) {   // no useful coarsening: smoother-only coarsest
        nc = 0;
        return XFK_OK;
    }
    if (!joined && (rc = joins_and_p()) != XFK_OK) return rc;
    A.nc = (int)nc;
    if (env_set("XFK_AMG_DEBUG")) std::fprintf(stderr, "[amg] level %d P nnz %lld\n", l, A.pnnz);
    // R = P^T: on the side stream (single-device levels) while the main
    // stream forms A P; the Galerkin product R (A P) waits for it
    AMG_CHECK(A.rrow.alloc((size_t)nc + 1));
    AMG_CHECK(A.rcol.alloc((size_t)std::max(1LL, A.pnnz)));
    AMG_CHECK(A.rval.alloc((size_t)std::max(1LL, A.pnnz)));
    const bool off = !A.dist && !dist;
    hipStream_t ts = s;
    if (off) {
        if ((rc = sw.init()) != XFK_OK) return rc;
        AMG_CHECK(hipEventRecord(sw.a, s));
        AMG_CHECK(hipStreamWaitEvent(sw.cs, sw.a, 0));
        ts = sw.cs;
        sw_used = true;
    }
    if ((rc = transpose_csr(off ? cnt2 : cnt, off ? cub_tmp2 : cub_tmp, ts, n, (int)nc, A.prow.p, A.pcol.p,
                            A.pval.p, A.rrow.p, A.rcol.p, A.rval.p)) != XFK_OK)
        return rc;
    if (off) {   // R (A P) waits for R itself; R's V-cycle forms below are joined at the end of the build
        AMG_CHECK(hipEventRecord(sw.b, sw.cs));
        rt_pending = true;
    }
    if (l == 0 && A.has16 && (rc = build_col16<256>(ts, (int)nc, A.rrow.p, A.rcol.p, A.pnnz, A.r16, A.r16b)) != XFK_OK)
        return rc;
    if (l == 0 && A.has32 && (rc = to_f32(ts, (int)nc, A.rrow.p, A.pnnz, A.rval.p, A.r32)) != XFK_OK) return rc;
    if (l == 0 && A.has32 && A.dist &&   // the sharded level 0 prolongs through P itself (no fold)
        ((rc = to_f32(ts, n, A.prow.p, A.pnnz, A.pval.p, A.p32)) != XFK_OK ||
         (rc = build_col16<256>(ts, n, A.prow.p, A.pcol.p, A.pnnz, A.p16, A.p16b)) != XFK_OK))
        return rc;
    if (g_prof) g_prof->end();
    return XFK_OK;
}

// joins of the MIS-2 roots' neighbourhoods (agg), then P = (I - omega D_F^-1 A_F) P_tent
int Amg::joins_and_p_impl(hipStream_t s, int l)
{
    AmgLevel &A = *L[l];
    const int n = A.n;
    const ColView cv{A.col, A.has16 ? A.a16.p : nullptr, A.has16 ? A.a16b.p : nullptr};
    const std::string lv = g_prof ? "setup L" + std::to_string(l) + " " : std::string();
    AMG_CHECK(agg1.alloc(n));
    AMG_CHECK(agg.alloc(n));
    // lanes per row for the joins (XFK_JOIN_LANES: 1 = one thread per row)
    const int jg = join_lanes((double)A.nnz / std::max(1, n));
    auto joins = [&](auto g) {
        constexpr int G = decltype(g)::value;
        const int blocks = nb((long long)n * G);
        k_agg_join1<G><<<blocks, kB, 0, s>>>(n, A.rowptr, cv, sflag.p, key.p, cursor.p, agg1.p);
        k_agg_join2<G><<<blocks, kB, 0, s>>>(n, A.rowptr, cv, sflag.p, key.p, agg1.p, agg.p);
        k_agg_join3<G><<<blocks, kB, 0, s>>>(n, A.ncol_lim, A.rowptr, cv, A.val, agg.p, agg1.p);
    };
    if (jg == 8) joins(std::integral_constant<int, 8>{});
    else if (jg == 4) joins(std::integral_constant<int, 4>{});
    else joins(std::integral_constant<int, 1>{});
    std::swap(agg.p, agg1.p);   // agg = the joined map
    std::swap(agg.n, agg1.n);
    if (g_prof) g_prof->end();
    if (env_set("XFK_AMG_DEBUG")) {
        DBuf<int> d;
        AMG_CHECK(d.alloc(3));
        AMG_CHECK(hipMemsetAsync(d.p, 0, 3 * sizeof(int), s));
        k_debug_unagg<<<nb(n), kB, 0, s>>>(n, A.rowptr, A.col, cnt.p, agg.p, d.p);
        int h[3];
        unsigned long long r2[2];
        AMG_CHECK(hipMemcpyAsync(h, d.p, sizeof(h), hipMemcpyDeviceToHost, s));
        AMG_CHECK(hipMemcpyAsync(r2, rho.p + 2 * l, sizeof(r2), hipMemcpyDeviceToHost, s));
        AMG_CHECK(hipStreamSynchronize(s));
        double ra, rf;
        std::memcpy(&ra, &r2[0], 8);
        std::memcpy(&rf, &r2[1], 8);
        std::fprintf(stderr, "[amg] rank %d level %d n %d nnz %lld nc %lld unaggregated: strong %d weak-only %d isolated %d "
                     "rhoA/omega %.4g rhoF %.4g mis_rounds %d\n", dist ? rank : 0, l, n, A.nnz, (long long)host_int[8], h[0], h[1],
                     h[2], ra, rf, host_int[10]);
    }
    // P = (I - omega D_F^-1 A_F) P_tent
    SgX XS{A.rowptr, A.col, A.val, A.ncol_lim, sflag.p, dfinv.p, wF.p, cv.c16, cv.cbase};
    SgY YT{nullptr, nullptr, nullptr, agg.p};
    if (g_prof) g_prof->begin(lv + "P = (I - w D^-1 A) P_tent, R = P^T", 0.0);
    // (a sharded level needs P's length on the host at once -- the halo rows'
    // plan -- so it takes its capacity hint without deferring the length)
    return spgemm<true>(*this, s, n, XS, YT, A.prow, A.pcol, A.pval, A.pnnz, 4 * l, !A.dist);
}

// the V-cycle's per-level vectors
int Amg::alloc_vectors()
{
    for (int k = 0; k < nlev; ++k) {
        AmgLevel &A = *L[k];
        const size_t nv = (size_t)std::max(1, std::max(A.n, A.ncol_smooth));
        AMG_CHECK(A.xa.alloc(nv));
        AMG_CHECK(A.xb.alloc(nv));
        AMG_CHECK(A.r.alloc((size_t)std::max(1, A.n)));
        if (k > 0) AMG_CHECK(A.b.alloc((size_t)std::max(1, A.n)));
    }
    return XFK_OK;
}

// levels l0.. of the hierarchy (L[l0] set up by the caller), then the
// smoother vectors and the dense coarsest inverse
int Amg::build(hipStream_t s, int l0)
{
    int l = l0;
    for (;; ++l) {
        AmgLevel &A = *L[l];
        const int n = A.n;
        stats.n[l] = n;
        stats.nnz[l] = A.nnz;
        A.nc = 0;
        AMG_CHECK(A.dinv.alloc(n));
        AMG_CHECK(absd.alloc(n));
        AMG_CHECK(dfinv.alloc(n));
        AMG_CHECK(wF.alloc(n));
        AMG_CHECK(cnt.alloc((size_t)n + 1));
        const std::string lv = g_prof ? "setup L" + std::to_string(l) + " " : std::string();
        if (g_prof) g_prof->begin(lv + "diagonal, strength, rho", 0.0);
        k_amg_diag<<<nb(n), kB, 0, s>>>(n, A.rowptr, A.col, A.val, absd.p, A.dinv.p);
        if (n <= dense_max) {
            if (g_prof) g_prof->end();
            dense_coarse = true;
            break;
        }
        // level 0 (single device): 16-bit tile columns of A for the SpMV and
        // the sweeps, built off the critical path (they are read from the
        // first V-cycle on, after the join at the end of the build)
        A.has16 = l == 0 && !A.dist && !dist && col16 != 0;
        A.has32 = A.has16 && prec32 != 0;
        if (A.has16) {   // (on the main stream: the aggregation reads them too)
            int rc0 = build_col16<kCgBlock>(s, n, A.rowptr, A.col, A.nnz, A.a16, A.a16b);
            if (rc0 != XFK_OK) return rc0;
        }
        AMG_CHECK(sflag.alloc((size_t)A.nnz));
        AMG_CHECK(rho_part.alloc(2 * (size_t)nb_str(n)));
        k_amg_strength<<<nb_str(n), kB, 0, s>>>(n, A.ncol_lim, theta_at(l), A.rowptr,
                                                ColView{A.col, A.has16 ? A.a16.p : nullptr, A.has16 ? A.a16b.p : nullptr},
                                                A.val, absd.p, A.dinv.p, sflag.p, cnt.p,
                                                dfinv.p, wF.p, rho_part.p);
        k_max_reduce<<<1, kMaxReduceT, 0, s>>>(nb_str(n), rho_part.p, omega, rho.p + 2 * l);
        if (g_prof) g_prof->end();
        if (trace) {   // (the P SpGEMM below reuses cnt)
            int rct = trace_strength(s, l);
            if (rct != XFK_OK) return rct;
        }
        if (l == kAmgMaxLevels - 1) break;   // smoother-only coarsest level
        long long nc = 0;
        int rc = aggregate(s, l, nc, true);
        if (rc != XFK_OK) return rc;
        if (nc == 0) break;
        if (trace && (rc = trace_aggregates(s, l)) != XFK_OK) return rc;
        // AP = A P, then A_c = R (A P)
        SgX XA{A.rowptr, A.col, A.val, A.ncol_lim, nullptr, nullptr, nullptr, A.has16 ? A.a16.p : nullptr,
               A.has16 ? A.a16b.p : nullptr};
        SgY YP{A.prow.p, A.pcol.p, A.pval.p, nullptr};
        if (fold_pending) {   // the previous level's folded transfer still reads A P's buffers
            AMG_CHECK(hipStreamWaitEvent(s, sw.c, 0));
            fold_pending = false;
        }
        if (g_prof) g_prof->begin(lv + "SpGEMM A P", 0.0);
        // A P's row pointers go straight to the level (they are P~'s when it
        // folds): no copy before the next level reuses the A P buffers
        // packed sort words (level 0: 164 -> 134 us and 135 -> 98 us on configs[2])
        const bool pack = !A.dist && nc < kPackMaxCol && spgemm_pack_on();
        XA.pack = pack;
        rc = spgemm<false>(*this, s, n, XA, YP, A.ftrow, ap_col, ap_val, ap_nnz, 4 * l + 1);
        if (g_prof) g_prof->end();
        if (rc != XFK_OK) return rc;
        if ((int)L.size() <= l + 1) L.emplace_back(new AmgLevel());
        AmgLevel &C = *L[l + 1];
        SgX XR{A.rrow.p, A.rcol.p, A.rval.p, INT_MAX, nullptr, nullptr, nullptr};
        XR.pack = pack;
        SgY YAP{A.ftrow.p, ap_col.p, ap_val.p, nullptr};
        if (rt_pending) {   // R = P^T from the side stream
            AMG_CHECK(hipStreamWaitEvent(s, sw.b, 0));
            rt_pending = false;
        }
        if (g_prof) g_prof->begin(lv + "SpGEMM R (A P)", 0.0);
        rc = spgemm<false>(*this, s, (int)nc, XR, YAP, C.rowptr_o, C.col_o, C.val_o, C.nnz, 4 * l + 2);
        if (g_prof) g_prof->end();
        if (rc != XFK_OK) return rc;
        // folded level (l >= 1): P~ from A P before the next level reuses its buffers
        A.fold = fold_on != 0 && sweeps == 1 && !A.dist;
        A.fold_formed = A.fold;
        if (A.fold) {
            if (g_prof) g_prof->begin(lv + "folded transfer P~ = (I - w D^-1 A) P, R~ = P~^T", 0.0);
            A.fnnz = ap_nnz;   // an upper bound while the A P length is deferred
            AMG_CHECK(A.ftrow.alloc((size_t)n + 1));
            AMG_CHECK(A.ftcol.alloc((size_t)std::max(1LL, ap_nnz)));
            AMG_CHECK(A.ftval.alloc((size_t)std::max(1LL, ap_nnz)));
            if (l > 0) {
                AMG_CHECK(A.frrow.alloc((size_t)nc + 1));
                AMG_CHECK(A.frcol.alloc((size_t)std::max(1LL, ap_nnz)));
                AMG_CHECK(A.frval.alloc((size_t)std::max(1LL, ap_nnz)));
            }
            // P~ and R~ on the side stream: only the V-cycle reads them; the
            // next level's A P (which reuses A P's buffers) waits for P~
            if ((rc = sw.init()) != XFK_OK) return rc;
            AMG_CHECK(hipEventRecord(sw.a, s));
            AMG_CHECK(hipStreamWaitEvent(sw.cs, sw.a, 0));
            hipStream_t fs = sw.cs;
            sw_used = true;
            if (n > 0)
                k_fold_p<<<(int)(((long long)n * kFoldLanes + 255) / 256), 256, 0, fs>>>(
                    n, rho.p + 2 * l, A.dinv.p, A.ftrow.p, ap_col.p, ap_val.p, A.prow.p, A.pcol.p, A.pval.p, A.ftcol.p,
                    A.ftval.p);
            if (l == 0 && A.has16 &&
                (rc = build_col16<kCgBlock>(fs, n, A.ftrow.p, A.ftcol.p, ap_nnz, A.f16, A.f16b)) != XFK_OK)
                return rc;
            if (l == 0 && A.has32 && (rc = to_f32(fs, n, A.ftrow.p, ap_nnz, A.ftval.p, A.f32v)) != XFK_OK) return rc;
            AMG_CHECK(hipEventRecord(sw.c, sw.cs));
            fold_pending = true;
            // level 0 folds only its post-step (its pre-step keeps R r'): no R~
            if (l > 0)
                rc = transpose_csr(cnt2, cub_tmp2, fs, n, (int)nc, A.ftrow.p, A.ftcol.p, A.ftval.p, A.frrow.p,
                                   A.frcol.p, A.frval.p);
            if (rc != XFK_OK) return rc;
            // the exact length picks the V-cycle's lanes per row (and so the
            // summation order): from a deferred slot when A P's length is
            // deferred too, so hinted and measured setups agree bit for bit
            if (def_n > 0 && def_n + 2 <= kAmgDeferSlots) {
                AMG_CHECK(hipMemcpyAsync(def_dev.p + def_n + 1, A.ftrow.p + n, sizeof(int), hipMemcpyDeviceToDevice, s));
                def_target[def_n / 2] = &A.fnnz;
                def_n += 2;
            } else if (def_n > 0) {
                int len = 0;
                AMG_CHECK(hipMemcpyAsync(&len, A.ftrow.p + n, sizeof(int), hipMemcpyDeviceToHost, s));
                AMG_CHECK(hipStreamSynchronize(s));
                A.fnnz = len;
            }
            if (g_prof) g_prof->end();
        }
        C.n = (int)nc;
        C.ncol_lim = (int)nc;
        C.ncol_smooth = (int)nc;
        C.rowptr = C.rowptr_o.p;
        C.col = C.col_o.p;
        C.val = C.val_o.p;
    }
    nlev = l + 1;
    {
        // the SpGEMM lengths taken without a host check (capacity hints); an
        // overflow means a hint was too small: rebuild with measured capacities.
        // The dense coarsest inverse needs the nested-dissection plan, which
        // the host makes from the coarsest pattern; when the pattern equals
        // the one the cached plan was made for (compared on the device, read
        // with the deferred lengths), the inverse launched ahead of that read
        // stands -- otherwise (or on overflow) it is redone
        AmgLevel &C = *L[nlev - 1];
        const bool nd_spec = dense_coarse && !g_prof && def_n > 0 && nlev - 1 > l0 &&
                             C.n >= 8 * kBj && nd_key_n == C.n && C.col == C.col_o.p &&
                             (size_t)nd_key_nnz <= C.col_o.n && !env_set("XFK_NO_ND");
        if (nd_spec) {
            AMG_CHECK(mis_out.alloc(4));
            AMG_CHECK(hipMemsetAsync(mis_out.p + 3, 0, sizeof(int), s));
            const int nt = (int)std::max((long long)C.n + 1, nd_key_nnz);
            k_pattern_diff<<<nb(nt), kB, 0, s>>>(C.n, C.rowptr, C.col, nd_key_dev.p, (int)nd_key_nnz, mis_out.p + 3);
            AMG_CHECK(hipMemcpyAsync(host_int + 11, mis_out.p + 3, sizeof(int), hipMemcpyDeviceToHost, s));
        }
        int rc = fetch_deferred(s);
        if (rc != XFK_OK) return rc;
        if (nd_spec) {
            rc = alloc_vectors();
            if (rc != XFK_OK) return rc;
            nd_phases = nd_phases_key;
            if ((rc = dense_inverse(s, C, nd_ld)) != XFK_OK) return rc;
        }
        bool overflow = false;
        rc = wait_deferred(s, overflow);
        if (rc != XFK_OK) return rc;
        if (overflow) {
            if (sw_used) {   // nothing of this attempt may still run on the side stream
                AMG_CHECK(hipStreamSynchronize(sw.cs));
                sw_used = rt_pending = fold_pending = false;
            }
            cap_hint.clear();
            return build(s, l0);
        }
        for (int k = l0; k < nlev; ++k) stats.nnz[k] = L[k]->nnz;
        if (env_set("XFK_AMG_HINTS_PRINT")) {   // lab: the capacities / MIS rounds a setup measured
            std::fprintf(stderr, "[amg hints] levels %d:", nlev);
            for (auto &h : cap_hint) std::fprintf(stderr, " cap[%d.%d]=%d", h.first / 4, h.first % 4, h.second);
            for (auto &h : mis_hint) std::fprintf(stderr, " mis[%d]=%d", h.first, h.second);
            for (int k = 0; k < nlev; ++k) std::fprintf(stderr, " n%d=%d/%lld", k, L[k]->n, L[k]->nnz);
            std::fprintf(stderr, "\n");
        }
        stats.levels = nlev;
        double tot = 0;
        for (int k = 0; k < nlev; ++k) tot += (double)stats.nnz[k];
        stats.op_complexity = stats.nnz[0] > 0 ? tot / (double)stats.nnz[0] : 0.0;
        rc = alloc_vectors();
        if (rc != XFK_OK) return rc;
        if (dense_coarse && !(nd_spec && host_int[11] == 0)) {
            if (g_prof) g_prof->begin("setup L" + std::to_string(nlev - 1) + " dense inverse (blocked Gauss-Jordan)", 0.0);
            int ld = 0;
            if ((rc = nd_order(s, C, ld)) != XFK_OK) return rc;
            if ((rc = dense_inverse(s, C, ld)) != XFK_OK) return rc;
            if (g_prof) g_prof->end();
        }
    }
    if (sw_used) {   // the V-cycle reads R, P~, R~: join the side stream (after the dense inverse's launches)
        // by the time the host gets here (after the deferred read) the side
        // stream has usually drained: its work is complete and visible, and
        // the cross-stream wait -- ~15 us of barrier packet on the main
        // queue between the dense inverse and the PCG -- is skipped
        const hipError_t q = hipStreamQuery(sw.cs);
        if (q == hipErrorNotReady) {
            AMG_CHECK(hipEventRecord(sw.b, sw.cs));
            AMG_CHECK(hipStreamWaitEvent(s, sw.b, 0));
        } else {
            AMG_CHECK(q);
        }
        sw_used = rt_pending = fold_pending = false;
    }
    AMG_CHECK(hipGetLastError());   // no host check: nothing on the host waits for the device here
    return XFK_OK;
}


// ---------------------------------------------------------------------------
// sharded level 0
// ---------------------------------------------------------------------------

namespace {

// every rank's k doubles -> host (rank-major); collective
int gather_host(Amg &M, xfk_comm *comm, hipStream_t s, const double *vals, int k, std::vector<double> &out)
{
    DBuf<double> d;
    AMG_CHECK(d.alloc((size_t)k * (comm->size + 1)));
    AMG_CHECK(hipMemcpyAsync(d.p, vals, sizeof(double) * k, hipMemcpyHostToDevice, s));
    int rc = comm->allgather(d.p, d.p + k, (size_t)k, s);
    if (rc != XFK_OK) return rc;
    out.assign((size_t)k * comm->size, 0.0);
    AMG_CHECK(hipMemcpyAsync(out.data(), d.p + k, sizeof(double) * k * comm->size, hipMemcpyDeviceToHost, s));
    AMG_CHECK(hipStreamSynchronize(s));
    (void)M;
    return XFK_OK;
}

}  // namespace

// a folded sharded level 0: P~ in f32 with 16-bit columns in the V-cycle's
// 512-row tiles (a tile reaching the halo columns may keep the int columns,
// decided per tile), as the single-device level 0's
int Amg::fold_dist_tiles(hipStream_t s, int l)
{
    AmgLevel &A = *L[l];
    if (!A.fold || l != 0) return XFK_OK;
    int rc = XFK_OK;
    if (A.has16 && (rc = build_col16<kCgBlock>(s, A.n, A.ftrow.p, A.ftcol.p, A.fnnz, A.f16, A.f16b)) != XFK_OK)
        return rc;
    if (A.has32 && (rc = to_f32(s, A.n, A.ftrow.p, A.fnnz, A.ftval.p, A.f32v)) != XFK_OK) return rc;
    return XFK_OK;
}

int Amg::setup_dist(hipStream_t s, xfk_comm *comm_, const HaloPlan &halo_, int n, int nh, const int *rowptr,
                    const int *col, const double *val, long long nnz)
{
    dist = true;
    comm = comm_;
    overlap = overlap_enabled();
    nranks = comm->size;
    rank = comm->rank;
    int rc = init(s);
    if (rc != XFK_OK) return rc;
    {
        AmgLevel &A = *L[0];
        A.n = n;
        A.nnz = nnz;
        A.ncol_lim = n;            // aggregation and P: the owned block
        A.ncol_smooth = n + nh;    // smoother and residual: the full rows
        A.rowptr = rowptr;
        A.col = col;
        A.val = val;
        A.dist = true;
        A.plan = halo_;
        // 16-bit tile columns of the owned rows (the overlapped PCG SpMV and the
        // level-0 sweeps read them; a boundary tile reaching the halo ids spans
        // more than 65535 columns and keeps the int columns, decided per tile)
        A.has16 = col16 != 0;
        if (A.has16 && (rc = build_col16<kCgBlock>(s, n, rowptr, col, nnz, A.a16, A.a16b)) != XFK_OK) return rc;
        // f32 restriction / prolongation (converted after the aggregation)
        A.has32 = A.has16 && prec32 != 0;
    }
    for (int l = 0;; ++l) {
        AmgLevel &A = *L[l];
        const int nl = A.n;
        stats.n[l] = nl;
        stats.nnz[l] = A.nnz;
        AMG_CHECK(A.dinv.alloc(std::max(1, nl)));
        AMG_CHECK(absd.alloc(std::max(1, nl)));
        AMG_CHECK(dfinv.alloc(std::max(1, nl)));
        AMG_CHECK(wF.alloc(std::max(1, nl)));
        AMG_CHECK(cnt.alloc((size_t)nl + 1));
        AMG_CHECK(sflag.alloc((size_t)std::max(1LL, A.nnz)));
        AMG_CHECK(rho_part.alloc(2 * (size_t)std::max(1, nb_str(nl))));
        k_amg_diag<<<nb(nl), kB, 0, s>>>(nl, A.rowptr, A.col, A.val, absd.p, A.dinv.p);
        k_amg_strength<<<nb_str(nl), kB, 0, s>>>(nl, nl, theta_at(l), A.rowptr, ColView{A.col, nullptr, nullptr}, A.val,
                                                 absd.p, A.dinv.p, sflag.p, cnt.p, dfinv.p, wF.p, rho_part.p);
        k_max_reduce<<<1, kMaxReduceT, 0, s>>>(nb_str(nl), rho_part.p, omega, rho.p + 2 * l);
        long long nc = 0;
        rc = aggregate(s, l, nc, false);
        if (rc != XFK_OK && rc != XFK_ERR_UNSUPPORTED) return rc;
        // test hook: this rank reports an aggregation failure at level 0, so
        // every rank must agree on the Jacobi fallback through the collectives
        if (l == 0 && env_int("XFK_TEST_AMG_FAIL_RANK", -1) == rank) rc = XFK_ERR_UNSUPPORTED;
        bool rep = false;
        if ((rc = galerkin_dist(s, l, rc == XFK_OK ? 0 : 1, rep)) != XFK_OK) return rc;
        if (rep) {
            lrep = l + 1;
            const int te = tail_begin(s, 1);
            rc = build(s, l + 1);
            tail_end(s, te);
            return rc;
        }
    }
}

namespace {

// per peer: the smallest and largest of its ids this rank's columns reference
// (reduced per workgroup in LDS first: the entries of one peer all hit the
// same two words, and one global atomic per entry serialised ~150 us per call
// at configs[4] / 8 ranks)
constexpr int kSpanRanks = 64;
__global__ void __launch_bounds__(kB) k_peer_span(long long nnz, const int *__restrict__ col, int own0, int own1,
                                                  const int *__restrict__ c0, int nranks, int *lo, int *hi)
{
    __shared__ int slo[kSpanRanks], shi[kSpanRanks];
    for (int q = threadIdx.x; q < kSpanRanks; q += blockDim.x) {
        slo[q] = INT_MAX;
        shi[q] = -1;
    }
    __syncthreads();
    const long long e = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    if (e < nnz) {
        const int J = col[e];
        if (J < own0 || J >= own1) {
            int q = 0;
            while (c0[q + 1] <= J) ++q;
            atomicMin(&slo[q], J);
            atomicMax(&shi[q], J);
        }
    }
    __syncthreads();
    for (int q = threadIdx.x; q < nranks; q += blockDim.x)
        if (shi[q] >= 0) {
            atomicMin(&lo[q], slo[q]);
            atomicMax(&hi[q], shi[q]);
        }
}
// global ids -> local: own rows first, then the peers' spans in peer order
__global__ void k_localize(long long nnz, int *__restrict__ col, int own0, int own1, int n,
                           const int *__restrict__ c0, int nranks, const int *__restrict__ lo,
                           const int *__restrict__ off)
{
    const long long e = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    if (e >= nnz) return;
    const int J = col[e];
    if (J >= own0 && J < own1) {
        col[e] = J - own0;
        return;
    }
    int q = 0;
    while (c0[q + 1] <= J) ++q;
    col[e] = n + off[q] + (J - lo[q]);
}
__global__ void k_fill_int(int n, int *a, int v)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) a[i] = v;
}

}  // namespace

// A_{l+1} = R (A P_ext) on every rank for its own aggregates (P_ext: P plus
// the peers' P rows of the halo nodes, global coarse ids).  The result either
// stays sharded (own rows, halo spans and an exchange plan built here) or, once
// the global level has <= rep_rows rows, is all-gathered into the replicated
// level l+1 (rep = true).  st: this rank's status so far -- every rank makes
// the same collective calls whatever its status.
int Amg::galerkin_dist(hipStream_t s, int l, int st, bool &rep)
{
    AmgLevel &A = *L[l];
    const int n = A.n, nh = A.ncol_smooth - A.n;
    const int nc = st ? 0 : A.nc;
    std::vector<double> all;
    if (nranks > kSpanRanks) {   // (same on every rank)
        set_error("AMG: a sharded hierarchy of more than 64 ranks");
        return XFK_ERR_UNSUPPORTED;
    }
    // 1. aggregate counts and status of every rank
    {
        const double mine[2] = {(double)nc, (double)st};
        int rc = gather_host(*this, comm, s, mine, 2, all);
        if (rc != XFK_OK) return rc;
    }
    std::vector<int> cn(nranks + 1, 0);
    int cmax = 1, cmin = INT_MAX;
    bool fail = false;
    for (int q = 0; q < nranks; ++q) {
        cn[q + 1] = cn[q] + (int)all[2 * q];
        cmax = std::max(cmax, (int)all[2 * q]);
        cmin = std::min(cmin, (int)all[2 * q]);
        fail |= all[2 * q + 1] != 0.0;
    }
    const int NC = cn[nranks];
    if (fail || NC == 0) {
        set_error("AMG: a rank could not aggregate its rows");
        return XFK_ERR_UNSUPPORTED;
    }
    // replicate small levels (and never leave a rank without rows)
    rep = NC <= rep_rows || cmin == 0 || l + 2 >= kAmgMaxLevels;
    AMG_CHECK(c0_dev.alloc(nranks + 1));
    AMG_CHECK(hipMemcpyAsync(c0_dev.p, cn.data(), sizeof(int) * (nranks + 1), hipMemcpyHostToDevice, s));
    // 2. P rows of the halo nodes: lengths through the level's plan, then the
    //    entries through a plan over the P arrays (a peer's rows for one halo
    //    range are one contiguous run of its P entries)
    const long long pnnz = A.pnnz;
    const int ncl = n + nh;
    AMG_CHECK(ebuf.alloc((size_t)std::max(1, ncl)));
    if (n > 0) k_row_len_d<<<nb(n), kB, 0, s>>>(n, A.prow.p, ebuf.p);
    int rc = comm->exchange(A.plan, ebuf.p, s);
    if (rc != XFK_OK) return rc;
    AMG_CHECK(cnt.alloc((size_t)std::max(n, nh) + 1));
    AMG_CHECK(flag.alloc((size_t)nh + 1));
    if (nh > 0) k_dbl2int<<<nb(nh), kB, 0, s>>>(nh, ebuf.p + n, cnt.p);
    // flag = halo row pointer (its total, the halo rows' P entries, read with
    // the ranges' pointers below: one host check)
    if ((rc = scan_only(*this, s, cnt.p, flag.p, nh)) != XFK_OK) return rc;
    AMG_CHECK(pe_row.alloc((size_t)ncl + 1));
    k_pe_row<<<nb(ncl + 1), kB, 0, s>>>(n, nh, pnnz, A.prow.p, flag.p, pe_row.p);
    const HaloPlan &hp = A.plan;
    const int nsr = (int)(hp.send.size() + hp.recv.size());
    if ((rc = host_ints(2 * nsr + 1)) != XFK_OK) return rc;
    long long nhe = 0;
    {
        int k = 0;
        for (const HaloRange &t : hp.send) {
            AMG_CHECK(hipMemcpyAsync(host_big + k++, A.prow.p + t.off, sizeof(int), hipMemcpyDeviceToHost, s));
            AMG_CHECK(hipMemcpyAsync(host_big + k++, A.prow.p + t.off + t.len, sizeof(int), hipMemcpyDeviceToHost, s));
        }
        for (const HaloRange &r : hp.recv) {
            AMG_CHECK(hipMemcpyAsync(host_big + k++, flag.p + (r.off - n), sizeof(int), hipMemcpyDeviceToHost, s));
            AMG_CHECK(hipMemcpyAsync(host_big + k++, flag.p + (r.off - n) + r.len, sizeof(int),
                                     hipMemcpyDeviceToHost, s));
        }
        AMG_CHECK(hipMemcpyAsync(host_big + k, flag.p + nh, sizeof(int), hipMemcpyDeviceToHost, s));
        AMG_CHECK(hipStreamSynchronize(s));
        nhe = host_big[k];
    }
    HaloPlan ep;
    {
        int k = 0;
        for (const HaloRange &t : hp.send) {
            const int b0 = host_big[k++], b1 = host_big[k++];
            ep.send.push_back(HaloRange{t.peer, b0, b1 - b0, t.g0});
        }
        for (const HaloRange &r : hp.recv) {
            const int b0 = host_big[k++], b1 = host_big[k++];
            ep.recv.push_back(HaloRange{r.peer, (int)pnnz + b0, b1 - b0, r.g0});
        }
    }
    const size_t ne = (size_t)std::max(1LL, pnnz + nhe);
    AMG_CHECK(pe_val.alloc(ne));
    if (pnnz > 0)
        AMG_CHECK(hipMemcpyAsync(pe_val.p, A.pval.p, sizeof(double) * pnnz, hipMemcpyDeviceToDevice, s));
    if ((rc = comm->exchange(ep, pe_val.p, s)) != XFK_OK) return rc;
    // columns in global coarse ids (A.pcol itself stays rank-local: the
    // prolongation reads the own aggregates only)
    AMG_CHECK(pe_col.alloc(ne));
    if (pnnz > 0) {
        AMG_CHECK(hipMemcpyAsync(pe_col.p, A.pcol.p, sizeof(int) * pnnz, hipMemcpyDeviceToDevice, s));
        k_add_int<<<nb(pnnz), kB, 0, s>>>(pnnz, pe_col.p, cn[rank]);
    }
    AMG_CHECK(ebuf.alloc(ne));
    if (pnnz > 0) k_int2dbl<<<nb(pnnz), kB, 0, s>>>(pnnz, pe_col.p, ebuf.p);
    if ((rc = comm->exchange(ep, ebuf.p, s)) != XFK_OK) return rc;
    if (nhe > 0) k_dbl2int<<<nb(nhe), kB, 0, s>>>(nhe, ebuf.p + pnnz, pe_col.p + pnnz);
    // 3. AP over the full rows, then this rank's coarse rows R (AP)
    long long lnnz = 0, apnnz = 0;
    AMG_CHECK(l_row.alloc((size_t)cmax + 1));
    {
        SgX XA{A.rowptr, A.col, A.val, ncl, nullptr, nullptr, nullptr};
        SgY YP{pe_row.p, pe_col.p, pe_val.p, nullptr};
        // (the lengths are needed on the host at once: capacity hints of the
        // last setup, rank-local, taken without deferring -- one host check
        // per product instead of two)
        rc = spgemm<false>(*this, s, n, XA, YP, ap_row, ap_col, ap_val, apnnz, 4 * l + 1, false);
        if (rc == XFK_OK) {
            SgX XR{A.rrow.p, A.rcol.p, A.rval.p, INT_MAX, nullptr, nullptr, nullptr};
            SgY YAP{ap_row.p, ap_col.p, ap_val.p, nullptr};
            rc = spgemm<false>(*this, s, nc, XR, YAP, l_row, l_col, l_val, lnnz, 4 * l + 2, false);
        }
        if (rc != XFK_OK && rc != XFK_ERR_UNSUPPORTED) return rc;
    }
    // 4. folded post-step of this sharded level (V(1,1)): P~ = (I - w D^-1 A) P_ext
    //    over the pattern of A P_ext -- own rows, global coarse columns (the
    //    peers' aggregates next to the halo included); formed before the next
    //    level reuses A P's buffers.  The V-cycle's prolongation and post-sweep
    //    become one pass over P~ reading x_c with its coarse halo (a sharded
    //    next level: the columns are localised with its plan below; a
    //    replicated one: the global coarse vector every rank holds).
    const bool ok3 = rc == XFK_OK;
    A.fold = A.fold_formed =
        ok3 && sweeps == 1 && fold_on != 0;
    if (A.fold) {
        A.fnnz = apnnz;
        AMG_CHECK(A.ftrow.alloc((size_t)n + 1));
        AMG_CHECK(A.ftcol.alloc((size_t)std::max(1LL, apnnz)));
        AMG_CHECK(A.ftval.alloc((size_t)std::max(1LL, apnnz)));
        AMG_CHECK(hipMemcpyAsync(A.ftrow.p, ap_row.p, sizeof(int) * ((size_t)n + 1), hipMemcpyDeviceToDevice, s));
        if (n > 0)
            k_fold_p<<<(int)(((long long)n * kFoldLanes + 255) / 256), 256, 0, s>>>(
                n, rho.p + 2 * l, A.dinv.p, ap_row.p, ap_col.p, ap_val.p, pe_row.p, pe_col.p, pe_val.p, A.ftcol.p,
                A.ftval.p);
    }
    // 5. entry counts, status and -- the next level staying sharded -- the
    //    spans of the peers' aggregate ids this rank's A_{l+1} and P~ columns
    //    reference (what each peer must send): one all-gather, one host check
    const int own0 = cn[rank], own1 = cn[rank + 1];
    const int RW = 2 + 2 * nranks;   // per rank: lnnz, status, lo[nranks], hi[nranks]
    DBuf<double> recs;
    AMG_CHECK(recs.alloc((size_t)RW * (nranks + 1)));
    const double mine[2] = {(double)lnnz, ok3 ? 0.0 : 1.0};   // (read before the host check below)
    AMG_CHECK(hipMemcpyAsync(recs.p, mine, sizeof(mine), hipMemcpyHostToDevice, s));
    AMG_CHECK(span_dev.alloc(2 * (size_t)nranks));
    k_fill_int<<<1, 64, 0, s>>>(nranks, span_dev.p, INT_MAX);
    k_fill_int<<<1, 64, 0, s>>>(nranks, span_dev.p + nranks, -1);
    if (!rep && ok3) {
        if (lnnz > 0)
            k_peer_span<<<nb(lnnz), kB, 0, s>>>(lnnz, l_col.p, own0, own1, c0_dev.p, nranks, span_dev.p,
                                                 span_dev.p + nranks);
        if (A.fold && apnnz > 0)
            k_peer_span<<<nb(apnnz), kB, 0, s>>>(apnnz, A.ftcol.p, own0, own1, c0_dev.p, nranks, span_dev.p,
                                                  span_dev.p + nranks);
    }
    k_int2dbl<<<1, 256, 0, s>>>(2LL * nranks, span_dev.p, recs.p + 2);
    if ((rc = comm->allgather(recs.p, recs.p + RW, (size_t)RW, s)) != XFK_OK) return rc;
    all.assign((size_t)RW * nranks, 0.0);
    AMG_CHECK(hipMemcpyAsync(all.data(), recs.p + RW, sizeof(double) * RW * nranks, hipMemcpyDeviceToHost, s));
    AMG_CHECK(hipStreamSynchronize(s));
    std::vector<int> e0(nranks + 1, 0);
    long long nnzmax = 1;
    for (int q = 0; q < nranks; ++q) {
        e0[q + 1] = e0[q] + (int)all[(size_t)RW * q];
        nnzmax = std::max(nnzmax, (long long)all[(size_t)RW * q]);
        fail |= all[(size_t)RW * q + 1] != 0.0;
    }
    if (fail) {
        set_error("AMG: a SpGEMM row exceeds the LDS hash capacity");
        return XFK_ERR_UNSUPPORTED;
    }
    if ((int)L.size() <= l + 1) L.emplace_back(new AmgLevel());
    AmgLevel &C = *L[l + 1];
    if (!rep) {
        // 5a. stay sharded: own rows with local columns, halo spans per peer
        //     (what I need: my spans; what each peer needs from me: its spans
        //     of my ids)
        auto span_of = [&](int r, int q, bool hi) { return (int)all[(size_t)RW * r + 2 + (hi ? nranks : 0) + q]; };
        std::vector<int> span(2 * nranks);
        for (int q = 0; q < nranks; ++q) {
            span[q] = span_of(rank, q, false);
            span[nranks + q] = span_of(rank, q, true);
        }
        HaloPlan cp;
        std::vector<int> off(nranks, 0);
        int nhc = 0;
        for (int q = 0; q < nranks; ++q) {
            if (q == rank || span[q] > span[nranks + q]) continue;
            const int len = span[nranks + q] - span[q] + 1;
            off[q] = nhc;
            cp.recv.push_back(HaloRange{q, nc + nhc, len, span[q]});
            nhc += len;
        }
        for (int r = 0; r < nranks; ++r) {
            if (r == rank) continue;
            const int lo = span_of(r, rank, false), hi = span_of(r, rank, true);
            if (lo > hi) continue;
            cp.send.push_back(HaloRange{r, lo - own0, hi - lo + 1, lo});
        }
        AMG_CHECK(map_dev.alloc(nranks));
        AMG_CHECK(hipMemcpyAsync(map_dev.p, off.data(), sizeof(int) * nranks, hipMemcpyHostToDevice, s));
        AMG_CHECK(C.rowptr_o.alloc((size_t)nc + 1));
        AMG_CHECK(C.col_o.alloc((size_t)std::max(1LL, lnnz)));
        AMG_CHECK(C.val_o.alloc((size_t)std::max(1LL, lnnz)));
        AMG_CHECK(hipMemcpyAsync(C.rowptr_o.p, l_row.p, sizeof(int) * (nc + 1), hipMemcpyDeviceToDevice, s));
        if (lnnz > 0) {
            AMG_CHECK(hipMemcpyAsync(C.col_o.p, l_col.p, sizeof(int) * lnnz, hipMemcpyDeviceToDevice, s));
            AMG_CHECK(hipMemcpyAsync(C.val_o.p, l_val.p, sizeof(double) * lnnz, hipMemcpyDeviceToDevice, s));
            k_localize<<<nb(lnnz), kB, 0, s>>>(lnnz, C.col_o.p, own0, own1, nc, c0_dev.p, nranks, span_dev.p,
                                                map_dev.p);
        }
        if (A.fold && apnnz > 0)
            k_localize<<<nb(apnnz), kB, 0, s>>>(apnnz, A.ftcol.p, own0, own1, nc, c0_dev.p, nranks, span_dev.p,
                                                 map_dev.p);
        if ((rc = fold_dist_tiles(s, l)) != XFK_OK) return rc;
        C.n = nc;
        C.nnz = lnnz;
        C.ncol_lim = nc;
        C.ncol_smooth = nc + nhc;
        C.rowptr = C.rowptr_o.p;
        C.col = C.col_o.p;
        C.val = C.val_o.p;
        C.dist = true;
        C.plan = cp;
        AMG_CHECK(hipStreamSynchronize(s));
        return XFK_OK;
    }
    // 5b. all-gather the coarse rows (padded per rank) into the replicated level
    if ((rc = fold_dist_tiles(s, l)) != XFK_OK) return rc;
    c0 = cn;
    ncmax = cmax;
    AMG_CHECK(s_col.alloc((size_t)nnzmax));
    AMG_CHECK(s_val.alloc((size_t)nnzmax));
    if (lnnz > 0) {
        AMG_CHECK(hipMemcpyAsync(s_col.p, l_col.p, sizeof(int) * lnnz, hipMemcpyDeviceToDevice, s));
        AMG_CHECK(hipMemcpyAsync(s_val.p, l_val.p, sizeof(double) * lnnz, hipMemcpyDeviceToDevice, s));
    }
    AMG_CHECK(g_row.alloc((size_t)nranks * (ncmax + 1)));
    AMG_CHECK(g_col.alloc((size_t)nranks * nnzmax));
    AMG_CHECK(g_val.alloc((size_t)nranks * nnzmax));
    if ((rc = comm->allgather_bytes(l_row.p, g_row.p, sizeof(int) * (ncmax + 1), s)) != XFK_OK) return rc;
    if ((rc = comm->allgather_bytes(s_col.p, g_col.p, sizeof(int) * nnzmax, s)) != XFK_OK) return rc;
    if ((rc = comm->allgather(s_val.p, g_val.p, (size_t)nnzmax, s)) != XFK_OK) return rc;
    const long long NNZ = e0[nranks];
    AMG_CHECK(C.rowptr_o.alloc((size_t)NC + 1));
    AMG_CHECK(C.col_o.alloc((size_t)std::max(1LL, NNZ)));
    AMG_CHECK(C.val_o.alloc((size_t)std::max(1LL, NNZ)));
    AMG_CHECK(e0_dev.alloc(nranks + 1));
    AMG_CHECK(hipMemcpyAsync(e0_dev.p, e0.data(), sizeof(int) * (nranks + 1), hipMemcpyHostToDevice, s));
    k_concat_rowptr<<<nb(NC + 1), kB, 0, s>>>(NC, nranks, c0_dev.p, e0_dev.p, g_row.p, ncmax + 1, C.rowptr_o.p);
    for (int q = 0; q < nranks; ++q) {
        const long long cq = e0[q + 1] - e0[q];
        if (cq == 0) continue;
        AMG_CHECK(hipMemcpyAsync(C.col_o.p + e0[q], g_col.p + (size_t)q * nnzmax, sizeof(int) * cq,
                                 hipMemcpyDeviceToDevice, s));
        AMG_CHECK(hipMemcpyAsync(C.val_o.p + e0[q], g_val.p + (size_t)q * nnzmax, sizeof(double) * cq,
                                 hipMemcpyDeviceToDevice, s));
    }
    C.n = NC;
    C.nnz = NNZ;
    C.ncol_lim = NC;
    C.ncol_smooth = NC;
    C.rowptr = C.rowptr_o.p;
    C.col = C.col_o.p;
    C.val = C.val_o.p;
    C.dist = false;
    C.plan = HaloPlan();
    if (env_set("XFK_AMG_DEBUG") && rank == 0) {   // symmetry of the gathered A_1
        std::vector<int> hr(NC + 1), hc(NNZ);
        std::vector<double> hv(NNZ);
        AMG_CHECK(hipMemcpyAsync(hr.data(), C.rowptr, sizeof(int) * (NC + 1), hipMemcpyDeviceToHost, s));
        AMG_CHECK(hipMemcpyAsync(hc.data(), C.col, sizeof(int) * NNZ, hipMemcpyDeviceToHost, s));
        AMG_CHECK(hipMemcpyAsync(hv.data(), C.val, sizeof(double) * NNZ, hipMemcpyDeviceToHost, s));
        AMG_CHECK(hipStreamSynchronize(s));
        std::vector<std::pair<int, double>> row;
        std::vector<std::vector<std::pair<int, double>>> R(NC);
        double amax = 0, dmax = 0;
        long long missing = 0;
        for (int i = 0; i < NC; ++i) {
            for (int k = hr[i]; k < hr[i + 1]; ++k) R[i].push_back({hc[k], hv[k]});
            std::sort(R[i].begin(), R[i].end());
        }
        for (int i = 0; i < NC; ++i)
            for (auto &e : R[i]) {
                amax = std::max(amax, std::fabs(e.second));
                auto &Rj = R[e.first];
                auto it = std::lower_bound(Rj.begin(), Rj.end(), std::make_pair(i, -1e300));
                if (it == Rj.end() || it->first != i) {
                    ++missing;
                    dmax = std::max(dmax, std::fabs(e.second));
                } else {
                    dmax = std::max(dmax, std::fabs(e.second - it->second));
                }
            }
        std::fprintf(stderr, "[amg] A_1 %d rows %lld nnz: max|A - A^T| / max|A| = %.3e, %lld entries without a mirror\n",
                     NC, NNZ, dmax / amax, missing);
    }
    AMG_CHECK(cb_loc.alloc((size_t)ncmax));
    AMG_CHECK(cb_all.alloc((size_t)nranks * ncmax));
    return XFK_OK;
}

// XFK_AMG_REFOLD=0: a Newton refresh runs level 0 unfolded (the former way)
static bool refold_on()
{
    return env_int("XFK_AMG_REFOLD", 1) != 0;   // (read per refresh: tests toggle it)
}

static int refold_stage()
{
    return env_int("XFK_REFOLD_STAGE", 1) != 0;   // (read per refresh: tests toggle it)
}

int Amg::refresh(hipStream_t s, bool fold)
{
    AmgLevel &A = *L[0];
    const int n = A.n;
    // level 0's P~ belongs to the matrix it was formed from: re-formed below
    // for the new values (k_refold_p), or level 0 runs unfolded; a refresh
    // that unfolds keeps P~'s arrays, so a later one may fold again
    const bool refold = fold && A.fold_formed && !dist && refold_on() && A.fnnz > 0;
    A.fold = refold;
    AMG_CHECK(absd.alloc(std::max(1, n)));
    AMG_CHECK(rho_part.alloc(2 * (size_t)std::max(1, nb_str(n))));
    if (n > 0) {
        k_amg_rho<<<nb_str(n), kB, 0, s>>>(n, A.rowptr,
                                           ColView{A.col, A.has16 ? A.a16.p : nullptr, A.has16 ? A.a16b.p : nullptr},
                                           A.val, rho_part.p, absd.p, A.dinv.p);
        k_max_reduce<<<1, kMaxReduceT, 0, s>>>(nb_str(n), rho_part.p, omega, rho.p);
    }
    if (refold && n > 0) {   // P~ = (I - w D^-1 A_new) P over its own pattern (new D^-1 and rho above)
        if (A.has32) AMG_CHECK(A.f32v.alloc((size_t)std::max(1LL, A.fnnz)));   // (the setup's copy: same pattern)
        k_refold_p<<<(n + kRfRows - 1) / kRfRows, 256, 0, s>>>(n, rho.p, A.dinv.p, A.rowptr, A.col, A.val, A.prow.p,
                                                                A.pcol.p, A.pval.p, A.ftrow.p, A.ftcol.p, A.ftval.p,
                                                                A.has32 ? A.f32v.p : nullptr, refold_stage());
    }
    AMG_CHECK(hipGetLastError());
    return XFK_OK;
}

// ---------------------------------------------------------------------------
// diagnostics (xfk_amg_probe_*): the setup trace and copies of the hierarchy
// ---------------------------------------------------------------------------

namespace {

template <class T>
int fetch(hipStream_t s, std::vector<T> &h, const T *d, size_t n)
{
    h.resize(n);
    if (n > 0) AMG_CHECK(hipMemcpyAsync(h.data(), d, sizeof(T) * n, hipMemcpyDeviceToHost, s));
    AMG_CHECK(hipStreamSynchronize(s));
    return XFK_OK;
}

}  // namespace

// after k_amg_strength of level l (before the P SpGEMM reuses cnt)
int Amg::trace_strength(hipStream_t s, int l)
{
    const AmgLevel &A = *L[l];
    if ((int)trace->lev.size() <= l) trace->lev.resize((size_t)l + 1);
    AmgTrace::Level &T = trace->lev[l];
    T = AmgTrace::Level();
    T.n = A.n;
    std::vector<int> end;   // (a coarse level's nnz may still be a deferred bound)
    int rc = fetch(s, end, A.rowptr + A.n, 1);
    if (rc == XFK_OK) rc = fetch(s, T.sflag, (const unsigned char *)sflag.p, (size_t)end[0]);
    if (rc == XFK_OK) rc = fetch(s, T.sdeg, (const int *)cnt.p, (size_t)A.n);
    if (rc == XFK_OK) rc = fetch(s, T.dfinv, (const double *)dfinv.p, (size_t)A.n);
    if (rc == XFK_OK) rc = fetch(s, T.wF, (const double *)wF.p, (size_t)A.n);
    return rc;
}

// after the joins of level l: agg holds the joined map, agg1 the map before
// the weak join (k_agg_join3 read it), key the MIS-2 states
int Amg::trace_aggregates(hipStream_t s, int l)
{
    AmgTrace::Level &T = trace->lev[l];
    const size_t n = (size_t)L[l]->n;
    std::vector<MisKey> k;
    int rc = fetch(s, T.agg, (const int *)agg.p, n);
    if (rc == XFK_OK) rc = fetch(s, T.agg_pre, (const int *)agg1.p, n);
    if (rc == XFK_OK) rc = fetch(s, k, (const MisKey *)key.p, n);
    if (rc != XFK_OK) return rc;
    T.root.resize(n);
    for (size_t i = 0; i < n; ++i) T.root[i] = (k[i] >> 30) == kStIn;
    T.joined = true;
    return XFK_OK;
}

namespace {

struct ProbeView {
    int rows = 0, cols = 0;
    const int *rp = nullptr, *cl = nullptr;
    const double *v = nullptr;
    const unsigned short *c16 = nullptr;
    const int *cb = nullptr;
    int B = 0;                      // rows per 16-bit tile
    const float *v32 = nullptr;
};

int probe_view(Amg &M, int level, int sel, ProbeView &V)
{
    XFK_REQUIRE(!M.dist && level >= 0 && level < M.nlev, XFK_ERR_ARG, "AMG probe: no such level");
    const AmgLevel &A = *M.L[level];
    const int what = sel & 15;
    XFK_REQUIRE(what == XFK_AMG_A || (level < M.nlev - 1 && A.nc > 0), XFK_ERR_ARG,
                "AMG probe: the coarsest level has no transfer");
    V = ProbeView();
    switch (what) {
    case XFK_AMG_A:
        V.rows = V.cols = A.n;
        V.rp = A.rowptr, V.cl = A.col, V.v = A.val;
        if (A.has16) V.c16 = A.a16.p, V.cb = A.a16b.p, V.B = kCgBlock;
        break;
    case XFK_AMG_P:
        V.rows = A.n, V.cols = A.nc;
        V.rp = A.prow.p, V.cl = A.pcol.p, V.v = A.pval.p;
        break;
    case XFK_AMG_R:
        V.rows = A.nc, V.cols = A.n;
        V.rp = A.rrow.p, V.cl = A.rcol.p, V.v = A.rval.p;
        if (A.has16) V.c16 = A.r16.p, V.cb = A.r16b.p, V.B = 256;
        if (A.has32) V.v32 = A.r32.p;
        break;
    case XFK_AMG_PF:
        XFK_REQUIRE(A.fold_formed, XFK_ERR_ARG, "AMG probe: the level has no folded transfer");
        V.rows = A.n, V.cols = A.nc;
        V.rp = A.ftrow.p, V.cl = A.ftcol.p, V.v = A.ftval.p;
        if (A.has16) V.c16 = A.f16.p, V.cb = A.f16b.p, V.B = kCgBlock;
        if (A.has32) V.v32 = A.f32v.p;
        break;
    case XFK_AMG_RF:
        XFK_REQUIRE(A.fold_formed && level > 0, XFK_ERR_ARG, "AMG probe: the level has no folded restriction");
        V.rows = A.nc, V.cols = A.n;
        V.rp = A.frrow.p, V.cl = A.frcol.p, V.v = A.frval.p;
        break;
    default:
        set_error("AMG probe: unknown operator");
        return XFK_ERR_ARG;
    }
    return XFK_OK;
}

}  // namespace

int amg_probe_info(Amg &M, hipStream_t s, xfk_amg_info *info)
{
    *info = xfk_amg_info{};
    info->levels = M.nlev;
    info->dense_coarse = M.dense_coarse;
    info->cinv_f64 = M.cinv_f64;
    info->traced = M.trace != nullptr;
    std::vector<unsigned long long> r;
    int rc = fetch(s, r, (const unsigned long long *)M.rho.p, (size_t)2 * kAmgMaxLevels);
    if (rc != XFK_OK) return rc;
    for (int l = 0; l < M.nlev && l < 16; ++l) {
        const AmgLevel &A = *M.L[l];
        xfk_amg_level_info &I = info->level[l];
        const bool last = l == M.nlev - 1;
        I.n = A.n;
        I.nnz = A.nnz;
        I.nc = last ? 0 : A.nc;
        I.pnnz = last ? 0 : A.pnnz;
        I.fnnz = (last || !A.fold_formed) ? 0 : A.fnnz;
        I.fold = !last && A.fold;
        I.has16 = A.has16;
        I.has32 = A.has32;
        I.w_at = !last && M.w_at(l);
        double ra, rf;
        std::memcpy(&ra, &r[2 * l], 8);
        std::memcpy(&rf, &r[2 * l + 1], 8);
        I.weight = ra > 0.0 ? 1.0 / ra : 0.0;
        I.rho_f = rf;
    }
    return XFK_OK;
}

int amg_probe_level_size(Amg &M, hipStream_t s, int level, int sel, int *rows, int *cols, long long *nnz)
{
    ProbeView V;
    int rc = probe_view(M, level, sel, V);
    if (rc != XFK_OK) return rc;
    std::vector<int> end;
    if ((rc = fetch(s, end, V.rp + V.rows, 1)) != XFK_OK) return rc;
    *rows = V.rows;
    *cols = V.cols;
    *nnz = end[0];
    return XFK_OK;
}

int amg_probe_level_csr(Amg &M, hipStream_t s, int level, int sel, int *rowptr, int *col, double *val)
{
    ProbeView V;
    int rc = probe_view(M, level, sel, V);
    if (rc != XFK_OK) return rc;
    std::vector<int> rp, cl, cb;
    std::vector<double> v;
    if ((rc = fetch(s, rp, V.rp, (size_t)V.rows + 1)) != XFK_OK) return rc;
    const size_t nz = (size_t)rp[V.rows];
    if ((rc = fetch(s, cl, V.cl, nz)) != XFK_OK) return rc;
    if (V.c16 && !(sel & XFK_AMG_PLAIN_COLS)) {
        // the tile logic of ColView / cg_tile_spmv16: a tile with a base reads base + offset
        std::vector<unsigned short> c16;
        const int nt = (V.rows + V.B - 1) / V.B;
        if ((rc = fetch(s, c16, V.c16, nz)) != XFK_OK || (rc = fetch(s, cb, V.cb, (size_t)nt)) != XFK_OK) return rc;
        for (int t = 0; t < nt; ++t) {
            if (cb[t] == kNoColBase) continue;
            for (int k = rp[t * V.B]; k < rp[std::min(V.rows, (t + 1) * V.B)]; ++k) cl[k] = cb[t] + (int)c16[k];
        }
    }
    if (V.v32 && !(sel & XFK_AMG_F64_VALS)) {
        std::vector<float> f;
        if ((rc = fetch(s, f, V.v32, nz)) != XFK_OK) return rc;
        v.assign(f.begin(), f.end());
    } else if ((rc = fetch(s, v, V.v, nz)) != XFK_OK) {
        return rc;
    }
    std::copy(rp.begin(), rp.end(), rowptr);
    std::copy(cl.begin(), cl.end(), col);
    std::copy(v.begin(), v.end(), val);
    return XFK_OK;
}

int amg_probe_tiles(Amg &M, hipStream_t s, int sel, int *tiles, int *wide)
{
    ProbeView V;
    int rc = probe_view(M, 0, sel, V);
    if (rc != XFK_OK) return rc;
    *tiles = *wide = 0;
    if (!V.c16) return XFK_OK;
    std::vector<int> cb;
    const int nt = (V.rows + V.B - 1) / V.B;
    if ((rc = fetch(s, cb, V.cb, (size_t)nt)) != XFK_OK) return rc;
    *tiles = nt;
    for (int t = 0; t < nt; ++t) *wide += cb[t] == kNoColBase;
    return XFK_OK;
}

int amg_probe_vector(Amg &M, hipStream_t s, int level, int what, double *out)
{
    XFK_REQUIRE(!M.dist && level >= 0 && level < M.nlev, XFK_ERR_ARG, "AMG probe: no such level");
    const AmgLevel &A = *M.L[level];
    std::vector<double> v;
    int rc;
    if (what == XFK_AMG_DINV) {
        if ((rc = fetch(s, v, (const double *)A.dinv.p, (size_t)A.n)) != XFK_OK) return rc;
        std::copy(v.begin(), v.end(), out);
        return XFK_OK;
    }
    XFK_REQUIRE(what == XFK_AMG_DENSE && level == M.nlev - 1 && M.dense_coarse, XFK_ERR_ARG,
                "AMG probe: not the dense coarsest level");
    const size_t ld = (size_t)M.cinv_ld, n = (size_t)A.n;
    std::vector<double> sc;
    if ((rc = fetch(s, sc, (const double *)M.cinv_sc.p, ld)) != XFK_OK) return rc;
    if (M.cinv_f64) {
        if ((rc = fetch(s, v, (const double *)M.cinv_o64.p, ld * ld)) != XFK_OK) return rc;
    } else {
        std::vector<float> f;
        if ((rc = fetch(s, f, M.cinv_apply, ld * ld)) != XFK_OK) return rc;
        v.assign(f.begin(), f.end());
    }
    // k_dense_mv on a unit vector: x_i = S_i (M_ij (S_j 1))
    for (size_t i = 0; i < n; ++i)
        for (size_t j = 0; j < n; ++j) out[i * n + j] = sc[i] * (v[i * ld + j] * sc[j]);
    return XFK_OK;
}

int amg_probe_trace(Amg &M, int level, int what, void *out)
{
    XFK_REQUIRE(M.trace && level >= 0 && level < (int)M.trace->lev.size(), XFK_ERR_ARG,
                "AMG probe: the level was not traced");
    const AmgTrace::Level &T = M.trace->lev[level];
    auto put = [&](const auto &v) {
        if (!v.empty()) std::memcpy(out, v.data(), v.size() * sizeof(v[0]));
        return XFK_OK;
    };
    XFK_REQUIRE(T.joined || what == XFK_AMG_TR_SFLAG || what == XFK_AMG_TR_SDEG || what >= XFK_AMG_TR_DFINV,
                XFK_ERR_ARG, "AMG probe: the level was not coarsened");
    switch (what) {
    case XFK_AMG_TR_SFLAG: return put(T.sflag);
    case XFK_AMG_TR_SDEG: return put(T.sdeg);
    case XFK_AMG_TR_AGG: return put(T.agg);
    case XFK_AMG_TR_AGG_PRE: return put(T.agg_pre);
    case XFK_AMG_TR_ROOT: return put(T.root);
    case XFK_AMG_TR_DFINV: return put(T.dfinv);
    case XFK_AMG_TR_WF: return put(T.wF);
    default: set_error("AMG probe: unknown trace array"); return XFK_ERR_ARG;
    }
}

}  // namespace xfk

// xfk_device_init: loads this translation unit's code object onto the device
// (the first use of any of its kernels would otherwise do it inside a solve)
hipError_t xfk::warm_module_amg()
{
    hipFuncAttributes a;
    return hipFuncGetAttributes(&a, reinterpret_cast<const void *>(&k_max_reduce));
}
