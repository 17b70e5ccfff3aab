// The AMG setup's SpGEMM C = X Y (xfk_amg.h): the Galerkin products A P and
// R (A P) and the smoothed prolongator.  Kernels, capacity classes and the
// host driver; every sum runs in a fixed order (see the kernels).
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <climits>

#include "xfk_amg_impl.h"

namespace xfk {

namespace {

// --------------------------------------------------------------------------
// setup: row-merge SpGEMM C = X Y, one wavefront per row
// --------------------------------------------------------------------------
//
// Products of row r are enumerated in a fixed order (X entries in row order,
// each Y row in column order), 64 at a time: a wave prefix sum of the Y-row
// lengths of up to 64 X entries maps lane products to (X entry, Y position).
// Pass COUNT inserts the output columns into an LDS hash set and returns the
// row length; pass FILL inserts them again, ranks them (sorted columns) and
// accumulates each product into its column in enumeration order: within a
// group of 64 products, the first lane of each column sums the group's
// products of that column in lane order, then adds the group sum to the LDS
// accumulator -- the same operation order on every run.
//
// PMODE builds the smoothed prolongator P = S P_tent directly: X is the level
// matrix masked to its strong entries and diagonal, with values
// S = I - omega D_F^-1 A_F, and Y = P_tent is given by the aggregate map
// (row k = {agg[k] : 1}, empty when k is not aggregated).

constexpr int kSgMax = 512;        // distinct output columns per row (COUNT pass hash: 2 kSgMax slots)

constexpr int ilog2(int v) { return v <= 1 ? 0 : 1 + ilog2(v >> 1); }

// CAP: distinct columns a row may have (FILL is launched with the smallest
// CAP that covers the longest row the COUNT pass found, so typical levels run
// with a few KiB of LDS per wave and full occupancy); hash slots = 2 CAP.
template <bool FILL, bool PMODE, int CAP>
__global__ void __launch_bounds__(64) k_spgemm(int nrows, SgX X, SgY Y, int *__restrict__ cnt_out,
                                               const int *__restrict__ crow, int *__restrict__ ccol,
                                               double *__restrict__ cval, int *overflow)
{
    constexpr int kSgHash = 2 * CAP;
    constexpr int kHashShift = 32 - ilog2(kSgHash);
    __shared__ int hk[kSgHash];
    __shared__ int hr[FILL ? kSgHash : 1];
    __shared__ int lst[FILL ? CAP : 1], lslot[FILL ? CAP : 1];
    __shared__ double acc[FILL ? CAP : 1];
    __shared__ int c_off[64], c_ys[64];
    __shared__ double c_xv[64];
    __shared__ __attribute__((aligned(16))) int s_rank[64];
    __shared__ double s_val[64];
    __shared__ int s_cnt, s_ovf, s_m;

    const int row = blockIdx.x;
    const int lane = threadIdx.x;
    if (row >= nrows) return;
    for (int t = lane; t < kSgHash; t += 64) hk[t] = -1;
    if (lane == 0) {
        s_cnt = 0;
        s_ovf = 0;
        s_m = 0;
    }
    __syncthreads();
    const int xs = X.rowptr[row], xe = X.rowptr[row + 1];
    double omega = 0.0, dfi = 0.0;
    if (PMODE) {
        omega = X.wF[row];
        dfi = X.dfinv[row];
    }

    auto insert = [&](int key) {
        unsigned h = ((unsigned)key * 2654435761u) >> kHashShift;
        for (int probe = 0; probe < kSgHash; ++probe) {
            const int old = atomicCAS(&hk[h], -1, key);
            if (old == -1) {
                atomicAdd(&s_cnt, 1);
                return;
            }
            if (old == key) return;
            h = (h + 1) & (kSgHash - 1);
        }
        s_ovf = 1;
    };
    auto lookup = [&](int key) -> int {
        unsigned h = ((unsigned)key * 2654435761u) >> kHashShift;
        for (int probe = 0; probe < kSgHash; ++probe) {
            const int k = hk[h];
            if (k == key) return (int)h;
            if (k == -1) return -1;
            h = (h + 1) & (kSgHash - 1);
        }
        return -1;
    };
    // stage up to 64 X entries of [e0, xe); returns the group's product count
    auto stage = [&](int e0) -> int {
        const int e = e0 + lane;
        int len = 0, ys = 0;
        double xv = 0.0;
        if (e < xe) {
            const int k = X.col[e];
            if (k < X.col_lim) {
                if (PMODE) {
                    const unsigned char f = X.mask[e];
                    if (f != 0 && Y.agg[k] >= 0) {
                        ys = k;
                        len = 1;
                        xv = (f == 2) ? 1.0 - omega : -omega * dfi * X.val[e];
                    }
                } else {
                    ys = Y.rowptr[k];
                    len = Y.rowptr[k + 1] - ys;
                    xv = X.val[e];
                }
            }
        }
        int incl = len;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int t = __shfl_up(incl, off, 64);
            if (lane >= off) incl += t;
        }
        const int total = __shfl(incl, 63, 64);
        c_off[lane] = incl - len;
        c_ys[lane] = ys;
        c_xv[lane] = xv;
        __syncthreads();
        return total;
    };
    // product p of the staged group -> (column, value)
    auto product = [&](int p, int &key, double &v) {
        int lo = 0, hi = 63;   // largest staged entry with c_off <= p
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (c_off[mid] <= p) lo = mid;
            else hi = mid - 1;
        }
        if (PMODE) {
            key = Y.agg[c_ys[lo]];
            v = c_xv[lo];
        } else {
            const int q = c_ys[lo] + (p - c_off[lo]);
            key = Y.col[q];
            if (FILL) v = c_xv[lo] * Y.val[q];
        }
    };

    // pass 1: the set of output columns
    for (int e0 = xs; e0 < xe; e0 += 64) {
        const int total = stage(e0);
        for (int p = lane; p < total; p += 64) {
            int key;
            double v;
            product(p, key, v);
            insert(key);
        }
        __syncthreads();
    }
    if (!FILL) {
        if (lane == 0) {
            cnt_out[row] = s_cnt;
            if (s_ovf || s_cnt > CAP) atomicOr(overflow, 1);
        }
        return;
    }
    // rank the columns (sorted order) and map hash slot -> rank
    for (int t = lane; t < kSgHash; t += 64)
        if (hk[t] != -1) {
            const int m = atomicAdd(&s_m, 1);
            if (m < CAP) {
                lst[m] = hk[t];
                lslot[m] = t;
            }
        }
    __syncthreads();
    const int cnt = min(s_m, CAP);
    const int cb = crow[row];
    for (int m = lane; m < cnt; m += 64) {
        const int key = lst[m];
        int rank = 0;
        for (int q = 0; q < cnt; ++q) rank += lst[q] < key;
        hr[lslot[m]] = rank;
        ccol[cb + rank] = key;
        acc[rank] = 0.0;
    }
    __syncthreads();
    // pass 2: values in enumeration order
    const int4 *r4 = reinterpret_cast<const int4 *>(s_rank);
    for (int e0 = xs; e0 < xe; e0 += 64) {
        const int total = stage(e0);
        for (int p0 = 0; p0 < total; p0 += 64) {
            const int p = p0 + lane;
            int rank = -1;
            double v = 0.0;
            if (p < total) {
                int key;
                product(p, key, v);
                const int h = lookup(key);
                rank = (h >= 0) ? hr[h] : -1;
            }
            s_rank[lane] = rank;
            s_val[lane] = v;
            __syncthreads();
            if (rank >= 0) {
                bool leader = true;
                double sum = 0.0;
#pragma unroll
                for (int m4 = 0; m4 < 16; ++m4) {
                    const int4 q = r4[m4];
                    const int m = 4 * m4;
                    if (q.x == rank) { leader &= (m < lane) ? false : true; sum += s_val[m]; }
                    if (q.y == rank) { leader &= (m + 1 < lane) ? false : true; sum += s_val[m + 1]; }
                    if (q.z == rank) { leader &= (m + 2 < lane) ? false : true; sum += s_val[m + 2]; }
                    if (q.w == rank) { leader &= (m + 3 < lane) ? false : true; sum += s_val[m + 3]; }
                }
                if (leader) acc[rank] += sum;
            }
            __syncthreads();
        }
    }
    for (int m = lane; m < cnt; m += 64) cval[cb + m] = acc[m];
}

// Products per row (upper bound of the output row length), for the choice
// between the sub-wave and the wave-per-row SpGEMM.
template <bool PMODE>
__global__ void k_spgemm_nprod(int nrows, SgX X, SgY Y, int *__restrict__ nprod)
{
    const int row = blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= nrows) return;
    int c = 0;
    for (int e = X.rowptr[row]; e < X.rowptr[row + 1]; ++e) {
        const int k = X.col[e];
        if (k >= X.col_lim) continue;
        if (PMODE) c += (X.mask[e] != 0 && Y.agg[k] >= 0);
        else c += Y.rowptr[k + 1] - Y.rowptr[k];
    }
    nprod[row] = c;
}

// Sub-wave SpGEMM (the fine levels: A P, the prolongator, R (A P)): G lanes
// per row, 64 / G rows per wavefront.  Groups of one wavefront advance
// independently; their LDS regions are private, and LDS traffic inside a
// wavefront is ordered, so no workgroup barriers are needed (wave_barrier
// keeps the compiler from reordering).

__device__ __forceinline__ void wave_lds_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// w of lane (lane ^ LM), LM < 16: DPP moves inside the 16-lane row (no LDS
// pipe); LM = 16 through the shuffle
__device__ __forceinline__ unsigned xor_lanes(unsigned w, int lm)
{
    const int x = (int)w;
    switch (lm) {
    case 1: return (unsigned)__builtin_amdgcn_update_dpp(x, x, 0xB1, 0xF, 0xF, false);    // quad_perm:[1,0,3,2]
    case 2: return (unsigned)__builtin_amdgcn_update_dpp(x, x, 0x4E, 0xF, 0xF, false);    // quad_perm:[2,3,0,1]
    case 4: {
        const int t = __builtin_amdgcn_update_dpp(x, x, 0x104, 0xF, 0x5, false);          // row_shl:4 -> lanes 0-3, 8-11
        return (unsigned)__builtin_amdgcn_update_dpp(t, x, 0x114, 0xF, 0xA, false);       // row_shr:4 -> lanes 4-7, 12-15
    }
    case 8: return (unsigned)__builtin_amdgcn_update_dpp(x, x, 0x128, 0xF, 0xF, false);   // row_ror:8
    default: return (unsigned)__shfl_xor(x, lm, 64);
    }
}

// Sort-based single-pass SpGEMM for rows of at most CAP products: a group of
// G lanes per row (64 / G rows per wavefront).  Lane l expands X entries
// l, l + G, ... (its Y row) into the row's product list in LDS -- the fixed
// enumeration order -- then the list is loaded as CAP virtual slots, S = CAP / G
// consecutive slots per lane in registers, and sorted by column with a bitonic
// network (in-lane compare-exchanges for distances < S, shuffles across the
// group for the others).  A segmented inclusive scan then sums each column's
// products and counts the distinct columns; the last slot of each column
// writes it at its rank.  The network and the scan are fixed, so the sums
// are the same bits on every run.  Only the product list (12 B per product)
// lives in LDS: several times more rows in flight than the hash kernels.
// The wavefront's W rows are written back to back into its slab
// (blockIdx.x * W * CAP: the exclusive prefix of the W lengths, which the
// wavefront holds in registers, places each row) with the row lengths and
// the slab's length; k_spgemm_compact_slab moves each slab -- one dense run
// on both sides -- to its CSR place after the length scan.  slab_n == null
// (XFK_SPGEMM_SLAB=0): every row padded at row * CAP, moved by k_spgemm_compact.
// PACK (the Galerkin products, columns < kPackMaxCol): the network moves one 32-bit word per
// slot, column << log2(CAP) | slot, compared by its column alone, and the
// values are fetched from the product list once the slots are final.  The
// network makes the same comparisons and never exchanges equal columns in
// either form, so every product ends in the same slot and the sums keep
// their bits; a third of the registers move, and across lanes by DPP.
template <bool PMODE, int G, int CAP, bool PACK = false>
__global__ void __launch_bounds__(64) k_spgemm_sort(int nrows, SgX X, SgY Y, int *__restrict__ cnt_out,
                                                    int *__restrict__ pcol, double *__restrict__ pval, int *ovf,
                                                    int *need, int *__restrict__ slab_n)
{
    constexpr int W = 64 / G;
    constexpr int S = CAP / G;
    static_assert(S >= 1 && S * G == CAP, "CAP must be a multiple of G");
    __shared__ int pk_all[W][CAP];
    __shared__ double pv_all[W][CAP];
    const int g = threadIdx.x / G, l = threadIdx.x % G;
    const int row = blockIdx.x * W + g;
    int *pk = pk_all[g];
    double *pv = pv_all[g];
    const bool live = row < nrows;
    int np = 0;
    if (live) {
        const int xs = X.rowptr[row], xe = X.rowptr[row + 1];
        const ColView xc{X.col, X.c16, X.cbase};
        const int cb = xc.base(row);
        double omega = 0.0, dfi = 0.0;
        if (PMODE) {
            omega = X.wF[row];
            dfi = X.dfinv[row];
        }
        for (int e0 = xs; e0 < xe; e0 += G) {
            const int e = e0 + l;
            int len = 0, ys = 0;
            double xv = 0.0;
            if (e < xe) {
                const int k = xc.at(cb, e);
                if (k < X.col_lim) {
                    if (PMODE) {
                        const unsigned char f = X.mask[e];
                        if (f != 0 && Y.agg[k] >= 0) {
                            ys = Y.agg[k];
                            len = 1;
                            xv = (f == 2) ? 1.0 - omega : -omega * dfi * X.val[e];
                        }
                    } else {
                        ys = Y.rowptr[k];
                        len = Y.rowptr[k + 1] - ys;
                        xv = X.val[e];
                    }
                }
            }
            int incl = len;
#pragma unroll
            for (int off = 1; off < G; off <<= 1) {
                const int t = __shfl_up(incl, off, G);
                if (l >= off) incl += t;
            }
            const int total = __shfl(incl, G - 1, G);
            const int o = np + incl - len;
            if (PMODE) {
                if (len && o < CAP) {
                    pk[o] = ys;
                    pv[o] = xv;
                }
            } else {
                // the first U entries of the Y row loaded together (rows of P
                // hold ~2.5, of A P ~5: one memory latency instead of one per entry)
                constexpr int U = CAP >= 128 ? 8 : 4;
                int yc[U];
                double yv[U];
#pragma unroll
                for (int q = 0; q < U; ++q)
                    if (q < len) {
                        yc[q] = Y.col[ys + q];
                        yv[q] = Y.val[ys + q];
                    }
#pragma unroll
                for (int q = 0; q < U; ++q)
                    if (q < len && o + q < CAP) {
                        pk[o + q] = yc[q];
                        pv[o + q] = xv * yv[q];
                    }
                for (int q = U; q < len && o + q < CAP; ++q) {
                    pk[o + q] = Y.col[ys + q];
                    pv[o + q] = xv * Y.val[ys + q];
                }
            }
            np += total;
        }
        // a capacity taken from another problem (need != null): some row must
        // need more than half of it, else a measurement would have taken a
        // smaller class (whose sort order -- and so whose bits -- differ)
        if (need && np > CAP / 2 && l == 0 && *(volatile int *)need == 0) *need = 1;
        // more products than slots (a capacity taken from an earlier setup):
        // the row is garbage, the host redoes the product with a measured capacity
        if (np > CAP) {
            if (l == 0) *ovf = 1;
            np = CAP;
        }
    }
    wave_lds_sync();
    int key[S];
    double val[S];
    if constexpr (PACK) {
        constexpr int B = ilog2(CAP);
        unsigned w[S];
#pragma unroll
        for (int s = 0; s < S; ++s) {
            const int v = l * S + s;
            w[s] = v < np ? ((unsigned)pk[v] << B) | (unsigned)v : ~0u;
        }
        // the same network as below on the words' columns (an empty slot's
        // column, all ones, is above every real one, as INT_MAX is there)
#pragma unroll
        for (int k = 2; k <= CAP; k <<= 1) {
#pragma unroll
            for (int j = k >> 1; j > 0; j >>= 1) {
                if (j < S) {
#pragma unroll
                    for (int s = 0; s < S; ++s) {
                        const int t = s ^ j;
                        if (t > s) {
                            const bool up = ((l * S + s) & k) == 0;
                            const unsigned a = w[s] >> B, b = w[t] >> B;
                            if ((a > b) == up && a != b) {
                                const unsigned tw = w[s];
                                w[s] = w[t];
                                w[t] = tw;
                            }
                        }
                    }
                } else {
                    const int lm = j / S;
                    const bool lower = (l & lm) == 0;
#pragma unroll
                    for (int s = 0; s < S; ++s) {
                        const unsigned ow = xor_lanes(w[s], lm);
                        const unsigned a = w[s] >> B, b = ow >> B;
                        const bool up = ((l * S + s) & k) == 0;
                        const bool take = (lower == up) ? (b < a) : (b > a);
                        if (take) w[s] = ow;
                    }
                }
            }
        }
#pragma unroll
        for (int s = 0; s < S; ++s) {
            const bool real = w[s] != ~0u;
            key[s] = real ? (int)(w[s] >> B) : INT_MAX;
            val[s] = real ? pv[w[s] & (unsigned)(CAP - 1)] : 0.0;
        }
    } else {
#pragma unroll
        for (int s = 0; s < S; ++s) {
            const int v = l * S + s;
            key[s] = v < np ? pk[v] : INT_MAX;
            val[s] = v < np ? pv[v] : 0.0;
        }
        // bitonic sort of the CAP slots (slot v = l * S + s) by key
#pragma unroll
        for (int k = 2; k <= CAP; k <<= 1) {
#pragma unroll
            for (int j = k >> 1; j > 0; j >>= 1) {
                if (j < S) {
#pragma unroll
                    for (int s = 0; s < S; ++s) {
                        const int t = s ^ j;
                        if (t > s) {
                            const bool up = ((l * S + s) & k) == 0;
                            if ((key[s] > key[t]) == up && key[s] != key[t]) {
                                const int tk = key[s];
                                key[s] = key[t];
                                key[t] = tk;
                                const double tv = val[s];
                                val[s] = val[t];
                                val[t] = tv;
                            }
                        }
                    }
                } else {
                    const int lm = j / S;
                    const bool lower = (l & lm) == 0;
#pragma unroll
                    for (int s = 0; s < S; ++s) {
                        const int ok = __shfl_xor(key[s], lm, G);
                        const double ov = __shfl_xor(val[s], lm, G);
                        const bool up = ((l * S + s) & k) == 0;
                        // the lower slot of an ascending pair keeps the smaller key
                        const bool take = (lower == up) ? (ok < key[s]) : (ok > key[s]);
                        if (take) {
                            key[s] = ok;
                            val[s] = ov;
                        }
                    }
                }
            }
        }
    }
    // segmented inclusive scan: head = first slot of a column
    const int prev_last = __shfl_up(key[S - 1], 1, G);
    int head[S], nh = 0;
    double run[S];
#pragma unroll
    for (int s = 0; s < S; ++s) {
        const int pk_ = s > 0 ? key[s - 1] : (l > 0 ? prev_last : -1);
        head[s] = (key[s] != INT_MAX && key[s] != pk_) ? 1 : 0;
        run[s] = (s > 0 && !head[s]) ? run[s - 1] + val[s] : val[s];
        nh += head[s];
    }
    // carry from earlier lanes into this lane's leading (headless) slots
    int seg_open = 1;   // no head in this lane yet: the lane continues the previous segment
#pragma unroll
    for (int s = 0; s < S; ++s) seg_open &= !head[s];
    double carry = run[S - 1];   // this lane's trailing partial
    int hpre = nh;
    int open = seg_open;
#pragma unroll
    for (int off = 1; off < G; off <<= 1) {
        const double oc = __shfl_up(carry, off, G);
        const int oo = __shfl_up(open, off, G);
        const int oh = __shfl_up(hpre, off, G);
        if (l >= off) {
            if (open) carry = oc + carry;
            open = open && oo;
            hpre += oh;
        }
    }
    // carry / head count of the lanes before this one
    double cin = __shfl_up(carry, 1, G);
    int hin = __shfl_up(hpre, 1, G);
    if (l == 0) {
        cin = 0.0;
        hin = 0;
    }
    const int cnt = __shfl(hpre, G - 1, G);
    // slab layout: the wavefront's W rows back to back from blockIdx.x * W * CAP
    // (inclusive scan of the W counts, every lane of a group holding its row's;
    // a dead row counts 0)
    int upto = cnt;
#pragma unroll
    for (int off = G; off < 64; off <<= 1) {
        const int t = __shfl_up(upto, off, 64);
        if ((int)threadIdx.x >= off) upto += t;
    }
    if (slab_n && threadIdx.x == 63) slab_n[blockIdx.x] = upto;
    if (!live) return;
    const size_t base = slab_n ? (size_t)blockIdx.x * (W * CAP) + (upto - cnt) : (size_t)row * CAP;
    int h = hin;
#pragma unroll
    for (int s = 0; s < S; ++s) {
        bool lead = true;   // slots before this lane's first head continue the incoming segment
#pragma unroll
        for (int q = 0; q <= s; ++q) lead = lead && !head[q];
        const double tot = lead ? cin + run[s] : run[s];
        h += head[s];
        const int nk = s + 1 < S ? key[s + 1] : __shfl_down(key[0], 1, G);
        const bool tail = key[s] != INT_MAX && (nk != key[s] || (s + 1 == S && l == G - 1));
        if (tail) {
            pcol[base + h - 1] = key[s];
            pval[base + h - 1] = tot;
        }
    }
    if (l == 0) cnt_out[row] = cnt;
}

// padded rows (row * cap) -> CSR; 16 lanes per row, so a row's reads and
// writes are contiguous runs
// nnz_out (optional): the product's length, for a deferred host read;
// L lanes per row (a quarter of the slot capacity: the rows hold about that many)
template <int L>
__global__ void k_spgemm_compact(int nrows, int cap, const int *__restrict__ crow, const int *__restrict__ pcol,
                                 const double *__restrict__ pval, int *__restrict__ ccol, double *__restrict__ cval,
                                 int *nnz_out)
{
    const long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    if (t == 0 && nnz_out) *nnz_out = crow[nrows];
    const int row = (int)(t / L), l = (int)(t % L);
    if (row >= nrows) return;
    const int b = crow[row], n = crow[row + 1] - b;
    for (int m = l; m < n; m += L) {
        ccol[b + m] = pcol[(size_t)row * cap + m];
        cval[b + m] = pval[(size_t)row * cap + m];
    }
}

// dense slabs (k_spgemm_sort: slab b holds rows b * W ... back to back, slab_n[b]
// entries from b * stride) -> CSR.  A slab's rows are consecutive, so it lands
// as one run at crow[b * W]: both sides are dense, whatever the row lengths.
// kSlabLanes lanes per slab (slabs of level-0 products hold 40-100 entries),
// a workgroup moves 16 slabs.
constexpr int kSlabLanes = 16;
__global__ void k_spgemm_compact_slab(int nrows, int nslab, int W, int stride, const int *__restrict__ crow,
                                      const int *__restrict__ slab_n, const int *__restrict__ pcol,
                                      const double *__restrict__ pval, int *__restrict__ ccol,
                                      double *__restrict__ cval, int *nnz_out)
{
    const long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    if (t == 0 && nnz_out) *nnz_out = crow[nrows];
    const int b = (int)(t / kSlabLanes), l = (int)(t % kSlabLanes);
    if (b >= nslab) return;
    const int d = crow[b * W], n = slab_n[b];
    const size_t src = (size_t)b * stride;
    for (int m = l; m < n; m += kSlabLanes) {
        ccol[d + m] = pcol[src + m];
        cval[d + m] = pval[src + m];
    }
}

// XFK_SPGEMM_SLAB=0: the sub-wave SpGEMM writes padded rows (row * cap) and the
// compaction moves them row by row (the layout before the dense slabs)
static bool spgemm_slab_on()
{
    return env_int("XFK_SPGEMM_SLAB", 1) != 0;
}
// rows per k_spgemm_sort wavefront (64 / G of the instance launch_sort takes for `cap`)
static int sort_rows_per_wave(int cap) { return cap == 16 ? 16 : cap <= 64 ? 8 : cap == 128 ? 4 : 2; }

// slab_n: the slab lengths (null: padded rows)
void launch_compact(hipStream_t s, int nrows, int cap, const int *crow, const int *slab_n, const int *pc,
                    const double *pv, int *ccol, double *cval, int *nnz_out)
{
    if (slab_n) {
        const int W = sort_rows_per_wave(cap), nslab = (nrows + W - 1) / W;
        k_spgemm_compact_slab<<<(unsigned)(((long long)nslab * kSlabLanes + kB - 1) / kB), kB, 0, s>>>(
            nrows, nslab, W, W * cap, crow, slab_n, pc, pv, ccol, cval, nnz_out);
    } else if (cap <= 16)
        k_spgemm_compact<4><<<(unsigned)(((long long)nrows * 4 + kB - 1) / kB), kB, 0, s>>>(nrows, cap, crow, pc, pv,
                                                                                             ccol, cval, nnz_out);
    else if (cap <= 32)
        k_spgemm_compact<8><<<(unsigned)(((long long)nrows * 8 + kB - 1) / kB), kB, 0, s>>>(nrows, cap, crow, pc, pv,
                                                                                             ccol, cval, nnz_out);
    else
        k_spgemm_compact<16><<<(unsigned)(((long long)nrows * 16 + kB - 1) / kB), kB, 0, s>>>(nrows, cap, crow, pc,
                                                                                               pv, ccol, cval, nnz_out);
}

}  // namespace

// C = X Y (rowptr/col/val allocated here); XFK_ERR_UNSUPPORTED on LDS overflow
template <bool PMODE>
int spgemm(Amg &M, hipStream_t s, int nrows, const SgX &X, const SgY &Y, DBuf<int> &crow, DBuf<int> &ccol,
           DBuf<double> &cval, long long &cnnz, int key, bool defer)
{
    // (behind the row lengths: the slab lengths, at most one per two rows)
    AMG_CHECK(M.cnt.alloc((size_t)nrows + 1 + ((size_t)nrows + 1) / 2));
    AMG_CHECK(crow.alloc((size_t)nrows + 1));
    int *slab_n = spgemm_slab_on() ? M.cnt.p + nrows + 1 : nullptr;
    // the sort kernel of the capacity class (rows of at most `cap` slots,
    // nrows * cap slots in pad_col / pad_val in either layout)
    int *sovf = M.dev_int.p + 6;
    auto launch_sort = [&](int cap, int *ovf, int *need = nullptr) {
        int *pc = M.pad_col.p;
        double *pv = M.pad_val.p;
        if (nrows > 0) {
            // few lanes per row, 4-8 sorted slots per lane: many rows per
            // wavefront to overlap their dependent gathers
            // (the prolongator never packs: for PMODE both names are the one unpacked instance)
#define XFK_SORT(GG, CC, WW)                                                       \
    (X.pack ? k_spgemm_sort<PMODE, GG, CC, !PMODE> : k_spgemm_sort<PMODE, GG, CC>) \
        <<<(nrows + WW - 1) / WW, 64, 0, s>>>(nrows, X, Y, M.cnt.p, pc, pv, ovf, need, slab_n)
            if (cap == 16) XFK_SORT(4, 16, 16);
            else if (cap == 32) XFK_SORT(8, 32, 8);
            else if (cap == 64) XFK_SORT(8, 64, 8);
            else if (cap == 128) XFK_SORT(16, 128, 4);
            else XFK_SORT(32, 256, 2);
#undef XFK_SORT
        }
    };
    // single pass into padded rows of `cap` slots (sort-based), then scan +
    // compaction; returns the overflow flag (rows with more products than
    // slots), read back with the scan's own synchronisation
    auto sort_pass = [&](int cap, bool &overflow) -> int {
        AMG_CHECK(M.pad_col.alloc((size_t)nrows * cap));
        AMG_CHECK(M.pad_val.alloc((size_t)nrows * cap));
        AMG_CHECK(hipMemsetAsync(sovf, 0, sizeof(int), s));
        launch_sort(cap, sovf);
        AMG_CHECK(hipMemcpyAsync(M.host_int + 4, sovf, sizeof(int), hipMemcpyDeviceToHost, s));
        int rc = scan_total(M, s, M.cnt.p, crow.p, nrows, cnnz);   // synchronises
        if (rc != XFK_OK) return rc;
        overflow = M.host_int[4] != 0;
        if (overflow) return XFK_OK;
        AMG_CHECK(ccol.alloc((size_t)std::max(1LL, cnnz)));
        AMG_CHECK(cval.alloc((size_t)std::max(1LL, cnnz)));
        if (nrows > 0)
            launch_compact(s, nrows, cap, crow.p, slab_n, M.pad_col.p, M.pad_val.p, ccol.p, cval.p, nullptr);
        return XFK_OK;
    };
    // the slot capacity this product needed in the previous setup (same
    // call site): taken without measuring the longest product list first,
    // and without any host synchronisation -- the output is sized for
    // nrows x cap, its length and the kernel's overflow flag land in a
    // deferred slot that the setup reads once at its end (an overflow there
    // rebuilds the hierarchy with measured capacities)
    auto deferred_pass = [&](int cap, bool verify = false) -> int {
        int *slot = M.def_dev.p + M.def_n;
        // (a capacity from another problem: its class is checked on the device)
        int *need = (verify && cap > 16) ? M.def_dev.p + kAmgDeferSlots + M.def_n / 2 : nullptr;
        M.def_verify[M.def_n / 2] = need ? cap : 0;
        AMG_CHECK(M.pad_col.alloc((size_t)nrows * cap));
        AMG_CHECK(M.pad_val.alloc((size_t)nrows * cap));
        AMG_CHECK(ccol.alloc((size_t)std::max(1LL, (long long)nrows * cap)));
        AMG_CHECK(cval.alloc((size_t)std::max(1LL, (long long)nrows * cap)));
        launch_sort(cap, slot, need);
        int rc = scan_only(M, s, M.cnt.p, crow.p, nrows);
        if (rc != XFK_OK) return rc;
        if (nrows > 0)
            launch_compact(s, nrows, cap, crow.p, slab_n, M.pad_col.p, M.pad_val.p, ccol.p, cval.p, slot + 1);
        else
            AMG_CHECK(hipMemsetAsync(slot + 1, 0, sizeof(int), s));
        M.def_target[M.def_n / 2] = &cnnz;
        M.def_n += 2;
        cnnz = (long long)nrows * cap;   // an upper bound until the deferred read
        return XFK_OK;
    };
    if (key >= 0) {
        auto hint = M.cap_hint.find(key);
        if (hint != M.cap_hint.end()) {
            if (defer && M.def_n + 2 <= kAmgDeferSlots) return deferred_pass(hint->second, M.foreign);
            if (M.foreign) {   // (no slot to check another problem's capacity in: measure)
                M.cap_hint.erase(hint);
                hint = M.cap_hint.end();
            }
        }
        if (hint != M.cap_hint.end()) {
            bool overflow = false;
            int rc = sort_pass(hint->second, overflow);
            if (rc != XFK_OK || !overflow) return rc;
            M.cap_hint.erase(hint);
        }
    }
    // longest product list -> sub-wave (<= 64 products per row) or wave-per-row kernels
    int maxprod = 0;
    if (nrows > 0) {
        k_spgemm_nprod<PMODE><<<nb(nrows), kB, 0, s>>>(nrows, X, Y, M.cnt.p);
        size_t bytes = 0;
        AMG_CHECK(hipcub::DeviceReduce::Max(nullptr, bytes, M.cnt.p, M.dev_int.p + 3, nrows, s));
        AMG_CHECK(M.cub_tmp.alloc(bytes ? bytes : 1));
        AMG_CHECK(hipcub::DeviceReduce::Max(M.cub_tmp.p, bytes, M.cnt.p, M.dev_int.p + 3, nrows, s));
        int rc = read_flag(M, s, 3, maxprod);
        if (rc != XFK_OK) return rc;
    }
    if (maxprod <= kSortCap) {
        const int cap = maxprod <= 16 ? 16 : maxprod <= 32 ? 32 : maxprod <= 64 ? 64 : maxprod <= 128 ? 128 : 256;
        int rc = XFK_OK;
        if (defer && key >= 0 && M.def_n + 2 <= kAmgDeferSlots) {
            // the measured capacity (no overflow possible) through the
            // deferred slot as a hinted one: the same kernels, so the same
            // bits, without the host check for the length (~20 us per call
            // site of a first setup)
            rc = deferred_pass(cap);
        } else {
            bool overflow = false;
            rc = sort_pass(cap, overflow);
            if (rc == XFK_OK && overflow) {
                set_error("AMG: internal SpGEMM capacity error");
                return XFK_ERR_HIP;
            }
        }
        if (rc != XFK_OK) return rc;
        if (key >= 0) {
            // XFK_AMG_TEST_SMALL_HINT=1 (tests only): store a too-small capacity so
            // the next setup takes the overflow-and-rebuild path
            const bool small = env_set("XFK_AMG_TEST_SMALL_HINT");
            M.cap_hint[key] = small ? 16 : cap;   // (16: the smallest capacity the kernels have)
        }
        return XFK_OK;
    }
    AMG_CHECK(hipMemsetAsync(M.dev_int.p + 2, 0, 2 * sizeof(int), s));
    if (nrows > 0)
        k_spgemm<false, PMODE, kSgMax><<<nrows, 64, 0, s>>>(nrows, X, Y, M.cnt.p, nullptr, nullptr, nullptr,
                                                            M.dev_int.p + 2);
    if (nrows > 0) {   // longest row -> LDS capacity of the FILL pass
        size_t bytes = 0;
        AMG_CHECK(hipcub::DeviceReduce::Max(nullptr, bytes, M.cnt.p, M.dev_int.p + 3, nrows, s));
        AMG_CHECK(M.cub_tmp.alloc(bytes ? bytes : 1));
        AMG_CHECK(hipcub::DeviceReduce::Max(M.cub_tmp.p, bytes, M.cnt.p, M.dev_int.p + 3, nrows, s));
    }
    AMG_CHECK(hipMemcpyAsync(M.host_int + 2, M.dev_int.p + 2, 2 * sizeof(int), hipMemcpyDeviceToHost, s));
    int rc = scan_total(M, s, M.cnt.p, crow.p, nrows, cnnz);   // synchronises
    if (rc != XFK_OK) return rc;
    const int ovf = M.host_int[2], maxrow = M.host_int[3];
    if (ovf) {
        set_error("AMG: a SpGEMM row exceeds the LDS hash capacity");
        return XFK_ERR_UNSUPPORTED;
    }
    AMG_CHECK(ccol.alloc((size_t)std::max(1LL, cnnz)));
    AMG_CHECK(cval.alloc((size_t)std::max(1LL, cnnz)));
    if (nrows > 0) {
        int *of = M.dev_int.p + 2;
        if (maxrow <= 32)
            k_spgemm<true, PMODE, 32><<<nrows, 64, 0, s>>>(nrows, X, Y, nullptr, crow.p, ccol.p, cval.p, of);
        else if (maxrow <= 128)
            k_spgemm<true, PMODE, 128><<<nrows, 64, 0, s>>>(nrows, X, Y, nullptr, crow.p, ccol.p, cval.p, of);
        else
            k_spgemm<true, PMODE, kSgMax><<<nrows, 64, 0, s>>>(nrows, X, Y, nullptr, crow.p, ccol.p, cval.p, of);
    }
    return XFK_OK;
}

template int spgemm<false>(Amg &, hipStream_t, int, const SgX &, const SgY &, DBuf<int> &, DBuf<int> &,
                           DBuf<double> &, long long &, int, bool);
template int spgemm<true>(Amg &, hipStream_t, int, const SgX &, const SgY &, DBuf<int> &, DBuf<int> &,
                          DBuf<double> &, long long &, int, bool);

}  // namespace xfk

// xfk_device_init: loads this translation unit's code object onto the device
hipError_t xfk::warm_module_amg_spgemm()
{
    hipFuncAttributes a;
    return hipFuncGetAttributes(&a, reinterpret_cast<const void *>(&k_spgemm_compact_slab));
}
