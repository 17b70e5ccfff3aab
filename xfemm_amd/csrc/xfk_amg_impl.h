// Private to the xfk_amg*.hip translation units: what more than one of them
// needs.  xfk_amg.h is the interface the rest of the library sees.
//   xfk_amg.hip         strength, MIS-2, joins, R = P^T, the folded transfer's
//                       setup, scans, stream pool, hints, build, sharded
//                       Galerkin path, probes
//   xfk_amg_spgemm.hip  the SpGEMM kernels and their host driver
//   xfk_amg_dense.hip   the dense coarsest inverse (blocked Gauss-Jordan,
//                       nested dissection)
//   xfk_amg_cycle.hip   smoothers, SpMV, folded steps, the V/W-cycle hosts
#pragma once

#include <string>

#include "xfk_amg.h"
#include "xfk_spmv.h"

// shared between the files, not with the library's users: no dynamic symbol
#define XFK_AMG_LOCAL __attribute__((visibility("hidden")))

#define AMG_CHECK(call)                                                          \
    do {                                                                         \
        hipError_t _e = (call);                                                  \
        if (_e != hipSuccess) {                                                  \
            ::xfk::set_error(std::string(#call) + ": " + hipGetErrorString(_e)); \
            return XFK_ERR_HIP;                                                  \
        }                                                                        \
    } while (0)

namespace xfk {

constexpr int kB = 256;
static inline int nb(long long n) { return (int)((n + kB - 1) / kB); }

// The columns of a level's CSR as the aggregation reads them: the int array,
// or (level 0) the 16-bit offsets from the row's 512-row tile base
// (xfk_spmv.h k_tile_col16; a tile without a base reads the int array)
struct ColView {
    const int *col;
    const unsigned short *c16;   // null: int columns only
    const int *cbase;
    __device__ __forceinline__ int base(int i) const { return c16 ? cbase[i / kCgBlock] : kNoColBase; }
    __device__ __forceinline__ int at(int cb, int k) const { return cb != kNoColBase ? cb + (int)c16[k] : col[k]; }
};

__device__ __forceinline__ double rho_of(const unsigned long long *p)
{
    return __longlong_as_double((long long)*p);
}

// the SpGEMM's operands (xfk_amg_spgemm.hip)
struct SgX {
    const int *rowptr, *col;
    const double *val;
    int col_lim;                   // X columns >= col_lim are skipped (sharded halo)
    const unsigned char *mask;     // PMODE: sflag (1 strong, 2 diagonal)
    const double *dfinv;           // PMODE: D_F^-1
    const double *wF;              // PMODE: per-row smoothing weight
    const unsigned short *c16 = nullptr;   // level 0: 16-bit tile columns (k_spgemm_sort reads them)
    const int *cbase = nullptr;
    int pack = 0;                  // k_spgemm_sort: sort (column, slot) words, not (column, value) pairs
};
struct SgY {
    const int *rowptr, *col;
    const double *val;
    const int *agg;                // PMODE: P_tent
};

constexpr int kSortCap = 256;         // k_spgemm_sort: rows of at most this many products
// columns a packed sort word can hold next to the slot index of the largest class
constexpr int kPackMaxCol = (1 << (32 - 8)) - 1;

// block width of the dense coarsest inverse (xfk_amg_dense.hip)
constexpr int kBj = 64;

// XFK_AMG_NO_FOREIGN=1: fresh problems measure everything (the hint store, xfk_amg.hip)
static inline bool foreign_on() { return !env_set("XFK_AMG_NO_FOREIGN"); }

// out[0..n] = exclusive scan of in[0..n-1], out[n] = total; returns total
// (host-synchronising).  scan_only: the same without reading the total back,
// with the given temporary storage; `in` must hold n + 1 readable entries.
// read_flag: dev_int[idx] on the host.  (xfk_amg.hip)
XFK_AMG_LOCAL int scan_total(Amg &A, hipStream_t s, const int *in, int *out, int n, long long &total);
XFK_AMG_LOCAL int scan_only(DBuf<char> &tmp, hipStream_t s, const int *in, int *out, int n);
XFK_AMG_LOCAL int scan_only(Amg &A, hipStream_t s, const int *in, int *out, int n);
XFK_AMG_LOCAL int read_flag(Amg &A, hipStream_t s, int idx, int &v);

// C = X Y (rowptr/col/val allocated here); XFK_ERR_UNSUPPORTED on LDS overflow.
// PMODE: the smoothed prolongator (xfk_amg_spgemm.hip, which instantiates both)
template <bool PMODE>
XFK_AMG_LOCAL int spgemm(Amg &M, hipStream_t s, int nrows, const SgX &X, const SgY &Y, DBuf<int> &crow,
                         DBuf<int> &ccol, DBuf<double> &cval, long long &cnnz, int key = -1, bool defer = true);
extern template int spgemm<false>(Amg &, hipStream_t, int, const SgX &, const SgY &, DBuf<int> &, DBuf<int> &,
                                  DBuf<double> &, long long &, int, bool);
extern template int spgemm<true>(Amg &, hipStream_t, int, const SgX &, const SgY &, DBuf<int> &, DBuf<int> &,
                                 DBuf<double> &, long long &, int, bool);

}  // namespace xfk
