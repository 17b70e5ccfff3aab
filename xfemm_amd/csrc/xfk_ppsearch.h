// What the post-processors of the scalar-potential problems (xfk_postproc.hip)
// and of the magnetostatic problems (xfk_magpost.hip) share: the search for the
// element containing a point over a cell grid, and the layout of a batch of
// contours.  Both work on a mesh (x, y, p) in the problem's length units; a
// problem is of one kind, so the grid lives in one place (the pp_ group of
// xfk_problem).  Included after the including file's `fp contract(off)`: the
// edge tests decide which element a point belongs to.
#pragma once
#include "xfk_potential.h"

namespace xfk {

// abs(CComplex) (femmcomplex.cpp:749-757)
__host__ __device__ __forceinline__ double pp_cabs(double re, double im)
{
    if ((re == 0) && (im == 0)) return 0.;
    if (fabs(re) > fabs(im)) return fabs(re) * sqrt(1. + (im / re) * (im / re));
    return fabs(im) * sqrt(1. + (re / im) * (re / im));
}

// --- the cell grid ----------------------------------------------------------

struct PpGrid {
    double x0, y0, ihx, ihy;
    int nx, ny;
};

// The cell grid and the oversize list as the search reads them
struct PpLists {
    const int *ptr, *cell_el, *big;
    int nbig;
};

__device__ __forceinline__ int pp_cell1(double v, double v0, double ih, int n)
{
    const double f = floor((v - v0) * ih);
    if (!(f > 0.)) return 0;
    if (f >= (double)(n - 1)) return n - 1;
    return (int)f;
}

// InTriangleTest (PostProcessor.cpp:359-398, fpproc.cpp:3387-3424) as written:
// every edge oriented from its lower-numbered node, < 0 rejecting one way and
// > 0 the other
__device__ __forceinline__ bool pp_in_triangle(const double *__restrict__ xs, const double *__restrict__ ys,
                                               const int *__restrict__ p, int i, double x, double y)
{
    const int n[3] = {p[3 * i], p[3 * i + 1], p[3 * i + 2]};
    const double X[3] = {xs[n[0]], xs[n[1]], xs[n[2]]}, Y[3] = {ys[n[0]], ys[n[1]], ys[n[2]]};
    bool in = true;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const int k = (j + 1) % 3;
        if (n[k] > n[j]) {
            const double z = (X[k] - X[j]) * (y - Y[j]) - (Y[k] - Y[j]) * (x - X[j]);
            if (z < 0) in = false;
        } else {
            const double z = (X[j] - X[k]) * (y - Y[k]) - (Y[j] - Y[k]) * (x - X[k]);
            if (z > 0) in = false;
        }
    }
    return in;
}

// The lowest-numbered element of the mesh (xs, ys, p) containing (x, y), or -1
// when none does (or a coordinate is NaN); ntests: the elements the point was
// tested against
__device__ __forceinline__ int pp_find(const double *__restrict__ xs, const double *__restrict__ ys,
                                       const int *__restrict__ p, const PpGrid &G, const PpLists &L, double x,
                                       double y, int &ntests)
{
    int k = 0x7fffffff;
    ntests = 0;
    if (x == x && y == y) {
        const int c = pp_cell1(y, G.y0, G.ihy, G.ny) * G.nx + pp_cell1(x, G.x0, G.ihx, G.nx);
        ntests = L.ptr[c + 1] - L.ptr[c] + L.nbig;
        for (int m = L.ptr[c]; m < L.ptr[c + 1]; ++m) {
            const int e = L.cell_el[m];
            if (e < k && pp_in_triangle(xs, ys, p, e, x, y)) k = e;
        }
        for (int m = 0; m < L.nbig; ++m) {
            const int e = L.big[m];
            if (e < k && pp_in_triangle(xs, ys, p, e, x, y)) k = e;
        }
    }
    return k == 0x7fffffff ? -1 : k;
}

// host side (xfk_postproc.hip).  pp_grid_dims: the grid over the bounding box
// of the host coordinates, cells of twice the mean element area, into P.
// pp_grid_build: count, exclusive scan, fill over the device mesh -- once per
// problem (P->pp_grid_ready).
void pp_grid_dims(xfk_problem *P, const double *x, const double *y, int N, int NE);
int pp_grid_build(xfk_problem *P, const double *x, const double *y, const int *p);

inline PpGrid pp_grid_args(const xfk_problem *P)
{
    return PpGrid{P->pp_x0, P->pp_y0, P->pp_ihx, P->pp_ihy, P->pp_nx, P->pp_ny};
}

inline PpLists pp_lists(const xfk_problem *P)
{
    return PpLists{P->pp_cell_ptr.p, P->pp_cell_el.p, P->pp_big.p, P->pp_nbig};
}

// --- contour integrals --------------------------------------------------------

constexpr int kPpLineIntegralPoints = 400;   // d_LineIntegralPoints (PostProcessor.cpp:76, fpproc.cpp:99)

// A batch of contours checked and laid out for a contour kernel: contour c
// holds the vertices cptr[c] .. cptr[c + 1) and owns the workgroups (of
// kPotQBlock samples) bptr[c] .. bptr[c + 1)
struct PpContours {
    int nc = 0, type = 0, smooth = 0, npts = 0;
    std::vector<int> cptr, bptr;   // vertices and workgroups of each contour
    DBuf<int> d_cptr, d_bptr;
    DBuf<double> d_xy;             // the vertices: all x, then all y
    DBuf<double> part;             // 3 per workgroup, then 3 per contour
    int groups() const { return bptr.empty() ? 0 : bptr.back(); }
    double *sums() { return part.p + 3 * (size_t)groups(); }
};

// the batch's arrays as a caller may pass them (the type's range is the caller's to check)
int pp_contour_check(int nc, const int *ptr, const double *x, const double *y);
// the layout of the batch, its vertices and offsets on the device, the partials allocated
int pp_contour_layout(xfk_problem *P, int nc, const int *ptr, const double *x, const double *y, int type, int smooth,
                      int npts, PpContours &J);
// one workgroup per contour: its workgroups' partials in a fixed order into J.sums()
void launch_contour_sum(hipStream_t s, PpContours &J);

}  // namespace xfk
