// What the post-processors of the scalar-potential problems (xfk_postproc.hip)
// and of the magnetostatic problems (xfk_magpost.hip) share: the search for the
// element containing a point over a cell grid, and the layout of a batch of
// contours, and the host plumbing of their point and contour entry points.
// Both work on a mesh (x, y, p) in the problem's length units; a problem is of
// one kind, so the grid and the point batch live in one place (the pp_ group
// of xfk_problem).  Included after the including file's `fp contract(off)`: the
// edge tests decide which element a point belongs to.
#pragma once
#include "xfk_post.h"
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

// --- host plumbing of the point and contour entry points ------------------------

// the node -> element lists of a host mesh p in element order (each node's list ascending)
inline void node_elements(const int *p, int N, int NE, std::vector<int> &ptr, std::vector<int> &lst)
{
    ptr.assign((size_t)N + 1, 0);
    for (size_t k = 0; k < 3 * (size_t)NE; ++k) ptr[p[k] + 1]++;
    for (int i = 0; i < N; ++i) ptr[i + 1] += ptr[i];
    lst.resize(3 * (size_t)NE);
    std::vector<int> fill(ptr.begin(), ptr.end() - 1);
    for (int e = 0; e < NE; ++e)
        for (int j = 0; j < 3; ++j) lst[fill[p[3 * (size_t)e + j]]++] = e;
}

// a batch of points on the device: x, y, then nvals values each (pp_pts), and each point's element (pp_pel)
inline int upload_points(xfk_problem *P, int n, const double *x, const double *y, int nvals)
{
    XFK_CHECK(P->pp_pts.alloc((2 + (size_t)nvals) * (size_t)n));
    XFK_CHECK(P->pp_pel.alloc((size_t)n));
    XFK_CHECK(hipMemcpyAsync(P->pp_pts.p, x, sizeof(double) * n, hipMemcpyHostToDevice, P->stream));
    XFK_CHECK(hipMemcpyAsync(P->pp_pts.p + n, y, sizeof(double) * n, hipMemcpyHostToDevice, P->stream));
    return XFK_OK;
}

// each contour's first and last vertex, in that order: the 2 nc points of lineIntegral type 0
inline void contour_end_points(int nc, const int *ptr, const double *x, const double *y, std::vector<double> &ex,
                               std::vector<double> &ey)
{
    ex.resize(2 * (size_t)nc);
    ey.resize(2 * (size_t)nc);
    for (int c = 0; c < nc; ++c) {
        ex[2 * c] = x[ptr[c]];
        ey[2 * c] = y[ptr[c]];
        ex[2 * c + 1] = x[ptr[c + 1] - 1];
        ey[2 * c + 1] = y[ptr[c + 1] - 1];
    }
}

// A polyline's length and, with swept, the area it sweeps about the axis, both
// in user units: the sums of lineIntegral type 2 (epproc.cpp:574-595,
// hpproc.cpp:727-744, fpproc.cpp:4119-4130, 4200-4213) before the caller's
// scaling to metres
inline void polyline_sums(int n, const double *x, const double *y, bool swept, double &len, double &area)
{
    len = 0;
    area = 0;
    for (int i = 0; i < n - 1; ++i) len += pp_cabs(x[i + 1] - x[i], y[i + 1] - y[i]);
    if (swept)
        for (int i = 0; i < n - 1; ++i) area += (kPI * (x[i] + x[i + 1]) * pp_cabs(x[i + 1] - x[i], y[i + 1] - y[i]));
}

// The body of xfk_*_contour_samples: the sample points of one contour and the
// element of each.  check(P, nc, ptr, x, y, type), prepare(P, nc, ptr, x, y,
// type, smooth, npts, J) and launch(P, J, xy, elem) are the caller's.
template <class C, class R, class L>
int contour_samples(xfk_problem *P, int n, const double *x, const double *y, int type, int npts, double *xy, int *elem,
                    C check, R prepare, L launch)
{
    XFK_REQUIRE(n >= 0, XFK_ERR_ARG, "negative number of contour points");
    const int ptr[2] = {0, n};
    int rc = check(P, 1, ptr, x, y, type);
    if (rc != XFK_OK) return rc;
    XFK_REQUIRE(type != 0 && type != 2, XFK_ERR_ARG, "line integral types 0 and 2 take no samples");
    XFK_REQUIRE(xy && elem, XFK_ERR_ARG, "null output");
    PpContours J;
    if ((rc = prepare(P, 1, ptr, x, y, type, 0, npts, J)) != XFK_OK) return rc;
    const size_t ns = (size_t)(n - 1) * J.npts;
    DBuf<double> dxy;
    DBuf<int> del;
    XFK_CHECK(dxy.alloc(2 * ns));
    XFK_CHECK(del.alloc(ns));
    if ((rc = launch(P, J, dxy.p, del.p)) != XFK_OK) return rc;
    XFK_CHECK(d2h(xy, dxy.p, sizeof(double) * 2 * ns, P->stream));
    XFK_CHECK(d2h(elem, del.p, sizeof(int) * ns, P->stream));
    return XFK_OK;
}

// The body of xfk_*_contour_time after the caller's check of its own
// arguments: the median time of the contour launch over a batch
template <class C, class R, class L>
int contour_time(xfk_problem *P, int nc, const int *ptr, const double *x, const double *y, int type, int smooth,
                 int npts, int repeats, double *ms, C check, R prepare, L launch)
{
    int rc = check(P, nc, ptr, x, y, type);
    if (rc != XFK_OK) return rc;
    XFK_REQUIRE(type != 0 && type != 2, XFK_ERR_ARG, "line integral types 0 and 2 launch no contour kernel");
    PpContours J;
    if ((rc = prepare(P, nc, ptr, x, y, type, smooth, npts, J)) != XFK_OK) return rc;
    return timed_median(P->stream, repeats, [&] { return launch(P, J, nullptr, nullptr); }, *ms);
}

}  // namespace xfk
