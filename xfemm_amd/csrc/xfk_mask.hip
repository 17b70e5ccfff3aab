// The weighted stress tensor mask on the device, for MI355X (gfx950): what the
// reference's PostProcessor::makeMask (PostProcessor.cpp:497-725, with isKosher
// 400-430, FindBoundaryEdges 1097-1150 and isSelectionOnAxis,
// epproc.cpp:471-487) and FPProc::MakeMask (makemask.cpp:48-414, with
// FindBoundaryEdges, fpproc.cpp:5356-5415) compute, which are one algorithm.
//
// A second finite-element problem on the same mesh: a Laplacian weighted per
// element by its label's mesh-size specification, nodal values fixed by the
// rules of PostProcessor.cpp:545-629 (makemask.cpp:136-201), solved and
// thresholded at 0.5 into a 0/1 nodal mask; the force and the torque of the
// callers then sum a stress expression against the gradient of that mask over
// all elements.  The rules are independent per node apart from their order,
// so a thread per node applies them in that order; the solve is the static
// driver's, on an auxiliary problem over the mesh's own connectivity (no
// conductors, no periodic pairs, as the reference).
//
// The two callers (xfk_postproc.hip: electrostatics; xfk_magpost.hip:
// magnetostatics) differ in where "selected" and "not air" come from, which
// they settle on the host into two bytes per entry of their label table, and
// in two rules only the electrostatic mask has: conductor nodes and selected
// nodes.  All arithmetic is the reference's, operation by operation, in
// double, without contraction into fused multiply-adds.
#include "xfk_potential.h"

#include <chrono>

#pragma clang fp contract(off)

namespace xfk {

// FindBoundaryEdges (PostProcessor.cpp:1097-1150): one thread per (element,
// side).  Side j runs from p[(j + 1) % 3] to p[(j + 2) % 3]; it is exterior
// when no other element around its first node holds its second.  ext (zeroed
// by the caller) marks both ends; every store writes the same 1.
__global__ void __launch_bounds__(kBlock) k_mask_exterior(int NE, const int *__restrict__ p,
                                                          const int *__restrict__ n2e_ptr,
                                                          const int *__restrict__ n2e, unsigned char *__restrict__ ext)
{
    const int t = blockIdx.x * kBlock + threadIdx.x;
    if (t >= 3 * NE) return;
    const int e = t / 3, j = t - 3 * e;
    const int org = p[3 * e + (j + 1) % 3], dest = p[3 * e + (j + 2) % 3];
    bool done = false;
    for (int m = n2e_ptr[org]; m < n2e_ptr[org + 1] && !done; ++m) {
        const int ei = n2e[m];
        if (ei == e) continue;
        done = p[3 * ei] == dest || p[3 * ei + 1] == dest || p[3 * ei + 2] == dest;
    }
    if (!done) {
        ext[org] = 1;
        ext[dest] = 1;
    }
}

// What the rules read, for either caller
struct MaskRules {
    const double *x;               // user length units
    const int *p, *lbl;
    const int *n2e_ptr, *n2e;      // node -> elements of p, in the caller's order
    const unsigned char *lflag;    // per entry of the label table: selected, then not air
    const unsigned char *ext;      // the node ends an exterior edge
    const unsigned char *point;    // the node carries a point property
    const int *q;                  // the conductor marks (-2: none); null: no node is a conductor's
    const unsigned char *nsel;     // the selected nodes; null: none
    int axi;
};

// isSelectionOnAxis (epproc.cpp:471-487, PostProcessor.cpp:479-494; bOnAxis,
// makemask.cpp:94-106), for an axisymmetric problem: a selected element or a
// selected node at r < 1e-6.  One thread per element and, with selected nodes,
// per node; flag[0] (zeroed by the caller) is set.
__global__ void __launch_bounds__(kBlock) k_mask_on_axis(int NE, int N, MaskRules A, int *__restrict__ flag)
{
    const int t = blockIdx.x * kBlock + threadIdx.x;
    bool on = false;
    if (t < NE && A.lflag[2 * A.lbl[t]])
        for (int j = 0; j < 3; ++j) on |= A.x[A.p[3 * t + j]] < 1.e-6;
    if (A.nsel && t < N && A.nsel[t]) on |= A.x[t] < 1.e-6;
    if (on) flag[0] = 1;
}

// The fixed values L.V of makeMask (PostProcessor.cpp:545-629,
// makemask.cpp:136-201), one thread per node, the rules in the reference's
// order so that a later one overwrites an earlier one as the sequential code
// does; -1: free.
__global__ void __launch_bounds__(kBlock) k_mask_fix(int N, MaskRules A, const int *__restrict__ flag,
                                                     double *__restrict__ lv)
{
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= N) return;
    const int l0 = A.n2e_ptr[i], l1 = A.n2e_ptr[i + 1];
    // a fixed point property or any conductor node
    double v = (A.q && A.q[i] != -2) ? 0. : -1.;
    // the ends of exterior edges; with the selection on the axis only where isKosher (PostProcessor.cpp:400-430,
    // makemask.cpp:383-414)
    if (A.ext[i]) {
        bool kosher = true;
        if (flag[0] && A.axi && !(A.x[i] > 1.e-6)) {
            int score = 0;
            for (int m = l0; m < l1; ++m)
                for (int j = 0; j < 3; ++j) {
                    const int n = A.p[3 * A.n2e[m] + j];
                    if ((n != i) && (A.x[n] < 1.e-6)) score++;
                }
            kosher = !(score > 1);
        }
        if (kosher) v = 0.;
    }
    // the nodes of selected elements 1, of unselected elements that are not
    // air 0, in element order: the highest-numbered such element decides,
    // whatever the order of the node's list (angle-sorted or ascending)
    int last = -1;
    bool last_sel = false;
    for (int m = l0; m < l1; ++m) {
        const int e = A.n2e[m];
        if (e < last) continue;
        const unsigned char *f = A.lflag + 2 * A.lbl[e];
        if (f[0] || f[1]) {
            last = e;
            last_sel = f[0] != 0;
        }
    }
    if (last >= 0) v = last_sel ? 1. : 0.;
    // a still-free node with a point property
    if (A.point[i] && (v < 0)) v = 0.;
    // a selected node
    if (A.nsel && A.nsel[i]) v = 1.;
    lv[i] = v;
}

// makeMask's consistency check (PostProcessor.cpp:655-671,
// makemask.cpp:233-254): an unselected element that is not air with a node not
// fixed at exactly 0 sets flag[1]
__global__ void __launch_bounds__(kBlock) k_mask_valid(int NE, MaskRules A, const double *__restrict__ lv,
                                                       int *__restrict__ flag)
{
    const int e = blockIdx.x * kBlock + threadIdx.x;
    if (e >= NE) return;
    const unsigned char *f = A.lflag + 2 * A.lbl[e];
    if (f[0] || !f[1]) return;
    int k = 0;
    for (int j = 0; j < 3; ++j)
        if (lv[A.p[3 * e + j]] == 0) k++;
    if (k < 3) flag[1] = 1;
}

// One element of makeMask (PostProcessor.cpp:631-708) for the row gather of
// xfk_potential.h: Me = v (p_j p_k + q_j q_k) / area with v the square root of
// the label's MaxArea (of the element's area when that is <= 0), prescribed
// values eliminated per element.  The reference stores the negated system
// (L.Put(L.Get - Me), b -= be), which is what the gather's "-=" builds; the
// element hands it -Me and -be, so the assembled system is the positive
// definite one the PCG needs.  It has the same solution.  The mask Laplacian
// is planar for both problem types.
struct MaskPhys {
    struct Args {
        const double *lv, *max_area;
    };

    template <bool AXI>
    static __device__ __forceinline__ void element(int e, const int (&g)[3], const RowArgs &A, const Args &S,
                                                   const double (&X)[3], const double (&Y)[3], const PotLabel &,
                                                   double (&Me)[3][3], double (&be)[3])
    {
        double p[3], q[3];
        p[0] = Y[1] - Y[2]; p[1] = Y[2] - Y[0]; p[2] = Y[0] - Y[1];
        q[0] = X[2] - X[1]; q[1] = X[0] - X[2]; q[2] = X[1] - X[0];
        const double area = (p[0] * q[1] - p[1] * q[0]) / 2.;
        double v = S.max_area ? S.max_area[A.lbl[e]] : 0.;
        if (v <= 0) v = sqrt(area);
        else v = sqrt(v);
        const double V[3] = {S.lv[g[0]], S.lv[g[1]], S.lv[g[2]]};
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            be[j] = 0.;
#pragma unroll
            for (int k = 0; k < 3; ++k) Me[j][k] = v * (p[j] * p[k] + q[j] * q[k]) / area;
        }
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            if (V[j] >= 0) {
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    if (j != k) {
                        be[k] -= Me[k][j] * V[j];
                        Me[k][j] = 0.;
                        Me[j][k] = 0.;
                    }
                }
                be[j] = V[j] * Me[j][j];
            }
        }
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            be[j] = -be[j];
#pragma unroll
            for (int k = 0; k < 3; ++k) Me[j][k] = -Me[j][k];
        }
    }
};

void launch_mask_rows(hipStream_t s, xfk_problem *P)
{
    launch_pot_rows<MaskPhys>(s, P, MaskPhys::Args{P->mask_lv_p, P->mask_area_p});
}

__global__ void __launch_bounds__(kBlock) k_mask_threshold(int N, const double *__restrict__ W,
                                                           double *__restrict__ msk)
{
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i < N) msk[i] = (W[i] > 0.5) ? 1. : 0.;
}

// --- host side ---------------------------------------------------------------

hipError_t warm_module_mask()
{
    hipFuncAttributes a;
    return hipFuncGetAttributes(&a, reinterpret_cast<const void *>(&k_mask_threshold));
}

// The auxiliary problem of the mask, owned by P (P->mask_aux): the mesh's own
// connectivity p (a floating conductor's nodes stay apart), coordinates in
// user units, no boundary data at all -- the element eliminates the prescribed
// values itself.  lab: a table the length of the problem's labels (the mask's
// element reads none of it).  Created once and kept with P.
int mask_aux_create(xfk_problem *P, const std::vector<double> &x, const std::vector<double> &y,
                    const std::vector<int> &p, const std::vector<int> &lbl, const std::vector<PotLabel> &lab,
                    int length_units)
{
    if (P->mask_aux) return XFK_OK;
    const int N = P->N, NE = P->NE;
    GlobalPrep G;
    G.blk.assign(1, DevBlock{});
    G.lab.assign(1, DevLabel{});
    G.lin.assign(1, DevLine{});
    G.circ.assign(1, DevCirc{});
    G.hB.assign(1, 0.);
    G.hH.assign(1, 0.);
    G.hS.assign(1, 0.);
    G.ebits.assign(NE, 0);
    G.fixed.assign(N, 0);
    G.first.assign(N, 0.0);
    G.last = G.first;
    xfk_problem_desc md = {};
    md.n_nodes = N;
    md.x = x.data();
    md.y = y.data();
    md.n_elems = NE;
    md.p = p.data();
    md.lbl = lbl.data();
    md.n_blocks = 1;
    md.n_labels = (int)lab.size();
    md.precision = P->precision;
    md.length_units = length_units;
    md.relax = 1.0;
    md.problem_type = XFK_PLANAR;
    xfk_problem *Q = nullptr;
    int rc = build_local(&md, G, nullptr, P->device, nullptr, &Q);
    if (rc != XFK_OK) return rc;
    {
        ArenaScope arena_scope(&Q->arena);
        const std::vector<unsigned char> none(N, 0);
        hipError_t e = upload(Q->pot_p, p.data(), p.size(), Q->stream);
        if (e == hipSuccess) e = upload(Q->pot_labels, lab.data(), lab.size(), Q->stream);
        if (e == hipSuccess) e = upload(Q->pot_slave, none.data(), none.size(), Q->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(Q->stream);
        if (e != hipSuccess) {
            set_error(std::string("upload failed: ") + hipGetErrorString(e));
            xfk_problem_destroy(Q);
            return XFK_ERR_HIP;
        }
    }
    Q->mask = true;
    Q->pot_depth = 1;
    rc = reserve_first_solve(&Q);
    if (rc != XFK_OK) {
        xfk_problem_destroy(Q);
        return rc;
    }
    P->mask_aux = Q;
    return XFK_OK;
}

// The Laplace solve of the mask on P's auxiliary problem, from the fixed
// values in P->mask_lv and the labels' MaxArea in P->mask_area: symbolic phase
// (first call), row gather, AMG-PCG to the problem's Precision; then the
// threshold into P->mask_msk.  Host-synchronising.
int mask_aux_solve(xfk_problem *P, xfk_result *res)
{
    xfk_problem *Q = P->mask_aux;
    hipStream_t s = P->stream;
    const int N = P->N;
    Q->mask_lv_p = P->mask_lv.p;
    Q->mask_area_p = P->mask_area.p;
    Q->precision = P->precision;
    Q->precond = P->precond;
    int rc;
    {
        ArenaScope arena_scope(&Q->arena);
        rc = static2d_run(Q, 0, res);
        problem_recycle(Q);
    }
    if (rc != XFK_OK) return rc;
    k_mask_threshold<<<(N + kBlock - 1) / kBlock, kBlock, 0, s>>>(N, Q->V.p, P->mask_msk.p);
    XFK_CHECK(hipGetLastError());
    XFK_CHECK(hipStreamSynchronize(s));
    return XFK_OK;
}

// what xfk_pot_mask_info / xfk_mag_mask_info report of the last mask
void mask_set_info(xfk_problem *P, const xfk_result &res, double ms_create, double ms_rules, double ms_total)
{
    double *o = P->mask_info;
    o[0] = (double)res.cg_iters;
    o[1] = ms_create;
    o[2] = ms_rules;
    o[3] = res.ms_symbolic;
    o[4] = res.ms_assemble;
    o[5] = res.ms_amg_setup;
    o[6] = res.ms_solve;
    o[7] = ms_total;
}

// FindBoundaryEdges into ext[N] (zeroed here) for a mesh and its node -> element lists
int launch_mask_exterior(hipStream_t s, int N, int NE, const int *p, const int *n2e_ptr, const int *n2e,
                         unsigned char *ext)
{
    XFK_CHECK(hipMemsetAsync(ext, 0, (size_t)N, s));
    k_mask_exterior<<<(3 * NE + kBlock - 1) / kBlock, kBlock, 0, s>>>(NE, p, n2e_ptr, n2e, ext);
    XFK_CHECK(hipGetLastError());
    return XFK_OK;
}

// What the mask reads of the mesh alone, once per problem: the point marks and
// FindBoundaryEdges into P->mask_ext for the device mesh p and its lists
int mask_mesh_marks(xfk_problem *P, const int *p, const int *n2e_ptr, const int *n2e, const unsigned char *point)
{
    if (P->mask_ext_ready) return XFK_OK;
    hipStream_t s = P->stream;
    const int N = P->N, NE = P->NE;
    XFK_CHECK(upload(P->mask_point, point, (size_t)N, s));
    XFK_CHECK(P->mask_ext.alloc((size_t)N));
    const int rc = launch_mask_exterior(s, N, NE, p, n2e_ptr, n2e, P->mask_ext.p);
    if (rc == XFK_OK) P->mask_ext_ready = true;
    return rc;
}

int mask_make(xfk_problem *P, const MaskInputs &I)
{
    hipStream_t s = P->stream;
    const int N = P->N, NE = P->NE;
    // the fixed values and the validity of the selection
    XFK_CHECK(upload(P->mask_lflag, I.lflag, 2 * I.nentries, s));
    XFK_CHECK(upload(P->mask_area, I.area, I.nentries, s));
    if (I.nsel) XFK_CHECK(upload(P->mask_nsel, I.nsel, (size_t)N, s));
    int rc = mask_mesh_marks(P, I.p, I.n2e_ptr, I.n2e, I.point);   // (a no-op where the caller did it before)
    if (rc != XFK_OK) return rc;
    XFK_CHECK(P->mask_flag.alloc(2));
    XFK_CHECK(P->mask_lv.alloc((size_t)N));
    XFK_CHECK(P->mask_msk.alloc((size_t)N));
    XFK_CHECK(hipMemsetAsync(P->mask_flag.p, 0, 2 * sizeof(int), s));
    MaskRules A = {};
    A.x = I.x;
    A.p = I.p;
    A.lbl = I.lbl;
    A.n2e_ptr = I.n2e_ptr;
    A.n2e = I.n2e;
    A.lflag = P->mask_lflag.p;
    A.ext = P->mask_ext.p;
    A.point = P->mask_point.p;
    A.q = I.q;
    A.nsel = I.nsel ? P->mask_nsel.p : nullptr;
    A.axi = P->axi ? 1 : 0;
    const int GE = (NE + kBlock - 1) / kBlock, GN = (N + kBlock - 1) / kBlock;
    if (P->axi) k_mask_on_axis<<<A.nsel ? std::max(GE, GN) : GE, kBlock, 0, s>>>(NE, N, A, P->mask_flag.p);
    k_mask_fix<<<GN, kBlock, 0, s>>>(N, A, P->mask_flag.p, P->mask_lv.p);
    k_mask_valid<<<GE, kBlock, 0, s>>>(NE, A, P->mask_lv.p, P->mask_flag.p);
    XFK_CHECK(hipGetLastError());
    int flag[2] = {0, 0};
    XFK_CHECK(d2h(flag, P->mask_flag.p, sizeof(flag), s));   // (the stream is idle after this: the host tables were read)
    XFK_REQUIRE(!flag[1], XFK_ERR_ARG, I.invalid);
    const double ms_rules = wall_ms(I.t_rules);

    xfk_result res{};
    if ((rc = mask_aux_solve(P, &res)) != XFK_OK) return rc;
    P->mask_sel.assign(I.sel, I.sel + I.nsel_labels);
    P->mask_ready = true;
    mask_set_info(P, res, I.ms_create, ms_rules, wall_ms(I.t_all));
    return XFK_OK;
}

bool mask_matches(const xfk_problem *P, const unsigned char *sel, size_t n)
{
    if (!P->mask_ready || !sel || P->mask_sel.size() != n) return false;
    for (size_t k = 0; k < n; ++k)
        if ((P->mask_sel[k] != 0) != (sel[k] != 0)) return false;
    return true;
}

}  // namespace xfk
