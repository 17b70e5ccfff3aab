// What the scalar-potential problems share: electrostatics (xfk_electro.hip,
// the reference's esolver) and heat flow (xfk_heat.hip, hsolver) are the same
// first-order triangle problem -- a potential per node, conductors that fix it
// or carry a prescribed total source, fixed / mixed / source edges -- and
// differ in the element's coefficients.  Here, once: the row gather
// (k_pot_rows, the structure of xfk_device.hip's assemble_rows) with the
// element as its one hook, the merged-conductor kernels, the fixed-order sums
// of the conductor integrals, and the host build from a descriptor
// (validation, merged connectivity, edge fields, fixed values, point sources,
// conductor lists, uploads).  A problem type supplies a Phys struct (device:
// Args and element) and a traits struct (host: what its descriptor calls the
// fixed values, and how it scales the sources).
//
// A CircType 0 conductor (a prescribed total charge / heat flow) is one
// unknown.  The reference borders the system with one row per conductor and
// slaves every conductor node to it (esolver.cpp:568-585); here the
// conductor's nodes are merged onto its lowest-numbered node (the
// representative) in the connectivity the symbolic phase and the row gather
// see (xfk_problem::p_raw), so that node's row is the conductor's equation --
// the Galerkin projection of the element matrices onto "one value per
// conductor" -- and the merged-away nodes are identity rows that receive the
// representative's value after the solve.
#pragma once

#include "xfk_kernels.h"
#include "xfk_spmv.h"

#include <atomic>
#include <cmath>

namespace xfk {

constexpr int kPotRowBlock = 128;
constexpr int kPotRowAcc = 12;
constexpr int kPotQBlock = 256;   // the conductor integrals and their sums

// what the row gather reads and writes, whatever the physics
struct RowArgs {
    const double *x, *y;           // the solver's length unit (mm: esolver, m: hsolver)
    const int *pm;                 // merged connectivity: rows and columns
    const int *pg;                 // mesh connectivity: geometry and nodal values
    const int *lbl, *ebits;
    const int *n2e_ptr, *n2e, *rowptr, *col;
    const PotLabel *labels;
    const unsigned char *slave;    // merged-away node: identity row
    double *val, *b;
    int *miss;
    double depth;                  // planar
    double ext_ri, ext_ro, ext_zo;
};

__device__ __forceinline__ double pot_sqr(double v) { return v * v; }

// What both elements open with (esolver.cpp:448-470, hsolver.cpp:546-575), in
// the reference's operation order.  X is x (planar) or r (axisymmetric).
struct PotGeom {
    double l[3], p[3], q[3];
    double a, r;
    double Depth, kludge;   // kludge: the coefficient warp of the conformally mapped exterior region
};

template <bool AXI>
__device__ __forceinline__ void pot_geometry(const RowArgs &A, const double (&X)[3], const double (&Y)[3],
                                             const PotLabel &lab, PotGeom &G)
{
    G.p[0] = Y[1] - Y[2]; G.p[1] = Y[2] - Y[0]; G.p[2] = Y[0] - Y[1];
    G.q[0] = X[2] - X[1]; G.q[1] = X[0] - X[2]; G.q[2] = X[1] - X[0];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const int k = (j + 1) % 3;
        G.l[j] = sqrt(pot_sqr(X[k] - X[j]) + pot_sqr(Y[k] - Y[j]));
    }
    G.a = (G.p[0] * G.q[1] - G.p[1] * G.q[0]) / 2.;
    G.r = (X[0] + X[1] + X[2]) / 3.;
    G.Depth = A.depth;
    G.kludge = 1;
    if (AXI) {
        G.Depth = 2. * kPI * G.r;
        if (lab.external) {
            const double z = (Y[0] + Y[1] + Y[2]) / 3. - A.ext_zo;
            G.kludge = (G.r * G.r + z * z) / (A.ext_ri * A.ext_ro);
        }
    }
}

// (heat flow: the element of xfk_heat.hip and the post-processor of
// xfk_postproc.hip read the conductivities through this)
// CHMaterialProp::GetK (CMaterialProp.cpp:1388-1409): Kx in kx, Ky in ky.  A
// table gives both directions the same value: the first K at or below the
// first knot, the last at or above the last, else the FIRST interval with
// T[i] <= t <= T[i+1]; a t no rule catches (NaN, a table that is not
// ascending) falls through to Kx, Ky as the reference does.
__device__ __forceinline__ void hf_getk(const HfBlock &bp, const double *__restrict__ tkT,
                                        const double *__restrict__ tkK, double t, double &kx, double &ky)
{
    kx = bp.kx;
    ky = bp.ky;
    const int npts = bp.npts;
    if (npts == 0) return;
    const double *T = tkT + bp.off, *K = tkK + bp.off;
    if (npts == 1 || t <= T[0]) {
        kx = ky = K[0];
        return;
    }
    if (t >= T[npts - 1]) {
        kx = ky = K[npts - 1];
        return;
    }
    for (int i = 0, j = 1; j < npts; ++i, ++j)
        if (t >= T[i] && t <= T[j]) {
            kx = ky = K[i] + (K[j] - K[i]) * (t - T[i]) / (T[j] - T[i]);
            return;
        }
}

// Row gather: one thread per CSR row i sums the contributions of the elements
// incident on node i of the merged connectivity, in ascending element order --
// the order the reference's Put(Get() - Me) accumulates each entry in.  Rows
// of <= kPotRowAcc entries accumulate in LDS; longer ones (a merged
// conductor's row, periodic corners) in place in val, their columns found by
// bisection.  An element with two or three nodes on one merged conductor
// appears that many times in the representative's list (adjacent: the list is
// sorted) and is taken once, every one of its merged vertices contributing
// its row of Me.  No atomics, no colouring: every entry of val and b has one
// writer.
//
// Phys::element<AXI>(e, g, A, X, Xc, Yc, lab, Me, be) is one element of the
// reference's AnalyzeProblem: Me / be before the sign of the global assembly.
// It loads its own block, edge fields and nodal values (through g).
template <class Phys, bool AXI>
__global__ void __launch_bounds__(kPotRowBlock) k_pot_rows(int N, RowArgs A, typename Phys::Args X)
{
    __shared__ double s_acc[kPotRowAcc * kPotRowBlock];
    __shared__ int s_col[kPotRowAcc * kPotRowBlock];
    const int i0 = xcd_tile(blockIdx.x, gridDim.x) * kPotRowBlock;
    const int i = i0 + threadIdx.x;
    const bool live = i < N;   // (every thread reaches the barriers below)
    const int rs = live ? A.rowptr[i] : 0, L = live ? A.rowptr[i + 1] - rs : 0;
    const bool lds = L <= kPotRowAcc;
    double *acc = lds ? s_acc + threadIdx.x : A.val + rs;
    const int stride = lds ? kPotRowBlock : 1;
    const int *cols = lds ? s_col + threadIdx.x : A.col + rs;
    for (int k = 0; k < L; ++k) {
        acc[k * stride] = 0.;
        if (lds) s_col[k * kPotRowBlock + threadIdx.x] = A.col[rs + k];
    }
    // position of column c in the row (L >= 1: every row holds its diagonal)
    auto find = [&](int c) -> int {
        if (lds) {
            int pos = 0;
            while (pos < L - 1 && cols[pos * stride] != c) ++pos;
            return pos;
        }
        int lo = 0, hi = L - 1;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (cols[mid] < c) lo = mid + 1;
            else hi = mid;
        }
        return lo;
    };
    double bi = 0.;
    bool miss = false;
    const int t0 = live ? A.n2e_ptr[i] : 0, t1 = live ? A.n2e_ptr[i + 1] : 0;
    int e_prev = -1;
    for (int t = t0; t < t1; ++t) {
        const int e = A.n2e[t];
        if (e == e_prev) continue;
        e_prev = e;
        const int n[3] = {A.pm[3 * e], A.pm[3 * e + 1], A.pm[3 * e + 2]};
        const int g[3] = {A.pg[3 * e], A.pg[3 * e + 1], A.pg[3 * e + 2]};
        const PotLabel lab = A.labels[A.lbl[e]];
        const double Xc[3] = {A.x[g[0]], A.x[g[1]], A.x[g[2]]};
        const double Yc[3] = {A.y[g[0]], A.y[g[1]], A.y[g[2]]};
        double Me[3][3], be[3];
        Phys::template element<AXI>(e, g, A, X, Xc, Yc, lab, Me, be);
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            if (n[j] != i) continue;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const int pos = find(n[k]);
                miss |= cols[pos * stride] != n[k];
                acc[pos * stride] -= Me[j][k];
            }
            bi -= be[j];
        }
    }
    if (live && A.slave[i]) acc[find(i) * stride] = 1.;   // merged-away node: 0 until the copy after the solve
    if (miss && A.miss) *A.miss = 1;
    // (as assemble_rows: a block whose rows all sat in LDS writes its run of
    // val with consecutive lanes on consecutive entries)
    if (__syncthreads_and(lds)) {
        double r[kPotRowAcc];
#pragma unroll
        for (int k = 0; k < kPotRowAcc; ++k) r[k] = k < L ? s_acc[k * kPotRowBlock + threadIdx.x] : 0.;
        const int rb0 = A.rowptr[min(i0, N)], rb1 = A.rowptr[min(i0 + kPotRowBlock, N)];
        __syncthreads();
#pragma unroll
        for (int k = 0; k < kPotRowAcc; ++k)
            if (k < L) s_acc[rs - rb0 + k] = r[k];
        __syncthreads();
        for (int m = threadIdx.x; m < rb1 - rb0; m += kPotRowBlock) A.val[rb0 + m] = s_acc[m];
    } else if (lds) {
        for (int k = 0; k < L; ++k) A.val[rs + k] = s_acc[k * kPotRowBlock + threadIdx.x];
    }
    if (live) A.b[i] = bi;
}

// the row gather of problem P with the physics' own arguments X (writes every
// entry of val and b)
template <class Phys>
void launch_pot_rows(hipStream_t s, xfk_problem *P, const typename Phys::Args &X)
{
    const int N = P->NR;
    if (N <= 0) return;
    RowArgs A = {};
    A.x = P->x.p;
    A.y = P->y.p;
    A.pm = P->p_raw.p;
    A.pg = P->pot_p.p;
    A.lbl = P->lbl_raw.p;
    A.ebits = P->ebits_raw.p;
    A.n2e_ptr = P->n2e_ptr.p;
    A.n2e = P->n2e.p;
    A.rowptr = P->rowptr.p;
    A.col = P->col.p;
    A.labels = P->pot_labels.p;
    A.slave = P->pot_slave.p;
    A.val = P->val.p;
    A.b = P->b.p;
    A.miss = P->asm_miss.p;
    A.depth = P->pot_depth;
    A.ext_ri = P->ext_ri;
    A.ext_ro = P->ext_ro;
    A.ext_zo = P->ext_zo;
    const int g = (N + kPotRowBlock - 1) / kPotRowBlock;
    if (P->axi) k_pot_rows<Phys, true><<<g, kPotRowBlock, 0, s>>>(N, A, X);
    else k_pot_rows<Phys, false><<<g, kPotRowBlock, 0, s>>>(N, A, X);
}

// merged-away nodes take their conductor's value (bit-equal), or zero (their
// identity rows' solution: the value a warm-started PCG expects)
// (static: a copy per translation unit that includes this header)
static __global__ void k_pot_set_slaves(int n, const int *__restrict__ node, const int *__restrict__ rep, int zero,
                                        double *__restrict__ V)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < n) V[node[t]] = zero ? 0. : V[rep[t]];
}

static inline void launch_pot_set_slaves(xfk_problem *P, int zero)
{
    const int ns = P->pot_nslave;
    if (ns)
        k_pot_set_slaves<<<(ns + kBlock - 1) / kBlock, kBlock, 0, P->stream>>>(ns, P->pot_slave_node.p,
                                                                               P->pot_slave_rep.p, zero, P->V.p);
}

// the workgroup's K sums of v (wave shuffles, then the waves in order) into
// out[K wg .. K wg + K); workgroups of kPotQBlock threads
template <int K>
__device__ __forceinline__ void block_sums(const double (&v)[K], double *__restrict__ out)
{
    __shared__ double red[K * (kPotQBlock / 64)];
    double a[K];
#pragma unroll
    for (int c = 0; c < K; ++c) a[c] = cg_wave_sum(v[c]);
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int c = 0; c < K; ++c) red[K * (threadIdx.x >> 6) + c] = a[c];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double s[K];
#pragma unroll
        for (int c = 0; c < K; ++c) s[c] = 0.;
        for (int w = 0; w < kPotQBlock / 64; ++w) {
#pragma unroll
            for (int c = 0; c < K; ++c) s[c] += red[K * w + c];
        }
#pragma unroll
        for (int c = 0; c < K; ++c) out[K * blockIdx.x + c] = s[c];
    }
}

// G workgroups' K partials each in a fixed order: strided per thread, then
// the workgroup's sums; out[0 .. K) = the sums (one workgroup)
template <int K>
__global__ void __launch_bounds__(kPotQBlock) k_pot_sum(int G, const double *__restrict__ part,
                                                        double *__restrict__ out)
{
    double s[K];
#pragma unroll
    for (int c = 0; c < K; ++c) s[c] = 0.;
    for (int i = threadIdx.x; i < G; i += kPotQBlock) {
#pragma unroll
        for (int c = 0; c < K; ++c) s[c] += part[K * i + c];
    }
    block_sums<K>(s, out);
}

// The integral of conductor c over the elements touching one of its nodes,
// into *q_host (host-synchronising).  launch(G, n, els, part) starts the
// physics' kernel: G workgroups of kPotQBlock threads, one element of
// els[0 .. n) per thread, K partials per workgroup into part, of which the
// first is the integral's.  buf holds the largest conductor's partials and
// K sums.
template <int K, class Launch>
int conductor_integral(xfk_problem *P, int c, double *buf, double *q_host, Launch launch)
{
    hipStream_t s = P->stream;
    const int e0 = P->pot_cel_ptr[c], n = P->pot_cel_ptr[c + 1] - e0;
    if (n == 0) {
        *q_host = 0.;
        return XFK_OK;
    }
    const int G = (n + kPotQBlock - 1) / kPotQBlock;
    double *out = buf + K * G;
    launch(G, n, P->pot_cel.p + e0, buf);
    k_pot_sum<K><<<1, kPotQBlock, 0, s>>>(G, buf, out);
    XFK_CHECK(hipGetLastError());
    XFK_CHECK(d2h(q_host, out, sizeof(double), s));
    return XFK_OK;
}

// ---------------------------------------------------------------------------
// Host build.  Desc is xfk_es_problem_desc or xfk_hf_problem_desc: the same
// fields under the same names, apart from what Traits names.
// ---------------------------------------------------------------------------

// the checks both descriptors share; conductor_words: what CircType 0 and 1
// prescribe, as the message says it
template <class Desc>
int validate_potential(const Desc *d, const char *conductor_words)
{
    XFK_REQUIRE(d->n_nodes > 0 && d->n_elems > 0, XFK_ERR_ARG, "empty mesh");
    XFK_REQUIRE(d->x && d->y && d->p && d->lbl, XFK_ERR_ARG, "missing mesh arrays");
    XFK_REQUIRE(d->n_blocks > 0 && d->blocks && d->n_labels > 0 && d->labels, XFK_ERR_ARG,
                "missing block or label tables");
    XFK_REQUIRE(d->n_lines >= 0 && (d->n_lines == 0 || d->lines), XFK_ERR_ARG, "missing boundary table");
    XFK_REQUIRE(d->n_points >= 0 && (d->n_points == 0 || d->points), XFK_ERR_ARG, "missing point table");
    XFK_REQUIRE(d->n_conductors >= 0 && (d->n_conductors == 0 || d->conductors), XFK_ERR_ARG,
                "missing conductor table");
    XFK_REQUIRE(d->n_pbc >= 0 && (d->n_pbc == 0 || d->pbc), XFK_ERR_ARG, "missing pbc table");
    XFK_REQUIRE(d->length_units >= 0 && d->length_units < 6, XFK_ERR_ARG, "bad length units");
    XFK_REQUIRE(d->problem_type == XFK_PLANAR || d->problem_type == XFK_AXISYMMETRIC, XFK_ERR_ARG,
                "problem type must be planar or axisymmetric");
    XFK_REQUIRE(d->problem_type == XFK_AXISYMMETRIC || d->depth > 0, XFK_ERR_ARG,
                "depth must be positive on a planar problem");
    const int N = d->n_nodes, NE = d->n_elems, NLB = d->n_labels;
    std::atomic<int> bad{0};
    host_par_for(NE, 1 << 17, [&](long long a, long long b) {
        bool okp = true, okl = true, oke = true;
        for (long long k = 3 * a; k < 3 * b; ++k) okp &= (unsigned)d->p[k] < (unsigned)N;
        for (long long i = a; i < b; ++i) okl &= (unsigned)d->lbl[i] < (unsigned)NLB;
        if (d->e)
            for (long long k = 3 * a; k < 3 * b; ++k) oke &= d->e[k] >= -1 && d->e[k] < d->n_lines;
        if (!okp || !okl || !oke) bad |= (okp ? 0 : 1) | (okl ? 0 : 2) | (oke ? 0 : 4);
    });
    XFK_REQUIRE(!(bad & 1), XFK_ERR_ARG, "element node index out of range");
    XFK_REQUIRE(!(bad & 2), XFK_ERR_ARG, "element label out of range");
    XFK_REQUIRE(!(bad & 4), XFK_ERR_ARG, "edge boundary-property index out of range");
    for (int k = 0; k < d->n_labels; ++k) {
        XFK_REQUIRE(d->labels[k].block >= 0 && d->labels[k].block < d->n_blocks, XFK_ERR_ARG,
                    "label block index out of range");
        XFK_REQUIRE(!(d->problem_type == XFK_AXISYMMETRIC && d->labels[k].is_external) ||
                        (d->ext_ro > 0 && d->ext_ri > 0),
                    XFK_ERR_ARG, "exterior region needs [extRo] > 0 and [extRi] > 0");
    }
    for (int k = 0; k < d->n_conductors; ++k)
        XFK_REQUIRE(d->conductors[k].type == 0 || d->conductors[k].type == 1, XFK_ERR_ARG,
                    std::string("conductor type must be ") + conductor_words);
    for (int i = 0; i < N; ++i) {
        XFK_REQUIRE(!d->marker || (d->marker[i] >= -1 && d->marker[i] < d->n_points), XFK_ERR_ARG,
                    "node point-property index out of range");
        XFK_REQUIRE(!d->conductor || (d->conductor[i] >= -1 && d->conductor[i] < d->n_conductors), XFK_ERR_ARG,
                    "node conductor index out of range");
    }
    for (int k = 0; k < d->n_pbc; ++k)
        for (int m = 0; m < 2; ++m)
            XFK_REQUIRE((unsigned)d->pbc[3 * k + m] < (unsigned)N, XFK_ERR_ARG, "pbc node index out of range");
    auto floating = [&](int i) {
        return d->conductor && d->conductor[i] >= 0 && d->conductors[d->conductor[i]].type == 0;
    };
    for (int i = 0; i < N; ++i)
        XFK_REQUIRE(!(floating(i) && d->marker && d->marker[i] >= 0), XFK_ERR_ARG,
                    "point property on a node of a floating conductor");
    if (d->e && d->conductor)
        for (long long i = 0; i < NE; ++i)
            for (int j = 0; j < 3; ++j) {
                const int ej = d->e[3 * i + j];
                if (ej < 0 || d->lines[ej].format != 0) continue;
                XFK_REQUIRE(!floating(d->p[3 * i + j]) && !floating(d->p[3 * i + (j + 1) % 3]), XFK_ERR_ARG,
                            "node of a floating conductor is fixed by a boundary property");
            }
    for (int k = 0; k < d->n_pbc; ++k)
        XFK_REQUIRE(!floating(d->pbc[3 * k]) && !floating(d->pbc[3 * k + 1]), XFK_ERR_UNSUPPORTED,
                    "periodic pair on a node of a floating conductor");
    if (d->e) {   // the packed edge fields index the properties the mesh uses
        std::vector<char> used(std::max(1, d->n_lines), 0);
        for (long long k = 0; k < 3LL * NE; ++k)
            if (d->e[k] >= 0) used[d->e[k]] = 1;
        long long nused = 0;
        for (char u : used) nused += u;
        XFK_REQUIRE(nused <= 1022, XFK_ERR_UNSUPPORTED, "at most 1022 distinct boundary properties on element edges");
    }
    return XFK_OK;
}

// what a create function derives from its descriptor before the device is touched
struct PotentialPrep {
    GlobalPrep G;                         // what the shared build (build_local) reads: boundary data in its form
    xfk_problem_desc md = {};             // ... and the mesh under the merged connectivity
    double depth = 0;                     // [Depth] in the solver's length unit
    double unit = 1;                      // user length units -> the solver's
    std::vector<int> rep;                 // conductor -> representative node (CircType 0 with nodes), else -1
    std::vector<int> pm;                  // merged connectivity
    std::vector<unsigned char> slave;     // per node: merged away
    std::vector<int> slave_node, slave_rep;
    std::vector<int> lin_used;            // boundary properties used on edges, ascending: the compact line table
    std::vector<int> cel_ptr, cel;        // conductor -> the elements touching one of its nodes, ascending
    std::vector<int> ncond;               // per node: conductor or -1
    std::vector<int> qmark;               // per node: L.Q as the reference writes it (the post-processor's smoothing)
    int qmax = 0;                         // the longest of those lists
};

// Traits: point_value(point), conductor_value(conductor), line_value(line) --
// the fixed value each prescribes; point_source(Depth, qp) and
// conductor_source(q) -- the right-hand side of a point source and of a
// CircType 0 conductor's row.  u: user length units -> the solver's.
template <class Traits, class Desc>
void prepare_potential(const Desc *d, double u, PotentialPrep &R)
{
    const int N = d->n_nodes, NE = d->n_elems, NC = d->n_conductors;
    const bool axi = d->problem_type == XFK_AXISYMMETRIC;
    R.depth = d->depth * u;
    R.unit = u;
    auto marker = [&](int i) { return d->marker ? d->marker[i] : -1; };
    auto cond = [&](int i) { return d->conductor ? d->conductor[i] : -1; };
    auto floating = [&](int c) { return c >= 0 && d->conductors[c].type == 0; };

    GlobalPrep &G = R.G;
    G.axi = axi;
    G.ext_ro = d->ext_ro * u;
    G.ext_ri = d->ext_ri * u;
    G.ext_zo = d->ext_zo * u;
    G.blk.assign(1, DevBlock{});
    G.lab.assign(1, DevLabel{});
    G.lin.assign(1, DevLine{});
    G.circ.assign(1, DevCirc{});
    G.hB.assign(1, 0.);
    G.hH.assign(1, 0.);
    G.hS.assign(1, 0.);

    // floating conductors: representative = lowest-numbered node
    R.rep.assign(std::max(1, NC), -1);
    R.ncond.resize(N);
    for (int i = 0; i < N; ++i) {
        const int c = R.ncond[i] = cond(i);
        if (floating(c) && R.rep[c] < 0) R.rep[c] = i;
    }
    R.pm.assign(d->p, d->p + 3LL * NE);
    R.slave.assign(N, 0);
    for (int i = 0; i < N; ++i) {
        const int c = cond(i);
        if (floating(c) && R.rep[c] != i) {
            R.slave[i] = 1;
            R.slave_node.push_back(i);
            R.slave_rep.push_back(R.rep[c]);
        }
    }
    if (!R.slave_node.empty())
        for (long long k = 0; k < 3LL * NE; ++k) {
            const int c = cond(R.pm[k]);
            if (floating(c)) R.pm[k] = R.rep[c];
        }

    // boundary properties used on edges, compacted into the 10-bit edge fields
    G.ebits.assign(NE, 0);
    if (d->e) {
        std::vector<int> lmap(std::max(1, d->n_lines), -1);
        std::vector<char> used(std::max(1, d->n_lines), 0);
        for (long long k = 0; k < 3LL * NE; ++k)
            if (d->e[k] >= 0) used[d->e[k]] = 1;
        for (int k = 0; k < d->n_lines; ++k)
            if (used[k]) {
                lmap[k] = (int)R.lin_used.size();
                R.lin_used.push_back(k);
            }
        for (long long i = 0; i < NE; ++i) {
            unsigned bits = 0;
            for (int j = 0; j < 3; ++j)
                if (d->e[3 * i + j] >= 0) bits |= (unsigned)(lmap[d->e[3 * i + j]] + 1) << (10 * j);
            G.ebits[i] = (int)bits;
        }
    }

    // fixed values (esolver.cpp:410-444, hsolver.cpp:499-533): point
    // properties with qp == 0, the nodes of CircType 1 conductors, both ends
    // of BdryFormat 0 edges in element order -- the last assignment is the
    // node's value
    G.fixed.assign(N, 0);
    G.first.assign(N, 0.0);
    for (int i = 0; i < N; ++i) {
        const int m = marker(i), c = cond(i);
        if (m >= 0 && d->points[m].qp == 0) {
            G.first[i] = Traits::point_value(d->points[m]);
            G.fixed[i] = 1;
        }
        if (c >= 0 && d->conductors[c].type == 1) {
            G.first[i] = Traits::conductor_value(d->conductors[c]);
            G.fixed[i] = 1;
        }
    }
    if (d->e)
        for (long long i = 0; i < NE; ++i)
            for (int j = 0; j < 3; ++j) {
                const int ej = d->e[3 * i + j];
                if (ej < 0 || d->lines[ej].format != 0) continue;
                for (int v : {d->p[3 * i + j], d->p[3 * i + (j + 1) % 3]}) {
                    G.first[v] = Traits::line_value(d->lines[ej]);
                    G.fixed[v] = 1;
                }
            }
    G.last = G.first;
    // L.Q as the solution file carries it (esolver.cpp:412-440, 592-600;
    // hsolver.cpp:501-529, 766-774): a conductor's index on its nodes whatever
    // its type, else -1 on a node with a point property (fixed by it, or marked
    // when its point source is added) or on a BdryFormat 0 edge, else -2
    R.qmark.resize(N);
    for (int i = 0; i < N; ++i) R.qmark[i] = cond(i) >= 0 ? cond(i) : (marker(i) >= 0 || G.fixed[i]) ? -1 : -2;

    // point sources on free nodes (esolver.cpp:590-597, hsolver.cpp:764-771),
    // and the source of a floating conductor on its row (esolver.cpp:628,
    // hsolver.cpp:802), through the point-source launch
    for (int i = 0; i < N; ++i) {
        const int m = marker(i);
        if (m < 0 || G.fixed[i]) continue;
        const double Depth = axi ? 2. * kPI * d->x[i] : R.depth;
        G.pt_nodes.push_back(i);
        G.pt_J.push_back(Traits::point_source(Depth, d->points[m].qp));
    }
    for (int c = 0; c < NC; ++c)
        if (R.rep[c] >= 0) {
            G.pt_nodes.push_back(R.rep[c]);
            G.pt_J.push_back(Traits::conductor_source(d->conductors[c].q));
        }

    // elements touching a node of each conductor, ascending (ChargeOnConductor)
    R.cel_ptr.assign(NC + 1, 0);
    if (NC > 0 && d->conductor) {
        std::vector<std::vector<int>> per(NC);
        for (int i = 0; i < NE; ++i) {
            const int c0 = cond(d->p[3LL * i]), c1 = cond(d->p[3LL * i + 1]), c2 = cond(d->p[3LL * i + 2]);
            if (c0 >= 0) per[c0].push_back(i);
            if (c1 >= 0 && c1 != c0) per[c1].push_back(i);
            if (c2 >= 0 && c2 != c0 && c2 != c1) per[c2].push_back(i);
        }
        for (int c = 0; c < NC; ++c) {
            R.cel.insert(R.cel.end(), per[c].begin(), per[c].end());
            R.cel_ptr[c + 1] = (int)R.cel.size();
        }
    }
    for (int c = 0; c < NC; ++c) R.qmax = std::max(R.qmax, R.cel_ptr[c + 1] - R.cel_ptr[c]);

    xfk_problem_desc &md = R.md;
    md.n_nodes = N;
    md.x = d->x;
    md.y = d->y;
    md.n_elems = NE;
    md.p = R.pm.data();
    md.lbl = d->lbl;
    md.n_blocks = d->n_blocks;
    md.n_labels = d->n_labels;
    md.n_lines = d->n_lines;
    md.n_pbc = d->n_pbc;
    md.pbc = d->pbc;
    md.precision = d->precision;
    md.length_units = d->length_units;
    md.relax = 1.0;
    md.problem_type = d->problem_type;
}

// the compact line table: make(line) for every property an edge uses (one
// default entry when none does, so the buffer is never empty)
template <class Line, class Desc, class Make>
std::vector<Line> potential_lines(const Desc *d, const PotentialPrep &R, Make make)
{
    std::vector<Line> lin;
    for (int k : R.lin_used) lin.push_back(make(d->lines[k]));
    if (lin.empty()) lin.push_back(Line{});
    return lin;
}

// the uploads and host fields every potential problem has (the pot_* group of
// xfk_problem); ordered on P's stream, not synchronised
template <class Desc>
hipError_t upload_potential_common(xfk_problem *P, const PotentialPrep &R, const Desc *d)
{
    const int NC = d->n_conductors;
    P->pot_depth = R.depth;
    P->pot_cond_rep.assign(R.rep.begin(), R.rep.begin() + NC);
    P->pot_cel_ptr = R.cel_ptr;
    P->pot_nslave = (int)R.slave_node.size();
    P->pot_qmark = R.qmark;
    P->pot_has_point.assign(d->n_nodes, 0);
    if (d->marker)
        for (int i = 0; i < d->n_nodes; ++i) P->pot_has_point[i] = d->marker[i] >= 0;
    P->pot_length_units = d->length_units;
    P->pot_unit = R.unit;
    P->pot_depth_user = d->depth;
    P->pot_ext_user[0] = d->ext_ro;
    P->pot_ext_user[1] = d->ext_ri;
    P->pot_ext_user[2] = d->ext_zo;
    std::vector<PotLabel> lab(d->n_labels);
    for (int k = 0; k < d->n_labels; ++k) lab[k] = PotLabel{d->labels[k].block, d->labels[k].is_external ? 1 : 0};
    hipStream_t s = P->stream;
    hipError_t e = upload(P->pot_p, d->p, 3 * (size_t)d->n_elems, s);
    if (e == hipSuccess) e = upload(P->pot_labels, lab.data(), lab.size(), s);
    if (e == hipSuccess) e = upload(P->pot_slave, R.slave.data(), R.slave.size(), s);
    if (e == hipSuccess) e = upload(P->pot_slave_node, R.slave_node.data(), R.slave_node.size(), s);
    if (e == hipSuccess) e = upload(P->pot_slave_rep, R.slave_rep.data(), R.slave_rep.size(), s);
    if (e == hipSuccess) e = upload(P->pot_cel, R.cel.data(), R.cel.size(), s);
    if (e == hipSuccess) e = upload(P->pot_node_cond, R.ncond.data(), R.ncond.size(), s);
    return e;
}

// The device problem of a prepared descriptor: the shared build, the common
// uploads, then own(P, s) -- the physics' host fields, tables and buffers,
// ordered on s -- and the first solve's reservation.  A failure destroys the
// problem.
template <class Desc, class Own>
int create_potential(const Desc *d, const PotentialPrep &R, int device, xfk_problem **out, Own own)
{
    int rc = build_local(&R.md, R.G, nullptr, device, nullptr, out);
    if (rc != XFK_OK) return rc;
    xfk_problem *P = *out;
    {
        ArenaScope arena_scope(&P->arena);
        hipError_t e = upload_potential_common(P, R, d);
        if (e == hipSuccess) e = own(P, P->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(P->stream);
        if (e != hipSuccess) {
            set_error(std::string("upload failed: ") + hipGetErrorString(e));
            xfk_problem_destroy(P);
            *out = nullptr;
            return XFK_ERR_HIP;
        }
    }
    return reserve_first_solve(out);
}

// Per conductor after a solve: the prescribed (CircType 1) or solved
// (CircType 0) value and the integrated (CircType 1) or prescribed (CircType
// 0) source.  Either array may be null.
template <class Traits, class Cond>
int get_conductor_values(xfk_problem *P, const std::vector<Cond> &table, double *V, double *q)
{
    XFK_CHECK(hipSetDevice(P->device));
    for (int c = 0; c < (int)table.size(); ++c) {
        if (q) q[c] = table[c].q;
        if (!V) continue;
        V[c] = Traits::conductor_value(table[c]);
        if (table[c].type == 0) {
            V[c] = 0.;   // (a conductor without nodes: the reference's placeholder row)
            if (P->pot_cond_rep[c] >= 0)
                XFK_CHECK(d2h(&V[c], P->V.p + P->pot_cond_rep[c], sizeof(double), P->stream));
        }
    }
    return XFK_OK;
}

}  // namespace xfk
