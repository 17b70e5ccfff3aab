// Electrostatic problems on the device: ESolver::AnalyzeProblem
// (reference cfemm/esolver/esolver.cpp:389-646) and ESolver::ChargeOnConductor
// (esolver.cpp:797-844) for MI355X (gfx950).
//
// What is new here: the electrostatic element with its boundary terms inside
// a row gather of its own (k_es_rows, the structure of xfk_device.hip's
// assemble_rows), the conductor tables, the charge integral and the C-ABI
// entry points.  Everything else is the static magnetics path unchanged: the
// symbolic phase, the point-source launch (point charges, and the charge of a
// floating conductor on its row), the Dirichlet kernels (point properties
// with qp == 0, prescribed-voltage conductors, BdryFormat 0 edges), the
// (anti)periodic averaging map and the AMG-PCG (static2d_run, one pass).
//
// A floating conductor (CircType 0) is one unknown.  The reference borders the
// system with one row per conductor and slaves every conductor node to it
// (esolver.cpp:568-585); here the conductor's nodes are merged onto its
// lowest-numbered node (the representative) in the connectivity the symbolic
// phase and the row gather see (xfk_problem::p_raw), so that node's row is the
// conductor's equation -- the Galerkin projection of the element matrices
// onto "one value per conductor" -- and the merged-away nodes are identity
// rows that receive the representative's value after the solve.
#include "xfk_kernels.h"
#include "xfk_spmv.h"

#include <atomic>
#include <cmath>

namespace xfk {

constexpr double kEo = 8.85418781762e-12;   // femmconstants.h:24
constexpr double kEsC = (1.e-6) / kEo;       // esolver.cpp:398

struct EsArgs {
    const double *x, *y;           // mm
    const int *pm;                 // merged connectivity: rows and columns
    const int *pg;                 // mesh connectivity: geometry
    const int *lbl, *ebits;
    const int *n2e_ptr, *n2e, *rowptr, *col;
    const EsLabel *labels;
    const EsBlock *blocks;
    const EsLine *lines;
    const unsigned char *slave;    // merged-away node: identity row
    double *val, *b;
    int *miss;
    double depth;                  // mm (planar)
    double ext_ri, ext_ro, ext_zo; // mm
};

__device__ __forceinline__ double es_sqr(double v) { return v * v; }

// One element of ESolver::AnalyzeProblem (esolver.cpp:448-548), in the
// reference's operation order: Me / be before the sign of the global assembly.
// X is x (planar) or r (axisymmetric), in mm; eb the element's three packed
// 10-bit boundary-property fields.
template <bool AXI>
__device__ __forceinline__ void es_element(int eb, const EsArgs &A, const double (&X)[3], const double (&Y)[3],
                                           const EsLabel &lab, const EsBlock &bp, double (&Me)[3][3], double (&be)[3])
{
    double l[3], p[3], q[3];
    p[0] = Y[1] - Y[2]; p[1] = Y[2] - Y[0]; p[2] = Y[0] - Y[1];
    q[0] = X[2] - X[1]; q[1] = X[0] - X[2]; q[2] = X[1] - X[0];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const int k = (j + 1) % 3;
        l[j] = sqrt(es_sqr(X[k] - X[j]) + es_sqr(Y[k] - Y[j]));
    }
    const double a = (p[0] * q[1] - p[1] * q[0]) / 2.;
    const double r = (X[0] + X[1] + X[2]) / 3.;
    double Depth = A.depth, kludge = 1;
    if (AXI) {
        Depth = 2. * kPI * r;
        // the permittivity warp of the conformally mapped exterior region
        if (lab.external) {
            const double z = (Y[0] + Y[1] + Y[2]) / 3. - A.ext_zo;
            kludge = (r * r + z * z) / (A.ext_ri * A.ext_ro);
        }
    }
    // x- and y-contributions (upper values mirrored: exact symmetry)
    const double Kx = -Depth * bp.ex / (4. * a) / kludge;
    const double Ky = -Depth * bp.ey / (4. * a) / kludge;
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
        for (int k = j; k < 3; ++k) {
            double m = Kx * p[j] * p[k];
            m += Ky * q[j] * q[k];
            Me[j][k] = m;
            Me[k][j] = m;
        }
    // volume charge density
    const double Kv = -Depth * kEsC * (bp.qv) * a / 3.;
    be[0] = Kv; be[1] = Kv; be[2] = Kv;
    if (eb) {
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const int ej = ((eb >> (10 * j)) & 1023) - 1;
            if (ej < 0) continue;
            const int k = (j + 1) % 3;
            if (AXI) Depth = kPI * (X[j] + X[k]);
            const EsLine ln = A.lines[ej];
            if (ln.format == 1) {   // mixed boundary condition
                double K = -1000. * Depth * kEsC * ln.c0 * l[j] / 6.;
                // (selected without dynamic register indexing)
#pragma unroll
                for (int u = 0; u < 3; ++u)
#pragma unroll
                    for (int v = 0; v < 3; ++v) {
                        const bool on = (u == j || u == k) && (v == j || v == k);
                        if (on) Me[u][v] += (u == v) ? K * 2. : K;
                    }
                K = 1000. * Depth * kEsC * ln.c1 * l[j] / 2.;
#pragma unroll
                for (int u = 0; u < 3; ++u)
                    if (u == j || u == k) be[u] += K;
            }
            if (ln.format == 2) {   // surface charge density
                const double K = -1000. * Depth * kEsC * ln.qs * l[j] / 2.;
#pragma unroll
                for (int u = 0; u < 3; ++u)
                    if (u == j || u == k) be[u] += K;
            }
        }
    }
}

// Row gather (the structure of xfk_device.hip's assemble_rows): one thread
// per CSR row i sums the contributions of the elements incident on node i of
// the merged connectivity, in ascending element order -- the order the
// reference's Put(Get() - Me) accumulates each entry in.  Rows of <= kEsRowAcc
// entries accumulate in LDS; longer ones (a floating conductor's row, periodic
// corners) in place in val, their columns found by bisection.  An element
// with two or three nodes on one floating conductor appears that many times
// in the representative's list (adjacent: the list is sorted) and is taken
// once, every one of its merged vertices contributing its row of Me.
constexpr int kEsRowBlock = 128;
constexpr int kEsRowAcc = 12;

template <bool AXI>
__global__ void __launch_bounds__(kEsRowBlock) k_es_rows(int N, EsArgs A)
{
    __shared__ double s_acc[kEsRowAcc * kEsRowBlock];
    __shared__ int s_col[kEsRowAcc * kEsRowBlock];
    const int i0 = xcd_tile(blockIdx.x, gridDim.x) * kEsRowBlock;
    const int i = i0 + threadIdx.x;
    const bool live = i < N;   // (every thread reaches the barriers below)
    const int rs = live ? A.rowptr[i] : 0, L = live ? A.rowptr[i + 1] - rs : 0;
    const bool lds = L <= kEsRowAcc;
    double *acc = lds ? s_acc + threadIdx.x : A.val + rs;
    const int stride = lds ? kEsRowBlock : 1;
    const int *cols = lds ? s_col + threadIdx.x : A.col + rs;
    for (int k = 0; k < L; ++k) {
        acc[k * stride] = 0.;
        if (lds) s_col[k * kEsRowBlock + threadIdx.x] = A.col[rs + k];
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
        const EsLabel lab = A.labels[A.lbl[e]];
        const EsBlock bp = A.blocks[lab.blk];
        const double X[3] = {A.x[g[0]], A.x[g[1]], A.x[g[2]]};
        const double Y[3] = {A.y[g[0]], A.y[g[1]], A.y[g[2]]};
        double Me[3][3], be[3];
        es_element<AXI>(A.ebits[e], A, X, Y, lab, bp, Me, be);
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
    if (live && A.slave[i]) acc[find(i) * stride] = 1.;   // merged-away node: V_i = 0 until the copy after the solve
    if (miss && A.miss) *A.miss = 1;
    // (as assemble_rows: a block whose rows all sat in LDS writes its run of
    // val with consecutive lanes on consecutive entries)
    if (__syncthreads_and(lds)) {
        double r[kEsRowAcc];
#pragma unroll
        for (int k = 0; k < kEsRowAcc; ++k) r[k] = k < L ? s_acc[k * kEsRowBlock + threadIdx.x] : 0.;
        const int rb0 = A.rowptr[min(i0, N)], rb1 = A.rowptr[min(i0 + kEsRowBlock, N)];
        __syncthreads();
#pragma unroll
        for (int k = 0; k < kEsRowAcc; ++k)
            if (k < L) s_acc[rs - rb0 + k] = r[k];
        __syncthreads();
        for (int m = threadIdx.x; m < rb1 - rb0; m += kEsRowBlock) A.val[rb0 + m] = s_acc[m];
    } else if (lds) {
        for (int k = 0; k < L; ++k) A.val[rs + k] = s_acc[k * kEsRowBlock + threadIdx.x];
    }
    if (live) A.b[i] = bi;
}

// merged-away nodes take their conductor's potential (bit-equal)
__global__ void k_es_copy_slaves(int n, const int *__restrict__ node, const int *__restrict__ rep,
                                 double *__restrict__ V)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < n) V[node[t]] = V[rep[t]];
}

// ESolver::ChargeOnConductor (esolver.cpp:797-844) over the elements touching
// a node of the conductor (els[0 .. n), ascending): one element per thread,
// the workgroup's sum (wave shuffles, then the waves in order) into part[wg]
constexpr int kEsQBlock = 256;

__global__ void __launch_bounds__(kEsQBlock) k_es_charge(int n, const int *__restrict__ els, int conductor,
                                                         const int *__restrict__ pg, const int *__restrict__ lbl,
                                                         const EsLabel *__restrict__ labels,
                                                         const EsBlock *__restrict__ blocks,
                                                         const double *__restrict__ x, const double *__restrict__ y,
                                                         const double *__restrict__ V,
                                                         const int *__restrict__ node_cond, int axi, double depth,
                                                         double *__restrict__ part)
{
    __shared__ double red[kEsQBlock / 64];
    const int t = blockIdx.x * kEsQBlock + threadIdx.x;
    double Z = 0.;
    if (t < n) {
        const int e = els[t];
        const int g[3] = {pg[3 * e], pg[3 * e + 1], pg[3 * e + 2]};
        const double X[3] = {x[g[0]], x[g[1]], x[g[2]]}, Y[3] = {y[g[0]], y[g[1]], y[g[2]]};
        const double Pn[3] = {node_cond[g[0]] == conductor ? 1. : 0., node_cond[g[1]] == conductor ? 1. : 0.,
                              node_cond[g[2]] == conductor ? 1. : 0.};
        const double Vn[3] = {V[g[0]], V[g[1]], V[g[2]]};
        const EsBlock bp = blocks[labels[lbl[e]].blk];
        const double LengthConv = 0.001;
        double b[3], c[3];
        b[0] = Y[1] - Y[2]; b[1] = Y[2] - Y[0]; b[2] = Y[0] - Y[1];
        c[0] = X[2] - X[1]; c[1] = X[0] - X[2]; c[2] = X[1] - X[0];
        const double da = (b[0] * c[1] - b[1] * c[0]);
        double a = da * LengthConv * LengthConv / 2.;
        if (axi) a *= (2. * kPI * LengthConv * (X[0] + X[1] + X[2]) / 3.);
        else a *= (depth * LengthConv);
        double vx = 0, vy = 0, Dx = 0, Dy = 0;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            vx -= (Pn[k] * b[k]) / (da * LengthConv);
            vy -= (Pn[k] * c[k]) / (da * LengthConv);
            Dx -= (Vn[k] * b[k]) / (da * LengthConv);
            Dy -= (Vn[k] * c[k]) / (da * LengthConv);
        }
        Dx *= (kEo * bp.ex);
        Dy *= (kEo * bp.ey);
        Z = a * (Dx * vx + Dy * vy);
    }
    Z = cg_wave_sum(Z);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = Z;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.;
        for (int w = 0; w < kEsQBlock / 64; ++w) s += red[w];
        part[blockIdx.x] = s;
    }
}

// the workgroup partials in a fixed order: strided per thread, then the
// workgroup's sum; *out = the charge
__global__ void __launch_bounds__(kEsQBlock) k_es_charge_sum(int G, const double *__restrict__ part,
                                                             double *__restrict__ out)
{
    __shared__ double red[kEsQBlock / 64];
    double s = 0.;
    for (int i = threadIdx.x; i < G; i += kEsQBlock) s += part[i];
    s = cg_wave_sum(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        double z = 0.;
        for (int w = 0; w < kEsQBlock / 64; ++w) z += red[w];
        *out = z;
    }
}

void launch_electro_rows(hipStream_t s, xfk_problem *P)
{
    const int N = P->NR;
    if (N <= 0) return;
    EsArgs A = {};
    A.x = P->x.p;
    A.y = P->y.p;
    A.pm = P->p_raw.p;
    A.pg = P->es_p.p;
    A.lbl = P->lbl_raw.p;
    A.ebits = P->ebits_raw.p;
    A.n2e_ptr = P->n2e_ptr.p;
    A.n2e = P->n2e.p;
    A.rowptr = P->rowptr.p;
    A.col = P->col.p;
    A.labels = P->es_labels.p;
    A.blocks = P->es_blocks.p;
    A.lines = P->es_lines.p;
    A.slave = P->es_slave.p;
    A.val = P->val.p;
    A.b = P->b.p;
    A.miss = P->asm_miss.p;
    A.depth = P->es_depth;
    A.ext_ri = P->ext_ri;
    A.ext_ro = P->ext_ro;
    A.ext_zo = P->ext_zo;
    const int g = (N + kEsRowBlock - 1) / kEsRowBlock;
    if (P->axi) k_es_rows<true><<<g, kEsRowBlock, 0, s>>>(N, A);
    else k_es_rows<false><<<g, kEsRowBlock, 0, s>>>(N, A);
}

// the charge integral of one conductor into *q_host (host-synchronising)
static int conductor_charge(xfk_problem *P, int c, double *q_host)
{
    hipStream_t s = P->stream;
    const int e0 = P->es_cel_ptr[c], n = P->es_cel_ptr[c + 1] - e0;
    if (n == 0) {
        *q_host = 0.;
        return XFK_OK;
    }
    const int G = (n + kEsQBlock - 1) / kEsQBlock;   // (es_qpart holds the largest conductor's partials + 1)
    double *part = P->es_qpart.p, *out = P->es_qpart.p + G;
    k_es_charge<<<G, kEsQBlock, 0, s>>>(n, P->es_cel.p + e0, c, P->es_p.p, P->lbl_raw.p, P->es_labels.p,
                                        P->es_blocks.p, P->x.p, P->y.p, P->V.p, P->es_node_cond.p, P->axi ? 1 : 0,
                                        P->es_depth, part);
    k_es_charge_sum<<<1, kEsQBlock, 0, s>>>(G, part, out);
    XFK_CHECK(hipGetLastError());
    XFK_CHECK(d2h(q_host, out, sizeof(double), s));
    return XFK_OK;
}

// ESolver's units[] (esolver.cpp:65): user length units -> mm
static const double kEsUnits[] = {25.4, 1., 10., 1000., 0.0254, 0.001};

static int validate_es(const xfk_es_problem_desc *d)
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
                    "conductor type must be 0 (charge) or 1 (voltage)");
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

}  // namespace xfk

using namespace xfk;

hipError_t xfk::warm_module_electro()
{
    hipFuncAttributes a;
    return hipFuncGetAttributes(&a, reinterpret_cast<const void *>(&k_es_copy_slaves));
}

extern "C" {

int xfk_problem_create_electrostatic(const xfk_es_problem_desc *d, int device, xfk_problem **out)
{
    XFK_REQUIRE(d && out, XFK_ERR_ARG, "null argument");
    *out = nullptr;
    int rc = validate_es(d);
    if (rc == XFK_OK) rc = check_device(device);
    if (rc != XFK_OK) return rc;
    const int N = d->n_nodes, NE = d->n_elems, NC = d->n_conductors;
    const bool axi = d->problem_type == XFK_AXISYMMETRIC;
    const double u = kEsUnits[d->length_units];
    const double depth = d->depth * u;   // esolver.cpp:399
    auto marker = [&](int i) { return d->marker ? d->marker[i] : -1; };
    auto cond = [&](int i) { return d->conductor ? d->conductor[i] : -1; };
    auto edge = [&](long long k) { return d->e ? d->e[k] : -1; };

    // what the shared build (build_local) reads: the mesh under the merged
    // connectivity, and the boundary data in GlobalPrep's form
    GlobalPrep G;
    G.axi = axi;
    G.ext_ro = d->ext_ro * u;   // esolver.cpp:400-402 (mm)
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
    std::vector<int> rep(std::max(1, NC), -1);
    for (int i = 0; i < N; ++i) {
        const int c = cond(i);
        if (c >= 0 && d->conductors[c].type == 0 && rep[c] < 0) rep[c] = i;
    }
    std::vector<int> pm(d->p, d->p + 3LL * NE), slave_node, slave_rep;
    std::vector<unsigned char> slave(N, 0);
    for (int i = 0; i < N; ++i) {
        const int c = cond(i);
        if (c >= 0 && d->conductors[c].type == 0 && rep[c] != i) {
            slave[i] = 1;
            slave_node.push_back(i);
            slave_rep.push_back(rep[c]);
        }
    }
    if (!slave_node.empty())
        for (long long k = 0; k < 3LL * NE; ++k) {
            const int c = cond(pm[k]);
            if (c >= 0 && d->conductors[c].type == 0) pm[k] = rep[c];
        }

    // boundary properties used on edges, compacted into the 10-bit edge fields
    std::vector<int> lmap(std::max(1, d->n_lines), -1);
    std::vector<EsLine> lin;
    G.ebits.assign(NE, 0);
    if (d->e) {
        std::vector<char> used(std::max(1, d->n_lines), 0);
        for (long long k = 0; k < 3LL * NE; ++k)
            if (d->e[k] >= 0) used[d->e[k]] = 1;
        for (int k = 0; k < d->n_lines; ++k)
            if (used[k]) {
                lmap[k] = (int)lin.size();
                const xfk_es_line_desc &l = d->lines[k];
                lin.push_back(EsLine{l.c0, l.c1, l.qs, l.format, 0});
            }
        for (long long i = 0; i < NE; ++i) {
            unsigned bits = 0;
            for (int j = 0; j < 3; ++j)
                if (d->e[3 * i + j] >= 0) bits |= (unsigned)(lmap[d->e[3 * i + j]] + 1) << (10 * j);
            G.ebits[i] = (int)bits;
        }
    }
    if (lin.empty()) lin.push_back(EsLine{});

    // fixed values (esolver.cpp:410-444): point properties with qp == 0, the
    // nodes of prescribed-voltage conductors, both ends of BdryFormat 0 edges
    // in element order -- the last assignment is the node's value
    G.fixed.assign(N, 0);
    G.first.assign(N, 0.0);
    for (int i = 0; i < N; ++i) {
        const int m = marker(i), c = cond(i);
        if (m >= 0 && d->points[m].qp == 0) {
            G.first[i] = d->points[m].V;
            G.fixed[i] = 1;
        }
        if (c >= 0 && d->conductors[c].type == 1) {
            G.first[i] = d->conductors[c].V;
            G.fixed[i] = 1;
        }
    }
    if (d->e)
        for (long long i = 0; i < NE; ++i)
            for (int j = 0; j < 3; ++j) {
                const int ej = edge(3 * i + j);
                if (ej < 0 || d->lines[ej].format != 0) continue;
                for (int v : {d->p[3 * i + j], d->p[3 * i + (j + 1) % 3]}) {
                    G.first[v] = d->lines[ej].V;
                    G.fixed[v] = 1;
                }
            }
    G.last = G.first;

    // point charges on free nodes (esolver.cpp:590-597), and the charge of a
    // floating conductor on its row (esolver.cpp:628), through the
    // point-source launch
    for (int i = 0; i < N; ++i) {
        const int m = marker(i);
        if (m < 0 || G.fixed[i]) continue;
        const double Depth = axi ? 2. * kPI * d->x[i] : depth;
        G.pt_nodes.push_back(i);
        G.pt_J.push_back(((1.e6) * Depth * kEsC * d->points[m].qp));
    }
    for (int c = 0; c < NC; ++c)
        if (rep[c] >= 0) {
            G.pt_nodes.push_back(rep[c]);
            G.pt_J.push_back((1.e9) * kEsC * d->conductors[c].q);
        }

    // elements touching a node of each conductor, ascending (ChargeOnConductor)
    std::vector<int> cel_ptr(NC + 1, 0), cel;
    if (NC > 0 && d->conductor) {
        std::vector<std::vector<int>> per(NC);
        for (int i = 0; i < NE; ++i) {
            const int c0 = cond(d->p[3LL * i]), c1 = cond(d->p[3LL * i + 1]), c2 = cond(d->p[3LL * i + 2]);
            if (c0 >= 0) per[c0].push_back(i);
            if (c1 >= 0 && c1 != c0) per[c1].push_back(i);
            if (c2 >= 0 && c2 != c0 && c2 != c1) per[c2].push_back(i);
        }
        for (int c = 0; c < NC; ++c) {
            cel.insert(cel.end(), per[c].begin(), per[c].end());
            cel_ptr[c + 1] = (int)cel.size();
        }
    }
    int qmax = 0;
    for (int c = 0; c < NC; ++c) qmax = std::max(qmax, cel_ptr[c + 1] - cel_ptr[c]);

    xfk_problem_desc md = {};
    md.n_nodes = N;
    md.x = d->x;
    md.y = d->y;
    md.n_elems = NE;
    md.p = pm.data();
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
    rc = build_local(&md, G, nullptr, device, nullptr, out);
    if (rc != XFK_OK) return rc;
    xfk_problem *P = *out;
    auto fail = [&](int code) {
        xfk_problem_destroy(P);
        *out = nullptr;
        return code;
    };
    {
        ArenaScope arena_scope(&P->arena);
        P->electro = true;
        P->es_depth = depth;
        P->es_cond.assign(d->conductors, d->conductors + NC);
        for (auto &c : P->es_cond)
            if (c.type == 1) c.q = 0;
        P->es_cond_rep.assign(rep.begin(), rep.begin() + NC);
        P->es_cel_ptr = cel_ptr;
        P->es_nslave = (int)slave_node.size();
        std::vector<EsBlock> blk(d->n_blocks);
        for (int k = 0; k < d->n_blocks; ++k) blk[k] = EsBlock{d->blocks[k].ex, d->blocks[k].ey, d->blocks[k].qv};
        std::vector<EsLabel> lab(d->n_labels);
        for (int k = 0; k < d->n_labels; ++k) lab[k] = EsLabel{d->labels[k].block, d->labels[k].is_external ? 1 : 0};
        std::vector<int> ncond(N);
        for (int i = 0; i < N; ++i) ncond[i] = cond(i);
        hipStream_t s = P->stream;
        hipError_t e = hipSuccess;
#define UP(buf, ptr, n) if (e == hipSuccess) e = upload(buf, ptr, n, s)
        UP(P->es_p, d->p, 3 * (size_t)NE);
        UP(P->es_blocks, blk.data(), blk.size());
        UP(P->es_labels, lab.data(), lab.size());
        UP(P->es_lines, lin.data(), lin.size());
        UP(P->es_slave, slave.data(), slave.size());
        UP(P->es_slave_node, slave_node.data(), slave_node.size());
        UP(P->es_slave_rep, slave_rep.data(), slave_rep.size());
        UP(P->es_cel, cel.data(), cel.size());
        UP(P->es_node_cond, ncond.data(), ncond.size());
#undef UP
        if (e == hipSuccess) e = P->es_qpart.alloc((size_t)(qmax + kEsQBlock - 1) / kEsQBlock + 2);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) {
            set_error(std::string("upload failed: ") + hipGetErrorString(e));
            return fail(XFK_ERR_HIP);
        }
    }
    return reserve_first_solve(out);
}

int xfk_electrostatic(xfk_problem *P, int flags, xfk_result *res)
{
    XFK_REQUIRE(P && P->electro, XFK_ERR_ARG, "not an electrostatic problem (xfk_problem_create_electrostatic)");
    ArenaScope arena_scope(&P->arena);
    P->es_solved = false;
    int rc = static2d_run(P, flags, res);
    if (rc == XFK_OK) {
        if (P->es_nslave)
            k_es_copy_slaves<<<(P->es_nslave + kBlock - 1) / kBlock, kBlock, 0, P->stream>>>(
                P->es_nslave, P->es_slave_node.p, P->es_slave_rep.p, P->V.p);
        // the charge of the prescribed-voltage conductors (esolver.cpp:641-643)
        for (int c = 0; c < (int)P->es_cond.size() && rc == XFK_OK; ++c)
            if (P->es_cond[c].type == 1) rc = conductor_charge(P, c, &P->es_cond[c].q);
        if (rc == XFK_OK && hipStreamSynchronize(P->stream) != hipSuccess) {
            set_error("electrostatic post-processing failed");
            rc = XFK_ERR_HIP;
        }
        P->es_solved = rc == XFK_OK;
    }
    problem_recycle(P);
    return rc;
}

int xfk_get_conductors(xfk_problem *P, double *V, double *q)
{
    XFK_REQUIRE(P && P->electro, XFK_ERR_ARG, "not an electrostatic problem");
    XFK_REQUIRE(P->es_solved, XFK_ERR_ARG, "no solution yet");
    XFK_CHECK(hipSetDevice(P->device));
    for (int c = 0; c < (int)P->es_cond.size(); ++c) {
        if (q) q[c] = P->es_cond[c].q;
        if (!V) continue;
        V[c] = P->es_cond[c].V;
        if (P->es_cond[c].type == 0) {
            V[c] = 0.;   // (a conductor without nodes: the reference's placeholder row)
            if (P->es_cond_rep[c] >= 0)
                XFK_CHECK(d2h(&V[c], P->V.p + P->es_cond_rep[c], sizeof(double), P->stream));
        }
    }
    return XFK_OK;
}

int xfk_conductor_charge(xfk_problem *P, int conductor, double *q)
{
    XFK_REQUIRE(P && P->electro && q, XFK_ERR_ARG, "null argument or not an electrostatic problem");
    XFK_REQUIRE(P->es_solved, XFK_ERR_ARG, "no solution yet");
    XFK_REQUIRE(conductor >= 0 && conductor < (int)P->es_cond.size(), XFK_ERR_ARG, "conductor index out of range");
    XFK_CHECK(hipSetDevice(P->device));
    return conductor_charge(P, conductor, q);
}

}  // extern "C"
