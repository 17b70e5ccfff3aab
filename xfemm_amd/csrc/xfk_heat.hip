// Heat-flow problems on the device: HSolver::AnalyzeProblem
// (reference cfemm/hsolver/hsolver.cpp:458-852) and HSolver::ChargeOnConductor
// (hsolver.cpp:987-1035) for MI355X (gfx950).
//
// What is new here: the heat-flow element -- conductivities from the K(T)
// tables at the last solution's nodal temperatures, the lumped capacity term
// of a time step, volume heating, flux / convection / linearised radiation
// edges -- inside a row gather of its own (k_hf_rows, the structure of
// xfk_electro.hip's k_es_rows), the outer fixed-point loop with its change
// norm, the heat flow through a conductor and the C-ABI entry points.
// Everything else is the static path unchanged, as for electrostatics: the
// symbolic phase, the point-source launch, the Dirichlet kernels, the
// (anti)periodic averaging map and the AMG-PCG, one pass at a time
// (static_assemble_pass / static_pcg_pass).
//
// A CircType 0 conductor (a prescribed total heat flow) is merged onto its
// lowest-numbered node exactly as xfk_electro.hip merges a floating conductor;
// the problem's es_* buffers hold the merged connectivity's companions with
// the same meaning.
#include "xfk_kernels.h"
#include "xfk_spmv.h"
#include "xfk_amg.h"

#include <atomic>
#include <cmath>
#include <cstdio>

namespace xfk {

constexpr double kKsb = 5.67032e-8;   // Stefan-Boltzmann constant, W/(m^2 K^4) (femmconstants.h)

struct HfArgs {
    const double *x, *y;           // m
    const int *pm;                 // merged connectivity: rows and columns
    const int *pg;                 // mesh connectivity: geometry, Vo, Tprev
    const int *lbl, *ebits;
    const int *n2e_ptr, *n2e, *rowptr, *col;
    const EsLabel *labels;
    const HfBlock *blocks;
    const HfLine *lines;
    const double *tkT, *tkK;       // the K(T) knots of all blocks
    const double *vo;              // the last solution (Vo)
    const double *tprev;           // the previous time step's solution (dt != 0)
    const unsigned char *slave;    // merged-away node: identity row
    double *val, *b;
    int *miss;
    double depth;                  // m (planar)
    double dt;
    double ext_ri, ext_ro, ext_zo; // m
};

__device__ __forceinline__ double hf_sqr(double v) { return v * v; }

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

// One element of HSolver::AnalyzeProblem (hsolver.cpp:546-722), in the
// reference's operation order: Me / be before the sign of the global assembly.
// X is x (planar) or r (axisymmetric), in m; eb the element's three packed
// 10-bit boundary-property fields; Vo / Tp the last solution and the previous
// time step's at the element's nodes.
template <bool AXI>
__device__ __forceinline__ void hf_element(int eb, const HfArgs &A, const double (&X)[3], const double (&Y)[3],
                                           const double (&Vo)[3], const double (&Tp)[3], const EsLabel &lab,
                                           const HfBlock &bp, double (&Me)[3][3], double (&be)[3])
{
    double l[3], p[3], q[3];
    p[0] = Y[1] - Y[2]; p[1] = Y[2] - Y[0]; p[2] = Y[0] - Y[1];
    q[0] = X[2] - X[1]; q[1] = X[0] - X[2]; q[2] = X[1] - X[0];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const int k = (j + 1) % 3;
        l[j] = sqrt(hf_sqr(X[k] - X[j]) + hf_sqr(Y[k] - Y[j]));
    }
    const double a = (p[0] * q[1] - p[1] * q[0]) / 2.;
    const double r = (X[0] + X[1] + X[2]) / 3.;
    // the conductivities of this element: the mean of GetK at its nodes
    double k0x, k0y, k1x, k1y, k2x, k2y;
    hf_getk(bp, A.tkT, A.tkK, Vo[0], k0x, k0y);
    hf_getk(bp, A.tkT, A.tkK, Vo[1], k1x, k1y);
    hf_getk(bp, A.tkT, A.tkK, Vo[2], k2x, k2y);
    const double knx = (k0x + k1x + k2x) / 3., kny = (k0y + k1y + k2y) / 3.;
    double Depth = A.depth, kludge = 1;
    if (AXI) {
        Depth = 2. * kPI * r;
        // the conductivity warp of the conformally mapped exterior region
        if (lab.external) {
            const double z = (Y[0] + Y[1] + Y[2]) / 3. - A.ext_zo;
            kludge = (r * r + z * z) / (A.ext_ri * A.ext_ro);
        }
    }
    // x- and y-contributions (upper values mirrored: exact symmetry)
    const double Kx = -Depth * knx / (4. * a) / kludge;
    const double Ky = -Depth * kny / (4. * a) / kludge;
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
        for (int k = j; k < 3; ++k) {
            double m = Kx * p[j] * p[k];
            m += Ky * q[j] * q[k];
            Me[j][k] = m;
            Me[k][j] = m;
        }
    be[0] = 0.; be[1] = 0.; be[2] = 0.;
    // the time-transient term: lumped capacity on the diagonal
    if (A.dt != 0) {
        const double K = -Depth * bp.kt * a / (3. * A.dt);
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            Me[j][j] += K;
            be[j] += K * Tp[j];
        }
    }
    // volume heating
    const double Kv = -Depth * (bp.qv) * a / 3.;
    be[0] += Kv; be[1] += Kv; be[2] += Kv;
    if (eb) {
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const int ej = ((eb >> (10 * j)) & 1023) - 1;
            if (ej < 0) continue;
            const int k = (j + 1) % 3;
            if (AXI) Depth = kPI * (X[j] + X[k]);
            const HfLine ln = A.lines[ej];
            const int bf = ln.format;
            if (bf != 1 && bf != 2 && bf != 3) continue;
            double c0 = 0., c1 = 0.;
            if (bf == 1) {          // heat flux
                c1 = ln.qs;
                c0 = 0;
            } else if (bf == 2) {   // convection
                c0 = ln.h;
                c1 = -c0 * ln.tinf;
            } else {                // radiation, linearised around the last solution
                const double bta = ln.beta, Tinf = ln.tinf;
                const double Tlast = (Vo[j] + Vo[k]) / 2.;
                // (the reference's pow(T, 3.) and pow(T, 4.) as plain products)
                const double T2 = Tlast * Tlast, I2 = Tinf * Tinf;
                c0 = 4. * bta * kKsb * (T2 * Tlast);
                c1 = -(bta * kKsb * (I2 * I2 + 3. * (T2 * T2)));
            }
            if (AXI) {
                double K = -2. * kPI * c0 * l[j] / 6.;
                Me[j][j] += K * 2. * (3. * X[j] + X[k]) / 4.;
                Me[k][k] += K * 2. * (X[j] + 3. * X[k]) / 4.;
                Me[j][k] += K * (X[j] + X[k]) / 2.;
                Me[k][j] += K * (X[j] + X[k]) / 2.;
                K = 2. * kPI * c1 * l[j] / 2.;
                be[j] += K * (2. * X[j] + X[k]) / 3.;
                be[k] += K * (X[j] + 2. * X[k]) / 3.;
            } else {
                double K = -Depth * c0 * l[j] / 6.;
                Me[j][j] += K * 2.;
                Me[k][k] += K * 2.;
                Me[j][k] += K;
                Me[k][j] += K;
                K = Depth * c1 * l[j] / 2.;
                be[j] += K;
                be[k] += K;
            }
        }
    }
}

// Row gather (the structure of k_es_rows / assemble_rows): one thread per CSR
// row i sums the contributions of the elements incident on node i of the
// merged connectivity, in ascending element order -- the order the
// reference's Put(Get() - Me) accumulates each entry in.  Rows of <= kHfRowAcc
// entries accumulate in LDS; longer ones (a merged conductor's row, periodic
// corners) in place in val, their columns found by bisection.  An element
// with two or three nodes on one merged conductor appears that many times in
// the representative's list (adjacent: the list is sorted) and is taken once,
// every one of its merged vertices contributing its row of Me.  No atomics,
// no colouring: every entry of val and b has one writer.
constexpr int kHfRowBlock = 128;
constexpr int kHfRowAcc = 12;

template <bool AXI>
__global__ void __launch_bounds__(kHfRowBlock) k_hf_rows(int N, HfArgs A)
{
    __shared__ double s_acc[kHfRowAcc * kHfRowBlock];
    __shared__ int s_col[kHfRowAcc * kHfRowBlock];
    const int i0 = xcd_tile(blockIdx.x, gridDim.x) * kHfRowBlock;
    const int i = i0 + threadIdx.x;
    const bool live = i < N;   // (every thread reaches the barriers below)
    const int rs = live ? A.rowptr[i] : 0, L = live ? A.rowptr[i + 1] - rs : 0;
    const bool lds = L <= kHfRowAcc;
    double *acc = lds ? s_acc + threadIdx.x : A.val + rs;
    const int stride = lds ? kHfRowBlock : 1;
    const int *cols = lds ? s_col + threadIdx.x : A.col + rs;
    for (int k = 0; k < L; ++k) {
        acc[k * stride] = 0.;
        if (lds) s_col[k * kHfRowBlock + threadIdx.x] = A.col[rs + k];
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
        const HfBlock bp = A.blocks[lab.blk];
        const double X[3] = {A.x[g[0]], A.x[g[1]], A.x[g[2]]};
        const double Y[3] = {A.y[g[0]], A.y[g[1]], A.y[g[2]]};
        const double Vo[3] = {A.vo[g[0]], A.vo[g[1]], A.vo[g[2]]};
        double Tp[3] = {0., 0., 0.};
        if (A.dt != 0) {
            Tp[0] = A.tprev[g[0]];
            Tp[1] = A.tprev[g[1]];
            Tp[2] = A.tprev[g[2]];
        }
        double Me[3][3], be[3];
        hf_element<AXI>(A.ebits[e], A, X, Y, Vo, Tp, lab, bp, Me, be);
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
    if (live && A.slave[i]) acc[find(i) * stride] = 1.;   // merged-away node: T_i = 0 until the copy after the solve
    if (miss && A.miss) *A.miss = 1;
    // (as assemble_rows: a block whose rows all sat in LDS writes its run of
    // val with consecutive lanes on consecutive entries)
    if (__syncthreads_and(lds)) {
        double r[kHfRowAcc];
#pragma unroll
        for (int k = 0; k < kHfRowAcc; ++k) r[k] = k < L ? s_acc[k * kHfRowBlock + threadIdx.x] : 0.;
        const int rb0 = A.rowptr[min(i0, N)], rb1 = A.rowptr[min(i0 + kHfRowBlock, N)];
        __syncthreads();
#pragma unroll
        for (int k = 0; k < kHfRowAcc; ++k)
            if (k < L) s_acc[rs - rb0 + k] = r[k];
        __syncthreads();
        for (int m = threadIdx.x; m < rb1 - rb0; m += kHfRowBlock) A.val[rb0 + m] = s_acc[m];
    } else if (lds) {
        for (int k = 0; k < L; ++k) A.val[rs + k] = s_acc[k * kHfRowBlock + threadIdx.x];
    }
    if (live) A.b[i] = bi;
}

// merged-away nodes take their conductor's temperature (bit-equal), or zero
// (their identity rows' solution: the value the warm-started PCG expects)
__global__ void k_hf_set_slaves(int n, const int *__restrict__ node, const int *__restrict__ rep, int zero,
                                double *__restrict__ V)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < n) V[node[t]] = zero ? 0. : V[rep[t]];
}

constexpr int kHfQBlock = 256;

// the workgroup's sums of a and b (wave shuffles, then the waves in order)
// into part[2 wg], part[2 wg + 1]
__device__ __forceinline__ void hf_block_sum2(double a, double b, double *__restrict__ part)
{
    __shared__ double red[2 * (kHfQBlock / 64)];
    a = cg_wave_sum(a);
    b = cg_wave_sum(b);
    if ((threadIdx.x & 63) == 0) {
        red[2 * (threadIdx.x >> 6)] = a;
        red[2 * (threadIdx.x >> 6) + 1] = b;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double sa = 0., sb = 0.;
        for (int w = 0; w < kHfQBlock / 64; ++w) {
            sa += red[2 * w];
            sb += red[2 * w + 1];
        }
        part[2 * blockIdx.x] = sa;
        part[2 * blockIdx.x + 1] = sb;
    }
}

// the outer loop's change norm (hsolver.cpp:827-830): e1 = sum (V - Vo)^2,
// e2 = sum Vo^2, one node per thread, a pair of partials per workgroup
__global__ void __launch_bounds__(kHfQBlock) k_hf_change(int N, const double *__restrict__ V,
                                                         const double *__restrict__ Vo, double *__restrict__ part)
{
    const int t = blockIdx.x * kHfQBlock + threadIdx.x;
    double e1 = 0., e2 = 0.;
    if (t < N) {
        const double v = V[t], vo = Vo[t];
        e1 = (v - vo) * (v - vo);
        e2 = (vo * vo);
    }
    hf_block_sum2(e1, e2, part);
}

// the workgroup pairs in a fixed order: strided per thread, then the
// workgroup's sums; out[0], out[1] = the two sums
__global__ void __launch_bounds__(kHfQBlock) k_hf_sum2(int G, const double *__restrict__ part,
                                                       double *__restrict__ out)
{
    double a = 0., b = 0.;
    for (int i = threadIdx.x; i < G; i += kHfQBlock) {
        a += part[2 * i];
        b += part[2 * i + 1];
    }
    hf_block_sum2(a, b, out);   // (one workgroup: blockIdx.x == 0)
}

// HSolver::ChargeOnConductor (hsolver.cpp:987-1035) over the elements touching
// a node of the conductor (els[0 .. n), ascending): one element per thread,
// the conductivities at the solved temperatures of its nodes
__global__ void __launch_bounds__(kHfQBlock) k_hf_flow(int n, const int *__restrict__ els, int conductor,
                                                       const int *__restrict__ pg, const int *__restrict__ lbl,
                                                       const EsLabel *__restrict__ labels,
                                                       const HfBlock *__restrict__ blocks,
                                                       const double *__restrict__ tkT,
                                                       const double *__restrict__ tkK,
                                                       const double *__restrict__ x, const double *__restrict__ y,
                                                       const double *__restrict__ V,
                                                       const int *__restrict__ node_cond, int axi, double depth,
                                                       double *__restrict__ part)
{
    const int t = blockIdx.x * kHfQBlock + threadIdx.x;
    double Z = 0.;
    if (t < n) {
        const int e = els[t];
        const int g[3] = {pg[3 * e], pg[3 * e + 1], pg[3 * e + 2]};
        const double X[3] = {x[g[0]], x[g[1]], x[g[2]]}, Y[3] = {y[g[0]], y[g[1]], y[g[2]]};
        const double Pn[3] = {node_cond[g[0]] == conductor ? 1. : 0., node_cond[g[1]] == conductor ? 1. : 0.,
                              node_cond[g[2]] == conductor ? 1. : 0.};
        const double Vn[3] = {V[g[0]], V[g[1]], V[g[2]]};
        const HfBlock bp = blocks[labels[lbl[e]].blk];
        double b[3], c[3];
        b[0] = Y[1] - Y[2]; b[1] = Y[2] - Y[0]; b[2] = Y[0] - Y[1];
        c[0] = X[2] - X[1]; c[1] = X[0] - X[2]; c[2] = X[1] - X[0];
        const double da = (b[0] * c[1] - b[1] * c[0]);
        double a = da / 2.;
        if (axi) a *= (2. * kPI * (X[0] + X[1] + X[2]) / 3.);
        else a *= depth;
        double vx = 0, vy = 0, Dx = 0, Dy = 0, knx = 0, kny = 0;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            vx -= (Pn[k] * b[k]) / da;
            vy -= (Pn[k] * c[k]) / da;
            Dx -= (Vn[k] * b[k]) / da;
            Dy -= (Vn[k] * c[k]) / da;
            double kx, ky;
            hf_getk(bp, tkT, tkK, Vn[k], kx, ky);
            knx += kx / 3.;
            kny += ky / 3.;
        }
        Dx *= knx;
        Dy *= kny;
        Z = a * (Dx * vx + Dy * vy);
    }
    hf_block_sum2(Z, 0., part);
}

void launch_heat_rows(hipStream_t s, xfk_problem *P)
{
    const int N = P->NR;
    if (N <= 0) return;
    HfArgs A = {};
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
    A.blocks = P->hf_blocks.p;
    A.lines = P->hf_lines.p;
    A.tkT = P->hf_tk_T.p;
    A.tkK = P->hf_tk_K.p;
    A.vo = P->hf_vo;
    A.tprev = P->hf_tprev.p;
    A.slave = P->es_slave.p;
    A.val = P->val.p;
    A.b = P->b.p;
    A.miss = P->asm_miss.p;
    A.depth = P->es_depth;
    A.dt = P->hf_dt;
    A.ext_ri = P->ext_ri;
    A.ext_ro = P->ext_ro;
    A.ext_zo = P->ext_zo;
    const int g = (N + kHfRowBlock - 1) / kHfRowBlock;
    if (P->axi) k_hf_rows<true><<<g, kHfRowBlock, 0, s>>>(N, A);
    else k_hf_rows<false><<<g, kHfRowBlock, 0, s>>>(N, A);
}

// the heat flow through one conductor into *q_host (host-synchronising)
static int conductor_flow(xfk_problem *P, int c, double *q_host)
{
    hipStream_t s = P->stream;
    const int e0 = P->es_cel_ptr[c], n = P->es_cel_ptr[c + 1] - e0;
    if (n == 0) {
        *q_host = 0.;
        return XFK_OK;
    }
    const int G = (n + kHfQBlock - 1) / kHfQBlock;   // (hf_part holds the largest conductor's pairs + 1)
    double *part = P->hf_part.p, *out = P->hf_part.p + 2 * G;
    k_hf_flow<<<G, kHfQBlock, 0, s>>>(n, P->es_cel.p + e0, c, P->es_p.p, P->lbl_raw.p, P->es_labels.p,
                                      P->hf_blocks.p, P->hf_tk_T.p, P->hf_tk_K.p, P->x.p, P->y.p, P->V.p,
                                      P->es_node_cond.p, P->axi ? 1 : 0, P->es_depth, part);
    k_hf_sum2<<<1, kHfQBlock, 0, s>>>(G, part, out);
    XFK_CHECK(hipGetLastError());
    XFK_CHECK(d2h(q_host, out, sizeof(double), s));
    return XFK_OK;
}

// HSolver's units[] (hsolver.cpp:65): user length units -> m
static const double kHfUnits[] = {0.0254, 0.001, 0.01, 1, 2.54e-5, 1.e-6};

static int validate_hf(const xfk_hf_problem_desc *d)
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
    // (the reference resets dT to 0 with a warning when the previous solution
    // cannot be loaded, and solves another problem than the one asked for)
    XFK_REQUIRE(!(d->dt < 0), XFK_ERR_ARG, "dT must not be negative");
    XFK_REQUIRE(d->dt == 0 || d->t_prev, XFK_ERR_ARG, "dT != 0 needs the previous solution (t_prev)");
    for (int k = 0; k < d->n_blocks; ++k) {
        XFK_REQUIRE(d->blocks[k].npts >= 0, XFK_ERR_ARG, "K(T) table with a negative number of points");
        XFK_REQUIRE(d->blocks[k].npts == 0 || (d->blocks[k].T && d->blocks[k].K), XFK_ERR_ARG,
                    "K(T) table without its T or K array");
    }
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
                    "conductor type must be 0 (heat flow) or 1 (temperature)");
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

// HSolver::AnalyzeProblem's outer loop (hsolver.cpp:491-842): every pass
// assembles from the last solution and warm-starts the PCG from it
static int heat_run(xfk_problem *P, int flags, xfk_result *res)
{
    XFK_CHECK(hipSetDevice(P->device));
    hipStream_t s = P->stream;
    ScopedEvents<2> ev;
    XFK_CHECK(ev.create());
    hipEvent_t es0 = ev[0], es1 = ev[1];
    xfk_result R{};
    int rc = XFK_OK;
    float ms = 0;
    P->pcg_tol = 0;
    P->pcg_tol_rel = 0;
    P->time_spmv = false;
    P->spmv_used = 0;
    P->nws_at_poll = false;
    if (P->amg) {
        P->amg->time_tail = false;
        P->amg->tail_used = 0;
    }
    P->last.ms_amg_setup = 0;
    P->last.amg_levels = 0;
    P->last.amg_op_complexity = 0;
    P->setup_used = 0;
    P->setup_ms_pending = 0;
    XFK_CHECK(hipEventRecord(es0, s));
    if (!P->symbolic_ready || (flags & XFK_REBUILD_SYMBOLIC)) {
        P->symbolic_ready = false;
        rc = build_symbolic(P);
        if (rc != XFK_OK) return rc;
    }
    XFK_CHECK(hipEventRecord(es1, s));

    const int N = P->N;
    const int G = (N + kHfQBlock - 1) / kHfQBlock;
    double *part = P->hf_part.p, *sums = P->hf_part.p + 2 * (size_t)G;
    XFK_CHECK(hipMemsetAsync(P->V.p, 0, sizeof(double) * P->NL, s));   // CBigLinProb::Create: V = 0
    P->amg_reusable = false;   // a hierarchy is reused only inside one solve
    P->pc_used = XFK_PRECOND_JACOBI;
    const int ns = P->es_nslave;
    const int gs = (ns + kBlock - 1) / kBlock;
    double resn = 0;
    int Iter = 0;
    for (bool again = true; again;) {
        while ((int)P->pass_ev.size() < 3 * (Iter + 1)) {
            hipEvent_t ev_new = nullptr;
            XFK_CHECK(hipEventCreate(&ev_new));
            P->pass_ev.push_back(ev_new);
        }
        XFK_CHECK(hipEventRecord(P->pass_ev[3 * Iter], s));
        // copy old solution: Vo
        XFK_CHECK(hipMemcpyAsync(P->Vold.p, P->V.p, sizeof(double) * N, hipMemcpyDeviceToDevice, s));
        P->hf_vo = P->Vold.p;
        rc = static_assemble_pass(P, Iter);
        if (rc != XFK_OK) return rc;
        if (ns && Iter > 0) k_hf_set_slaves<<<gs, kBlock, 0, s>>>(ns, P->es_slave_node.p, P->es_slave_rep.p, 1, P->V.p);
        XFK_CHECK(hipEventRecord(P->pass_ev[3 * Iter + 1], s));
        rc = static_pcg_pass(P, Iter);   // L.PCGSolve(iter++)
        if (rc != XFK_OK) return rc;
        XFK_CHECK(hipEventRecord(P->pass_ev[3 * Iter + 2], s));
        R.cg_iters += P->pcg_host->iters;
        R.final_er = P->pcg_host->er;
        P->amg_last_iters = P->pcg_host->iters - P->pcg_discarded;
        if (P->amg_fresh) P->amg_fresh_iters = P->pcg_host->iters - P->pcg_discarded;
        if (ns) k_hf_set_slaves<<<gs, kBlock, 0, s>>>(ns, P->es_slave_node.p, P->es_slave_rep.p, 0, P->V.p);
        again = false;
        if (P->hf_nonlinear) {
            double e[2] = {0., 0.};
            k_hf_change<<<G, kHfQBlock, 0, s>>>(N, P->V.p, P->Vold.p, part);
            k_hf_sum2<<<1, kHfQBlock, 0, s>>>(G, part, sums);
            XFK_CHECK(hipGetLastError());
            XFK_CHECK(d2h(e, sums, 2 * sizeof(double), s));
            // (no test while sum Vo^2 == 0 -- the first pass; a solution that is
            // and stays zero would keep the reference in its loop: stop)
            if (e[1] != 0) {
                resn = sqrt(e[0] / e[1]);
                again = !(resn < P->precision * 100.);
            } else {
                again = e[0] != 0;
            }
        }
        Iter++;
        if (again && Iter >= P->hf_max_passes) {
            char msg[96];
            std::snprintf(msg, sizeof msg, "heat-flow iteration did not converge in %d passes", Iter);
            set_error(msg);
            return XFK_ERR_NOCONV;
        }
    }
    XFK_CHECK(hipStreamSynchronize(s));
    XFK_CHECK(hipEventElapsedTime(&ms, es0, es1));
    R.ms_symbolic = ms;
    for (int k = 0; k < Iter; ++k) {
        XFK_CHECK(hipEventElapsedTime(&ms, P->pass_ev[3 * k], P->pass_ev[3 * k + 1]));
        R.ms_assemble += ms;
        XFK_CHECK(hipEventElapsedTime(&ms, P->pass_ev[3 * k + 1], P->pass_ev[3 * k + 2]));
        R.ms_solve += ms;
    }
    for (int k = 0; k < P->setup_used; ++k) {
        float m = 0;
        XFK_CHECK(hipEventElapsedTime(&m, P->setup_ev[2 * k], P->setup_ev[2 * k + 1]));
        P->last.ms_amg_setup += m;
    }
    P->last.ms_amg_setup += P->setup_ms_pending;
    P->setup_used = 0;
    P->setup_ms_pending = 0;
    R.prec_fallback = P->f64_fallback ? 1 : 0;
    R.newton_iters = Iter;
    R.last_res = resn;
    R.nnz = P->nnz_own;
    R.ncolors = P->ncolors;
    R.color_rounds = P->color_rounds;
    R.precond = P->pc_used;
    R.amg_levels = P->last.amg_levels;
    R.amg_op_complexity = P->last.amg_op_complexity;
    R.ms_amg_setup = P->last.ms_amg_setup;
    P->last = R;
    if (res) *res = R;
    return XFK_OK;
}

}  // namespace xfk

using namespace xfk;

hipError_t xfk::warm_module_heat()
{
    hipFuncAttributes a;
    return hipFuncGetAttributes(&a, reinterpret_cast<const void *>(&k_hf_set_slaves));
}

extern "C" {

int xfk_problem_create_heatflow(const xfk_hf_problem_desc *d, int device, xfk_problem **out)
{
    XFK_REQUIRE(d && out, XFK_ERR_ARG, "null argument");
    *out = nullptr;
    int rc = validate_hf(d);
    if (rc == XFK_OK) rc = check_device(device);
    if (rc != XFK_OK) return rc;
    const int N = d->n_nodes, NE = d->n_elems, NC = d->n_conductors;
    const bool axi = d->problem_type == XFK_AXISYMMETRIC;
    const double u = kHfUnits[d->length_units];
    const double depth = d->depth * u;   // hsolver.cpp:471
    auto marker = [&](int i) { return d->marker ? d->marker[i] : -1; };
    auto cond = [&](int i) { return d->conductor ? d->conductor[i] : -1; };
    auto edge = [&](long long k) { return d->e ? d->e[k] : -1; };

    // what the shared build (build_local) reads: the mesh under the merged
    // connectivity, and the boundary data in GlobalPrep's form
    GlobalPrep G;
    G.axi = axi;
    G.ext_ro = d->ext_ro * u;   // hsolver.cpp:472-474 (m)
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
    std::vector<HfLine> lin;
    bool nonlinear = false;
    G.ebits.assign(NE, 0);
    if (d->e) {
        std::vector<char> used(std::max(1, d->n_lines), 0);
        for (long long k = 0; k < 3LL * NE; ++k)
            if (d->e[k] >= 0) used[d->e[k]] = 1;
        for (int k = 0; k < d->n_lines; ++k)
            if (used[k]) {
                lmap[k] = (int)lin.size();
                const xfk_hf_line_desc &l = d->lines[k];
                lin.push_back(HfLine{l.qs, l.beta, l.h, l.Tinf, l.format, 0});
                nonlinear |= l.format == 3;   // a radiation edge (hsolver.cpp:673)
            }
        for (long long i = 0; i < NE; ++i) {
            unsigned bits = 0;
            for (int j = 0; j < 3; ++j)
                if (d->e[3 * i + j] >= 0) bits |= (unsigned)(lmap[d->e[3 * i + j]] + 1) << (10 * j);
            G.ebits[i] = (int)bits;
        }
    }
    if (lin.empty()) lin.push_back(HfLine{});
    // a K(T) table on the block of ANY element (the reference's scan reads the
    // blocks of the first NumNodes elements only: INTEGRATION.md)
    for (long long i = 0; i < NE && !nonlinear; ++i) nonlinear = d->blocks[d->labels[d->lbl[i]].block].npts > 0;

    // fixed values (hsolver.cpp:499-533): point properties with qp == 0, the
    // nodes of prescribed-temperature conductors, both ends of BdryFormat 0
    // edges in element order -- the last assignment is the node's value
    G.fixed.assign(N, 0);
    G.first.assign(N, 0.0);
    for (int i = 0; i < N; ++i) {
        const int m = marker(i), c = cond(i);
        if (m >= 0 && d->points[m].qp == 0) {
            G.first[i] = d->points[m].T;
            G.fixed[i] = 1;
        }
        if (c >= 0 && d->conductors[c].type == 1) {
            G.first[i] = d->conductors[c].T;
            G.fixed[i] = 1;
        }
    }
    if (d->e)
        for (long long i = 0; i < NE; ++i)
            for (int j = 0; j < 3; ++j) {
                const int ej = edge(3 * i + j);
                if (ej < 0 || d->lines[ej].format != 0) continue;
                for (int v : {d->p[3 * i + j], d->p[3 * i + (j + 1) % 3]}) {
                    G.first[v] = d->lines[ej].Tset;
                    G.fixed[v] = 1;
                }
            }
    G.last = G.first;

    // point sources on free nodes (hsolver.cpp:764-771), and the heat flow of
    // a floating conductor on its row (hsolver.cpp:802, unscaled), through the
    // point-source launch
    for (int i = 0; i < N; ++i) {
        const int m = marker(i);
        if (m < 0 || G.fixed[i]) continue;
        const double Depth = axi ? 2. * kPI * d->x[i] : depth;
        G.pt_nodes.push_back(i);
        G.pt_J.push_back((Depth * d->points[m].qp));
    }
    for (int c = 0; c < NC; ++c)
        if (rep[c] >= 0) {
            G.pt_nodes.push_back(rep[c]);
            G.pt_J.push_back(d->conductors[c].q);
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

    // the K(T) tables of all blocks in one array, an offset and a count per block
    std::vector<HfBlock> blk(d->n_blocks);
    std::vector<double> tkT, tkK;
    for (int k = 0; k < d->n_blocks; ++k) {
        const xfk_hf_block_desc &b = d->blocks[k];
        blk[k] = HfBlock{b.kx, b.ky, b.kt, b.qv, b.npts, (int)tkT.size()};
        tkT.insert(tkT.end(), b.T, b.T + (b.npts > 0 ? b.npts : 0));
        tkK.insert(tkK.end(), b.K, b.K + (b.npts > 0 ? b.npts : 0));
    }

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
        P->heat = true;
        P->hf_nonlinear = nonlinear;
        P->hf_dt = d->dt;
        P->es_depth = depth;
        P->hf_cond.assign(d->conductors, d->conductors + NC);
        for (auto &c : P->hf_cond)
            if (c.type == 1) c.q = 0;
        P->es_cond_rep.assign(rep.begin(), rep.begin() + NC);
        P->es_cel_ptr = cel_ptr;
        P->es_nslave = (int)slave_node.size();
        std::vector<EsLabel> lab(d->n_labels);
        for (int k = 0; k < d->n_labels; ++k) lab[k] = EsLabel{d->labels[k].block, d->labels[k].is_external ? 1 : 0};
        std::vector<int> ncond(N);
        for (int i = 0; i < N; ++i) ncond[i] = cond(i);
        hipStream_t s = P->stream;
        hipError_t e = hipSuccess;
#define UP(buf, ptr, n) if (e == hipSuccess) e = upload(buf, ptr, n, s)
        UP(P->es_p, d->p, 3 * (size_t)NE);
        UP(P->hf_blocks, blk.data(), blk.size());
        UP(P->es_labels, lab.data(), lab.size());
        UP(P->hf_lines, lin.data(), lin.size());
        UP(P->hf_tk_T, tkT.data(), tkT.size());
        UP(P->hf_tk_K, tkK.data(), tkK.size());
        UP(P->es_slave, slave.data(), slave.size());
        UP(P->es_slave_node, slave_node.data(), slave_node.size());
        UP(P->es_slave_rep, slave_rep.data(), slave_rep.size());
        UP(P->es_cel, cel.data(), cel.size());
        UP(P->es_node_cond, ncond.data(), ncond.size());
#undef UP
        if (e == hipSuccess) e = P->hf_tprev.alloc((size_t)N);
        if (e == hipSuccess) {
            if (d->t_prev) e = hipMemcpyAsync(P->hf_tprev.p, d->t_prev, sizeof(double) * N, hipMemcpyHostToDevice, s);
            else e = hipMemsetAsync(P->hf_tprev.p, 0, sizeof(double) * N, s);
        }
        // pairs of partials: the change norm's over the nodes, a conductor's over its elements
        const size_t chunks = (size_t)(std::max(N, qmax) + kHfQBlock - 1) / kHfQBlock;
        if (e == hipSuccess) e = P->hf_part.alloc(2 * chunks + 4);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) {
            set_error(std::string("upload failed: ") + hipGetErrorString(e));
            return fail(XFK_ERR_HIP);
        }
    }
    return reserve_first_solve(out);
}

int xfk_heatflow(xfk_problem *P, int flags, xfk_result *res)
{
    XFK_REQUIRE(P && P->heat, XFK_ERR_ARG, "not a heat-flow problem (xfk_problem_create_heatflow)");
    ArenaScope arena_scope(&P->arena);
    P->es_solved = false;
    int rc = heat_run(P, flags, res);
    if (rc == XFK_OK) {
        // the heat flow of the prescribed-temperature conductors (hsolver.cpp:846-848)
        for (int c = 0; c < (int)P->hf_cond.size() && rc == XFK_OK; ++c)
            if (P->hf_cond[c].type == 1) rc = conductor_flow(P, c, &P->hf_cond[c].q);
        if (rc == XFK_OK && hipStreamSynchronize(P->stream) != hipSuccess) {
            set_error("heat-flow post-processing failed");
            rc = XFK_ERR_HIP;
        }
        P->es_solved = rc == XFK_OK;
    }
    problem_recycle(P);
    return rc;
}

int xfk_heatflow_assemble(xfk_problem *P, const double *T)
{
    XFK_REQUIRE(P && P->heat, XFK_ERR_ARG, "not a heat-flow problem (xfk_problem_create_heatflow)");
    ArenaScope arena_scope(&P->arena);
    XFK_CHECK(hipSetDevice(P->device));
    hipStream_t s = P->stream;
    int rc = XFK_OK;
    if (!P->symbolic_ready) rc = build_symbolic(P);
    if (rc == XFK_OK) {
        // (Vold: the loop's Vo buffer; the solution in V stays)
        hipError_t e = T ? hipMemcpyAsync(P->Vold.p, T, sizeof(double) * P->N, hipMemcpyHostToDevice, s)
                         : hipMemsetAsync(P->Vold.p, 0, sizeof(double) * P->N, s);
        if (e != hipSuccess) {
            set_error(std::string("upload failed: ") + hipGetErrorString(e));
            rc = XFK_ERR_HIP;
        }
    }
    if (rc == XFK_OK) {
        P->hf_vo = P->Vold.p;
        rc = static_assemble_pass(P, 0);
    }
    if (rc == XFK_OK && hipStreamSynchronize(s) != hipSuccess) {
        set_error("heat-flow assembly failed");
        rc = XFK_ERR_HIP;
    }
    problem_recycle(P);
    return rc;
}

int xfk_heatflow_set_step(xfk_problem *P, double dt, const double *t_prev)
{
    XFK_REQUIRE(P && P->heat, XFK_ERR_ARG, "not a heat-flow problem (xfk_problem_create_heatflow)");
    XFK_REQUIRE(!(dt < 0), XFK_ERR_ARG, "dT must not be negative");
    XFK_REQUIRE(dt == 0 || t_prev, XFK_ERR_ARG, "dT != 0 needs the previous solution (t_prev)");
    XFK_CHECK(hipSetDevice(P->device));
    if (t_prev) {
        XFK_CHECK(hipMemcpyAsync(P->hf_tprev.p, t_prev, sizeof(double) * P->N, hipMemcpyHostToDevice, P->stream));
        XFK_CHECK(hipStreamSynchronize(P->stream));
    }
    P->hf_dt = dt;
    return XFK_OK;
}

int xfk_heatflow_advance(xfk_problem *P, double dt)
{
    XFK_REQUIRE(P && P->heat, XFK_ERR_ARG, "not a heat-flow problem (xfk_problem_create_heatflow)");
    XFK_REQUIRE(!(dt < 0), XFK_ERR_ARG, "dT must not be negative");
    XFK_REQUIRE(P->es_solved, XFK_ERR_ARG, "no solution yet");
    XFK_CHECK(hipSetDevice(P->device));
    XFK_CHECK(hipMemcpyAsync(P->hf_tprev.p, P->V.p, sizeof(double) * P->N, hipMemcpyDeviceToDevice, P->stream));
    XFK_CHECK(hipStreamSynchronize(P->stream));
    P->hf_dt = dt;
    return XFK_OK;
}

int xfk_hf_get_conductors(xfk_problem *P, double *T, double *q)
{
    XFK_REQUIRE(P && P->heat, XFK_ERR_ARG, "not a heat-flow problem");
    XFK_REQUIRE(P->es_solved, XFK_ERR_ARG, "no solution yet");
    XFK_CHECK(hipSetDevice(P->device));
    for (int c = 0; c < (int)P->hf_cond.size(); ++c) {
        if (q) q[c] = P->hf_cond[c].q;
        if (!T) continue;
        T[c] = P->hf_cond[c].T;
        if (P->hf_cond[c].type == 0) {
            T[c] = 0.;   // (a conductor without nodes: the reference's placeholder row)
            if (P->es_cond_rep[c] >= 0)
                XFK_CHECK(d2h(&T[c], P->V.p + P->es_cond_rep[c], sizeof(double), P->stream));
        }
    }
    return XFK_OK;
}

int xfk_hf_conductor_flow(xfk_problem *P, int conductor, double *q)
{
    XFK_REQUIRE(P && P->heat && q, XFK_ERR_ARG, "null argument or not a heat-flow problem");
    XFK_REQUIRE(P->es_solved, XFK_ERR_ARG, "no solution yet");
    XFK_REQUIRE(conductor >= 0 && conductor < (int)P->hf_cond.size(), XFK_ERR_ARG, "conductor index out of range");
    XFK_CHECK(hipSetDevice(P->device));
    return conductor_flow(P, conductor, q);
}

}  // extern "C"
