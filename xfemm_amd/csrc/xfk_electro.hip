// Electrostatic problems on the device: ESolver::AnalyzeProblem
// (reference cfemm/esolver/esolver.cpp:389-646) and ESolver::ChargeOnConductor
// (esolver.cpp:797-844) for MI355X (gfx950).
//
// What is here: the electrostatic element with its boundary terms, the
// per-element arithmetic of the charge integral, the conductor table and the
// C-ABI entry points.  The row gather the element runs in, the merging of a
// floating conductor (CircType 0) onto its representative node and the host
// build from the descriptor are xfk_potential.h's, shared with heat flow.
// Everything else is the static magnetics path unchanged: the symbolic phase,
// the point-source launch (point charges, and the charge of a floating
// conductor on its row), the Dirichlet kernels (point properties with
// qp == 0, prescribed-voltage conductors, BdryFormat 0 edges), the
// (anti)periodic averaging map and the AMG-PCG (static2d_run, one pass).
#include "xfk_potential.h"

namespace xfk {

constexpr double kEo = 8.85418781762e-12;   // femmconstants.h:24
constexpr double kEsC = (1.e-6) / kEo;       // esolver.cpp:398

// One element of ESolver::AnalyzeProblem (esolver.cpp:448-548), in the
// reference's operation order; lengths in mm.
struct EsPhys {
    struct Args {
        const EsBlock *blocks;
        const EsLine *lines;
    };

    template <bool AXI>
    static __device__ __forceinline__ void element(int e, const int (&g)[3], const RowArgs &A, const Args &S,
                                                   const double (&X)[3], const double (&Y)[3], const PotLabel &lab,
                                                   double (&Me)[3][3], double (&be)[3])
    {
        const EsBlock bp = S.blocks[lab.blk];
        const int eb = A.ebits[e];   // the element's three packed 10-bit boundary-property fields
        PotGeom G;
        pot_geometry<AXI>(A, X, Y, lab, G);
        const double(&l)[3] = G.l, (&p)[3] = G.p, (&q)[3] = G.q;
        const double a = G.a, kludge = G.kludge;
        double Depth = G.Depth;
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
                const EsLine ln = S.lines[ej];
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
};

// ESolver::ChargeOnConductor (esolver.cpp:797-844) over the elements touching
// a node of the conductor (els[0 .. n), ascending): one element per thread,
// the workgroup's sum (wave shuffles, then the waves in order) into part[wg]
__global__ void __launch_bounds__(kPotQBlock) k_es_charge(int n, const int *__restrict__ els, int conductor,
                                                          const int *__restrict__ pg, const int *__restrict__ lbl,
                                                          const PotLabel *__restrict__ labels,
                                                          const EsBlock *__restrict__ blocks,
                                                          const double *__restrict__ x, const double *__restrict__ y,
                                                          const double *__restrict__ V,
                                                          const int *__restrict__ node_cond, int axi, double depth,
                                                          double *__restrict__ part)
{
    const int t = blockIdx.x * kPotQBlock + threadIdx.x;
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
    const double z[1] = {Z};
    block_sums<1>(z, part);
}

void launch_electro_rows(hipStream_t s, xfk_problem *P)
{
    launch_pot_rows<EsPhys>(s, P, EsPhys::Args{P->es_blocks.p, P->es_lines.p});
}

// the charge integral of one conductor into *q_host (host-synchronising;
// es_qpart holds the largest conductor's partials + 1)
static int conductor_charge(xfk_problem *P, int c, double *q_host)
{
    return conductor_integral<1>(P, c, P->es_qpart.p, q_host, [&](int G, int n, const int *els, double *part) {
        k_es_charge<<<G, kPotQBlock, 0, P->stream>>>(n, els, c, P->pot_p.p, P->lbl_raw.p, P->pot_labels.p,
                                                     P->es_blocks.p, P->x.p, P->y.p, P->V.p, P->pot_node_cond.p,
                                                     P->axi ? 1 : 0, P->pot_depth, part);
    });
}

// the charge of the prescribed-voltage conductors from the solution in V
// (esolver.cpp:641-643); also after xfk_pot_set_solution
int electro_conductor_integrals(xfk_problem *P)
{
    int rc = XFK_OK;
    for (int c = 0; c < (int)P->es_cond.size() && rc == XFK_OK; ++c)
        if (P->es_cond[c].type == 1) rc = conductor_charge(P, c, &P->es_cond[c].q);
    return rc;
}

// ESolver's units[] (esolver.cpp:65): user length units -> mm
static const double kEsUnits[] = {25.4, 1., 10., 1000., 0.0254, 0.001};

// what the descriptor calls the fixed values, and the scaling of its sources
struct EsTraits {
    static double point_value(const xfk_es_point_desc &p) { return p.V; }
    static double conductor_value(const xfk_es_conductor_desc &c) { return c.V; }
    static double line_value(const xfk_es_line_desc &l) { return l.V; }
    static double point_source(double Depth, double qp) { return ((1.e6) * Depth * kEsC * qp); }
    static double conductor_source(double q) { return (1.e9) * kEsC * q; }
};

}  // namespace xfk

using namespace xfk;

hipError_t xfk::warm_module_electro()
{
    hipFuncAttributes a;
    return hipFuncGetAttributes(&a, reinterpret_cast<const void *>(&k_pot_set_slaves));
}

extern "C" {

int xfk_problem_create_electrostatic(const xfk_es_problem_desc *d, int device, xfk_problem **out)
{
    XFK_REQUIRE(d && out, XFK_ERR_ARG, "null argument");
    *out = nullptr;
    int rc = validate_potential(d, "0 (charge) or 1 (voltage)");
    if (rc == XFK_OK) rc = check_device(device);
    if (rc != XFK_OK) return rc;
    PotentialPrep prep;
    prepare_potential<EsTraits>(d, kEsUnits[d->length_units], prep);   // (esolver.cpp:399-402: mm)
    const std::vector<EsLine> lin = potential_lines<EsLine>(
        d, prep, [](const xfk_es_line_desc &l) { return EsLine{l.c0, l.c1, l.qs, l.format, 0}; });
    std::vector<EsBlock> blk(d->n_blocks);
    for (int k = 0; k < d->n_blocks; ++k) blk[k] = EsBlock{d->blocks[k].ex, d->blocks[k].ey, d->blocks[k].qv};
    return create_potential(d, prep, device, out, [&](xfk_problem *P, hipStream_t s) {
        P->electro = true;
        P->es_cond.assign(d->conductors, d->conductors + d->n_conductors);
        for (auto &c : P->es_cond)
            if (c.type == 1) c.q = 0;
        hipError_t e = upload(P->es_blocks, blk.data(), blk.size(), s);
        if (e == hipSuccess) e = upload(P->es_lines, lin.data(), lin.size(), s);
        if (e == hipSuccess) e = P->es_qpart.alloc((size_t)(prep.qmax + kPotQBlock - 1) / kPotQBlock + 2);
        return e;
    });
}

int xfk_electrostatic(xfk_problem *P, int flags, xfk_result *res)
{
    XFK_REQUIRE(P && P->electro, XFK_ERR_ARG, "not an electrostatic problem (xfk_problem_create_electrostatic)");
    XFK_REQUIRE(!P->pot_from_file, XFK_ERR_UNSUPPORTED,
                "the problem was opened from a solution file: it carries no boundary conditions to solve with");
    ArenaScope arena_scope(&P->arena);
    P->pot_solved = false;
    pp_invalidate(P);
    int rc = static2d_run(P, flags, res);
    if (rc == XFK_OK) {
        launch_pot_set_slaves(P, 0);
        rc = electro_conductor_integrals(P);
        if (rc == XFK_OK && hipStreamSynchronize(P->stream) != hipSuccess) {
            set_error("electrostatic post-processing failed");
            rc = XFK_ERR_HIP;
        }
        P->pot_solved = rc == XFK_OK;
    }
    problem_recycle(P);
    return rc;
}

int xfk_get_conductors(xfk_problem *P, double *V, double *q)
{
    XFK_REQUIRE(P && P->electro, XFK_ERR_ARG, "not an electrostatic problem");
    XFK_REQUIRE(P->pot_solved, XFK_ERR_ARG, "no solution yet");
    return get_conductor_values<EsTraits>(P, P->es_cond, V, q);
}

int xfk_conductor_charge(xfk_problem *P, int conductor, double *q)
{
    XFK_REQUIRE(P && P->electro && q, XFK_ERR_ARG, "null argument or not an electrostatic problem");
    XFK_REQUIRE(P->pot_solved, XFK_ERR_ARG, "no solution yet");
    XFK_REQUIRE(conductor >= 0 && conductor < (int)P->es_cond.size(), XFK_ERR_ARG, "conductor index out of range");
    XFK_CHECK(hipSetDevice(P->device));
    return conductor_charge(P, conductor, q);
}

}  // extern "C"
