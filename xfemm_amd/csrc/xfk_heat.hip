// Heat-flow problems on the device: HSolver::AnalyzeProblem
// (reference cfemm/hsolver/hsolver.cpp:458-852) and HSolver::ChargeOnConductor
// (hsolver.cpp:987-1035) for MI355X (gfx950).
//
// What is here: the heat-flow element -- conductivities from the K(T) tables
// at the last solution's nodal temperatures, the lumped capacity term of a
// time step, volume heating, flux / convection / linearised radiation edges
// --, the outer fixed-point loop with its change norm, the per-element
// arithmetic of the heat flow through a conductor, the table packing and the
// C-ABI entry points.  The row gather the element runs in, the merging of a
// CircType 0 conductor (a prescribed total heat flow) onto its representative
// node and the host build from the descriptor are xfk_potential.h's, shared
// with electrostatics.  Everything else is the static path unchanged: the
// symbolic phase, the point-source launch, the Dirichlet kernels, the
// (anti)periodic averaging map and the AMG-PCG, one pass at a time
// (static_assemble_pass / static_pcg_pass).
#include "xfk_potential.h"
#include "xfk_amg.h"

#include <cstdio>

namespace xfk {

constexpr double kKsb = 5.67032e-8;   // Stefan-Boltzmann constant, W/(m^2 K^4) (femmconstants.h)

// One element of HSolver::AnalyzeProblem (hsolver.cpp:546-722), in the
// reference's operation order; lengths in m.
struct HfPhys {
    struct Args {
        const HfBlock *blocks;
        const HfLine *lines;
        const double *tkT, *tkK;   // the K(T) knots of all blocks
        const double *vo;          // the last solution (Vo)
        const double *tprev;       // the previous time step's solution (dt != 0)
        double dt;
    };

    template <bool AXI>
    static __device__ __forceinline__ void element(int e, const int (&g)[3], const RowArgs &A, const Args &S,
                                                   const double (&X)[3], const double (&Y)[3], const PotLabel &lab,
                                                   double (&Me)[3][3], double (&be)[3])
    {
        const HfBlock bp = S.blocks[lab.blk];
        // the last solution and the previous time step's at the element's nodes
        const double Vo[3] = {S.vo[g[0]], S.vo[g[1]], S.vo[g[2]]};
        double Tp[3] = {0., 0., 0.};
        if (S.dt != 0) {
            Tp[0] = S.tprev[g[0]];
            Tp[1] = S.tprev[g[1]];
            Tp[2] = S.tprev[g[2]];
        }
        const int eb = A.ebits[e];   // the element's three packed 10-bit boundary-property fields
        PotGeom G;
        pot_geometry<AXI>(A, X, Y, lab, G);
        const double(&l)[3] = G.l, (&p)[3] = G.p, (&q)[3] = G.q;
        const double a = G.a, kludge = G.kludge;
        double Depth = G.Depth;
        // the conductivities of this element: the mean of GetK at its nodes
        double k0x, k0y, k1x, k1y, k2x, k2y;
        hf_getk(bp, S.tkT, S.tkK, Vo[0], k0x, k0y);
        hf_getk(bp, S.tkT, S.tkK, Vo[1], k1x, k1y);
        hf_getk(bp, S.tkT, S.tkK, Vo[2], k2x, k2y);
        const double knx = (k0x + k1x + k2x) / 3., kny = (k0y + k1y + k2y) / 3.;
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
        if (S.dt != 0) {
            const double K = -Depth * bp.kt * a / (3. * S.dt);
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
                const HfLine ln = S.lines[ej];
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
};

// the outer loop's change norm (hsolver.cpp:827-830): e1 = sum (V - Vo)^2,
// e2 = sum Vo^2, one node per thread, a pair of partials per workgroup
__global__ void __launch_bounds__(kPotQBlock) k_hf_change(int N, const double *__restrict__ V,
                                                          const double *__restrict__ Vo, double *__restrict__ part)
{
    const int t = blockIdx.x * kPotQBlock + threadIdx.x;
    double e1 = 0., e2 = 0.;
    if (t < N) {
        const double v = V[t], vo = Vo[t];
        e1 = (v - vo) * (v - vo);
        e2 = (vo * vo);
    }
    const double e[2] = {e1, e2};
    block_sums<2>(e, part);
}

// HSolver::ChargeOnConductor (hsolver.cpp:987-1035) over the elements touching
// a node of the conductor (els[0 .. n), ascending): one element per thread,
// the conductivities at the solved temperatures of its nodes
// (a pair of partials per workgroup, the second zero: hf_part is laid out in pairs)
__global__ void __launch_bounds__(kPotQBlock) k_hf_flow(int n, const int *__restrict__ els, int conductor,
                                                        const int *__restrict__ pg, const int *__restrict__ lbl,
                                                        const PotLabel *__restrict__ labels,
                                                        const HfBlock *__restrict__ blocks,
                                                        const double *__restrict__ tkT,
                                                        const double *__restrict__ tkK,
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
    const double z[2] = {Z, 0.};
    block_sums<2>(z, part);
}

void launch_heat_rows(hipStream_t s, xfk_problem *P)
{
    launch_pot_rows<HfPhys>(s, P, HfPhys::Args{P->hf_blocks.p, P->hf_lines.p, P->hf_tk_T.p, P->hf_tk_K.p, P->hf_vo,
                                               P->hf_tprev.p, P->hf_dt});
}

// the heat flow through one conductor into *q_host (host-synchronising;
// hf_part holds the largest conductor's pairs + 1)
static int conductor_flow(xfk_problem *P, int c, double *q_host)
{
    return conductor_integral<2>(P, c, P->hf_part.p, q_host, [&](int G, int n, const int *els, double *part) {
        k_hf_flow<<<G, kPotQBlock, 0, P->stream>>>(n, els, c, P->pot_p.p, P->lbl_raw.p, P->pot_labels.p,
                                                   P->hf_blocks.p, P->hf_tk_T.p, P->hf_tk_K.p, P->x.p, P->y.p,
                                                   P->V.p, P->pot_node_cond.p, P->axi ? 1 : 0, P->pot_depth, part);
    });
}

// the heat flow of the prescribed-temperature conductors from the solution in
// V (hsolver.cpp:846-848); also after xfk_pot_set_solution
int heat_conductor_integrals(xfk_problem *P)
{
    int rc = XFK_OK;
    for (int c = 0; c < (int)P->hf_cond.size() && rc == XFK_OK; ++c)
        if (P->hf_cond[c].type == 1) rc = conductor_flow(P, c, &P->hf_cond[c].q);
    return rc;
}

// HSolver's units[] (hsolver.cpp:65): user length units -> m
static const double kHfUnits[] = {0.0254, 0.001, 0.01, 1, 2.54e-5, 1.e-6};

// what the descriptor calls the fixed values, and its sources (unscaled)
struct HfTraits {
    static double point_value(const xfk_hf_point_desc &p) { return p.T; }
    static double conductor_value(const xfk_hf_conductor_desc &c) { return c.T; }
    static double line_value(const xfk_hf_line_desc &l) { return l.Tset; }
    static double point_source(double Depth, double qp) { return (Depth * qp); }
    static double conductor_source(double q) { return q; }
};

// (after the shared checks: the block table is there)
static int validate_hf(const xfk_hf_problem_desc *d)
{
    const int rc = validate_potential(d, "0 (heat flow) or 1 (temperature)");
    if (rc != XFK_OK) return rc;
    // (the reference resets dT to 0 with a warning when the previous solution
    // cannot be loaded, and solves another problem than the one asked for)
    XFK_REQUIRE(!(d->dt < 0), XFK_ERR_ARG, "dT must not be negative");
    XFK_REQUIRE(d->dt == 0 || d->t_prev, XFK_ERR_ARG, "dT != 0 needs the previous solution (t_prev)");
    for (int k = 0; k < d->n_blocks; ++k) {
        XFK_REQUIRE(d->blocks[k].npts >= 0, XFK_ERR_ARG, "K(T) table with a negative number of points");
        XFK_REQUIRE(d->blocks[k].npts == 0 || (d->blocks[k].T && d->blocks[k].K), XFK_ERR_ARG,
                    "K(T) table without its T or K array");
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
    const int G = (N + kPotQBlock - 1) / kPotQBlock;
    double *part = P->hf_part.p, *sums = P->hf_part.p + 2 * (size_t)G;
    XFK_CHECK(hipMemsetAsync(P->V.p, 0, sizeof(double) * P->NL, s));   // CBigLinProb::Create: V = 0
    P->amg_reusable = false;   // a hierarchy is reused only inside one solve
    P->pc_used = XFK_PRECOND_JACOBI;
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
        if (Iter > 0) launch_pot_set_slaves(P, 1);   // (the warm start of their identity rows)
        XFK_CHECK(hipEventRecord(P->pass_ev[3 * Iter + 1], s));
        rc = static_pcg_pass(P, Iter);   // L.PCGSolve(iter++)
        if (rc != XFK_OK) return rc;
        XFK_CHECK(hipEventRecord(P->pass_ev[3 * Iter + 2], s));
        R.cg_iters += P->pcg_host->iters;
        R.final_er = P->pcg_host->er;
        P->amg_last_iters = P->pcg_host->iters - P->pcg_discarded;
        if (P->amg_fresh) P->amg_fresh_iters = P->pcg_host->iters - P->pcg_discarded;
        launch_pot_set_slaves(P, 0);
        again = false;
        if (P->hf_nonlinear) {
            double e[2] = {0., 0.};
            k_hf_change<<<G, kPotQBlock, 0, s>>>(N, P->V.p, P->Vold.p, part);
            k_pot_sum<2><<<1, kPotQBlock, 0, s>>>(G, part, sums);
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
    return hipFuncGetAttributes(&a, reinterpret_cast<const void *>(&k_pot_set_slaves));
}

extern "C" {

int xfk_problem_create_heatflow(const xfk_hf_problem_desc *d, int device, xfk_problem **out)
{
    XFK_REQUIRE(d && out, XFK_ERR_ARG, "null argument");
    *out = nullptr;
    int rc = validate_hf(d);
    if (rc == XFK_OK) rc = check_device(device);
    if (rc != XFK_OK) return rc;
    const int N = d->n_nodes;
    PotentialPrep prep;
    prepare_potential<HfTraits>(d, kHfUnits[d->length_units], prep);   // (hsolver.cpp:471-474: m)
    const std::vector<HfLine> lin = potential_lines<HfLine>(
        d, prep, [](const xfk_hf_line_desc &l) { return HfLine{l.qs, l.beta, l.h, l.Tinf, l.format, 0}; });
    // a radiation edge (hsolver.cpp:673), or a K(T) table on the block of ANY
    // element (the reference's scan reads the blocks of the first NumNodes
    // elements only: INTEGRATION.md)
    bool nonlinear = false;
    for (const HfLine &l : lin) nonlinear |= l.format == 3;
    for (long long i = 0; i < d->n_elems && !nonlinear; ++i)
        nonlinear = d->blocks[d->labels[d->lbl[i]].block].npts > 0;

    // the K(T) tables of all blocks in one array, an offset and a count per block
    std::vector<HfBlock> blk(d->n_blocks);
    std::vector<double> tkT, tkK;
    for (int k = 0; k < d->n_blocks; ++k) {
        const xfk_hf_block_desc &b = d->blocks[k];
        blk[k] = HfBlock{b.kx, b.ky, b.kt, b.qv, b.npts, (int)tkT.size()};
        tkT.insert(tkT.end(), b.T, b.T + (b.npts > 0 ? b.npts : 0));
        tkK.insert(tkK.end(), b.K, b.K + (b.npts > 0 ? b.npts : 0));
    }

    return create_potential(d, prep, device, out, [&](xfk_problem *P, hipStream_t s) {
        P->heat = true;
        P->hf_nonlinear = nonlinear;
        P->hf_dt = d->dt;
        P->hf_cond.assign(d->conductors, d->conductors + d->n_conductors);
        for (auto &c : P->hf_cond)
            if (c.type == 1) c.q = 0;
        hipError_t e = upload(P->hf_blocks, blk.data(), blk.size(), s);
        if (e == hipSuccess) e = upload(P->hf_lines, lin.data(), lin.size(), s);
        if (e == hipSuccess) e = upload(P->hf_tk_T, tkT.data(), tkT.size(), s);
        if (e == hipSuccess) e = upload(P->hf_tk_K, tkK.data(), tkK.size(), s);
        if (e == hipSuccess) e = P->hf_tprev.alloc((size_t)N);
        if (e == hipSuccess) {
            if (d->t_prev) e = hipMemcpyAsync(P->hf_tprev.p, d->t_prev, sizeof(double) * N, hipMemcpyHostToDevice, s);
            else e = hipMemsetAsync(P->hf_tprev.p, 0, sizeof(double) * N, s);
        }
        // pairs of partials: the change norm's over the nodes, a conductor's over its elements
        const size_t chunks = (size_t)(std::max(N, prep.qmax) + kPotQBlock - 1) / kPotQBlock;
        if (e == hipSuccess) e = P->hf_part.alloc(2 * chunks + 4);
        return e;
    });
}

int xfk_heatflow(xfk_problem *P, int flags, xfk_result *res)
{
    XFK_REQUIRE(P && P->heat, XFK_ERR_ARG, "not a heat-flow problem (xfk_problem_create_heatflow)");
    XFK_REQUIRE(!P->pot_from_file, XFK_ERR_UNSUPPORTED,
                "the problem was opened from a solution file: it carries no boundary conditions to solve with");
    ArenaScope arena_scope(&P->arena);
    P->pot_solved = false;
    pp_invalidate(P);
    int rc = heat_run(P, flags, res);
    if (rc == XFK_OK) {
        rc = heat_conductor_integrals(P);
        if (rc == XFK_OK && hipStreamSynchronize(P->stream) != hipSuccess) {
            set_error("heat-flow post-processing failed");
            rc = XFK_ERR_HIP;
        }
        P->pot_solved = rc == XFK_OK;
    }
    problem_recycle(P);
    return rc;
}

int xfk_heatflow_assemble(xfk_problem *P, const double *T)
{
    XFK_REQUIRE(P && P->heat, XFK_ERR_ARG, "not a heat-flow problem (xfk_problem_create_heatflow)");
    XFK_REQUIRE(!P->pot_from_file, XFK_ERR_UNSUPPORTED,
                "the problem was opened from a solution file: it carries no boundary conditions to solve with");
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
    XFK_REQUIRE(P->pot_solved, XFK_ERR_ARG, "no solution yet");
    XFK_CHECK(hipSetDevice(P->device));
    XFK_CHECK(hipMemcpyAsync(P->hf_tprev.p, P->V.p, sizeof(double) * P->N, hipMemcpyDeviceToDevice, P->stream));
    XFK_CHECK(hipStreamSynchronize(P->stream));
    P->hf_dt = dt;
    return XFK_OK;
}

int xfk_hf_get_conductors(xfk_problem *P, double *T, double *q)
{
    XFK_REQUIRE(P && P->heat, XFK_ERR_ARG, "not a heat-flow problem");
    XFK_REQUIRE(P->pot_solved, XFK_ERR_ARG, "no solution yet");
    return get_conductor_values<HfTraits>(P, P->hf_cond, T, q);
}

int xfk_hf_conductor_flow(xfk_problem *P, int conductor, double *q)
{
    XFK_REQUIRE(P && P->heat && q, XFK_ERR_ARG, "null argument or not a heat-flow problem");
    XFK_REQUIRE(P->pot_solved, XFK_ERR_ARG, "no solution yet");
    XFK_REQUIRE(conductor >= 0 && conductor < (int)P->hf_cond.size(), XFK_ERR_ARG, "conductor index out of range");
    XFK_CHECK(hipSetDevice(P->device));
    return conductor_flow(P, conductor, q);
}

}  // extern "C"
