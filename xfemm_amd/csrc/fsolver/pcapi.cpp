// extern "C" surface of ESolver and HSolver (include/xfemm_psolver.h): one
// set of bodies over PSolver, instantiated under the two prefixes.
#include "../../../include/xfemm_psolver.h"

#include <new>
#include <stdexcept>
#include <string>

#include "psolver.h"

struct xfemm_esolver {
    xfemm::ESolver s;
};
struct xfemm_hsolver {
    xfemm::HSolver s;
};

namespace {

using xfemm::PSolver;

// No C++ exception crosses the C-ABI: a host allocation failure (or any
// other exception) of a step becomes its false return, with the reason in
// last_error.
template <class F>
int guarded(PSolver *s, F &&f)
{
    if (!s) return 0;
    try {
        return f() ? 1 : 0;
    } catch (const std::bad_alloc &) {
        s->join_removals();
        s->lastError = "out of host memory\n";
    } catch (const std::exception &e) {
        s->join_removals();
        s->lastError = std::string(e.what()) + "\n";
    }
    s->WarnMessage("%s", s->lastError.c_str());
    return 0;
}

int set_pathname(PSolver *s, const char *path)
{
    if (!s || !path) return 0;
    std::string p(path);
    const std::string ext = s->input_ext();
    if (p.size() > 4 && p.compare(p.size() - 4, 4, ext) == 0) p.resize(p.size() - 4);
    s->PathName = p;
    return 1;
}

int load_mesh(PSolver *s)
{
    return guarded(s, [&] {
        xfemm::LoadMeshErr err = s->LoadMesh(s->deleteMeshFiles);
        s->join_removals();
        if (err != xfemm::NOERROR) {
            s->lastError = PSolver::getErrorString(err);
            return false;
        }
        return true;
    });
}

int cuthill(PSolver *s)
{
    return guarded(s, [&] {
        const int ok = s->Cuthill(s->deleteMeshFiles);
        s->join_removals();
        return ok != 0;
    });
}

int get_nodes(PSolver *s, double *x, double *y, int *marker, int *conductor)
{
    if (!s) return 0;
    for (int i = 0; i < s->NumNodes; i++) {
        if (x) x[i] = s->meshnode[i].x;
        if (y) y[i] = s->meshnode[i].y;
        if (marker) marker[i] = s->meshnode[i].BoundaryMarker;
        if (conductor) conductor[i] = s->meshnode[i].InConductor;
    }
    return 1;
}

int get_element_edges(PSolver *s, int *e)
{
    if (!s || !e) return 0;
    for (int i = 0; i < s->NumEls; i++)
        for (int q = 0; q < 3; q++) e[3 * i + q] = s->meshele[i].e[q];
    return 1;
}

int get_pbcs(PSolver *s, int *pbc3)
{
    if (!s || !pbc3) return 0;
    for (int k = 0; k < s->NumPBCs; k++) {
        pbc3[3 * k] = s->pbclist[k].x;
        pbc3[3 * k + 1] = s->pbclist[k].y;
        pbc3[3 * k + 2] = s->pbclist[k].t;
    }
    return 1;
}

int get_solution(PSolver *s, double *x, double *y, double *V, int *Q)
{
    if (!s || (int)s->V.size() != s->NumNodes || (int)s->Q.size() != s->NumNodes) return 0;
    const double cf = s->unit();
    for (int i = 0; i < s->NumNodes; i++) {
        if (x) x[i] = s->meshnode[i].x / cf;
        if (y) y[i] = s->meshnode[i].y / cf;
        if (V) V[i] = s->V[i];
        if (Q) Q[i] = s->Q[i];
    }
    return 1;
}

int get_elements(PSolver *s, int *p, int *lbl)
{
    if (!s) return 0;
    for (int i = 0; i < s->NumEls; i++) {
        for (int q = 0; q < 3; q++)
            if (p) p[3 * i + q] = s->meshele[i].p[q];
        if (lbl) lbl[i] = s->meshele[i].lbl;
    }
    return 1;
}

int get_conductors(PSolver *s, double *V, double *q)
{
    if (!s || s->condV.size() != s->circproplist.size()) return 0;
    for (size_t i = 0; i < s->condV.size(); i++) {
        if (V) V[i] = s->condV[i];
        if (q) q[i] = s->condq[i];
    }
    return 1;
}

int get_header(PSolver *s, double *o)
{
    if (!s || !o) return 0;
    o[0] = s->Precision;
    o[1] = s->Depth;
    o[2] = (double)s->LengthUnits;
    o[3] = (double)s->ProblemTypeV;
    o[4] = s->extZo;
    o[5] = s->extRo;
    o[6] = s->extRi;
    o[7] = s->dT;
    return 1;
}

int get_point_prop(PSolver *s, int k, double *o)
{
    if (!s || !o || k < 0 || k >= (int)s->nodeproplist.size()) return -1;
    o[0] = s->nodeproplist[k].V;
    o[1] = s->nodeproplist[k].qp;
    return 2;
}

int get_line_prop(PSolver *s, int k, double *o)
{
    if (!s || !o || k < 0 || k >= (int)s->lineproplist.size()) return -1;
    const xfemm::CPBoundaryProp &b = s->lineproplist[k];
    const double v[8] = {(double)b.BdryFormat, b.V, b.qs, b.c0, b.c1, b.beta, b.h, b.Tinf};
    for (int i = 0; i < 8; i++) o[i] = v[i];
    return 8;
}

int get_block_prop(PSolver *s, int k, double *o)
{
    if (!s || !o || k < 0 || k >= (int)s->blockproplist.size()) return -1;
    const xfemm::CPMaterialProp &m = s->blockproplist[k];
    const double v[5] = {m.kx, m.ky, m.Kt, m.qv, (double)m.T.size()};
    for (int i = 0; i < 5; i++) o[i] = v[i];
    return 5;
}

int get_conductor_prop(PSolver *s, int k, double *o)
{
    if (!s || !o || k < 0 || k >= (int)s->circproplist.size()) return -1;
    o[0] = (double)s->circproplist[k].CircType;
    o[1] = s->circproplist[k].V;
    o[2] = s->circproplist[k].q;
    return 3;
}

int get_block_label(PSolver *s, int k, double *o)
{
    if (!s || !o || k < 0 || k >= (int)s->labellist.size()) return -1;
    o[0] = (double)s->labellist[k].BlockType;
    o[1] = s->labellist[k].IsExternal ? 1. : 0.;
    o[2] = s->labellist[k].IsDefault ? 1. : 0.;
    return 3;
}

int get_block_table(PSolver *s, int k, double *T, double *K)
{
    if (!s || k < 0 || k >= (int)s->blockproplist.size()) return -1;
    const xfemm::CPMaterialProp &m = s->blockproplist[k];
    for (size_t i = 0; i < m.T.size(); i++) {
        if (T) T[i] = m.T[i];
        if (K) K[i] = m.K[i];
    }
    return (int)m.T.size();
}

}  // namespace

#define S(h) ((h) ? static_cast<PSolver *>(&(h)->s) : nullptr)

#define XFEMM_PSOLVER_CAPI(NAME)                                                                                       \
    xfemm_##NAME *xfemm_##NAME##_create(void)                                                                          \
    {                                                                                                                  \
        try {                                                                                                          \
            return new xfemm_##NAME();                                                                                 \
        } catch (...) {                                                                                                \
            return nullptr;                                                                                            \
        }                                                                                                              \
    }                                                                                                                  \
    void xfemm_##NAME##_destroy(xfemm_##NAME *h) { delete h; }                                                         \
    void xfemm_##NAME##_set_message_handlers(xfemm_##NAME *h, xfemm_message_fn warn, xfemm_message_fn print)           \
    {                                                                                                                  \
        if (!h) return;                                                                                                \
        if (warn) h->s.WarnMessage = warn;                                                                             \
        if (print) h->s.PrintMessage = print;                                                                          \
    }                                                                                                                  \
    int xfemm_##NAME##_set_pathname(xfemm_##NAME *h, const char *path) { return set_pathname(S(h), path); }           \
    int xfemm_##NAME##_set_device(xfemm_##NAME *h, int device)                                                         \
    {                                                                                                                  \
        if (!h || device < 0) return 0;                                                                                \
        h->s.device = device;                                                                                          \
        return 1;                                                                                                      \
    }                                                                                                                  \
    int xfemm_##NAME##_set_delete_mesh_files(xfemm_##NAME *h, int del)                                                 \
    {                                                                                                                  \
        if (!h) return 0;                                                                                              \
        h->s.deleteMeshFiles = del != 0;                                                                               \
        return 1;                                                                                                      \
    }                                                                                                                  \
    int xfemm_##NAME##_load_problem_file(xfemm_##NAME *h)                                                              \
    {                                                                                                                  \
        return guarded(S(h), [&] { return h->s.LoadProblemFile(); });                                                  \
    }                                                                                                                  \
    int xfemm_##NAME##_run_solver(xfemm_##NAME *h, int verbose)                                                        \
    {                                                                                                                  \
        return guarded(S(h), [&] { return h->s.runSolver(verbose != 0); });                                            \
    }                                                                                                                  \
    int xfemm_##NAME##_load_mesh(xfemm_##NAME *h) { return load_mesh(S(h)); }                                          \
    int xfemm_##NAME##_cuthill(xfemm_##NAME *h) { return cuthill(S(h)); }                                              \
    int xfemm_##NAME##_get_nodes(xfemm_##NAME *h, double *x, double *y, int *marker, int *conductor)                   \
    {                                                                                                                  \
        return get_nodes(S(h), x, y, marker, conductor);                                                               \
    }                                                                                                                  \
    int xfemm_##NAME##_get_element_edges(xfemm_##NAME *h, int *e) { return get_element_edges(S(h), e); }              \
    int xfemm_##NAME##_get_pbcs(xfemm_##NAME *h, int *pbc3) { return get_pbcs(S(h), pbc3); }                          \
    int xfemm_##NAME##_num_pbcs(xfemm_##NAME *h) { return h ? h->s.NumPBCs : 0; }                                      \
    int xfemm_##NAME##_bandwidth(xfemm_##NAME *h) { return h ? h->s.BandWidth : 0; }                                   \
    int xfemm_##NAME##_num_nodes(xfemm_##NAME *h) { return h ? h->s.NumNodes : 0; }                                    \
    int xfemm_##NAME##_num_elements(xfemm_##NAME *h) { return h ? h->s.NumEls : 0; }                                   \
    int xfemm_##NAME##_get_solution(xfemm_##NAME *h, double *x, double *y, double *V, int *Q)                          \
    {                                                                                                                  \
        return get_solution(S(h), x, y, V, Q);                                                                         \
    }                                                                                                                  \
    int xfemm_##NAME##_get_elements(xfemm_##NAME *h, int *p, int *lbl) { return get_elements(S(h), p, lbl); }         \
    int xfemm_##NAME##_num_conductors(xfemm_##NAME *h) { return h ? (int)h->s.circproplist.size() : -1; }             \
    int xfemm_##NAME##_get_conductors(xfemm_##NAME *h, double *V, double *q) { return get_conductors(S(h), V, q); }   \
    int xfemm_##NAME##_get_stats(xfemm_##NAME *h, xfk_result *out)                                                     \
    {                                                                                                                  \
        if (!h || !out) return 0;                                                                                      \
        *out = h->s.stats;                                                                                             \
        return 1;                                                                                                      \
    }                                                                                                                  \
    int xfemm_##NAME##_get_times(xfemm_##NAME *h, double *ms)                                                          \
    {                                                                                                                  \
        if (!h || !ms) return 0;                                                                                       \
        for (int k = 0; k < 5; ++k) ms[k] = h->s.ms_phase[k];                                                          \
        return 1;                                                                                                      \
    }                                                                                                                  \
    const char *xfemm_##NAME##_last_error(xfemm_##NAME *h) { return h ? h->s.lastError.c_str() : ""; }                \
    xfk_problem *xfemm_##NAME##_problem(xfemm_##NAME *h) { return h ? h->s.problem() : nullptr; }                      \
    int xfemm_##NAME##_get_header(xfemm_##NAME *h, double *out8) { return get_header(S(h), out8); }                   \
    int xfemm_##NAME##_num_line_props(xfemm_##NAME *h) { return h ? (int)h->s.lineproplist.size() : -1; }             \
    int xfemm_##NAME##_num_node_props(xfemm_##NAME *h) { return h ? (int)h->s.nodeproplist.size() : -1; }             \
    int xfemm_##NAME##_num_block_props(xfemm_##NAME *h) { return h ? (int)h->s.blockproplist.size() : -1; }           \
    int xfemm_##NAME##_num_block_labels(xfemm_##NAME *h) { return h ? (int)h->s.labellist.size() : -1; }              \
    int xfemm_##NAME##_get_point_prop(xfemm_##NAME *h, int k, double *o) { return get_point_prop(S(h), k, o); }       \
    int xfemm_##NAME##_get_line_prop(xfemm_##NAME *h, int k, double *o) { return get_line_prop(S(h), k, o); }         \
    int xfemm_##NAME##_get_block_prop(xfemm_##NAME *h, int k, double *o) { return get_block_prop(S(h), k, o); }       \
    int xfemm_##NAME##_get_conductor_prop(xfemm_##NAME *h, int k, double *o)                                           \
    {                                                                                                                  \
        return get_conductor_prop(S(h), k, o);                                                                         \
    }                                                                                                                  \
    int xfemm_##NAME##_get_block_label(xfemm_##NAME *h, int k, double *o) { return get_block_label(S(h), k, o); }     \
    int xfemm_##NAME##_get_block_table(xfemm_##NAME *h, int k, double *T, double *K)                                   \
    {                                                                                                                  \
        return get_block_table(S(h), k, T, K);                                                                         \
    }

extern "C" {

XFEMM_PSOLVER_CAPI(esolver)
XFEMM_PSOLVER_CAPI(hsolver)

int xfemm_hsolver_set_previous_solution(xfemm_hsolver *h, const double *T, int n)
{
    return guarded(S(h), [&] { return h->s.set_previous_solution(T, n); });
}

const char *xfemm_hsolver_previous_solution_file(xfemm_hsolver *h)
{
    return h ? h->s.previousSolutionFile.c_str() : "";
}

}  // extern "C"
