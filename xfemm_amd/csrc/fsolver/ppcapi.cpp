// EPProc / HPProc: the reference's file-based post-processors
// (cfemm/epproc/epproc.cpp, cfemm/hpproc/hpproc.cpp, libfemm/PostProcessor.cpp)
// over the device post-processing of include/xfemm_kernels.h (xfk_pot_*), and
// their extern "C" surface (include/xfemm_pproc.h): one set of bodies,
// instantiated under the two prefixes.
#include "../../../include/xfemm_pproc.h"

#include <algorithm>
#include <new>
#include <stdexcept>
#include <string>

#include "meshhost.h"
#include "pproc.h"

namespace {

using namespace xfemm;

// user length units -> the solvers' (mm: esolver.cpp:65, m: hsolver.cpp:65):
// the descriptors take the solvers' coordinates, the post-processing divides
// them back by the same unit
constexpr double kUnitsE[] = {25.4, 1., 10., 1000., 0.0254, 0.001};
constexpr double kUnitsH[] = {0.0254, 0.001, 0.01, 1, 2.54e-5, 1.e-6};

struct PProc {
    explicit PProc(PotentialKind k) : kind(k), WarnMessage(&PrintWarningMsg), PrintMessage(&PrintWarningMsg) {}
    ~PProc() { drop(); }
    PProc(const PProc &) = delete;
    PProc &operator=(const PProc &) = delete;

    const PotentialKind kind;
    int (*WarnMessage)(const char *, ...);
    int (*PrintMessage)(const char *, ...);
    int device = 0;
    std::string lastError;
    SolutionFile file;
    bool have_file = false;
    xfk_problem *prob = nullptr;
    std::vector<unsigned char> selected;   // per block label
    bool smooth = true;                    // PostProcessor::Smooth
    bool multiply_defined = false;
    ContourHost contour;
    ElementWalk walk;                      // PostProcessor::InTriangle's memory of the element found last

    void drop()
    {
        if (prob) xfk_problem_destroy(prob);
        prob = nullptr;
    }
    bool fail(const std::string &m)
    {
        lastError = m;
        WarnMessage("%s\n", m.c_str());
        return false;
    }
    bool xfk(int rc)
    {
        if (rc == XFK_OK) return true;
        return fail(std::string("GPU post-processing error: ") + xfk_last_error());
    }
    bool need_doc() { return prob ? true : fail("no document is open (open_document)"); }

    bool read(const char *path)
    {
        drop();
        have_file = false;
        contour.clear();
        selected.clear();
        multiply_defined = false;
        if (!path) return fail("null path");
        std::string err;
        if (!ReadSolutionFile(path, kind, file, err)) return fail(err);
        have_file = true;
        selected.assign(file.labellist.size(), 0);
        walk.build(file);
        return true;
    }

    template <class D>
    void fill(D &d, std::vector<double> &x, std::vector<double> &y, std::vector<int> &cond)
    {
        const int N = file.NumNodes;
        const double cf = (kind == POT_HEATFLOW ? kUnitsH : kUnitsE)[file.LengthUnits];
        x.resize(N);
        y.resize(N);
        cond.resize(N);
        for (int i = 0; i < N; ++i) {
            x[i] = file.x[i] * cf;
            y[i] = file.y[i] * cf;
            cond[i] = file.Q[i] >= 0 ? file.Q[i] : -1;
        }
        d.n_nodes = N; d.x = x.data(); d.y = y.data(); d.marker = nullptr; d.conductor = cond.data();
        // (no edge codes: the file has none and post-processing reads none)
        d.n_elems = file.NumEls; d.p = file.p.data(); d.e = nullptr; d.lbl = file.lbl.data();
        d.n_pbc = 0; d.pbc = nullptr;
        d.precision = file.Precision;
        d.length_units = (int)file.LengthUnits;
        d.problem_type = file.ProblemTypeV == AXISYMMETRIC ? XFK_AXISYMMETRIC : XFK_PLANAR;
        d.depth = file.Depth;
        d.ext_zo = file.extZo;
        d.ext_ro = file.extRo;
        d.ext_ri = file.extRi;
    }

    bool open(const char *path)
    {
        if (!read(path)) return false;
        if (file.NumNodes < 1 || file.NumEls < 1) return fail(std::string(path) + ": the solution has no mesh");
        if (file.blockproplist.empty()) return fail(std::string(path) + ": no block properties defined");
        for (int i = 0; i < file.NumEls; ++i)
            if (file.labellist[file.lbl[i]].BlockType < 0)
                return fail(std::string(path) + ": an element lies in a region without material");
        std::vector<double> x, y;
        std::vector<int> cond;
        const size_t nb = file.blockproplist.size(), nl = file.labellist.size(), nli = file.lineproplist.size(),
                     np = file.nodeproplist.size(), nc = file.circproplist.size();
        int rc;
        if (kind == POT_ELECTROSTATIC) {
            std::vector<xfk_es_block_desc> blk(nb);
            std::vector<xfk_es_label_desc> lab(nl);
            std::vector<xfk_es_line_desc> lin(nli);
            std::vector<xfk_es_point_desc> pts(np);
            std::vector<xfk_es_conductor_desc> cir(nc);
            for (size_t k = 0; k < nb; k++)
                blk[k] = xfk_es_block_desc{file.blockproplist[k].kx, file.blockproplist[k].ky, file.blockproplist[k].qv};
            for (size_t k = 0; k < nl; k++)
                lab[k] = xfk_es_label_desc{std::max(0, file.labellist[k].BlockType), file.labellist[k].IsExternal ? 1 : 0};
            for (size_t k = 0; k < nli; k++) {
                const CPBoundaryProp &b = file.lineproplist[k];
                lin[k] = xfk_es_line_desc{b.BdryFormat, b.V, b.qs, b.c0, b.c1};
            }
            for (size_t k = 0; k < np; k++) pts[k] = xfk_es_point_desc{file.nodeproplist[k].V, file.nodeproplist[k].qp};
            for (size_t k = 0; k < nc; k++)
                cir[k] = xfk_es_conductor_desc{file.circproplist[k].CircType, file.circproplist[k].V, file.circproplist[k].q};
            xfk_es_problem_desc d{};
            fill(d, x, y, cond);
            d.n_blocks = (int)nb; d.blocks = blk.data();
            d.n_labels = (int)nl; d.labels = lab.data();
            d.n_lines = (int)nli; d.lines = lin.empty() ? nullptr : lin.data();
            d.n_points = (int)np; d.points = pts.empty() ? nullptr : pts.data();
            d.n_conductors = (int)nc; d.conductors = cir.empty() ? nullptr : cir.data();
            rc = xfk_problem_create_electrostatic(&d, device, &prob);
        } else {
            std::vector<xfk_hf_block_desc> blk(nb);
            std::vector<xfk_hf_label_desc> lab(nl);
            std::vector<xfk_hf_line_desc> lin(nli);
            std::vector<xfk_hf_point_desc> pts(np);
            std::vector<xfk_hf_conductor_desc> cir(nc);
            for (size_t k = 0; k < nb; k++) {
                const CPMaterialProp &m = file.blockproplist[k];
                blk[k] = xfk_hf_block_desc{m.kx, m.ky, m.Kt, m.qv, (int)m.T.size(), m.T.empty() ? nullptr : m.T.data(),
                                           m.K.empty() ? nullptr : m.K.data()};
            }
            for (size_t k = 0; k < nl; k++)
                lab[k] = xfk_hf_label_desc{std::max(0, file.labellist[k].BlockType), file.labellist[k].IsExternal ? 1 : 0};
            for (size_t k = 0; k < nli; k++) {
                const CPBoundaryProp &b = file.lineproplist[k];
                lin[k] = xfk_hf_line_desc{b.BdryFormat, b.V, b.qs, b.beta, b.h, b.Tinf};
            }
            for (size_t k = 0; k < np; k++) pts[k] = xfk_hf_point_desc{file.nodeproplist[k].V, file.nodeproplist[k].qp};
            for (size_t k = 0; k < nc; k++)
                cir[k] = xfk_hf_conductor_desc{file.circproplist[k].CircType, file.circproplist[k].V, file.circproplist[k].q};
            xfk_hf_problem_desc d{};
            fill(d, x, y, cond);
            d.n_blocks = (int)nb; d.blocks = blk.data();
            d.n_labels = (int)nl; d.labels = lab.data();
            d.n_lines = (int)nli; d.lines = lin.empty() ? nullptr : lin.data();
            d.n_points = (int)np; d.points = pts.empty() ? nullptr : pts.data();
            d.n_conductors = (int)nc; d.conductors = cir.empty() ? nullptr : cir.data();
            // (a post-processed time step needs no previous solution: the step is not taken again)
            d.dt = 0;
            d.t_prev = nullptr;
            rc = xfk_problem_create_heatflow(&d, device, &prob);
        }
        if (rc != XFK_OK) prob = nullptr;
        if (!xfk(rc) || !xfk(xfk_pot_set_qmarks(prob, file.Q.data())) || !xfk(xfk_pot_set_solution(prob, file.V.data()))) {
            drop();
            return false;
        }
        // Regions tagged by more than one block label (epproc.cpp:235-263): one
        // batch of point locations over the label positions
        if (nl) {
            std::vector<double> lx(nl), ly(nl), out(8 * nl);
            std::vector<int> el(nl);
            for (size_t k = 0; k < nl; k++) {
                lx[k] = file.labellist[k].x;
                ly[k] = file.labellist[k].y;
            }
            if (!xfk(xfk_pot_point_values(prob, (int)nl, lx.data(), ly.data(), 0, el.data(), out.data()))) {
                drop();
                return false;
            }
            // (the reference locates the labels with its walk, which leaves its
            // starting element behind for the first point looked up afterwards)
            for (size_t k = 0; k < nl; k++) walk.find(file, lx[k], ly[k]);
            for (size_t k = 0; k < nl; k++)
                if (el[k] >= 0 && file.lbl[el[k]] != (int)k) {
                    selected[file.lbl[el[k]]] = 1;
                    if (!multiply_defined)
                        WarnMessage("Some regions in the problem have been defined\n"
                                    "by more than one block label.  These potentially\n"
                                    "problematic regions will appear as selected in\n"
                                    "the initial view.\n");
                    multiply_defined = true;
                }
        }
        return true;
    }

    bool block_integral(int type, double *out2)
    {
        if (!need_doc()) return false;
        if (!out2) return fail("null output");
        if (selected.empty()) return fail("the problem has no block labels");
        if ((type == 5 || type == 6) && kind == POT_ELECTROSTATIC) {
            std::vector<double> area(file.labellist.size());
            for (size_t k = 0; k < area.size(); k++) area[k] = file.labellist[k].MaxArea;
            if (!xfk(xfk_pot_make_mask(prob, selected.data(), nullptr, area.data()))) return false;
        }
        if (type >= 0 && type <= 4) {
            // in the reference's order of summation, so that the programs print its digits
            double o[7];
            if (!xfk(xfk_pot_block_integrals_ordered(prob, selected.data(), o))) return false;
            out2[0] = type < 3 ? o[type] : o[3 + 2 * (type - 3)];
            out2[1] = type < 3 ? 0. : o[4 + 2 * (type - 3)];
            return true;
        }
        return xfk(xfk_pot_block_integral(prob, selected.data(), type, out2));
    }

    bool line_integral(int type, double *out2)
    {
        if (!need_doc()) return false;
        if (!out2) return fail("null output");
        const int n = (int)contour.pts.size();
        std::vector<double> x(std::max(1, n)), y(std::max(1, n));
        for (int i = 0; i < n; ++i) {
            x[i] = contour.pts[i].first;
            y[i] = contour.pts[i].second;
        }
        return xfk(xfk_pot_line_integral(prob, n, x.data(), y.data(), type, smooth ? 1 : 0, 0, out2, nullptr));
    }
};

// No C++ exception crosses the C-ABI: a host allocation failure (or any
// other exception) of a step becomes its false return, with the reason in
// last_error.
template <class F>
int guarded(PProc *s, F &&f)
{
    if (!s) return 0;
    try {
        return f() ? 1 : 0;
    } catch (const std::bad_alloc &) {
        s->lastError = "out of host memory";
    } catch (const std::exception &e) {
        s->lastError = e.what();
    } catch (...) {
        s->lastError = "unknown exception";
    }
    s->WarnMessage("%s\n", s->lastError.c_str());
    return 0;
}

int get_nodes(PProc *s, double *x, double *y, double *V, int *Q)
{
    if (!s || !s->have_file) return 0;
    for (int i = 0; i < s->file.NumNodes; i++) {
        if (x) x[i] = s->file.x[i];
        if (y) y[i] = s->file.y[i];
        if (V) V[i] = s->file.V[i];
        if (Q) Q[i] = s->file.Q[i];
    }
    return 1;
}

int get_elements(PProc *s, int *p, int *lbl)
{
    if (!s || !s->have_file) return 0;
    if (p) std::copy(s->file.p.begin(), s->file.p.end(), p);
    if (lbl) std::copy(s->file.lbl.begin(), s->file.lbl.end(), lbl);
    return 1;
}

int get_conductors(PProc *s, double *V, double *q)
{
    if (!s || !s->have_file) return 0;
    if (V) std::copy(s->file.condV.begin(), s->file.condV.end(), V);
    if (q) std::copy(s->file.condq.begin(), s->file.condq.end(), q);
    return 1;
}

int get_header(PProc *s, double *o)
{
    if (!s || !o || !s->have_file) return 0;
    const SolutionFile &f = s->file;
    const double v[8] = {f.Precision, f.Depth, (double)f.LengthUnits, (double)f.ProblemTypeV, f.extZo, f.extRo, f.extRi, f.dT};
    std::copy(v, v + 8, o);
    return 1;
}

int get_block_label(PProc *s, int k, double *o)
{
    if (!s || !o || !s->have_file || k < 0 || k >= (int)s->file.labellist.size()) return -1;
    const CPBlockLabel &l = s->file.labellist[k];
    const double v[6] = {l.x, l.y, (double)l.BlockType, (double)l.InGroup, l.IsExternal ? 1. : 0., l.IsDefault ? 1. : 0.};
    std::copy(v, v + 6, o);
    return 6;
}

int get_block_prop(PProc *s, int k, double *o)
{
    if (!s || !o || !s->have_file || k < 0 || k >= (int)s->file.blockproplist.size()) return -1;
    const CPMaterialProp &m = s->file.blockproplist[k];
    const double v[5] = {m.kx, m.ky, m.Kt, m.qv, (double)m.T.size()};
    std::copy(v, v + 5, o);
    return 5;
}

int geometry_counts(PProc *s, int *o)
{
    if (!s || !o || !s->have_file) return 0;
    const PotGeometry &g = s->file.geom;
    o[0] = (int)g.points.size();
    o[1] = (int)g.segments.size();
    o[2] = (int)g.arcs.size();
    o[3] = (int)g.holes.size();
    return 1;
}

int get_geometry_points(PProc *s, double *x, double *y, int *group)
{
    if (!s || !s->have_file) return 0;
    const auto &v = s->file.geom.points;
    for (size_t i = 0; i < v.size(); i++) {
        if (x) x[i] = v[i].x;
        if (y) y[i] = v[i].y;
        if (group) group[i] = v[i].group;
    }
    return 1;
}

int get_geometry_segments(PProc *s, int *n01, int *group)
{
    if (!s || !s->have_file) return 0;
    const auto &v = s->file.geom.segments;
    for (size_t i = 0; i < v.size(); i++) {
        if (n01) {
            n01[2 * i] = v[i].n0;
            n01[2 * i + 1] = v[i].n1;
        }
        if (group) group[i] = v[i].group;
    }
    return 1;
}

int get_geometry_arcs(PProc *s, int *n01, double *lm, int *group)
{
    if (!s || !s->have_file) return 0;
    const auto &v = s->file.geom.arcs;
    for (size_t i = 0; i < v.size(); i++) {
        if (n01) {
            n01[2 * i] = v[i].n0;
            n01[2 * i + 1] = v[i].n1;
        }
        if (lm) {
            lm[2 * i] = v[i].ArcLength;
            lm[2 * i + 1] = v[i].MaxSideLength;
        }
        if (group) group[i] = v[i].group;
    }
    return 1;
}

int toggle_label(PProc *s, int k)
{
    if (!s || k < 0 || k >= (int)s->selected.size()) return 0;
    s->selected[k] = !s->selected[k];
    return 1;
}

int toggle_group(PProc *s, int g)
{
    if (!s || !s->have_file) return 0;
    for (size_t k = 0; k < s->selected.size(); k++)
        if (s->file.labellist[k].InGroup == g) s->selected[k] = !s->selected[k];
    return 1;
}

int point_values(PProc *s, int n, const double *x, const double *y, int *elem, double *out)
{
    return guarded(s, [&] {
        if (!s->need_doc()) return false;
        return s->xfk(xfk_pot_point_values(s->prob, n, x, y, s->smooth ? 1 : 0, elem, out));
    });
}

// getPointValues: the element by the reference's walk from the one found last
int point_value(PProc *s, double x, double y, double *out8)
{
    if (!out8) return 0;
    return guarded(s, [&] {
        if (!s->need_doc()) return false;
        const int el = s->walk.find(s->file, x, y);
        if (el < 0) return false;
        return s->xfk(xfk_pot_point_values_at(s->prob, 1, &x, &y, &el, s->smooth ? 1 : 0, out8));
    });
}

}  // namespace

struct xfemm_epproc {
    PProc s{xfemm::POT_ELECTROSTATIC};
};
struct xfemm_hpproc {
    PProc s{xfemm::POT_HEATFLOW};
};

#define S(h) ((h) ? &(h)->s : nullptr)

#define XFEMM_PPROC_CAPI(NAME)                                                                                         \
    xfemm_##NAME *xfemm_##NAME##_create(void)                                                                          \
    {                                                                                                                  \
        try {                                                                                                          \
            return new xfemm_##NAME();                                                                                 \
        } catch (...) {                                                                                                \
            return nullptr;                                                                                            \
        }                                                                                                              \
    }                                                                                                                  \
    void xfemm_##NAME##_destroy(xfemm_##NAME *h) { delete h; }                                                         \
    int xfemm_##NAME##_set_device(xfemm_##NAME *h, int device)                                                         \
    {                                                                                                                  \
        if (!h || device < 0) return 0;                                                                                \
        h->s.device = device;                                                                                          \
        return 1;                                                                                                      \
    }                                                                                                                  \
    void xfemm_##NAME##_set_message_handlers(xfemm_##NAME *h, xfemm_message_fn warn, xfemm_message_fn print)           \
    {                                                                                                                  \
        if (!h) return;                                                                                                \
        if (warn) h->s.WarnMessage = warn;                                                                             \
        if (print) h->s.PrintMessage = print;                                                                          \
    }                                                                                                                  \
    int xfemm_##NAME##_read(xfemm_##NAME *h, const char *path)                                                         \
    {                                                                                                                  \
        return guarded(S(h), [&] { return h->s.read(path); });                                                         \
    }                                                                                                                  \
    int xfemm_##NAME##_num_nodes(xfemm_##NAME *h) { return h ? h->s.file.NumNodes : 0; }                               \
    int xfemm_##NAME##_num_elements(xfemm_##NAME *h) { return h ? h->s.file.NumEls : 0; }                              \
    int xfemm_##NAME##_num_conductors(xfemm_##NAME *h) { return h ? (int)h->s.file.condV.size() : -1; }               \
    int xfemm_##NAME##_get_nodes(xfemm_##NAME *h, double *x, double *y, double *V, int *Q)                             \
    {                                                                                                                  \
        return get_nodes(S(h), x, y, V, Q);                                                                            \
    }                                                                                                                  \
    int xfemm_##NAME##_get_elements(xfemm_##NAME *h, int *p, int *lbl) { return get_elements(S(h), p, lbl); }         \
    int xfemm_##NAME##_get_conductors(xfemm_##NAME *h, double *V, double *q) { return get_conductors(S(h), V, q); }   \
    int xfemm_##NAME##_get_header(xfemm_##NAME *h, double *o) { return get_header(S(h), o); }                         \
    int xfemm_##NAME##_num_line_props(xfemm_##NAME *h) { return h ? (int)h->s.file.lineproplist.size() : -1; }        \
    int xfemm_##NAME##_num_node_props(xfemm_##NAME *h) { return h ? (int)h->s.file.nodeproplist.size() : -1; }        \
    int xfemm_##NAME##_num_block_props(xfemm_##NAME *h) { return h ? (int)h->s.file.blockproplist.size() : -1; }      \
    int xfemm_##NAME##_num_block_labels(xfemm_##NAME *h) { return h ? (int)h->s.file.labellist.size() : -1; }         \
    int xfemm_##NAME##_get_block_label(xfemm_##NAME *h, int k, double *o) { return get_block_label(S(h), k, o); }     \
    int xfemm_##NAME##_get_block_prop(xfemm_##NAME *h, int k, double *o) { return get_block_prop(S(h), k, o); }       \
    int xfemm_##NAME##_geometry_counts(xfemm_##NAME *h, int *o) { return geometry_counts(S(h), o); }                  \
    int xfemm_##NAME##_get_geometry_points(xfemm_##NAME *h, double *x, double *y, int *g)                              \
    {                                                                                                                  \
        return get_geometry_points(S(h), x, y, g);                                                                     \
    }                                                                                                                  \
    int xfemm_##NAME##_get_geometry_segments(xfemm_##NAME *h, int *n, int *g)                                          \
    {                                                                                                                  \
        return get_geometry_segments(S(h), n, g);                                                                      \
    }                                                                                                                  \
    int xfemm_##NAME##_get_geometry_arcs(xfemm_##NAME *h, int *n, double *lm, int *g)                                  \
    {                                                                                                                  \
        return get_geometry_arcs(S(h), n, lm, g);                                                                      \
    }                                                                                                                  \
    int xfemm_##NAME##_open_document(xfemm_##NAME *h, const char *path)                                                \
    {                                                                                                                  \
        return guarded(S(h), [&] { return h->s.open(path); });                                                         \
    }                                                                                                                  \
    int xfemm_##NAME##_clear_selection(xfemm_##NAME *h)                                                                \
    {                                                                                                                  \
        if (!h) return 0;                                                                                              \
        std::fill(h->s.selected.begin(), h->s.selected.end(), 0);                                                      \
        return 1;                                                                                                      \
    }                                                                                                                  \
    int xfemm_##NAME##_select_block_label(xfemm_##NAME *h, double x, double y)                                         \
    {                                                                                                                  \
        return h ? toggle_label(S(h), xfemm::ClosestLabel(h->s.file, x, y)) : 0;                                       \
    }                                                                                                                  \
    int xfemm_##NAME##_toggle_label(xfemm_##NAME *h, int k) { return toggle_label(S(h), k); }                         \
    int xfemm_##NAME##_toggle_group(xfemm_##NAME *h, int g) { return toggle_group(S(h), g); }                         \
    int xfemm_##NAME##_get_selection(xfemm_##NAME *h, unsigned char *sel)                                              \
    {                                                                                                                  \
        if (!h || !sel) return 0;                                                                                      \
        std::copy(h->s.selected.begin(), h->s.selected.end(), sel);                                                    \
        return 1;                                                                                                      \
    }                                                                                                                  \
    int xfemm_##NAME##_set_smoothing(xfemm_##NAME *h, int on)                                                          \
    {                                                                                                                  \
        if (!h) return 0;                                                                                              \
        h->s.smooth = on != 0;                                                                                         \
        return 1;                                                                                                      \
    }                                                                                                                  \
    int xfemm_##NAME##_block_integral(xfemm_##NAME *h, int type, double *out2)                                         \
    {                                                                                                                  \
        return guarded(S(h), [&] { return h->s.block_integral(type, out2); });                                         \
    }                                                                                                                  \
    int xfemm_##NAME##_get_point_values(xfemm_##NAME *h, double x, double y, double *out8)                             \
    {                                                                                                                  \
        return point_value(S(h), x, y, out8);                                                                          \
    }                                                                                                                  \
    int xfemm_##NAME##_get_point_values_batch(xfemm_##NAME *h, int n, const double *x, const double *y, int *elem,     \
                                               double *out)                                                            \
    {                                                                                                                  \
        return point_values(S(h), n, x, y, elem, out);                                                                 \
    }                                                                                                                  \
    int xfemm_##NAME##_add_contour_point(xfemm_##NAME *h, double x, double y)                                          \
    {                                                                                                                  \
        return guarded(S(h), [&] { return h->s.contour.add(x, y), true; });                                            \
    }                                                                                                                  \
    int xfemm_##NAME##_add_contour_point_from_node(xfemm_##NAME *h, double x, double y)                                \
    {                                                                                                                  \
        return guarded(S(h), [&] {                                                                                     \
            if (!h->s.have_file) return h->s.fail("no file has been read");                                            \
            h->s.contour.add_from_node(h->s.file.geom, x, y);                                                          \
            return true;                                                                                               \
        });                                                                                                            \
    }                                                                                                                  \
    int xfemm_##NAME##_bend_contour(xfemm_##NAME *h, double angle, double step)                                        \
    {                                                                                                                  \
        return guarded(S(h), [&] { return h->s.contour.bend(angle, step), true; });                                    \
    }                                                                                                                  \
    int xfemm_##NAME##_clear_contour(xfemm_##NAME *h)                                                                  \
    {                                                                                                                  \
        if (!h) return 0;                                                                                              \
        h->s.contour.clear();                                                                                          \
        return 1;                                                                                                      \
    }                                                                                                                  \
    int xfemm_##NAME##_num_contour_points(xfemm_##NAME *h) { return h ? (int)h->s.contour.pts.size() : 0; }           \
    int xfemm_##NAME##_get_contour(xfemm_##NAME *h, double *x, double *y)                                              \
    {                                                                                                                  \
        if (!h) return 0;                                                                                              \
        for (size_t i = 0; i < h->s.contour.pts.size(); i++) {                                                         \
            if (x) x[i] = h->s.contour.pts[i].first;                                                                   \
            if (y) y[i] = h->s.contour.pts[i].second;                                                                  \
        }                                                                                                              \
        return 1;                                                                                                      \
    }                                                                                                                  \
    int xfemm_##NAME##_line_integral(xfemm_##NAME *h, int type, double *out2)                                          \
    {                                                                                                                  \
        return guarded(S(h), [&] { return h->s.line_integral(type, out2); });                                          \
    }                                                                                                                  \
    int xfemm_##NAME##_plot_bounds(xfemm_##NAME *h, double *out6)                                                      \
    {                                                                                                                  \
        return guarded(S(h), [&] { return h->s.need_doc() && h->s.xfk(xfk_pot_plot_bounds(h->s.prob, out6)); });       \
    }                                                                                                                  \
    int xfemm_##NAME##_has_multiply_defined_labels(xfemm_##NAME *h) { return h && h->s.multiply_defined ? 1 : 0; }    \
    xfk_problem *xfemm_##NAME##_problem(xfemm_##NAME *h) { return h ? h->s.prob : nullptr; }                           \
    const char *xfemm_##NAME##_last_error(xfemm_##NAME *h) { return h ? h->s.lastError.c_str() : ""; }

extern "C" {

XFEMM_PPROC_CAPI(epproc)
XFEMM_PPROC_CAPI(hpproc)

}  // extern "C"
