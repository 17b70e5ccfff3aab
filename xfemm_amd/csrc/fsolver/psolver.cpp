// ESolver / HSolver host logic over the MI355X kernels (see psolver.h).
#include "psolver.h"

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include <sys/stat.h>

#include "meshhost_impl.h"

namespace xfemm {

using namespace meshio;

namespace {
// conversion to the internal working units: mm (esolver.cpp:65), m (hsolver.cpp:65)
constexpr double kUnitsE[] = {25.4, 1., 10., 1000., 0.0254, 0.001};
constexpr double kUnitsH[] = {0.0254, 0.001, 0.01, 1, 2.54e-5, 1.e-6};
}  // namespace

PSolver::PSolver(PotentialKind k) : kind(k) {}

PSolver::~PSolver() { drop_problem(); }

void PSolver::drop_problem()
{
    if (prob_) xfk_problem_destroy(prob_);
    prob_ = nullptr;
}

double PSolver::unit() const { return (kind == POT_HEATFLOW ? kUnitsH : kUnitsE)[LengthUnits]; }

std::string PSolver::getErrorString(LoadMeshErr err)
{
    // FEASolver::getErrorString (feasolver.cpp:587-611)
    switch (err) {
    case NOERROR: return std::string();
    case BADEDGEFILE: return "problem loading mesh:\nCould not open .edge file.\n";
    case BADELEMENTFILE: return "problem loading mesh:\nCould not open .ele file.\n";
    case BADFEMFILE: return "problem loading mesh:\nCould not open .fem file.\n";
    case BADNODEFILE: return "problem loading mesh:\nCould not open .node file.\n";
    case BADPBCFILE: return "problem loading mesh:\nCould not open .pbc file.\n";
    case MISSINGMATPROPS: return "problem loading mesh:\nMaterial properties have not been defined for all regions.\n";
    case ELMLABELTOOBIG:
        return "problem loading mesh:\nElemnet label number was greater than the number of labels in the problem.\n";
    case UNSUPPORTEDMESH: return "problem loading mesh:\nunsupported mesh.\n";
    }
    return std::string();
}

bool PSolver::LoadProblemFile()
{
    start_hip_warmup();
    std::string err;
    PotProblemData &base = *this;
    if (!ParsePotentialFile(PathName + input_ext(), kind, base, err)) {
        warn(err);
        return false;
    }
    return true;
}

bool PSolver::set_previous_solution(const double *T, int n)
{
    if (kind != POT_HEATFLOW || n < 0 || (n > 0 && !T)) return false;
    Tprev_.assign(T, T + n);
    return true;
}

LoadMeshErr PSolver::LoadMesh(bool deleteFiles)
{
    LoadTrace tr;
    TextBuf tb;
    {   // one buffer for the three mesh files: the largest one's size
        struct stat st;
        for (const char *ext : {".node", ".ele", ".edge"})
            if (::stat((PathName + ext).c_str(), &st) == 0) tb.hint = std::max(tb.hint, (size_t)st.st_size + 1);
    }
    // nodes: the low 16 bits of the marker minus 2 give the point property,
    // the high bits minus 1 the conductor (esolver.cpp:155-181); a missing
    // .node file is BADELEMENTFILE in both solvers (esolver.cpp:136-142)
    const double cf = unit();
    if (!read_node_file(tb, meshnode, [cf](CPNode &node, double x, double y, int n) {
            int j;
            if (n > 1) {
                j = (n & 0xffff) - 2;
                if (j < 0) j = -1;
                n = (n - (n & 0xffff)) / 0x10000 - 1;
            } else {
                j = -1;
                n = -1;
            }
            node.BoundaryMarker = j;
            node.InConductor = n;
            node.x = x * cf;
            node.y = y * cf;
        }))
        return BADELEMENTFILE;

    // periodic pairs: one count line, then a token stream (esolver.cpp:185-204)
    {
        TextBuf pb;
        if (!pb.load(PathName + ".pbc")) return BADPBCFILE;
        int k = 0;
        if (!pb.header_int(k)) k = 0;
        NumPBCs = std::max(0, k);
        pbclist.clear();
        for (int i = 0; i < NumPBCs; i++) {
            int j;
            CCommonPoint pbc;
            if (!pb.next_int(j) || !pb.next_int(pbc.x) || !pb.next_int(pbc.y) || !pb.next_int(pbc.t) || pbc.x < 0 ||
                pbc.y < 0 || pbc.x >= NumNodes || pbc.y >= NumNodes)
                return BADPBCFILE;
            pbclist.push_back(pbc);
        }
    }

    if (!read_element_file(tb, meshele)) return BADELEMENTFILE;
    int defaultLabel = -1;
    for (int i = 0; i < (int)labellist.size(); i++)
        if (labellist[i].IsDefault) defaultLabel = i;
    auto remove_files = [&]() {
        for (const char *ext : {".ele", ".node", ".pbc", ".poly", ".edge"}) remove((PathName + ext).c_str());
    };
    {
        const ElementCheck bad = check_elements(meshele, (int)labellist.size(), defaultLabel,
                                                [&](int lbl) { return labellist[lbl].BlockType; });
        if (bad.code == 1) {   // esolver.cpp:229-250
            warn("Material properties have not been defined for\n"
                 "all regions. Press the \"Run Mesh Generator\"\n"
                 "button to highlight the problem regions.");
            if (deleteFiles) remove_files();
            return MISSINGMATPROPS;
        }
        if (bad.code == 2) {   // (the reference indexes past labellist here)
            if (deleteFiles) remove_files();
            return ELMLABELTOOBIG;
        }
        if (bad.code) return BADELEMENTFILE;
    }
    tr.mark("elements");

    std::vector<int> marked;
    if (!read_edge_file(tb, marked)) return BADEDGEFILE;
    // esolver.cpp:303-352 on the edges with a negative marker, in file order:
    // the conductor goes onto both end nodes; the boundary property onto every
    // element around n0 that holds the edge, in element order -- only the
    // first such element for a BdryFormat 2 property.  The node -> element
    // lists are built for the first nodes of those edges only.
    {
        struct Todo {
            int n0, n1, j;
        };
        std::vector<Todo> todo;
        std::vector<char> need(NumNodes, 0);
        for (int i : marked) {
            const auto &e = edges_[i];
            int n = -e[2];
            int j = (n & 0xffff) - 2;
            if (j < 0) j = -1;
            n = (n - (n & 0xffff)) / 0x10000 - 1;
            if (n >= 0) {
                meshnode[e[0]].InConductor = n;
                meshnode[e[1]].InConductor = n;
            }
            if (j >= 0) {
                todo.push_back(Todo{e[0], e[1], j});
                need[e[0]] = 1;
            }
        }
        if (!todo.empty()) {
            const int T = 64;
            std::vector<std::vector<std::array<int, 2>>> found(T);   // (node, element), ascending elements
            par_for(T, 1, [&](long long t0, long long t1) {
                for (long long t = t0; t < t1; ++t) {
                    const int a = (int)((long long)NumEls * t / T), b = (int)((long long)NumEls * (t + 1) / T);
                    for (int i = a; i < b; i++)
                        for (int q = 0; q < 3; q++)
                            if (need[meshele[i].p[q]]) found[t].push_back({meshele[i].p[q], i});
                }
            });
            std::vector<int> nmbr(NumNodes + 1, 0);
            for (auto &f : found)
                for (auto &pr : f) nmbr[pr[0] + 1]++;
            for (int i = 0; i < NumNodes; i++) nmbr[i + 1] += nmbr[i];
            std::vector<int> mbr(nmbr[NumNodes]), cur(nmbr.begin(), nmbr.end() - 1);
            for (auto &f : found)
                for (auto &pr : f) mbr[cur[pr[0]]++] = pr[1];
            const int nlp = (int)lineproplist.size();
            for (const Todo &t : todo) {
                const int n0 = t.n0, n1 = t.n1, j = t.j;
                const bool first_only = j < nlp && lineproplist[j].BdryFormat == 2;
                bool n = false;
                for (int q = nmbr[n0]; q < nmbr[n0 + 1]; q++) {
                    CPElement &elm = meshele[mbr[q]];
                    for (int s = 0; s < 3; s++) {
                        const int a = elm.p[s], b = elm.p[(s + 1) % 3];
                        if ((a == n0 && b == n1) || (a == n1 && b == n0)) {
                            elm.e[s] = j;
                            n = true;
                        }
                    }
                    // line charge distributions go to at most one element (esolver.cpp:346-348)
                    if (first_only && n) break;
                }
            }
        }
    }
    tr.mark("edges");
    // (the .edge file stays for Cuthill, esolver.cpp:360-371)
    if (deleteFiles) remove_async({PathName + ".ele", PathName + ".node", PathName + ".pbc", PathName + ".poly"});
    return NOERROR;
}

int PSolver::SortElements() { return sort_mesh_elements(meshele); }

int PSolver::Cuthill(bool deleteFiles)
{
    // The reference's SortNodes (esolver.cpp:848-860) moves the nodes only;
    // a previous solution is carried along here.
    return cuthill_mesh(meshnode, meshele, deleteFiles, [&](const BigVec<int> &newnum) {
        if ((int)Tprev_.size() != NumNodes) return;
        std::vector<double> sorted(NumNodes);
        for (int k = 0; k < NumNodes; k++) sorted[newnum[k]] = Tprev_[k];
        Tprev_.swap(sorted);
    });
}

bool PSolver::load_prev(bool &loaded)
{
    loaded = false;
    if (kind != POT_HEATFLOW) return true;
    if (dT != 0 && !Tprev_.empty()) {
        if ((int)Tprev_.size() != NumNodes) {
            warn("the previous solution set has " + std::to_string(Tprev_.size()) + " values, the mesh " +
                 std::to_string(NumNodes) + " nodes\n");
            return false;
        }
        loaded = true;
        return true;
    }
    if (previousSolutionFile.empty()) {
        if (dT != 0) {   // hsolver.cpp:129-137
            dT = 0;
            WarnMessage("Warning: no previous solution set even though dT is non-zero. Resetting dT...\n");
        }
        return true;
    }
    if (dT != 0) {
        warn("time step from a file refused: [PrevSoln] = \"" + previousSolutionFile +
             "\" with [dT] != 0.  The reference reads the previous temperatures by line number from a file "
             "written in renumbered order; give them with set_previous_solution, or step in memory "
             "(xfk_heatflow_advance)\n");
        return false;
    }
    return true;   // (dT == 0: the previous solution is not used)
}

namespace {
template <class D>
void fill_mesh(D &d, const PSolver &s, std::vector<double> &x, std::vector<double> &y, std::vector<int> &marker,
               std::vector<int> &cond, std::vector<int> &p, std::vector<int> &e, std::vector<int> &lbl,
               std::vector<int> &pbc)
{
    const int N = s.NumNodes, NE = s.NumEls;
    const int nnp = (int)s.nodeproplist.size(), nlp = (int)s.lineproplist.size(), ncp = (int)s.circproplist.size();
    for (auto *v : {&x, &y}) {
        huge_reserve(*v, (size_t)N);
        v->resize(N);
    }
    for (auto *v : {&marker, &cond}) {
        huge_reserve(*v, (size_t)N);
        v->resize(N);
    }
    huge_reserve(p, 3ull * NE);
    huge_reserve(e, 3ull * NE);
    huge_reserve(lbl, (size_t)NE);
    p.resize(3ull * NE);
    e.resize(3ull * NE);
    lbl.resize(NE);
    par_for(N, 1 << 16, [&](long long a, long long b) {
        for (long long i = a; i < b; i++) {
            const CPNode &n = s.meshnode[i];
            x[i] = n.x;
            y[i] = n.y;
            marker[i] = n.BoundaryMarker >= nnp ? -1 : n.BoundaryMarker;
            cond[i] = n.InConductor >= ncp ? -1 : n.InConductor;
        }
    });
    par_for(NE, 1 << 16, [&](long long a, long long b) {
        for (long long i = a; i < b; i++) {
            const CPElement &el = s.meshele[i];
            for (int q = 0; q < 3; q++) {
                p[3 * i + q] = el.p[q];
                e[3 * i + q] = (el.e[q] >= 0 && el.e[q] < nlp) ? el.e[q] : -1;
            }
            lbl[i] = el.lbl;
        }
    });
    pbc.resize(3ull * s.NumPBCs);
    for (int k = 0; k < s.NumPBCs; k++) {
        pbc[3 * k] = s.pbclist[k].x;
        pbc[3 * k + 1] = s.pbclist[k].y;
        pbc[3 * k + 2] = s.pbclist[k].t;
    }
    d.n_nodes = N; d.x = x.data(); d.y = y.data(); d.marker = marker.data(); d.conductor = cond.data();
    d.n_elems = NE; d.p = p.data(); d.e = e.data(); d.lbl = lbl.data();
    d.n_pbc = s.NumPBCs; d.pbc = s.NumPBCs ? pbc.data() : nullptr;
    d.precision = s.Precision;
    d.length_units = (int)s.LengthUnits;
    d.problem_type = s.ProblemTypeV == AXISYMMETRIC ? XFK_AXISYMMETRIC : XFK_PLANAR;
    d.depth = s.Depth;
    d.ext_zo = s.extZo;
    d.ext_ro = s.extRo;
    d.ext_ri = s.extRi;
}
}  // namespace

bool PSolver::solve_on_device()
{
    join_hip_warmup();
    auto t = std::chrono::steady_clock::now();
    drop_problem();
    if (blockproplist.empty()) {
        warn("no block properties defined\n");
        return false;
    }
    for (long long i = 0; i < NumEls; i++)
        if (labellist[meshele[i].lbl].BlockType < 0) {
            warn("an element lies in a region without material (hole label)\n");
            return false;
        }
    std::vector<double> x, y;
    std::vector<int> marker, cond, p, e, lbl, pbc;
    const size_t nb = blockproplist.size(), nl = labellist.size(), nli = lineproplist.size(),
                 np = nodeproplist.size(), nc = circproplist.size();
    int rc;
    if (kind == POT_ELECTROSTATIC) {
        std::vector<xfk_es_block_desc> blk(nb);
        std::vector<xfk_es_label_desc> lab(nl);
        std::vector<xfk_es_line_desc> lin(nli);
        std::vector<xfk_es_point_desc> pts(np);
        std::vector<xfk_es_conductor_desc> cir(nc);
        for (size_t k = 0; k < nb; k++) blk[k] = xfk_es_block_desc{blockproplist[k].kx, blockproplist[k].ky, blockproplist[k].qv};
        for (size_t k = 0; k < nl; k++) lab[k] = xfk_es_label_desc{std::max(0, labellist[k].BlockType), labellist[k].IsExternal ? 1 : 0};
        for (size_t k = 0; k < nli; k++) {
            const CPBoundaryProp &b = lineproplist[k];
            lin[k] = xfk_es_line_desc{b.BdryFormat, b.V, b.qs, b.c0, b.c1};
        }
        for (size_t k = 0; k < np; k++) pts[k] = xfk_es_point_desc{nodeproplist[k].V, nodeproplist[k].qp};
        for (size_t k = 0; k < nc; k++) cir[k] = xfk_es_conductor_desc{circproplist[k].CircType, circproplist[k].V, circproplist[k].q};
        xfk_es_problem_desc d{};
        fill_mesh(d, *this, x, y, marker, cond, p, e, lbl, pbc);
        d.n_blocks = (int)nb; d.blocks = blk.data();
        d.n_labels = (int)nl; d.labels = lab.data();
        d.n_lines = (int)nli; d.lines = lin.empty() ? nullptr : lin.data();
        d.n_points = (int)np; d.points = pts.empty() ? nullptr : pts.data();
        d.n_conductors = (int)nc; d.conductors = cir.empty() ? nullptr : cir.data();
        rc = xfk_problem_create_electrostatic(&d, device, &prob_);
        ms_phase[2] = ms_since(t);
        if (rc == XFK_OK) rc = xfk_electrostatic(prob_, 0, &stats);
    } else {
        std::vector<xfk_hf_block_desc> blk(nb);
        std::vector<xfk_hf_label_desc> lab(nl);
        std::vector<xfk_hf_line_desc> lin(nli);
        std::vector<xfk_hf_point_desc> pts(np);
        std::vector<xfk_hf_conductor_desc> cir(nc);
        for (size_t k = 0; k < nb; k++) {
            const CPMaterialProp &m = blockproplist[k];
            blk[k] = xfk_hf_block_desc{m.kx, m.ky, m.Kt, m.qv, (int)m.T.size(), m.T.empty() ? nullptr : m.T.data(),
                                       m.K.empty() ? nullptr : m.K.data()};
        }
        for (size_t k = 0; k < nl; k++) lab[k] = xfk_hf_label_desc{std::max(0, labellist[k].BlockType), labellist[k].IsExternal ? 1 : 0};
        for (size_t k = 0; k < nli; k++) {
            const CPBoundaryProp &b = lineproplist[k];
            lin[k] = xfk_hf_line_desc{b.BdryFormat, b.V, b.qs, b.beta, b.h, b.Tinf};
        }
        for (size_t k = 0; k < np; k++) pts[k] = xfk_hf_point_desc{nodeproplist[k].V, nodeproplist[k].qp};
        for (size_t k = 0; k < nc; k++) cir[k] = xfk_hf_conductor_desc{circproplist[k].CircType, circproplist[k].V, circproplist[k].q};
        xfk_hf_problem_desc d{};
        fill_mesh(d, *this, x, y, marker, cond, p, e, lbl, pbc);
        d.n_blocks = (int)nb; d.blocks = blk.data();
        d.n_labels = (int)nl; d.labels = lab.data();
        d.n_lines = (int)nli; d.lines = lin.empty() ? nullptr : lin.data();
        d.n_points = (int)np; d.points = pts.empty() ? nullptr : pts.data();
        d.n_conductors = (int)nc; d.conductors = cir.empty() ? nullptr : cir.data();
        d.dt = dT;
        d.t_prev = dT != 0 ? Tprev_.data() : nullptr;
        rc = xfk_problem_create_heatflow(&d, device, &prob_);
        ms_phase[2] = ms_since(t);
        if (rc == XFK_OK) rc = xfk_heatflow(prob_, 0, &stats);
    }
    if (rc == XFK_OK) {
        V.assign(NumNodes, 0.0);
        rc = xfk_get_solution(prob_, V.data());
    }
    if (rc == XFK_OK) {
        Q.assign(NumNodes, -2);
        rc = xfk_pot_get_qmarks(prob_, Q.data());
    }
    if (rc == XFK_OK) {
        condV.assign(std::max<size_t>(1, nc), 0.0);
        condq.assign(std::max<size_t>(1, nc), 0.0);
        rc = kind == POT_ELECTROSTATIC ? xfk_get_conductors(prob_, condV.data(), condq.data())
                                       : xfk_hf_get_conductors(prob_, condV.data(), condq.data());
        condV.resize(nc);
        condq.resize(nc);
    }
    if (rc != XFK_OK) {
        warn(std::string("GPU solver error: ") + xfk_last_error() + "\n");
        drop_problem();
        V.clear();
    }
    ms_phase[3] = ms_since(t);
    return rc == XFK_OK;
}

int PSolver::WriteResults()
{
    const std::string fin = PathName + input_ext(), fout = PathName + output_ext();
    FILE *fz = fopen(fin.c_str(), "rt");
    if (!fz) {
        printf("Couldn't open %s\n", fin.c_str());
        return false;
    }
    clear_old_output(fout);
    FILE *fp = fopen(fout.c_str(), "wt");
    if (!fp) {
        fclose(fz);
        printf("Couldn't write to %s", fout.c_str());
        return false;
    }
    char c[1024];
    while (fgets(c, 1024, fz) != nullptr) fputs(c, fp);
    fclose(fz);
    fprintf(fp, "[Solution]\n");
    // the coordinate was multiplied by cf on input and is divided on output
    const double cf = unit();
    fprintf(fp, "%i\n", NumNodes);
    fflush(fp);
    bool ok = write_lines(fp, NumNodes, 112, [&](int i, char *q) {
        for (double v : {meshnode[i].x / cf, meshnode[i].y / cf, V[i]}) {
            q = put_g17(q, v);
            *q++ = '\t';
        }
        q = put_i(q, Q[i]);
        *q++ = '\n';
        return q;
    });
    if (ok) fprintf(fp, "%i\n", NumEls);
    fflush(fp);
    ok = ok && write_lines(fp, NumEls, 64, [&](int i, char *q) {
        for (int m = 0; m < 3; ++m) {
            q = put_i(q, meshele[i].p[m]);
            *q++ = '\t';
        }
        q = put_i(q, meshele[i].lbl);
        *q++ = '\n';
        return q;
    });
    if (!ok) {
        fclose(fp);
        warn(std::string("couldn't allocate the ") + output_ext() + " text\n");
        return false;
    }
    fprintf(fp, "%i\n", (int)circproplist.size());
    for (size_t i = 0; i < circproplist.size(); i++) fprintf(fp, "%.17g\t%.17g\n", condV[i], condq[i]);
    fclose(fp);
    return true;
}

bool PSolver::runSolver(bool verbose)
{
    struct JoinRemovals {   // the mesh files are gone when runSolver returns, as in the reference
        PSolver *s;
        ~JoinRemovals() { s->join_removals(); }
    } join_at_exit{this};
    for (double &m : ms_phase) m = 0;
    auto t = std::chrono::steady_clock::now();
    // a run of its own: the previous solution is taken anew in file order
    const std::vector<double> prev_in = Tprev_;
    struct RestorePrev {
        std::vector<double> &dst;
        const std::vector<double> &src;
        ~RestorePrev() { dst = src; }
    } restore_prev{Tprev_, prev_in};
    LoadMeshErr err = LoadMesh(deleteMeshFiles);
    ms_phase[0] = ms_since(t);
    if (err != NOERROR) {
        WarnMessage("problem loading mesh:\n");
        warn(getErrorString(err));
        return false;
    }
    bool loaded = false;
    if (!load_prev(loaded)) return false;
    if (loaded && verbose) PrintMessage("Loading previous solution\n");
    if (verbose) PrintMessage("renumbering nodes\n");
    if (!Cuthill(deleteMeshFiles)) {
        warn("problem renumbering node points\n");
        return false;
    }
    ms_phase[1] = ms_since(t);
    if (verbose) {
        PrintMessage("solving...");
        const std::string stats_msg = "Problem Statistics:\n" + std::to_string(NumNodes) + " nodes\n" +
                                      std::to_string(NumEls) + " elements\n" + "Precision: " +
                                      std::to_string(Precision) + "\n";
        PrintMessage("%s", stats_msg.c_str());
    }
    if (!solve_on_device()) {
        WarnMessage("Couldn't solve the problem\n");
        return false;
    }
    if (verbose) PrintMessage("Problem solved\n");
    t = std::chrono::steady_clock::now();
    if (!WriteResults()) {
        // (hsolver.cpp:907-911 returns 6 here, which its bool return turns into success)
        warn("couldn't write results to disk\n");
        return false;
    }
    ms_phase[4] = ms_since(t);
    if (verbose) PrintMessage("results written to disk\n");
    return true;
}

}  // namespace xfemm
