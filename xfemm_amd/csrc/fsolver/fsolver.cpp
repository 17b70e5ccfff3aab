// FSolver host logic over the MI355X kernels (see fsolver.h).
#include "fsolver.h"

#include <algorithm>
#include <atomic>
#include <cctype>
#include <charconv>
#include <chrono>
#include <complex>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <new>
#include <type_traits>
#include <thread>
#include <unordered_map>
#include <utility>

#include <fcntl.h>
#include <immintrin.h>
#include <sys/stat.h>
#include <unistd.h>

#include "fastnum.h"
#include "hostmem.h"
#include "hostpool.h"
#include "meshhost_impl.h"

namespace xfemm {

using namespace meshio;

FSolver::FSolver() {}

FSolver::~FSolver()
{
    if (ele_fmt_.joinable()) ele_fmt_.join();
    if (problem) xfk_problem_destroy(problem);
}

bool FSolver::writes_output() const { return !comm || xfk_comm_rank(comm) == 0; }

void FSolver::remove_mesh_files_after_collective_solve()
{
    // what a one-device run deletes: LoadMesh's four files whenever it read
    // them (not for a mesh taken from the previous solution, fsolver.cpp:357-360),
    // the .edge only after Cuthill (which runs without a previous solution)
    if (!comm || !deleteMeshFiles || xfk_comm_rank(comm) != 0 || meshLoadedFromPrevSolution) return;
    std::vector<std::string> v;
    for (const char *ext : {".ele", ".node", ".pbc", ".poly"}) v.push_back(PathName + ext);
    if (previousSolutionFile.empty()) v.push_back(PathName + ".edge");
    remove_async(std::move(v));
}

std::string FSolver::getErrorString(LoadMeshErr err)
{
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
    case UNSUPPORTEDMESH: return "problem loading mesh:\nmalformed air-gap element data.\n";
    }
    return std::string();
}

bool FSolver::LoadProblemFile()
{
    if (!comm) start_hip_warmup();   // (a sharded FSolver's communicator has brought the device up already)
    Relax = 1.;
    std::string err;
    FemmProblemData &base = *this;
    // a previous-solution file set by the caller survives the parse unless the
    // .fem names one itself (FEASolver::CleanUp keeps previousSolutionFile,
    // feasolver.cpp:134-172; femmcli sets it before LoadProblemFile,
    // LuaMagneticsCommands.cpp:824)
    const std::string presetPrev = previousSolutionFile;
    if (!ParseFemFile(PathName + ".fem", base, err)) {
        warn(err);
        return false;
    }
    if (!prevSolnInFile) previousSolutionFile = presetPrev;
    meshLoadedFromPrevSolution = false;
    if (!previousSolutionFile.empty()) {
        // fsolver.cpp:224-238: the mesh (and A, for PrevType != 0) come from
        // the previous solution, and LoadProblemFile returns right there --
        // before GetSlopes and the serial-circuit expansion below.  On a B-H
        // block or a serial circuit the reference then runs on uncomputed
        // slopes / an unexpanded circuit (undefined); refused here.
        for (auto &prop : blockproplist)
            if (prop.BHpoints > 0) {
                warn("B-H curves with a previous solution: the reference never computes their slopes "
                     "(fsolver.cpp:224-238)\n");
                return false;
            }
        for (auto &c : circproplist)
            if (c.CircType == 1) {
                warn("serial circuits with a previous solution: the reference skips their expansion "
                     "(fsolver.cpp:224-238)\n");
                return false;
            }
        return loadPreviousSolution(PrevType != 0);
    }
    // B-H curves: GetSlopes(Frequency * 2 pi) (fsolver.cpp:241-276; the
    // harmonic curve is complex: effective sinusoidal-H amplitude, hysteresis
    // lag, lamination eddy currents)
    for (auto &prop : blockproplist)
        if (prop.BHpoints > 0) {
            if (!(Frequency != 0 ? prop.GetSlopesAC(Frequency * 2. * kPi) : prop.GetSlopes())) {
                warn("bad B-H curve in material " + prop.BlockName + "\n");
                return false;
            }
            prop.MuMax = 0;
        }
    const int NumBlockLabels = (int)labellist.size();
    for (auto &lb : labellist)
        if (lb.InCircuit >= (int)circproplist.size()) {
            warn("block label refers to an undefined circuit\n");
            return false;
        }
    int NumCircProps = (int)circproplist.size();
    if (NumCircProps == 0) return true;
    // serial circuits -> one parallel circuit per block label (fsolver.cpp:280-317)
    for (auto &c : circproplist) c.OrigCirc = -1;
    NumCircPropsOrig = NumCircProps;
    for (int k = 0; k < NumBlockLabels; k++)
        if (labellist[k].InCircuit >= 0) {
            int ic = labellist[k].InCircuit;
            if (circproplist[ic].CircType == 1) {
                CMCircuit ncirc = circproplist[ic];
                ncirc.OrigCirc = ic;
                ncirc.Amps_im *= labellist[k].Turns;
                ncirc.Amps_re *= labellist[k].Turns;
                circproplist.push_back(ncirc);
                labellist[k].InCircuit = NumCircProps;
                NumCircProps++;
            }
        }
    for (auto &c : circproplist)
        if (c.CircType == 1) c.CircType = 0;
    return true;
}

// FSolver::loadPreviousSolution (fsolver.cpp:990-1081) and its readers
// (:801-988).  A WriteStatic2D .ans has p0 p1 p2 lbl per element, so the
// 8-field scan leaves e[] and Jprev at the CMElement defaults of the
// reference -- e = {0, 0, 0} (CElement.cpp:30-39): every edge carries boundary
// property 0 -- and Jprev = 0.
bool FSolver::loadPreviousSolution(bool loadAprev)
{
    if (previousSolutionFile.empty()) return false;
    FILE *fp = fopen(previousSolutionFile.c_str(), "rt");
    if (!fp) {
        warn("Failed to open the specified previous solution file, file path was:\n" + previousSolutionFile + "\n");
        return false;
    }
    char s[1024];
    bool hasSolution = false;
    while (fgets(s, 1024, fp) != nullptr) {
        char q[256] = {0};
        sscanf(s, "%255s", q);
        std::string key(q);
        for (auto &ch : key) ch = (char)tolower((unsigned char)ch);
        if (key.compare(0, 11, "[frequency]") == 0) {
            double prevFreq = 0;
            const char *v = strchr(s, '=');
            if (v) sscanf(v + 1, "%lf", &prevFreq);
            if (prevFreq != 0) {
                fclose(fp);
                warn("Previous solution file (" + previousSolutionFile +
                     ") appears to be an AC problem, only DC previous solutions are presently supported\n");
                return false;
            }
        }
        if (key.compare(0, 10, "[solution]") == 0) {
            hasSolution = true;
            break;
        }
    }
    if (!hasSolution) {
        fclose(fp);
        warn("No solution was found in previous solution file, file path was:\n" + previousSolutionFile + "\n");
        return false;
    }
    auto fail = [&](const char *what) {
        fclose(fp);
        warn(std::string("malformed previous solution file (") + what + "): " + previousSolutionFile + "\n");
        return false;
    };
    // nodes: x y A marker, lengths back to cm (fsolver.cpp:801-840)
    if (!fgets(s, 1024, fp) || sscanf(s, "%i", &NumNodes) != 1 || NumNodes < 0) return fail("node count");
    Aprev.clear();
    meshnode.assign(NumNodes, CNode());
    const double conv = 100 * kLengthConvMeters[LengthUnits];
    for (int i = 0; i < NumNodes; i++) {
        CNode node;
        double a = 0;
        if (!fgets(s, 1024, fp) || sscanf(s, "%lf %lf %lf %i", &node.x, &node.y, &a, &node.BoundaryMarker) < 3)
            return fail("node line");
        node.x *= conv;
        node.y *= conv;
        if (loadAprev) Aprev.push_back(a);
        meshnode[i] = node;
    }
    // elements: p0 p1 p2 lbl [e0 e1 e2 Jprev] (fsolver.cpp:842-880)
    if (!fgets(s, 1024, fp) || sscanf(s, "%i", &NumEls) != 1 || NumEls < 0) return fail("element count");
    meshele.assign(NumEls, CMElement());
    for (int i = 0; i < NumEls; i++) {
        CMElement elm;
        elm.e[0] = elm.e[1] = elm.e[2] = 0;
        if (!fgets(s, 1024, fp) ||
            sscanf(s, "%i %i %i %i %i %i %i %lf", &elm.p[0], &elm.p[1], &elm.p[2], &elm.lbl, &elm.e[0], &elm.e[1],
                   &elm.e[2], &elm.Jprev) < 4)
            return fail("element line");
        if (elm.lbl < 0 || elm.lbl >= (int)labellist.size()) return fail("element label");
        for (int q = 0; q < 3; q++)
            if (elm.p[q] < 0 || elm.p[q] >= NumNodes) return fail("element node");
        elm.blk = labellist[elm.lbl].BlockType;
        meshele[i] = elm;
    }
    // block-label circuit lines: skipped
    int numLabels = 0;
    if (!fgets(s, 1024, fp) || sscanf(s, "%i", &numLabels) != 1) return fail("label count");
    for (int i = 0; i < numLabels; i++)
        if (!fgets(s, 1024, fp)) return fail("label line");
    // periodic pairs (fsolver.cpp:882-909)
    NumPBCs = 0;
    pbclist.clear();
    if (fgets(s, 1024, fp) != nullptr) {
        sscanf(s, "%i", &NumPBCs);
        for (int i = 0; i < NumPBCs; i++) {
            CCommonPoint pbc;
            if (!fgets(s, 1024, fp) || sscanf(s, "%i %i %i", &pbc.x, &pbc.y, &pbc.t) != 3) return fail("pbc line");
            pbclist.push_back(pbc);
        }
    }
    // air-gap elements (fsolver.cpp:911-988): name (80 characters), parameters, quadNodes
    NumAirGapElems = 0;
    agelist.clear();
    if (fgets(s, 1024, fp) != nullptr) sscanf(s, "%i", &NumAirGapElems);
    for (int i = 0; i < NumAirGapElems; i++) {
        AirGap g;
        if (!fgets(s, 80, fp)) return fail("air-gap name");
        g.name = s;
        if (!fgets(s, 1024, fp) ||
            sscanf(s, "%i %lf %lf %lf %lf %lf %lf %lf %i %lf %lf", &g.format, &g.inner_angle, &g.outer_angle, &g.ri,
                   &g.ro, &g.arc, &g.agc_re, &g.agc_im, &g.n_arc, &g.inner_shift, &g.outer_shift) != 11 ||
            g.n_arc <= 0)
            return fail("air-gap parameters");
        for (int k = 0; k <= g.n_arc; k++) {
            int n[4];
            double w[4];
            if (!fgets(s, 1024, fp) ||
                sscanf(s, "%i %lf %i %lf %i %lf %i %lf", &n[0], &w[0], &n[1], &w[1], &n[2], &w[2], &n[3], &w[3]) != 8)
                return fail("air-gap quadNode");
            for (int m = 0; m < 4; m++) {
                if (n[m] < 0 || n[m] >= NumNodes) {
                    fclose(fp);
                    warn("An error occured while reading pbc file, quadNode has negative node number.\n");
                    return false;
                }
                g.qn.push_back(n[m]);
                g.qw.push_back(w[m]);
            }
        }
        agelist.push_back(g);
    }
    fclose(fp);
    BandWidth = 0;
    meshLoadedFromPrevSolution = true;
    return true;
}


LoadMeshErr FSolver::LoadMesh(bool deleteFiles)
{
    if (meshLoadedFromPrevSolution) return NOERROR;   // fsolver.cpp:357-360
    LoadTrace tr;
    char s[1024];
    std::string infile;
    TextBuf tb;
    {   // one buffer for the three mesh files: the largest one's size
        struct stat st;
        for (const char *ext : {".node", ".ele", ".edge"})
            if (::stat((PathName + ext).c_str(), &st) == 0) tb.hint = std::max(tb.hint, (size_t)st.st_size + 1);
    }
    int j = 0;
    const double conv = 100 * kLengthConvMeters[LengthUnits];
    if (!read_node_file(tb, meshnode, [conv](CNode &node, double x, double y, int m) {
            node.BoundaryMarker = (m > 1) ? m - 2 : -1;
            node.x = x * conv;   // lengths in cm (fsolver.cpp:386-388)
            node.y = y * conv;
        }))
        return BADNODEFILE;

    infile = PathName + ".pbc";
    FILE *fp = fopen(infile.c_str(), "rt");
    if (!fp) return BADPBCFILE;
    NumPBCs = 0;
    if (fgets(s, 1024, fp)) sscanf(s, "%i", &NumPBCs);
    pbclist.clear();
    for (int i = 0; i < NumPBCs; i++) {
        CCommonPoint pbc;
        if (!fgets(s, 1024, fp) || sscanf(s, "%i %i %i %i", &j, &pbc.x, &pbc.y, &pbc.t) != 4) {
            fclose(fp);
            return BADPBCFILE;
        }
        pbclist.push_back(pbc);
    }
    // air-gap elements: name, parameter line, totalArcElements + 1 quadNodes
    NumAirGapElems = 0;
    if (fgets(s, 1024, fp)) sscanf(s, "%i", &NumAirGapElems);
    agelist.clear();
    for (int i = 0; i < NumAirGapElems; i++) {
        AirGap g;
        bool ok = fgets(s, 1024, fp) != nullptr;
        g.name = s;
        ok = ok && fgets(s, 1024, fp) &&
             sscanf(s, "%i %lf %lf %lf %lf %lf %lf %lf %i %lf %lf", &g.format, &g.inner_angle, &g.outer_angle,
                    &g.ri, &g.ro, &g.arc, &g.agc_re, &g.agc_im, &g.n_arc, &g.inner_shift, &g.outer_shift) == 11;
        ok = ok && g.n_arc > 0;
        for (int k = 0; ok && k <= g.n_arc; k++) {
            int n[4];
            double w[4];
            ok = fgets(s, 1024, fp) && sscanf(s, "%i %lf %i %lf %i %lf %i %lf", &n[0], &w[0], &n[1], &w[1], &n[2],
                                              &w[2], &n[3], &w[3]) == 8;
            for (int m = 0; ok && m < 4; m++) {
                ok = n[m] >= 0 && n[m] < NumNodes;   // negative quadNode: the reference rejects the file too
                g.qn.push_back(n[m]);
                g.qw.push_back(w[m]);
            }
        }
        if (!ok) {
            fclose(fp);
            return BADPBCFILE;
        }
        agelist.push_back(g);
    }
    fclose(fp);

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
        if (bad.code == 1) {
            char buf[256];
            snprintf(buf, sizeof buf, "The element number %i had label %i\n", bad.index, meshele[bad.index].lbl);
            warn(std::string("Material properties have not been defined for all regions.\n") + buf);
            if (deleteFiles) remove_files();
            return MISSINGMATPROPS;
        }
        if (bad.code == 2) {
            if (deleteFiles) remove_files();
            return ELMLABELTOOBIG;
        }
        if (bad.code) return BADELEMENTFILE;
    }
    tr.mark("elements");

    std::vector<int> marked;
    if (!read_edge_file(tb, marked)) return BADEDGEFILE;
    // boundary-marked edges (marker < 0) set the boundary property of the
    // element sides they match (fsolver.cpp:660-704: per edge, every element
    // around its first node whose side k joins the two nodes).  The last such
    // edge in file order wins a side, so the side takes the property of the
    // last marked edge with its node pair: a map from the (unordered) pair,
    // filled in file order, looked up per element side in parallel -- no
    // node -> element membership lists
    {
        std::unordered_map<unsigned long long, int> side_bc;
        std::vector<char> on_marked(NumNodes, 0);
        auto pair_key = [](int a, int b) {
            return ((unsigned long long)(unsigned)std::min(a, b) << 32) | (unsigned)std::max(a, b);
        };
        for (int i : marked) {
            const auto &e = edges_[i];
            side_bc[pair_key(e[0], e[1])] = -(e[2] + 2);
            on_marked[e[0]] = on_marked[e[1]] = 1;
        }
        if (!side_bc.empty())
            par_for(NumEls, 1 << 15, [&](long long a, long long b) {
                for (long long i = a; i < b; i++) {
                    CMElement &el = meshele[i];
                    for (int q = 0; q < 3; q++) {
                        const int n0 = el.p[q], n1 = el.p[(q + 1) % 3];
                        if (!on_marked[n0] || !on_marked[n1]) continue;
                        auto it = side_bc.find(pair_key(n0, n1));
                        if (it != side_bc.end()) el.e[q] = it->second;
                    }
                }
            });
    }
    tr.mark("edges");
    if (deleteFiles) remove_async({PathName + ".ele", PathName + ".node", PathName + ".pbc", PathName + ".poly"});
    return NOERROR;
}


int FSolver::SortElements() { return sort_mesh_elements(meshele); }

int FSolver::Cuthill(bool deleteFiles)
{
    return cuthill_mesh(meshnode, meshele, deleteFiles, [&](const BigVec<int> &newnum) {
        for (auto &g : agelist)   // cuthill.cpp:321-330
            for (int &q : g.qn) q = newnum[q];
    });
}

void FSolver::GetFillFactor(int lbl)
{
    // bIsWound, and at AC the proximity-effect permeability of a wound
    // LamType > 2 region (fsolver.cpp:1083-1193): an equivalent-foil model for
    // rectangular wire, a fitted frequency-dependent permeability for round
    // wire (magnet, stranded, litz, copper-clad aluminium)
    CMBlockLabel &bl = labellist[lbl];
    const int lt = (bl.BlockType >= 0) ? blockproplist[bl.BlockType].LamType : 0;
    bl.bIsWound = (std::abs(bl.Turns) > 1) || (lt > 2);
    bl.ProxMu_re = 1;
    bl.ProxMu_im = 0;
    if (Frequency == 0 || lt < 3) return;
    // the region's area, m^2 (ElmArea, fsolver.cpp:1196-1210)
    double atot = 0;
    for (const auto &el : meshele) {
        if (el.lbl != lbl) continue;
        const CNode &a = meshnode[el.p[0]], &b = meshnode[el.p[1]], &c = meshnode[el.p[2]];
        const double b0 = b.y - c.y, b1 = c.y - a.y, c0 = c.x - b.x, c1 = a.x - c.x;
        atot += 0.0001 * (b0 * c1 - b1 * c0) / 2.;
    }
    if (atot == 0) return;   // ProximityMu keeps its previous value (1 here)
    const CMSolverMaterialProp &bp = blockproplist[bl.BlockType];
    if (bp.Cduct == 0) return;
    using cd = std::complex<double>;
    const cd I(0, 1);
    const double muo = 4.e-7 * kPi;
    const int wiretype = lt - 3;
    cd mu;
    if (wiretype == 3) {   // rectangular wire: equivalent foil
        const double W = 2. * kPi * Frequency, d = bp.WireD * 0.001;
        double fill = std::fabs(d * d * (double)bl.Turns / atot);
        const double pitch = d / std::sqrt(fill);
        fill = d / pitch;
        const double o = bp.Cduct * fill * 1.e6;
        const cd k = std::sqrt(I * W * o * muo) * d / 2.;
        const cd ufd = muo * std::tanh(k) / k;
        mu = (fill * ufd + (1. - fill) * muo) / muo;
    } else {
        double R = 0, awire = 0;
        const double turns = (double)bl.Turns, ns = (double)bp.NStrands;
        if (wiretype == 0 || wiretype == 2) {   // magnet wire, litz: NStrands strands of WireD
            R = bp.WireD * 0.0005;
            awire = kPi * R * R * ns * turns;
        } else if (wiretype == 1) {             // stranded, non-litz: one conductor of the bundle's area
            R = bp.WireD * 0.0005 * std::sqrt(ns);
            awire = kPi * R * R * turns;
        }                                       // CCA (4, 5): the reference leaves R and awire at 0
        const double fill = std::fabs(awire / atot);
        const double W = 2. * kPi * Frequency * bp.Cduct * 1.e6 * muo * R * R / 2.;
        double c1 = 0, c2 = 0;
        if (wiretype <= 2) {
            c1 = 0.7756067409818643 + fill * (0.6873854335408803 + fill * (0.06841584481674128 - 0.07143732702512284 * fill));
            c2 = 1.5 * fill / c1;
        } else if (wiretype == 4) {
            c1 = 0.7270741505617485 + 0.8902950067721367 * fill + 0.11894736885885195 * fill * fill -
                 0.12247276254503957 * fill * fill * fill;
            c2 = 0.006784920229549677 + 1.8942880489198526 * fill - 1.3631438759519217 * fill * fill +
                 0.504431701685587 * fill * fill * fill;
        } else if (wiretype == 5) {
            c1 = 0.7486913529860821 + 0.9042845510838825 * fill + 0.1361040321433224 * fill * fill -
                 0.10652380745682069 * fill * fill * fill;
            c2 = 0.006790468527313965 + 1.8945509985370095 * fill - 1.3643501010185972 * fill * fill +
                 0.5036765577982594 * fill * fill * fill;
        }
        const cd z = std::sqrt(c1 * I * W);
        mu = c2 * (std::tanh(z) / z) + (1. - c2);
    }
    bl.ProxMu_re = mu.real();
    bl.ProxMu_im = mu.imag();
}

// the C-ABI descriptor of the current problem and the arrays it points into
struct FSolver::DescStore {
    std::vector<xfk_block_desc> blk;
    std::vector<xfk_label_desc> lab;
    std::vector<xfk_line_desc> lin;
    std::vector<xfk_point_desc> pts;
    std::vector<xfk_circuit_desc> cir;
    std::vector<double> x, y;
    std::vector<int> marker, p, e, lbl, pbc;
    std::vector<xfk_age_desc> age;
    xfk_problem_desc d{};
};

bool FSolver::make_desc(DescStore &ds)
{
    for (int i = 0; i < (int)labellist.size(); i++) GetFillFactor(i);
    ds.blk.resize(blockproplist.size());
    for (size_t k = 0; k < blockproplist.size(); k++) {
        const CMSolverMaterialProp &m = blockproplist[k];
        xfk_block_desc &d = ds.blk[k];
        d.mu_x = m.mu_x; d.mu_y = m.mu_y; d.H_c = m.H_c; d.J_re = m.J_re; d.Cduct = m.Cduct;
        d.LamFill = m.LamFill; d.LamType = m.LamType; d.BHpoints = m.BHpoints;
        d.B = m.Bdata.empty() ? nullptr : m.Bdata.data();
        d.H = m.Hdata.empty() ? nullptr : m.Hdata.data();
        d.slope = m.slope.empty() ? nullptr : m.slope.data();
    }
    if (ds.blk.empty()) {
        warn("no block properties defined\n");
        return false;
    }
    ds.lab.resize(labellist.size());
    for (size_t k = 0; k < labellist.size(); k++) {
        ds.lab[k].block = labellist[k].BlockType >= 0 ? labellist[k].BlockType : 0;
        ds.lab[k].in_circuit = labellist[k].InCircuit;
        ds.lab[k].mag_dir = labellist[k].MagDir;
        ds.lab[k].is_wound = labellist[k].bIsWound ? 1 : 0;
        ds.lab[k].is_external = labellist[k].IsExternal ? 1 : 0;
        ds.lab[k].mag_dir_fctn = labellist[k].MagDirFctn.empty() ? nullptr : labellist[k].MagDirFctn.c_str();
    }
    ds.lin.resize(lineproplist.size());
    for (size_t k = 0; k < lineproplist.size(); k++) {
        const CMBoundaryProp &b = lineproplist[k];
        ds.lin[k] = xfk_line_desc{b.BdryFormat, b.A0, b.A1, b.A2, b.phi, b.c0_re, b.c1_re};
    }
    ds.pts.resize(nodeproplist.size());
    for (size_t k = 0; k < nodeproplist.size(); k++)
        ds.pts[k] = xfk_point_desc{nodeproplist[k].A_re, nodeproplist[k].A_im, nodeproplist[k].J_re,
                                   nodeproplist[k].J_im};
    ds.cir.resize(circproplist.size());
    for (size_t k = 0; k < circproplist.size(); k++)
        ds.cir[k] = xfk_circuit_desc{circproplist[k].CircType, circproplist[k].Amps_re, circproplist[k].dVolts_re};
    // the mesh arrays: huge-page storage, filled in parallel
    huge_reserve(ds.x, (size_t)NumNodes);
    huge_reserve(ds.y, (size_t)NumNodes);
    huge_reserve(ds.marker, (size_t)NumNodes);
    huge_reserve(ds.p, 3ull * NumEls);
    huge_reserve(ds.e, 3ull * NumEls);
    huge_reserve(ds.lbl, (size_t)NumEls);
    ds.x.resize(NumNodes);
    ds.y.resize(NumNodes);
    ds.marker.resize(NumNodes);
    ds.p.resize(3LL * NumEls);
    ds.e.resize(3LL * NumEls);
    ds.lbl.resize(NumEls);
    ds.pbc.resize(3LL * NumPBCs);
    const int nnp = (int)nodeproplist.size(), nlp = (int)lineproplist.size();
    par_for(NumNodes, 1 << 16, [&](long long a, long long b) {
        for (long long i = a; i < b; i++) {
            ds.x[i] = meshnode[i].x;
            ds.y[i] = meshnode[i].y;
            const int m = meshnode[i].BoundaryMarker;
            ds.marker[i] = m >= nnp ? -1 : m;
        }
    });
    std::atomic<bool> hole{false};
    par_for(NumEls, 1 << 16, [&](long long a, long long b) {
        for (long long i = a; i < b; i++) {
            const CMElement &el = meshele[i];
            if (labellist[el.lbl].BlockType < 0) hole = true;
            for (int q = 0; q < 3; q++) {
                ds.p[3 * i + q] = el.p[q];
                const int eq = el.e[q];
                ds.e[3 * i + q] = (eq >= 0 && eq < nlp) ? eq : -1;
            }
            ds.lbl[i] = el.lbl;
        }
    });
    if (hole) {
        warn("an element lies in a region without material (hole label)\n");
        return false;
    }
    for (int k = 0; k < NumPBCs; k++) {
        ds.pbc[3 * k] = pbclist[k].x;
        ds.pbc[3 * k + 1] = pbclist[k].y;
        ds.pbc[3 * k + 2] = pbclist[k].t;
    }
    xfk_problem_desc &d = ds.d;
    d.n_nodes = NumNodes; d.x = ds.x.data(); d.y = ds.y.data(); d.marker = ds.marker.data();
    d.n_elems = NumEls; d.p = ds.p.data(); d.e = ds.e.data(); d.lbl = ds.lbl.data();
    d.n_blocks = (int)ds.blk.size(); d.blocks = ds.blk.data();
    d.n_labels = (int)ds.lab.size(); d.labels = ds.lab.data();
    d.n_lines = (int)ds.lin.size(); d.lines = ds.lin.empty() ? nullptr : ds.lin.data();
    d.n_points = (int)ds.pts.size(); d.points = ds.pts.empty() ? nullptr : ds.pts.data();
    d.n_circs = (int)ds.cir.size(); d.circs = ds.cir.empty() ? nullptr : ds.cir.data();
    d.n_pbc = NumPBCs; d.pbc = NumPBCs ? ds.pbc.data() : nullptr;
    ds.age.clear();
    for (const AirGap &g : agelist) {
        xfk_age_desc a{};
        a.format = g.format; a.ri = g.ri; a.ro = g.ro; a.total_arc_length = g.arc;
        a.inner_shift = g.inner_shift; a.outer_shift = g.outer_shift; a.n_arc = g.n_arc;
        a.qn = g.qn.data(); a.qw = g.qw.data();
        ds.age.push_back(a);
    }
    d.n_ages = (int)ds.age.size(); d.ages = ds.age.empty() ? nullptr : ds.age.data();
    d.precision = Precision;
    d.length_units = (int)LengthUnits;
    d.coords = (int)Coords;
    d.relax = Relax;
    d.problem_type = ProblemTypeV == AXISYMMETRIC ? XFK_AXISYMMETRIC : XFK_PLANAR;
    d.ext_zo = extZo;
    d.ext_ro = extRo;
    d.ext_ri = extRi;
    return true;
}

int FSolver::Static2D()
{
    join_hip_warmup();
    auto t = std::chrono::steady_clock::now();
    DescStore ds;
    if (!make_desc(ds)) return false;
    // the .ans element section depends on the mesh only: formatted while the
    // device solves (joined by WriteStatic2D, or below on failure)
    if (ele_fmt_.joinable()) ele_fmt_.join();
    if (writes_output())
        ele_fmt_ = std::thread([this] {
            ele_text_ = format_static_elements();
            node_parts_ = format_static_node_parts();
        });
    if (problem) {   // (a kept problem of the last solve)
        xfk_problem_destroy(problem);
        problem = nullptr;
    }
    xfk_problem *prob = nullptr;
    int rc = comm ? xfk_problem_create_dist(&ds.d, device, comm, &prob) : xfk_problem_create(&ds.d, device, &prob);
    ms_phase[2] = ms_since(t);
    if (rc == XFK_OK) rc = xfk_static2d(prob, 0, &stats);
    if (rc == XFK_OK) {
        A.assign(NumNodes, 0.0);
        rc = xfk_get_solution(prob, A.data());
    }
    if (rc == XFK_OK && !circproplist.empty()) {
        std::vector<int> cc(circproplist.size());
        std::vector<double> J(circproplist.size()), dV(circproplist.size());
        rc = xfk_get_circuits(prob, cc.data(), J.data(), dV.data());
        for (size_t k = 0; rc == XFK_OK && k < circproplist.size(); k++) {
            circproplist[k].Case = cc[k];
            circproplist[k].J = J[k];
            circproplist[k].dV = dV[k];
        }
    }
    if (rc != XFK_OK) {
        warn(std::string("GPU solver error: ") + xfk_last_error() + "\n");
        if (ele_fmt_.joinable()) ele_fmt_.join();
        ele_text_ = Formatted();
        node_parts_ = NodeParts();
    }
    if (rc == XFK_OK && keepProblem && !comm && xfk_mag_set_depth(prob, Depth) == XFK_OK) {
        problem = prob;   // post-processed by the caller (the xfk_mag_ entry points)
        prob = nullptr;
    }
    if (prob) xfk_problem_destroy(prob);
    ms_phase[3] = ms_since(t);
    return rc == XFK_OK;
}

int FSolver::Harmonic2D()
{
    join_hip_warmup();
    auto t = std::chrono::steady_clock::now();
    DescStore ds;
    if (!make_desc(ds)) return false;
    std::vector<xfk_block_ac_desc> bac(blockproplist.size());
    for (size_t k = 0; k < blockproplist.size(); k++) {
        const CMSolverMaterialProp &m = blockproplist[k];
        const bool bh = m.BHpoints > 0;
        bac[k] = xfk_block_ac_desc{m.J_im, m.Theta_hx, m.Theta_hy, m.Lam_d, bh ? m.Hdata_im.data() : nullptr,
                                   bh ? m.slope_im.data() : nullptr};
    }
    std::vector<xfk_line_ac_desc> lac(lineproplist.size());
    for (size_t k = 0; k < lineproplist.size(); k++) {
        const CMBoundaryProp &b = lineproplist[k];
        lac[k] = xfk_line_ac_desc{b.c0_im, b.c1_im, b.Mu, b.Sig};
    }
    std::vector<xfk_circuit_ac_desc> cac(circproplist.size());
    for (size_t k = 0; k < circproplist.size(); k++)
        cac[k] = xfk_circuit_ac_desc{circproplist[k].Amps_im, circproplist[k].dVolts_im};
    std::vector<double> prox(2 * std::max<size_t>(1, labellist.size()), 0.0);
    for (size_t k = 0; k < labellist.size(); k++) {
        if (!std::isfinite(labellist[k].ProxMu_re) || !std::isfinite(labellist[k].ProxMu_im)) {
            // copper-clad aluminium wire (LamType 7, 8): the reference's
            // GetFillFactor leaves the wire radius at 0, ProximityMu = 0/0
            warn("copper-clad aluminium windings (LamType 7, 8) have no defined proximity permeability "
                 "(the reference computes 0/0); not supported\n");
            return false;
        }
        prox[2 * k] = labellist[k].ProxMu_re;
        prox[2 * k + 1] = labellist[k].ProxMu_im;
    }
    xfk_harmonic_desc ac{Frequency, bac.data(), lac.empty() ? nullptr : lac.data(),
                         cac.empty() ? nullptr : cac.data(), ACSolver, prox.data(),
                         previousSolutionFile.empty() ? 0 : PrevType};
    if (problem) {   // (a kept problem of the last solve)
        xfk_problem_destroy(problem);
        problem = nullptr;
    }
    xfk_problem *prob = nullptr;
    int rc = comm ? xfk_problem_create_harmonic_dist(&ds.d, &ac, device, comm, &prob)
                  : xfk_problem_create_harmonic(&ds.d, &ac, device, &prob);
    ms_phase[2] = ms_since(t);
    if (rc == XFK_OK) rc = xfk_harmonic2d(prob, 0, &stats);
    std::vector<double> Ac;
    if (rc == XFK_OK) {
        Ac.assign(2 * (size_t)NumNodes, 0.0);
        rc = xfk_get_solution_complex(prob, Ac.data());
    }
    if (rc == XFK_OK) {
        A.resize(NumNodes);
        A_im.resize(NumNodes);
        for (int i = 0; i < NumNodes; i++) {
            A[i] = Ac[2 * i];
            A_im[i] = Ac[2 * i + 1];
        }
    }
    if (rc == XFK_OK && !circproplist.empty()) {
        const size_t nc = circproplist.size();
        std::vector<int> cc(nc);
        std::vector<double> J(2 * nc), dV(2 * nc);
        rc = xfk_get_circuits_complex(prob, cc.data(), J.data(), dV.data());
        for (size_t k = 0; rc == XFK_OK && k < nc; k++) {
            circproplist[k].Case = cc[k];
            circproplist[k].J = J[2 * k];
            circproplist[k].J_im = J[2 * k + 1];
            circproplist[k].dV = dV[2 * k];
            circproplist[k].dV_im = dV[2 * k + 1];
        }
    }
    if (rc != XFK_OK) warn(std::string("GPU solver error: ") + xfk_last_error() + "\n");
    if (rc == XFK_OK && keepProblem && !comm && xfk_mag_set_depth(prob, Depth) == XFK_OK) {
        problem = prob;   // post-processed by the caller (the xfk_mag_ac_ entry points)
        prob = nullptr;
    }
    if (prob) xfk_problem_destroy(prob);
    ms_phase[3] = ms_since(t);
    return rc == XFK_OK;
}

FSolver::Formatted FSolver::format_static_elements() const
{
    return format_lines(NumEls, 64, [&](int i, char *q) {
        for (int m = 0; m < 3; ++m) {
            q = put_i(q, meshele[i].p[m]);
            *q++ = '\t';
        }
        q = put_i(q, meshele[i].lbl);
        *q++ = '\n';
        return q;
    });
}

FSolver::NodeParts FSolver::format_static_node_parts() const
{
    const double unitconv[] = {2.54, 0.1, 1., 100., 0.00254, 1.e-04};
    const double cf = unitconv[LengthUnits];
    NodeParts np;
    const int n = NumNodes, T = format_chunks(n);
    np.lo.resize(T + 1);
    for (int t = 0; t <= T; ++t) np.lo[t] = (int)((long long)n * t / T);
    np.pre.resize(n);
    np.suf.resize(n);
    np.f = format_lines(n, 104, [&](int i, char *q) {
        char *q0 = q;
        q = put_g17(q, meshnode[i].x / cf);
        *q++ = '\t';
        q = put_g17(q, meshnode[i].y / cf);
        *q++ = '\t';
        np.pre[i] = (unsigned char)(q - q0);
        q0 = q;
        *q++ = '\t';
        q = put_i(q, meshnode[i].BoundaryMarker);
        // static2d.cpp:1093-1101: Aprev follows the marker with no separator
        if (!Aprev.empty()) q = put_g17(q, Aprev[i]);
        *q++ = '\n';
        np.suf[i] = (unsigned char)(q - q0);
        return q;
    });
    return np;
}

int FSolver::WriteStatic2D()
{
    LoadTrace tr;
    const double unitconv[] = {2.54, 0.1, 1., 100., 0.00254, 1.e-04};
    std::string fin = PathName + ".fem", fout = PathName + ".ans";
    FILE *fz = fopen(fin.c_str(), "rt");
    if (!fz) {
        warn("Couldn't open " + fin + "\n");
        return false;
    }
    clear_old_output(fout);
    FILE *fp = fopen(fout.c_str(), "wt");
    if (!fp) {
        fclose(fz);
        warn("Couldn't write to " + fout + "\n");
        return false;
    }
    char c[1024];
    while (fgets(c, 1024, fz) != nullptr) fputs(c, fp);
    fclose(fz);
    tr.mark("  .fem echo");
    fprintf(fp, "[Solution]\n");
    const double cf = unitconv[LengthUnits];
    fprintf(fp, "%i\n", NumNodes);
    fflush(fp);
    if (ele_fmt_.joinable()) ele_fmt_.join();   // (element text and node parts formatted beside the device solve)
    Formatted nodes_text;
    NodeParts &np = node_parts_;
    if (np.lo.size() >= 2 && np.lo.back() == NumNodes && (int)np.f.buf.size() == (int)np.lo.size() - 1) {
        // the parts around A, with A put in between
        const int T = (int)np.lo.size() - 1;
        nodes_text.buf.resize(T);
        nodes_text.len.assign(T, 0);
        par_for(T, 1, [&](long long t0, long long t1) {
            for (long long t = t0; t < t1; ++t) {
                const int a = np.lo[t], b = np.lo[t + 1];
                if (!nodes_text.buf[t].allocate(np.f.len[t] + (size_t)(b - a) * 25 + 1)) continue;
                const char *p = np.f.buf[t].data();
                char *q = nodes_text.buf[t].data();
                for (int i = a; i < b; ++i) {
                    std::memcpy(q, p, np.pre[i]);
                    q += np.pre[i];
                    p += np.pre[i];
                    q = put_g17(q, A[i]);
                    std::memcpy(q, p, np.suf[i]);
                    q += np.suf[i];
                    p += np.suf[i];
                }
                nodes_text.len[t] = (size_t)(q - nodes_text.buf[t].data());
            }
        });
    } else {
        nodes_text = format_lines(NumNodes, 128, [&](int i, char *q) {
            q = put_g17(q, meshnode[i].x / cf);
            *q++ = '\t';
            q = put_g17(q, meshnode[i].y / cf);
            *q++ = '\t';
            q = put_g17(q, A[i]);
            *q++ = '\t';
            q = put_i(q, meshnode[i].BoundaryMarker);
            // static2d.cpp:1093-1101: Aprev follows the marker with no separator
            if (!Aprev.empty()) q = put_g17(q, Aprev[i]);
            *q++ = '\n';
            return q;
        });
    }
    node_parts_ = NodeParts();
    tr.mark("  .ans nodes formatted");
    if (!write_formatted(fp, nodes_text)) {
        fclose(fp);
        warn("couldn't allocate the .ans node text\n");
        return false;
    }
    tr.mark("  .ans nodes written");
    fprintf(fp, "%i\n", NumEls);
    fflush(fp);
    if (ele_text_.buf.empty()) ele_text_ = format_static_elements();
    tr.mark("  .ans element text joined");
    const bool ele_ok = write_formatted(fp, ele_text_);
    ele_text_ = Formatted();
    if (!ele_ok) {
        fclose(fp);
        warn("couldn't allocate the .ans element text\n");
        return false;
    }
    tr.mark("  .ans elements");
    fprintf(fp, "%i\n", (int)labellist.size());
    for (size_t k = 0; k < labellist.size(); k++) {
        int i = labellist[k].InCircuit;
        if (i < 0) fprintf(fp, "1\t0\n");
        else {
            if (circproplist[i].Case == 0) fprintf(fp, "0\t%.17g\n", circproplist[i].dV);
            if (circproplist[i].Case == 1) fprintf(fp, "1\t%.17g\n", circproplist[i].J);
        }
    }
    fprintf(fp, "%i\n", NumPBCs);
    for (int k = 0; k < NumPBCs; k++) fprintf(fp, "%i\t%i\t%i\n", pbclist[k].x, pbclist[k].y, pbclist[k].t);
    WriteAirGapElements(fp);
    fclose(fp);
    tr.mark("  .ans close");
    return true;
}

void FSolver::WriteAirGapElements(FILE *fp) const
{
    // static2d.cpp:1161-1190 / harmonic2d.cpp:1002-1030: per AGE its name as
    // read from the .pbc (newline kept), the parameter line, and the
    // totalArcElements + 1 quadNodes in the renumbered node ids -- the input
    // fpproc's gap integrals (torque, force) read back
    fprintf(fp, "%i\n", NumAirGapElems);
    for (const AirGap &g : agelist) {
        fprintf(fp, "%s", g.name.c_str());
        fprintf(fp, "%i %.17g %.17g %.17g %.17g %.17g %.17g %.17g %i %.17g %.17g\n", g.format, g.inner_angle,
                g.outer_angle, g.ri, g.ro, g.arc, g.agc_re, g.agc_im, g.n_arc, g.inner_shift, g.outer_shift);
        for (int k = 0; k <= g.n_arc; k++)
            fprintf(fp, "%i %.17g %i %.17g %i %.17g %i %.17g\n", g.qn[4 * k], g.qw[4 * k], g.qn[4 * k + 1],
                    g.qw[4 * k + 1], g.qn[4 * k + 2], g.qw[4 * k + 2], g.qn[4 * k + 3], g.qw[4 * k + 3]);
    }
}

int FSolver::WriteHarmonic2D()
{
    // harmonic2d.cpp:793-960: echo the .fem, then nodes (x, y, A re, A im,
    // marker), elements (p, label, edge markers), circuit data per label,
    // periodic pairs, air-gap elements
    const double unitconv[] = {2.54, 0.1, 1., 100., 0.00254, 1.e-04};
    std::string fin = PathName + ".fem", fout = PathName + ".ans";
    FILE *fz = fopen(fin.c_str(), "rt");
    if (!fz) {
        warn("Couldn't open " + fin + "\n");
        return false;
    }
    FILE *fp = fopen(fout.c_str(), "wt");
    if (!fp) {
        fclose(fz);
        warn("Couldn't write to " + fout + "\n");
        return false;
    }
    char c[1024];
    while (fgets(c, 1024, fz) != nullptr) fputs(c, fp);
    fclose(fz);
    fprintf(fp, "[Solution]\n");
    const double cf = unitconv[LengthUnits];
    fprintf(fp, "%i\n", NumNodes);
    // incremental problems add A of the previous solution per node and J per
    // element (harmonic2d.cpp:929-949)
    fflush(fp);
    bool text_ok = write_lines(fp, NumNodes, 160, [&](int i, char *q) {
        for (double v : {meshnode[i].x / cf, meshnode[i].y / cf, A[i], A_im[i]}) {
            q = put_g17(q, v);
            *q++ = '\t';
        }
        q = put_i(q, meshnode[i].BoundaryMarker);
        if (!Aprev.empty()) {
            *q++ = '\t';
            q = put_g17(q, Aprev[i]);
        }
        *q++ = '\n';
        return q;
    });
    if (text_ok) fprintf(fp, "%i\n", NumEls);
    fflush(fp);
    text_ok = text_ok && write_lines(fp, NumEls, 128, [&](int i, char *q) {
        const CMElement &e = meshele[i];
        for (int v : {e.p[0], e.p[1], e.p[2], e.lbl, e.e[0], e.e[1]}) {
            q = put_i(q, v);
            *q++ = '\t';
        }
        q = put_i(q, e.e[2]);
        if (!Aprev.empty()) {
            *q++ = '\t';
            q = put_g17(q, e.Jprev);
        }
        *q++ = '\n';
        return q;
    });
    if (!text_ok) {
        fclose(fp);
        warn("couldn't allocate the .ans text\n");
        return false;
    }
    fprintf(fp, "%i\n", (int)labellist.size());
    for (size_t k = 0; k < labellist.size(); k++) {
        int i = labellist[k].InCircuit;
        if (i < 0) fprintf(fp, "1\t0\t0\n");
        else {
            const CMCircuit &C = circproplist[i];
            if (C.Case == 0) fprintf(fp, "0\t%.17g\t%.17g\n", C.dV, C.dV_im);
            if (C.Case == 1) fprintf(fp, "1\t%.17g\t%.17g\n", C.J, C.J_im);
        }
    }
    fprintf(fp, "%i\n", NumPBCs);
    for (int k = 0; k < NumPBCs; k++) fprintf(fp, "%i  %i %i\n", pbclist[k].x, pbclist[k].y, pbclist[k].t);
    WriteAirGapElements(fp);
    fclose(fp);
    return true;
}

bool FSolver::runSolver(bool verbose)
{
    struct JoinRemovals {   // the mesh files are gone when runSolver returns, as in the reference
        FSolver *s;
        ~JoinRemovals() { s->join_removals(); }
    } join_at_exit{this};
    for (double &m : ms_phase) m = 0;
    auto t = std::chrono::steady_clock::now();
    // sharded (set_comm): every rank reads the same mesh files; they are
    // deleted by rank 0 once the collective solve has run (every rank has
    // read them by then)
    const bool delete_now = deleteMeshFiles && !comm;
    LoadMeshErr err = LoadMesh(delete_now);
    ms_phase[0] = ms_since(t);
    if (err != NOERROR) {
        warn(getErrorString(err));
        return false;
    }
    if (previousSolutionFile.empty()) {
        if (verbose) PrintMessage("renumbering nodes using Cuthill-McKee method\n");
        if (!Cuthill(delete_now)) {
            warn("problem renumbering node points\n");
            return false;
        }
    }
    ms_phase[1] = ms_since(t);
    if (!previousSolutionFile.empty()) {   // fsolver.cpp:1245-1320
        if (Frequency == 0 && PrevType != 0) {
            warn("Cannot handle incremental permeability problems with frequency 0.\n");
            return false;
        }
        if (Frequency != 0 && ProblemTypeV == AXISYMMETRIC) {
            warn("Cannot handle harmonic axisymmetric incremental problems.\n");
            return false;
        }
        if (Frequency != 0)
            warn("Harmonic planar incremental permeability problems are work in progress. RESULTS WON'T BE VALID!\n");
    }
    if (verbose) {
        PrintMessage("solving...\n");
        PrintMessage("Problem Statistics:\n%i nodes\n%i elements\nPrecision: %f\n", NumNodes, NumEls, Precision);
    }
    if (Frequency != 0) {   // Harmonic2D / HarmonicAxisymmetric, one .ans layout (fsolver.cpp:1312-1336)
        const bool solved = Harmonic2D();
        remove_mesh_files_after_collective_solve();
        if (!solved) {
            warn("Couldn't solve the problem\n");
            return false;
        }
        if (!writes_output()) return true;   // (sharded: rank 0 writes the .ans)
        if (verbose)
            PrintMessage(ProblemTypeV == AXISYMMETRIC ? "Harmonic axisymmetric problem solved\n"
                                                      : "Harmonic 2-D problem solved\n");
        t = std::chrono::steady_clock::now();
        if (!WriteHarmonic2D()) {
            warn("couldn't write results to disk\n");
            return false;
        }
        ms_phase[4] = ms_since(t);
        if (verbose) PrintMessage("results written to disk\n");
        return true;
    }
    const bool solved = Static2D();
    remove_mesh_files_after_collective_solve();
    if (!solved) {
        warn("Couldn't solve the problem\n");
        return false;
    }
    if (!writes_output()) return true;   // (sharded: rank 0 writes the .ans)
    if (verbose)
        PrintMessage(ProblemTypeV == AXISYMMETRIC ? "Static axisymmetric problem solved\n" : "Static 2-D problem solved\n");
    t = std::chrono::steady_clock::now();
    if (!WriteStatic2D()) {
        warn("couldn't write results to disk\n");
        return false;
    }
    ms_phase[4] = ms_since(t);
    if (verbose) PrintMessage("results written to disk\n");
    return true;
}

}  // namespace xfemm

