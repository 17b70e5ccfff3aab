// Problem description of an electrostatic .fee or a heat-flow .feh file, as the
// reference's ESolver / HSolver hold it after LoadProblemFile.
//
// One set of types for both kinds (the reference has a pair of each with the
// same shape): CSPointProp / CHPointProp (CPointProp.h), CSBoundaryProp /
// CHBoundaryProp (CBoundaryProp.h), CSMaterialProp / CHMaterialProp
// (CMaterialProp.h), CSCircuit / CHConductor (CCircuit.h), CSBlockLabel /
// CHBlockLabel (CBlockLabel.h), and the solvers' CNode / femmsolver::CElement.
// The parser restates FEASolver::LoadProblemFile (libfemm/feasolver.cpp) with
// the fromStream readers of those types (femm_problem.cpp).
#pragma once

#include <string>
#include <vector>

#include "femm_problem.h"

namespace xfemm {

enum PotentialKind { POT_ELECTROSTATIC = 0, POT_HEATFLOW = 1 };

struct CPPointProp {
    std::string PointName = "New Point Property";
    double V = 0;    // <Vp> / <Tp>
    double qp = 0;
};

struct CPBoundaryProp {
    std::string BdryName = "New Boundary";
    int BdryFormat = 0;
    double V = 0;    // <Vs> / <Tset>
    double qs = 0;
    double c0 = 0, c1 = 0;              // electrostatics
    double beta = 0, h = 0, Tinf = 0;   // heat flow
};

struct CPMaterialProp {
    std::string BlockName = "New Material";
    double kx = 1, ky = 1;   // <ex> <ey> / <Kx> <Ky>
    double Kt = 0;           // heat flow
    double qv = 0;
    std::vector<double> T, K;   // <TKPoints>
};

struct CPConductor {
    std::string CircName = "New Circuit";
    int CircType = 0;
    double V = 0;    // <Vc> / <Tc>
    double q = 0;
};

struct CPBlockLabel {
    double x = 0, y = 0;
    int BlockType = -1;
    double MaxArea = 0;
    int InGroup = 0;
    bool IsDefault = false, IsExternal = false;
};

struct CPNode {
    double x = 0, y = 0;     // mm (electrostatics) or m (heat flow) after LoadMesh
    int BoundaryMarker = -1;
    int InConductor = -1;
};

struct CPElement {
    int p[3] = {0, 0, 0};
    int e[3] = {-1, -1, -1};
    int blk = 0, lbl = 0;
};

struct PotProblemData {
    double FileFormat = -1;
    double Precision = 1.e-08;
    double MinAngle = 0.;
    double Depth = -1;
    LengthUnit LengthUnits = LengthInches;
    CoordsType Coords = CART;
    ProblemType ProblemTypeV = PLANAR;
    double extZo = 0, extRo = 0, extRi = 0;
    double dT = 0;                       // heat flow: [dT]
    std::string previousSolutionFile;    // heat flow: [PrevSoln]
    std::string comment;
    std::vector<CPPointProp> nodeproplist;
    std::vector<CPBoundaryProp> lineproplist;
    std::vector<CPMaterialProp> blockproplist;
    std::vector<CPConductor> circproplist;
    std::vector<CPBlockLabel> labellist;
};

// The input geometry of a .fee / .feh, which the solvers skip and the
// post-processors keep (contours along input segments and arcs): the lines
// under [NumPoints], [NumSegments], [NumArcSegments] and [NumHoles].  Indices
// are 0-based; `prop` is the file's 1-based property number less one (-1:
// none), `cond` likewise.
struct PotGeometry {
    struct Point {
        double x = 0, y = 0;
        int prop = -1, group = 0, cond = -1;
    };
    struct Segment {
        int n0 = 0, n1 = 0;
        double MaxSideLength = -1;
        int prop = -1, hidden = 0, group = 0, cond = -1;
    };
    struct Arc {
        int n0 = 0, n1 = 0;
        double ArcLength = 90, MaxSideLength = 10;   // degrees
        int prop = -1, hidden = 0, group = 0, cond = -1;
    };
    struct Hole {
        double x = 0, y = 0;
        int group = 0;
    };
    std::vector<Point> points;
    std::vector<Segment> segments;
    std::vector<Arc> arcs;
    std::vector<Hole> holes;
};

// FEASolver::LoadProblemFile on a .fee / .feh: returns false and fills `err`
// on a parse error.
bool ParsePotentialFile(const std::string &path, PotentialKind kind, PotProblemData &out, std::string &err);
// The same on text already in memory (the header a .res / .anh echoes before
// its [Solution]); `path` only names the file in messages.  geom (may be
// null) receives the geometry lists.
bool ParsePotentialText(const char *text, size_t len, const std::string &path, PotentialKind kind, PotProblemData &out,
                        PotGeometry *geom, std::string &err);

}  // namespace xfemm
