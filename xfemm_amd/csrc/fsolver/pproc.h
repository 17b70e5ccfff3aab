// Solution files of the scalar-potential solvers on the host: the reader of a
// .res (electrostatics) / .anh (heat flow), and the host-side pieces of the
// reference's post-processors that work on the file's input geometry.
//
// A solution file is the .fee / .feh text, then [Solution] and, in this order
// (esolver.cpp:720-790, hsolver.cpp:921-981, what psolver.cpp writes):
//   the node count,      then that many lines  x y V Q   (T for heat flow)
//   the element count,   then that many lines  p0 p1 p2 lbl
//   the conductor count, then that many lines  V q
// Coordinates stay in the problem's length units, as the reference's
// post-processors hold them.  Nothing here touches the device: the file (and
// what uses it, tests/native/pproc_read_check.cpp) builds without the kernels.
#pragma once

#include <string>
#include <utility>
#include <vector>

#include "hostmem.h"
#include "pot_problem.h"

namespace xfemm {

struct SolutionFile : PotProblemData {
    PotGeometry geom;
    int NumNodes = 0, NumEls = 0;
    BigVec<double> x, y, V;    // per node; x, y in the problem's length units
    BigVec<int> Q;             // per node: the conductor, or -1 fixed, -2 free
    BigVec<int> p;             // 3 per element
    BigVec<int> lbl;           // per element
    std::vector<double> condV, condq;
    void clear();
};

// Reads `path` into `out`.  false with `err` naming the fault, and `out`
// cleared, on: a file that cannot be read, a header the .fee / .feh parser
// refuses, a missing [Solution], a count line that is no count, a section with
// fewer lines than its count says (a truncated file) or a line that is not of
// its section's form (a count that disagrees with the lines present), a node
// index outside the node range, a label beyond the label list, text after the
// conductor lines.  Large files are read by parallel pread and parsed by line
// chunks on the persistent host pool (meshhost_impl.h, fastnum.h).
bool ReadSolutionFile(const std::string &path, PotentialKind kind, SolutionFile &out, std::string &err);

// The contour of the reference's post-processors on the host
// (PostProcessor.cpp:167-298, 772-820), in the problem's length units.
struct ContourHost {
    std::vector<std::pair<double, double>> pts;
    void clear() { pts.clear(); }
    // addContourPoint: a point equal to the last is dropped
    void add(double x, double y);
    // addContourPointFromNode: the input point closest to (mx, my); when it
    // and the last contour point are the two ends of an arc segment (the one
    // closest to (mx, my) among such segments and arcs) the arc is followed in
    // ceil(ArcLength / MaxSideLength) steps; a step back onto the point before
    // the last ends the call
    void add_from_node(const PotGeometry &g, double mx, double my);
    // bendContour: the last segment becomes an arc of `angle` degrees in steps
    // of `step` degrees
    void bend(double angle, double step);
};

// The reference's point location (PostProcessor::InTriangle,
// PostProcessor.cpp:300-355, over InTriangleTest, 359-398): the search starts
// at the element found last and walks outwards from it in both directions,
// testing the elements whose circle about the centroid (epproc.cpp:106-120)
// holds the point.  At a point several elements hold -- a mesh node, an edge
// -- the answer therefore depends on the point looked up before; the
// reference's recorded outputs contain such points.  The device's search takes
// the lowest-numbered element instead; the single-point calls of the
// post-processors use this walk so that they answer as the reference does.
struct ElementWalk {
    std::vector<double> cx, cy, rsqr;
    int last = 0;
    void build(const SolutionFile &f);
    bool holds(const SolutionFile &f, double x, double y, int i) const;
    int find(const SolutionFile &f, double x, double y);   // -1: no element
};

// closestNode over the input points (-1: none)
int ClosestGeometryPoint(const PotGeometry &g, double x, double y);
// the label closest to (x, y) (-1: none)
int ClosestLabel(const PotProblemData &pr, double x, double y);

}  // namespace xfemm
