// ESolver and HSolver: the electrostatics and heat-flow solver objects of the
// reference (cfemm/esolver/esolver.h, cfemm/hsolver/hsolver.h), re-hosted over
// the MI355X kernels (include/xfemm_kernels.h: xfk_electrostatic, xfk_heatflow).
//
// A .fee / .feh with its mesh files goes in, a .res / .anh comes out:
//   PathName, LoadProblemFile(), LoadMesh(), Cuthill(), runSolver(verbose),
//   WriteResults(), WarnMessage / PrintMessage hooks.
// The two reference classes differ in their file names, units table, property
// tokens and the time step; PSolver holds both, told apart by its kind.  The
// mesh steps are MeshHost's, shared with FSolver.  The linear system never
// exists on the host.
#pragma once

#include <string>
#include <vector>

#include "meshhost.h"
#include "pot_problem.h"

namespace xfemm {

class PSolver : public PotProblemData, public MeshHost {
public:
    explicit PSolver(PotentialKind kind);
    ~PSolver();

    const PotentialKind kind;
    BigVec<CPNode> meshnode;      // (parallel first touch: hostmem.h)
    BigVec<CPElement> meshele;

    bool LoadProblemFile();                          // esolver.cpp:109-116, hsolver.cpp:119-125
    LoadMeshErr LoadMesh(bool deleteFiles = true);   // esolver.cpp:127-374, hsolver.cpp:187-431
    int Cuthill(bool deleteFiles = true);            // cuthill.cpp:88-390
    int SortElements();                              // cuthill.cpp:39-86
    bool runSolver(bool verbose = false);            // esolver.cpp:648-709, hsolver.cpp:854-916
    int WriteResults();                              // esolver.cpp:720-790, hsolver.cpp:921-981
    static std::string getErrorString(LoadMeshErr err);

    // Heat flow: the previous time step's solution, one value per node in the
    // order of the .node file (Cuthill carries it along with the nodes).  The
    // only way to a time step through this object: a [PrevSoln] file with
    // [dT] != 0 is refused.
    bool set_previous_solution(const double *T, int n);

    // user length units -> the solver's (mm / m): esolver.cpp:65, hsolver.cpp:65
    double unit() const;
    const char *input_ext() const { return kind == POT_HEATFLOW ? ".feh" : ".fee"; }
    const char *output_ext() const { return kind == POT_HEATFLOW ? ".anh" : ".res"; }

    // after a solve, in meshnode order: V (T), the marks the reference's L.Q
    // holds, and per conductor the .res / .anh line (V, q)
    std::vector<double> V;
    std::vector<int> Q;
    std::vector<double> condV, condq;
    // the solved problem on the device, kept until the next run or the
    // object's end: xfk_pot_* post-processing needs no reload
    xfk_problem *problem() const { return prob_; }

private:
    xfk_problem *prob_ = nullptr;
    std::vector<double> Tprev_;
    bool load_prev(bool &loaded);                    // hsolver.cpp:127-185
    bool solve_on_device();
    void drop_problem();
};

class ESolver : public PSolver {
public:
    ESolver() : PSolver(POT_ELECTROSTATIC) {}
};

class HSolver : public PSolver {
public:
    HSolver() : PSolver(POT_HEATFLOW) {}
};

}  // namespace xfemm
