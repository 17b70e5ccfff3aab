// MeshHost: what the three file-based solvers (FSolver, ESolver, HSolver) share
// on the host, as the reference's FEASolver (libfemm/feasolver.h, cuthill.cpp)
// does for its own: the parallel readers of the .node / .ele / .edge files,
// Cuthill-McKee and SortElements (host and device comb sort), the removal of
// mesh files, the move-aside of an old output and the parallel line formatter.
//
// The node and element types are the solver's own, so the mesh steps are
// member templates (meshhost_impl.h) over them: a node has x, y; an element
// has p[3], lbl.
#pragma once

#include <array>
#include <string>
#include <thread>
#include <vector>

#include "../../../include/xfemm_kernels.h"
#include "femm_problem.h"
#include "hostmem.h"

namespace xfemm {

enum LoadMeshErr { NOERROR, BADFEMFILE, BADNODEFILE, BADPBCFILE, BADELEMENTFILE, BADEDGEFILE, MISSINGMATPROPS,
                   ELMLABELTOOBIG, UNSUPPORTEDMESH };

int PrintWarningMsg(const char *fmt, ...);

namespace meshio {
struct TextBuf;
}

class MeshHost {
public:
    MeshHost();
    ~MeshHost();
    MeshHost(const MeshHost &) = delete;
    MeshHost &operator=(const MeshHost &) = delete;

    // General problem attributes (feasolver.h)
    std::string PathName;
    int NumNodes = 0, NumEls = 0, BandWidth = 0, NumPBCs = 0;
    std::vector<CCommonPoint> pbclist;

    int (*WarnMessage)(const char *, ...);
    int (*PrintMessage)(const char *, ...);

    // GPU selection and file handling
    int device = 0;
    bool deleteMeshFiles = true;

    void join_removals();   // wait for the mesh-file deletions LoadMesh / Cuthill started
    // output text formatted in parallel chunks (meshhost_impl.h: format_lines)
    struct Formatted {
        std::vector<HugeBuf<char>> buf;
        std::vector<size_t> len;
        // every chunk's buffer was allocated (a failed chunk is left empty)
        bool ok() const
        {
            for (const auto &b : buf)
                if (!b.data()) return false;
            return true;
        }
    };

    xfk_result stats{};
    // wall milliseconds of the last runSolver: LoadMesh, Cuthill, problem
    // creation (descriptor + host -> HBM upload), solve (device + solution
    // read-back), write (the output file)
    double ms_phase[5] = {};
    std::string lastError;

protected:
    BigVec<std::array<int, 3>> edges_;        // .edge content: n0, n1, marker
    std::vector<std::thread> removers_;       // mesh-file deletions in flight (joined by runSolver)
    void remove_async(std::vector<std::string> paths);
    // HIP runtime / device / code-object bring-up (xfk_device_init) started by
    // LoadProblemFile on a thread of its own, so a fresh process pays it beside
    // LoadMesh and Cuthill instead of inside the first device call; joined
    // before the first device use
    std::thread hip_warm_;
    void start_hip_warmup();
    void join_hip_warmup();
    void clear_old_output(const std::string &path);
    void warn(const std::string &msg);

    // the .node file: NumNodes and node(i) = decode(x, y, marker) per record
    template <class Node, class Decode>
    bool read_node_file(meshio::TextBuf &tb, BigVec<Node> &meshnode, Decode decode);
    // the .ele file: NumEls and p[3], lbl (1-based, as in the file) per record
    template <class Elem>
    bool read_element_file(meshio::TextBuf &tb, BigVec<Elem> &meshele);
    // labels and node ids checked per element, in parallel: lbl made 0-based,
    // the default label applied, blk looked up.  code 0: fine; else the first
    // failing element (in file order): 1 no label, 2 label too big, 3 bad node id
    struct ElementCheck {
        int code = 0, index = -1;
    };
    template <class Elem, class BlockOf>
    ElementCheck check_elements(BigVec<Elem> &meshele, int n_labels, int defaultLabel, BlockOf blockOf);
    // the .edge file into edges_, node ids checked; marked: the edges with a
    // negative marker, in file order
    bool read_edge_file(meshio::TextBuf &tb, std::vector<int> &marked);

    // cuthill.cpp:88-390 on edges_; renumbered(newnum) runs after pbclist is
    // renumbered (for what else a solver keeps by node id)
    template <class Node, class Elem, class Hook>
    int cuthill_mesh(BigVec<Node> &meshnode, BigVec<Elem> &meshele, bool deleteFiles, Hook renumbered);
    // cuthill.cpp:39-86
    template <class Elem>
    int sort_mesh_elements(BigVec<Elem> &meshele);
    template <class Elem, class Src>
    bool permute_elements(BigVec<Elem> &meshele, Src src);
    // the comb sort's permutation of n elements by score (device, or host)
    bool sort_permutation(const unsigned *score, int n, int *perm);
};

}  // namespace xfemm
