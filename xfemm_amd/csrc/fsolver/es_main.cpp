// esolver command line: same usage as the reference (cfemm/esolver/main.cpp):
//   esolver <problem path without .fee>     -> writes <problem>.res
// Options (this build): --device N, --keep-mesh (do not delete mesh files).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "psolver.h"

int main(int argc, char **argv)
{
    xfemm::ESolver solverInstance;
    std::string path;
    for (int i = 1; i < argc; i++) {
        if (!strcmp(argv[i], "--device") && i + 1 < argc) solverInstance.device = atoi(argv[++i]);
        else if (!strcmp(argv[i], "--keep-mesh")) solverInstance.deleteMeshFiles = false;
        else if (path.empty()) path = argv[i];
        else {
            printf("Too many arguments");
            return 1;
        }
    }
    if (path.empty()) {
        char buf[512];
        printf("Enter fee file name without extension:\n");
        if (!fgets(buf, sizeof buf, stdin)) return 1;
        char *pos = strchr(buf, '\n');
        if (pos) *pos = '\0';
        path = buf;
    }
    if (path.size() > 4 && path.compare(path.size() - 4, 4, ".fee") == 0) path.resize(path.size() - 4);
    solverInstance.PathName = path;
    if (!solverInstance.LoadProblemFile()) {
        solverInstance.WarnMessage("problem loading .fee file");
        return 1;
    }
    if (!solverInstance.runSolver(true)) return 2;
    return 0;
}
