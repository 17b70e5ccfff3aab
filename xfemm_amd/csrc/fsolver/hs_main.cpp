// hsolver command line: same usage as the reference (cfemm/hsolver/main.cpp):
//   hsolver <problem path without .feh>     -> writes <problem>.anh
// Options (this build): --device N, --keep-mesh (do not delete mesh files).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "psolver.h"

int main(int argc, char **argv)
{
    xfemm::HSolver theHSolver;
    std::string path;
    for (int i = 1; i < argc; i++) {
        if (!strcmp(argv[i], "--device") && i + 1 < argc) theHSolver.device = atoi(argv[++i]);
        else if (!strcmp(argv[i], "--keep-mesh")) theHSolver.deleteMeshFiles = false;
        else if (path.empty()) path = argv[i];
        else {
            printf("Too many arguments");
            return 1;
        }
    }
    if (path.empty()) {
        char buf[512];
        printf("Enter feh file name without extension:\n");
        if (!fgets(buf, sizeof buf, stdin)) return 1;
        char *pos = strchr(buf, '\n');
        if (pos) *pos = '\0';
        path = buf;
    }
    if (path.size() > 4 && path.compare(path.size() - 4, 4, ".feh") == 0) path.resize(path.size() - 4);
    theHSolver.PathName = path;
    if (!theHSolver.LoadProblemFile()) {
        theHSolver.WarnMessage("problem loading .feh file");
        return 1;
    }
    if (!theHSolver.runSolver(true)) return 2;
    return 0;
}
