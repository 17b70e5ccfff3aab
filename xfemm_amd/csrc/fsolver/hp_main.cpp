// hpproc <file.anh> [out]: opens a heat-flow solution, selects block label 0
// and prints the block integrals 0-4 and the point values at two points with
// field smoothing off and on -- the lines of the reference's recorded
// hpproc/test/Temp0.out.check.  Exit status 1 when the file does not open.
#include <cstdio>

#include "../../../include/xfemm_pproc.h"

int main(int argc, char **argv)
{
    if (argc < 2 || argc > 3) {
        std::fprintf(stderr, "usage: hpproc <file.anh> [out]\n");
        return 1;
    }
    xfemm_hpproc *pp = xfemm_hpproc_create();
    if (!pp || !xfemm_hpproc_open_document(pp, argv[1])) {
        std::fprintf(stderr, "hpproc: couldn't open %s\n", argv[1]);
        xfemm_hpproc_destroy(pp);
        return 1;
    }
    FILE *o = argc == 3 ? std::fopen(argv[2], "wt") : stdout;
    if (!o) {
        std::fprintf(stderr, "hpproc: couldn't write to %s\n", argv[2]);
        xfemm_hpproc_destroy(pp);
        return 1;
    }
    int status = 0;
    xfemm_hpproc_clear_selection(pp);
    xfemm_hpproc_toggle_label(pp, 0);
    static const char *const scalar[] = {"Block Temperature Integral", "Block Cross-section Area Integral",
                                         "Block Volume Integral"};
    static const char *const pair[] = {"Block Average F Integral", "Block Average G Integral"};
    static const char *const comp[][2] = {{"Fx", "Fy"}, {"Gx", "Gy"}};
    for (int type = 0; type < 5; ++type) {
        double v[2] = {0, 0};
        if (!xfemm_hpproc_block_integral(pp, type, v)) status = 1;
        if (type < 3) std::fprintf(o, "%s for block 0 %f\n", scalar[type], v[0]);
        else std::fprintf(o, "%s for block 0 %s: %f, %s: %f\n", pair[type - 3], comp[type - 3][0], v[0], comp[type - 3][1], v[1]);
    }
    const double pts[2][2] = {{0.01, 0.01}, {0.005, 0.005}};
    for (int smooth = 0; smooth < 2; ++smooth) {
        xfemm_hpproc_set_smoothing(pp, smooth);
        std::fprintf(o, "Field Smoothing %s\n", smooth ? "ON" : "OFF");
        for (const auto &p : pts) {
            double u[8];
            std::fprintf(o, "Point vals at x = %f, y = %f\n", p[0], p[1]);
            if (xfemm_hpproc_get_point_values(pp, p[0], p[1], u))   // T, Fx, Fy, Kx, Ky, Gx, Gy
                std::fprintf(o, "T: %f\tFx: %f\tFy: %f\tKx: %f\tKy: %f\tGx: %f\tGy: %f\n", u[0], u[1], u[2], u[3], u[4], u[5],
                             u[6]);
            else
                status = 1;
        }
    }
    if (o != stdout) std::fclose(o);
    xfemm_hpproc_destroy(pp);
    return status;
}
