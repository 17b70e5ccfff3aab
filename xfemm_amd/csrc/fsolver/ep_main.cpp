// epproc <file.res> [out]: opens an electrostatic solution, selects block
// label 0 and prints the block integrals 0-6 and the point values at two
// points with field smoothing off and on -- the lines of the reference's
// recorded epproc/test/test.out.check.  Exit status 1 when the file does not
// open.
#include <cstdio>

#include "../../../include/xfemm_pproc.h"

int main(int argc, char **argv)
{
    if (argc < 2 || argc > 3) {
        std::fprintf(stderr, "usage: epproc <file.res> [out]\n");
        return 1;
    }
    xfemm_epproc *pp = xfemm_epproc_create();
    if (!pp || !xfemm_epproc_open_document(pp, argv[1])) {
        std::fprintf(stderr, "epproc: couldn't open %s\n", argv[1]);
        xfemm_epproc_destroy(pp);
        return 1;
    }
    FILE *o = argc == 3 ? std::fopen(argv[2], "wt") : stdout;
    if (!o) {
        std::fprintf(stderr, "epproc: couldn't write to %s\n", argv[2]);
        xfemm_epproc_destroy(pp);
        return 1;
    }
    int status = 0;
    xfemm_epproc_clear_selection(pp);
    xfemm_epproc_toggle_label(pp, 0);
    static const char *const scalar[] = {"Stored Energy Integral", "Block Cross-section Integral", "Block Volume Integral"};
    static const char *const pair[] = {"Average D Integral", "Average E Integral", "Weighted Stress Tensor Force Integral",
                                       "Weighted Stress Tensor Torque Integral"};
    static const char *const comp[][2] = {{"Fx", "Fy"}, {"Gx", "Gy"}, {"Gx", "Gy"}, {"Gx", "Gy"}};
    for (int type = 0; type < 7; ++type) {
        double v[2] = {0, 0};
        if (!xfemm_epproc_block_integral(pp, type, v)) status = 1;
        if (type < 3) std::fprintf(o, "%s for block 0 %f\n", scalar[type], v[0]);
        else std::fprintf(o, "%s for block 0 %s: %f, %s: %f\n", pair[type - 3], comp[type - 3][0], v[0], comp[type - 3][1], v[1]);
    }
    const double pts[2][2] = {{0.25, 0.0}, {0.1, 0.8}};
    for (int smooth = 0; smooth < 2; ++smooth) {
        xfemm_epproc_set_smoothing(pp, smooth);
        std::fprintf(o, "Field Smoothing %s\n", smooth ? "ON" : "OFF");
        for (const auto &p : pts) {
            double u[8];
            std::fprintf(o, "Point vals at x = %f, y = %f\n", p[0], p[1]);
            if (xfemm_epproc_get_point_values(pp, p[0], p[1], u))   // V, Dx, Dy, Ex, Ey, ex, ey, nrg
                std::fprintf(o, "Dx: %f\tDy: %f\tEx: %f\tEy: %f\tV: %f\tex: %f\tey: %f\t nrg: %f\n", u[1], u[2], u[3], u[4],
                             u[0], u[5], u[6], u[7]);
            else
                status = 1;
        }
    }
    if (o != stdout) std::fclose(o);
    xfemm_epproc_destroy(pp);
    return status;
}
