/* xfemm_pproc.h -- C-ABI of the file-based post-processors: EPProc
 * (electrostatics, a .res) and HPProc (heat flow, an .anh), whose fields,
 * integrals and point values are computed on MI355X
 * (include/xfemm_kernels.h: xfk_pot_*).
 *
 * The surface is shaped like xfemm_psolver.h and follows the reference's
 * PostProcessor (libfemm/PostProcessor.h, epproc/epproc.h, hpproc/hpproc.h);
 * the two have the same functions under their own prefix.  Boolean results
 * follow the reference: 1 = success, 0 = failure, the reason in last_error.
 * No C++ exception crosses this boundary.  Lengths are the problem's length
 * units.  A time step from a [PrevSoln] file, fpproc and femmcli's eo_ / ho_
 * commands are not offered.
 */
#ifndef XFEMM_PPROC_H
#define XFEMM_PPROC_H

#include "xfemm_fsolver.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct xfemm_epproc xfemm_epproc;
typedef struct xfemm_hpproc xfemm_hpproc;

#define XFEMM_PPROC_API(NAME)                                                                                          \
    xfemm_##NAME *xfemm_##NAME##_create(void);                                                                         \
    void xfemm_##NAME##_destroy(xfemm_##NAME *s);                                                                      \
    int xfemm_##NAME##_set_device(xfemm_##NAME *s, int device);                                                        \
    void xfemm_##NAME##_set_message_handlers(xfemm_##NAME *s, xfemm_message_fn warn, xfemm_message_fn print);          \
    /* the host-only step: the file into memory, nothing on the device */                                              \
    int xfemm_##NAME##_read(xfemm_##NAME *s, const char *path);                                                        \
    int xfemm_##NAME##_num_nodes(xfemm_##NAME *s);                                                                     \
    int xfemm_##NAME##_num_elements(xfemm_##NAME *s);                                                                  \
    int xfemm_##NAME##_num_conductors(xfemm_##NAME *s);                                                                \
    /* x, y in the problem's length units, the potential, the Q mark; any may be NULL */                               \
    int xfemm_##NAME##_get_nodes(xfemm_##NAME *s, double *x, double *y, double *V, int *Q);                            \
    int xfemm_##NAME##_get_elements(xfemm_##NAME *s, int *p, int *lbl);                                                \
    /* the conductor lines of the file: V (T), q */                                                                    \
    int xfemm_##NAME##_get_conductors(xfemm_##NAME *s, double *V, double *q);                                          \
    /* out8 = Precision, Depth, LengthUnits, ProblemType, extZo, extRo, extRi, dT */                                   \
    int xfemm_##NAME##_get_header(xfemm_##NAME *s, double *out8);                                                      \
    int xfemm_##NAME##_num_line_props(xfemm_##NAME *s);                                                                \
    int xfemm_##NAME##_num_node_props(xfemm_##NAME *s);                                                                \
    int xfemm_##NAME##_num_block_props(xfemm_##NAME *s);                                                               \
    int xfemm_##NAME##_num_block_labels(xfemm_##NAME *s);                                                              \
    /* label k: x, y, BlockType, InGroup, IsExternal, IsDefault; returns 6, -1 on a bad index */                       \
    int xfemm_##NAME##_get_block_label(xfemm_##NAME *s, int k, double *out6);                                          \
    /* block k: ex (Kx), ey (Ky), Kt, qv, TKPoints; returns 5 */                                                       \
    int xfemm_##NAME##_get_block_prop(xfemm_##NAME *s, int k, double *out5);                                           \
    /* the input geometry: out4 = the numbers of points, segments, arc segments, holes */                              \
    int xfemm_##NAME##_geometry_counts(xfemm_##NAME *s, int *out4);                                                    \
    int xfemm_##NAME##_get_geometry_points(xfemm_##NAME *s, double *x, double *y, int *group);                         \
    int xfemm_##NAME##_get_geometry_segments(xfemm_##NAME *s, int *n01, int *group);                                   \
    /* arcs: n0, n1 per arc; ArcLength, MaxSideLength (degrees) per arc */                                             \
    int xfemm_##NAME##_get_geometry_arcs(xfemm_##NAME *s, int *n01, double *length_maxside, int *group);               \
    /* OpenDocument: read, then the problem on the device with the file's                                             \
     * solution and Q marks loaded, the multiply-defined-label check made */                                           \
    int xfemm_##NAME##_open_document(xfemm_##NAME *s, const char *path);                                               \
    /* the selection of block labels */                                                                                \
    int xfemm_##NAME##_clear_selection(xfemm_##NAME *s);                                                               \
    int xfemm_##NAME##_select_block_label(xfemm_##NAME *s, double x, double y); /* toggles the closest label */        \
    int xfemm_##NAME##_toggle_label(xfemm_##NAME *s, int k);                                                           \
    int xfemm_##NAME##_toggle_group(xfemm_##NAME *s, int group);                                                       \
    int xfemm_##NAME##_get_selection(xfemm_##NAME *s, unsigned char *selected);                                        \
    int xfemm_##NAME##_set_smoothing(xfemm_##NAME *s, int on);                                                         \
    /* blockIntegral(type) over the selection, types 0-4 summed element by element as the reference sums;             \
     * types 5 and 6 (EPProc) make the mask first */                                                                   \
    int xfemm_##NAME##_block_integral(xfemm_##NAME *s, int type, double *out2);                                        \
    /* getPointValues: 8 doubles as xfk_pot_point_values orders them; 0 when no element holds the point.              \
     * The element is found as the reference finds it, walking from the element of the point looked up                \
     * before; the batched form takes the lowest-numbered containing element of every point */                         \
    int xfemm_##NAME##_get_point_values(xfemm_##NAME *s, double x, double y, double *out8);                            \
    int xfemm_##NAME##_get_point_values_batch(xfemm_##NAME *s, int n, const double *x, const double *y, int *elem,     \
                                               double *out);                                                           \
    /* the contour */                                                                                                  \
    int xfemm_##NAME##_add_contour_point(xfemm_##NAME *s, double x, double y);                                         \
    int xfemm_##NAME##_add_contour_point_from_node(xfemm_##NAME *s, double x, double y);                               \
    int xfemm_##NAME##_bend_contour(xfemm_##NAME *s, double angle, double step);                                       \
    int xfemm_##NAME##_clear_contour(xfemm_##NAME *s);                                                                 \
    int xfemm_##NAME##_num_contour_points(xfemm_##NAME *s);                                                            \
    int xfemm_##NAME##_get_contour(xfemm_##NAME *s, double *x, double *y);                                             \
    int xfemm_##NAME##_line_integral(xfemm_##NAME *s, int type, double *out2);                                         \
    /* d_PlotBounds: min, max of the potential, of |D| (|F|) and of |E| (|G|) */                                       \
    int xfemm_##NAME##_plot_bounds(xfemm_##NAME *s, double *out6);                                                     \
    /* 1 when a label's position lies in an element of another label; those elements' labels start selected */        \
    int xfemm_##NAME##_has_multiply_defined_labels(xfemm_##NAME *s);                                                   \
    /* the live problem (NULL before open_document), owned by the post-processor */                                    \
    xfk_problem *xfemm_##NAME##_problem(xfemm_##NAME *s);                                                              \
    const char *xfemm_##NAME##_last_error(xfemm_##NAME *s);

XFEMM_PPROC_API(epproc)
XFEMM_PPROC_API(hpproc)

#ifdef __cplusplus
}
#endif
#endif
