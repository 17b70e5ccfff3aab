/* xfemm_psolver.h -- C-ABI of the file-based scalar-potential solvers: ESolver
 * (electrostatics, .fee in, .res out) and HSolver (heat flow, .feh in, .anh
 * out), whose hot path runs on MI355X (include/xfemm_kernels.h:
 * xfk_electrostatic, xfk_heatflow).
 *
 * The surface mirrors xfemm_fsolver.h entry for entry; the reference's mains
 * (cfemm/esolver/main.cpp, cfemm/hsolver/main.cpp) drive it the same way:
 * create, set PathName, LoadProblemFile(), runSolver(verbose), return 1 / 2 on
 * failure.  The two solvers have the same functions under their own prefix:
 *
 *   xfemm_esolver_create / _destroy     ESolver                            esolver/esolver.cpp:79
 *   xfemm_esolver_load_problem_file     ESolver::LoadProblemFile()         esolver/esolver.cpp:109
 *   xfemm_esolver_run_solver            ESolver::runSolver(verbose)        esolver/esolver.cpp:648
 *   xfemm_hsolver_...                   HSolver, the same                  hsolver/hsolver.cpp:119, 854
 *
 * Boolean results follow the reference: 1 = success (true), 0 = failure.  No
 * C++ exception crosses this boundary.  Output: <PathName>.res / .anh in the
 * reference's WriteResults layout (esolver.cpp:720-790, hsolver.cpp:921-981).
 * Sharded solves are not offered (there is no set_comm).
 */
#ifndef XFEMM_PSOLVER_H
#define XFEMM_PSOLVER_H

#include "xfemm_fsolver.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct xfemm_esolver xfemm_esolver;
typedef struct xfemm_hsolver xfemm_hsolver;

/* ---- ESolver ---------------------------------------------------------- */
xfemm_esolver *xfemm_esolver_create(void);
void xfemm_esolver_destroy(xfemm_esolver *s);
void xfemm_esolver_set_message_handlers(xfemm_esolver *s, xfemm_message_fn warn, xfemm_message_fn print);
int xfemm_esolver_set_pathname(xfemm_esolver *s, const char *path_without_extension);
int xfemm_esolver_set_device(xfemm_esolver *s, int device);
int xfemm_esolver_set_delete_mesh_files(xfemm_esolver *s, int delete_files);
int xfemm_esolver_load_problem_file(xfemm_esolver *s);
int xfemm_esolver_run_solver(xfemm_esolver *s, int verbose);
/* Host-only steps of runSolver, for callers that drive them one by one:
 * ESolver::LoadMesh (esolver.cpp:127) and Cuthill (cuthill.cpp:88).  Nodes:
 * coordinates in the solver's unit (mm; HSolver: m), the point property and
 * the conductor of each node or -1.  Any output may be NULL. */
int xfemm_esolver_load_mesh(xfemm_esolver *s);
int xfemm_esolver_cuthill(xfemm_esolver *s);
int xfemm_esolver_get_nodes(xfemm_esolver *s, double *x, double *y, int *marker, int *conductor);
int xfemm_esolver_get_element_edges(xfemm_esolver *s, int *e);
int xfemm_esolver_get_pbcs(xfemm_esolver *s, int *pbc3);
int xfemm_esolver_num_pbcs(xfemm_esolver *s);
int xfemm_esolver_bandwidth(xfemm_esolver *s);
/* state after run_solver (renumbered order, as written to the .res):
 * get_solution gives x, y in the problem's length units, V and the Q mark of
 * every node; get_conductors the (V, q) of the conductor lines. */
int xfemm_esolver_num_nodes(xfemm_esolver *s);
int xfemm_esolver_num_elements(xfemm_esolver *s);
int xfemm_esolver_get_solution(xfemm_esolver *s, double *x, double *y, double *V, int *Q);
int xfemm_esolver_get_elements(xfemm_esolver *s, int *p, int *lbl);
int xfemm_esolver_num_conductors(xfemm_esolver *s);
int xfemm_esolver_get_conductors(xfemm_esolver *s, double *V, double *q);
int xfemm_esolver_get_stats(xfemm_esolver *s, xfk_result *out);
/* Wall milliseconds of the last runSolver, as xfemm_fsolver_get_times: ms[0]
 * LoadMesh, ms[1] Cuthill-McKee, ms[2] problem creation, ms[3] solve, ms[4]
 * the .res write. */
int xfemm_esolver_get_times(xfemm_esolver *s, double *ms);
const char *xfemm_esolver_last_error(xfemm_esolver *s);
/* The solved problem on the device (NULL before a successful run_solver),
 * owned by the solver and valid until its next run or its destruction:
 * xfk_pot_* post-processing works on it without reloading anything. */
xfk_problem *xfemm_esolver_problem(xfemm_esolver *s);
/* what LoadProblemFile read: out8 = Precision, Depth, LengthUnits,
 * ProblemType, extZo, extRo, extRi, dT; the sizes of the property lists */
int xfemm_esolver_get_header(xfemm_esolver *s, double *out8);
int xfemm_esolver_num_line_props(xfemm_esolver *s);
int xfemm_esolver_num_node_props(xfemm_esolver *s);
int xfemm_esolver_num_block_props(xfemm_esolver *s);
int xfemm_esolver_num_block_labels(xfemm_esolver *s);
/* property k of a list as doubles -- point: V, qp; line: BdryFormat, V, qs,
 * c0, c1, beta, h, Tinf; block: ex (Kx), ey (Ky), Kt, qv, TKPoints;
 * conductor: CircType, V, q; label: BlockType, IsExternal, IsDefault.
 * Returns the number of values, -1 on a bad index. */
int xfemm_esolver_get_point_prop(xfemm_esolver *s, int k, double *out2);
int xfemm_esolver_get_line_prop(xfemm_esolver *s, int k, double *out8);
int xfemm_esolver_get_block_prop(xfemm_esolver *s, int k, double *out5);
int xfemm_esolver_get_conductor_prop(xfemm_esolver *s, int k, double *out3);
int xfemm_esolver_get_block_label(xfemm_esolver *s, int k, double *out3);
/* the K(T) table of block k (heat flow); returns its length */
int xfemm_esolver_get_block_table(xfemm_esolver *s, int k, double *T, double *K);

/* ---- HSolver: the same, and the time step ------------------------------- */
xfemm_hsolver *xfemm_hsolver_create(void);
void xfemm_hsolver_destroy(xfemm_hsolver *s);
void xfemm_hsolver_set_message_handlers(xfemm_hsolver *s, xfemm_message_fn warn, xfemm_message_fn print);
int xfemm_hsolver_set_pathname(xfemm_hsolver *s, const char *path_without_extension);
int xfemm_hsolver_set_device(xfemm_hsolver *s, int device);
int xfemm_hsolver_set_delete_mesh_files(xfemm_hsolver *s, int delete_files);
int xfemm_hsolver_load_problem_file(xfemm_hsolver *s);
int xfemm_hsolver_run_solver(xfemm_hsolver *s, int verbose);
int xfemm_hsolver_load_mesh(xfemm_hsolver *s);
int xfemm_hsolver_cuthill(xfemm_hsolver *s);
int xfemm_hsolver_get_nodes(xfemm_hsolver *s, double *x, double *y, int *marker, int *conductor);
int xfemm_hsolver_get_element_edges(xfemm_hsolver *s, int *e);
int xfemm_hsolver_get_pbcs(xfemm_hsolver *s, int *pbc3);
int xfemm_hsolver_num_pbcs(xfemm_hsolver *s);
int xfemm_hsolver_bandwidth(xfemm_hsolver *s);
int xfemm_hsolver_num_nodes(xfemm_hsolver *s);
int xfemm_hsolver_num_elements(xfemm_hsolver *s);
int xfemm_hsolver_get_solution(xfemm_hsolver *s, double *x, double *y, double *T, int *Q);
int xfemm_hsolver_get_elements(xfemm_hsolver *s, int *p, int *lbl);
int xfemm_hsolver_num_conductors(xfemm_hsolver *s);
int xfemm_hsolver_get_conductors(xfemm_hsolver *s, double *T, double *q);
int xfemm_hsolver_get_stats(xfemm_hsolver *s, xfk_result *out);
int xfemm_hsolver_get_times(xfemm_hsolver *s, double *ms);
const char *xfemm_hsolver_last_error(xfemm_hsolver *s);
xfk_problem *xfemm_hsolver_problem(xfemm_hsolver *s);
int xfemm_hsolver_get_header(xfemm_hsolver *s, double *out8);
int xfemm_hsolver_num_line_props(xfemm_hsolver *s);
int xfemm_hsolver_num_node_props(xfemm_hsolver *s);
int xfemm_hsolver_num_block_props(xfemm_hsolver *s);
int xfemm_hsolver_num_block_labels(xfemm_hsolver *s);
int xfemm_hsolver_get_point_prop(xfemm_hsolver *s, int k, double *out2);
int xfemm_hsolver_get_line_prop(xfemm_hsolver *s, int k, double *out8);
int xfemm_hsolver_get_block_prop(xfemm_hsolver *s, int k, double *out5);
int xfemm_hsolver_get_conductor_prop(xfemm_hsolver *s, int k, double *out3);
int xfemm_hsolver_get_block_label(xfemm_hsolver *s, int k, double *out3);
int xfemm_hsolver_get_block_table(xfemm_hsolver *s, int k, double *T, double *K);
/* The previous time step's temperatures, one per node in the order of the
 * .node file (the solver renumbers them with the nodes), for a .feh with
 * [dT] != 0.  Time steps from a file are refused: with [dT] != 0, a non-empty
 * [PrevSoln] and no temperatures set here run_solver fails with a message
 * naming the file; with an empty [PrevSoln] and none set, dT is reset to 0
 * with the reference's warning (hsolver.cpp:129-137).  n == 0 clears them. */
int xfemm_hsolver_set_previous_solution(xfemm_hsolver *s, const double *T, int n);
const char *xfemm_hsolver_previous_solution_file(xfemm_hsolver *s);

#ifdef __cplusplus
}
#endif
#endif
