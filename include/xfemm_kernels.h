/* xfemm_kernels.h -- C-ABI of the MI355X (gfx950) fsolver hot path.
 *
 * Thin boundary between the C++ host side (FSolver, include/xfemm_fsolver.h)
 * and the hand-written HIP kernels: plain pointers and sizes, no C++ or torch
 * types.  One xfk_problem holds one static-2D magnetostatic problem resident
 * in HBM; xfk_static2d() runs the whole reference Static2D on the GPU:
 * element assembly into CSR, point/segment/(anti)periodic boundary conditions,
 * the preconditioned conjugate-gradient solve and the nonlinear B-H Newton loop.
 *
 * Reference interfaces replaced (temudschin/xfemm @ 2025-02-04):
 *   xfk_static2d          FSolver::Static2D(CBigLinProb&)   cfemm/fsolver/static2d.cpp:53
 *                         (called from FSolver::runSolver   cfemm/fsolver/fsolver.cpp:1266)
 *   xfk_pcg_solve         CBigLinProb::PCGSolve(int flag)   cfemm/libfemm/spars.cpp:238
 *   xfk_csr_*             CBigLinProb::MultA / Dot          cfemm/libfemm/spars.cpp:167,187
 *   xfk_problem_create    the state FSolver::LoadMesh + LoadProblemFile leave behind
 *                         (meshnode, meshele, the prop lists)      cfemm/fsolver/fsolver.cpp:202,350
 *
 * All functions return XFK_OK (0) or a negative error code; xfk_last_error()
 * gives the message of the last failure on the calling thread.  There is no
 * CPU fallback: without a usable gfx950 device every call fails.
 */
#ifndef XFEMM_KERNELS_H
#define XFEMM_KERNELS_H

#ifdef __cplusplus
extern "C" {
#endif

enum {
    XFK_OK = 0,
    XFK_ERR_ARG = -1,
    XFK_ERR_HIP = -2,
    XFK_ERR_SINGULAR = -3,      /* zero diagonal: "singular flag tripped" (spars.cpp:245) */
    XFK_ERR_NOCONV = -4,        /* iteration cap reached */
    XFK_ERR_UNSUPPORTED = -5
};

/* CMSolverMaterialProp after GetSlopes(0) (CMaterialProp.h:193). */
typedef struct {
    double mu_x, mu_y;          /* relative permeability */
    double H_c;                 /* coercivity, A/m */
    double J_re;                /* applied current density, MA/m^2 */
    double Cduct;               /* conductivity, MS/m */
    double LamFill;
    int LamType;
    int BHpoints;               /* 0 = linear */
    const double *B;            /* BHpoints: processed B-H curve (T) */
    const double *H;            /* BHpoints: A/m (real parts) */
    const double *slope;        /* BHpoints: dH/dB at the knots */
} xfk_block_desc;

/* CMBlockLabel (CBlockLabel.h:153) after FSolver::GetFillFactor. */
typedef struct {
    int block;                  /* index into blocks */
    int in_circuit;             /* -1 = none */
    double mag_dir;             /* magnetisation direction, degrees */
    int is_wound;
    int is_external;            /* axisymmetric: conformally mapped exterior region ([IsExternal]) */
    const char *mag_dir_fctn;   /* MagDirFctn: Lua expression of the element centroid (x y r z theta R)
                                   giving the direction per element (static2d.cpp:511-581,
                                   staticaxi.cpp:354-404); NULL or "" = the constant mag_dir.
                                   Static problems only, as in the reference. */
} xfk_label_desc;

/* CMBoundaryProp (CBoundaryProp.h). */
typedef struct {
    int format;                 /* BdryFormat: 0 prescribed A, 2 mixed, 4 periodic, 5 antiperiodic */
    double A0, A1, A2, phi;
    double c0, c1;
} xfk_line_desc;

/* CMPointProp (CPointProp.h). */
typedef struct {
    double A_re, A_im, J_re, J_im;
} xfk_point_desc;

/* CMCircuit (CCircuit.h) after FSolver::LoadProblemFile's serial expansion. */
typedef struct {
    int type;                   /* 0 parallel/voltage, 1 not expected here */
    double amps_re;
    double dvolts_re;
} xfk_circuit_desc;

/* CAirGapElement (cfemm/libfemm/CAirGapElement.h) as FSolver::LoadMesh reads it
 * from the .pbc file (fsolver.cpp:425-515): an unmeshed annulus between two
 * rings of equally spaced boundary nodes, coupled by totalArcElements
 * "air-gap elements" (static2d.cpp:191-344, harmonic2d.cpp:227-380). */
typedef struct {
    int format;                 /* BdryFormat: 0 periodic, 1 antiperiodic copies */
    double ri, ro;              /* inner / outer radius */
    double total_arc_length;    /* degrees spanned by the AGE */
    double inner_shift, outer_shift;   /* InnerShift / OuterShift, in arc elements */
    int n_arc;                  /* totalArcElements */
    const int *qn;              /* 4 * (n_arc + 1): quadNode[k].n0 n1 n2 n3 */
    const double *qw;           /* 4 * (n_arc + 1): quadNode[k].w0 w1 w2 w3 */
} xfk_age_desc;

typedef struct {
    int n_nodes;
    const double *x, *y;        /* node coordinates, cm */
    const int *marker;          /* point-prop index or -1 (may be NULL) */
    int n_elems;
    const int *p;               /* 3 per element */
    const int *e;               /* 3 per element: boundary-prop index or -1 (may be NULL) */
    const int *lbl;             /* block label of each element */
    int n_blocks;  const xfk_block_desc *blocks;
    int n_labels;  const xfk_label_desc *labels;
    int n_lines;   const xfk_line_desc *lines;
    int n_points;  const xfk_point_desc *points;
    int n_circs;   const xfk_circuit_desc *circs;
    int n_pbc;     const int *pbc;      /* 3 per pair: node, node, type (0 periodic, 1 anti) */
    double precision;           /* [Precision] */
    int length_units;           /* femm::LengthUnit */
    int coords;                 /* 0 cartesian, 1 polar */
    double relax;               /* FSolver::Relax, 1.0 */
    int problem_type;           /* [ProblemType]: XFK_PLANAR (Static2D) or XFK_AXISYMMETRIC
                                   (FSolver::StaticAxisymmetric, staticaxi.cpp:45-794: x is r, y is z) */
    double ext_zo, ext_ro, ext_ri;   /* [extZo] [extRo] [extRi]: axisymmetric exterior region, user units */
    int n_ages;  const xfk_age_desc *ages;   /* air-gap elements (planar; ignored when axisymmetric,
                                                as StaticAxisymmetric / HarmonicAxisymmetric do) */
} xfk_problem_desc;

enum { XFK_PLANAR = 0, XFK_AXISYMMETRIC = 1 };

typedef struct {
    int newton_iters;           /* linear solves performed */
    long long cg_iters;         /* total PCG iterations */
    double last_res;            /* last nonlinear residual */
    double final_er;            /* last PCG preconditioned residual ratio */
    long long nnz;              /* CSR nonzeros (full symmetric storage) */
    int ncolors;                /* element colours of the assembly scatter */
    double ms_symbolic;         /* device time, ms */
    double ms_assemble;
    double ms_solve;
    double spmv_ms_avg;         /* XFK_TIME_SPMV: mean HIP-event time of one SpMV launch */
    int spmv_samples;           /* launches sampled (every 16th PCG iteration) */
    int color_rounds;           /* Jones-Plassmann rounds of the element colouring */
    int precond;                /* preconditioner of the last solve (XFK_PRECOND_*) */
    int amg_levels;             /* AMG: levels of the last hierarchy */
    double amg_op_complexity;   /* AMG: sum of level nonzeros / fine nonzeros */
    double ms_amg_setup;        /* AMG: device time of the hierarchy setups, ms (inside ms_solve) */
    /* sharded solves with XFK_TIME_TAIL: device time of the replicated coarse
     * levels (every rank builds and applies them): the V-cycles' all-gather of
     * the coarse right-hand side + the replicated cycle, summed over the solve,
     * and the setup's build of the replicated levels */
    double ms_rep_cycle;
    int rep_cycles;             /* V-cycles timed */
    double ms_rep_setup;
    int prec_fallback;          /* 1: a stagnating PCG switched the AMG's f32 parts (level-0 transfers,
                                   coarsest inverse) to f64 and restarted; kept for the problem's life */
} xfk_result;

typedef struct xfk_problem xfk_problem;

const char *xfk_last_error(void);
int xfk_device_count(void);
/* Bring up the HIP runtime on `device` ahead of the first solve: the runtime
 * and the device context (~0.4 s in a fresh process), every code object of
 * this library, and a few streams for the process's stream pool.  Idempotent
 * and thread-safe; the FSolver runs it on a thread of its own beside
 * LoadMesh / Cuthill, so a fresh `fsolver` process does not wait for it in
 * series.  XFK_OK, or XFK_ERR_HIP when there is no such device. */
int xfk_device_init(int device);

/* Upload a problem; nothing is computed yet.  Host arrays may be freed after. */
int xfk_problem_create(const xfk_problem_desc *desc, int device, xfk_problem **out);
void xfk_problem_destroy(xfk_problem *prob);

enum { XFK_REBUILD_SYMBOLIC = 1, XFK_TIME_SPMV = 2, XFK_TIME_TAIL = 4 };

/* Solver options.  The reference preconditions its PCG with a sequential
 * SSOR sweep (spars.cpp:186-236, CBigLinProb::MultPC); the device offers
 *   XFK_PRECOND_AMG    smoothed-aggregation AMG V-cycle (default; rebuilt for
 *                      every matrix the Newton loop assembles; sharded solves
 *                      use it as a rank-local block preconditioner)
 *   XFK_PRECOND_JACOBI diag(A)
 * Both keep the reference's stopping test sqrt(z.r / z0.b) <= Precision.
 * A hierarchy whose SpGEMM rows overflow the LDS tables falls back to Jacobi
 * for that solve (xfk_result.precond tells which one ran). */
enum { XFK_PRECOND_JACOBI = 0, XFK_PRECOND_AMG = 1 };
enum {
    XFK_OPT_PRECOND = 1,        /* XFK_PRECOND_* */
    XFK_OPT_AMG_SWEEPS = 2,     /* Jacobi sweeps before and after the coarse correction (1..8, default 1) */
    XFK_OPT_AMG_THETA = 3,      /* strength threshold (0..1, default 0.08) */
    XFK_OPT_AMG_OMEGA = 4,      /* Jacobi weight factor: weight = omega / rho(D^-1 A) (0..2, default 1.75) */
    XFK_OPT_AMG_REPLICATE = 5,  /* sharded solve: coarse levels of at most this many global rows are
                                   replicated on every rank, larger ones stay sharded (default 250000) */
    XFK_OPT_AMG_REUSE = 6,      /* 1 (default): later Newton iterations of one solve keep the hierarchy
                                   and refresh only the fine-level smoother, rebuilt when the PCG needs
                                   2x the iterations of the last fresh build; 0: rebuild every time */
    XFK_OPT_AMG_DENSE = 7,      /* coarsening stops at a level of at most this many rows, which is
                                   solved by its dense inverse (16..2048, default 2048) */
    XFK_OPT_AMG_FOLD = 8,       /* 1 (default): V(1,1) levels
                                   run folded (one pass over P~ = (I - w D^-1 A) P for prolongation +
                                   post-sweep, coarse pre-steps with R~ = P~^T); 0: the plain cycle */
    XFK_OPT_AMG_COL16 = 9,      /* 1 (default): single-device level-0
                                   operators (the PCG SpMV, the sweeps, P~, R) read 16-bit column
                                   offsets per row tile (tiles spanning > 65535 columns read the int
                                   columns); 0: int columns.  The same column indices: the same bits. */
    XFK_OPT_AMG_WLEVEL = 10,    /* the folded coarse level that runs a W-cycle (two coarse
                                   corrections); -2 (default): the level above the last V-cycle
                                   level, -1: a plain V-cycle */
    XFK_OPT_AMG_F32 = 11,       /* 1 (default; needs 16-bit columns):
                                   the V-cycle's level-0 transfers (R, P~) store f32 values,
                                   products and sums in f64; 0: f64 values.  The sweeps and the
                                   PCG's own SpMV keep A in f64. */
    XFK_OPT_HEAT_MAX_PASSES = 13, /* heat flow: the outer loop's pass cap (>= 1, default 100) */
    XFK_OPT_NEWTON_INEXACT = 12 /* 1 (default, unless XFK_NEWTON_INEXACT=0 is set): the nonlinear
                                   loop's passes before the last solve their linear system to a
                                   forcing tolerance (Eisenstat-Walker: eta times the last Newton
                                   change |dV| / |V|, clamped to [Precision, 1e-3]); a pass that
                                   meets the loop's stop test (|dV| / |V| < 100 Precision) at a
                                   tolerance looser than Precision is followed by one more pass
                                   solved to Precision, so the answer is always that of a pass
                                   solved to the reference's tolerance.  0: every pass to
                                   Precision, as the reference (static2d.cpp:997-1008). */
};
int xfk_set_option(xfk_problem *prob, int option, double value);

/* FSolver::Static2D on the device.  flags: XFK_REBUILD_SYMBOLIC rebuilds the
 * CSR pattern, colouring and boundary maps (they are cached otherwise);
 * XFK_TIME_SPMV brackets every 16th SpMV launch with HIP events on the
 * solver stream and reports the mean launch duration; XFK_TIME_TAIL (sharded
 * solves) brackets the replicated coarse levels of every V-cycle and of the
 * setup (ms_rep_cycle, ms_rep_setup). */
int xfk_static2d(xfk_problem *prob, int flags, xfk_result *res);

/* A at every node (V * c, the value fsolver writes to .ans), host copy. */
int xfk_get_solution(xfk_problem *prob, double *A_host);

/* Circuit results after xfk_static2d: case (0/1), J, dV per circuit. */
int xfk_get_circuits(xfk_problem *prob, int *ccase, double *J, double *dV);

/* ---------------------------------------------------------------------------
 * Sharded solve (one large mesh across ranks, configs[4]).
 *
 * Rows (nodes, in the caller's -- normally Cuthill-McKee -- numbering) are
 * split into contiguous blocks, one per rank; each rank assembles the
 * elements touching its rows (ghost elements replicated, no communication),
 * exchanges the halo of the PCG vector before every SpMV, and all-reduces the
 * PCG's per-block dot-product partials once per iteration.  Boundary
 * conditions and circuits are evaluated on the GLOBAL mesh, so every rank
 * passes the same global description.  Periodic / antiperiodic pairs and
 * air-gap nodes ("coupled nodes") are assembled on every rank that needs them
 * (the averaging map of its owned rows then finds every entry locally).
 *
 * xfk_static2d and xfk_get_solution are collective over the communicator
 * (every rank calls them); xfk_get_solution returns the global solution on
 * every rank.
 * ------------------------------------------------------------------------- */
typedef struct xfk_comm xfk_comm;

/* RCCL, one process per GPU: rank 0 creates the 128-byte unique id, the caller
 * distributes it (e.g. torch.distributed broadcast), every rank then calls
 * xfk_comm_create_rccl (collective). */
int xfk_comm_unique_id(void *out, int bytes);
int xfk_comm_create_rccl(const void *unique_id, int bytes, int rank, int nranks, int device, xfk_comm **out);
/* In-process group of nranks communicators (one host thread per rank, any
 * devices, including several ranks on one device): the test transport. */
int xfk_comm_create_local(int nranks, xfk_comm **out_array);
void xfk_comm_destroy(xfk_comm *comm);
int xfk_comm_rank(const xfk_comm *comm);
int xfk_comm_size(const xfk_comm *comm);

/* Issue order and recording.  Every collective of a communicator runs after
 * the previous one in device order: when a collective is enqueued on another
 * stream than the previous collective, the communicator first makes that
 * stream wait for the event recorded after the previous one (RCCL matches
 * collectives by issue order; the sharded path issues halo exchanges on a side
 * stream and all-reduces / all-gathers on the main stream).
 *
 * xfk_comm_record(comm, mode) starts an empty recording (mode 1: the sequence
 * of collectives; mode 2: the sequence and every byte the rank receives, kept
 * in device memory, for xfk_comm_create_replay), or stops it (mode 0; the log
 * is kept).  xfk_comm_log copies the log: one ALLREDUCE / ALLGATHER / EXCHANGE
 * record per collective call, each EXCHANGE followed by one SEND / RECV
 * record per halo range.  Every rank of a correct program produces the same
 * sequence of calls (op, stream, bytes), and the send of rank a to rank b in
 * exchange k matches the receive of b from a in the same exchange. */
enum { XFK_COMM_ALLREDUCE = 1, XFK_COMM_EXCHANGE = 2, XFK_COMM_SEND = 3, XFK_COMM_RECV = 4, XFK_COMM_ALLGATHER = 5 };
typedef struct {
    long long seq;              /* collective number since the recording started */
    int op;                     /* XFK_COMM_* */
    int stream;                 /* stream index in first-use order (0: the first stream this communicator saw) */
    int waited;                 /* 1: another stream than the previous collective's; the communicator
                                   made it wait for that collective's completion event */
    int peer;                   /* SEND / RECV: the peer rank; -1 otherwise */
    long long bytes;            /* payload: ALLREDUCE the reduced bytes, ALLGATHER the bytes per rank,
                                   SEND / RECV the range; EXCHANGE 0 */
    long long g0;               /* SEND / RECV: the range's first global row; EXCHANGE: its range count */
} xfk_comm_op;
int xfk_comm_record(xfk_comm *comm, int mode);
int xfk_comm_log(const xfk_comm *comm, xfk_comm_op *out, int cap, int *count);
/* A communicator that replays the recording (mode 2) of `recorded`: same rank
 * and size, no peers; every collective checks that it is the next one of the
 * recording (op and sizes, else XFK_ERR_ARG) and copies the recorded received
 * bytes into place.  The recording is cut into one segment per solve
 * (xfk_static2d); replayed solve k is served segment k, the last segment
 * repeating, and must issue exactly that segment's collectives (a first and a
 * repeated solve differ: the PCG's batching uses the last solve's iteration
 * count).  It runs one rank of a sharded solve alone on its GPU with the
 * exact inputs of the recorded run: the per-rank compute time without the
 * transport. */
int xfk_comm_create_replay(const xfk_comm *recorded, xfk_comm **out);
/* Time inside collectives (the N > 1 bench line's diagnosis).  With timing on
 * (xfk_comm_time(comm, 1)) every collective is bracketed by two HIP events on
 * the stream it is issued on: the interval covers the transfer and any wait
 * for the peers' matching call (an RCCL kernel starts only when its peers'
 * have).  xfk_comm_timing waits for those events and returns, per op
 * (index 0 all-reduce, 1 halo exchange, 2 all-gather), the number of calls
 * and the summed and longest microseconds since the last read, then clears
 * them.  Timing off (the default): no events. */
int xfk_comm_time(xfk_comm *comm, int on);
int xfk_comm_timing(xfk_comm *comm, long long calls[3], double us_total[3], double us_max[3]);

typedef struct {
    int rank, nranks;
    int n_global;               /* global nodes */
    int row0, n_own;            /* owned rows [row0, row0 + n_own) */
    int n_halo;                 /* halo nodes (local ids n_own .. n_own + n_halo - 1) */
    int n_elems;                /* local (owned + ghost) elements */
    int n_send, n_recv;         /* halo ranges */
    int n_extra;                /* coupled nodes owned elsewhere, assembled here (local ids n_own ..) */
} xfk_dist_info;

/* Host-only partition plan (no device needed).  Call once with null arrays to
 * get the sizes in *info, then with l2g[n_own + n_halo], elems[n_elems],
 * recv[4 * n_recv] and send[4 * n_send] ({peer, local offset, length, first
 * global row} per range). */
int xfk_partition_plan(int n_nodes, int n_elems, const int *p, int rank, int nranks, xfk_dist_info *info,
                       int *l2g, int *elems, int *recv, int *send);
/* The same with coupled nodes (periodic pairs, air-gap quad nodes): every
 * element touching one is local on every rank, the coupled nodes owned
 * elsewhere are the first n_extra halo nodes (assembled rows), and a peer may
 * send several ranges (coupled nodes first).  xfk_problem_create_dist plans
 * this way for problems with periodic boundaries or air gaps. */
int xfk_partition_plan_coupled(int n_nodes, int n_elems, const int *p, int rank, int nranks, int n_coupled,
                               const int *coupled, xfk_dist_info *info, int *l2g, int *elems, int *recv, int *send);

/* This rank's part of the global problem `desc` on `device`. */
int xfk_problem_create_dist(const xfk_problem_desc *desc, int device, xfk_comm *comm, xfk_problem **out);
int xfk_dist_get_info(const xfk_problem *prob, xfk_dist_info *info);

/* ---------------------------------------------------------------------------
 * Time-harmonic planar problems: FSolver::Harmonic2D
 * (cfemm/fsolver/harmonic2d.cpp:36-790) with CBigComplexLinProb::PBCGSolveMod
 * (cspars.cpp:822-895, 1062-1081) as the solver.
 *
 * The base descriptor carries the real parts; these arrays (same lengths as
 * desc->blocks / lines / circs) carry what the AC formulation adds.  Blocks
 * with a B-H curve run the reference's successive-approximation loop
 * (ACSolver 0: averaged secant / incremental permeability per element,
 * residual correction on the right-hand side, relaxation after 5 iterations,
 * stop at |dV| / |V| < 100 Precision).  Case-2 circuits -- a specified
 * current in a conducting region, whose voltage gradient is an extra
 * unknown -- are solved through the Schur complement of the bordered system
 * (one extra COCG solve per such circuit; not with periodic boundaries).
 * ac_solver = 1 selects the reference's Newton AC solver instead
 * (harmonic2d.cpp:611-639, harmonicaxi.cpp:520-547): after the first pass the
 * nonlinear elements add their Newton terms -- Mn to the matrix, the
 * Hermitian / conj-symmetric / anti-Hermitian remainders to three auxiliary
 * matrices -- and every pass solves M V + Mh V + Ms conj(V) + Ma V = b by the
 * reference's KludgeSolve (cspars.cpp:1000-1060: at most 10 COCG solves on M
 * with the auxiliary terms moved to the right-hand side, each followed by a
 * line search on the true residual) at the adaptive precision
 * min(1e-4, 0.001 res) >= Precision (harmonic2d.cpp:821-825).
 * The reference itself rejects LamType 1/2 in AC analyses; wound regions
 * with proximity effects (LamType > 2) return XFK_ERR_UNSUPPORTED.  Single
 * device.
 * ------------------------------------------------------------------------- */
typedef struct {
    double J_im;                /* imaginary part of the source current density, MA/m^2 */
    double Theta_hx, Theta_hy;  /* hysteresis lag, degrees */
    double Lam_d;               /* lamination thickness, mm */
    /* nonlinear blocks (desc->blocks[k].BHpoints > 0, LamType 0): the curve
     * processed by GetSlopes(omega) (xfemm_bh_get_slopes_ac) -- B and the real
     * parts of H and slope in desc->blocks[k], the imaginary parts here; mu_x /
     * mu_y there are the curve's initial permeability, Theta_hx / Theta_hy
     * its Theta_hn.  NULL for linear blocks. */
    const double *H_im;
    const double *slope_im;
} xfk_block_ac_desc;

typedef struct {
    double c0_im, c1_im;        /* mixed BC, imaginary parts */
    double Mu, Sig;             /* small-skin-depth BC (BdryFormat 1): relative mu, MS/m */
} xfk_line_ac_desc;

typedef struct {
    double amps_im, dvolts_im;
} xfk_circuit_ac_desc;

typedef struct {
    double frequency;           /* Hz, > 0 */
    const xfk_block_ac_desc *blocks;
    const xfk_line_ac_desc *lines;      /* may be NULL when n_lines == 0 */
    const xfk_circuit_ac_desc *circs;   /* may be NULL when n_circs == 0 */
    int ac_solver;              /* [ACSolver]: 0 successive approximation, 1 Newton */
    const double *label_prox_mu;   /* 2 per label (re, im): CMBlockLabel::ProximityMu after
                                      FSolver::GetFillFactor (fsolver.cpp:1083-1193), the relative
                                      permeability of a wound region of a LamType > 2 block
                                      (harmonic2d.cpp:664-668); read for those labels only;
                                      NULL: 1 for every label */
    int prev_type;              /* [PrevType] of the file the problem was loaded from (0: none).  The
                                   solve does not read it; xfk_mag_ac_* refuses a problem with
                                   prev_type != 0 (incremental permeability is not post-processed) */
} xfk_harmonic_desc;

int xfk_problem_create_harmonic(const xfk_problem_desc *desc, const xfk_harmonic_desc *ac, int device,
                                xfk_problem **out);
/* The same problem sharded over comm's ranks (row blocks, as
 * xfk_problem_create_dist): every rank passes the GLOBAL descriptors;
 * xfk_harmonic2d and xfk_get_solution_complex are collective.  COCG exchanges
 * the halo of its vectors before every SpMV and all-reduces its per-block
 * partials once per iteration; the AMG preconditioner is the sharded hierarchy
 * of the real surrogate (Amg::setup_dist).  Linear problems and the
 * successive-approximation nonlinear loop (ACSolver 0), the Newton AC solver
 * (ACSolver 1: the auxiliary matrices assembled per rank, the KludgeSolve
 * products exchange V / the step at the halo, its dot products all-reduced)
 * and Case-2 circuits (each rank holds the border columns of its rows; C . y
 * all-reduced, the small circuit system solved on every rank alike). */
int xfk_problem_create_harmonic_dist(const xfk_problem_desc *desc, const xfk_harmonic_desc *ac, int device,
                                     xfk_comm *comm, xfk_problem **out);
/* FSolver::Harmonic2D, or HarmonicAxisymmetric (harmonicaxi.cpp:1-800) when
 * desc->problem_type is XFK_AXISYMMETRIC, on the device (complex-symmetric
 * COCG, the reference's stopping test |r| / |b| <= Precision).  flags as for
 * xfk_static2d. */
int xfk_harmonic2d(xfk_problem *prob, int flags, xfk_result *res);
/* A = V * c at every node, interleaved (re, im); axisymmetric problems: the
 * flux V * c * 2 pi r * 0.01 (harmonicaxi.cpp:790). */
int xfk_get_solution_complex(xfk_problem *prob, double *A_host);
/* Circuit results: case, J and dV interleaved (re, im) per circuit. */
int xfk_get_circuits_complex(xfk_problem *prob, int *ccase, double *J, double *dV);
/* Assembled complex system after all boundary conditions (val, b interleaved). */
int xfk_get_csr_complex(xfk_problem *prob, int *rowptr, int *col, double *val, double *b);

/* ---------------------------------------------------------------------------
 * Electrostatic problems: ESolver::AnalyzeProblem
 * (cfemm/esolver/esolver.cpp:389-646) over the same assembly, boundary maps
 * and AMG-PCG as the static magnetics path, and ESolver::ChargeOnConductor
 * (esolver.cpp:797-844).  Single device.
 *
 * The descriptors carry the state ESolver::LoadProblemFile and LoadMesh leave
 * behind: coordinates in mm, 0-based indices, -1 for "none".
 *
 * Prescribed-voltage conductors (CircType 1) fix their nodes; a floating
 * conductor (CircType 0, a prescribed total charge) is one unknown: its nodes
 * are merged onto the conductor's lowest-numbered node, whose row carries
 * 1e9 c q (c = 1e-6 / eo) on its right-hand side, and take that node's value
 * after the solve (bit-equal).  xfk_get_csr shows the merged system: the
 * other nodes of a floating conductor are identity rows.  The reference's
 * bordered form replaces the conductor's diagonal by minus its off-diagonal
 * row sum (esolver.cpp:625-628), which drops the stiffness towards directly
 * adjacent fixed nodes and any mixed-boundary terms from it, and assigns
 * 1e9 c q to its right-hand side over what the elements left there; the
 * merged row keeps both.  The two agree when free nodes in charge-free
 * material surround the conductor.
 * ------------------------------------------------------------------------- */
/* CMaterialProp of esolver (CMaterialProp.h): relative permittivities, C/m^3. */
typedef struct {
    double ex, ey;
    double qv;
} xfk_es_block_desc;

/* CSBlockLabel. */
typedef struct {
    int block;                  /* index into blocks */
    int is_external;            /* axisymmetric: conformally mapped exterior region */
} xfk_es_label_desc;

/* CSBoundaryProp. */
typedef struct {
    int format;                 /* BdryFormat: 0 fixed V, 1 mixed, 2 surface charge, 3 periodic, 4 antiperiodic */
    double V;
    double qs;                  /* C/m^2 */
    double c0, c1;
} xfk_es_line_desc;

/* CSPointProp: qp == 0 fixes V at the node, else a point charge qp (C/m; C when axisymmetric). */
typedef struct {
    double V, qp;
} xfk_es_point_desc;

/* CSCircuit. */
typedef struct {
    int type;                   /* CircType: 1 prescribed voltage V, 0 prescribed total charge q */
    double V, q;
} xfk_es_conductor_desc;

typedef struct {
    int n_nodes;
    const double *x, *y;        /* node coordinates, mm (ESolver::LoadMesh) */
    const int *marker;          /* point-prop index or -1 (may be NULL) */
    const int *conductor;       /* conductor index or -1 (may be NULL) */
    int n_elems;
    const int *p;               /* 3 per element */
    const int *e;               /* 3 per element: boundary-prop index or -1 (may be NULL) */
    const int *lbl;             /* block label of each element */
    int n_blocks;      const xfk_es_block_desc *blocks;
    int n_labels;      const xfk_es_label_desc *labels;
    int n_lines;       const xfk_es_line_desc *lines;
    int n_points;      const xfk_es_point_desc *points;
    int n_conductors;  const xfk_es_conductor_desc *conductors;
    int n_pbc;         const int *pbc;   /* 3 per pair: node, node, type (0 periodic, 1 anti) */
    double precision;           /* [Precision] */
    int length_units;           /* femm::LengthUnit */
    int problem_type;           /* XFK_PLANAR or XFK_AXISYMMETRIC (x is r, y is z) */
    double depth;               /* [Depth], user units (planar) */
    double ext_zo, ext_ro, ext_ri;   /* [extZo] [extRo] [extRi], user units */
} xfk_es_problem_desc;

/* Upload an electrostatic problem.  The descriptor is checked before the
 * device is touched (XFK_ERR_ARG with a message naming the cause): indices
 * out of range, a non-positive depth on a planar problem, a point property on
 * a node of a floating conductor, a node both in a floating conductor and
 * fixed by a line or point property.  xfk_get_csr, xfk_set_option,
 * xfk_problem_memory and xfk_problem_destroy work on the problem;
 * xfk_static2d and xfk_harmonic2d refuse it (XFK_ERR_ARG). */
int xfk_problem_create_electrostatic(const xfk_es_problem_desc *desc, int device, xfk_problem **out);
/* ESolver::AnalyzeProblem on the device; flags and result as xfk_static2d
 * (one linear solve).  The charges of the prescribed-voltage conductors are
 * integrated after the solve, as the reference does.  xfk_get_solution then
 * returns V at every node, unscaled.  XFK_ERR_ARG on a magnetics problem. */
int xfk_electrostatic(xfk_problem *prob, int flags, xfk_result *res);
/* Per conductor after xfk_electrostatic: V the prescribed (CircType 1) or
 * solved (CircType 0) potential -- the .res conductor line's first column,
 * L.V[NumNodes + i] -- and q the integrated (CircType 1) or prescribed
 * (CircType 0) charge, C.  Either array may be NULL. */
int xfk_get_conductors(xfk_problem *prob, double *V, double *q);
/* ChargeOnConductor(conductor) of the last solution, any conductor type:
 * the sum over the elements touching a node of the conductor, in element
 * order within fixed workgroup chunks and over the chunks in order, so two
 * runs give the same bits. */
int xfk_conductor_charge(xfk_problem *prob, int conductor, double *q);

/* ---------------------------------------------------------------------------
 * Heat flow (the reference's hsolver: HSolver::AnalyzeProblem,
 * cfemm/hsolver/hsolver.cpp:458-852, and HSolver::ChargeOnConductor, 987-1035).
 *
 * The descriptors carry what HSolver::LoadProblemFile and LoadMesh leave
 * behind, as the electrostatic ones do, except that HSolver works in metres:
 * coordinates in m, depth and ext_* in the problem's length units (inches
 * 0.0254 m, mm 0.001, cm 0.01, m 1, mils 2.54e-5, um 1e-6), 0-based indices,
 * -1 for "none".
 *
 * The problem is nonlinear when the block of any element has a K(T) table or
 * any edge carries a radiation property; xfk_heatflow then repeats assembly
 * and solve until sqrt(sum (T - To)^2 / sum To^2) < 100 Precision, as the
 * reference does.  Conductors behave as in electrostatics: CircType 1 fixes
 * the temperature of its nodes, CircType 0 (a prescribed total heat flow q, W)
 * is merged onto its lowest-numbered node (see above and INTEGRATION.md).
 * ------------------------------------------------------------------------- */
/* CHMaterialProp: conductivities W/(m K), volumetric heat capacity Kt
 * J/(m^3 K), volume heating qv W/m^3, and the K(T) table (npts knots, the same
 * value for both directions; npts == 0: kx, ky). */
typedef struct {
    double kx, ky;
    double kt;
    double qv;
    int npts;
    const double *T, *K;
} xfk_hf_block_desc;

/* CHBlockLabel. */
typedef struct {
    int block;                  /* index into blocks */
    int is_external;            /* axisymmetric: conformally mapped exterior region */
} xfk_hf_label_desc;

/* CHBoundaryProp. */
typedef struct {
    int format;                 /* BdryFormat: 0 fixed T, 1 heat flux qs, 2 convection h (T - Tinf),
                                   3 radiation beta ksb (T^4 - Tinf^4), 4 periodic, 5 antiperiodic */
    double Tset;
    double qs;                  /* W/m^2 */
    double beta;
    double h;                   /* W/(m^2 K) */
    double Tinf;
} xfk_hf_line_desc;

/* CHPointProp: qp == 0 fixes T at the node, else a point source qp (W/m; W when axisymmetric). */
typedef struct {
    double T, qp;
} xfk_hf_point_desc;

/* CHConductor. */
typedef struct {
    int type;                   /* CircType: 1 prescribed temperature T, 0 prescribed total heat flow q */
    double T, q;
} xfk_hf_conductor_desc;

typedef struct {
    int n_nodes;
    const double *x, *y;        /* node coordinates, m (HSolver::LoadMesh) */
    const int *marker;          /* point-prop index or -1 (may be NULL) */
    const int *conductor;       /* conductor index or -1 (may be NULL) */
    int n_elems;
    const int *p;               /* 3 per element */
    const int *e;               /* 3 per element: boundary-prop index or -1 (may be NULL) */
    const int *lbl;             /* block label of each element */
    int n_blocks;      const xfk_hf_block_desc *blocks;
    int n_labels;      const xfk_hf_label_desc *labels;
    int n_lines;       const xfk_hf_line_desc *lines;
    int n_points;      const xfk_hf_point_desc *points;
    int n_conductors;  const xfk_hf_conductor_desc *conductors;
    int n_pbc;         const int *pbc;   /* 3 per pair: node, node, type (0 periodic, 1 anti) */
    double precision;           /* [Precision] */
    int length_units;           /* femm::LengthUnit */
    int problem_type;           /* XFK_PLANAR or XFK_AXISYMMETRIC (x is r, y is z) */
    double depth;               /* [Depth], user units (planar) */
    double ext_zo, ext_ro, ext_ri;   /* [extZo] [extRo] [extRi], user units */
    double dt;                  /* [dT], s; 0: steady */
    const double *t_prev;       /* n_nodes: the previous time step's solution (dt != 0) */
} xfk_hf_problem_desc;

/* Upload a heat-flow problem.  The descriptor is checked before the device is
 * touched (XFK_ERR_ARG with a message naming the cause): what
 * xfk_problem_create_electrostatic refuses, and dt != 0 without t_prev, dt < 0,
 * a K(T) table with npts < 0 or without its arrays.  xfk_static2d,
 * xfk_harmonic2d and xfk_electrostatic refuse the problem (XFK_ERR_ARG). */
int xfk_problem_create_heatflow(const xfk_hf_problem_desc *desc, int device, xfk_problem **out);
/* HSolver::AnalyzeProblem on the device; flags: XFK_REBUILD_SYMBOLIC (the
 * timing flags of xfk_static2d are ignored).  Every pass
 * assembles from the last solution (the first from T = 0) and warm-starts the
 * PCG from it.  A linear problem runs one pass, a nonlinear one at least two
 * (no test is made while sum To^2 == 0).  The loop also ends when the solution
 * did not change at all (the reference would spin), and with XFK_ERR_NOCONV
 * ("heat-flow iteration did not converge in N passes") at the pass cap,
 * XFK_OPT_HEAT_MAX_PASSES (default 100).  res->newton_iters is the pass count,
 * res->last_res the last change.  The heat flows of the prescribed-temperature
 * conductors are integrated after the solve.  xfk_get_solution then returns T
 * at every node.  XFK_ERR_ARG on any other kind of problem. */
int xfk_heatflow(xfk_problem *prob, int flags, xfk_result *res);
/* One pass's system assembled from the nodal temperatures T (n_nodes; NULL:
 * zeros) without solving; xfk_get_csr then shows it.  The solution, if any,
 * is kept. */
int xfk_heatflow_assemble(xfk_problem *prob, const double *T);
/* The time step: dt (0: steady) and the previous solution (n_nodes; may be
 * NULL when dt == 0).  xfk_heatflow_advance copies the last solution into the
 * previous-solution buffer on the device and sets dt, so a time-stepping loop
 * uploads nothing and keeps its symbolic phase. */
int xfk_heatflow_set_step(xfk_problem *prob, double dt, const double *t_prev);
int xfk_heatflow_advance(xfk_problem *prob, double dt);
/* Per conductor after xfk_heatflow: T the prescribed (CircType 1) or solved
 * (CircType 0) temperature and q the integrated (CircType 1) or prescribed
 * (CircType 0) heat flow, W.  Either array may be NULL. */
int xfk_hf_get_conductors(xfk_problem *prob, double *T, double *q);
/* ChargeOnConductor(conductor) of the last solution, any conductor type, with
 * the conductivities at the solved temperatures; summed in a fixed order, so
 * two runs give the same bits. */
int xfk_hf_conductor_flow(xfk_problem *prob, int conductor, double *q);

/* ---------------------------------------------------------------------------
 * Post-processing of a solved electrostatic or heat-flow problem on the
 * device: what the reference's epproc and hpproc compute (getElementD,
 * getNodalD, blockIntegral types 0-6 with makeMask, getPointValues,
 * lineIntegral), in the reference's operation order.  Lengths are the problem's own length units, as the
 * reference's post-processors read them.
 *
 * Every function returns XFK_ERR_ARG with a message naming the cause on a
 * magnetics problem, on a problem without a solution, on a NULL argument it
 * needs and on a negative point count.  The mesh tables (node -> element
 * lists of the mesh's own connectivity in counter-clockwise order, the cell
 * grid of the point search) are built at the first call that needs them and
 * kept; the element and corner fields are cached until the next solve or
 * xfk_pot_set_solution.  xfk_problem_memory counts all of them.
 * ------------------------------------------------------------------------- */
/* Load a nodal solution (n_nodes values: V, or T) into a potential problem
 * and mark it solved: post-processing of a loaded .res / .anh.  The charges
 * (heat flows) of the prescribed-value conductors are integrated from it, as
 * after a solve, so xfk_get_conductors / xfk_hf_get_conductors describe the
 * loaded solution. */
int xfk_pot_set_solution(xfk_problem *prob, const double *V);
/* The mark of every node as the reference's L.Q holds it and its .res / .anh
 * node lines carry it (n_nodes ints): a conductor's index on its nodes, else
 * -1 on a node with a point property or on a BdryFormat 0 edge, else -2.
 * Derived from the descriptor at creation (the post-processor's smoothing
 * reads the same marks); no solution needed.  Host data: no device work. */
int xfk_pot_get_qmarks(xfk_problem *prob, int *Q);
/* The marks of a solution file (n_nodes ints: the Q column of a .res / .anh)
 * in place of the descriptor rule xfk_pot_get_qmarks restates; call it before
 * xfk_pot_set_solution.  XFK_ERR_ARG on a mark that is neither -2, -1 nor a
 * conductor's index.  A problem marked this way was opened from a file, which
 * holds no boundary conditions: xfk_electrostatic, xfk_heatflow and
 * xfk_heatflow_assemble return XFK_ERR_UNSUPPORTED on it from then on. */
int xfk_pot_set_qmarks(xfk_problem *prob, const int *Q);
/* d_PlotBounds of the reference's OpenDocument (epproc.cpp:184-225, and its
 * twin in hpproc.cpp): out6 = min, max of the potential over the nodes, of
 * |D| (|F|) and of |E| (|G|) over the elements whose label is not external.
 * The reference's starting values are kept: |D| starts from the element whose
 * index is the number of external elements (element 0 when every element is
 * external, where the reference reads past its list), |E| from element 0,
 * external or not.  One fixed-order min / max reduction without atomics: two
 * runs give equal bits. */
int xfk_pot_plot_bounds(xfk_problem *prob, double *out6);
/* Per element D (C/m^2) and E (V/m), or F (W/m^2) and G (K/m): x and y
 * components interleaved, 2 n_elems each.  Either may be NULL. */
int xfk_pot_element_fields(xfk_problem *prob, double *D, double *E);
/* The smoothed D (F) at the three corners of every element: 6 n_elems
 * (element, corner, component). */
int xfk_pot_corner_fields(xfk_problem *prob, double *d);
/* Block integrals over the elements whose label is selected (one byte per
 * block label), every type 0-4 in one pass:
 *   out7[0]     type 0: stored energy, J (electrostatics); average T, K (heat flow)
 *   out7[1]     type 1: cross-section area, m^2
 *   out7[2]     type 2: volume, m^3
 *   out7[3..4]  type 3: average D (F), x and y
 *   out7[5..6]  type 4: average E (G), x and y
 * summed in a fixed order, so two runs give the same bits.
 * xfk_pot_block_integral returns one type in the reference's numbering
 * (out2[1] is 0 for the scalar types).  Types 5 and 6, the weighted stress
 * tensor force (N: x and y, or 0 and z on an axisymmetric problem) and torque
 * about the origin (N m; 0 on an axisymmetric problem), are summed over all
 * elements against the gradient of the mask: they succeed on an
 * electrostatic problem that holds a mask made for the same label selection
 * (xfk_pot_make_mask) and are refused otherwise, and always on a heat-flow
 * problem. */
int xfk_pot_block_integrals(xfk_problem *prob, const unsigned char *label_selected, double *out7);
int xfk_pot_block_integral(xfk_problem *prob, const unsigned char *label_selected, int type, double *out2);
/* xfk_pot_block_integrals with the sums taken in the reference's order,
 * element by element with one rounding per selected element, instead of the
 * fixed tree: the value the reference's own loop leaves, so that a sum on a
 * tie of its "%f" prints as the reference prints it.  One workgroup walks the
 * elements (about 3 ns each); the file-based post-processors use it. */
int xfk_pot_block_integrals_ordered(xfk_problem *prob, const unsigned char *label_selected, double *out7);
/* The mask of the weighted stress tensor integrals (the reference's
 * PostProcessor::makeMask) for the selected labels (one byte per block label),
 * electrostatic problems only: a Laplace problem of its own on the mesh's
 * connectivity, weighted per element by sqrt(label_max_area[label]) (the
 * element's own area where that is <= 0; NULL: everywhere), 1 on the selected
 * labels' and the selected nodes' nodes (node_selected: one byte per node, may
 * be NULL), 0 on exterior edges, conductors, fixed points and every other
 * label that is not air, solved by the problem's own AMG-PCG to its Precision
 * and thresholded at 0.5.  XFK_ERR_ARG with the reference's message when the
 * selection abuts a region that is not free space.  A new solution (a solve,
 * xfk_pot_set_solution) or a new xfk_pot_make_mask drops the mask.
 * xfk_pot_get_mask: the solved W and the 0/1 mask, n_nodes doubles each;
 * either may be NULL. */
int xfk_pot_make_mask(xfk_problem *prob, const unsigned char *label_selected, const unsigned char *node_selected,
                      const double *label_max_area);
int xfk_pot_get_mask(xfk_problem *prob, double *W, double *msk);
/* getPointValues at n points.  elem[i] is the lowest-numbered element that
 * contains point i by the reference's InTriangleTest, or -1 when none does;
 * out holds 8 doubles per point --
 *   electrostatics: V, Dx, Dy, Ex, Ey, ex, ey, nrg
 *   heat flow:      T, Fx, Fy, Kx, Ky, Gx, Gy, 0
 * -- all NaN for a point outside the mesh.  smooth != 0 blends the smoothed
 * corner values instead of taking the element's D (F). */
int xfk_pot_point_values(xfk_problem *prob, int n, const double *x, const double *y, int smooth, int *elem,
                         double *out);
/* The same values with the element of every point given (elem[i] in
 * [0, n_elems), or -1: NaN), without the search: for a caller that locates
 * points itself, as the file-based post-processors do with the reference's
 * own walk from the element found last. */
int xfk_pot_point_values_at(xfk_problem *prob, int n, const double *x, const double *y, const int *elem, int smooth,
                            double *out);
/* Contour (line) integrals, the reference's lineIntegral, for a batch of
 * contours: contour c is the polyline through the vertices ptr[c] .. ptr[c+1]
 * of (x, y), in the problem's length units; ptr has n_contours + 1 entries.
 * Every segment is sampled at npts midpoints (npts <= 0: the reference's 400),
 * each shifted by 1e-6 length units to the segment's left (n = i t) except for
 * the heat-flow average temperature; the samples are made on the device.  A
 * sample takes the lowest-numbered element that contains it, as
 * xfk_pot_point_values does; a sample no element contains adds nothing and is
 * counted in missed[c] (may be NULL).  smooth != 0 blends the smoothed corner
 * values, the reference's default.  out holds 2 doubles per contour, type in
 * the reference's numbering --
 *   electrostatics                         heat flow
 *   0  V(first) - V(last), 0               0  T(first) - T(last), 0
 *   1  flux of D (C), its average (C/m^2)  1  flux of F (W), its average (W/m^2)
 *   2  length (m), swept area (m^2)        2  length (m), swept area (m^2)
 *   3  stress tensor force (N): x, y;      3  average T (K), the weight sum (m^2)
 *      0, z on an axisymmetric problem
 *   4  stress tensor torque about the
 *      origin (N m), 0; 0 on an
 *      axisymmetric problem
 * Type 0 is NaN when an end lies outside the mesh (missed: the ends outside);
 * an average over a contour wholly outside is 0/0 = NaN.  The sums run in a
 * fixed order per contour: two runs give the same bits, and a contour gives
 * the same bits alone or inside any batch.  XFK_ERR_ARG also for a type the
 * physics does not have, a contour with fewer than 2 points, a zero-length
 * segment, a NaN or infinite vertex and a negative count.
 * xfk_pot_line_integral: one contour of n points. */
int xfk_pot_line_integrals(xfk_problem *prob, int n_contours, const int *ptr, const double *x, const double *y,
                           int type, int smooth, int npts, double *out, int *missed);
int xfk_pot_line_integral(xfk_problem *prob, int n, const double *x, const double *y, int type, int smooth, int npts,
                          double *out2, int *missed);

/* Diagnostics of the post-processor, for tests and the lab probe; not part of
 * the interface a caller should build on.
 * xfk_pot_corner_branches: which case of getNodalD each (element, corner)
 * took, 3 n_elems bytes: 0 the least-squares fit, 1-5 the reference's five
 * "punt" cases in its order (5: the 10.0001 degree rule), 6 a singular fit
 * (det == 0).  Runs the corner kernel again.
 * xfk_pot_grid_info: the cell grid of the point search (built if need be):
 * origin x0, y0, cells per length unit in x and y, cells nx, ny, the number of
 * oversize elements, the total length of the cell lists.
 * xfk_pot_time: HIP-event times in ms, each the median of `repeats` runs after
 * a warm-up, of [1] the cell-grid build (count, scan, fill), [2] the
 * element-field launch, [3] the corner-field launch, [4] the block-integral
 * launch and its sum, [5], [6] the point kernel on the n given points with
 * smoothing off and on; [0] is the host build of the mesh tables (wall clock).
 * *tests_per_point: the mean number of elements a point is tested against. */
int xfk_pot_corner_branches(xfk_problem *prob, unsigned char *branch);
int xfk_pot_grid_info(xfk_problem *prob, double *out8);
int xfk_pot_time(xfk_problem *prob, int n, const double *x, const double *y, int repeats, double *ms7,
                 double *tests_per_point);
/* ... and of the weighted stress tensor mask.
 * xfk_pot_mask_info: [0] 1 while the problem holds a mask; of the last
 * xfk_pot_make_mask [1] the PCG iterations, [2] ms creating the auxiliary
 * problem (host wall clock; 0 once it exists), [3] ms for the fixed values and
 * the validity check (wall clock, with its one read-back), [4] - [7] the mask
 * solve's HIP-event times as xfk_result has them: symbolic phase, assembly,
 * AMG setup, PCG, [8] ms of the whole call (wall clock).
 * xfk_pot_mask_problem: the auxiliary problem the mask is solved in (owned by
 * prob), for xfk_get_csr of its assembled system.
 * xfk_pot_stress_time: HIP-event ms of the integral launch for types 5 and 6
 * and its sum, the median of `repeats` runs after a warm-up. */
int xfk_pot_mask_info(xfk_problem *prob, double *out9);
int xfk_pot_mask_problem(xfk_problem *prob, xfk_problem **aux);
int xfk_pot_stress_time(xfk_problem *prob, int repeats, double *ms);
/* ... and of the contour integrals.
 * xfk_pot_contour_samples: the samples of one contour of n points for a
 * sampled type (1, 3, 4; heat flow 1, 3) as the kernel makes them: xy, 2
 * doubles per sample, and elem, the element each took (-1: none),
 * (n - 1) npts of each (npts <= 0: 400).
 * xfk_pot_contour_time: HIP-event ms of the sample launch and its
 * per-contour sum for a batch of a sampled type, the median of `repeats` runs
 * after a warm-up. */
int xfk_pot_contour_samples(xfk_problem *prob, int n, const double *x, const double *y, int type, int npts,
                            double *xy, int *elem);
int xfk_pot_contour_time(xfk_problem *prob, int n_contours, const int *ptr, const double *x, const double *y,
                         int type, int smooth, int npts, int repeats, double *ms);

/* ---------------------------------------------------------------------------
 * Post-processing of a magnetostatic problem: the element flux density and the
 * block integrals of the reference's fpproc that need no mask (the masked
 * ones, 18-23, follow below)
 * (FPProc::GetElementB, fpproc.cpp:2970-3082; FPProc::BlockIntegral, 3642-4092;
 * CMMaterialProp::DoEnergy / DoCoEnergy, CMaterialProp.cpp:595-677), of a
 * problem made by xfk_problem_create, planar or axisymmetric, after
 * xfk_static2d or xfk_mag_set_solution.  fpproc's arithmetic in its operation
 * order, in the problem's length units; the sums are taken per workgroup and
 * then over the workgroups in a fixed order, so a call repeats bit for bit.
 *
 * Refused, with the cause in xfk_last_error: a harmonic problem and a sharded
 * problem (XFK_ERR_UNSUPPORTED), an electrostatic or heat-flow problem
 * (XFK_ERR_ARG); and by the block integrals a selection holding a label whose
 * block has LamType > 2 (a wound region with proximity effects) or is a
 * nonlinear permanent magnet (H_c != 0 with a B-H curve)
 * (XFK_ERR_UNSUPPORTED).  The problem stays usable after a refusal.
 *
 * A label's circuit columns (Case, J, dVolts: what GetJA reads,
 * fpproc.cpp:3495-3578) are the solve's circuit results (xfk_get_circuits),
 * the ones FSolver writes to the .ans label lines.  The conductivity of a
 * specified-voltage region is the solver's (0 in a wound label,
 * static2d.cpp:118-122); the descriptor carries no Lam_d, so fpproc's zero
 * conductivity of an in-plane laminated block with Lam_d != 0 is not applied.
 *
 * xfk_mag_set_solution: A[n_nodes] as the .ans carries it (A, or the flux
 * 2 pi r A on an axisymmetric problem: what xfk_get_solution returns) replaces
 * the solution for post-processing, without a solve; the next xfk_static2d
 * replaces it again.
 * xfk_mag_set_depth: [Depth] in the problem's length units; -1 (a .fem without
 * the line), and a problem it was never called on: the reference's default of
 * 1 m (fpproc.cpp:1618).
 * xfk_mag_element_b: B1[n_elems], B2[n_elems] (either may be NULL).
 * xfk_mag_block_integrals: label_selected[n_labels] (non-zero: selected);
 * out[52]: (re, im) of inttype 0 .. 25.  Answered: 0 A.J, 1 A, 2 stored energy,
 * 5 area, 7 total current, 8 9 B over the volume, 10 volume, 11 12 Lorentz
 * force (11 is 0 when axisymmetric), 15 Lorentz torque (planar, else 0),
 * 17 coenergy, 24 moment of inertia, 25 centroid (re x, im y; 0 / 0 = NaN with
 * nothing selected).  0 for every other type: 3, 13, 14 and 16 are 0 at
 * Frequency 0 in the reference as well; 4 (resistive losses) and 6 (total
 * losses) are not built; 18-23 (below) are filled when the problem holds the
 * mask of this very selection, and are 0 otherwise.
 * xfk_mag_block_integral: one type into out2[2]; a type in 18-23 without the
 * mask of this very selection is refused (XFK_ERR_ARG, naming xfk_mag_make_mask).
 * xfk_mag_time: HIP-event ms of the element-B launch (ms[0]) and of the
 * integral launch with its sum, every label selected (ms[1]): the median of
 * `repeats` runs after a warm-up.
 * ------------------------------------------------------------------------- */
int xfk_mag_set_solution(xfk_problem *prob, const double *A);
int xfk_mag_set_depth(xfk_problem *prob, double depth);
int xfk_mag_element_b(xfk_problem *prob, double *B1, double *B2);
int xfk_mag_block_integrals(xfk_problem *prob, const unsigned char *label_selected, double *out);
int xfk_mag_block_integral(xfk_problem *prob, const unsigned char *label_selected, int type, double *out2);
int xfk_mag_time(xfk_problem *prob, int repeats, double *ms);

/* ---------------------------------------------------------------------------
 * Post-processing of a time-harmonic problem (xfk_problem_create_harmonic,
 * planar or axisymmetric, one device): the complex element flux density and
 * fpproc's block integrals at Frequency != 0 (FPProc::GetElementB,
 * fpproc.cpp:2970-3082; GetJA, 3495-3578; BlockIntegral, 3642-3963;
 * OpenDocument's mu_fdx / mu_fdy, 1703-1758; CMMaterialProp::GetMu(CComplex)
 * and GetH(CComplex), CMaterialProp.cpp:722-772, 493-519), after xfk_harmonic2d
 * or xfk_mag_ac_set_solution.  The entry points above keep refusing a harmonic
 * problem; these refuse a static one.  fpproc's arithmetic in its operation
 * order; the sums per workgroup, then over the workgroups in a fixed order: a
 * call repeats bit for bit.  Depth: xfk_mag_set_depth.
 *
 * A label's Case / J / dVolts are the solve's circuit results
 * (xfk_get_circuits_complex), as the .ans label lines carry them: a Case-2
 * circuit (a specified current in a conducting region) is written as Case 0
 * with its solved voltage gradient (harmonic2d.cpp:988-990).  A nonlinear
 * block's permeability is evaluated over the curve the descriptor carries
 * (GetSlopes(omega)).  Where the label's conductivity is 0, fpproc's
 * sig = 1e6 / Re(1 / o) of type 4 is 0 / 0; no loss is added there.
 *
 * xfk_mag_ac_set_solution: A[2 n_nodes], interleaved (re, im), as the .ans
 * carries it (what xfk_get_solution_complex returns) replaces the solution for
 * post-processing; the next xfk_harmonic2d replaces it again.
 * xfk_mag_ac_element_b: B1[2 n_elems], B2[2 n_elems], interleaved (either may
 * be NULL); answered whatever the blocks are.
 * xfk_mag_ac_block_integrals: label_selected[n_labels]; out[52]: (re, im) of
 * inttype 0 .. 25:
 *    0 A.conj(J)        1 A                 2 stored energy (time average)
 *    3 hysteresis and lamination loss       4 resistive loss     5 area
 *    6 total loss (3 + 4)                   7 total current      8 9 B over the volume
 *   10 volume          11 12 steady Lorentz force (11: 0 when axisymmetric)
 *   13 14 double-frequency Lorentz force (13: planar only)
 *   15 steady Lorentz torque, 16 its double-frequency part (planar only)
 *   17 coenergy (= 2)  24 moment of inertia 25 centroid (0 / 0 = NaN with nothing selected)
 * Types 18-23 need the weighted stress tensor mask, which stays refused for
 * harmonic problems: they are answered with 0.
 * xfk_mag_ac_block_integral: one type into out2[2].
 * xfk_mag_ac_time: HIP-event ms of the element-B launch (ms[0]) and of the
 * integral launch with its sum, every answerable label selected (ms[1]): the
 * median of `repeats` runs after a warm-up.
 *
 * Refused before any launch, with the cause in xfk_last_error, the problem
 * staying usable: a static problem ("use xfk_mag_*") and a scalar-potential
 * problem (XFK_ERR_ARG); a sharded problem and one created with
 * prev_type != 0 (XFK_ERR_UNSUPPORTED); no solution yet and none set
 * (XFK_ERR_ARG); by both integral calls and for every type, a selection holding
 * a label whose block has LamType > 2 (XFK_ERR_UNSUPPORTED: its J, conductivity
 * and permeability need FPProc::GetFillFactor, whose wire data the descriptor
 * does not carry); an unknown type (XFK_ERR_ARG).
 * ------------------------------------------------------------------------- */
int xfk_mag_ac_set_solution(xfk_problem *prob, const double *A_re_im);
int xfk_mag_ac_element_b(xfk_problem *prob, double *B1_re_im, double *B2_re_im);
int xfk_mag_ac_block_integrals(xfk_problem *prob, const unsigned char *label_selected, double *out);
int xfk_mag_ac_block_integral(xfk_problem *prob, const unsigned char *label_selected, int type, double *out2);
int xfk_mag_ac_time(xfk_problem *prob, int repeats, double *ms);

/* The weighted stress tensor force and torque of a magnetostatic problem:
 * fpproc's block integrals 18-23 (fpproc.cpp:3966-4079, HenrotteVector
 * 3614-3640) over the mask of FPProc::MakeMask (makemask.cpp:48-379,
 * WeightingScheme 0; IsKosher 383-414; FindBoundaryEdges, fpproc.cpp:5356-5415).
 *
 * xfk_mag_make_mask fixes nodal values by the reference's rules in its order, a
 * later rule overwriting an earlier one (free nodes -1): the ends of exterior
 * edges 0 (an edge no other element around its first node shares, the rings
 * of an air-gap element and periodic edges included; with an axisymmetric
 * selection touching r < 1e-6 only where IsKosher holds); the nodes of
 * selected elements 1 and of unselected elements that are not air 0, in
 * element order; a still-free node with a point property 0.  A block is not
 * air when mu_x != 1, mu_y != 1, BHpoints != 0, LamType != 0, H_c != 0,
 * J_re != 0, Cduct != 0 or block_not_air[block] != 0 (one byte per block, may
 * be NULL: the descriptor carries no hysteresis angles Theta_hn / hx / hy, a
 * caller who knows one to be non-zero says so here); a label in a circuit is
 * not air.  The reference matches the input geometry's points to mesh nodes
 * by their coordinates; here a node carries a point property when its
 * descriptor marker is >= 0.  An unselected element that is not air with a
 * node not fixed at 0 refuses the selection (XFK_ERR_ARG, the reference's
 * two-line message); the problem stays usable.  The Laplacian, weighted per
 * element by sqrt(label_max_area[label]) (sqrt of the element's area where that
 * is <= 0 or label_max_area is NULL), is formed in the problem's length units,
 * planar for both problem types, and solved by the AMG-PCG to the problem's
 * Precision on an auxiliary problem over the mesh's connectivity (no periodic
 * pairs, no air-gap elements, no circuits); the result is thresholded at 0.5.
 * A solve, xfk_mag_set_solution and a new xfk_mag_make_mask drop the mask.
 *
 * With the mask of the very selection passed, xfk_mag_block_integrals fills
 * and xfk_mag_block_integral answers, summed over ALL elements in a fixed
 * order (a call repeats bit for bit): 18 / 19 the x (r) / y (z) force, N;
 * 20 / 21 their "2x" parts, which the reference evaluates at Frequency 0 as
 * well; 22 / 23 the torque about the origin and its 2x part, N m.  18, 20, 22
 * and 23 are 0 on an axisymmetric problem.  Asked singly
 * (xfk_mag_block_integral), they are answered whatever the selected labels'
 * blocks are: the LamType > 2 and nonlinear-magnet refusals above concern the
 * energy integrals, which xfk_mag_block_integrals makes in the same pass.
 *
 * xfk_mag_get_mask: W[n_nodes] the solved values, msk[n_nodes] the 0 / 1 mask
 * (either may be NULL).  xfk_mag_mask_info: the layout of xfk_pot_mask_info.
 * xfk_mag_mask_problem: the auxiliary problem (owned by prob), for xfk_get_csr.
 * xfk_mag_stress_time: HIP-event ms of the launch of types 18-23 with its sum,
 * the median of `repeats` runs after a warm-up. */
int xfk_mag_make_mask(xfk_problem *prob, const unsigned char *label_selected, const double *label_max_area,
                      const unsigned char *block_not_air);
int xfk_mag_get_mask(xfk_problem *prob, double *W, double *msk);
int xfk_mag_mask_info(xfk_problem *prob, double *out9);
int xfk_mag_mask_problem(xfk_problem *prob, xfk_problem **aux);
int xfk_mag_stress_time(xfk_problem *prob, int repeats, double *ms);

/* Point values and contour integrals of a magnetostatic problem: fpproc's
 * GetNodalB (fpproc.cpp:2704-2967), GetPointValues with GetPointB (2257-2498,
 * 2669-2702) and LineIntegral (4094-4515) at Frequency 0, planar and
 * axisymmetric, in double in the reference's operation order.  Coordinates are
 * in the problem's length units.
 *
 * The element of a point is the lowest-numbered element whose InTriangleTest
 * (3387-3424) accepts it; the reference's InTriangle walks from the element of
 * its previous call and LineIntegral over the neighbours of the previous
 * sample's element, so the two differ only for a point exactly on an edge or a
 * node.  A point no element contains gets element -1 and NaN values.
 *
 * Refused before any launch, with the cause in xfk_last_error and the problem
 * left usable: a harmonic and a sharded problem; a problem holding a label
 * whose block has LamType > 2 (its fill factor, conductivity and energy need
 * GetFillFactor) or is a nonlinear permanent magnet (H_c != 0 with a B-H curve:
 * its energy needs fpproc's shifted curve and Nrg) -- for the whole problem,
 * wherever the points lie (XFK_ERR_UNSUPPORTED).  A static problem with
 * PrevType != 0 is refused when it is loaded, as in the reference.
 *
 * xfk_mag_corner_b: b[6 n_elems], GetNodalB of every element: (b1, b2) of its
 * corners 0, 1, 2.  Made at the first smoothed request and kept until a new
 * solution.  Two labels are the "same material" when they are the same label,
 * or their blocks' mu_x, mu_y, H_c and their directions are equal (mu_x, mu_y
 * as fpproc holds them after GetSlopes; two directions are equal when their
 * cosines and sines are).  A node carries a point current when its descriptor
 * marker names a point property with J != 0.
 * xfk_mag_point_values: n points; elem[n] out; out[13 n], per point
 *   0 A (the flux 2 pi r A when axisymmetric)   1 2  B1 B2, T
 *   3 4  mu1 mu2 (relative, divided by AECF)     5 6  H1 H2, A/m (less Hc)
 *   7 Js, MA/m^2   8 c, MS/m   9 E, J/m^3   10 11 Hc (re, im), A/m
 *   12 ff (1 in a wound label, else -1)
 * (Je, Ph and Pe are 0 at Frequency 0).  smooth != 0: B interpolated from the
 * corner values, else the element's.
 * xfk_mag_point_values_at: the same with elem[n] given (-1: none).
 * xfk_mag_line_integrals: the layout of xfk_pot_line_integrals; type 0 B.n (Wb,
 * and its average), 1 H.t (A, and its average), 2 length and area, 3 stress
 * tensor force (x, y; N; x is 0 when axisymmetric), 4 stress tensor torque
 * about the origin (N m; 0 on an axisymmetric problem, where the reference
 * multiplies by a depth that has no meaning), 5 (B.n)^2 and its average.
 * out[2 n_contours], missed[n_contours] (may be NULL): the samples no element
 * contains, which add nothing.  A contour has the same bits alone, in any
 * batch and on a second run.
 * xfk_mag_contour_samples: xy[2 ns], elem[ns] of one contour's samples
 * (ns = (n - 1) npts), for tests.
 * xfk_mag_point_time: HIP-event ms (medians of `repeats` runs after a warm-up)
 * of ms4[0] the corner kernel, [1] the cell grid, [2] [3] the point kernel on
 * the n points with smoothing off and on.  xfk_mag_contour_time: of the
 * contour kernel with its sums over the batch. */
int xfk_mag_corner_b(xfk_problem *prob, double *b);
int xfk_mag_point_values(xfk_problem *prob, int n, const double *x, const double *y, int smooth, int *elem,
                         double *out);
int xfk_mag_point_values_at(xfk_problem *prob, int n, const double *x, const double *y, const int *elem, int smooth,
                            double *out);
int xfk_mag_line_integrals(xfk_problem *prob, int n_contours, const int *ptr, const double *x, const double *y,
                           int type, int smooth, int npts, double *out, int *missed);
int xfk_mag_line_integral(xfk_problem *prob, int n, const double *x, const double *y, int type, int smooth, int npts,
                          double *out2, int *missed);
int xfk_mag_contour_samples(xfk_problem *prob, int n, const double *x, const double *y, int type, int npts,
                            double *xy, int *elem);
int xfk_mag_point_time(xfk_problem *prob, int n, const double *x, const double *y, int repeats, double *ms4);
int xfk_mag_contour_time(xfk_problem *prob, int n_contours, const int *ptr, const double *x, const double *y,
                         int type, int smooth, int npts, int repeats, double *ms);

/* Diagnostics of the AMG hierarchy (single device), for tests; not part of the
 * interface a caller should build on.  A probe holds one hierarchy built from
 * a host CSR (full symmetric, a diagonal in every row) with the options the
 * solver copies into it; XFK_ERR_UNSUPPORTED of the setup is passed on.
 * trace != 0 also keeps host copies of the setup's per-level scratch.
 * xfk_amg_probe_level_size / _level_csr: one operator of a level as the cycle
 * reads it -- sel XFK_AMG_A / _P / _R / _PF (P~) / _RF (R~); level 0 with
 * 16-bit tile columns returns the decoded columns unless XFK_AMG_PLAIN_COLS
 * is or'ed in, with f32 transfers R and P~ return the widened f32 values
 * unless XFK_AMG_F64_VALS is or'ed in.
 * xfk_amg_probe_tiles: tiles and int-fallback tiles of level 0's 16-bit form.
 * xfk_amg_probe_vector: XFK_AMG_DINV (n doubles), or XFK_AMG_DENSE, the n x n
 * operator the coarsest level applies, S M S as k_dense_mv composes it.
 * xfk_amg_probe_trace: XFK_AMG_TR_SFLAG (nnz bytes), _SDEG, _AGG, _AGG_PRE
 * (before the weak join), _ROOT (n ints each), _DFINV, _WF (n doubles), of a
 * level that was coarsened.
 * xfk_amg_probe_apply: U[:, k] = V-cycle(R[:, k]), nvec columns of n doubles
 * each stored one after the other.
 * xfk_amg_probe_refresh: new level-0 values (same pattern), Amg::refresh.
 * xfk_amg_probe_create takes the CSR under xfk_pcg_solve_csr's input contract
 * (below) and refuses what breaks it in the same way. */
typedef struct xfk_amg_probe xfk_amg_probe;
typedef struct {
    int sweeps;
    double theta, omega;
    int dense_max, fold, col16, f32, wlevel;
} xfk_amg_probe_opts;
typedef struct {
    int n, nc, fold, has16, has32, w_at;
    long long nnz, pnnz, fnnz;
    double weight, rho_f;       /* 1 / rho[0] (the smoother's weight) and rho[1] */
} xfk_amg_level_info;
typedef struct {
    int levels, dense_coarse, cinv_f64, traced;
    xfk_amg_level_info level[16];
} xfk_amg_info;
enum { XFK_AMG_A = 0, XFK_AMG_P = 1, XFK_AMG_R = 2, XFK_AMG_PF = 3, XFK_AMG_RF = 4,
       XFK_AMG_PLAIN_COLS = 16, XFK_AMG_F64_VALS = 32 };
enum { XFK_AMG_DINV = 0, XFK_AMG_DENSE = 1 };
enum { XFK_AMG_TR_SFLAG = 0, XFK_AMG_TR_SDEG = 1, XFK_AMG_TR_AGG = 2, XFK_AMG_TR_AGG_PRE = 3,
       XFK_AMG_TR_ROOT = 4, XFK_AMG_TR_DFINV = 5, XFK_AMG_TR_WF = 6 };
int xfk_amg_probe_create(int n, const int *rowptr, const int *col, const double *val, int device,
                         const xfk_amg_probe_opts *opts, int trace, xfk_amg_probe **out);
int xfk_amg_probe_info(xfk_amg_probe *probe, xfk_amg_info *info);
int xfk_amg_probe_level_size(xfk_amg_probe *probe, int level, int sel, int *rows, int *cols, long long *nnz);
int xfk_amg_probe_level_csr(xfk_amg_probe *probe, int level, int sel, int *rowptr, int *col, double *val);
int xfk_amg_probe_tiles(xfk_amg_probe *probe, int sel, int *tiles, int *wide);
int xfk_amg_probe_vector(xfk_amg_probe *probe, int level, int what, double *out);
int xfk_amg_probe_trace(xfk_amg_probe *probe, int level, int what, void *out);
int xfk_amg_probe_apply(xfk_amg_probe *probe, int nvec, const double *R, double *U);
int xfk_amg_probe_refresh(xfk_amg_probe *probe, const double *val, int fold);
void xfk_amg_probe_destroy(xfk_amg_probe *probe);

/* Device views for the bench / tests (stream-ordered on the problem's stream). */
int xfk_get_csr(xfk_problem *prob, int *rowptr, int *col, double *val, double *b);
/* The system of a Newton pass at a given iterate, without solving (a static
 * planar or axisymmetric problem).  V is npass x n_nodes, in the solver's own
 * unit (the V of b - K V: xfk_get_solution / c, axisymmetric: before the
 * 2 pi r factor).  The iteration-0 system is assembled from V = 0 as the first
 * pass of xfk_static2d does; then for k = 0 .. npass-1 row k of V is the
 * iterate of Newton pass k + 1, which reads the permeability state pass k
 * wrote.  npass == 0 gives the iteration-0 system.  xfk_get_csr then shows the
 * last pass's system and xfk_get_element_state the state it wrote.  Any
 * earlier solution is gone afterwards; a later xfk_static2d is unaffected.
 * XFK_ERR_ARG on a null, electrostatic, heat-flow, harmonic or mask problem,
 * XFK_ERR_UNSUPPORTED on a sharded one. */
int xfk_static2d_assemble_at(xfk_problem *prob, int npass, const double *V);
/* The per-element permeability state (mu1, mu2; n_elems each, the caller's
 * element order) the last pass wrote -- what the next pass would read.
 * XFK_ERR_ARG before the first pass and on a linear problem, which keeps no
 * state. */
int xfk_get_element_state(xfk_problem *prob, double *mu1, double *mu2);
long long xfk_get_nnz(xfk_problem *prob);
/* Column-index bytes per nonzero the last solve's PCG SpMV read: 2 with the
   AMG's 16-bit tile offsets (plus 2 for every nonzero of a tile whose columns
   span more than 65535), 4 without them; -1 for a null problem. */
double xfk_spmv_col_bytes(xfk_problem *prob);
int xfk_get_stream(xfk_problem *prob, void **hip_stream);

/* Stand-alone PCG on a host-supplied full symmetric CSR (testing the solver
 * alone, CBigLinProb::PCGSolve semantics with the device preconditioner).
 * V is the initial guess (used when flag != 0) and receives the solution.
 * Input contract, checked on the host before any device work: rowptr[0] == 0
 * and ascending, every column in [0, n), and no column twice in one row --
 * each is refused with XFK_ERR_ARG; a row without a diagonal entry is
 * XFK_ERR_SINGULAR.  The columns of a row may come in any order, with either
 * preconditioner.  The matrix is taken to be symmetric positive definite
 * (not checked).
 * iters is the index of the iteration whose test stopped the solve and er its
 * sqrt(r.M^-1 r / b.M^-1 b).  b == 0 returns at once (iters 0, er 0; V is 0
 * with flag == 0 and left as given otherwise), and so does an initial guess
 * whose residual is exactly zero (iters 0, er 0, V as given). */
int xfk_pcg_solve_csr(int n, const int *rowptr, const int *col, const double *val,
                      const double *b, double *V, int flag, double precision,
                      int device, long long *iters, double *er);
/* The same with a chosen preconditioner (XFK_PRECOND_*). */
int xfk_pcg_solve_csr_pc(int n, const int *rowptr, const int *col, const double *val,
                         const double *b, double *V, int flag, double precision,
                         int device, int precond, long long *iters, double *er);

/* Air-gap element matrix of one arc element (host math, no device needed):
 * MG (10 x 10, row-major) for the reduced ring shifts ci, co and
 * K = dr / (R dtheta), Ki = 1 / K.  Replaces the closed form of
 * cfemm/fsolver/static2d.cpp:209-263 (harmonic2d.cpp:245-300). */
int xfk_age_element_matrix(double ci, double co, double K, double Ki, double *MG);

/* Timing probe of the CG kernels (profiles / roofline): run `iters` PCG
 * iterations on the assembled system without a convergence stop; returns the
 * mean device time (ms) of the SpMV kernel and of one whole iteration. */
int xfk_pcg_time(xfk_problem *prob, int iters, double *ms_spmv, double *ms_iter);

/* Per-phase profile of a solved static problem (single device, AMG
 * preconditioner): with XFK_PROFILE_SETUP the AMG hierarchy is rebuilt for the
 * assembled matrix, then `iters` PCG iterations run without a convergence stop;
 * every phase -- setup steps per level, each V-cycle launch per level, the
 * PCG SpMV and update -- is bracketed by HIP events on the problem's stream.
 * Phases come back in first-seen order, aggregated by name: launches, total
 * device time, algorithmic bytes per launch (0 where the phase is not a
 * streaming kernel).  *count = phases written (<= cap). */
typedef struct {
    char name[64];
    int calls;
    double ms_total;
    double bytes_per_call;
} xfk_phase;
enum { XFK_PROFILE_SETUP = 1 };
int xfk_phase_profile(xfk_problem *prob, int iters, int flags, xfk_phase *out, int cap, int *count);

/* Diagnostics: device allocations of the library since the last reset, process
 * wide -- out[0] hipMalloc calls, out[1] their host ms, out[2] hipFree calls,
 * out[3] their host ms (a hipFree waits for the device).  Blocks served from
 * the process cache (what destroyed problems returned: xfk_problem_destroy
 * keeps their device blocks for the next problem of the process) are not
 * counted.  reset != 0 zeroes the counters after reading. */
int xfk_alloc_stats(double *out4, int reset);

/* Device memory of one problem (diagnostics): out4[0] bytes of the arena
 * chunks it holds, out4[1] their count, out4[2] bytes carved and live,
 * out4[3] bytes freed by its solves and kept for reuse by the next ones.  A
 * problem solved repeatedly stays at the footprint of its largest solve. */
int xfk_problem_memory(const xfk_problem *prob, long long *out4);
/* The process-wide caches a destroyed problem leaves for the next one: device
 * blocks (at most XFK_POOL_CAP_MB, default 64 GiB), pinned host buffers (at
 * most XFK_PIN_CAP_MB, default 1 GiB) and idle streams.  xfk_cache_stats:
 * out3[0] cached device bytes, out3[1] cached pinned bytes, out3[2] idle
 * streams.  xfk_release_cache gives all of them back to HIP (live problems
 * keep theirs). */
int xfk_cache_stats(long long *out3);
int xfk_release_cache(void);

/* AMG hints across problems (no reference counterpart: the reference rebuilds
 * nothing on the device).  The last single-device AMG setup of the process
 * leaves its SpGEMM slot capacities, MIS-2 round counts and coarsest
 * nested-dissection plan behind, keyed by the fine level's rows and nonzeros;
 * the next fresh problem of that size takes them as speculation checked on
 * the device (a capacity must be the class a measurement would pick, the plan
 * must match the coarsest pattern -- else that part is measured and redone),
 * so answers are bit-identical with or without them.  xfk_amg_forget_hints
 * drops them (XFK_AMG_NO_FOREIGN=1 never keeps any). */
int xfk_amg_forget_hints(void);

/* FEASolver::SortElements (cfemm/libfemm/cuthill.cpp:39-86; called from
 * FSolver::Cuthill) on the device: the reference's comb sort -- gap * 10 / 13
 * (9, 10 -> 11), swap on a strictly greater score, stop after the first pass
 * without a swap or after the first gap-1 pass (`while ((gap > 1) && (i > 0))`,
 * so the result need not be fully sorted) -- of the elements by
 * score[i] = p0 + p1 + p2 of element i, every pass simulated: the reference's
 * order, equal scores included.  perm[k] = the element at position k after
 * the sort. */
int xfk_sort_elements(int n_elems, const unsigned *score, int device, int *perm);

/* Magnetisation-direction function of a block label, evaluated for elements
 * as the reference's element loop does (FSolver::Static2D,
 * cfemm/fsolver/static2d.cpp:509-583; StaticAxisymmetric staticaxi.cpp:350-406):
 * the centroid of element i (nodes p[3i..3i+2], coordinates x, y in cm)
 * in drawing units gives x y r z theta R, and t[i] is the real part of the
 * last value `fctn` returns, in degrees (mag_dir when it returns nothing).
 * The chunk runs on a native restatement of the reference's Lua 4
 * interpreter (complex numbers; the base, string and math libraries; tables,
 * closures, LuaInstance's Complex and pi; xfk_lua.h lists what is refused),
 * one interpreter for all n_elems elements in order, globals persisting from
 * one to the next; errors carry the reference's messages ("Lua error occurred
 * when evaluating: ...", "... does not evaluate to a numerical value").
 * Host only: no device is needed. */
int xfk_magdir_eval(const char *fctn, int n_elems, const int *p, const double *x, const double *y,
                    int length_units, double mag_dir, double *t);

/* A whole problem's element loop (what xfk_problem_create runs): element i
 * runs its label lbl[i]'s function fctns[lbl[i]] (NULL or "": the label's
 * mag_dirs[lbl[i]], nothing run) on ONE interpreter, in element order, as the
 * reference's one Lua state per FSolver does; `axisymmetric` selects
 * staticaxi.cpp's chunk (r and z set first).  `repeats` != 0: the problem is
 * nonlinear, whose Newton loop re-runs the element loop every pass
 * (static2d.cpp:997-1008) -- refused (XFK_ERR_ARG, "not supported") when a
 * chunk changed state a later pass would see or left values on the stack. */
/* A whole Lua chunk on a fresh interpreter of the kind MagDirFctn runs on (a
 * femmcli-style script: the reference's LuaInstance, LuaInstance.cpp:185-208,
 * through lua_dostring): what print / write send to the standard output is
 * returned in out (NUL-terminated, at most cap - 1 bytes; *out_len the full
 * length).  0; -2 when the chunk raised a Lua error (syntax or run-time), -1
 * for a construct the interpreter refuses.  Host only. */
int xfk_lua_run(const char *chunk, char *out, long long cap, long long *out_len);

int xfk_magdir_eval_labels(int n_labels, const char *const *fctns, const double *mag_dirs, int n_elems,
                           const int *p, const int *lbl, const double *x, const double *y, int length_units,
                           int axisymmetric, int repeats, double *t);

#ifdef __cplusplus
}
#endif
#endif
