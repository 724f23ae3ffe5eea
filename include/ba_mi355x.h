/*
 * ba_mi355x.h -- C ABI of libba_mi355x.so: the MI355X (gfx950) Levenberg-Marquardt bundle-adjustment hot path
 * behind the executable / solver-symbol interface of jasvob/BundleAdjustment_Benchmarks.
 *
 * The reference has no FFI: its one seam is `lm.minimize(params)` called from main()
 * (src/bundle_adjustment_large.cpp:130-165) plus the functor calls the LM classes make
 * (src/Eigen_ext/BacktrackLevMarqQRChol.h:213,216-217,257,264,365,368).  Each entry point below names the
 * reference interface it replaces.  Plain pointers and sizes only; no torch / HIP types in signatures
 * (streams travel as void*).
 *
 * All functions return 0 (BA_OK) on success or a BA_ERR_* code; nothing throws across the boundary.
 * A handle is not thread-safe; one host thread drives one solver (the reference is single-threaded).
 */
#ifndef BA_MI355X_H
#define BA_MI355X_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- codes ------------------------------------------------------------------------------------------- */

/* ReturnCodes of the reference executable (bundle_adjustment_large.cpp:26-31) + library errors. */
enum {
    BA_OK = 0,
    BA_ERR_USAGE = 1, /* WrongInputParams */
    BA_ERR_FILE = 2,  /* WrongInputFile   */
    BA_ERR_PARSE = 3, /* new: the reference does not check stream errors */
    BA_ERR_ARG = 4,
    BA_ERR_HIP = 5,   /* HIP runtime error or no gfx950 device: the product path never falls back to a CPU */
    BA_ERR_NOMEM = 6,
    BA_ERR_COMM = 7,
    BA_ERR_SINGULAR = 8 /* ba_solver_covariance_compute: J'J + lambda I is not positive definite on the free parameters */
};

/* Solver symbols of the reference build (src/CMakeLists.txt:95-178; src/Optimization/BAFunctor.h:98-117).
 * BA_MOREQR (src/Eigen_ext/BacktrackLevMarqMore.h): two QR factorisations per step -- J once per outer iteration,
 * [R ; sqrt(lambda) I] per trial -- and lambda0 = 1e-6 * max column norm of J.  Both are QR all the way (:288-345): per-point
 * Householder QRs for the point columns, dense Householder QRs for the camera columns (J2bot(lambda = 0) per outer iteration,
 * [rows left by the per-point 6 x 3 QRs ; R22 ; sqrt(lambda) I] per trial) -- no normal equations; needs (6 M + 2 D)(D + 1) scalars
 * of device memory (BA_ERR_NOMEM beyond).  Environment BA_MOREQR_QR=0 at solver creation: the right block by LDL^T of the reduced
 * camera system instead (rounds 1 - 3's variant). */
/* BA_QRSPQR (SuiteSparseQR on the whole [J ; sqrt(lambda) I], BAFunctor.h:113-116, bundle_adjustment_large.cpp:151-157, README.md:17;
 * the library itself is absent): a sparse QR of this matrix under a fill-reducing column ordering eliminates the 3-column point
 * blocks first and is left with one dense front, J2bot -- which is the factorisation the QRKIT path performs, so the symbol runs
 * that path (per-point Householder QR, dense Householder QR of J2bot); same LM loop as QRKIT (Eigen::BacktrackLevMarq).  The
 * equivalence is tested against a whole-matrix Householder QR with no block elimination (tests: test_qrspqr_against_the_whole_matrix_qr).
 * Sharded (shard_world > 1), BA_QRKIT and BA_QRSPQR keep their dense QR: every shard factors its own rows of J2bot, the exchange step
 * sums a zeroed stack into which each shard has put its D x D triangle R (+ the head of Q^T rhs, g_c, energy), and the QR of the stack
 * runs redundantly (distributed TSQR) -- never the normal equations these symbols exist to avoid. */
/* BA_ITERSCHUR (no reference counterpart, no parity claim with any reference trajectory): CHOLESKY's linearisation and point elimination,
 * then the reduced camera system S dx_c = rhs -- the same S and rhs CHOLESKY assembles, lambda on the diagonal -- solved by block-Jacobi
 * preconditioned conjugate gradients from dx_c = 0, with products by S computed from the elimination's records and S never formed.  A
 * step is inexact: the iteration stops at |rhs - S dx_c| <= rel_tol |rhs| (recurrence residual) or after max_iter iterations
 * (ba_solver_set_pcg; defaults BA_PCG_MAX_ITER_DEFAULT, BA_PCG_REL_TOL_DEFAULT), or, when asked for, once the model decrease has
 * converged (ba_solver_set_pcg_model_tol).  The LM loop is CHOLESKY's; its rhoScale dx'(lambda dx + g) is the model decrease of the
 * truncated step up to rounding, since an early PCG iterate from dx_c = 0 is orthogonal to its residual (ba_solver_set_pcg_model_tol
 * says how far that holds for a long solve).  Device memory O(K + 81 N) (ba_solver_device_bytes), no D x D
 * matrix and none of the dense symbols' limits on N or K; single shard only (shard_world > 1: BA_ERR_ARG).  BA_GET_S: BA_ERR_ARG. */
typedef enum { BA_QRKIT = 0, BA_QRCHOL = 1, BA_CHOLESKY = 2, BA_MOREQR = 3, BA_QRSPQR = 4, BA_ITERSCHUR = 5 } ba_solver_kind;

/* `typedef double Scalar;` / `typedef float Scalar;` (src/BATypeUtils.h:6-7). */
typedef enum { BA_F64 = 0, BA_F32 = 1 } ba_scalar;

/* BacktrackLevMarq*Info::Status (BacktrackLevMarqQRChol.h:39-46, BacktrackLevMarqCholesky.h:27-34). */
typedef enum {
    BA_NOT_STARTED = -2,
    BA_RUNNING = -1, /* also returned when the max_trials extension stopped the loop */
    BA_SUCCESS = 0,
    BA_EXCEEDED_LAMBDA_MAX = 1,
    BA_TOO_MANY_FUN_EVALS = 2,
    BA_MAX_ITERS = 3
} ba_status;

/* statusToString (BacktrackLevMarqQRChol.h:48-63). */
const char *ba_status_string(int status);
const char *ba_error_string(int err);

/* ---- problem: BAL loader (bundle_adjustment_large.cpp:59-107) ------------------------------------------ */

typedef struct ba_problem ba_problem;

/* Parses `N M K`, K x `cam pt u v`, 9N camera scalars (omega(3), T(3), f, k1, k2), 3M point scalars.
 * BA_ERR_FILE if the file cannot be opened (reference: "Cannot open <path>", exit 2). */
int ba_problem_load_bal(const char *path, ba_problem **out);
/* Same problem from caller-owned arrays (copied). meas is 2K interleaved (u,v); cams9 is 9N; pts is 3M. */
int ba_problem_create(int N, int M, int K, const int *cam_idx, const int *pt_idx, const double *meas,
                      const double *cams9, const double *pts, ba_problem **out);
/* Seeded synthetic BAL problem with exactly (N, M, K) (stand-in for the data files missing from the reference
 * checkout and for the 1024-camera scaling config; generator described in DESIGN.md). mean_obs is informative only. */
int ba_problem_synthetic(int N, int M, int K, unsigned long long seed, ba_problem **out);
int ba_problem_save_bal(const ba_problem *p, const char *path);
/* Binary cache of a parsed problem (`ifstream >>` / strtod parsing of a 280 MB text file takes seconds; the
 * cache is the same arrays, little-endian, behind a 32-byte header) -- an extension, the BAL text format stays the interface. */
int ba_problem_save_cache(const ba_problem *p, const char *path);
int ba_problem_load_cache(const char *path, ba_problem **out);
void ba_problem_free(ba_problem *p);
int ba_problem_dims(const ba_problem *p, int *N, int *M, int *K);
/* Copies out the arrays (any pointer may be NULL). */
int ba_problem_get(const ba_problem *p, int *cam_idx, int *pt_idx, double *meas, double *cams9, double *pts);

/* Host-only view of the static structure ba_solver_create would build for shard `rank` of `world` (no GPU needed):
 * out8 = {p0, p1, o0, o1, entries, chunks, camera pairs, input_was_sorted_by_point}.  Points are split into contiguous
 * ranges balanced by observation count; entries are the (point, camera pair) contributions to the reduced matrix. */
int ba_shard_plan(const ba_problem *p, int shard_rank, int shard_world, long long *out8);

/* ---- solver: device-resident LM state ------------------------------------------------------------------ */

typedef struct ba_solver ba_solver;

/* LMParams + Lambda (BacktrackLevMarqQRChol.h:124-146).  max_trials / verbose are extensions (0 = reference). */
typedef struct {
    double lambda_min;           /* 1e-10 */
    double lambda_max;           /* 1e10  */
    double lambda_decrease;      /* 10 (unused by the reference loop) */
    double lambda_increase_base; /* 2     */
    double lambda_init;          /* 1e-3 (overwritten by 1e-12*max diag(J'J) at iteration 1; BA_DAMP_MARQUARDT: lambda0 itself) */
    double tol_fun;              /* 1e-8  */
    int max_iter;                /* 1e6   */
    int max_fun_ev;              /* 1e6   */
    int max_trials;              /* extension: stop after this many table rows (0 = unlimited) */
    int verbose;                 /* print the reference's iteration table to stdout */
} ba_lm_params;
void ba_lm_params_default(ba_lm_params *p);

typedef struct {
    int status;          /* ba_status */
    int iterations;      /* outer iterations started */
    int trials;          /* table rows (accepted + rejected) */
    int fun_evals;
    double energy;       /* m_energy at exit */
    double lambda;
    double seconds;      /* wall time of minimize */
    double schur_ms;     /* mean device time per trial of elimination + Schur assembly + reduced solve + back-substitution */
    double linearize_ms; /* mean device time per outer iteration of residual + Jacobian + gradient */
} ba_result;

/* One row of the reference's table (outputIter, BacktrackLevMarqQRChol.h:84-93): f is the energy BEFORE the step. */
typedef void (*ba_trial_cb)(void *user, int iter, int accepted, double f, double rho, double lambda, double elapsed_s);

/* A collective on `count` scalars of type `scalar` in DEVICE memory across the ranks that shard one problem, in place; called on
 * the host thread between kernels, `stream` is the hipStream_t the solver enqueues on (the callback must order itself against
 * that stream).  op (low byte; round 4 added the last two for the distributed factor, BA_DIST_FACTOR):
 *   BA_OP_SUM / BA_OP_MAX    all-reduce;
 *   BA_OP_BCAST | root << 8  broadcast of dev_buf[0 .. count) from rank `root`;
 *   BA_OP_REDUCE_SCATTER     dev_buf holds shard_world chunks of `count` scalars; on return chunk `shard_rank` of THIS rank's buffer
 *                            is the sum over the ranks of their chunk `shard_rank` (ncclReduceScatter's in-place form; the other
 *                            chunks are unspecified).
 * A transport supplied by the host layer -- used by the gloo tests; the production transport is RCCL inside the library
 * (ba_solver_comm_init: ncclAllReduce / ncclBroadcast / ncclReduceScatter).  Never called when shard_world == 1. */
#define BA_OP_SUM 0
#define BA_OP_MAX 1
#define BA_OP_BCAST 2
#define BA_OP_REDUCE_SCATTER 3
typedef int (*ba_allreduce_fn)(void *user, void *dev_buf, size_t count, int scalar, int op, void *stream);

/* ---- communication of a sharded solve (no reference counterpart: the reference is one process) ------------------------- */

/* RCCL inside the library.  ba_comm_unique_id: rank 0 creates the 128-byte id of a new communicator (ncclGetUniqueId); the host
 * layer carries it to the other ranks (torch.distributed / MPI / a file: ba_comm_id_via_file); then EVERY rank of the shard
 * group calls ba_solver_comm_init (collective: ncclCommInitRank with the solver's shard_rank / shard_world, on the solver's
 * device).  From then on the per-trial all-reduces of the packed reduced camera system and of the step scalars are
 * ncclAllReduce calls on the solver's stream, enqueued by ba_minimize without a host synchronisation. */
#define BA_COMM_ID_BYTES 128
int ba_comm_unique_id(void *id_out /* BA_COMM_ID_BYTES */);
/* Rendezvous through a file for processes started by hand: rank 0 removes whatever an earlier run left at `path`, creates the id and
 * publishes it (O_EXCL temporary file, mode 0600, atomic rename); the others wait up to BA_COMM_WAIT_S (60) seconds for a file that
 * belongs to THIS launch: the nonce of the environment variable BA_COMM_NONCE when the launcher sets one; else a file written after
 * the reader's PROCESS start (library load, less two seconds) at once, an older one only after it has stayed unchanged for
 * BA_COMM_GRACE_S (5) seconds -- this launch's rank 0 would have removed a dead run's leftover at its own start.  ba_comm_id_file_done: call after ba_solver_comm_init has returned (it is collective: every rank has the id
 * by then); rank 0 removes the file, so that no id outlives its launch. */
int ba_comm_id_via_file(const char *path, int rank, void *id_out);
int ba_comm_id_file_done(const char *path, int rank);

/* Replaces the construction of BAFunctor + the LM object (bundle_adjustment_large.cpp:117-131): copies the problem
 * to HBM in SoA layout, builds the static camera-pair structure.  Points (and their observations) are partitioned
 * into shard_world contiguous ranges balanced by observation count; this handle owns range shard_rank.
 * device < 0 keeps the current HIP device. Fails with BA_ERR_HIP when no GPU is present, with BA_ERR_ARG when a QR symbol
 * meets a point with more than 1024 observations (the per-point QR keeps a track in registers; CHOLESKY and BA_ITERSCHUR have no
 * limit), with BA_ERR_ARG for BA_ITERSCHUR with shard_world > 1 and for a dense symbol with N > 65 535 cameras (host side, before any
 * device allocation). */
int ba_solver_create(const ba_problem *p, ba_solver_kind kind, ba_scalar scalar, int device, int shard_rank,
                     int shard_world, ba_solver **out);
void ba_solver_free(ba_solver *s);
int ba_solver_set_allreduce(ba_solver *s, ba_allreduce_fn fn, void *user); /* host-language transport (gloo tests); RCCL: next line */
int ba_solver_comm_init(ba_solver *s, const void *id /* BA_COMM_ID_BYTES, from ba_comm_unique_id on rank 0 */);
/* Enqueue on a caller-owned hipStream_t (e.g. torch's current stream) instead of the solver's own stream. */
int ba_solver_set_stream(ba_solver *s, void *hip_stream);
/* Point range [p0,p1) and observation range [o0,o1) owned by this shard. */
int ba_solver_shard(const ba_solver *s, int *p0, int *p1, int *o0, int *o1);

/* lm.minimize(params) (bundle_adjustment_large.cpp:134,141,162): runs the LM loop of the solver symbol on the GPU,
 * parameters stay resident and are updated in place (quirk kept: the flat-line exit happens before x = xTest). */
int ba_minimize(ba_solver *s, const ba_lm_params *lm, ba_trial_cb cb, void *user, ba_result *out);

/* Step-level seam = what the LM classes call on the functor / solver, for parity tests and external LM drivers:
 *   linearize : m_functor(x, r); energy; m_functor.df(x, J); JtRes; column norms (BacktrackLevMarqQRChol.h:257-280)
 *   try_step  : m_solver.compute ... dx; xTest = x (+) dx; m_functor(xTest); rhoScale (BacktrackLevMarqQRChol.h:291-375)
 *   accept    : x = xTest (BacktrackLevMarqQRChol.h:428) */
int ba_solver_linearize(ba_solver *s, double *energy, double *diag_max);
int ba_solver_try_step(ba_solver *s, double lambda, double *energy_test, double *rho_scale, double *dx_norm);
int ba_solver_accept(ba_solver *s);
/* Utils::showErrorStatistics + showObjective (Utils.h:15-68) on the resident parameters:
 * out4 = {mean reprojection error, inlier mean error, nInliers, "True objective"}. */
int ba_solver_stats(ba_solver *s, double *out4);

/* Copy device arrays to the host as doubles (own shard only for per-observation / per-point arrays). */
typedef enum {
    BA_GET_RESIDUALS = 0, /* 2K  obs-major interleaved, order of the input file */
    BA_GET_JC = 1,        /* 18K per obs 2x9 row-major, columns [T, omega, f, k1, k2] */
    BA_GET_JP = 2,        /* 6K  per obs 2x3 row-major */
    BA_GET_GRAD = 3,      /* 3M+9N  = -J'r, points first */
    BA_GET_S = 4,         /* D*D column-major reduced camera matrix (full symmetric) of the last try_step (BA_ITERSCHUR: none) */
    BA_GET_RHS = 5,       /* D reduced right-hand side (BA_ITERSCHUR: always kept) */
    BA_GET_DX = 6,        /* 3M+9N step of the last try_step */
    BA_GET_CAMS = 7,      /* 15N  R(9 row-major), T(3), f, k1, k2 */
    BA_GET_POINTS = 8,    /* 3M */
    BA_GET_CAMS_TEST = 9,
    BA_GET_POINTS_TEST = 10
} ba_get_what;
int ba_solver_get(ba_solver *s, int what, double *out, size_t n);
/* Keep a copy of the reduced camera matrix / rhs of each try_step before it is factored in place, so that
 * BA_GET_S / BA_GET_RHS can return it (parity tests; costs one D x D device copy per trial). */
int ba_solver_keep_intermediates(ba_solver *s, int on);
/* Overwrite the resident parameters x (cam15: 15N, pts: 3M of this shard, file order). */
int ba_solver_set_state(ba_solver *s, const double *cam15, const double *pts);

/* Per-phase device time (ms, HIP events on the solver's stream) accumulated since the last reset. */
typedef struct {
    double linearize_ms;  /* residual + Jacobian + gradient / J_c^T J_c, per outer iteration */
    double eliminate_ms;  /* per-point elimination (3x3 LDL^T or Householder QR) */
    double schur_ms;      /* reduced camera matrix assembly (BA_ITERSCHUR: preconditioner + reduced rhs) */
    double factor_ms;     /* dense LDL^T + triangular solves (BA_ITERSCHUR: the PCG solve) */
    double backsub_ms;    /* point back-substitution + retraction */
    double test_eval_ms;  /* residual at xTest + scalar reductions */
    double comm_ms;       /* device time of the all-reduces (HIP events around them on the solver's stream) */
    double trial_ms;      /* whole trial, device time (the only per-trial figure when the trial is replayed as hipGraphs) */
    long long n_linearize, n_trials, n_graph_trials;
} ba_timing;
int ba_solver_timing(ba_solver *s, ba_timing *out, int reset);

/* Bench hooks: replay one phase `reps` times on the solver's stream and return the mean device ms per launch
 * (HIP events on that stream).  phase: 0 residual eval, 1 residual+Jacobian, 2 point elimination,
 * 3 Schur assembly, 4 Schur assembly + dense factor + solve, 5 back-substitution + retraction,
 * 6 dense factorisation only, 7 backward sweep only (6 / 7 rebuild S untimed before every repetition).
 * BA_ITERSCHUR: 4 = preconditioner + rhs + the PCG solve; 3, 6 and 7 return BA_ERR_ARG (there is no S); with a forest
 * preconditioner in force 9 = the edge blocks S_ab alone (BA_PRECOND_VISIBILITY_FOREST), 10 = the forest's factor alone (B_a
 * rebuilt untimed before every repetition); BA_ERR_ARG without one.  11 = k_jg of ba_solver_dogleg_prepare alone (BA_ERR_ARG unless a
 * prepare has been made on the linearisation in place; it leaves that prepare valid). */
int ba_solver_time_phase(ba_solver *s, int phase, int reps, double lambda, double *ms_per_launch);

/* A hand-off between workgroups of one launch that times out (the fused factorisation's row flag, the one-launch back sweep's
 * sentinel: waits bounded by design) does not end ba_minimize: the trial is repeated -- and the run continued -- with one launch per
 * step, where nobody waits for anybody; a second failure returns BA_ERR_HIP.  ba_solver_recoveries counts such repeats.
 * ba_minimize gives up with BA_ERR_HIP when no LM row appears for BA_WATCHDOG_S seconds (default 600): it does NOT wait for the
 * stream then, the handle is dead (every later call returns BA_ERR_HIP, ba_solver_free releases no device memory) and a retry
 * belongs in a fresh process.  BA_ERR_COMM: the shards of a sharded solve took different accept / stop decisions (guard slot of the
 * scalar all-reduce). */
int ba_solver_recoveries(const ba_solver *s);

/* Test hook for the failure paths of the in-launch hand-offs (no reference counterpart).  which = 2: arms a fault -- the row
 * workgroups of the fused factorisation stay silent and the panel's wait is short -- so that the next ba_minimize meets the
 * time-out on its first trial and has to recover (returns BA_ERR_ARG when the reduced system is a single block column).
 * which = 3: arms a 4-second kernel in front of the next LM trial (with BA_WATCHDOG_S = 1 ba_minimize must give up).  which = 1: runs the one-launch
 * backward sweep with the workgroup at the head of its dependency chain missing and a short spin bound, so the others
 * wait for unknowns that are never published.  Returns what the production path returns for that: BA_ERR_HIP (the kernels
 * raise a device error word that is read back with the trial's scalars); BA_ERR_ARG when the reduced system has fewer than
 * four 64-wide block columns (a single group has nobody to wait for). */
int ba_solver_selftest(ba_solver *s, int which);

/* ---- BA_ITERSCHUR (no reference counterpart) ---------------------------------------------------------------------------------- */

/* Defaults of a new BA_ITERSCHUR solver (profiles/r05_iterschur_*.txt: the measurements behind them). */
#define BA_PCG_MAX_ITER_DEFAULT 100
#define BA_PCG_REL_TOL_DEFAULT 1e-6
/* max_iter >= 1 iterations at most per trial, stop at |r| <= rel_tol |rhs| (0 < rel_tol < 1).  Every iteration slot is enqueued (four
 * launches; those behind convergence return at once), so max_iter bounds the launches of a trial too.  BA_ERR_ARG for another kind
 * or a bad value. */
int ba_solver_set_pcg(ba_solver *s, int max_iter, double rel_tol);
/* Counted on the device by every solve (try_step, and every trial of ba_minimize up to the row that ends the run): solves, iterations
 * summed over them; of the last solve its iterations, whether it met rel_tol, and |rhs - S dx_c| / |rhs| of its step (recomputed
 * with one more product by S, not the recurrence's residual).  reset != 0 clears the counters after reading them.  BA_ERR_ARG for
 * another kind. */
typedef struct {
    long long solves, total_iters;
    int last_iters, last_converged;
    double last_rel_residual;
} ba_pcg_stats;
int ba_solver_pcg_stats(ba_solver *s, ba_pcg_stats *out, int reset);
/* The model-decrease stopping rule of truncated Newton methods (Nash and Sofer; Ceres' ITERATIVE_SCHUR stops on it by default; DESIGN.md
 * section 20).
 * eta = 0: off, a new solver's setting.  0 < eta < 1: a trial's solve ALSO stops at the head of iteration k >= 1 when
 *   zeta_k = k (s_k - s_{k-1}) / s_k < eta,   s_k = x_k'(rhs + r_k) = -2 Q(x_k),  s_0 = 0,
 * with Q(x) = x'Sx / 2 - x'rhs the model the reduced system minimises.  The residual rule and the cap of ba_solver_set_pcg stay in
 * force; whichever holds first ends the solve (residual tested first).  s_k <= 0 or not finite: the rule does not fire.
 * s_k is summed in fp64 for both scalar types from x_k, rhs and the recurrence's r_k as they are stored (with shared intrinsics all three
 * are in range(Pi), so the same sum holds).  Takes effect at the next ba_solver_try_step / ba_minimize; drops the captured trial graph like
 * ba_solver_set_pcg; leaves the linearisation and a pending step alone.  Legal for both scalar types and with every other setting of a
 * BA_ITERSCHUR solver.  With eta = 0 the solver enqueues the launches and returns the bits of one that never had the rule.
 * With the rule on, ba_pcg_stats.last_iters is the k at which the solve stopped and last_converged is 1 when either rule stopped it;
 * last_rel_residual keeps its meaning, the true residual of the returned step -- which is now often well above rel_tol: the rule exists to
 * stop a solve whose model decrease is complete while its residual is not small.  The LM loop's rhoScale dx'(lambda dx + g) is the
 * model decrease of such a step up to rounding (x_k is orthogonal to r_k), so the gain ratio is not degraded by it.  The orthogonality is
 * a property of early iterates: CG loses it geometrically with k in any arithmetic (measured in long double: |x_k'r_k| / s_k <= 7e-18 up
 * to the rule's stop at eta = 0.01, 1e-4 by k = 81 on problem-21 at lambda = 1e-12 max diag J'J), so a long solve ended by the residual
 * rule returns a rhoScale that is off by that share.
 * ba_solver_covariance_pcg does not use the rule (a covariance column is a linear solve, not a Newton step); ba_solver_time_phase(4) uses
 * the rule in force.
 * Memory: the first call with eta > 0 allocates one more list of block partials, 3 * ceil(N / 256) * 8 bytes, kept until the solver is
 * freed and counted by ba_solver_device_bytes.
 * BA_ERR_ARG, solver unchanged: another kind than BA_ITERSCHUR; eta < 0, eta >= 1 or not finite. */
int ba_solver_set_pcg_model_tol(ba_solver *s, double eta);
/* Which rule ended the solves made with eta > 0 (a solve with eta = 0 runs the kernels of a solver without the rule and leaves these
 * alone), counted like ba_pcg_stats: trials that ba_minimize enqueued behind the row that ended a run are not counted.  A solve that
 * reaches max_iter with |r| <= rel_tol there counts as ended by the residual.  reset != 0 clears all six after reading them.
 * BA_ERR_ARG for another kind. */
typedef struct {
    long long by_residual, by_model, at_cap; /* solves ended by each, since the last reset */
    int last_rule;                           /* 0 cap, 1 residual, 2 model */
    double last_zeta, last_model;            /* zeta_k and s_k at the last solve's final iterate (k >= 1; else 0) */
} ba_pcg_stop_stats;
int ba_solver_pcg_stop_stats(ba_solver *s, ba_pcg_stop_stats *out, int reset);
/* Sum of the handle's device allocations in bytes (every kind; the buffers a sharded solve allocates on its first trial included once
 * they exist). */
int ba_solver_device_bytes(const ba_solver *s, size_t *bytes);

/* ---- parameters held constant (no reference counterpart; Ceres' constant parameter blocks, g2o's fixed vertices) ------------------- */

/* Bit q of a camera mask word = camera parameter q, in the order of the camera block of BA_GET_JC / BA_GET_DX / BA_GET_GRAD. */
#define BA_FIX_T          0x007u /* T0 T1 T2 (bits 0..2, each on its own) */
#define BA_FIX_OMEGA      0x038u /* w0 w1 w2 (bits 3..5, all three or none) */
#define BA_FIX_POSE       0x03Fu
#define BA_FIX_INTRINSICS 0x1C0u /* f k1 k2 (bits 6..8, each on its own) */
#define BA_FIX_CAMERA     0x1FFu
/* Removes the masked parameters from the optimisation, every kind, both scalar types, sharded or not: J's columns of a fixed parameter
 * are zero (BA_GET_JC / BA_GET_JP / BA_GET_GRAD return zeros there; every other column is the unmasked solver's, bit for bit), and so is
 * everything built from J -- S, rhs, lambda0 = 1e-12 max diag J'J, MOREQR's column norms, rho, the stop tests.  The damping stays
 * lambda I (a fixed row of S is lambda alone; the reduced system keeps D = 9N).  The step of a fixed parameter is exactly 0 (BA_GET_DX)
 * and its value keeps its bits through try_step, accept and ba_minimize (a camera whose omega is fixed keeps all 9 entries of R).
 * cam_mask: N words (NULL = none); pt_fixed: M bytes of the PROBLEM, problem order, != 0 = the point's 3 coordinates fixed (NULL = none;
 * a shard reads its own range [p0, p1)).  Masks that are NULL or all zero restore the unmasked path exactly.  The mask takes effect at
 * the next ba_solver_linearize or ba_minimize; a ba_solver_try_step before that returns BA_ERR_ARG.  BA_ERR_ARG, the solver unchanged:
 * bits above 8, omega partly fixed, every parameter fixed. */
int ba_solver_set_constant(ba_solver *s, const unsigned short *cam_mask, const unsigned char *pt_fixed);
/* Host only (no GPU): ORs into cam_mask (N words) a mask that fixes the 7-dimensional similarity gauge of J'J -- BA_FIX_POSE on camera
 * ref_cam, and for the scale one component k of T_b of the camera b whose centre C_b = -R_b^T T_b lies farthest from C_ref (lowest index
 * on a tie), k = argmax |(T_b + R_b C_ref)_k| (dT_b / ds under a scaling about C_ref; lowest k on a tie).  R = Rodrigues(omega) as the
 * solver initialises it.  BA_ERR_ARG for N < 2 or ref_cam out of range. */
int ba_problem_gauge_mask(const ba_problem *p, int ref_cam, unsigned short *cam_mask);

/* ---- covariance blocks (no reference counterpart; Ceres' Covariance, g2o's computeMarginals) ---------------------------------------- */

/* With J the Jacobian of the last ba_solver_linearize (robustified, weighted residuals e of the measurement model in force, masked columns
 * zero), F the set of free parameters and H = (J'J + lambda I) restricted to F:   Sigma = H^-1 on F x F, exactly 0 in every row and column
 * of a fixed parameter.  Sigma is in the solver's own tangent parametrisation (camera block in the order of BA_GET_DX: T, omega, f, k1, k2;
 * point block x, y, z).  With BA_LOSS_TRIVIAL and weights w_o = 1 / sigma_o (ba_solver_set_loss, ba_solver_set_obs_weights; sigma_o the
 * standard deviation of observation o in pixels, per coordinate) J'J is the information matrix of the measurements and Sigma simply the
 * covariance of the estimate -- nothing is left to scale.  Under a robust loss (the default psi included) Sigma is the Gauss-Newton
 * covariance of the robustified problem: the inverse of J'J for e = sqrt(rho(s) / s) r, i.e. for unit variance of e, in which an
 * observation beyond the loss's scale counts for little (psi: for nothing).  lambda = 0 is the meaningful value once the gauge is
 * fixed (ba_problem_gauge_mask); lambda > 0 gives the damped inverse.  Any loss and any weights are accepted.
 * compute: assembles S(lambda) from the current linearisation as a trial does, factors the symmetrically scaled matrix
 * diag(S)^-1/2 S diag(S)^-1/2 (fixed rows: unit diagonal) by the dense LDL^T with the scaling stacked below it, and forms the inverse
 * of the free block on the device.  BA_CHOLESKY and BA_QRCHOL, BA_F64, shard_world == 1; anything else BA_ERR_ARG, as are lambda < 0 or
 * not finite, no ba_solver_linearize since creation / ba_solver_set_state / ba_minimize, and a mask or a measurement model set since the
 * last linearisation.
 * BA_ERR_SINGULAR, no result left behind: a pivot <= 0 of S or of a free point's 3 x 3 block (lambda = 0 without a gauge mask, a
 * parameter nobody observes) -- found on the device, a flag word read back with the call.  x, xTest, the linearisation and the mask are
 * untouched: a ba_solver_try_step or ba_minimize behind it returns the bits it returns without it, and behind a ba_solver_try_step the
 * step (BA_GET_DX), the kept S / rhs (BA_GET_S, BA_GET_RHS), xTest and ba_solver_accept are what they were.  What a compute does spend
 * is internal: the last trial's elimination records and the factored S, which every trial rebuilds.
 * Memory: one buffer of its own, allocated by the first compute, counted by ba_solver_device_bytes, released by ba_solver_free:
 *   8 (ldc (Dp + 128) + 4096 ceil(D / 64) + 4 Dp + 128) + 4 bytes,  D = 9 N, Dp = 64 ceil((D + 3) / 64), ldc = 64 ceil((Dp + D + 3) / 64) + 64
 * (the inverse rides the factorisation as D extra rows: ~2 D x D scalars).  BA_ERR_NOMEM when it does not fit, the solver stays usable. */
int ba_solver_covariance_compute(ba_solver *s, double lambda);
/* Blocks of the last computed covariance.  cam_pairs: n_pairs x (a, b) -> 81 doubles each, row-major block Sigma_ab (Sigma_ba is its
 * transpose bit for bit); pt_ids: n_pts points in the PROBLEM's numbering -> 9 doubles each, computed on the device for these points
 * only (O(t^2) 9 x 9 blocks for a track of t observations).  Either list may be empty.  BA_ERR_ARG: no successful compute yet, or a
 * ba_solver_linearize / ba_solver_accept / ba_solver_set_state / ba_solver_set_constant / ba_solver_set_loss / ba_solver_set_obs_weights /
 * ba_minimize since (the result is stale), an index out of range.  A ba_solver_try_step in between does not invalidate the result. */
int ba_solver_covariance_get(ba_solver *s, int n_pairs, const int *cam_pairs, double *cam_cov, int n_pts, const int *pt_ids, double *pt_cov);
/* Device ms (HIP events): ms4 = {elimination + assembly of S + staging, factorisation, inverse from the factor} of the last compute and
 * the point kernel of the last ba_solver_covariance_get that asked for points. */
int ba_solver_covariance_timing(ba_solver *s, double *ms4);

/* ---- covariance blocks of BA_ITERSCHUR: matrix-free, by a multi-column PCG ---------------------------------- */

/* The contract of ba_solver_covariance_compute / _get above -- blocks of Sigma = (J'J + lambda I)^-1 on the free parameters at the last
 * ba_solver_linearize, exactly 0 in the rows and columns of fixed parameters, the order of BA_GET_DX -- for the one kind that never
 * forms S, solved inexactly and in one call.  Sigma_cc = S^-1, so Sigma_ab is rows a of the solution of S X = E_b (9 columns), and
 * Sigma_pp = U_p^-1 + Y_p' S^-1 Y_p with Y_p = W_p U_p^-1 (3 columns).  The columns are solved nine at a time by preconditioned conjugate
 * gradients whose product by S reads every elimination record once for all nine (csrc/ba_pcg_multi.hip.h).
 * Right-hand sides: a pair (a, b) is served from column block max(a, b), so Sigma_ab and Sigma_ba of one call are each other's transpose
 * bit for bit; pairs with the same column block share one solve; a diagonal block and a point block are returned symmetrised,
 * (X + X') / 2; points are packed three to a batch; the column of a fixed parameter is not solved (a fully fixed camera or a fixed point:
 * zeros without a launch); a point nobody observes returns I / lambda, or BA_ERR_SINGULAR at lambda = 0.  Every sum has a fixed order that
 * involves the column's own data only, and there are no atomics: a block's bits do not depend on what else is in the request.
 * Operator: S(lambda) of the current linearisation (the elimination is run again at this lambda; priors are in V and U0, the relative-pose
 * blocks H_ab are applied per column); the row of a fixed parameter is the identity.  Preconditioner: block Jacobi at this lambda, B_a
 * inverted in fp64, whatever ba_solver_set_preconditioner holds (that setting is left alone).
 * max_iter = 0 / rel_tol = 0: the values of ba_solver_set_pcg.  A column stops at |r_k| <= rel_tol |b| (the recurrence's residual, as in a
 * trial's solve) or at max_iter.  A column that ends at the cap is no error: BA_OK, and stats->unconverged counts such columns.
 * Accuracy per column: |x - S^-1 b|_2 <= |S^-1|_2 |b - S x|_2, and stats->worst_rel_residual is the largest |b - S x| / |b| (|b| = 1 for a
 * camera column), from one more product by S behind each batch.
 * BA_ERR_SINGULAR (device flags read back with the call; the output arrays are then unspecified): a pivot <= 0 of a free point's 3 x 3
 * block, a B_a that is not positive definite (the trial's fallback to the block's diagonal would hide a rank defect), p'Sp <= 0 or not
 * finite for a live column.  NOT detected: an S that is merely semidefinite (lambda = 0 without a gauge) whose Krylov spaces never show
 * it -- such a solve ends as `unconverged` with a large residual, so look at the stats.
 * BA_ERR_ARG, decided on the host before any launch, the solver unchanged: a kind other than BA_ITERSCHUR, BA_F32, no ba_solver_linearize
 * since creation / ba_solver_set_state / ba_minimize, a mask or a measurement model set since the last linearisation, lambda < 0 or not
 * finite, max_iter < 0, rel_tol outside [0, 1), an index out of range, a negative count, a NULL array with a positive count.
 * The LM state is untouched, as with ba_solver_covariance_compute: a ba_solver_try_step or ba_minimize behind the call returns the bits it
 * returns without it; behind a ba_solver_try_step, BA_GET_DX, BA_GET_RHS, xTest and ba_solver_accept are what they were, and
 * ba_solver_pcg_stats does not count these solves.  What the call spends are the last trial's elimination records (the fused
 * linearisation's pre-made ones included) and scratch every trial rebuilds.
 * Memory: work vectors of its own, allocated by the first call, counted by ba_solver_device_bytes, released by ba_solver_free:
 *   8 (6 * 81 N + 27 max(M, 1) + 81 max(chunks, 1) + 81 N + 27 ceil(N / 28)) + sizeof(state) bytes
 * (x, r, z, p, S p and the right-hand sides at 9 columns x 9 N; the point pass; the slab of the camera chunks of <= 32 observations;
 * B_a^-1; three lists of workgroup partials), plus 12 n_pairs + 24 + 8 (81 n_pairs + 9 n_pts + 1) bytes for the length of the call.
 * BA_ERR_NOMEM when they do not fit; the solver stays usable. */
typedef struct {
    long long columns, batches, total_iters; /* live right-hand sides solved; 9-column batches; sum over batches of the batch's iterations */
    int max_iters, unconverged;              /* slowest column; columns that ended at the cap */
    double worst_rel_residual;               /* max over columns of |b - S x| / |b|, from one more product by S behind each batch */
    double ms;                               /* device ms of the call (HIP events) */
} ba_cov_pcg_stats;
int ba_solver_covariance_pcg(ba_solver *s, double lambda, int max_iter, double rel_tol, int n_pairs, const int *cam_pairs, double *cam_cov,
                             int n_pts, const int *pt_ids, double *pt_cov, ba_cov_pcg_stats *stats /* may be NULL */);

/* ---- measurement model (no reference counterpart beyond its psi; Ceres' LossFunction, g2o's robust kernels and information) ---------- */

/* With r_o = w_o (pi(cam, pt) - meas_o) the weighted reprojection residual of observation o in pixels (w_o = 1 without weights) and
 * s = |r_o|^2, the solver minimises sum_o rho(s_o):
 *   BA_LOSS_REFERENCE  psi(s) = s (2 - s / tau^2) / 4 below tau^2, tau^2 / 4 above (BAFunctor.h:147); scale = tau.  A new solver is
 *                      (BA_LOSS_REFERENCE, 0.5): INLIER_THRESHOLD of bundle_adjustment_large.cpp:36, chosen for the BAL "-pre" files
 *   BA_LOSS_TRIVIAL    s: plain least squares; scale is ignored
 *   BA_LOSS_HUBER      s for s <= delta^2, 2 delta sqrt(s) - delta^2 above; scale = delta > 0
 *   BA_LOSS_CAUCHY     c^2 log(1 + s / c^2); scale = c > 0
 * the way the reference does for psi: the residual handed to LM is e_o = g r_o, g = sqrt(rho(s) / s), and J is the full derivative of e,
 *   de/dr = g (I - rh rh') + (rho'(s) sqrt(s) / sqrt(rho(s))) rh rh',  rh = r / sqrt(s)
 * (finite and continuous at s = 0, where g = sqrt(rho'(0)); BA_LOSS_TRIVIAL and Huber's quadratic part are e = r, de/dr = I exactly), so
 * that sum e^2 = sum rho.  Every kind, both scalar types, sharded or not.  Everything built from e and J follows: S, rhs, lambda0, MOREQR's
 * column norms, rho, the stop tests, the mask of ba_solver_set_constant (masked columns of the new J are zero), BA_ITERSCHUR's operator,
 * the covariance.  BA_GET_RESIDUALS returns e.  ba_solver_stats keeps its meaning: the reference's statistics of the UNWEIGHTED pixel
 * errors with the reference's threshold 0.5, whatever the model.
 * w: K weights of the PROBLEM, in the order of the input file (NULL = none; a shard reads those of its own observations, and the solver
 * applies its own observation order to them -- unsorted input included); copied.
 * Either call takes effect at the next ba_solver_linearize or ba_minimize; a ba_solver_try_step before that returns BA_ERR_ARG, and a
 * computed covariance becomes stale.  ba_solver_set_loss(BA_LOSS_REFERENCE, 0.5) together with ba_solver_set_obs_weights(NULL) restores
 * the default path bit for bit.  BA_ERR_ARG, the solver unchanged: an unknown kind; a scale <= 0, NaN or infinite (in the solver's scalar
 * type) for a kind that uses it; a weight that is not finite or <= 0. */
typedef enum { BA_LOSS_REFERENCE = 0, BA_LOSS_TRIVIAL = 1, BA_LOSS_HUBER = 2, BA_LOSS_CAUCHY = 3 } ba_loss_kind;
int ba_solver_set_loss(ba_solver *s, int kind, double scale);
int ba_solver_set_obs_weights(ba_solver *s, const double *w /* K of the PROBLEM, file order; NULL = none */);

/* ---- Gaussian priors (no reference counterpart; Ceres' residual blocks on one parameter block, g2o's unary edges) --------------------- */

/* Soft constraints on the parameters themselves: the solver minimises  sum_o rho(|r_o|^2) + sum_priors |e|^2  -- priors carry no robust
 * loss -- with, in the units of BA_GET_CAMS / BA_GET_POINTS (the solver's own parametrisation: f, k1, k2 as the solver holds them after
 * the load-time scaling, f = -f_file, k1 = k1_file f^2, k2 = k2_file f^4),
 *   point       e = L (X_p - X0)                              3 rows, Jacobian L on the point's columns
 *   centre      e = L (C_a - C0),  C_a = -R_a^T T_a           3 rows, Jacobian L [-R^T | -R^T [T]x | 0 0 0] on the camera's columns
 *                                                             (T, omega, f, k1, k2), for the retraction T + dT, R <- Rodrigues(d omega) R
 *   intrinsics  e_q = w_q (x_q - x0_q),  q in (f, k1, k2)     up to 3 rows, Jacobian w_q on column 6 + q; w_q = 0: no row for q
 * L: any real 3 x 3, row-major (usually the upper Cholesky factor of the inverse covariance; diag(1 / sigma) for independent axes).
 * Prior rows are rows of J like any other: they enter J'J (U of the point, the camera's 9 x 9 block), g = -J'e (BA_GET_GRAD), the
 * energy that ba_solver_linearize, ba_solver_try_step and the LM table report, lambda0 = 1e-12 max diag J'J, rho and the stop tests, S,
 * rhs, BA_ITERSCHUR's operator and preconditioner, and the covariance (ba_solver_covariance_compute(s, 0) of a problem whose gauge the
 * priors fix is BA_OK).  BA_GET_RESIDUALS / BA_GET_JC / BA_GET_JP stay the 2K observation rows, ba_solver_stats keeps its meaning.
 * With ba_solver_set_constant the prior's columns of a fixed parameter are zero like every other column of J; a prior whose parameters
 * are all fixed is a constant in the energy.
 * ids: n indices of the PROBLEM, each at most once; x0 / c0: 3n; sqrt_info: 9n; w: 3n; copied.  n = 0 removes the priors of that type;
 * with all three removed the solver runs the path without priors again, bit for bit.  A call takes effect at the next
 * ba_solver_linearize or ba_minimize; a ba_solver_try_step before that returns BA_ERR_ARG, and a computed covariance becomes stale.
 * BA_CHOLESKY and BA_ITERSCHUR (they share the point elimination, for which a prior is an addition to blocks that already exist),
 * BA_F64 and BA_F32, shard_world == 1.  With priors set every trial runs the point elimination as a launch of its own (the fused
 * linearisation eliminates the next trial's points before a prior could join them: those records are not used).
 * BA_ERR_ARG, the solver unchanged: another kind (the QR kinds would need extra rows in the per-point QR and in J2bot: not built), a
 * sharded solver (not built), an index out of range or listed twice, a value that is not finite (in the solver's scalar type), n < 0,
 * a NULL array with n > 0. */
int ba_solver_set_point_priors(ba_solver *s, int n, const int *pt_ids, const double *x0, const double *sqrt_info);
int ba_solver_set_centre_priors(ba_solver *s, int n, const int *cam_ids, const double *c0, const double *sqrt_info);
int ba_solver_set_intrinsics_priors(ba_solver *s, int n, const int *cam_ids, const double *x0, const double *w);
/* out3 = energy of the point, centre and intrinsics priors at x of the last linearisation (sum of e^2, each group; zeros without
 * priors).  BA_ERR_ARG: another kind, sharded, no linearisation, or a model set since the last one. */
int ba_solver_prior_energy(ba_solver *s, double *out3);

/* ---- Relative-pose constraints between camera pairs (no reference counterpart; Ceres' residual blocks on two pose blocks, g2o's
 * EdgeSE3): a rig's calibrated extrinsic, odometry between consecutive frames, a turntable's known rotation ------------------------- */

/* For a constraint between cameras a and b (x_cam = R X + T) the pose of a's frame seen from b's is
 *   R_ab = R_b R_a^T,   t_ab = T_b - R_ab T_a          (x_b = R_ab x_a + t_ab; both invariant under a rigid motion of the world)
 * and the constraint adds six rows to J, without a robust loss, like the priors:
 *   e_t = L_t (t_ab - t0)                              3 rows
 *   e_r = L_r phi,  phi = Log(R_ab R0^T)               3 rows (rotation vector, |phi| < pi; its accuracy degrades like eps / (pi - |phi|))
 * L_t = sqrt_info_trans, L_r = sqrt_info_rot: any real 3 x 3, row-major; all zero: no rows of that kind.  The solver minimises
 *   sum_o rho(|r_o|^2) + sum_priors |e|^2 + sum_constraints (|e_t|^2 + |e_r|^2).
 * Jacobian on the pose columns (T, omega) of the two cameras for the retraction T + dT, R <- Rodrigues(d omega) R (intrinsics columns 0),
 * with u = R_ab T_a and Jl^-1 = I - [phi]x / 2 + c [phi]x^2, c = 1 / theta^2 - (1 + cos theta) / (2 theta sin theta):
 *   d e_t / d(T_a, omega_a) = L_t [-R_ab | -R_ab [T_a]x]      d e_t / d(T_b, omega_b) = L_t [I | [u]x]
 *   d e_r / d(T_a, omega_a) = L_r [  0   | -Jl^-1 R_ab  ]      d e_r / d(T_b, omega_b) = L_r [0 | Jl^-1]
 * These rows enter J'J (the 9 x 9 blocks of both cameras AND the block between them -- also for a pair that shares no point), g = -J'e
 * (BA_GET_GRAD), the energy that ba_solver_linearize, ba_solver_try_step and the LM table report, lambda0, rho and the stop tests, S
 * (BA_GET_S with ba_solver_keep_intermediates), rhs, BA_ITERSCHUR's operator and preconditioner, and the covariance.  BA_GET_RESIDUALS /
 * BA_GET_JC / BA_GET_JP stay the 2K observation rows.  With ba_solver_set_constant the columns of a fixed parameter are zero; a
 * constraint whose two poses are fixed is a constant in the energy.  May be combined with priors, any loss and weights.
 * cam_pairs: 2n indices (a, b) of the PROBLEM; R0: 9n row-major; t0: 3n; sqrt_info_rot, sqrt_info_trans: 9n each; copied.  n = 0 removes
 * the constraints and the solver runs the path without them again, bit for bit.  A call takes effect at the next ba_solver_linearize or
 * ba_minimize; a ba_solver_try_step before that returns BA_ERR_ARG, and a computed covariance becomes stale.
 * BA_CHOLESKY and BA_ITERSCHUR, BA_F64 and BA_F32, shard_world == 1.
 * BA_ERR_ARG, the solver unchanged: another kind (the QR kinds would need rows that span two camera blocks in J2bot: not built), a
 * sharded solver (not built), a == b or an index out of range, an unordered pair listed twice, a value that is not finite (in the
 * solver's scalar type), an R0 that is no rotation (max |R0 R0^T - I| > 1e-6 or det <= 0), n < 0, a NULL array with n > 0. */
int ba_solver_set_relative_poses(ba_solver *s, int n, const int *cam_pairs /* 2n: a, b */, const double *R0 /* 9n row-major */,
                                 const double *t0 /* 3n */, const double *sqrt_info_rot /* 9n */, const double *sqrt_info_trans /* 9n */);
/* out2 = {sum |e_r|^2, sum |e_t|^2} at x of the last linearisation (zeros without constraints).  BA_ERR_ARG: another kind, sharded, no
 * linearisation, or a model set since the last one. */
int ba_solver_relative_pose_energy(ba_solver *s, double *out2);

/* ---- BA_ITERSCHUR's preconditioner ----------------------------------------------------------------------
 * BA_PRECOND_BLOCK_JACOBI: M = blockdiag(B_a), B_a = V_a + lambda I - the self entries (the constraints' H_aa / H_bb are in V_a).
 * BA_PRECOND_CONSTRAINT_FOREST: M = blockdiag(B_a) + the cross blocks H_ab (6 x 6, pose corner) of a spanning forest of the
 * constraint graph, both triangles.  The forest: the constraints in list order through a union-find, one kept when it joins two
 * components and the merged one has at most max_tree cameras (the others keep their diagonal blocks in B_a only); a tree's root is
 * its lowest camera, its nodes in breadth-first order from the root (neighbours in list order), eliminated in the reverse of that
 * order.  On a forest the block LDL^T has no fill: factored once per trial (fp64 for both scalar types), applied by two sweeps per
 * PCG iteration, one wavefront per tree.  A tree with a pivot block that is not positive definite in working precision uses the
 * block-Jacobi inverses of its cameras for that solve.
 * BA_PRECOND_VISIBILITY_FOREST (Kushal and Agarwal's visibility-based preconditioning, what Ceres calls
 * CLUSTER_TRIDIAGONAL): M = blockdiag(B_a) + the whole off-diagonal blocks S_ab (9 x 9) of the reduced camera matrix on a spanning
 * forest of the co-visibility graph, both triangles.  The forest is the rule above on the list L = the solver's relative-pose pairs
 * in list order, then ba_problem_covisibility's pairs (weight descending): a greedy maximum-weight forest by shared points behind the
 * constraints.  S_ab = - sum over the common points p, o in a at p, o' in b at p, of Z_o diag(dinv_p) Z_o'^T (+ H_ab of a constraint
 * on that pair, pose corner) is computed once per trial from the elimination's records, S never formed, and kept in fp64.  This M is
 * NOT guaranteed positive definite; a tree with a pivot block that is not positive definite runs that solve on the block-Jacobi
 * inverses of its cameras and is counted (fallback_trees). */
/* (2 is not a kind and stays refused with BA_ERR_ARG, as it was before the visibility forest existed: callers and tests that probe
 * for an unknown kind with it keep their behaviour) */
typedef enum { BA_PRECOND_BLOCK_JACOBI = 0, BA_PRECOND_CONSTRAINT_FOREST = 1, BA_PRECOND_VISIBILITY_FOREST = 3 } ba_precond_kind;
/* The default max_tree: the largest tree measured (profiles/r12_forest_measure.txt).  On an odometry chain the whole chain in one tree
 * gave the fewest ms per trial at 257 and at 1024 cameras; a tree's factor and sweeps are sequential and grow linearly with its cameras. */
#define BA_PCG_MAX_TREE_DEFAULT 1024
/* The default max_tree of BA_PRECOND_VISIBILITY_FOREST: the setting with the fewest ms per trial at synthetic(70 000, 280 000, 1.12 M)
 * among 4, 8, 16, 64 and 256 (profiles/r13_visibility_measure.txt: 48.3 ms at 4, 66.0 at 8, 193.4 at 256; block Jacobi 44.8).  No
 * setting beat block Jacobi there; larger trees needed MORE iterations on that problem, whose camera pairs share one or two points. */
#define BA_PCG_VIS_MAX_TREE_DEFAULT 4
/* BA_ITERSCHUR only.  max_tree: cameras per tree at most (>= 1; 0 = BA_PCG_MAX_TREE_DEFAULT, BA_PCG_VIS_MAX_TREE_DEFAULT for the
 * visibility forest).  Takes effect at the next
 * try_step / ba_minimize; drops the captured trial graph like ba_solver_set_pcg.  A new solver uses BA_PRECOND_BLOCK_JACOBI; a forest
 * without a kept constraint (no constraints, max_tree = 1) runs the block-Jacobi launches and returns their bits.
 * ba_solver_set_relative_poses behind this call rebuilds the forest.  BA_ERR_ARG, solver unchanged: another solver kind, an unknown
 * kind, max_tree < 0. */
int ba_solver_set_preconditioner(ba_solver *s, int kind, int max_tree);
/* out6 = {kind, max_tree in force, trees with >= 2 cameras, kept constraints, dropped constraints, cameras of the largest tree}
 * (BA_PRECOND_VISIBILITY_FOREST: kept and dropped count the entries of L);
 * *fallback_trees (may be NULL): trees of the last solve that fell back to block Jacobi.  BA_ERR_ARG for another solver kind. */
int ba_solver_preconditioner_info(ba_solver *s, long long *out6, int *fallback_trees);
/* Host only (no GPU), the forest rule above on a bare pair list (a pair may occur more than once): parent[N] (-1: root or lone
 * camera), via[N] (constraint index of the edge to the parent, -1), order[N] (elimination order, tree after tree by ascending root,
 * lone cameras last by index), kept[n] (0/1).  BA_ERR_ARG: a == b, an index out of range, max_tree < 1, N < 0, n < 0, a NULL array. */
int ba_relpose_forest_plan(int N, int n, const int *cam_pairs, int max_tree, int *parent, int *via, int *order, unsigned char *kept);
/* Host only (no GPU): the co-visibility graph of a problem.  The weight of a camera pair (a < b) is the number of points that put it
 * together: a point seen by t <= track_max distinct cameras adds 1 to each of its t (t - 1) / 2 pairs, a longer track only to the
 * t - 1 pairs of cameras adjacent in ascending camera index (which bounds the work on long tracks); a camera that sees a point twice
 * counts once.  track_max = 0: BA_VIS_TRACK_MAX_DEFAULT.  Constant-parameter masks play no part.  Call with pairs = NULL for the count
 * *n_pairs, then with pairs[2 n] and weight[n]: ordered by (weight descending, a ascending, b ascending), whatever the order of the
 * problem's observations.  BA_ERR_ARG: a NULL problem or n_pairs, track_max < 0, one of pairs / weight NULL and the other not. */
#define BA_VIS_TRACK_MAX_DEFAULT 64
int ba_problem_covisibility(const ba_problem *p, int track_max, long long *n_pairs, int *pairs, int *weight);

/* ---- shared intrinsics for BA_ITERSCHUR (no reference counterpart; Ceres' one intrinsics parameter block handed to many residual
 * blocks): one physical camera behind many frames, the heads of a rig ------------------------------------ */

/* Host only (no GPU): the groups and chunks ba_solver_set_shared_intrinsics builds from one label per camera.  group_of[a] < 0: camera a
 * keeps its own intrinsics; equal labels >= 0 form a group; a label used once is no group.  Groups are numbered by their lowest member,
 * a group's members ascend; chunks hold at most `chunk` members (>= 1; the solver uses 256), never span groups and run in group order.
 *   *n_groups, group_ptr[n_groups + 1], members[group_ptr[n_groups]]           the members of group g: members[group_ptr[g] .. group_ptr[g + 1])
 *   *n_chunks, chunk_ptr[n_chunks + 1], chunk_group[n_chunks]                  chunk c: members[chunk_ptr[c] .. chunk_ptr[c + 1]) of chunk_group[c]
 * Every output pointer may be NULL (call with the arrays NULL for the counts; N / 2 + 1, N, N + 1 and N entries always suffice).
 * BA_ERR_ARG: N < 0, a NULL group_of with N > 0, chunk < 1. */
int ba_intrinsics_group_plan(int N, const int *group_of, int chunk, int *n_groups, int *group_ptr, int *members, int *n_chunks, int *chunk_ptr,
                             int *chunk_group);
/* The cameras of a group solve for ONE f, k1, k2.  BA_ITERSCHUR, BA_F64 and BA_F32.  The unknowns keep their layout (D = 9 N): with P
 * (9N x n_free) the matrix that copies a group's three intrinsics to rows 6..8 of each member, the step is dx_c = P y with
 *   (P'SP) y = P' rhs,      S and rhs exactly what BA_ITERSCHUR solves without groups (lambda I inside S),
 * computed as CG for Pi S on range(Pi), preconditioned by Pi M^-1, where Pi = P (P'P)^-1 P' replaces rows 6..8 of every member by the
 * group's mean and M is the preconditioner in force (all three kinds of ba_solver_set_preconditioner are legal).  Nothing else changes:
 * the linearisation, the point elimination, the back-substitution, the retraction and the LM control are the ungrouped solver's.
 * Damping: lambda P'P, that is lambda n_g on the shared parameter of a group of n_g cameras -- Marquardt's damping of the stacked
 * columns.  lambda0 = 1e-12 max diag J'J keeps its per-camera-column definition.  Under BA_DAMP_MARQUARDT (ba_solver_set_damping) the
 * same projected PCG implies lambda P'D P: lambda sum over the members a of D_a,q on a group's parameter q, Marquardt's damping of the
 * unknown itself.
 * What a caller sees: BA_GET_DX rows 6..8 are bit-equal inside a group, so f, k1, k2 of the members stay bit-equal through
 * ba_solver_try_step, ba_solver_accept and ba_minimize; BA_GET_RHS returns Pi rhs; ba_solver_pcg_stats keeps its meaning with the
 * residual |Pi (rhs - S dx_c)| / |Pi rhs|; BA_GET_GRAD, BA_GET_JC and the energy are per camera as before.  Priors, relative poses,
 * losses, weights and masks are rows and columns of the same J: an intrinsics prior on one member acts on the shared parameter.
 * group_of: N labels as for ba_intrinsics_group_plan (copied).  NULL, all negative, or no label used twice: no groups, and the solver
 * enqueues the launches and returns the bits of one that never had any.  Takes effect at the next ba_solver_try_step / ba_minimize (the
 * linearisation is untouched: no ba_solver_linearize needed); drops the captured trial graph like ba_solver_set_preconditioner.  A
 * step that is pending is dropped, as ba_solver_set_state drops it: xTest belongs to the other group set, so ba_solver_accept returns
 * BA_ERR_ARG until the next ba_solver_try_step.  BA_ERR_NOMEM: the host or device lists do not fit, the solver unchanged.  The
 * chunk lists and partials are device buffers counted by ba_solver_device_bytes: 44 bytes per chunk slot (the chunks, plus at most 7
 * empty slots in front of a group of 257 .. 2048 cameras), 4 per grouped camera, 4 per chunk of a group above 2048 cameras.
 * BA_ERR_ARG, the solver unchanged: another kind; members of a group whose f, k1, k2 in the resident state (read back at the call, in
 * the solver's scalar type) are not bit-equal -- equalise them with ba_solver_set_state first; members of a group that do not carry the
 * same bits 6..8 of the ba_solver_set_constant mask in force.
 * With groups in force, BA_ERR_ARG and nothing changed: ba_solver_set_state with unequal members; ba_solver_set_constant with intrinsics
 * bits that differ inside a group; ba_solver_covariance_pcg (the covariance under groups is not built).
 * Not built: a preconditioner that couples a group's pose blocks to its one intrinsics block (the arrowhead P'BP), the dense kinds,
 * sharded solvers. */
int ba_solver_set_shared_intrinsics(ba_solver *s, const int *group_of /* N, or NULL = none */);
/* out4 = {groups, grouped cameras, cameras of the largest group, chunks}.  BA_ERR_ARG for another solver kind. */
int ba_solver_shared_intrinsics_info(ba_solver *s, long long *out4);

/* ---- Marquardt's damping (no reference counterpart; Ceres' min_lm_diagonal / max_lm_diagonal, Marquardt 1963) -- */

/* BA_DAMP_IDENTITY: every trial solves (J'J + lambda I) dx = -J'e, as the reference does; a new solver's kind.
 * BA_DAMP_MARQUARDT: a trial solves (J'J + lambda D) dx = -J'e, D diagonal, D_ii = min(max((J'J)_ii, diag_min), diag_max), J'J that of the
 * last linearisation with every row and column of J in it: loss and weights, priors, the relative-pose blocks H_aa, the zero columns of
 * masked parameters.  The point block is U_p + lambda D_p, the reduced system S = (V + lambda D_c) - sum Z diag(dinv) Z', and the model
 * decrease the LM control divides by is rhoScale = dx'(lambda D dx + g).  lambda is dimensionless and the step is invariant under a
 * change of units of any parameter (while no clamp bites).
 * Rounding: d_i = fl(lambda clamp(diag_i)) in the solver's scalar type is formed first and then added exactly where lambda is added
 * under BA_DAMP_IDENTITY, in the same order of additions.
 * diag_min / diag_max: 0 = BA_DAMP_DIAG_MIN_DEFAULT / BA_DAMP_DIAG_MAX_DEFAULT; 0 < diag_min <= diag_max, both finite in the solver's
 * scalar type.  A fixed parameter (ba_solver_set_constant) has diagonal 0, so D = diag_min there, its row of S is lambda diag_min alone,
 * its step exactly 0 and its value keeps its bits.  A point nobody observes gets lambda diag_min and no step.
 * BA_CHOLESKY and BA_ITERSCHUR, BA_F64 and BA_F32, shard_world == 1; combines with masks, losses, weights, priors, relative poses, every
 * preconditioner and shared intrinsics.  With shared intrinsics the projected PCG is unchanged, so the damping of a group's parameter q
 * is lambda P'D P = lambda sum over the members a of D_a,q -- Marquardt's damping of the unknown itself.
 * A call takes effect at the next ba_solver_try_step / ba_minimize (the linearisation does not depend on the damping: no
 * ba_solver_linearize needed), drops the captured trial graphs like ba_solver_set_pcg, and leaves a pending step acceptable.
 * ba_minimize under BA_DAMP_MARQUARDT starts from lambda0 = lm.lambda_init (NOT overwritten by 1e-12 max diag J'J); lambda_min,
 * lambda_max, the accept / rho / flat-line control and the table are unchanged.  ba_solver_time_phase uses the damping in force.  With
 * BA_DAMP_MARQUARDT the fused linearisation's pre-made elimination records (made at lambda I) are not used: every trial runs the point
 * elimination as a launch of its own, as with priors.
 * NOT affected: ba_solver_covariance_compute / ba_solver_covariance_pcg keep their own lambda with the meaning (J'J + lambda I)^-1
 * whatever damping is set.
 * BA_ERR_ARG, the solver unchanged, for BA_DAMP_MARQUARDT only: BA_QRKIT, BA_QRCHOL, BA_QRSPQR and BA_MOREQR (they put sqrt(lambda) rows
 * into the per-point QR and into J2bot: not built), a sharded solver (not built), bad bounds; and an unknown kind.
 * ba_solver_set_damping(s, BA_DAMP_IDENTITY, ...) is legal for every solver kind and shard count (the bounds are ignored); a solver
 * switched to Marquardt and back enqueues the launches and returns the bits of one that never was.  ba_solver_get_damping: every kind;
 * any pointer may be NULL; the bounds are those of the last accepted BA_DAMP_MARQUARDT call (the defaults before one). */
typedef enum { BA_DAMP_IDENTITY = 0, BA_DAMP_MARQUARDT = 1 } ba_damping_kind;
#define BA_DAMP_DIAG_MIN_DEFAULT 1e-6 /* Ceres' min_lm_diagonal */
#define BA_DAMP_DIAG_MAX_DEFAULT 1e32 /* Ceres' max_lm_diagonal */
int ba_solver_set_damping(ba_solver *s, int kind, double diag_min, double diag_max);
int ba_solver_get_damping(ba_solver *s, int *kind, double *diag_min, double *diag_max);

/* ---- Powell's dogleg: a second trust-region strategy for BA_CHOLESKY (no reference counterpart; Ceres' DOGLEG, g2o's
 * OptimizationAlgorithmDogleg, GTSAM's DoglegOptimizer) ---------------------------------------------------------- */

/* All vectors are in the solver's tangent parametrisation, in the order of BA_GET_DX.  With E = sum e^2 the energy, g = -J'e
 * (BA_GET_GRAD), H = J'J of the last ba_solver_linearize and the model E(x (+) dx) ~ E - 2 g'dx + dx'H dx, the predicted decrease of a
 * step is pred(dx) = 2 g'dx - dx'H dx (for an LM step: the rhoScale of ba_solver_try_step).  Once per linearisation, for a mu > 0:
 *   dx_gn solves (H + mu I) dx_gn = g              -- exactly the step of ba_solver_try_step(s, mu)
 *   dx_sd = alpha g,  alpha = |g|^2 / q,  q = |J g|^2   -- the Cauchy step
 * and the fp64 scalars g2 = |g|^2, q, gn2 = |dx_gn|^2, g_dot_gn = g'dx_gn are kept.  For a radius > 0 (infinity is legal) the step is
 * dx = a g + c dx_gn, chosen in this order:
 *   branch 0 (Gauss-Newton)     sqrt(gn2) <= radius                a = 0, c = 1
 *   branch 1 (scaled gradient)  else alpha sqrt(g2) >= radius      a = radius / sqrt(g2), c = 0
 *   branch 2 (interpolated)     else                               a = alpha (1 - beta), c = beta
 * beta in (0, 1] the root of |dx_sd + beta (dx_gn - dx_sd)| = radius: with A = gn2 - 2 alpha d + alpha^2 g2, B = alpha d - alpha^2 g2,
 * C = alpha^2 g2 - radius^2 (d = g_dot_gn), beta = (-B + sqrt(B^2 - A C)) / A when B <= 0 and -C / (B + sqrt(B^2 - A C)) otherwise.
 *   pred = 2 (a g2 + c d) - (a^2 q + 2 a c (g2 - mu d) + c^2 (d - mu gn2))           (H dx_gn = g - mu dx_gn)
 * g2 = 0: a = c = 0, branch 0, pred = 0.
 * ba_dogleg_coefficients: this rule, host only (no GPU).  Any output pointer may be NULL.  BA_ERR_ARG: a scalar that is not finite or
 * is negative, mu <= 0 or not finite, radius <= 0 or NaN, q <= 0 with g2 > 0. */
typedef struct { double mu, g2, q, gn2, g_dot_gn, alpha, energy_gn, rho_scale_gn; } ba_dogleg_info;
int ba_dogleg_coefficients(double g2, double q, double gn2, double g_dot_gn, double mu, double radius, double *a, double *c, int *branch,
                           double *pred);
/* ba_solver_dogleg_prepare: runs the trial segments of ba_solver_try_step(s, mu) unchanged -- BA_GET_DX, xTest, out->energy_gn and
 * out->rho_scale_gn are that call's bits, and a ba_solver_accept behind it takes the full Gauss-Newton step -- then keeps a copy of
 * dx_gn, forms g2, gn2, g_dot_gn (one launch, fused with the copy) and q (k_jg: one pass over J), all accumulated in fp64 for both
 * scalar types in a fixed order without atomics: the same bits on every run.  alpha = g2 / q (0 when g2 = 0).  `out` may be NULL.
 * The prepared state survives any number of ba_solver_try_dogleg and ba_solver_try_step calls; ba_solver_linearize, ba_solver_accept,
 * ba_solver_set_state, ba_minimize, ba_minimize_dogleg, ba_solver_set_constant, ba_solver_set_loss and ba_solver_set_obs_weights
 * make it stale, as they do a pending step or a computed covariance.
 * ba_solver_try_dogleg: the coefficients from the kept scalars by ba_dogleg_coefficients on the host, handed to the device as kernel
 * arguments in the solver's scalar type; one launch forms dx = a g + c dx_gn into the step buffers (BA_GET_DX returns the dogleg step)
 * and xTest = x (+) dx -- points by addition, cameras by the retraction every trial uses; the test-energy launches of a trial follow.
 * Returns E(xTest), pred, |dx| (summed in fp64 from the step as stored) and the branch; any pointer may be NULL.  A ba_solver_accept
 * behind it takes the step.  Branch 0 returns the bits of the prepare: BA_GET_DX, BA_GET_CAMS_TEST, BA_GET_POINTS_TEST and the
 * test energy (1 * x is x, -0 included; a point nobody observes keeps a zero step and a copy of x).
 * BA_CHOLESKY, BA_F64 and BA_F32, shard_world == 1; any loss and weights (they are in J); with ba_solver_set_constant a fixed
 * parameter has g = 0 and dx_gn = 0: its step is exactly 0 and its value keeps its bits, R of an omega-fixed camera included.
 * BA_ERR_ARG, the solver unchanged: another solver kind; a sharded solver; priors or relative poses set (their rows would have to
 * enter q: not built); BA_DAMP_MARQUARDT in force (H dx_gn = g - mu D dx_gn and a scaled norm: not built); no valid linearisation, or a
 * mask or measurement model pending; mu <= 0 or not finite (in the solver's scalar type); radius <= 0 or NaN; ba_solver_try_dogleg
 * without a valid prepare.
 * Memory: the first prepare allocates the copy of dx_gn and the lists of block partials, kept until ba_solver_free and counted by
 * ba_solver_device_bytes:   sizeof(scalar) (3 M + 9 N) + 8 (ceil(K / 256) + 3 ceil((3 M + 9 N) / 256) + ceil(M / 256) + 1 + 8) bytes.
 * BA_ERR_NOMEM when they do not fit; the solver stays usable. */
int ba_solver_dogleg_prepare(ba_solver *s, double mu, ba_dogleg_info *out);
int ba_solver_try_dogleg(ba_solver *s, double radius, double *energy_test, double *pred, double *dx_norm, int *branch);

/* ba_minimize_dogleg: a host-synchronous driver built from ba_solver_linearize, ba_solver_dogleg_prepare, ba_solver_try_dogleg and
 * ba_solver_accept, one scalar read-back per trial (ba_minimize and its captured graphs are untouched; a device-side control is not
 * built).  Per outer iteration: mu = mu_rel m max diag(J'J) of this linearisation; m starts at 1 and is multiplied by 10 whenever a
 * prepare returns a pred of the full Gauss-Newton step that is <= 0 or not finite (scalars that ba_dogleg_coefficients refuses, a step
 * that is not finite, count as that; such a retry is no trial), the driver gives up
 * with BA_EXCEEDED_LAMBDA_MAX once mu_rel m > mu_rel_max, and after a good prepare m <- max(1, m / 5).  The first radius is
 * radius_init, or |dx_gn| of the first iteration when that is 0.  The first trial of an iteration with sqrt(gn2) <= radius is the
 * prepare's own xTest, used as it is and not evaluated again.  A trial is accepted iff pred > 0 and E_test < E; with
 * rho = (E - E_test) / pred the radius becomes min(radius_max, max(radius, 3 |dx|)) behind an accepted step with rho > 0.75, radius / 2
 * behind an accepted step with rho < 0.25 and behind a rejected one.
 * Status: BA_SUCCESS behind an accepted step with (E - E_test) / E < tol_fun (the step is taken) or when g2 = 0;
 * BA_EXCEEDED_LAMBDA_MAX when the radius falls below radius_min (or mu_rel m exceeds mu_rel_max); BA_MAX_ITERS; BA_TOO_MANY_FUN_EVALS
 * (counted: the first linearisation, every prepare, every ba_solver_try_dogleg); BA_RUNNING when max_trials rows have been made.
 * The callback and the verbose table are ba_minimize's, WITH THE RADIUS OF THE TRIAL IN THE LAMBDA COLUMN; ba_result.lambda is the
 * final radius.  Refusals: those of ba_solver_dogleg_prepare, decided before anything is touched, and radius_init < 0 or NaN,
 * radius_min / radius_max / mu_rel / mu_rel_max / tol_fun not positive. */
typedef struct {
    double radius_init; /* 0: |dx_gn| of the first iteration */
    double radius_min;  /* 1e-32 */
    double radius_max;  /* 1e16  */
    double mu_rel;      /* 1e-12 (the project's lambda0 rule) */
    double mu_rel_max;  /* 1     */
    double tol_fun;     /* 1e-8  */
    int max_iter;       /* those of ba_lm_params_default */
    int max_fun_ev;
    int max_trials;     /* stop after this many table rows (0 = unlimited) */
    int verbose;
} ba_dogleg_params;
void ba_dogleg_params_default(ba_dogleg_params *p);
int ba_minimize_dogleg(ba_solver *s, const ba_dogleg_params *p, ba_trial_cb cb, void *user, ba_result *out);

/* ---- triangulation: re-seat points from the cameras that see them (no reference counterpart; COLMAP's retriangulation between
 * bundle-adjustment rounds, Ceres and g2o pipelines' triangulation front ends) ---------------------------------- */

/* Model: XX = R X + T, xu = XX_01 / XX_2, kr = 1 + k1 |xu|^2 + k2 |xu|^4, pi = f kr xu, with R, T, f, k1, k2 the 15 scalars of
 * BA_GET_CAMS.  BAL's camera looks down -z: X is in front of camera a iff (R_a X + T_a)_2 < 0.  All geometry below is fp64 for both
 * scalar types; it reads the resident state as stored, and the new point is rounded once to the solver's scalar type.
 * The rule per point (csrc/ba_triangulate.hip.h, one text for the host function and the kernel), over its t observations o:
 * 1. Undistort: m = meas_o / f; rho solves rho (1 + k1 rho^2 + k2 rho^4) = |m| by 12 Newton steps from rho = |m|; xu = m rho / |m|
 *    (0 when |m| = 0).  The observation is UNUSABLE if a derivative 1 + 3 k1 rho^2 + 5 k2 rho^4 met on the way or at the end is <= 0, a
 *    value is not finite, rho ends <= 0, or the equation is missed by more than 1e-12 |m|.  Ray d_o = R' (-(xu, 1)) normalised, centre
 *    C_o = -R'T.
 * 2. theta = the largest angle between two usable rays, from the largest chord: theta = 2 atan2(c, sqrt(4 - c^2)), c = max |d_i - d_j|.
 *    Fewer than two usable observations: BA_TRI_FEW_VIEWS.  theta < min_angle_deg: BA_TRI_LOW_ANGLE.
 * 3. Midpoint: X minimises sum_o w_o^2 |(I - d_o d_o')(X - C_o)|^2 over the usable observations (w_o: ba_solver_set_obs_weights, else 1),
 *    a 3 x 3 Cholesky; a pivot <= 0 or not finite: BA_TRI_DEGENERATE.
 * 4. refine_iters monotone IRLS Gauss-Newton steps on the point's own term c(X) = sum_o rho(s_o), s_o = w_o^2 |pi_o(X) - meas_o|^2, rho the
 *    loss in force, over ALL its observations: H = sum rho'(s_o) J_o'J_o, g = sum rho'(s_o) J_o'r_o (r_o = w_o (pi_o - meas_o), J_o its
 *    derivative by X), mu = 1e-9 tr(H) / 3, X' = X - (H + mu I)^-1 g, taken iff c(X') < c(X) (1 - 1e-11) -- a decrease that an fp64
 *    evaluation of c can tell from rounding; a plain c(X') < c(X) would let the order of a sum decide the last step --; otherwise, or
 *    when a pivot of H + mu I is <= 0, the refinement stops.  rho' = 1 (TRIVIAL), (1 - s / tau^2) / 2 below tau^2 and 0 above (REFERENCE), 1 up to delta^2 and
 *    delta / sqrt(s) above (HUBER), 1 / (1 + s / c^2) (CAUCHY).
 * 5. The candidate must lie in front of every camera of the track, else BA_TRI_BEHIND; with max_reproj_px > 0 every usable observation
 *    must have an unweighted |pi - meas| <= max_reproj_px, else BA_TRI_REPROJ; with only_if_better c(X_new) < c(X_old) is required,
 *    else BA_TRI_NOT_BETTER.  A point held constant by ba_solver_set_constant or carrying a point prior is BA_TRI_FIXED and never
 *    touched; a point nobody observes is BA_TRI_FEW_VIEWS.  BA_TRI_REPLACED = 0: the resident point takes X_new.  Any other status keeps
 *    the point's bits.
 * Sums over a track: the host function adds in observation order; the kernel gives a point 8 lanes of a wavefront, lane l adds the
 * observations l, l + 8, ... in order and the lanes are combined by a fixed butterfly: a point's result and status are the same bits on
 * every run, whatever else is in the request and wherever the point stands in it.  No atomics. */
typedef enum {
    BA_TRI_REPLACED = 0, BA_TRI_FEW_VIEWS = 1, BA_TRI_LOW_ANGLE = 2, BA_TRI_DEGENERATE = 3, BA_TRI_BEHIND = 4, BA_TRI_REPROJ = 5,
    BA_TRI_NOT_BETTER = 6, BA_TRI_FIXED = 7
} ba_triangulate_status;
typedef struct { double min_angle_deg; double max_reproj_px; int refine_iters; int only_if_better; } ba_triangulate_params;
void ba_triangulate_params_default(ba_triangulate_params *p); /* 1.5 (COLMAP's min_tri_angle), 0 = off, 5, 1 */
/* cost_before / cost_after: sum of c(X) over the asked points before the call and behind it (a refused point counts its old c twice),
 * fp64, block partials of 32 points reduced in a fixed order; ms: device time of the call's launches. */
typedef struct { long long asked, by_status[8]; double cost_before, cost_after; double ms; } ba_triangulate_stats;
/* ba_solver_triangulate_points: the rule for the points pt_ids[0 .. n_pts) (PROBLEM numbering), or for all M points when pt_ids is NULL
 * and n_pts is 0, on the resident state x.  status (may be NULL) receives one byte per asked point in the order of the request (M bytes
 * for all points); stats may be NULL; p == NULL means the defaults.  Every solver kind, BA_F64 and BA_F32, shard_world == 1.
 * A successful call invalidates what ba_solver_set_state(s, NULL, pts) invalidates -- the linearisation, a pending step, a computed
 * covariance, a prepared dogleg -- and, J being another state's, ba_solver_try_step returns BA_ERR_ARG until the next
 * ba_solver_linearize or ba_minimize, as it does behind a setter.  It leaves the cameras, xTest, masks, priors, groups and captured
 * graphs alone.  With no point replaced the state keeps every bit.
 * BA_ERR_ARG, decided on the host, the solver unchanged: a sharded solver (not built); an id out of range or listed twice; n_pts < 0;
 * pt_ids NULL with n_pts > 0; min_angle_deg outside [0, 180), max_reproj_px < 0, refine_iters < 0 or any of them not finite; a
 * ba_solver_set_loss or ba_solver_set_obs_weights call that no ba_solver_linearize or ba_minimize has followed (which loss is "in
 * force" would be ambiguous).
 * Memory, allocated by the first call, kept until ba_solver_free and counted by ba_solver_device_bytes:
 *   24 K (the rays) + 6 M (status, request, fixed flags: 1 + 4 + 1) + 8 (10 max(1, ceil(8 M / 256)) + 16) bytes.
 * BA_ERR_NOMEM when they do not fit; the solver stays usable. */
int ba_solver_triangulate_points(ba_solver *s, const ba_triangulate_params *p, int n_pts, const int *pt_ids, unsigned char *status,
                                 ba_triangulate_stats *stats);
/* ba_triangulate_point: the rule on one track, host only (no GPU).  cam15: 15 t (one BA_GET_CAMS row per observation), meas: 2 t,
 * w: t or NULL.  x_new receives the candidate where the rule formed one (statuses 0, 4, 5, 6) and x_old otherwise; cost_new its c,
 * or c(x_old); angle_deg theta (0 with fewer than two usable observations).  Any output pointer may be NULL; p == NULL: the defaults.
 * BA_ERR_ARG: t < 0, a missing array, parameters as above, an unknown loss, a scale or weight that is not positive and finite. */
int ba_triangulate_point(int t, const double *cam15, const double *meas, const double *w, int loss_kind, double loss_scale,
                         const ba_triangulate_params *p, const double *x_old, double *x_new, int *status, double *cost_old,
                         double *cost_new, double *angle_deg);

/* ---- the active mask and the observation filter (no reference counterpart; COLMAP's FilterObservations / FilterPoints between
 * bundle-adjustment rounds, Ceres users rebuild the problem) --------------------------------------------------- */

/* ba_solver_set_obs_active: an INACTIVE observation contributes exactly +0 to e and to its rows of J -- by selection, not by a product
 * with 0, so also where its projection is not finite (a point on the camera's principal plane, an inf).  Everything built from e and J
 * follows, as for the weights above: energy, g, U, V, S, rhs, lambda0, rho, the stop tests, BA_ITERSCHUR's operator and its
 * preconditioners, Marquardt's D, the dogleg's q, both covariances.  BA_GET_RESIDUALS, BA_GET_JC and BA_GET_JP return zeros at an inactive
 * observation.  ba_solver_stats keeps its meaning (all K observations); ba_problem_covisibility and the visibility forest's plan are
 * functions of the problem and do not change.
 * active: K bytes of the PROBLEM in the order of the input file, != 0 = active; NULL = all active; copied.  The solver keeps the
 * effective weight w_eff = active ? w_o : 0 as one device array in its own observation order; the weights and the mask stay independent
 * settings: ba_solver_set_obs_weights(NULL) keeps the mask, ba_solver_set_obs_active(NULL) keeps the weights.  While an observation is
 * inactive the solver runs the measurement model's instantiations of the linearisation; a mask that is NULL or all non-zero restores the
 * path without one bit for bit (with the default loss and no weights: the default kernels).
 * A point whose observations are all inactive behaves as a point nobody observes: U = lambda I (lambda diag_min under Marquardt), a step
 * of exactly 0, its bits kept; at lambda = 0 the covariance calls return BA_ERR_SINGULAR for it unless it is held constant.  A camera
 * with no active observation: the same on its 9 x 9 block.
 * State: as ba_solver_set_obs_weights -- the change takes effect at the next ba_solver_linearize or ba_minimize, a ba_solver_try_step
 * before that returns BA_ERR_ARG, a computed covariance and a prepared dogleg become stale, ba_solver_triangulate_points refuses until a
 * linearisation has taken the mask up.  A call that leaves the mask as it was (the same bytes after != 0) changes no flag.
 * ba_solver_triangulate_points under a mask: an inactive observation is not part of its track (no ray, not in the angle, the midpoint,
 * the refinement's cost, cost_before / cost_after, the front test or the max_reproj_px test); fewer than two active usable
 * observations: BA_TRI_FEW_VIEWS.
 * BA_ERR_ARG, the solver unchanged: a kind other than BA_CHOLESKY or BA_ITERSCHUR (an emptied track would put a zero column block into
 * the per-point QR: not built); shard_world > 1 (not built).
 * Memory, allocated by the first mask with an inactive observation (or the first applying filter call), kept until ba_solver_free and
 * counted by ba_solver_device_bytes: K (1 + sizeof(scalar)) bytes -- the active bytes and w_eff. */
int ba_solver_set_obs_active(ba_solver *s, const unsigned char *active /* K of the PROBLEM, file order; != 0 = active; NULL = all */);
/* active (may be NULL) receives K bytes 0 / 1 in file order, n_active (may be NULL) their sum.  Every kind; all ones where no mask can be set. */
int ba_solver_get_obs_active(ba_solver *s, unsigned char *active /* K, file order */, long long *n_active);

/* The filter.  Per point, on the resident state x (model and fp64 geometry as for the triangulation above: XX = R X + T, in front iff
 * XX_2 < 0, the state read as stored), one text for the host function and the kernels (csrc/ba_filter.hip.h):
 * 1. An observation that is already inactive is BA_OBS_WAS_OFF and takes no further part.
 * 2. Per active observation: BA_OBS_BEHIND if require_front and not (XX_2 < 0) (a NaN counts as behind); otherwise, with
 *    err = |pi(X) - meas| (unweighted, pixels): BA_OBS_NONFINITE if err is not finite, BA_OBS_REPROJ if max_reproj_px > 0 and
 *    err > max_reproj_px.  The others are survivors.
 * 3. Fewer than min_track survivors: the point is BA_FPT_SHORT.
 * 4. With min_angle_deg > 0 and the point not short: theta = the largest angle between two survivors' rays d_o = (C_o - X) / |C_o - X|,
 *    C_o = -R'T -- the rays of the CURRENT point, as COLMAP takes them --, from the largest chord: theta = 2 atan2(c, sqrt(4 - c^2)),
 *    c = max |d_i - d_j|.  A survivor with |C_o - X| = 0 or not finite has no ray.  theta < min_angle_deg: BA_FPT_LOW_ANGLE.  (The kernel
 *    needs the decision only and leaves a lane's pair loop at a chord that decides it; ba_filter_track returns the full theta.)
 * 5. Every survivor of a point that is not kept becomes BA_OBS_POINT.
 * 6. apply != 0: every observation whose status is not BA_OBS_KEPT becomes inactive, w_eff rewritten on the device by the same launch;
 *    if at least one was deactivated the state changes exactly as with ba_solver_set_obs_active, otherwise it keeps every bit and every
 *    flag.  apply == 0: a measurement; nothing changes, not even a flag.
 * Points held constant or carrying a prior are filtered like any other: their observations constrain cameras.
 * err_px: |pi - meas| of every active observation, whatever the arithmetic gives (BEHIND ones too); NaN at BA_OBS_WAS_OFF.
 * A point's statuses are the same bits on every run; no atomics. */
typedef enum { BA_OBS_KEPT = 0, BA_OBS_WAS_OFF = 1, BA_OBS_BEHIND = 2, BA_OBS_NONFINITE = 3, BA_OBS_REPROJ = 4, BA_OBS_POINT = 5 } ba_obs_status;
typedef enum { BA_FPT_KEPT = 0, BA_FPT_SHORT = 1, BA_FPT_LOW_ANGLE = 2 } ba_filter_point_status;
typedef struct { double max_reproj_px; double min_angle_deg; int min_track; int require_front; } ba_filter_params;
void ba_filter_params_default(ba_filter_params *p); /* 4.0 (COLMAP's filter_max_reproj_error), 1.5 (its min_tri_angle), 2, 1 */
/* active_before = K - by_status[BA_OBS_WAS_OFF], active_after = by_status[BA_OBS_KEPT]; err_sum_before: sum of err_px over the active
 * observations with a finite err_px, err_sum_after: over the kept ones; fp64, lane sums combined by a fixed butterfly per point, block
 * partials of 32 points reduced in a fixed order.  ms: device time of the call's launches. */
typedef struct {
    long long active_before, active_after, by_status[6], points_short, points_low_angle;
    double err_sum_before, err_sum_after;
    double ms;
} ba_filter_stats;
/* ba_solver_filter_observations: the rule for all points.  obs_status (K bytes, file order), pt_status (M bytes), err_px (K doubles, file
 * order), stats: any may be NULL; p == NULL means the defaults.  BA_CHOLESKY and BA_ITERSCHUR, BA_F64 and BA_F32, shard_world == 1.
 * BA_ERR_ARG, decided on the host, the solver unchanged: another kind, a sharded solver (neither built); max_reproj_px < 0 or not
 * finite; min_angle_deg outside [0, 180) or not finite; min_track < 0.
 * Memory, allocated by the first call, kept until ba_solver_free and counted by ba_solver_device_bytes:
 *   K (34 + sizeof(scalar)) (status 1, err_px 8, rays 24, the new active bytes 1, the new w_eff) + M (point status)
 *   + 8 (10 max(1, ceil(8 M / 256)) + 16) bytes; a call with apply != 0 also allocates the mask's K (1 + sizeof(scalar)) above.
 * BA_ERR_NOMEM when they do not fit; the solver stays usable. */
int ba_solver_filter_observations(ba_solver *s, const ba_filter_params *p, int apply, unsigned char *obs_status /* K, file order */,
                                  unsigned char *pt_status /* M */, double *err_px /* K, file order */, ba_filter_stats *stats);
/* ba_filter_track: the rule on one track, host only (no GPU).  cam15: 15 t (one BA_GET_CAMS row per observation), meas: 2 t, active: t
 * bytes or NULL (all active), X: the point.  obs_status: t bytes, err_px: t, angle_deg: the full theta (0 where step 4 did not run).
 * Any output pointer may be NULL; p == NULL: the defaults.  BA_ERR_ARG: t < 0, a missing array, parameters as above. */
int ba_filter_track(int t, const double *cam15, const double *meas, const unsigned char *active, const double *X,
                    const ba_filter_params *p, unsigned char *obs_status, int *pt_status, double *err_px, double *angle_deg);

/* Library / device info: fills name (<= n bytes), returns the number of CUs via *cus. */
int ba_device_info(int device, char *name, size_t n, int *cus);
const char *ba_version(void);

#ifdef __cplusplus
}
#endif
#endif /* BA_MI355X_H */
