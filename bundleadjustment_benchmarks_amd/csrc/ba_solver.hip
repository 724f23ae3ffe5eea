// ba_solver.hip -- device-resident LM solver behind the C ABI of include/ba_mi355x.h.
//
// Host control flow = the LM classes of the reference:
//   src/Eigen_ext/BacktrackLevMarqQRChol.h:204-436   (QRCHOL; QRKIT reuses the loop)
//   src/Eigen_ext/BacktrackLevMarqCholesky.h:190-361 (CHOLESKY)
// Everything the loops call on the functor / linear solver runs as HIP kernels on resident data; per trial only
// a handful of scalars (test energy, rho denominator, |dx|^2) cross PCIe.
// There is NO CPU fallback: without a HIP device ba_solver_create fails with BA_ERR_HIP.
#include "ba_internal.h"
#include "ba_kernels.hip.h"
#include "ba_dense.hip.h"
#include "ba_qr.hip.h"
#include "ba_pcg.hip.h"
#include "ba_cov.hip.h"
#include "ba_pcg_multi.hip.h"
#include "ba_pcg_share.hip.h"
#include "ba_prior.hip.h"
#include "ba_relpose.hip.h"
#include "ba_dogleg.hip.h"
#include "ba_triangulate.hip.h"
#include "ba_filter.hip.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <numeric>
#include <string>
#include <type_traits>

#define HIPCHK(x)                                                                                   \
    do {                                                                                            \
        hipError_t e_ = (x);                                                                        \
        if (e_ != hipSuccess) {                                                                     \
            fprintf(stderr, "ba_mi355x: %s failed: %s (%s:%d)\n", #x, hipGetErrorString(e_), __FILE__, __LINE__); \
            return BA_ERR_HIP;                                                                      \
        }                                                                                           \
    } while (0)

namespace {

constexpr int NB = BA_NB;    // block-column width of the dense LDL^T
constexpr int NAUG = 3;      // augmented rows: D = reduced rhs, D+1 = g_c, D+2 = spare
constexpr int NSCAL = 24;    // device scalar slots
// SC_ETEST .. SC_ERR are contiguous: the ONE scalar all-reduce behind a sharded trial sums these five
enum { SC_ENERGY = 0, SC_DMAX_P = 1, SC_ETEST = 2, SC_RHO_P = 3, SC_DN_P = 4,
       SC_GUARD = 5 /* the previous trial's decision (accepted + 2 stop) of this shard: summed, it must be world x the same (k_lm_control) */,
       SC_ERR = 6 /* device error word: a BA_DEVERR_* code written by a kernel whose in-launch hand-off wait ran out (sharded: summed, so
                     that every shard sees a time-out of any shard on the same trial) */,
       SC_DMAX_C = 7, SC_ST0 = 8 /* ..11 stats */, SC_LAMBDA = 12 /* lambda of the current trial, read by the kernels */,
       SC_ZERO = 13 /* always 0: the 'lambda' of MOREQR's outer factorisation */,
       SC_ELOC = 15 /* sharded: this shard's part of the energy of the latest linearisation (rides on the next packed all-reduce) */,
       SC_RHO_C = 16, SC_DN_C = 17 };
constexpr int N_STEP_SCALARS = 5; // SC_ETEST, SC_RHO_P, SC_DN_P, SC_GUARD, SC_ERR
enum { EV_T0 = 0, EV_T1, EV_T2, EV_T3, EV_T4, EV_T5, EV_T6, EV_L0, EV_L1, EV_N };
constexpr int RING_EV = 8; // event slots of the trials in flight under ba_minimize (LM_DEPTH + the ones not yet harvested)
constexpr int RING_NE = 6; // per slot: trial start | before / after the matrix all-reduce | before / after the scalar all-reduce | after control + linearisation

// a run-time flag as a template argument: with_flag(b, [&](auto B) { launch k<..., B()> with one argument list })
template <typename F> void with_flag(bool b, F &&f)
{
    if (b) f(std::bool_constant<true>{});
    else f(std::bool_constant<false>{});
}
template <typename F> void with_flags(bool a, bool b, F &&f)
{
    with_flag(a, [&](auto A) { with_flag(b, [&](auto B) { f(A, B); }); });
}
template <int V> using int_c = std::integral_constant<int, V>; // (a template argument that is not a flag: k_eval's FUSE)

// Owns its device memory: movable (the source is left empty), not copyable
template <typename T> struct DevBuf {
    T *p = nullptr;
    size_t n = 0;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    DevBuf(DevBuf &&o) noexcept : p(o.p), n(o.n) { o.p = nullptr; o.n = 0; }
    DevBuf &operator=(DevBuf &&o) noexcept { if (this != &o) { release(); p = o.p; n = o.n; o.p = nullptr; o.n = 0; } return *this; } // (frees what it held)
    int alloc(size_t count)
    {
        n = count;
        if (count == 0) return BA_OK;
        hipError_t e = hipMalloc((void **)&p, sizeof(T) * count);
        if (e != hipSuccess) { p = nullptr; return e == hipErrorOutOfMemory ? BA_ERR_NOMEM : BA_ERR_HIP; }
        return BA_OK;
    }
    int upload(const std::vector<T> &h)
    {
        int rc = alloc(h.size());
        if (rc) return rc;
        if (!h.empty() && hipMemcpy(p, h.data(), sizeof(T) * h.size(), hipMemcpyHostToDevice) != hipSuccess) return BA_ERR_HIP;
        return BA_OK;
    }
    // a plan's flat ints (ba_internal.h) as the records the kernels read; the caller asserts the ints per record
    int upload_ints(const std::vector<int> &h)
    {
        static_assert(sizeof(T) % sizeof(int) == 0 && std::is_trivially_copyable<T>::value, "not a record of ints");
        int rc = alloc(h.size() / (sizeof(T) / sizeof(int)));
        if (rc) return rc;
        if (!h.empty() && hipMemcpy(p, h.data(), sizeof(int) * h.size(), hipMemcpyHostToDevice) != hipSuccess) return BA_ERR_HIP;
        return BA_OK;
    }
    void release()
    {
        if (p) (void)hipFree(p);
        p = nullptr; n = 0;
    }
    ~DevBuf() { release(); }
};
static_assert(!std::is_copy_constructible<DevBuf<int>>::value); static_assert(!std::is_copy_assignable<DevBuf<int>>::value);
template <typename B> size_t bytes_of(const B &b) { return b.p ? sizeof(*b.p) * b.n : 0; }

struct SolverBase {
    virtual ~SolverBase() {}
    virtual int init(const ba_problem *p, ba_solver_kind kind, int rank, int world) = 0;
    virtual int linearize(double *energy, double *diag_max) = 0;
    virtual int try_step(double lambda, double *e_test, double *rho_scale, double *dx_norm) = 0;
    virtual int accept() = 0;
    virtual int dogleg_prepare(double mu, ba_dogleg_info *out) = 0;
    virtual int try_dogleg(double radius, double *e_test, double *pred, double *dx_norm, int *branch) = 0;
    virtual int minimize_dogleg(const ba_dogleg_params *dp, ba_trial_cb cb, void *user, ba_result *out) = 0;
    virtual int triangulate(const ba_triangulate_params *p, int n_pts, const int *pt_ids, unsigned char *status, ba_triangulate_stats *stats) = 0;
    virtual int stats(double *out4) = 0;
    virtual int get(int what, double *out, size_t n) = 0;
    virtual int set_state(const double *cam15, const double *pts) = 0;
    virtual void set_stream_hook() {}
    virtual int minimize(const ba_lm_params *lm, ba_trial_cb cb, void *user, ba_result *out) = 0;
    virtual int time_phase(int phase, int reps, double lambda, double *ms) = 0;
    virtual int selftest(int which) = 0;
    virtual int set_pcg(int max_iter, double rel_tol) = 0;
    virtual int pcg_stats(ba_pcg_stats *out, int reset) = 0;
    virtual int set_pcg_model_tol(double eta) = 0;
    virtual int pcg_stop_stats(ba_pcg_stop_stats *out, int reset) = 0;
    virtual int set_damping(int kind, double diag_min, double diag_max) = 0;
    virtual int get_damping(int *kind, double *diag_min, double *diag_max) = 0;
    virtual int set_precond(int kind, int max_tree) = 0;
    virtual int precond_info(long long *out6, int *fallback_trees) = 0;
    virtual int set_shared(const int *group_of) = 0;
    virtual int shared_info(long long *out4) = 0;
    virtual int set_constant(const unsigned short *cam_mask, const unsigned char *pt_fixed) = 0;
    virtual int set_loss(int kind, double scale) = 0;
    virtual int set_obs_weights(const double *w) = 0;
    virtual int set_obs_active(const unsigned char *active) = 0;
    virtual int get_obs_active(unsigned char *active, long long *n_active) = 0;
    virtual int filter(const ba_filter_params *p, int apply, unsigned char *obs_status, unsigned char *pt_status, double *err_px, ba_filter_stats *stats) = 0;
    virtual int set_priors(int type, int n, const int *ids, const double *x0, const double *info) = 0;
    virtual int prior_energy(double *out3) = 0;
    virtual int set_relposes(int n, const int *pairs, const double *R0, const double *t0, const double *Lr, const double *Lt) = 0;
    virtual int relpose_energy(double *out2) = 0;
    virtual size_t device_bytes() const = 0;
    virtual int cov_compute(double lambda) = 0;
    virtual int cov_get(int n_pairs, const int *cam_pairs, double *cam_cov, int n_pts, const int *pt_ids, double *pt_cov) = 0;
    virtual int cov_timing(double *ms4) = 0;
    virtual int cov_pcg(double lambda, int max_iter, double rel_tol, int n_pairs, const int *cam_pairs, double *cam_cov, int n_pts, const int *pt_ids,
                        double *pt_cov, ba_cov_pcg_stats *stats) = 0;
    bool poisoned = false; // the watchdog gave up on a launch that never finished: every later call fails, nothing is freed
    int recoveries = 0;    // trials repeated through the launch-per-step factorisation after a hand-off time-out
    ba_allreduce_fn ar_fn = nullptr;
    void *ar_user = nullptr;
    void *comm = nullptr; // ncclComm_t of the shard group (ba_solver_comm_init)
    hipStream_t st = nullptr;
    bool own_stream = false;
    bool keep = false; // keep a copy of S / rhs before the factorisation (parity tests)
    ba_structure sx;
    ba_timing tm{};
    int rank = 0, world = 1;
};

template <typename T> void host_rodrigues(const T *om, T *R)
{
    // Math::createRotationMatrixRodrigues, src/MathUtils.h:66-82
    const T th = std::sqrt(om[0] * om[0] + om[1] * om[1] + om[2] * om[2]);
    for (int i = 0; i < 9; i++) R[i] = (i % 4 == 0) ? (T)1 : (T)0;
    if (std::fabs(th) > (T)1e-6) {
        const T J[9] = {0, -om[2], om[1], om[2], 0, -om[0], -om[1], om[0], 0};
        T J2[9];
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) {
                T a = 0;
                for (int k = 0; k < 3; k++) a += J[i * 3 + k] * J[k * 3 + j];
                J2[i * 3 + j] = a;
            }
        const T c1 = std::sin(th) / th, c2 = ((T)1.0 - std::cos(th)) / (th * th);
        for (int i = 0; i < 9; i++) R[i] = R[i] + c1 * J[i] + c2 * J2[i];
    }
}

template <typename T> struct Solver final : SolverBase {
    ba_solver_kind kind = BA_CHOLESKY;
    int N = 0, D = 0, Dp = 0, ld = 0, Ml = 0, Kl = 0;
    T tau = (T)0.5; // INLIER_THRESHOLD, src/bundle_adjustment_large.cpp:36
    // structure
    DevBuf<int> d_obs_cam, d_obs_pt, d_pt_ptr, d_pair_hi, d_pair_lo, d_pair_chunk_ptr,
        d_dchunk_ptr, d_cam_dchunk_ptr, d_cam_obs, d_qr_pts, d_flags, d_pperm /* column permutation of every point's 3x3 block */;
    DevBuf<int4> d_chunk_info; // per chunk of the pair kernel: first entry, count | BA_CHUNK_SINGLE, cameras hi | lo << 16, chunk id
    DevBuf<int2> d_ent;        // per entry: row observation, column observation (~point for a self entry)
    DevBuf<int> d_wave_ptr;    // per wavefront of the pair kernel: its range of chunk descriptors
    DevBuf<int> d_red_pairs;   // pairs k_schur_reduce writes: those without entries and those with several chunks
    int schur_window = 0;
    int nred = 0;
    bool no_fold = false; // BA_NO_FOLD (dev switch): every launch of its own again (A/B timing on one box)
    bool trial_head = false; // BA_TRIAL_HEAD=1 (dev switch): every trial starts with its own elimination and pair assembly again (A/B, bit-equal)
    bool rec_coop = true; // BA_REC_PLAIN (dev switch) clears it: every thread stores its own record of rec / JcA again (A/B, bit-equal)
    int schur_grid = 1, schur_wgs = 4 /* workgroups of k_schur_pairs per CU */, schur_bands = 8, schur_nband = 1;
    // state: x = d_cam[0], d_pts[0]; xTest = d_cam[1], d_pts[1] (x = xTest is a device-side copy, k_commit)
    // linearisation at x (r, J, J^T r, block diagonals, MOREQR's outer factors): one set
    DevBuf<T> d_r, d_Jc, d_Jp, d_JcA, d_U0, d_gp, d_V, d_gc, d_rec0, d_dinv0, d_tvec0, d_tri0;
    DevBuf<T> d_cam[2], d_pts[2], d_meas, d_gcg, d_dslab, d_rec, d_dinv, d_tvec, d_tri,
        d_slab, d_S, d_pack, d_Skeep, d_Wp, d_Winv, d_dxc, d_dxp, d_part_e, d_part_pm, d_part_bs, d_part_st, d_scal;
    DevBuf<ba_lm_dev<T>> d_lm; // LM state of the device-side step control (k_lm_control)
    // QRKIT (single shard): dense J2bot (+ rhs column) for the Householder QR of the right block, its reflector scalars, the thin Q rows
    DevBuf<T> d_qA, d_qtau, d_q1obs, d_q1lam;
    size_t q_lda = 0, q_tau_stride = 0;
    hipStream_t st_qr = nullptr;   // second stream of the dense QR: trailing updates beside the panel's chunk chain (ba_qr_solve)
    hipEvent_t ev_qr[2] = {nullptr, nullptr};
    ba_qr_side qr_side() const
    {
        ba_qr_side sd;
        sd.st2 = st_qr; sd.ev_chunk = ev_qr[0]; sd.ev_apply = ev_qr[1];
        return sd;
    }
    int q_rows = 0;
    // QRKIT / QRSPQR always run the dense QR of J2bot -- sharded too (distributed TSQR: launch_qr_stack), never QRCHOL's normal
    // equations under another name
    // (round 4) ... and so does MOREQR: its right block is the dense QR of [rows left by the per-point QRs ; R22 ; sqrt(lambda) I]
    // (BacktrackLevMarqMore.h:297-345), R22 from one dense QR of J2bot(lambda = 0) per outer iteration (:288) -- no S, no LDL^T, sharded
    // through the same TSQR stack.  BA_MOREQR_QR=0 (read at solver creation) selects rounds 1 - 3's variant instead, which eliminates the
    // points by QR and then factors S = (Jc'Jc + lambda I) - sum Z Z' by LDL^T: 20x faster, but normal equations.
    bool more_qr_on = true;
    bool dense_qr() const { return kind == BA_QRKIT || kind == BA_QRSPQR || more_qr(); }
    // CHOLESKY's linearisation (AoS camera records, fused k_eval<T, true, 3>, or 2 with the owners' stores) and point elimination (k_elim_chol): CHOLESKY and BA_ITERSCHUR
    bool chol_elim() const { return kind == BA_CHOLESKY || kind == BA_ITERSCHUR; }
    bool iterative() const { return kind == BA_ITERSCHUR; } // the reduced system by PCG (ba_pcg.hip.h): no S, no camera pairs
    bool more_qr() const { return kind == BA_MOREQR && more_qr_on; }
    DevBuf<T> d_mQl, d_mQR, d_R22; // MOREQR: the inner point blocks' thin Q (lambda rows, R1 rows: [Ml][9] each); R22 | c2 of the outer QR, D x (D + 1)
    int outer_rows() const { return 2 * Kl + 3 * Ml + D; }               // J2bot (QRKIT / QRSPQR per trial; MOREQR per outer iteration, lambda = 0)
    int inner_rows() const { return more_qr() ? 6 * Ml + 2 * D : outer_rows(); } // the matrix a TRIAL factors
    DevBuf<T> d_qB; // sharded: the stack of the shards' R factors (+ rhs column), behind it g_c and the energy (one all-reduce)
    size_t qb_ld() const { return (size_t)world * D + 64; }
    size_t qb_nmat() const { return qb_ld() * (size_t)(D + 1); }
    size_t qb_count() const { return qb_nmat() + (size_t)D + 1; }
    ba_lm_host *h_log = nullptr, *d_log = nullptr; // table rows + progress counter in pinned host memory (host / device address)
    T h_scal[NSCAL];
    T *h_lam = nullptr; // pinned staging word for lambda
    // one LM iteration as hipGraphs: world == 1: g_trial = elimination ... test energy, control, x = xTest, linearisation in ONE graph
    // (two graphs with events between them left 18 + 27 us of idle GPU per iteration at config 4: 0.872 -> 0.852 ms);
    // sharded: g_a (elimination, assembly, pack) | all-reduce | g_b (unpack ... test energy) | all-reduce | g_ctl
    // g_trial_nh: the iteration without its head (elimination, pair assembly) -- the tail of the iteration in front of it has done that
    // (tail_prepares())
    hipGraphExec_t g_trial = nullptr, g_trial_nh = nullptr, g_a = nullptr, g_b = nullptr, g_ctl = nullptr;
    bool seg_head = true; // the segments enqueue_trial is launching or capturing start with the explicit head
    bool use_graph = true;
    hipEvent_t ev[EV_N] = {};
    struct EvSlot { hipEvent_t e[RING_NE]; };
    EvSlot ring[RING_EV] = {};
    int gK = 0, gM = 0, gB = 0; // grids (observations, points, points x 8 lanes)
    // Workgroups of k_eval: point-aligned observation ranges (at most 256, whole points) whenever no point has more than 256
    // observations -- for the residual-only evaluation too, so that an energy is the same bits whichever instantiation sums it.
    // fuse: the linearisation behind an accepted step then also does the point part of the gradient and (CHOLESKY) the elimination
    // of the trial that follows (k_eval<T, true, FUSE>); BA_NO_FUSE=1 keeps the separate launches on the same ranges (A/B, bit-equal).
    int gE = 0;
    bool fuse = false;
    DevBuf<int> d_eb;
    bool step_level = false; // inside try_step: the segments add the phase events, the kept S, the QR self-check and their own test-energy sum
    int num_cus = 256; // of the device the solver lives on
    double wall_khz = 1e5;
    // A hand-off between workgroups of one launch that timed out (device error word) is survivable: the trial is repeated with the
    // factorisation and the back sweep as one launch per step (nobody waits for anybody), and the solver stays in that mode.
    bool safe_factor = false;
    ba_ldlt_plan ldlt_plan; // trailing-update jobs of the fused factor (ba_dense.hip.h), device copy in d_ldlt_jobs
    DevBuf<int> d_ldlt_jobs;
    int fault_rowflag = 0;    // self-test (2): the fused steps' row workgroups stay silent, the panel's wait is short
    double spin_next_s = 0;   // self-test (3): a kernel of that many seconds in front of the next trial
    double watchdog_s = 600;  // no LM row for that long = a hung launch (BA_WATCHDOG_S)

    // ---- the state of the optional features: one struct each, as Forest `fo` and Share `sh` further down ------------------------------
    // A struct holds its feature's buffers, counts and flags and sums its bytes.  A setter or a first-use allocator fills a new one --
    // everything that can fail -- and commits it with one move: the solver is unchanged behind any error, the old buffers leave there.
    struct Mask { // ba_solver_set_constant
        DevBuf<unsigned short> cmask; // [N]
        DevBuf<unsigned char> pfix;   // [Ml] of this shard
        bool on = false;              // some bit is set: the masked instantiations
        size_t bytes() const { return bytes_of(cmask) + bytes_of(pfix); }
    } mk;
    struct Model { // ba_solver_set_loss / ba_solver_set_obs_weights
        int loss_kind = BA_LOSS_REFERENCE;
        T loss_scale = (T)0.5;
        DevBuf<T> wobs; // [Kl] of this shard, the solver's observation order (like d_meas)
        size_t bytes() const { return bytes_of(wobs); }
    } md;
    struct PriorList { // one type's compact lists: what a call of ba_solver_set_point_priors / _centre_priors / _intrinsics_priors replaces
        DevBuf<int> id;
        DevBuf<T> x0, info;
        int n = 0;
        size_t bytes() const { return bytes_of(id) + bytes_of(x0) + bytes_of(info); }
    };
    struct Priors {
        PriorList of[3];    // 0 points (info = L, 9 per prior), 1 centres (L), 2 intrinsics (info = w, 3 per prior)
        DevBuf<int> lonely; // the points with a prior and no observation (k_prior_lonely)
        DevBuf<T> part;     // [3][g] prior energies of the last linearisation
        int g = 0;          // workgroups of k_prior
        size_t bytes() const { return of[0].bytes() + of[1].bytes() + of[2].bytes() + bytes_of(lonely) + bytes_of(part); }
    } pr;
    struct RelPoses { // ba_solver_set_relative_poses: the lists, the per-constraint records, the CSR of every camera's incident constraints
        DevBuf<int> pair, ptr, inc;
        DevBuf<T> R0, t0, Lr, Lt, rec, part; // part: [2][g] energies of the last linearisation
        int n = 0, g = 0;                    // g: workgroups of k_relpose
        std::vector<int> h_pair;             // the constraint list as set (host copy for the forest)
        size_t bytes() const { return bytes_of(pair) + bytes_of(ptr) + bytes_of(inc) + bytes_of(R0) + bytes_of(t0) + bytes_of(Lr) + bytes_of(Lt) + bytes_of(rec) + bytes_of(part); }
    } rp;
    struct Dogleg { // allocated by the first ba_solver_dogleg_prepare
        DevBuf<T> keep;        // the copy of dx_gn [3 Ml + D]
        DevBuf<double> part;   // [q partials: gK | g2, gn2, g'dx_gn partials: 3 dl_gd() | |dx|^2 partials: gM + 1 | the eight sums]
        ba_dogleg_info info{}; // the scalars of the last prepare
        size_t bytes() const { return bytes_of(keep) + bytes_of(part); }
    } dg;
    struct Triang { // allocated by the first ba_solver_triangulate_points
        DevBuf<double> ray, part;        // the rays [3][Kl]; [block partials: 10 tri_gmax() | the ten sums, padded to 16]
        DevBuf<int> ids;                 // [Ml] the request
        DevBuf<unsigned char> stat, fix; // [Ml] each
        size_t bytes() const { return bytes_of(ray) + bytes_of(part) + bytes_of(ids) + bytes_of(stat) + bytes_of(fix); }
    } tr;
    struct Active { // ba_solver_set_obs_active / an applying ba_solver_filter_observations; allocated by the first inactive observation
        DevBuf<unsigned char> act;        // [Kl] solver order, 1 = active
        DevBuf<T> weff;                   // [Kl] the effective weight active ? w_o : 0: what k_eval reads in place of md.wobs while on()
        std::vector<unsigned char> h_act; // the host's copy of act (empty: all active)
        long long n_off = 0;
        bool on() const { return n_off > 0; } // some observation is inactive
        size_t bytes() const { return bytes_of(act) + bytes_of(weff); }
    } ac;
    struct Filter { // allocated by the first ba_solver_filter_observations
        DevBuf<unsigned char> st, pst, nact; // observation statuses [Kl], point statuses [Ml], the new active bytes [Kl]
        DevBuf<double> err, ray, part;       // [Kl]; [3][Kl]; [block partials: BA_FLT_NSUM tri_gmax() | the sums, padded to 16]
        DevBuf<T> nweff;                     // [Kl] the new effective weights
        size_t bytes() const { return bytes_of(st) + bytes_of(pst) + bytes_of(nact) + bytes_of(err) + bytes_of(ray) + bytes_of(part) + bytes_of(nweff); }
    } fl;
    struct Cov { // allocated by the first ba_solver_covariance_compute
        DevBuf<T> buf; // the work buffer (cov_wp() ... cov_count() below)
        DevBuf<int> flag;
        double lambda = 0, ms[4] = {0, 0, 0, 0};
        size_t bytes() const { return bytes_of(buf) + bytes_of(flag); }
    } cv;

    // ---- what is valid: six flags, written by these transitions alone (entry point x flag: the table in DESIGN.md section 1) ----------
    struct Valid {
        bool have_lin = false;      // a linearisation at x exists
        bool have_step = false;     // xTest is the step of a trial: ba_solver_accept may take it
        bool cov_valid = false;     // ba_solver_covariance_get may return the computed blocks
        bool dl_valid = false;      // a prepared dogleg of the linearisation in place
        bool mask_pending = false;  // a setter or triangulate() since the last linearisation: J is the old one's, try_step refuses
        bool model_pending = false; // ba_solver_set_loss / _set_obs_weights since the last linearisation: triangulate() refuses
        void results_dropped() { cov_valid = false; dl_valid = false; } // (a covariance, a prepared dogleg: of the linearisation they came from)
        void lin_dropped() { results_dropped(); have_lin = false; }     // J is another state's
        void step_dropped() { have_step = false; }
        void stepped() { have_step = true; }
        void accepted() { step_dropped(); }                             // x = xTest has happened
        void x_moved() { lin_dropped(); step_dropped(); }               // behind a driver: a ba_solver_linearize at the final x comes first
        void points_reseated() { x_moved(); mask_pending = true; }      // what set_state(NULL, pts) drops, and try_step refuses as behind a setter
        void model_changed(bool measurement) { results_dropped(); step_dropped(); mask_pending = true; model_pending = model_pending || measurement; }
        void pending_taken() { mask_pending = false; model_pending = false; } // J, g and the records are now the current mask's and model's
        void linearised() { have_lin = true; }
        void cov_dropped() { cov_valid = false; }
        void cov_computed() { cov_valid = true; }
        void dogleg_dropped() { dl_valid = false; }
        void dogleg_prepared() { dl_valid = true; }
    } vf;

    // ---- the block partials the second-stage sums read, their layout stated here alone ----------------------------------------------
    // d_part_e  = [gE of k_eval | 3 gP of k_prior | 2 gR of k_relpose]: energies, summed in this fixed order (gP = pr.g, gR = rp.g)
    // d_part_pm = [gM of k_point_prep | gP of k_prior]: point diagonals (behind the points' own: the ones a point prior has raised)
    size_t part_e_count(int gp, int gr) const { return (size_t)gE + 3 * (size_t)gp + 2 * (size_t)gr; }
    size_t part_pm_count(int gp) const { return (size_t)gM + (size_t)gp; }
    int part_e_n() const { return (int)part_e_count(pr.g, rp.g); }
    int part_pm_n() const { return (int)part_pm_count(pr.g); }
    T *part_e_priors() const { return d_part_e.p + part_e_count(0, 0); }
    T *part_e_relposes() const { return d_part_e.p + part_e_count(pr.g, 0); }
    T *part_pm_priors() const { return d_part_pm.p + part_pm_count(0); }
    // both buffers anew, zero-filled, for (gP, gR): the last step of a setter that can fail, directly in front of its commit
    int resize_partials(int gp, int gr)
    {
        DevBuf<T> ne, nm;
        int rc;
        if ((rc = ne.alloc(part_e_count(gp, gr))) || (rc = nm.alloc(part_pm_count(gp)))) { (void)hipGetLastError(); return rc; }
        HIPCHK(hipMemset(ne.p, 0, sizeof(T) * ne.n));
        HIPCHK(hipMemset(nm.p, 0, sizeof(T) * nm.n));
        d_part_e = std::move(ne); d_part_pm = std::move(nm);
        return BA_OK;
    }

    // ---- argument checks the setters share --------------------------------------------------------------------------------------------
    // finite as doubles and in the solver's scalar type
    static bool finite_in_T(const double *v, size_t cnt) { return std::all_of(v, v + cnt, [](double x) { return std::isfinite(x) && std::isfinite((T)x); }); }
    static bool positive_in_T(double v) { return v > 0 && std::isfinite(v) && (T)v > 0 && std::isfinite((T)v); } // (a NaN fails the comparisons)
    static bool distinct_ids(int n, const int *ids, int lim) // n ids in [0, lim), none listed twice
    {
        if (n > lim) return false;
        std::vector<char> seen((size_t)(lim > 0 ? lim : 1), 0);
        for (int q = 0; q < n; q++) {
            if (ids[q] < 0 || ids[q] >= lim || seen[ids[q]]) return false;
            seen[ids[q]] = 1;
        }
        return true;
    }

    ~Solver() override
    {
        if (poisoned) return; // (ba_solver_free does not even get here: a HIP call could block on the launch that never ended)
        for (auto &e : ev)
            if (e) (void)hipEventDestroy(e);
        for (auto &sl : ring)
            for (auto &e : sl.e)
                if (e) (void)hipEventDestroy(e);
        drop_trial_graphs();
        if (h_lam) (void)hipHostFree(h_lam);
        if (h_log) (void)hipHostFree((void *)h_log);
        if (comm) ba_rccl_destroy(comm);
        if (own_stream && st) (void)hipStreamDestroy(st);
        if (st_qr) (void)hipStreamDestroy(st_qr);
        for (hipEvent_t e : ev_qr) if (e) (void)hipEventDestroy(e);
    }

    int init(const ba_problem *p, ba_solver_kind k, int rk, int wd) override
    {
        kind = k; rank = rk; world = wd;
        more_qr_on = !(getenv("BA_MOREQR_QR") != nullptr && atoi(getenv("BA_MOREQR_QR")) == 0);
        if (iterative() && wd > 1) return BA_ERR_ARG; // (a sharded PCG would need an all-reduce of a D-vector per iteration)
        int rc = ba_build_structure(p, rk, wd, BA_CHUNK, 32 /* lanes of a k_cam_gram group */, &sx, /*pairs*/ !iterative());
        if (rc) return rc;
        N = p->N; D = 9 * N; Ml = sx.Ml; Kl = sx.Kl;
        Dp = ((D + NAUG + NB - 1) / NB) * NB;
        ld = Dp + 64;
        gK = (Kl + 255) / 256; gM = (Ml + 255) / 256;
        if (gK < 1) gK = 1;
        if (gM < 1) gM = 1;
        gB = (int)(((size_t)Ml * 8 + 255) / 256);
        if (gB < 1) gB = 1;
        gE = gK;
        std::vector<int> eb;
        ba_plan_eval_ranges(sx, eb);
        if (!eb.empty()) {
            gE = (int)eb.size() - 1;
            if ((rc = d_eb.upload(eb))) return rc;
            fuse = getenv("BA_NO_FUSE") == nullptr;
        }
        if (!chol_elim() && sx.kmax > 1024) return BA_ERR_ARG; // more than 1024 observations of one point: not supported by k_elim_qr
        if (!st) { HIPCHK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking)); own_stream = true; }
        for (auto &e : ev) HIPCHK(hipEventCreate(&e));
        for (auto &sl : ring)
            for (auto &e : sl.e) HIPCHK(hipEventCreate(&e));
        HIPCHK(hipHostMalloc((void **)&h_lam, sizeof(T)));
        // the LM table rows and the progress counter the control kernel writes: pinned, mapped, coherent host memory
        HIPCHK(hipHostMalloc((void **)&h_log, sizeof(ba_lm_host), hipHostMallocMapped | hipHostMallocCoherent));
        memset((void *)h_log, 0, sizeof(ba_lm_host));
        HIPCHK(hipHostGetDevicePointer((void **)&d_log, (void *)h_log, 0));
        use_graph = getenv("BA_NO_GRAPH") == nullptr;
        no_fold = getenv("BA_NO_FOLD") != nullptr;
        trial_head = getenv("BA_TRIAL_HEAD") != nullptr && atoi(getenv("BA_TRIAL_HEAD")) != 0;
        rec_coop = getenv("BA_REC_PLAIN") == nullptr;
        dbg_qrcheck = getenv("BA_DBG_QRCHECK") != nullptr;
        dist_factor = getenv("BA_DIST_FACTOR") != nullptr && atoi(getenv("BA_DIST_FACTOR")) != 0;
        if (const char *wd = getenv("BA_WATCHDOG_S")) { const double v = atof(wd); if (v > 0) watchdog_s = v; }
        {
            int dev = 0;
            hipDeviceProp_t pr;
            if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&pr, dev) == hipSuccess && pr.multiProcessorCount > 0)
                num_cus = pr.multiProcessorCount;
            int khz = 0; // rate of wall_clock64(), the constant-frequency counter behind the per-trial device times (100 MHz on gfx950)
            if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, dev) == hipSuccess && khz > 0) wall_khz = khz;
        }
#define UP(buf, vec) if ((rc = buf.upload(vec))) return rc
        UP(d_obs_cam, sx.obs_cam); UP(d_obs_pt, sx.obs_pt); UP(d_pt_ptr, sx.pt_ptr); UP(d_pair_hi, sx.pair_hi); // (BA_ITERSCHUR: no pairs)
        UP(d_pair_lo, sx.pair_lo);
        UP(d_pair_chunk_ptr, sx.pair_chunk_ptr); UP(d_dchunk_ptr, sx.dchunk_ptr); UP(d_cam_dchunk_ptr, sx.cam_dchunk_ptr);
        UP(d_cam_obs, sx.cam_obs); UP(d_qr_pts, sx.qr_pts);
#undef UP
        if (!iterative()) {
            // Records beyond the Infinity Cache (256 MB; config 5: 1 GB): the kernel is bound by the traffic between the L2s and
            // memory, and fewer wavefronts in flight walking the pair list side by side leave more of a row camera's records in the
            // L2 (2.23 -> 2.07 ms at config 5; nothing either way at config 4, whose 58 MB of records stay in the Infinity Cache).
            if ((unsigned long long)Kl * BA_REC * sizeof(T) > (256ull << 20)) { schur_wgs = 2; schur_window = 1; }
            if (const char *ev = getenv("BA_SCHUR_WGS")) schur_wgs = std::max(1, std::min(8, atoi(ev)));
            if (const char *ev = getenv("BA_SCHUR_BANDS")) schur_bands = atoi(ev);
            if (const char *ev = getenv("BA_SCHUR_WINDOW")) schur_window = std::max(0, atoi(ev));
            if (N > 65535) return BA_ERR_ARG; // (hi | lo << 16 in the chunk descriptor; a reduced matrix of that size would not fit anyway)
            if ((unsigned long long)Kl * BA_REC * sizeof(T) >= 0xf0000000ull) return BA_ERR_ARG; // 32-bit record offsets: <= 15 M observations per shard (fp64)
            {
                // every wavefront of the persistent grid must be resident at once (the dealing assumes they run side by side)
                int nb = 0;
                const hipError_t oe = kind == BA_CHOLESKY ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, k_schur_pairs<T, true>, 256, 0)
                                                          : hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, k_schur_pairs<T, false>, 256, 0);
                if (oe == hipSuccess && nb >= 1) schur_wgs = std::min(schur_wgs, nb);
            }
            ba_schur_plan sp; // the chunks dealt to the wavefronts of the persistent pair kernel
            ba_plan_schur(sx, schur_wgs, num_cus, schur_bands, schur_window, sp);
            schur_grid = sp.grid; schur_nband = sp.nband;
            if ((rc = d_wave_ptr.upload(sp.wave_ptr))) return rc;
            nred = (int)sp.red_pairs.size();
            if ((rc = d_red_pairs.upload(sp.red_pairs))) return rc;
            static_assert(sizeof(int4) == 4 * sizeof(int) && sizeof(int2) == 2 * sizeof(int), "ba_schur_plan: 4 ints per chunk, 2 per entry");
            if ((rc = d_chunk_info.upload_ints(sp.chunk_info)) || (rc = d_ent.upload_ints(sp.ent))) return rc;
        }
        // parameters: bundle_adjustment_large.cpp:81-107 (K00 = -f, R = Rodrigues(omega), distortion (k1 f^2, k2 f^4))
        std::vector<T> cam((size_t)15 * N), pts((size_t)3 * (Ml > 0 ? Ml : 1)), meas((size_t)2 * (Kl > 0 ? Kl : 1));
        for (int i = 0; i < N; i++) {
            const double *c = &p->cams9[9 * (size_t)i];
            T om[3] = {(T)c[0], (T)c[1], (T)c[2]}, R[9];
            host_rodrigues<T>(om, R);
            for (int q = 0; q < 9; q++) cam[(size_t)q * N + i] = R[q];
            for (int q = 0; q < 3; q++) cam[(size_t)(9 + q) * N + i] = (T)c[3 + q];
            const T f = (T)c[6], k1 = (T)c[7], k2 = (T)c[8], f2 = f * f;
            cam[(size_t)12 * N + i] = -f / (T)1.0;
            cam[(size_t)13 * N + i] = k1 * f2;
            cam[(size_t)14 * N + i] = k2 * f2 * f2;
        }
        for (int j = 0; j < Ml; j++)
            for (int q = 0; q < 3; q++) pts[(size_t)q * Ml + j] = (T)p->pts[3 * (size_t)(sx.p0 + j) + q];
        for (int i = 0; i < Kl; i++) {
            const int src = sx.perm[sx.o0 + i];
            meas[i] = (T)p->meas[2 * (size_t)src];              // / avg_focal_length (= 1.0, :35,72)
            meas[(size_t)Kl + i] = (T)p->meas[2 * (size_t)src + 1];
        }
        if ((rc = d_cam[0].upload(cam)) || (rc = d_cam[1].upload(cam)) || (rc = d_pts[0].upload(pts)) ||
            (rc = d_pts[1].upload(pts)) || (rc = d_meas.upload(meas)))
            return rc;
        const size_t K1 = Kl > 0 ? Kl : 1, M1 = Ml > 0 ? Ml : 1;
#define AL(buf, n) if ((rc = buf.alloc(n))) return rc
        AL(d_r, 2 * K1); if (!chol_elim()) AL(d_Jc, 18 * K1); /* CHOLESKY, ITERSCHUR: JcA alone */ AL(d_JcA, 20 * K1); AL(d_Jp, 6 * K1); AL(d_U0, 6 * M1); AL(d_gp, 3 * M1);
        AL(d_V, (size_t)81 * N); AL(d_gc, (size_t)D);
        if (kind == BA_MOREQR) { AL(d_rec0, (size_t)BA_REC * K1); AL(d_dinv0, 3 * M1); AL(d_tvec0, 3 * M1); AL(d_tri0, 6 * M1); }
        if ((rc = d_lm.alloc(1))) return rc;
        if ((rc = d_pperm.upload(std::vector<int>(M1, 0 | (1 << 2) | (2 << 4))))) return rc; // identity (CHOLESKY never pivots)
        if (dense_qr()) {
            {
                // k_qr_backsolve keeps the D right-hand sides and a 64 x 64 triangle in dynamic LDS: a D whose request exceeds the
                // device's limit per workgroup (MI355X: 160 KiB, fp64 D <= 16 320) is refused -- its launch would fail
                int dev = 0, lim = 0;
                HIPCHK(hipGetDevice(&dev));
                HIPCHK(hipDeviceGetAttribute(&lim, hipDeviceAttributeMaxSharedMemoryPerBlock, dev));
                if (sizeof(T) * ((size_t)D + 64 + 64 * 64) > (size_t)lim) return BA_ERR_ARG;
            }
            {
                // diagnostic switch BA_QR_HW_SQRT (ba_qr.hip.h: ba_qr_sqrt), written at every creation: the flag is process-global
                const char *ev = getenv("BA_QR_HW_SQRT");
                const int on = ev ? atoi(ev) : 0; // 0 (default): v_sqrt_f32 + one Newton step, 1: the bare instruction, 2: sqrtf
                HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(ba_qr_hw_sqrt_flag), &on, sizeof(int)));
            }
            // J2bot is dense: (2K + 3M + D) x (D + 1) scalars (config 3: 256 MB in fp32; a problem whose J2bot does not fit is refused)
            // (a camera may see a point more than once: k_qrkit_build / k_more_build add such observations' blocks up -- rounds 2 - 3 refused them)
            q_rows = std::max(outer_rows(), inner_rows());
            if (more_qr()) { AL(d_mQl, 9 * M1); AL(d_mQR, 9 * M1); AL(d_R22, (size_t)D * (D + 1)); }
            if (!getenv("BA_QR_ONE_STREAM")) {
                HIPCHK(hipStreamCreateWithFlags(&st_qr, hipStreamNonBlocking));
                for (auto &e : ev_qr) HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
            }
            q_lda = (size_t)q_rows + 64;
            q_tau_stride = (size_t)((std::max(q_rows, world * D) + ba_qr_cfg<T>::CH - 1) / ba_qr_cfg<T>::CH + 2) * BA_QR_PB * BA_QR_PB; // a 32 x 32 T factor per chunk (of J2bot's rows or, sharded, of the stack's)
            AL(d_qA, q_lda * (size_t)(D + 1)); AL(d_qtau, BA_QR_TAU_LEVELS * q_tau_stride); AL(d_q1obs, 6 * K1); AL(d_q1lam, 9 * M1);
            if (world > 1) AL(d_qB, qb_count());
        }
        AL(d_gcg, (size_t)D); AL(d_dslab, (size_t)BA_SLAB * (sx.ndchunks > 0 ? sx.ndchunks : 1));
        AL(d_rec, (size_t)BA_REC * K1); AL(d_dinv, 3 * M1); AL(d_tvec, 3 * M1); AL(d_tri, 6 * M1);
        if (iterative()) {
            // no S, Wp, Winv, flags or pair slab: the solution, the PCG vectors, the block-Jacobi inverses and fp64 block partials
            // (the camera pass's chunk partials live in d_dslab, which the linearisation has consumed by then)
            pcg_gc = (N + 255) / 256; pcg_gq = (int)(((size_t)9 * N + 255) / 256);
            if (pcg_gc < 1) pcg_gc = 1;
            if (pcg_gq < 1) pcg_gq = 1;
            AL(d_dxc, (size_t)D); AL(d_dxp, 3 * M1);
            AL(d_pcg_M, (size_t)81 * N); AL(d_pcg_b, (size_t)D); AL(d_pcg_r, (size_t)D); AL(d_pcg_z, (size_t)D); AL(d_pcg_p, (size_t)D);
            AL(d_pcg_y, (size_t)D); AL(d_pcg_w, 3 * M1);
            if ((rc = d_pcg_part.alloc((size_t)6 * pcg_gc + 2 * (size_t)pcg_gq))) return rc; // r'z (3 slots), |r|^2 (3 slots), p'Sp, |rhs - S x|^2
            if ((rc = d_pcg.alloc(1))) return rc;
            HIPCHK(hipMemset(d_pcg.p, 0, sizeof(ba_pcg_dev)));
        } else {
            AL(d_slab, (size_t)BA_SLAB * (sx.nchunks > 0 ? sx.nchunks : 1));
            AL(d_S, (size_t)ld * (Dp + 64)); AL(d_Wp, (size_t)ba_ldlt_wp_panels(D, NB) * ld * NB); /* the Y history of the fused steps (ba_ldlt_factor) */ AL(d_Winv, (size_t)((D + NB - 1) / NB) * NB * NB); AL(d_dxc, (size_t)2 * Dp + 2 * NB); /* the solution + the back sweep's hand-over vector */ AL(d_dxp, 3 * M1);
            if ((rc = d_flags.alloc((size_t)Dp / NB + 2))) return rc;
            // the trailing-update schedule of the fused factor: a function of D alone, made and uploaded here, once per solver
            ldlt_plan = ba_ldlt_make_plan(D + 1, D, NB);
            if ((rc = d_ldlt_jobs.upload(ldlt_plan.jobs))) return rc;
            ldlt_plan.d_jobs = d_ldlt_jobs.p;
        }
        AL(d_part_e, part_e_count(0, 0)); AL(d_part_pm, part_pm_count(0));
        AL(d_part_bs, (size_t)2 * gB); AL(d_part_st, (size_t)4 * gK); AL(d_scal, NSCAL);
#undef AL
        if (d_S.p) HIPCHK(hipMemset(d_S.p, 0, sizeof(T) * d_S.n));
        if (d_Wp.p) HIPCHK(hipMemset(d_Wp.p, 0, sizeof(T) * d_Wp.n));
        HIPCHK(hipMemset(d_scal.p, 0, sizeof(T) * NSCAL));
        HIPCHK(hipMemset(d_dxc.p, 0, sizeof(T) * d_dxc.n));
        HIPCHK(hipMemset(d_part_bs.p, 0, sizeof(T) * d_part_bs.n));
        HIPCHK(hipMemset(d_part_e.p, 0, sizeof(T) * d_part_e.n));
        HIPCHK(hipMemset(d_part_pm.p, 0, sizeof(T) * d_part_pm.n));
        HIPCHK(hipDeviceSynchronize());
        return BA_OK;
    }

    // Sum / max over the ranks that shard the problem, in place, ordered on the solver's stream: RCCL inside the library
    // (ba_solver_comm_init) or the host layer's callback (ba_solver_set_allreduce; the gloo tests).
    int allreduce(void *buf, size_t count, int op)
    {
        if (world <= 1 && !comm) return BA_OK;
        if (comm) return ba_rccl_allreduce(comm, buf, count, sizeof(T) == 8, op, (void *)st);
        if (!ar_fn) return BA_ERR_COMM;
        return ar_fn(ar_user, buf, count, sizeof(T) == 8 ? BA_F64 : BA_F32, op, (void *)st) ? BA_ERR_COMM : BA_OK;
    }
    bool sharded() const { return world > 1 || comm != nullptr; }
    // (round 4) the distributed factor's collectives: a broadcast from the owner of a block column, a reduce-scatter to the owners
    int bcast(void *buf, size_t count, int root)
    {
        if (world <= 1 && !comm) return BA_OK;
        if (comm) return ba_rccl_broadcast(comm, buf, count, sizeof(T) == 8, root, (void *)st);
        if (!ar_fn) return BA_ERR_COMM;
        return ar_fn(ar_user, buf, count, sizeof(T) == 8 ? BA_F64 : BA_F32, BA_OP_BCAST | (root << 8), (void *)st) ? BA_ERR_COMM : BA_OK;
    }
    int reduce_scatter(void *buf, size_t count_per_rank)
    {
        if (world <= 1 && !comm) return BA_OK;
        if (comm) return ba_rccl_reduce_scatter(comm, buf, count_per_rank, sizeof(T) == 8, rank, (void *)st);
        if (!ar_fn) return BA_ERR_COMM;
        return ar_fn(ar_user, buf, count_per_rank, sizeof(T) == 8 ? BA_F64 : BA_F32, BA_OP_REDUCE_SCATTER, (void *)st) ? BA_ERR_COMM : BA_OK;
    }

    int fetch_scalars()
    {
        HIPCHK(hipMemcpyAsync(h_scal, d_scal.p, sizeof(T) * NSCAL, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        return check_device_error();
    }

    // The device error word (SC_ERR) of the scalars just read: a kernel's bounded wait for another workgroup of its launch ran
    // out (k_ldlt_step's row-update flag, k_ldlt_backflow's sentinel poll), so the step is garbage.  Loud, and cleared for the next call.
    int check_device_error()
    {
        if (h_scal[SC_ERR] == (T)0) return BA_OK;
        report_device_error((int)h_scal[SC_ERR]);
        h_scal[SC_ERR] = 0;
        (void)hipMemsetAsync(d_scal.p + SC_ERR, 0, sizeof(T), st);
        return BA_ERR_HIP;
    }
    static void report_device_error(int code)
    {
        fprintf(stderr, "ba_mi355x: device error %d: %s\n", code,
                code == BA_DEVERR_DIVERGED ? "k_lm_control: the shards did not take the same accept / stop decision"
                : code >= BA_DEVERR_SWEEP  ? "k_ldlt_backflow: an unknown of the backward sweep was never published"
                                           : "k_ldlt_step: the look-ahead update of a row block was never announced");
    }

    double ev_ms(hipEvent_t a, hipEvent_t b)
    {
        float ms = 0;
        if (hipEventElapsedTime(&ms, a, b) != hipSuccess) return 0;
        return ms;
    }
    double ev_ms(int a, int b) { return ev_ms(ev[a], ev[b]); }

    // which: 0 = x, 1 = xTest
    // commit (with jac, which = 1): the linearisation AT xTest also performs x = xTest (k_commit's copy rides on k_eval)
    // fused (with jac): the point part of the gradient and, CHOLESKY, the next trial's elimination in the same pass (k_eval<T, true, FUSE>)
    void launch_eval(bool jac, int which, const int *go = nullptr, bool commit = false, bool fused = false)
    {
        const T tau2 = md.loss_scale * md.loss_scale; // (the square of the loss's scale: tau^2 of the reference's psi by default)
        ba_fuse_args<T> fa{};
        fa.eb = d_eb.p; // (nullptr when a point has more than 256 observations: plain runs of 256)
        fa.pt_ptr = d_pt_ptr.p; fa.lam = d_scal.p + SC_LAMBDA; fa.U0 = d_U0.p; fa.gp = d_gp.p;
        fa.rec = d_rec.p; fa.dinv = d_dinv.p; fa.tvec = d_tvec.p; fa.tri = d_tri.p; fa.fresh = &d_lm.p->rec_fresh;
        fa.cmask = mk.cmask.p; fa.pfix = mk.pfix.p;
        fa.wobs = ac.on() ? ac.weff.p : md.wobs.p; fa.loss = md.loss_kind; fa.lscale = md.loss_scale;
        // (CHOLESKY keeps the camera blocks in the AoS records alone: SOA = false, d_Jc is not even allocated)
        // eval_coop: the fused CHOLESKY linearisation stores its records a wavefront's run at a time (FUSE = 3 in place of 2) -- except in
        // fp32 on a problem of one round of workgroups, where it measured 2 % slower than the owners' stores (profiles/EXPERIMENTS.md, 7)
        const bool eval_coop = rec_coop && !(sizeof(T) == 4 && gE <= 2 * num_cus);
        auto launch = [&](auto JAC, auto FUSE, auto SOA, auto MASK, auto MODEL) {
            hipLaunchKernelGGL((k_eval<T, JAC(), FUSE(), SOA(), MASK(), MODEL()>), dim3(gE), dim3(256), 0, st, Kl, N, Ml, d_cam[which].p, d_pts[which].p,
                               d_obs_cam.p, d_obs_pt.p, d_meas.p, tau2, d_r.p, d_Jc.p, d_Jp.p, d_JcA.p, d_part_e.p, go, commit ? d_cam[0].p : (T *)nullptr,
                               commit ? d_pts[0].p : (T *)nullptr, fa);
        };
        // masked: the instantiations that zero the fixed columns (ba_solver_set_constant); the residual-only evaluation has no columns
        // model(): the instantiations of the general measurement model (ba_solver_set_loss / ba_solver_set_obs_weights); the reference's
        // psi at 0.5 px without weights stays on the kernels it always ran
        auto linearisation = [&](auto FUSE, auto SOA) {
            with_flags(mk.on, model(), [&](auto MASK, auto MODEL) { launch(std::true_type{}, FUSE, SOA, MASK, MODEL); });
        };
        constexpr std::false_type aos{};
        constexpr std::true_type soa{};
        // the five (FUSE, SOA) pairs that exist, and no other
        if (!jac) with_flag(model(), [&](auto MODEL) { launch(std::false_type{}, int_c<0>{}, soa, std::false_type{}, MODEL); });
        else if (chol_elim()) {
            if (!(fused && fuse)) linearisation(int_c<0>{}, aos);
            else if (eval_coop) linearisation(int_c<3>{}, aos);
            else linearisation(int_c<2>{}, aos);
        }
        else if (fused && fuse) linearisation(int_c<1>{}, soa);
        else linearisation(int_c<0>{}, soa);
    }

    // tail: the energy reduction that closes the linearisation, as one more block of the last launch (+ the control segment's end stamp)
    // next_trial (tail_prepares(), behind the step control): the next trial's records on the rejected path and its pair assembly on
    // both ride here -- the assembly in ONE launch with the camera Gram (k_pairs_gram)
    void launch_grad(const int *go = nullptr, const ba_red_job *tail = nullptr, bool points = true /* false: the fused k_eval has done them */,
                     bool next_trial = false)
    {
        if (next_trial) {
            if constexpr (sizeof(T) == 8) { // (tail_prepares() says so)
                launch_eliminate(&d_lm.p->elim_skip); // rejected step: the records at the new lambda (accepted: the fused k_eval has left them)
                const ba_tail_grid tg = ba_plan_tail_grid(schur_grid, sx.ndchunks);
                hipLaunchKernelGGL((k_pairs_gram<T>), dim3(tg.pair_wgs + tg.gram_wgs), dim3(256), 0, st, tg.pair_wgs, (const int *)&d_lm.p->asm_go, d_wave_ptr.p,
                                   schur_nband, d_chunk_info.p, d_ent.p, d_rec.p, (unsigned)(sizeof(T) * d_rec.n), d_tvec.p, Ml, d_slab.p, d_V.p, d_gc.p, D, ld,
                                   d_S.p, go, sx.ndchunks, Kl, d_dchunk_ptr.p, d_cam_obs.p, d_JcA.p, d_dslab.p);
            }
        } else if (!points) {
            if (sx.ndchunks > 0)
                hipLaunchKernelGGL((k_cam_gram<T>), dim3((sx.ndchunks + 7) / 8), dim3(256), 0, st, sx.ndchunks, Kl,
                                   d_dchunk_ptr.p, d_cam_obs.p, d_JcA.p, d_dslab.p, go);
        } else if (sx.ndchunks > 0 && gM <= 2 * num_cus && !no_fold) // a point part of one round of workgroups: both in one launch (k_grad_prep)
            hipLaunchKernelGGL((k_grad_prep<T>), dim3(gM + (sx.ndchunks + 7) / 8), dim3(256), 0, st, gM, Ml, Kl, d_pt_ptr.p, d_Jp.p, d_r.p, d_U0.p, d_gp.p,
                               d_part_pm.p, sx.ndchunks, d_dchunk_ptr.p, d_cam_obs.p, d_JcA.p, d_dslab.p, go);
        else {
            hipLaunchKernelGGL((k_point_prep<T>), dim3(gM), dim3(256), 0, st, Ml, Kl, d_pt_ptr.p, d_Jp.p, d_r.p, d_U0.p, d_gp.p, d_part_pm.p, go);
            if (sx.ndchunks > 0)
                hipLaunchKernelGGL((k_cam_gram<T>), dim3((sx.ndchunks + 7) / 8), dim3(256), 0, st, sx.ndchunks, Kl,
                                   d_dchunk_ptr.p, d_cam_obs.p, d_JcA.p, d_dslab.p, go);
        }
        hipLaunchKernelGGL((k_cam_gram_reduce<T>), dim3((N * BA_SLAB + 255) / 256 + (tail ? 1 : 0)), dim3(256), 0, st, N, d_cam_dchunk_ptr.p,
                           d_dslab.p, d_V.p, d_gc.p, go, tail ? *tail : ba_red_job{nullptr, 0, 0, 0}, d_scal.p, tail ? &d_lm.p->t_end : (long long *)nullptr);
    }

    // The launch sequence of a linearisation at the state `which` (linearize_enqueue; time_phase 1 and 8): r, J and the energy partials,
    // the gradient and the block diagonals, then what joins them in place.
    //   priors: behind the linearisation's launches, in front of the trial's k_elim_chol (fused_records());
    //   relative-pose constraints: records, then the per-camera gather into V / gc.  They touch no point block, so the fused pass's
    //   elimination records stay valid (fused_records()): V and gc are first read by the assembly / the PCG preparation of the trial.
    void launch_linearisation(int which, const int *go, bool commit, bool fused, const ba_red_job *tail, bool points, bool next_trial = false)
    {
        launch_eval(true, which, go, commit, fused);
        launch_grad(go, tail, points, next_trial);
        if (priors()) launch_prior(true, which, go);
        if (relposes()) launch_relpose(true, which, go);
    }

    // m_functor(x, r); energy; m_functor.df(x, J); JtRes; column norms (BacktrackLevMarqQRChol.h:257-280), host-synchronous
    int linearize(double *energy, double *diag_max) override
    {
        int rc;
        vf.results_dropped();
        if ((rc = linearize_enqueue(diag_max != nullptr, nullptr))) return rc;
        vf.pending_taken();
        if (more_qr() && (rc = more_outer_finish(nullptr))) return rc;
        if (sharded()) { // the kernels left this shard's part in SC_ELOC (it also rides on the next trial's packed all-reduce)
            HIPCHK(hipMemcpyAsync(d_scal.p + SC_ENERGY, d_scal.p + SC_ELOC, sizeof(T), hipMemcpyDeviceToDevice, st));
            if ((rc = allreduce(d_scal.p + SC_ENERGY, 1, 0))) return rc;
        }
        if (diag_max && (rc = allreduce(d_scal.p + SC_DMAX_P, 1, 1))) return rc;
        if ((rc = fetch_scalars())) return rc;
        HIPCHK(hipGetLastError());
        tm.linearize_ms += ev_ms(EV_L0, EV_L1);
        tm.n_linearize++;
        if (energy) *energy = (double)h_scal[SC_ENERGY];
        if (diag_max) *diag_max = std::max((double)h_scal[SC_DMAX_P], (double)h_scal[SC_DMAX_C]);
        vf.linearised();
        return BA_OK;
    }

    // The launches of the linearisation at x.  go != nullptr: conditional on the device-side step control (the kernels return
    // at once unless the trial in front of them was accepted).  The energy lands in SC_ENERGY, or -- sharded -- this shard's part
    // in SC_ELOC.
    int linearize_enqueue(bool want_dmax, const int *go, bool next_trial = false)
    {
        int rc;
        if (!go) HIPCHK(hipEventRecord(ev[EV_L0], st));
        // behind a trial (go != nullptr): the linearisation is AT xTest and carries x = xTest along (no k_commit launch), and the
        // energy sum rides on the last launch of launch_grad (no k_reduce_scalars launch) unless MOREQR's outer QR follows it
        ba_red_jobs jobs{};
        int nj = 0;
        jobs.j[nj++] = {d_part_e.p, part_e_n(), 0, sharded() ? SC_ELOC : SC_ENERGY};
        const bool tail = go != nullptr && !want_dmax && kind != BA_MOREQR && !priors() && !relposes(); // (their energy partials come behind launch_grad)
        // behind a trial the point part of J^T r / J^T J and (CHOLESKY) the elimination of the next trial are part of the k_eval launch;
        // the first, host-synchronous linearisation (lambda0 is not known yet, max diag J^T J is wanted) keeps the separate launches
        const bool fz = fuse && go != nullptr && !want_dmax;
        launch_linearisation(go ? 1 : 0, go, go != nullptr, fz, tail ? &jobs.j[0] : nullptr, !fz, next_trial);
        if (kind == BA_MOREQR) { // m_solver.compute(J) + Q^T r, once per outer iteration (BacktrackLevMarqMore.h:288-291): the point blocks ...
            launch_elim_qr(d_scal.p + SC_ZERO, d_rec0.p, d_dinv0.p, d_tvec0.p, d_tri0.p, go, /*thin Q for J2bot*/ more_qr());
            if (more_qr() && (rc = launch_more_outer(go))) return rc; // ... and the dense QR of J2bot(lambda = 0); its part 2 follows where a collective may stand
        }
        if (tail) { vf.step_dropped(); return BA_OK; }
        if (want_dmax) {
            // max diag(J^T J): point part per shard, camera part from the (summed over shards) diagonal of J_c^T J_c
            T *tmp = d_dxc.p;
            hipLaunchKernelGGL((k_vdiag<T>), dim3((D + 255) / 256), dim3(256), 0, st, N, d_V.p, tmp);
            if ((rc = allreduce(tmp, (size_t)D, 0))) return rc;
            jobs.j[nj++] = {d_part_pm.p, part_pm_n(), 1, SC_DMAX_P};
            jobs.j[nj++] = {tmp, D, 1, SC_DMAX_C};
        }
        hipLaunchKernelGGL((k_reduce_scalars<T>), dim3(nj), dim3(256), 0, st, jobs, d_scal.p, go, &d_lm.p->t_end);
        if (!go) HIPCHK(hipEventRecord(ev[EV_L1], st));
        vf.step_dropped();
        return BA_OK;
    }

    // skip != nullptr: the launch behind the step control (launch_grad, next_trial); it leaves at once where *skip != 0
    void launch_eliminate(const int *skip = nullptr)
    {
        if (chol_elim()) {
            // (Marquardt never meets the fused linearisation's records: they were made at lambda I, and fused_records() says so)
            with_flags(marq(), rec_coop, [&](auto MARQ, auto COOP) {
                hipLaunchKernelGGL((k_elim_chol<T, MARQ(), COOP()>), dim3(gK), dim3(256), 0, st, Kl, Ml, d_obs_pt.p, d_pt_ptr.p, d_JcA.p, d_Jp.p,
                                   d_U0.p, d_gp.p, d_scal.p + SC_LAMBDA, d_rec.p, d_dinv.p, d_tvec.p, d_tri.p,
                                   skip ? skip : fused_records() ? (const int *)&d_lm.p->rec_fresh : (const int *)nullptr, damp_args());
            });
        } else if (kind == BA_MOREQR) {
            if (Kl > 0) // BacktrackLevMarqMore.h:297-345, the per-trial QR of [R ; sqrt(lambda) I]
                hipLaunchKernelGGL((k_more_trial<T>), dim3(gK), dim3(256), 0, st, Kl, Ml, d_obs_pt.p, d_pt_ptr.p, d_scal.p + SC_LAMBDA,
                                   d_rec0.p, d_tri0.p, d_tvec0.p, d_rec.p, d_dinv.p, d_tvec.p, d_tri.p, d_mQl.p, d_mQR.p);
        } else {
            launch_elim_qr(d_scal.p + SC_LAMBDA, d_rec.p, d_dinv.p, d_tvec.p, d_tri.p, nullptr, dense_qr());
        }
    }

    // per-point QR, one launch per non-empty track-length bucket (ba_structure: lanes per point x observations per lane)
    void launch_elim_qr(const T *lam, T *rec, T *dinv, T *tvec, T *tri, const int *go, bool thin_q = false)
    {
        T *qo = thin_q ? d_q1obs.p : nullptr, *ql = thin_q ? d_q1lam.p : nullptr;
#define BA_QR(B, L, SLOTS)                                                                                                       \
        if (sx.qr_bucket_ptr[B + 1] > sx.qr_bucket_ptr[B]) {                                                                   \
            const int np_ = sx.qr_bucket_ptr[B + 1] - sx.qr_bucket_ptr[B];                                                       \
            hipLaunchKernelGGL((k_elim_qr<T, L, SLOTS>), dim3(((size_t)np_ * L + 255) / 256), dim3(256), 0, st, np_,           \
                               d_qr_pts.p + sx.qr_bucket_ptr[B], Ml, Kl, d_pt_ptr.p, d_Jc.p, d_Jp.p, d_r.p, lam, rec, dinv, tvec, tri, go, qo, ql, d_pperm.p); \
        }
        BA_QR(0, 8, 4)
        BA_QR(1, 16, 4)
        BA_QR(2, 32, 4)
        BA_QR(3, 64, 4)
        BA_QR(4, 64, 16)
#undef BA_QR
    }

    // single shard: k_post_reduce's work rides on the two Schur launches (see k_schur_reduce)
    bool post_folded() const { return !sharded() && nred > 0 && !no_fold; }
    bool ctl_reduces() const { return !sharded() && !no_fold; }

    // pairs = false: the tail of the iteration in front of this trial has run them (tail_prepares())
    void launch_schur(bool pairs = true)
    {
        const T *lamf = post_folded() ? d_scal.p + SC_LAMBDA : nullptr;
        if (pairs && sx.nchunks > 0) {
            // persistent: schur_wgs workgroups per CU, every wavefront walks its own balanced list of chunks (see k_schur_pairs)
            const dim3 gp(schur_grid);
#define BA_PAIRS(SC) hipLaunchKernelGGL((k_schur_pairs<T, SC>), gp, dim3(256), 0, st, d_wave_ptr.p, schur_nband, d_chunk_info.p, d_ent.p, d_rec.p, \
                                                  (unsigned)(sizeof(T) * d_rec.n), d_tvec.p, Ml, d_slab.p, d_V.p, d_gc.p, D, ld, d_S.p)
            // SCALED: CHOLESKY is the only symbol whose point blocks carry a diagonal D (dinv != 1)
            if (kind == BA_CHOLESKY) BA_PAIRS(true); else BA_PAIRS(false);
#undef BA_PAIRS
        }
        const int post_blocks = lamf ? (Dp + 2) / 3 : 0;
        const long long nthr = (long long)nred * BA_SLAB;
        if (nred > 0)
            with_flag(marq(), [&](auto MARQ) {
                hipLaunchKernelGGL((k_schur_reduce<T, MARQ()>), dim3((unsigned)((nthr + 191) / 192) + post_blocks), dim3(192), 0, st, nred, d_red_pairs.p, D,
                                   ld, d_pair_hi.p, d_pair_lo.p, d_pair_chunk_ptr.p, d_slab.p, d_V.p, d_gc.p, d_S.p, lamf, post_blocks, Dp, d_gcg.p, d_dxc.p,
                                   damp_args());
            });
        // every block of this S is written: the constraints' cross blocks join it here, for a trial and for the covariance alike
        if (relposes())
            hipLaunchKernelGGL((k_relpose_schur<T>), dim3((unsigned)(((size_t)rp.n * 36 + 255) / 256)), dim3(256), 0, st, rp.n, (const int *)rp.pair.p,
                               (const T *)rp.rec.p, ld, d_S.p);
    }

    // ---- distributed factor (BA_DIST_FACTOR=1, sharded LDL^T symbols; SURVEY 8e "consider distributing K6" -- FUNCTIONAL, unmeasured: this
    // pool gives one GPU).  1-D block-cyclic over the ranks: rank p % world owns block column p.
    //   exchange (round 4): every rank only needs the SUM of the block columns it owns, so the shards' partial
    //   systems meet in a REDUCE-SCATTER -- the trapezoid packed owner by owner into world chunks of equal length (k_pack_owner), half
    //   the bytes of the all-reduce per rank -- and the camera gradient + energy (D + 1 scalars, needed everywhere) in a small all-reduce;
    //   factor: per block column the owner factors it (k_ldlt_panel: L into S, Y = L D into Wp, the block's inverse into Winv), the
    //   three pieces travel in ONE broadcast from the owner (staged contiguously, k_panel_stage; round 3: three sum all-reduces of zeroed
    //   copies), and every rank applies the panel to the block columns IT owns (k_ldlt_update with the owner filter).
    // Behind the last column every rank holds the whole L and runs the back sweep redundantly.  The launch-per-step kernels: nobody
    // waits for anybody inside a launch; one collective per block column on the factor's critical path -- a design to measure once
    // there is a node, not a speed claim (at D = 2313 the factor is latency-bound and every hop is on its critical path).
    bool dist_factor = false;
    DevBuf<T> d_stage;       // one block column's [L | Y | W] for the broadcast
    DevBuf<int> d_own_off;   // per block column: offset of its first scalar in the owner-packed buffer, as a count of 64-scalar units (fits 32 bits)
    size_t own_chunk = 0;    // scalars per rank in the owner-packed buffer
    bool dist_on() const { return dist_factor && sharded() && !dense_qr(); }
    int dist_setup()
    {
        if (d_own_off.p) return BA_OK;
        static_assert(NB == 64, "k_pack_owner counts its offsets in units of 64 scalars");
        std::vector<int> off;
        own_chunk = ba_plan_owner_offsets(Dp, NB, world, off);
        int rc;
        if ((rc = d_own_off.upload(off))) return rc;
        if ((rc = d_pack.alloc((size_t)world * own_chunk + (size_t)D + 2))) return rc; // behind the chunks: g_c (D) + the energy
        return d_stage.alloc((size_t)(2 * (size_t)ld + NB) * NB);
    }
    size_t dist_small_off() const { return (size_t)world * own_chunk; }
    // segment A's tail / segment B's head in this mode
    int launch_dist_pack()
    {
        int rc;
        if ((rc = dist_setup())) return rc;
        HIPCHK(hipMemsetAsync(d_pack.p, 0, sizeof(T) * (size_t)world * own_chunk, st)); // (the padding behind the shorter chunks)
        const dim3 g((Dp + 255) / 256 > 8 ? 8 : (Dp + 255) / 256, Dp);
        hipLaunchKernelGGL((k_pack_owner<T, false>), g, dim3(256), 0, st, Dp, D, ld, d_S.p, d_pack.p, d_own_off.p, world, rank, dist_small_off(), d_scal.p,
                           (int)SC_ELOC, (int)SC_ENERGY);
        return BA_OK;
    }
    int launch_dist_unpack()
    {
        const dim3 g((Dp + 255) / 256 > 8 ? 8 : (Dp + 255) / 256, Dp);
        hipLaunchKernelGGL((k_pack_owner<T, true>), g, dim3(256), 0, st, Dp, D, ld, d_S.p, d_pack.p, d_own_off.p, world, rank, dist_small_off(), d_scal.p,
                           (int)SC_ELOC, (int)SC_ENERGY);
        return BA_OK;
    }
    int dist_exchange()
    {
        int rc;
        if ((rc = reduce_scatter(d_pack.p, own_chunk))) return rc;
        return allreduce(d_pack.p + dist_small_off(), (size_t)D + 1, 0);
    }
    int launch_factor_solve_dist()
    {
        const int nrows = D + 1, ncols = D, nblk = (ncols + NB - 1) / NB;
        int rc;
        for (int p = 0; p < nblk; p++) {
            const int p0 = p * NB, below = nrows - (p0 + NB), npanel = below > 0 ? (below + 63) / 64 : 1, owner = p % world;
            const int h = Dp - p0; // rows of the block column from its diagonal block down (the rhs row D among them)
            T *wcol = d_Wp.p, *winv = d_Winv.p + (size_t)p * NB * NB;
            const dim3 gs((h + 255) / 256, 2 * NB + 1);
            if (owner == rank) {
                hipLaunchKernelGGL((k_ldlt_panel<T, NB>), dim3(npanel), dim3(256), 0, st, nrows, ncols, ld, p0, d_S.p, wcol, winv, (int *)nullptr, 0);
                hipLaunchKernelGGL((k_panel_stage<T, NB, false>), gs, dim3(256), 0, st, h, p0, ld, d_S.p, wcol, winv, d_stage.p);
            }
            if ((rc = bcast(d_stage.p, (size_t)(2 * h + NB) * NB, owner))) return rc;
            if (owner != rank) hipLaunchKernelGGL((k_panel_stage<T, NB, true>), gs, dim3(256), 0, st, h, p0, ld, d_S.p, wcol, winv, d_stage.p);
            const int p1 = p0 + NB;
            if (p1 < ncols) {
                const int nti = (nrows - p1 + 63) / 64, ntj = (ncols - p1 + 63) / 64;
                hipLaunchKernelGGL((k_ldlt_update<T, NB>), dim3(ntj, nti), dim3(256), 0, st, nrows, ncols, ld, p0, d_S.p, (const T *)wcol, world, rank);
            }
        }
        ba_ldlt_backsweep<T, NB>(st, D, ld, D, d_S.p, d_Winv.p, d_dxc.p, d_dxc.p + Dp, /*armed by k_post_reduce*/ true, num_cus, d_scal.p + SC_ERR, /*safe*/ true);
        return BA_OK;
    }
    void launch_factor_solve() { launch_factor(); launch_backsweep(); }

    // QRKIT's right block (BAFunctor.h:101): J2bot built densely, Householder QR (ba_qr.hip.h), dx_c from R y = -Q^T qtb2
    void launch_qrkit_build()
    {
        if (more_qr()) { launch_more_build(); return; }
        (void)hipMemsetAsync(d_qA.p, 0, sizeof(T) * d_qA.n, st);
        const int nthr = std::max(Kl, D);
        hipLaunchKernelGGL((k_qrkit_build<T>), dim3((nthr + 255) / 256), dim3(256), 0, st, Kl, Ml, D, d_obs_cam.p, d_obs_pt.p, d_pt_ptr.p, d_Jc.p, d_r.p,
                           d_rec.p, d_q1obs.p, d_q1lam.p, d_tvec.p, d_scal.p + SC_LAMBDA, d_qA.p, q_lda, rank == 0 ? 1 : 0);
    }
    // MOREQR per trial (behind k_more_trial): the dense matrix the inner QR factors (k_more_build, k_more_tail)
    void launch_more_build()
    {
        (void)hipMemsetAsync(d_qA.p, 0, sizeof(T) * d_qA.n, st);
        if (Kl > 0)
            hipLaunchKernelGGL((k_more_build<T>), dim3(gK), dim3(256), 0, st, Kl, Ml, D, d_obs_cam.p, d_obs_pt.p, d_pt_ptr.p, d_rec0.p, d_rec.p, d_mQl.p, d_mQR.p,
                               d_tvec0.p, d_tvec.p, d_qA.p, q_lda);
        if (rank == 0) hipLaunchKernelGGL((k_more_tail<T>), dim3(D + 1), dim3(256), 0, st, Ml, D, d_R22.p, d_scal.p + SC_LAMBDA, d_qA.p, q_lda);
    }
    // MOREQR per outer iteration (behind k_elim_qr with lambda = 0; BacktrackLevMarqMore.h:288-291): the dense QR of J2bot(lambda = 0).
    // Part 1 (capturable): build + this shard's factorisation (+ sharded: its R | c2 into the zeroed stack).  Part 2: sharded -- the
    // all-reduce of the stack and its QR (distributed TSQR, like QRKIT's trial) --, then R22 | c2 out of the factored matrix.  Every
    // kernel is conditional on the step control (go): behind a rejected trial R22 stays what it was.
    int launch_more_outer(const int *go)
    {
        (void)hipMemsetAsync(d_qA.p, 0, sizeof(T) * d_qA.n, st);
        if (Kl > 0)
            hipLaunchKernelGGL((k_qrkit_build<T>), dim3((std::max(Kl, D) + 255) / 256), dim3(256), 0, st, Kl, Ml, D, d_obs_cam.p, d_obs_pt.p, d_pt_ptr.p, d_Jc.p, d_r.p,
                               d_rec0.p, d_q1obs.p, d_q1lam.p, d_tvec0.p, d_scal.p + SC_ZERO, d_qA.p, q_lda, 0, go);
        ba_qr_side sd = qr_side();
        sd.go = go;
        ba_qr_factor<T>(st, d_qA.p, q_lda, outer_rows(), D, d_qtau.p, q_tau_stride, sd);
        if (sharded()) {
            int rc;
            if (!d_qB.p && (rc = d_qB.alloc(qb_count()))) return rc;
            HIPCHK(hipMemsetAsync(d_qB.p, 0, sizeof(T) * qb_nmat(), st));
            hipLaunchKernelGGL((k_qr_stack_pack<T>), dim3(D + 2), dim3(256), 0, st, (const T *)d_qA.p, q_lda, D, rank, d_qB.p, qb_ld(), qb_nmat(), (const T *)d_gc.p,
                               (const T *)d_scal.p, (int)SC_ELOC);
        }
        return BA_OK;
    }
    int more_outer_finish(const int *go)
    {
        if (sharded()) {
            int rc;
            if ((rc = allreduce(d_qB.p, qb_count(), 0))) return rc;
            ba_qr_side sd = qr_side();
            sd.go = go;
            ba_qr_factor<T>(st, d_qB.p, qb_ld(), world * D, D, d_qtau.p, q_tau_stride, sd);
            hipLaunchKernelGGL((k_copy_r22<T>), dim3(D + 1), dim3(256), 0, st, D, (const T *)d_qB.p, qb_ld(), d_R22.p, go);
        } else
            hipLaunchKernelGGL((k_copy_r22<T>), dim3(D + 1), dim3(256), 0, st, D, (const T *)d_qA.p, q_lda, d_R22.p, go);
        return BA_OK;
    }
    bool dbg_qrcheck = false; // BA_DBG_QRCHECK
    DevBuf<T> d_qAcopy, d_dbgr, d_dbg2;
    void launch_qrkit_solve()
    {
        // BA_DBG_QRCHECK (diagnostic, step-level calls only): a copy of the matrix, and behind the solve its normal-equation residual (getter 14)
        const bool chk = dbg_qrcheck && step_level;
        if (chk) {
            if (!d_qAcopy.p) { (void)d_qAcopy.alloc(d_qA.n); (void)d_dbgr.alloc(q_lda); (void)d_dbg2.alloc((size_t)2 * D); }
            (void)hipMemcpyAsync(d_qAcopy.p, d_qA.p, sizeof(T) * d_qA.n, hipMemcpyDeviceToDevice, st);
        }
        ba_qr_solve<T>(st, d_qA.p, q_lda, inner_rows(), D, d_qtau.p, q_tau_stride, d_dxc.p, qr_side());
        if (chk) {
            const int rows = inner_rows();
            hipLaunchKernelGGL((k_dbg_resid<T>), dim3((rows + 255) / 256), dim3(256), 0, st, rows, D, (const T *)d_qAcopy.p, q_lda, (const T *)d_dxc.p, d_dbgr.p);
            hipLaunchKernelGGL((k_dbg_atv<T>), dim3(D), dim3(256), 0, st, rows, D, (const T *)d_qAcopy.p, q_lda, (const T *)d_dbgr.p, d_dbg2.p);
            hipLaunchKernelGGL((k_dbg_atv<T>), dim3(D), dim3(256), 0, st, rows, D, (const T *)d_qAcopy.p, q_lda, (const T *)(d_qAcopy.p + (size_t)D * q_lda), d_dbg2.p + D);
        }
        (void)hipMemcpyAsync(d_gcg.p, d_gc.p, sizeof(T) * (size_t)D, hipMemcpyDeviceToDevice, st); // the camera gradient of the rho denominator
    }
    // Sharded QRKIT (distributed TSQR, ba_qr.hip.h): the QR of this shard's rows, its R + rhs head into the zeroed stack ...
    int launch_qr_stack_pack()
    {
        int rc;
        if (!d_qB.p && (rc = d_qB.alloc(qb_count()))) return rc;
        ba_qr_factor<T>(st, d_qA.p, q_lda, inner_rows(), D, d_qtau.p, q_tau_stride, qr_side());
        HIPCHK(hipMemsetAsync(d_qB.p, 0, sizeof(T) * qb_nmat(), st));
        hipLaunchKernelGGL((k_qr_stack_pack<T>), dim3(D + 2), dim3(256), 0, st, (const T *)d_qA.p, q_lda, D, rank, d_qB.p, qb_ld(), qb_nmat(), (const T *)d_gc.p,
                           (const T *)d_scal.p, (int)SC_ELOC);
        return BA_OK;
    }
    // ... and, behind the all-reduce, the QR of the stack and the camera step (redundantly on every shard)
    void launch_qr_stack_solve()
    {
        hipLaunchKernelGGL((k_qr_stack_unpack<T>), dim3((D + 255) / 256), dim3(256), 0, st, (const T *)d_qB.p, qb_nmat(), D, d_gcg.p, d_scal.p, (int)SC_ENERGY);
        ba_qr_solve<T>(st, d_qB.p, qb_ld(), world * D, D, d_qtau.p, q_tau_stride, d_dxc.p, qr_side());
    }
    // what the exchange step of a sharded trial sums: the packed reduced camera system, or (QRKIT / QRSPQR) the stack of R factors
    T *xchg_ptr() { return dense_qr() ? d_qB.p : d_pack.p; }
    size_t xchg_count() const { return dense_qr() ? qb_count() : pack_count() + 1; }

    void launch_factor()
    {
        ba_ldlt_factor<T, NB>(st, D + 1, D, ld, d_S.p, d_Wp.p, d_Winv.p, d_flags.p, (int)d_flags.n, d_scal.p + SC_ERR, safe_factor,
                              safe_factor ? 0 : fault_rowflag, &ldlt_plan);
    }

    // backward sweep: one data-flow launch (k_ldlt_backflow) while its groups are certainly co-resident
    void launch_backsweep()
    {
        ba_ldlt_backsweep<T, NB>(st, D, ld, D, d_S.p, d_Winv.p, d_dxc.p, d_dxc.p + Dp, /*armed by k_post_reduce*/ true, num_cus, d_scal.p + SC_ERR,
                                 safe_factor);
    }

    void launch_post_reduce()
    {
        if (post_folded()) return;
        with_flag(marq(), [&](auto MARQ) { // (Marquardt is single shard: the diagonal of V is the diagonal of J_c'J_c)
            hipLaunchKernelGGL((k_post_reduce<T, MARQ()>), dim3((Dp + 3) / 4), dim3(256), 0, st, D, Dp, ld, d_scal.p + SC_LAMBDA, d_S.p, d_gcg.p, d_dxc.p,
                               (const T *)d_V.p, damp_args());
        });
    }

    // ---- BA_ITERSCHUR (ba_pcg.hip.h) ------------------------------------------------------------------------------------------------
    DevBuf<T> d_pcg_M /* [N][81] B_a, then B_a^-1 */, d_pcg_b /* reduced rhs */, d_pcg_r, d_pcg_z, d_pcg_p, d_pcg_y /* S p */, d_pcg_w /* [3][Ml] point pass */;
    DevBuf<double> d_pcg_part; // block partials: r'z [3][gc] | |r|^2 [3][gc] | p'Sp [gq] | |rhs - S x|^2 [gq]
    DevBuf<ba_pcg_dev> d_pcg;
    int pcg_gc = 1, pcg_gq = 1; // blocks of the per-camera and per-(camera, row) launches
    int pcg_max_iter = BA_PCG_MAX_ITER_DEFAULT;
    double pcg_rel_tol = BA_PCG_REL_TOL_DEFAULT;
    double pcg_eta = 0;            // ba_solver_set_pcg_model_tol: > 0 launches the *_q kernels (ba_pcg.hip.h)
    DevBuf<double> d_pcg_part_s;   // their block partials of x'(rhs + r) [3][gc], allocated by the first eta > 0
    bool qstop_on() const { return pcg_eta > 0; }
    // (with a forest the list of r'z is longer by one partial per tree and the four lists live in the forest's own buffer)
    int pcg_gz() const { return pcg_gc + (forest_on() ? fo.nparts() : 0); }
    double *pcg_part_rz() const { return forest_on() ? fo.part.p : d_pcg_part.p; }
    double *pcg_part_rr() const { return pcg_part_rz() + (size_t)3 * pcg_gz(); }
    double *pcg_part_py() const { return pcg_part_rr() + (size_t)3 * pcg_gc; }
    double *pcg_part_res() const { return pcg_part_py() + pcg_gq; }

    // ---- BA_PRECOND_CONSTRAINT_FOREST / BA_PRECOND_VISIBILITY_FOREST (ba_pcg_forest.hip.h; DESIGN.md sections 15, 16) --------------------
    // The lists of ba_relpose_forest_plan in elimination order, tree after tree, built by set_precond / set_relposes.  Without a kept
    // constraint there is no buffer and not one launch or argument differs from block Jacobi.  The visibility forest plans the list
    // L = the constraints, then the co-visibility pairs, has cross blocks of width 9 and the record pairs of every kept edge.
    struct Forest {
        DevBuf<int> tree_ptr, node_cam, node_par, node_rec, bad, edge_ptr, edge_oo;
        DevBuf<unsigned char> in_tree;
        DevBuf<T> fac, u;
        DevBuf<double> work, part, xc, tpart;
        int ntrees = 0, nodes = 0, kept = 0, dropped = 0, largest = 0, width = 6;
        // partials of r'z behind the per-camera ones: one per tree, width 9 one per 256 trees (k_pcg_forest_rz)
        int nparts() const { return width == 9 ? (ntrees + 255) / 256 : ntrees; }
        size_t bytes() const
        {
            return bytes_of(tree_ptr) + bytes_of(node_cam) + bytes_of(node_par) + bytes_of(node_rec) + bytes_of(bad) + bytes_of(in_tree) + bytes_of(fac) +
                   bytes_of(u) + bytes_of(work) + bytes_of(part) + bytes_of(edge_ptr) + bytes_of(edge_oo) + bytes_of(xc) + bytes_of(tpart);
        }
    } fo;
    int precond_kind = BA_PRECOND_BLOCK_JACOBI, precond_max_tree = BA_PCG_MAX_TREE_DEFAULT;
    bool forest_on() const { return precond_kind != BA_PRECOND_BLOCK_JACOBI && fo.ntrees > 0; }
    ba_forest_dev<T> forest_dev() const
    {
        return ba_forest_dev<T>{fo.tree_ptr.p, fo.node_cam.p, fo.node_par.p, fo.node_rec.p, fo.fac.p, fo.work.p, fo.u.p, fo.bad.p,
                                fo.edge_ptr.p, fo.edge_oo.p, fo.xc.p};
    }
    // the forest's launches by the cross blocks' width
    void launch_forest_edges()
    {
        hipLaunchKernelGGL((k_pcg_forest_edges<T>), dim3(fo.nodes), dim3(256), 0, st, forest_dev(), (const T *)d_rec.p, (const T *)rp.rec.p);
    }
    void launch_forest_factor()
    {
        with_flag(fo.width == 9, [&](auto W9) {
            hipLaunchKernelGGL((k_pcg_forest_factor<T, W9() ? 9 : 6>), dim3(fo.ntrees), dim3(64), 0, st, forest_dev(), (const T *)d_pcg_M.p, (const T *)rp.rec.p);
        });
    }
    template <bool START> void launch_forest_apply(double *part)
    {
        if (fo.width == 9) {
            hipLaunchKernelGGL((k_pcg_forest_apply<T, START, 9>), dim3(fo.ntrees), dim3(64), sizeof(T) * 9 * (size_t)std::min(fo.largest, BA_FOREST_LDS), st,
                               forest_dev(), (const T *)d_pcg_r.p, d_pcg_z.p, fo.tpart.p, (const ba_pcg_dev *)d_pcg.p);
            hipLaunchKernelGGL((k_pcg_forest_rz<START>), dim3(fo.nparts()), dim3(256), 0, st, (const double *)fo.tpart.p, fo.ntrees, part,
                               (const ba_pcg_dev *)d_pcg.p);
        } else
            hipLaunchKernelGGL((k_pcg_forest_apply<T, START>), dim3(fo.ntrees), dim3(64), 0, st, forest_dev(), (const T *)d_pcg_r.p, d_pcg_z.p, part,
                               (const ba_pcg_dev *)d_pcg.p);
    }
    // the forest of `pairs` under (kind, max_tree) into `out`; everything that can fail, nothing of the solver touched
    int build_forest(const std::vector<int> &rp_pairs, int kind, int max_tree, Forest &out) const
    {
        ba_forest_plan fp;
        int rc = ba_plan_forest(sx, rp_pairs, kind, max_tree, fp);
        if (rc) return rc;
        out.ntrees = fp.ntrees; out.nodes = fp.nodes; out.kept = fp.kept; out.dropped = fp.dropped; out.largest = fp.largest; out.width = fp.width;
        if (fp.kept == 0) return BA_OK;
        if (out.width == 9) {
            if ((rc = out.edge_ptr.upload(fp.edge_ptr)) || (rc = out.edge_oo.upload(fp.edge_oo)) || (rc = out.xc.alloc((size_t)out.nodes * 81)) ||
                (rc = out.tpart.alloc((size_t)out.ntrees))) {
                (void)hipGetLastError();
                return rc;
            }
            HIPCHK(hipMemset(out.xc.p, 0, sizeof(double) * out.xc.n));
            HIPCHK(hipMemset(out.tpart.p, 0, sizeof(double) * out.tpart.n));
        }
        if ((rc = out.tree_ptr.upload(fp.tree_ptr)) || (rc = out.node_cam.upload(fp.node_cam)) || (rc = out.node_par.upload(fp.node_par)) ||
            (rc = out.node_rec.upload(fp.node_rec)) || (rc = out.in_tree.upload(fp.in_tree)) || (rc = out.bad.alloc((size_t)out.ntrees)) ||
            (rc = out.fac.alloc((size_t)out.nodes * BA_FOREST_FAC(out.width))) || (rc = out.work.alloc((size_t)out.nodes * 81)) ||
            (rc = out.u.alloc(out.largest > BA_FOREST_LDS ? (size_t)out.nodes * 9 : 0)) ||
            (rc = out.part.alloc((size_t)3 * (pcg_gc + out.ntrees) + (size_t)3 * pcg_gc + 2 * (size_t)pcg_gq))) { (void)hipGetLastError(); return rc; }
        HIPCHK(hipMemset(out.bad.p, 0, sizeof(int) * out.bad.n));
        HIPCHK(hipMemset(out.part.p, 0, sizeof(double) * out.part.n));
        return BA_OK;
    }
    int set_precond(int kind, int max_tree) override
    {
        if (!iterative() || (kind != BA_PRECOND_BLOCK_JACOBI && kind != BA_PRECOND_CONSTRAINT_FOREST && kind != BA_PRECOND_VISIBILITY_FOREST) || max_tree < 0)
            return BA_ERR_ARG;
        if (max_tree == 0) max_tree = kind == BA_PRECOND_VISIBILITY_FOREST ? BA_PCG_VIS_MAX_TREE_DEFAULT : BA_PCG_MAX_TREE_DEFAULT;
        Forest nf;
        int rc;
        if ((rc = build_forest(rp.h_pair, kind, max_tree, nf))) return rc;
        HIPCHK(hipStreamSynchronize(st));
        fo = std::move(nf);
        precond_kind = kind; precond_max_tree = max_tree;
        drop_trial_graphs(); // (captured with the old launch sequence)
        return BA_OK;
    }
    int precond_info(long long *out6, int *fallback_trees) override
    {
        if (!iterative()) return BA_ERR_ARG;
        if (out6) {
            out6[0] = precond_kind; out6[1] = precond_max_tree; out6[2] = fo.ntrees; out6[3] = fo.kept; out6[4] = fo.dropped; out6[5] = fo.largest;
        }
        if (fallback_trees) {
            *fallback_trees = 0;
            if (forest_on()) {
                std::vector<int> h((size_t)fo.ntrees);
                HIPCHK(hipStreamSynchronize(st));
                HIPCHK(hipMemcpy(h.data(), fo.bad.p, sizeof(int) * h.size(), hipMemcpyDeviceToHost));
                for (int v : h) *fallback_trees += v;
            }
        }
        return BA_OK;
    }

    // ---- shared intrinsics (ba_solver_set_shared_intrinsics; ba_pcg_share.hip.h) -------------------------------
    // The lists of ba_intrinsics_group_plan with chunks of BA_SHARE_CHUNK members, laid into chunk slots, 8 to a workgroup of
    // k_pcg_share: a group of 2 .. BA_SHARE_LOCAL chunks never crosses a workgroup (empty slots in front of it where it would).
    // Without a group there is no buffer and not one launch differs from a solver that never had one.
    struct Share {
        int ngroups = 0, ngrouped = 0, largest = 0, nchunks = 0, nslots = 0, nwide = 0;
        DevBuf<ba_share_chunk> desc; // [nslots]
        DevBuf<int> members, wide;   // [ngrouped]; [nwide]: the slots of groups of more than BA_SHARE_LOCAL chunks
        DevBuf<double> part;         // [nslots][3]
        std::vector<int> h_gptr, h_members; // host copy: the refusals of set_state / set_constant
        size_t bytes() const { return bytes_of(desc) + bytes_of(members) + bytes_of(wide) + bytes_of(part); }
    } sh;
    bool share_on() const { return sh.ngroups > 0; }
    // v <- Pi v.  CHECK: a launch of the iteration, which returns at once behind convergence
    template <bool CHECK> void launch_share(T *v)
    {
        hipLaunchKernelGGL((k_pcg_share<T, CHECK>), dim3((sh.nslots + 7) / 8), dim3(256), 0, st, sh.nslots, (const ba_share_chunk *)sh.desc.p,
                           (const int *)sh.members.p, v, sh.part.p, (const ba_pcg_dev *)d_pcg.p);
        if (sh.nwide > 0)
            hipLaunchKernelGGL((k_pcg_share_wide<T, CHECK>), dim3((sh.nwide + 7) / 8), dim3(256), 0, st, sh.nwide, (const int *)sh.wide.p,
                               (const ba_share_chunk *)sh.desc.p, (const int *)sh.members.p, v, (const double *)sh.part.p, (const ba_pcg_dev *)d_pcg.p);
    }
    // true when the members of every group of (gptr, members) hold the same bits in f, k1, k2 of cam (SoA [15][N], rows 12..14)
    static bool share_equal(const std::vector<int> &gptr, const std::vector<int> &members, const T *cam, int N)
    {
        for (size_t g = 0; g + 1 < gptr.size(); g++)
            for (int m = gptr[g] + 1; m < gptr[g + 1]; m++)
                for (int q = 12; q < 15; q++)
                    if (std::memcmp(cam + (size_t)q * N + members[m], cam + (size_t)q * N + members[gptr[g]], sizeof(T)) != 0) return false;
        return true;
    }
    // ... and the same bits 6..8 of a camera mask (nullptr: no mask)
    static bool share_mask_uniform(const std::vector<int> &gptr, const std::vector<int> &members, const unsigned short *cm)
    {
        for (size_t g = 0; cm && g + 1 < gptr.size(); g++)
            for (int m = gptr[g] + 1; m < gptr[g + 1]; m++)
                if ((cm[members[m]] & BA_FIX_INTRINSICS) != (cm[members[gptr[g]]] & BA_FIX_INTRINSICS)) return false;
        return true;
    }
    int set_shared(const int *group_of) override
    {
        try {
            return set_shared_impl(group_of);
        } catch (const std::bad_alloc &) { // (the host lists; nothing of the solver has been touched yet)
            return BA_ERR_NOMEM;
        }
    }
    int set_shared_impl(const int *group_of)
    {
        if (!iterative()) return BA_ERR_ARG;
        Share ns;
        int rc;
        if (group_of) {
            std::vector<int> gptr((size_t)N / 2 + 2), members((size_t)N + 1), cptr((size_t)N + 2), cgrp((size_t)N + 1);
            if ((rc = ba_intrinsics_group_plan(N, group_of, BA_SHARE_CHUNK, &ns.ngroups, gptr.data(), members.data(), &ns.nchunks, cptr.data(), cgrp.data())))
                return rc;
            gptr.resize((size_t)ns.ngroups + 1);
            ns.ngrouped = gptr[ns.ngroups];
            members.resize((size_t)ns.ngrouped);
            if (ns.ngroups > 0) {
                // refusals: the members' f, k1, k2 in the resident state, their mask bits 6..8
                std::vector<T> hc;
                if ((rc = dl(d_cam[0].p, 15 * (size_t)N, hc))) return rc;
                if (!share_equal(gptr, members, hc.data(), N)) return BA_ERR_ARG;
                if (mk.on && mk.cmask.p) {
                    std::vector<unsigned short> hm((size_t)N);
                    HIPCHK(hipMemcpy(hm.data(), mk.cmask.p, sizeof(unsigned short) * (size_t)N, hipMemcpyDeviceToHost));
                    if (!share_mask_uniform(gptr, members, hm.data())) return BA_ERR_ARG;
                }
                ba_share_plan pl;
                ba_plan_share_slots(ns.ngroups, ns.nchunks, gptr.data(), cptr.data(), cgrp.data(), pl);
                ns.largest = pl.largest; ns.nslots = pl.nslots; ns.nwide = pl.nwide;
                static_assert(sizeof(ba_share_chunk) == 5 * sizeof(int), "ba_share_plan: 5 ints per slot");
                if ((rc = ns.desc.upload_ints(pl.desc)) || (rc = ns.members.upload(members)) || (rc = ns.wide.upload(pl.wide)) ||
                    (rc = ns.part.alloc((size_t)3 * ns.nslots))) { (void)hipGetLastError(); return rc; }
                HIPCHK(hipMemset(ns.part.p, 0, sizeof(double) * ns.part.n));
                ns.h_gptr.swap(gptr); ns.h_members.swap(members);
            }
        }
        HIPCHK(hipStreamSynchronize(st));
        sh = std::move(ns);
        drop_trial_graphs(); // (captured with the old launch sequence)
        vf.step_dropped(); // (xTest is the step of the other group set: its members' f, k1, k2 need not be equal)
        return BA_OK;
    }
    int shared_info(long long *out4) override
    {
        if (!iterative() || !out4) return BA_ERR_ARG;
        out4[0] = sh.ngroups; out4[1] = sh.ngrouped; out4[2] = sh.largest; out4[3] = sh.nchunks;
        return BA_OK;
    }

    // segment A behind k_elim_chol: block-Jacobi preconditioner, reduced rhs, g_c for the retraction's rho terms, x_0 = 0 and the
    // recurrence's start (p_{-1} = 0, z_0, slot-0 partials, |rhs|^2)
    // (Bm, rhs, gc_out: the trial's own buffers unless ba_solver_covariance_pcg hands in its scratch)
    void launch_pcg_blocks(T *Bm = nullptr, T *rhs = nullptr, T *gc_out = nullptr)
    {
        if (sx.ndchunks > 0)
            hipLaunchKernelGGL((k_pcg_prec_chunks<T>), dim3((sx.ndchunks + 7) / 8), dim3(256), 0, st, sx.ndchunks, d_dchunk_ptr.p, d_cam_obs.p, d_obs_pt.p,
                               d_rec.p, d_tvec.p, Ml, d_dslab.p);
        with_flag(marq(), [&](auto MARQ) {
            hipLaunchKernelGGL((k_pcg_prec_reduce<T, MARQ()>), dim3((unsigned)(((size_t)N * BA_SLAB + 255) / 256)), dim3(256), 0, st, N, d_cam_dchunk_ptr.p,
                               d_dslab.p, d_V.p, d_gc.p, d_scal.p + SC_LAMBDA, Bm ? Bm : d_pcg_M.p, rhs ? rhs : d_pcg_b.p, gc_out ? gc_out : d_gcg.p,
                               damp_args());
        });
    }
    void launch_pcg_prep()
    {
        launch_pcg_blocks();
        if (share_on()) launch_share<false>(d_pcg_b.p); // rhs <- Pi rhs: r_0, |rhs|^2 and z_0 see it (BA_GET_RHS returns it)
        const bool forest = forest_on(); // the factor reads B_a in front of its inversion in place; z_0 and r_0'z_0 of the trees behind it
        if (forest) {
            if (fo.width == 9) launch_forest_edges(); // (behind the elimination's and the constraints' records)
            launch_forest_factor();
        }
        with_flag(forest, [&](auto FOREST) {
            hipLaunchKernelGGL((k_pcg_prec_inv<T, FOREST()>), dim3(pcg_gc), dim3(256), 0, st, N, d_pcg_M.p, d_pcg_b.p, d_dxc.p, d_pcg_r.p, d_pcg_z.p, d_pcg_p.p,
                               pcg_part_rz(), pcg_part_rr(), FOREST() ? (const unsigned char *)fo.in_tree.p : nullptr);
        });
        if (forest) launch_forest_apply<true>(pcg_part_rz() + pcg_gc);
        if (share_on()) launch_share<false>(d_pcg_z.p); // z_0 <- Pi z_0 (r_0'z_0 of the unprojected z_0 is r_0'(Pi z_0): r_0 is in range(Pi))
        if (qstop_on()) hipLaunchKernelGGL(k_pcg_start_q, dim3(1), dim3(256), 0, st, pcg_part_rr(), pcg_gc, d_pcg.p, d_pcg_part_s.p);
        else
        hipLaunchKernelGGL(k_pcg_start, dim3(1), dim3(256), 0, st, pcg_part_rr(), pcg_gc, d_pcg.p);
    }
    // y = S v: the point pass, then the camera pass (chunk partials in d_dslab, then per camera)
    template <bool FINAL> void launch_pcg_matvec(int k, double tol2)
    {
        const T *lam = d_scal.p + SC_LAMBDA;
        if (Ml > 0)
            with_flag(!FINAL && qstop_on(), [&](auto QS) { // (the model rule sits behind the residual's, at the head of an iteration)
                if constexpr (decltype(QS)::value)
                    hipLaunchKernelGGL((k_pcg_point_q<T, 8>), dim3((unsigned)(((size_t)Ml * 8 + 255) / 256)), dim3(256), 0, st, k, Ml, d_pt_ptr.p, d_obs_cam.p,
                                       d_rec.p, d_dinv.p, d_pcg_z.p, d_pcg_p.p, pcg_part_rz(), pcg_part_rr(), pcg_gc, pcg_gz(), tol2, d_pcg.p, d_pcg_w.p,
                                       pcg_eta, (const double *)d_pcg_part_s.p);
                else
            hipLaunchKernelGGL((k_pcg_point<T, 8, FINAL>), dim3((unsigned)(((size_t)Ml * 8 + 255) / 256)), dim3(256), 0, st, k, Ml, d_pt_ptr.p, d_obs_cam.p,
                               d_rec.p, d_dinv.p, d_pcg_z.p, d_pcg_p.p, d_dxc.p, pcg_part_rz(), pcg_part_rr(), pcg_gc, pcg_gz(), tol2, d_pcg.p, d_pcg_w.p);
            });
        if (sx.ndchunks > 0)
            hipLaunchKernelGGL((k_pcg_cam_chunks<T, FINAL>), dim3((sx.ndchunks + 7) / 8), dim3(256), 0, st, sx.ndchunks, d_dchunk_ptr.p, d_cam_obs.p,
                               d_obs_pt.p, d_rec.p, Ml, d_pcg_w.p, d_dslab.p, d_pcg.p);
        with_flag(marq(), [&](auto MARQ) {
            hipLaunchKernelGGL((k_pcg_cam<T, FINAL, MARQ()>), dim3(pcg_gq), dim3(256), 0, st, k, N, d_cam_dchunk_ptr.p, d_dslab.p, d_V.p, lam, d_pcg_z.p, d_pcg_p.p,
                               d_dxc.p, d_pcg_b.p, pcg_part_rz(), pcg_gz(), d_pcg_y.p, FINAL ? pcg_part_res() : pcg_part_py(), d_pcg.p, damp_args());
        });
        if (relposes()) // (+ the constraints' cross blocks: y and the block partials, directly behind)
            hipLaunchKernelGGL((k_pcg_relpose<T, FINAL>), dim3(pcg_gq), dim3(256), 0, st, k, N, relpose_csr(), (const T *)d_pcg_z.p, (const T *)d_pcg_p.p,
                               (const T *)d_dxc.p, (const T *)d_pcg_b.p, (const double *)pcg_part_rz(), pcg_gz(), d_pcg_y.p,
                               FINAL ? pcg_part_res() : pcg_part_py(), (const ba_pcg_dev *)d_pcg.p);
        if (share_on()) { // y <- Pi y (p'y of the unprojected y is p'(Pi y)); FINAL: |Pi (rhs - S x)|^2 from the projected y
            launch_share<!FINAL>(d_pcg_y.p);
            if (FINAL)
                hipLaunchKernelGGL((k_pcg_share_res<T>), dim3(pcg_gq), dim3(256), 0, st, N, (const T *)d_pcg_b.p, (const T *)d_pcg_y.p, pcg_part_res());
        }
    }
    // segment B's solve: pcg_max_iter iterations of four launches (the ones behind convergence return at once), the product S x of the
    // step and the statistics.  The solution is d_dxc, where launch_backsub_retract reads it.
    void launch_pcg_solve()
    {
        const double tol2 = pcg_rel_tol * pcg_rel_tol;
        for (int k = 0; k < pcg_max_iter; k++) {
            launch_pcg_matvec<false>(k, tol2);
            with_flag(forest_on(), [&](auto FOREST) {
                if (qstop_on())
                    hipLaunchKernelGGL((k_pcg_update_q<T, FOREST()>), dim3(pcg_gc), dim3(256), 0, st, k, N, d_pcg_M.p, d_pcg_y.p, d_pcg_z.p, d_pcg_p.p,
                                       d_dxc.p, d_pcg_r.p, pcg_part_rz(), pcg_part_rr(), pcg_part_py(), pcg_gc, pcg_gz(), pcg_gq, d_pcg.p,
                                       FOREST() ? (const unsigned char *)fo.in_tree.p : nullptr, (const T *)d_pcg_b.p, d_pcg_part_s.p);
                else
                hipLaunchKernelGGL((k_pcg_update<T, FOREST()>), dim3(pcg_gc), dim3(256), 0, st, k, N, d_pcg_M.p, d_pcg_y.p, d_pcg_z.p, d_pcg_p.p, d_dxc.p,
                                   d_pcg_r.p, pcg_part_rz(), pcg_part_rr(), pcg_part_py(), pcg_gc, pcg_gz(), pcg_gq, d_pcg.p,
                                   FOREST() ? (const unsigned char *)fo.in_tree.p : nullptr);
            });
            if (forest_on()) launch_forest_apply<false>(pcg_part_rz() + (size_t)((k + 1) % 3) * pcg_gz() + pcg_gc);
            if (share_on()) launch_share<true>(d_pcg_z.p); // z_{k+1} <- Pi z_{k+1}, behind whatever produced it
        }
        launch_pcg_matvec<true>(pcg_max_iter, tol2);
        // (a trial ba_minimize enqueued behind the row that ended the run is not counted: lm->stop is already set when it runs)
        if (qstop_on())
            hipLaunchKernelGGL(k_pcg_finish_q, dim3(1), dim3(256), 0, st, pcg_max_iter, pcg_part_rr(), pcg_gc, pcg_part_res(), pcg_gq, tol2, d_pcg.p,
                               step_level ? (const int *)nullptr : (const int *)&d_lm.p->stop, (const double *)d_pcg_part_s.p);
        else
        hipLaunchKernelGGL(k_pcg_finish, dim3(1), dim3(256), 0, st, pcg_max_iter, pcg_part_rr(), pcg_gc, pcg_part_res(), pcg_gq, tol2, d_pcg.p,
                           step_level ? (const int *)nullptr : (const int *)&d_lm.p->stop);
    }
    int set_pcg(int max_iter, double rel_tol) override
    {
        if (!iterative() || max_iter < 1 || !(rel_tol > 0 && rel_tol < 1)) return BA_ERR_ARG;
        pcg_max_iter = max_iter; pcg_rel_tol = rel_tol;
        if (g_trial) { (void)hipGraphExecDestroy(g_trial); g_trial = nullptr; } // (captured with the old launch sequence)
        return BA_OK;
    }
    // the model-decrease rule of the solve: the *_q kernels while eta > 0, the kernels of a solver that never had
    // the rule at eta = 0.  The linearisation and a pending step do not depend on it.
    int set_pcg_model_tol(double eta) override
    {
        if (!iterative() || !(eta >= 0 && eta < 1)) return BA_ERR_ARG; // (a NaN fails both comparisons)
        if (eta > 0 && !d_pcg_part_s.p) {
            HIPCHK(hipStreamSynchronize(st));
            int rc;
            if ((rc = d_pcg_part_s.alloc((size_t)3 * pcg_gc))) { d_pcg_part_s.release(); return rc; }
            HIPCHK(hipMemset(d_pcg_part_s.p, 0, sizeof(double) * d_pcg_part_s.n));
        }
        if (eta != pcg_eta && g_trial) { (void)hipGraphExecDestroy(g_trial); g_trial = nullptr; } // (captured with the other kernels or eta)
        pcg_eta = eta;
        return BA_OK;
    }
    int pcg_stop_stats(ba_pcg_stop_stats *out, int reset) override
    {
        if (!iterative()) return BA_ERR_ARG;
        ba_pcg_dev h{};
        HIPCHK(hipStreamSynchronize(st));
        HIPCHK(hipMemcpy(&h, d_pcg.p, sizeof h, hipMemcpyDeviceToHost));
        if (out) {
            out->by_residual = h.by_residual; out->by_model = h.by_model; out->at_cap = h.at_cap;
            out->last_rule = h.last_rule; out->last_zeta = h.last_zeta; out->last_model = h.last_model;
        }
        if (reset) {
            h.by_residual = 0; h.by_model = 0; h.at_cap = 0; h.last_rule = 0; h.last_zeta = 0; h.last_model = 0;
            HIPCHK(hipMemcpy(d_pcg.p, &h, sizeof h, hipMemcpyHostToDevice));
        }
        return BA_OK;
    }
    // ---- Marquardt's damping (ba_solver_set_damping) ------------------------------------------------------------
    // lambda diag(J'J), clamped, instead of lambda I: the MARQ instantiations of the kernels that add lambda.  damp_off: inside the
    // covariance calls, whose lambda keeps the meaning (J'J + lambda I)^-1.
    int damp_kind = BA_DAMP_IDENTITY;
    double damp_min = BA_DAMP_DIAG_MIN_DEFAULT, damp_max = BA_DAMP_DIAG_MAX_DEFAULT;
    bool damp_off = false;
    bool marq() const { return damp_kind == BA_DAMP_MARQUARDT && !damp_off; }
    ba_damp_args<T> damp_args() const { return ba_damp_args<T>{(T)damp_min, (T)damp_max}; }
    ba_damp_diag<T> damp_diag() const { return ba_damp_diag<T>{(const T *)d_U0.p, (const T *)d_V.p, damp_args()}; }
    struct DampOff { // the identity instantiations for the length of a covariance call
        bool &f, was;
        explicit DampOff(bool &flag) : f(flag), was(flag) { f = true; }
        ~DampOff() { f = was; }
    };
    int set_damping(int k, double dmin, double dmax) override
    {
        if (k == BA_DAMP_IDENTITY) {
            if (damp_kind != k) drop_trial_graphs();
            damp_kind = k;
            return BA_OK;
        }
        if (k != BA_DAMP_MARQUARDT || !chol_elim() || sharded()) return BA_ERR_ARG;
        if (dmin == 0) dmin = BA_DAMP_DIAG_MIN_DEFAULT;
        if (dmax == 0) dmax = BA_DAMP_DIAG_MAX_DEFAULT;
        const T tmin_ = (T)dmin, tmax_ = (T)dmax; // (the kernels see them in the solver's scalar type)
        if (!positive_in_T(dmin) || !positive_in_T(dmax) || !(tmin_ <= tmax_)) return BA_ERR_ARG;
        drop_trial_graphs(); // (captured with the other instantiations or other bounds)
        damp_kind = k; damp_min = (double)tmin_; damp_max = (double)tmax_;
        return BA_OK;
    }
    int get_damping(int *k, double *dmin, double *dmax) override
    {
        if (k) *k = damp_kind;
        if (dmin) *dmin = damp_min;
        if (dmax) *dmax = damp_max;
        return BA_OK;
    }
    void drop_trial_graphs()
    {
        for (hipGraphExec_t *g : {&g_trial, &g_trial_nh, &g_a, &g_b, &g_ctl})
            if (*g) { (void)hipGraphExecDestroy(*g); *g = nullptr; }
    }
    int pcg_stats(ba_pcg_stats *out, int reset) override
    {
        if (!iterative()) return BA_ERR_ARG;
        ba_pcg_dev h{};
        HIPCHK(hipStreamSynchronize(st));
        HIPCHK(hipMemcpy(&h, d_pcg.p, sizeof h, hipMemcpyDeviceToHost));
        if (out) {
            out->solves = h.solves; out->total_iters = h.total_iters; out->last_iters = h.last_iters;
            out->last_converged = h.last_converged; out->last_rel_residual = h.last_rel_residual;
        }
        if (reset) {
            h.solves = 0; h.total_iters = 0; h.last_iters = 0; h.last_converged = 0; h.last_rel_residual = 0;
            HIPCHK(hipMemcpy(d_pcg.p, &h, sizeof h, hipMemcpyHostToDevice));
        }
        return BA_OK;
    }
    size_t device_bytes() const override
    {
        size_t n = 0;
        for (const auto *b : {&d_obs_cam, &d_obs_pt, &d_pt_ptr, &d_pair_hi, &d_pair_lo, &d_pair_chunk_ptr, &d_dchunk_ptr, &d_cam_dchunk_ptr, &d_cam_obs,
                              &d_qr_pts, &d_flags, &d_ldlt_jobs, &d_pperm, &d_wave_ptr, &d_red_pairs, &d_eb, &d_own_off})
            n += bytes_of(*b);
        for (const auto *b : {&d_r, &d_Jc, &d_Jp, &d_JcA, &d_U0, &d_gp, &d_V, &d_gc, &d_rec0, &d_dinv0, &d_tvec0, &d_tri0, &d_cam[0], &d_cam[1],
                              &d_pts[0], &d_pts[1], &d_meas, &d_gcg, &d_dslab, &d_rec, &d_dinv, &d_tvec, &d_tri, &d_slab, &d_S, &d_pack, &d_Skeep,
                              &d_Wp, &d_Winv, &d_dxc, &d_dxp, &d_part_e, &d_part_pm, &d_part_bs, &d_part_st, &d_scal, &d_qA, &d_qtau, &d_q1obs,
                              &d_q1lam, &d_mQl, &d_mQR, &d_R22, &d_qB, &d_qAcopy, &d_dbgr, &d_dbg2, &d_stage, &d_pcg_M, &d_pcg_b, &d_pcg_r,
                              &d_pcg_z, &d_pcg_p, &d_pcg_y, &d_pcg_w})
            n += bytes_of(*b);
        n += bytes_of(d_chunk_info) + bytes_of(d_ent) + bytes_of(d_lm) + bytes_of(d_pcg_part) + bytes_of(d_pcg_part_s) + bytes_of(d_pcg) + mc_bytes();
        return n + mk.bytes() + md.bytes() + pr.bytes() + rp.bytes() + dg.bytes() + tr.bytes() + ac.bytes() + fl.bytes() + cv.bytes() + fo.bytes() + sh.bytes();
    }

    // ---- covariance blocks (ba_solver_covariance_compute / _get; ba_cov.hip.h) -----------------------------------
    // The work buffer cv.buf is the solver's only state of this feature: [C: cov_ld x (Dp + 64) | one panel Y: cov_ld x NB | the blocks'
    // inverses W | the pivots (Dp) | the scaling (Dp) | the last trial's dx_c while the assembly borrows its buffer], allocated by the first compute.  The LM trial's own S, Wp, Winv and flags are not
    // used by the factorisation here (S is assembled as a trial assembles it and then only read), x, xTest, J and the mask not at all.
    int cov_ld() const { return ((Dp + D + NAUG + NB - 1) / NB) * NB + 64; }
    size_t cov_nmat() const { return (size_t)cov_ld() * (Dp + 64); }
    T *cov_wp() const { return cv.buf.p + cov_nmat(); }
    T *cov_winv() const { return cov_wp() + (size_t)cov_ld() * NB; }
    T *cov_dv() const { return cov_winv() + (size_t)((D + NB - 1) / NB) * NB * NB; }
    T *cov_sc() const { return cov_dv() + Dp; }
    T *cov_dxsave() const { return cov_sc() + Dp; }
    size_t cov_count() const { return cov_nmat() + (size_t)cov_ld() * NB + (size_t)((D + NB - 1) / NB) * NB * NB + 2 * (size_t)Dp + d_dxc.n; }

    // What both covariance routes start from, at the lambda in SC_LAMBDA: the elimination, a fixed point's records cleared (its
    // U_p = lambda I is never inverted: its records are the zeros they stand for), every free point's block checked into *flag
    void launch_cov_eliminate(int *flag)
    {
        launch_eliminate();
        if (mk.on && mk.pfix.p)
            hipLaunchKernelGGL((k_cov_fixed_records<T>), dim3((std::max(Kl, Ml) + 255) / 256), dim3(256), 0, st, Kl, Ml, (int)BA_REC, (const int *)d_obs_pt.p,
                               (const unsigned char *)mk.pfix.p, d_rec.p, d_dinv.p, d_tvec.p, d_tri.p);
        if (Ml <= 0) return;
        if (priors()) // (a point prior is in U0 and in no observation's Jp)
            hipLaunchKernelGGL((k_cov_points_check_u0<T>), dim3(gM), dim3(256), 0, st, Ml, (const T *)d_U0.p, (const unsigned char *)mk.pfix.p,
                               (const T *)(d_scal.p + SC_LAMBDA), flag);
        else
            hipLaunchKernelGGL((k_cov_points_check<T>), dim3(gM), dim3(256), 0, st, Ml, Kl, (const int *)d_pt_ptr.p, (const T *)d_Jp.p,
                               (const unsigned char *)mk.pfix.p, (const T *)(d_scal.p + SC_LAMBDA), flag);
    }
    // a request for blocks: counts, null pointers, index ranges (single shard: the shard's points are the problem's)
    bool cov_request_ok(int n_pairs, const int *cam_pairs, const double *cam_cov, int n_pts, const int *pt_ids, const double *pt_cov) const
    {
        if (n_pairs < 0 || n_pts < 0 || (n_pairs > 0 && (!cam_pairs || !cam_cov)) || (n_pts > 0 && (!pt_ids || !pt_cov))) return false;
        for (int q = 0; q < 2 * n_pairs; q++)
            if (cam_pairs[q] < 0 || cam_pairs[q] >= N) return false;
        for (int q = 0; q < n_pts; q++)
            if (pt_ids[q] < 0 || pt_ids[q] >= Ml) return false;
        return true;
    }

    int cov_compute(double lambda) override
    {
        if constexpr (!std::is_same<T, double>::value) return BA_ERR_ARG; // (a single-precision inverse at these condition numbers is noise)
        else {
            // refusals: host side, before any launch
            if ((kind != BA_CHOLESKY && kind != BA_QRCHOL) || sharded() || !vf.have_lin || vf.mask_pending || !(lambda >= 0) || !std::isfinite(lambda))
                return BA_ERR_ARG;
            const DampOff identity(damp_off); // (this call's lambda means J'J + lambda I whatever ba_solver_set_damping holds)
            vf.cov_dropped();
            int rc;
            if (!cv.buf.p) {
                Cov nc;
                if ((rc = nc.buf.alloc(cov_count())) || (rc = nc.flag.alloc(1))) { (void)hipGetLastError(); return rc; } // (the solver stays usable)
                cv = std::move(nc);
            }
            const int ldc = cov_ld();
            int flag = 0;
            HIPCHK(hipMemsetAsync(cv.flag.p, 0, sizeof(int), st));
            if ((rc = set_lambda((T)lambda))) return rc;
            HIPCHK(hipEventRecord(ev[EV_T0], st));
            // S(lambda) as a trial assembles it (segment A + the diagonal's lambda), left unfactored in d_S.  The assembly arms the back
            // sweep's hand-over vector, which is where the last trial's dx_c lives (BA_GET_DX): kept aside and put back.
            HIPCHK(hipMemcpyAsync(cov_dxsave(), d_dxc.p, sizeof(T) * d_dxc.n, hipMemcpyDeviceToDevice, st));
            launch_cov_eliminate(cv.flag.p);
            launch_schur();
            launch_post_reduce();
            HIPCHK(hipMemcpyAsync(d_dxc.p, cov_dxsave(), sizeof(T) * d_dxc.n, hipMemcpyDeviceToDevice, st));
            HIPCHK(hipMemsetAsync(cv.buf.p, 0, sizeof(T) * cov_nmat(), st));
            hipLaunchKernelGGL((k_cov_scale<T>), dim3((D + 255) / 256), dim3(256), 0, st, D, ld, (const T *)d_S.p, (const unsigned short *)mk.cmask.p,
                               cov_sc(), cv.flag.p);
            hipLaunchKernelGGL((k_cov_stage<T>), dim3(((D + NB - 1) / NB) * NB), dim3(256), 0, st, D, Dp, ld, (const T *)d_S.p, (const T *)cov_sc(), ldc, cv.buf.p);
            HIPCHK(hipEventRecord(ev[EV_T1], st));
            HIPCHK(hipMemcpyAsync(&flag, cv.flag.p, sizeof(int), hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));
            if (flag) return BA_ERR_SINGULAR; // a free parameter nobody observes: nothing is factored
            // launch-per-step factorisation (no workgroup waits for another one) with the stacked rows riding along
            ba_ldlt_factor<T, NB>(st, Dp + D, ((D + NB - 1) / NB) * NB /* the last block column padded with unit pivots */, ldc, cv.buf.p, cov_wp(), cov_winv(), (int *)nullptr, 0, (T *)nullptr, /*safe*/ true, 0);
            HIPCHK(hipEventRecord(ev[EV_T2], st));
            hipLaunchKernelGGL((k_cov_diag<T>), dim3((Dp + 255) / 256), dim3(256), 0, st, D, Dp, ldc, (const T *)cv.buf.p, (const T *)cov_sc(), cov_dv(), cv.flag.p);
            const int nt = (D + 63) / 64;
            hipLaunchKernelGGL((k_cov_syrk<T>), dim3(nt * (nt + 1) / 2), dim3(256), 0, st, D, Dp, ldc, cv.buf.p, (const T *)cov_dv());
            HIPCHK(hipEventRecord(ev[EV_T3], st));
            HIPCHK(hipMemcpyAsync(&flag, cv.flag.p, sizeof(int), hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));
            HIPCHK(hipGetLastError());
            cv.ms[0] = ev_ms(EV_T0, EV_T1); cv.ms[1] = ev_ms(EV_T1, EV_T2); cv.ms[2] = ev_ms(EV_T2, EV_T3);
            if (flag) return BA_ERR_SINGULAR; // a pivot <= 0 (or not finite): no result is left behind
            cv.lambda = lambda;
            vf.cov_computed();
            return BA_OK;
        }
    }

    int cov_get(int n_pairs, const int *cam_pairs, double *cam_cov, int n_pts, const int *pt_ids, double *pt_cov) override
    {
        if constexpr (!std::is_same<T, double>::value) return BA_ERR_ARG;
        else {
            if (!vf.cov_valid || !cov_request_ok(n_pairs, cam_pairs, cam_cov, n_pts, pt_ids, pt_cov)) return BA_ERR_ARG;
            const int ldc = cov_ld();
            int rc;
            HIPCHK(hipStreamSynchronize(st));
            if (n_pairs > 0) {
                DevBuf<int> d_idx;
                DevBuf<double> d_out;
                if ((rc = d_idx.alloc((size_t)2 * n_pairs)) || (rc = d_out.alloc((size_t)81 * n_pairs))) { (void)hipGetLastError(); return rc; }
                HIPCHK(hipMemcpy(d_idx.p, cam_pairs, sizeof(int) * 2 * (size_t)n_pairs, hipMemcpyHostToDevice));
                hipLaunchKernelGGL((k_cov_get_cams<T>), dim3((unsigned)(((size_t)81 * n_pairs + 255) / 256)), dim3(256), 0, st, n_pairs, (const int *)d_idx.p, ldc,
                                   (const T *)cv.buf.p, (const unsigned short *)mk.cmask.p, d_out.p);
                HIPCHK(hipStreamSynchronize(st));
                HIPCHK(hipMemcpy(cam_cov, d_out.p, sizeof(double) * 81 * (size_t)n_pairs, hipMemcpyDeviceToHost));
            }
            if (n_pts > 0) {
                DevBuf<int> d_idx;
                DevBuf<double> d_out;
                if ((rc = d_idx.alloc((size_t)n_pts)) || (rc = d_out.alloc((size_t)9 * n_pts))) { (void)hipGetLastError(); return rc; }
                HIPCHK(hipMemcpy(d_idx.p, pt_ids, sizeof(int) * (size_t)n_pts, hipMemcpyHostToDevice));
                // J of the linearisation, not the elimination's records: those are a later trial's by now
                HIPCHK(hipEventRecord(ev[EV_T4], st));
                if (priors()) // (CHOLESKY: the only kind with both)
                    hipLaunchKernelGGL((k_cov_points_u0<T, true>), dim3(n_pts), dim3(64), 0, st, n_pts, (const int *)d_idx.p, Kl, (const int *)d_pt_ptr.p,
                                       (const int *)d_obs_cam.p, (const T *)d_JcA.p, (const T *)d_Jp.p, (const unsigned char *)mk.pfix.p, (T)cv.lambda, ldc,
                                       (const T *)cv.buf.p, d_out.p, (const T *)d_U0.p, Ml);
                else if (chol_elim())
                    hipLaunchKernelGGL((k_cov_points<T, true>), dim3(n_pts), dim3(64), 0, st, n_pts, (const int *)d_idx.p, Kl, (const int *)d_pt_ptr.p,
                                       (const int *)d_obs_cam.p, (const T *)d_JcA.p, (const T *)d_Jp.p, (const unsigned char *)mk.pfix.p, (T)cv.lambda, ldc,
                                       (const T *)cv.buf.p, d_out.p);
                else
                    hipLaunchKernelGGL((k_cov_points<T, false>), dim3(n_pts), dim3(64), 0, st, n_pts, (const int *)d_idx.p, Kl, (const int *)d_pt_ptr.p,
                                       (const int *)d_obs_cam.p, (const T *)d_Jc.p, (const T *)d_Jp.p, (const unsigned char *)mk.pfix.p, (T)cv.lambda, ldc,
                                       (const T *)cv.buf.p, d_out.p);
                HIPCHK(hipEventRecord(ev[EV_T5], st));
                HIPCHK(hipStreamSynchronize(st));
                cv.ms[3] = ev_ms(EV_T4, EV_T5);
                HIPCHK(hipMemcpy(pt_cov, d_out.p, sizeof(double) * 9 * (size_t)n_pts, hipMemcpyDeviceToHost));
            }
            HIPCHK(hipGetLastError());
            return BA_OK;
        }
    }
    // ms of the last compute: assembly (elimination, S, staging) | factorisation | inverse (pivots + rank-D update); of the last get
    // with points: the point kernel
    int cov_timing(double *ms4) override
    {
        for (int q = 0; q < 4; q++) ms4[q] = cv.ms[q];
        return BA_OK;
    }

    // ---- covariance blocks by multi-column PCG (ba_solver_covariance_pcg; ba_pcg_multi.hip.h) ---------------------
    // Work vectors of its own, allocated by the first call: x, r, z, p, y and the right-hand sides B ([9 N][9] each), the point pass
    // ([3 Ml][9]), the chunk slab ([ndchunks][9][9]), B_a^-1 ([N][81]), three lists of workgroup partials ([gm][9]) and the state.  The
    // trial's own vectors (d_dxc, d_pcg_*) are not touched; what the call spends are the elimination's records and d_dslab.
    // (double only: the members below are instantiated for the fp64 solver alone, from cov_pcg's fp64 branch)
    DevBuf<double> d_mc_vec, d_mc_w, d_mc_slab, d_mc_M, d_mc_part;
    DevBuf<ba_mc_dev> d_mc;
    int mc_gm() const { return (N + BA_MC_CPB - 1) / BA_MC_CPB; }
    size_t mc_bytes() const { return bytes_of(d_mc_vec) + bytes_of(d_mc_w) + bytes_of(d_mc_slab) + bytes_of(d_mc_M) + bytes_of(d_mc_part) + bytes_of(d_mc); }
    void mc_release() { d_mc_vec.release(); d_mc_w.release(); d_mc_slab.release(); d_mc_M.release(); d_mc_part.release(); d_mc.release(); }
    // one call: where its vectors are, its stopping rule, the mask in force, the statistics so far
    struct McRun {
        double *x, *r, *z, *p, *y, *b, *part_rz, *part_rr, *part_py;
        int gm, max_iter;
        double tol2;
        const unsigned short *cmask;
        const unsigned char *pfix;
        ba_cov_pcg_stats acc;
    };
    int mc_begin(int max_iter, double rel_tol, McRun &c)
    {
        int rc;
        const size_t DV = (size_t)D * BA_MC_NR;
        const int gm = mc_gm();
        if (!d_mc.p) {
            if ((rc = d_mc_vec.alloc(6 * DV)) || (rc = d_mc_w.alloc((size_t)27 * (Ml > 0 ? Ml : 1))) ||
                (rc = d_mc_slab.alloc((size_t)81 * (sx.ndchunks > 0 ? sx.ndchunks : 1))) || (rc = d_mc_M.alloc((size_t)81 * N)) ||
                (rc = d_mc_part.alloc((size_t)3 * gm * BA_MC_NR)) || (rc = d_mc.alloc(1))) {
                (void)hipGetLastError(); // (the solver stays usable)
                mc_release();
                return rc;
            }
        }
        double *v = d_mc_vec.p, *pt = d_mc_part.p;
        c = McRun{v, v + DV, v + 2 * DV, v + 3 * DV, v + 4 * DV, v + 5 * DV, pt, pt + (size_t)gm * BA_MC_NR, pt + 2 * (size_t)gm * BA_MC_NR, gm, max_iter,
                  rel_tol * rel_tol, mk.on ? (const unsigned short *)mk.cmask.p : nullptr, mk.on ? (const unsigned char *)mk.pfix.p : nullptr,
                  ba_cov_pcg_stats{}};
        return BA_OK;
    }
    // Once per call: the elimination at lambda and the block-Jacobi blocks B_a as a trial forms them (launch_pcg_blocks into this call's
    // buffers: the reduced rhs of the last trial, BA_GET_RHS, stays where it is), every free point's block and every B_a positive definite
    int mc_prepare(double lambda, const McRun &c)
    {
        int rc;
        ba_mc_dev *ms = d_mc.p;
        HIPCHK(hipMemsetAsync(&ms->flag, 0, sizeof(int), st));
        if ((rc = set_lambda((T)lambda))) return rc;
        HIPCHK(hipEventRecord(ev[EV_T0], st));
        launch_cov_eliminate(&ms->flag);
        launch_pcg_blocks((T *)d_mc_M.p, (T *)c.y, (T *)c.z);
        hipLaunchKernelGGL(k_mc_prec_inv, dim3((N + 255) / 256), dim3(256), 0, st, N, d_mc_M.p, c.cmask, &ms->flag);
        ba_mc_dev h{};
        HIPCHK(hipMemcpyAsync(&h, ms, sizeof h, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        HIPCHK(hipGetLastError());
        return h.flag ? BA_ERR_SINGULAR : BA_OK;
    }
    // y = S v for the nine columns (FINAL: v = x) and the one-workgroup launch behind it (alpha; FINAL: |b - S x|^2)
    template <bool FINAL> void mc_matvec(const McRun &c)
    {
        const ba_mc_dev *ms = d_mc.p;
        const double *lam = (const double *)(d_scal.p + SC_LAMBDA);
        if (Ml > 0)
            hipLaunchKernelGGL((k_mc_point<FINAL>), dim3((unsigned)(((size_t)Ml * 8 + 255) / 256)), dim3(256), 0, st, Ml, (const int *)d_pt_ptr.p,
                               (const int *)d_obs_cam.p, (const double *)d_rec.p, (const double *)d_dinv.p, (const double *)c.z, (const double *)c.p,
                               (const double *)c.x, ms, d_mc_w.p);
        if (sx.ndchunks > 0)
            hipLaunchKernelGGL((k_mc_cam_chunks<FINAL>), dim3((sx.ndchunks + 7) / 8), dim3(256), 0, st, sx.ndchunks, (const int *)d_dchunk_ptr.p,
                               (const int *)d_cam_obs.p, (const int *)d_obs_pt.p, (const double *)d_rec.p, (const double *)d_mc_w.p, d_mc_slab.p, ms);
        with_flag(relposes(), [&](auto RP) {
            hipLaunchKernelGGL((k_mc_cam<FINAL, RP()>), dim3(c.gm), dim3(256), 0, st, N, (const int *)d_cam_dchunk_ptr.p, (const double *)d_mc_slab.p,
                               (const double *)d_V.p, lam, (const double *)c.z, (const double *)c.p, (const double *)c.x, (const double *)c.b,
                               RP() ? relpose_csr() : ba_relpose_csr<double>{nullptr, nullptr, nullptr, nullptr}, c.cmask, c.y, c.part_py, ms);
        });
        hipLaunchKernelGGL((k_mc_alpha<FINAL>), dim3(1), dim3(256), 0, st, c.gm, (const double *)c.part_py, d_mc.p);
    }
    // One batch, its right-hand sides in c.b (`live` of them not zero): rounds of iterations with the state read back between them,
    // then the product S X; the solution stays in c.x, the batch joins the statistics
    int mc_solve_batch(McRun &c, int live)
    {
        ba_mc_dev *ms = d_mc.p;
        ba_mc_dev h{};
        hipLaunchKernelGGL(k_mc_init, dim3(c.gm), dim3(256), 0, st, N, (const double *)d_mc_M.p, (const double *)c.b, c.x, c.r, c.z, c.p, c.part_rz, c.part_rr);
        hipLaunchKernelGGL((k_mc_scal<true>), dim3(1), dim3(256), 0, st, 0, c.gm, (const double *)c.part_rz, (const double *)c.part_rr, c.tol2, ms);
        constexpr int ROUND = 16;
        for (int k = 0; k < c.max_iter;) {
            for (int e = std::min(c.max_iter, k + ROUND); k < e; k++) {
                mc_matvec<false>(c);
                hipLaunchKernelGGL(k_mc_update, dim3(c.gm), dim3(256), 0, st, N, (const double *)d_mc_M.p, (const double *)c.y, c.z, c.p, c.x, c.r, c.part_rz,
                                   c.part_rr, (const ba_mc_dev *)ms);
                hipLaunchKernelGGL((k_mc_scal<false>), dim3(1), dim3(256), 0, st, k, c.gm, (const double *)c.part_rz, (const double *)c.part_rr, c.tol2, ms);
            }
            HIPCHK(hipMemcpyAsync(&h, ms, sizeof h, hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));
            if (h.alldone) break;
        }
        if (h.singular) return BA_ERR_SINGULAR;
        mc_matvec<true>(c);
        HIPCHK(hipMemcpyAsync(&h, ms, sizeof h, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        HIPCHK(hipGetLastError());
        int bmax = 0;
        for (int q = 0; q < BA_MC_NR; q++) {
            if (!(h.bb[q] > 0)) continue;
            bmax = std::max(bmax, h.iters[q]);
            if (!h.done[q]) c.acc.unconverged++;
            c.acc.worst_rel_residual = std::max(c.acc.worst_rel_residual, std::sqrt(h.res[q] / h.bb[q]));
        }
        c.acc.columns += live; c.acc.batches++; c.acc.total_iters += bmax;
        c.acc.max_iters = std::max(c.acc.max_iters, bmax);
        return BA_OK;
    }
    // Up to three points (ids, output slots): with_solve = their Y_p as one batch and the solve; then Sigma_pp out of c.x (a point nobody
    // observes: I / lambda, no solve)
    int mc_point_batch(McRun &c, const std::vector<int> &ids, const std::vector<int> &slots, bool with_solve, int *rq_pts, double *out_p)
    {
        const int np = (int)ids.size();
        if (np == 0) return BA_OK;
        int hreq[6] = {0, 0, 0, 0, 0, 0}, rc;
        for (int i = 0; i < np; i++) { hreq[i] = ids[i]; hreq[3 + i] = slots[i]; }
        HIPCHK(hipStreamSynchronize(st));
        HIPCHK(hipMemcpy(rq_pts, hreq, sizeof hreq, hipMemcpyHostToDevice));
        if (with_solve) {
            HIPCHK(hipMemsetAsync(c.b, 0, sizeof(double) * (size_t)D * BA_MC_NR, st));
            hipLaunchKernelGGL(k_mc_rhs_pts, dim3(1), dim3(64), 0, st, np, (const int *)rq_pts, Ml, (const int *)d_pt_ptr.p, (const int *)d_obs_cam.p,
                               (const double *)d_rec.p, (const double *)d_dinv.p, (const double *)d_tri.p, c.pfix, c.b);
            if ((rc = mc_solve_batch(c, 3 * np))) return rc;
        }
        hipLaunchKernelGGL(k_mc_get_pts, dim3(1), dim3(64), 0, st, np, (const int *)rq_pts, (const int *)(rq_pts + 3), Ml, (const int *)d_pt_ptr.p,
                           (const int *)d_obs_cam.p, (const double *)d_rec.p, (const double *)d_dinv.p, (const double *)d_tri.p, c.pfix,
                           (const double *)(d_scal.p + SC_LAMBDA), (const double *)c.x, out_p);
        return BA_OK;
    }

    int cov_pcg(double lambda, int max_iter, double rel_tol, int n_pairs, const int *cam_pairs, double *cam_cov, int n_pts, const int *pt_ids,
                double *pt_cov, ba_cov_pcg_stats *stats) override
    {
        if constexpr (!std::is_same<T, double>::value) return BA_ERR_ARG;
        else {
            // refusals: host side, before any launch
            if (!iterative() || sharded() || share_on() || !vf.have_lin || vf.mask_pending || !(lambda >= 0) || !std::isfinite(lambda) || max_iter < 0 ||
                !(rel_tol >= 0 && rel_tol < 1) || !cov_request_ok(n_pairs, cam_pairs, cam_cov, n_pts, pt_ids, pt_cov))
                return BA_ERR_ARG;
            const DampOff identity(damp_off); // (this call's lambda means J'J + lambda I whatever ba_solver_set_damping holds)
            int rc;
            McRun c;
            if ((rc = mc_begin(max_iter ? max_iter : pcg_max_iter, rel_tol != 0 ? rel_tol : pcg_rel_tol, c))) return rc;
            // the mask on the host: which columns are live, which requests need no launch
            std::vector<unsigned short> hcm((size_t)N, 0);
            std::vector<unsigned char> hpf((size_t)(Ml > 0 ? Ml : 1), 0);
            HIPCHK(hipStreamSynchronize(st));
            if (mk.on && mk.cmask.p) HIPCHK(hipMemcpy(hcm.data(), mk.cmask.p, sizeof(unsigned short) * (size_t)N, hipMemcpyDeviceToHost));
            if (mk.on && mk.pfix.p && Ml > 0) HIPCHK(hipMemcpy(hpf.data(), mk.pfix.p, (size_t)Ml, hipMemcpyDeviceToHost));
            DevBuf<int> d_req; // pairs [2 n_pairs] | order [n_pairs] | point batch: ids [3], slots [3]
            DevBuf<double> d_out;
            if ((rc = d_req.alloc((size_t)3 * n_pairs + 6)) || (rc = d_out.alloc((size_t)81 * n_pairs + (size_t)9 * n_pts + 1))) { (void)hipGetLastError(); return rc; }
            int *rq_pairs = d_req.p, *rq_order = rq_pairs + 2 * (size_t)n_pairs, *rq_pts = rq_order + n_pairs;
            double *out_c = d_out.p, *out_p = out_c + (size_t)81 * n_pairs;
            // camera pairs by column block max(a, b), a block's pairs in request order
            std::vector<int> order((size_t)n_pairs);
            std::iota(order.begin(), order.end(), 0);
            auto blk = [&](int q) { return std::max(cam_pairs[2 * q], cam_pairs[2 * q + 1]); };
            std::stable_sort(order.begin(), order.end(), [&](int u, int v) { return blk(u) < blk(v); });
            if (n_pairs > 0) {
                HIPCHK(hipMemcpy(rq_pairs, cam_pairs, sizeof(int) * 2 * (size_t)n_pairs, hipMemcpyHostToDevice));
                HIPCHK(hipMemcpy(rq_order, order.data(), sizeof(int) * (size_t)n_pairs, hipMemcpyHostToDevice));
            }
            HIPCHK(hipMemsetAsync(d_out.p, 0, sizeof(double) * d_out.n, st)); // (a fully fixed camera or a fixed point: zeros, no launch)
            if ((rc = mc_prepare(lambda, c))) return rc;
            // camera column blocks
            for (int lo = 0; lo < n_pairs;) {
                int hi = lo;
                const int b = blk(order[lo]);
                while (hi < n_pairs && blk(order[hi]) == b) hi++;
                int live = 0;
                for (int q = 0; q < 9; q++) live += !((hcm[b] >> q) & 1);
                if (live > 0) {
                    HIPCHK(hipMemsetAsync(c.b, 0, sizeof(double) * (size_t)D * BA_MC_NR, st));
                    hipLaunchKernelGGL(k_mc_rhs_cam, dim3(1), dim3(64), 0, st, b, c.cmask, c.b);
                    if ((rc = mc_solve_batch(c, live))) return rc;
                    hipLaunchKernelGGL(k_mc_get_cams, dim3((unsigned)(((size_t)(hi - lo) * 81 + 255) / 256)), dim3(256), 0, st, hi - lo, (const int *)(rq_order + lo),
                                       (const int *)rq_pairs, b, (const double *)c.x, c.cmask, out_c);
                }
                lo = hi;
            }
            // points, three to a batch: first the ones that need a solve (free, observed), in request order; then the ones nobody
            // observes (I / lambda; lambda = 0 never gets here: the point check has refused).  A fixed point's zeros are in place.
            for (int pass = 0; pass < 2; pass++) {
                std::vector<int> ids, slots;
                for (int q = 0; q < n_pts; q++) {
                    const int j = pt_ids[q];
                    if (hpf[j] || (sx.pt_ptr[j] == sx.pt_ptr[j + 1]) != (pass == 1)) continue;
                    ids.push_back(j); slots.push_back(q);
                    if (ids.size() == 3) {
                        if ((rc = mc_point_batch(c, ids, slots, pass == 0, rq_pts, out_p))) return rc;
                        ids.clear(); slots.clear();
                    }
                }
                if ((rc = mc_point_batch(c, ids, slots, pass == 0, rq_pts, out_p))) return rc;
            }
            HIPCHK(hipEventRecord(ev[EV_T1], st));
            HIPCHK(hipStreamSynchronize(st));
            HIPCHK(hipGetLastError());
            if (n_pairs > 0) HIPCHK(hipMemcpy(cam_cov, out_c, sizeof(double) * 81 * (size_t)n_pairs, hipMemcpyDeviceToHost));
            if (n_pts > 0) HIPCHK(hipMemcpy(pt_cov, out_p, sizeof(double) * 9 * (size_t)n_pts, hipMemcpyDeviceToHost));
            c.acc.ms = ev_ms(EV_T0, EV_T1);
            if (stats) *stats = c.acc;
            return BA_OK;
        }
    }

    int set_lambda(T lambda)
    {
        *h_lam = lambda;
        HIPCHK(hipMemcpyAsync(d_scal.p + SC_LAMBDA, h_lam, sizeof(T), hipMemcpyHostToDevice, st));
        // a lambda from the host: whatever records a fused linearisation left behind were for another one
        HIPCHK(hipMemsetAsync(&d_lm.p->rec_fresh, 0, sizeof(int), st));
        return BA_OK;
    }

    void launch_backsub_retract()
    {
        if (Ml > 0) { // the camera retraction rides as one more block at the end of the grid
            const ba_cam_retract_args cr{N, d_cam[0].p, d_dxc.p, d_gcg.p, d_cam[1].p, d_scal.p, (int)SC_RHO_C};
            // masked: the first reader of dx_c behind every kind's reduced solve forces the fixed rows (and fixed points) to a zero step
            with_flags(mk.on, marq(), [&](auto MASKED, auto MARQ) {
                hipLaunchKernelGGL((k_backsub<T, 8, MASKED(), MARQ()>), dim3(gB + 1), dim3(256), 0, st, Ml, d_pt_ptr.p, d_obs_cam.p, d_rec.p, d_dinv.p,
                                   d_tvec.p, d_tri.p, d_dxc.p, d_gp.p, d_pts[0].p, d_scal.p + SC_LAMBDA, d_dxp.p, d_pts[1].p, d_part_bs.p, d_pperm.p, gB, cr,
                                   ba_fix_args{mk.cmask.p, mk.pfix.p}, damp_diag());
            });
        } else // (an empty shard keeps the zero partial sums written at creation)
            with_flags(mk.on, marq(), [&](auto MASKED, auto MARQ) {
                hipLaunchKernelGGL((k_retract_cams<T, MASKED(), MARQ()>), dim3(1), dim3(256), 0, st, N, d_cam[0].p, d_dxc.p, d_gcg.p, d_scal.p + SC_LAMBDA,
                                   d_cam[1].p, d_scal.p, (int)SC_RHO_C, (const unsigned short *)mk.cmask.p, damp_diag());
            });
    }

    // ---- parameters held constant (ba_solver_set_constant) ---------------------------------------------------------------------------
    // A mask with a bit set selects the masked instantiations of k_eval, k_backsub and k_retract_cams; nothing else changes (S, the
    // records, J2bot and the reduced solves see zero columns).  No mask: no buffers, the kernels of a solver that never had one.
    int set_constant(const unsigned short *cm, const unsigned char *pf) override
    {
        bool any = false, all = sx.M > 0 || N > 0;
        for (int a = 0; cm && a < N; a++) {
            const unsigned m = cm[a];
            if (m & ~(unsigned)BA_FIX_CAMERA) return BA_ERR_ARG;                          // bits above 8
            if ((m & BA_FIX_OMEGA) != 0 && (m & BA_FIX_OMEGA) != BA_FIX_OMEGA) return BA_ERR_ARG; // omega partly fixed
            any = any || m != 0;
            all = all && m == BA_FIX_CAMERA;
        }
        if (!cm) all = all && N == 0;
        for (int j = 0; pf && j < sx.M; j++) {
            any = any || pf[j] != 0;
            all = all && pf[j] != 0;
        }
        if (!pf) all = all && sx.M == 0;
        if (any && all) return BA_ERR_ARG; // nothing left to optimise
        if (share_on() && !share_mask_uniform(sh.h_gptr, sh.h_members, cm)) return BA_ERR_ARG; // (a shared parameter is fixed for all or for none)
        HIPCHK(hipStreamSynchronize(st));
        vf.cov_dropped(); // (in front of everything that can fail, as ever: ba_solver_covariance_get reads the mask)
        Mask nm;
        if (any) {
            int rc;
            std::vector<unsigned short> hc((size_t)N, 0);
            std::vector<unsigned char> hp((size_t)(Ml > 0 ? Ml : 1), 0);
            for (int a = 0; cm && a < N; a++) hc[a] = cm[a];
            for (int j = 0; pf && j < Ml; j++) hp[j] = pf[sx.p0 + j] != 0;
            if ((rc = nm.cmask.upload(hc)) || (rc = nm.pfix.upload(hp))) { (void)hipGetLastError(); return rc; }
            nm.on = true;
        }
        mk = std::move(nm);
        return model_changed();
    }

    // ---- measurement model (ba_solver_set_loss / ba_solver_set_obs_weights) -----------------------------------------------------------
    // Anything but the reference's psi at its 0.5 px without weights selects the MODEL instantiations of k_eval; nothing else changes
    // (everything downstream is built from e and J).  psi at another tau goes there too: the default kernels keep the reference's
    // clamps 1 / max(1e-15, .), which falsify dE/dr below |r|^2 = 1e-15, and the model's contract is a derivative that is right down to 0.  `tau` stays the reference's threshold: ba_solver_stats is its only other consumer.
    bool model() const { return md.loss_kind != BA_LOSS_REFERENCE || md.loss_scale != (T)0.5 || md.wobs.p != nullptr || ac.on(); }
    // the end of every setter that changes what a linearisation computes (mask, model, priors, constraints): the captured iterations
    // hold the other instantiations, kernel arguments and buffer addresses and are captured again on the next ba_minimize
    // (measurement: the loss or the weights, which triangulate() must not meet before a linearisation has taken them up)
    int model_changed(bool measurement = false) { drop_trial_graphs(); vf.model_changed(measurement); return BA_OK; }
    int set_loss(int kind, double scale) override
    {
        if (kind < BA_LOSS_REFERENCE || kind > BA_LOSS_CAUCHY) return BA_ERR_ARG;
        if (kind == BA_LOSS_TRIVIAL) scale = 1.0; // (ignored)
        else if (!positive_in_T(scale)) return BA_ERR_ARG;
        HIPCHK(hipStreamSynchronize(st));
        md.loss_kind = kind; md.loss_scale = (T)scale;
        return model_changed(true);
    }
    int set_obs_weights(const double *w) override
    {
        for (int i = 0; w && i < sx.K; i++)
            if (!positive_in_T(w[i])) return BA_ERR_ARG;
        HIPCHK(hipStreamSynchronize(st));
        DevBuf<T> nw;
        if (w) {
            std::vector<T> hw((size_t)(Kl > 0 ? Kl : 1), (T)1.0);
            for (int i = 0; i < Kl; i++) hw[i] = (T)w[sx.perm[sx.o0 + i]];
            int rc;
            if ((rc = nw.upload(hw))) { (void)hipGetLastError(); return rc; }
        }
        if (ac.on()) { // the mask stays: w_eff anew from the new weights
            std::vector<T> he((size_t)Kl);
            for (int i = 0; i < Kl; i++) he[i] = ac.h_act[i] ? (w ? (T)w[sx.perm[sx.o0 + i]] : (T)1.0) : (T)0;
            HIPCHK(hipMemcpy(ac.weff.p, he.data(), sizeof(T) * he.size(), hipMemcpyHostToDevice));
        }
        md.wobs = std::move(nw);
        return model_changed(true);
    }

    // ---- the active mask and the filter (ba_solver_set_obs_active / ba_solver_filter_observations; ba_filter.hip.h)
    // An inactive observation is an effective weight of 0, which the MODEL instantiations of k_eval select to e = 0, J = 0; nothing else
    // changes (everything downstream is built from e and J).  Active ac: the bytes, w_eff and the host's copy; its device buffers are
    // allocated once and stay (ac.on() says whether they are read).
    bool active_refused() const { return !chol_elim() || sharded(); }
    int active_alloc() // everything of Active that can fail
    {
        if (ac.act.p) return BA_OK;
        DevBuf<unsigned char> na;
        DevBuf<T> ne;
        int rc;
        if ((rc = na.alloc((size_t)(Kl > 0 ? Kl : 1))) || (rc = ne.alloc((size_t)(Kl > 0 ? Kl : 1)))) { (void)hipGetLastError(); return rc; }
        ac.act = std::move(na); ac.weff = std::move(ne);
        return BA_OK;
    }
    int set_obs_active(const unsigned char *active) override
    {
        if (active_refused()) return BA_ERR_ARG;
        std::vector<unsigned char> ha;
        long long off = 0;
        if (active) {
            ha.resize((size_t)Kl);
            for (int i = 0; i < Kl; i++) { ha[i] = active[sx.perm[sx.o0 + i]] != 0; off += !ha[i]; }
        }
        if (off == 0) ha.clear();
        if (ha == ac.h_act) return BA_OK; // the mask as it was: no flag changes
        HIPCHK(hipStreamSynchronize(st));
        if (off > 0) {
            int rc;
            if ((rc = active_alloc())) return rc;
            std::vector<T> he((size_t)Kl, (T)1.0);
            if (md.wobs.p) HIPCHK(hipMemcpy(he.data(), md.wobs.p, sizeof(T) * he.size(), hipMemcpyDeviceToHost));
            for (int i = 0; i < Kl; i++) if (!ha[i]) he[i] = (T)0;
            HIPCHK(hipMemcpy(ac.act.p, ha.data(), ha.size(), hipMemcpyHostToDevice));
            HIPCHK(hipMemcpy(ac.weff.p, he.data(), sizeof(T) * he.size(), hipMemcpyHostToDevice));
        }
        ac.h_act = std::move(ha);
        ac.n_off = off;
        return model_changed(true);
    }
    int get_obs_active(unsigned char *active, long long *n_active) override
    {
        for (int i = 0; active && i < Kl; i++) active[sx.perm[sx.o0 + i]] = ac.on() ? ac.h_act[i] : 1;
        if (n_active) *n_active = (long long)Kl - ac.n_off;
        return BA_OK;
    }
    int filter(const ba_filter_params *pp, int apply, unsigned char *obs_status, unsigned char *pt_status, double *err_px, ba_filter_stats *stats) override
    {
        ba_filter_params fp;
        if (pp) fp = *pp; else ba_filter_params_default(&fp);
        if (active_refused() || ba_filter_params_check(&fp)) return BA_ERR_ARG;
        int rc;
        if (!fl.part.p) { // everything that can fail first: the solver is unchanged behind an error
            Filter nf;
            const size_t k1 = (size_t)(Kl > 0 ? Kl : 1), m1 = (size_t)(Ml > 0 ? Ml : 1);
            if ((rc = nf.st.alloc(k1)) || (rc = nf.pst.alloc(m1)) || (rc = nf.nact.alloc(k1)) || (rc = nf.err.alloc(k1)) || (rc = nf.ray.alloc(3 * k1)) ||
                (rc = nf.part.alloc((size_t)BA_FLT_NSUM * tri_gmax() + 16)) || (rc = nf.nweff.alloc(k1))) { (void)hipGetLastError(); return rc; }
            HIPCHK(hipMemset(nf.part.p, 0, sizeof(double) * nf.part.n));
            fl = std::move(nf);
        }
        if (apply && (rc = active_alloc())) return rc;
        HIPCHK(hipStreamSynchronize(st));
        const double amin = fp.min_angle_deg * (M_PI / 180.0);
        const ba_flt_cfg cf{fp.max_reproj_px, amin, ba_flt_chord2_exit(amin), fp.min_track, fp.require_front != 0};
        const int g = tri_gmax();
        double *sums = fl.part.p + (size_t)BA_FLT_NSUM * g;
        const unsigned char *act = ac.on() ? (const unsigned char *)ac.act.p : nullptr;
        HIPCHK(hipEventRecord(ev[EV_T0], st));
        hipLaunchKernelGGL((k_filter_obs<T, TRI_LANES>), dim3(g), dim3(256), 0, st, N, Ml, Kl, (const int *)d_pt_ptr.p, (const int *)d_obs_cam.p,
                           (const T *)d_cam[0].p, (const T *)d_pts[0].p, (const T *)d_meas.p, act, cf, fl.st.p, fl.err.p, fl.ray.p);
        hipLaunchKernelGGL((k_filter_points<T, TRI_LANES>), dim3(g), dim3(256), 0, st, Ml, Kl, (const int *)d_pt_ptr.p, cf, fl.st.p, (const double *)fl.err.p,
                           (const double *)fl.ray.p, (const T *)md.wobs.p, fl.pst.p, apply ? fl.nact.p : (unsigned char *)nullptr,
                           apply ? fl.nweff.p : (T *)nullptr, fl.part.p);
        ba_red_jobs jobs{};
        for (int k = 0; k < 8; k++) jobs.j[k] = {fl.part.p + (size_t)k * g, g, 0, k};
        hipLaunchKernelGGL((k_reduce_scalars<double>), dim3(8), dim3(256), 0, st, jobs, sums, (const int *)nullptr, (long long *)nullptr);
        ba_red_jobs jobs2{};
        for (int k = 0; k < 2; k++) jobs2.j[k] = {fl.part.p + (size_t)(8 + k) * g, g, 0, 8 + k};
        hipLaunchKernelGGL((k_reduce_scalars<double>), dim3(2), dim3(256), 0, st, jobs2, sums, (const int *)nullptr, (long long *)nullptr);
        HIPCHK(hipEventRecord(ev[EV_T1], st));
        double h[BA_FLT_NSUM];
        HIPCHK(hipMemcpyAsync(h, sums, sizeof h, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        HIPCHK(hipGetLastError());
        ba_filter_stats fs{};
        for (int k = 0; k < 6; k++) fs.by_status[k] = (long long)h[k];
        fs.points_short = (long long)h[6]; fs.points_low_angle = (long long)h[7];
        fs.err_sum_before = h[8]; fs.err_sum_after = h[9];
        fs.active_before = (long long)Kl - fs.by_status[BA_OBS_WAS_OFF];
        fs.active_after = fs.by_status[BA_OBS_KEPT];
        fs.ms = ev_ms(EV_T0, EV_T1);
        // the outputs in file order, as set_obs_weights takes its input
        if (obs_status) {
            std::vector<unsigned char> hs((size_t)Kl);
            if (Kl) HIPCHK(hipMemcpy(hs.data(), fl.st.p, hs.size(), hipMemcpyDeviceToHost));
            for (int i = 0; i < Kl; i++) obs_status[sx.perm[sx.o0 + i]] = hs[i];
        }
        if (err_px) {
            std::vector<double> he((size_t)Kl);
            if (Kl) HIPCHK(hipMemcpy(he.data(), fl.err.p, sizeof(double) * he.size(), hipMemcpyDeviceToHost));
            for (int i = 0; i < Kl; i++) err_px[sx.perm[sx.o0 + i]] = he[i];
        }
        if (pt_status && Ml) HIPCHK(hipMemcpy(pt_status, fl.pst.p, (size_t)Ml, hipMemcpyDeviceToHost));
        if (stats) *stats = fs;
        if (!apply || fs.active_after == fs.active_before) return BA_OK; // a measurement, or nothing deactivated: every bit and flag stays
        std::vector<unsigned char> ha((size_t)Kl);
        HIPCHK(hipMemcpy(ha.data(), fl.nact.p, ha.size(), hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(ac.act.p, fl.nact.p, ha.size(), hipMemcpyDeviceToDevice));
        HIPCHK(hipMemcpy(ac.weff.p, fl.nweff.p, sizeof(T) * ha.size(), hipMemcpyDeviceToDevice));
        ac.h_act = std::move(ha);
        ac.n_off = (long long)Kl - fs.active_after;
        return model_changed(true);
    }

    // ---- Gaussian priors (ba_solver_set_point_priors / _centre_priors / _intrinsics_priors; ba_prior.hip.h) ------
    // Compact device lists per type; the block partials of k_prior live behind k_eval's in d_part_e (energies) and behind
    // k_point_prep's in d_part_pm (point diagonals), so that the existing second-stage jobs sum them in their fixed order.  No prior:
    // no list, pr.g = 0, the buffers at their old sizes and not one launch or argument more.
    bool priors() const { return pr.g > 0; }
    // The fused linearisation eliminates the next trial's points from registers, before a prior could join U0: with priors its records
    // are not used -- every trial runs k_elim_chol on the U0 / gp that k_prior has completed -- while J, U0, gp and the energy partials
    // still come from the kernel a solver without priors runs (so priors without information leave its bits alone, fp32 included,
    // where the separate-launch linearisation does not reproduce the fused one's bits).
    bool fused_records() const { return fuse && !priors() && !marq(); } // (Marquardt: the records of a lambda I elimination are not the trial's)
    // lin: the linearisation part (adds into U0 / gp / V / gc of the state `which`); else the energy at xTest alone
    void launch_prior(bool lin, int which, const int *go)
    {
        ba_prior_args<T> pa{pr.of[0].n, pr.of[1].n, pr.of[2].n, pr.of[0].id.p, pr.of[1].id.p, pr.of[2].id.p, pr.of[0].x0.p, pr.of[0].info.p,
                            pr.of[1].x0.p, pr.of[1].info.p, pr.of[2].x0.p, pr.of[2].info.p};
        // (the mask is a property of the linearisation: the energy at xTest always runs the unmasked instantiation, MASK = LIN && ...)
        with_flags(lin, mk.on, [&](auto LIN, auto MASKED) {
            hipLaunchKernelGGL((k_prior<T, LIN(), LIN() && MASKED()>), dim3(pr.g), dim3(256), 0, st, pa, N, Ml, (const T *)d_cam[which].p,
                               (const T *)d_pts[which].p, d_U0.p, d_gp.p, d_V.p, d_gc.p, part_e_priors(), pr.part.p, part_pm_priors(), go,
                               (const unsigned short *)mk.cmask.p, (const unsigned char *)mk.pfix.p);
        });
    }
    // type 0 points (info = L, 9 per prior), 1 centres (L), 2 intrinsics (info = w, 3 per prior)
    int set_priors(int type, int n, const int *ids, const double *x0, const double *info) override
    {
        if (!chol_elim() || sharded() || n < 0 || (n > 0 && (!ids || !x0 || !info))) return BA_ERR_ARG;
        const int lim = type == 0 ? sx.M : N, ni = type == 2 ? 3 : 9;
        if (!distinct_ids(n, ids, lim) || !finite_in_T(x0, (size_t)3 * n) || !finite_in_T(info, (size_t)ni * n)) return BA_ERR_ARG;
        HIPCHK(hipStreamSynchronize(st));
        const int tot = pr.of[0].n + pr.of[1].n + pr.of[2].n - pr.of[type].n + n, gp_new = (tot + 255) / 256;
        int rc;
        // everything that can fail first: the solver is unchanged behind an error
        PriorList nl;
        DevBuf<int> nlone;
        DevBuf<T> npart;
        if (type == 0) {
            std::vector<int> lone;
            for (int q = 0; q < n; q++)
                if (sx.pt_ptr[ids[q] + 1] == sx.pt_ptr[ids[q]]) lone.push_back(ids[q]);
            if ((rc = nlone.upload(lone))) { (void)hipGetLastError(); return rc; }
        }
        if (n > 0) {
            std::vector<int> hid(ids, ids + n);
            std::vector<T> hx((size_t)3 * n), hi((size_t)ni * n);
            for (size_t q = 0; q < hx.size(); q++) hx[q] = (T)x0[q];
            for (size_t q = 0; q < hi.size(); q++) hi[q] = (T)info[q];
            if ((rc = nl.id.upload(hid)) || (rc = nl.x0.upload(hx)) || (rc = nl.info.upload(hi))) { (void)hipGetLastError(); return rc; }
            nl.n = n;
        }
        if (gp_new != pr.g) {
            if ((rc = npart.alloc(3 * (size_t)gp_new))) { (void)hipGetLastError(); return rc; }
            if (npart.p) HIPCHK(hipMemset(npart.p, 0, sizeof(T) * npart.n));
            if ((rc = resize_partials(gp_new, rp.g))) return rc;
            pr.part = std::move(npart);
            pr.g = gp_new;
        }
        pr.of[type] = std::move(nl); // (one type's lists are what a call replaces: the other two stay)
        if (type == 0) pr.lonely = std::move(nlone);
        return model_changed();
    }
    // the energies a linearisation kept aside: q rows of g block partials, each summed in index order in T (zeros for g = 0)
    int kept_energy(const T *part, int q, int g, double *out)
    {
        if (!chol_elim() || sharded() || !vf.have_lin || vf.mask_pending) return BA_ERR_ARG;
        std::vector<T> h;
        int rc;
        if (g > 0 && (rc = dl(part, (size_t)q * g, h))) return rc;
        for (int r = 0; r < q; r++) {
            T a = 0;
            for (int b = 0; b < g; b++) a += h[(size_t)r * g + b];
            out[r] = (double)a;
        }
        return BA_OK;
    }
    // the three sums of the last linearisation's partials
    int prior_energy(double *out3) override { return kept_energy(pr.part.p, 3, pr.g, out3); }

    // ---- relative-pose constraints (ba_solver_set_relative_poses; ba_relpose.hip.h) -------------------------------
    // The lists, the per-constraint records and the CSR of every camera's incident constraints (built here, list order); the block
    // partials of k_relpose live behind the priors' in d_part_e.  No constraint: no buffer, rp.g = 0, not one launch more.
    bool relposes() const { return rp.n > 0; }
    ba_relpose_csr<T> relpose_csr() const { return ba_relpose_csr<T>{rp.ptr.p, rp.inc.p, rp.pair.p, rp.rec.p}; }
    // lin: the linearisation part (records, then the gather into V / gc of the state `which`); else the energy at xTest alone
    void launch_relpose(bool lin, int which, const int *go)
    {
        ba_relpose_args<T> ra{rp.n, rp.pair.p, rp.R0.p, rp.t0.p, rp.Lr.p, rp.Lt.p};
        with_flags(lin, mk.on && mk.cmask.p, [&](auto LIN, auto MASKED) { // (MASK = LIN && ..., as in launch_prior)
            hipLaunchKernelGGL((k_relpose<T, LIN(), LIN() && MASKED()>), dim3(rp.g), dim3(256), 0, st, ra, N, (const T *)d_cam[which].p, rp.rec.p,
                               part_e_relposes(), rp.part.p, go, (const unsigned short *)mk.cmask.p);
        });
        if (!lin) return;
        hipLaunchKernelGGL((k_relpose_gather<T>), dim3((unsigned)(((size_t)N * BA_RP_ENT + 255) / 256)), dim3(256), 0, st, N, relpose_csr(), d_V.p, d_gc.p, go);
    }
    int set_relposes(int n, const int *pairs, const double *R0, const double *t0, const double *Lr, const double *Lt) override
    {
        if (!chol_elim() || sharded() || n < 0 || (n > 0 && (!pairs || !R0 || !t0 || !Lr || !Lt))) return BA_ERR_ARG;
        {
            std::vector<long long> seen;
            seen.reserve((size_t)n);
            for (int q = 0; q < n; q++) {
                const int a = pairs[2 * q], b = pairs[2 * q + 1];
                if (a < 0 || b < 0 || a >= N || b >= N || a == b) return BA_ERR_ARG;
                seen.push_back((long long)std::max(a, b) * N + std::min(a, b));
            }
            std::sort(seen.begin(), seen.end());
            if (std::adjacent_find(seen.begin(), seen.end()) != seen.end()) return BA_ERR_ARG; // (an unordered pair listed twice)
        }
        if (n > 0 && !(finite_in_T(R0, (size_t)9 * n) && finite_in_T(t0, (size_t)3 * n) && finite_in_T(Lr, (size_t)9 * n) && finite_in_T(Lt, (size_t)9 * n)))
            return BA_ERR_ARG;
        for (int q = 0; q < n; q++) { // R0 a rotation
            const double *R = R0 + 9 * (size_t)q;
            double dev = 0;
            for (int i = 0; i < 3; i++)
                for (int j = 0; j < 3; j++)
                    dev = std::max(dev, std::fabs(R[3 * i] * R[3 * j] + R[3 * i + 1] * R[3 * j + 1] + R[3 * i + 2] * R[3 * j + 2] - (i == j ? 1.0 : 0.0)));
            const double det = R[0] * (R[4] * R[8] - R[5] * R[7]) - R[1] * (R[3] * R[8] - R[5] * R[6]) + R[2] * (R[3] * R[7] - R[4] * R[6]);
            if (!(dev <= 1e-6) || !(det > 0)) return BA_ERR_ARG;
        }
        HIPCHK(hipStreamSynchronize(st));
        int rc;
        // everything that can fail first: the solver is unchanged behind an error
        RelPoses nr;
        nr.n = n; nr.g = (n + 255) / 256;
        nr.h_pair.assign(pairs, pairs + 2 * (size_t)n);
        if (n > 0) {
            std::vector<int> ptr, inc;
            ba_plan_relpose_csr(N, n, pairs, ptr, inc);
            auto conv = [](const double *v, size_t cnt) { std::vector<T> h(cnt); for (size_t q = 0; q < cnt; q++) h[q] = (T)v[q]; return h; };
            if ((rc = nr.pair.upload(nr.h_pair)) || (rc = nr.ptr.upload(ptr)) || (rc = nr.inc.upload(inc)) || (rc = nr.R0.upload(conv(R0, (size_t)9 * n))) ||
                (rc = nr.t0.upload(conv(t0, (size_t)3 * n))) || (rc = nr.Lr.upload(conv(Lr, (size_t)9 * n))) || (rc = nr.Lt.upload(conv(Lt, (size_t)9 * n))) ||
                (rc = nr.rec.alloc((size_t)BA_RP_REC * n)) || (rc = nr.part.alloc(2 * (size_t)nr.g))) { (void)hipGetLastError(); return rc; }
            HIPCHK(hipMemset(nr.rec.p, 0, sizeof(T) * nr.rec.n));
            HIPCHK(hipMemset(nr.part.p, 0, sizeof(T) * nr.part.n));
        }
        Forest nf; // (ba_solver_set_preconditioner in front of this call: the forest of the new list)
        if (iterative() && (rc = build_forest(nr.h_pair, precond_kind, precond_max_tree, nf))) return rc;
        if (nr.g != rp.g && (rc = resize_partials(pr.g, nr.g))) return rc;
        rp = std::move(nr);
        fo = std::move(nf);
        return model_changed();
    }
    // {sum |e_r|^2, sum |e_t|^2} of the last linearisation's partials
    int relpose_energy(double *out2) override { return kept_energy(rp.part.p, 2, rp.g, out2); }

    ba_red_jobs test_energy_jobs() const
    {
        ba_red_jobs jobs{};
        jobs.j[0] = {d_part_e.p, part_e_n(), 0, SC_ETEST};
        jobs.j[1] = {d_part_bs.p, gB, 0, SC_RHO_P};
        jobs.j[2] = {d_part_bs.p + gB, gB, 0, SC_DN_P};
        return jobs;
    }
    // reduce: false when the control kernel behind this trial sums the partials itself (launch_seg_ctl, single shard)
    void launch_test_energy(bool reduce = true)
    {
        launch_eval(false, 1);
        if (priors()) launch_prior(false, 1, nullptr);
        if (relposes()) launch_relpose(false, 1, nullptr);
        if (reduce) hipLaunchKernelGGL((k_reduce_scalars<T>), dim3(3), dim3(256), 0, st, test_energy_jobs(), d_scal.p, (const int *)nullptr);
    }

    // sharded: the block-lower trapezoid of S (matrix + rhs row + g_c row: half the bytes of the full buffer) + one tail scalar
    size_t pack_count() const
    {
        const int nbc = Dp / NB;
        return (size_t)64 * ((size_t)nbc * Dp - (size_t)32 * nbc * (nbc - 1));
    }
    int launch_pack(bool unpack)
    {
        const size_t npk = pack_count();
        int rc;
        if (!d_pack.p && (rc = d_pack.alloc(npk + 1))) return rc;
        const dim3 gpk((Dp + 255) / 256 > 8 ? 8 : (Dp + 255) / 256, Dp);
        with_flag(unpack, [&](auto UNPACK) {
            hipLaunchKernelGGL((k_pack_lower<T, UNPACK()>), gpk, dim3(256), 0, st, Dp, ld, d_S.p, d_pack.p, npk, d_scal.p, (int)SC_ELOC, (int)SC_ENERGY);
        });
        return BA_OK;
    }

    // S, or (QRKIT / QRSPQR / MOREQR) the dense J2bot
    void launch_assemble(bool pairs = true) { if (dense_qr()) launch_qrkit_build(); else launch_schur(pairs); }
    // The tail of an iteration prepares the next trial: behind the step control, which has left the next lambda, the records are made
    // (the fused k_eval behind an accepted step, k_elim_chol behind a rejected one) and the pairs assembled beside the camera Gram.  The
    // trial that follows starts at k_schur_reduce (enqueue_trial: head = false).  Where fused_records() holds, for the plain CHOLESKY
    // solve in fp64 on one shard; every other configuration keeps the head in front of every trial.
    bool tail_prepares() const
    {
        return !trial_head && kind == BA_CHOLESKY && sizeof(T) == 8 && fused_records() && !sharded() && !relposes() && !mk.on && post_folded() &&
               sx.nchunks > 0 && sx.ndchunks > 0;
    }
    // a phase boundary of try_step's timing (ba_timing); nothing in a captured segment
    int mark(int e) { if (step_level) HIPCHK(hipEventRecord(ev[e], st)); return BA_OK; }
    // The segments of one trial (everything behind lambda in SC_LAMBDA).  Single shard: A + B back to back; sharded: the
    // exchange between A and B and an all-reduce of the step scalars behind B.  try_step runs the same segments (step_level).
    int launch_seg_a()
    {
        int rc;
        const bool head = seg_head || !tail_prepares();
        if (head) launch_eliminate();
        if ((rc = mark(EV_T1))) return rc;
        if (iterative()) { launch_pcg_prep(); return mark(EV_T2); } // (single shard: nothing to exchange)
        launch_assemble(head);
        if ((rc = mark(EV_T2))) return rc;
        if (dense_qr()) return sharded() ? launch_qr_stack_pack() : BA_OK;
        if (dist_on()) return launch_dist_pack();
        return sharded() ? launch_pack(false) : BA_OK;
    }
    int launch_seg_b()
    {
        int rc;
        if (dist_on()) { if ((rc = launch_dist_unpack())) return rc; }
        else if (sharded() && !dense_qr() && (rc = launch_pack(true))) return rc;
        if ((rc = mark(EV_T3))) return rc;
        if (iterative()) launch_pcg_solve();
        else if (dense_qr()) { if (sharded()) launch_qr_stack_solve(); else launch_qrkit_solve(); }
        else {
            launch_post_reduce();
            if (keep && step_level) {
                if (!d_Skeep.p && (rc = d_Skeep.alloc(d_S.n))) return rc;
                HIPCHK(hipMemcpyAsync(d_Skeep.p, d_S.p, sizeof(T) * d_S.n, hipMemcpyDeviceToDevice, st));
            }
            if (dist_on()) { if ((rc = launch_factor_solve_dist())) return rc; }
            else launch_factor_solve();
        }
        if ((rc = mark(EV_T4))) return rc;
        launch_backsub_retract();
        if (pr.lonely.n > 0) { // (points with a prior and no observation: none on a usual problem, no launch then)
            with_flag(mk.on, [&](auto MASKED) { // (two kernels, not two instantiations of one: the Marquardt one takes the bounds)
                const unsigned char *pfix = MASKED() ? (const unsigned char *)mk.pfix.p : nullptr;
                if (marq())
                    hipLaunchKernelGGL((k_prior_lonely_marq<T, MASKED()>), dim3(1), dim3(256), 0, st, (int)pr.lonely.n, (const int *)pr.lonely.p, Ml,
                                       (const T *)d_U0.p, (const T *)d_gp.p, (const T *)(d_scal.p + SC_LAMBDA), (const T *)d_pts[0].p, d_dxp.p, d_pts[1].p,
                                       d_part_bs.p, gB, pfix, damp_args());
                else
                    hipLaunchKernelGGL((k_prior_lonely<T, MASKED()>), dim3(1), dim3(256), 0, st, (int)pr.lonely.n, (const int *)pr.lonely.p, Ml,
                                       (const T *)d_U0.p, (const T *)d_gp.p, (const T *)(d_scal.p + SC_LAMBDA), (const T *)d_pts[0].p, d_dxp.p, d_pts[1].p,
                                       d_part_bs.p, gB, pfix);
            });
        }
        if ((rc = mark(EV_T5))) return rc;
        launch_test_energy(step_level || !ctl_reduces()); // (single shard: k_lm_control sums the three partial arrays at its head)
        return BA_OK;
    }
    // reduced camera system (or stack of R factors) + rhs + g_c + energy tail; the distributed factor only needs each rank's own
    // block columns summed: a reduce-scatter (half the bytes) + g_c and the energy in a small all-reduce.  Single shard: nothing.
    int exchange() { return dist_on() ? dist_exchange() : allreduce(xchg_ptr(), xchg_count(), 0); }
    // step control on the device, x = xTest and the linearisation of the next outer iteration, the latter two conditional
    int launch_seg_ctl()
    {
        ba_lm_slots sl{SC_ENERGY, SC_ETEST, SC_RHO_P, SC_RHO_C, SC_DN_P, SC_DN_C, SC_LAMBDA, SC_ERR, SC_GUARD, world};
        hipLaunchKernelGGL((k_lm_control<T>), dim3(1), dim3(256 * BA_LM_JOBS), 0, st, d_scal.p, d_lm.p, d_log, sl, test_energy_jobs(), ctl_reduces() ? 3 : 0);
        int rc = linearize_enqueue(false, &d_lm.p->go, tail_prepares()); // (x = xTest happens inside its first kernel)
        if (!rc && more_qr() && !sharded()) rc = more_outer_finish(&d_lm.p->go); // (sharded: behind the segment, it holds an all-reduce -- enqueue_trial)
        return rc;
    }

    // m_solver.compute .. dx; xTest = x (+) dx; m_functor(xTest); rhoScale (BacktrackLevMarqQRChol.h:291-375): the step-level
    // seam, host-synchronous: the segments ba_minimize replays as graphs under device-side control, with per-phase events.
    int try_step(double lambda_d, double *e_test, double *rho_scale, double *dx_norm) override
    {
        int rc;
        if (vf.mask_pending) return BA_ERR_ARG; // (the linearisation in place was made under another mask)
        if ((rc = set_lambda((T)lambda_d))) return rc;
        HIPCHK(hipEventRecord(ev[EV_T0], st));
        step_level = true;
        if (!(rc = launch_seg_a()) && !(rc = exchange())) rc = launch_seg_b();
        step_level = false;
        if (rc) return rc;
        HIPCHK(hipEventRecord(ev[EV_T6], st));
        if ((rc = allreduce(d_scal.p + SC_ETEST, N_STEP_SCALARS, 0))) return rc; // (the error word too: a time-out of one shard fails the step on all)
        if ((rc = fetch_scalars())) return rc;
        HIPCHK(hipGetLastError());
        tm.eliminate_ms += ev_ms(EV_T0, EV_T1);
        tm.schur_ms += ev_ms(EV_T1, EV_T2);
        if (sharded()) tm.comm_ms += ev_ms(EV_T2, EV_T3);
        tm.factor_ms += ev_ms(EV_T3, EV_T4);
        tm.backsub_ms += ev_ms(EV_T4, EV_T5);
        tm.test_eval_ms += ev_ms(EV_T5, EV_T6);
        tm.trial_ms += ev_ms(EV_T0, EV_T6);
        tm.n_trials++;
        if (e_test) *e_test = (double)h_scal[SC_ETEST];
        if (rho_scale) *rho_scale = (double)(h_scal[SC_RHO_P] + h_scal[SC_RHO_C]);
        if (dx_norm) *dx_norm = std::sqrt((double)(h_scal[SC_DN_P] + h_scal[SC_DN_C]));
        vf.stepped();
        return BA_OK;
    }

    // x = xTest (BacktrackLevMarqQRChol.h:428)
    int accept() override
    {
        if (!vf.have_step) return BA_ERR_ARG;
        vf.results_dropped(); // (have_lin stays: J is still the old x's, and ba_solver_try_step is not refused behind an accept)
        const int ncam = 15 * N, npts = 3 * Ml;
        hipLaunchKernelGGL((k_commit<T>), dim3((ncam + npts + 255) / 256), dim3(256), 0, st, ncam, npts, d_cam[1].p, d_pts[1].p, d_cam[0].p, d_pts[0].p,
                           (const int *)nullptr);
        HIPCHK(hipStreamSynchronize(st));
        vf.accepted();
        return BA_OK;
    }

    // ---- Powell's dogleg (ba_solver_dogleg_prepare / ba_solver_try_dogleg / ba_minimize_dogleg; ba_dogleg.hip.h) --
    // State of its own (Dogleg dg): the copy of dx_gn and one fp64 buffer of partials and sums, both allocated by the first prepare;
    // the scalars of the last prepare on the host.
    enum { DL_Q = 0, DL_G2, DL_GN2, DL_D, DL_DN, DL_NOUT = 8 };
    int dl_gd() const { return (int)(((size_t)3 * Ml + D + 255) / 256); }
    double *dl_part_q() const { return dg.part.p; }
    double *dl_part_dots() const { return dg.part.p + gK; }
    double *dl_part_dn() const { return dl_part_dots() + 3 * (size_t)dl_gd(); }
    double *dl_out() const { return dl_part_dn() + gM + 1; }
    // what every dogleg call refuses, the solver unchanged
    bool dogleg_kind_ok() const { return kind == BA_CHOLESKY && !sharded() && !priors() && !relposes() && damp_kind != BA_DAMP_MARQUARDT; }
    bool dogleg_ok() const { return dogleg_kind_ok() && vf.have_lin && !vf.mask_pending; }
    int dl_fetch(double *h)
    {
        HIPCHK(hipMemcpyAsync(h, dl_out(), sizeof(double) * DL_NOUT, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        return BA_OK;
    }

    void launch_jg()
    {
        hipLaunchKernelGGL((k_jg<T>), dim3(gK), dim3(256), 0, st, Kl, Ml, (const int *)d_obs_cam.p, (const int *)d_obs_pt.p, (const T *)d_JcA.p,
                           (const T *)d_Jp.p, (const T *)d_gc.p, (const T *)d_gp.p, dl_part_q());
    }

    int dogleg_prepare(double mu, ba_dogleg_info *out) override
    {
        if (!dogleg_ok() || !positive_in_T(mu)) return BA_ERR_ARG;
        int rc;
        if (!dg.keep.p || !dg.part.p) {
            Dogleg nd;
            if ((rc = nd.keep.alloc((size_t)3 * Ml + D)) || (rc = nd.part.alloc((size_t)gK + 3 * (size_t)dl_gd() + gM + 1 + DL_NOUT))) { (void)hipGetLastError(); return rc; }
            HIPCHK(hipMemset(nd.part.p, 0, sizeof(double) * nd.part.n));
            dg = std::move(nd);
        }
        vf.dogleg_dropped();
        double e_gn = 0, rs_gn = 0;
        if ((rc = try_step(mu, &e_gn, &rs_gn, nullptr))) return rc;
        hipLaunchKernelGGL((k_dogleg_dots<T>), dim3(dl_gd()), dim3(256), 0, st, 3 * Ml, D, (const T *)d_gp.p, (const T *)d_gc.p, (const T *)d_dxp.p,
                           (const T *)d_dxc.p, dg.keep.p, dl_part_dots());
        launch_jg();
        ba_red_jobs jobs{};
        jobs.j[0] = {dl_part_q(), gK, 0, DL_Q};
        for (int k = 0; k < 3; k++) jobs.j[1 + k] = {dl_part_dots() + (size_t)k * dl_gd(), dl_gd(), 0, DL_G2 + k};
        hipLaunchKernelGGL((k_reduce_scalars<double>), dim3(4), dim3(256), 0, st, jobs, dl_out(), (const int *)nullptr, (long long *)nullptr);
        double h[DL_NOUT];
        if ((rc = dl_fetch(h))) return rc;
        HIPCHK(hipGetLastError());
        dg.info.mu = mu; dg.info.g2 = h[DL_G2]; dg.info.q = h[DL_Q]; dg.info.gn2 = h[DL_GN2]; dg.info.g_dot_gn = h[DL_D];
        dg.info.alpha = dg.info.g2 > 0 ? dg.info.g2 / dg.info.q : 0.0;
        dg.info.energy_gn = e_gn; dg.info.rho_scale_gn = rs_gn;
        vf.dogleg_prepared();
        if (out) *out = dg.info;
        return BA_OK;
    }

    int try_dogleg(double radius, double *e_test, double *pred, double *dx_norm, int *branch) override
    {
        if (!dogleg_ok() || !vf.dl_valid || !(radius > 0)) return BA_ERR_ARG;
        double a = 0, c = 0, pred_v = 0;
        int br = 0, rc;
        if ((rc = ba_dogleg_coefficients(dg.info.g2, dg.info.q, dg.info.gn2, dg.info.g_dot_gn, dg.info.mu, radius, &a, &c, &br, &pred_v))) return rc;
        const ba_cam_retract_args cr{N, d_cam[0].p, d_dxc.p, d_gcg.p, d_cam[1].p, d_scal.p, (int)SC_RHO_C};
        with_flag(mk.on, [&](auto MASKED) {
            hipLaunchKernelGGL((k_dogleg_step<T, MASKED()>), dim3(gM + 1), dim3(256), 0, st, Ml, gM, (T)a, (T)c, (const int *)d_pt_ptr.p, (const T *)d_gp.p,
                               (const T *)d_gc.p, (const T *)dg.keep.p, (const T *)d_pts[0].p, d_dxp.p, d_dxc.p, d_pts[1].p,
                               (const T *)(d_scal.p + SC_LAMBDA), dl_part_dn(), cr, ba_fix_args{mk.cmask.p, mk.pfix.p});
        });
        launch_test_energy();
        ba_red_jobs jobs{};
        jobs.j[0] = {dl_part_dn(), gM + 1, 0, DL_DN};
        hipLaunchKernelGGL((k_reduce_scalars<double>), dim3(1), dim3(256), 0, st, jobs, dl_out(), (const int *)nullptr, (long long *)nullptr);
        double h[DL_NOUT];
        if ((rc = fetch_scalars()) || (rc = dl_fetch(h))) return rc;
        HIPCHK(hipGetLastError());
        if (e_test) *e_test = (double)h_scal[SC_ETEST];
        if (pred) *pred = pred_v;
        if (dx_norm) *dx_norm = std::sqrt(h[DL_DN]);
        if (branch) *branch = br;
        vf.stepped();
        return BA_OK;
    }

    // The control rule of include/ba_mi355x.h, host-synchronous; tests/dogleg_checks.py holds the same rule in Python.
    int minimize_dogleg(const ba_dogleg_params *dpp, ba_trial_cb cb, void *user, ba_result *out) override
    {
        if (poisoned) return BA_ERR_HIP;
        ba_dogleg_params dp;
        if (dpp) dp = *dpp; else ba_dogleg_params_default(&dp);
        if (!dogleg_kind_ok()) return BA_ERR_ARG; // (the driver linearises itself: a pending mask or model is taken up there)
        if (!(dp.radius_init >= 0) || !(dp.radius_min > 0) || !(dp.radius_max > 0) || !(dp.mu_rel > 0) || !(dp.mu_rel_max > 0) || !(dp.tol_fun > 0))
            return BA_ERR_ARG;
        const auto tbeg = std::chrono::steady_clock::now();
        const ba_timing tm0 = tm;
        const bool talk = dp.verbose != 0;
        if (talk) { // ba_minimize's table; the lambda column holds the radius of the trial
            printf("############################## Dogleg ##########################################\n");
            printf("--------------------------------------------------------------------------------\n");
            printf(" Iter%15s%15s%15s%15s%15s\n", "Status", "f", "rho", "radius", "Elapsed");
            printf("--------------------------------------------------------------------------------\n");
        }
        int rc = BA_OK, status = BA_RUNNING, iter = 0, trials = 0, fun_evals = 0;
        bool rows_done = false; // max_trials rows have been made
        double E = 0, dmax = 0, radius = dp.radius_init, m = 1;
        auto tlast = std::chrono::steady_clock::now();
        if (dp.max_trials >= 0 && !(rc = linearize(&E, &dmax))) {
            fun_evals = 1;
            while (status == BA_RUNNING && !rc && !rows_done) {
                if (++iter > dp.max_iter) { status = BA_MAX_ITERS; break; }
                ba_dogleg_info in{};
                double pred_gn = 0;
                bool ready = false;
                while (!ready) { // the Gauss-Newton step of this linearisation; a model that does not decrease: more regularisation, no trial
                    if (dp.mu_rel * m > dp.mu_rel_max) { status = BA_EXCEEDED_LAMBDA_MAX; break; }
                    if (fun_evals >= dp.max_fun_ev) { status = BA_TOO_MANY_FUN_EVALS; break; }
                    if ((rc = dogleg_prepare(dp.mu_rel * m * dmax, &in))) break;
                    fun_evals++;
                    if (in.g2 == 0) { status = BA_SUCCESS; break; }
                    // (scalars the rule refuses -- a step that is not finite: the factorisation broke down -- count as a pred that is not finite)
                    if (ba_dogleg_coefficients(in.g2, in.q, in.gn2, in.g_dot_gn, in.mu, INFINITY, nullptr, nullptr, nullptr, &pred_gn)) pred_gn = NAN;
                    if (pred_gn > 0 && std::isfinite(pred_gn)) ready = true;
                    else m *= 10;
                }
                if (!ready) break;
                m = std::max(1.0, m / 5);
                const double gn_norm = std::sqrt(in.gn2);
                if (iter == 1 && radius == 0) radius = gn_norm;
                for (bool first = true; status == BA_RUNNING && !rc; first = false) {
                    if (radius < dp.radius_min) { status = BA_EXCEEDED_LAMBDA_MAX; break; }
                    double e_test = in.energy_gn, pred = pred_gn, dxn = gn_norm;
                    if (!(first && gn_norm <= radius)) { // (else: the prepare's own xTest, used as it is)
                        if (fun_evals >= dp.max_fun_ev) { status = BA_TOO_MANY_FUN_EVALS; break; }
                        if ((rc = try_dogleg(radius, &e_test, &pred, &dxn, nullptr))) break;
                        fun_evals++;
                    }
                    trials++;
                    rows_done = dp.max_trials > 0 && trials >= dp.max_trials; // (this row is the last: what it decides is still carried out)
                    const bool accepted = pred > 0 && e_test < E;
                    const double rho = (E - e_test) / pred;
                    const auto tnow = std::chrono::steady_clock::now();
                    const double el = std::chrono::duration<double>(tnow - tlast).count();
                    tlast = tnow;
                    if (cb) cb(user, iter, accepted ? 1 : 0, E, rho, radius, el);
                    if (talk) printf("%5d%15s%15g%15g%15g%14gs\n", iter, accepted ? "Accepted" : "Rejected", E, rho, radius, el);
                    if (!accepted) {
                        radius /= 2;
                        if (rows_done) break;
                        continue;
                    }
                    const bool flat = (E - e_test) / E < dp.tol_fun;
                    if (rho > 0.75) radius = std::min(dp.radius_max, std::max(radius, 3 * dxn));
                    else if (rho < 0.25) radius /= 2;
                    if ((rc = accept())) break;
                    if (flat) { E = e_test; status = BA_SUCCESS; break; }
                    rc = linearize(&E, &dmax);
                    break;
                }
            }
        }
        if (talk) printf("--------------------------------------------------------------------------------\n");
        vf.x_moved(); // (as behind ba_minimize)
        if (out) {
            out->status = status; out->iterations = iter; out->trials = trials; out->fun_evals = fun_evals;
            out->energy = E; out->lambda = radius;
            out->seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - tbeg).count();
            const long long nt = tm.n_trials - tm0.n_trials, nl = tm.n_linearize - tm0.n_linearize;
            out->schur_ms = nt ? (tm.trial_ms - tm0.trial_ms) / nt : 0.0; // (the prepares: the trials that factor)
            out->linearize_ms = nl ? (tm.linearize_ms - tm0.linearize_ms) / nl : 0.0;
        }
        return rc;
    }

    // ---- triangulation (ba_solver_triangulate_points; ba_triangulate.hip.h) -------------------------------------
    // Buffers of its own (Triang tr), all allocated by the first call.
    enum { TRI_LANES = 8, TRI_NSUM = 10 };
    int tri_gmax() const { return std::max(1, (int)(((size_t)Ml * TRI_LANES + 255) / 256)); }

    int triangulate(const ba_triangulate_params *pp, int n_pts, const int *pt_ids, unsigned char *status, ba_triangulate_stats *stats) override
    {
        ba_triangulate_params tp;
        if (pp) tp = *pp; else ba_triangulate_params_default(&tp);
        if (sharded() || ba_triangulate_params_check(&tp) || n_pts < 0 || (!pt_ids && n_pts > 0) || vf.model_pending) return BA_ERR_ARG;
        const int n = pt_ids ? n_pts : Ml;
        if (pt_ids && !distinct_ids(n, pt_ids, Ml)) return BA_ERR_ARG;
        int rc;
        if (!tr.part.p) { // everything that can fail first: the solver is unchanged behind an error
            Triang nt;
            const size_t m1 = (size_t)(Ml > 0 ? Ml : 1);
            if ((rc = nt.ray.alloc((size_t)3 * (Kl > 0 ? Kl : 1))) || (rc = nt.part.alloc((size_t)TRI_NSUM * tri_gmax() + 16)) || (rc = nt.ids.alloc(m1)) ||
                (rc = nt.stat.alloc(m1)) || (rc = nt.fix.alloc(m1))) { (void)hipGetLastError(); return rc; }
            HIPCHK(hipMemset(nt.part.p, 0, sizeof(double) * nt.part.n));
            tr = std::move(nt);
        }
        HIPCHK(hipStreamSynchronize(st));
        ba_triangulate_stats ts{};
        ts.asked = n;
        if (n > 0) {
            // a point held constant or carrying a prior is never touched
            const bool any_fix = (mk.on && mk.pfix.p) || pr.of[0].n > 0;
            if (any_fix) {
                std::vector<unsigned char> hf((size_t)Ml, 0);
                if (mk.on && mk.pfix.p) HIPCHK(hipMemcpy(hf.data(), mk.pfix.p, (size_t)Ml, hipMemcpyDeviceToHost));
                if (pr.of[0].n > 0) {
                    std::vector<int> hid((size_t)pr.of[0].n);
                    HIPCHK(hipMemcpy(hid.data(), pr.of[0].id.p, sizeof(int) * hid.size(), hipMemcpyDeviceToHost));
                    for (int id : hid) hf[id] = 1;
                }
                HIPCHK(hipMemcpy(tr.fix.p, hf.data(), hf.size(), hipMemcpyHostToDevice));
            }
            if (pt_ids) HIPCHK(hipMemcpy(tr.ids.p, pt_ids, sizeof(int) * (size_t)n, hipMemcpyHostToDevice));
            const int *ids = pt_ids ? (const int *)tr.ids.p : nullptr;
            const int g = (int)(((size_t)n * TRI_LANES + 255) / 256);
            const ba_tri_cfg cf{tp.min_angle_deg * (M_PI / 180.0), tp.max_reproj_px, tp.refine_iters, tp.only_if_better, md.loss_kind, (double)md.loss_scale};
            double *sums = tr.part.p + (size_t)TRI_NSUM * tri_gmax();
            HIPCHK(hipEventRecord(ev[EV_T0], st));
            // (an inactive observation is not part of its track; no mask: a null pointer)
            const unsigned char *act = ac.on() ? (const unsigned char *)ac.act.p : nullptr;
            hipLaunchKernelGGL((k_tri_rays<T, TRI_LANES>), dim3(g), dim3(256), 0, st, n, ids, N, Kl, (const int *)d_pt_ptr.p, (const int *)d_obs_cam.p,
                               (const T *)d_cam[0].p, (const T *)d_meas.p, act, tr.ray.p);
            hipLaunchKernelGGL((k_tri_points<T, TRI_LANES>), dim3(g), dim3(256), 0, st, n, ids, N, Ml, Kl, (const int *)d_pt_ptr.p, (const int *)d_obs_cam.p,
                               (const T *)d_cam[0].p, (const T *)d_meas.p, (const T *)md.wobs.p, act, (const double *)tr.ray.p,
                               any_fix ? (const unsigned char *)tr.fix.p : (const unsigned char *)nullptr, cf, d_pts[0].p, tr.stat.p, tr.part.p);
            ba_red_jobs jobs{};
            for (int k = 0; k < 8; k++) jobs.j[k] = {tr.part.p + (size_t)k * g, g, 0, k};
            hipLaunchKernelGGL((k_reduce_scalars<double>), dim3(8), dim3(256), 0, st, jobs, sums, (const int *)nullptr, (long long *)nullptr);
            ba_red_jobs jobs2{};
            for (int k = 0; k < 2; k++) jobs2.j[k] = {tr.part.p + (size_t)(8 + k) * g, g, 0, 8 + k};
            hipLaunchKernelGGL((k_reduce_scalars<double>), dim3(2), dim3(256), 0, st, jobs2, sums, (const int *)nullptr, (long long *)nullptr);
            HIPCHK(hipEventRecord(ev[EV_T1], st));
            double h[TRI_NSUM];
            HIPCHK(hipMemcpyAsync(h, sums, sizeof h, hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));
            HIPCHK(hipGetLastError());
            if (status) HIPCHK(hipMemcpy(status, tr.stat.p, (size_t)n, hipMemcpyDeviceToHost));
            for (int k = 0; k < 8; k++) ts.by_status[k] = (long long)h[k];
            ts.cost_before = h[8]; ts.cost_after = h[9];
            ts.ms = ev_ms(EV_T0, EV_T1);
        }
        // what ba_solver_set_state(s, NULL, pts) invalidates; and J is another state's: ba_solver_try_step refuses until the next
        // linearisation, as it does behind a setter
        vf.points_reseated();
        if (stats) *stats = ts;
        return BA_OK;
    }

    int stats(double *out4) override
    {
        hipLaunchKernelGGL((k_stats<T>), dim3(gK), dim3(256), 0, st, Kl, N, Ml, d_cam[0].p, d_pts[0].p, d_obs_cam.p,
                           d_obs_pt.p, d_meas.p, tau, d_part_st.p);
        ba_red_jobs jobs{};
        for (int q = 0; q < 4; q++) jobs.j[q] = {d_part_st.p + (size_t)q * gK, gK, 0, SC_ST0 + q};
        hipLaunchKernelGGL((k_reduce_scalars<T>), dim3(4), dim3(256), 0, st, jobs, d_scal.p);
        int rc;
        if ((rc = allreduce(d_scal.p + SC_ST0, 4, 0))) return rc;
        if ((rc = fetch_scalars())) return rc;
        const double K = (double)sx.K;
        // accumulate and divide in Scalar like the reference (Utils.h:24-40)
        out4[0] = (double)(h_scal[SC_ST0] / (T)K);
        out4[1] = (double)(h_scal[SC_ST0 + 1] / h_scal[SC_ST0 + 2]);
        out4[2] = (double)h_scal[SC_ST0 + 2];
        out4[3] = (double)h_scal[SC_ST0 + 3];
        return BA_OK;
    }

    int dl(const T *src, size_t n, std::vector<T> &h)
    {
        h.resize(n);
        HIPCHK(hipStreamSynchronize(st));
        if (n) HIPCHK(hipMemcpy(h.data(), src, sizeof(T) * n, hipMemcpyDeviceToHost));
        return BA_OK;
    }

    // the device's SoA [Q][n] as the ABI's AoS [n][Q], and back
    static void soa_to_aos(const std::vector<T> &h, size_t n, int Q, double *out)
    {
        for (size_t i = 0; i < n; i++)
            for (int q = 0; q < Q; q++) out[Q * i + q] = h[q * n + i];
    }
    static std::vector<T> aos_to_soa(const double *in, size_t n, int Q)
    {
        std::vector<T> h(Q * n);
        for (size_t i = 0; i < n; i++)
            for (int q = 0; q < Q; q++) h[q * n + i] = (T)in[Q * i + q];
        return h;
    }

    int get(int what, double *out, size_t n) override
    {
        std::vector<T> h, h2;
        int rc;
        switch (what) {
        case BA_GET_RESIDUALS: {
            if (n != 2 * (size_t)Kl) return BA_ERR_ARG;
            if ((rc = dl(d_r.p, 2 * (size_t)Kl, h))) return rc;
            // file order inside the shard when the input was sorted; sorted order otherwise (perm documents it)
            for (int i = 0; i < Kl; i++) { out[2 * (size_t)i] = h[i]; out[2 * (size_t)i + 1] = h[(size_t)Kl + i]; }
            return BA_OK;
        }
        case BA_GET_JC: {
            if (n != 18 * (size_t)Kl) return BA_ERR_ARG;
            if (chol_elim()) { // the AoS records [Kl][20] are the only copy
                if ((rc = dl(d_JcA.p, 20 * (size_t)Kl, h))) return rc;
                for (int i = 0; i < Kl; i++)
                    for (int q = 0; q < 18; q++) out[18 * (size_t)i + q] = h[20 * (size_t)i + q];
                return BA_OK;
            }
            if ((rc = dl(d_Jc.p, 18 * (size_t)Kl, h))) return rc;
            for (int i = 0; i < Kl; i++)
                for (int q = 0; q < 18; q++) out[18 * (size_t)i + q] = h[(size_t)q * Kl + i];
            return BA_OK;
        }
        case BA_GET_JP: {
            if (n != 6 * (size_t)Kl) return BA_ERR_ARG;
            if ((rc = dl(d_Jp.p, 6 * (size_t)Kl, h))) return rc;
            soa_to_aos(h, Kl, 6, out);
            return BA_OK;
        }
        case BA_GET_GRAD:
        case BA_GET_DX: { // points, then cameras
            const bool grad = what == BA_GET_GRAD;
            if (n != 3 * (size_t)Ml + D) return BA_ERR_ARG;
            if ((rc = dl(grad ? d_gp.p : d_dxp.p, 3 * (size_t)Ml, h)) || (rc = dl(grad ? d_gc.p : d_dxc.p, D, h2))) return rc;
            soa_to_aos(h, Ml, 3, out);
            for (int c = 0; c < D; c++) out[3 * (size_t)Ml + c] = h2[c];
            return BA_OK;
        }
        case BA_GET_S:
        case BA_GET_RHS: {
            if (iterative()) { // no S; the reduced rhs of the last trial stays in d_pcg_b
                if (what == BA_GET_S || n != (size_t)D) return BA_ERR_ARG;
                if ((rc = dl(d_pcg_b.p, (size_t)D, h))) return rc;
                for (int c = 0; c < D; c++) out[c] = h[c];
                return BA_OK;
            }
            if (!d_Skeep.p) return BA_ERR_ARG;
            if ((rc = dl(d_Skeep.p, d_Skeep.n, h))) return rc;
            if (what == BA_GET_RHS) {
                if (n != (size_t)D) return BA_ERR_ARG;
                for (int c = 0; c < D; c++) out[c] = h[(size_t)c * ld + D];
            } else {
                if (n != (size_t)D * D) return BA_ERR_ARG;
                for (int c = 0; c < D; c++)
                    for (int rr = c; rr < D; rr++) out[(size_t)c * D + rr] = out[(size_t)rr * D + c] = h[(size_t)c * ld + rr];
            }
            return BA_OK;
        }
        case 11: { // diagnostic (QRKIT / QRSPQR, single shard, behind a step): the diagonal of R of the dense QR of J2bot (= the betas of the top TSQR level)
            if (!dense_qr() || n != (size_t)D || !d_qA.p) return BA_ERR_ARG;
            HIPCHK(hipStreamSynchronize(st));
            std::vector<T> col(1);
            for (int c = 0; c < D; c++) {
                HIPCHK(hipMemcpy(col.data(), d_qA.p + (size_t)c * q_lda + c, sizeof(T), hipMemcpyDeviceToHost));
                out[c] = (double)col[0];
            }
            return BA_OK;
        }
        case 14: { // diagnostic (BA_DBG_QRCHECK): [A^T (b - A y) | A^T b] of the last dense least-squares solve, 2 D values
            if (!dense_qr() || n != (size_t)2 * D || !d_dbg2.p) return BA_ERR_ARG;
            std::vector<T> hh;
            int rcg;
            if ((rcg = dl(d_dbg2.p, (size_t)2 * D, hh))) return rcg;
            for (int c = 0; c < 2 * D; c++) out[c] = (double)hh[c];
            return BA_OK;
        }
        case 15:   // diagnostic (BA_DBG_QRCHECK): the matrix of the last dense solve as built, inner_rows() x (D + 1) column-major
        case 16: { // diagnostic: the same matrix as the factorisation left it (R, reflectors in place, Q^T rhs in column D)
            const size_t rows = (size_t)inner_rows();
            const T *src = what == 15 ? d_qAcopy.p : d_qA.p;
            if (!dense_qr() || n != rows * (D + 1) || !src) return BA_ERR_ARG;
            HIPCHK(hipStreamSynchronize(st));
            std::vector<T> col(rows);
            for (int c = 0; c <= D; c++) {
                HIPCHK(hipMemcpy(col.data(), src + (size_t)c * q_lda, sizeof(T) * rows, hipMemcpyDeviceToHost));
                for (size_t i = 0; i < rows; i++) out[(size_t)c * rows + i] = (double)col[i];
            }
            return BA_OK;
        }
        case 17: { // diagnostic: the T factors of the LAST panel factored (BA_QR_TAU_LEVELS level slots of q_tau_stride scalars)
            if (!dense_qr() || n != (size_t)BA_QR_TAU_LEVELS * q_tau_stride || !d_qtau.p) return BA_ERR_ARG;
            std::vector<T> hh;
            int rcg;
            if ((rcg = dl(d_qtau.p, n, hh))) return rcg;
            for (size_t c = 0; c < n; c++) out[c] = (double)hh[c];
            return BA_OK;
        }
        case 12: { // diagnostic: the first D rows of the factored matrix, all D + 1 columns (R | the head of Q^T rhs), column-major D x (D + 1)
            if (!dense_qr() || n != (size_t)D * (D + 1) || !d_qA.p) return BA_ERR_ARG;
            HIPCHK(hipStreamSynchronize(st));
            std::vector<T> col((size_t)D);
            for (int c = 0; c <= D; c++) {
                HIPCHK(hipMemcpy(col.data(), d_qA.p + (size_t)c * q_lda, sizeof(T) * (size_t)D, hipMemcpyDeviceToHost));
                for (int i = 0; i < D; i++) out[(size_t)c * D + i] = (c < D && i > c) ? 0.0 : (double)col[i];
            }
            return BA_OK;
        }
        case BA_GET_CAMS:
        case BA_GET_CAMS_TEST: {
            if (n != 15 * (size_t)N) return BA_ERR_ARG;
            if ((rc = dl(d_cam[what == BA_GET_CAMS ? 0 : 1].p, 15 * (size_t)N, h))) return rc;
            soa_to_aos(h, N, 15, out);
            return BA_OK;
        }
        case BA_GET_POINTS:
        case BA_GET_POINTS_TEST: {
            if (n != 3 * (size_t)Ml) return BA_ERR_ARG;
            if ((rc = dl(d_pts[what == BA_GET_POINTS ? 0 : 1].p, 3 * (size_t)Ml, h))) return rc;
            soa_to_aos(h, Ml, 3, out);
            return BA_OK;
        }
        }
        return BA_ERR_ARG;
    }

    int set_state(const double *cam15, const double *pts) override
    {
        const std::vector<T> h = cam15 ? aos_to_soa(cam15, N, 15) : std::vector<T>();
        if (cam15 && share_on() && !share_equal(sh.h_gptr, sh.h_members, h.data(), N)) return BA_ERR_ARG; // (state unchanged)
        HIPCHK(hipStreamSynchronize(st));
        vf.lin_dropped();
        if (cam15) HIPCHK(hipMemcpy(d_cam[0].p, h.data(), sizeof(T) * h.size(), hipMemcpyHostToDevice));
        if (pts && Ml > 0) {
            const std::vector<T> hp = aos_to_soa(pts, Ml, 3);
            HIPCHK(hipMemcpy(d_pts[0].p, hp.data(), sizeof(T) * hp.size(), hipMemcpyHostToDevice));
        }
        vf.step_dropped();
        return BA_OK;
    }

    // ---- the LM loop: BacktrackLevMarqQRChol.h:204-436 == BacktrackLevMarqCholesky.h:190-361 (Scalar arithmetic in T) ------------
    // The first outer iteration is linearised host-synchronously (lambda0 needs max diag J'J); from then on the host only ENQUEUES:
    // every trial is the captured segments + k_lm_control, which decides accept / rho / lambda / flat-line on the device and gates
    // x = xTest and the next linearisation.  The host keeps at most LM_DEPTH trials in the stream, watches the progress counter
    // the control kernel bumps in pinned memory, and prints / forwards the table rows as they appear there.
    static constexpr int LM_DEPTH = 3;

    int capture(hipGraphExec_t *g, int (Solver::*seg)())
    {
        if (*g) return BA_OK;
        hipGraph_t gr = nullptr;
        HIPCHK(hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
        const int rc = (this->*seg)();
        const hipError_t e = hipStreamEndCapture(st, &gr); // (also on the error path: never leave the stream capturing)
        if (rc) { if (gr) (void)hipGraphDestroy(gr); return rc; }
        if (e != hipSuccess) { fprintf(stderr, "ba_mi355x: hipStreamEndCapture: %s\n", hipGetErrorString(e)); return BA_ERR_HIP; }
        const hipError_t ei = hipGraphInstantiate(g, gr, nullptr, nullptr, 0);
        (void)hipGraphDestroy(gr);
        if (ei != hipSuccess) { *g = nullptr; return BA_ERR_HIP; }
        return BA_OK;
    }
    int launch_seg_ab() { int rc = launch_seg_a(); return rc ? rc : launch_seg_b(); }
    int launch_seg_iter() { int rc = launch_seg_ab(); return rc ? rc : launch_seg_ctl(); }

    // one segment: replay its graph, or (legacy stream, BA_NO_GRAPH, sharding through a host callback) launch it directly
    int run_seg(hipGraphExec_t *g, int (Solver::*seg)(), bool graphs)
    {
        if (!graphs) return (this->*seg)();
        int rc = capture(g, seg);
        if (rc) return rc;
        HIPCHK(hipGraphLaunch(*g, st));
        return BA_OK;
    }

    // head = false: the trial in front of this one has run in this stream since the last host-side change, and its tail has left this
    // trial's records and pair blocks (tail_prepares())
    int enqueue_trial(int slot, bool graphs, bool head)
    {
        int rc;
        EvSlot &e = ring[slot];
        if (spin_next_s > 0) { // self-test (3): a launch that outlasts the watchdog (it ends by itself)
            hipLaunchKernelGGL(k_spin, dim3(1), dim3(64), 0, st, (long long)(spin_next_s * wall_khz * 1e3));
            spin_next_s = 0;
        }
        if (!sharded()) // ONE graph per LM iteration and no event between the launches: the times come from the device's wall clock
        {
            seg_head = head || !tail_prepares();
            rc = run_seg(seg_head ? &g_trial : &g_trial_nh, &Solver::launch_seg_iter, graphs);
            seg_head = true; // (try_step and everything else that launches the segments itself)
            return rc;
        }
        HIPCHK(hipEventRecord(e.e[0], st));
        {
            if ((rc = run_seg(&g_a, &Solver::launch_seg_a, graphs))) return rc;
            HIPCHK(hipEventRecord(e.e[1], st));
            if ((rc = exchange())) return rc;
            HIPCHK(hipEventRecord(e.e[2], st));
            if ((rc = run_seg(&g_b, &Solver::launch_seg_b, graphs && !dist_on()))) return rc; // (the distributed factor's collectives sit INSIDE segment B)
            HIPCHK(hipEventRecord(e.e[3], st));
            // test energy, rho denominator, |dx|^2 (point parts) + the guard slot and the error word
            if ((rc = allreduce(d_scal.p + SC_ETEST, N_STEP_SCALARS, 0))) return rc;
        }
        HIPCHK(hipEventRecord(e.e[4], st));
        if ((rc = run_seg(&g_ctl, &Solver::launch_seg_ctl, graphs))) return rc;
        if (more_qr() && (rc = more_outer_finish(&d_lm.p->go))) return rc; // MOREQR's outer R22: the shards' R factors meet in one more all-reduce
        HIPCHK(hipEventRecord(e.e[5], st));
        return BA_OK;
    }

    void harvest(int slot, bool accepted)
    {
        EvSlot &e = ring[slot];
        tm.trial_ms += ev_ms(e.e[0], e.e[4]);
        if (sharded()) tm.comm_ms += ev_ms(e.e[1], e.e[2]) + ev_ms(e.e[3], e.e[4]);
        tm.n_trials++;
        tm.n_graph_trials++;
        if (accepted) { tm.linearize_ms += ev_ms(e.e[4], e.e[5]); tm.n_linearize++; }
    }

    int minimize(const ba_lm_params *lmp, ba_trial_cb cb, void *user, ba_result *out) override
    {
        if (poisoned) return BA_ERR_HIP;
        ba_lm_params lm;
        if (lmp) lm = *lmp; else ba_lm_params_default(&lm);
        const auto tbeg = std::chrono::steady_clock::now();
        const ba_timing tm0 = tm;
        const bool talk = lm.verbose && rank == 0;
        if (talk) {
            // outputHeader / outputIterHeader, BacktrackLevMarqQRChol.h:65-82
            printf("############################## Backtrack LevMarq ###############################\n");
            printf("--------------------------------------------------------------------------------\n");
            printf(" Iter%15s%15s%15s%15s%15s\n", "Status", "f", "rho", "lambda", "Elapsed");
            printf("--------------------------------------------------------------------------------\n");
        }
        int rc = BA_OK;
        ba_lm_dev<T> h{};
        h.lam_min = (T)lm.lambda_min; h.lam_max = (T)lm.lambda_max; h.tol_fun = (T)lm.tol_fun; h.inc_base = (T)lm.lambda_increase_base;
        h.lambda = (T)lm.lambda_init; h.lambda_inc = h.inc_base;
        h.max_iter = lm.max_iter; h.max_fun_ev = lm.max_fun_ev; h.max_trials = lm.max_trials;
        h.status = BA_RUNNING;
        h.iter = 1;
        int launched = 0, consumed = 0, harvested = 0;
        std::vector<char> acc_of(RING_EV, 0);
        if (h.iter > lm.max_iter) { h.status = BA_MAX_ITERS; h.stop = 1; }
        else if (lm.max_trials < 0) { h.stop = 1; }
        else {
            // outer iteration 1: m_functor(x, r), df, JtRes, column norms; lambda0 = 1e-12 max diag J'J (:257-280; Cholesky.h:263-265);
            // MOREQR: 1e-6 * max column norm (BacktrackLevMarqMore.h:272-284)
            // Marquardt's damping: lambda is dimensionless, lambda0 = lambda_init, and the diagonal's maximum is not asked for
            double e = 0, dmax = 0;
            if ((rc = linearize(&e, damp_kind == BA_DAMP_MARQUARDT ? nullptr : &dmax))) return rc;
            h.energy = (T)e;
            h.fun_evals = 1;
            if (damp_kind != BA_DAMP_MARQUARDT) h.lambda = kind == BA_MOREQR ? (T)(1e-6 * std::sqrt(dmax)) : (T)(1e-12 * dmax);
        }
        if (!h.stop && dist_on() && (rc = dist_setup())) return rc; // (never inside a stream capture)
        if (!h.stop && sharded() && !dense_qr() && !d_pack.p && (rc = d_pack.alloc(pack_count() + 1))) return rc;
        if (!h.stop && sharded() && dense_qr() && !d_qB.p && (rc = d_qB.alloc(qb_count()))) return rc;
        if (!h.stop) {
            h_log->done = 0; h_log->stop = 0; h_log->status = BA_RUNNING;
            if ((rc = set_lambda(h.lambda))) return rc;
            static_assert(SC_ERR == SC_GUARD + 1, "cleared together");
            HIPCHK(hipMemsetAsync(d_scal.p + SC_GUARD, 0, 2 * sizeof(T), st)); // the guard slot of trial 0 (no decision yet), no error
            HIPCHK(hipMemcpyAsync(d_lm.p, &h, sizeof h, hipMemcpyHostToDevice, st));
            HIPCHK(hipStreamSynchronize(st)); // (h is on the stack)
            // graphs unless the stream cannot be captured (legacy stream) or a host callback sits between the segments anyway
            const bool graphs = use_graph && st != nullptr; // (the distributed factor keeps segments A and C as graphs; B holds its collectives)
            auto tlast = std::chrono::steady_clock::now();
            auto drain = [&]() { // table rows that have appeared since the last look
                const int done = __atomic_load_n(&h_log->done, __ATOMIC_ACQUIRE);
                while (consumed < done) {
                    const ba_lm_row r = h_log->rows[consumed % BA_LM_RING];
                    const auto tnow = std::chrono::steady_clock::now();
                    const double el = std::chrono::duration<double>(tnow - tlast).count();
                    tlast = tnow;
                    acc_of[consumed % RING_EV] = r.accepted != 0;
                    consumed++;
                    if (r.stop == 2.0) continue; // ended by a device error: not a row of the table (the trial is repeated or the run fails)
                    if (!sharded()) { // device wall-clock stamps (k_lm_control): no events sit between the launches of an iteration
                        tm.n_graph_trials++;
                        if (r.trial_ticks >= 0) { tm.trial_ms += r.trial_ticks / wall_khz; tm.n_trials++; } // (not the first: host time sits in front of it)
                        if (r.ctl_ticks_prev >= 0 && r.prev_go != 0) { tm.linearize_ms += r.ctl_ticks_prev / wall_khz; tm.n_linearize++; }
                    }
                    if (cb) cb(user, (int)r.iter, (int)r.accepted, r.f, r.rho, r.lambda, el);
                    if (talk) // outputIter, BacktrackLevMarqQRChol.h:84-93 (f is the energy BEFORE the step)
                        printf("%5d%15s%15g%15g%15g%14gs\n", (int)r.iter, r.accepted != 0 ? "Accepted" : "Rejected", r.f, r.rho, r.lambda, el);
                }
                while (harvested + 1 < consumed) { if (sharded()) harvest(harvested % RING_EV, acc_of[harvested % RING_EV]); harvested++; } // (its events are complete)
                return done;
            };
            for (int attempt = 0;; attempt++) {
                // How many trials are enqueued depends on DEVICE DATA ONLY: trial n goes into the stream iff n < LM_DEPTH or row
                // n - LM_DEPTH has arrived with its stop mark clear (and n < max_trials).  The row that ends the run is row s on
                // every shard (same control kernel, same all-reduced scalars), so every rank enqueues exactly s + LM_DEPTH trials
                // and with them the same number of collectives -- whatever its host's timing.  (Looking at a global "stopped"
                // word instead made that number depend on WHEN a host looked: a rank one trial ahead then sat in ncclAllReduce
                // for ever.)  Trials behind row s run as no-ops (k_lm_control returns at once, nothing is accepted).
                auto tprog = std::chrono::steady_clock::now(); // last time the device made progress (a trial finished)
                bool head = true; // the first trial behind the host's linearisation, or the repeat behind a device error: nobody has prepared it
                int seen = consumed;
                while (true) {
                    const int done = drain();
                    if (done != seen) { seen = done; tprog = std::chrono::steady_clock::now(); }
                    bool may = !(lm.max_trials > 0 && launched >= lm.max_trials), final = !may;
                    if (may && launched >= LM_DEPTH) {
                        const int need = launched - LM_DEPTH;
                        if (done <= need) may = false;                                                       // (not there yet)
                        else if (h_log->rows[need % BA_LM_RING].stop != 0.0) { may = false; final = true; }   // the run ended at row `need`
                    }
                    if (may) {
                        if ((rc = enqueue_trial(launched % RING_EV, graphs, head))) break;
                        head = false;
                        launched++;
                        continue;
                    }
                    if (final) break; // nothing more will ever be enqueued: wait for what is in the stream
                    // LM_DEPTH trials are in the stream: wait for a row (a trial is 0.1 ... 20 ms; watchdog_s without one = a hung launch)
                    if (std::chrono::duration<double>(std::chrono::steady_clock::now() - tprog).count() > watchdog_s) {
                        // Nothing can be waited for and nothing freed: the stream holds the launch that never ends (a synchronise or
                        // a hipFree would block for ever).  The handle is dead from here on; a retry belongs in a fresh process.
                        fprintf(stderr, "ba_mi355x: no LM trial completed within %g s -- giving up on this solver (nothing is freed)\n", watchdog_s);
                        poisoned = true;
                        return BA_ERR_HIP;
                    }
                    __builtin_ia32_pause();
                }
                if (!rc) { // wait for the stream with the same watchdog (a trial enqueued behind the last row may be the one that hangs)
                    const auto tw = std::chrono::steady_clock::now();
                    hipError_t eq;
                    while ((eq = hipStreamQuery(st)) == hipErrorNotReady) {
                        (void)drain(); // rows still arrive (up to LM_DEPTH of them): deliver each when it lands, with its own elapsed time
                        if (std::chrono::duration<double>(std::chrono::steady_clock::now() - tw).count() > watchdog_s) {
                            fprintf(stderr, "ba_mi355x: the stream did not drain within %g s -- giving up on this solver (nothing is freed)\n", watchdog_s);
                            poisoned = true;
                            return BA_ERR_HIP;
                        }
                        __builtin_ia32_pause();
                    }
                    if (eq != hipSuccess) { fprintf(stderr, "ba_mi355x: %s\n", hipGetErrorString(eq)); return BA_ERR_HIP; }
                } else {
                    const hipError_t es = hipStreamSynchronize(st);
                    if (es != hipSuccess) { fprintf(stderr, "ba_mi355x: %s\n", hipGetErrorString(es)); return BA_ERR_HIP; }
                }
                drain();
                while (harvested < consumed) { if (sharded()) harvest(harvested % RING_EV, acc_of[harvested % RING_EV]); harvested++; }
                if (rc) return rc;
                HIPCHK(hipMemcpy(&h, d_lm.p, sizeof h, hipMemcpyDeviceToHost));
                if (h.status != BA_DEV_FAILED) break;
                report_device_error(h.deverr);
                if (h.deverr == BA_DEVERR_DIVERGED) return BA_ERR_COMM;
                if (safe_factor || attempt > 0) return BA_ERR_HIP; // (the launch-per-step path has no hand-offs: cannot happen)
                // ---- a hand-off inside a fused launch timed out (a row workgroup not resident in time: a GPU shared with another
                // process, say).  x, lambda and the linearisation are untouched (nothing was accepted); repeat the trial -- and run
                // the rest -- with one launch per step.  Sharded: the error word rode on the scalar all-reduce, every rank is here.
                fprintf(stderr, "ba_mi355x: repeating LM trial %d with the launch-per-step factorisation\n", h.trials - 1);
                safe_factor = true;
                recoveries++;
                for (hipGraphExec_t *g : {&g_trial, &g_trial_nh, &g_b})
                    if (*g) { (void)hipGraphExecDestroy(*g); *g = nullptr; }
                h.trials -= 1; h.fun_evals -= 1; // the failed trial's row does not count
                h.status = BA_RUNNING; h.stop = 0; h.deverr = 0; h.go = 0; h.timed = 0; h.prev_go = 0;
                // (h.prev_code: k_lm_control overwrote it with the FAILED trial's code -- rejected + stop = 2 -- on every shard alike; the
                // guard slot gets that same value back, so the repeated trial's check "sum == world x mine" holds on both sides)
                {
                    const T code = (T)h.prev_code;
                    *h_lam = code; // (pinned staging word; lambda itself lives on the device)
                    HIPCHK(hipMemcpyAsync(d_scal.p + SC_GUARD, h_lam, sizeof(T), hipMemcpyHostToDevice, st));
                    // (the trials that were in the stream behind the failed one ran the same fused launches and raised the word again)
                    HIPCHK(hipMemsetAsync(d_scal.p + SC_ERR, 0, sizeof(T), st));
                }
                HIPCHK(hipMemcpyAsync(d_lm.p, &h, sizeof h, hipMemcpyHostToDevice, st));
                HIPCHK(hipStreamSynchronize(st));
                launched = consumed = harvested = h.trials;
                if (lm.max_trials > 0) { /* rows already delivered count: the device compares s.trials with max_trials itself */ }
                __atomic_store_n(&h_log->done, h.trials, __ATOMIC_RELEASE);
                h_log->stop = 0; h_log->status = BA_RUNNING;
            }
            if (h.fresh) { // stopped (max_trials) right behind an accepted step: the energy of the linearisation that followed it
                if ((rc = fetch_scalars())) return rc;
                if (sharded()) { // (only this shard's part is there until a trial carries it through the all-reduce)
                    HIPCHK(hipMemcpyAsync(d_scal.p + SC_ENERGY, d_scal.p + SC_ELOC, sizeof(T), hipMemcpyDeviceToDevice, st));
                    if ((rc = allreduce(d_scal.p + SC_ENERGY, 1, 0)) || (rc = fetch_scalars())) return rc;
                }
                h.energy = h_scal[SC_ENERGY];
            }
            HIPCHK(hipGetLastError());
        }
        if (talk) printf("--------------------------------------------------------------------------------\n");
        vf.x_moved(); // (ba_solver_covariance_compute wants a ba_solver_linearize at the final x first)
        if (out) {
            out->status = h.status; out->iterations = h.iter; out->trials = h.trials; out->fun_evals = h.fun_evals;
            out->energy = (double)h.energy; out->lambda = (double)h.lambda;
            out->seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - tbeg).count();
            const long long nt = tm.n_trials - tm0.n_trials, nl = tm.n_linearize - tm0.n_linearize; // (the timed ones)
            out->schur_ms = nt ? (tm.trial_ms - tm0.trial_ms) / nt : 0.0; // whole trial incl. the test-energy evaluation and the all-reduces
            out->linearize_ms = nl ? (tm.linearize_ms - tm0.linearize_ms) / nl : 0.0;
        }
        return rc;
    }

    // which = 1: the backward sweep with the group at the head of its chain missing (and a short spin bound): the groups behind
    // it wait for unknowns that are never published -- the production path's reaction to that must be BA_ERR_HIP.
    int selftest(int which) override
    {
        if (iterative() && which != 3) return BA_ERR_ARG; // (no dense factorisation, no back sweep)
        if (which == 2) { // arm: the fused factorisation's row workgroups stay silent and the panel's wait is short -- the next
                          // ba_minimize meets BA_DEVERR_ROW_FLAG on its first trial and must recover through the launch-per-step path
            if ((D + NB - 1) / NB < 2 || safe_factor) return BA_ERR_ARG; // (a single block column has no fused step)
            fault_rowflag = 1;
            for (hipGraphExec_t *g : {&g_trial, &g_trial_nh, &g_b})
                if (*g) { (void)hipGraphExecDestroy(*g); *g = nullptr; }
            return BA_OK;
        }
        if (which == 3) { // arm: a 4-second kernel in front of the next trial -- with BA_WATCHDOG_S below that, ba_minimize must give up
            spin_next_s = 4.0;
            return BA_OK;
        }
        if (which != 1) return BA_ERR_ARG;
        const int nblk = (D + NB - 1) / NB, groups = (nblk + 1) / 2;
        if (groups < 2 || 2 * groups > num_cus) return BA_ERR_ARG;
        hipLaunchKernelGGL((k_fill_sentinel<T>), dim3((2 * Dp + 2 * NB + 255) / 256), dim3(256), 0, st, 2 * Dp + 2 * NB, d_dxc.p);
        hipLaunchKernelGGL((k_ldlt_backflow<T, NB>), dim3(2 * groups), dim3(256), 0, st, D, ld, D, nblk, d_S.p, d_Winv.p, d_dxc.p, d_dxc.p + Dp,
                           d_scal.p + SC_ERR, 1 << 10, groups - 1);
        vf.step_dropped();
        return fetch_scalars();
    }

    int time_phase(int phase, int reps, double lambda_d, double *ms) override
    {
        if (reps < 1 || !ms) return BA_ERR_ARG;
        if (iterative() && (phase == 3 || phase == 6 || phase == 7)) return BA_ERR_ARG; // (no S)
        if ((phase == 9 || phase == 10) && !(iterative() && forest_on() && (phase == 10 || fo.width == 9))) return BA_ERR_ARG;
        if (phase == 11 && !(dogleg_ok() && dg.part.p)) return BA_ERR_ARG; // (k_jg writes the dogleg's partial list: a prepare comes first)
        double acc_ms = 0;
        int rcl = set_lambda((T)lambda_d);
        if (rcl) return rcl;
        HIPCHK(hipStreamSynchronize(st));
        HIPCHK(hipEventRecord(ev[EV_T0], st));
        for (int k = 0; k < reps; k++) {
            switch (phase) {
            case 0: launch_eval(false, 0); break;
            case 1: launch_linearisation(0, nullptr, false, false, nullptr, true); break;
            case 2: launch_eliminate(); break;
            case 3: launch_assemble(); break; // (QRKIT: J2bot instead of S)
            case 4:
                if (iterative()) { launch_pcg_prep(); launch_pcg_solve(); break; }
                launch_assemble(); // the factorisation is in place: rebuild S first (timed separately by phase 3)
                if (dense_qr()) launch_qrkit_solve();
                else { launch_post_reduce(); launch_factor_solve(); }
                break;
            case 5: launch_backsub_retract(); break;
            case 8: // the linearisation as ba_minimize runs it behind an accepted step: fused point part (+ CHOLESKY: the next trial's records)
                launch_linearisation(0, nullptr, false, /*fused*/ true, nullptr, /*points*/ !fuse);
                break;
            case 9: launch_forest_edges(); break;
            case 11: launch_jg(); break; // q = |J g|^2 of the dogleg's prepare: the block partials alone (the same values every time)
            case 10: // the forest's factor alone: events around it, per rep (it needs B_a, which the trial inverts in place)
                launch_pcg_blocks();
                if (fo.width == 9) launch_forest_edges();
                HIPCHK(hipEventRecord(ev[EV_T2], st));
                launch_forest_factor();
                HIPCHK(hipEventRecord(ev[EV_T3], st));
                HIPCHK(hipStreamSynchronize(st));
                acc_ms += ev_ms(EV_T2, EV_T3);
                break;
            case 6: // dense factorisation only (k_ldlt_panel + k_ldlt_step / k_ldlt_update; QRKIT: the Householder QR + solve): events around it, per rep
            case 7: // backward sweep only (k_ldlt_backflow; QRKIT: nothing, the solve is part of 6)
                launch_assemble();
                if (dense_qr()) {
                    HIPCHK(hipEventRecord(ev[EV_T2], st));
                    if (phase == 6) launch_qrkit_solve();
                    HIPCHK(hipEventRecord(ev[EV_T3], st));
                    HIPCHK(hipStreamSynchronize(st));
                    acc_ms += ev_ms(EV_T2, EV_T3);
                    break;
                }
                launch_post_reduce();
                if (phase == 6) HIPCHK(hipEventRecord(ev[EV_T2], st));
                launch_factor();
                if (phase == 6) HIPCHK(hipEventRecord(ev[EV_T3], st));
                if (phase == 7) HIPCHK(hipEventRecord(ev[EV_T2], st));
                launch_backsweep();
                if (phase == 7) HIPCHK(hipEventRecord(ev[EV_T3], st));
                HIPCHK(hipStreamSynchronize(st));
                acc_ms += ev_ms(EV_T2, EV_T3);
                break;
            default: return BA_ERR_ARG;
            }
        }
        HIPCHK(hipEventRecord(ev[EV_T1], st));
        HIPCHK(hipStreamSynchronize(st));
        HIPCHK(hipGetLastError());
        *ms = ((phase == 6 || phase == 7 || phase == 10) ? acc_ms : ev_ms(EV_T0, EV_T1)) / reps;
        vf.step_dropped();
        return BA_OK;
    }
};

} // namespace

struct ba_solver {
    SolverBase *impl = nullptr;
};

extern "C" {

int ba_device_info(int device, char *name, size_t n, int *cus)
{
    int cnt = 0;
    if (hipGetDeviceCount(&cnt) != hipSuccess || cnt <= 0) return BA_ERR_HIP;
    if (device < 0) { if (hipGetDevice(&device) != hipSuccess) return BA_ERR_HIP; }
    if (device >= cnt) return BA_ERR_ARG;
    hipDeviceProp_t pr;
    if (hipGetDeviceProperties(&pr, device) != hipSuccess) return BA_ERR_HIP;
    if (name && n) { snprintf(name, n, "%s (%s)", pr.name, pr.gcnArchName); }
    if (cus) *cus = pr.multiProcessorCount;
    return BA_OK;
}

int ba_solver_create(const ba_problem *p, ba_solver_kind kind, ba_scalar scalar, int device, int shard_rank, int shard_world,
                     ba_solver **out)
{
    if (!p || !out || shard_world < 1 || shard_rank < 0 || shard_rank >= shard_world) return BA_ERR_ARG;
    if (kind != BA_QRKIT && kind != BA_QRCHOL && kind != BA_CHOLESKY && kind != BA_MOREQR && kind != BA_QRSPQR && kind != BA_ITERSCHUR) return BA_ERR_ARG;
    if (kind == BA_ITERSCHUR && shard_world > 1) return BA_ERR_ARG; // single shard (ba_mi355x.h)
    if (scalar != BA_F64 && scalar != BA_F32) return BA_ERR_ARG;
    *out = nullptr;
    int cnt = 0;
    if (hipGetDeviceCount(&cnt) != hipSuccess || cnt <= 0) {
        fprintf(stderr, "ba_mi355x: no HIP device -- the solver has no CPU path\n");
        return BA_ERR_HIP;
    }
    if (device >= 0) {
        if (device >= cnt) return BA_ERR_ARG;
        HIPCHK(hipSetDevice(device));
    }
    SolverBase *impl = (scalar == BA_F64) ? (SolverBase *)new (std::nothrow) Solver<double>() : (SolverBase *)new (std::nothrow) Solver<float>();
    if (!impl) return BA_ERR_NOMEM;
    int rc = impl->init(p, kind, shard_rank, shard_world);
    if (rc) { delete impl; return rc; }
    ba_solver *s = new (std::nothrow) ba_solver;
    if (!s) { delete impl; return BA_ERR_NOMEM; }
    s->impl = impl;
    *out = s;
    return BA_OK;
}

void ba_solver_free(ba_solver *s)
{
    if (!s) return;
    // a solver the watchdog gave up on still has a launch in its stream that may never end: every HIP call that frees or
    // synchronises could block with it -- its device memory is left to the end of the process
    if (!s->impl->poisoned) delete s->impl;
    delete s;
}

int ba_solver_recoveries(const ba_solver *s) { return s ? s->impl->recoveries : -1; }

int ba_solver_set_allreduce(ba_solver *s, ba_allreduce_fn fn, void *user)
{
    if (!s) return BA_ERR_ARG;
    s->impl->ar_fn = fn; s->impl->ar_user = user;
    return BA_OK;
}

int ba_solver_comm_init(ba_solver *s, const void *id)
{
    if (!s || !id) return BA_ERR_ARG;
    if (s->impl->comm) return BA_ERR_ARG;
    return ba_rccl_init(&s->impl->comm, id, s->impl->rank, s->impl->world);
}

int ba_solver_set_stream(ba_solver *s, void *hip_stream)
{
    if (!s) return BA_ERR_ARG;
    if (s->impl->poisoned) return BA_ERR_HIP;
    if (s->impl->own_stream && s->impl->st) { (void)hipStreamSynchronize(s->impl->st); (void)hipStreamDestroy(s->impl->st); }
    s->impl->st = (hipStream_t)hip_stream;
    s->impl->own_stream = false;
    return BA_OK;
}

int ba_solver_keep_intermediates(ba_solver *s, int on)
{
    if (!s) return BA_ERR_ARG;
    s->impl->keep = on != 0;
    return BA_OK;
}

int ba_solver_shard(const ba_solver *s, int *p0, int *p1, int *o0, int *o1)
{
    if (!s) return BA_ERR_ARG;
    if (p0) *p0 = s->impl->sx.p0;
    if (p1) *p1 = s->impl->sx.p1;
    if (o0) *o0 = s->impl->sx.o0;
    if (o1) *o1 = s->impl->sx.o1;
    return BA_OK;
}

int ba_minimize(ba_solver *s, const ba_lm_params *lm, ba_trial_cb cb, void *user, ba_result *out)
{
    return s ? s->impl->minimize(lm, cb, user, out) : BA_ERR_ARG;
}
#define BA_LIVE(s) ((s) && !(s)->impl->poisoned)
int ba_solver_linearize(ba_solver *s, double *energy, double *diag_max) { return !s ? BA_ERR_ARG : !BA_LIVE(s) ? BA_ERR_HIP : s->impl->linearize(energy, diag_max); }
int ba_solver_try_step(ba_solver *s, double lambda, double *energy_test, double *rho_scale, double *dx_norm)
{
    return !s ? BA_ERR_ARG : !BA_LIVE(s) ? BA_ERR_HIP : s->impl->try_step(lambda, energy_test, rho_scale, dx_norm);
}
int ba_solver_accept(ba_solver *s) { return !s ? BA_ERR_ARG : !BA_LIVE(s) ? BA_ERR_HIP : s->impl->accept(); }
int ba_solver_dogleg_prepare(ba_solver *s, double mu, ba_dogleg_info *out) { return !s ? BA_ERR_ARG : !BA_LIVE(s) ? BA_ERR_HIP : s->impl->dogleg_prepare(mu, out); }
int ba_solver_try_dogleg(ba_solver *s, double radius, double *energy_test, double *pred, double *dx_norm, int *branch)
{
    return !s ? BA_ERR_ARG : !BA_LIVE(s) ? BA_ERR_HIP : s->impl->try_dogleg(radius, energy_test, pred, dx_norm, branch);
}
int ba_minimize_dogleg(ba_solver *s, const ba_dogleg_params *p, ba_trial_cb cb, void *user, ba_result *out)
{
    return !s ? BA_ERR_ARG : !BA_LIVE(s) ? BA_ERR_HIP : s->impl->minimize_dogleg(p, cb, user, out);
}
int ba_solver_triangulate_points(ba_solver *s, const ba_triangulate_params *p, int n_pts, const int *pt_ids, unsigned char *status,
                                 ba_triangulate_stats *stats)
{
    return !s ? BA_ERR_ARG : !BA_LIVE(s) ? BA_ERR_HIP : s->impl->triangulate(p, n_pts, pt_ids, status, stats);
}
int ba_solver_stats(ba_solver *s, double *out4) { return !(s && out4) ? BA_ERR_ARG : !BA_LIVE(s) ? BA_ERR_HIP : s->impl->stats(out4); }
int ba_solver_get(ba_solver *s, int what, double *out, size_t n) { return !(s && out) ? BA_ERR_ARG : !BA_LIVE(s) ? BA_ERR_HIP : s->impl->get(what, out, n); }
int ba_solver_set_state(ba_solver *s, const double *cam15, const double *pts) { return !s ? BA_ERR_ARG : !BA_LIVE(s) ? BA_ERR_HIP : s->impl->set_state(cam15, pts); }

int ba_solver_timing(ba_solver *s, ba_timing *out, int reset)
{
    if (!s) return BA_ERR_ARG;
    if (out) *out = s->impl->tm;
    if (reset) s->impl->tm = ba_timing{};
    return BA_OK;
}

int ba_solver_time_phase(ba_solver *s, int phase, int reps, double lambda, double *ms_per_launch)
{
    return !s ? BA_ERR_ARG : !BA_LIVE(s) ? BA_ERR_HIP : s->impl->time_phase(phase, reps, lambda, ms_per_launch);
}

int ba_solver_selftest(ba_solver *s, int which) { return !s ? BA_ERR_ARG : !BA_LIVE(s) ? BA_ERR_HIP : s->impl->selftest(which); }

int ba_solver_set_pcg(ba_solver *s, int max_iter, double rel_tol) { return !s ? BA_ERR_ARG : !BA_LIVE(s) ? BA_ERR_HIP : s->impl->set_pcg(max_iter, rel_tol); }
int ba_solver_set_constant(ba_solver *s, const unsigned short *cam_mask, const unsigned char *pt_fixed)
{
    return !s ? BA_ERR_ARG : !BA_LIVE(s) ? BA_ERR_HIP : s->impl->set_constant(cam_mask, pt_fixed);
}
int ba_solver_set_loss(ba_solver *s, int kind, double scale) { return !s ? BA_ERR_ARG : !BA_LIVE(s) ? BA_ERR_HIP : s->impl->set_loss(kind, scale); }
int ba_solver_set_obs_weights(ba_solver *s, const double *w) { return !s ? BA_ERR_ARG : !BA_LIVE(s) ? BA_ERR_HIP : s->impl->set_obs_weights(w); }
int ba_solver_set_obs_active(ba_solver *s, const unsigned char *active) { return !s ? BA_ERR_ARG : !BA_LIVE(s) ? BA_ERR_HIP : s->impl->set_obs_active(active); }
int ba_solver_get_obs_active(ba_solver *s, unsigned char *active, long long *n_active)
{
    return !s ? BA_ERR_ARG : !BA_LIVE(s) ? BA_ERR_HIP : s->impl->get_obs_active(active, n_active);
}
int ba_solver_filter_observations(ba_solver *s, const ba_filter_params *p, int apply, unsigned char *obs_status, unsigned char *pt_status, double *err_px,
                                  ba_filter_stats *stats)
{
    return !s ? BA_ERR_ARG : !BA_LIVE(s) ? BA_ERR_HIP : s->impl->filter(p, apply, obs_status, pt_status, err_px, stats);
}
int ba_solver_set_point_priors(ba_solver *s, int n, const int *pt_ids, const double *x0, const double *sqrt_info)
{
    return !s ? BA_ERR_ARG : !BA_LIVE(s) ? BA_ERR_HIP : s->impl->set_priors(0, n, pt_ids, x0, sqrt_info);
}
int ba_solver_set_centre_priors(ba_solver *s, int n, const int *cam_ids, const double *c0, const double *sqrt_info)
{
    return !s ? BA_ERR_ARG : !BA_LIVE(s) ? BA_ERR_HIP : s->impl->set_priors(1, n, cam_ids, c0, sqrt_info);
}
int ba_solver_set_intrinsics_priors(ba_solver *s, int n, const int *cam_ids, const double *x0, const double *w)
{
    return !s ? BA_ERR_ARG : !BA_LIVE(s) ? BA_ERR_HIP : s->impl->set_priors(2, n, cam_ids, x0, w);
}
int ba_solver_prior_energy(ba_solver *s, double *out3) { return !(s && out3) ? BA_ERR_ARG : !BA_LIVE(s) ? BA_ERR_HIP : s->impl->prior_energy(out3); }
int ba_solver_set_relative_poses(ba_solver *s, int n, const int *cam_pairs, const double *R0, const double *t0, const double *sqrt_info_rot,
                                 const double *sqrt_info_trans)
{
    return !s ? BA_ERR_ARG : !BA_LIVE(s) ? BA_ERR_HIP : s->impl->set_relposes(n, cam_pairs, R0, t0, sqrt_info_rot, sqrt_info_trans);
}
int ba_solver_relative_pose_energy(ba_solver *s, double *out2) { return !(s && out2) ? BA_ERR_ARG : !BA_LIVE(s) ? BA_ERR_HIP : s->impl->relpose_energy(out2); }
int ba_solver_set_preconditioner(ba_solver *s, int kind, int max_tree) { return !s ? BA_ERR_ARG : !BA_LIVE(s) ? BA_ERR_HIP : s->impl->set_precond(kind, max_tree); }
int ba_solver_preconditioner_info(ba_solver *s, long long *out6, int *fallback_trees)
{
    return !s ? BA_ERR_ARG : !BA_LIVE(s) ? BA_ERR_HIP : s->impl->precond_info(out6, fallback_trees);
}
int ba_solver_set_shared_intrinsics(ba_solver *s, const int *group_of) { return !s ? BA_ERR_ARG : !BA_LIVE(s) ? BA_ERR_HIP : s->impl->set_shared(group_of); }
int ba_solver_shared_intrinsics_info(ba_solver *s, long long *out4) { return !s ? BA_ERR_ARG : !BA_LIVE(s) ? BA_ERR_HIP : s->impl->shared_info(out4); }
int ba_solver_set_damping(ba_solver *s, int kind, double diag_min, double diag_max)
{
    return !s ? BA_ERR_ARG : !BA_LIVE(s) ? BA_ERR_HIP : s->impl->set_damping(kind, diag_min, diag_max);
}
int ba_solver_get_damping(ba_solver *s, int *kind, double *diag_min, double *diag_max)
{
    return !s ? BA_ERR_ARG : !BA_LIVE(s) ? BA_ERR_HIP : s->impl->get_damping(kind, diag_min, diag_max);
}
int ba_solver_pcg_stats(ba_solver *s, ba_pcg_stats *out, int reset) { return !s ? BA_ERR_ARG : !BA_LIVE(s) ? BA_ERR_HIP : s->impl->pcg_stats(out, reset); }
int ba_solver_set_pcg_model_tol(ba_solver *s, double eta) { return !s ? BA_ERR_ARG : !BA_LIVE(s) ? BA_ERR_HIP : s->impl->set_pcg_model_tol(eta); }
int ba_solver_pcg_stop_stats(ba_solver *s, ba_pcg_stop_stats *out, int reset)
{
    return !s ? BA_ERR_ARG : !BA_LIVE(s) ? BA_ERR_HIP : s->impl->pcg_stop_stats(out, reset);
}
int ba_solver_device_bytes(const ba_solver *s, size_t *bytes)
{
    if (!s || !bytes) return BA_ERR_ARG;
    *bytes = s->impl->device_bytes();
    return BA_OK;
}
int ba_solver_covariance_compute(ba_solver *s, double lambda) { return !s ? BA_ERR_ARG : !BA_LIVE(s) ? BA_ERR_HIP : s->impl->cov_compute(lambda); }
int ba_solver_covariance_get(ba_solver *s, int n_pairs, const int *cam_pairs, double *cam_cov, int n_pts, const int *pt_ids, double *pt_cov)
{
    return !s ? BA_ERR_ARG : !BA_LIVE(s) ? BA_ERR_HIP : s->impl->cov_get(n_pairs, cam_pairs, cam_cov, n_pts, pt_ids, pt_cov);
}
int ba_solver_covariance_pcg(ba_solver *s, double lambda, int max_iter, double rel_tol, int n_pairs, const int *cam_pairs, double *cam_cov, int n_pts,
                             const int *pt_ids, double *pt_cov, ba_cov_pcg_stats *stats)
{
    return !s ? BA_ERR_ARG : !BA_LIVE(s) ? BA_ERR_HIP : s->impl->cov_pcg(lambda, max_iter, rel_tol, n_pairs, cam_pairs, cam_cov, n_pts, pt_ids, pt_cov, stats);
}
int ba_solver_covariance_timing(ba_solver *s, double *ms4) { return !(s && ms4) ? BA_ERR_ARG : s->impl->cov_timing(ms4); }

} // extern "C"
