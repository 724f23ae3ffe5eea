// ba_internal.h -- host-side types shared by the translation units of libba_mi355x.so (not part of the ABI), the plans of the
// solver's device lists and the constants those plans share with the kernels (the kernel headers include this file for them).
#ifndef BA_INTERNAL_H
#define BA_INTERNAL_H

#include "../../include/ba_mi355x.h"

#include <cstdint>
#include <vector>

// BAL problem as parsed (src/bundle_adjustment_large.cpp:59-107): observation order of the file.
struct ba_problem {
    int N = 0, M = 0, K = 0;
    std::vector<int> cam_idx, pt_idx;
    std::vector<double> meas;  // 2K interleaved (u,v)
    std::vector<double> cams9; // 9N: omega(3), T(3), f, k1, k2
    std::vector<double> pts;   // 3M
};

// Static structure of one shard, built once on the host (ba_structure.cpp) and copied to HBM.
//
// Observations are stably sorted by point (the reference's row-interleave of [J; sqrt(lambda) I] needs that order,
// src/Eigen_ext/BacktrackLevMarqQRChol.h:291-309); a shard owns a contiguous point range and its observations.
// The reduced camera matrix is assembled per camera pair (hi >= lo): every point seen by both cameras contributes
// one ENTRY (row observation, column observation); entries are grouped by pair and cut into CHUNKS of at most
// `chunk_len` entries so that the work is spread evenly over wavefronts and summed in a fixed order.
struct ba_structure {
    int N = 0;              // cameras (global)
    int M = 0, K = 0;       // global points / observations
    int p0 = 0, p1 = 0;     // owned point range
    int o0 = 0, o1 = 0;     // owned observation range (in sorted order)
    int Ml = 0, Kl = 0;     // local counts
    bool was_sorted = true; // input already sorted by point
    std::vector<int> perm;  // sorted position -> file position (size K, global)
    std::vector<int> obs_cam, obs_pt; // local (obs_pt is the LOCAL point index), size Kl
    std::vector<int> pt_ptr;          // Ml + 1
    int kmax = 0;                     // max observations per point in this shard
    // points bucketed by track length for the per-point QR (lanes per point x observations per lane):
    // <= 32 (8 x 4), <= 64 (16 x 4), <= 128 (32 x 4), <= 256 (64 x 4), <= 1024 (64 x 16)
    std::vector<int> qr_pts;          // Ml local point indices, bucket by bucket (file order inside a bucket)
    int qr_bucket_ptr[6] = {0, 0, 0, 0, 0, 0};
    // camera pairs
    int npairs = 0;                   // N (N + 1) / 2, pair id = hi (hi + 1) / 2 + lo
    std::vector<int> pair_hi, pair_lo;
    long long E = 0;                  // entries
    std::vector<int> ent_r, ent_c;    // row / column observation (local index) per entry, grouped by pair
    int chunk_len = 64;
    int nchunks = 0;
    std::vector<int> chunk_ptr;       // nchunks + 1 offsets into entries
    std::vector<int> chunk_pair;      // pair id per chunk
    std::vector<int> pair_chunk_ptr;  // npairs + 1 offsets into chunks
    // diagonal pairs only = observations of one camera (camera-sorted view), used for J_c^T J_c and g_c
    int ndchunks = 0;
    std::vector<int> dchunk_ptr;      // ndchunks + 1 offsets into cam_obs
    std::vector<int> dchunk_cam;      // camera per diagonal chunk
    std::vector<int> cam_dchunk_ptr;  // N + 1
    std::vector<int> cam_obs;         // Kl observations grouped by camera
};

// chunk_len: entries per chunk of a camera pair (one wavefront of k_schur_pairs); dchunk_len: observations per chunk of a camera (k_cam_gram)
// pairs = false (BA_ITERSCHUR, which never forms the reduced camera matrix): no camera pairs, entries or chunks (steps 3 and 4) --
// npairs, E and nchunks stay 0 -- and none of their limits; the camera-sorted view (step 5) is built as always.
int ba_build_structure(const ba_problem *p, int shard_rank, int shard_world, int chunk_len, int dchunk_len, ba_structure *out, bool pairs = true);

// The co-visibility list of ba_problem_covisibility (ba_mi355x.h states the rule) from point-sorted observations: pt_ptr[M + 1] into
// obs_cam.  pairs: 2n (a < b), weight: n, ordered by (weight descending, a, b).
int ba_covisibility(int N, int M, const int *pt_ptr, const int *obs_cam, int track_max, std::vector<int> &pairs, std::vector<int> &weight);

// ---- the plans of the solver's device lists (ba_structure.cpp): host vectors in, host vectors out, no HIP.  The solver asks the device
// and the environment, hands the answers in as plain numbers, uploads what comes back and launches; tests/plans_check.cpp checks the
// lists against the invariants the kernels rely on.  Device records come out as flat ints: 4 per chunk descriptor (int4), 2 per entry
// (int2), 5 per share slot (ba_share_chunk).

// constants a plan and a kernel share
#define BA_CHUNK 64               /* entries of one camera pair per chunk = per wavefront of the pair kernel */
#define BA_CHUNK_SINGLE (1 << 16) /* flag in chunk_info.y: the only chunk of its pair */
#define BA_SHARE_CHUNK 256        /* members per chunk at most (8 per lane) */
#define BA_SHARE_LOCAL 8          /* chunks of a group that k_pcg_share finishes itself at most: the chunk slots of a workgroup */

// k_eval's workgroups: point-aligned observation ranges of at most 256 (its threads), each as long as whole points allow (eb: ranges + 1
// boundaries).  None (eb empty) when a point has more observations than that or the shard has none.
void ba_plan_eval_ranges(const ba_structure &s, std::vector<int> &eb);

// The chunks dealt to the wavefronts of the persistent k_schur_pairs.  wgs_per_cu: the workgroup cap per CU behind the occupancy clamp;
// bands, window: BA_SCHUR_BANDS / BA_SCHUR_WINDOW or their defaults.
struct ba_schur_plan {
    int grid = 1, nband = 1;     // workgroups (4 wavefronts each), a multiple of nband
    std::vector<int> wave_ptr;   // 4 grid + 1: every wavefront's range of chunk descriptors
    std::vector<int> chunk_info; // [nchunks][4]: first entry, count | BA_CHUNK_SINGLE, cameras hi | lo << 16, chunk id
    std::vector<int> ent;        // [E][2]: row observation, column observation (~point for a self entry)
    std::vector<int> red_pairs;  // pairs k_schur_reduce writes: those without entries, with several chunks, and the diagonal ones
};
void ba_plan_schur(const ba_structure &s, int wgs_per_cu, int num_cus, int bands, int window, ba_schur_plan &out);

// The grid of k_pairs_gram: the pair workgroups of the plan first (they keep their block indices, and with them their bands), one
// workgroup per eight chunks of the camera-sorted view behind them.
struct ba_tail_grid { int pair_wgs, gram_wgs; };
inline ba_tail_grid ba_plan_tail_grid(int schur_grid, int ndchunks) { return ba_tail_grid{schur_grid, ndchunks > 0 ? (ndchunks + 7) / 8 : 0}; }

// The forest of ba_relpose_forest_plan over L = rp_pairs (BA_PRECOND_VISIBILITY_FOREST: then the co-visibility pairs) in elimination
// order, tree after tree.  kept == 0: no lists.  BA_ERR_NOMEM when a count leaves 32 bits.
struct ba_forest_plan {
    int ntrees = 0, nodes = 0, kept = 0, dropped = 0, largest = 0, width = 6; // width: of the cross blocks (9: visibility)
    std::vector<int> tree_ptr, node_cam, node_par /* position in the list, -1: root */;
    std::vector<int> node_rec;         // 2 constraint + side whose camera is the node; -1: a root or a co-visibility edge
    std::vector<unsigned char> in_tree; // [N]
    std::vector<int> edge_ptr, edge_oo; // visibility: per node the record pairs (o of the node, o' of its parent) of their common points
};
int ba_plan_forest(const ba_structure &s, const std::vector<int> &rp_pairs, int kind, int max_tree, ba_forest_plan &out);

// The chunks of ba_intrinsics_group_plan (gptr, cptr, cgrp) laid into the chunk slots of k_pcg_share, 8 to a workgroup.
struct ba_share_plan {
    int nslots = 0, nwide = 0, largest = 0; // largest: cameras of the largest group
    std::vector<int> desc; // [nslots][5]: m0, len, c0, nc, ng (ba_share_chunk); an empty slot is {0, 0, 0, 1, 1}
    std::vector<int> wide; // the slots of groups of more than BA_SHARE_LOCAL chunks
};
void ba_plan_share_slots(int ngroups, int nchunks, const int *gptr, const int *cptr, const int *cgrp, ba_share_plan &out);

// CSR of every camera's incident constraints: inc[ptr[a] .. ptr[a + 1]) holds 2 q (a is the first camera of q) / 2 q + 1 (the second)
void ba_plan_relpose_csr(int N, int n, const int *pairs, std::vector<int> &ptr, std::vector<int> &inc);

// Distributed factor: block column p (nb wide, Dp - nb p scalars high) belongs to rank p % world; off[p] = its offset in the
// owner-packed buffer of `world` chunks of equal length, in units of nb scalars.  Returns that length (scalars): the largest fill.
size_t ba_plan_owner_offsets(int Dp, int nb, int world, std::vector<int> &off);

// ba_solver_triangulate_points' and ba_triangulate_point's common refusals (ba_triangulate.cpp): BA_ERR_ARG for min_angle_deg outside
// [0, 180), max_reproj_px < 0, refine_iters < 0 or a value that is not finite
int ba_triangulate_params_check(const ba_triangulate_params *p);
// ba_solver_filter_observations' and ba_filter_track's common refusals (ba_filter.cpp): BA_ERR_ARG for max_reproj_px < 0, min_angle_deg
// outside [0, 180), either not finite, min_track < 0
int ba_filter_params_check(const ba_filter_params *p);

// RCCL transport (ba_comm.cpp); comm is an ncclComm_t
int ba_rccl_init(void **comm_out, const void *id128, int rank, int world);
void ba_rccl_destroy(void *comm);
int ba_rccl_allreduce(void *comm, void *buf, size_t count, int f64, int op, void *stream);
int ba_rccl_broadcast(void *comm, void *buf, size_t count, int f64, int root, void *stream);
int ba_rccl_reduce_scatter(void *comm, void *buf, size_t count_per_rank, int f64, int rank, void *stream);

#endif
