// ba_pcg_share.hip.h -- shared intrinsics for BA_ITERSCHUR (ba_solver_set_shared_intrinsics): the projector of the projected PCG.
//
// A group of cameras solves for one f, k1, k2.  With P (9N x n_free) the matrix that copies a group's three intrinsics to rows 6..8 of
// each member (identity elsewhere) the shared step is dx_c = P y, (P'SP) y = P' rhs, and with Pi = P (P'P)^-1 P' -- the orthogonal
// projector that replaces rows 6..8 of every member by the group's mean -- that is CG for Pi S on range(Pi), preconditioned by
// Pi M^-1, in the 9N layout the solver already has.  r, p and x stay in range(Pi) bit for bit, so the block
// partials of r'z and p'Sp formed from the unprojected z and y = S p are already the right scalars, and Pi is applied in three
// places only: to rhs and z_0 (launch_pcg_prep), to y = S p in front of k_pcg_update, to z behind it.  The damping of the shared
// parameter is lambda P'P = lambda n_g: Marquardt's damping of the stacked columns.
//
// The kernels here are that projection,  v[9 a + 6 + q] <- mean over the group of a,  q = 0..2, for every grouped camera; nothing else
// is written.  This file family's rules hold: no atomics, no workgroup waits for another, sums accumulate in fp64 for both scalar
// types, and the order of a group's sum depends on the group alone -- its members in ascending order cut into chunks of at most
// BA_SHARE_CHUNK (ba_intrinsics_group_plan) -- never on the grid or on the other groups of the launch:
//   chunk      a 32-lane group: lane l adds members l, l + 32, ... of the chunk in that order, then a butterfly over the 32 lanes
//              (every lane ends with the same bits)
//   group      of one chunk: the chunk's sum.  Of several: every chunk of the group sums the group's chunk partials itself -- lane l
//              adds partials l, l + 32, ..., then the butterfly -- as the consumers of ba_pcg_sum do
//   mean       (T)(sum / n_g) in fp64, the same bits to every member
// so a group of 2 costs one short lane loop and a group of 70 000 is 274 chunks side by side, and then 274 partials per chunk.
// A lane issues all its loads (8 members at most) before it adds the first: the sums keep their order, the latencies overlap.
// k_pcg_share does the chunk sums and finishes in the same launch every group of up to BA_SHARE_LOCAL chunks (2048 cameras): the
// solver lays the chunks of such a group into the 8 slots of ONE workgroup (empty slots pad the list), and the chunk sums meet in
// LDS.  k_pcg_share_wide, launched only when there is a longer group and only over the chunks of such groups, finishes those from
// the partials k_pcg_share left in memory.  Which of the two a group takes depends on its own size alone.
#ifndef BA_PCG_SHARE_HIP_H
#define BA_PCG_SHARE_HIP_H

#include "ba_pcg.hip.h" /* (BA_SHARE_CHUNK, BA_SHARE_LOCAL: ba_internal.h, with ba_plan_share_slots) */

// one chunk slot: members[m0 .. m0 + len) of a group of ng cameras whose chunks are the slots c0 .. c0 + nc - 1 (an empty slot: len 0)
struct ba_share_chunk { int m0, len, c0, nc, ng; };

// the lane's members of the chunk (-1: none) and their rows 6..8 of v, every load issued before the first use
template <typename T>
__device__ __forceinline__ void ba_share_load(const ba_share_chunk &d, int sub, const int *__restrict__ members, const T *__restrict__ v, int *idx,
                                              double &s0, double &s1, double &s2)
{
    T a[BA_SHARE_CHUNK / 32][3];
#pragma unroll
    for (int u = 0; u < BA_SHARE_CHUNK / 32; u++) idx[u] = sub + 32 * u < d.len ? members[d.m0 + sub + 32 * u] : -1;
#pragma unroll
    for (int u = 0; u < BA_SHARE_CHUNK / 32; u++) {
        const T *va = v + 9 * (size_t)(idx[u] >= 0 ? idx[u] : 0) + 6;
        a[u][0] = idx[u] >= 0 ? va[0] : (T)0; a[u][1] = idx[u] >= 0 ? va[1] : (T)0; a[u][2] = idx[u] >= 0 ? va[2] : (T)0;
    }
    s0 = 0; s1 = 0; s2 = 0;
#pragma unroll
    for (int u = 0; u < BA_SHARE_CHUNK / 32; u++)
        if (idx[u] >= 0) { s0 += (double)a[u][0]; s1 += (double)a[u][1]; s2 += (double)a[u][2]; }
}

template <typename T>
__device__ __forceinline__ void ba_share_write(const ba_share_chunk &d, const int *idx, double s0, double s1, double s2, T *__restrict__ v)
{
    const double ng = (double)d.ng;
    const T m0 = (T)(s0 / ng), m1 = (T)(s1 / ng), m2 = (T)(s2 / ng);
#pragma unroll
    for (int u = 0; u < BA_SHARE_CHUNK / 32; u++)
        if (idx[u] >= 0) {
            T *va = v + 9 * (size_t)idx[u] + 6;
            va[0] = m0; va[1] = m1; va[2] = m2;
        }
}

// Per chunk slot (a 32-lane group, 8 to a block): the chunk's sums of v's rows 6..8.  A group of one chunk gets its mean at once; one of
// up to BA_SHARE_LOCAL chunks, all in this block, after the chunk sums have met in LDS; a chunk of a longer group leaves its three sums
// in part[slot][3].  CHECK: a launch of the iteration (returns at once behind convergence).
template <typename T, bool CHECK>
__global__ __launch_bounds__(256) void k_pcg_share(int nslots, const ba_share_chunk *__restrict__ desc, const int *__restrict__ members,
                                                   T *__restrict__ v, double *__restrict__ part, const ba_pcg_dev *__restrict__ pcg)
{
    __shared__ double meet[8][3];
    if (CHECK && pcg->done) return; // (uniform)
    const int gl = threadIdx.x >> 5, c = blockIdx.x * 8 + gl, sub = threadIdx.x & 31;
    ba_share_chunk d{0, 0, 0, 1, 1};
    if (c < nslots) d = desc[c];
    int idx[BA_SHARE_CHUNK / 32];
    double s0, s1, s2;
    ba_share_load<T>(d, sub, members, v, idx, s0, s1, s2);
    s0 = group_sum<double, 32>(s0); s1 = group_sum<double, 32>(s1); s2 = group_sum<double, 32>(s2);
    const bool local = d.nc > 1 && d.nc <= BA_SHARE_LOCAL;
    if (local && sub == 0) { meet[gl][0] = s0; meet[gl][1] = s1; meet[gl][2] = s2; }
    __syncthreads();
    if (local) { // the group's chunk sums in chunk order: lane l holds partial l, then the butterfly (k_pcg_share_wide's order)
        const int l0 = d.c0 - blockIdx.x * 8;
        s0 = sub < d.nc ? meet[l0 + sub][0] : 0.0; s1 = sub < d.nc ? meet[l0 + sub][1] : 0.0; s2 = sub < d.nc ? meet[l0 + sub][2] : 0.0;
        s0 = group_sum<double, 32>(s0); s1 = group_sum<double, 32>(s1); s2 = group_sum<double, 32>(s2);
    }
    if (d.nc <= BA_SHARE_LOCAL) ba_share_write<T>(d, idx, s0, s1, s2, v);
    else if (sub == 0) { part[3 * (size_t)c] = s0; part[3 * (size_t)c + 1] = s1; part[3 * (size_t)c + 2] = s2; }
}

// Per chunk of a group of more than BA_SHARE_LOCAL chunks (wide[]: those slots, 8 to a block): the group's sum from all its chunk
// partials -- four loads in flight per lane, added in ascending order --, the mean to the chunk's own members.
template <typename T, bool CHECK>
__global__ __launch_bounds__(256) void k_pcg_share_wide(int nwide, const int *__restrict__ wide, const ba_share_chunk *__restrict__ desc,
                                                        const int *__restrict__ members, T *__restrict__ v, const double *__restrict__ part,
                                                        const ba_pcg_dev *__restrict__ pcg)
{
    if (CHECK && pcg->done) return;
    const int w = blockIdx.x * 8 + (threadIdx.x >> 5), sub = threadIdx.x & 31;
    ba_share_chunk d{0, 0, 0, 0, 1};
    if (w < nwide) d = desc[wide[w]];
    int idx[BA_SHARE_CHUNK / 32];
#pragma unroll
    for (int u = 0; u < BA_SHARE_CHUNK / 32; u++) idx[u] = sub + 32 * u < d.len ? members[d.m0 + sub + 32 * u] : -1;
    double s0 = 0, s1 = 0, s2 = 0;
    for (int j = sub; j < d.nc; j += 128) {
        double a[4][3];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const bool in = j + 32 * u < d.nc;
            const double *pj = part + 3 * (size_t)(d.c0 + (in ? j + 32 * u : 0));
            a[u][0] = in ? pj[0] : 0.0; a[u][1] = in ? pj[1] : 0.0; a[u][2] = in ? pj[2] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < 4; u++)
            if (j + 32 * u < d.nc) { s0 += a[u][0]; s1 += a[u][1]; s2 += a[u][2]; }
    }
    s0 = group_sum<double, 32>(s0); s1 = group_sum<double, 32>(s1); s2 = group_sum<double, 32>(s2);
    ba_share_write<T>(d, idx, s0, s1, s2, v);
}

// Behind the projection of y = S x (FINAL): the block partials of |rhs - y|^2 again, from the projected y, in k_pcg_cam's thread layout
// and order (one thread per (camera, row)) -- what k_pcg_finish reads is |Pi (rhs - S x)|^2, rhs being Pi rhs already.
template <typename T>
__global__ __launch_bounds__(256) void k_pcg_share_res(int N, const T *__restrict__ rhs, const T *__restrict__ y, double *__restrict__ part)
{
    __shared__ double red[4];
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    double acc = 0;
    if (idx < 9 * (size_t)N) { const double d = (double)rhs[idx] - (double)y[idx]; acc = d * d; }
    acc = block_reduce<double, false>(acc, red);
    if (threadIdx.x == 0) part[blockIdx.x] = acc;
}

#endif
