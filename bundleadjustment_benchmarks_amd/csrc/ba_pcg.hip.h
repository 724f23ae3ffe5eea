// ba_pcg.hip.h -- BA_ITERSCHUR: the reduced camera system S dx_c = rhs solved by preconditioned conjugate gradients, S never formed.
//
// S is the matrix CHOLESKY assembles (k_schur_pairs<T, true> + k_schur_reduce + k_post_reduce), from the same records k_elim_chol
// leaves (BA_REC: Z_o = A_o^T B_o L_p^-T per observation o, the point's 1 / D at BA_REC_DINV; t_p = L_p^-1 g_p per point):
//   S_ab = delta_ab (V_a + lambda I) - sum_p sum_{o in a, o' in b, both at p} Z_o diag(dinv_p) Z_o'^T
//   rhs_a = g_c,a - sum_{o in a} Z_o (dinv_p(o) o t_p(o))
// so one product y = S v is two passes over the records:
//   point pass   w_p = dinv_p o sum_{o at p} Z_o^T v_cam(o)                       (k_pcg_point: point-sorted, k_backsub's gather)
//   camera pass  y_a = (V_a + lambda I) v_a - sum_{o in a} Z_o w_p(o)              (k_pcg_cam_chunks over the camera-sorted chunks of
//                                                                                  <= 32 observations, then k_pcg_cam per camera)
// The preconditioner is block Jacobi: B_a = V_a + lambda I - sum_{o in a} Z_o diag(dinv) Z_o^T (the self entries of the camera's
// diagonal pair: the whole diagonal block of S unless a camera sees a point twice), inverted per camera in fp64.
//
// Every sum has a fixed order -- butterflies inside 32-lane groups, chunk partials summed per camera in chunk order, block partials
// summed by every consumer block in the same order -- and there are no atomics, so a solve is the same bits on every run, eager or
// replayed as a graph.  Dot products accumulate in fp64 for both scalar types.
//
// Loop control is on the device: the host enqueues max_iter iterations of four launches each.  Iteration k's first launch
// (k_pcg_point) reads |r_k|^2 from the block partials; when |r_k| <= rel_tol |rhs| it sets pcg->done and every later launch of the
// solve returns at once.  The scalars of the recurrence (r'z, p'Sp) are never stored as one value: each consumer block sums the
// block partials itself (same order, same bits), the partials of r'z kept for the last three iterations (k writes slot k + 1, reads
// k and k - 1).  p_k = z_k + beta_k p_{k-1} is formed on the fly by the consumers of iteration k and stored by its last launch.
// Behind the iterations one more product S x gives the true residual |rhs - S x| / |rhs| of the step (k_pcg_finish records it).
//
// BA_PRECOND_CONSTRAINT_FOREST (ba_pcg_forest.hip.h): the cameras of the forest's trees (in_tree) get their z from k_pcg_forest_apply,
// launched behind k_pcg_prec_inv and behind every k_pcg_update, which leave those cameras' z and r'z alone (FOREST instantiations).  The
// trees' partials of r'z follow the gc per-camera ones, so the list of r'z has gz = gc + trees entries per slot (gz = gc without a
// forest) while |r|^2 keeps gc.  BA_PRECOND_VISIBILITY_FOREST is the same with one partial per 256 trees (k_pcg_forest_rz).
//
// Shared intrinsics (ba_pcg_share.hip.h): with groups of cameras that solve for one f, k1, k2 the projection Pi (rows 6..8 of a group's
// members <- their mean) is launched on rhs in front of k_pcg_prec_inv and on z_0 behind it, on y = S p behind k_pcg_cam /
// k_pcg_relpose, on z behind k_pcg_update (behind the forest's apply), and the partials of |rhs - y|^2 are formed again from the
// projected y; the kernels of this file do not know about it.
//
// The model-decrease rule (ba_solver_set_pcg_model_tol; the kernels named *_q, launched instead of their namesakes
// when eta > 0): k_pcg_update_q also leaves the block partials of s_{k+1} = x_{k+1}'(rhs + r_{k+1}) = -2 Q(x_{k+1}) in slot k + 1 of a
// fourth list (part_s, gc entries per slot like |r|^2; slot 0 = 0 from k_pcg_start_q), and k_pcg_point_q, behind its residual test, stops
// the solve at k >= 1 when zeta_k = k (s_k - s_{k-1}) / s_k < eta.  k_pcg_update and its _q namesake are one body (ba_pcg_update_body<..., QS>)
// behind two entry points, the other three kernels of their own, so with eta = 0 a solve runs the kernels, the argument lists and the instructions it ran without the rule.
//
// What ba_pcg_multi.hip.h (the nine-column PCG of ba_solver_covariance_pcg) computes alike it takes from here: ba_chol9 / ba_chol9_inverse
// (a B_a's Cholesky and inverse), ba_pcg_dir (the direction formed on the fly), ba_dot9 (a block row by a 9-vector).  The chunk-order
// sums are spelled out per kernel: their tails differ on purpose, and the order of a sum is behaviour here.
#ifndef BA_PCG_HIP_H
#define BA_PCG_HIP_H

#include "ba_kernels.hip.h"
#include "ba_relpose.hip.h"

#define BA_PCG_CW 9 /* scalars per camera chunk of the camera pass in the chunk slab */

// solve state + counters for ba_solver_pcg_stats (device memory; read back by the host)
struct ba_pcg_dev {
    double bb;           // |rhs|^2 of the current solve
    int done, iters;     // converged at iteration `iters` (set by k_pcg_point)
    long long solves, total_iters;
    int last_iters, last_converged;
    double last_rel_residual;
    // the model-decrease rule (written by the *_q kernels alone)
    int rule, last_rule; // what set `done`: 1 residual, 2 model (k_pcg_point_q); of the last counted solve, 0 = the cap
    long long by_residual, by_model, at_cap;
    double last_zeta, last_model;
};

#include "ba_pcg_forest.hip.h" /* (needs ba_pcg_dev) */

// the block's fixed-order sum of n fp64 partials, returned to every thread (all 256 threads must call it)
__device__ __forceinline__ double ba_pcg_sum(const double *__restrict__ a, int n, double *lds)
{
    double v = 0;
    for (int k = threadIdx.x; k < n; k += 256) v += a[k];
    return block_reduce<double, false>(v, lds);
}
__device__ __forceinline__ int ba_pcg_slot(int k) { return k % 3; }
// the search direction at o, formed on the fly: p_k = z_k + beta_k p_{k-1} (FINAL, the product S x: x)
template <bool FINAL, typename T>
__device__ __forceinline__ T ba_pcg_dir(const T *x, const T *z, const T *p, T beta, size_t o)
{
    return FINAL ? x[o] : z[o] + beta * p[o];
}
// one row of a 9 x 9 block by a 9-vector, summed from entry 0 up
template <typename T> __device__ __forceinline__ T ba_dot9(const T *row, const T *v)
{
    T s = 0;
#pragma unroll
    for (int q = 0; q < 9; q++) s += row[q] * v[q];
    return s;
}
// B = L L^T in place on the packed lower triangle, (i, j) at i (i + 1) / 2 + j.  False on a pivot <= 0 (FINITE: or not finite); a pivot
// <= 0 is replaced by 1.
template <bool FINITE> __device__ __forceinline__ bool ba_chol9(double (&L)[45])
{
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 9; j++) {
        double d = L[j * (j + 1) / 2 + j];
#pragma unroll
        for (int k = 0; k < j; k++) d -= L[j * (j + 1) / 2 + k] * L[j * (j + 1) / 2 + k];
        ok = ok && d > 0 && (!FINITE || d < INFINITY);
        const double ljj = d > 0 ? sqrt(d) : 1.0;
        L[j * (j + 1) / 2 + j] = ljj;
#pragma unroll
        for (int i = j + 1; i < 9; i++) {
            double s = L[i * (i + 1) / 2 + j];
#pragma unroll
            for (int k = 0; k < j; k++) s -= L[i * (i + 1) / 2 + k] * L[j * (j + 1) / 2 + k];
            L[i * (i + 1) / 2 + j] = s / ljj;
        }
    }
    return ok;
}
// Mi = (L L^T)^-1 = W^T W, full 9 x 9, with W = L^-1 (packed lower)
__device__ __forceinline__ void ba_chol9_inverse(const double (&L)[45], double (&Mi)[81])
{
    double W[45];
#pragma unroll
    for (int i = 0; i < 9; i++) {
        const double inv = 1.0 / L[i * (i + 1) / 2 + i];
        W[i * (i + 1) / 2 + i] = inv;
#pragma unroll
        for (int j = 0; j < i; j++) {
            double s = 0;
#pragma unroll
            for (int k = j; k < i; k++) s += L[i * (i + 1) / 2 + k] * W[k * (k + 1) / 2 + j];
            W[i * (i + 1) / 2 + j] = -s * inv;
        }
    }
#pragma unroll
    for (int i = 0; i < 9; i++)
#pragma unroll
        for (int j = 0; j <= i; j++) {
            double s = 0;
#pragma unroll
            for (int k = i; k < 9; k++) s += W[k * (k + 1) / 2 + i] * W[k * (k + 1) / 2 + j];
            Mi[9 * i + j] = s;
            Mi[9 * j + i] = s;
        }
}

// ---- once per trial: block-Jacobi preconditioner, reduced rhs, start of the recurrence --------------------------------------------------
// Per camera chunk of <= 32 observations (one 32-lane group, lane = observation): the 45 lower-triangle entries of
// Z diag(dinv) Z^T and the 9 of Z (dinv o t), summed over the lanes through LDS in lane order (k_cam_gram's layout) into dslab.
template <typename T>
__global__ __launch_bounds__(256) void k_pcg_prec_chunks(int ndchunks, const int *__restrict__ dchunk_ptr, const int *__restrict__ cam_obs,
                                                         const int *__restrict__ obs_pt, const T *__restrict__ rec, const T *__restrict__ tvec,
                                                         int Ml, T *__restrict__ dslab)
{
    __shared__ T xch[8][27][33];
    const int gl = threadIdx.x >> 5, g = blockIdx.x * 8 + gl, sub = threadIdx.x & 31;
    const bool gok = g < ndchunks;
    const int e0 = gok ? dchunk_ptr[g] : 0, len = gok ? dchunk_ptr[g + 1] - e0 : 0;
    T v[54];
#pragma unroll
    for (int q = 0; q < 54; q++) v[q] = 0;
    if (sub < len) {
        const int o = cam_obs[e0 + sub];
        const size_t j = (size_t)obs_pt[o];
        const T *Z = rec + (size_t)o * BA_REC;
        T z[27], zd[27];
        const T d0 = Z[BA_REC_DINV], d1 = Z[BA_REC_DINV + 1], d2 = Z[BA_REC_DINV + 2];
#pragma unroll
        for (int q = 0; q < 27; q++) z[q] = Z[q];
#pragma unroll
        for (int c = 0; c < 9; c++) { zd[3 * c] = z[3 * c] * d0; zd[3 * c + 1] = z[3 * c + 1] * d1; zd[3 * c + 2] = z[3 * c + 2] * d2; }
        const T t0 = tvec[j], t1 = tvec[(size_t)Ml + j], t2 = tvec[2 * (size_t)Ml + j];
        int q = 0;
#pragma unroll
        for (int r = 0; r < 9; r++)
#pragma unroll
            for (int c = 0; c <= r; c++) v[q++] = zd[3 * r] * z[3 * c] + zd[3 * r + 1] * z[3 * c + 1] + zd[3 * r + 2] * z[3 * c + 2];
#pragma unroll
        for (int r = 0; r < 9; r++) v[45 + r] = zd[3 * r] * t0 + zd[3 * r + 1] * t1 + zd[3 * r + 2] * t2;
    }
#pragma unroll
    for (int pass = 0; pass < 2; pass++) {
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 27; q++) xch[gl][q][sub] = v[27 * pass + q];
        __syncthreads();
        if (gok && sub < 27) {
            T a = 0;
#pragma unroll
            for (int l = 0; l < 32; l++) a += xch[gl][sub][l];
            dslab[(size_t)g * BA_SLAB + 27 * pass + sub] = a;
        }
    }
}

// Per (camera, entry): the chunk partials summed in chunk order (k_cam_gram_reduce's order), then
//   B_a = (V_a - s) + lambda I  into Bm (full 9 x 9, inverted in place by k_pcg_prec_inv),  rhs_a = g_c,a - s,  g_c copied to gc_out.
// MARQ (ba_solver_set_damping): (V_a - s) + d with d = fl(lambda clamp(V_a,qq)) on the diagonal.
template <typename T, bool MARQ = false>
__global__ __launch_bounds__(256) void k_pcg_prec_reduce(int N, const int *__restrict__ cam_dchunk_ptr, const T *__restrict__ dslab,
                                                         const T *__restrict__ V, const T *__restrict__ gc, const T *__restrict__ lam,
                                                         T *__restrict__ Bm, T *__restrict__ rhs, T *__restrict__ gc_out,
                                                         ba_damp_args<T> da = ba_damp_args<T>{})
{
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t a = idx / BA_SLAB;
    const int e = (int)(idx - a * BA_SLAB);
    if (a >= (size_t)N || e >= 54) return;
    T s4[4] = {0, 0, 0, 0};
    const int c1 = cam_dchunk_ptr[a + 1];
    int c = cam_dchunk_ptr[a];
    for (; c + 15 < c1; c += 16) {
        T x[16];
#pragma unroll
        for (int u = 0; u < 16; u++) x[u] = dslab[(size_t)(c + u) * BA_SLAB + e];
#pragma unroll
        for (int u = 0; u < 16; u++) s4[u & 3] += x[u];
    }
    for (; c + 3 < c1; c += 4) {
#pragma unroll
        for (int u = 0; u < 4; u++) s4[u] += dslab[(size_t)(c + u) * BA_SLAB + e];
    }
    for (; c < c1; c++) s4[0] += dslab[(size_t)c * BA_SLAB + e];
    const T s = (s4[0] + s4[1]) + (s4[2] + s4[3]);
    if (e < 45) {
        int rr = 0;
        while ((rr + 1) * (rr + 2) / 2 <= e) rr++;
        const int cc = e - rr * (rr + 1) / 2;
        T v = -s;
        const T vd = V[a * 81 + 9 * rr + cc];
        v += vd;
        if (rr == cc) v += ba_damp<MARQ, T>(*lam, vd, da);
        Bm[a * 81 + 9 * rr + cc] = v;
        Bm[a * 81 + 9 * cc + rr] = v;
    } else {
        const size_t r = 9 * a + (e - 45);
        const T g = gc[r];
        rhs[r] = g - s;
        gc_out[r] = g;
    }
}

// Per camera (one thread): B_a = L L^T in fp64 and Bm <- B_a^-1 = L^-T L^-1 in place (a block that is not positive definite in
// working precision -- fp32 at a tiny lambda -- falls back to the inverse of its diagonal); x_0 = 0, r_0 = rhs, z_0 = M^-1 r_0,
// p_{-1} = 0; the block partials of r_0'z_0 and |r_0|^2 into slot 0.
template <typename T, bool FOREST = false>
__global__ __launch_bounds__(256) void k_pcg_prec_inv(int N, T *__restrict__ Bm, const T *__restrict__ rhs, T *__restrict__ x, T *__restrict__ r,
                                                      T *__restrict__ z, T *__restrict__ p, double *__restrict__ part_rz, double *__restrict__ part_rr,
                                                      const unsigned char *__restrict__ in_tree)
{
    __shared__ double red[4];
    const int a = blockIdx.x * 256 + threadIdx.x;
    double rz = 0, rr = 0;
    if (a < N) {
        T *B = Bm + (size_t)a * 81;
        double L[45]; // packed lower triangle, (i, j) at i (i + 1) / 2 + j
#pragma unroll
        for (int i = 0; i < 9; i++)
#pragma unroll
            for (int j = 0; j <= i; j++) L[i * (i + 1) / 2 + j] = (double)B[9 * i + j];
        double Mi[81];
        if (ba_chol9<false>(L)) ba_chol9_inverse(L, Mi);
        else {
#pragma unroll
            for (int q = 0; q < 81; q++) Mi[q] = 0;
#pragma unroll
            for (int i = 0; i < 9; i++) {
                const double d = (double)B[10 * i];
                Mi[10 * i] = d > 0 ? 1.0 / d : 0.0;
            }
        }
        T Mt[81];
#pragma unroll
        for (int q = 0; q < 81; q++) { Mt[q] = (T)Mi[q]; B[q] = Mt[q]; }
        T b[9];
#pragma unroll
        for (int i = 0; i < 9; i++) b[i] = rhs[9 * (size_t)a + i];
#pragma unroll
        for (int i = 0; i < 9; i++) {
            T zi = 0; // (not ba_dot9: in fp32 with FOREST the compiler then fuses products that it leaves unfused here)
#pragma unroll
            for (int k = 0; k < 9; k++) zi += Mt[9 * i + k] * b[k];
            const size_t o = 9 * (size_t)a + i;
            x[o] = 0; r[o] = b[i]; z[o] = zi; p[o] = 0;
            if (!(FOREST && in_tree[a])) rz += (double)b[i] * (double)zi;
            rr += (double)b[i] * (double)b[i];
        }
    }
    rz = block_reduce<double, false>(rz, red);
    rr = block_reduce<double, false>(rr, red);
    if (threadIdx.x == 0) { part_rz[blockIdx.x] = rz; part_rr[blockIdx.x] = rr; }
}

// one block: |rhs|^2 of this solve, the loop state cleared
__global__ __launch_bounds__(256) void k_pcg_start(const double *__restrict__ part_rr, int gc, ba_pcg_dev *__restrict__ pcg)
{
    __shared__ double red[4];
    const double bb = ba_pcg_sum(part_rr, gc, red);
    if (threadIdx.x == 0) { pcg->bb = bb; pcg->done = 0; pcg->iters = 0; }
}

// with the model rule: s_0 = 0 into slot 0 of part_s as well
__global__ __launch_bounds__(256) void k_pcg_start_q(const double *__restrict__ part_rr, int gc, ba_pcg_dev *__restrict__ pcg, double *__restrict__ part_s)
{
    __shared__ double red[4];
    const double bb = ba_pcg_sum(part_rr, gc, red);
    for (int i = threadIdx.x; i < gc; i += 256) part_s[i] = 0.0;
    if (threadIdx.x == 0) { pcg->bb = bb; pcg->done = 0; pcg->iters = 0; pcg->rule = 0; }
}

// zeta_k = k (s_k - s_{k-1}) / s_k and s_k from the block partials of slots k and k - 1 (k >= 1); every block sums them itself
__device__ __forceinline__ double ba_pcg_zeta(int k, const double *__restrict__ part_s, int gc, double *red, double *s_out)
{
    const double sk = ba_pcg_sum(part_s + (size_t)ba_pcg_slot(k) * gc, gc, red);
    const double sm = ba_pcg_sum(part_s + (size_t)ba_pcg_slot(k + 2) * gc, gc, red);
    *s_out = sk;
    return (double)k * (sk - sm) / sk;
}

// ---- per iteration k (FINAL: the product S x behind the last iteration) -----------------------------------------------------------------
// beta_k = (r_k'z_k) / (r_{k-1}'z_{k-1}) from the block partials (0 at k = 0); every block sums them itself
__device__ __forceinline__ double ba_pcg_beta(int k, const double *__restrict__ part_rz, int gz, double *red)
{
    if (k == 0) return 0.0;
    const double rzk = ba_pcg_sum(part_rz + (size_t)ba_pcg_slot(k) * gz, gz, red);
    const double rzm = ba_pcg_sum(part_rz + (size_t)ba_pcg_slot(k + 2) * gz, gz, red);
    return rzk / rzm;
}

// Point pass, LPP lanes per point (k_backsub's gather): w_p = dinv_p o sum_{o at p} Z_o^T v_cam(o), v = p_k = z_k + beta_k p_{k-1}
// (FINAL: v = x).  Iteration k's convergence test sits at its head.
template <typename T, int LPP, bool FINAL>
__global__ __launch_bounds__(256) void k_pcg_point(int k, int Ml, const int *__restrict__ pt_ptr, const int *__restrict__ obs_cam,
                                                   const T *__restrict__ rec, const T *__restrict__ dinv, const T *__restrict__ z,
                                                   const T *__restrict__ p, const T *__restrict__ x, const double *__restrict__ part_rz,
                                                   const double *__restrict__ part_rr, int gc, int gz, double tol2, ba_pcg_dev *__restrict__ pcg,
                                                   T *__restrict__ w)
{
    __shared__ double red[4];
    T beta = 0;
    if (!FINAL) {
        if (pcg->done) return; // (uniform)
        const double rr = ba_pcg_sum(part_rr + (size_t)ba_pcg_slot(k) * gc, gc, red);
        if (rr <= tol2 * pcg->bb) { // |r_k| <= rel_tol |rhs|: every block sees the same sums
            if (blockIdx.x == 0 && threadIdx.x == 0) { pcg->done = 1; pcg->iters = k; }
            return;
        }
        beta = (T)ba_pcg_beta(k, part_rz, gz, red);
    }
    const int gid = (blockIdx.x * 256 + threadIdx.x) / LPP, lg = threadIdx.x % LPP;
    const bool ok = gid < Ml;
    const int b = ok ? pt_ptr[gid] : 0, e = ok ? pt_ptr[gid + 1] : 0;
    T s0 = 0, s1 = 0, s2 = 0;
    for (int i = b + lg; i < e; i += LPP) {
        const T *Z = rec + (size_t)i * BA_REC;
        const size_t c0 = 9 * (size_t)obs_cam[i];
#pragma unroll
        for (int c = 0; c < 9; c++) {
            const T v = ba_pcg_dir<FINAL>(x, z, p, beta, c0 + c);
            s0 += Z[3 * c] * v; s1 += Z[3 * c + 1] * v; s2 += Z[3 * c + 2] * v;
        }
    }
    s0 = group_sum<T, LPP>(s0); s1 = group_sum<T, LPP>(s1); s2 = group_sum<T, LPP>(s2);
    if (ok && lg == 0) {
        const size_t j = (size_t)gid, M = (size_t)Ml;
        const bool empty = b == e; // (no record ever wrote this point's dinv)
        w[j] = empty ? (T)0 : dinv[j] * s0;
        w[M + j] = empty ? (T)0 : dinv[M + j] * s1;
        w[2 * M + j] = empty ? (T)0 : dinv[2 * M + j] * s2;
    }
}
// k_pcg_point<T, LPP, false> with the model rule behind the residual's.  A kernel of its own and not one body behind two entry points like
// k_pcg_update: inlined into two kernels the fp64 gather came out with another base address for its record loads, and the kernels of a
// solve without the rule are to stay the instructions they were.
template <typename T, int LPP>
__global__ __launch_bounds__(256) void k_pcg_point_q(int k, int Ml, const int *__restrict__ pt_ptr, const int *__restrict__ obs_cam,
                                                     const T *__restrict__ rec, const T *__restrict__ dinv, const T *__restrict__ z,
                                                     const T *__restrict__ p, const double *__restrict__ part_rz,
                                                     const double *__restrict__ part_rr, int gc, int gz, double tol2, ba_pcg_dev *__restrict__ pcg,
                                                     T *__restrict__ w, double eta, const double *__restrict__ part_s)
{
    __shared__ double red[4];
    if (pcg->done) return; // (uniform)
    const double rr = ba_pcg_sum(part_rr + (size_t)ba_pcg_slot(k) * gc, gc, red);
    if (rr <= tol2 * pcg->bb) {
        if (blockIdx.x == 0 && threadIdx.x == 0) { pcg->done = 1; pcg->iters = k; pcg->rule = 1; }
        return;
    }
    if (k >= 1) { // zeta_k < eta: the model has stopped decreasing (s_k <= 0 or not finite: no verdict); every block sees the same sums
        double sk;
        const double zeta = ba_pcg_zeta(k, part_s, gc, red, &sk);
        if (sk > 0 && sk < INFINITY && zeta < eta) {
            if (blockIdx.x == 0 && threadIdx.x == 0) { pcg->done = 1; pcg->iters = k; pcg->rule = 2; }
            return;
        }
    }
    const T beta = (T)ba_pcg_beta(k, part_rz, gz, red);
    const int gid = (blockIdx.x * 256 + threadIdx.x) / LPP, lg = threadIdx.x % LPP;
    const bool ok = gid < Ml;
    const int b = ok ? pt_ptr[gid] : 0, e = ok ? pt_ptr[gid + 1] : 0;
    T s0 = 0, s1 = 0, s2 = 0;
    for (int i = b + lg; i < e; i += LPP) {
        const T *Z = rec + (size_t)i * BA_REC;
        const size_t c0 = 9 * (size_t)obs_cam[i];
#pragma unroll
        for (int c = 0; c < 9; c++) {
            const T v = ba_pcg_dir<false>((const T *)nullptr, z, p, beta, c0 + c);
            s0 += Z[3 * c] * v; s1 += Z[3 * c + 1] * v; s2 += Z[3 * c + 2] * v;
        }
    }
    s0 = group_sum<T, LPP>(s0); s1 = group_sum<T, LPP>(s1); s2 = group_sum<T, LPP>(s2);
    if (ok && lg == 0) {
        const size_t j = (size_t)gid, M = (size_t)Ml;
        const bool empty = b == e; // (no record ever wrote this point's dinv)
        w[j] = empty ? (T)0 : dinv[j] * s0;
        w[M + j] = empty ? (T)0 : dinv[M + j] * s1;
        w[2 * M + j] = empty ? (T)0 : dinv[2 * M + j] * s2;
    }
}

// Camera pass, part 1: per camera chunk of <= 32 observations (a 32-lane group, lane = observation) sum_o Z_o w_p(o), a butterfly over
// the group, into slab[chunk][9]
template <typename T, bool FINAL>
__global__ __launch_bounds__(256) void k_pcg_cam_chunks(int ndchunks, const int *__restrict__ dchunk_ptr, const int *__restrict__ cam_obs,
                                                        const int *__restrict__ obs_pt, const T *__restrict__ rec, int Ml, const T *__restrict__ w,
                                                        T *__restrict__ slab, const ba_pcg_dev *__restrict__ pcg)
{
    if (!FINAL && pcg->done) return;
    const int g = blockIdx.x * 8 + (threadIdx.x >> 5), sub = threadIdx.x & 31;
    const bool gok = g < ndchunks;
    const int e0 = gok ? dchunk_ptr[g] : 0, len = gok ? dchunk_ptr[g + 1] - e0 : 0;
    T y[9];
#pragma unroll
    for (int q = 0; q < 9; q++) y[q] = 0;
    if (sub < len) {
        const int o = cam_obs[e0 + sub];
        const size_t j = (size_t)obs_pt[o], M = (size_t)Ml;
        const T *Z = rec + (size_t)o * BA_REC;
        const T w0 = w[j], w1 = w[M + j], w2 = w[2 * M + j];
#pragma unroll
        for (int q = 0; q < 9; q++) y[q] = Z[3 * q] * w0 + Z[3 * q + 1] * w1 + Z[3 * q + 2] * w2;
    }
#pragma unroll
    for (int q = 0; q < 9; q++) y[q] = group_sum<T, 32>(y[q]);
    if (gok && sub == 0) {
#pragma unroll
        for (int q = 0; q < 9; q++) slab[(size_t)g * BA_PCG_CW + q] = y[q];
    }
}

// Camera pass, part 2, one thread per (camera, row): y_a,r = ((V_a + lambda I) v_a)_r - sum of the camera's chunk partials (chunk order);
// the block partials of v'y (iteration) or |rhs - y|^2 (FINAL, y = S x) into part[blockIdx]
// MARQ (ba_solver_set_damping): (t + d v_r) - s with d = fl(lambda clamp(V_a,rr)).
template <typename T, bool FINAL, bool MARQ = false>
__global__ __launch_bounds__(256) void k_pcg_cam(int k, int N, const int *__restrict__ cam_dchunk_ptr, const T *__restrict__ slab,
                                                 const T *__restrict__ V, const T *__restrict__ lam, const T *__restrict__ z,
                                                 const T *__restrict__ p, const T *__restrict__ x, const T *__restrict__ rhs,
                                                 const double *__restrict__ part_rz, int gz, T *__restrict__ y, double *__restrict__ part,
                                                 const ba_pcg_dev *__restrict__ pcg, ba_damp_args<T> da = ba_damp_args<T>{})
{
    __shared__ double red[4];
    T beta = 0;
    if (!FINAL) {
        if (pcg->done) return;
        beta = (T)ba_pcg_beta(k, part_rz, gz, red);
    }
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t a = idx / 9;
    const int r = (int)(idx - 9 * a);
    double acc = 0;
    if (a < (size_t)N) {
        T s4[4] = {0, 0, 0, 0};
        const int c1 = cam_dchunk_ptr[a + 1];
        int c = cam_dchunk_ptr[a];
        for (; c + 15 < c1; c += 16) {
            T xx[16];
#pragma unroll
            for (int u = 0; u < 16; u++) xx[u] = slab[(size_t)(c + u) * BA_PCG_CW + r];
#pragma unroll
            for (int u = 0; u < 16; u++) s4[u & 3] += xx[u];
        }
        for (; c < c1; c++) s4[0] += slab[(size_t)c * BA_PCG_CW + r];
        const T s = (s4[0] + s4[1]) + (s4[2] + s4[3]);
        const T *Va = V + a * 81 + 9 * r;
        T t = 0, vr = 0;
#pragma unroll
        for (int q = 0; q < 9; q++) {
            const size_t o = 9 * a + q;
            const T v = ba_pcg_dir<FINAL>(x, z, p, beta, o);
            t += Va[q] * v;
            if (q == r) vr = v;
        }
        const T yr = (t + ba_damp<MARQ, T>(*lam, MARQ ? Va[r] : (T)0, da) * vr) - s;
        y[9 * a + r] = yr;
        if (FINAL) { const double d = (double)rhs[9 * a + r] - (double)yr; acc = d * d; }
        else acc = (double)vr * (double)yr;
    }
    acc = block_reduce<double, false>(acc, red);
    if (threadIdx.x == 0) part[blockIdx.x] = acc;
}

// Relative-pose constraints (ba_relpose.hip.h), directly behind k_pcg_cam and with its thread layout: y_a,r += sum over the camera's
// incident constraints (H_ab v_b)_r in the CSR's order, and the block partial follows -- v'y gains the block's sum of v_r times that
// term, |rhs - y|^2 (FINAL) is formed again from the new y in k_pcg_cam's order.  A launch of its own and not an instantiation of
// k_pcg_cam: which products of a sum the compiler fuses is its choice per instantiation (in fp32 k_pcg_cam's V_a v is unfused, the same
// lines with the constraint term behind them came out fused), and constraints without information must leave every bit of the solve alone
// -- here they add exact zeros to y and to the partial.
template <typename T, bool FINAL>
__global__ __launch_bounds__(256) void k_pcg_relpose(int k, int N, ba_relpose_csr<T> cs, const T *__restrict__ z, const T *__restrict__ p,
                                                     const T *__restrict__ x, const T *__restrict__ rhs, const double *__restrict__ part_rz,
                                                     int gz, T *__restrict__ y, double *__restrict__ part, const ba_pcg_dev *__restrict__ pcg)
{
    __shared__ double red[4];
    T beta = 0;
    if (!FINAL) {
        if (pcg->done) return;
        beta = (T)ba_pcg_beta(k, part_rz, gz, red);
    }
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t a = idx / 9;
    const int r = (int)(idx - 9 * a);
    double acc = 0;
    if (a < (size_t)N) {
        const T rp = ba_relpose_matvec_row<T>(cs, (int)a, r, [&](size_t o) { return ba_pcg_dir<FINAL>(x, z, p, beta, o); });
        const T yr = y[9 * a + r] + rp;
        y[9 * a + r] = yr;
        if (FINAL) { const double d = (double)rhs[9 * a + r] - (double)yr; acc = d * d; }
        else acc = (double)ba_pcg_dir<false>(x, z, p, beta, 9 * a + r) * (double)rp;
    }
    acc = block_reduce<double, false>(acc, red);
    if (threadIdx.x == 0) part[blockIdx.x] = FINAL ? acc : part[blockIdx.x] + acc;
}

// Per camera (one thread): alpha_k = r_k'z_k / p_k'S p_k; x += alpha p_k; r -= alpha S p_k; p <- p_k; z = M^-1 r; the block partials of
// r_{k+1}'z_{k+1} and |r_{k+1}|^2 into slot k + 1
// (QS, k_pcg_update_q: also the block partials of s_{k+1} = x_{k+1}'(rhs + r_{k+1}), from the values just written, into slot k + 1)
template <typename T, bool FOREST, bool QS>
__device__ __forceinline__ void ba_pcg_update_body(int k, int N, const T *__restrict__ Minv, const T *__restrict__ y, T *__restrict__ z,
                                                   T *__restrict__ p, T *__restrict__ x, T *__restrict__ r, double *__restrict__ part_rz,
                                                   double *__restrict__ part_rr, const double *__restrict__ part_py, int gc, int gz, int gq,
                                                   const ba_pcg_dev *__restrict__ pcg, const unsigned char *__restrict__ in_tree,
                                                   const T *__restrict__ rhs, double *__restrict__ part_s)
{
    __shared__ double red[4];
    if (pcg->done) return;
    const double rzk = ba_pcg_sum(part_rz + (size_t)ba_pcg_slot(k) * gz, gz, red);
    const T beta = (T)ba_pcg_beta(k, part_rz, gz, red);
    const double py = ba_pcg_sum(part_py, gq, red);
    const T alpha = (T)(rzk / py);
    const int a = blockIdx.x * 256 + threadIdx.x;
    double rz = 0, rr = 0, sx = 0;
    if (a < N) {
        const size_t o = 9 * (size_t)a;
        T rv[9];
#pragma unroll
        for (int q = 0; q < 9; q++) {
            const T pv = z[o + q] + beta * p[o + q];
            const T xv = x[o + q] + alpha * pv;
            x[o + q] = xv;
            p[o + q] = pv;
            rv[q] = r[o + q] - alpha * y[o + q];
            r[o + q] = rv[q];
            if (QS) sx += (double)xv * ((double)rhs[o + q] + (double)rv[q]);
        }
        const T *Mi = Minv + (size_t)a * 81;
        const bool tree = FOREST && in_tree[a]; // (z and r'z of this camera: k_pcg_forest_apply, directly behind)
#pragma unroll
        for (int i = 0; i < 9; i++) {
            T zi = 0; // (not ba_dot9: the fp32 FOREST instantiation then needs 82 registers instead of 80, one wave less per SIMD)
#pragma unroll
            for (int q = 0; q < 9; q++) zi += Mi[9 * i + q] * rv[q];
            if (!tree) {
                z[o + i] = zi;
                rz += (double)rv[i] * (double)zi;
            }
            rr += (double)rv[i] * (double)rv[i];
        }
    }
    rz = block_reduce<double, false>(rz, red);
    rr = block_reduce<double, false>(rr, red);
    if (threadIdx.x == 0) {
        part_rz[(size_t)ba_pcg_slot(k + 1) * gz + blockIdx.x] = rz;
        part_rr[(size_t)ba_pcg_slot(k + 1) * gc + blockIdx.x] = rr;
    }
    if (QS) {
        sx = block_reduce<double, false>(sx, red);
        if (threadIdx.x == 0) part_s[(size_t)ba_pcg_slot(k + 1) * gc + blockIdx.x] = sx;
    }
}
template <typename T, bool FOREST = false>
__global__ __launch_bounds__(256) void k_pcg_update(int k, int N, const T *__restrict__ Minv, const T *__restrict__ y, T *__restrict__ z,
                                                    T *__restrict__ p, T *__restrict__ x, T *__restrict__ r, double *__restrict__ part_rz,
                                                    double *__restrict__ part_rr, const double *__restrict__ part_py, int gc, int gz, int gq,
                                                    const ba_pcg_dev *__restrict__ pcg, const unsigned char *__restrict__ in_tree)
{
    ba_pcg_update_body<T, FOREST, false>(k, N, Minv, y, z, p, x, r, part_rz, part_rr, part_py, gc, gz, gq, pcg, in_tree, nullptr, nullptr);
}
template <typename T, bool FOREST = false>
__global__ __launch_bounds__(256) void k_pcg_update_q(int k, int N, const T *__restrict__ Minv, const T *__restrict__ y, T *__restrict__ z,
                                                      T *__restrict__ p, T *__restrict__ x, T *__restrict__ r, double *__restrict__ part_rz,
                                                      double *__restrict__ part_rr, const double *__restrict__ part_py, int gc, int gz, int gq,
                                                      const ba_pcg_dev *__restrict__ pcg, const unsigned char *__restrict__ in_tree,
                                                      const T *__restrict__ rhs, double *__restrict__ part_s)
{
    ba_pcg_update_body<T, FOREST, true>(k, N, Minv, y, z, p, x, r, part_rz, part_rr, part_py, gc, gz, gq, pcg, in_tree, rhs, part_s);
}

// One block, behind the product S x: iterations used, convergence, |rhs - S x| / |rhs|.  Counted unless `skip` is set (a trial that
// ba_minimize enqueued behind the end of the run: k_lm_control ignores it, so do the statistics).
__global__ __launch_bounds__(256) void k_pcg_finish(int max_iter, const double *__restrict__ part_rr, int gc, const double *__restrict__ part_res,
                                                    int gq, double tol2, ba_pcg_dev *__restrict__ pcg, const int *__restrict__ skip)
{
    __shared__ double red[4];
    const double rr = ba_pcg_sum(part_rr + (size_t)ba_pcg_slot(max_iter) * gc, gc, red);
    const double res = ba_pcg_sum(part_res, gq, red);
    if (threadIdx.x != 0) return;
    const double bb = pcg->bb;
    const bool done = pcg->done != 0;
    const int iters = done ? pcg->iters : max_iter;
    const int conv = (done || rr <= tol2 * bb) ? 1 : 0;
    if (skip && *skip) return;
    pcg->solves += 1;
    pcg->total_iters += iters;
    pcg->last_iters = iters;
    pcg->last_converged = conv;
    pcg->last_rel_residual = bb > 0 ? sqrt(res / bb) : 0.0;
}
// with the model rule: also which rule ended the solve (at the cap: the residual's when |r_max_iter| meets it, else none), zeta and s of
// the final iterate, and the three counters -- counted as above
__global__ __launch_bounds__(256) void k_pcg_finish_q(int max_iter, const double *__restrict__ part_rr, int gc, const double *__restrict__ part_res,
                                                      int gq, double tol2, ba_pcg_dev *__restrict__ pcg, const int *__restrict__ skip,
                                                      const double *__restrict__ part_s)
{
    __shared__ double red[4];
    const double rr = ba_pcg_sum(part_rr + (size_t)ba_pcg_slot(max_iter) * gc, gc, red);
    const double res = ba_pcg_sum(part_res, gq, red);
    const bool done = pcg->done != 0; // (uniform: nothing writes it behind the iterations)
    const int iters = done ? pcg->iters : max_iter;
    double sk = 0, zeta = 0;
    if (iters >= 1) zeta = ba_pcg_zeta(iters, part_s, gc, red, &sk);
    if (threadIdx.x != 0) return;
    const double bb = pcg->bb;
    const int rule = done ? pcg->rule : rr <= tol2 * bb ? 1 : 0;
    if (skip && *skip) return;
    pcg->solves += 1;
    pcg->total_iters += iters;
    pcg->last_iters = iters;
    pcg->last_converged = rule != 0;
    pcg->last_rel_residual = bb > 0 ? sqrt(res / bb) : 0.0;
    pcg->last_rule = rule;
    pcg->last_zeta = zeta;
    pcg->last_model = sk;
    if (rule == 1) pcg->by_residual += 1;
    else if (rule == 2) pcg->by_model += 1;
    else pcg->at_cap += 1;
}

#endif
