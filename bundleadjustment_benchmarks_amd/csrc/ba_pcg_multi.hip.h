// ba_pcg_multi.hip.h -- ba_solver_covariance_pcg: covariance blocks of BA_ITERSCHUR by a PCG on NR = 9 right-hand sides at once, gfx950, fp64.
//
// Sigma_cc = S^-1 and Sigma_pp = U_p^-1 + Y_p^T S^-1 Y_p (Y_p = W_p U_p^-1), so a block is the solution of S X = B
// for a few sparse columns: E_b (9 columns) for the camera pairs of column block b, Y_p (3 columns) for a point, three points to a batch.
// The product by S is bound by reading the elimination's records (ba_pcg.hip.h: 256 B per observation, twice per product); here one
// read of a record, of a V_a or of an H_ab serves all nine columns.  The columns are independent conjugate-gradient recurrences that
// merely share the launches: each has its own alpha, beta, partial sums, done flag and iteration count.
//
// Layout: every vector is [9 N][NR], a row's nine column values contiguous (72 B).  Camera kernels run one thread per (camera, column),
// 28 cameras (252 threads) per workgroup.
//
// Per batch:    k_mc_rhs_cam | k_mc_rhs_pts -> B;  k_mc_init (x = 0, r = B, z = M^-1 r, p = 0);  k_mc_scal<true>
// Iteration k:  k_mc_point       w_p = dinv_p o sum_{o at p} Z_o^T v_cam(o)          v = p_k = z_k + beta_k p_{k-1}, formed on the fly
//               k_mc_cam_chunks  per chunk of <= 32 observations sum_o Z_o w_p(o)     (butterflies over the 32-lane group)
//               k_mc_cam         y_a = (V_a + lambda I) v_a - chunk partials (chunk order) + sum_b H_ab v_b;  block partials of v'y
//               k_mc_alpha       (one workgroup) p'Sp per column from the block partials, alpha = r'z / p'Sp; p'Sp <= 0 -> singular
//               k_mc_update      x += alpha p, r -= alpha y, p <- p_k, z = M^-1 r;  block partials of r'z and |r|^2
//               k_mc_scal        (one workgroup) r'z, |r|^2 per column, beta, the convergence test |r| <= rel_tol |b|
// Behind them:  the product S X (FINAL instantiations) and k_mc_alpha<true>: |b - S x|^2 per column.
//
// The two one-workgroup launches hold the recurrence's scalars in ba_mc_dev, so no consumer sums partial lists itself.  Every sum has a
// fixed order that depends on the column's own data only -- 8-lane and 32-lane butterflies, chunk partials in chunk order, the 28
// cameras of a workgroup in index order, the workgroups' partials in 16 strided lanes and a butterfly -- and there are no atomics: a
// column's bits do not depend on what shares its batch.  A column that is done (converged, or a zero right-hand side) is frozen:
// k_mc_update leaves its x, r, z, p alone.  No workgroup waits for another.  Every launch returns at once when all columns are done
// or a singular flag is up; the host enqueues rounds of iterations and reads the state word back between them.
//
// The arithmetic is the trial's (ba_pcg.hip.h: ba_chol9, ba_chol9_inverse, ba_pcg_dir, ba_dot9); the kernels stay apart from their
// k_pcg_* counterparts because their loop control differs.
#ifndef BA_PCG_MULTI_HIP_H
#define BA_PCG_MULTI_HIP_H

#include "ba_pcg.hip.h" /* ba_chol9, ba_chol9_inverse, ba_pcg_dir, ba_dot9 */

#define BA_MC_NR 9   /* columns of a batch */
#define BA_MC_CPB 28 /* cameras per workgroup of the camera kernels (28 x 9 = 252 threads of 256) */

struct ba_mc_dev {
    double bb[BA_MC_NR], rz[BA_MC_NR], beta[BA_MC_NR], alpha[BA_MC_NR], rr[BA_MC_NR], res[BA_MC_NR];
    int done[BA_MC_NR], iters[BA_MC_NR];
    int alldone, singular, flag /* the preparation's: a point block or a B_a that is not positive definite */;
};

// The nine per-column sums of a partial list [n][NR]: lane l of column c's 16 lanes adds rows l, l + 16, ..., a butterfly closes it.
// All 256 threads call; out[] (LDS, >= NR) is valid behind the call.
__device__ __forceinline__ void ba_mc_sums(const double *__restrict__ part, int n, double *out)
{
    const int c = threadIdx.x >> 4, l = threadIdx.x & 15;
    double s = 0;
    if (c < BA_MC_NR)
        for (int b = l; b < n; b += 16) s += part[(size_t)b * BA_MC_NR + c];
    s = group_sum<double, 16>(s);
    __syncthreads();
    if (c < BA_MC_NR && l == 0) out[c] = s;
    __syncthreads();
}

// The workgroup's per-column sum of one value per (camera, column) thread, cameras in index order; thread c < NR returns column c's.
__device__ __forceinline__ double ba_mc_block_cols(double v, double *sh /* [256] */)
{
    __syncthreads();
    sh[threadIdx.x] = v;
    __syncthreads();
    double s = 0;
    if (threadIdx.x < BA_MC_NR)
        for (int la = 0; la < BA_MC_CPB; la++) s += sh[BA_MC_NR * la + threadIdx.x];
    return s;
}

// ---- once per call ---------------------------------------------------------------------------------------------------------------------
// Per camera (one thread): the fixed rows and columns of B_a (k_pcg_prec_reduce's block at this lambda) become the identity, then
// B_a = L L^T in fp64 and Bm <- B_a^-1 in place.  A block that is not positive definite raises the flag: the trial's fallback to the
// block's diagonal would hide a rank defect.
__global__ __launch_bounds__(256) void k_mc_prec_inv(int N, double *__restrict__ Bm, const unsigned short *__restrict__ cmask, int *__restrict__ flag)
{
    const int a = blockIdx.x * 256 + threadIdx.x;
    if (a >= N) return;
    double *B = Bm + (size_t)a * 81;
    const unsigned cm = cmask ? (unsigned)cmask[a] : 0u;
    double L[45]; // packed lower triangle, (i, j) at i (i + 1) / 2 + j
#pragma unroll
    for (int i = 0; i < 9; i++)
#pragma unroll
        for (int j = 0; j <= i; j++) {
            const bool fx = ((cm >> i) | (cm >> j)) & 1u;
            L[i * (i + 1) / 2 + j] = fx ? (i == j ? 1.0 : 0.0) : B[9 * i + j];
        }
    if (!ba_chol9<true>(L)) *flag = 1; // (every writer stores the same value)
    double Mi[81];
    ba_chol9_inverse(L, Mi);
#pragma unroll
    for (int q = 0; q < 81; q++) B[q] = Mi[q];
}

// ---- right-hand sides (the vector is zeroed in front) ------------------------------------------------------------------------------------
// E_b: column c is the unit vector of parameter c of camera b; the column of a fixed parameter stays zero and is never live
__global__ __launch_bounds__(64) void k_mc_rhs_cam(int b, const unsigned short *__restrict__ cmask, double *__restrict__ rhs)
{
    const int c = threadIdx.x;
    if (c >= BA_MC_NR) return;
    if (cmask && (((unsigned)cmask[b] >> c) & 1u)) return;
    rhs[(9 * (size_t)b + c) * BA_MC_NR + c] = 1.0;
}

// L^-1 of the point's unit lower factor out of tri ([6][Ml]: 1, l10, l20, 1, l21, 1) and its 1 / D
struct ba_mc_pt { double li10, li20, li21, d0, d1, d2; };
__device__ __forceinline__ ba_mc_pt ba_mc_point_factor(int j, int Ml, const double *__restrict__ tri, const double *__restrict__ dinv)
{
    const size_t M = (size_t)Ml;
    const double l10 = tri[M + j], l20 = tri[2 * M + j], l21 = tri[4 * M + j];
    ba_mc_pt f;
    f.li10 = -l10; f.li21 = -l21; f.li20 = l10 * l21 - l20;
    f.d0 = dinv[j]; f.d1 = dinv[M + j]; f.d2 = dinv[2 * M + j];
    return f;
}
// row r of Y_o = Z_o D^-1 L^-1 (W_o U^-1 with U = L D L^T and Z_o = W_o L^-T)
__device__ __forceinline__ void ba_mc_yrow(const double *__restrict__ Z, int r, const ba_mc_pt &f, double (&y)[3])
{
    const double a0 = Z[3 * r] * f.d0, a1 = Z[3 * r + 1] * f.d1, a2 = Z[3 * r + 2] * f.d2;
    y[0] = a0 + a1 * f.li10 + a2 * f.li20;
    y[1] = a1 + a2 * f.li21;
    y[2] = a2;
}

// Y_p for up to three points: thread i owns point i and columns 3 i .. 3 i + 2, its observations in order (a camera that sees the
// point twice gets the sum).  A fixed point's columns stay zero.
__global__ __launch_bounds__(64) void k_mc_rhs_pts(int np, const int *__restrict__ ids, int Ml, const int *__restrict__ pt_ptr,
                                                   const int *__restrict__ obs_cam, const double *__restrict__ rec, const double *__restrict__ dinv,
                                                   const double *__restrict__ tri, const unsigned char *__restrict__ pfix, double *__restrict__ rhs)
{
    const int i = threadIdx.x;
    if (i >= np) return;
    const int j = ids[i];
    if (pfix && pfix[j]) return;
    const int o0 = pt_ptr[j], o1 = pt_ptr[j + 1];
    if (o0 == o1) return;
    const ba_mc_pt f = ba_mc_point_factor(j, Ml, tri, dinv);
    for (int o = o0; o < o1; o++) {
        const double *Z = rec + (size_t)o * BA_REC;
        const size_t row0 = 9 * (size_t)obs_cam[o];
        for (int r = 0; r < 9; r++) {
            double y[3];
            ba_mc_yrow(Z, r, f, y);
            double *dst = rhs + (row0 + r) * BA_MC_NR + 3 * i;
            dst[0] += y[0]; dst[1] += y[1]; dst[2] += y[2];
        }
    }
}

// ---- start of a batch --------------------------------------------------------------------------------------------------------------------
// thread (camera a, column c): x = 0, r = b, z = B_a^-1 b, p = 0; the workgroup's partials of r'z and |r|^2
__global__ __launch_bounds__(256) void k_mc_init(int N, const double *__restrict__ Minv, const double *__restrict__ rhs, double *__restrict__ x,
                                                 double *__restrict__ r, double *__restrict__ z, double *__restrict__ p,
                                                 double *__restrict__ part_rz, double *__restrict__ part_rr)
{
    __shared__ double sh[256];
    const int la = threadIdx.x / BA_MC_NR, c = threadIdx.x - BA_MC_NR * la, a = blockIdx.x * BA_MC_CPB + la;
    double rz = 0, rr = 0;
    if (la < BA_MC_CPB && a < N) {
        const double *Mi = Minv + (size_t)a * 81;
        const size_t o = 9 * (size_t)a * BA_MC_NR + c;
        double b[9];
#pragma unroll
        for (int q = 0; q < 9; q++) b[q] = rhs[o + BA_MC_NR * q];
#pragma unroll
        for (int i = 0; i < 9; i++) {
            const double zi = ba_dot9(Mi + 9 * i, b);
            x[o + BA_MC_NR * i] = 0; r[o + BA_MC_NR * i] = b[i]; z[o + BA_MC_NR * i] = zi; p[o + BA_MC_NR * i] = 0;
            rz += b[i] * zi;
            rr += b[i] * b[i];
        }
    }
    const double srz = ba_mc_block_cols(rz, sh), srr = ba_mc_block_cols(rr, sh);
    if (threadIdx.x < BA_MC_NR) {
        part_rz[(size_t)blockIdx.x * BA_MC_NR + threadIdx.x] = srz;
        part_rr[(size_t)blockIdx.x * BA_MC_NR + threadIdx.x] = srr;
    }
}

// One workgroup, behind k_mc_init (START) or behind iteration k's k_mc_update: r'z and |r|^2 per column; beta of the next iteration;
// the test |r| <= rel_tol |b| (a zero right-hand side is done at once, with 0 iterations).
template <bool START>
__global__ __launch_bounds__(256) void k_mc_scal(int k, int gm, const double *__restrict__ part_rz, const double *__restrict__ part_rr, double tol2,
                                                 ba_mc_dev *__restrict__ st)
{
    __shared__ double srz[BA_MC_NR], srr[BA_MC_NR];
    __shared__ int live;
    if (!START && st->alldone) return; // (uniform)
    ba_mc_sums(part_rz, gm, srz);
    ba_mc_sums(part_rr, gm, srr);
    if (threadIdx.x == 0) live = 0;
    __syncthreads();
    const int c = threadIdx.x;
    if (c < BA_MC_NR) {
        if (START) {
            st->bb[c] = srr[c]; st->rz[c] = srz[c]; st->rr[c] = srr[c]; st->beta[c] = 0; st->alpha[c] = 0; st->res[c] = 0;
            st->iters[c] = 0;
            const int d = !(srr[c] > 0) ? 1 : 0;
            st->done[c] = d;
            if (!d) live = 1; // (every writer stores the same value)
        } else if (!st->done[c]) {
            st->beta[c] = srz[c] / st->rz[c];
            st->rz[c] = srz[c];
            st->rr[c] = srr[c];
            st->iters[c] = k + 1;
            if (srr[c] <= tol2 * st->bb[c]) st->done[c] = 1;
            else live = 1;
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        if (START) { st->singular = 0; st->alldone = live ? 0 : 1; }
        else if (!live) st->alldone = 1;
    }
}

// ---- the product y = S v for nine columns (FINAL: v = x) ---------------------------------------------------------------------------------
// Point pass, 8 lanes per point: w_p[xyz][c] = dinv_p o sum_{o at p} Z_o^T v_cam(o)
template <bool FINAL>
__global__ __launch_bounds__(256) void k_mc_point(int Ml, const int *__restrict__ pt_ptr, const int *__restrict__ obs_cam, const double *__restrict__ rec,
                                                  const double *__restrict__ dinv, const double *__restrict__ z, const double *__restrict__ p,
                                                  const double *__restrict__ x, const ba_mc_dev *__restrict__ st, double *__restrict__ w)
{
    if (!FINAL && st->alldone) return; // (uniform)
    double beta[BA_MC_NR];
#pragma unroll
    for (int c = 0; c < BA_MC_NR; c++) beta[c] = FINAL ? 0.0 : st->beta[c];
    const int gid = (blockIdx.x * 256 + threadIdx.x) / 8, lg = threadIdx.x % 8;
    const bool ok = gid < Ml;
    const int b = ok ? pt_ptr[gid] : 0, e = ok ? pt_ptr[gid + 1] : 0;
    double s[3][BA_MC_NR];
#pragma unroll
    for (int q = 0; q < 3; q++)
#pragma unroll
        for (int c = 0; c < BA_MC_NR; c++) s[q][c] = 0;
    for (int i = b + lg; i < e; i += 8) {
        const double *Z = rec + (size_t)i * BA_REC;
        const size_t c0 = 9 * (size_t)obs_cam[i] * BA_MC_NR;
#pragma unroll
        for (int q = 0; q < 9; q++) {
            const double z0 = Z[3 * q], z1 = Z[3 * q + 1], z2 = Z[3 * q + 2];
#pragma unroll
            for (int c = 0; c < BA_MC_NR; c++) {
                const size_t o = c0 + BA_MC_NR * q + c;
                const double v = ba_pcg_dir<FINAL>(x, z, p, beta[c], o);
                s[0][c] += z0 * v; s[1][c] += z1 * v; s[2][c] += z2 * v;
            }
        }
    }
#pragma unroll
    for (int q = 0; q < 3; q++)
#pragma unroll
        for (int c = 0; c < BA_MC_NR; c++) s[q][c] = group_sum<double, 8>(s[q][c]);
    if (ok && lg == 0) {
        const size_t j = (size_t)gid, M = (size_t)Ml;
        const bool empty = b == e; // (no record ever wrote this point's dinv)
#pragma unroll
        for (int q = 0; q < 3; q++) {
            const double d = empty ? 0.0 : dinv[q * M + j];
#pragma unroll
            for (int c = 0; c < BA_MC_NR; c++) w[(3 * j + q) * BA_MC_NR + c] = empty ? 0.0 : d * s[q][c];
        }
    }
}

// Camera pass, part 1: per camera chunk of <= 32 observations (a 32-lane group, lane = observation) sum_o Z_o w_p(o) for the nine
// columns, row by row, a butterfly over the group, into slab[chunk][9 rows][NR]
template <bool FINAL>
__global__ __launch_bounds__(256) void k_mc_cam_chunks(int ndchunks, const int *__restrict__ dchunk_ptr, const int *__restrict__ cam_obs,
                                                       const int *__restrict__ obs_pt, const double *__restrict__ rec, const double *__restrict__ w,
                                                       double *__restrict__ slab, const ba_mc_dev *__restrict__ st)
{
    if (!FINAL && st->alldone) return; // (uniform)
    const int g = blockIdx.x * 8 + (threadIdx.x >> 5), sub = threadIdx.x & 31;
    const bool gok = g < ndchunks;
    const int e0 = gok ? dchunk_ptr[g] : 0, len = gok ? dchunk_ptr[g + 1] - e0 : 0;
    const bool have = sub < len;
    double Zr[27], wv[3][BA_MC_NR];
#pragma unroll
    for (int q = 0; q < 27; q++) Zr[q] = 0;
#pragma unroll
    for (int q = 0; q < 3; q++)
#pragma unroll
        for (int c = 0; c < BA_MC_NR; c++) wv[q][c] = 0;
    if (have) {
        const int o = cam_obs[e0 + sub];
        const size_t j = (size_t)obs_pt[o];
        const double *Z = rec + (size_t)o * BA_REC;
#pragma unroll
        for (int q = 0; q < 27; q++) Zr[q] = Z[q];
#pragma unroll
        for (int q = 0; q < 3; q++)
#pragma unroll
            for (int c = 0; c < BA_MC_NR; c++) wv[q][c] = w[(3 * j + q) * BA_MC_NR + c];
    }
#pragma unroll
    for (int r = 0; r < 9; r++) {
        double y[BA_MC_NR];
#pragma unroll
        for (int c = 0; c < BA_MC_NR; c++) y[c] = group_sum<double, 32>(Zr[3 * r] * wv[0][c] + Zr[3 * r + 1] * wv[1][c] + Zr[3 * r + 2] * wv[2][c]);
        if (gok && sub == 0) {
#pragma unroll
            for (int c = 0; c < BA_MC_NR; c++) slab[((size_t)g * 9 + r) * BA_MC_NR + c] = y[c];
        }
    }
}

// Camera pass, part 2, thread (camera a, column c): y_a = (V_a + lambda I) v_a - the camera's chunk partials (chunk order)
// [+ sum_b H_ab v_b over the camera's relative-pose constraints, RP], the identity in a fixed parameter's row; the workgroup's partials of v'y (FINAL: of |b - y|^2)
template <bool FINAL, bool RP>
__global__ __launch_bounds__(256) void k_mc_cam(int N, const int *__restrict__ cam_dchunk_ptr, const double *__restrict__ slab, const double *__restrict__ V,
                                                const double *__restrict__ lam, const double *__restrict__ z, const double *__restrict__ p,
                                                const double *__restrict__ x, const double *__restrict__ rhs, ba_relpose_csr<double> cs,
                                                const unsigned short *__restrict__ cmask, double *__restrict__ y, double *__restrict__ part, const ba_mc_dev *__restrict__ st)
{
    __shared__ double sh[256];
    if (!FINAL && st->alldone) return; // (uniform)
    const int la = threadIdx.x / BA_MC_NR, c = threadIdx.x - BA_MC_NR * la, a = blockIdx.x * BA_MC_CPB + la;
    double acc = 0;
    if (la < BA_MC_CPB && a < N) {
        const double beta = FINAL ? 0.0 : st->beta[c];
        const size_t o = 9 * (size_t)a * BA_MC_NR + c;
        double v[9], s[9];
#pragma unroll
        for (int q = 0; q < 9; q++) {
            v[q] = ba_pcg_dir<FINAL>(x, z, p, beta, o + BA_MC_NR * q);
            s[q] = 0;
        }
        for (int g = cam_dchunk_ptr[a], g1 = cam_dchunk_ptr[a + 1]; g < g1; g++) {
#pragma unroll
            for (int q = 0; q < 9; q++) s[q] += slab[((size_t)g * 9 + q) * BA_MC_NR + c];
        }
        const double *Va = V + (size_t)a * 81;
        const double lambda = *lam;
        const unsigned cm = cmask ? (unsigned)cmask[a] : 0u;
#pragma unroll
        for (int i = 0; i < 9; i++) {
            const double t = ba_dot9(Va + 9 * i, v);
            double yi = (t + lambda * v[i]) - s[i];
            if (RP)
                yi += ba_relpose_matvec_row<double>(cs, a, i, [&](size_t u) {
                    return ba_pcg_dir<FINAL>(x, z, p, beta, u * BA_MC_NR + c);
                });
            if ((cm >> i) & 1u) yi = v[i]; // a fixed parameter's row of the operator is the identity (v is 0 there throughout)
            y[o + BA_MC_NR * i] = yi;
            if (FINAL) { const double d = rhs[o + BA_MC_NR * i] - yi; acc += d * d; }
            else acc += v[i] * yi;
        }
    }
    const double sa = ba_mc_block_cols(acc, sh);
    if (threadIdx.x < BA_MC_NR) part[(size_t)blockIdx.x * BA_MC_NR + threadIdx.x] = sa;
}

// One workgroup behind k_mc_cam: p'Sp per column and alpha = r'z / p'Sp; a live column with p'Sp <= 0 or not finite raises the
// singular flag and ends the batch.  FINAL: |b - S x|^2 per column.
template <bool FINAL>
__global__ __launch_bounds__(256) void k_mc_alpha(int gm, const double *__restrict__ part, ba_mc_dev *__restrict__ st)
{
    __shared__ double sp[BA_MC_NR];
    if (!FINAL && st->alldone) return; // (uniform)
    ba_mc_sums(part, gm, sp);
    const int c = threadIdx.x;
    if (c >= BA_MC_NR) return;
    if (FINAL) { st->res[c] = sp[c]; return; }
    if (st->done[c]) return;
    const double py = sp[c];
    if (!(py > 0) || !(py < INFINITY)) { st->singular = 1; st->alldone = 1; return; } // (every writer stores the same value)
    st->alpha[c] = st->rz[c] / py;
}

// thread (camera a, column c): x += alpha p_k, r -= alpha S p_k, p <- p_k, z = B_a^-1 r; the workgroup's partials of r'z and |r|^2.
// A column that is done keeps its bits.
__global__ __launch_bounds__(256) void k_mc_update(int N, const double *__restrict__ Minv, const double *__restrict__ y, double *__restrict__ z,
                                                   double *__restrict__ p, double *__restrict__ x, double *__restrict__ r,
                                                   double *__restrict__ part_rz, double *__restrict__ part_rr, const ba_mc_dev *__restrict__ st)
{
    __shared__ double sh[256];
    if (st->alldone) return; // (uniform)
    const int la = threadIdx.x / BA_MC_NR, c = threadIdx.x - BA_MC_NR * la, a = blockIdx.x * BA_MC_CPB + la;
    double rz = 0, rr = 0;
    if (la < BA_MC_CPB && a < N && !st->done[c]) {
        const double beta = st->beta[c], alpha = st->alpha[c];
        const double *Mi = Minv + (size_t)a * 81;
        const size_t o = 9 * (size_t)a * BA_MC_NR + c;
        double rv[9];
#pragma unroll
        for (int q = 0; q < 9; q++) {
            const size_t oq = o + BA_MC_NR * q;
            const double pv = z[oq] + beta * p[oq];
            x[oq] += alpha * pv;
            p[oq] = pv;
            rv[q] = r[oq] - alpha * y[oq];
            r[oq] = rv[q];
        }
#pragma unroll
        for (int i = 0; i < 9; i++) {
            const double zi = ba_dot9(Mi + 9 * i, rv);
            z[o + BA_MC_NR * i] = zi;
            rz += rv[i] * zi;
            rr += rv[i] * rv[i];
        }
    }
    const double srz = ba_mc_block_cols(rz, sh), srr = ba_mc_block_cols(rr, sh);
    if (threadIdx.x < BA_MC_NR) {
        part_rz[(size_t)blockIdx.x * BA_MC_NR + threadIdx.x] = srz;
        part_rr[(size_t)blockIdx.x * BA_MC_NR + threadIdx.x] = srr;
    }
}

// ---- the blocks out of X -------------------------------------------------------------------------------------------------------------------
// The pairs served by column block b (order[lo .. hi) into the request): Sigma_ab = rows a of X for (a, b), its transpose for (b, a),
// (X_b + X_b^T) / 2 for (b, b); exact zeros in the rows and columns of fixed parameters.
__global__ __launch_bounds__(256) void k_mc_get_cams(int cnt, const int *__restrict__ order, const int *__restrict__ pairs, int b,
                                                     const double *__restrict__ x, const unsigned short *__restrict__ cmask, double *__restrict__ out)
{
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= cnt * 81) return;
    const int q = order[idx / 81], e = idx % 81, r = e / 9, c = e % 9;
    const int pa = pairs[2 * q], pb = pairs[2 * q + 1];
    const bool fixed = cmask && ((((unsigned)cmask[pa] >> r) | ((unsigned)cmask[pb] >> c)) & 1u);
    double v;
    if (pa == pb) v = 0.5 * (x[(9 * (size_t)b + r) * BA_MC_NR + c] + x[(9 * (size_t)b + c) * BA_MC_NR + r]);
    else if (pb == b) v = x[(9 * (size_t)pa + r) * BA_MC_NR + c];
    else v = x[(9 * (size_t)pb + c) * BA_MC_NR + r];
    out[(size_t)q * 81 + e] = fixed ? 0.0 : v;
}

// Sigma_pp = U_p^-1 + Y_p^T X_p for the batch's points (thread i: point i, columns 3 i .. 3 i + 2, its observations in order),
// symmetrised.  A fixed point: zeros.  A point nobody observes: I / lambda.
__global__ __launch_bounds__(64) void k_mc_get_pts(int np, const int *__restrict__ ids, const int *__restrict__ slots, int Ml, const int *__restrict__ pt_ptr,
                                                   const int *__restrict__ obs_cam, const double *__restrict__ rec, const double *__restrict__ dinv,
                                                   const double *__restrict__ tri, const unsigned char *__restrict__ pfix, const double *__restrict__ lam,
                                                   const double *__restrict__ x, double *__restrict__ out)
{
    const int i = threadIdx.x;
    if (i >= np) return;
    const int j = ids[i];
    double *o9 = out + 9 * (size_t)slots[i];
    double m[3][3];
#pragma unroll
    for (int u = 0; u < 3; u++)
#pragma unroll
        for (int v = 0; v < 3; v++) m[u][v] = 0;
    const int o0 = pt_ptr[j], o1 = pt_ptr[j + 1];
    if (pfix && pfix[j]) {
        for (int e = 0; e < 9; e++) o9[e] = 0.0;
        return;
    }
    if (o0 == o1) {
        const double il = 1.0 / *lam;
        for (int e = 0; e < 9; e++) o9[e] = (e % 4 == 0) ? il : 0.0;
        return;
    }
    const ba_mc_pt f = ba_mc_point_factor(j, Ml, tri, dinv);
    for (int o = o0; o < o1; o++) {
        const double *Z = rec + (size_t)o * BA_REC;
        const size_t row0 = 9 * (size_t)obs_cam[o];
        for (int r = 0; r < 9; r++) {
            double y[3];
            ba_mc_yrow(Z, r, f, y);
            const double *xr = x + (row0 + r) * BA_MC_NR + 3 * i;
#pragma unroll
            for (int u = 0; u < 3; u++)
#pragma unroll
                for (int v = 0; v < 3; v++) m[u][v] += y[u] * xr[v];
        }
    }
    // U^-1 = L^-T D^-1 L^-1
    const double Li[3][3] = {{1.0, 0.0, 0.0}, {f.li10, 1.0, 0.0}, {f.li20, f.li21, 1.0}};
    const double d[3] = {f.d0, f.d1, f.d2};
#pragma unroll
    for (int u = 0; u < 3; u++)
#pragma unroll
        for (int v = 0; v <= u; v++) {
            double ui = 0;
#pragma unroll
            for (int k = 0; k < 3; k++) ui += Li[k][u] * d[k] * Li[k][v];
            const double val = ui + 0.5 * (m[u][v] + m[v][u]);
            o9[3 * u + v] = val;
            o9[3 * v + u] = val;
        }
}

#endif
