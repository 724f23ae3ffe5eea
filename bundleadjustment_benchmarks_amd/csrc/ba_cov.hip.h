// ba_cov.hip.h -- covariance blocks of cameras and points (ba_solver_covariance_compute / _get), gfx950.
//
// With H = J^T J + lambda I on the free parameters, Sigma = H^-1.  By the Schur complement the camera part is S^-1 (S: the reduced
// camera matrix the LM trial assembles) and a point's block is U_p^-1 + U_p^-1 (sum_ab W_ap^T Sigma_ab W_bp) U_p^-1.
//
// The inverse rides the dense LDL^T (ba_dense.hip.h, unchanged) as extra rows: the factorisation turns a row b^T stacked under the
// matrix into (D^-1 L^-1 b)^T, so E = diag(s) stacked under the scaled matrix E S E (s_i = S_ii^-1/2, 0 for a fixed parameter) comes
// out as B = E L^-T D^-1 -- upper triangular -- and
//     Sigma_cc = B D B^T,       Sigma_ij = sum_{k >= max(i, j)} B_ik d_k B_jk,
// one symmetric rank-D update on the matrix cores (k_cov_syrk: 64 x 64 tiles of the lower triangle, the k loop of a tile row starts
// at its own first column).  Layout of the work buffer C (column-major, ldc rows): rows [0, D) the scaled matrix, then L and D, then
// -- written by k_cov_syrk over L -- the lower triangle of Sigma_cc; rows [Dp, Dp + D) the stacked E, then B.
//
//   k_cov_fixed_records  the elimination's records of fixed points = 0 (lambda = 0: U_p = 0 is never inverted)
//   k_cov_scale    s and the staging's singularity test (a free diagonal entry <= 0)
//   k_cov_stage    scaled lower triangle + unit diagonal of the fixed rows + the stacked E
//   k_cov_diag     the pivots d_k = s_k / B_kk, the test pivot > 0 (device flag word)
//   k_cov_syrk     Sigma_cc = B D B^T
//   k_cov_points_check / k_cov_points    every free point's U_p is positive definite / the blocks of the points asked for
//   k_cov_get_cams the camera blocks asked for (the upper triangle is read as the transpose of the lower: Sigma_ab == Sigma_ba^T in bits)
// No workgroup waits for another one, no atomics: the same bits run after run.
#ifndef BA_COV_HIP_H
#define BA_COV_HIP_H

#include "ba_mfma.hip.h"

// A fixed point takes no part in the elimination: its Jp is zero, so its records are zero whenever U_p = lambda I can be inverted -- and
// 0 / 0 at lambda = 0.  Behind the elimination kernels (unchanged) its observations' records and its own factors are set to the zeros
// they stand for; the next trial's elimination writes them again.
template <typename T>
__global__ __launch_bounds__(256) void k_cov_fixed_records(int K, int Ml, int rec_len, const int *__restrict__ obs_pt, const unsigned char *__restrict__ pfix,
                                                           T *__restrict__ rec, T *__restrict__ dinv, T *__restrict__ tvec, T *__restrict__ tri)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < K && pfix[obs_pt[i]])
        for (int q = 0; q < rec_len; q++) rec[(size_t)i * rec_len + q] = (T)0;
    if (i < Ml && pfix[i]) {
        for (int q = 0; q < 3; q++) { dinv[(size_t)q * Ml + i] = (T)0; tvec[(size_t)q * Ml + i] = (T)0; }
        for (int q = 0; q < 6; q++) tri[(size_t)q * Ml + i] = (T)0;
    }
}

// one workgroup of 256 threads per 256 parameters
template <typename T>
__global__ __launch_bounds__(256) void k_cov_scale(int D, int ld, const T *__restrict__ S, const unsigned short *__restrict__ cmask,
                                                   T *__restrict__ sc, int *__restrict__ flag)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= D) return;
    if (cmask && ((cmask[i / 9] >> (i % 9)) & 1)) { sc[i] = (T)0; return; }
    const T d = S[(size_t)i * ld + i];
    if (!(d > (T)0) || !(d < (T)INFINITY)) { *flag = 1; sc[i] = (T)1; return; } // (every writer stores the same value)
    sc[i] = (T)1 / sqrt(d);
}

// column j of the work buffer (zeroed before): rows [j, D) of the scaled matrix, the stacked row Dp + j.  Columns [D, 64 ceil(D / 64))
// pad the last block column with unit pivots: the panel step only carries the rows below a FULL block column along.
template <typename T>
__global__ __launch_bounds__(256) void k_cov_stage(int D, int Dp, int ld, const T *__restrict__ S, const T *__restrict__ sc, int ldc, T *__restrict__ C)
{
    const int j = blockIdx.x;
    if (j >= D) {
        if (threadIdx.x == 0) C[(size_t)j * ldc + j] = (T)1;
        return;
    }
    const T sj = sc[j];
    for (int i = j + threadIdx.x; i < D; i += 256) {
        const T si = sc[i];
        T v;
        if (si == (T)0 || sj == (T)0) v = i == j ? (T)1 : (T)0; // a fixed parameter: unit diagonal, decoupled
        else v = si * sj * S[(size_t)j * ld + i];
        C[(size_t)j * ldc + i] = v;
    }
    if (threadIdx.x == 0) C[(size_t)j * ldc + Dp + j] = sj;
}

// The pivots.  The panel step does not write a factored diagonal block back (nobody reads it again), so d_k comes out of the stacked
// rows: B_kk = s_k / d_k.  A fixed parameter's pivot is the unit diagonal it was given (its row and column of B are zero).
template <typename T>
__global__ __launch_bounds__(256) void k_cov_diag(int D, int Dp, int ldc, const T *__restrict__ C, const T *__restrict__ sc, T *__restrict__ dv,
                                                  int *__restrict__ flag)
{
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= Dp) return;
    T d = (T)0;
    if (k < D) {
        d = (T)1;
        if (sc[k] != (T)0) {
            const T bkk = C[(size_t)k * ldc + Dp + k];
            if (!(bkk > (T)0) || !(bkk < (T)INFINITY)) *flag = 1;
            d = sc[k] / bkk;
        }
    }
    dv[k] = d;
}

// Sigma tile (ti, tj), tj <= ti, of the lower triangle: wave w owns a 32 x 32 quadrant (2 x 2 accumulators), operands straight from
// L2 with eight k-steps in flight -- the shape of ba_update_quad.  The MFMA forms the transposed tile, so that the 16-wide index of the
// C/D fragment runs along the rows of the column-major buffer.  Workgroups in tile-row order: the long k loops first.
template <typename T>
__global__ __launch_bounds__(256) void k_cov_syrk(int D, int Dp, int ldc, T *__restrict__ C, const T *__restrict__ dv)
{
    int u = blockIdx.x, ti = 0;
    for (; u > ti; ti++) u -= ti + 1;
    const int tj = u;
    const int quad = threadIdx.x >> 6, lane = threadIdx.x & 63, li = lane & 15, lk = lane >> 4;
    const int qr = 32 * (quad >> 1), qc = 32 * (quad & 1);
    if (ti == tj && qc > qr) return;
    const int row0 = 64 * ti + qr, col0 = 64 * tj + qc;
    const T *__restrict__ B = C + Dp; // B_ik = B[k * ldc + i]
    typename ba_acc<T>::type acc[2][2];
#pragma unroll
    for (int t = 0; t < 2; t++)
#pragma unroll
        for (int w = 0; w < 2; w++)
#pragma unroll
            for (int v = 0; v < 4; v++) acc[t][w][v] = (T)0;
    constexpr int CH = 8;
    for (int k0 = 64 * ti; k0 < Dp; k0 += 4 * CH) { // (B_ik = 0 for k < i: nothing in front of the tile row's first column)
        T a[CH][2], b[CH][2];
#pragma unroll
        for (int q = 0; q < CH; q++) {
            const int k = k0 + 4 * q + lk;
            const T dk = dv[k];
            const T *col = B + (size_t)k * ldc;
#pragma unroll
            for (int t = 0; t < 2; t++) a[q][t] = col[col0 + 16 * t + li] * dk; // A[j][k] = B_jk d_k
#pragma unroll
            for (int w = 0; w < 2; w++) b[q][w] = col[row0 + 16 * w + li];      // B[k][i] = B_ik
        }
#pragma unroll
        for (int q = 0; q < CH; q++)
#pragma unroll
            for (int t = 0; t < 2; t++)
#pragma unroll
                for (int w = 0; w < 2; w++) acc[t][w] = ba_mfma(a[q][t], b[q][w], acc[t][w]);
    }
#pragma unroll
    for (int t = 0; t < 2; t++)
#pragma unroll
        for (int w = 0; w < 2; w++)
#pragma unroll
            for (int v = 0; v < 4; v++) {
                const int cc = col0 + 16 * t + ba_crow<T>(lk, v), rr = row0 + 16 * w + li;
                if (rr < D && cc <= rr) C[(size_t)cc * ldc + rr] = acc[t][w][v];
            }
}

// entry (i, j) of Sigma_cc out of the lower triangle
template <typename T> __device__ __forceinline__ T ba_cov_sigma(const T *__restrict__ C, int ldc, int i, int j)
{
    return i >= j ? C[(size_t)j * ldc + i] : C[(size_t)i * ldc + j];
}

template <typename T>
__global__ __launch_bounds__(256) void k_cov_get_cams(int n_pairs, const int *__restrict__ pairs, int ldc, const T *__restrict__ C,
                                                      const unsigned short *__restrict__ cmask, double *__restrict__ out)
{
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)n_pairs * 81) return;
    const int q = (int)(idx / 81), e = (int)(idx % 81), r = e / 9, c = e % 9;
    const int a = pairs[2 * q], b = pairs[2 * q + 1];
    const bool fixed = cmask && ((((unsigned)cmask[a] >> r) | ((unsigned)cmask[b] >> c)) & 1u);
    out[idx] = fixed ? 0.0 : (double)ba_cov_sigma<T>(C, ldc, 9 * a + r, 9 * b + c);
}

// ---- points --------------------------------------------------------------------------------------------------------------------------
// An observation's blocks out of the linearisation (the result stays readable behind later trials, which overwrite the elimination's
// records but not J).  AOS: CHOLESKY's camera records [K][20]; else [18][K].  Jp: [6][K].
template <typename T, bool AOS>
__device__ __forceinline__ void ba_cov_obs(int i, int K, const T *__restrict__ Jc, const T *__restrict__ Jp, T (&G)[9][3])
{
    T c[18], p[6];
#pragma unroll
    for (int q = 0; q < 18; q++) c[q] = AOS ? Jc[(size_t)20 * i + q] : Jc[(size_t)q * K + i];
#pragma unroll
    for (int q = 0; q < 6; q++) p[q] = Jp[(size_t)q * K + i];
#pragma unroll
    for (int r = 0; r < 9; r++)
#pragma unroll
        for (int x = 0; x < 3; x++) G[r][x] = c[r] * p[x] + c[9 + r] * p[3 + x]; // Jc^T Jp
}

// U = sum Jp^T Jp + lambda I as (xx, xy, xz, yy, yz, zz), and its LDL^T: false when a pivot is not positive
template <typename T> struct ba_cov_u3 { T l10, l20, l21, d0, d1, d2; };
template <typename T> __device__ __forceinline__ bool ba_cov_ldl3(const T (&U)[6], ba_cov_u3<T> &f)
{
    f.d0 = U[0];
    f.l10 = U[1] / f.d0; f.l20 = U[2] / f.d0;
    f.d1 = U[3] - f.l10 * U[1];
    f.l21 = (U[4] - f.l20 * U[1]) / f.d1;
    f.d2 = U[5] - f.l20 * U[2] - f.l21 * f.l21 * f.d1;
    return f.d0 > (T)0 && f.d1 > (T)0 && f.d2 > (T)0 && f.d2 < (T)INFINITY;
}
// x = U^-1 b
template <typename T> __device__ __forceinline__ void ba_cov_solve3(const ba_cov_u3<T> &f, const T (&b)[3], T (&x)[3])
{
    const T y0 = b[0], y1 = b[1] - f.l10 * y0, y2 = b[2] - f.l20 * y0 - f.l21 * y1;
    x[2] = y2 / f.d2;
    x[1] = y1 / f.d1 - f.l21 * x[2];
    x[0] = y0 / f.d0 - f.l10 * x[1] - f.l20 * x[2];
}

template <typename T>
__device__ __forceinline__ void ba_cov_point_u(int o0, int o1, int K, const T *__restrict__ Jp, T lambda, int lane, int nl, T (&U)[6])
{
#pragma unroll
    for (int q = 0; q < 6; q++) U[q] = (T)0;
    for (int i = o0 + lane; i < o1; i += nl) {
        T p[6];
#pragma unroll
        for (int q = 0; q < 6; q++) p[q] = Jp[(size_t)q * K + i];
        U[0] += p[0] * p[0] + p[3] * p[3]; U[1] += p[0] * p[1] + p[3] * p[4]; U[2] += p[0] * p[2] + p[3] * p[5];
        U[3] += p[1] * p[1] + p[4] * p[4]; U[4] += p[1] * p[2] + p[4] * p[5]; U[5] += p[2] * p[2] + p[5] * p[5];
    }
    if (nl > 1) {
#pragma unroll
        for (int q = 0; q < 6; q++) U[q] = ba_wave_sum_all<T>(U[q]);
    }
    U[0] += lambda; U[3] += lambda; U[5] += lambda;
}

// U0 = the linearisation's own [6][Ml] blocks (k_point_prep + the point priors, ba_prior.hip.h) instead of the sum over Jp: a solver with
// priors has rows of J that are in no observation
template <typename T> __device__ __forceinline__ void ba_cov_point_u0(int j, int Ml, const T *__restrict__ U0, T lambda, T (&U)[6])
{
#pragma unroll
    for (int q = 0; q < 6; q++) U[q] = U0[(size_t)q * Ml + j];
    U[0] += lambda; U[3] += lambda; U[5] += lambda;
}
template <typename T>
__global__ __launch_bounds__(256) void k_cov_points_check_u0(int Ml, const T *__restrict__ U0, const unsigned char *__restrict__ pfix,
                                                             const T *__restrict__ lam, int *__restrict__ flag)
{
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= Ml || (pfix && pfix[j])) return;
    T U[6];
    ba_cov_point_u0<T>(j, Ml, U0, *lam, U);
    ba_cov_u3<T> f;
    if (!ba_cov_ldl3<T>(U, f)) *flag = 1;
}

// every free point: U_p positive definite, or the flag word (one thread per point)
template <typename T>
__global__ __launch_bounds__(256) void k_cov_points_check(int Ml, int K, const int *__restrict__ pt_ptr, const T *__restrict__ Jp,
                                                          const unsigned char *__restrict__ pfix, const T *__restrict__ lam, int *__restrict__ flag)
{
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= Ml || (pfix && pfix[j])) return;
    T U[6];
    ba_cov_point_u<T>(pt_ptr[j], pt_ptr[j + 1], K, Jp, *lam, 0, 1, U);
    ba_cov_u3<T> f;
    if (!ba_cov_ldl3<T>(U, f)) *flag = 1;
}

// One wavefront per point asked for: M = sum over the pairs (o, o') of its track of G_o^T Sigma_{c(o) c(o')} G_o' (the lanes stride
// over the pairs, a fixed-order wave sum closes it), then Sigma_pp = U^-1 + U^-1 M U^-1, symmetrised.  A fixed point: zeros.
// (FROMU0: U of the point from the linearisation's blocks, k_cov_points_u0 below)
template <typename T, bool AOS, bool FROMU0>
__device__ __forceinline__ void ba_cov_points_body(int n_pts, const int *__restrict__ ids, int K, const int *__restrict__ pt_ptr,
                                                   const int *__restrict__ obs_cam, const T *__restrict__ Jc, const T *__restrict__ Jp,
                                                   const unsigned char *__restrict__ pfix, T lambda, int ldc, const T *__restrict__ C,
                                                   double *__restrict__ out, const T *__restrict__ U0, int Ml)
{
    const int j = ids[blockIdx.x], lane = threadIdx.x;
    double *o9 = out + (size_t)9 * blockIdx.x;
    if (pfix && pfix[j]) {
        if (lane < 9) o9[lane] = 0.0;
        return;
    }
    const int o0 = pt_ptr[j], o1 = pt_ptr[j + 1], t = o1 - o0;
    T U[6];
    if constexpr (FROMU0) ba_cov_point_u0<T>(j, Ml, U0, lambda, U);
    else ba_cov_point_u<T>(o0, o1, K, Jp, lambda, lane, 64, U);
    T m[3][3];
#pragma unroll
    for (int x = 0; x < 3; x++)
#pragma unroll
        for (int y = 0; y < 3; y++) m[x][y] = (T)0;
    const long long npair = (long long)t * t;
    for (long long q = lane; q < npair; q += 64) {
        const int i1 = o0 + (int)(q / t), i2 = o0 + (int)(q % t);
        T G1[9][3], G2[9][3], v[9][3];
        ba_cov_obs<T, AOS>(i1, K, Jc, Jp, G1);
        ba_cov_obs<T, AOS>(i2, K, Jc, Jp, G2);
        const int a = 9 * obs_cam[i1], b = 9 * obs_cam[i2];
#pragma unroll
        for (int r = 0; r < 9; r++) {
            T s[9];
#pragma unroll
            for (int c = 0; c < 9; c++) s[c] = ba_cov_sigma<T>(C, ldc, a + r, b + c);
#pragma unroll
            for (int y = 0; y < 3; y++) {
                T acc = (T)0;
#pragma unroll
                for (int c = 0; c < 9; c++) acc += s[c] * G2[c][y];
                v[r][y] = acc;
            }
        }
#pragma unroll
        for (int x = 0; x < 3; x++)
#pragma unroll
            for (int y = 0; y < 3; y++) {
                T acc = (T)0;
#pragma unroll
                for (int r = 0; r < 9; r++) acc += G1[r][x] * v[r][y];
                m[x][y] += acc;
            }
    }
#pragma unroll
    for (int x = 0; x < 3; x++)
#pragma unroll
        for (int y = 0; y < 3; y++) m[x][y] = ba_wave_sum_all<T>(m[x][y]);
    if (lane != 0) return;
    ba_cov_u3<T> f;
    (void)ba_cov_ldl3<T>(U, f); // (positive definite: k_cov_points_check saw every free point at compute time)
    // Ui = U^-1 column by column; Y = M_sym Ui; R = Ui + Ui^T Y
    T Ui[3][3], Y[3][3], R[3][3];
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const T e[3] = {c == 0 ? (T)1 : (T)0, c == 1 ? (T)1 : (T)0, c == 2 ? (T)1 : (T)0};
        T x[3];
        ba_cov_solve3<T>(f, e, x);
#pragma unroll
        for (int r = 0; r < 3; r++) Ui[r][c] = x[r];
    }
#pragma unroll
    for (int x = 0; x < 3; x++)
#pragma unroll
        for (int y = 0; y < 3; y++) {
            T acc = (T)0;
#pragma unroll
            for (int k = 0; k < 3; k++) acc += (T)0.5 * (m[x][k] + m[k][x]) * Ui[k][y];
            Y[x][y] = acc;
        }
#pragma unroll
    for (int x = 0; x < 3; x++)
#pragma unroll
        for (int y = 0; y < 3; y++) {
            T acc = Ui[x][y];
#pragma unroll
            for (int k = 0; k < 3; k++) acc += Ui[k][x] * Y[k][y];
            R[x][y] = acc;
        }
#pragma unroll
    for (int x = 0; x < 3; x++)
#pragma unroll
        for (int y = 0; y < 3; y++) o9[3 * x + y] = (double)((T)0.5 * (R[x][y] + R[y][x]));
}
template <typename T, bool AOS>
__global__ __launch_bounds__(64) void k_cov_points(int n_pts, const int *__restrict__ ids, int K, const int *__restrict__ pt_ptr,
                                                   const int *__restrict__ obs_cam, const T *__restrict__ Jc, const T *__restrict__ Jp,
                                                   const unsigned char *__restrict__ pfix, T lambda, int ldc, const T *__restrict__ C,
                                                   double *__restrict__ out)
{
    ba_cov_points_body<T, AOS, false>(n_pts, ids, K, pt_ptr, obs_cam, Jc, Jp, pfix, lambda, ldc, C, out, (const T *)nullptr, 0);
}
template <typename T, bool AOS>
__global__ __launch_bounds__(64) void k_cov_points_u0(int n_pts, const int *__restrict__ ids, int K, const int *__restrict__ pt_ptr,
                                                      const int *__restrict__ obs_cam, const T *__restrict__ Jc, const T *__restrict__ Jp,
                                                      const unsigned char *__restrict__ pfix, T lambda, int ldc, const T *__restrict__ C,
                                                      double *__restrict__ out, const T *__restrict__ U0, int Ml)
{
    ba_cov_points_body<T, AOS, true>(n_pts, ids, K, pt_ptr, obs_cam, Jc, Jp, pfix, lambda, ldc, C, out, U0, Ml);
}

#endif
