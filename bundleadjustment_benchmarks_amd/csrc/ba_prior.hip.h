// ba_prior.hip.h -- Gaussian priors on points, camera centres and intrinsics (ba_solver_set_*_priors).
//
// A prior is a handful of rows of J on ONE parameter block, so all it owes the normal equations is an addition to blocks the
// linearisation has already formed: U0 / gp of its point, the 9 x 9 block of V and the 9 entries of gc of its camera.  Everything
// behind those arrays (k_elim_chol, the Schur assembly, BA_ITERSCHUR's operator and preconditioner, k_backsub, the rho terms, the
// covariance) follows without code of its own.
//   point       e = L (X - X0)                                J = L                                   (3 x 3, point columns)
//   centre      e = L (C - C0),  C = -R^T T                   J = L [-R^T | -R^T [T]x | 0 0 0]        (3 x 9, camera columns T, omega, f, k1, k2)
//   intrinsics  e_q = w_q (x_q - x0_q),  q in (f, k1, k2)     J = w_q on column 6 + q
// (retraction of ba_retract_cams: T + dT, R <- Rodrigues(d omega) R, so dC = -R^T dT - R^T [T]x d omega).
// One thread per prior through compact lists: [0, npp) points, [npp, npp + npc) centres, then the intrinsics.  At most one prior of a
// type per point / camera, and the centre and the intrinsics prior of one camera touch disjoint entries of its block: no atomics.
// Every sum is in a fixed order (per thread sequentially, block_reduce across the workgroup), so a trial is the same bits eager,
// under ba_solver_try_step and replayed as a hipGraph.
#ifndef BA_PRIOR_HIP_H
#define BA_PRIOR_HIP_H

#include "ba_kernels.hip.h"

template <typename T> struct ba_prior_args {
    int npp, npc, npi;
    const int *pp_id, *pc_id, *pi_id;  // point of the shard / camera
    const T *pp_x0, *pp_L;             // [npp][3], [npp][9] row-major
    const T *pc_c0, *pc_L;             // [npc][3], [npc][9] row-major
    const T *pi_x0, *pi_w;             // [npi][3] each: f, k1, k2 in the solver's units; w = 0: no row
};

// e = L d and |e|^2 with one rounding per operation: the trial part and the linearisation part are two instantiations, and which
// product of a sum the compiler fuses is its choice per call site (see ba_pt_terms) -- an energy must be the same bits from both.
template <typename T> __device__ __forceinline__ T ba_prior_rows(const T (&L)[9], const T (&d)[3], T (&e)[3])
{
#pragma clang fp contract(off)
#pragma unroll
    for (int k = 0; k < 3; k++) e[k] = (L[3 * k] * d[0] + L[3 * k + 1] * d[1]) + L[3 * k + 2] * d[2];
    return (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2];
}
// d = C - C0 = -R^T T - C0.  A GNSS-grade prior pulls C to within a few sigma of C0, five or more digits below |C|: the plain sum
// would leave eps |R|'|T| / |d| in e (measured: 2e-4 of the centre energy in fp32, 1e-12 in fp64).  So the three products and the four
// additions are error-free transformations (fma for the product's tail, TwoSum for the sum's) and the tails are added at the end:
// d is good to eps |d| + eps^2 |R|'|T|.
template <typename T> __device__ __forceinline__ void ba_two_sum(T a, T b, T &s, T &err)
{
#pragma clang fp contract(off)
    s = a + b;
    const T bb = s - a;
    err = (a - (s - bb)) + (b - bb);
}
template <typename T> __device__ __forceinline__ void ba_prior_centre(const T (&R)[9], const T (&Tt)[3], const T *__restrict__ c0, T (&d)[3])
{
#pragma clang fp contract(off)
#pragma unroll
    for (int i = 0; i < 3; i++) {
        T s = -c0[i], tail = 0, e1;
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const T p = R[3 * k + i] * Tt[k];
            tail = tail - ba_fma(R[3 * k + i], Tt[k], -p); // (the product's rounding error, exactly)
            ba_two_sum<T>(s, -p, s, e1);
            tail = tail + e1;
        }
        d[i] = s + tail;
    }
}
template <typename T> __device__ __forceinline__ T ba_prior_intr(T w, T x, T x0, T &e2)
{
#pragma clang fp contract(off)
    const T e = w * (x - x0);
    e2 = e2 + e * e;
    return e;
}

// LIN = false (the trial part): the prior energy at cam / pts (xTest) as block partials part_e[3][gridDim.x] -- points, centres,
// intrinsics -- which the second stage sums behind k_eval's partials of the same array.
// LIN = true (the linearisation part, behind k_point_prep / k_cam_gram_reduce and in front of the first elimination): also adds J^T J
// and -J^T e into U0 / gp / V / gc in place, leaves the maxima of the point diagonals it touched in part_dmax[gridDim.x] (the camera
// diagonals are read from V by k_vdiag) and a second copy of the energy partials in part_keep (ba_solver_prior_energy: a trial
// overwrites part_e).  MASK: the columns of the parameters held constant are zero, by the mask words of k_eval<MASK>; such a prior
// still counts in the energy.
template <typename T, bool LIN, bool MASK = false>
__global__ __launch_bounds__(256) void k_prior(ba_prior_args<T> pa, int N, int Ml, const T *__restrict__ cam, const T *__restrict__ pts,
                                               T *__restrict__ U0, T *__restrict__ gp, T *__restrict__ V, T *__restrict__ gc,
                                               T *__restrict__ part_e, T *__restrict__ part_keep, T *__restrict__ part_dmax,
                                               const int *__restrict__ go, const unsigned short *__restrict__ cmask,
                                               const unsigned char *__restrict__ pfix)
{
    __shared__ T red[4];
    if (go && *go == 0) return; // (uniform) the trial in front of this linearisation was rejected
    const int t = blockIdx.x * 256 + threadIdx.x;
    T ep = 0, ec = 0, ei = 0, dm = 0;
    if (t < pa.npp) {
        const int j = pa.pp_id[t];
        const size_t M = (size_t)Ml;
        T L[9], d[3], e[3];
#pragma unroll
        for (int q = 0; q < 9; q++) L[q] = pa.pp_L[9 * (size_t)t + q];
#pragma unroll
        for (int q = 0; q < 3; q++) d[q] = pts[q * M + j] - pa.pp_x0[3 * (size_t)t + q];
        ep = ba_prior_rows<T>(L, d, e);
        if (LIN && !(MASK && pfix[j] != 0)) {
            int u = 0;
#pragma unroll
            for (int r = 0; r < 3; r++)
#pragma unroll
                for (int c = r; c < 3; c++, u++) { // 00 01 02 11 12 22
                    const T s = U0[u * M + j] + (L[r] * L[c] + L[3 + r] * L[3 + c] + L[6 + r] * L[6 + c]);
                    U0[u * M + j] = s;
                    if (r == c) dm = tmax(dm, s);
                }
#pragma unroll
            for (int r = 0; r < 3; r++) gp[r * M + j] = gp[r * M + j] - (L[r] * e[0] + L[3 + r] * e[1] + L[6 + r] * e[2]);
        }
    } else if (t < pa.npp + pa.npc) {
        const int u = t - pa.npp, a = pa.pc_id[u];
        T R[9], Tt[3], L[9], d[3], e[3];
#pragma unroll
        for (int q = 0; q < 9; q++) { R[q] = cam[(size_t)q * N + a]; L[q] = pa.pc_L[9 * (size_t)u + q]; }
#pragma unroll
        for (int q = 0; q < 3; q++) Tt[q] = cam[(size_t)(9 + q) * N + a];
        ba_prior_centre<T>(R, Tt, pa.pc_c0 + 3 * (size_t)u, d);
        ec = ba_prior_rows<T>(L, d, e);
        if (LIN) {
            // dC / d(T, omega) = [-R^T | -R^T [T]x]
            const T Tx[9] = {0, -Tt[2], Tt[1], Tt[2], 0, -Tt[0], -Tt[1], Tt[0], 0};
            T Jd[3][6], G[3][6];
#pragma unroll
            for (int i = 0; i < 3; i++)
#pragma unroll
                for (int c = 0; c < 3; c++) {
                    Jd[i][c] = -R[3 * c + i];
                    Jd[i][3 + c] = -(R[i] * Tx[c] + R[3 + i] * Tx[3 + c] + R[6 + i] * Tx[6 + c]);
                }
            const unsigned cm = MASK ? (unsigned)cmask[a] : 0u;
#pragma unroll
            for (int k = 0; k < 3; k++)
#pragma unroll
                for (int c = 0; c < 6; c++) {
                    const T g = L[3 * k] * Jd[0][c] + L[3 * k + 1] * Jd[1][c] + L[3 * k + 2] * Jd[2][c];
                    G[k][c] = (MASK && ((cm >> c) & 1u)) ? (T)0 : g;
                }
            T *Va = V + (size_t)a * 81;
#pragma unroll
            for (int r = 0; r < 6; r++) {
#pragma unroll
                for (int c = 0; c <= r; c++) { // the lower triangle, mirrored: V stays symmetric in bits
                    const T s = Va[9 * r + c] + (G[0][r] * G[0][c] + G[1][r] * G[1][c] + G[2][r] * G[2][c]);
                    Va[9 * r + c] = s;
                    Va[9 * c + r] = s;
                }
                gc[9 * a + r] = gc[9 * a + r] - (G[0][r] * e[0] + G[1][r] * e[1] + G[2][r] * e[2]);
            }
        }
    } else if (t < pa.npp + pa.npc + pa.npi) {
        const int u = t - pa.npp - pa.npc, a = pa.pi_id[u];
        const unsigned cm = (LIN && MASK) ? (unsigned)cmask[a] : 0u;
#pragma unroll
        for (int q = 0; q < 3; q++) {
            const T w = pa.pi_w[3 * (size_t)u + q];
            const T e = ba_prior_intr<T>(w, cam[(size_t)(12 + q) * N + a], pa.pi_x0[3 * (size_t)u + q], ei);
            if (LIN && !(MASK && ((cm >> (6 + q)) & 1u))) {
                V[(size_t)a * 81 + 10 * (6 + q)] = V[(size_t)a * 81 + 10 * (6 + q)] + w * w;
                gc[9 * a + 6 + q] = gc[9 * a + 6 + q] - w * e;
            }
        }
    }
    const size_t g = gridDim.x;
    ep = block_reduce<T, false>(ep, red);
    ec = block_reduce<T, false>(ec, red);
    ei = block_reduce<T, false>(ei, red);
    if (LIN) dm = block_reduce<T, true>(dm, red);
    if (threadIdx.x == 0) {
        part_e[blockIdx.x] = ep; part_e[g + blockIdx.x] = ec; part_e[2 * g + blockIdx.x] = ei;
        if (LIN) {
            part_keep[blockIdx.x] = ep; part_keep[g + blockIdx.x] = ec; part_keep[2 * g + blockIdx.x] = ei;
            part_dmax[blockIdx.x] = dm;
        }
    }
}

// A point nobody observes has no elimination record and k_backsub leaves it where it is -- right without a prior (its block is
// lambda I, its gradient 0).  With a point prior its block is L'L + lambda I and its gradient -L'e: this kernel, behind k_backsub and
// only when such points are listed, takes their step (U0 + lambda I) dx = gp by the 3 x 3 LDL^T of k_elim_chol, retracts them and
// adds their rho and |dx|^2 terms to the partials of k_backsub's block 0.  One workgroup; a fixed point keeps k_backsub's copy.
// MARQ (ba_solver_set_damping): the pivots and the rho terms take d_q = fl(lambda clamp(U0[0, 3, 5])) of the point instead of lambda.
template <typename T, bool MASK, bool MARQ>
__device__ __forceinline__ void ba_prior_lonely(int n, const int *__restrict__ ids, int Ml, const T *__restrict__ U0, const T *__restrict__ gp,
                                                const T *__restrict__ lam, const T *__restrict__ pts, T *__restrict__ dxp,
                                                T *__restrict__ pts_test, T *__restrict__ partial, int npart,
                                                const unsigned char *__restrict__ pfix, ba_damp_args<T> da)
{
    __shared__ T red[4];
    const size_t M = (size_t)Ml;
    const T lambda = *lam;
    T rho = 0, dn = 0;
    for (int q = threadIdx.x; q < n; q += 256) {
        const int j = ids[q];
        if (MASK && pfix[j] != 0) continue;
        const T g0 = gp[j], g1 = gp[M + j], g2 = gp[2 * M + j];
        T d0 = lambda, d1 = lambda, d2 = lambda;
        if constexpr (MARQ) { d0 = ba_damp<true, T>(lambda, U0[j], da); d1 = ba_damp<true, T>(lambda, U0[3 * M + j], da); d2 = ba_damp<true, T>(lambda, U0[5 * M + j], da); }
        const ba_chol3_t<T> c3 = ba_chol3<T>(U0[j], U0[M + j], U0[2 * M + j], U0[3 * M + j], U0[4 * M + j], U0[5 * M + j], g0, g1, g2, d0, d1, d2);
        const T x2 = c3.t2 * c3.i2;
        const T x1 = c3.t1 * c3.i1 - c3.l21 * x2;
        const T x0 = c3.t0 * c3.i0 - c3.l10 * x1 - c3.l20 * x2;
        dxp[j] = x0; dxp[M + j] = x1; dxp[2 * M + j] = x2;
        pts_test[j] = pts[j] + x0; pts_test[M + j] = pts[M + j] + x1; pts_test[2 * M + j] = pts[2 * M + j] + x2;
        rho += x0 * (d0 * x0 + g0) + x1 * (d1 * x1 + g1) + x2 * (d2 * x2 + g2);
        dn += x0 * x0 + x1 * x1 + x2 * x2;
    }
    rho = block_reduce<T, false>(rho, red);
    dn = block_reduce<T, false>(dn, red);
    if (threadIdx.x == 0) { partial[0] = partial[0] + rho; partial[npart] = partial[npart] + dn; }
}
template <typename T, bool MASK = false>
__global__ __launch_bounds__(256) void k_prior_lonely(int n, const int *__restrict__ ids, int Ml, const T *__restrict__ U0, const T *__restrict__ gp,
                                                      const T *__restrict__ lam, const T *__restrict__ pts, T *__restrict__ dxp,
                                                      T *__restrict__ pts_test, T *__restrict__ partial, int npart,
                                                      const unsigned char *__restrict__ pfix)
{
    ba_prior_lonely<T, MASK, false>(n, ids, Ml, U0, gp, lam, pts, dxp, pts_test, partial, npart, pfix, ba_damp_args<T>{});
}
// (a kernel of its own: k_prior_lonely keeps its parameter list)
template <typename T, bool MASK = false>
__global__ __launch_bounds__(256) void k_prior_lonely_marq(int n, const int *__restrict__ ids, int Ml, const T *__restrict__ U0, const T *__restrict__ gp,
                                                           const T *__restrict__ lam, const T *__restrict__ pts, T *__restrict__ dxp,
                                                           T *__restrict__ pts_test, T *__restrict__ partial, int npart,
                                                           const unsigned char *__restrict__ pfix, ba_damp_args<T> da)
{
    ba_prior_lonely<T, MASK, true>(n, ids, Ml, U0, gp, lam, pts, dxp, pts_test, partial, npart, pfix, da);
}

#endif
