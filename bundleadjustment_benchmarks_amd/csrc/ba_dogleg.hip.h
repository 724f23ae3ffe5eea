// ba_dogleg.hip.h -- kernels of Powell's dogleg for BA_CHOLESKY (ba_solver_dogleg_prepare / ba_solver_try_dogleg).
//
// Once per linearisation (prepare, behind the trial segments of ba_solver_try_step(mu)):
//   k_dogleg_dots   keeps a copy of the Gauss-Newton step and forms the block partials of |g|^2, |dx_gn|^2 and g'dx_gn
//   k_jg            block partials of q = |J g|^2 -- the one kernel here that reads all of J
// Per trial (try_dogleg):
//   k_dogleg_step   dx = a g + c dx_gn into the step buffers, xTest = x (+) dx, block partials of |dx|^2
// Every sum is accumulated in fp64 for both scalar types, per workgroup in the order of block_reduce, and the partial lists are summed by
// k_reduce_scalars<double> (thread k, k + 256, ...; tree inside a wave; waves in index order): no atomics, the same bits on every run.
#pragma once

#include "ba_kernels.hip.h"

// a g + c dx_gn in T.  a == 0 (the Gauss-Newton branch, c == 1): c * dx_gn alone, so that 1 * x returns x's bits (-0 included) whatever
// the gradient holds; one rounding per product and one for the sum otherwise (no contraction: the same bits on every call site).
template <typename T> __device__ __forceinline__ T ba_dogleg_combine(T a, T c, T g, T gn)
{
#pragma clang fp contract(off)
    if (a == (T)0) return c * gn;
    const T ag = a * g, cg = c * gn;
    return ag + cg;
}

// Element i of the step vector in the solver's device order: the points' SoA [3][Ml] first, then the cameras' 9N.  keep[i] = dx_gn[i];
// partial[0 .. 3)[grid] = block sums of g^2, dx_gn^2, g dx_gn.  A fixed parameter and a point nobody observes have g = dx_gn = 0.
template <typename T>
__global__ __launch_bounds__(256) void k_dogleg_dots(int n_pts3, int D, const T *__restrict__ gp, const T *__restrict__ gc, const T *__restrict__ dxp,
                                                     const T *__restrict__ dxc, T *__restrict__ keep, double *__restrict__ partial /* [3][grid] */)
{
    __shared__ double red[4];
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x, n = (size_t)n_pts3 + (size_t)D;
    double s_gg = 0, s_nn = 0, s_gn = 0;
    if (i < n) {
        const bool pt = i < (size_t)n_pts3;
        const T g = pt ? gp[i] : gc[i - n_pts3], x = pt ? dxp[i] : dxc[i - n_pts3];
        keep[i] = x;
        const double gd = (double)g, xd = (double)x;
        s_gg = gd * gd; s_nn = xd * xd; s_gn = gd * xd;
    }
    s_gg = block_reduce<double, false>(s_gg, red);
    s_nn = block_reduce<double, false>(s_nn, red);
    s_gn = block_reduce<double, false>(s_gn, red);
    if (threadIdx.x == 0) {
        const size_t gr = gridDim.x;
        partial[blockIdx.x] = s_gg; partial[gr + blockIdx.x] = s_nn; partial[2 * gr + blockIdx.x] = s_gn;
    }
}

// q = |J g|^2: one thread per observation in the solver's point-sorted order.  The observation's camera block comes in by 16-byte loads
// of its own AoS record (the way k_elim_chol reads it: the vector L1 merges a wavefront's loads into whole lines), the point block from
// the SoA rows (coalesced), the 9 + 3 entries of the full gradient by gather (consecutive observations share their point and, per
// camera, an L2-resident line).  y = J_c g_c + J_p g_p and |y|^2 in fp64 for both scalar types.  26 scalars and two indices per
// observation and 42 flops: bound by memory; 256-thread workgroups with a few dozen VGPRs keep every SIMD full of wavefronts.
template <typename T>
__global__ __launch_bounds__(256) void k_jg(int K, int Ml, const int *__restrict__ obs_cam, const int *__restrict__ obs_pt,
                                            const T *__restrict__ JcA /* [K][20] */, const T *__restrict__ Jp /* [6][K] */,
                                            const T *__restrict__ gc, const T *__restrict__ gp, double *__restrict__ partial /* [grid] */)
{
    __shared__ double red[4];
    const int i = blockIdx.x * 256 + threadIdx.x;
    double v = 0;
    if (i < K) {
        const int ci = obs_cam[i], pj = obs_pt[i];
        T A[18];
        {
            typedef T vec_t __attribute__((ext_vector_type(16 / sizeof(T))));
            constexpr int VW = 16 / sizeof(T);
            const vec_t *src = (const vec_t *)(JcA + (size_t)i * 20);
#pragma unroll
            for (int q = 0; q < 20 / VW; q++) {
                const vec_t w = src[q];
#pragma unroll
                for (int u = 0; u < VW; u++)
                    if (VW * q + u < 18) A[VW * q + u] = w[u];
            }
        }
        double y0 = 0, y1 = 0;
#pragma unroll
        for (int c = 0; c < 9; c++) {
            const double g = (double)gc[9 * (size_t)ci + c];
            y0 += (double)A[c] * g; y1 += (double)A[9 + c] * g;
        }
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const double g = (double)gp[(size_t)c * Ml + pj];
            y0 += (double)Jp[(size_t)c * K + i] * g; y1 += (double)Jp[(size_t)(3 + c) * K + i] * g;
        }
        v = y0 * y0 + y1 * y1;
    }
    v = block_reduce<double, false>(v, red);
    if (threadIdx.x == 0) partial[blockIdx.x] = v;
}

// dx = a g + c dx_gn (kept by k_dogleg_dots), written to the step buffers; points: xTest = x + dx, one thread per point, a fixed point and
// one nobody observes keep a zero step and a copy of x (k_backsub's treatment: the same bits, -0 included); cameras: the last block
// of the grid forms the camera rows of dx and hands them to ba_retract_cams, the device function behind every trial's retraction (its
// rho terms go to the slots of the trial's and are not read).  partial[0 .. npart] = block sums of |dx|^2 in fp64, the camera block last.
template <typename T, bool MASK>
__global__ __launch_bounds__(256) void k_dogleg_step(int Ml, int npart, T a, T c, const int *__restrict__ pt_ptr, const T *__restrict__ gp,
                                                     const T *__restrict__ gc, const T *__restrict__ keep, const T *__restrict__ pts,
                                                     T *__restrict__ dxp, T *__restrict__ dxc, T *__restrict__ pts_test, const T *__restrict__ lam,
                                                     double *__restrict__ partial /* [npart + 1] */, ba_cam_retract_args cr, ba_fix_args fx)
{
    __shared__ double redd[4];
    __shared__ T red[4];
    double dn = 0;
    if ((int)blockIdx.x == npart) {
        const T *kc = keep + 3 * (size_t)Ml;
        for (int cam = threadIdx.x; cam < cr.N; cam += 256) {
            const unsigned cm = MASK ? (unsigned)fx.cmask[cam] : 0u;
#pragma unroll
            for (int q = 0; q < 9; q++) {
                T d = ba_dogleg_combine<T>(a, c, gc[9 * (size_t)cam + q], kc[9 * (size_t)cam + q]);
                if (MASK && ((cm >> q) & 1u)) d = 0;
                dxc[9 * (size_t)cam + q] = d;
                dn += (double)d * (double)d;
            }
        }
        __syncthreads(); // (every camera's nine rows are read back below by the thread that wrote them; the barrier orders the rest)
        ba_retract_cams<T, MASK, false>(cr.N, (const T *)cr.cam, (const T *)dxc, (const T *)cr.gc, lam, (T *)cr.cam_test, (T *)cr.scal, cr.dst, red,
                                        fx.cmask, ba_damp_diag<T>{});
    } else {
        const int j = blockIdx.x * 256 + threadIdx.x;
        if (j < Ml) {
            const size_t M = (size_t)Ml;
            const bool still = pt_ptr[j] == pt_ptr[j + 1] || (MASK && fx.pfix[j] != 0);
#pragma unroll
            for (int q = 0; q < 3; q++) {
                const size_t o = q * M + j;
                const T x = pts[o];
                T d = 0;
                if (!still) d = ba_dogleg_combine<T>(a, c, gp[o], keep[o]);
                dxp[o] = d;
                pts_test[o] = still ? x : x + d;
                dn += (double)d * (double)d;
            }
        }
    }
    dn = block_reduce<double, false>(dn, redd);
    if (threadIdx.x == 0) partial[blockIdx.x] = dn;
}
