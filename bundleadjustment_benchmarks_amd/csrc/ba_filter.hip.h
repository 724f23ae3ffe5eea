// ba_filter.hip.h -- the observation filter (ba_solver_filter_observations / ba_filter_track; include/ba_mi355x.h):
// COLMAP's FilterObservations / FilterPoints rule on the resident state.  As in ba_triangulate.hip.h the per-point rule is written ONCE
// here, for L cooperating lanes, a reader of the point's track and a reducer over the lanes: the host function (ba_filter.cpp) runs it
// with L = 1, the kernels below with L = 8 lanes of one wavefront per point.  All geometry is fp64 for both scalar types; the resident
// state is read as stored.
//
// Model (k_eval, ba_problem.cpp): XX = R X + T, xu = XX_01 / XX_2, kr = 1 + k1 |xu|^2 + k2 |xu|^4, pi = f kr xu; the camera looks
// down -z: X is in front of it iff XX_2 < 0.  A camera is the 15 scalars of BA_GET_CAMS: R row-major, T, f, k1, k2.
//
// Two passes.  The first (ba_flt_observation) is per observation and stores its status, its pixel error and the ray from the CURRENT
// point to the camera centre; the second (ba_flt_point) reads what the first has stored -- so that in a launch no lane reads what
// another lane of the same launch writes -- counts the survivors, takes the largest chord between two survivors' rays and turns the
// survivors of a dropped point into BA_OBS_POINT.  A count or an error sum over a track is: lane l adds its observations l, l + L, ...
// in index order, then the L lane sums are added by the XOR butterfly (1, 2, 4).  A maximum is order-free.  No atomics.
#pragma once

#include <math.h>

#if defined(__HIP__)
#include <hip/hip_runtime.h>
#define BA_FLT_HD __host__ __device__ inline
#else
#define BA_FLT_HD inline
#endif

// statuses (ba_obs_status / ba_filter_point_status of include/ba_mi355x.h)
#define BA_FLT_K_KEPT 0
#define BA_FLT_K_WAS_OFF 1
#define BA_FLT_K_BEHIND 2
#define BA_FLT_K_NONFINITE 3
#define BA_FLT_K_REPROJ 4
#define BA_FLT_K_POINT 5
#define BA_FLT_K_PT_KEPT 0
#define BA_FLT_K_PT_SHORT 1
#define BA_FLT_K_PT_LOW_ANGLE 2

// The kernels' pair loop may stop at a squared chord >= chord2_exit = (2 sin(min_angle / 2))^2 (1 + BA_FLT_EXIT_MARGIN): the angle of such
// a chord is above min_angle by far more than atan2 and sqrt round (a few 1e-16 relative), the full maximum is no smaller, and so the
// decision theta < min_angle is the one the full loop takes.  Below the margin the loop simply goes on.
#define BA_FLT_EXIT_MARGIN 1e-12

struct ba_flt_cfg {
    double max_reproj_px, min_angle_rad, chord2_exit;
    int min_track, require_front;
};
struct ba_flt_obs { double c[15], m0, m1; };

BA_FLT_HD bool ba_flt_finite(double x) { return fabs(x) <= 1.7976931348623157e308; } // (false for NaN)
BA_FLT_HD double ba_flt_chord2_exit(double min_angle_rad)
{
    const double s = 2.0 * sin(0.5 * min_angle_rad);
    return s * s * (1.0 + BA_FLT_EXIT_MARGIN);
}
BA_FLT_HD double ba_flt_angle(double c2max)
{
    const double rest = 4.0 - c2max;
    return 2.0 * atan2(sqrt(c2max), sqrt(rest > 0.0 ? rest : 0.0));
}

// Step 2 for one ACTIVE observation: its status (KEPT = survivor so far), err = |pi(X) - meas| (unweighted, pixels; whatever the
// arithmetic gives, NaN and inf included) and the unit ray d = (C - X) / |C - X|, C = -R'T (zeros: no ray).
BA_FLT_HD int ba_flt_observation(const ba_flt_obs &o, const double X[3], const ba_flt_cfg &cf, double &err, double d[3])
{
    const double *R = o.c;
    const double XX0 = R[0] * X[0] + R[1] * X[1] + R[2] * X[2] + o.c[9];
    const double XX1 = R[3] * X[0] + R[4] * X[1] + R[5] * X[2] + o.c[10];
    const double XX2 = R[6] * X[0] + R[7] * X[1] + R[8] * X[2] + o.c[11];
    const double xu0 = XX0 / XX2, xu1 = XX1 / XX2, r2u = xu0 * xu0 + xu1 * xu1, r4u = r2u * r2u;
    const double f = o.c[12], k1 = o.c[13], k2 = o.c[14], kr = 1.0 + k1 * r2u + k2 * r4u;
    const double e0 = f * kr * xu0 - o.m0, e1 = f * kr * xu1 - o.m1;
    err = sqrt(e0 * e0 + e1 * e1);
    double v[3];
    for (int k = 0; k < 3; k++) v[k] = -(R[k] * o.c[9] + R[3 + k] * o.c[10] + R[6 + k] * o.c[11]) - X[k];
    const double n = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    if (n > 0.0 && ba_flt_finite(n)) { d[0] = v[0] / n; d[1] = v[1] / n; d[2] = v[2] / n; }
    else { d[0] = 0.0; d[1] = 0.0; d[2] = 0.0; }
    if (cf.require_front && !(XX2 < 0.0)) return BA_FLT_K_BEHIND; // (a NaN is behind)
    if (!ba_flt_finite(err)) return BA_FLT_K_NONFINITE;
    if (cf.max_reproj_px > 0.0 && err > cf.max_reproj_px) return BA_FLT_K_REPROJ;
    return BA_FLT_K_KEPT;
}

// Steps 3 - 5 on what step 2 has stored.  Trk: status(i), set_status(i, s), ray(i, d).  EARLY: the pair loop of a lane stops at the
// first chord that decides (chord2_exit), and angle_rad is then the angle of that chord, not the largest; the status is the same.
// Every lane of the group leaves with the same pt_status and angle_rad.
template <int L, bool EARLY, class Trk, class Red>
BA_FLT_HD void ba_flt_point(int lane, int t, Trk &tk, const Red &rd, const ba_flt_cfg &cf, int &pt_status, double &angle_rad)
{
    double ns = 0.0;
    for (int i = lane; i < t; i += L)
        if (tk.status(i) == BA_FLT_K_KEPT) ns += 1.0;
    ns = rd.sum(ns);
    pt_status = BA_FLT_K_PT_KEPT;
    angle_rad = 0.0;
    if (ns < (double)cf.min_track) pt_status = BA_FLT_K_PT_SHORT;
    else if (cf.min_angle_rad > 0.0) {
        double c2max = 0.0;
        bool done = false;
        for (int i = lane; i < t && !done; i += L) {
            if (tk.status(i) != BA_FLT_K_KEPT) continue;
            double di[3];
            tk.ray(i, di);
            if (di[0] == 0.0 && di[1] == 0.0 && di[2] == 0.0) continue;
            for (int j = 0; j < i; j++) {
                if (tk.status(j) != BA_FLT_K_KEPT) continue;
                double dj[3];
                tk.ray(j, dj);
                if (dj[0] == 0.0 && dj[1] == 0.0 && dj[2] == 0.0) continue;
                const double e0 = di[0] - dj[0], e1 = di[1] - dj[1], e2 = di[2] - dj[2], c2 = e0 * e0 + e1 * e1 + e2 * e2;
                if (c2 > c2max) c2max = c2;
                if (EARLY && c2 >= cf.chord2_exit) { done = true; break; }
            }
        }
        c2max = rd.max(c2max);
        angle_rad = ba_flt_angle(c2max);
        if (angle_rad < cf.min_angle_rad) pt_status = BA_FLT_K_PT_LOW_ANGLE;
    }
    if (pt_status != BA_FLT_K_PT_KEPT)
        for (int i = lane; i < t; i += L)
            if (tk.status(i) == BA_FLT_K_KEPT) tk.set_status(i, BA_FLT_K_POINT);
}

#if defined(__HIP__)
// ---- the kernels: L = 8 lanes of a wavefront per point, 32 points per 256-thread workgroup (k_tri_points' mapping) ----------------
template <int L> struct ba_flt_red_dev {
    __device__ double sum(double v) const
    {
#pragma unroll
        for (int m = 1; m < L; m <<= 1) v += __shfl_xor(v, m, L);
        return v;
    }
    __device__ double max(double v) const
    {
#pragma unroll
        for (int m = 1; m < L; m <<= 1) { const double u = __shfl_xor(v, m, L); v = u > v ? u : v; }
        return v;
    }
};
struct ba_flt_trk_dev {
    size_t K, o0;
    unsigned char *st;  // [K] by observation
    const double *rays; // [3][K] by observation; zeros = no ray
    __device__ int status(int i) const { return (int)st[o0 + i]; }
    __device__ void set_status(int i, int s) { st[o0 + i] = (unsigned char)s; }
    __device__ void ray(int i, double d[3]) const
    {
        const size_t q = o0 + i;
        d[0] = rays[q]; d[1] = rays[K + q]; d[2] = rays[2 * K + q];
    }
};

// Step 2 for every observation of every point: lane l of a point's group takes its observations l, l + 8, ...  act == nullptr: all active.
// An inactive observation: WAS_OFF, err = NaN, no ray.
template <typename T, int L>
__global__ __launch_bounds__(256) void k_filter_obs(int N, int M, int K, const int *__restrict__ pt_ptr, const int *__restrict__ obs_cam,
                                                    const T *__restrict__ cam, const T *__restrict__ pts, const T *__restrict__ meas,
                                                    const unsigned char *__restrict__ act, ba_flt_cfg cf, unsigned char *__restrict__ st,
                                                    double *__restrict__ err, double *__restrict__ rays)
{
    const int j = (int)((blockIdx.x * 256u + threadIdx.x) / L), lane = threadIdx.x % L;
    if (j >= M) return;
    const double X[3] = {(double)pts[j], (double)pts[(size_t)M + j], (double)pts[2 * (size_t)M + j]};
    const int e = pt_ptr[j + 1];
    for (int i = pt_ptr[j] + lane; i < e; i += L) {
        int s = BA_FLT_K_WAS_OFF;
        double er = NAN, d[3] = {0.0, 0.0, 0.0};
        if (!act || act[i]) {
            ba_flt_obs o;
            const int a = obs_cam[i];
#pragma unroll
            for (int k = 0; k < 15; k++) o.c[k] = (double)cam[(size_t)k * N + a];
            o.m0 = (double)meas[i]; o.m1 = (double)meas[(size_t)K + i];
            s = ba_flt_observation(o, X, cf, er, d);
        }
        st[i] = (unsigned char)s;
        err[i] = er;
        rays[i] = d[0]; rays[(size_t)K + i] = d[1]; rays[2 * (size_t)K + i] = d[2];
    }
}

// Steps 3 - 6 per point.  nact / nweff != nullptr (apply): the new active byte and the new effective weight (kept ? w_o : 0; wobs ==
// nullptr: w_o = 1) of every observation.  part: [BA_FLT_NSUM][gridDim.x] block partials -- the six observation counts, the two point
// counts, the error sum over the finite active observations and over the kept ones -- each the sum over the block's 32 points in index
// order of the points' butterfly sums.
#define BA_FLT_NSUM 10
template <typename T, int L>
__global__ __launch_bounds__(256) void k_filter_points(int M, int K, const int *__restrict__ pt_ptr, ba_flt_cfg cf, unsigned char *st,
                                                       const double *__restrict__ err, const double *__restrict__ rays,
                                                       const T *__restrict__ wobs, unsigned char *__restrict__ pst,
                                                       unsigned char *__restrict__ nact, T *__restrict__ nweff, double *__restrict__ part)
{
    constexpr int G = 256 / L;
    __shared__ double sh[BA_FLT_NSUM][G];
    const int grp = threadIdx.x / L, lane = threadIdx.x % L, j = (int)blockIdx.x * G + grp;
    double v[BA_FLT_NSUM];
#pragma unroll
    for (int k = 0; k < BA_FLT_NSUM; k++) v[k] = 0.0;
    if (j < M) {
        const int o0 = pt_ptr[j], t = pt_ptr[j + 1] - o0;
        ba_flt_trk_dev tk{(size_t)K, (size_t)o0, st, rays};
        const ba_flt_red_dev<L> rd{};
        int ps;
        double ang;
        ba_flt_point<L, true>(lane, t, tk, rd, cf, ps, ang);
        for (int i = lane; i < t; i += L) {
            const size_t q = (size_t)o0 + i;
            const int s = (int)st[q]; // (this lane's own observations: its own stores)
            const double er = err[q];
#pragma unroll
            for (int k = 0; k < 6; k++) v[k] += s == k ? 1.0 : 0.0;
            if (s != BA_FLT_K_WAS_OFF && ba_flt_finite(er)) v[8] += er;
            if (s == BA_FLT_K_KEPT) v[9] += er;
            if (nact) {
                nact[q] = s == BA_FLT_K_KEPT ? 1 : 0;
                nweff[q] = s == BA_FLT_K_KEPT ? (wobs ? wobs[q] : (T)1.0) : (T)0;
            }
        }
#pragma unroll
        for (int k = 0; k < BA_FLT_NSUM; k++) v[k] = rd.sum(v[k]);
        v[6] = ps == BA_FLT_K_PT_SHORT ? 1.0 : 0.0;
        v[7] = ps == BA_FLT_K_PT_LOW_ANGLE ? 1.0 : 0.0;
        if (lane == 0) pst[j] = (unsigned char)ps;
    }
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < BA_FLT_NSUM; k++) sh[k][grp] = v[k];
    }
    __syncthreads();
    if (threadIdx.x < BA_FLT_NSUM) {
        double a = 0.0;
        for (int k = 0; k < G; k++) a += sh[threadIdx.x][k];
        part[(size_t)threadIdx.x * gridDim.x + blockIdx.x] = a;
    }
}
#endif // __HIP__
