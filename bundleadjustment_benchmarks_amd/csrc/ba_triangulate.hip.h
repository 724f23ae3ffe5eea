// ba_triangulate.hip.h -- re-seating points from the cameras that see them (ba_solver_triangulate_points / ba_triangulate_point;
// include/ba_mi355x.h).  The per-point rule is written ONCE here, for L cooperating lanes, a reader of the
// point's observations and a reducer over the lanes: the host function (ba_triangulate.cpp) runs it with L = 1, the kernels below
// with L = 8 lanes of one wavefront per point, as k_pcg_point maps its points.  All geometry is fp64 for both scalar types; the
// resident state is read as stored and the new point is rounded once to the solver's scalar type.
//
// Model (k_eval, ba_problem.cpp): XX = R X + T, xu = XX_01 / XX_2, kr = 1 + k1 |xu|^2 + k2 |xu|^4, pi = f kr xu; the camera looks
// down -z: X is in front of it iff XX_2 < 0.  A camera is the 15 scalars of BA_GET_CAMS: R row-major, T, f, k1, k2.
//
// Every sum over a track is: lane l adds its observations l, l + L, ... in index order, then the L lane sums are added by the XOR
// butterfly (1, 2, 4), which leaves the same bits in every lane.  It depends on the track alone: a point's result is the same bits on
// every run, whatever else is asked for and wherever the point stands in the request.  No atomics.
#pragma once

#include <math.h>

#if defined(__HIP__)
#include <hip/hip_runtime.h>
#define BA_TRI_HD __host__ __device__ inline
#else
#define BA_TRI_HD inline
#endif

// statuses (BA_TRI_* of include/ba_mi355x.h)
#define BA_TRI_K_REPLACED 0
#define BA_TRI_K_FEW_VIEWS 1
#define BA_TRI_K_LOW_ANGLE 2
#define BA_TRI_K_DEGENERATE 3
#define BA_TRI_K_BEHIND 4
#define BA_TRI_K_REPROJ 5
#define BA_TRI_K_NOT_BETTER 6
#define BA_TRI_K_FIXED 7

// Undistortion: Newton on h(rho) = rho (1 + k1 rho^2 + k2 rho^4) - |m| from rho = |m|, this many steps; the observation is unusable
// unless every h' met on the way and at the end is > 0, every value is finite, rho ends > 0 and |h(rho)| <= BA_TRI_UNDISTORT_TOL |m|.
#define BA_TRI_NEWTON_ITERS 12
#define BA_TRI_UNDISTORT_TOL 1e-12
// Refinement: X' = X - (H + mu I)^-1 g with H = sum w_o J'J, mu = BA_TRI_MU_REL tr(H) / 3
#define BA_TRI_MU_REL 1e-9
// X' is taken iff c(X') < c(X) (1 - BA_TRI_MIN_DECREASE).  A plain c(X') < c(X) is decided by rounding once the refinement has
// converged -- the last step, some 1e-11 long, is then taken or not by the luck of the sum's order, and host, kernel and any check of
// them part by that step.  1e-11 is well above what an fp64 evaluation of c resolves (a few 1e-13 relative) and far below any decrease
// that moves X by more than its conditioning allows.
#define BA_TRI_MIN_DECREASE 1e-11

struct ba_tri_cfg {
    double min_angle_rad, max_reproj_px;
    int refine_iters, only_if_better;
    int loss;      // ba_loss_kind
    double lscale; // tau / delta / c
};
struct ba_tri_obs { double c[15], m0, m1, w; };
struct ba_tri_out { double x[3]; int status; double cost_old, cost_new, angle_rad; };
struct ba_tri_acc { double c, H[6], g[3], maxrep, behind; };

BA_TRI_HD bool ba_tri_finite(double x) { return fabs(x) <= 1.7976931348623157e308; } // (false for NaN)

// rho(s) and rho'(s) of the measurement model (ba_solver_set_loss), s = w^2 |pi - meas|^2
BA_TRI_HD void ba_tri_rho(int kind, double sc, double s, double &rho, double &drho)
{
    const double sc2 = sc * sc;
    rho = s; drho = 1.0; // BA_LOSS_TRIVIAL and Huber's quadratic part
    if (kind == 0) { // BA_LOSS_REFERENCE: psi
        if (s < sc2) { rho = s * (2.0 - s / sc2) / 4.0; drho = (1.0 - s / sc2) / 2.0; }
        else { rho = sc2 / 4.0; drho = 0.0; }
    } else if (kind == 2) { // BA_LOSS_HUBER
        if (s > sc2) { const double n = sqrt(s); rho = 2.0 * sc * n - sc2; drho = sc / n; }
    } else if (kind == 3) { // BA_LOSS_CAUCHY
        rho = sc2 * log1p(s / sc2); drho = 1.0 / (1.0 + s / sc2);
    }
}

// The forward ray of one observation in the world, unit length; false (and d = 0) when the observation is unusable.
BA_TRI_HD bool ba_tri_ray(const ba_tri_obs &o, double d[3])
{
    d[0] = d[1] = d[2] = 0.0;
    const double f = o.c[12], k1 = o.c[13], k2 = o.c[14];
    const double m0 = o.m0 / f, m1 = o.m1 / f, rm = sqrt(m0 * m0 + m1 * m1);
    if (!ba_tri_finite(rm)) return false;
    double xu0 = 0.0, xu1 = 0.0;
    if (rm > 0.0) {
        double rho = rm;
        bool ok = true;
        for (int it = 0; it < BA_TRI_NEWTON_ITERS; it++) {
            const double r2 = rho * rho, dh = 1.0 + r2 * (3.0 * k1 + 5.0 * k2 * r2), h = rho * (1.0 + r2 * (k1 + k2 * r2)) - rm;
            if (!(dh > 0.0) || !ba_tri_finite(dh) || !ba_tri_finite(h)) { ok = false; break; }
            rho -= h / dh;
        }
        if (!ok || !ba_tri_finite(rho) || !(rho > 0.0)) return false;
        const double r2 = rho * rho, dh = 1.0 + r2 * (3.0 * k1 + 5.0 * k2 * r2), h = rho * (1.0 + r2 * (k1 + k2 * r2)) - rm;
        if (!(dh > 0.0) || !ba_tri_finite(dh) || !(fabs(h) <= BA_TRI_UNDISTORT_TOL * rm)) return false;
        const double sc = rho / rm;
        xu0 = m0 * sc; xu1 = m1 * sc;
    }
    // d = R' (-(xu, 1)), normalised
    double v[3];
    for (int k = 0; k < 3; k++) v[k] = -(o.c[k] * xu0 + o.c[3 + k] * xu1 + o.c[6 + k]);
    const double n = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    if (!(n > 0.0) || !ba_tri_finite(n)) return false;
    d[0] = v[0] / n; d[1] = v[1] / n; d[2] = v[2] / n;
    return true;
}

// A x = b for the symmetric A = (00, 01, 02, 11, 12, 22) by Cholesky; false on a pivot that is <= 0 or not finite
BA_TRI_HD bool ba_tri_chol3_solve(const double A[6], const double b[3], double x[3])
{
    const double p0 = A[0];
    if (!(p0 > 0.0) || !ba_tri_finite(p0)) return false;
    const double l00 = sqrt(p0), l10 = A[1] / l00, l20 = A[2] / l00;
    const double p1 = A[3] - l10 * l10;
    if (!(p1 > 0.0) || !ba_tri_finite(p1)) return false;
    const double l11 = sqrt(p1), l21 = (A[4] - l20 * l10) / l11;
    const double p2 = A[5] - l20 * l20 - l21 * l21;
    if (!(p2 > 0.0) || !ba_tri_finite(p2)) return false;
    const double l22 = sqrt(p2);
    const double y0 = b[0] / l00, y1 = (b[1] - l10 * y0) / l11, y2 = (b[2] - l20 * y0 - l21 * y1) / l22;
    x[2] = y2 / l22;
    x[1] = (y1 - l21 * x[2]) / l11;
    x[0] = (y0 - l10 * x[1] - l20 * x[2]) / l00;
    return ba_tri_finite(x[0]) && ba_tri_finite(x[1]) && ba_tri_finite(x[2]);
}

// One pass over the track at X: the point's own term c = sum rho(s_o) of the objective, H = sum w J'J and g = sum w J'r of its IRLS
// Gauss-Newton model, whether some camera does not have X in front, and the largest unweighted |pi - meas| of a usable observation.
template <int L, class Obs, class Red>
BA_TRI_HD void ba_tri_pass(int lane, int t, const Obs &ob, const Red &rd, int loss, double lscale, const double X[3], ba_tri_acc &a)
{
    double c = 0.0, H[6] = {0, 0, 0, 0, 0, 0}, g[3] = {0, 0, 0}, maxrep = 0.0, behind = 0.0;
    for (int i = lane; i < t; i += L) {
        if (!ob.active(i)) continue; // (ba_solver_set_obs_active: not part of the track)
        ba_tri_obs o;
        ob.load(i, o);
        const double *R = o.c;
        const double XX0 = R[0] * X[0] + R[1] * X[1] + R[2] * X[2] + o.c[9];
        const double XX1 = R[3] * X[0] + R[4] * X[1] + R[5] * X[2] + o.c[10];
        const double XX2 = R[6] * X[0] + R[7] * X[1] + R[8] * X[2] + o.c[11];
        if (!(XX2 < 0.0)) behind = 1.0;
        const double xu0 = XX0 / XX2, xu1 = XX1 / XX2, r2u = xu0 * xu0 + xu1 * xu1, r4u = r2u * r2u;
        const double f = o.c[12], k1 = o.c[13], k2 = o.c[14], kr = 1.0 + k1 * r2u + k2 * r4u;
        const double e0 = f * kr * xu0 - o.m0, e1 = f * kr * xu1 - o.m1; // unweighted
        double dr[3];
        ob.ray(i, dr);
        if (dr[0] != 0.0 || dr[1] != 0.0 || dr[2] != 0.0) {
            double rp = sqrt(e0 * e0 + e1 * e1);
            if (rp != rp) rp = INFINITY; // (a value that is not a number fails every bound)
            if (rp > maxrep) maxrep = rp;
        }
        const double r0 = o.w * e0, r1 = o.w * e1, s = r0 * r0 + r1 * r1;
        double rho, om;
        ba_tri_rho(loss, lscale, s, rho, om);
        c += rho;
        // J = w dpi/dXX R (k_eval's dpX)
        const double a00 = 1.0 / XX2, a02 = -XX0 / (XX2 * XX2), a12 = -XX1 / (XX2 * XX2);
        const double dkr = 2.0 * k1 + 4.0 * k2 * r2u;
        const double p00 = o.w * f * (kr + xu0 * xu0 * dkr), p01 = o.w * f * (xu0 * xu1 * dkr), p11 = o.w * f * (kr + xu1 * xu1 * dkr);
        const double q0[3] = {p00 * a00, p01 * a00, p00 * a02 + p01 * a12}, q1[3] = {p01 * a00, p11 * a00, p01 * a02 + p11 * a12};
        double J0[3], J1[3];
        for (int k = 0; k < 3; k++) {
            J0[k] = q0[0] * R[k] + q0[1] * R[3 + k] + q0[2] * R[6 + k];
            J1[k] = q1[0] * R[k] + q1[1] * R[3 + k] + q1[2] * R[6 + k];
        }
        H[0] += om * (J0[0] * J0[0] + J1[0] * J1[0]);
        H[1] += om * (J0[0] * J0[1] + J1[0] * J1[1]);
        H[2] += om * (J0[0] * J0[2] + J1[0] * J1[2]);
        H[3] += om * (J0[1] * J0[1] + J1[1] * J1[1]);
        H[4] += om * (J0[1] * J0[2] + J1[1] * J1[2]);
        H[5] += om * (J0[2] * J0[2] + J1[2] * J1[2]);
        for (int k = 0; k < 3; k++) g[k] += om * (J0[k] * r0 + J1[k] * r1);
    }
    a.c = rd.sum(c);
    for (int k = 0; k < 6; k++) a.H[k] = rd.sum(H[k]);
    for (int k = 0; k < 3; k++) a.g[k] = rd.sum(g[k]);
    a.maxrep = rd.max(maxrep);
    a.behind = rd.max(behind);
}

// The rule.  `fixed`: the point is held constant or carries a prior (the solver's call only).  Every lane of the point's group leaves
// with the same `out`; out.x is the candidate where one was formed and x_old otherwise.
template <int L, class Obs, class Red>
BA_TRI_HD void ba_tri_point(int lane, int t, const Obs &ob, const Red &rd, const ba_tri_cfg &cf, const double xold[3], int fixed, ba_tri_out &out)
{
    ba_tri_acc cur;
    out.x[0] = xold[0]; out.x[1] = xold[1]; out.x[2] = xold[2];
    out.angle_rad = 0.0;
    ba_tri_pass<L>(lane, t, ob, rd, cf.loss, cf.lscale, xold, cur);
    out.cost_old = out.cost_new = cur.c;
    if (fixed) { out.status = BA_TRI_K_FIXED; return; }
    // 2. the largest angle between two usable rays: the largest chord |d_i - d_j|, theta = 2 atan2(chord, sqrt(4 - chord^2))
    double nus = 0.0, c2max = 0.0;
    for (int i = lane; i < t; i += L) { // (an inactive observation has no ray)
        double di[3];
        ob.ray(i, di);
        if (di[0] == 0.0 && di[1] == 0.0 && di[2] == 0.0) continue;
        nus += 1.0;
        for (int j = 0; j < i; j++) {
            double dj[3];
            ob.ray(j, dj);
            if (dj[0] == 0.0 && dj[1] == 0.0 && dj[2] == 0.0) continue;
            const double e0 = di[0] - dj[0], e1 = di[1] - dj[1], e2 = di[2] - dj[2], c2 = e0 * e0 + e1 * e1 + e2 * e2;
            if (c2 > c2max) c2max = c2;
        }
    }
    nus = rd.sum(nus);
    c2max = rd.max(c2max);
    if (nus < 2.0) { out.status = BA_TRI_K_FEW_VIEWS; return; }
    const double rest = 4.0 - c2max;
    out.angle_rad = 2.0 * atan2(sqrt(c2max), sqrt(rest > 0.0 ? rest : 0.0));
    if (out.angle_rad < cf.min_angle_rad) { out.status = BA_TRI_K_LOW_ANGLE; return; }
    // 3. midpoint: (sum w^2 (I - d d')) X = sum w^2 (I - d d') C over the usable observations
    double A[6] = {0, 0, 0, 0, 0, 0}, b[3] = {0, 0, 0};
    for (int i = lane; i < t; i += L) {
        double d[3];
        ob.ray(i, d);
        if (d[0] == 0.0 && d[1] == 0.0 && d[2] == 0.0) continue;
        ba_tri_obs o;
        ob.load(i, o);
        double C[3];
        for (int k = 0; k < 3; k++) C[k] = -(o.c[k] * o.c[9] + o.c[3 + k] * o.c[10] + o.c[6 + k] * o.c[11]);
        const double w2 = o.w * o.w, dc = d[0] * C[0] + d[1] * C[1] + d[2] * C[2];
        A[0] += w2 * (1.0 - d[0] * d[0]); A[1] += w2 * (-d[0] * d[1]); A[2] += w2 * (-d[0] * d[2]);
        A[3] += w2 * (1.0 - d[1] * d[1]); A[4] += w2 * (-d[1] * d[2]); A[5] += w2 * (1.0 - d[2] * d[2]);
        for (int k = 0; k < 3; k++) b[k] += w2 * (C[k] - d[k] * dc);
    }
    for (int k = 0; k < 6; k++) A[k] = rd.sum(A[k]);
    for (int k = 0; k < 3; k++) b[k] = rd.sum(b[k]);
    double X[3], Xt[3];
    if (!ba_tri_chol3_solve(A, b, Xt)) { out.status = BA_TRI_K_DEGENERATE; return; }
    // 4. monotone refinement: the midpoint is taken as it is, a later X' only with a c smaller by BA_TRI_MIN_DECREASE relative
    for (int it = 0;; it++) {
        ba_tri_acc at;
        ba_tri_pass<L>(lane, t, ob, rd, cf.loss, cf.lscale, Xt, at);
        if (it > 0 && !(at.c < cur.c * (1.0 - BA_TRI_MIN_DECREASE))) break;
        cur = at;
        X[0] = Xt[0]; X[1] = Xt[1]; X[2] = Xt[2];
        if (it >= cf.refine_iters) break;
        const double mu = BA_TRI_MU_REL * (cur.H[0] + cur.H[3] + cur.H[5]) / 3.0;
        const double Hm[6] = {cur.H[0] + mu, cur.H[1], cur.H[2], cur.H[3] + mu, cur.H[4], cur.H[5] + mu};
        double dx[3];
        if (!ba_tri_chol3_solve(Hm, cur.g, dx)) break;
        Xt[0] = X[0] - dx[0]; Xt[1] = X[1] - dx[1]; Xt[2] = X[2] - dx[2];
    }
    out.x[0] = X[0]; out.x[1] = X[1]; out.x[2] = X[2];
    out.cost_new = cur.c;
    // 5. the tests on the candidate
    if (cur.behind != 0.0 || !ba_tri_finite(X[0]) || !ba_tri_finite(X[1]) || !ba_tri_finite(X[2])) { out.status = BA_TRI_K_BEHIND; return; }
    if (cf.max_reproj_px > 0.0 && !(cur.maxrep <= cf.max_reproj_px)) { out.status = BA_TRI_K_REPROJ; return; }
    if (cf.only_if_better && !(out.cost_new < out.cost_old)) { out.status = BA_TRI_K_NOT_BETTER; return; }
    out.status = BA_TRI_K_REPLACED;
}

#if defined(__HIP__)
// ---- the kernels: L = 8 lanes of a wavefront per requested point, 32 points per 256-thread workgroup ----------------------------
template <int L> struct ba_tri_red_dev {
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
template <typename T> struct ba_tri_obs_dev {
    int N, K, o0;
    const T *cam, *meas, *wobs;
    const int *obs_cam;
    const double *rays; // [3][K], by observation; zeros = unusable
    const unsigned char *act; // by observation, 0 = inactive (ba_solver_set_obs_active); nullptr = all active
    __device__ bool active(int i) const { return !act || act[o0 + i] != 0; }
    __device__ void load(int i, ba_tri_obs &o) const
    {
        const int q = o0 + i, a = obs_cam[q];
#pragma unroll
        for (int k = 0; k < 15; k++) o.c[k] = (double)cam[(size_t)k * N + a];
        o.m0 = (double)meas[q]; o.m1 = (double)meas[(size_t)K + q];
        o.w = wobs ? (double)wobs[q] : 1.0;
    }
    __device__ void ray(int i, double d[3]) const
    {
        const size_t q = (size_t)o0 + i;
        d[0] = rays[q]; d[1] = rays[(size_t)K + q]; d[2] = rays[2 * (size_t)K + q];
    }
};

// the rays of the requested points' observations (ids == nullptr: point q of the request is point q)
template <typename T, int L>
__global__ __launch_bounds__(256) void k_tri_rays(int n, const int *__restrict__ ids, int N, int K, const int *__restrict__ pt_ptr,
                                                  const int *__restrict__ obs_cam, const T *__restrict__ cam, const T *__restrict__ meas,
                                                  const unsigned char *__restrict__ act, double *__restrict__ rays)
{
    const int q = (int)((blockIdx.x * 256u + threadIdx.x) / L), lane = threadIdx.x % L;
    if (q >= n) return;
    const int j = ids ? ids[q] : q;
    const ba_tri_obs_dev<T> ob{N, K, 0, cam, meas, nullptr, obs_cam, nullptr, act};
    const int e = pt_ptr[j + 1];
    for (int i = pt_ptr[j] + lane; i < e; i += L) {
        double d[3] = {0.0, 0.0, 0.0};
        if (ob.active(i)) {
            ba_tri_obs o;
            ob.load(i, o);
            (void)ba_tri_ray(o, d);
        }
        rays[i] = d[0]; rays[(size_t)K + i] = d[1]; rays[2 * (size_t)K + i] = d[2];
    }
}

// The rule per requested point; lane 0 of a group writes the status (request order) and, for status 0, the point.  part: [10][gridDim.x]
// block partials -- the eight status counts, cost_before, cost_after -- each the sum over the block's 32 points in index order.
template <typename T, int L>
__global__ __launch_bounds__(256) void k_tri_points(int n, const int *__restrict__ ids, int N, int M, int K, const int *__restrict__ pt_ptr,
                                                    const int *__restrict__ obs_cam, const T *__restrict__ cam, const T *__restrict__ meas,
                                                    const T *__restrict__ wobs, const unsigned char *__restrict__ act,
                                                    const double *__restrict__ rays, const unsigned char *__restrict__ fixed, ba_tri_cfg cf, T *__restrict__ pts,
                                                    unsigned char *__restrict__ status, double *__restrict__ part)
{
    constexpr int G = 256 / L;
    __shared__ int sh_st[G];
    __shared__ double sh_c[2][G];
    const int grp = threadIdx.x / L, lane = threadIdx.x % L, q = (int)blockIdx.x * G + grp;
    if (q < n) {
        const int j = ids ? ids[q] : q;
        const int o0 = pt_ptr[j], t = pt_ptr[j + 1] - o0;
        const ba_tri_obs_dev<T> ob{N, K, o0, cam, meas, wobs, obs_cam, rays, act};
        const double xold[3] = {(double)pts[j], (double)pts[(size_t)M + j], (double)pts[2 * (size_t)M + j]};
        ba_tri_out out;
        ba_tri_point<L>(lane, t, ob, ba_tri_red_dev<L>{}, cf, xold, fixed ? (int)fixed[j] : 0, out);
        if (lane == 0) {
            status[q] = (unsigned char)out.status;
            if (out.status == BA_TRI_K_REPLACED) {
                pts[j] = (T)out.x[0]; pts[(size_t)M + j] = (T)out.x[1]; pts[2 * (size_t)M + j] = (T)out.x[2];
            }
            sh_st[grp] = out.status;
            sh_c[0][grp] = out.cost_old;
            sh_c[1][grp] = out.status == BA_TRI_K_REPLACED ? out.cost_new : out.cost_old;
        }
    } else if (lane == 0) {
        sh_st[grp] = -1;
        sh_c[0][grp] = 0.0; sh_c[1][grp] = 0.0;
    }
    __syncthreads();
    if (threadIdx.x < 10) {
        double a = 0.0;
        for (int k = 0; k < G; k++) a += threadIdx.x < 8 ? (sh_st[k] == (int)threadIdx.x ? 1.0 : 0.0) : sh_c[threadIdx.x - 8][k];
        part[(size_t)threadIdx.x * gridDim.x + blockIdx.x] = a;
    }
}
#endif // __HIP__

