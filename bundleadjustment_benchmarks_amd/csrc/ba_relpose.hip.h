// ba_relpose.hip.h -- relative-pose constraints between camera pairs (ba_solver_set_relative_poses).
//
// A constraint between cameras a and b (x_cam = R X + T) is six rows of J on TWO pose blocks:
//   R_ab = R_b R_a^T,  t_ab = T_b - R_ab T_a            (x_b = R_ab x_a + t_ab; both invariant under a rigid motion of the world)
//   e_t = L_t (t_ab - t0)                                d e_t / d(T_a, omega_a) = L_t [-R_ab | -R_ab [T_a]x]   d(T_b, omega_b) = L_t [I | [u]x],  u = R_ab T_a
//   e_r = L_r phi,  phi = Log(R_ab R0^T)                 d e_r / d(T_a, omega_a) = L_r [0 | -Jl^-1 R_ab]        d(T_b, omega_b) = L_r [0 | Jl^-1]
//   Jl^-1 = I - [phi]x / 2 + c [phi]x^2,  c = 1 / theta^2 - (1 + cos theta) / (2 theta sin theta)  (series below theta = 0.05)
// (retraction of ba_retract_cams: T + dT, R <- Rodrigues(d omega) R; the intrinsics columns are zero).  So it owes the normal equations
// two 6 x 6 diagonal additions (V_a, V_b), two 6-vectors (gc_a, gc_b) and ONE cross block H_ab = J_a^T J_b, the first entry of the
// reduced camera system that no shared point produces.
//
// A camera may sit in many constraints (two in an odometry chain, dozens at a rig's hub), so the thread of a constraint cannot own a
// diagonal block.  Two stages, no atomics:
//   k_relpose          one thread per constraint: e_t, e_r, the energy partials (behind the priors' in the array the second-stage jobs
//                      sum); LIN: the record [H_aa 36 | H_bb 36 | H_ab 36 | g_a 6 | g_b 6] (BA_RP_REC scalars, masked columns zero)
//   k_relpose_gather   one thread per (camera, entry of its 6 x 6 + 6): adds the camera's records into V_a / gc_a in the order of a
//                      CSR list the host built at set time (list order).  The records are symmetric in bits and so is V: entry (r, c)
//                      and entry (c, r) add the same numbers in the same order.
//   k_relpose_schur    BA_CHOLESKY: one thread per (constraint, entry of the cross block) adds H_ab into the block of S the
//                      factorisation reads (lower block triangle), behind the assembly; each unordered pair occurs once.
//   BA_ITERSCHUR       k_pcg_relpose, directly behind k_pcg_cam, adds  sum over the incident constraints H_ab v_b  (CSR order) to y_a and
//                      the term to the block partials (ba_pcg.hip.h).
// The geometry of a constraint (R_ab, t_ab - t0, Log, Jl^-1, the 6 x 6 products) is evaluated in fp64 for both scalar types: t_ab - t0
// cancels like the centre prior's C - C0, and n threads of fp64 cost nothing here; the record and the energies are rounded to T once.
// Every sum is in a fixed order, so a trial is the same bits eager, under ba_solver_try_step and replayed as a hipGraph.
#ifndef BA_RELPOSE_HIP_H
#define BA_RELPOSE_HIP_H

#include "ba_kernels.hip.h"

#define BA_RP_REC 120 /* H_aa | H_bb | H_ab (6 x 6 row-major each) | g_a | g_b */
#define BA_RP_HAB 72
#define BA_RP_G 108
#define BA_RP_ENT 42 /* entries of one camera's gather: 36 of V, 6 of gc */

template <typename T> struct ba_relpose_args {
    int n;
    const int *pair;                 // [n][2]: a, b
    const T *R0, *t0, *Lr, *Lt;      // [n][9] row-major, [n][3], [n][9], [n][9]
};
// a camera's incident constraints, in list order: inc = 2 * constraint + (0: the camera is a, 1: it is b)
template <typename T> struct ba_relpose_csr {
    const int *ptr, *inc, *pair;     // [N + 1], [2 n], [n][2]
    const T *rec;                    // [n][BA_RP_REC]
};

// Everything of one constraint in fp64.  e = (e_t, e_r); LIN: Ja, Jb (6 x 6 row-major: rows e_t then e_r, columns T then omega).
// One rounding per operation (the trial and the linearisation instantiations must give the same energy bits).
template <bool LIN>
__device__ __forceinline__ void ba_relpose_eval(const double (&Ra)[9], const double (&Ta)[3], const double (&Rb)[9], const double (&Tb)[3],
                                                const double (&R0)[9], const double (&t0)[3], const double (&Lr)[9], const double (&Lt)[9],
                                                double (&e)[6], double (&Ja)[36], double (&Jb)[36])
{
#pragma clang fp contract(off)
    double Rab[9], E[9], u[3], d[3], phi[3];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) Rab[3 * i + j] = (Rb[3 * i] * Ra[3 * j] + Rb[3 * i + 1] * Ra[3 * j + 1]) + Rb[3 * i + 2] * Ra[3 * j + 2];
#pragma unroll
    for (int i = 0; i < 3; i++) {
        u[i] = (Rab[3 * i] * Ta[0] + Rab[3 * i + 1] * Ta[1]) + Rab[3 * i + 2] * Ta[2];
        d[i] = (Tb[i] - u[i]) - t0[i];
    }
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) E[3 * i + j] = (Rab[3 * i] * R0[3 * j] + Rab[3 * i + 1] * R0[3 * j + 1]) + Rab[3 * i + 2] * R0[3 * j + 2];
    // Log: E - E^T = 2 sin(theta) [n]x, trace = 1 + 2 cos(theta); theta from atan2 (good at both ends), |phi| < pi
    const double v0 = 0.5 * (E[7] - E[5]), v1 = 0.5 * (E[2] - E[6]), v2 = 0.5 * (E[3] - E[1]);
    const double s2 = (v0 * v0 + v1 * v1) + v2 * v2, s = sqrt(s2), c = 0.5 * (((E[0] + E[4]) + E[8]) - 1.0);
    const double theta = atan2(s, c);
    // theta / sin(theta): asin's series in s below 1e-3 (c > 0 there unless theta is at pi, where Log is not defined)
    const double f = (s < 1e-3 && c > 0) ? 1.0 + s2 * (1.0 / 6.0 + s2 * (3.0 / 40.0)) : theta / s;
    phi[0] = f * v0; phi[1] = f * v1; phi[2] = f * v2;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        e[k] = (Lt[3 * k] * d[0] + Lt[3 * k + 1] * d[1]) + Lt[3 * k + 2] * d[2];
        e[3 + k] = (Lr[3 * k] * phi[0] + Lr[3 * k + 1] * phi[1]) + Lr[3 * k + 2] * phi[2];
    }
    if (LIN) {
        const double th2 = theta * theta;
        const double cc = theta < 0.05 ? 1.0 / 12.0 + th2 * (1.0 / 720.0 + th2 * (1.0 / 30240.0 + th2 * (1.0 / 1209600.0)))
                                       : 1.0 / th2 - (1.0 + cos(theta)) / (2.0 * theta * sin(theta));
        const double P[9] = {0, -phi[2], phi[1], phi[2], 0, -phi[0], -phi[1], phi[0], 0};
        const double Tx[9] = {0, -Ta[2], Ta[1], Ta[2], 0, -Ta[0], -Ta[1], Ta[0], 0};
        const double Ux[9] = {0, -u[2], u[1], u[2], 0, -u[0], -u[1], u[0], 0};
        double Ji[9], At[18], Ar[9]; // Jl^-1; -R_ab | -R_ab [T_a]x; -Jl^-1 R_ab
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = 0; j < 3; j++) {
                const double p2 = (P[3 * i] * P[j] + P[3 * i + 1] * P[3 + j]) + P[3 * i + 2] * P[6 + j];
                Ji[3 * i + j] = ((i == j ? 1.0 : 0.0) - 0.5 * P[3 * i + j]) + cc * p2;
            }
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = 0; j < 3; j++) {
                At[6 * i + j] = -Rab[3 * i + j];
                At[6 * i + 3 + j] = -((Rab[3 * i] * Tx[j] + Rab[3 * i + 1] * Tx[3 + j]) + Rab[3 * i + 2] * Tx[6 + j]);
                Ar[3 * i + j] = -((Ji[3 * i] * Rab[j] + Ji[3 * i + 1] * Rab[3 + j]) + Ji[3 * i + 2] * Rab[6 + j]);
            }
#pragma unroll
        for (int k = 0; k < 3; k++)
#pragma unroll
            for (int j = 0; j < 3; j++) {
                Ja[6 * k + j] = (Lt[3 * k] * At[j] + Lt[3 * k + 1] * At[6 + j]) + Lt[3 * k + 2] * At[12 + j];
                Ja[6 * k + 3 + j] = (Lt[3 * k] * At[3 + j] + Lt[3 * k + 1] * At[9 + j]) + Lt[3 * k + 2] * At[15 + j];
                Ja[6 * (3 + k) + j] = 0.0;
                Ja[6 * (3 + k) + 3 + j] = (Lr[3 * k] * Ar[j] + Lr[3 * k + 1] * Ar[3 + j]) + Lr[3 * k + 2] * Ar[6 + j];
                Jb[6 * k + j] = Lt[3 * k + j];
                Jb[6 * k + 3 + j] = (Lt[3 * k] * Ux[j] + Lt[3 * k + 1] * Ux[3 + j]) + Lt[3 * k + 2] * Ux[6 + j];
                Jb[6 * (3 + k) + j] = 0.0;
                Jb[6 * (3 + k) + 3 + j] = (Lr[3 * k] * Ji[j] + Lr[3 * k + 1] * Ji[3 + j]) + Lr[3 * k + 2] * Ji[6 + j];
            }
    }
}

// X^T Y of two 6 x 6 (row-major, rows = the six residual rows), entry (r, c), summed over the rows in order
__device__ __forceinline__ double ba_relpose_dot(const double (&X)[36], const double (&Y)[36], int r, int c)
{
#pragma clang fp contract(off)
    double a = X[r] * Y[c];
#pragma unroll
    for (int k = 1; k < 6; k++) a = a + X[6 * k + r] * Y[6 * k + c];
    return a;
}

// LIN = false (the trial part): the constraint energies at cam (xTest) as block partials part_e[2][gridDim.x] -- rotation, translation.
// LIN = true (the linearisation part, behind k_prior, in front of k_relpose_gather and the first elimination): also the records and a
// second copy of the partials in part_keep (ba_solver_relative_pose_energy: a trial overwrites part_e).  MASK: the columns of the
// parameters held constant are zero in everything stored, by the mask words of k_eval<MASK>; the constraint still counts in the energy.
template <typename T, bool LIN, bool MASK = false>
__global__ __launch_bounds__(256) void k_relpose(ba_relpose_args<T> ra, int N, const T *__restrict__ cam, T *__restrict__ rec,
                                                 T *__restrict__ part_e, T *__restrict__ part_keep, const int *__restrict__ go,
                                                 const unsigned short *__restrict__ cmask)
{
    __shared__ T red[4];
    if (go && *go == 0) return; // (uniform) the trial in front of this linearisation was rejected
    const int t = blockIdx.x * 256 + threadIdx.x;
    T er = 0, et = 0;
    if (t < ra.n) {
        const int a = ra.pair[2 * t], b = ra.pair[2 * t + 1];
        double Ra[9], Rb[9], R0[9], Lr[9], Lt[9], Ta[3], Tb[3], t0[3], e[6], Ja[36], Jb[36];
#pragma unroll
        for (int q = 0; q < 9; q++) {
            Ra[q] = (double)cam[(size_t)q * N + a]; Rb[q] = (double)cam[(size_t)q * N + b];
            R0[q] = (double)ra.R0[9 * (size_t)t + q]; Lr[q] = (double)ra.Lr[9 * (size_t)t + q]; Lt[q] = (double)ra.Lt[9 * (size_t)t + q];
        }
#pragma unroll
        for (int q = 0; q < 3; q++) {
            Ta[q] = (double)cam[(size_t)(9 + q) * N + a]; Tb[q] = (double)cam[(size_t)(9 + q) * N + b];
            t0[q] = (double)ra.t0[3 * (size_t)t + q];
        }
        ba_relpose_eval<LIN>(Ra, Ta, Rb, Tb, R0, t0, Lr, Lt, e, Ja, Jb);
        {
#pragma clang fp contract(off)
            et = (T)((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]);
            er = (T)((e[3] * e[3] + e[4] * e[4]) + e[5] * e[5]);
        }
        if (LIN) {
            if (MASK) {
                const unsigned ma = cmask[a], mb = cmask[b];
#pragma unroll
                for (int c = 0; c < 6; c++) {
                    if ((ma >> c) & 1u) {
#pragma unroll
                        for (int k = 0; k < 6; k++) Ja[6 * k + c] = 0.0;
                    }
                    if ((mb >> c) & 1u) {
#pragma unroll
                        for (int k = 0; k < 6; k++) Jb[6 * k + c] = 0.0;
                    }
                }
            }
            T *o = rec + (size_t)t * BA_RP_REC;
#pragma unroll
            for (int r = 0; r < 6; r++) {
#pragma unroll
                for (int c = 0; c <= r; c++) { // the lower triangle, mirrored: the records are symmetric in bits
                    const T haa = (T)ba_relpose_dot(Ja, Ja, r, c), hbb = (T)ba_relpose_dot(Jb, Jb, r, c);
                    o[6 * r + c] = haa; o[6 * c + r] = haa;
                    o[36 + 6 * r + c] = hbb; o[36 + 6 * c + r] = hbb;
                }
#pragma unroll
                for (int c = 0; c < 6; c++) o[BA_RP_HAB + 6 * r + c] = (T)ba_relpose_dot(Ja, Jb, r, c);
                double ga = Ja[r] * e[0], gb = Jb[r] * e[0];
#pragma unroll
                for (int k = 1; k < 6; k++) { ga = ga + Ja[6 * k + r] * e[k]; gb = gb + Jb[6 * k + r] * e[k]; }
                o[BA_RP_G + r] = (T)(-ga);
                o[BA_RP_G + 6 + r] = (T)(-gb);
            }
        }
    }
    const size_t g = gridDim.x;
    er = block_reduce<T, false>(er, red);
    et = block_reduce<T, false>(et, red);
    if (threadIdx.x == 0) {
        part_e[blockIdx.x] = er; part_e[g + blockIdx.x] = et;
        if (LIN) { part_keep[blockIdx.x] = er; part_keep[g + blockIdx.x] = et; }
    }
}

// One thread per (camera, entry): entries 0..35 the 6 x 6 pose corner of V_a (row-major r, c), 36..41 gc_a.  Behind k_relpose<T, true>.
template <typename T>
__global__ __launch_bounds__(256) void k_relpose_gather(int N, ba_relpose_csr<T> cs, T *__restrict__ V, T *__restrict__ gc, const int *__restrict__ go)
{
    if (go && *go == 0) return;
    const int idx = blockIdx.x * 256 + threadIdx.x;
    const int a = idx / BA_RP_ENT, e = idx - a * BA_RP_ENT;
    if (a >= N) return;
    const int k0 = cs.ptr[a], k1 = cs.ptr[a + 1];
    if (k0 == k1) return;
    T *dst = e < 36 ? V + (size_t)a * 81 + 9 * (e / 6) + (e % 6) : gc + 9 * (size_t)a + (e - 36);
    T v = *dst;
    for (int k = k0; k < k1; k++) {
        const int w = cs.inc[k], side = w & 1;
        const T *o = cs.rec + (size_t)(w >> 1) * BA_RP_REC;
        v = v + (e < 36 ? o[36 * side + e] : o[BA_RP_G + 6 * side + (e - 36)]);
    }
    *dst = v;
}

// BA_CHOLESKY, behind the Schur assembly (every block of this trial's S is written) and in front of the factorisation: the cross
// block of every constraint into the lower block triangle, S[(9 lo + c) ld + 9 hi + r] += (J_hi^T J_lo)[r][c].
template <typename T>
__global__ __launch_bounds__(256) void k_relpose_schur(int n, const int *__restrict__ pair, const T *__restrict__ rec, int ld, T *__restrict__ S)
{
    const int idx = blockIdx.x * 256 + threadIdx.x;
    const int t = idx / 36, e = idx - 36 * t;
    if (t >= n) return;
    const int a = pair[2 * t], b = pair[2 * t + 1], r = e / 6, c = e - 6 * r;
    const T *H = rec + (size_t)t * BA_RP_REC + BA_RP_HAB;
    const int hi = a > b ? a : b, lo = a > b ? b : a;
    const T h = a > b ? H[6 * r + c] : H[6 * c + r];
    T *dst = S + (size_t)(9 * lo + c) * ld + 9 * hi + r;
    *dst = *dst + h;
}

// BA_ITERSCHUR: row r of  sum over the incident constraints of camera a  H_ab v_b  (H_ba = H_ab^T), CSR order; v through `val`
template <typename T, typename F>
__device__ __forceinline__ T ba_relpose_matvec_row(const ba_relpose_csr<T> &cs, int a, int r, F val)
{
    T acc = 0;
    if (r >= 6) return acc;
    for (int k = cs.ptr[a], k1 = cs.ptr[a + 1]; k < k1; k++) {
        const int w = cs.inc[k], side = w & 1, t = w >> 1;
        const int other = cs.pair[2 * t + 1 - side];
        const T *H = cs.rec + (size_t)t * BA_RP_REC + BA_RP_HAB;
        T s = 0;
#pragma unroll
        for (int q = 0; q < 6; q++) s += (side ? H[6 * q + r] : H[6 * r + q]) * val(9 * (size_t)other + q);
        acc += s;
    }
    return acc;
}

#endif
