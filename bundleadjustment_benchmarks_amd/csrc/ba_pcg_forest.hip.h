// ba_pcg_forest.hip.h -- BA_PRECOND_CONSTRAINT_FOREST: the block-Jacobi preconditioner of ba_pcg.hip.h plus the cross blocks of a
// spanning forest of the relative-pose constraints (ba_mi355x.h states the forest rule, DESIGN.md section 15 the measurements).
//
//   M = blockdiag(B_a) + sum over the kept constraints (a, b) of X_ab at (a, b) and X_ab^T at (b, a),  X_ab = H_ab in the pose corner
//
// M is positive definite for every subset of kept edges (blockdiag(S_points + lambda I) + the kept edges' whole PSD matrices + the
// dropped edges' PSD diagonal parts), and on a forest its block LDL^T has no fill.  With the nodes of a tree in elimination order
// (children before parents; the host lays the lists out that way, tree after tree) and C_i = M_{i, parent(i)}:
//
//   factor (once per trial, fp64 for both scalar types)   D_i = B_i - sum over the children c of C_c^T G_c,  G_i = D_i^-1 C_i (9 x 6)
//   apply z = M^-1 r (z_0 and every iteration)            forward, elimination order:   u_i = r_i - sum over the children G_c^T u_c
//                                                         backward, the reverse:        z_i = D_i^-1 u_i - G_i z_parent(i)
//
// One workgroup of one wavefront per tree, the nodes of the tree one after the other, lanes over the entries of the 9 x 9 and 9 x 6
// products; trees do not talk to each other, so there is no wait and no atomic here.  The running vector u (then z) of a tree of at
// most BA_FOREST_LDS cameras lives in LDS, a longer one in a global scratch buffer at the same indices (the same code through a flat
// pointer).  The order of the nodes is static, so the rows of the next node's D^-1 and G are loaded before the current node's
// products.  The tree's share of r'z is summed in node order per row and then over the nine rows in row order into one partial per
// tree, behind the per-camera launches' partials (ba_pcg.hip.h: every consumer sums the longer list in the same order).
// A tree with a pivot that is not positive in working precision has bad[tree] set and runs that solve with the block-Jacobi inverse
// of each of its B_a (k_pcg_prec_inv's arithmetic and its diagonal fallback) and G = 0.
#ifndef BA_PCG_FOREST_HIP_H
#define BA_PCG_FOREST_HIP_H

#include "ba_kernels.hip.h"
#include "ba_relpose.hip.h"

#define BA_FOREST_FAC 135 /* per node: D^-1 (81, row-major) | G (54, 9 x 6 row-major) */
#define BA_FOREST_LDS 256 /* cameras of a tree whose running vector fits the workgroup's LDS */

struct ba_pcg_dev;

template <typename T> struct ba_forest_dev {
    const int *tree_ptr; // [trees + 1] node positions
    const int *node_cam; // [nodes] elimination order, tree after tree
    const int *node_par; // [nodes] position of the parent, -1 at a root
    const int *node_rec; // [nodes] 2 * constraint + (0: the node is the record's a, 1: its b), -1 at a root
    T *fac;              // [nodes][BA_FOREST_FAC]
    double *work;        // [nodes][81] D_i while the tree is factored
    T *u;                // [nodes][9] running vectors of the trees above BA_FOREST_LDS cameras
    int *bad;            // [trees] the last factorisation fell back
};

// A (9 x 9 in LDS, lower triangle read) <- A^-1 = L^-T L^-1 (both triangles, symmetric in bits), X: 81 doubles of LDS scratch.
// Every lane of the 64 calls it behind a barrier; the return value (all pivots positive) is the same in every lane.
__device__ __forceinline__ bool ba_forest_invert9(double *A, double *X, int l)
{
    bool ok = true;
    for (int j = 0; j < 9; j++) {
        const double d = A[10 * j];
        ok = ok && d > 0;
        const double ljj = d > 0 ? sqrt(d) : 1.0;
        __syncthreads();
        if (l >= j && l < 9) A[9 * l + j] = l == j ? ljj : A[9 * l + j] / ljj;
        __syncthreads();
        for (int e = l; e < 81; e += 64) {
            const int i = e / 9, k = e - 9 * i;
            if (k > j && k <= i) A[e] -= A[9 * i + j] * A[9 * k + j];
        }
        __syncthreads();
    }
    if (l < 9) { // column l of L^-1
        X[10 * l] = 1.0 / A[10 * l];
        for (int i = l + 1; i < 9; i++) {
            double s = 0;
            for (int k = l; k < i; k++) s += A[9 * i + k] * X[9 * k + l];
            X[9 * i + l] = -s / A[10 * i];
        }
    }
    __syncthreads();
    for (int e = l; e < 81; e += 64) {
        const int i = e / 9, k = e - 9 * i, hi = i > k ? i : k, lo = i > k ? k : i;
        double s = 0;
        for (int q = hi; q < 9; q++) s += X[9 * q + hi] * X[9 * q + lo];
        A[e] = s;
    }
    __syncthreads();
    return ok;
}

// Behind k_pcg_prec_reduce (Bm = B_a) and in front of k_pcg_prec_inv (which inverts Bm in place).  grid = trees, block = 64.
template <typename T>
__global__ __launch_bounds__(64) void k_pcg_forest_factor(ba_forest_dev<T> fd, const T *__restrict__ Bm, const T *__restrict__ rec)
{
    __shared__ double A[81], X[81], Cm[36], G[54];
    const int t = blockIdx.x, l = threadIdx.x;
    const int n0 = fd.tree_ptr[t], n1 = fd.tree_ptr[t + 1];
    for (int e = l; e < 81 * (n1 - n0); e += 64) {
        const int i = n0 + e / 81, q = e % 81;
        fd.work[(size_t)i * 81 + q] = (double)Bm[(size_t)fd.node_cam[i] * 81 + q];
    }
    __syncthreads();
    bool ok = true;
    for (int i = n0; i < n1; i++) {
        const int pp = fd.node_par[i];
        for (int e = l; e < 81; e += 64) A[e] = fd.work[(size_t)i * 81 + e];
        if (pp >= 0 && l < 36) { // C_i = M_{i, parent}: H_ab when the node is a, H_ab^T when it is b
            const int w = fd.node_rec[i], r = l / 6, c = l - 6 * r;
            const T *H = rec + (size_t)(w >> 1) * BA_RP_REC + BA_RP_HAB;
            Cm[l] = (double)((w & 1) ? H[6 * c + r] : H[6 * r + c]);
        }
        __syncthreads();
        ok = ba_forest_invert9(A, X, l);
        if (!ok) break; // (uniform)
        if (pp >= 0) {
            if (l < 54) { // G = D^-1 C: rows 6 .. 8 of C are zero
                const int r = l / 6, c = l - 6 * r;
                double s = 0;
#pragma unroll
                for (int q = 0; q < 6; q++) s += A[9 * r + q] * Cm[6 * q + c];
                G[l] = s;
            }
            __syncthreads();
            if (l < 36) { // D_parent -= C^T G, the pose corner
                const int r = l / 6, c = l - 6 * r;
                double s = 0;
#pragma unroll
                for (int q = 0; q < 6; q++) s += Cm[6 * q + r] * G[6 * q + c];
                fd.work[(size_t)pp * 81 + 9 * r + c] -= s;
            }
        }
        T *F = fd.fac + (size_t)i * BA_FOREST_FAC;
        for (int e = l; e < 81; e += 64) F[e] = (T)A[e];
        if (l < 54) F[81 + l] = pp >= 0 ? (T)G[l] : (T)0;
        __syncthreads();
    }
    if (!ok) { // the whole tree on the block-Jacobi inverses of its B_a
        for (int i = n0; i < n1; i++) {
            const T *B = Bm + (size_t)fd.node_cam[i] * 81;
            __syncthreads();
            for (int e = l; e < 81; e += 64) A[e] = (double)B[e];
            __syncthreads();
            const bool pd = ba_forest_invert9(A, X, l);
            T *F = fd.fac + (size_t)i * BA_FOREST_FAC;
            for (int e = l; e < 81; e += 64) {
                double v = A[e];
                if (!pd) { // k_pcg_prec_inv's fallback: the inverse of the diagonal
                    const double d = (double)B[e];
                    v = (e % 10 == 0 && d > 0) ? 1.0 / d : 0.0;
                }
                F[e] = (T)v;
            }
            if (l < 54) F[81 + l] = (T)0;
        }
    }
    if (l == 0) fd.bad[t] = ok ? 0 : 1;
}

// z = M^-1 r on the cameras of the trees, the tree's r'z into part[tree].  grid = trees, block = 64.  START: z_0 (in front of
// k_pcg_start, which clears pcg->done); else behind k_pcg_update, a no-op once the solve has converged.
template <typename T, bool START>
__global__ __launch_bounds__(64) void k_pcg_forest_apply(ba_forest_dev<T> fd, const T *__restrict__ r, T *__restrict__ z, double *__restrict__ part,
                                                         const ba_pcg_dev *__restrict__ pcg)
{
    __shared__ T us[9 * BA_FOREST_LDS];
    __shared__ double red[9];
    if (!START && pcg->done) return; // (uniform)
    const int t = blockIdx.x, l = threadIdx.x;
    const int n0 = fd.tree_ptr[t], nn = fd.tree_ptr[t + 1] - n0;
    const int *cam = fd.node_cam + n0, *par = fd.node_par + n0;
    const T *fac = fd.fac + (size_t)n0 * BA_FOREST_FAC;
    T *u = nn <= BA_FOREST_LDS ? us : fd.u + 9 * (size_t)n0;
    for (int e = l; e < 9 * nn; e += 64) u[e] = r[9 * (size_t)cam[e / 9] + e % 9];
    __syncthreads();
    // forward: u_parent -= G_i^T u_i (lane c < 6: column c of G_i); u_i is final when its turn comes
    {
        T gn[9];
        int pn = par[0];
#pragma unroll
        for (int q = 0; q < 9; q++) gn[q] = l < 6 ? fac[81 + 6 * q + l] : (T)0;
        for (int i = 0; i < nn; i++) {
            T g[9];
#pragma unroll
            for (int q = 0; q < 9; q++) g[q] = gn[q];
            const int pp = pn;
            if (i + 1 < nn) { // the next node's column while this one is multiplied
                const T *Fn = fac + (size_t)(i + 1) * BA_FOREST_FAC;
                pn = par[i + 1];
#pragma unroll
                for (int q = 0; q < 9; q++) gn[q] = l < 6 ? Fn[81 + 6 * q + l] : (T)0;
            }
            if (pp >= 0 && l < 6) {
                T s = 0;
#pragma unroll
                for (int q = 0; q < 9; q++) s += g[q] * u[9 * i + q];
                u[9 * (pp - n0) + l] -= s;
            }
            __syncthreads();
        }
    }
    // backward: z_i = D_i^-1 u_i - G_i z_parent (lane row < 9), z over u in place
    double acc = 0;
    {
        const int row = l < 9 ? l : 0;
        T dn[9], gn[6], rn;
        int pn = par[nn - 1], cn = cam[nn - 1];
        {
            const T *Fn = fac + (size_t)(nn - 1) * BA_FOREST_FAC;
#pragma unroll
            for (int q = 0; q < 9; q++) dn[q] = Fn[9 * row + q];
#pragma unroll
            for (int q = 0; q < 6; q++) gn[q] = Fn[81 + 6 * row + q];
            rn = r[9 * (size_t)cn + row];
        }
        for (int i = nn - 1; i >= 0; i--) {
            T d[9], g[6];
#pragma unroll
            for (int q = 0; q < 9; q++) d[q] = dn[q];
#pragma unroll
            for (int q = 0; q < 6; q++) g[q] = gn[q];
            const T ri = rn;
            const int pp = pn, c = cn;
            if (i > 0) {
                const T *Fn = fac + (size_t)(i - 1) * BA_FOREST_FAC;
                pn = par[i - 1]; cn = cam[i - 1];
#pragma unroll
                for (int q = 0; q < 9; q++) dn[q] = Fn[9 * row + q];
#pragma unroll
                for (int q = 0; q < 6; q++) gn[q] = Fn[81 + 6 * row + q];
                rn = r[9 * (size_t)cn + row];
            }
            T s = 0;
#pragma unroll
            for (int q = 0; q < 9; q++) s += d[q] * u[9 * i + q];
            if (pp >= 0) {
                T w = 0;
#pragma unroll
                for (int q = 0; q < 6; q++) w += g[q] * u[9 * (pp - n0) + q];
                s -= w;
            }
            __syncthreads(); // (every lane has read u_i)
            if (l < 9) {
                u[9 * i + l] = s;
                z[9 * (size_t)c + l] = s;
                acc += (double)ri * (double)s;
            }
            __syncthreads();
        }
    }
    if (l < 9) red[l] = acc;
    __syncthreads();
    if (l == 0) {
        double s = red[0];
#pragma unroll
        for (int q = 1; q < 9; q++) s += red[q];
        part[t] = s;
    }
}

#endif
