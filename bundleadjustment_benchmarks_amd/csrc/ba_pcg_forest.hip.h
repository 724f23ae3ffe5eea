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
// tree, behind the per-camera launches' partials (ba_pcg.hip.h: every consumer sums the longer list in the same order; W = 9: one per
// 256 trees, k_pcg_forest_rz).
// A tree with a pivot that is not positive in working precision has bad[tree] set and runs that solve with the block-Jacobi inverse
// of each of its B_a (k_pcg_prec_inv's arithmetic and its diagonal fallback) and G = 0.
//
// BA_PRECOND_VISIBILITY_FOREST is the same factor and sweeps with whole 9 x 9 cross blocks -- the kernels are
// templates over the cross block's width W, 6 above and 9 here (G 9 x 9, D_parent -= C^T G on all 81 entries, nine lanes in the forward
// sweep) -- on a forest of the co-visibility graph, with X_ab = S_ab, the off-diagonal block of the reduced camera matrix:
//
//   X = - sum over the points p seen by both, o in child at p, o' in parent at p, of Z_o diag(dinv_p) Z_o'^T  (+ H_ab in the pose corner)
//
// k_pcg_forest_edges forms it once per trial from the elimination's records, in front of the factor: one workgroup per node, the
// host's list of (o, o') record pairs of the edge to its parent (ascending point, then observation order) cut into three contiguous
// thirds, thread (third, entry) sums its third in list order in fp64, the three partials are added in order.  That M need not be
// positive definite; the tree-wide fallback above is what catches it.
#ifndef BA_PCG_FOREST_HIP_H
#define BA_PCG_FOREST_HIP_H

#include "ba_kernels.hip.h"
#include "ba_relpose.hip.h"

#define BA_FOREST_FAC(W) (81 + 9 * (W)) /* per node: D^-1 (81, row-major) | G (9 x W row-major) */
#define BA_FOREST_LDS 256 /* cameras of a tree whose running vector fits the workgroup's LDS */

struct ba_pcg_dev;

template <typename T> struct ba_forest_dev {
    const int *tree_ptr; // [trees + 1] node positions
    const int *node_cam; // [nodes] elimination order, tree after tree
    const int *node_par; // [nodes] position of the parent, -1 at a root
    const int *node_rec; // [nodes] 2 * constraint + (0: the node is the record's a, 1: its b), -1 at a root
    T *fac;              // [nodes][BA_FOREST_FAC(W)]
    double *work;        // [nodes][81] D_i while the tree is factored
    T *u;                // [nodes][9] running vectors of the trees above BA_FOREST_LDS cameras
    int *bad;            // [trees] the last factorisation fell back
    // W = 9 only
    const int *edge_ptr; // [nodes + 1] the node's range of record pairs (empty at a root)
    const int *edge_oo;  // [pairs][2] records o of the node's camera, o' of its parent's, both at one point
    double *xc;          // [nodes][81] X = M_{node, parent}
};

// The cross blocks of BA_PRECOND_VISIBILITY_FOREST.  grid = nodes, block = 256 (243 at work: 3 thirds of the list x 81 entries).
template <typename T>
__global__ __launch_bounds__(256) void k_pcg_forest_edges(ba_forest_dev<T> fd, const T *__restrict__ rec, const T *__restrict__ rprec)
{
    __shared__ double part[3][81];
    const int i = blockIdx.x, t = threadIdx.x;
    if (fd.node_par[i] < 0) return; // (uniform: a root has no cross block)
    const int e0 = fd.edge_ptr[i], len = fd.edge_ptr[i + 1] - e0;
    const int seg = t / 81, e = t - 81 * seg, r = e / 9, c = e - 9 * r;
    if (seg < 3) {
        const int q0 = e0 + (int)((long long)len * seg / 3), q1 = e0 + (int)((long long)len * (seg + 1) / 3);
        double s = 0;
        for (int q = q0; q < q1; q++) {
            const T *Za = rec + (size_t)fd.edge_oo[2 * (size_t)q] * BA_REC, *Zb = rec + (size_t)fd.edge_oo[2 * (size_t)q + 1] * BA_REC;
            s += (double)Za[3 * r] * (double)Za[BA_REC_DINV] * (double)Zb[3 * c] + (double)Za[3 * r + 1] * (double)Za[BA_REC_DINV + 1] * (double)Zb[3 * c + 1] +
                 (double)Za[3 * r + 2] * (double)Za[BA_REC_DINV + 2] * (double)Zb[3 * c + 2];
        }
        part[seg][e] = s;
    }
    __syncthreads();
    if (t < 81) {
        double x = -((part[0][t] + part[1][t]) + part[2][t]);
        const int w = fd.node_rec[i];
        if (w >= 0 && r < 6 && c < 6) { // a constraint on this pair: H_ab when the node is a, H_ab^T when it is b
            const T *H = rprec + (size_t)(w >> 1) * BA_RP_REC + BA_RP_HAB;
            x += (double)((w & 1) ? H[6 * c + r] : H[6 * r + c]);
        }
        fd.xc[(size_t)i * 81 + t] = x;
    }
}

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
template <typename T, int W = 6>
__global__ __launch_bounds__(64) void k_pcg_forest_factor(ba_forest_dev<T> fd, const T *__restrict__ Bm, const T *__restrict__ rec)
{
    __shared__ double A[81], X[81], Cm[W * W], G[9 * W];
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
        if constexpr (W == 9) { // C_i = M_{i, parent}: k_pcg_forest_edges' X
            if (pp >= 0)
                for (int e = l; e < 81; e += 64) Cm[e] = fd.xc[(size_t)i * 81 + e];
        } else if (pp >= 0 && l < 36) { // C_i = M_{i, parent}: H_ab when the node is a, H_ab^T when it is b
            const int w = fd.node_rec[i], r = l / 6, c = l - 6 * r;
            const T *H = rec + (size_t)(w >> 1) * BA_RP_REC + BA_RP_HAB;
            Cm[l] = (double)((w & 1) ? H[6 * c + r] : H[6 * r + c]);
        }
        __syncthreads();
        ok = ba_forest_invert9(A, X, l);
        if (!ok) break; // (uniform)
        if (pp >= 0) {
            for (int e = l; e < 9 * W; e += 64) { // G = D^-1 C (W = 6: rows 6 .. 8 of C are zero)
                const int r = e / W, c = e - W * r;
                double s = 0;
#pragma unroll
                for (int q = 0; q < W; q++) s += A[9 * r + q] * Cm[W * q + c];
                G[e] = s;
            }
            __syncthreads();
            for (int e = l; e < W * W; e += 64) { // D_parent -= C^T G (W = 6: the pose corner)
                const int r = e / W, c = e - W * r;
                double s = 0;
#pragma unroll
                for (int q = 0; q < W; q++) s += Cm[W * q + r] * G[W * q + c];
                fd.work[(size_t)pp * 81 + 9 * r + c] -= s;
            }
        }
        T *F = fd.fac + (size_t)i * BA_FOREST_FAC(W);
        for (int e = l; e < 81; e += 64) F[e] = (T)A[e];
        for (int e = l; e < 9 * W; e += 64) F[81 + e] = pp >= 0 ? (T)G[e] : (T)0;
        __syncthreads();
    }
    if (!ok) { // the whole tree on the block-Jacobi inverses of its B_a
        for (int i = n0; i < n1; i++) {
            const T *B = Bm + (size_t)fd.node_cam[i] * 81;
            __syncthreads();
            for (int e = l; e < 81; e += 64) A[e] = (double)B[e];
            __syncthreads();
            const bool pd = ba_forest_invert9(A, X, l);
            T *F = fd.fac + (size_t)i * BA_FOREST_FAC(W);
            for (int e = l; e < 81; e += 64) {
                double v = A[e];
                if (!pd) { // k_pcg_prec_inv's fallback: the inverse of the diagonal
                    const double d = (double)B[e];
                    v = (e % 10 == 0 && d > 0) ? 1.0 / d : 0.0;
                }
                F[e] = (T)v;
            }
            for (int e = l; e < 9 * W; e += 64) F[81 + e] = (T)0;
        }
    }
    if (l == 0) fd.bad[t] = ok ? 0 : 1;
}

// z = M^-1 r on the cameras of the trees, the tree's r'z into part[tree].  grid = trees, block = 64 (W = 9: dynamic LDS, see below).  START: z_0 (in front of
// k_pcg_start, which clears pcg->done); else behind k_pcg_update, a no-op once the solve has converged.
template <typename T, bool START, int W = 6>
__global__ __launch_bounds__(64) void k_pcg_forest_apply(ba_forest_dev<T> fd, const T *__restrict__ r, T *__restrict__ z, double *__restrict__ part,
                                                         const ba_pcg_dev *__restrict__ pcg)
{
    // W = 6: the static array of the constraint forest's launches; W = 9: 9 x min(largest tree, BA_FOREST_LDS) scalars of dynamic LDS, so
    // that a forest of many small trees is not held to the few workgroups per CU that the largest possible tree's LDS would allow
    __shared__ T us_fixed[W == 6 ? 9 * BA_FOREST_LDS : 1];
    extern __shared__ double ba_forest_lds[];
    T *us = W == 6 ? us_fixed : reinterpret_cast<T *>(ba_forest_lds);
    __shared__ double red[9];
    if (!START && pcg->done) return; // (uniform)
    const int t = blockIdx.x, l = threadIdx.x;
    const int n0 = fd.tree_ptr[t], nn = fd.tree_ptr[t + 1] - n0;
    const int *cam = fd.node_cam + n0, *par = fd.node_par + n0;
    constexpr int FAC = BA_FOREST_FAC(W);
    const T *fac = fd.fac + (size_t)n0 * FAC;
    T *u = nn <= BA_FOREST_LDS ? us : fd.u + 9 * (size_t)n0;
    for (int e = l; e < 9 * nn; e += 64) u[e] = r[9 * (size_t)cam[e / 9] + e % 9];
    __syncthreads();
    // forward: u_parent -= G_i^T u_i (lane c < W: column c of G_i); u_i is final when its turn comes
    {
        T gn[9];
        int pn = par[0];
#pragma unroll
        for (int q = 0; q < 9; q++) gn[q] = l < W ? fac[81 + W * q + l] : (T)0;
        for (int i = 0; i < nn; i++) {
            T g[9];
#pragma unroll
            for (int q = 0; q < 9; q++) g[q] = gn[q];
            const int pp = pn;
            if (i + 1 < nn) { // the next node's column while this one is multiplied
                const T *Fn = fac + (size_t)(i + 1) * FAC;
                pn = par[i + 1];
#pragma unroll
                for (int q = 0; q < 9; q++) gn[q] = l < W ? Fn[81 + W * q + l] : (T)0;
            }
            if (pp >= 0 && l < W) {
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
        T dn[9], gn[W], rn;
        int pn = par[nn - 1], cn = cam[nn - 1];
        {
            const T *Fn = fac + (size_t)(nn - 1) * FAC;
#pragma unroll
            for (int q = 0; q < 9; q++) dn[q] = Fn[9 * row + q];
#pragma unroll
            for (int q = 0; q < W; q++) gn[q] = Fn[81 + W * row + q];
            rn = r[9 * (size_t)cn + row];
        }
        for (int i = nn - 1; i >= 0; i--) {
            T d[9], g[W];
#pragma unroll
            for (int q = 0; q < 9; q++) d[q] = dn[q];
#pragma unroll
            for (int q = 0; q < W; q++) g[q] = gn[q];
            const T ri = rn;
            const int pp = pn, c = cn;
            if (i > 0) {
                const T *Fn = fac + (size_t)(i - 1) * FAC;
                pn = par[i - 1]; cn = cam[i - 1];
#pragma unroll
                for (int q = 0; q < 9; q++) dn[q] = Fn[9 * row + q];
#pragma unroll
                for (int q = 0; q < W; q++) gn[q] = Fn[81 + W * row + q];
                rn = r[9 * (size_t)cn + row];
            }
            T s = 0;
#pragma unroll
            for (int q = 0; q < 9; q++) s += d[q] * u[9 * i + q];
            if (pp >= 0) {
                T w = 0;
#pragma unroll
                for (int q = 0; q < W; q++) w += g[q] * u[9 * (pp - n0) + q];
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

// BA_PRECOND_VISIBILITY_FOREST has thousands of small trees on a large problem, and every consumer block of r'z sums the whole list of
// partials: the trees' shares (k_pcg_forest_apply<T, START, 9> writes them to a list of their own) are summed here in groups of 256,
// in tree order, one partial per group behind the per-camera ones.  grid = ceil(trees / 256), block = 256.
template <bool START>
__global__ __launch_bounds__(256) void k_pcg_forest_rz(const double *__restrict__ tpart, int ntrees, double *__restrict__ part,
                                                       const ba_pcg_dev *__restrict__ pcg)
{
    __shared__ double red[4];
    if (!START && pcg->done) return; // (uniform)
    const int t = blockIdx.x * 256 + threadIdx.x;
    const double s = block_reduce<double, false>(t < ntrees ? tpart[t] : 0.0, red);
    if (threadIdx.x == 0) part[blockIdx.x] = s;
}

#endif
