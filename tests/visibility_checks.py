"""Yardstick of BA_PRECOND_VISIBILITY_FOREST (ba_solver_set_preconditioner, ba_problem_covisibility; include/ba_mi355x.h, DESIGN.md
section 16) -- TEST INFRASTRUCTURE ONLY (tests/test_visibility_checks.py, tests/test_gpu_visibility_forest.py), restated from the rule
and not taken from the library.

Co-visibility: the weight of a camera pair (a < b) is the number of points that put it together.  A point seen by t <= track_max
distinct cameras adds 1 to each of its t (t - 1) / 2 pairs, a longer track only to the t - 1 pairs adjacent in ascending camera index; a
camera that sees a point twice counts once.  The list is ordered by (weight descending, a, b).

The forest is forest_checks.plan on L = the relative-pose pairs in list order, then the co-visibility pairs.  The preconditioner, with
B [N, 9, 9] the block-Jacobi blocks and X [len(L), 9, 9] the blocks S[a, b] of the reduced camera matrix for the kept (a, b) of L:

    M = blockdiag(B) + sum over the kept (a, b) of X_ab at block (a, b) and X_ab' at (b, a)

factored and applied as forest_checks does, with whole 9 x 9 cross blocks (forest_checks.apply and .pcg are used as they are: they never
look at the width).  M is not positive definite for every S; `working` counts the trees that fall back like the library's.

The keyword arguments narrow and skip_update (factor) and drop_backward (forest_checks.apply) plant the defects
tests/test_visibility_checks.py uses to show that the bound of the GPU test has teeth; nothing else passes them.
"""
import numpy as np

import forest_checks as FC
import pcg_checks as PC

LD = np.longdouble
TRACK_MAX_DEFAULT = 64


# ---- co-visibility -------------------------------------------------------------------------------------------------------------------------
def covisibility(N, cam_idx, pt_idx, track_max=0):
    """(pairs [n, 2] int32 with a < b, weight [n] int32) by brute force over the points."""
    track_max = track_max or TRACK_MAX_DEFAULT
    seen = {}
    for c, j in zip(np.asarray(cam_idx).tolist(), np.asarray(pt_idx).tolist()):
        seen.setdefault(j, set()).add(c)
    w = {}
    for cams in seen.values():
        cams = sorted(cams)
        t = len(cams)
        if t <= track_max:
            both = [(cams[i], cams[k]) for i in range(t) for k in range(i + 1, t)]
        else:
            both = [(cams[i], cams[i + 1]) for i in range(t - 1)]
        for ab in both:
            w[ab] = w.get(ab, 0) + 1
    items = sorted(w.items(), key=lambda kv: (-kv[1], kv[0][0], kv[0][1]))
    pairs = np.array([kv[0] for kv in items], np.int32).reshape(-1, 2)
    return pairs, np.array([kv[1] for kv in items], np.int32)


def edge_list(rp_pairs, cov_pairs):
    """L: the relative-pose pairs in list order, then the co-visibility pairs."""
    return np.concatenate([np.asarray(rp_pairs, np.int64).reshape(-1, 2), np.asarray(cov_pairs, np.int64).reshape(-1, 2)])


def plan(N, rp_pairs, cov_pairs, max_tree):
    """(forest_checks.plan on L, L)."""
    L = edge_list(rp_pairs, cov_pairs)
    return FC.plan(N, L, max_tree), L


# ---- the preconditioner ----------------------------------------------------------------------------------------------------------------------
def cross_blocks(S, L, kept):
    """X [len(L), 9, 9] in the dtype of S: S[a, b] for the kept (a, b) of L, zero for the others."""
    S = np.asarray(S)
    X = np.zeros((len(L), 9, 9), S.dtype)
    for q, (a, b) in enumerate(L):
        if kept[q]:
            X[q] = S[9 * a:9 * a + 9, 9 * b:9 * b + 9]
    return X


def cross9(X, L, q, node):
    """C = M[node, other] of the entry q of L: X_ab when the node is a, X_ab' when it is b."""
    return X[q] if int(L[q][0]) == int(node) else X[q].T


def dense_M(B, X, L, kept):
    B = np.asarray(B)
    N = len(B)
    M = np.zeros((9 * N, 9 * N), B.dtype)
    for a in range(N):
        M[9 * a:9 * a + 9, 9 * a:9 * a + 9] = B[a]
    for q, (a, b) in enumerate(L):
        if kept[q]:
            M[9 * a:9 * a + 9, 9 * b:9 * b + 9] += X[q]
            M[9 * b:9 * b + 9, 9 * a:9 * a + 9] += X[q].T
    return M


def factor(B, X, L, pl, dt=LD, skip_update=None, narrow=False):
    """forest_checks.factor with 9 x 9 cross blocks: (Dinv [N, 9, 9], G [N, 9, 9], ok [N]) in dt.  The planted defects: narrow, rows and
    columns 6 .. 8 of every cross block dropped (the 6-wide path); skip_update (a camera), that child's C'G is not subtracted from
    its parent's D."""
    D = np.array(B, dt)
    Xd = np.asarray(X, dt)
    N = len(D)
    Dinv, G, ok = np.zeros((N, 9, 9), dt), np.zeros((N, 9, 9), dt), np.ones(N, bool)
    for i in pl["order"]:
        Dinv[i], ok[i] = FC._inv9(D[i], dt)
        p = pl["parent"][i]
        if p >= 0:
            C = np.array(cross9(Xd, L, pl["via"][i], i))
            if narrow:
                C[6:, :] = 0
                C[:, 6:] = 0
            G[i] = Dinv[i] @ C
            if skip_update is None or i != skip_update:
                D[p] -= C.T @ G[i]
    return Dinv, G, ok


def working(B, X, L, pl, dtype):
    """The library's factor for a solver of scalar type `dtype` (forest_checks.working): B and X rounded to it, the factor in float64,
    D^-1 and G rounded to dtype; a tree with a block that is not positive definite in float64 on the block-Jacobi inverses, G = 0.
    Returns (Dinv, G, the number of such trees)."""
    Bw, Xw = np.asarray(B).astype(dtype).astype(np.float64), np.asarray(X).astype(dtype).astype(np.float64)
    Dinv, G, ok = factor(Bw, Xw, L, pl, np.float64)
    bad = 0
    for t in pl["trees"]:
        if not ok[t].all():
            bad += 1
            for a in t:
                Dinv[a], pd = FC._inv9(Bw[a], np.float64)
                if not pd:
                    Dinv[a] = PC.diagonal_inverse(Bw[a][None])[0]
                G[a] = 0
    return Dinv.astype(dtype), G.astype(dtype), bad


def min_eig(M):
    """The smallest eigenvalue of the diagonally scaled M (float64)."""
    M = np.asarray(M, np.float64)
    d = 1 / np.sqrt(np.diagonal(M))
    return float(np.linalg.eigvalsh(M * d[:, None] * d[None, :]).min())


# ---- the problems and cases of the GPU test (tests/test_visibility_checks.py checks their inputs on the CPU) ------------------------------
def twice_problem(ba):
    """synthetic(5, 60, 200, 3) with one (camera, point 7) observed three times (test_pcg_checks.py's), as a library Problem."""
    p = ba.Problem.synthetic(5, 60, 200, 3)
    a = p.arrays()
    src = int(np.nonzero(a["pt_idx"] == 7)[0][0])
    cam_idx = np.concatenate([a["cam_idx"], [a["cam_idx"][src]] * 2])
    pt_idx = np.concatenate([a["pt_idx"], [7, 7]])
    m = a["meas"].reshape(-1, 2)
    meas = np.concatenate([m, m[src] + [[0.3, -0.2], [-0.1, 0.4]]])
    return ba.Problem.from_arrays(p.N, p.M, p.K + 2, cam_idx, pt_idx, meas.ravel(), a["cams9"], a["pts"])


# name: (problem, max_tree (0: N), relative-pose constraints, the root's pose fixed)
GPU_CASES = {
    "p21-one-tree": ("p21", 0, False, False),
    "p21-cut-at-4": ("p21", 4, False, False),
    "ragged-cut-at-5": ("ragged", 5, False, False),
    "syn257-trees-of-64": ("syn257", 64, False, False),
    "syn257-one-tree": ("syn257", 0, False, False),
    "p21-constraints": ("p21", 0, True, False),
    "p21-root-fixed": ("p21", 0, False, True),
    "twice-one-tree": ("twice", 0, False, False),
}
LAM_REL = 1e-6
