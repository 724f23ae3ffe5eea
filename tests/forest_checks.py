"""Yardstick of BA_PRECOND_CONSTRAINT_FOREST (ba_solver_set_preconditioner; include/ba_mi355x.h) -- TEST
INFRASTRUCTURE ONLY (tests/test_forest_checks.py, tests/test_gpu_forest_precond.py), restated from the rule and not taken from the library.

The forest of a constraint list `pairs` ([n, 2] cameras a, b) with at most max_tree cameras per tree:

    the constraints in list order through a union-find; one is KEPT when it joins two components and the merged one has at most
    max_tree cameras; a tree's root is its lowest camera; its nodes in breadth-first order from the root, a node's neighbours in list
    order; eliminated in the reverse of that order (children before parents); the trees by ascending root, lone cameras last.

The preconditioner, with B [N, 9, 9] the block-Jacobi blocks and H [n, 6, 6] the constraints' cross blocks H_ab = J_a'J_b:

    M = blockdiag(B) + sum over the kept (a, b) of H_ab at the pose corner of block (a, b) and H_ab' at (b, a)
    factor   in elimination order, C_i = M[i, parent(i)]:  D_i = B_i - sum over the children c of C_c' G_c,  G_i = D_i^-1 C_i  (9 x 6)
    apply    forward in elimination order   u_i = r_i - sum over the children G_c' u_c
             backward in the reverse        z_i = D_i^-1 u_i - G_i z_parent(i)

in np.longdouble the reference; `working`: the library's arithmetic -- the factor in float64 for both scalar types, D^-1 and G rounded
to the working precision, the sweeps in it.  pcg() is pcg_checks.pcg with the preconditioner as a callback.

The keyword arguments skip_update (factor), drop_backward (apply) and rz_rows (pcg) plant the defects tests/test_forest_checks.py uses to
show that the metrics of the GPU test have teeth; nothing else passes them.
"""
import numpy as np

import pcg_checks as PC

LD = np.longdouble


# ---- the forest ------------------------------------------------------------------------------------------------------------------------
def plan(N, pairs, max_tree):
    """dict(parent [N], via [N], order [N], kept [n] bool, trees: the cameras of each tree in elimination order)."""
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    comp = {a: {a} for a in range(N)}  # camera -> the set of its component (shared by its members)
    kept = np.zeros(len(pairs), bool)
    nb = [[] for _ in range(N)]  # kept neighbours, list order: (other camera, constraint)
    for q, (a, b) in enumerate(pairs):
        a, b = int(a), int(b)
        if comp[a] is comp[b] or len(comp[a]) + len(comp[b]) > max_tree:
            continue
        kept[q] = True
        merged = comp[a] | comp[b]
        for c in merged:
            comp[c] = merged
        nb[a].append((b, q))
        nb[b].append((a, q))
    parent, via = np.full(N, -1, np.int64), np.full(N, -1, np.int64)
    order, trees, done = [], [], set()
    for root in range(N):
        if root in done or not nb[root]:
            continue
        bfs = [root]
        done.add(root)
        for c in bfs:  # (grows while it is walked)
            for o, q in nb[c]:
                if o not in done:
                    done.add(o)
                    parent[o], via[o] = c, q
                    bfs.append(o)
        trees.append(bfs[::-1])
        order += bfs[::-1]
    order += [a for a in range(N) if a not in done]
    return dict(parent=parent, via=via, order=np.array(order, np.int64), kept=kept, trees=trees)


def counts(pl):
    """(trees with >= 2 cameras, kept, dropped, cameras of the largest tree) -- ba_solver_preconditioner_info's out6[2:]."""
    return len(pl["trees"]), int(pl["kept"].sum()), int((~pl["kept"]).sum()), max([len(t) for t in pl["trees"]] + [1])


def cross9(H, pairs, q, node):
    """C = M[node, other] of constraint q, 9 x 9: H_ab in the pose corner when the node is a, H_ab' when it is b."""
    C = np.zeros((9, 9), np.asarray(H).dtype)
    C[:6, :6] = H[q] if int(pairs[q][0]) == int(node) else H[q].T
    return C


def dense_M(B, H, pairs, kept):
    B, H = np.asarray(B), np.asarray(H)
    N = len(B)
    M = np.zeros((9 * N, 9 * N), B.dtype)
    for a in range(N):
        M[9 * a:9 * a + 9, 9 * a:9 * a + 9] = B[a]
    for q, (a, b) in enumerate(np.asarray(pairs).reshape(-1, 2)):
        if kept[q]:
            M[9 * a:9 * a + 6, 9 * b:9 * b + 6] += H[q]
            M[9 * b:9 * b + 6, 9 * a:9 * a + 6] += H[q].T
    return M


def _inv9(A, dt):
    Mi, ok = PC.invert_blocks(np.asarray(A)[None], dt)
    return Mi[0], bool(ok[0])


def factor(B, H, pairs, pl, dt=LD, skip_update=None):
    """(Dinv [N, 9, 9], G [N, 9, 9] (columns 6 .. 8 zero; zero at roots and lone cameras), ok [N]) in dt.  Lone cameras: the inverse of
    B_a.  ok[a] False: D_a is not positive definite in dt.  skip_update (a camera): the planted defect, that child's C'G is not
    subtracted from its parent's D."""
    pairs = np.asarray(pairs).reshape(-1, 2)
    D = np.array(B, dt)
    Hd = np.asarray(H, dt)
    N = len(D)
    Dinv, G, ok = np.zeros((N, 9, 9), dt), np.zeros((N, 9, 9), dt), np.ones(N, bool)
    for i in pl["order"]:
        Dinv[i], ok[i] = _inv9(D[i], dt)
        p = pl["parent"][i]
        if p >= 0:
            C = cross9(Hd, pairs, pl["via"][i], i)
            G[i] = Dinv[i] @ C
            if skip_update is None or i != skip_update:
                D[p] -= C.T @ G[i]
    return Dinv, G, ok


def apply(pl, Dinv, G, r, drop_backward=False):
    """z = M^-1 r by the two sweeps, in the dtype of Dinv.  drop_backward: the planted defect, z_i = D_i^-1 u_i."""
    dt = Dinv.dtype.type
    N = len(Dinv)
    u = np.array(r, dt).reshape(N, 9).copy()
    for i in pl["order"]:
        p = pl["parent"][i]
        if p >= 0:
            u[p] -= G[i].T @ u[i]
    z = np.zeros_like(u)
    for i in pl["order"][::-1]:
        z[i] = Dinv[i] @ u[i]
        p = pl["parent"][i]
        if p >= 0 and not drop_backward:
            z[i] -= G[i] @ z[p]
    return z.reshape(-1)


def working(B, H, pairs, pl, dtype, Minv_bj=None):
    """The library's factor for a solver of scalar type `dtype`: B and H rounded to it, the factor in float64, D^-1 and G rounded to
    dtype.  A tree with a block that is not positive definite in float64 uses the block-Jacobi inverses (G = 0).  Returns (Dinv, G,
    the number of such trees)."""
    Bw, Hw = np.asarray(B).astype(dtype).astype(np.float64), np.asarray(H).astype(dtype).astype(np.float64)
    Dinv, G, ok = factor(Bw, Hw, pairs, pl, np.float64)
    bad = 0
    for t in pl["trees"]:
        if not ok[t].all():
            bad += 1
            for a in t:
                Dinv[a], pd = _inv9(Bw[a], np.float64)
                if not pd:
                    Dinv[a] = PC.diagonal_inverse(Bw[a][None])[0]
                G[a] = 0
    return Dinv.astype(dtype), G.astype(dtype), bad


# ---- PCG with any preconditioner ----------------------------------------------------------------------------------------------------------
def pcg(S, rhs, prec, max_iter, rel_tol=0.0, dtype=LD, keep=None, V=None, rz_rows=None):
    """pcg_checks.pcg's recurrence with z = prec(r) a callback.  V ([N, 9, 9]): the product the matrix-free way, V p - (V - S) p, both
    terms rounded to dtype (pcg_checks.pcg).  rz_rows (bool mask): the planted defect, only those rows enter r'z."""
    b = np.asarray(rhs, dtype)
    keep = set(keep or ())
    if V is None:
        Sd = np.asarray(S, dtype)
        product = lambda p: Sd @ p
    else:
        N = len(V)
        Vd = np.asarray(V, dtype)
        E = PC._minus_blocks(np.asarray(S, LD), np.asarray(V, LD)).astype(dtype)
        product = lambda p: np.einsum("nij,nj->ni", Vd, p.reshape(N, 9)).reshape(-1) - E @ p
    tol2 = dtype(rel_tol) * dtype(rel_tol)
    dot_rz = (lambda r, z: (r * z).sum()) if rz_rows is None else (lambda r, z: (r[rz_rows] * z[rz_rows]).sum())
    x, r, p = np.zeros_like(b), b.copy(), np.zeros_like(b)
    z = np.asarray(prec(r), dtype)
    bb = (b * b).sum()
    rz, rr = [dot_rz(r, z)], [(r * r).sum()]
    xs, k, conv = {}, 0, False
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        while True:
            if rr[k] <= tol2 * bb:
                conv = True
                break
            if k == max_iter:
                break
            p = z + (dtype(0) if k == 0 else rz[k] / rz[k - 1]) * p
            y = product(p)
            alpha = rz[k] / (p * y).sum()
            x = x + alpha * p
            r = r - alpha * y
            z = np.asarray(prec(r), dtype)
            rz.append(dot_rz(r, z))
            rr.append((r * r).sum())
            k += 1
            if k in keep:
                xs[k] = x.copy()
    return dict(x=x, iters=k, converged=conv, xs=xs, rr=np.array([float(v / bb) for v in rr]))


def block_jacobi(Minv):
    Mi = np.asarray(Minv)
    return lambda r: np.einsum("nij,nj->ni", Mi, r.reshape(len(Mi), 9)).reshape(-1)


def forest(pl, Dinv, G):
    return lambda r: apply(pl, Dinv, G, r)


# ---- a synthetic system for the CPU tests --------------------------------------------------------------------------------------------------
def synthetic(N, pairs, seed, stiff=1.0, coupling=0.05):
    """(S [9N, 9N], rhs, B [N, 9, 9], H [n, 6, 6]) long double: S = blockdiag(P_a) + a weak symmetric coupling of all cameras (the part
    a Schur complement of points leaves) + the constraints' J'J with J = stiff x a seeded 6 x 12; B its diagonal blocks."""
    rng = np.random.default_rng(seed)
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    D = 9 * N
    W = rng.standard_normal((D, 3))
    S = (coupling * (W @ W.T)).astype(LD)
    for a in range(N):
        A = rng.standard_normal((9, 9))
        S[9 * a:9 * a + 9, 9 * a:9 * a + 9] += (A @ A.T + 0.5 * np.eye(9)).astype(LD)
    H = np.zeros((len(pairs), 6, 6), LD)
    for q, (a, b) in enumerate(pairs):
        J = (stiff * rng.standard_normal((6, 12))).astype(LD)
        Ja, Jb = J[:, :6], J[:, 6:]
        S[9 * a:9 * a + 6, 9 * a:9 * a + 6] += Ja.T @ Ja
        S[9 * b:9 * b + 6, 9 * b:9 * b + 6] += Jb.T @ Jb
        S[9 * a:9 * a + 6, 9 * b:9 * b + 6] += Ja.T @ Jb
        S[9 * b:9 * b + 6, 9 * a:9 * a + 6] += Jb.T @ Ja
        H[q] += Ja.T @ Jb
    B = PC.exact_blocks(S, N).astype(LD)
    rhs = rng.standard_normal(D).astype(LD)
    return S, rhs, B, H
