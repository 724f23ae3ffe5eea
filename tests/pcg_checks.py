"""BA_ITERSCHUR's PCG, iterate by iterate -- TEST INFRASTRUCTURE ONLY (tests/test_pcg_checks.py, tests/test_gpu_pcg_stages.py).

A plain numpy PCG of the recurrence in csrc/ba_pcg.hip.h's header comment, on a DENSE S (the quad assembly from the GPU's own J and
residuals, oracle_lib.referee_reduced_from_jacobian):

    x_0 = 0, r_0 = rhs, z_0 = M^-1 r_0
    iteration k = 0, 1, ...:  stop when |r_k| <= rel_tol |rhs|  (the count of iterations done: ba_pcg_stats' last_iters)
        beta_k = r_k'z_k / r_{k-1}'z_{k-1} (0 at k = 0),  p_k = z_k + beta_k p_{k-1}
        alpha_k = r_k'z_k / p_k'S p_k,  x_{k+1} = x_k + alpha_k p_k,  r_{k+1} = r_k - alpha_k S p_k,  z_{k+1} = M^-1 r_{k+1}

with M block Jacobi, 9 x 9 per camera.  In np.longdouble (64-bit significand) it is the reference; in float64 / float32 -- S, rhs and
the blocks rounded to that type, the blocks inverted and every sum formed in it -- the yardstick: what a CPU implementation in working
precision achieves on the same S.  A solver capped at k iterations with a rel_tol it cannot meet returns x_k, so the library's
internals are measured through its public API:

    x_1 = alpha_0 M^-1 rhs            the reduced rhs, every B_a^-1 (direction), one product p'Sp (length)
    x_2                               M^-1 (rhs - alpha_0 S z_0): the whole vector S p, camera by camera
    x_3, x_4, x_7                     beta through all three rotating slots of the partials of r'z, twice

Two builders for the blocks: exact_blocks (the diagonal 9 x 9 blocks of S) and documented_blocks (the library's B_a: the self entries
of the camera's diagonal pair only, which leaves out the products of two DIFFERENT observations of one point by one camera).

iterate_error is the metric of an iterate: max_i |x - x_ref|_i sqrt(S_ii) / max_i |x_ref|_i sqrt(S_ii) (stage_checks.eta's scaling:
sqrt(S_ii) |x_i| is the size of unknown i in the energy norm, whatever the units of its column).

The keyword arguments beta, rz_rows and S_product of pcg() plant the defects tests/test_pcg_checks.py uses to show that the metric has
teeth; nothing else passes them.
"""
import numpy as np

LD = np.longdouble
EPS = {np.dtype(t): float(np.finfo(t).eps) for t in (np.float32, np.float64, np.longdouble)}


# ---- 9 x 9 blocks ----------------------------------------------------------------------------------------------------------------------
def exact_blocks(S, N):
    """[N, 9, 9]: the diagonal blocks of S."""
    S = np.asarray(S)
    return np.stack([S[9 * a:9 * a + 9, 9 * a:9 * a + 9] for a in range(N)])


def _inv3(A):
    """Inverses of symmetric 3 x 3 matrices [n, 3, 3] by cofactors, in the dtype of A."""
    a, b, c = A[:, 0, 0], A[:, 0, 1], A[:, 0, 2]
    d, e, f = A[:, 1, 1], A[:, 1, 2], A[:, 2, 2]
    C = np.empty_like(A)
    C[:, 0, 0], C[:, 0, 1], C[:, 0, 2] = d * f - e * e, c * e - b * f, b * e - c * d
    C[:, 1, 1], C[:, 1, 2], C[:, 2, 2] = a * f - c * c, b * c - a * e, a * d - b * b
    C[:, 1, 0], C[:, 2, 0], C[:, 2, 1] = C[:, 0, 1], C[:, 0, 2], C[:, 1, 2]
    det = a * C[:, 0, 0] + b * C[:, 0, 1] + c * C[:, 0, 2]
    return C / det[:, None, None]


def repeated_groups(p):
    """(group id per observation or -1, number of groups): the observations that share their (camera, point) with another one."""
    key = p.pt_idx.astype(np.int64) * p.N + p.cam_idx
    _, inv, cnt = np.unique(key, return_inverse=True, return_counts=True)
    rep = cnt[inv] > 1
    gid = np.full(p.K, -1, np.int64)
    ids, gid[rep] = np.unique(inv[rep], return_inverse=True)
    return gid, len(ids)


def documented_blocks(p, Jc, Jp, lam, S):
    """[N, 9, 9] long double: B_a = V_a + lam I - sum_{o in a} W_o (V_p(o) + lam I)^-1 W_o' (W_o = Jc_o'Jp_o, V_p = sum Jp'Jp over the
    point's observations), the block k_pcg_prec_reduce builds.  It is the diagonal block of S plus the terms S has and B_a has not:
    per (camera, point) seen more than once, sum over o != o' of W_o C W_o'' = (sum W_o) C (sum W_o)' - sum W_o C W_o', C = (V_p +
    lam I)^-1 -- formed that way, from the quad S and those few terms in long double, so that the blocks of an ordinary camera carry
    the accuracy of the quad assembly.  (p: point-sorted oracle problem; J as the solver's getters return it.)"""
    B = exact_blocks(S, p.N).astype(LD)
    gid, ng = repeated_groups(p)
    if ng == 0:
        return B
    o = np.nonzero(gid >= 0)[0]
    Jc = np.asarray(Jc, np.float64).reshape(p.K, 2, 9).astype(LD)
    Jp = np.asarray(Jp, np.float64).reshape(p.K, 2, 3).astype(LD)
    pts = np.unique(p.pt_idx[o])
    sel = np.isin(p.pt_idx, pts)
    Vp = np.zeros((p.M, 3, 3), LD)
    np.add.at(Vp, p.pt_idx[sel], np.einsum("kri,krj->kij", Jp[sel], Jp[sel]))
    Vp[pts] += LD(lam) * np.eye(3, dtype=LD)
    Ci = np.zeros((p.M, 3, 3), LD)
    Ci[pts] = _inv3(Vp[pts])
    W = np.einsum("kri,krj->kij", Jc[o], Jp[o])  # [n, 9, 3]
    Co = Ci[p.pt_idx[o]]
    Wsum = np.zeros((ng, 9, 3), LD)
    np.add.at(Wsum, gid[o], W)
    first = np.zeros(ng, np.int64)
    first[gid[o][::-1]] = o[::-1]  # one observation per group: its camera and point
    np.add.at(B, p.cam_idx[first], np.einsum("gij,gjl,gml->gim", Wsum, Ci[p.pt_idx[first]], Wsum))
    np.add.at(B, p.cam_idx[o], -np.einsum("kij,kjl,kml->kim", W, Co, W))
    return B


def invert_blocks(B, dtype=LD):
    """([N, 9, 9] inverses, [N] bool ok): B_a = L L' and B_a^-1 = L^-T L^-1 in `dtype`, all blocks at once.  ok[a] is False where a
    pivot is not positive in that arithmetic (the inverse of that block is then NaN): k_pcg_prec_inv's condition for its diagonal
    fallback."""
    A = np.array(B, dtype)
    N = A.shape[0]
    L = np.zeros_like(A)
    ok = np.ones(N, bool)
    with np.errstate(invalid="ignore", divide="ignore"):
        for j in range(9):
            d = A[:, j, j] - (L[:, j, :j] * L[:, j, :j]).sum(axis=1)
            ok &= d > 0
            ljj = np.sqrt(np.where(d > 0, d, np.nan))
            L[:, j, j] = ljj
            for i in range(j + 1, 9):
                L[:, i, j] = (A[:, i, j] - (L[:, i, :j] * L[:, j, :j]).sum(axis=1)) / ljj
        W = np.zeros_like(A)  # L^-1
        for i in range(9):
            W[:, i, i] = 1 / L[:, i, i]
            for j in range(i):
                W[:, i, j] = -(L[:, i, j:i] * W[:, j:i, j]).sum(axis=1) * W[:, i, i]
        Mi = np.einsum("nki,nkj->nij", W, W)
    return Mi, ok


def diagonal_inverse(B, cams=None, Minv=None):
    """k_pcg_prec_inv's fallback, the inverse of the block's diagonal, for the cameras `cams` (None: all) -- the other blocks from Minv."""
    B = np.asarray(B)
    out = np.array(Minv if Minv is not None else np.zeros_like(B))
    for a in (range(B.shape[0]) if cams is None else cams):
        d = np.diagonal(B[a])
        out[a] = np.diag(np.where(d > 0, 1 / np.where(d > 0, d, 1), 0))
    return out


def scaled_min_eig(B):
    """Per block, the smallest eigenvalue of D^-1/2 B D^-1/2, D = diag B: how far a block is from losing positive definiteness to
    rounding errors of relative size eps in its entries (a few x 9 eps is the danger zone)."""
    B = np.asarray(B, np.float64)
    d = 1 / np.sqrt(np.einsum("nii->ni", B))
    return np.linalg.eigvalsh(B * d[:, :, None] * d[:, None, :])[:, 0]


# ---- the recurrence ------------------------------------------------------------------------------------------------------------------------
def pcg(S, rhs, Minv, max_iter, rel_tol=0.0, dtype=LD, keep=None, beta="cg", rz_rows=None, S_product=None, V=None):
    """PCG as in the module docstring, everything in `dtype`.  Returns dict(x: the last iterate, iters, converged, xs: {k: x_k for k
    in keep}, rr: [|r_k|^2 / |rhs|^2 of the recurrence, k = 0 ... iters]).
    V ([N, 9, 9], the blocks V_a + lam I of camera_blocks): the product formed the matrix-free way, S p = V p - (V - S) p with both
    terms rounded to dtype, as ba_pcg.hip.h forms it (the working-precision yardstick; the reference multiplies by S).
    Planted defects (tests/test_pcg_checks.py only): beta = "zero" (p_k = z_k: steepest descent in the M-norm) or "stale" (the
    denominator of beta_k from iteration k - 2 for k >= 2: the slot one iteration stale); rz_rows: a bool mask of the rows that
    enter r'z (one block of partials left out); S_product: another matrix for the products S p (one block of the product missing)."""
    S = np.asarray(S, dtype)  # (no copy when the caller already holds S in dtype)
    Sp_mat = S if S_product is None else np.asarray(S_product, dtype)
    b = np.asarray(rhs, dtype)
    Mi = np.asarray(Minv, dtype)
    N = Mi.shape[0]
    keep = set(keep or ())
    if V is not None:
        Vd = np.asarray(V, dtype)
        E = _minus_blocks(np.asarray(S, LD), np.asarray(V, LD)).astype(dtype)  # V - S, formed in long double
    tol2 = dtype(rel_tol) * dtype(rel_tol)

    def prec(r):
        return np.einsum("nij,nj->ni", Mi, r.reshape(N, 9)).reshape(-1)

    def dot_rz(r, z):
        return (r * z).sum() if rz_rows is None else (r[rz_rows] * z[rz_rows]).sum()

    x = np.zeros_like(b)
    r = b.copy()
    z = prec(r)
    p = np.zeros_like(b)
    bb = (b * b).sum()
    rz = [dot_rz(r, z)]
    rr = [(r * r).sum()]
    xs = {0: x.copy()} if 0 in keep else {}
    k, conv = 0, False
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        while True:
            if rr[k] <= tol2 * bb:
                conv = True
                break
            if k == max_iter:
                break
            if k == 0 or beta == "zero":
                bk = dtype(0)
            elif beta == "stale" and k >= 2:
                bk = rz[k] / rz[k - 2]
            else:
                bk = rz[k] / rz[k - 1]
            p = z + bk * p
            y = Sp_mat @ p if V is None else np.einsum("nij,nj->ni", Vd, p.reshape(N, 9)).reshape(-1) - E @ p
            alpha = rz[k] / (p * y).sum()
            x = x + alpha * p
            r = r - alpha * y
            z = prec(r)
            rz.append(dot_rz(r, z))
            rr.append((r * r).sum())
            k += 1
            if k in keep:
                xs[k] = x.copy()
    return dict(x=x, iters=k, converged=conv, xs=xs, rr=np.array([float(v / bb) for v in rr]))


def _minus_blocks(S, V):
    """blockdiag(V) - S."""
    E = -S
    for a in range(V.shape[0]):
        E[9 * a:9 * a + 9, 9 * a:9 * a + 9] += V[a]
    return E


def camera_blocks(p, Jc, lam):
    """[N, 9, 9] long double: V_a + lam I, V_a = sum of Jc_o'Jc_o over the camera's observations -- the first term of the matrix-free
    product, before the elimination takes its share away."""
    Jc = np.asarray(Jc, np.float64).reshape(p.K, 2, 9).astype(LD)
    V = np.zeros((p.N, 9, 9), LD)
    np.add.at(V, p.cam_idx, np.einsum("kri,krj->kij", Jc, Jc))
    return V + LD(lam) * np.eye(9, dtype=LD)


def yardstick(S, rhs, B, max_iter, rel_tol=0.0, dtype=np.float64, keep=None, V=None, g=None):
    """The PCG in working precision `dtype` on S, rhs and the blocks B rounded to it, the blocks inverted in it.  None when a block is
    not positive definite in that arithmetic or an iterate is not finite (the caller then scales the fp64 yardstick by eps / eps64).
    V: the product in the matrix-free form (pcg).  The library never holds S: it subtracts the eliminated part from V p in working
    precision, and where the elimination cancels most of V (few observations per unknown, a small lambda) that difference carries
    an error of eps |V| |p|, not eps |S| |p|; a yardstick that multiplies by the quad S has no such term and is then no measure of what
    working precision can achieve.  Likewise B_a = V_a - (its eliminated part) and, with g (the camera part of the gradient),
    rhs = g - (its eliminated part): both differences formed in dtype, as k_pcg_prec_reduce forms them."""
    if V is not None:
        Vl, Bl = np.asarray(V, LD), np.asarray(B, LD)
        B = np.asarray(V).astype(dtype) - (Vl - Bl).astype(dtype)
        if g is not None:
            gl, rl = np.asarray(g, LD), np.asarray(rhs, LD)
            rhs = np.asarray(g).astype(dtype) - (gl - rl).astype(dtype)
    Mi, ok = invert_blocks(np.asarray(B).astype(dtype), dtype)
    if not ok.all():
        return None
    out = pcg(np.asarray(S).astype(dtype) if V is None else S, np.asarray(rhs).astype(dtype), Mi, max_iter, rel_tol, dtype, keep, V=V)
    if not all(np.all(np.isfinite(v.astype(np.float64))) for v in list(out["xs"].values()) + [out["x"]]):
        return None
    return out


# ---- metrics ---------------------------------------------------------------------------------------------------------------------------
def iterate_error(x, x_ref, S):
    """max_i |x - x_ref|_i sqrt(S_ii) / max_i |x_ref|_i sqrt(S_ii); NaN when x holds one (a NaN must fail every bound)."""
    d = np.sqrt(np.diagonal(np.asarray(S)).astype(LD))
    x, x_ref = np.asarray(x).astype(LD), np.asarray(x_ref).astype(LD)
    if not np.all(np.isfinite(x.astype(np.float64))):
        return float("nan")
    den = (np.abs(x_ref) * d).max()
    num = (np.abs(x - x_ref) * d).max()
    return float(num / den) if den > 0 else (0.0 if num == 0 else float("inf"))


def worst_camera(x, x_ref, S):
    """The camera holding the largest entry of iterate_error's numerator (for the message of a failing case)."""
    d = np.sqrt(np.diagonal(np.asarray(S)).astype(LD))
    e = np.abs(np.asarray(x).astype(LD) - np.asarray(x_ref).astype(LD)) * d
    return int(np.argmax(np.where(np.isfinite(e.astype(np.float64)), e, np.inf)) // 9)


def working_residual(S, x, rhs, dtype, V=None):
    """|rhs - S x| / |rhs| formed in `dtype` from S, x and rhs rounded to it: the yardstick of the device's own residual (the product
    S x behind the last iteration).  V: the product in the matrix-free form (pcg)."""
    x, b = np.asarray(x).astype(dtype), np.asarray(rhs).astype(dtype)
    if V is None:
        y = np.asarray(S).astype(dtype) @ x
    else:
        N = V.shape[0]
        y = np.einsum("nij,nj->ni", np.asarray(V, dtype), x.reshape(N, 9)).reshape(-1) - _minus_blocks(np.asarray(S, LD), np.asarray(V, LD)).astype(dtype) @ x
    r = b - y
    return float(np.sqrt((r * r).sum() / (b * b).sum()))
