"""Marquardt's damping, one LM trial restated -- TEST INFRASTRUCTURE ONLY (tests/test_damping_checks.py, tests/test_gpu_damping.py).

ba_solver_set_damping(BA_DAMP_MARQUARDT) (include/ba_mi355x.h): a trial solves

    (J'J + lambda D) dx = g,   g = -J'e,   D_ii = min(max((J'J)_ii, diag_min), diag_max)

by eliminating the points (through the L D L' of every damped point block, as the kernels do).  With U_p = sum Jp'Jp, V_a = sum Jc'Jc, W_o = Jc_o'Jp_o over the observations (plus whatever priors and
relative poses add to U, V, g and between two cameras: add_U, add_V, add_g, add_cross) and d = fl(lambda clamp(diag)):

    point block   U_p + diag(d_p)
    S             blockdiag(V_a + diag(d_a)) + add_cross - sum_p W_p (U_p + diag(d_p))^-1 W_p'
    rhs           g_c - sum_p W_p (U_p + diag(d_p))^-1 g_p
    dx_c = S^-1 rhs (with groups: P y of (P'SP) y = P' rhs, shared_checks.dense_solve),   dx_p = (U_p + diag(d_p))^-1 (g_p - W_p' dx_c)
    rhoScale      dx'(d o dx + g)

`trial` does this in np.longdouble (the reference) or, with dtype = float64 / float32, with every product and sum of the elimination
and the assembly rounded to that type (the working-precision yardstick: what a CPU implementation achieves on the same J).  kind = 0
is the identity damping d = lambda, by the same code.  The metrics are stage_checks' with d in place of lambda.
"""
import numpy as np

import shared_checks as SH
import stage_checks as SC

LD = np.longdouble
IDENTITY, MARQUARDT = 0, 1
DIAG_MIN, DIAG_MAX = 1e-6, 1e32


def clamp(diag, dmin=DIAG_MIN, dmax=DIAG_MAX):
    return np.minimum(np.maximum(diag, diag.dtype.type(dmin)), diag.dtype.type(dmax))


def damping(diag, lam, kind=MARQUARDT, dmin=DIAG_MIN, dmax=DIAG_MAX, round_to=None):
    """d = fl(lambda clamp(diag)) per unknown (kind 0: lambda), in the dtype of diag; round_to: the solver's scalar type -- lambda, the
    bounds and the product rounded to it as the kernels round them, returned in the dtype of diag."""
    dt = diag.dtype.type
    if round_to is not None:
        r = np.dtype(round_to).type
        if kind == IDENTITY:
            return np.full(diag.shape, dt(r(lam)))
        return (r(lam) * clamp(diag.astype(r), r(dmin), r(dmax))).astype(diag.dtype)
    if kind == IDENTITY:
        return np.full(diag.shape, dt(lam))
    return dt(lam) * clamp(diag, dmin, dmax)


def normal_blocks(p, Jc, Jp, e, dtype=LD, add_U=None, add_V=None, add_g=None):
    """U [M, 3, 3], V [N, 9, 9], g (3M + 9N, points first) of the observations of p (+ the additions), in dtype."""
    Jc = np.asarray(Jc).reshape(p.K, 2, 9).astype(dtype)  # (doubles from a getter, or long doubles from scale_columns)
    Jp = np.asarray(Jp).reshape(p.K, 2, 3).astype(dtype)
    e = np.asarray(e).reshape(p.K, 2).astype(dtype)
    U, V, g = np.zeros((p.M, 3, 3), dtype), np.zeros((p.N, 9, 9), dtype), np.zeros(3 * p.M + 9 * p.N, dtype)
    np.add.at(U, p.pt_idx, np.einsum("kai,kaj->kij", Jp, Jp))
    np.add.at(V, p.cam_idx, np.einsum("kai,kaj->kij", Jc, Jc))
    np.add.at(g[:3 * p.M].reshape(p.M, 3), p.pt_idx, -np.einsum("kai,ka->ki", Jp, e))
    np.add.at(g[3 * p.M:].reshape(p.N, 9), p.cam_idx, -np.einsum("kai,ka->ki", Jc, e))
    if add_U is not None:
        U = U + np.asarray(add_U).astype(dtype)
    if add_V is not None:
        V = V + np.asarray(add_V).astype(dtype)
    if add_g is not None:
        g = g + np.asarray(add_g).astype(dtype)
    return U, V, g


def diagonals(U, V):
    """(diag J'J of the points [3M], of the cameras [9N])."""
    return np.einsum("mii->mi", U).reshape(-1).copy(), np.einsum("nii->ni", V).reshape(-1).copy()


def _ldl3(A):
    """(l10, l20, l21, [n, 3] 1 / D) of the unpivoted L D L' of symmetric 3 x 3 matrices [n, 3, 3] (the kernels' factorisation), in the
    dtype of A."""
    a, b, c, d, e, f = A[:, 0, 0], A[:, 0, 1], A[:, 0, 2], A[:, 1, 1], A[:, 1, 2], A[:, 2, 2]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        d0 = a
        l10, l20 = b / d0, c / d0
        d1 = d - l10 * l10 * d0
        l21 = (e - l20 * l10 * d0) / d1
        d2 = f - l20 * l20 * d0 - l21 * l21 * d1
        return l10, l20, l21, np.stack([1 / d0, 1 / d1, 1 / d2], axis=1)


def eliminate(p, Jc, Jp, Ud, gp, dtype=LD, chunk=4096):
    """The elimination in the kernels' form: Ud_p = L D L', Z_o = W_o L^-T (W_o = Jc_o'Jp_o), t = L^-1 g_p, so that
    W Ud^-1 W' = Z D^-1 Z' and W Ud^-1 g_p = Z D^-1 t -- no inverse of an ill-conditioned block is formed.  Returns (E [9N, 9N] =
    sum_p Z_p D_p^-1 Z_p', r [9N] = sum_p Z_p D_p^-1 t_p, fac = (l10, l20, l21, 1 / D, t): the points' factors, (Z, wp, wc): the
    (point, camera) blocks, own [N, 9, 9] = sum over the OBSERVATIONS o of a camera of Z_o D^-1 Z_o': what the library's B_a takes off
    V_a), all in dtype.  Ud [M, 3, 3]: the damped point blocks; a point nobody observes takes no part."""
    Jc = np.asarray(Jc).reshape(p.K, 2, 9).astype(dtype)
    Jp = np.asarray(Jp).reshape(p.K, 2, 3).astype(dtype)
    l10, l20, l21, di = _ldl3(np.asarray(Ud, dtype))
    g3 = np.asarray(gp, dtype).reshape(p.M, 3)
    t = np.empty_like(g3)
    t[:, 0] = g3[:, 0]
    t[:, 1] = g3[:, 1] - l10 * t[:, 0]
    t[:, 2] = g3[:, 2] - l20 * t[:, 0] - l21 * t[:, 1]
    Wo = np.einsum("kai,kaj->kij", Jc, Jp)
    j = p.pt_idx
    Zo = np.empty_like(Wo)
    Zo[:, :, 0] = Wo[:, :, 0]
    Zo[:, :, 1] = Wo[:, :, 1] - l10[j, None] * Zo[:, :, 0]
    Zo[:, :, 2] = Wo[:, :, 2] - l20[j, None] * Zo[:, :, 0] - l21[j, None] * Zo[:, :, 1]
    own = np.zeros((p.N, 9, 9), dtype)
    np.add.at(own, p.cam_idx, np.einsum("kil,kl,kjl->kij", Zo, di[j], Zo))
    # one block per (point, camera): Z_pa = the sum over the observations of p by a
    key = p.pt_idx.astype(np.int64) * p.N + p.cam_idx
    uk, inv = np.unique(key, return_inverse=True)
    Z = np.zeros((len(uk), 9, 3), dtype)
    np.add.at(Z, inv, Zo)
    wp, wc = (uk // p.N).astype(np.int64), (uk % p.N).astype(np.int64)
    r = np.zeros((p.N, 9), dtype)
    np.add.at(r, wc, np.einsum("kil,kl->ki", Z, (di * t)[wp]))
    E = np.zeros((p.N, 9, p.N, 9), dtype)
    start = np.flatnonzero(np.r_[True, wp[1:] != wp[:-1], True])  # (uk is sorted by point)
    cnt = np.diff(start)
    for n_t in np.unique(cnt):
        first = start[:-1][cnt == n_t]
        step = max(1, chunk // (n_t * n_t))
        for c0 in range(0, len(first), step):
            idx = first[c0:c0 + step][:, None] + np.arange(n_t)[None, :]                       # [n, t]
            blocks = np.einsum("nsil,nl,ntjl->nstij", Z[idx], di[wp[idx[:, 0]]], Z[idx])        # [n, t, t, 9, 9]
            ca = np.broadcast_to(wc[idx][:, :, None], blocks.shape[:3]).reshape(-1)
            cb = np.broadcast_to(wc[idx][:, None, :], blocks.shape[:3]).reshape(-1)
            np.add.at(E, (ca, slice(None), cb, slice(None)), blocks.reshape(-1, 9, 9))
    return E.reshape(9 * p.N, 9 * p.N), r.reshape(-1), (l10, l20, l21, di, t), (Z, wp, wc), own


def solve(A, b):
    """A^-1 b for a symmetric positive definite A in long double: the symmetrically scaled matrix inverted in double, then iterative
    refinement with long double residuals until the corrections stop shrinking (shared_checks.dense_solve's scheme)."""
    A, b = np.asarray(A, LD), np.asarray(b, LD)
    d = 1 / np.sqrt(np.diagonal(A))
    As, bs = A * d[:, None] * d[None, :], b * d
    Ai = np.linalg.inv(As.astype(np.float64))
    x, last = np.zeros(len(bs), LD), np.inf
    for _ in range(30):
        dx = (Ai @ (bs - As @ x).astype(np.float64)).astype(LD)
        step = float(np.abs(dx).max())
        if step > 0.5 * last:
            break
        x, last = x + dx, step
    return x * d


def trial(p, Jc, Jp, e, lam, kind=MARQUARDT, dmin=DIAG_MIN, dmax=DIAG_MAX, dtype=LD, add_U=None, add_V=None, add_g=None, add_cross=None,
          groups=None, g=None, round_to=None, want_step=True):
    """One trial (module docstring).  g: the gradient to use instead of -J'e (a device's own GET_GRAD).  round_to: damping()'s.
    Returns dict(U, V, g, diag_p, diag_c: the raw diagonals; d_p, d_c: the dampings; S, rhs; B [N, 9, 9]: the library's block-Jacobi
    blocks V_a + diag(d_a) - the camera's self entries; Vd [N, 9, 9] = V_a + diag(d_a); dx_c, dx_p, dx (points first), rho_scale -- the
    step always in long double from the S and rhs of `dtype`)."""
    U, V, g0 = normal_blocks(p, Jc, Jp, e, dtype, add_U, add_V, add_g)
    g = g0 if g is None else np.asarray(g, np.float64).astype(dtype)
    diag_p, diag_c = diagonals(U, V)
    d_p = damping(diag_p, lam, kind, dmin, dmax, round_to)
    d_c = damping(diag_c, lam, kind, dmin, dmax, round_to)
    Ud = U.copy()
    Ud[:, np.arange(3), np.arange(3)] += d_p.reshape(p.M, 3)
    E, r, fac, (Z, wp, wc), own = eliminate(p, Jc, Jp, Ud, g[:3 * p.M], dtype)
    S = E  # (in place: 9N x 9N long doubles are half a gigabyte at N = 600)
    np.negative(S, out=S)
    E = -S[:0]  # (no longer used whole: the diagonal blocks below read -S)
    for a in range(p.N):
        blk = V[a] + S[9 * a:9 * a + 9, 9 * a:9 * a + 9]  # (V - s) + d: the order of the kernels
        blk[np.arange(9), np.arange(9)] += d_c[9 * a:9 * a + 9]
        S[9 * a:9 * a + 9, 9 * a:9 * a + 9] = blk
    if add_cross is not None:
        S += np.asarray(add_cross).astype(dtype)
    rhs = g[3 * p.M:] - r
    Vd = V.copy()
    Vd[:, np.arange(9), np.arange(9)] += d_c.reshape(p.N, 9)
    out = dict(U=U, V=V, g=g, diag_p=diag_p, diag_c=diag_c, d_p=d_p, d_c=d_c, S=S, rhs=rhs, B=(V - own) + (Vd - V), Vd=Vd)
    if not want_step:
        return out
    Sl, rl = np.asarray(S, LD), rhs.astype(LD)
    dx_c = SH.dense_solve(Sl, rl, groups) if groups else solve(Sl, rl)
    l10, l20, l21, di, t = (v.astype(LD) for v in fac)
    zx = np.zeros((p.M, 3), LD)
    np.add.at(zx, wp, np.einsum("kil,ki->kl", Z.astype(LD), dx_c.reshape(p.N, 9)[wc]))
    u = di * (t - zx)  # dx_p = L^-T D^-1 (t - Z' dx_c)
    dx_p = np.empty_like(u)
    dx_p[:, 2] = u[:, 2]
    dx_p[:, 1] = u[:, 1] - l21 * dx_p[:, 2]
    dx_p[:, 0] = u[:, 0] - l10 * dx_p[:, 1] - l20 * dx_p[:, 2]
    seen = np.bincount(p.pt_idx, minlength=p.M) > 0
    if add_U is not None:
        seen |= np.abs(np.asarray(add_U, np.float64)).sum(axis=(1, 2)) > 0
    dx_p[~seen] = 0  # (a point nobody observes: lambda diag_min on its block, a zero gradient, no step)
    dx = np.concatenate([dx_p.reshape(-1), dx_c])
    out.update(dx_c=dx_c, dx_p=dx_p.reshape(-1), dx=dx, rho_scale=rho_scale(dx, np.concatenate([d_p, d_c]), g))
    return out


def rho_scale(dx, d, g):
    """dx'(d o dx + g) in long double."""
    dx, d, g = np.asarray(dx).astype(LD), np.asarray(d).astype(LD), np.asarray(g).astype(LD)
    return (dx * (d * dx + g)).sum()


def dense_system(p, Jc, Jp, e, lam, kind=MARQUARDT, dmin=DIAG_MIN, dmax=DIAG_MAX, col_scale=None):
    """(H = J'J + diag(d), g = -J'e, d) of the WHOLE problem from the dense J [2K, 3M + 9N] (small problems only), long double.
    col_scale [3M + 9N]: J's columns multiplied by it first."""
    Jc = np.asarray(Jc).reshape(p.K, 2, 9)
    Jp = np.asarray(Jp).reshape(p.K, 2, 3)
    n = 3 * p.M + 9 * p.N
    J = np.zeros((2 * p.K, n), LD)
    for k in range(p.K):
        J[2 * k:2 * k + 2, 3 * p.pt_idx[k]:3 * p.pt_idx[k] + 3] += Jp[k]
        J[2 * k:2 * k + 2, 3 * p.M + 9 * p.cam_idx[k]:3 * p.M + 9 * p.cam_idx[k] + 9] += Jc[k]
    if col_scale is not None:
        J = J * np.asarray(col_scale, LD)[None, :]
    H = J.T @ J
    g = -(J.T @ np.asarray(e).reshape(-1).astype(LD))
    d = damping(np.diagonal(H).copy(), lam, kind, dmin, dmax)
    return H + np.diag(d), g, d


def scale_columns(p, Jc, Jp, cp, cc):
    """(Jc, Jp) with the columns of unknown i multiplied by c_i: cp [3M] for the points, cc [9N] for the cameras; long double, so
    that the scaled J is the scaled problem's to 2^-64 and not a rounded neighbour of it."""
    Jc = np.asarray(Jc).reshape(p.K, 2, 9).astype(LD) * np.asarray(cc).astype(LD).reshape(p.N, 9)[p.cam_idx][:, None, :]
    Jp = np.asarray(Jp).reshape(p.K, 2, 3).astype(LD) * np.asarray(cp).astype(LD).reshape(p.M, 3)[p.pt_idx][:, None, :]
    return Jc, Jp


def step_difference(x, y):
    """max_i |x - y|_i / max_i |y|_i."""
    x, y = np.asarray(x).astype(LD), np.asarray(y).astype(LD)
    return float(np.abs(x - y).max() / np.abs(y).max())


# ---- stage_checks' metrics with d in place of lambda --------------------------------------------------------------------------------------
def assembly_errors(p, Jc, Jp, f, d_c, S, rhs, S_ref, rhs_ref, diag_c=None):
    """stage_checks.assembly_errors with sqrt((V_ii + d_i)(V_jj + d_j)) as the scale of S_ij (diag_c: V's diagonal when priors or
    constraints have added to it; default: the observations' own)."""
    V = SC.camera_diag(p, Jc) if diag_c is None else np.asarray(diag_c, np.float64)
    sc = np.sqrt(V + np.asarray(d_c, np.float64))
    out = {}
    if S is not None:
        dS = np.abs(np.asarray(S).astype(LD) - np.asarray(S_ref).astype(LD)).astype(np.float64)
        dS /= sc[:, None]
        dS /= sc[None, :]
        out["S"] = float(dS.max()) if np.all(np.isfinite(np.asarray(S, np.float64))) else float("nan")
    den = SC.abs_grad(p, Jc, Jp, f)[3 * p.M:] + np.abs(np.asarray(rhs_ref).astype(np.float64))
    num = np.abs(np.asarray(rhs).astype(LD) - np.asarray(rhs_ref).astype(LD)).astype(np.float64)
    out["rhs"] = float(SC._ratio(num, den).max())
    return out


def backsub_errors(p, Jc, Jp, dx, g, d_p, add_U=None):
    """stage_checks.backsub_errors with diag(d_p) for lambda I (add_U [M, 3, 3]: what priors add to the point blocks)."""
    M, N, K = p.M, p.N, p.K
    Jc = np.asarray(Jc, np.float64).reshape(K, 2, 9).astype(LD)
    Jp = np.asarray(Jp, np.float64).reshape(K, 2, 3).astype(LD)
    dx = np.asarray(dx, np.float64)
    dxp, dxc = dx[:3 * M].reshape(M, 3).astype(LD), dx[3 * M:].reshape(N, 9).astype(LD)
    gp = np.asarray(g, np.float64)[:3 * M].reshape(M, 3).astype(LD)
    dp = np.asarray(d_p).astype(LD).reshape(M, 3)
    u = np.einsum("krc,kc->kr", Jp, dxp[p.pt_idx]) + np.einsum("krc,kc->kr", Jc, dxc[p.cam_idx])
    ua = np.einsum("krc,kc->kr", np.abs(Jp), np.abs(dxp[p.pt_idx])) + np.einsum("krc,kc->kr", np.abs(Jc), np.abs(dxc[p.cam_idx]))
    res, den = np.zeros((M, 3), LD), np.zeros((M, 3), LD)
    np.add.at(res, p.pt_idx, np.einsum("krc,kr->kc", Jp, u))
    np.add.at(den, p.pt_idx, np.einsum("krc,kr->kc", np.abs(Jp), ua))
    if add_U is not None:
        Ua = np.asarray(add_U).astype(LD)
        res += np.einsum("mij,mj->mi", Ua, dxp)
        den += np.einsum("mij,mj->mi", np.abs(Ua), np.abs(dxp))
    res += dp * dxp - gp
    den += dp * np.abs(dxp) + np.abs(gp)
    return float(SC._ratio(np.abs(res).astype(np.float64), den.astype(np.float64)).max())


def rho_scale_error(rho, dx, d, g):
    """|rho - dx'(d o dx + g)| / sum |dx| (d |dx| + |g|) (stage_checks.trial_scalar_errors' rho_scale)."""
    dx, d, g = np.asarray(dx).astype(LD), np.asarray(d).astype(LD), np.asarray(g).astype(LD)
    return float(abs(LD(rho) - rho_scale(dx, d, g)) / (np.abs(dx) * (d * np.abs(dx) + np.abs(g))).sum())
