"""Host references for the covariance blocks (ba_solver_covariance_compute / _get) -- TEST INFRASTRUCTURE ONLY.

With H = J'J + lam I on the free parameters, Sigma = H^-1 there and 0 in the rows / columns of fixed ones.  Two independent routes:

  dense_covariance       the inverse of the whole H (cameras and points together), numpy
  reference_covariance   the Schur formulas of DESIGN.md section 11: Sigma_cc = S^-1, Sigma_pp = U^-1 + U^-1 (sum_ab W_ap' Sigma_ab W_bp) U^-1

and the yardsticks of the GPU tests: column_errors (|S Sigma e_j - e_j| / (|S|_F |Sigma e_j|) with the residual in quad precision,
oracle/ba_referee.c: ref_sym_residual), refined_inverse (Sigma_cc beyond double: Newton steps with extended-precision residuals on the
symmetrically scaled matrix) and ldlt_inverse (the device's algorithm restated in numpy: LDL^T without pivoting, with and without the
diagonal scaling -- what settles on the CPU whether the scaling is needed).

Jc [K, 2, 9] and Jp [K, 2, 3] are in the order of p.cam_idx / p.pt_idx; camera block order T, omega, f, k1, k2.
"""
import numpy as np

EPS = float(np.finfo(np.float64).eps)


def sorted_oracle_problem(O, pg):
    """The oracle's view of a GPU problem in the point-sorted order of the GPU's getters (test_gpu_stages.py)."""
    a = pg.arrays()
    order = np.argsort(a["pt_idx"], kind="stable")
    return O.Problem(pg.N, pg.M, pg.K, a["cam_idx"][order], a["pt_idx"][order], a["meas"].reshape(-1, 2)[order].ravel(), a["cams9"],
                     a["pts"])


def free_sets(p, cam_mask=None, pt_fixed=None):
    """(free camera parameters bool[9N], free points bool[M])."""
    fc = np.ones(9 * p.N, bool)
    if cam_mask is not None:
        bits = (np.asarray(cam_mask, np.uint32)[:, None] >> np.arange(9)[None, :]) & 1
        fc = bits.reshape(-1) == 0
    fp = np.ones(p.M, bool) if pt_fixed is None else np.asarray(pt_fixed).astype(bool) == 0
    return fc, fp


def mask_jacobian(p, Jc, Jp, cam_mask=None, pt_fixed=None):
    """Copies of (Jc, Jp) with the columns of fixed parameters zero (what BA_GET_JC / BA_GET_JP return under a mask)."""
    fc, fp = free_sets(p, cam_mask, pt_fixed)
    Jc = np.array(Jc, np.float64).reshape(p.K, 2, 9) * fc.reshape(p.N, 9)[p.cam_idx][:, None, :]
    Jp = np.array(Jp, np.float64).reshape(p.K, 2, 3) * fp[p.pt_idx][:, None, None]
    return Jc, Jp


def dense_covariance(p, Jc, Jp, lam, cam_mask=None, pt_fixed=None):
    """Inverse of the whole J'J + lam I on the free parameters: cc (9N x 9N), pp (M, 3, 3), cond(H), zeros for fixed parameters."""
    D, n = 9 * p.N, 9 * p.N + 3 * p.M
    fc, fp = free_sets(p, cam_mask, pt_fixed)
    Jc, Jp = mask_jacobian(p, Jc, Jp, cam_mask, pt_fixed)
    J = np.zeros((2 * p.K, n))
    for o in range(p.K):
        a, j = int(p.cam_idx[o]), int(p.pt_idx[o])
        J[2 * o:2 * o + 2, 9 * a:9 * a + 9] = Jc[o]
        J[2 * o:2 * o + 2, D + 3 * j:D + 3 * j + 3] = Jp[o]
    H = J.T @ J + lam * np.eye(n)
    free = np.concatenate([fc, np.repeat(fp, 3)])
    idx = np.flatnonzero(free)
    Hf = H[np.ix_(idx, idx)]
    full = np.zeros((n, n))
    full[np.ix_(idx, idx)] = np.linalg.inv(Hf)
    pp = np.stack([full[D + 3 * j:D + 3 * j + 3, D + 3 * j:D + 3 * j + 3] for j in range(p.M)]) if p.M else np.zeros((0, 3, 3))
    return dict(cc=full[:D, :D], pp=pp, cond=float(np.linalg.cond(Hf)))


def point_blocks(p, Jc, Jp, lam, dtype=np.float64):
    """U (M, 3, 3) = sum Jp'Jp + lam I and G (K, 9, 3) = Jc'Jp per observation, in dtype."""
    Jc = np.asarray(Jc, dtype).reshape(p.K, 2, 9)
    Jp = np.asarray(Jp, dtype).reshape(p.K, 2, 3)
    U = np.zeros((p.M, 3, 3), dtype)
    np.add.at(U, p.pt_idx, np.einsum("oix,oiy->oxy", Jp, Jp))
    U += dtype(lam) * np.eye(3, dtype=dtype)
    return U, np.einsum("oir,oix->orx", Jc, Jp)


def reduced_matrix(p, Jc, Jp, lam, fp):
    """S = Jc'Jc + lam I - sum_p W_p U_p^-1 W_p' in double (numpy); a fixed point (Jp = 0) contributes nothing."""
    D = 9 * p.N
    Jc = np.asarray(Jc, np.float64).reshape(p.K, 2, 9)
    U, G = point_blocks(p, Jc, Jp, lam)
    S = lam * np.eye(D)
    V = np.einsum("oir,ois->ors", Jc, Jc)
    for o in range(p.K):
        a = int(p.cam_idx[o])
        S[9 * a:9 * a + 9, 9 * a:9 * a + 9] += V[o]
    order = np.argsort(p.pt_idx, kind="stable")
    ptr = np.searchsorted(p.pt_idx[order], np.arange(p.M + 1))
    for j in np.flatnonzero(fp):
        obs = order[ptr[j]:ptr[j + 1]]
        if len(obs) == 0:
            continue
        Ui = np.linalg.inv(U[j])
        for o1 in obs:
            a = int(p.cam_idx[o1])
            for o2 in obs:
                b = int(p.cam_idx[o2])
                S[9 * a:9 * a + 9, 9 * b:9 * b + 9] -= G[o1] @ Ui @ G[o2].T
    return S


def inv_free(S, fc):
    """numpy.linalg.inv of the free block, zeros elsewhere: the plain fp64 CPU route."""
    idx = np.flatnonzero(fc)
    out = np.zeros_like(S, dtype=np.float64)
    out[np.ix_(idx, idx)] = np.linalg.inv(np.asarray(S, np.float64)[np.ix_(idx, idx)])
    return out


def refined_inverse(S, fc, steps=4):
    """The inverse of the free block beyond double precision, as a long-double array (zeros elsewhere): numpy's inverse of the
    symmetrically scaled matrix E S E (E = diag(S)^-1/2; its condition number is the scaled one, 1e5 .. 1e7 here), then Newton steps
    X += X (I - A X) with everything in extended precision (64-bit mantissa), scaled back."""
    LD = np.longdouble
    idx = np.flatnonzero(fc)
    A = np.asarray(S, np.float64)[np.ix_(idx, idx)].astype(LD)
    e = 1 / np.sqrt(np.diag(A))
    A = A * e[:, None] * e[None, :]
    X = np.linalg.inv(A.astype(np.float64)).astype(LD)
    eye = np.eye(len(idx), dtype=LD)
    for _ in range(steps):
        X = X + X @ (eye - A @ X)
        X = (X + X.T) / 2
    out = np.zeros(np.shape(S), LD)
    out[np.ix_(idx, idx)] = X * e[:, None] * e[None, :]
    return out


def ldlt_inverse(S, fc, scaled=True):
    """The device's route in numpy fp64: E S E = L D L' without pivoting (unit diagonal for fixed rows), B = E L^-T D^-1,
    Sigma = B D B'.  Raises FloatingPointError on a pivot <= 0."""
    S = np.asarray(S, np.float64)
    D = S.shape[0]
    e = np.where(fc, (1 / np.sqrt(np.diag(S))) if scaled else 1.0, 0.0)
    A = S * e[:, None] * e[None, :]
    fx = np.flatnonzero(~np.asarray(fc))
    A[fx, fx] = 1.0
    L, d = np.eye(D), np.zeros(D)
    for k in range(D):
        d[k] = A[k, k]
        if not d[k] > 0:
            raise FloatingPointError("pivot %d = %g" % (k, d[k]))
        L[k + 1:, k] = A[k + 1:, k] / d[k]
        A[k + 1:, k + 1:] -= np.outer(L[k + 1:, k], A[k + 1:, k])
    Z = np.linalg.solve(L, np.diag(e))  # L^-1 E
    B = (Z / d[:, None]).T                                                   # E L^-T D^-1
    return (B * d[None, :]) @ B.T


def column_errors(O, S, Sigma, fc):
    """eta_j = |S Sigma e_j - e_j|_2 / (|S_FF|_F |Sigma e_j|_2) for every free column j, the residual evaluated in quad precision."""
    S = np.asfortranarray(S, np.float64)
    Sigma = np.asarray(Sigma, np.float64)
    idx = np.flatnonzero(fc)
    nS = float(np.linalg.norm(S[np.ix_(idx, idx)]))
    eta = np.zeros(len(idx))
    for n, j in enumerate(idx):
        x = np.ascontiguousarray(Sigma[:, j])
        b = np.zeros(S.shape[0])
        b[j] = 1.0
        num, _ = O.referee_sym_residual(S, x, b)
        eta[n] = np.linalg.norm(num[idx]) / (nS * np.linalg.norm(x))
    return eta


def point_covariance(p, Jc, Jp, lam, fp, sigma_cc, points=None, dtype=np.float64):
    """Sigma_pp = U^-1 + U^-1 (sum_{o, o'} G_o' Sigma_{c(o) c(o')} G_o') U^-1 for the points asked for, in dtype; 0 for a fixed point.
    Points of equal track length are evaluated together (batched einsum; the sums run in the track's observation order)."""
    pts = np.arange(p.M) if points is None else np.asarray(points)
    U, G = point_blocks(p, Jc, Jp, lam, dtype)
    Sig = np.ascontiguousarray(np.asarray(sigma_cc, dtype).reshape(p.N, 9, p.N, 9).transpose(0, 2, 1, 3))  # [a, b, r, c]
    order = np.argsort(p.pt_idx, kind="stable")
    ptr = np.searchsorted(p.pt_idx[order], np.arange(p.M + 1))
    out = np.zeros((len(pts), 3, 3), dtype)
    tlen = (ptr[1:] - ptr[:-1])[pts]
    free = np.asarray(fp)[pts]
    for t in np.unique(tlen[free]):
        sel = np.flatnonzero(free & (tlen == t))
        step = max(1, 40000 // int(t * t))
        for c0 in range(0, len(sel), step):
            idx = sel[c0:c0 + step]
            obs = order[ptr[pts[idx]][:, None] + np.arange(t)[None, :]]  # (n, t)
            cams = p.cam_idx[obs]
            g = G[obs]                                                    # (n, t, 9, 3)
            blocks = Sig[cams[:, :, None], cams[:, None, :]]              # (n, t, t, 9, 9)
            v = np.einsum("nabrs,nbsy->nary", blocks, g)
            M = np.einsum("narx,nary->nxy", g, v)
            Ui = _inv3_batch(U[pts[idx]])
            out[idx] = Ui + np.einsum("nxa,nab,nby->nxy", Ui, M, Ui)
    return out


def _inv3_batch(U):
    """3 x 3 inverses by cofactors, (n, 3, 3), any dtype (long double included)."""
    c = np.empty_like(U)
    for i in range(3):
        for j in range(3):
            r = [k for k in range(3) if k != j]
            q = [k for k in range(3) if k != i]
            c[:, i, j] = (-1) ** (i + j) * (U[:, r[0], q[0]] * U[:, r[1], q[1]] - U[:, r[0], q[1]] * U[:, r[1], q[0]])
    det = U[:, 0, 0] * c[:, 0, 0] + U[:, 0, 1] * c[:, 1, 0] + U[:, 0, 2] * c[:, 2, 0]
    return c / det[:, None, None]


def _inv3(U):
    """3 x 3 inverse by cofactors (any dtype, long double included)."""
    c = np.array([[U[1, 1] * U[2, 2] - U[1, 2] * U[2, 1], U[0, 2] * U[2, 1] - U[0, 1] * U[2, 2], U[0, 1] * U[1, 2] - U[0, 2] * U[1, 1]],
                  [U[1, 2] * U[2, 0] - U[1, 0] * U[2, 2], U[0, 0] * U[2, 2] - U[0, 2] * U[2, 0], U[0, 2] * U[1, 0] - U[0, 0] * U[1, 2]],
                  [U[1, 0] * U[2, 1] - U[1, 1] * U[2, 0], U[0, 1] * U[2, 0] - U[0, 0] * U[2, 1], U[0, 0] * U[1, 1] - U[0, 1] * U[1, 0]]])
    return c / (U[0, 0] * c[0, 0] + U[0, 1] * c[1, 0] + U[0, 2] * c[2, 0])


def reference_covariance(p, Jc, Jp, lam, cam_mask=None, pt_fixed=None, sigma_cc=None, points=None, dtype=np.float64):
    """The Schur formulas: cc = S^-1 on the free camera parameters (numpy's inverse of numpy's S unless sigma_cc is given), pp the
    point blocks from it (all points, or `points`)."""
    fc, fp = free_sets(p, cam_mask, pt_fixed)
    Jc, Jp = mask_jacobian(p, Jc, Jp, cam_mask, pt_fixed)
    if sigma_cc is None:
        sigma_cc = inv_free(reduced_matrix(p, Jc, Jp, lam, fp), fc)
    return dict(cc=np.asarray(sigma_cc), pp=point_covariance(p, Jc, Jp, lam, fp, sigma_cc, points, dtype))


def block_errors(got, ref):
    """Relative Frobenius error per block (n, r, r); 0 where both are exactly 0."""
    got, ref = np.asarray(got, np.longdouble), np.asarray(ref, np.longdouble)
    num = np.sqrt(((got - ref) ** 2).sum(axis=(1, 2)))
    den = np.sqrt((ref ** 2).sum(axis=(1, 2)))
    return np.asarray(np.where(den > 0, num / np.where(den > 0, den, 1), num), np.float64)


def cov_buffer_bytes(N):
    """Bytes ba_solver_device_bytes grows by at the first covariance compute (include/ba_mi355x.h)."""
    D = 9 * N
    Dp = 64 * ((D + 3 + 63) // 64)
    ldc = 64 * ((Dp + D + 3 + 63) // 64) + 64
    return 8 * (ldc * (Dp + 128) + 4096 * ((D + 63) // 64) + 4 * Dp + 128) + 4


def quad_reduced(O, kind, p, Jc, Jp, lam, fp):
    """The reduced camera matrix assembled in quad precision from (masked) Jc, Jp at lam (oracle/ba_referee.c), D x D symmetric.

    The referee eliminates every point, and a fixed point at lam = 0 would have it invert U_p = 0.  Every fixed point -- its Jp is zero,
    so all its observations contribute is Jc'Jc -- is therefore handed over with two more observations (camera 0, Jc = 0,
    Jp = [e1; e2] and [e3; 0]): its U becomes (1 + lam) I, W = Jc'Jp is still zero for every one of its observations, so its
    elimination subtracts exactly nothing and S is the S of the formulas, with no special case inside the yardstick."""
    Jc = np.asarray(Jc, np.float64).reshape(p.K, 2, 9)
    Jp = np.asarray(Jp, np.float64).reshape(p.K, 2, 3)
    fixed = np.flatnonzero(~np.asarray(fp))
    if len(fixed) == 0:
        return O.referee_reduced_from_jacobian(kind, p, Jc, Jp, np.zeros(2 * p.K), lam)["S"]
    assert not Jp[~np.asarray(fp)[p.pt_idx]].any()
    n = len(fixed)
    extra = np.array([[[1.0, 0, 0], [0, 1.0, 0]], [[0, 0, 1.0], [0, 0, 0]]])
    pt = np.concatenate([p.pt_idx, np.repeat(fixed, 2)]).astype(np.int32)
    order = np.argsort(pt, kind="stable")
    cam = np.concatenate([p.cam_idx, np.zeros(2 * n, np.int32)]).astype(np.int32)[order]
    Jc2 = np.concatenate([Jc, np.zeros((2 * n, 2, 9))])[order]
    Jp2 = np.concatenate([Jp, np.tile(extra, (n, 1, 1))])[order]
    K2 = len(pt)
    p2 = O.Problem(p.N, p.M, K2, cam, pt[order], np.zeros(2 * K2), p.cams9, p.pts)
    return O.referee_reduced_from_jacobian(kind, p2, Jc2, Jp2, np.zeros(2 * K2), lam)["S"]
