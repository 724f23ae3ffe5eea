"""Shared intrinsics for BA_ITERSCHUR -- TEST INFRASTRUCTURE ONLY (tests/test_shared_checks.py, tests/test_gpu_shared_intrinsics.py).

A group of cameras solves for one f, k1, k2 (include/ba_mi355x.h, ba_solver_set_shared_intrinsics).  With P (9N x n_free) the matrix
that copies a group's three intrinsics to rows 6..8 of each member and is the identity elsewhere, the step is dx_c = P y with

    (P'SP) y = P' rhs                                   (dense_solve: long double)

and the library computes it in the 9N layout as CG for Pi S on range(Pi) with preconditioner Pi M^-1, Pi = P (P'P)^-1 P' the
orthogonal projector that replaces rows 6..8 of every member by the group's mean:

    x_0 = 0, r_0 = Pi rhs, z_0 = Pi M^-1 r_0
    iteration k:  stop when |r_k| <= rel_tol |Pi rhs|
        beta_k = r_k'z_k / r_{k-1}'z_{k-1},  p_k = z_k + beta_k p_{k-1}
        alpha_k = r_k'z_k / p_k'S p_k,  x_{k+1} = x_k + alpha_k p_k,  r_{k+1} = r_k - alpha_k Pi S p_k,  z_{k+1} = Pi M^-1 r_{k+1}

projected_pcg is pcg_checks.pcg's recurrence with that operator and that preconditioner (M^-1 any callable r -> z: block Jacobi, a
forest).  Its keyword arguments project_z, mean and mean_rhs plant the defects tests/test_shared_checks.py uses to show that the
comparison has teeth; nothing else passes them.  (A sum for the mean in ALL three places is no defect of the limit: with Q = P P' it
is CG for Q S preconditioned by Q M^-1 on Q rhs, which solves the same P'S x = P' rhs on range(P) -- through other iterates.  The
sum in the iteration's two projections alone, under a rhs projected by the mean, solves Q S x = Pi rhs: another x.)

plan restates ba_intrinsics_group_plan: equal labels >= 0 form a group, a label used once is none, groups are numbered by their lowest
member with their members ascending, chunks hold at most `chunk` members, never span groups and run in group order.
"""
import numpy as np

import pcg_checks as PC

LD = PC.LD


def plan(N, group_of, chunk=256):
    """dict(group_ptr, members, chunk_ptr, chunk_group) by the rule of the module docstring, in plain Python."""
    by = {}
    for a in range(N):
        if group_of[a] >= 0:
            by.setdefault(int(group_of[a]), []).append(a)
    groups = sorted((m for m in by.values() if len(m) >= 2), key=lambda m: m[0])
    group_ptr, members, chunk_ptr, chunk_group = [0], [], [], []
    for g, m in enumerate(groups):
        for k in range(0, len(m), chunk):
            chunk_ptr.append(len(members) + k)
            chunk_group.append(g)
        members += m
        group_ptr.append(len(members))
    chunk_ptr.append(len(members))
    return dict(group_ptr=np.array(group_ptr, np.int32), members=np.array(members, np.int32), chunk_ptr=np.array(chunk_ptr, np.int32),
                chunk_group=np.array(chunk_group, np.int32))


def groups_of(N, group_of):
    """The groups as a list of index arrays (the plan's numbering)."""
    pl = plan(N, group_of)
    return [pl["members"][pl["group_ptr"][g]:pl["group_ptr"][g + 1]].astype(np.int64) for g in range(len(pl["group_ptr"]) - 1)]


def lift_matrix(N, groups, dtype=LD):
    """P [9N, n_free]: the free unknowns are the 9N rows with rows 6..8 of every member but a group's first removed."""
    rep, cols = _representatives(N, groups)
    P = np.zeros((9 * N, len(cols)), dtype)
    P[np.arange(9 * N), np.searchsorted(cols, rep)] = 1
    return P


def _representatives(N, groups):
    """(rep [9N]: the row that stands for row i -- rows 6..8 of a group's first member for those of every member; the kept rows)."""
    rep = np.arange(9 * N)
    for m in groups:
        for a in m[1:]:
            rep[9 * a + 6:9 * a + 9] = 9 * m[0] + 6 + np.arange(3)
    return rep, np.unique(rep)


def project(v, groups, mean=True):
    """Pi v: rows 6..8 of every member <- the group's mean (mean=False, a planted defect: the group's sum)."""
    v = np.array(v)
    w = v.reshape(-1, 9)
    for m in groups:
        s = w[m, 6:9].sum(axis=0)
        w[m, 6:9] = s / len(m) if mean else s
    return v


def reduced_system(S, rhs, groups):
    """(P'SP, P' rhs, rep, cols) in long double: the rows and columns of a group's members summed into its first member's."""
    N = len(rhs) // 9
    rep, cols = _representatives(N, groups)
    A, c = np.array(S, LD), np.array(rhs, LD)
    for m in groups:
        for q in range(6, 9):
            idx = 9 * np.asarray(m) + q
            A[idx[0], :] = A[idx, :].sum(axis=0)
            c[idx[0]] = c[idx].sum()
    for m in groups:
        for q in range(6, 9):
            idx = 9 * np.asarray(m) + q
            A[:, idx[0]] = A[:, idx].sum(axis=1)
    return A[np.ix_(cols, cols)], c[cols], rep, cols


def dense_solve(S, rhs, groups, info=None):
    """P y of (P'SP) y = P' rhs in long double: the symmetrically scaled matrix inverted in double, then iterative refinement with
    residuals in long double until the corrections stop shrinking.  info (a dict): gets `refinements` and
    `rel_residual` = |P'rhs - P'SP y| / |P'rhs| of the scaled system."""
    A, c, rep, cols = reduced_system(S, rhs, groups)
    d = 1 / np.sqrt(np.diagonal(A))
    As, cs = A * d[:, None] * d[None, :], c * d
    Ai = np.linalg.inv(As.astype(np.float64))
    x, last = np.zeros(len(cs), LD), np.inf
    for it in range(1, 31):
        dx = (Ai @ (cs - As @ x).astype(np.float64)).astype(LD)
        step = float(np.abs(dx).max())
        if step > 0.5 * last:  # (the corrections have reached the rounding errors of the long double residual)
            break
        x, last = x + dx, step
    r = cs - As @ x
    if info is not None:
        info.update(refinements=it, rel_residual=float(np.sqrt((r * r).sum() / (cs * cs).sum())))
    return (x * d)[np.searchsorted(cols, rep)]


def block_prec(Minv, dtype=LD):
    Mi = np.asarray(Minv, dtype)
    N = Mi.shape[0]
    return lambda r: np.einsum("nij,nj->ni", Mi, r.reshape(N, 9)).reshape(-1)


def projected_pcg(S, rhs, prec, groups, max_iter, rel_tol=0.0, dtype=LD, keep=None, project_z=True, mean=True, mean_rhs=True, matvec=None):
    """The recurrence of the module docstring in `dtype`.  prec: r -> M^-1 r; matvec: p -> S p (None: the dense S).  Returns dict(x,
    iters, converged, xs: {k: x_k for k in keep}, in_range: max over the iterates of the spread of rows 6..8 inside a group, 0 when the
    iterates stay in range(Pi) bit for bit).  Planted defects: project_z=False (z is not projected), mean=False (the projections of y
    and z by the sum), mean_rhs=False (that of rhs by the sum)."""
    S = np.asarray(S, dtype) if matvec is None else None
    b = project(np.asarray(rhs, dtype), groups, mean_rhs)
    keep = set(keep or ())
    tol2 = dtype(rel_tol) * dtype(rel_tol)
    mv = (lambda p: S @ p) if matvec is None else matvec

    def pz(r):
        z = prec(r)
        return project(z, groups, mean) if project_z else z

    def spread(v):
        w = v.reshape(-1, 9)
        return max([float(np.abs(w[m, 6:9] - w[m[0], 6:9]).max()) for m in groups] + [0.0])

    x = np.zeros_like(b)
    r = b.copy()
    z = pz(r)
    p = np.zeros_like(b)
    bb = (b * b).sum()
    rz = [(r * z).sum()]
    rr = [(r * r).sum()]
    xs = {}
    k, conv, out_of_range = 0, False, 0.0
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        while True:
            if rr[k] <= tol2 * bb:
                conv = True
                break
            if k == max_iter:
                break
            p = z + (dtype(0) if k == 0 else rz[k] / rz[k - 1]) * p
            y = project(mv(p), groups, mean)
            alpha = rz[k] / (p * y).sum()
            x = x + alpha * p
            r = r - alpha * y
            z = pz(r)
            rz.append((r * z).sum())
            rr.append((r * r).sum())
            k += 1
            out_of_range = max(out_of_range, spread(x))
            if k in keep:
                xs[k] = x.copy()
    return dict(x=x, iters=k, converged=conv, xs=xs, in_range=out_of_range)


def projected_rel_residual(S, x, rhs, groups):
    """|Pi (rhs - S x)| / |Pi rhs| in long double."""
    S, x, b = np.asarray(S).astype(LD), np.asarray(x).astype(LD), np.asarray(rhs).astype(LD)
    r, pb = project(b - S @ x, groups), project(b, groups)
    return float(np.sqrt((r * r).sum() / (pb * pb).sum()))


# ---- the working-precision yardstick (pcg_checks.yardstick with the projections) ---------------------------------------------------------
class Working:
    """S, rhs and the blocks B as the library forms them in `dtype` (pcg_checks.yardstick says why): B = V - (its eliminated part),
    rhs = g - (its eliminated part), the product S p = V p - (V - S) p, every difference of two terms rounded to dtype; the blocks
    inverted in dtype.  ok: every block positive definite in that arithmetic.  (S, rhs, B, V long double; g the camera part of the
    gradient.)"""

    def __init__(self, S, rhs, B, V, g, dtype):
        Sl, Vl, Bl = np.asarray(S, LD), np.asarray(V, LD), np.asarray(B, LD)
        gl, rl = np.asarray(g, LD), np.asarray(rhs, LD)
        self.dtype, self.N = dtype, len(Bl)
        self.rhs = gl.astype(dtype) - (gl - rl).astype(dtype)
        Mi, ok = PC.invert_blocks(Vl.astype(dtype) - (Vl - Bl).astype(dtype), dtype)
        self.ok = bool(ok.all())
        self.prec = block_prec(Mi, dtype)
        self.Vd = Vl.astype(dtype)
        self.E = PC._minus_blocks(Sl, Vl).astype(dtype)

    def matvec(self, p):
        return np.einsum("nij,nj->ni", self.Vd, p.reshape(self.N, 9)).reshape(-1) - self.E @ p

    def pcg(self, groups, max_iter, rel_tol=0.0, keep=None):
        """The projected PCG in dtype; None when a block is not positive definite or an iterate is not finite (the caller then scales
        the fp64 yardstick by eps / eps64, tests/test_gpu_stages.py's rule)."""
        if not self.ok:
            return None
        out = projected_pcg(None, self.rhs, self.prec, groups, max_iter, rel_tol, self.dtype, keep, matvec=self.matvec)
        if not all(np.all(np.isfinite(v.astype(np.float64))) for v in list(out["xs"].values()) + [out["x"]]):
            return None
        return out

    def rel_residual(self, x, groups):
        """|Pi (rhs - S x)| / |Pi rhs| formed in dtype: the yardstick of the device's own residual statistic."""
        x = np.asarray(x).astype(self.dtype)
        b = project(self.rhs, groups)
        r = b - project(self.matvec(x), groups)
        return float(np.sqrt((r * r).sum() / (b * b).sum()))


# ---- an end-to-end scene: every camera IS one physical camera ---------------------------------------------------------------------------
def _rodrigues(w):
    th = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    return np.eye(3) if th < 1e-12 else np.eye(3) + np.sin(th) / th * K + (1 - np.cos(th)) / th ** 2 * (K @ K)


def _log_so3(R):
    th = np.arccos(np.clip((np.trace(R) - 1) / 2, -1, 1))
    v = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]]) / 2
    return v if th < 1e-12 else v * th / np.sin(th)


def project_pre(cams9, pts, cam_idx, pt_idx):
    """The camera model of the BAL "-pre" files as the loader reads them (include/ba_mi355x.h: the solver holds f = -f_file,
    k1 = k1_file f^2, k2 = k2_file f^4): P = R(omega) X + T, u = P_xy / P_z, pixel = f (1 + k1 |u|^2 + k2 |u|^4) u; cams9 rows
    (omega, T, f_file, k1_file, k2_file)."""
    c = np.asarray(cams9, np.float64).reshape(-1, 9)
    X = np.asarray(pts, np.float64).reshape(-1, 3)
    R = np.stack([_rodrigues(w) for w in c[:, :3]])
    P = np.einsum("kij,kj->ki", R[cam_idx], X[pt_idx]) + c[cam_idx, 3:6]
    u = P[:, :2] / P[:, 2:3]
    n = (u * u).sum(axis=1)
    f = -c[cam_idx, 6]
    return (f * (1 + c[cam_idx, 7] * f ** 2 * n + c[cam_idx, 8] * f ** 4 * n * n))[:, None] * u


def one_camera_scene(N=12, M=400, noise=0.5, seed=17, intr=(-900.0, -0.06, 0.012)):
    """dict(N, M, K, cam_idx, pt_idx, meas, cams9, pts, noise_energy): N frames of ONE camera (f, k1, k2 = intr in the solver's units, the
    last three of BA_GET_CAMS) on a ring around M points in a ball, every frame sees every point, Gaussian noise of `noise` px per
    coordinate on the measurements; cams9 and pts are the truth."""
    rng = np.random.default_rng(seed)
    pts = rng.uniform(-1, 1, (4 * M, 3))
    pts = pts[(pts * pts).sum(axis=1) <= 1][:M]
    assert len(pts) == M
    cams = np.zeros((N, 9))
    for a in range(N):
        phi = 2 * np.pi * a / N
        C = np.array([6 * np.cos(phi), 6 * np.sin(phi), 1.5 * np.sin(3 * phi) + 0.5 * rng.standard_normal()])
        z = C / np.linalg.norm(C)  # the camera looks down its -z axis: z points away from the scene
        x = np.cross([0, 0, 1.0], z)
        x /= np.linalg.norm(x)
        R = np.stack([x, np.cross(z, x), z])
        cams[a, :3], cams[a, 3:6] = _log_so3(R), -R @ C
        cams[a, 6:] = -intr[0], intr[1] / intr[0] ** 2, intr[2] / intr[0] ** 4
    cam_idx = np.tile(np.arange(N, dtype=np.int32), M)
    pt_idx = np.repeat(np.arange(M, dtype=np.int32), N)  # (sorted by point)
    exact = project_pre(cams, pts, cam_idx, pt_idx)
    meas = exact + noise * rng.standard_normal((N * M, 2))
    return dict(N=N, M=M, K=N * M, cam_idx=cam_idx, pt_idx=pt_idx, meas=meas.ravel(), cams9=cams, pts=pts,
                noise_energy=float(((meas - exact) ** 2).sum()))


def end_to_end(ba):
    """12 frames of one physical camera, 400 points, 0.5 px noise, plain least squares, the gauge fixed (one_camera_scene).
    ITERSCHUR with one group of all cameras from the truth with the shared f off by 1 %, to its own stop, against CHOLESKY with the
    intrinsics held at the truth from the truth.  Returns dict(shared, fixed: the two ba_minimize results; f_true, f_start, f_end;
    stats: ba_solver_pcg_stats of the shared run; noise_energy)."""
    sc = one_camera_scene()
    pg = ba.Problem.from_arrays(sc["N"], sc["M"], sc["K"], sc["cam_idx"], sc["pt_idx"], sc["meas"], sc["cams9"], sc["pts"])
    gauge = pg.gauge_mask(0)
    out = dict(noise_energy=sc["noise_energy"])
    c = ba.Solver(pg, ba.CHOLESKY, ba.F64)
    c.set_loss(ba.LOSS_TRIVIAL)
    c.set_constant(gauge | np.uint16(ba.FIX_INTRINSICS), None)
    out["fixed"] = c.minimize(max_trials=500)
    s = ba.Solver(pg, ba.ITERSCHUR, ba.F64)
    s.set_loss(ba.LOSS_TRIVIAL)
    s.set_constant(gauge, None)
    cams = s.get(ba.GET_CAMS).reshape(-1, 15).copy()
    out["f_true"] = float(cams[0, 12])
    assert np.all(cams[:, 12:15] == cams[0, 12:15])
    cams[:, 12] = cams[0, 12] * 1.01
    out["f_start"] = float(cams[0, 12])
    s.set_state(cams.ravel(), None)
    s.set_shared_intrinsics(np.zeros(sc["N"], np.int32))
    out["shared"] = s.minimize(max_trials=500)
    end = s.get(ba.GET_CAMS).reshape(-1, 15)
    out["equal"] = bool(np.all(end[:, 12:15].view(np.uint64) == end[0, 12:15].view(np.uint64)))
    out["f_end"] = float(end[0, 12])
    out["stats"] = s.pcg_stats()
    return out
