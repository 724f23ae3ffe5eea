"""Yardstick of the relative-pose constraints (ba_solver_set_relative_poses; include/ba_mi355x.h) -- TEST
INFRASTRUCTURE ONLY, np.longdouble throughout, restated from the formulas and not taken from the library.

For cameras a, b of a state cam15 [N, 15] = R (9, row-major), T (3), f, k1, k2 (x_cam = R X + T):

    R_ab = R_b R_a',  t_ab = T_b - R_ab T_a
    e_t = L_t (t_ab - t0)                      e_r = L_r phi,  phi = Log(R_ab R0')
    d e_t / d(T_a, om_a) = L_t [-R_ab | -R_ab [T_a]x]        d e_t / d(T_b, om_b) = L_t [I | [u]x],  u = R_ab T_a
    d e_r / d(T_a, om_a) = L_r [0 | -Jl^-1 R_ab]             d e_r / d(T_b, om_b) = L_r [0 | Jl^-1]
    Jl^-1 = I - [phi]x / 2 + c [phi]x^2,  c = 1 / th^2 - (1 + cos th) / (2 th sin th)

for the retraction T + dT, R <- Rodrigues(d omega) R (prior_checks.retract).  A constraint's rows are ordered (e_t, e_r), its columns
(T_a, om_a, T_b, om_b).  tests/test_relpose_checks.py pins this file on the CPU."""
import numpy as np

from prior_checks import LD, skew, rodrigues, retract  # noqa: F401  (retract: re-exported for the tests)


class Constraints:
    """The lists as the C ABI takes them (empty by default)."""

    def __init__(self, pairs=(), R0=(), t0=(), Lr=(), Lt=()):
        self.pairs = np.asarray(pairs, np.int32).reshape(-1, 2)
        n = len(self.pairs)
        self.R0 = np.asarray(R0, np.float64).reshape(n, 3, 3)
        self.t0 = np.asarray(t0, np.float64).reshape(n, 3)
        self.Lr = np.asarray(Lr, np.float64).reshape(n, 3, 3)
        self.Lt = np.asarray(Lt, np.float64).reshape(n, 3, 3)

    def __len__(self):
        return len(self.pairs)

    def rounded(self, dtype):
        """The lists as a solver of that scalar type holds them."""
        r = lambda a: a.astype(dtype).astype(np.float64)
        return Constraints(self.pairs, r(self.R0), r(self.t0), r(self.Lr), r(self.Lt))

    def apply(self, s):
        s.set_relative_poses(self.pairs, self.R0, self.t0, sqrt_info_rot=self.Lr, sqrt_info_trans=self.Lt)


def log_so3(E, dt=LD):
    """Rotation vector of a rotation matrix, |phi| < pi (asin's series below sin(theta) = 1e-4).  dt, here and below: the arithmetic -- long double for the
    yardstick; a working precision gives the plain evaluation of the same formulas in it, the "oracle's own error" of the GPU tests."""
    E = np.asarray(E, dt)
    v = dt(0.5) * np.array([E[2, 1] - E[1, 2], E[0, 2] - E[2, 0], E[1, 0] - E[0, 1]], dt)
    s2 = (v * v).sum()
    s, c = np.sqrt(s2), dt(0.5) * (np.trace(E) - 1)
    th = np.arctan2(s, c)
    f = 1 + s2 / 6 + 3 * s2 * s2 / 40 + 15 * s2 ** 3 / 336 if (s < 1e-4 and c > 0) else th / s
    return f * v


def jl(phi):
    """Left Jacobian of SO(3): I + (1 - cos th) / th^2 [phi]x + (th - sin th) / th^3 [phi]x^2."""
    phi = np.asarray(phi, LD)
    th2 = (phi * phi).sum()
    th = np.sqrt(th2)
    if th < 0.05:  # (the closed forms lose eps / th^2 to cancellation; the series' next terms are below 1e-21 here)
        a = LD(0.5) - th2 / 24 + th2 ** 2 / 720 - th2 ** 3 / 40320 + th2 ** 4 / 3628800
        b = LD(1) / 6 - th2 / 120 + th2 ** 2 / 5040 - th2 ** 3 / 362880 + th2 ** 4 / 39916800
    else:
        a, b = (1 - np.cos(th)) / th2, (th - np.sin(th)) / (th2 * th)
    P = skew(phi)
    return np.eye(3, dtype=LD) + a * P + b * (P @ P)


def jl_inv(phi, dt=LD):
    """I - [phi]x / 2 + c [phi]x^2, c = 1 / th^2 - (1 + cos th) / (2 th sin th) (the series of cot below th = 0.02)."""
    phi = np.asarray(phi, dt)
    th2 = (phi * phi).sum()
    th = np.sqrt(th2)
    if th < 0.02:
        c = dt(1) / 12 + th2 / 720 + th2 ** 2 / 30240 + th2 ** 3 / 1209600 + th2 ** 4 / 47900160
    else:
        c = 1 / th2 - (1 + np.cos(th)) / (2 * th * np.sin(th))
    P = skew(phi)
    return np.eye(3, dtype=dt) - P / 2 + c * (P @ P)


def relative_pose(cam15, a, b, dt=LD):
    c = np.asarray(cam15, dt).reshape(-1, 15)
    Rab = c[b, :9].reshape(3, 3) @ c[a, :9].reshape(3, 3).T
    return Rab, c[b, 9:12] - Rab @ c[a, 9:12]


def residuals(cs, cam15, dt=LD):
    """(e_t [n, 3], e_r [n, 3], phi [n, 3]) in long double."""
    et, er, ph = np.zeros((len(cs), 3), dt), np.zeros((len(cs), 3), dt), np.zeros((len(cs), 3), dt)
    for q, (a, b) in enumerate(cs.pairs):
        Rab, tab = relative_pose(cam15, a, b, dt)
        ph[q] = log_so3(Rab @ cs.R0[q].astype(dt).T, dt)
        et[q] = cs.Lt[q].astype(dt) @ (tab - cs.t0[q].astype(dt))
        er[q] = cs.Lr[q].astype(dt) @ ph[q]
    return et, er, ph


def energies(cs, cam15):
    """[sum |e_r|^2, sum |e_t|^2] (the order of ba_solver_relative_pose_energy)."""
    et, er, _ = residuals(cs, cam15)
    return np.array([(er * er).sum(), (et * et).sum()], LD)


def jacobians(cs, cam15, cam_mask=None, dt=LD):
    """[n, 6, 12]: rows (e_t, e_r), columns (T_a, om_a, T_b, om_b); masked columns zero."""
    c = np.asarray(cam15, dt).reshape(-1, 15)
    J = np.zeros((len(cs), 6, 12), dt)
    _, _, ph = residuals(cs, cam15, dt)
    for q, (a, b) in enumerate(cs.pairs):
        Rab, _ = relative_pose(c, a, b, dt)
        Ta = c[a, 9:12]
        Ji, Lt, Lr = jl_inv(ph[q], dt), cs.Lt[q].astype(dt), cs.Lr[q].astype(dt)
        J[q, :3, 0:3] = Lt @ (-Rab)
        J[q, :3, 3:6] = Lt @ (-Rab @ skew(Ta))
        J[q, :3, 6:9] = Lt
        J[q, :3, 9:12] = Lt @ skew(Rab @ Ta)
        J[q, 3:, 3:6] = Lr @ (-Ji @ Rab)
        J[q, 3:, 9:12] = Lr @ Ji
        if cam_mask is not None:
            for side, cam in ((0, a), (1, b)):
                free = ((int(cam_mask[cam]) >> np.arange(6)) & 1) == 0
                J[q, :, 6 * side:6 * side + 6] *= free[None, :]
    return J


def direct(cs, N, cam15, cam_mask=None, dt=LD):
    """dict(V [N, 9, 9], g (9N: -J'e), cross {(a, b): H_ab 6 x 6 = J_a'J_b}, S (9N x 9N: V's blocks and the cross blocks, both
    triangles), energies (2: rotation, translation), energy): what the constraints add to the camera part of the normal equations --
    the point elimination touches none of it, so S is also what they add to the reduced matrix."""
    et, er, _ = residuals(cs, cam15, dt)
    J = jacobians(cs, cam15, cam_mask, dt)
    V, g, S, cross = np.zeros((N, 9, 9), dt), np.zeros(9 * N, dt), np.zeros((9 * N, 9 * N), dt), {}
    for q, (a, b) in enumerate(cs.pairs):
        e = np.concatenate([et[q], er[q]])
        Ja, Jb = J[q, :, :6], J[q, :, 6:]
        V[a, :6, :6] += Ja.T @ Ja
        V[b, :6, :6] += Jb.T @ Jb
        g[9 * a:9 * a + 6] -= Ja.T @ e
        g[9 * b:9 * b + 6] -= Jb.T @ e
        cross[(int(a), int(b))] = Ja.T @ Jb
        S[9 * a:9 * a + 6, 9 * b:9 * b + 6] += Ja.T @ Jb
        S[9 * b:9 * b + 6, 9 * a:9 * a + 6] += Jb.T @ Ja
    for a in range(N):
        S[9 * a:9 * a + 9, 9 * a:9 * a + 9] += V[a]
    en = np.array([(er * er).sum(), (et * et).sum()], dt)
    return dict(V=V, g=g, cross=cross, S=S, energies=en, energy=en.sum())


def stacked(cs, N, cam15, cam_mask=None):
    """(J [6n, 9N] dense, e [6n]) of the stacked constraint rows."""
    et, er, _ = residuals(cs, cam15)
    Jq = jacobians(cs, cam15, cam_mask)
    J, e = np.zeros((6 * len(cs), 9 * N), LD), np.zeros(6 * len(cs), LD)
    for q, (a, b) in enumerate(cs.pairs):
        J[6 * q:6 * q + 6, 9 * a:9 * a + 6] = Jq[q, :, :6]
        J[6 * q:6 * q + 6, 9 * b:9 * b + 6] = Jq[q, :, 6:]
        e[6 * q:6 * q + 3], e[6 * q + 3:6 * q + 6] = et[q], er[q]
    return J, e


def reduced(S_base, rhs_base, d):
    """The reduced camera system of the constrained problem: cov_checks' / the referee's reduced matrix and rhs of the (prior-augmented)
    observations plus the additions of `direct` (long double)."""
    return np.asarray(S_base).astype(LD) + d["S"], np.asarray(rhs_base).astype(LD) + d["g"]


def standard_constraints(N, cam_idx, pt_idx, cam15, Vdiag, seed=11, kappa_t=10.0, kappa_r=1.0, angle=0.05):
    """The constraint set of the GPU tests: an odometry chain (a, a + 1) over all cameras plus one hub camera tied to 40 others (to all
    of them if N <= 41; pairs the chain already holds are left out).  The hub is the camera that shares no point with the most others,
    so that pairs without a common point occur whenever the problem has one.  R0, t0: the start state's relative pose perturbed by a
    rotation of `angle` rad (one value, or one per constraint, cycled if shorter than the list; 0.05 by default: the cot-series switch
    of ba_relpose_eval) about a seeded axis and by 1 % of |t_ab| in a seeded direction.  Information, sized like
    prior_checks.standard_priors: kappa x the median own diagonal of the blocks joined (Vdiag [N, 9] = diag of sum Jc'Jc), i.e.
    sigma_t = 1 / sqrt(kappa_t median V_TT), sigma_r = 1 / sqrt(kappa_r median V_omega omega), kappa_t = 10 (an upper-triangular L_t with
    off-diagonals 0.3 / sigma), kappa_r = 1 (isotropic), both inside [1e-2, 1e2].  Returns (Constraints, dict(sigma_t, sigma_r, hub,
    n, n_no_common, max_common))."""
    rng = np.random.default_rng(seed)
    cam15 = np.asarray(cam15, np.float64).reshape(N, 15)
    cov = np.zeros((N, N), np.int64)  # common points per pair
    order = np.argsort(pt_idx, kind="stable")
    ci, pi = np.asarray(cam_idx)[order], np.asarray(pt_idx)[order]
    start = np.flatnonzero(np.r_[True, pi[1:] != pi[:-1], True])
    for s0, s1 in zip(start[:-1], start[1:]):
        cs_ = np.unique(ci[s0:s1])
        cov[np.ix_(cs_, cs_)] += 1
    hub = int(np.argmax((cov == 0).sum(axis=1)))
    pairs = [(a, a + 1) for a in range(N - 1)]
    have = {frozenset(p) for p in pairs}
    others = [b for b in range(N) if b != hub and frozenset((hub, b)) not in have]
    others.sort(key=lambda b: (cov[hub, b] != 0, b))  # the ones without a common point first
    pairs += [(hub, b) if k % 2 == 0 else (b, hub) for k, b in enumerate(others[:40])]
    pairs = np.array(pairs, np.int32).reshape(-1, 2)
    n = len(pairs)
    Vdiag = np.asarray(Vdiag, np.float64).reshape(N, 9)
    st = 1 / np.sqrt(kappa_t * np.median(Vdiag[:, :3]))
    sr = 1 / np.sqrt(kappa_r * np.median(Vdiag[:, 3:6]))
    R0, t0 = np.zeros((n, 3, 3)), np.zeros((n, 3))
    ang = np.resize(np.asarray(angle, np.float64), n)
    for q, (a, b) in enumerate(pairs):
        Rab, tab = relative_pose(cam15, a, b)
        ax, dr = rng.standard_normal(3), rng.standard_normal(3)
        R0[q] = (rodrigues(ang[q] * ax / np.linalg.norm(ax)) @ Rab).astype(np.float64)
        t0[q] = (tab + 0.01 * np.sqrt(float((tab * tab).sum())) * dr / np.linalg.norm(dr)).astype(np.float64)
    Lt = np.tile(np.array([[1.0, 0.3, 0.3], [0, 1.0, 0.3], [0, 0, 1.0]]) / st, (n, 1, 1))
    Lr = np.tile(np.eye(3) / sr, (n, 1, 1))
    common = cov[pairs[:, 0], pairs[:, 1]]
    return Constraints(pairs, R0, t0, Lr, Lt), dict(sigma_t=st, sigma_r=sr, hub=hub, n=n, n_no_common=int((common == 0).sum()),
                                                    max_common=int(common.max()))


def lm_dense(fun, x0, retract_fn, max_iter=60, lam0=1e-3):
    """A plain long-double Levenberg-Marquardt on dense normal equations: fun(x) -> (J [m, n], e [m]) of all rows, retract_fn(x, dx).
    Accept when the energy drops (lambda / 10), else lambda x 10.  Returns the last accepted state and its energy."""
    x = x0
    J, e = fun(x)
    E = (e * e).sum()
    lam = LD(lam0) * np.max(np.einsum("ij,ij->j", J, J))
    for _ in range(max_iter):
        H = J.T @ J
        g = -J.T @ e
        A = H + lam * np.eye(H.shape[0], dtype=LD)
        # long-double solve: numpy's LAPACK has none, so Gaussian elimination with partial pivoting here
        dx = _solve(A, g)
        xt = retract_fn(x, dx)
        Jt, et = fun(xt)
        Et = (et * et).sum()
        if Et < E:
            done = (E - Et) <= LD(1e-30) * E
            x, J, e, E, lam = xt, Jt, et, Et, lam / 10
            if done:
                break
        else:
            lam = lam * 10
            if lam > 1e30:
                break
    return x, E


def _solve(A, b):
    A, b = np.array(A, LD), np.array(b, LD)
    n = len(b)
    for k in range(n):
        p = k + int(np.argmax(np.abs(A[k:, k])))
        if p != k:
            A[[k, p]], b[[k, p]] = A[[p, k]], b[[p, k]]
        if A[k, k] == 0:
            continue
        m = A[k + 1:, k] / A[k, k]
        A[k + 1:, k:] -= m[:, None] * A[k, k:][None, :]
        b[k + 1:] -= m * b[k]
    x = np.zeros(n, LD)
    for k in range(n - 1, -1, -1):
        x[k] = (b[k] - (A[k, k + 1:] * x[k + 1:]).sum()) / A[k, k] if A[k, k] != 0 else 0
    return x
