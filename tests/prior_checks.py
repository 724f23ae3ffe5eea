"""Yardstick of the Gaussian priors (ba_solver_set_point_priors / _centre_priors / _intrinsics_priors; include/ba_mi355x.h, DESIGN.md
section 13) -- TEST INFRASTRUCTURE ONLY, np.longdouble throughout.

    point       e = L (X - X0)                              J = L on the point's 3 columns
    centre      e = L (C - C0),  C = -R' T                  J = L [-R' | -R' [T]x | 0 0 0] on the camera's columns (T, omega, f, k1, k2)
    intrinsics  e_q = w_q (x_q - x0_q), q in (f, k1, k2)    J = w_q on column 6 + q

for the retraction T + dT, R <- Rodrigues(d omega) R, additive f, k1, k2 and points (restated here as `retract`, not taken from the
library).  The states are the solver's own: cam15 [N, 15] = R (9, row-major), T (3), f, k1, k2; pts [M, 3].

Two forms of the same thing: `direct` (the additions to the per-point U, the per-camera V, g and the energy) and `augment` (every
prior as pseudo-observations of an augmented problem, so that the per-observation functions of cov_checks.py -- reduced_matrix,
reference_covariance, quad_reduced, mask_jacobian -- serve unchanged: a point prior is two 2-row observations with Jc = 0, the
fourth row zero; a centre or intrinsics prior has Jp = 0).  tests/test_prior_checks.py pins this file on the CPU.
"""
import numpy as np

LD = np.longdouble


class Priors:
    """The three lists, as the C ABI takes them (empty by default)."""

    def __init__(self, pt_ids=(), pt_x0=(), pt_L=(), c_ids=(), c_c0=(), c_L=(), i_ids=(), i_x0=(), i_w=()):
        self.pt_ids = np.asarray(pt_ids, np.int32).reshape(-1)
        self.pt_x0 = np.asarray(pt_x0, np.float64).reshape(-1, 3)
        self.pt_L = np.asarray(pt_L, np.float64).reshape(-1, 3, 3)
        self.c_ids = np.asarray(c_ids, np.int32).reshape(-1)
        self.c_c0 = np.asarray(c_c0, np.float64).reshape(-1, 3)
        self.c_L = np.asarray(c_L, np.float64).reshape(-1, 3, 3)
        self.i_ids = np.asarray(i_ids, np.int32).reshape(-1)
        self.i_x0 = np.asarray(i_x0, np.float64).reshape(-1, 3)
        self.i_w = np.asarray(i_w, np.float64).reshape(-1, 3)

    def rounded(self, dtype):
        """The lists as a solver of that scalar type holds them."""
        r = lambda a: a.astype(dtype).astype(np.float64)
        return Priors(self.pt_ids, r(self.pt_x0), r(self.pt_L), self.c_ids, r(self.c_c0), r(self.c_L), self.i_ids, r(self.i_x0), r(self.i_w))

    def apply(self, s):
        """Hands the lists to a bundleadjustment_benchmarks_amd.Solver."""
        s.set_point_priors(self.pt_ids, self.pt_x0, sqrt_info=self.pt_L)
        s.set_centre_priors(self.c_ids, self.c_c0, sqrt_info=self.c_L)
        lib, _p = _binding()
        rc = lib.ba_solver_set_intrinsics_priors(s._h, len(self.i_ids), _p(np.ascontiguousarray(self.i_ids)), _p(np.ascontiguousarray(self.i_x0)),
                                                 _p(np.ascontiguousarray(self.i_w)))  # (w itself, zeros included: the binding takes sigma)
        assert rc == 0, rc


def _binding():
    import bundleadjustment_benchmarks_amd as ba
    return ba.lib(), ba._p


def skew(t):
    z = np.zeros_like(t[..., 0])
    return np.stack([np.stack([z, -t[..., 2], t[..., 1]], -1), np.stack([t[..., 2], z, -t[..., 0]], -1),
                     np.stack([-t[..., 1], t[..., 0], z], -1)], -2)


def centres(cam15):
    c = np.asarray(cam15, LD).reshape(-1, 15)
    return -np.einsum("nki,nk->ni", c[:, :9].reshape(-1, 3, 3), c[:, 9:12])


def rodrigues(w):
    """exp([w]x) in long double (series below 1e-4: no 0 / 0)."""
    w = np.asarray(w, LD)
    th = np.sqrt((w * w).sum())
    K = skew(w)
    if th < 1e-4:
        c1, c2 = 1 - th * th / 6 + th ** 4 / 120, LD(0.5) - th * th / 24 + th ** 4 / 720
    else:
        c1, c2 = np.sin(th) / th, (1 - np.cos(th)) / (th * th)
    return np.eye(3, dtype=LD) + c1 * K + c2 * (K @ K)


def retract(cam15, pts, dx):
    """x (+) dx: dx = [3M points | 9N cameras (T, omega, f, k1, k2)]; T + dT, R <- Rodrigues(d omega) R, the rest additive."""
    c = np.array(cam15, LD).reshape(-1, 15)
    x = np.array(pts, LD).reshape(-1, 3)
    dx = np.asarray(dx, LD)
    M, N = len(x), len(c)
    x = x + dx[:3 * M].reshape(M, 3)
    d = dx[3 * M:].reshape(N, 9)
    for a in range(N):
        if d[a, 3:6].any():
            c[a, :9] = (rodrigues(d[a, 3:6]) @ c[a, :9].reshape(3, 3)).reshape(-1)
    c[:, 9:12] += d[:, :3]
    c[:, 12:15] += d[:, 6:9]
    return c, x


def rows(pr, cam15, pts):
    """(e_pt [n, 3], e_centre [n, 3], e_intrinsics [n, 3]) in long double."""
    c = np.asarray(cam15, LD).reshape(-1, 15)
    x = np.asarray(pts, LD).reshape(-1, 3)
    ep = np.einsum("nij,nj->ni", pr.pt_L.astype(LD), x[pr.pt_ids] - pr.pt_x0.astype(LD))
    ec = np.einsum("nij,nj->ni", pr.c_L.astype(LD), centres(c)[pr.c_ids] - pr.c_c0.astype(LD))
    ei = pr.i_w.astype(LD) * (c[pr.i_ids, 12:15] - pr.i_x0.astype(LD))
    return ep, ec, ei


def energies(pr, cam15, pts):
    return np.array([(e * e).sum() for e in rows(pr, cam15, pts)], LD)


def jacobians(pr, cam15, cam_mask=None, pt_fixed=None):
    """(J_pt [n, 3, 3] on the point's columns, J_centre [n, 3, 9], J_intrinsics [n, 3, 9] on the camera's), masked columns zero."""
    c = np.asarray(cam15, LD).reshape(-1, 15)
    R, T = c[pr.c_ids, :9].reshape(-1, 3, 3), c[pr.c_ids, 9:12]
    Rt = np.swapaxes(R, 1, 2)
    dC = np.concatenate([-Rt, -np.einsum("nij,njk->nik", Rt, skew(T)), np.zeros((len(R), 3, 3), LD)], axis=2)
    Jc = np.einsum("nij,njk->nik", pr.c_L.astype(LD), dC)
    Ji = np.zeros((len(pr.i_ids), 3, 9), LD)
    for q in range(3):
        Ji[:, q, 6 + q] = pr.i_w[:, q]
    Jp = pr.pt_L.astype(LD).copy()
    if cam_mask is not None:
        free = ((np.asarray(cam_mask, np.uint32)[:, None] >> np.arange(9)[None, :]) & 1) == 0
        Jc = Jc * free[pr.c_ids][:, None, :]
        Ji = Ji * free[pr.i_ids][:, None, :]
    if pt_fixed is not None:
        Jp = Jp * (np.asarray(pt_fixed)[pr.pt_ids] == 0)[:, None, None]
    return Jp, Jc, Ji


def direct(pr, N, M, cam15, pts, cam_mask=None, pt_fixed=None):
    """dict(U [M, 3, 3], V [N, 9, 9], g (3M + 9N, points first: -J'e), energies (3), energy): what the priors add."""
    ep, ec, ei = rows(pr, cam15, pts)
    Jp, Jc, Ji = jacobians(pr, cam15, cam_mask, pt_fixed)
    U, V, g = np.zeros((M, 3, 3), LD), np.zeros((N, 9, 9), LD), np.zeros(3 * M + 9 * N, LD)
    np.add.at(U, pr.pt_ids, np.einsum("nki,nkj->nij", Jp, Jp))
    np.add.at(g[:3 * M].reshape(M, 3), pr.pt_ids, -np.einsum("nki,nk->ni", Jp, ep))
    for ids, J, e in ((pr.c_ids, Jc, ec), (pr.i_ids, Ji, ei)):
        np.add.at(V, ids, np.einsum("nki,nkj->nij", J, J))
        np.add.at(g[3 * M:].reshape(N, 9), ids, -np.einsum("nki,nk->ni", J, e))
    en = np.array([(e * e).sum() for e in (ep, ec, ei)], LD)
    return dict(U=U, V=V, g=g, energies=en, energy=en.sum())


def augment(pr, cam_idx, pt_idx, Jc, Jp, e, cam15, pts, cam_mask=None, pt_fixed=None):
    """The observations (cam_idx, pt_idx, Jc [K, 2, 9], Jp [K, 2, 3], e [K, 2]) followed by the priors as pseudo-observations, sorted by
    point (stable): (cam_idx, pt_idx, Jc, Jp, e) of the augmented problem, long double.  A camera prior's pseudo-observations (Jp = 0)
    are booked on point (camera mod M), so that no track grows by more than a few of them."""
    M = len(np.asarray(pts).reshape(-1, 3))
    ep, ec, ei = rows(pr, cam15, pts)
    Jpp, Jcc, Jci = jacobians(pr, cam15, cam_mask, pt_fixed)
    ca, pa, JC, JP, E = [np.asarray(cam_idx, np.int32)], [np.asarray(pt_idx, np.int32)], [np.asarray(Jc, LD)], [np.asarray(Jp, LD)], [np.asarray(e, LD).reshape(-1, 2)]

    def two(J3, e3):  # 3 rows -> two 2-row blocks, the fourth row zero
        n, w = J3.shape[0], J3.shape[2]
        J4 = np.concatenate([J3, np.zeros((n, 1, w), LD)], axis=1).reshape(2 * n, 2, w)
        e4 = np.concatenate([e3, np.zeros((n, 1), LD)], axis=1).reshape(2 * n, 2)
        return J4, e4
    J4, e4 = two(Jpp, ep)
    ca.append(np.zeros(len(J4), np.int32)); pa.append(np.repeat(pr.pt_ids, 2)); JC.append(np.zeros((len(J4), 2, 9), LD)); JP.append(J4); E.append(e4)
    for ids, J3, e3 in ((pr.c_ids, Jcc, ec), (pr.i_ids, Jci, ei)):
        J4, e4 = two(J3, e3)
        ca.append(np.repeat(ids, 2)); pa.append(np.repeat(ids % M, 2).astype(np.int32)); JC.append(J4); JP.append(np.zeros((len(J4), 2, 3), LD)); E.append(e4)
    ca, pa, JC, JP, E = [np.concatenate(v) for v in (ca, pa, JC, JP, E)]
    o = np.argsort(pa, kind="stable")
    return ca[o].astype(np.int32), pa[o].astype(np.int32), JC[o], JP[o], E[o]


def normal_blocks(N, M, cam_idx, pt_idx, Jc, Jp, e):
    """U [M, 3, 3], V [N, 9, 9], g = -J'e (3M + 9N) and sum e^2 of per-observation blocks, long double."""
    Jc, Jp, e = np.asarray(Jc, LD), np.asarray(Jp, LD), np.asarray(e, LD).reshape(-1, 2)
    U, V, g = np.zeros((M, 3, 3), LD), np.zeros((N, 9, 9), LD), np.zeros(3 * M + 9 * N, LD)
    np.add.at(U, pt_idx, np.einsum("kai,kaj->kij", Jp, Jp))
    np.add.at(V, cam_idx, np.einsum("kai,kaj->kij", Jc, Jc))
    np.add.at(g[:3 * M].reshape(M, 3), pt_idx, -np.einsum("kai,ka->ki", Jp, e))
    np.add.at(g[3 * M:].reshape(N, 9), cam_idx, -np.einsum("kai,ka->ki", Jc, e))
    return U, V, g, (e * e).sum()


def standard_priors(N, M, K, pt_idx, cam15, pts, Jc, Jp, cam_idx, seed=5, frac=0.01):
    """The prior set of the GPU tests, sized from the problem's own J'J (Jc [K, 2, 9], Jp [K, 2, 3] of a linearisation, doubles):
    points -- about 1 % (seeded) plus every point with fewer than 3 observations; centres -- all cameras; intrinsics -- f and k1 of
    every second camera, w = 0 for k2.  Targets X0 / C0 / x0 are the state moved by a seeded fraction of sigma.  Each prior's
    information is  kappa x (the median own diagonal of the blocks it joins), i.e. sigma = 1 / sqrt(kappa median), with
        kappa = 1 (points: isotropic L = I / sigma), kappa = 10 (centres: an upper-triangular L with off-diagonals 0.3 / sigma),
        kappa = 0.1 (f) and 1 (k1),
    all inside the [1e-2, 1e2] x median band the issue sets.  Returns (Priors, dict of the sigmas)."""
    rng = np.random.default_rng(seed)
    cam15 = np.asarray(cam15, np.float64).reshape(N, 15)
    pts = np.asarray(pts, np.float64).reshape(M, 3)
    U = np.zeros((M, 3)); np.add.at(U, pt_idx, (np.asarray(Jp, np.float64) ** 2).sum(axis=1))
    V = np.zeros((N, 9)); np.add.at(V, cam_idx, (np.asarray(Jc, np.float64) ** 2).sum(axis=1))
    cnt = np.bincount(pt_idx, minlength=M)
    sel = np.zeros(M, bool)
    sel[rng.choice(M, max(1, int(round(frac * M))), replace=False)] = True
    sel |= cnt < 3
    pid = np.flatnonzero(sel).astype(np.int32)
    sp = 1 / np.sqrt(1.0 * np.median(U[U > 0]))
    # a centre moves like T (dC = -R' dT): the T diagonals are the block it joins
    sc = 1 / np.sqrt(10.0 * np.median(V[:, :3]))
    sf, sk1 = 1 / np.sqrt(0.1 * np.median(V[:, 6])), 1 / np.sqrt(1.0 * np.median(V[:, 7]))
    Lc = np.array([[1.0, 0.3, 0.3], [0, 1.0, 0.3], [0, 0, 1.0]]) / sc
    cid = np.arange(N, dtype=np.int32)
    iid = np.arange(0, N, 2, dtype=np.int32)
    C = np.asarray(centres(cam15), np.float64)
    pr = Priors(pid, pts[pid] + 0.5 * sp * rng.standard_normal((len(pid), 3)), np.tile(np.eye(3) / sp, (len(pid), 1, 1)),
                cid, C + 0.5 * sc * rng.standard_normal((N, 3)), np.tile(Lc, (N, 1, 1)),
                iid, cam15[iid, 12:15] + 0.5 * np.array([sf, sk1, 0.0]) * rng.standard_normal((len(iid), 3)),
                np.tile(np.array([1 / sf, 1 / sk1, 0.0]), (len(iid), 1)))
    return pr, dict(point=sp, centre=sc, f=sf, k1=sk1)
