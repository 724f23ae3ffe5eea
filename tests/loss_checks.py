"""Yardstick of the measurement model (ba_solver_set_loss / ba_solver_set_obs_weights; include/ba_mi355x.h).

It does not restate the projection.  oracle_lib.referee_linearize(p, cam15, pts, tau) takes tau as an argument, and at tau = 1e100
psi(s) = s (2 - s / tau^2) / 4 is s / 2 to 1e-200, far below quad rounding: sqrt(2) x (its residual, its Jacobian) are the raw
r = pi(cam, pt) - meas and dr/dx, computed in __float128 and rounded once to double.  One exception is handled here: the referee keeps
the reference's clamps 1 / max(1e-15, .) on |r| and |r|^2 (BAFunctor.h:159), which falsify its outer derivative below |r|^2 = 1e-15.
dr/dx does not depend on the measurement, so an observation with |r| < 1e-3 px is evaluated a second time against a measurement
moved by one pixel in u and v, and its r is put together again in long double: r = r_aux + (meas_aux - meas).

On top of the raw quantities, in np.longdouble: r_o = w_o (pi - meas_o), s = |r_o|^2, rho and rho' of the kind, e = g r with
g = sqrt(rho / s), and the full derivative

    de/dr = g (I - rh rh') + (rho' sqrt(s) / sqrt(rho)) rh rh',     rh = r / sqrt(s)

(g = sqrt(rho'(0)) and de/dr = g I at s = 0).  tests/test_loss_checks.py pins this file on the CPU: rho = psi at tau = 0.5 reproduces
referee_linearize(..., 0.5); J is the Richardson finite difference of e; sum e^2 = sum rho.
"""
import numpy as np

LD = np.longdouble
REFERENCE, TRIVIAL, HUBER, CAUCHY = 0, 1, 2, 3
KIND_NAMES = {REFERENCE: "reference", TRIVIAL: "trivial", HUBER: "huber", CAUCHY: "cauchy"}
BIG_TAU = 1e100
SMALL_R2 = 1e-6  # |r| < 1e-3 px: evaluated against a moved measurement (module docstring)


def rho(kind, s, scale):
    """(rho(s), rho'(s)) in long double; s an array of squared weighted residuals."""
    s = np.asarray(s, LD)
    c2 = LD(scale) * LD(scale)
    if kind == REFERENCE:
        below = s < c2
        return np.where(below, s * (2 - s / c2) / 4, c2 / 4), np.where(below, (1 - s / c2) / 2, LD(0))
    if kind == TRIVIAL:
        return s.copy(), np.ones_like(s)
    if kind == HUBER:
        below = s <= c2
        sq = np.sqrt(np.where(below, c2, s))  # (no 1 / 0 in the branch not taken)
        return np.where(below, s, 2 * LD(scale) * sq - c2), np.where(below, LD(1), LD(scale) / sq)
    if kind == CAUCHY:
        return c2 * np.log1p(s / c2), 1 / (1 + s / c2)
    raise ValueError(kind)


def raw(O, p, cam15, pts):
    """Unweighted r [K,2], dr/dcam [K,2,9], dr/dpt [K,2,3] at the double state (cam15, pts), long double (from quad, rounded to double)."""
    R = O.referee_linearize(p, cam15, pts, BIG_TAU)
    rt2 = np.sqrt(LD(2))
    r = rt2 * R["f"].reshape(p.K, 2).astype(LD)
    Jc, Jp = rt2 * R["Jc"].astype(LD), rt2 * R["Jp"].astype(LD)
    small = np.where((r * r).sum(axis=1) < SMALL_R2)[0]
    if len(small):
        m = p.meas.reshape(p.K, 2).copy()
        m[small] += 1.0
        R2 = O.referee_linearize(O.Problem(p.N, p.M, p.K, p.cam_idx, p.pt_idx, m.ravel(), p.cams9, p.pts), cam15, pts, BIG_TAU)
        moved = m[small].astype(LD) - p.meas.reshape(p.K, 2)[small].astype(LD)
        r[small] = rt2 * R2["f"].reshape(p.K, 2)[small].astype(LD) + moved
        Jc[small], Jp[small] = rt2 * R2["Jc"][small].astype(LD), rt2 * R2["Jp"][small].astype(LD)
    return r, Jc, Jp


def apply_model(p, r, Jc, Jp, kind, scale, w=None):
    """The model on raw (r, Jc, Jp): dict(e [K,2], Jc [K,2,9], Jp [K,2,3], g = -J'e (3M + 9N, points first), energy = sum e^2,
    s [K], rho [K]) in long double.  w: K weights in the order of p's observations."""
    w = np.ones(p.K, LD) if w is None else np.asarray(w, LD)
    r = r * w[:, None]
    s = (r * r).sum(axis=1)
    ro, dro = rho(kind, s, scale)
    pos = s > 0
    ss = np.where(pos, s, LD(1))
    g = np.where(pos, np.sqrt(ro / ss), np.sqrt(dro))
    rh = np.where(pos[:, None], r / np.sqrt(ss)[:, None], LD(0))
    P = rh[:, :, None] * rh[:, None, :]
    radial = np.where(pos, dro * np.sqrt(ss) / np.sqrt(np.where(pos, ro, LD(1))), g)
    dedr = g[:, None, None] * (np.eye(2, dtype=LD)[None] - P) + radial[:, None, None] * P
    dedr = dedr * w[:, None, None]  # dr/dx = w dpi/dx
    e = g[:, None] * r
    Jce = np.einsum("kab,kbc->kac", dedr, Jc)
    Jpe = np.einsum("kab,kbc->kac", dedr, Jp)
    grad = np.zeros(3 * p.M + 9 * p.N, LD)
    np.add.at(grad[:3 * p.M].reshape(p.M, 3), p.pt_idx, -np.einsum("kac,ka->kc", Jpe, e))
    np.add.at(grad[3 * p.M:].reshape(p.N, 9), p.cam_idx, -np.einsum("kac,ka->kc", Jce, e))
    return dict(e=e, Jc=Jce, Jp=Jpe, g=grad, energy=(e * e).sum(), s=s, rho=ro)


def model(O, p, cam15, pts, kind, scale, w=None):
    """apply_model at the state (cam15, pts)."""
    r, Jc, Jp = raw(O, p, cam15, pts)
    return apply_model(p, r, Jc, Jp, kind, scale, w)


def energy(O, p, cam15, pts, kind, scale, w=None):
    """sum rho(s) at the state, long double."""
    r, _, _ = raw(O, p, cam15, pts)
    w = np.ones(p.K, LD) if w is None else np.asarray(w, LD)
    return rho(kind, ((r * w[:, None]) ** 2).sum(axis=1), scale)[0].sum()
