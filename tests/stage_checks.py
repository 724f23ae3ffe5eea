"""Stage-by-stage metrics of one LM trial -- TEST INFRASTRUCTURE ONLY (tests/test_stage_checks.py, tests/test_gpu_stages.py).

Each stage's output is measured against the same stage computed in quad precision (oracle/ba_referee.c) on the stage's OWN inputs --
for a GPU trial, the GPU's state, J, S and step -- so no difference made upstream enters a stage's bound.  Every metric is a scaled
error: 0 for exact arithmetic, about the unit roundoff for a backward-stable stage, whatever the conditioning of the problem.

  linearisation   residual per observation relative to |r_i| + sum |Jp_i| |X| (its sensitivity to the point), each Jacobian entry
                  relative to its own sensitivity to the inputs (quad_linearization); quad at the same state
  gradient        g = -J'r of the SAME J and r, g_i relative to sum_k |J_ki| |r_k|
  assembly        S_ij relative to sqrt((U_ii + lam)(U_jj + lam)), U = sum J_c' J_c before the elimination; rhs_i relative to
                  sum_k |J_ki| |r_k| + |rhs_i|
  factor + sweep  eta(S, x, b) = max_i |S x - b|_i / (sqrt(S_ii) sum_j sqrt(S_jj) |x_j| + |b_i|): the backward error of a solve of
                  S x = b (the sign convention of the solver: S dx_c = rhs, GET_RHS)
  back-subst.     per point, |(V_j + lam I) dx_p + W_j' dx_c - g_p| relative to the same sum of absolute values
  retraction      x (+) dx entry by entry (quad) in units of eps x the entry's scale
  trial scalars   the test energy against quad at the same trial point; rho denominator and |dx| of the same dx and g (relative to
                  sums of absolute values for the rho denominator)
  dense QR        (ba_qr.hip.h, on the matrix A | b it was handed and what it left: R, Q^T b in column D, y) gram: max |R'R - A'A|_ij /
                  (|a_i| |a_j|), the factor's backward error (or, for large m D^2, | |Rz|^2 - |Az|^2 | / | |A||z| |^2 over column-scaled probes z);
                  qtb_head: max |R'c - A'b|_i / (|a_i| |b|); orth: | |Q^T b|^2 - |b|^2 | / |b|^2 (a reflector that is not
                  orthogonal); tri: max |R y - c|_i / (|R| |y| + |c|)_i, the back substitution alone
The sums over observations of the gradient, back-substitution and trial-scalar metrics are in long double (64-bit significand: 2048x
finer than fp64), the dense-QR sums in blocks of long double added in quad, the rest in quad.
"""
import numpy as np

import oracle_lib as O

TINY = 1e-300


def _ratio(num, den):
    num = np.asarray(num, np.float64)
    den = np.asarray(den, np.float64)
    out = np.zeros_like(num)
    nz = den > 0
    out[nz] = num[nz] / den[nz]
    out[~nz & (num > 0)] = np.inf
    out[np.isnan(num) | np.isnan(den)] = np.nan  # (a NaN anywhere must fail every bound, not read as 0)
    return out


def eta(S, x, b):
    """Backward error of the symmetric solve S x = b (lower triangle of S read), residual in quad."""
    num, den = O.referee_sym_residual(S, x, b)
    return float(_ratio(num, den).max())


def abs_grad(p, Jc, Jp, f):
    """sum_k |J_ki| |r_k| per unknown ([3M points | 9N cameras]): the scale of g = -J'r."""
    Jc = np.abs(np.asarray(Jc, np.float64).reshape(p.K, 2, 9))
    Jp = np.abs(np.asarray(Jp, np.float64).reshape(p.K, 2, 3))
    r = np.abs(np.asarray(f, np.float64).reshape(p.K, 2))
    out = np.zeros(3 * p.M + 9 * p.N)
    np.add.at(out[: 3 * p.M].reshape(p.M, 3), p.pt_idx, np.einsum("krc,kr->kc", Jp, r))
    np.add.at(out[3 * p.M:].reshape(p.N, 9), p.cam_idx, np.einsum("krc,kr->kc", Jc, r))
    return out


def camera_diag(p, Jc):
    """diag(sum J_c' J_c) per camera unknown (D): U of the scaling of S, before the elimination and lambda."""
    Jc = np.asarray(Jc, np.float64).reshape(p.K, 2, 9)
    out = np.zeros(p.D)
    np.add.at(out.reshape(p.N, 9), p.cam_idx, (Jc * Jc).sum(axis=1))
    return out


def quad_linearization(p, cam15, pts, rel=1e-6):
    """The quad linearisation at (cam15, pts) (referee_linearize) and, per Jacobian entry, its sensitivity to relative perturbations of
    the inputs it is computed from: jac_scale[k, r, c] = |J| + sum_x |dJ/dx| |x| over the point's three coordinates, the camera's
    translation and focal length and the two measurement coordinates -- the error that rounding those inputs (or quantities of their
    size inside the formulas, such as R X + T) to the unit roundoff leaves in the entry, per unit roundoff.  Each partial comes from a
    forward difference in quad, with every point (camera, measurement) perturbed at once: an observation's block depends on its own
    point, camera and measurement only.  c: 0-8 the camera columns, 9-11 the point's."""
    L = O.referee_linearize(p, cam15, pts)
    J = np.concatenate([L["Jc"], L["Jp"]], axis=2)
    scale = np.abs(J)
    cam15 = np.asarray(cam15, np.float64).reshape(p.N, 15)
    pts = np.asarray(pts, np.float64).reshape(p.M, 3)

    def add(x_obs, x_obs_new, Lp):
        d = (x_obs_new - x_obs) / np.where(x_obs != 0, x_obs, 1.0)  # the perturbation actually made, relative
        Jn = np.concatenate([Lp["Jc"], Lp["Jp"]], axis=2)
        with np.errstate(invalid="ignore", divide="ignore"):
            part = np.where(d[:, None, None] != 0, np.abs(Jn - J) / np.abs(d)[:, None, None], 0.0)
        scale[...] += part

    for c in range(3):
        q = pts.copy()
        q[:, c] *= 1 + rel
        add(pts[p.pt_idx, c], q[p.pt_idx, c], O.referee_linearize(p, cam15, q))
    for c in (9, 10, 11, 12):
        q = cam15.copy()
        q[:, c] *= 1 + rel
        add(cam15[p.cam_idx, c], q[p.cam_idx, c], O.referee_linearize(p, q, pts))
    meas = p.meas.reshape(p.K, 2)
    for c in range(2):
        m = meas.copy()
        m[:, c] *= 1 + rel
        pm = O.Problem(p.N, p.M, p.K, p.cam_idx, p.pt_idx, m.ravel(), p.cams9, p.pts)
        add(meas[:, c], m[:, c], O.referee_linearize(pm, cam15, pts))
    L["jac_scale"] = scale
    return L


def linearization_errors(p, cam15, pts, f, Jc, Jp, energy=None, ref=None):
    """The linearisation (f, Jc, Jp, energy -- what GET_RESIDUALS / _JC / _JP and linearize() return) against quad at the SAME state
    (cam15, pts); ref: quad_linearization of that state (computed when not given).  Observations in the order of p (point-sorted).
    Jacobian: max over the entries of |dJ| / jac_scale."""
    L = quad_linearization(p, cam15, pts) if ref is None else ref
    K = p.K
    f = np.asarray(f, np.float64).reshape(K, 2)
    J = np.concatenate([np.asarray(Jc, np.float64).reshape(K, 2, 9), np.asarray(Jp, np.float64).reshape(K, 2, 3)], axis=2)
    X = np.abs(np.asarray(pts, np.float64).reshape(p.M, 3))[p.pt_idx]
    fr = L["f"].reshape(K, 2)
    sc_r = np.abs(fr).max(axis=1) + np.einsum("krc,kc->kr", np.abs(L["Jp"]), X).max(axis=1)
    out = dict(res=float(_ratio(np.abs(f - fr).max(axis=1), sc_r).max()))
    Jr = np.concatenate([L["Jc"], L["Jp"]], axis=2)
    out["jac"] = float(_ratio(np.abs(J - Jr), L["jac_scale"]).max())
    if energy is not None:
        out["energy"] = abs(energy - L["energy"]) / L["energy"]
    return out


def grad_errors(p, Jc, Jp, f, g):
    """g = -J'r (GET_GRAD) against the same sum over the SAME J and r in long double, relative to sum_k |J_ki| |r_k|."""
    LD = np.longdouble
    Jc = np.asarray(Jc, np.float64).reshape(p.K, 2, 9).astype(LD)
    Jp = np.asarray(Jp, np.float64).reshape(p.K, 2, 3).astype(LD)
    r = np.asarray(f, np.float64).reshape(p.K, 2).astype(LD)
    ref = np.zeros(3 * p.M + 9 * p.N, LD)
    np.add.at(ref[: 3 * p.M].reshape(p.M, 3), p.pt_idx, -np.einsum("krc,kr->kc", Jp, r))
    np.add.at(ref[3 * p.M:].reshape(p.N, 9), p.cam_idx, -np.einsum("krc,kr->kc", Jc, r))
    err = np.abs(np.asarray(g, np.float64).astype(LD) - ref).astype(np.float64)
    return float(_ratio(err, abs_grad(p, Jc.astype(np.float64), Jp.astype(np.float64), r.astype(np.float64))).max())


def assembly_errors(p, Jc, f, lam, S, rhs, S_ref, rhs_ref, Jp=None):
    """S and rhs against (S_ref, rhs_ref) -- assembled in quad from the same J (referee_reduced_from_jacobian) -- entry by entry
    scaled by sqrt((U_ii + lam)(U_jj + lam)), and by sum_k |J_ki| |r_k| + |rhs_i| (Jp: for that sum; without it, the camera part
    needs only Jc)."""
    d = np.sqrt(camera_diag(p, Jc) + lam)
    out = {}
    if S is not None:
        dS = np.abs(np.asarray(S) - np.asarray(S_ref))
        dS /= d[:, None]
        dS /= d[None, :]
        out["S"] = float(dS.max())
    Jp = np.zeros((p.K, 2, 3)) if Jp is None else Jp
    sc = abs_grad(p, Jc, Jp, f)[3 * p.M:] + np.abs(rhs_ref)
    out["rhs"] = float(_ratio(np.abs(np.asarray(rhs) - rhs_ref), sc).max())
    return out


def backsub_errors(p, Jc, Jp, dx, g, lam):
    """Per point j: |(V_j + lam I) dx_p + W_j' dx_c - g_p| / (|Jp|'(|Jp| |dx_p| + |Jc| |dx_c|) + lam |dx_p| + |g_p|), max over the
    point's three rows and over the points, in long double (V_j = sum Jp'Jp, W_j = sum Jc'Jp over the point's observations)."""
    LD = np.longdouble
    M, N, K = p.M, p.N, p.K
    Jc = np.asarray(Jc, np.float64).reshape(K, 2, 9).astype(LD)
    Jp = np.asarray(Jp, np.float64).reshape(K, 2, 3).astype(LD)
    dx = np.asarray(dx, np.float64)
    dxp = dx[: 3 * M].reshape(M, 3).astype(LD)
    dxc = dx[3 * M:].reshape(N, 9).astype(LD)
    gp = np.asarray(g, np.float64)[: 3 * M].reshape(M, 3).astype(LD)
    u = np.einsum("krc,kc->kr", Jp, dxp[p.pt_idx]) + np.einsum("krc,kc->kr", Jc, dxc[p.cam_idx])
    ua = np.einsum("krc,kc->kr", np.abs(Jp), np.abs(dxp[p.pt_idx])) + np.einsum("krc,kc->kr", np.abs(Jc), np.abs(dxc[p.cam_idx]))
    res = np.zeros((M, 3), LD)
    den = np.zeros((M, 3), LD)
    np.add.at(res, p.pt_idx, np.einsum("krc,kr->kc", Jp, u))
    np.add.at(den, p.pt_idx, np.einsum("krc,kr->kc", np.abs(Jp), ua))
    res += LD(lam) * dxp - gp
    den += LD(lam) * np.abs(dxp) + np.abs(gp)
    return float(_ratio(np.abs(res).astype(np.float64), den.astype(np.float64)).max())


def retraction_ulps(p, cam15, pts, dx, cam_test, pts_test, eps):
    """x (+) dx (GET_CAMS_TEST / GET_POINTS_TEST) against the quad retraction of the same x and dx, in units of eps x scale: 1 for
    the rotation entries, |x| + |dx| for the translation, focal length, distortion and the points."""
    co, po = O.referee_retract(p, cam15, pts, dx)
    cam15 = np.asarray(cam15, np.float64).reshape(p.N, 15)
    dxc = np.abs(np.asarray(dx, np.float64)[3 * p.M:].reshape(p.N, 9))
    sc = np.ones((p.N, 15))
    sc[:, 9:12] = np.abs(cam15[:, 9:12]) + dxc[:, 0:3]
    sc[:, 12:15] = np.abs(cam15[:, 12:15]) + dxc[:, 6:9]
    sp = np.abs(np.asarray(pts, np.float64)) + np.abs(np.asarray(dx, np.float64)[: 3 * p.M])
    ec = _ratio(np.abs(np.asarray(cam_test, np.float64).reshape(p.N, 15) - co.reshape(p.N, 15)), sc).max()
    ep = _ratio(np.abs(np.asarray(pts_test, np.float64) - po), sp).max() if p.M else 0.0
    return float(max(ec, ep) / eps)


def trial_scalar_errors(p, lam, dx, g, e_test, rho_scale, dx_norm, cam_test, pts_test):
    """The trial's scalars against quad at the GPU's own inputs: e_test vs the quad energy at the GPU's trial point, rho_scale vs
    sum dx (lam dx + g) (relative to sum |dx| (lam |dx| + |g|)), |dx| vs the quad norm of the GPU's dx."""
    dx = np.asarray(dx, np.float64)
    g = np.asarray(g, np.float64)
    e_ref = O.referee_energy(p, cam_test, pts_test)
    LD = np.longdouble
    dxl, gl = dx.astype(LD), g.astype(LD)
    rs = (dxl * (LD(lam) * dxl + gl)).sum()
    rs_abs = (np.abs(dxl) * (LD(lam) * np.abs(dxl) + np.abs(gl))).sum()
    dn = np.sqrt((dxl * dxl).sum())
    return dict(e_test=abs(e_test - e_ref) / e_ref, rho_scale=float(abs(LD(rho_scale) - rs) / rs_abs),
                dx_norm=float(abs(LD(dx_norm) - dn) / dn))


def qr_metrics(Ab, F, m, D, y=None, probes=0, seed=0):
    """The dense QR's metrics (module docstring) from Ab, the matrix the QR was handed, and F, the matrix it left -- both
    [D + 1 columns, >= m rows], the right-hand side in column D -- and y (tri: None = not measured).  probes > 0: gram in the probe
    form over that many Gaussian z (seeded), each entry divided by its column's norm: every column weighs the same in the probe
    whatever the column scales."""
    Z = None
    if probes:
        nrm = np.linalg.norm(np.asarray(Ab)[:D, :m], axis=1)
        Z = np.random.default_rng(seed).standard_normal((probes, D)) / np.where(nrm > 0, nrm, 1.0)
    num, den = O.referee_qr_gram(Ab, F, m, D, Z)
    out = dict(gram=float(_ratio(num, den).max()))
    (hn, hd), (on, od) = O.referee_qr_rhs(Ab, F, m, D)
    out["qtb_head"] = float(_ratio(hn, hd).max())
    out["orth"] = float(_ratio([on], [od]).max())
    if y is not None:
        tn, td = O.referee_tri_residual(F, D, y)
        out["tri"] = float(_ratio(tn, td).max())
    return out
