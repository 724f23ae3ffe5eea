"""A restatement of the triangulation rule of include/ba_mi355x.h (csrc/ba_triangulate.hip.h) in numpy, in any float type: long double
is the reference, fp64 measures that reference's own rounding.  Vectorised over points: the tracks are padded to the longest one and
masked, every sum over a track is numpy's over the padded axis.  Nothing here is shared with the library.

triangulate(dt, pt_ptr, cam15, meas, w, x_old, loss, scale, ...) takes the observations sorted by point (pt_ptr: first observation of
every point, + end; cam15: one BA_GET_CAMS row PER OBSERVATION) and returns per point: x, status, cost_old, cost_new, angle_deg, and
for the bounds: kappa (condition of the midpoint's 3 x 3 matrix), size (|X| + max |C_o|) and margin, the smallest relative distance of
a quantity from the threshold it was compared with on the way to the status."""
import numpy as np

REPLACED, FEW_VIEWS, LOW_ANGLE, DEGENERATE, BEHIND, REPROJ, NOT_BETTER, FIXED = range(8)
NEWTON_ITERS, UNDISTORT_TOL, MU_REL, MIN_DECREASE = 12, 1e-12, 1e-9, 1e-11
TRACE = None  # a list: the refinement's relative decreases and step lengths are appended (diagnostics)
LD = np.longdouble


def rho_of(dt, kind, sc, s):
    sc2 = dt(sc) * dt(sc)
    if kind == 1:
        return s.copy(), np.ones_like(s)
    if kind == 0:
        below = s < sc2
        return np.where(below, s * (2 - s / sc2) / 4, sc2 / 4), np.where(below, (1 - s / sc2) / 2, dt(0))
    if kind == 2:
        n = np.sqrt(np.where(s > sc2, s, sc2))
        return np.where(s > sc2, 2 * dt(sc) * n - sc2, s), np.where(s > sc2, dt(sc) / n, dt(1))
    if kind == 3:
        return sc2 * np.log1p(s / sc2), 1 / (1 + s / sc2)
    raise ValueError(kind)


def rays(dt, cam, meas):
    """cam [..., 15], meas [..., 2] -> (usable [...], d [..., 3], margin [...]): step 1 of the rule."""
    f, k1, k2 = cam[..., 12], cam[..., 13], cam[..., 14]
    with np.errstate(all="ignore"):
        m = meas / f[..., None]
        rm = np.sqrt(m[..., 0] ** 2 + m[..., 1] ** 2)
        ok = np.isfinite(rm)
        rho = rm.copy()
        dhmin = np.full(rm.shape, np.inf, dt)
        for _ in range(NEWTON_ITERS + 1):
            r2 = rho * rho
            dh = 1 + r2 * (3 * k1 + 5 * k2 * r2)
            h = rho * (1 + r2 * (k1 + k2 * r2)) - rm
            good = (dh > 0) & np.isfinite(dh) & np.isfinite(h)
            ok = ok & (good | (rm == 0))
            dhmin = np.minimum(dhmin, np.where(np.isfinite(dh), dh, -np.inf))
            if _ < NEWTON_ITERS:
                rho = np.where(ok & (rm > 0), rho - h / np.where(dh != 0, dh, 1), rho)
        nz = rm > 0
        tol = dt(UNDISTORT_TOL) * rm
        ok = ok & (~nz | (np.isfinite(rho) & (rho > 0) & (np.abs(h) <= tol)))
        # how far the usability decision is from flipping: the smallest h' against 1, the residual against its bound
        margin = np.where(nz, np.minimum(np.abs(dhmin), np.abs(np.abs(h) - tol) / np.where(tol > 0, tol, 1)), dt(np.inf))
        margin = np.where(np.isfinite(margin), margin, dt(np.inf))
        sc = np.where(nz, rho / np.where(nz, rm, 1), dt(0))
        xu = m * sc[..., None]
        R = cam[..., :9].reshape(cam.shape[:-1] + (3, 3))
        v3 = np.concatenate([xu, np.ones(xu.shape[:-1] + (1,), dt)], -1)
        v = -np.einsum("...rk,...r->...k", R, v3)
        n = np.sqrt((v * v).sum(-1))
        ok = ok & (n > 0) & np.isfinite(n)
        d = np.where(ok[..., None], v / np.where(ok, n, 1)[..., None], dt(0))
    return ok, d, margin


def _pass(dt, cam, meas, w, mask, usable, loss, scale, X):
    """cam [P, t, 15], X [P, 3]: c, H [P, 3, 3], g [P, 3], behind [P], maxrep [P], front margin [P], saturation margin [P] (psi only: how
    far the least saturated observation is beyond tau^2, relative; 0 unless every observation is beyond it)."""
    with np.errstate(all="ignore"):
        R = cam[..., :9].reshape(cam.shape[:-1] + (3, 3))
        XX = np.einsum("ptrk,pk->ptr", R, X) + cam[..., 9:12]
        behind = (~(XX[..., 2] < 0) & mask).any(1)
        fm = np.where(mask, np.abs(XX[..., 2]) / np.sqrt((XX * XX).sum(-1)), dt(np.inf)).min(1, initial=dt(np.inf))
        xu = XX[..., :2] / XX[..., 2:3]
        r2u = (xu * xu).sum(-1)
        f, k1, k2 = cam[..., 12], cam[..., 13], cam[..., 14]
        kr = 1 + k1 * r2u + k2 * r2u * r2u
        e = (f * kr)[..., None] * xu - meas
        rp = np.sqrt((e * e).sum(-1))
        rp = np.where(np.isnan(rp), dt(np.inf), rp)
        maxrep = np.where(mask & usable, rp, dt(0)).max(1, initial=dt(0))
        r = w[..., None] * e
        s = (r * r).sum(-1)
        rho, om = rho_of(dt, loss, scale, s)
        c = np.where(mask, rho, dt(0)).sum(1)
        sc2 = dt(scale) * dt(scale)
        sat = np.where(mask, s / sc2 - 1, dt(np.inf)).min(1, initial=dt(np.inf)) if loss == 0 else np.zeros(len(X), dt)
        sat = np.where(np.isfinite(sat) & (sat > 0), sat, dt(0))
        a00 = 1 / XX[..., 2]
        a02 = -XX[..., 0] / XX[..., 2] ** 2
        a12 = -XX[..., 1] / XX[..., 2] ** 2
        dkr = 2 * k1 + 4 * k2 * r2u
        wf = w * f
        p00, p01, p11 = wf * (kr + xu[..., 0] ** 2 * dkr), wf * (xu[..., 0] * xu[..., 1] * dkr), wf * (kr + xu[..., 1] ** 2 * dkr)
        q = np.stack([np.stack([p00 * a00, p01 * a00, p00 * a02 + p01 * a12], -1),
                      np.stack([p01 * a00, p11 * a00, p01 * a02 + p11 * a12], -1)], -2)  # [P, t, 2, 3]
        J = np.einsum("ptij,ptjk->ptik", q, R)
        om = np.where(mask, om, dt(0))
        J = np.where(mask[..., None, None], J, dt(0))
        r = np.where(mask[..., None], r, dt(0))
        H = np.einsum("pt,ptik,ptil->pkl", om, J, J)
        g = np.einsum("pt,ptik,pti->pk", om, J, r)
    return c, H, g, behind, maxrep, fm, sat


def _chol_solve(dt, A, b):
    """A [P, 3, 3] symmetric, b [P, 3]: (ok [P], x [P, 3], smallest pivot relative to its diagonal entry [P])."""
    with np.errstate(all="ignore"):
        P = len(A)
        ok = np.ones(P, bool)
        rel = np.full(P, np.inf, dt)
        Lm = np.zeros((P, 3, 3), dt)
        for i in range(3):
            for j in range(i + 1):
                sm = A[:, i, j] - (Lm[:, i, :j] * Lm[:, j, :j]).sum(-1)
                if i == j:
                    good = (sm > 0) & np.isfinite(sm)
                    ok = ok & good
                    rel = np.minimum(rel, np.where(np.isfinite(sm), np.abs(sm) / np.where(A[:, i, i] != 0, np.abs(A[:, i, i]), 1), dt(0)))
                    Lm[:, i, i] = np.sqrt(np.where(good, sm, 1))
                else:
                    Lm[:, i, j] = sm / Lm[:, j, j]
        y = np.zeros((P, 3), dt)
        for i in range(3):
            y[:, i] = (b[:, i] - (Lm[:, i, :i] * y[:, :i]).sum(-1)) / Lm[:, i, i]
        x = np.zeros((P, 3), dt)
        for i in (2, 1, 0):
            x[:, i] = (y[:, i] - (Lm[:, i + 1:, i] * x[:, i + 1:]).sum(-1)) / Lm[:, i, i]
        ok = ok & np.isfinite(x).all(-1)
    return ok, x, rel


def _chunk(dt, cam, meas, w, mask, x_old, loss, scale, min_angle_deg, max_reproj_px, refine_iters, only_if_better):
    P, t = mask.shape
    inf = dt(np.inf)
    status = np.full(P, -1, np.int64)
    margin = np.full(P, inf, dt)
    usable, d, um = rays(dt, cam, meas)
    usable = usable & mask
    d = np.where(usable[..., None], d, dt(0))
    margin = np.minimum(margin, np.where(mask, um, inf).min(1, initial=inf))
    c_old, _, _, _, _, _, sat_old = _pass(dt, cam, meas, w, mask, usable, loss, scale, x_old)
    x = x_old.copy()
    c_new = c_old.copy()
    nus = usable.sum(1)
    status[nus < 2] = FEW_VIEWS
    # 2. the largest chord
    diff = d[:, :, None, :] - d[:, None, :, :]
    c2 = (diff * diff).sum(-1)
    c2 = np.where(usable[:, :, None] & usable[:, None, :], c2, dt(0)).max((1, 2), initial=dt(0))
    with np.errstate(all="ignore"):
        ang = 2 * np.arctan2(np.sqrt(c2), np.sqrt(np.maximum(4 - c2, dt(0))))
    ang = np.where(nus < 2, dt(0), ang)
    amin = dt(min_angle_deg) * dt(np.pi) / 180
    live = status < 0
    if min_angle_deg > 0:
        margin = np.where(live, np.minimum(margin, np.abs(ang - amin) / amin), margin)
    status[live & (ang < amin)] = LOW_ANGLE
    # 3. midpoint
    with np.errstate(all="ignore"):
        R = cam[..., :9].reshape(P, t, 3, 3)
        C = -np.einsum("ptrk,ptr->ptk", R, cam[..., 9:12])
        w2 = np.where(usable, w * w, dt(0))
        Pm = np.eye(3, dtype=dt) - d[..., :, None] * d[..., None, :]
        A = np.einsum("pt,ptkl->pkl", w2, Pm)
        b = np.einsum("pt,ptkl,ptl->pk", w2, Pm, np.where(usable[..., None], C, dt(0)))
        okA, Xm, relA = _chol_solve(dt, A, b)
        ev = np.linalg.eigvalsh(np.where(np.isfinite(A), A, 0).astype(np.float64))
        kappa = np.where(ev[:, 0] > 0, ev[:, 2] / np.where(ev[:, 0] > 0, ev[:, 0], 1), np.inf)
        size = np.sqrt((Xm * Xm).sum(-1)) + np.sqrt(np.where(usable, (C * C).sum(-1), dt(0)).max(1, initial=dt(0)))
    live = status < 0
    margin = np.where(live, np.minimum(margin, relA), margin)
    status[live & ~okA] = DEGENERATE
    # 4. refinement (on the points still live; the others carry dummies along)
    live = status < 0
    Xt = np.where(live[:, None], Xm, x_old)
    X = Xt.copy()
    cur = None
    going = live.copy()
    rmargin = np.full(P, inf, dt)
    xfloor = dt(np.finfo(np.float64).eps) * np.where(np.isfinite(kappa), kappa, 0) * size
    for it in range(refine_iters + 1):
        at = _pass(dt, cam, meas, w, mask, usable, loss, scale, Xt)
        with np.errstate(all="ignore"):
            take = going & ((at[0] < cur[0] * (1 - dt(MIN_DECREASE))) if it > 0 else True)
            if it > 0:
                # how far the acceptance is from flipping: the decrease against its threshold -- counted where the step is longer than
                # the floor of the X bound (a step below it moves X by less than the bound allows, whoever takes it)
                thr = dt(MIN_DECREASE) * cur[0]
                far = np.abs((cur[0] - at[0]) - thr) / np.where(thr > 0, thr, 1)
                step = np.sqrt(((Xt - X) ** 2).sum(-1))
                rmargin = np.where(going & (step > xfloor) & np.isfinite(far), np.minimum(rmargin, far), rmargin)
                if TRACE is not None:
                    TRACE.append((it, ((cur[0] - at[0]) / cur[0]).astype(np.float64), step.astype(np.float64), going.copy()))
        going = going & take
        if cur is None:
            cur = [a.copy() for a in at]
        else:
            for k in range(len(at)):
                cur[k] = np.where(take.reshape((-1,) + (1,) * (at[k].ndim - 1)), at[k], cur[k])
        X = np.where(take[:, None], Xt, X)
        if it == refine_iters:
            break
        with np.errstate(all="ignore"):
            mu = dt(MU_REL) * (cur[1][:, 0, 0] + cur[1][:, 1, 1] + cur[1][:, 2, 2]) / 3
            okH, dx, _ = _chol_solve(dt, cur[1] + mu[:, None, None] * np.eye(3, dtype=dt), cur[2])
        going = going & okH
        Xt = np.where(going[:, None], X - np.where(okH[:, None], dx, 0), X)
    c_cand, _, _, behind, maxrep, fm, sat_new = cur
    x = np.where(live[:, None], X, x)
    c_new = np.where(live, c_cand, c_new)
    # 5. the tests
    margin = np.where(live, np.minimum(margin, fm), margin)
    status[live & (behind | ~np.isfinite(X).all(-1))] = BEHIND
    live = status < 0
    if max_reproj_px > 0:
        margin = np.where(live, np.minimum(margin, np.abs(maxrep - dt(max_reproj_px)) / dt(max_reproj_px)), margin)
        status[live & ~(maxrep <= dt(max_reproj_px))] = REPROJ
    live = status < 0
    if only_if_better:
        with np.errstate(all="ignore"):
            # (psi with every observation beyond tau^2 at x_old AND at the candidate: both costs are t tau^2 / 4 exactly, and stay so
            # under any perturbation smaller than the saturation margin -- the tie is a stable decision, not a close one)
            better = np.maximum(np.abs(c_new - c_old) / np.where(c_old > 0, c_old, 1), np.minimum(sat_old, sat_new))
            margin = np.where(live, np.minimum(margin, better), margin)
            status[live & ~(c_new < c_old)] = NOT_BETTER
    status[status < 0] = REPLACED
    return dict(x=x, status=status, cost_old=c_old, cost_new=c_new, angle_deg=ang * 180 / dt(np.pi), kappa=kappa, size=size, margin=margin,
                rmargin=rmargin)


def triangulate(dt, pt_ptr, cam15, meas, w, x_old, loss=0, scale=0.5, min_angle_deg=1.5, max_reproj_px=0.0, refine_iters=5,
                only_if_better=True, budget=3_000_000):
    pt_ptr = np.asarray(pt_ptr, np.int64)
    P = len(pt_ptr) - 1
    cam15 = np.asarray(cam15, dt).reshape(-1, 15)
    meas = np.asarray(meas, dt).reshape(-1, 2)
    w = np.ones(len(cam15), dt) if w is None else np.asarray(w, dt).reshape(-1)
    x_old = np.asarray(x_old, dt).reshape(P, 3)
    tl = np.diff(pt_ptr)
    out = {}
    order = np.argsort(tl, kind="stable")
    pos = 0
    pieces = []
    while pos < P:  # chunks of points of similar track length, so that the padding and the [P, t, t] chords stay small
        t = max(int(tl[order[pos]]), 1)
        end = pos + 1
        while end < P:
            t2 = max(int(tl[order[end]]), 1)
            if (end + 1 - pos) * t2 * t2 > budget or t2 > 2 * t + 4:
                break
            end += 1
        idx = order[pos:end]
        tm = max(int(tl[idx].max()), 1)
        sel = pt_ptr[idx][:, None] + np.arange(tm)[None, :]
        mask = np.arange(tm)[None, :] < tl[idx][:, None]
        sel = np.where(mask, sel, 0) if len(cam15) else np.zeros_like(sel)
        if len(cam15):
            cc, mm, ww = cam15[sel], meas[sel], w[sel]
        else:
            cc, mm, ww = np.zeros(sel.shape + (15,), dt), np.zeros(sel.shape + (2,), dt), np.ones(sel.shape, dt)
        # a padded slot is a harmless camera (identity, f = 1) that the mask keeps out of every sum
        pad = np.zeros(15, dt)
        pad[[0, 4, 8, 12]] = 1
        pad[11] = -1
        cc = np.where(mask[..., None], cc, pad)
        mm = np.where(mask[..., None], mm, dt(0))
        ww = np.where(mask, ww, dt(1))
        pieces.append((idx, _chunk(dt, cc, mm, ww, mask, x_old[idx], loss, scale, min_angle_deg, max_reproj_px, refine_iters, only_if_better)))
        pos = end
    for key in ("x", "status", "cost_old", "cost_new", "angle_deg", "kappa", "size", "margin", "rmargin"):
        first = pieces[0][1][key]
        full = np.zeros((P,) + first.shape[1:], first.dtype)
        for idx, r in pieces:
            full[idx] = r[key]
        out[key] = full
    return out


# ---- designed tracks ---------------------------------------------------------------------------------------------------------------
def rodrigues(om):
    th = np.linalg.norm(om)
    if th == 0:
        return np.eye(3)
    k = om / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx


def project(cam15, X):
    """The camera model in long double: cam15 [t, 15], X [3] -> ([t, 2] measurements, [t] depth XX_2)."""
    c = np.asarray(cam15, LD).reshape(-1, 15)
    R = c[:, :9].reshape(-1, 3, 3)
    XX = R @ np.asarray(X, LD) + c[:, 9:12]
    xu = XX[:, :2] / XX[:, 2:3]
    r2 = (xu * xu).sum(-1)
    kr = 1 + c[:, 13] * r2 + c[:, 14] * r2 * r2
    return ((c[:, 12] * kr)[:, None] * xu).astype(np.float64), XX[:, 2].astype(np.float64)


def ring_cameras(rng, t, X, radius=6.0, spread=1.0, f=800.0, k1=-0.05, k2=0.01, jitter=0.3):
    """t cameras on an arc of `spread` radians around X at distance ~radius, each looking at X down its -z axis (plus a small random
    rotation, so that X is off-centre and the distortion matters): [t, 15]."""
    cams = np.zeros((t, 15))
    for i in range(t):
        a = spread * ((i / max(t - 1, 1)) - 0.5)
        C = X + radius * (1 + 0.2 * rng.uniform(-1, 1)) * np.array([np.sin(a), 0.3 * rng.uniform(-1, 1), np.cos(a)])
        z = (C - X) / np.linalg.norm(C - X)  # the camera's +z points AWAY from X
        x = np.cross([0.0, 1.0, 0.0], z)
        x /= np.linalg.norm(x)
        y = np.cross(z, x)
        R = rodrigues(jitter * 0.1 * rng.uniform(-1, 1, 3)) @ np.stack([x, y, z])
        cams[i, :9] = R.reshape(-1)
        cams[i, 9:12] = -R @ C
        cams[i, 12:] = f, k1, k2
    return cams


X_TRUE = np.array([0.4, -0.2, 1.5])
X_OFF = np.array([0.05, -0.03, 0.04])
T_SIZES = (2, 3, 8, 9, 64, 65, 300)


def _case(name, cams, x_true=X_TRUE, meas=None, w=None, x_old=None, expect=REPLACED, exact=False, loss=0, scale=0.5, **params):
    meas0, depth = project(cams, x_true) if len(cams) else (np.zeros((0, 2)), np.zeros(0))
    par = dict(min_angle_deg=1.5, max_reproj_px=0.0, refine_iters=5, only_if_better=True)
    par.update(params)
    return dict(name=name, cams=np.asarray(cams, np.float64).reshape(-1, 15), x_true=np.asarray(x_true, np.float64),
                meas=meas0 if meas is None else meas, w=w, x_old=x_true + X_OFF if x_old is None else x_old, expect=expect, exact=exact,
                loss=loss, scale=scale, params=par, depth=depth)


def two_rays(angle_deg, X=X_TRUE, radius=5.0, f=800.0):
    """Two cameras in the plane y = X_y whose lines of sight to X are angle_deg apart (X a little off their axes)."""
    cams = np.zeros((2, 15))
    for i, a in enumerate((-0.5, 0.5)):
        a = np.deg2rad(angle_deg) * a
        C = X + radius * np.array([np.sin(a), 0.0, np.cos(a)])
        z = (C - X) / radius
        x = np.cross([0.0, 1.0, 0.0], z)
        x /= np.linalg.norm(x)
        R = rodrigues(np.array([0.01, -0.02, 0.03])) @ np.stack([x, np.cross(z, x), z])
        cams[i, :9], cams[i, 9:12], cams[i, 12] = R.reshape(-1), -R @ C, f
    return cams


def designed_cases(seed=20):
    """The designed tracks of the tests: every case misses every threshold of the rule by a factor >= 2.  `exact`: noiseless, the rule must
    return x_true.  Measurements are made by project() (long double) from x_true; pack() makes them again from
    cameras rounded to another type."""
    rng = np.random.default_rng(seed)
    cs = []
    for t in T_SIZES:
        cs.append(_case("t%d" % t, ring_cameras(rng, t, X_TRUE), exact=True))
    cs.append(_case("distort", ring_cameras(rng, 5, X_TRUE, f=300.0, k1=-0.25, k2=0.08, jitter=3.0), exact=True))
    # an observation whose distortion has no inverse: rho - 0.3 rho^3 never reaches |m| = 2
    cams = ring_cameras(rng, 4, X_TRUE, k1=0.0, k2=0.0)
    cams[0, 13:] = -0.3, 0.0
    meas, _ = project(cams, X_TRUE)
    meas[0] = 2 * cams[0, 12], 0.0
    cs.append(_case("noinverse", cams, meas=meas, exact=True))
    cs.append(_case("t1", ring_cameras(rng, 1, X_TRUE), expect=FEW_VIEWS))
    cs.append(_case("t0", np.zeros((0, 15)), expect=FEW_VIEWS))
    cs.append(_case("angle_half", two_rays(0.75), expect=LOW_ANGLE))
    cs.append(_case("angle_twice", two_rays(3.0), exact=True))
    # one camera turned round (about its y axis): x_true is behind it, on the same line of sight
    cams = ring_cameras(rng, 3, X_TRUE, k1=0.0, k2=0.0)
    flip = np.diag([-1.0, 1.0, -1.0])
    R = flip @ cams[1, :9].reshape(3, 3)
    cams[1, :9], cams[1, 9:12] = R.reshape(-1), flip @ cams[1, 9:12]
    cs.append(_case("behind", cams, expect=BEHIND))
    # one gross outlier (200 px): the midpoint is dragged away from a correct x_old; refine_iters = 0 keeps it there
    cams = ring_cameras(rng, 6, X_TRUE)
    meas, _ = project(cams, X_TRUE)
    meas[2, 0] += 200.0
    cs.append(_case("outlier_notbetter", cams, meas=meas, x_old=X_TRUE.copy(), expect=NOT_BETTER, refine_iters=0))
    cs.append(_case("outlier_reproj", cams, meas=meas, expect=REPROJ, refine_iters=0, only_if_better=False, max_reproj_px=50.0))
    cams = ring_cameras(rng, 8, X_TRUE)
    meas, _ = project(cams, X_TRUE)
    noisy = meas + 0.3 * rng.standard_normal(meas.shape)
    cs.append(_case("noise_refine0", cams, meas=noisy, loss=1, scale=1.0, refine_iters=0))
    cs.append(_case("noise_refine5", cams, meas=noisy, loss=1, scale=1.0, refine_iters=5))
    cams = ring_cameras(rng, 9, X_TRUE)
    meas, _ = project(cams, X_TRUE)
    noisy = meas + 0.1 * rng.standard_normal(meas.shape)
    wts = rng.uniform(0.5, 2.0, 9)
    for kind, sc in ((0, 0.5), (1, 1.0), (2, 0.4), (3, 1.0)):
        cs.append(_case("loss%d_weights" % kind, cams, meas=noisy, w=wts, loss=kind, scale=sc))
    return cs


def run_case(dt, c):
    t = len(c["cams"])
    r = triangulate(dt, [0, t], c["cams"], c["meas"], c["w"], c["x_old"][None], c["loss"], c["scale"], **c["params"])
    return {k: v[0] for k, v in r.items()}


def x_bound(r64, rld, ulp_half=0.0):
    """The bound on |x - x_ld| per point of the issue: 10 x the fp64 restatement's own deviation from the long-double one, floored by
    eps64 kappa (|X| + max |C_o|), plus half an ulp of the scalar type at |x|."""
    dev = np.abs(np.asarray(r64["x"], LD) - rld["x"]).max(-1).astype(np.float64)
    floor = np.finfo(np.float64).eps * np.asarray(rld["kappa"], np.float64) * np.asarray(rld["size"], np.float64)
    return 10 * np.maximum(dev, floor) + ulp_half


COST_FLOOR = 1e-13  # test_gpu_stages.BOUND[("energy", 0)]: the floor for an fp64 sum of products (the rule is fp64 for both scalar types)
TINY_RMS_PX = 1e-3  # a track whose root-mean-square weighted residual is below this is "noiseless": its cost is rounding, not signal


def cost_bound(c64, cld, t, meas_max, w_max=1.0):
    """The same rule for a cost c = sum rho(s_o), per point: 10 x max(the fp64 restatement's deviation, COST_FLOOR c).
    Only for a noiseless track -- c <= t TINY_RMS_PX^2, where c is the square of residuals that are themselves differences of numbers
    of size |meas| and a relative floor means nothing (fp32 state, t = 2: c = 1e-9, the GPU and the reference part by 4.8e-21, COST_FLOOR c
    is 1e-22) -- the floor also holds what the residuals' rounding d = COST_FLOOR w (1 + |meas|) does to c: 2 sqrt(t c) d + t d^2, with
    the track's OWN largest |meas| and weight.  t, meas_max, w_max: per point (arrays) or scalars of one track."""
    dev = np.abs(np.asarray(c64, LD) - cld).astype(np.float64)
    c = np.abs(np.asarray(cld, np.float64))
    t = np.asarray(t, np.float64)
    d = COST_FLOOR * np.asarray(w_max, np.float64) * (1 + np.asarray(meas_max, np.float64))
    tiny = c <= t * TINY_RMS_PX ** 2
    floor = COST_FLOOR * c + np.where(tiny, 2 * np.sqrt(t * c) * d + t * d * d, 0.0)
    return 10 * np.maximum(dev, floor)


# ---- whole problems ----------------------------------------------------------------------------------------------------------------
def tracks(cam_idx, pt_idx, M):
    """(order, pt_ptr): the observations sorted by point (stable), and the first observation of every point (+ end)."""
    order = np.argsort(np.asarray(pt_idx), kind="stable")
    return order, np.concatenate([[0], np.cumsum(np.bincount(np.asarray(pt_idx), minlength=M))])


def reference(dt, cam15, pts, cam_idx, pt_idx, meas, w, **kw):
    """The rule for every point of a problem at the state (cam15 [N, 15], pts [M, 3]); meas [K, 2] and w [K] in problem order."""
    M = len(pts)
    order, pt_ptr = tracks(cam_idx, pt_idx, M)
    return triangulate(dt, pt_ptr, np.asarray(cam15).reshape(-1, 15)[np.asarray(cam_idx)[order]], np.asarray(meas).reshape(-1, 2)[order],
                       None if w is None else np.asarray(w)[order], pts, **kw)


def pack(cases, M, ftype=np.float64, seed=3):
    """A problem of M points that cycles through `cases` (one loss, one parameter set).  Every case brings cameras of its own, rounded to
    ftype; its copies share them and move the point a little (0.001 per copy along x), the measurements made again from the rounded
    cameras and rounded to ftype; the observations come in a shuffled order.  Returns dict(N, K, cam_idx, pt_idx, meas [K, 2], w [K] or
    None, cam15 [N, 15], pts [M, 3], expect [M], exact [M], x_true [M, 3], name [M])."""
    rng = np.random.default_rng(seed)
    cam15, first, ci, pi, meas, w, pts, expect, exact, xt, names = [], [], [], [], [], [], [], [], [], [], []
    n = 0
    for c in cases[:M]:
        first.append(n)
        cam15.append(c["cams"].astype(ftype).astype(np.float64))
        n += len(c["cams"])
    weighted = any(c["w"] is not None for c in cases)
    for j in range(M):
        q = j % len(cases)
        c, cams = cases[q], cam15[q]
        t = len(cams)
        sh = np.array([0.001 * (j // len(cases)), 0.0, 0.0])
        old, _ = project(c["cams"], c["x_true"]) if t else (np.zeros((0, 2)), None)
        new, _ = project(cams, c["x_true"] + sh) if t else (np.zeros((0, 2)), None)
        delta = c["meas"] - old  # what the case added to its projections (noise, an outlier) ...
        m = new + delta
        if t:
            big = np.abs(delta).max(-1) > 1000  # ... or wrote over them (the observation without an inverse)
            m[big] = c["meas"][big]
        ci += list(range(first[q], first[q] + t))
        pi += [j] * t
        meas.append(m)
        w.append(np.ones(t) if c["w"] is None else c["w"])
        pts.append(c["x_old"] + sh)
        expect.append(c["expect"])
        exact.append(c["exact"])
        xt.append(c["x_true"] + sh)
        names.append(c["name"])
    K = len(ci)
    cam15 = np.concatenate(cam15) if n else np.zeros((0, 15))
    meas = np.concatenate(meas).astype(ftype).astype(np.float64)
    w = np.concatenate(w).astype(ftype).astype(np.float64)
    perm = rng.permutation(K)
    return dict(N=len(cam15), K=K, cam_idx=np.asarray(ci, np.int32)[perm], pt_idx=np.asarray(pi, np.int32)[perm], meas=meas[perm],
                w=w[perm] if weighted else None, cam15=cam15, pts=np.asarray(pts).astype(ftype).astype(np.float64),
                expect=np.asarray(expect), exact=np.asarray(exact), x_true=np.asarray(xt), name=names)
