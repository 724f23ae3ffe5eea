"""A restatement of the observation filter's rule of include/ba_mi355x.h (csrc/ba_filter.hip.h) in numpy, in any float type: long double
is the reference, fp64 measures that reference's own rounding.  The per-observation step is vectorised over all observations; the
angle step over points, the tracks padded to the longest one of a chunk and masked.  Nothing here is shared with the library.

filter_rule(dt, pt_ptr, cam15, meas, active, pts, ...) takes the observations sorted by point (pt_ptr: first observation of every point,
+ end; cam15: one BA_GET_CAMS row PER OBSERVATION) and returns obs_status [K], pt_status [M], err [K] (NaN where inactive),
angle_deg [M] (the full theta, 0 where the angle step did not run), survivors [M], and the margins of the decisions:
  obs_margin [K]  the smallest relative distance of a compared quantity from its threshold on the way to the observation's own status:
                  |XX_2| / |XX| against 0 (require_front), |err - max_reproj_px| / max_reproj_px.  XX_2 == 0 exactly is a tie the rule
                  decides (not in front) and every float type computes it as the same 0: it counts as decided (inf).
  pt_margin [M]   |theta - min_angle| / min_angle where the angle step ran, and the survivor count against min_track: the count is
                  an integer, the threshold lies at min_track - 1/2, its margin is |count - (min_track - 1/2)| / (1 / 2) >= 1.
A status can depend on the margins of all observations of its point: point_margin() folds them."""
import numpy as np

import triangulate_checks as TC

KEPT, WAS_OFF, BEHIND, NONFINITE, REPROJ, POINT = range(6)
PT_KEPT, PT_SHORT, PT_LOW_ANGLE = range(3)
LD = np.longdouble
DEFAULTS = dict(max_reproj_px=4.0, min_angle_deg=1.5, min_track=2, require_front=True)


def observations(dt, cam, meas, X, max_reproj_px, require_front):
    """Step 2 for every observation as if active: cam [K, 15], meas [K, 2], X [K, 3] (its point) -> status, err, ray d [K, 3], margin."""
    inf = dt(np.inf)
    with np.errstate(all="ignore"):
        R = cam[:, :9].reshape(-1, 3, 3)
        XX = np.einsum("krc,kc->kr", R, X) + cam[:, 9:12]
        xu = XX[:, :2] / XX[:, 2:3]
        r2u = (xu * xu).sum(-1)
        f, k1, k2 = cam[:, 12], cam[:, 13], cam[:, 14]
        kr = 1 + k1 * r2u + k2 * r2u * r2u
        e = (f * kr)[:, None] * xu - meas
        err = np.sqrt((e * e).sum(-1))
        C = -np.einsum("krc,kr->kc", R, cam[:, 9:12])
        v = C - X
        n = np.sqrt((v * v).sum(-1))
        has = (n > 0) & np.isfinite(n)
        d = np.where(has[:, None], v / np.where(has, n, 1)[:, None], dt(0))
        behind = ~(XX[:, 2] < 0) if require_front else np.zeros(len(cam), bool)
        nonfin = ~np.isfinite(err)
        rep = (err > dt(max_reproj_px)) if max_reproj_px > 0 else np.zeros(len(cam), bool)
        status = np.where(behind, BEHIND, np.where(nonfin, NONFINITE, np.where(rep, REPROJ, KEPT)))
        nxx = np.sqrt((XX * XX).sum(-1))
        fm = np.where(XX[:, 2] == 0, inf, np.abs(XX[:, 2]) / np.where(nxx > 0, nxx, 1))
        fm = np.where(np.isfinite(fm), fm, inf) if require_front else np.full(len(cam), inf, dt)
        rm = np.abs(err - dt(max_reproj_px)) / dt(max_reproj_px) if max_reproj_px > 0 else np.full(len(cam), inf, dt)
        rm = np.where(np.isfinite(rm), rm, inf)
        margin = np.where(behind, fm, np.where(nonfin, fm, np.minimum(fm, rm)))
    return status, err, d, margin


def filter_rule(dt, pt_ptr, cam15, meas, active, pts, max_reproj_px=4.0, min_angle_deg=1.5, min_track=2, require_front=True, budget=3_000_000):
    pt_ptr = np.asarray(pt_ptr, np.int64)
    M = len(pt_ptr) - 1
    cam15 = np.asarray(cam15, dt).reshape(-1, 15)
    K = len(cam15)
    meas = np.asarray(meas, dt).reshape(-1, 2)
    pts = np.asarray(pts, dt).reshape(M, 3)
    act = np.ones(K, bool) if active is None else np.asarray(active).reshape(-1) != 0
    tl = np.diff(pt_ptr)
    pid = np.repeat(np.arange(M), tl)
    st, err, d, om = observations(dt, cam15, meas, pts[pid], max_reproj_px, require_front)
    st = np.where(act, st, WAS_OFF)
    err = np.where(act, err, dt(np.nan))
    om = np.where(act, om, dt(np.inf))
    surv = st == KEPT
    ns = np.bincount(pid[surv], minlength=M) if K else np.zeros(M, np.int64)
    pst = np.where(ns < min_track, PT_SHORT, PT_KEPT)
    pm = np.abs(ns - (min_track - 0.5)).astype(dt) / dt(0.5)
    ang = np.zeros(M, dt)
    if min_angle_deg > 0:
        todo = np.nonzero(pst == PT_KEPT)[0]
        todo = todo[np.argsort(tl[todo], kind="stable")]
        pos = 0
        while pos < len(todo):
            end = pos + 1
            while end < len(todo) and (end + 1 - pos) * max(int(tl[todo[end]]), 1) ** 2 <= budget:
                end += 1
            idx = todo[pos:end]
            tm = max(int(tl[idx].max()), 1)
            mask = np.arange(tm)[None, :] < tl[idx][:, None]
            sel = np.where(mask, pt_ptr[idx][:, None] + np.arange(tm)[None, :], 0) if K else np.zeros((len(idx), tm), np.int64)
            if K:
                dd = d[sel]
                ok = mask & surv[sel] & (dd != 0).any(-1)
            else:
                dd, ok = np.zeros(sel.shape + (3,), dt), np.zeros(sel.shape, bool)
            diff = dd[:, :, None, :] - dd[:, None, :, :]
            c2 = (diff * diff).sum(-1)
            c2 = np.where(ok[:, :, None] & ok[:, None, :], c2, dt(0)).reshape(len(idx), -1).max(-1)
            with np.errstate(all="ignore"):
                ang[idx] = 2 * np.arctan2(np.sqrt(c2), np.sqrt(np.maximum(4 - c2, dt(0))))
            pos = end
        amin = dt(min_angle_deg) * dt(np.pi) / 180
        ran = pst == PT_KEPT
        pst = np.where(ran & (ang < amin), PT_LOW_ANGLE, pst)
        pm = np.where(ran, np.minimum(pm, np.abs(ang - amin) / amin), pm)
        ang = np.where(ran, ang, dt(0))
    dropped = (pst != PT_KEPT)[pid] if K else np.zeros(0, bool)
    st = np.where(surv & dropped, POINT, st)
    return dict(obs_status=st.astype(np.int64), pt_status=pst.astype(np.int64), err=err, angle_deg=ang * 180 / dt(np.pi), survivors=ns,
                obs_margin=om, pt_margin=pm, pid=pid)


def point_margin(r):
    """Per point: the smallest margin of anything its statuses depend on (its own and its observations')."""
    m = np.asarray(r["pt_margin"], np.float64).copy()
    if len(r["pid"]):
        np.minimum.at(m, r["pid"], np.asarray(r["obs_margin"], np.float64))
    return m


# ---- designed tracks ---------------------------------------------------------------------------------------------------------------
X0 = TC.X_TRUE  # (0.4, -0.2, 1.5): z is a short binary fraction, pack() moves the copies along x alone
T_SIZES = (0, 1, 2, 7, 8, 9, 17, 300)  # the lane-stride edges of 8 lanes, and a long track


def cam_at(angle_deg, X=X0, radius=5.0, f=800.0):
    """One camera in the plane y = X_y whose line of sight to X makes angle_deg with the z axis (two_rays' construction)."""
    a = np.deg2rad(angle_deg)
    C = X + radius * np.array([np.sin(a), 0.0, np.cos(a)])
    z = (C - X) / radius
    x = np.cross([0.0, 1.0, 0.0], z)
    x /= np.linalg.norm(x)
    R = TC.rodrigues(np.array([0.01, -0.02, 0.03])) @ np.stack([x, np.cross(z, x), z])
    cam = np.zeros(15)
    cam[:9], cam[9:12], cam[12] = R.reshape(-1), -R @ C, f
    return cam


def plane_camera(X=X0, f=800.0):
    """A camera with R = I whose principal plane holds X: XX_2 = 1 * X_2 + (-X_2) = 0 exactly in every float type (0 * x + 0 * y + z - z),
    also for a copy of the point moved along x."""
    cam = np.zeros(15)
    cam[[0, 4, 8]] = 1.0
    cam[9:12] = 0.3, -0.1, -X[2]
    cam[12] = f
    return cam


def _case(name, cams, expect_obs, expect_pt, shift=None, active=None, X=X0):
    cams = np.asarray(cams, np.float64).reshape(-1, 15)
    t = len(cams)
    sh = np.zeros((t, 2)) if shift is None else np.asarray(shift, np.float64)
    return dict(name=name, cams=cams, X=np.asarray(X, np.float64), shift=sh, active=np.ones(t, bool) if active is None else np.asarray(active, bool),
                expect_obs=np.asarray(expect_obs, np.int64).reshape(-1), expect_pt=int(expect_pt))


def case_meas(c, cams=None, X=None):
    """The case's measurements: the (long double) projections of X, plus what the case adds; an observation that has no finite
    projection (the principal plane) measures (0, 0)."""
    cams = c["cams"] if cams is None else cams
    if not len(cams):
        return np.zeros((0, 2))
    with np.errstate(all="ignore"):
        m, _ = TC.project(cams, c["X"] if X is None else X)
    return np.where(np.isfinite(m).all(-1)[:, None], m, 0.0) + c["shift"]


def designed_cases(require_front=True, seed=23, max_reproj_px=4.0):
    """The designed tracks: every case misses every threshold of the rule by a factor >= 2 (or hits XX_2 = 0 exactly).  One parameter set:
    max_reproj_px, 1.5 degrees, min_track 2, and require_front as given (which decides what the principal-plane and the behind
    observations are)."""
    rng = np.random.default_rng(seed)
    px = max_reproj_px
    cs = []
    for t in T_SIZES:
        cams = TC.ring_cameras(rng, t, X0) if t else np.zeros((0, 15))
        cs.append(_case("t%d" % t, cams, [KEPT if t >= 2 else POINT] * t, PT_KEPT if t >= 2 else PT_SHORT))
    # one observation at 2 x and one at 0.5 x of max_reproj_px
    sh = np.zeros((5, 2))
    sh[1] = 2 * px, 0.0
    sh[3] = 0.0, 0.5 * px
    cs.append(_case("reproj", TC.ring_cameras(rng, 5, X0), [KEPT, REPROJ, KEPT, KEPT, KEPT], PT_KEPT, shift=sh))
    # one camera turned round (about its y axis): X is behind it, on the same line of sight (so its projection is still exact)
    cams = TC.ring_cameras(rng, 4, X0, k1=0.0, k2=0.0)
    flip = np.diag([-1.0, 1.0, -1.0])
    R = flip @ cams[1, :9].reshape(3, 3)
    cams[1, :9], cams[1, 9:12] = R.reshape(-1), flip @ cams[1, 9:12]
    cs.append(_case("behind", cams, [KEPT, BEHIND if require_front else KEPT, KEPT, KEPT], PT_KEPT))
    # X on a camera's principal plane
    cams = np.concatenate([TC.ring_cameras(rng, 3, X0), plane_camera()[None]])
    cs.append(_case("plane", cams, [KEPT, KEPT, KEPT, BEHIND if require_front else NONFINITE], PT_KEPT))
    # min_track - 1 survivors: the last one goes with its point
    sh = np.zeros((2, 2))
    sh[0] = -2 * px, 0.0
    cs.append(_case("short_after", TC.ring_cameras(rng, 2, X0), [REPROJ, POINT], PT_SHORT, shift=sh))
    cs.append(_case("angle_half", [cam_at(-0.375), cam_at(0.375)], [POINT, POINT], PT_LOW_ANGLE))
    cs.append(_case("angle_twice", [cam_at(-1.5), cam_at(1.5)], [KEPT, KEPT], PT_KEPT))
    # three views whose only wide pair contains a REPROJ observation: LOW_ANGLE among the survivors
    sh = np.zeros((3, 2))
    sh[2] = 0.0, 2 * px
    cs.append(_case("wide_pair_reproj", [cam_at(-0.375), cam_at(0.375), cam_at(30.0)], [POINT, POINT, REPROJ], PT_LOW_ANGLE, shift=sh))
    # an observation already inactive that would rescue its point
    cs.append(_case("was_off", [cam_at(-0.375), cam_at(30.0), cam_at(0.375)], [POINT, WAS_OFF, POINT], PT_LOW_ANGLE, active=[1, 0, 1]))
    for c in cs:
        c["meas"] = case_meas(c)
    return cs


def run_case(dt, c, **par):
    t = len(c["cams"])
    return filter_rule(dt, [0, t], c["cams"], c["meas"], c["active"], c["X"][None], **par)


def err_bound(e64, eld, meas_abs):
    """Per observation: 10 max(the fp64 restatement's own deviation from long double, eps64 err), plus the rounding of the residual
    itself: err is the norm of differences of numbers of size |meas| (at a noiseless observation nothing else), each rounded to
    eps64 (1 + |meas|) at best, and one fp64 evaluation is one sample of that noise -- 8 such roundings (the projection's products
    and the subtraction, two components)."""
    eps = np.finfo(np.float64).eps
    with np.errstate(all="ignore"):
        dev = np.abs(np.asarray(e64, LD) - np.asarray(eld, LD)).astype(np.float64)
        e = np.abs(np.asarray(eld, np.float64))
    return 10 * np.maximum(dev, eps * e) + 8 * eps * (1 + np.asarray(meas_abs, np.float64))


# ---- whole problems ----------------------------------------------------------------------------------------------------------------
def reference(dt, cam15, pts, cam_idx, pt_idx, meas, active, **par):
    """The rule for every point of a problem at the state (cam15 [N, 15], pts [M, 3]); meas [K, 2] and active [K] in problem order.
    The per-observation results come back in problem order."""
    M = len(pts)
    order, pt_ptr = TC.tracks(cam_idx, pt_idx, M)
    act = None if active is None else np.asarray(active)[order]
    r = filter_rule(dt, pt_ptr, np.asarray(cam15).reshape(-1, 15)[np.asarray(cam_idx)[order]], np.asarray(meas).reshape(-1, 2)[order], act, pts, **par)
    inv = np.empty_like(order)
    inv[order] = np.arange(len(order))
    for k in ("obs_status", "err", "obs_margin", "pid"):
        r[k] = r[k][inv]
    return r


def pack(cases, M, ftype=np.float64, seed=5):
    """A problem of M points that cycles through `cases`.  Every case brings cameras of its own, rounded to ftype; its copies share
    them and move the point a little (0.001 per copy along x); the point is rounded to ftype and the measurements are made again from
    the rounded cameras and the rounded point, then rounded to ftype; the observations come in a shuffled order.  Returns dict(N, K,
    cam_idx, pt_idx, meas [K, 2], active [K] bool, cam15 [N, 15], pts [M, 3], expect_obs [K], expect_pt [M], name [M])."""
    rng = np.random.default_rng(seed)
    cam15, first = [], []
    n = 0
    for c in cases[:M]:
        first.append(n)
        cam15.append(c["cams"].astype(ftype).astype(np.float64))
        n += len(c["cams"])
    ci, pi, meas, act, pts, eo, ep, names = [], [], [], [], [], [], [], []
    for j in range(M):
        q = j % len(cases)
        c, cams = cases[q], cam15[q]
        t = len(cams)
        X = (c["X"] + np.array([0.001 * (j // len(cases)), 0.0, 0.0])).astype(ftype).astype(np.float64)
        ci += list(range(first[q], first[q] + t))
        pi += [j] * t
        meas.append(case_meas(c, cams, X))
        act.append(c["active"])
        eo.append(c["expect_obs"])
        pts.append(X)
        ep.append(c["expect_pt"])
        names.append(c["name"])
    K = len(ci)
    cam15 = np.concatenate(cam15) if n else np.zeros((0, 15))
    meas = np.concatenate(meas).astype(ftype).astype(np.float64)
    perm = rng.permutation(K)
    return dict(N=len(cam15), K=K, cam_idx=np.asarray(ci, np.int32)[perm], pt_idx=np.asarray(pi, np.int32)[perm], meas=meas[perm],
                active=np.concatenate(act)[perm], cam15=cam15, pts=np.asarray(pts), expect_obs=np.concatenate(eo)[perm],
                expect_pt=np.asarray(ep), name=names)
