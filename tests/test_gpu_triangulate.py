"""ba_solver_triangulate_points on the GPU against the long-double restatement of the rule (triangulate_checks.py), run on the device's
own state (BA_GET_CAMS / BA_GET_POINTS), fp64 and fp32.

The designed tracks (t = 2 ... 300, strong distortion, no inverse, t = 1 and 0, half and twice the minimum angle, behind one camera, a
gross outlier for NOT_BETTER and REPROJ, 0.3 px noise with and without refinement, every loss with weights) are packed into problems of
M = 1, 255, 256 and 257 points with shuffled observations: a workgroup holds 32 points, so the first, a full and a partial last block of
both kernels are hit.  Rows `TRIANG <case> <metric> <value> <bound>`:
  x per replaced point   <= 10 max(fp64 restatement - long double, eps64 kappa (|X| + max |C_o|)) + half an ulp of the scalar type
  cost sums              the same rule per point with test_gpu_stages.BOUND's floor for an fp64 sum of products, summed over the asked
                         points (a noiseless track's near-zero cost also gets its residuals' rounding: triangulate_checks.cost_bound)
  statuses               equal to the reference's AND to the designed ones, none left out (every threshold is missed by >= 2x)
  refused points         keep their bits
On problem-21 a point may be left out of the status comparison only where the long-double reference's own decision margin is below
1e-9 relative, and at most 0.1 % of the points.  Measured: 0 of 11315 points left out and 0 statuses differ, fp64 and fp32 (a tie of two
all-saturated psi costs counts as decided: triangulate_checks._chunk); test_triangulate_checks.test_reference_on_problem21 checks on
the CPU that the fp64 restatement against the long-double one stays inside that share too (0 left out)."""
import ctypes as C
import os

import numpy as np
import pytest

import bundleadjustment_benchmarks_amd as ba
import triangulate_checks as TC
from test_gpu_stages import BOUND

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = {c["name"]: c for c in TC.designed_cases()}
BASE = ["t%d" % t for t in TC.T_SIZES] + ["distort", "noinverse", "t1", "t0", "angle_half", "angle_twice", "behind"]
# (names, loss, scale, parameters): one loss and one parameter set per call
SETS = {
    "default": (BASE, 0, 0.5, {}),
    "notbetter": (["outlier_notbetter", "t2", "t9", "behind"], 0, 0.5, dict(refine_iters=0)),
    "reproj": (["outlier_reproj", "t3", "t8", "angle_half"], 0, 0.5, dict(refine_iters=0, only_if_better=False, max_reproj_px=50.0)),
    "noise0": (["noise_refine0", "t2"], 1, 1.0, dict(refine_iters=0)),
    "noise5": (["noise_refine5", "t3"], 1, 1.0, dict(refine_iters=5)),
    "loss0w": (["loss0_weights"], 0, 0.5, {}),
    "loss1w": (["loss1_weights"], 1, 1.0, {}),
    "loss2w": (["loss2_weights"], 2, 0.4, {}),
    "loss3w": (["loss3_weights"], 3, 1.0, {}),
}
FT = {ba.F64: np.float64, ba.F32: np.float32}
PAR = dict(min_angle_deg=1.5, max_reproj_px=0.0, refine_iters=5, only_if_better=True)


def make(setname, M, scalar, kind=ba.CHOLESKY):
    names, loss, scale, over = SETS[setname]
    scale = float(FT[scalar](scale))  # (the loss's scale as the solver stores it)
    P = TC.pack([CASES[n] for n in names], M, FT[scalar])
    cams9 = np.zeros((P["N"], 9))
    cams9[:, 6] = 800.0
    prob = ba.Problem.from_arrays(P["N"], M, P["K"], P["cam_idx"], P["pt_idx"], P["meas"].reshape(-1), cams9.reshape(-1), P["pts"].reshape(-1))
    s = ba.Solver(prob, kind, scalar, device=0)
    s.set_state(P["cam15"].reshape(-1), P["pts"].reshape(-1))
    if loss != 0 or scale != 0.5:
        s.set_loss(loss, scale)
    if P["w"] is not None:
        s.set_obs_weights(P["w"])
    if loss != 0 or scale != 0.5 or P["w"] is not None:
        s.linearize()  # (the model is in force from here)
    assert np.array_equal(s.get(ba.GET_CAMS), P["cam15"].reshape(-1)) and np.array_equal(s.get(ba.GET_POINTS), P["pts"].reshape(-1))
    par = dict(PAR)
    par.update(over)
    return s, P, dict(loss=loss, scale=scale, **par), par


def half_ulp(x, scalar):
    return 0.5 * np.spacing(np.abs(x).max(-1).astype(FT[scalar])).astype(np.float64)


def check_rows(rows):
    bad = []
    for case, m, v, b in rows:
        print("TRIANG %s %s %.3e %.3e" % (case, m, v, b))
        if not v <= b:
            bad.append((case, m, v, b))
    assert not bad, bad


def against_reference(tag, s, P, kw, par, scalar, points=None):
    cam15, pts0 = s.get(ba.GET_CAMS).reshape(-1, 15), s.get(ba.GET_POINTS).reshape(-1, 3)
    stats, status = s.triangulate_points(points, **par)
    pts1 = s.get(ba.GET_POINTS).reshape(-1, 3)
    rld = TC.reference(TC.LD, cam15, pts0, P["cam_idx"], P["pt_idx"], P["meas"], P["w"], **kw)
    r64 = TC.reference(np.float64, cam15, pts0, P["cam_idx"], P["pt_idx"], P["meas"], P["w"], **kw)
    ids = np.arange(len(pts0)) if points is None else np.asarray(points)
    rows = []
    assert np.array_equal(rld["status"], P["expect"]), "the designed statuses are the reference's"
    assert float(min(rld["margin"].min(), rld["rmargin"].min())) >= 0.5 - 1e-6, "a designed case misses a threshold by less than a factor 2"
    rows.append((tag, "status_mismatches", float((status != rld["status"][ids]).sum()), 0.0))
    rep = ids[rld["status"][ids] == TC.REPLACED]
    keep = np.setdiff1d(np.arange(len(pts0)), rep)
    rows.append((tag, "kept_points_changed", float((pts1[keep].view(np.uint64) != pts0[keep].view(np.uint64)).sum()), 0.0))
    if len(rep):
        xb = TC.x_bound({"x": r64["x"][rep]}, {k: rld[k][rep] for k in ("x", "kappa", "size")}, half_ulp(rld["x"][rep].astype(np.float64), scalar))
        err = np.abs(pts1[rep] - rld["x"][rep]).max(-1).astype(np.float64)
        worst = int(np.argmax(err / xb))
        rows.append((tag + ":" + P["name"][rep[worst]], "x", float(err[worst]), float(xb[worst])))
        assert (err <= xb).all(), [(P["name"][j], e, b) for j, e, b in zip(rep, err, xb) if not e <= b][:5]
    tl = np.bincount(P["pt_idx"], minlength=len(pts0))
    mm, wm = np.zeros(len(pts0)), np.ones(len(pts0))  # per point: its own largest |meas| and weight
    np.maximum.at(mm, P["pt_idx"], np.abs(P["meas"]).max(-1))
    if P["w"] is not None:
        np.maximum.at(wm, P["pt_idx"], P["w"])
    after_ld = np.where(rld["status"] == 0, rld["cost_new"], rld["cost_old"])
    after_64 = np.where(r64["status"] == 0, r64["cost_new"], r64["cost_old"])
    for name, got, cl, c6 in (("cost_before", stats["cost_before"], rld["cost_old"], r64["cost_old"]), ("cost_after", stats["cost_after"], after_ld, after_64)):
        b = TC.cost_bound(c6[ids], cl[ids], tl[ids], mm[ids], wm[ids]).sum()
        rows.append((tag, name, float(abs(got - cl[ids].sum())), float(b)))
    assert stats["asked"] == len(ids) and np.array_equal(stats["by_status"], np.bincount(status, minlength=8))
    check_rows(rows)
    return stats, status, pts1


@pytest.mark.parametrize("scalar", [ba.F64, ba.F32], ids=["f64", "f32"])
@pytest.mark.parametrize("M", [1, 255, 256, 257])
def test_designed_tracks_default_set(M, scalar):
    assert BOUND[("energy", 0)] == TC.COST_FLOOR
    s, P, kw, par = make("default", M, scalar)
    against_reference("default/M%d" % M, s, P, kw, par, scalar)


@pytest.mark.parametrize("scalar", [ba.F64, ba.F32], ids=["f64", "f32"])
@pytest.mark.parametrize("setname", [k for k in SETS if k != "default"])
def test_designed_tracks_other_sets(setname, scalar):
    s, P, kw, par = make(setname, 257, scalar)
    against_reference(setname, s, P, kw, par, scalar)


@pytest.mark.parametrize("kind", [ba.QRKIT, ba.QRCHOL, ba.MOREQR, ba.QRSPQR, ba.ITERSCHUR])
def test_every_solver_kind(kind):
    s, P, kw, par = make("default", 40, ba.F64, kind)
    against_reference("kind%d" % kind, s, P, kw, par, ba.F64)


@pytest.mark.parametrize("scalar", [ba.F64, ba.F32], ids=["f64", "f32"])
def test_request_shape_and_repeatability(scalar):
    """All points, a subset, the subset in another order, and the same call twice: the same bits per point, the same status."""
    s, P, kw, par = make("default", 257, scalar)
    cam, pts = P["cam15"].reshape(-1), P["pts"].reshape(-1)
    rng = np.random.default_rng(1)
    sub = rng.permutation(257)[:100]
    runs = []
    for points in (None, None, sub, sub[::-1].copy(), np.sort(sub)):
        s.set_state(cam, pts)
        st, status = s.triangulate_points(points, **par)
        ids = np.arange(257) if points is None else points
        full = np.full(257, 255, np.uint8)
        full[ids] = status
        runs.append((ids, full, s.get(ba.GET_POINTS).reshape(-1, 3).view(np.uint64), st))
    a = runs[0]
    assert np.array_equal(a[1], runs[1][1]) and np.array_equal(a[2], runs[1][2]), "two runs differ"
    assert a[3]["cost_before"] == runs[1][3]["cost_before"] and a[3]["cost_after"] == runs[1][3]["cost_after"]
    rest = np.setdiff1d(np.arange(257), sub)
    p0 = P["pts"].view(np.uint64)
    for ids, full, bits, st in runs[2:]:
        assert np.array_equal(full[sub], a[1][sub]) and np.array_equal(bits[sub], a[2][sub]), "a point depends on the request"
        assert np.array_equal(bits[rest], p0[rest]), "a point that was not asked for moved"
        assert st["asked"] == 100
    # an empty request: nothing happens
    s.set_state(cam, pts)
    st, status = s.triangulate_points(np.zeros(0, np.int32), **par)
    assert st["asked"] == 0 and len(status) == 0 and np.array_equal(s.get(ba.GET_POINTS), pts)


@pytest.mark.parametrize("scalar", [ba.F64, ba.F32], ids=["f64", "f32"])
def test_fixed_and_prior_points_keep_their_bits(scalar):
    s, P, kw, par = make("default", 64, scalar)
    fixed = np.zeros(64, np.uint8)
    fixed[[0, 5, 33]] = 1
    s.set_constant(None, fixed)
    s.set_point_priors([7, 40], P["pts"][[7, 40]], sigma=1.0)
    st, status = s.triangulate_points(None, **par)
    special = [0, 5, 33, 7, 40]
    assert (status[special] == ba.TRI_FIXED).all() and st["by_status"][ba.TRI_FIXED] == 5
    others = np.setdiff1d(np.arange(64), special)
    assert np.array_equal(status[others], P["expect"][others])
    got = s.get(ba.GET_POINTS).reshape(-1, 3)
    assert np.array_equal(got[special].view(np.uint64), P["pts"][special].view(np.uint64))
    assert (got[others][P["expect"][others] == 0] != P["pts"][others][P["expect"][others] == 0]).any(1).all()


def _raw(s, tp, n, ids, status=None):
    return ba.lib().ba_solver_triangulate_points(s._h, C.byref(tp) if tp is not None else None, n, None if ids is None else ids.ctypes.data_as(C.c_void_p),
                                                 None if status is None else status.ctypes.data_as(C.c_void_p), None)


def test_refusals_leave_the_solver_unchanged():
    s, P, kw, par = make("default", 64, ba.F64)
    fresh, _, _, _ = make("default", 64, ba.F64)
    e, dmax = s.linearize()
    bytes0 = s.device_bytes()
    tp = ba.TriangulateParams.default()
    ids = np.arange(10, dtype=np.int32)
    assert _raw(s, tp, -1, ids) == ba.ERR_ARG
    assert _raw(s, tp, 3, None) == ba.ERR_ARG
    assert _raw(s, tp, 10, np.array([0, 1, 2, 3, 4, 5, 6, 7, 8, 64], np.int32)) == ba.ERR_ARG
    assert _raw(s, tp, 10, np.array([0, 1, 2, 3, 4, 5, 6, 7, 8, -1], np.int32)) == ba.ERR_ARG
    assert _raw(s, tp, 10, np.array([0, 1, 2, 3, 4, 5, 6, 7, 8, 3], np.int32)) == ba.ERR_ARG
    for field, val in (("min_angle_deg", -0.1), ("min_angle_deg", 180.0), ("min_angle_deg", float("nan")), ("max_reproj_px", -1.0),
                       ("max_reproj_px", float("inf")), ("refine_iters", -1)):
        bad = ba.TriangulateParams.default()
        setattr(bad, field, val)
        assert _raw(s, bad, 10, ids) == ba.ERR_ARG, (field, val)
    sh = ba.Solver(s.problem, ba.CHOLESKY, ba.F64, device=0, shard_rank=0, shard_world=2)
    assert _raw(sh, tp, 0, None) == ba.ERR_ARG
    del sh
    assert s.device_bytes() == bytes0 and np.array_equal(s.get(ba.GET_POINTS), P["pts"].reshape(-1))
    ef, df = fresh.linearize()
    assert (e, dmax) == (ef, df)
    assert s.try_step(1e-6 * dmax) == fresh.try_step(1e-6 * dmax)
    assert np.array_equal(s.get(ba.GET_DX), fresh.get(ba.GET_DX))
    # a loss or weights call that is pending
    s.set_loss(ba.LOSS_HUBER, 1.0)
    assert _raw(s, tp, 10, ids) == ba.ERR_ARG
    s.linearize()
    assert _raw(s, tp, 10, ids) == 0
    s.set_obs_weights(np.ones(P["K"]))
    assert _raw(s, tp, 10, ids) == ba.ERR_ARG
    s.minimize(max_trials=1)
    assert _raw(s, tp, 10, ids) == 0


def test_invalidation_and_device_bytes():
    s, P, kw, par = make("default", 257, ba.F64)
    M, K = 257, P["K"]
    e0, dmax = s.linearize()
    s.try_step(1e-6 * dmax)
    s.covariance(lam=1e-3 * dmax, cams=[0], points=[0])
    s.dogleg_prepare(1e-6 * dmax)
    b0 = s.device_bytes()
    st, status = s.triangulate_points(None, **par)
    assert s.device_bytes() - b0 == 24 * K + 6 * M + 8 * (10 * max(1, -(-8 * M // 256)) + 16)
    for call in (lambda: s.try_step(1e-6 * dmax), lambda: s.accept(), lambda: s.covariance(cams=[0], compute=False), lambda: s.try_dogleg(1.0)):
        with pytest.raises(ba.BAError) as ei:
            call()
        assert ei.value.code == ba.ERR_ARG
    b1 = s.device_bytes()
    e1, dmax1 = s.linearize()
    s.try_step(1e-6 * dmax1)
    s.triangulate_points(None, **par)
    assert s.device_bytes() == b1, "the second call allocates nothing"
    # cost_after - cost_before is the energy change that linearize() sees, and with only_if_better the energy does not rise
    rel = BOUND[("energy", 0)]
    print("TRIANG default/M257 energy_change %.3e %.3e" % (abs((e1 - e0) - (st["cost_after"] - st["cost_before"])), 10 * rel * (e0 + e1)))
    assert abs((e1 - e0) - (st["cost_after"] - st["cost_before"])) <= 10 * rel * (e0 + e1)
    assert e1 <= e0


@pytest.mark.parametrize("scalar", [ba.F64, ba.F32], ids=["f64", "f32"])
def test_energy_change_and_all_refused(scalar):
    s, P, kw, par = make("noise5", 257, scalar)
    e0, _ = s.linearize()
    st, status = s.triangulate_points(None, **par)
    e1, _ = s.linearize()
    rel = BOUND[("energy", 1 if scalar == ba.F32 else 0)]
    d = abs((e1 - e0) - (st["cost_after"] - st["cost_before"]))
    print("TRIANG noise5 energy_change %.3e %.3e" % (d, 10 * rel * (e0 + e1)))
    assert d <= 10 * rel * (e0 + e1) and e1 <= e0
    # a call that refuses every point (no two rays are 179 degrees apart): the state keeps its bits, and ba_minimize returns the rows it
    # returns without the call
    before = s.get(ba.GET_POINTS)
    ref = make("noise5", 257, scalar)[0]
    ref.set_state(s.get(ba.GET_CAMS), before)
    st2, status2 = s.triangulate_points(None, min_angle_deg=179.0, max_reproj_px=0.0, refine_iters=5, only_if_better=True)
    assert st2["by_status"][ba.TRI_REPLACED] == 0 and np.array_equal(s.get(ba.GET_POINTS).view(np.uint64), before.view(np.uint64))
    assert st2["cost_before"] == st2["cost_after"]
    ra, rb = s.minimize(max_trials=3)["trace"], ref.minimize(max_trials=3)["trace"]
    assert np.array_equal(ra[:, :5], rb[:, :5])


def _problem21():
    p = ba.Problem.load_bal(os.path.join(ROOT, "data", "problem-21-11315-pre.txt"))
    return p, p.arrays()


@pytest.mark.parametrize("scalar", [ba.F64, ba.F32], ids=["f64", "f32"])
def test_problem21(scalar):
    p, a = _problem21()
    s = ba.Solver(p, ba.CHOLESKY, scalar, device=0)
    e0, _ = s.linearize()
    cam15, pts0 = s.get(ba.GET_CAMS).reshape(-1, 15), s.get(ba.GET_POINTS).reshape(-1, 3)
    st, status = s.triangulate_points(None, **PAR)
    e1, _ = s.linearize()
    meas = a["meas"].reshape(-1, 2).astype(FT[scalar]).astype(np.float64)
    rld = TC.reference(TC.LD, cam15, pts0, a["cam_idx"], a["pt_idx"], meas, None, loss=0, scale=0.5, **PAR)
    sure = rld["margin"] >= 1e-9
    left_out = int((~sure).sum())
    print("TRIANG problem21 left_out %d %.1f" % (left_out, 0.001 * p.M))
    print("TRIANG problem21 status_mismatches %d 0" % int((status[sure] != rld["status"][sure]).sum()))
    print("TRIANG problem21 statuses %s" % dict(zip(ba.TRI_NAMES, st["by_status"].tolist())))
    print("TRIANG problem21 energy %.9g -> %.9g" % (e0, e1))
    assert left_out <= 0.001 * p.M
    assert np.array_equal(status[sure], rld["status"][sure])
    assert e1 <= e0
    assert st["by_status"][ba.TRI_REPLACED] > 0
