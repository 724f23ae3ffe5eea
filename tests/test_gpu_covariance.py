"""GPU: covariance blocks of cameras and points (ba_solver_covariance_compute / _get, csrc/ba_cov.hip.h), CHOLESKY and QRCHOL, fp64.

The yardstick is never the code under test: the reduced camera matrix S is assembled in quad precision from the GPU's own BA_GET_JC /
BA_GET_JP at the same lambda (cov_checks.quad_reduced), residuals of S Sigma = I are evaluated in quad (referee_sym_residual), point
blocks are compared with the Schur formula in extended precision fed with an extended-precision Sigma_cc.  Bounds follow the
repository's rule (test_gpu_stages.py): max(10 x the error of the plain fp64 CPU route on the same inputs by the same metric, floor),
the CPU route being numpy.linalg.inv of the quad S (free rows) and the numpy formula in fp64.  Floors = the CPU route on problem-21 at
lambda = 1e-2 max diag J'J, rounded up to a power of ten (measured 5.6e-17 for the columns, 3.5e-16 for the point blocks).

Cases: no mask at lambda = 1e-6 and 1e-2 max diag J'J; `gauge0` = gauge mask + 1 % of the points fixed at lambda = 0.  FINDING, recorded
in DESIGN.md section 11: at the start state of problem-21, problem-39 and the synthetic problems `gauge0` is not positive definite
whatever the gauge -- the robustifier leaves an outlier observation a rank-1 Jacobian, and a point seen twice, both times as an outlier,
has a rank-2 U_p (3035 of problem-21's 11315 points, 4741 of problem-39's 18060; smallest / largest eigenvalue ~1e-16 of either sign).
The host decides that from the GPU's Jp alone (cov_checks, numpy): where some free point's U_p has lambda_min <= 1e-10 lambda_max the
required outcome is BA_ERR_SINGULAR or, the pivot being roundoff of either sign, a finite result -- the issue's own either-or for
roundoff pivots; where none has, the accuracy bounds apply.  So that lambda = 0 is measured all the same, the further case `gauge0fix`
fixes those ill-determined points as well (gauge mask + 1 % + them): positive definite, same bounds, fixed-point path in bulk.

Every figure is printed as `COV <case> <metric> <value> <bound>`."""
import hashlib

import numpy as np
import pytest

import cov_checks as CC

pytestmark = pytest.mark.gpu

FLOOR_ETA = 1e-16  # numpy.linalg.inv, problem-21, lambda = 1e-2 max diag: max eta 5.580e-17
FLOOR_PT = 1e-15   # numpy formula in fp64, same case: max relative block error 3.548e-16
KINDS = ["CHOLESKY", "QRCHOL"]
CASES = ["lam1e-6", "lam1e-2", "gauge0", "gauge0fix"]
_cpu_eta = {}
_quad_s = {}  # the last quad S, by the hash of its inputs


class Checker:
    def __init__(self, case):
        self.case, self.rows = case, []

    def __call__(self, metric, value, bound):
        self.rows.append((metric, float(value), float(bound)))
        print("COV %s %s %.3e %.1e" % (self.case, metric, value, bound))

    def done(self):
        bad = [r for r in self.rows if not (r[1] <= r[2])]
        assert not bad, (self.case, bad)


def _problem(ba, name, prob21, prob39):
    return {"p21": prob21, "p39": prob39}.get(name) or ba.Problem.synthetic(60, 2400, 9600, 160)


def _ill_points(po, Jp):
    """Points whose U_p = sum Jp'Jp is numerically rank deficient (lambda_min <= 1e-10 lambda_max), from the GPU's Jp on the host."""
    U, _ = CC.point_blocks(po, np.zeros((po.K, 2, 9)), Jp, 0.0)
    ev = np.linalg.eigvalsh(U)
    return ev[:, 0] <= 1e-10 * ev[:, 2]


def _linearised(ba, O, pg, kind, case, seed=1):
    """Solver at its linearisation under the case's mask: (solver, oracle problem, lam, cam_mask, pt_fixed, Jc, Jp, singular)."""
    po = CC.sorted_oracle_problem(O, pg)
    s = ba.Solver(pg, getattr(ba, kind), ba.F64)
    _, dmax = s.linearize()
    cm = pf = None
    singular = False
    if case.startswith("gauge0"):
        cm = pg.gauge_mask(0)
        pf = np.zeros(pg.M, np.uint8)
        pf[np.random.default_rng(seed).choice(pg.M, max(1, pg.M // 100), replace=False)] = 1
        ill = _ill_points(po, s.get(ba.GET_JP).reshape(-1, 2, 3))
        if case == "gauge0fix":
            pf[ill] = 1
        else:
            singular = bool((ill & (pf == 0)).any())
        s.set_constant(cm, pf)
        s.linearize()
    lam = {"lam1e-6": 1e-6 * dmax, "lam1e-2": 1e-2 * dmax}.get(case, 0.0)
    return s, po, lam, cm, pf, s.get(ba.GET_JC).reshape(-1, 2, 9), s.get(ba.GET_JP).reshape(-1, 2, 3), singular


def _all_pairs(N):
    a, b = np.meshgrid(np.arange(N), np.arange(N), indexing="ij")
    return np.stack([a.ravel(), b.ravel()], axis=1).astype(np.int32)


def _assemble(cc, N):
    return cc.reshape(N, N, 9, 9).transpose(0, 2, 1, 3).reshape(9 * N, 9 * N)


# ---- 3 + 4. camera blocks solve S Sigma = I; point blocks against the formula in extended precision -------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("prob", ["p21", "p39", "syn60"])
def test_blocks_against_the_quad_yardstick(ba, O, gpu_ok, prob21, prob39, prob, kind, case):
    ck = Checker("%s[%s,%s]" % (case, prob, kind))
    pg = _problem(ba, prob, prob21, prob39)
    s, po, lam, cm, pf, Jc, Jp, singular = _linearised(ba, O, pg, kind, case)
    N, M = pg.N, pg.M
    fc, fp = CC.free_sets(po, cm, pf)
    rng = np.random.default_rng(7)
    if prob == "p21":
        ids = np.arange(M, dtype=np.int32)
    else:
        track = np.bincount(po.pt_idx, minlength=M)
        ids = np.unique(np.concatenate([rng.choice(M, min(M, 2000), replace=False), [int(np.argmax(track))]])).astype(np.int32)
    try:
        cc, pp = s.covariance(lam, cam_pairs=_all_pairs(N), points=ids)
    except ba.BAError as e:
        print("COV %s returned %s (host: some free U_p rank deficient = %s)" % (ck.case, e.code, singular))
        assert singular and e.code == ba.ERR_SINGULAR, (e.code, singular)
        s.try_step(1e-3)  # solver usable
        return
    assert np.isfinite(cc).all() and np.isfinite(pp).all()
    if singular:  # roundoff pivots came out positive: finite, nothing more can be asked of an inverse that does not exist
        print("COV %s succeeded on a numerically singular H (roundoff pivots > 0)" % ck.case)
        return
    # symmetry bit for bit, fixed rows / columns exactly zero
    c4 = cc.reshape(N, N, 9, 9)
    assert np.array_equal(c4, c4.transpose(1, 0, 3, 2))
    Sig = _assemble(cc, N)
    assert not Sig[~fc].any() and not Sig[:, ~fc].any()
    assert not pp[~fp[ids]].any()
    # camera blocks
    # (the yardsticks depend on J, lambda and the mask alone: computed once where the two kinds' linearisations are the same bits)
    jkey = hashlib.sha1(Jc.tobytes() + Jp.tobytes() + np.float64(lam).tobytes() + fc.tobytes() + fp.tobytes()).hexdigest()
    if jkey not in _quad_s:
        _quad_s.clear()
        _quad_s[jkey] = CC.quad_reduced(O, O.CHOLESKY, po, Jc, Jp, lam, fp)
    S = _quad_s[jkey]
    key = hashlib.sha1(S.tobytes() + fc.tobytes()).hexdigest()
    if key not in _cpu_eta:
        _cpu_eta[key] = float(CC.column_errors(O, S, CC.inv_free(S, fc), fc).max())
    eta = CC.column_errors(O, S, Sig, fc)
    ck("eta_max(cpu %.1e)" % _cpu_eta[key], eta.max(), max(10 * _cpu_eta[key], FLOOR_ETA))
    # point blocks
    Sx = CC.refined_inverse(S, fc)
    ref = CC.point_covariance(po, Jc, Jp, lam, fp, Sx, ids, np.longdouble)
    cpu = CC.point_covariance(po, Jc, Jp, lam, fp, CC.inv_free(S, fc), ids, np.float64)
    e_cpu = float(CC.block_errors(cpu, ref).max())
    ck("point_blocks(cpu %.1e)" % e_cpu, CC.block_errors(pp, ref).max(), max(10 * e_cpu, FLOOR_PT))
    assert np.array_equal(pp, pp.transpose(0, 2, 1))
    np.linalg.cholesky(pp[fp[ids]])  # every free block positive definite (raises otherwise)
    ck.done()


# ---- 5. end to end on a small problem ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_small_problem_against_the_dense_inverse(ba, O, gpu_ok, kind):
    """synthetic(6, 40, 160, 3), gauge mask (+ the ill-determined points fixed, see the module text), lambda = 0: camera diagonal blocks
    and every point block against the dense inverse of the whole J'J from the GPU's own J.  Bound 8 cond(H) eps relative to the largest
    block of its kind (test_covariance_cpu.py's)."""
    ck = Checker("small[%s]" % kind)
    pg = ba.Problem.synthetic(6, 40, 160, 3)
    s, po, lam, cm, pf, Jc, Jp, _ = _linearised(ba, O, pg, kind, "gauge0fix")
    cc, pp = s.covariance(0.0, cams=np.arange(pg.N), points=np.arange(pg.M))
    dense = CC.dense_covariance(po, Jc, Jp, 0.0, cm, pf)
    bound = 8 * dense["cond"] * CC.EPS
    dd = np.stack([dense["cc"][9 * a:9 * a + 9, 9 * a:9 * a + 9] for a in range(pg.N)])
    nrm = lambda x: np.sqrt((x ** 2).sum(axis=(1, 2)))  # noqa: E731
    ck("camera_diagonal_blocks(cond %.1e)" % dense["cond"], nrm(cc - dd).max() / nrm(dd).max(), bound)
    ck("point_blocks", nrm(pp - dense["pp"]).max() / nrm(dense["pp"]).max(), bound)
    fc, fp = CC.free_sets(po, cm, pf)
    assert not pp[~fp].any() and not cc[0][:6].any() and not cc[0][:, :6].any()
    ck.done()


# ---- 6. no side effects -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_covariance_leaves_the_lm_state_alone(ba, gpu_ok, prob21, kind):
    def run(with_cov):
        s = ba.Solver(prob21, getattr(ba, kind), ba.F64)
        _, dmax = s.linearize()
        out = []
        if with_cov:
            out.append(s.covariance(1e-4 * dmax, cams=[0, 5], points=[0, 1, 2]))
            out.append(s.covariance(1e-4 * dmax, cams=[0, 5], points=[0, 1, 2]))
        step = s.try_step(1e-6 * dmax)
        state = [s.get(ba.GET_DX), s.get(ba.GET_CAMS_TEST), s.get(ba.GET_POINTS_TEST)]
        if with_cov:  # a try_step does not make the result stale
            out.append(s.covariance(cams=[0, 5], points=[0, 1, 2], compute=False))
        return step, state, out

    a, sa, _ = run(False)
    b, sb, cov = run(True)
    assert a == b
    for x, y in zip(sa, sb):
        assert np.array_equal(x, y)
    for k in (1, 2):  # two computes, and a read behind a try_step: the same bits
        assert np.array_equal(cov[0][0], cov[k][0]) and np.array_equal(cov[0][1], cov[k][1])

    # the other order: behind a try_step, a compute leaves the step, the kept S / rhs and xTest what they were, and accept works
    s = ba.Solver(prob21, getattr(ba, kind), ba.F64)
    s.keep_intermediates(True)
    _, dmax = s.linearize()
    s.try_step(1e-6 * dmax)
    what = (ba.GET_DX, ba.GET_S, ba.GET_RHS, ba.GET_CAMS_TEST, ba.GET_POINTS_TEST)
    before = [s.get(w) for w in what]
    s.covariance(1e-4 * dmax, cams=[0, 5], points=[0, 1, 2])
    for w, x in zip(what, before):
        assert np.array_equal(x, s.get(w)), w
    s.accept()
    assert np.array_equal(s.get(ba.GET_CAMS), before[3]) and np.array_equal(s.get(ba.GET_POINTS), before[4])

    def trace(with_cov):
        s = ba.Solver(prob21, getattr(ba, kind), ba.F64)
        if with_cov:
            _, dmax = s.linearize()
            s.covariance(1e-4 * dmax, cams=[0])
        return s.minimize(max_trials=20)["trace"][:, :5]

    assert np.array_equal(trace(False), trace(True))


# ---- 7. refusals, singularity, memory ---------------------------------------------------------------------------------------------------
def _code(ba, fn):
    try:
        fn()
    except ba.BAError as e:
        return e.code
    return 0


def test_refusals(ba, gpu_ok, prob21):
    for kind, scalar in ((ba.ITERSCHUR, ba.F64), (ba.QRKIT, ba.F64), (ba.QRSPQR, ba.F64), (ba.MOREQR, ba.F64), (ba.CHOLESKY, ba.F32)):
        s = ba.Solver(prob21, kind, scalar)
        _, dmax = s.linearize()
        assert _code(ba, lambda: s.covariance(1e-3 * dmax, cams=[0])) == ba.ERR_ARG, (kind, scalar)
        s.try_step(1e-3 * dmax)
    s = ba.Solver(prob21, ba.CHOLESKY, ba.F64, shard_rank=0, shard_world=2)
    assert _code(ba, lambda: s.covariance(1.0, cams=[0])) == ba.ERR_ARG  # sharded (and not linearised)
    s = ba.Solver(prob21, ba.CHOLESKY, ba.F64)
    b0 = s.device_bytes()
    assert _code(ba, lambda: s.covariance(1.0, cams=[0])) == ba.ERR_ARG  # no linearisation yet
    assert _code(ba, lambda: s.covariance(cams=[0], compute=False)) == ba.ERR_ARG  # get before compute
    _, dmax = s.linearize()
    lam = 1e-3 * dmax
    for bad in (-1.0, float("nan"), float("inf")):
        assert _code(ba, lambda: s.covariance(bad, cams=[0])) == ba.ERR_ARG
    assert s.device_bytes() == b0  # refusals come before any allocation
    s.covariance(lam, cams=[0])
    assert s.device_bytes() - b0 == CC.cov_buffer_bytes(prob21.N)
    for pairs, pts in (([[0, prob21.N]], None), ([[-1, 0]], None), (None, [prob21.M]), (None, [-1])):
        assert _code(ba, lambda: s.covariance(cam_pairs=pairs, points=pts, compute=False)) == ba.ERR_ARG
    s.covariance(cams=[0], compute=False)
    for stale in ("linearize", "accept", "set_state", "set_constant"):
        s.linearize()
        s.covariance(lam, cams=[0])
        if stale == "linearize":
            s.linearize()
        elif stale == "accept":
            s.try_step(lam)
            s.accept()
        elif stale == "set_state":
            s.set_state(s.get(ba.GET_CAMS), None)
        else:
            s.set_constant(prob21.gauge_mask(0), None)
        assert _code(ba, lambda: s.covariance(cams=[0], compute=False)) == ba.ERR_ARG, stale
    assert _code(ba, lambda: s.covariance(lam, cams=[0])) == ba.ERR_ARG  # a mask set since the last linearisation
    s.linearize()
    s.covariance(lam, cams=[0])
    assert s.device_bytes() - b0 >= CC.cov_buffer_bytes(prob21.N)  # (+ the mask's own buffers; the covariance buffer is allocated once)
    s.try_step(lam)


@pytest.mark.parametrize("kind", KINDS)
def test_singular_cases(ba, O, gpu_ok, prob21, kind):
    K = getattr(ba, kind)
    # lambda = 0 without a mask, and with camera 0's pose fixed but the scale free: BA_ERR_SINGULAR or roundoff pivots -- either, no NaN
    for mask in (None, "pose0"):
        s = ba.Solver(prob21, K, ba.F64)
        if mask:
            cm = np.zeros(prob21.N, np.uint16)
            cm[0] = ba.FIX_POSE
            s.set_constant(cm, None)
        _, dmax = s.linearize()
        try:
            cc, pp = s.covariance(0.0, cams=np.arange(prob21.N), points=np.arange(50))
            assert np.isfinite(cc).all() and np.isfinite(pp).all()
            print("COV singular[%s,%s] lambda=0 succeeded (roundoff pivots)" % (kind, mask))
        except ba.BAError as e:
            assert e.code == ba.ERR_SINGULAR
            print("COV singular[%s,%s] lambda=0 returned BA_ERR_SINGULAR" % (kind, mask))
            assert _code(ba, lambda: s.covariance(cams=[0], compute=False)) == ba.ERR_ARG  # no result left behind
        s.try_step(1e-6 * dmax)
        s.covariance(1e-3 * dmax, cams=[0])
    # S itself singular with diag S > 0 and every free U_p of full rank: no camera mask, the ill-determined points + 1 % fixed, lambda = 0
    # -- the seven gauge directions.  Nothing but a pivot of the factorisation (k_cov_diag) can refuse this one; either-or as above.
    po21 = CC.sorted_oracle_problem(O, prob21)
    s = ba.Solver(prob21, K, ba.F64)
    _, dmax = s.linearize()
    pf = _ill_points(po21, s.get(ba.GET_JP).reshape(-1, 2, 3)).astype(np.uint8)
    pf[np.random.default_rng(1).choice(prob21.M, prob21.M // 100, replace=False)] = 1
    s.set_constant(None, pf)
    s.linearize()
    assert not _ill_points(po21, s.get(ba.GET_JP).reshape(-1, 2, 3))[pf == 0].any()
    try:
        cc, pp = s.covariance(0.0, cams=np.arange(prob21.N), points=np.flatnonzero(pf == 0)[:50])
        assert np.isfinite(cc).all() and np.isfinite(pp).all()
        print("COV singular[%s,gauge_free] lambda=0 succeeded (roundoff pivots)" % kind)
    except ba.BAError as e:
        assert e.code == ba.ERR_SINGULAR
        print("COV singular[%s,gauge_free] lambda=0 returned BA_ERR_SINGULAR (a pivot of S)" % kind)
    s.try_step(1e-6 * dmax)
    # the unambiguous case: a camera nobody observes -- its diagonal block of S is exactly lambda I.  The ill-determined points (those the
    # removal leaves with one observation among them) are held fixed, so that the camera is the ONLY reason H is not positive definite:
    # with it fixed as well (the control) the same call succeeds.
    pg0 = ba.Problem.synthetic(6, 40, 160, 3)
    a = pg0.arrays()
    keep = a["cam_idx"] != pg0.N - 1
    pg = ba.Problem.from_arrays(pg0.N, pg0.M, int(keep.sum()), a["cam_idx"][keep], a["pt_idx"][keep], a["meas"].reshape(-1, 2)[keep].ravel(),
                                a["cams9"], a["pts"])
    po = CC.sorted_oracle_problem(O, pg)
    s = ba.Solver(pg, K, ba.F64)
    _, dmax = s.linearize()
    pf = _ill_points(po, s.get(ba.GET_JP).reshape(-1, 2, 3)).astype(np.uint8)
    assert 0 < pf.sum() < pg.M - 10
    gm = pg.gauge_mask(0)
    s.set_constant(gm, pf)
    s.linearize()
    s.try_step(1e-3 * dmax)  # (the existing kinds accept a camera without observations at lambda > 0)
    assert _code(ba, lambda: s.covariance(0.0, cams=[0])) == ba.ERR_SINGULAR
    assert _code(ba, lambda: s.covariance(cams=[0], compute=False)) == ba.ERR_ARG  # no result left behind
    ctl = gm.copy()
    ctl[pg.N - 1] = ba.FIX_CAMERA
    if gm[pg.N - 1]:  # (the gauge's scale component sat on the camera nobody observes: hold one of an observed camera instead)
        ctl[pg.N - 2] |= 0x004
    s.set_constant(ctl, pf)
    s.linearize()
    cc, pp = s.covariance(0.0, cams=np.arange(pg.N), points=np.arange(pg.M))  # the control: positive definite without that camera
    assert np.isfinite(cc).all() and np.isfinite(pp).all() and not cc[pg.N - 1].any()
    print("COV singular[%s] unobserved camera: BA_ERR_SINGULAR, and success with that camera fixed" % kind)
    s.set_constant(gm, pf)
    s.linearize()
    lam = 1e-3 * dmax
    cc, _ = s.covariance(lam, cams=[pg.N - 1])
    free = ((int(pg.gauge_mask(0)[pg.N - 1]) >> np.arange(9)) & 1) == 0  # (the gauge's scale component may sit on this camera)
    err = np.abs(cc[0] * lam - np.diag(free.astype(float))).max()
    print("COV singular[%s] unobserved_camera_block %.3e %.1e" % (kind, err, 1e-15))
    assert err <= 1e-15  # (I / lam: one division's rounding per entry, FLOOR_PT)
    s.try_step(lam)
