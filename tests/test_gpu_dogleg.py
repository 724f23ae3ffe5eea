"""GPU: Powell's dogleg for BA_CHOLESKY (ba_solver_dogleg_prepare / ba_solver_try_dogleg / ba_minimize_dogleg) against
tests/dogleg_checks.py in long double on the GPU's OWN J, residuals, gradient and kept Gauss-Newton step (BA_GET_JC / JP / RESIDUALS /
GRAD / DX), as tests/test_gpu_damping.py does for its trial.  Each value is printed as `DOGLEG <case> <metric> <value> <bound>`.

  scalars    q = |J g|^2, |g|^2, |dx_gn|^2, g'dx_gn against the long double sums of the same arrays; bound max(10 x the same sums on the CPU
             in the solver's scalar type with fp64 accumulation, test_gpu_stages.BOUND's floor for a sum of products)
  prepare    BA_GET_DX, xTest, the test energy and rho_scale are ba_solver_try_step(mu)'s bits
  branches   radii 2 |dx_gn|, inf, alpha |g| / 2, sqrt(alpha |g| |dx_gn|) -> branches 0, 0, 1, 2; branch 0 is the prepare bit for bit;
             branches 1, 2: the step per entry, its length, xTest, the test energy, pred
  masks      fixed parameters: zero step, bits kept through try_dogleg + accept
  state      what survives, what invalidates, what is refused, the memory
  driver     ba_minimize_dogleg's rows against a Python loop over the library's own calls (bit for bit) and the fp64 oracle (first row)
  default    ba_minimize behind the dogleg calls returns the rows of a solver that never made them
"""
import math

import numpy as np
import pytest

import dogleg_checks as DG
import stage_checks as SC
from test_gpu_parity import _long_track_problem, _ragged_problem
from test_gpu_stages import BOUND, EPS, sorted_oracle_problem

pytestmark = pytest.mark.gpu

LD = np.longdouble
LAMS = (1e-6, 1e-2)  # x max diag J'J: the stage tests' pair
DT = {0: np.float64, 1: np.float32}
TAG = {0: "f64", 1: "f32"}
ERR_ARG = 4


class Checker:
    def __init__(self, case):
        self.case, self.rows = case, []

    def __call__(self, metric, value, bound):
        self.rows.append((metric, float(value), float(bound)))
        print("DOGLEG %s %s %.3e %.1e" % (self.case, metric, value, bound))

    def done(self):
        bad = [r for r in self.rows if not (r[1] <= r[2])]
        assert not bad, (self.case, bad)


def _lonely_point_problem(ba):
    """synthetic(6, 60, 240) and one more point that nobody observes (ba_problem_create)."""
    p = ba.Problem.synthetic(6, 60, 240, 11)
    a = p.arrays()
    pts = np.concatenate([a["pts"], [0.1, -0.2, 0.3]])
    return ba.Problem.from_arrays(p.N, p.M + 1, p.K, a["cam_idx"], a["pt_idx"], a["meas"], a["cams9"], pts)


PROBLEMS = {
    "tiny": lambda ba, prob21: ba.Problem.synthetic(2, 2, 4, 5),  # a single partial block of every kernel, K << 256
    "ragged": lambda ba, prob21: _ragged_problem(ba),
    "longtrack": lambda ba, prob21: _long_track_problem(ba),
    "lonely": lambda ba, prob21: _lonely_point_problem(ba),
    "p21": lambda ba, prob21: prob21,                             # K = 36 455: 143 blocks of k_jg, the last one partial
}


class Dev:
    """A CHOLESKY solver at its linearisation with its own state, residuals, J and g read back (point-sorted)."""

    def __init__(self, ba, O, pg, scalar, cam_mask=None, pt_fixed=None):
        self.ba, self.scalar, self.pg = ba, scalar, pg
        self.po = po = sorted_oracle_problem(O, pg)
        self.s = s = ba.Solver(pg, ba.CHOLESKY, scalar)
        if cam_mask is not None or pt_fixed is not None:
            s.set_constant(cam_mask, pt_fixed)
        self.e, self.dmax = s.linearize()
        self.cam, self.pts = s.get(ba.GET_CAMS), s.get(ba.GET_POINTS)
        self.f = s.get(ba.GET_RESIDUALS)
        self.Jc, self.Jp = s.get(ba.GET_JC).reshape(po.K, 2, 9), s.get(ba.GET_JP).reshape(po.K, 2, 3)
        self.g = s.get(ba.GET_GRAD)

    def trial_bits(self):
        s, ba = self.s, self.ba
        return s.get(ba.GET_DX), s.get(ba.GET_CAMS_TEST), s.get(ba.GET_POINTS_TEST)

    def working_step(self, a, c, gn):
        """a g + c dx_gn with the coefficients as the kernel receives them (rounded to the solver's scalar type), in long double, and the
        magnitude of its two terms per entry."""
        t = DT[self.scalar]
        a, c = LD(t(a)), LD(t(c))
        g, gn = self.g.astype(LD), np.asarray(gn).astype(LD)
        return a * g + c * gn, np.abs(a * g) + np.abs(c * gn)


def _same(x, y):
    return np.array_equal(np.asarray(x).view(np.uint64), np.asarray(y).view(np.uint64))


def _bits(v):
    return np.float64(v).view(np.uint64)


@pytest.fixture(scope="module")
def problems(ba, prob21):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = PROBLEMS[name](ba, prob21)
        return cache[name]
    return get


CASES = [(n, sc, lam) for n in PROBLEMS for sc in (0, 1) for lam in LAMS]


@pytest.mark.parametrize("name,scalar,rel", CASES, ids=["%s-%s-%.0e" % (n, TAG[sc], lam) for n, sc, lam in CASES])
def test_prepare_scalars_and_branches(ba, O, gpu_ok, problems, name, scalar, rel):
    """Cases 1 - 3 of the module docstring on one prepare.
    Bounds.  Scalars: 10 x the working-precision CPU sums or BOUND[rho_scale] (the floor of a sum of products there: 2e-15 / 1e-6),
    whichever is larger.  The step per entry: fl(fl(a g) + fl(c dx_gn)) has three roundings of half an ulp, each of a quantity no larger
    than |a g| + |c dx_gn|: 2 eps of that sum.  Its length: a and c reach the kernel rounded to the solver's scalar type (eps / 2 each,
    both terms of |dx|^2 = a^2 g2 + 2 a c d + c^2 gn2 positive) on top of the scalars' own error and the root's: 8 eps + BOUND[dx_norm].
    xTest and the test energy: the stage tests' metrics and bounds.  pred: the scalars' rule against 2 g'dx - |J dx|^2 of the device's
    own step, relative to the sum of the magnitudes; the two differ by the residual of the solve behind dx_gn, which the working-precision
    CPU dogleg on the same dx_gn shares: max(10 x its error, BOUND[rho_scale]).
    Measured on an MI355X (profiles/r27_dogleg_tests.txt), worst over the 20 cases, fp64 / fp32: q 1.9e-16 / 2.9e-16 (yardstick 2.5e-16 /
    7.0e-17), g2 1.3e-16 / 1.2e-16, gn2 1.8e-16 / 1.6e-16, d 1.2e-16 / 2.4e-16; the step 0.97 / 0.97 of its 2 eps; |dx| against the radius
    1.8e-16 / 4.4e-8; xTest 0.5 / 0.6 ulp; e_test 1.8e-14 / 6.7e-6; pred 1.8e-16 / 1.8e-8 (yardstick 1.5e-16 / 8.9e-9).  Every problem had
    room for the interpolated branch.  The 30 tests of this file took 1.9 s."""
    ck = Checker("%s[%s]@%.0e" % (name, TAG[scalar], rel))
    d = Dev(ba, O, problems(name), scalar)
    s, po, eps = d.s, d.po, EPS[scalar]
    mu = rel * d.dmax
    # ---- case 2: prepare == try_step(mu)
    e0, rs0, dn0 = s.try_step(mu)
    want = d.trial_bits()
    info = s.dogleg_prepare(mu)
    gn, ct0, pt0 = got = d.trial_bits()
    ck("prepare_bits_differ", sum(0 if _same(x, y) else 1 for x, y in zip(got, want)), 0)
    ck("prepare_energy_bits_differ", int(_bits(info["energy_gn"]) != _bits(e0)) + int(_bits(info["rho_scale_gn"]) != _bits(rs0)), 0)
    assert info["mu"] == mu and info["alpha"] == (info["g2"] / info["q"] if info["g2"] > 0 else 0.0)
    # ---- case 1: the four sums
    ref = DG.Reference(po, d.Jc, d.Jp, d.f, d.g, mu, dx_gn=gn)
    yard = DG.working_scalars(po, d.Jc, d.Jp, d.g, gn, DT[scalar])
    for k, dev_v in (("q", info["q"]), ("g2", info["g2"]), ("gn2", info["gn2"]), ("d", info["g_dot_gn"])):
        want_v = ref.scalars()[k]
        scale = want_v if k != "d" else (np.abs(ref.g) * np.abs(ref.dx_gn)).sum()
        yerr = float(abs(LD(yard[k]) - want_v) / scale)
        ck("%s(yardstick %.1e)" % (k, yerr), float(abs(LD(dev_v) - want_v) / scale), max(10 * yerr, BOUND[("rho_scale", scalar)]))
    # ---- case 3: the branches
    sd, gnn = float(ref.sd_norm), float(ref.gn_norm)
    radii = [(2 * gnn, 0), (math.inf, 0), (0.5 * sd, 1)]
    if sd >= 0.9 * gnn:
        assert name not in ("p21", "p39"), (sd, gnn)  # (tests/test_dogleg_checks.py: reachable there)
        print("DOGLEG %s cauchy/gn %.3e: no room for the interpolated branch, skipped" % (ck.case, sd / gnn))
    else:
        radii.append((math.sqrt(sd * gnn), 2))
    for radius, branch in radii:
        e, pred, dn, br = s.try_dogleg(radius)
        tag = "b%d" % branch if radius != math.inf else "b0inf"
        ck(tag + "_branch_differs", abs(br - branch), 0)
        dx, ct, pt = got = d.trial_bits()
        if branch == 0:
            ck(tag + "_bits_differ", sum(0 if _same(x, y) else 1 for x, y in zip(got, (gn, ct0, pt0))) + int(_bits(e) != _bits(e0)), 0)
            continue
        a, c, cbr, cpred = ba.dogleg_coefficients(info["g2"], info["q"], info["gn2"], info["g_dot_gn"], mu, radius)
        assert cbr == br and _bits(cpred) == _bits(pred)
        step, mag = d.working_step(a, c, gn)
        ck(tag + "_dx_ulps", float(SC._ratio(np.abs(dx.astype(LD) - step).astype(np.float64), (eps * mag).astype(np.float64)).max()), 2.0)
        ck(tag + "_dx_norm_is_radius", abs(dn - radius) / radius, 8 * eps + BOUND[("dx_norm", scalar)])
        ck(tag + "_dx_norm_of_dx", abs(dn - float(np.sqrt((dx.astype(LD) ** 2).sum()))) / dn, BOUND[("dx_norm", scalar)])
        ck(tag + "_retract", SC.retraction_ulps(po, d.cam, d.pts, dx, ct, pt, eps), BOUND[("retract", scalar)])
        e_ref = O.referee_energy(po, ct, pt)
        ck(tag + "_e_test", abs(e - e_ref) / e_ref, BOUND[("e_test", scalar)])
        # pred: the device's against the direct form on its own step; the yardstick: the same rule on the working-precision sums
        y = DG.j_times(po, d.Jc, d.Jp, dx)
        scale = 2 * (np.abs(ref.g) * np.abs(dx.astype(LD))).sum() + (y * y).sum()
        wa, wc, _, wpred = DG.coefficients(yard["g2"], yard["q"], yard["gn2"], yard["d"], mu, radius, np.float64)
        wstep = LD(wa) * ref.g + LD(wc) * ref.dx_gn
        wy = DG.j_times(po, d.Jc, d.Jp, wstep)
        wscale = 2 * (np.abs(ref.g) * np.abs(wstep)).sum() + (wy * wy).sum()
        yerr = float(abs(LD(wpred) - ref.pred_direct(wstep)) / wscale)
        ck(tag + "_pred(yardstick %.1e)" % yerr, float(abs(LD(pred) - ref.pred_direct(dx)) / scale), max(10 * yerr, BOUND[("rho_scale", scalar)]))
    ck.done()


@pytest.mark.parametrize("scalar", [0, 1], ids=["f64", "f32"])
def test_masks(ba, O, gpu_ok, scalar):
    """The gauge mask plus three fixed points on synthetic(8, 400, 1500): in every branch the step of a fixed parameter is exactly 0,
    the other entries are a g + c dx_gn to 2 eps of |a g| + |c dx_gn|, and through try_dogleg + accept a fixed value keeps its bits, the nine
    entries of R of the omega-fixed camera included."""
    ck = Checker("masks[%s]" % TAG[scalar])
    pg = ba.Problem.synthetic(8, 400, 1500, 3)
    cm = pg.gauge_mask(0)
    pf = np.zeros(pg.M, np.uint8)
    pf[[0, 5, 17]] = 1
    d = Dev(ba, O, pg, scalar, cm, pf)
    s, po, eps = d.s, d.po, EPS[scalar]
    fixed = np.concatenate([np.repeat(pf != 0, 3), ((cm[:, None] >> np.arange(9)[None, :]) & 1).astype(bool).reshape(-1)])
    assert fixed.sum() == 9 + 7
    cam_fixed = np.zeros((pg.N, 15), bool)  # the slots of GET_CAMS a camera mask holds: R for omega, T, f k1 k2
    for a in range(pg.N):
        m = int(cm[a])
        cam_fixed[a, :9] = (m & ba.FIX_OMEGA) != 0
        for q in range(3):
            cam_fixed[a, 9 + q] = (m >> q) & 1
            cam_fixed[a, 12 + q] = (m >> (6 + q)) & 1
    mu = 1e-6 * d.dmax
    info = s.dogleg_prepare(mu)
    gn = s.get(ba.GET_DX)
    ck("grad_on_fixed", float(np.abs(d.g[fixed]).max()), 0)
    ref = DG.Reference(po, d.Jc, d.Jp, d.f, d.g, mu, dx_gn=gn)
    sd, gnn = float(ref.sd_norm), float(ref.gn_norm)
    assert sd < 0.9 * gnn
    for radius, branch in ((math.inf, 0), (0.5 * sd, 1), (math.sqrt(sd * gnn), 2)):
        e, pred, dn, br = s.try_dogleg(radius)
        assert br == branch
        dx, ct, pt = d.trial_bits()
        ck("b%d_step_on_fixed" % branch, float(np.abs(dx[fixed]).max()), 0)
        ck("b%d_fixed_points_moved" % branch, 0 if _same(pt.reshape(-1, 3)[pf != 0], d.pts.reshape(-1, 3)[pf != 0]) else 1, 0)
        ck("b%d_fixed_camera_slots_moved" % branch, 0 if _same(ct.reshape(-1, 15)[cam_fixed], d.cam.reshape(-1, 15)[cam_fixed]) else 1, 0)
        a, c, _, _ = ba.dogleg_coefficients(info["g2"], info["q"], info["gn2"], info["g_dot_gn"], mu, radius)
        step, mag = d.working_step(a, c, gn)
        free = ~fixed
        ck("b%d_dx_ulps" % branch, float(SC._ratio(np.abs(dx.astype(LD) - step).astype(np.float64)[free], (eps * mag).astype(np.float64)[free]).max()), 2.0)
        ck("b%d_retract" % branch, SC.retraction_ulps(po, d.cam, d.pts, dx, ct, pt, eps), BOUND[("retract", scalar)])
    s.accept()
    cam1, pts1 = s.get(ba.GET_CAMS), s.get(ba.GET_POINTS)
    ck("accepted_is_xtest", 0 if _same(cam1, ct) and _same(pts1, pt) else 1, 0)
    ck("fixed_bits_lost", 0 if _same(cam1.reshape(-1, 15)[cam_fixed], d.cam.reshape(-1, 15)[cam_fixed])
       and _same(pts1.reshape(-1, 3)[pf != 0], d.pts.reshape(-1, 3)[pf != 0]) else 1, 0)
    ck("free_moved", 0 if not _same(pts1, d.pts) else 1, 0)
    ck.done()


def _refused(ba, fn, *args):
    with pytest.raises(ba.BAError) as ei:
        fn(*args)
    assert ei.value.code == ERR_ARG, ei.value


def test_state_survives_and_goes_stale(ba, O, gpu_ok):
    """A try_step between prepare and try_dogleg does not change try_dogleg's bits; every call that makes a pending step or a covariance
    stale makes the prepared dogleg stale (try_dogleg: BA_ERR_ARG); the buffers are allocated by the first prepare and counted."""
    pg = ba.Problem.synthetic(8, 400, 1500, 3)
    s = ba.Solver(pg, ba.CHOLESKY, ba.F64)
    before = s.device_bytes()
    _, dmax = s.linearize()
    mu = 1e-6 * dmax
    info = s.dogleg_prepare(mu)
    n = 3 * pg.M + 9 * pg.N
    grew = 8 * n + 8 * ((pg.K + 255) // 256 + 3 * ((n + 255) // 256) + (pg.M + 255) // 256 + 1 + 8)
    assert s.device_bytes() - before == grew
    radius = 0.5 * math.sqrt(info["gn2"])

    def bits():
        out = s.try_dogleg(radius)
        return out, s.get(ba.GET_DX), s.get(ba.GET_CAMS_TEST), s.get(ba.GET_POINTS_TEST)
    r0 = bits()
    assert r0[0][3] in (1, 2)
    s.try_step(1e-3)
    s.try_step(mu)
    r1 = bits()
    assert r0[0] == r1[0] and all(_same(x, y) for x, y in zip(r0[1:], r1[1:]))
    s.dogleg_prepare(mu)
    assert s.device_bytes() - before == grew  # (once)
    r2 = bits()
    assert r0[0] == r2[0] and all(_same(x, y) for x, y in zip(r0[1:], r2[1:]))

    def again():
        s.linearize()
        s.dogleg_prepare(mu)
        s.try_dogleg(radius)
    cam, pts = s.get(ba.GET_CAMS), s.get(ba.GET_POINTS)
    stale = [
        ("linearize", lambda: s.linearize()),
        ("accept", lambda: s.accept()),
        ("set_state", lambda: s.set_state(cam, pts)),
        ("minimize", lambda: s.minimize(max_trials=1)),
        ("minimize_dogleg", lambda: s.minimize_dogleg(max_trials=1)),
        ("set_constant", lambda: s.set_constant(pg.gauge_mask(0), None)),
        ("set_loss", lambda: s.set_loss(ba.LOSS_HUBER, 1.0)),
        ("set_obs_weights", lambda: s.set_obs_weights(np.full(pg.K, 2.0))),
    ]
    for what, call in stale:
        again()
        call()
        with pytest.raises(ba.BAError) as ei:
            s.try_dogleg(radius)
        assert ei.value.code == ERR_ARG, what
    again()  # (and the mask, the loss and the weights of the last three are in force and legal)
    assert s.device_bytes() > before + grew  # (the mask and the weights; the dogleg's buffers still once)


def test_refusals_leave_the_solver_alone(ba, O, gpu_ok):
    """Everything the header lists under BA_ERR_ARG, and behind all of it on the CHOLESKY solver the bits of a try_step of a solver that
    never saw a dogleg call."""
    pg = ba.Problem.synthetic(8, 400, 1500, 3)
    for kind in (ba.QRCHOL, ba.ITERSCHUR):
        o = ba.Solver(pg, kind, ba.F64)
        o.linearize()
        _refused(ba, o.dogleg_prepare, 1e-3)
        _refused(ba, o.try_dogleg, 1.0)
        _refused(ba, o.minimize_dogleg)
    sh = ba.Solver(pg, ba.CHOLESKY, ba.F64, shard_rank=0, shard_world=2)  # (refused on the host: no collective is ever reached)
    _refused(ba, sh.dogleg_prepare, 1e-3)
    _refused(ba, sh.minimize_dogleg)
    s = ba.Solver(pg, ba.CHOLESKY, ba.F64)
    _refused(ba, s.dogleg_prepare, 1e-3)  # no linearisation yet
    _refused(ba, s.try_dogleg, 1.0)
    _, dmax = s.linearize()
    mu = 1e-6 * dmax
    _refused(ba, s.try_dogleg, 1.0)  # no prepare
    for bad in (0.0, -1.0, math.nan, math.inf):
        _refused(ba, s.dogleg_prepare, bad)
    s.dogleg_prepare(mu)
    for bad in (0.0, -1.0, math.nan):
        _refused(ba, s.try_dogleg, bad)
    for bad in (dict(radius_init=-1.0), dict(radius_init=math.nan), dict(radius_min=0.0), dict(radius_max=0.0), dict(mu_rel=0.0),
                dict(mu_rel_max=-1.0), dict(tol_fun=0.0)):
        _refused(ba, lambda kw=bad: s.minimize_dogleg(**kw))
    # Marquardt's damping in force
    s.set_damping(ba.DAMP_MARQUARDT)
    _refused(ba, s.dogleg_prepare, mu)
    _refused(ba, s.try_dogleg, 1.0)
    _refused(ba, s.minimize_dogleg)
    s.set_damping(ba.DAMP_IDENTITY)
    # priors, relative poses: refused while they are set, legal again once they are removed
    s.set_point_priors([3], [[0.0, 0.0, 1.0]], sigma=1.0)
    s.linearize()
    _refused(ba, s.dogleg_prepare, mu)
    _refused(ba, s.minimize_dogleg)
    s.set_point_priors([], np.zeros((0, 3)), sigma=1.0)
    R, t = ba.relative_pose(s.get(ba.GET_CAMS), 0, 1)
    s.set_relative_poses([[0, 1]], [R], [t], sigma_rot=0.1, sigma_trans=0.1)
    s.linearize()
    _refused(ba, s.dogleg_prepare, mu)
    _refused(ba, s.minimize_dogleg)
    s.set_relative_poses(np.zeros((0, 2), np.int32), np.zeros((0, 3, 3)), np.zeros((0, 3)))
    _refused(ba, s.dogleg_prepare, mu)  # a measurement model pending: no valid linearisation
    s.linearize()
    # a mask pending
    s.dogleg_prepare(mu)
    s.set_constant(pg.gauge_mask(0), None)
    _refused(ba, s.dogleg_prepare, mu)
    _refused(ba, s.try_dogleg, 1.0)
    s.set_constant(None, None)
    s.linearize()
    et = s.try_step(mu)
    got = s.get(ba.GET_DX), s.get(ba.GET_CAMS_TEST), s.get(ba.GET_POINTS_TEST)
    f = ba.Solver(pg, ba.CHOLESKY, ba.F64)
    f.linearize()
    assert f.try_step(mu) == et
    assert all(_same(x, y) for x, y in zip(got, (f.get(ba.GET_DX), f.get(ba.GET_CAMS_TEST), f.get(ba.GET_POINTS_TEST))))


class GpuCalls:
    """dogleg_checks.drive's four calls on the library's own."""

    def __init__(self, ba, s):
        self.ba, self.s = ba, s
        self.linearize, self.prepare, self.try_dogleg, self.accept = s.linearize, s.dogleg_prepare, s.try_dogleg, s.accept
        self.coefficients = ba.dogleg_coefficients


DRIVER = [("p21", 0), ("p21", 1), ("p39", 0)]


@pytest.mark.parametrize("name,scalar", DRIVER, ids=["%s-%s" % (n, TAG[sc]) for n, sc in DRIVER])
def test_driver_rows(ba, O, gpu_ok, prob21, prob39, name, scalar):
    """ba_minimize_dogleg with max_trials = 12: every row (iteration, accepted, f, rho, radius; e_test enters through rho and through the
    final energy) and the result are bit-equal to dogleg_checks.drive over linearize / dogleg_prepare / try_dogleg / accept of a second
    solver.  fp64: the first row's energy (to test_gpu_parity's 1e-6) and acceptance are the CPU reference driver's on the oracle."""
    pg = prob21 if name == "p21" else prob39
    res, rows = ba.Solver(pg, ba.CHOLESKY, scalar).minimize_dogleg(max_trials=12)
    loop = DG.drive(GpuCalls(ba, ba.Solver(pg, ba.CHOLESKY, scalar)), max_trials=12)
    for r in rows:
        print("DOGLEG driver[%s,%s] iter %d accepted %d f %.17g rho %.6g radius %.6g" % (name, TAG[scalar], r[0], r[1], r[2], r[3], r[4]))
    assert len(rows) == 12 == res["trials"] and res["status"] == DG.RUNNING
    assert np.array_equal(rows[:, :5].view(np.uint64), loop["rows"][:, :5].view(np.uint64)), (rows[:, :5], loop["rows"][:, :5])
    for k in ("status", "iterations", "trials", "fun_evals"):
        assert res[k] == loop[k], k
    assert _bits(res["energy"]) == _bits(loop["energy"]) and _bits(res["radius"]) == _bits(loop["radius"])
    assert rows[:, 1].sum() >= 1 and res["energy"] < rows[0, 2]
    if scalar == 0:
        from conftest import to_oracle
        ora = DG.drive(DG.OracleCalls(O, to_oracle(pg)), max_trials=1)["rows"]
        assert ora[0, 1] == rows[0, 1] and abs(ora[0, 2] - rows[0, 2]) <= 1e-6 * ora[0, 2], (ora[0], rows[0])


def test_driver_runs_to_its_stop(ba, gpu_ok, prob21):
    """problem-21, fp64, to the driver's own stop: BA_SUCCESS and a final energy below the initial one.  No bound on the final cost: the
    trajectory is chaotic (README, the ensemble section)."""
    res, rows = ba.Solver(prob21, ba.CHOLESKY, ba.F64).minimize_dogleg()
    print("DOGLEG stop[p21] status %d trials %d iterations %d fun_evals %d energy %.9g radius %.3g seconds %.3f"
          % (res["status"], res["trials"], res["iterations"], res["fun_evals"], res["energy"], res["radius"], res["seconds"]))
    assert res["status"] == DG.SUCCESS and res["energy"] < rows[0, 2] and res["trials"] == len(rows)


@pytest.mark.parametrize("scalar", [0, 1], ids=["f64", "f32"])
def test_default_path_is_untouched(ba, gpu_ok, prob21, scalar):
    """A CHOLESKY solver that has used the dogleg calls and then runs ba_minimize returns the rows of a solver that never did."""
    a = ba.Solver(prob21, ba.CHOLESKY, scalar)
    _, dmax = a.linearize()
    info = a.dogleg_prepare(1e-6 * dmax)
    a.try_dogleg(0.5 * math.sqrt(info["gn2"]))
    a.try_dogleg(math.inf)
    ra = a.minimize(max_trials=8)
    rb = ba.Solver(prob21, ba.CHOLESKY, scalar).minimize(max_trials=8)
    assert np.array_equal(ra["trace"][:, :5].view(np.uint64), rb["trace"][:, :5].view(np.uint64))
    assert _bits(ra["energy"]) == _bits(rb["energy"]) and ra["status"] == rb["status"]
