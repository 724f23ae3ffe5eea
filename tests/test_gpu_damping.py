"""GPU: Marquardt's damping lambda diag(J'J) (ba_solver_set_damping) against tests/damping_checks.py.

The reference is the long double trial of damping_checks.py on the GPU's OWN J, residuals and gradient, so each stage is measured on its
own inputs with the metrics and the bounds of the identity-damping stage tests (d = fl(lambda clamp(diag)) in place of lambda):

  CHOLESKY    S, rhs (assembly metric; bound max(10 x the working-precision CPU trial on the same J, test_gpu_stages.BOUND)), eta of the
              step in the GPU's own S and rhs, the back-substitution with U_p + diag(d_p), rho_scale against dx'(d o dx + g) of the GPU's
              own dx and g; the replayed graph of ba_minimize against eager try_step bit for bit (the elimination is a launch of its own
              under Marquardt: the fused linearisation's records are not used)
  ITERSCHUR   x_1 ... x_7 of capped solves against pcg_checks.pcg on the reference S with the reference block inverses, the device's
              residual against quad (test_gpu_pcg_stages' rule and FLOOR); the converged step under both forests and with groups of
              shared intrinsics against the dense solve
  clamps, masks, priors and relative poses, the default path bit for bit, ba_minimize's lambda, refusals and state.

lambda is dimensionless here: 1e-6 and 1e-2.  Each value is printed as `DAMP <case> <metric> <value> <bound>`.
"""
import hashlib

import numpy as np
import pytest

import damping_checks as DC
import forest_checks as FC
import pcg_checks as PC
import prior_checks as PR
import relpose_checks as RC
import shared_checks as SH
import stage_checks as SC
from test_gpu_parity import _long_track_problem, _ragged_problem
from test_gpu_pcg_stages import FLOOR, KS, quad_rel_residual
from test_gpu_stages import BOUND, EPS, _synthetic, sorted_oracle_problem

pytestmark = pytest.mark.gpu

LD = np.longdouble
DT = {0: np.float64, 1: np.float32}
SN = {0: "f64", 1: "f32"}
LAMS = (1e-6, 1e-2)
# The converged solves (the forests, shared intrinsics, masks).  In fp32 lambda = 1e-6 is 8 eps32 of every diagonal entry: the damping that
# makes problem-21's seven gauge directions definite is then below the rounding of the matrix-free product V p - (the eliminated part)
# (test_gpu_pcg_stages.LAMS_MOVED's finding), neither the device nor the fp32 CPU yardstick converges in any number of iterations, and a
# bound from that yardstick says nothing.  The fp32 cases take 1e-3 for it; the capped iterates of test_pcg_iterates keep both lambdas.
LAMS_CONVERGED = {0: (1e-6, 1e-2), 1: (1e-3, 1e-2)}
TIGHT = {0: 1e-13, 1: 1e-6}  # rel_tol of the converged solves (test_gpu_shared_intrinsics.py's)
CAP = 1000
CAP_SHARED = 20000  # problem-21 with shared intrinsics and no gauge fixed, lambda = 1e-6: block Jacobi needs thousands of iterations


class Checker:
    def __init__(self, case):
        self.case, self.rows = case, []

    def __call__(self, metric, value, bound):
        self.rows.append((metric, float(value), float(bound)))
        print("DAMP %s %s %.3e %.1e" % (self.case, metric, value, bound))

    def done(self):
        bad = [r for r in self.rows if not (r[1] <= r[2])]
        assert not bad, (self.case, bad)


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def problem(ba, name, prob21):
    return {"p21": lambda: prob21, "ragged": lambda: _ragged_problem(ba), "longtracks": lambda: _long_track_problem(ba),
            "syn2": lambda: _synthetic(ba, 2)}[name]()


_REF = {}


class Dev:
    """A solver under Marquardt's damping at its linearisation, its own J, residuals and gradient read back (point-sorted), and the
    reference / working-precision trials on them (cached per input and lambda: the fp64 cases of one problem share them)."""

    def __init__(self, ba, O, pg, kind, scalar, setup=None, bounds=(0.0, 0.0), adds=None):
        self.ba, self.O, self.scalar, self.kind = ba, O, scalar, kind
        self.po = po = sorted_oracle_problem(O, pg)
        self.s = s = ba.Solver(pg, kind, scalar)
        if setup is not None:
            setup(s)
        s.set_damping(ba.DAMP_MARQUARDT, *bounds)
        _, self.dmin, self.dmax = s.damping()
        if kind == ba.CHOLESKY:
            s.keep_intermediates(True)
        self.e, _ = s.linearize()
        self.Jc, self.Jp = s.get(ba.GET_JC).reshape(po.K, 2, 9), s.get(ba.GET_JP).reshape(po.K, 2, 3)
        self.f, self.g = s.get(ba.GET_RESIDUALS), s.get(ba.GET_GRAD)
        self.adds = adds(self) if adds is not None else {}
        self.key = hashlib.sha1(b"".join(np.ascontiguousarray(x).tobytes() for x in (po.cam_idx, po.pt_idx, self.Jc, self.Jp, self.f, self.g))
                                + repr((self.dmin, self.dmax, sorted(self.adds))).encode()).hexdigest()

    def trial(self, lam, dtype=LD, groups=None, want_step=True):
        k = (self.key, lam, np.dtype(dtype).name, None if not groups else tuple(len(m) for m in groups), want_step)
        if k not in _REF:
            if len(_REF) > 6:
                _REF.clear()
            _REF[k] = DC.trial(self.po, self.Jc, self.Jp, self.f, lam, dmin=self.dmin, dmax=self.dmax, dtype=dtype, g=self.g, groups=groups,
                               round_to=None if dtype is LD else dtype, want_step=want_step, **self.adds)
        return _REF[k]

    def assembly_yardstick(self, lam, ref):
        """The assembly metric of the working-precision CPU trial on the same J (fp32 that breaks down: fp64 scaled by eps32 / eps64,
        test_gpu_stages.py's rule)."""
        def err(dt):
            y = self.trial(lam, dt, want_step=False)
            return DC.assembly_errors(self.po, self.Jc, self.Jp, self.f, ref["d_c"], y["S"], y["rhs"], ref["S"], ref["rhs"], ref["diag_c"])
        out = err(DT[self.scalar])
        if not all(np.isfinite(v) for v in out.values()):
            out = {k: v * EPS[1] / EPS[0] for k, v in err(np.float64).items()}
        return out

    def pcg_yardstick(self, lam, run):
        """run(w, dtype) on the WORKING-PRECISION trial w of the same J (S, rhs, B, Vd eliminated and assembled in the solver's scalar type,
        handed on in long double) -- the yardstick of the identity-damping tests forms them from the quad assembly, which has no rounding
        of the elimination in it; under Marquardt every point block is as badly conditioned as 1 / lambda allows, and that rounding is
        what an iterate inherits first (the test's docstring has both numbers).  fp32 that breaks down: fp64 scaled by eps32 / eps64.
        Returns (result, scale, dtype, w)."""
        for dt, scale in ((DT[self.scalar], 1.0), (np.float64, EPS[1] / EPS[0])):
            w = self.trial(lam, dt, want_step=False)
            if all(np.all(np.isfinite(np.asarray(w[k], np.float64))) for k in ("S", "rhs", "B")):
                w = {k: np.asarray(w[k]).astype(LD) for k in ("S", "rhs", "B", "Vd")}
                out = run(w, dt)
                if out is not None:
                    return out, scale, dt, w
            if dt is np.float64:
                break
        raise AssertionError("the fp64 yardstick broke down")

    def device_damping(self, lam, ref):
        """d as the kernels form it: lambda, the bounds and the product in the solver's scalar type, from the reference diagonal."""
        diag = np.concatenate([ref["diag_p"], ref["diag_c"]])
        return DC.damping(diag, lam, DC.MARQUARDT, self.dmin, self.dmax, round_to=DT[self.scalar])


def check_cholesky_trial(ck, dev, lam, tag=""):
    """One try_step of a CHOLESKY solver under Marquardt: assembly, factor + sweep, back-substitution, rho_scale.  Returns (dx, ref)."""
    ba, s, po, sc = dev.ba, dev.s, dev.po, dev.scalar
    et, rs, dn = s.try_step(lam)
    dx, S, rhs = s.get(ba.GET_DX), s.get(ba.GET_S), s.get(ba.GET_RHS)
    ref = dev.trial(lam, want_step=False)
    yd = dev.assembly_yardstick(lam, ref)
    got = DC.assembly_errors(po, dev.Jc, dev.Jp, dev.f, ref["d_c"], S, rhs, ref["S"], ref["rhs"], ref["diag_c"])
    for k in ("S", "rhs"):
        ck("%s%s@%.0e(yardstick %.1e)" % (k, tag, lam, yd[k]), got[k], max(10 * yd[k], BOUND[(k, sc)]))
    ck("eta%s@%.0e" % (tag, lam), SC.eta(S, dx[3 * po.M:], rhs), BOUND[("eta", sc)])
    d = dev.device_damping(lam, ref)
    ck("backsub%s@%.0e" % (tag, lam), DC.backsub_errors(po, dev.Jc, dev.Jp, dx, dev.g, d[:3 * po.M], dev.adds.get("add_U")), BOUND[("backsub", sc)])
    ck("rho_scale%s@%.0e" % (tag, lam), DC.rho_scale_error(rs, dx, d, dev.g), BOUND[("rho_scale", sc)])
    ck("dx_norm%s@%.0e" % (tag, lam), abs(dn - np.linalg.norm(dx)) / np.linalg.norm(dx), BOUND[("dx_norm", sc)])
    return dx, ref


# ---- CHOLESKY ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scalar", [0, 1], ids=["f64", "f32"])
@pytest.mark.parametrize("prob", ["p21", "ragged", "longtracks", "syn2"])
def test_cholesky_stages(ba, O, gpu_ok, prob21, prob, scalar):
    """S, rhs, the step, the back-substitution and rho_scale of a CHOLESKY trial under Marquardt at lambda = 1e-6 and 1e-2, each on its
    own inputs with the identity case's bounds (module docstring).  At lambda = 1e-6 a point block U_p + lambda D_p has a scaled condition
    number of up to 3 / lambda and the elimination's rounding is amplified where identity's lambda0 I was not, so S and rhs need more than
    BOUND's floors there; the bound is then 10 x the working-precision CPU trial on the same J.  Measured on an MI355X
    (profiles/r20_damping_tests.txt), device / CPU trial, every case above its floor (all at lambda = 1e-6):
      S   (floor 1e-14 / 1e-5)   fp64 problem-21 4.0e-14 / 2.0e-14, ragged 6.7e-15 / 1.2e-14, long tracks 8.6e-16 / 1.6e-15, N = 2 1.8e-15 / 1.8e-15;
                                 fp32 problem-21 2.9e-5 / 3.1e-5, ragged 1.6e-6 / 2.2e-6
      rhs (floor 5e-15 / 5e-6)   fp64 problem-21 4.8e-14 / 5.4e-14, ragged 4.1e-16 / 7.6e-16, N = 2 3.8e-15 / 4.1e-15;
                                 fp32 problem-21 2.0e-5 / 1.2e-5, N = 2 5.0e-7 / 6.6e-7
    eta 1.1e-16 / 7.7e-8, back-substitution 2.5e-16 / 1.7e-7, rho_scale 8.9e-17 / 2.7e-8: inside the identity bounds."""
    ck = Checker("cholesky[%s,%s]" % (prob, SN[scalar]))
    dev = Dev(ba, O, problem(ba, prob, prob21), ba.CHOLESKY, scalar)
    for lam in LAMS:
        dx, _ = check_cholesky_trial(ck, dev, lam)
        if prob == "ragged":  # the blind camera and the point nobody observes: lambda diag_min on their blocks, no step
            ck("blind_camera_moved@%.0e" % lam, np.count_nonzero(dx[3 * dev.po.M + 45:3 * dev.po.M + 54]), 0)
            ck("empty_point_moved@%.0e" % lam, np.count_nonzero(dx[3 * 77:3 * 77 + 3]), 0)
    ck.done()


@pytest.mark.parametrize("kind_name,scalar,fused", [("CHOLESKY", 0, True), ("CHOLESKY", 0, False), ("CHOLESKY", 1, False), ("CHOLESKY", 1, True),
                                                    ("ITERSCHUR", 0, True), ("ITERSCHUR", 0, False), ("ITERSCHUR", 1, False), ("ITERSCHUR", 1, True)])
def test_replayed_graph_equals_eager_trials(ba, gpu_ok, prob21, monkeypatch, kind_name, scalar, fused):
    """ba_minimize's captured trial (behind the first linearisation, and behind an accepted step, where the fused linearisation has left
    lambda I records that a Marquardt trial must not use) against the eager seam: xTest and dx of trials 1 and 2, bit for bit.  The
    elimination is a launch of its own either way; `fused` is the linearisation in front of trial 2 (BA_NO_FUSE=1: the separate
    launches).  The fused fp32 linearisation is not bit-equal to the separate launches under identity damping either (measured: trial
    2's xTest differs with the feature switched off, and agrees with BA_NO_FUSE=1), so fp32 behind the fused linearisation compares
    trial 1 bit for bit and trial 2 through the energy at its trial point -- evaluated by one fresh solver at both xTest -- at
    test_gpu_stages' bound for the test energy in fp32 (the energy is stationary to first order in what the two linearisations'
    rounding moves of the step)."""
    if fused:
        monkeypatch.delenv("BA_NO_FUSE", raising=False)
    else:
        monkeypatch.setenv("BA_NO_FUSE", "1")
    kind = getattr(ba, kind_name)
    lam0 = 1e-4
    b = ba.Solver(prob21, kind, scalar)
    b.set_damping(ba.DAMP_MARQUARDT)
    rows = b.minimize(max_trials=1, lambda_init=lam0)["trace"]
    a = ba.Solver(prob21, kind, scalar)
    a.set_damping(ba.DAMP_MARQUARDT)
    a.linearize()
    a.try_step(lam0)
    for what in (ba.GET_CAMS_TEST, ba.GET_POINTS_TEST, ba.GET_DX):
        assert np.array_equal(bits(a.get(what)), bits(b.get(what))), (kind_name, what, 1)
    assert rows[0, 1] == 1, rows  # (the case needs an accepted first trial: the second is then behind the fused linearisation)
    c = ba.Solver(prob21, kind, scalar)
    c.set_damping(ba.DAMP_MARQUARDT)
    rows2 = c.minimize(max_trials=2, lambda_init=lam0)["trace"]
    assert np.array_equal(rows2[0, :5], rows[0, :5])
    a.accept()
    a.linearize()
    a.try_step(rows[0, 4])  # (an accepted row carries the lambda of the next trial)
    if scalar == 1 and fused:
        d = ba.Solver(prob21, kind, scalar)
        en = []
        for s in (a, c):
            d.set_state(s.get(ba.GET_CAMS_TEST), s.get(ba.GET_POINTS_TEST))
            en.append(d.linearize()[0])
        print("DAMP graph[%s,f32,fused] e_test eager %.9g graph %.9g relative %.3e bound %.1e" % (kind_name, en[0], en[1], abs(en[0] - en[1]) / en[0],
                                                                                                  BOUND[("e_test", 1)]))
        assert abs(en[0] - en[1]) <= BOUND[("e_test", 1)] * en[0], en
        return
    for what in (ba.GET_CAMS_TEST, ba.GET_POINTS_TEST, ba.GET_DX):
        assert np.array_equal(bits(a.get(what)), bits(c.get(what))), (kind_name, what, 2)


# ---- ITERSCHUR ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scalar", [0, 1], ids=["f64", "f32"])
@pytest.mark.parametrize("prob", ["p21", "ragged", "longtracks", "syn2"])
def test_pcg_iterates(ba, O, gpu_ok, prob21, prob, scalar):
    """x_k, k = 1, 2, 3, 4, 7, of capped block-Jacobi solves against the long double PCG on the reference S with the reference block
    inverses, and the device's residual under a cap against quad: test_gpu_pcg_stages' rule, max(10 x the working-precision yardstick
    in the matrix-free form, FLOOR).  The yardstick is the working-precision CPU trial of the same J -- S, rhs and B_a eliminated and
    assembled in the solver's scalar type -- under the same PCG (Dev.pcg_yardstick): the identity tests form theirs from the quad
    assembly, which has none of the elimination's rounding in it, and at lambda = 1e-6 that rounding is what an iterate inherits first.
    Measured on an MI355X (profiles/r20_damping_tests.txt), worst iterate per case at lambda = 1e-6, device / yardstick (floor 6e-13 /
    3e-3): fp64 problem-21 x_2 2.0e-11 / 5.8e-10, ragged x_4 4.8e-13 / 1.4e-12, long tracks x_7 4.6e-12 / 1.8e-12, N = 2 x_7 5.3e-11 /
    3.2e-11; fp32 problem-21 x_2 7.7e-3 / 7.8e-2, ragged x_3 2.8e-4 / 5.6e-4, long tracks x_7 2.3e-3 / 1.2e-3, N = 2 x_7 2.7e-2 / 6.7e-2.
    The residual under a cap (floor 2e-13 / 2e-4): fp64 ragged 7.5e-15 / 2.4e-14, N = 2 2.6e-10 / 7.0e-10; fp32 problem-21 2.5e-5 / 2.9e-5,
    N = 2 4.5e-2 / 1.9e-2.  In fp32 lambda = 1e-6 is 8 eps32 of every diagonal entry: the yardsticks of 7.8e-2 and 6.7e-2 say that the
    fp32 CPU trial itself has all but broken down there (test_gpu_pcg_stages.LAMS_MOVED's finding), and those bounds check little.  At
    lambda = 1e-2 every case is at its floor."""
    ck = Checker("pcg[%s,%s]" % (prob, SN[scalar]))
    dev = Dev(ba, O, problem(ba, prob, prob21), ba.ITERSCHUR, scalar)
    s, po, dt = dev.s, dev.po, DT[scalar]
    gc = dev.g[3 * po.M:]
    for q, lam in enumerate(LAMS):
        ref = dev.trial(lam, want_step=False)
        S_ld, rhs, S64 = ref["S"], ref["rhs"], ref["S"].astype(np.float64)
        Minv, ok = PC.invert_blocks(ref["B"])
        assert ok.all()
        want = PC.pcg(S_ld, rhs, Minv, max(KS), keep=KS)
        yard, scale, ydt, yV = dev.pcg_yardstick(lam, lambda w, t: PC.yardstick(w["S"], w["rhs"], w["B"], max(KS), dtype=t, keep=KS, V=w["Vd"], g=gc))
        for k in KS:
            s.set_pcg(k, 1e-30)
            s.try_step(lam)
            st = s.pcg_stats()
            xk = s.get(ba.GET_DX)[3 * po.M:]
            yerr = scale * PC.iterate_error(yard["xs"][k], want["xs"][k], S64)
            ck("x%d@%.0e(yardstick %.1e, worst camera %d)" % (k, lam, yerr, PC.worst_camera(xk, want["xs"][k], S64)),
               PC.iterate_error(xk, want["xs"][k], S64), max(10 * yerr, FLOOR[("iterate", scalar)]))
            ck("x%d_capped@%.0e" % (k, lam), 0 if (st["last_iters"] == k and st["last_converged"] == 0) else 1, 0)
            if k in (1, 3) and q == 0:
                quad = quad_rel_residual(O, S64, xk, rhs.astype(np.float64))
                yk = yard["xs"][k].astype(np.float64)
                yq = quad_rel_residual(O, S64, yk, rhs.astype(np.float64))
                yr = scale * abs(PC.working_residual(yV["S"], yk, yV["rhs"], ydt, V=yV["Vd"]) - yq) / yq
                ck("residual%d@%.0e(quad %.3e, yardstick %.1e)" % (k, lam, quad, yr), abs(st["last_rel_residual"] - quad) / quad,
                   max(10 * yr, FLOOR[("residual", scalar)]))
    ck.done()


def converged_step(ck, dev, lam, groups=None, tag="", cap=CAP, run=None):
    """A solve at TIGHT against the dense solve of the reference system (with groups: P y); bound max(10 x the working-precision PCG at
    the same tolerance, FLOOR) -- block Jacobi, or run(w, dtype) with the solver's own preconditioner: two preconditioners end at the
    same residual with differently distributed errors --; converged whenever that yardstick is.  Returns dx_c."""
    ba, s, po, sc = dev.ba, dev.s, dev.po, dev.scalar
    groups = groups or []
    ref = dev.trial(lam, groups=groups)
    S64 = ref["S"].astype(np.float64)
    s.set_pcg(cap, TIGHT[sc])
    s.try_step(lam)
    st = s.pcg_stats()
    dxc = s.get(ba.GET_DX)[3 * po.M:]
    gc = dev.g[3 * po.M:]
    if run is None:
        run = lambda w, t: SH.Working(w["S"], w["rhs"], w["B"], w["Vd"], gc, t).pcg(groups, cap, TIGHT[sc])
    yd, scale, _, _ = dev.pcg_yardstick(lam, run)
    yerr = scale * PC.iterate_error(yd["x"], ref["dx_c"], S64)
    print("DAMP %s%s@%.0e: device iterations %d converged %d residual %.2e; yardstick iterations %d converged %d"
          % (ck.case, tag, lam, st["last_iters"], st["last_converged"], st["last_rel_residual"], yd["iters"], yd["converged"]))
    ck("not_converged_where_the_yardstick_is%s@%.0e" % (tag, lam), 1 if (yd["converged"] and st["last_converged"] != 1) else 0, 0)
    ck("step%s@%.0e(yardstick %.1e, worst camera %d)" % (tag, lam, yerr, PC.worst_camera(dxc, ref["dx_c"], S64)),
       PC.iterate_error(dxc, ref["dx_c"], S64), max(10 * yerr, FLOOR[("iterate", sc)]))
    w = dxc.reshape(-1, 9)
    ck("dx_rows_differ_in_a_group%s@%.0e" % (tag, lam), sum(int(np.any(bits(w[m, 6:9]) != bits(w[m[0], 6:9]))) for m in groups), 0)
    return dxc


def _vdiag(dev):
    V = np.zeros((dev.po.N, 9))
    np.add.at(V, dev.po.cam_idx, (dev.Jc ** 2).sum(axis=1))
    return V


def _chain(ba, O, pg):
    """An odometry chain (a, a + 1) over all cameras: relpose_checks.standard_constraints' first N - 1 constraints."""
    po = sorted_oracle_problem(O, pg)
    s = ba.Solver(pg, ba.ITERSCHUR, ba.F64)
    s.linearize()
    V = np.zeros((pg.N, 9))
    np.add.at(V, po.cam_idx, (s.get(ba.GET_JC).reshape(-1, 2, 9) ** 2).sum(axis=1))
    cs = RC.standard_constraints(pg.N, po.cam_idx, po.pt_idx, s.get(ba.GET_CAMS), V)[0]
    idx = np.arange(pg.N - 1)
    return RC.Constraints(cs.pairs[idx], cs.R0[idx], cs.t0[idx], cs.Lr[idx], cs.Lt[idx])


def _relpose_adds(cs, cm=None):
    def adds(dev):
        d = RC.direct(cs, dev.po.N, dev.s.get(dev.ba.GET_CAMS), cm)
        cross = d["S"].copy()
        for a in range(dev.po.N):
            cross[9 * a:9 * a + 9, 9 * a:9 * a + 9] = 0
        return dict(add_V=d["V"], add_cross=cross)  # (g: the device's own GET_GRAD has the constraints' part)
    return adds


@pytest.mark.parametrize("scalar", [0, 1], ids=["f64", "f32"])
@pytest.mark.parametrize("forest", ["constraint", "visibility"])
def test_converged_step_under_the_forests(ba, O, gpu_ok, prob21, forest, scalar):
    """The constraint forest over a chain of relative poses (their H_aa are in V, hence in D) and the visibility forest: the converged
    step against the dense solve of the reference system.  Measured, device / working-precision CPU yardstick with the same preconditioner kind
    (floor 6e-13 / 3e-3): constraint forest fp64 at 1e-6 1.7e-9 / 7.5e-10 (against a block-Jacobi yardstick it reads 3.6e-11: two
    preconditioners end at the same residual with differently distributed errors); visibility forest fp64 at 1e-6 2.0e-11 / 5.9e-10, fp32
    at 1e-3 2.0e-5 / 5.8e-4."""
    ck = Checker("forest[%s,%s]" % (forest, SN[scalar]))
    if forest == "constraint":
        cs = _chain(ba, O, prob21)
        cs = cs.rounded(np.float32) if scalar == 1 else cs

        def setup(s):
            cs.apply(s)
            s.set_preconditioner(ba.PRECOND_CONSTRAINT_FOREST, 0)
        dev = Dev(ba, O, prob21, ba.ITERSCHUR, scalar, setup=setup, adds=_relpose_adds(cs))
        assert dev.s.preconditioner_info()["kept"] == 20
        pl = FC.plan(21, cs.pairs, 21)
        cross = RC.direct(cs, 21, dev.s.get(ba.GET_CAMS))["cross"]
        H = np.stack([cross[(int(a), int(b))] for a, b in cs.pairs])
        gc = dev.g[3 * dev.po.M:]

        def run(w, t):  # the library's forest factor of the working-precision blocks (forest_checks.working), the product matrix-free
            rhs = np.asarray(gc).astype(t) - (np.asarray(gc, LD) - w["rhs"]).astype(t)
            Dw, Gw, bad = FC.working(w["B"], H, cs.pairs, pl, t)
            out = FC.pcg(w["S"], rhs, FC.forest(pl, Dw, Gw), CAP, TIGHT[scalar], dtype=t, V=w["Vd"])
            return out if bad == 0 and np.all(np.isfinite(out["x"].astype(np.float64))) else None
    else:
        dev = Dev(ba, O, prob21, ba.ITERSCHUR, scalar, setup=lambda s: s.set_preconditioner(ba.PRECOND_VISIBILITY_FOREST, 0))
        assert dev.s.preconditioner_info()["kept"] > 0
    for lam in LAMS_CONVERGED[scalar]:
        converged_step(ck, dev, lam, run=run if forest == "constraint" else None)
    ck.done()


# ---- clamps ------------------------------------------------------------------------------------------------------------------------------
def test_clamps_bite_on_both_sides(ba, O, gpu_ok, prob21):
    """diag_min above some columns' diagonals and diag_max below others', chosen from the diagonal of the device's own J'J of problem-21
    (between two neighbouring values, so that no rounding decides a side): the stages against the reference with the same bounds, and
    the step differs from the step with open clamps by far more than either's error.  Measured at lambda = 1e-6, device / fp64 CPU trial:
    S 2.6e-14 / 3.7e-14 (floor 1e-14), rhs 5.3e-14 / 6.4e-14 (floor 5e-15)."""
    free = Dev(ba, O, prob21, ba.CHOLESKY, 0, bounds=(1e-300, 1e300))
    r0 = free.trial(1e-2, want_step=False)
    diag = np.concatenate([r0["diag_p"], r0["diag_c"]]).astype(np.float64)
    pos = np.sort(diag[diag > 0])
    n = len(pos)
    dmin, dmax = float(np.sqrt(pos[n // 4] * pos[n // 4 + 1])), float(np.sqrt(pos[3 * n // 4] * pos[3 * n // 4 + 1]))
    low, high = int((diag < dmin).sum()), int((diag > dmax).sum())
    cam_low, cam_high = int((diag[3 * free.po.M:] < dmin).sum()), int((diag[3 * free.po.M:] > dmax).sum())
    print("DAMP clamps: diag_min %.3e bites on %d unknowns (%d camera), diag_max %.3e on %d (%d camera), of %d" % (dmin, low, cam_low, dmax, high, cam_high, len(diag)))
    assert low > 0 and high > 0 and cam_low > 0 and cam_high > 0 and low + high < len(diag)
    ck = Checker("clamps[p21,f64]")
    dev = Dev(ba, O, prob21, ba.CHOLESKY, 0, bounds=(dmin, dmax))
    assert dev.s.damping() == (ba.DAMP_MARQUARDT, dmin, dmax)
    for lam in LAMS:
        dx, ref = check_cholesky_trial(ck, dev, lam)
        d = np.concatenate([ref["d_p"], ref["d_c"]]).astype(np.float64)
        assert np.all(d[diag < dmin] == lam * dmin) and np.all(d[diag > dmax] == lam * dmax)
        free.s.try_step(lam)
        moved = DC.step_difference(free.s.get(ba.GET_DX), dx)
        ck("clamped_step_equals_open_step@%.0e(moved %.1e)" % (lam, moved), 0 if moved > 1e-6 else 1, 0)
    ck.done()


# ---- masks and rows ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind_name,scalar", [("CHOLESKY", 0), ("CHOLESKY", 1), ("ITERSCHUR", 0)])
def test_fixed_parameters_keep_their_bits(ba, O, gpu_ok, prob21, kind_name, scalar):
    """The gauge mask, one camera's distortion and some fixed points: D = diag_min on their columns, their steps exactly 0 (the stages
    against the reference on the masked J), their values the same bits through accept and ba_minimize.  Measured at lambda = 1e-6,
    device / CPU trial: CHOLESKY fp64 S 4.0e-14 / 2.0e-14, rhs 4.8e-14 / 5.4e-14, fp32 S 2.9e-5 / 3.1e-5, rhs 2.0e-5 / 1.2e-5 (floors 1e-14,
    5e-15, 1e-5, 5e-6); ITERSCHUR fp64 step 1.8e-11 / 4.4e-10 (floor 6e-13)."""
    kind = getattr(ba, kind_name)
    cm = prob21.gauge_mask(0)
    cm[7] |= np.uint16(0x180)  # k1, k2 of camera 7
    pf = np.zeros(prob21.M, np.uint8)
    pf[[0, 5, 1000, prob21.M - 1]] = 1
    ck = Checker("masked[%s,%s]" % (kind_name, SN[scalar]))
    dev = Dev(ba, O, prob21, kind, scalar, setup=lambda s: s.set_constant(cm, pf))
    s, M = dev.s, dev.po.M
    fx = np.concatenate([np.repeat(pf != 0, 3), ((cm.astype(np.int64)[:, None] >> np.arange(9)[None, :]) & 1 == 1).ravel()])
    cams0, pts0 = s.get(ba.GET_CAMS).reshape(-1, 15), s.get(ba.GET_POINTS)
    for lam in (LAMS if kind == ba.CHOLESKY else LAMS_CONVERGED[scalar]):
        if kind == ba.CHOLESKY:
            dx, ref = check_cholesky_trial(ck, dev, lam)
            S = s.get(ba.GET_S)
            i = 0  # camera 0, T0: a fixed row of S is lambda diag_min alone
            row = S[i].copy()
            ck("fixed_row_diagonal@%.0e" % lam, abs(row[i] - DT[scalar](lam) * DT[scalar](dev.dmin)), 0)
            row[i] = 0
            ck("fixed_row_offdiagonal@%.0e" % lam, np.count_nonzero(row) + np.count_nonzero(S[:, i]) - 1, 0)
        else:
            dxc = converged_step(ck, dev, lam)
            dx = s.get(ba.GET_DX)
        ref = dev.trial(lam, want_step=False)
        assert np.all(np.concatenate([ref["diag_p"], ref["diag_c"]])[fx] == 0)
        ck("fixed_steps_nonzero@%.0e" % lam, np.count_nonzero(dx[fx]), 0)
    s.accept()
    cams1, pts1 = s.get(ba.GET_CAMS).reshape(-1, 15), s.get(ba.GET_POINTS)
    s.minimize(max_trials=6, lambda_init=1e-3)
    cams2, pts2 = s.get(ba.GET_CAMS).reshape(-1, 15), s.get(ba.GET_POINTS)

    def kept(c, p):
        n = int(np.any(bits(c[0, :12]) != bits(cams0[0, :12])))  # camera 0: R and T
        n += int(np.any(bits(c[7, 13:15]) != bits(cams0[7, 13:15])))
        n += int(np.any(bits(p.reshape(-1, 3)[pf != 0]) != bits(pts0.reshape(-1, 3)[pf != 0])))
        return n
    ck("fixed_values_changed_by_accept", kept(cams1, pts1), 0)
    ck("fixed_values_changed_by_minimize", kept(cams2, pts2), 0)
    ck("free_values_unchanged_by_minimize", 0 if np.any(cams2[3] != cams0[3]) else 1, 0)
    ck.done()


@pytest.mark.parametrize("prob", ["p21", "ragged"])
def test_priors_and_relative_poses_are_in_the_diagonal(ba, O, gpu_ok, prob21, prob):
    """Priors (prior_checks.standard_priors: points -- on `ragged` one nobody observes --, centres, intrinsics) and a chain of relative
    poses: their diagonal contributions are part of D.  The stages against the reference with their blocks added; the reference
    WITHOUT their part of the diagonal in D misses the device's S by far more than the bound.  Measured at lambda = 1e-6, device / fp64
    CPU trial: problem-21 S 1.0e-14 / 1.2e-14, rhs 2.9e-14 / 2.2e-14; ragged S 4.0e-15 / 8.5e-15 (floors 1e-14, 5e-15)."""
    pg = problem(ba, prob, prob21)
    cs = _chain(ba, O, pg)
    plain = Dev(ba, O, pg, ba.CHOLESKY, 0)
    po = plain.po
    pr, _ = PR.standard_priors(po.N, po.M, po.K, po.pt_idx, plain.s.get(ba.GET_CAMS), plain.s.get(ba.GET_POINTS), plain.Jc, plain.Jp, po.cam_idx)

    def setup(s):
        pr.apply(s)
        cs.apply(s)

    def adds(dev):
        cam15, pts = dev.s.get(ba.GET_CAMS), dev.s.get(ba.GET_POINTS)
        dp = PR.direct(pr, po.N, po.M, cam15, pts)
        out = _relpose_adds(cs)(dev)
        return dict(add_U=dp["U"], add_V=dp["V"] + out["add_V"], add_cross=out["add_cross"])
    ck = Checker("rows[%s,f64]" % prob)
    dev = Dev(ba, O, pg, ba.CHOLESKY, 0, setup=setup, adds=adds)
    for lam in LAMS:
        dx, ref = check_cholesky_trial(ck, dev, lam)
        base = plain.trial(lam, want_step=False)
        grown = int((ref["diag_c"] > base["diag_c"]).sum()), int((ref["diag_p"] > base["diag_p"]).sum())
        assert grown[0] >= 6 * po.N and grown[1] >= 3 * len(pr.pt_ids), grown  # every pose (centres, chain) and every prior point
        # the same system damped by the observations' diagonal alone: what a kernel that read the wrong diagonal would assemble
        stale = ref["S"].astype(np.float64) - np.diag((ref["d_c"] - base["d_c"]).astype(np.float64))
        miss = DC.assembly_errors(po, dev.Jc, dev.Jp, dev.f, ref["d_c"], dev.s.get(ba.GET_S), ref["rhs"], stale, ref["rhs"], ref["diag_c"])["S"]
        ck("stale_diagonal_is_noticed@%.0e(miss %.1e)" % (lam, miss), 0 if miss > 1e3 * BOUND[("S", 0)] else 1, 0)
    if prob == "ragged":
        lone = [j for j in pr.pt_ids if not np.any(po.pt_idx == j)]
        assert lone  # (k_prior_lonely's Marquardt instantiation runs)
        ck("lonely_prior_point_did_not_move", 0 if np.any(dx[3 * lone[0]:3 * lone[0] + 3] != 0) else 1, 0)
    ck.done()


# ---- shared intrinsics -------------------------------------------------------------------------------------------------------------------
def _equalise(ba, s, groups):
    cams = s.get(ba.GET_CAMS).reshape(-1, 15).copy()
    for m in groups:
        cams[m, 12:15] = cams[m[0], 12:15]
    s.set_state(cams.ravel(), None)


def _p21_groups(what):
    g = np.full(21, -1, np.int32)
    if what == "all":
        g[:] = 0
    else:  # three groups of 7, 7 and 7 cameras less the cameras 0 and 7, which keep their own
        g[:] = np.arange(21) % 3
        g[[0, 7]] = -1
    return g


@pytest.mark.parametrize("what,scalar", [("all", 0), ("all", 1), ("mod3", 0), ("mod3", 1)], ids=["all-f64", "all-f32", "mod3-f64", "mod3-f32"])
def test_shared_intrinsics_step(ba, O, gpu_ok, prob21, what, scalar):
    """The projected PCG is unchanged, so the damping it implies is lambda P'D P: the converged step against P y of the dense
    (P'SP) y = P' rhs with the Marquardt S, rows 6..8 bit-equal inside a group.  Measured, device / yardstick (floor 6e-13 / 3e-3): one
    group fp64 at 1e-6 8.4e-11 / 5.1e-10, fp32 at 1e-3 6.0e-5 / 1.3e-3; three groups fp64 6.6e-11 / 1.2e-9, fp32 4.1e-5 / 9.3e-4."""
    g = _p21_groups(what)
    groups = SH.groups_of(21, g)

    def setup(s):
        _equalise(ba, s, groups)
        s.set_shared_intrinsics(g)
    ck = Checker("shared[p21,%s,%s]" % (what, SN[scalar]))
    dev = Dev(ba, O, prob21, ba.ITERSCHUR, scalar, setup=setup)
    for lam in LAMS_CONVERGED[scalar]:
        converged_step(ck, dev, lam, groups, cap=CAP_SHARED)
    ck.done()


def test_shared_intrinsics_groups_of_256_and_257(ba, O, gpu_ok):
    """synthetic(600, 7200, 36 000) with a group of 256 (the largest of one chunk) and one of 257 (the smallest of two), members spread
    over the cameras; the other 87 keep their own intrinsics.  Measured at lambda = 1e-2: 8.3e-13 against a yardstick of 7.4e-13
    (floor 6e-13)."""
    pg = ba.Problem.synthetic(600, 7200, 36000, 4600)
    order = (np.arange(600) * 7) % 600
    g = np.full(600, -1, np.int32)
    g[order[:256]] = 1
    g[order[256:513]] = 0
    groups = SH.groups_of(600, g)

    def setup(s):
        _equalise(ba, s, groups)
        s.set_shared_intrinsics(g)
    ck = Checker("shared[syn600,256+257]")
    dev = Dev(ba, O, pg, ba.ITERSCHUR, 0, setup=setup)
    assert dev.s.shared_intrinsics_info()["chunks"] == 3
    converged_step(ck, dev, 1e-2, groups)
    ck.done()


# ---- the default path ---------------------------------------------------------------------------------------------------------------------
def _observe(ba, s):
    e, dmax = s.linearize()
    s.try_step(1e-9 * dmax)
    dx = s.get(ba.GET_DX)
    tr = s.minimize(max_trials=8)["trace"]
    return bits(dx), bits(s.get(ba.GET_CAMS)), bits(s.get(ba.GET_POINTS)), bits(tr[:, :5])


@pytest.mark.parametrize("kind_name,scalar", [("CHOLESKY", 0), ("CHOLESKY", 1), ("ITERSCHUR", 0), ("ITERSCHUR", 1)])
def test_default_path_is_untouched(ba, gpu_ok, prob21, kind_name, scalar):
    """A solver that never called set_damping, one that set Marquardt (and ran a trial and a minimize under it, from a state it then
    restored) and then identity, and one that set identity only: the same bits of BA_GET_DX, the state and an 8-row trace."""
    kind = getattr(ba, kind_name)
    never = ba.Solver(prob21, kind, scalar)
    want = _observe(ba, never)
    back = ba.Solver(prob21, kind, scalar)
    cams, pts = back.get(ba.GET_CAMS), back.get(ba.GET_POINTS)
    back.set_damping(ba.DAMP_MARQUARDT, 1e-3, 1e9)
    back.linearize()
    back.try_step(1e-3)
    back.minimize(max_trials=3)
    back.set_state(cams, pts)
    back.set_damping(ba.DAMP_IDENTITY)
    assert back.damping()[0] == ba.DAMP_IDENTITY
    only = ba.Solver(prob21, kind, scalar)
    only.set_damping(ba.DAMP_IDENTITY, 5.0, 7.0)
    for name, s in (("marquardt-and-back", back), ("identity-only", only)):
        got = _observe(ba, s)
        for what, a, b in zip(("dx", "cams", "points", "trace"), got, want):
            assert np.array_equal(a, b), (kind_name, scalar, name, what)


# ---- ba_minimize -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind_name", ["CHOLESKY", "ITERSCHUR"])
def test_minimize_starts_from_lambda_init(ba, gpu_ok, prob21, kind_name):
    """Plain least squares, the gauge fixed, 12 trials from lambda_init = 1e-3: the table's lambda follows the device control's rule
    FROM lambda_init (an accepted row carries lambda max(1 / 3, 1 - (2 rho - 1)^3) clamped to lambda_min, a rejected one the lambda it
    used, the next one lambda_inc times that, lambda_inc = 2, 2^1.5, ...), so the first trial ran at lambda_init and not at
    1e-12 max diag J'J; the energies of the accepted rows do not increase."""
    s = ba.Solver(prob21, getattr(ba, kind_name), ba.F64)
    s.set_loss(ba.LOSS_TRIVIAL)
    s.set_constant(prob21.gauge_mask(0), None)
    s.set_damping(ba.DAMP_MARQUARDT)
    lam0 = 1e-3
    out = s.minimize(max_trials=12, lambda_init=lam0)
    tr = out["trace"]
    assert len(tr) == 12 and tr[:, 1].sum() >= 3, tr
    lam, inc = lam0, 2.0
    for it, acc, f, rho, lam_row, _ in tr:
        if acc:
            t = 2.0 * rho - 1.0
            lam = max(lam * max(1.0 - t * t * t, 1.0 / 3.0), 1e-10)
            inc = 2.0
            assert abs(lam_row - lam) <= 1e-12 * lam, (it, lam_row, lam)
            lam = lam_row
        else:
            assert abs(lam_row - lam) <= 1e-12 * lam, (it, lam_row, lam)
            lam = lam_row * inc
            inc = inc ** 1.5
    fa = tr[tr[:, 1] == 1, 2]
    assert np.all(np.diff(fa) <= 0), fa  # (f is the energy BEFORE the step: each accepted row starts where the last accepted step ended)
    assert out["energy"] <= fa[-1]


# ---- refusals and state ------------------------------------------------------------------------------------------------------------------
def _refused(ba, fn, *args):
    with pytest.raises(ba.BAError) as ei:
        fn(*args)
    assert ei.value.code == ba.ERR_ARG, ei.value


def test_refusals_and_state(ba, gpu_ok, prob21, monkeypatch):
    monkeypatch.delenv("BA_MOREQR_QR", raising=False)
    small = ba.Problem.synthetic(4, 120, 400, 9)
    for kind in (ba.QRKIT, ba.QRCHOL, ba.MOREQR, ba.QRSPQR):
        s = ba.Solver(small, kind, ba.F64)
        n0 = s.device_bytes()
        _refused(ba, s.set_damping, ba.DAMP_MARQUARDT)
        assert s.damping() == (ba.DAMP_IDENTITY, 1e-6, 1e32) and s.device_bytes() == n0
        s.set_damping(ba.DAMP_IDENTITY)
    for scalar in (ba.F64, ba.F32):
        s = ba.Solver(small, ba.CHOLESKY, scalar)
        assert s.damping() == (ba.DAMP_IDENTITY, 1e-6, 1e32)
        s.set_damping(ba.DAMP_MARQUARDT, 1e-3, 1e5)
        want = (ba.DAMP_MARQUARDT, float(DT[scalar](1e-3)), float(DT[scalar](1e5)))  # (the bounds as the kernels see them)
        assert s.damping() == want
        n0 = s.device_bytes()
        for bad in ((2,), (-1,), (ba.DAMP_MARQUARDT, -1.0, 1.0), (ba.DAMP_MARQUARDT, 2.0, 1.0), (ba.DAMP_MARQUARDT, float("nan"), 1.0),
                    (ba.DAMP_MARQUARDT, 1.0, float("inf")), (ba.DAMP_MARQUARDT, 1e-6, 1e300 if scalar == ba.F32 else float("inf")),
                    (ba.DAMP_MARQUARDT, 1e-60 if scalar == ba.F32 else -0.5, 1.0)):
            _refused(ba, s.set_damping, *bad)
            assert s.damping() == want and s.device_bytes() == n0, bad
        s.set_damping(ba.DAMP_MARQUARDT)  # 0 = the defaults
        assert s.damping() == (ba.DAMP_MARQUARDT, float(DT[scalar](1e-6)), float(DT[scalar](1e32)))
    # a pending step stays acceptable; no new linearisation is needed
    s = ba.Solver(small, ba.CHOLESKY, ba.F64)
    _, dmax = s.linearize()
    s.try_step(1e-9 * dmax)
    xt = bits(s.get(ba.GET_CAMS_TEST))
    s.set_damping(ba.DAMP_MARQUARDT)
    s.accept()
    assert np.array_equal(bits(s.get(ba.GET_CAMS)), xt)
    s.linearize()
    a = s.try_step(1e-3)
    s.set_damping(ba.DAMP_IDENTITY)
    b = s.try_step(1e-3)
    s.set_damping(ba.DAMP_MARQUARDT)
    assert s.try_step(1e-3) == a and a != b


def test_covariance_calls_keep_lambda_identity(ba, gpu_ok, prob21):
    """ba_solver_covariance_compute / _pcg keep (J'J + lambda I)^-1 whatever damping is set: the same bits with Marquardt as without."""
    cm = prob21.gauge_mask(0)
    out = {}
    for damp in (ba.DAMP_IDENTITY, ba.DAMP_MARQUARDT):
        c = ba.Solver(prob21, ba.CHOLESKY, ba.F64)
        c.set_constant(cm, None)
        c.set_damping(damp)
        c.linearize()
        cc, cp = c.covariance(1e-3, cams=[1, 5], points=[3, 100])
        i = ba.Solver(prob21, ba.ITERSCHUR, ba.F64)
        i.set_constant(cm, None)
        i.set_damping(damp)
        i.linearize()
        ic, ip, _ = i.covariance_pcg(1e-3, cams=[1, 5], points=[3, 100])
        out[damp] = [bits(x) for x in (cc, cp, ic, ip)]
    for a, b in zip(out[ba.DAMP_IDENTITY], out[ba.DAMP_MARQUARDT]):
        assert np.array_equal(a, b)
