"""GPU: every stage of one LM trial against the same stage in quad precision on the GPU's OWN inputs of that stage (tests/stage_checks.py).

The whole-pipeline tests (test_gpu_parity.py, test_gpu_configs.py) compare with the fp64 oracle, and each stage there inherits every
difference made before it: S is checked to 1e-11 of max|S| (the focal-length rows of problem-21 are 1e-11 below that), the dense
LDL^T and its back sweep only through the step (1e-6) or a normal-equations residual, and the fp32 kernels hardly at all.  Here:

  linearisation   GPU f, J at the GPU's state (GET_CAMS / GET_POINTS) against quad; g against -J'r of the GPU's own J and r
  assembly        GPU S, rhs against the quad assembly from the GPU's own J and r, scaled by sqrt((U_ii + lam)(U_jj + lam)); bound
                  max(10 x the oracle's error on the same J, floor)
  factor + sweep  eta(S_gpu, dx_c, rhs_gpu), the backward error of the solve (S dx_c = rhs): fp64 <= 1e-14, fp32 <= 1e-5, at every
                  lambda, also where two solvers' steps can no longer be compared.  Branches: test_factor_and_sweep_backward_error
                  (the factor without time-out, one-launch sweep), test_launch_per_pair_back_sweep (k_ldlt_backpair + backstep),
                  test_gpu_configs.py::test_cfg5_full_size (D = 9216), test_gpu_failure_paths.py::test_row_flag_timeout_is_recovered
                  (safe factor: k_ldlt_panel + k_ldlt_update per block column, fp64)
  dense QR        (QRKIT, MOREQR: no S) eta of the GPU camera step against the quad S and rhs from the GPU's J: elimination error
                  included, bound max(10 x an fp64 QR solver on the same J, floor); the QR alone, at every TSQR shape and on the
                  matrices the solver factors: test_gpu_dense_qr.py
  back-subst.     per point, the rows of the normal equations with the GPU's J, g and step
  retraction      GET_CAMS_TEST / GET_POINTS_TEST against the quad retraction of the GPU's state and step, in ulps
  trial scalars   e_test against the quad energy at the GPU's trial point; rho denominator and |dx| against the same sums of the
                  GPU's dx and g

Each value is printed as `STAGE <case> <metric> <value> <bound>`; the docstrings record the worst values measured on an MI355X.  The
63 cases took 149 s on an MI355X box (most of it the quad assembly and residuals on the host); the 14 factor cases added since
(N = 16 ... 71, 334: test_factor_and_sweep_backward_error) bring that test to 52 cases in 24 s.
"""
import hashlib

import numpy as np
import pytest

import stage_checks as SC
from test_gpu_parity import _long_track_problem, _moreqr_default_route, _ragged_problem, moreqr_route  # noqa: F401 (autouse fixture)

pytestmark = pytest.mark.gpu

EPS = {0: float(np.finfo(np.float64).eps), 1: float(np.finfo(np.float32).eps)}

# Bounds, set from the first MI355X run with at least 10x headroom over the worst value measured over every case of this file (that
# value in the comment), within the ceilings eta <= 1e-14 (fp64) / 1e-5 (fp32).
BOUND = {
    # factor + sweep: fp64 6.4e-16 (N = 21, lambda = 1e-3); fp32 5.2e-7 (N = 13, lambda0) -- except for the case below
    ("eta", 0): 1e-14, ("eta", 1): 1e-5,
    # fp32, one block column (N <= 7), lambda < eps32 max S_ii (= 0.03 ... 0.19 there: lambda0, 1e-10, 1e-3): the seven gauge
    # directions of S are regularised by lambda alone, below the fp32 rounding of its entries, so S is not positive definite to
    # working precision and the bound |L| |D| |L'| <= sqrt(S_ii S_jj) behind eta ~ u no longer holds -- eta then measures the luck
    # of the rounding more than the kernel (the fp32 oracle's LDL^T of the same J breaks down to NaN there).  Measured: 4.0e-6
    # (N = 2, lambda = 1e-10), 1.1e-7 otherwise.
    ("eta_singular", 1): 1e-4,
    # linearisation at the GPU's own state, residual / Jacobian / energy / gradient: fp64 1.8e-15 / 8.3e-15 / 5.5e-15 / 2.6e-16;
    # fp32 9.5e-7 / 1.1e-5 / 2.1e-6 / 1.5e-7 (the Jacobian per entry, relative to its sensitivity to the inputs; the fp64 / fp32
    # oracle on problem-21: 8.0e-15 / 1.4e-5)
    ("res", 0): 2e-14, ("res", 1): 1e-5,
    ("jac", 0): 1e-13, ("jac", 1): 2e-4,
    ("energy", 0): 1e-13, ("energy", 1): 3e-5,
    ("grad", 0): 5e-15, ("grad", 1): 2e-6,
    # floors under 10x the oracle's error on the same J: the GPU was at most 0.15x the oracle's error on every case
    ("S", 0): 1e-14, ("S", 1): 1e-5,
    ("rhs", 0): 5e-15, ("rhs", 1): 5e-6,
    ("qr_eta", 0): 1e-15, ("qr_eta", 1): 5e-8,   # fp64 1.9e-17 (oracle 6-8e-17); fp32 4.5e-9 (no oracle)
    # back-substitution: fp64 1.8e-15, fp32 6.2e-7; retraction (ulps): fp64 1.0, fp32 2.0
    ("backsub", 0): 2e-14, ("backsub", 1): 1e-5,
    ("retract", 0): 4.0, ("retract", 1): 8.0,
    # trial scalars: e_test fp64 9.2e-15, fp32 4.3e-6; rho denominator 1.3e-16 / 5.2e-8; |dx| 1.4e-16 / 5.8e-8
    ("e_test", 0): 1e-13, ("e_test", 1): 5e-5,
    ("rho_scale", 0): 2e-15, ("rho_scale", 1): 1e-6,
    ("dx_norm", 0): 2e-15, ("dx_norm", 1): 1e-6,
}


class Checker:
    """Collects (case, metric, value, bound), prints every one, and asserts them all at the end -- one failing metric does not hide
    the values of the others."""

    def __init__(self, case):
        self.case, self.rows = case, []

    def __call__(self, metric, value, bound):
        self.rows.append((metric, float(value), float(bound)))
        print("STAGE %s %s %.3e %.1e" % (self.case, metric, value, bound))

    def done(self):
        bad = [r for r in self.rows if not (r[1] <= r[2])]
        assert not bad, (self.case, bad)


def sorted_oracle_problem(O, pg):
    """The oracle's view of a GPU problem in the order the GPU's getters return observations (point-sorted, stably: the file order
    when the input is sorted)."""
    a = pg.arrays()
    order = np.argsort(a["pt_idx"], kind="stable")
    return O.Problem(pg.N, pg.M, pg.K, a["cam_idx"][order], a["pt_idx"][order], a["meas"].reshape(-1, 2)[order].ravel(), a["cams9"],
                     a["pts"])


_QUAD_LIN = {}


def quad_linearization(po, cam, pts):
    """stage_checks.quad_linearization (nine quad linearisations), once per problem and state: every symbol of a problem starts from
    the same state, and the fp32 state is another one."""
    key = hashlib.sha1(b"".join(np.ascontiguousarray(x).tobytes() for x in (po.cam_idx, po.pt_idx, po.meas, cam, pts))).hexdigest()
    if key not in _QUAD_LIN:
        _QUAD_LIN[key] = SC.quad_linearization(po, cam, pts)
    return _QUAD_LIN[key]


class Trial:
    """A solver at its linearisation with the GPU's own state, residuals, J and g read back (point-sorted)."""

    def __init__(self, ba, O, pg, kind, scalar, ck):
        self.ba, self.O, self.scalar, self.ck = ba, O, scalar, ck
        self.po = po = sorted_oracle_problem(O, pg)
        self.s = s = ba.Solver(pg, kind, scalar)
        s.keep_intermediates(True)
        self.e, self.dmax = s.linearize()
        self.cam, self.pts = s.get(ba.GET_CAMS), s.get(ba.GET_POINTS)
        self.f = s.get(ba.GET_RESIDUALS)
        self.Jc, self.Jp = s.get(ba.GET_JC).reshape(po.K, 2, 9), s.get(ba.GET_JP).reshape(po.K, 2, 3)
        self.g = s.get(ba.GET_GRAD)

    def bound(self, metric):
        return BOUND[(metric, self.scalar)]

    def check_linearization(self):
        lin = SC.linearization_errors(self.po, self.cam, self.pts, self.f, self.Jc, self.Jp, self.e,
                                      ref=quad_linearization(self.po, self.cam, self.pts))
        for k in ("res", "jac", "energy"):
            self.ck(k, lin[k], self.bound(k))
        self.ck("grad", SC.grad_errors(self.po, self.Jc, self.Jp, self.f, self.g), self.bound("grad"))

    def step(self, lam, has_S, fp32_singular_bound=False):
        """try_step(lam) and the metrics of everything behind the assembly: factor + sweep (eta, when there is an S), back-substitution,
        retraction, trial scalars.  Returns (dx, S, rhs) for the caller's assembly / dense-QR checks.
        fp32_singular_bound: an fp32 S with lambda below eps32 max S_ii is measured against BOUND[("eta_singular", 1)]."""
        ba, s, po, ck = self.ba, self.s, self.po, self.ck
        et, rs, dn = s.try_step(lam)
        dx = s.get(ba.GET_DX)
        S = rhs = None
        if has_S:
            S, rhs = s.get(ba.GET_S), s.get(ba.GET_RHS)
            singular = fp32_singular_bound and self.scalar == 1 and lam < EPS[1] * np.diagonal(S).max()
            ck("eta@%.0e" % lam, SC.eta(S, dx[3 * po.M:], rhs), BOUND[("eta_singular", 1)] if singular else self.bound("eta"))
        ck("backsub@%.0e" % lam, SC.backsub_errors(po, self.Jc, self.Jp, dx, self.g, lam), self.bound("backsub"))
        ct, pt = s.get(ba.GET_CAMS_TEST), s.get(ba.GET_POINTS_TEST)
        ck("retract@%.0e" % lam, SC.retraction_ulps(po, self.cam, self.pts, dx, ct, pt, EPS[self.scalar]), self.bound("retract"))
        sc = SC.trial_scalar_errors(po, lam, dx, self.g, et, rs, dn, ct, pt)
        for k, v in sc.items():
            ck("%s@%.0e" % (k, lam), v, self.bound(k))
        return dx, S, rhs

    def oracle_dtype(self):
        return np.float64 if self.scalar == 0 else np.float32

    def oracle_step(self, kind, lam, want_S=True):
        """The oracle (fp64, or fp32 for an fp32 solver) fed the GPU's own J and residuals: the yardstick of what a CPU implementation
        of the same arithmetic achieves on the same inputs."""
        dt = self.oracle_dtype()
        return self.O.step(kind, self.po, self.Jc.astype(dt), self.Jp.astype(dt), self.f.astype(dt), lam, want_S=want_S)


# ---- factor + back sweep: the branches of ba_ldlt_factor / ba_ldlt_backsweep ------------------------------------------------------------
def _synthetic(ba, ncams):
    if ncams <= 23:  # test_dense_block_widths' problems
        npts = 40 * ncams
        return ba.Problem.synthetic(ncams, npts, min(4, ncams) * npts, 100 + ncams)
    npts = 12 * ncams  # test_fused_factor_paths' problems
    return ba.Problem.synthetic(ncams, npts, 5 * npts, 4000 + ncams)


FACTOR_CASES = [
    # one block column (D <= 63): panel + update launches of a single block column, one-group sweep
    2, 3, 4, 5, 6, 7,
    # fused k_ldlt_step, the last block column 9 N mod 64 = 17, 35, 44, 53, 62, 7, 61, 15 wide (sub-panel counts 1 ... 4)
    9, 11, 12, 13, 14, 15, 21, 23,
    # the sub-panel seams behind full block columns: N = 16, 32, 48 (D = 144, 288, 432) end in a block column 16, 32, 48 wide
    16, 32, 48,
    # N = 57 (D = 513): the last block column 1 wide beside the right-hand side row; N = 64 (D = 576 = 9 x 64): width 0, the right-hand
    # side row alone in a tenth row block; N = 71 (D = 639): 63 wide
    57, 64, 71,
    # N = 180: 26 block columns, k_ldlt_step with dyn_lds = 8192 throughout
    180,
    # N = 240: 34 block columns (32 <= nblk < 48), more update jobs per launch than CUs (dyn_lds = 8192 in every step, like N = 180)
    240,
    # N = 334: D = 3006, 47 block columns, the largest k_ldlt_step
    334,
    # N = 340: 48 block columns, k_ldlt_step2 in single-panel mode from step 1 (p_single = 1)
    340,
    # N = 340 with BA_LDLT_PAIR_MIN=8: k_ldlt_step2's pair phase with 128 x 128 macro tiles up to step 41, then single-panel
    "340pair8",
    # N = 600: 85 block columns, 13 of them in the pair phase (default pair_min 72)
    600,
]


@pytest.mark.parametrize("scalar", [0, 1], ids=["f64", "f32"])
@pytest.mark.parametrize("case", FACTOR_CASES, ids=[str(c) for c in FACTOR_CASES])
def test_factor_and_sweep_backward_error(ba, O, gpu_ok, monkeypatch, case, scalar):
    """eta of the GPU's camera step in the GPU's own S and rhs, at lambda = 1e-12 max diag J'J (the symbol's lambda0), 1e-10, 1e-3
    and 10, on the branches of ba_ldlt_factor that run without a hand-off time-out (single block column, k_ldlt_step with and without
    dynamic LDS, k_ldlt_step2 single-panel and pair phase) behind the one-launch back sweep (k_ldlt_backflow); with it the point back-substitution, the retraction and the
    trial scalars of the same trials.  Measured worst eta, fp64 / fp32: one block column 5.6e-16 / 4.0e-6; k_ldlt_step (N = 9 ... 23,
    180) 6.4e-16 / 5.2e-7; N = 240 1.8e-16 / 1.5e-8; N = 340 (single-panel and pair phase) 2.2e-16 / 1.5e-8; N = 600 1.4e-17 / 1.5e-8;
    the seams N = 16, 32, 48, 57, 64, 71 6.5e-16 / 5.0e-7; N = 334 2.9e-16 / 1.5e-8.  The kernels alone, at every block shape and on
    matrices that are no reduced camera matrix: test_gpu_ldlt_kernels.py."""
    if case == "340pair8":
        monkeypatch.setenv("BA_LDLT_PAIR_MIN", "8")
        ncams = 340
    else:
        monkeypatch.delenv("BA_LDLT_PAIR_MIN", raising=False)
        ncams = case
    ck = Checker("factor[%s,%s]" % (case, "f64" if scalar == 0 else "f32"))
    t = Trial(ba, O, _synthetic(ba, ncams), ba.CHOLESKY, scalar, ck)
    if ncams <= 23:
        t.check_linearization()
    for lam in (1e-12 * t.dmax, 1e-10, 1e-3, 10.0):
        t.step(lam, True, fp32_singular_bound=ncams <= 7)
    ck.done()


@pytest.mark.parametrize("scalar", [0, 1], ids=["f64", "f32"])
def test_launch_per_pair_back_sweep(ba, O, gpu_ok, scalar):
    """ba_ldlt_backsweep's other branch: with more block-column pairs than CUs (nblk > 2 x CUs) the one-launch data-flow sweep is no
    longer certain to have its whole grid resident, and the sweep runs one k_ldlt_backpair launch per pair of block columns and,
    for an odd count, k_ldlt_backstep for block column 0 -- with no fault injected.  N = 1825: D = 16425, 257 block columns (the
    factor: k_ldlt_step2 with 185 pair steps).  eta of the step in the GPU's own S and rhs at lambda0 (quad residual over a
    16425 x 16425 S: 8-9 s per precision).  Measured: 6.2e-18 (fp64), 2.5e-8 (fp32).
    (The other branch of ba_ldlt_factor, safe = panel + update launches, only runs after a hand-off time-out: it is checked in fp64
    by test_gpu_failure_paths.py::test_row_flag_timeout_is_recovered, whose D = 360 sweep is six block columns -- backpair only.)"""
    ncams = 1825
    nblk = (9 * ncams + 63) // 64
    assert nblk % 2 == 1 and 2 * ((nblk + 1) // 2) > gpu_ok[1], (nblk, gpu_ok)  # odd, and past the one-launch sweep's limit
    ck = Checker("pair_sweep[%s]" % ("f64" if scalar == 0 else "f32"))
    p = ba.Problem.synthetic(ncams, 12 * ncams, 60 * ncams, 4000 + ncams)
    s = ba.Solver(p, ba.CHOLESKY, scalar)
    s.keep_intermediates(True)
    e, dmax = s.linearize()
    et, _, _ = s.try_step(1e-12 * dmax)
    assert np.isfinite(et)
    S = s.get(ba.GET_S)
    ck("eta@lambda0", SC.eta(S, s.get(ba.GET_DX)[3 * s.Ml:], s.get(ba.GET_RHS)), BOUND[("eta", scalar)])
    ck.done()


# ---- assembly (both eliminations) and back-substitution on real and irregular problems -----------------------------------------------
def _problem(ba, name, prob21, prob39):
    if name == "p21":
        return prob21
    if name == "p39":
        return prob39
    if name == "ragged":
        return _ragged_problem(ba)  # unsorted input: the getters return point-sorted order (sorted_oracle_problem)
    return _long_track_problem(ba)


ASSEMBLY_CASES = [(prob, kind, 0) for prob in ("p21", "p39", "ragged", "longtracks") for kind in (2, 1, 13)] + \
    [("p21", 2, 1), ("p39", 1, 1)] + [(prob, kind, 1) for prob in ("ragged", "longtracks") for kind in (2, 1, 13)]


@pytest.mark.parametrize("prob,kind,scalar", ASSEMBLY_CASES,
                         ids=["%s-%s-%s" % (p, {2: "chol", 1: "qrchol", 13: "moreqr_ne"}[k], "f64" if s == 0 else "f32") for p, k, s in ASSEMBLY_CASES])
def test_assembly_and_backsub(ba, O, gpu_ok, prob21, prob39, monkeypatch, prob, kind, scalar):
    """S and rhs of the GPU (k_elim_chol / k_elim_qr / MOREQR's k_more_trial, then k_schur_pairs) against the quad assembly from the
    GPU's own J and residuals, scaled entry by entry by sqrt((U_ii + lam)(U_jj + lam)); bound: 10x the oracle's error fed the same J,
    or the floor in BOUND.  The linearisation at the GPU's state, eta, back-substitution, retraction and trial scalars on the same
    trials.  lambda = the symbol's lambda0 (where the 3 x 3 point blocks are the least well conditioned) and 10; problem-39 (quad
    assembly 5 s per call) at lambda0 only.  Measured worst, GPU / oracle: fp64 S 1.6e-12 / 2.1e-12 and rhs 4.1e-13 / 7.7e-13
    (problem-39, CHOLESKY, lambda0); fp32 S 2.1e-4 and rhs 8.3e-6 (long tracks, CHOLESKY, lambda0; fp64 oracle x eps32 / eps64:
    4.9e-5, 1.8e-6 -- the closest to a bound here), S 9.1e-5 and rhs 7.5e-5 (problem-21, CHOLESKY, lambda0; 1.3e-4, 1.1e-4)."""
    kind_s, has_S = moreqr_route(kind, monkeypatch, O)
    ck = Checker("assembly[%s,%s,%d]" % (prob, kind, scalar))
    t = Trial(ba, O, _problem(ba, prob, prob21, prob39), kind_s, scalar, ck)
    t.check_linearization()
    lams = (1e-12 * t.dmax,) if prob == "p39" else (1e-12 * t.dmax, 10.0)
    for lam in lams:
        dx, S, rhs = t.step(lam, has_S)
        R = O.referee_reduced_from_jacobian(kind_s, t.po, t.Jc, t.Jp, t.f, lam)
        st = t.oracle_step(kind_s, lam)
        got = SC.assembly_errors(t.po, t.Jc, t.f, lam, S, rhs, R["S"], R["rhs"], t.Jp)
        orc = SC.assembly_errors(t.po, t.Jc, t.f, lam, st["S"].astype(np.float64), st["rhs"].astype(np.float64), R["S"], R["rhs"], t.Jp)
        if not all(np.isfinite(v) for v in orc.values()):
            # the fp32 oracle's CHOLESKY elimination breaks down at lambda0 on p21 / ragged / longtracks (a 3 x 3 point block that is
            # singular in fp32): the fp64 oracle on the same J instead, its error scaled by eps32 / eps64
            s64 = O.step(kind_s, t.po, t.Jc, t.Jp, t.f, lam)
            o64 = SC.assembly_errors(t.po, t.Jc, t.f, lam, s64["S"], s64["rhs"], R["S"], R["rhs"], t.Jp)
            orc = {k: v * EPS[1] / EPS[0] for k, v in o64.items()}
        for k in ("S", "rhs"):
            ck("%s@%.0e(oracle %.1e)" % (k, lam, orc[k]), got[k], max(10 * orc[k], t.bound(k)))
    ck.done()


# ---- dense QR (no S) -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prob,kind,scalar", [("p21", 0, 0), ("p21", 3, 0), ("p39", 0, 1)], ids=["p21-qrkit-f64", "p21-moreqr-f64", "p39-qrkit-f32"])
def test_dense_qr_step(ba, O, gpu_ok, prob21, prob39, monkeypatch, prob, kind, scalar):
    """QRKIT / MOREQR never form S: their camera step comes from the dense Householder QR of J2bot (ba_qr.hip.h).  eta of that step
    against the quad S and rhs assembled from the GPU's own J -- the elimination's rounding is in it, so the bound is 10x an fp64
    QR solver fed the same J (the oracle's MOREQR, TSQR: its QRKIT loop takes minutes on problem-21), or the floor.  fp32 (config 3's
    shape, problem-39): the floor alone (the fp32 oracle's dense QR takes ~1/2 minute per trial).  Measured worst: fp64 1.9e-17
    (oracle 6.2e-17 ... 7.7e-17), fp32 4.5e-9."""
    moreqr_route(kind, monkeypatch, O)
    ck = Checker("dense_qr[%s,%d,%d]" % (prob, kind, scalar))
    t = Trial(ba, O, prob21 if prob == "p21" else prob39, kind, scalar, ck)
    t.check_linearization()
    lam0 = 1e-6 * np.sqrt(t.dmax) if kind == ba.MOREQR else 1e-12 * t.dmax
    lams = (lam0,) if scalar == 1 else (lam0, 10.0)
    for lam in lams:
        dx, _, _ = t.step(lam, False)
        R = O.referee_reduced_from_jacobian(ba.CHOLESKY, t.po, t.Jc, t.Jp, t.f, lam)
        got = SC.eta(R["S"], dx[3 * t.po.M:], R["rhs"])
        if scalar == 0:
            st = t.oracle_step(O.MOREQR, lam, want_S=False)
            orc = SC.eta(R["S"], st["dx"][3 * t.po.M:], R["rhs"])
            ck("qr_eta@%.0e(oracle %.1e)" % (lam, orc), got, max(10 * orc, t.bound("qr_eta")))
        else:
            ck("qr_eta@%.0e" % lam, got, t.bound("qr_eta"))
    ck.done()
