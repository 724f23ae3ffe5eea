"""GPU: BA_ITERSCHUR's PCG iterate by iterate against a long double PCG on the quad S and rhs of the GPU's OWN J (tests/pcg_checks.py).

test_gpu_iterative_schur.py checks the end of a solve, which a wrong preconditioner, a stale beta or a lost block of partials still
reaches -- later.  A solve capped at k iterations with a rel_tol it cannot meet (1e-30) returns x_k, so through the public API:

  prefix iterates   x_k, k = 1, 2, 3, 4, 7, at lambda = 1e-6 and 1e-2 x max diag J'J against the reference's x_k (pcg_checks.iterate_error);
                    bound max(10 x the working-precision yardstick's error on the same S at the same k, floor); the yardstick forms
                    S p as the library does, V p minus the eliminated part (pcg_checks.yardstick says why)
  capped residual   at k = 1, 3 and lambda = 1e-6 max diag J'J (at 1e-2 the reference converges in 2 ... 4 iterations and x_3's residual
                    is rounding noise again): the device's |rhs - S x_k| / |rhs| against the quad one of the returned x_k, relative;
                    bound max(10 x the yardstick's deviation, floor); at every k and lambda last_iters == k, not converged
  iterations        at the smaller lambda, rel_tol = 1e-8 (fp32: 1e-4), cap 1000: last_iters <= k_ref + allowance, k_ref the
                    reference's count with the documented B_a; the end of that solve: |S dx_c - rhs| / |rhs| <= 2 rel_tol in quad,
                    converged, the back-substitution at test_gpu_stages.py's bound
  constant params   the gauge mask + one fully fixed camera: the same on the masked S, fixed rows of every x_k exactly 0

on real data, the ragged and long-track problems, two-camera, gc = 2 and gc = 3 problems and cameras with exactly 1 ... 640
observations (CASES).  Each value is printed as `PCG <case> <metric> <value> <bound>`; FLOOR and ALLOWANCE record what an MI355X
measured (profiles/r08_pcg_stages.txt).
"""
import numpy as np
import pytest

import pcg_checks as PC
import stage_checks as SC
from test_gpu_parity import _long_track_problem, _ragged_problem
from test_gpu_stages import BOUND, EPS, sorted_oracle_problem

pytestmark = pytest.mark.gpu

KS = (1, 2, 3, 4, 7)
LAMS = (1e-6, 1e-2)  # x max diag J'J
# A finding of the first MI355X run, moved as the fp32 cases of a breakdown are: synthetic(2, 2, 4) in fp32 at 1e-6 max diag J'J
# (= 8 eps32 max diag).  Two points seen by two cameras leave S = lambda I on most of its space, and the matrix-free product
# V p - (eliminated part) then carries eps32 |V| |p| ~ 0.1 lambda |p|: the solve took 9 iterations for the reference's 5, reported
# convergence at a true residual of 2.5e-3 (rel_tol 1e-4), x_2 was off by 7.5e-2.  The fp32 yardstick in the same matrix-free form
# does the same on the CPU (9 iterations, 1.2e-3, 6.7e-2): a property of the arithmetic, not of a kernel.  The case sits at the
# smallest decade where that yardstick needs no more iterations than the reference (1e-5: 7 for 5, 1e-4: 6 for 5, 1e-3: 5 for 5).
LAMS_MOVED = {("syn2", 1): (1e-3, 1e-2)}
TOL = {0: 1e-8, 1: 1e-4}
CAP = 1000
DT = {0: np.float64, 1: np.float32}
SN = {0: "f64", 1: "f32"}

# Floors under 10 x the yardstick, set from the first MI355X run with at least 10x headroom over the worst value measured over every
# case of this file (that value in the comment).
FLOOR = {
    # iterates.  fp64: the values above 10 x their yardstick were 3.8e-15 (long tracks, x_7 at 1e-2; yardstick 3.6e-16) and, with the
    # rounding luck of another yardstick run, 5.4e-14 (synthetic(600, ...), x_1 at 1e-6; 2.7e-15).  fp32: 2.5e-4 (long tracks, x_3 at
    # 1e-6, camera 1, which sees one point 700 times; yardstick 1.8e-5) and six more of that case at 2.0 ... 2.3e-4; every other case
    # is inside 10 x its yardstick.  Worst values overall: fp64 2.3e-10 (synthetic(2, ...), x_3 at 1e-6; yardstick 1.5e-10: the
    # cancellation of the matrix-free product), otherwise 1.4e-13 (long tracks); fp32 2.5e-4.
    ("iterate", 0): 6e-13, ("iterate", 1): 3e-3,
    # the device's residual under a cap, relative to the quad one (the yardstick's deviation is often exactly 0 in fp64).  Worst above
    # 10 x yardstick: fp64 1.6e-14 (long tracks, k = 3; yardstick 3.5e-16); fp32 1.2e-5 (long tracks, k = 3; 3.5e-7), 1.1e-5 (chunk
    # edges, k = 3; 5.6e-7).  Worst overall: fp64 4.9e-11 (synthetic(2, ...), k = 1; yardstick 1.5e-11), fp32 1.8e-5.
    ("residual", 0): 2e-13, ("residual", 1): 2e-4,
}
# Iterations over k_ref: floor(min(ALLOWANCE_REL k_ref + 2, 0.25 k_ref)).  ALLOWANCE_REL = twice the worst (last_iters - k_ref) / k_ref
# measured: 12 / 55 (long tracks, fp32); then 8 / 70 (long tracks, fp64), 4 / 56 and 2 / 31 (ragged); 0 on the 14 other cases
# (profiles/r08_pcg_stages.txt has the table).  With it the 25 % ceiling decides from k_ref = 11 on.
ALLOWANCE_REL = 0.44

EDGE_COUNTS = (1, 31, 32, 33, 64, 65, 511, 512, 513, 544, 640)
EDGE_CHUNKS = (1, 1, 1, 2, 2, 3, 16, 16, 17, 17, 20)


class Checker:
    """Collects (metric, value, bound), prints every one, asserts them all at the end."""

    def __init__(self, case):
        self.case, self.rows = case, []

    def __call__(self, metric, value, bound):
        self.rows.append((metric, float(value), float(bound)))
        print("PCG %s %s %.3e %.1e" % (self.case, metric, value, bound))

    def done(self):
        bad = [r for r in self.rows if not (r[1] <= r[2])]
        assert not bad, (self.case, bad)


# ---- the cases -------------------------------------------------------------------------------------------------------------------------
def chunk_edge_problem(ba):
    """synthetic(14, 2800, 11200) (747 ... 856 observations per camera) with the last observations of cameras 0 ... 10 dropped so that
    they keep exactly EDGE_COUNTS observations: EDGE_CHUNKS chunks of 32 -- the 16-way loops of k_pcg_prec_reduce / k_pcg_cam alone
    (512), with a single remainder (513, 544), with a 4-way remainder (640), and none of them (1 ... 65)."""
    p = ba.Problem.synthetic(14, 2800, 11200, 160)
    a = p.arrays()
    keep = np.ones(p.K, bool)
    for cam, want in enumerate(EDGE_COUNTS):
        idx = np.nonzero(a["cam_idx"] == cam)[0]
        assert len(idx) >= want, (cam, len(idx))
        keep[idx[want:]] = False
    q = ba.Problem.from_arrays(p.N, p.M, int(keep.sum()), a["cam_idx"][keep], a["pt_idx"][keep], a["meas"].reshape(-1, 2)[keep].ravel(),
                               a["cams9"], a["pts"])
    n = np.bincount(q.arrays()["cam_idx"], minlength=q.N)
    assert tuple(n[:len(EDGE_COUNTS)]) == EDGE_COUNTS and tuple((n[:len(EDGE_COUNTS)] + 31) // 32) == EDGE_CHUNKS, n
    return q


def make_problem(ba, name, prob21=None, prob39=None):
    """(problem, camera mask or None) of a case of CASES."""
    if name in ("p21", "p21fixed"):
        p = prob21
    elif name == "p39":
        p = prob39
    elif name == "ragged":
        p = _ragged_problem(ba)
    elif name == "longtracks":
        p = _long_track_problem(ba)
    elif name == "syn2":
        p = ba.Problem.synthetic(2, 2, 4, 5)
    elif name in ("syn257", "syn600"):
        n = int(name[3:])
        p = ba.Problem.synthetic(n, 12 * n, 60 * n, 4000 + n)
    elif name == "edges":
        p = chunk_edge_problem(ba)
    else:
        raise KeyError(name)
    cm = None
    if name == "p21fixed":  # the gauge mask (reference camera 0) and camera 7 fixed altogether
        cm = p.gauge_mask(0)
        cm[7] = ba.FIX_CAMERA
    return p, cm


CASES = ["p21", "p39", "ragged", "longtracks", "syn2", "syn257", "syn600", "edges", "p21fixed"]


class Reference:
    """The quad S and rhs of one (J, residuals, lambda) with the documented blocks B_a, the long double iterates x_k and the
    working-precision yardstick's errors."""

    def __init__(self, O, po, Jc, Jp, f, gc, lam, scalar, want_count):
        R = O.referee_reduced_from_jacobian(O.CHOLESKY, po, Jc, Jp, f, lam)
        self.S, self.rhs = R["S"], R["rhs"]
        self.B = PC.documented_blocks(po, Jc, Jp, lam, self.S)
        self.Minv, ok = PC.invert_blocks(self.B)
        assert ok.all(), np.nonzero(~ok)[0]
        self.S_ld = self.S.astype(PC.LD)
        self.V = PC.camera_blocks(po, Jc, lam)  # the yardstick forms S p the matrix-free way, as the library does (pcg_checks.yardstick)
        self.ref = PC.pcg(self.S_ld, self.rhs, self.Minv, max(KS), keep=KS)
        dt = DT[scalar]
        self.scale = 1.0
        self.yard = PC.yardstick(self.S_ld, self.rhs, self.B, max(KS), dtype=dt, keep=KS, V=self.V, g=gc)
        self.yard_dtype = dt
        if self.yard is None:  # fp32 broke down: the fp64 yardstick scaled by eps32 / eps64 (test_gpu_stages.py's rule)
            self.yard = PC.yardstick(self.S_ld, self.rhs, self.B, max(KS), dtype=np.float64, keep=KS, V=self.V, g=gc)
            self.yard_dtype = np.float64
            self.scale = EPS[1] / EPS[0]
        assert self.yard is not None
        self.k_ref = None
        if want_count:
            full = PC.pcg(self.S_ld, self.rhs, self.Minv, CAP, TOL[scalar])
            assert full["converged"], full["iters"]  # (a case the reference cannot solve proves nothing)
            self.k_ref = full["iters"]

    def iterate_yardstick(self, k):
        return self.scale * PC.iterate_error(self.yard["xs"][k], self.ref["xs"][k], self.S)

    def residual_yardstick(self, O, k):
        """The yardstick's own |rhs - S x_k| / |rhs| (formed in working precision) against quad for the same x_k, relative."""
        xk = self.yard["xs"][k].astype(np.float64)
        quad = quad_rel_residual(O, self.S, xk, self.rhs)
        return self.scale * abs(PC.working_residual(self.S_ld, xk, self.rhs, self.yard_dtype, V=self.V) - quad) / quad


def quad_rel_residual(O, S, x, rhs):
    num, _ = O.referee_sym_residual(S, x, rhs)  # |S x - b| per row, in quad
    return float(np.linalg.norm(num) / np.linalg.norm(rhs))


def allowance(k_ref):
    return int(np.floor(min(ALLOWANCE_REL * k_ref + 2, 0.25 * k_ref)))


def fixed_rows(N, cm):
    """bool [9N]: the camera unknowns a mask holds constant (bit q of cm[a]: unknown q of camera a)."""
    cmv = np.zeros(N, np.int64) if cm is None else np.asarray(cm, np.int64)
    return ((cmv[:, None] >> np.arange(9)[None, :]) & 1 == 1).ravel()


@pytest.mark.parametrize("scalar", [0, 1], ids=["f64", "f32"])
@pytest.mark.parametrize("case", CASES)
def test_pcg_iterates(ba, O, gpu_ok, prob21, prob39, case, scalar):
    """The module docstring's four checks on one case and one scalar type.  Measured on an MI355X (profiles/r08_pcg_stages.txt): the
    worst values are in FLOOR's and ALLOWANCE_REL's comments; the 18 cases take 106 s (test_gpu_stages.py: 149 s), most of it the quad
    assembly and the long double products of the two largest cases on the host."""
    ck = Checker("%s,%s" % (case, SN[scalar]))
    pg, cm = make_problem(ba, case, prob21, prob39)
    po = sorted_oracle_problem(O, pg)
    s = ba.Solver(pg, ba.ITERSCHUR, scalar)
    if cm is not None:
        s.set_constant(cm, None)
    e, dmax = s.linearize()
    Jc, Jp = s.get(ba.GET_JC).reshape(po.K, 2, 9), s.get(ba.GET_JP).reshape(po.K, 2, 3)
    f, g = s.get(ba.GET_RESIDUALS), s.get(ba.GET_GRAD)
    fx = fixed_rows(po.N, cm)
    if case == "ragged":
        fx[9 * 5:9 * 5 + 9] = True  # the blind camera: B_a = lambda I, rhs_a = 0, its rows of every x_k exactly 0
    for q, x in enumerate(LAMS_MOVED.get((case, scalar), LAMS)):
        lam = x * dmax
        R = Reference(O, po, Jc, Jp, f, g[3 * po.M:], lam, scalar, want_count=q == 0)
        for k in KS:
            s.set_pcg(k, 1e-30)
            et, rs, dn = s.try_step(lam)
            st = s.pcg_stats()
            xk = s.get(ba.GET_DX)[3 * po.M:]
            yd = R.iterate_yardstick(k)
            err = PC.iterate_error(xk, R.ref["xs"][k], R.S)
            ck("x%d@%.0e(yardstick %.1e, worst camera %d)" % (k, x, yd, PC.worst_camera(xk, R.ref["xs"][k], R.S)), err,
               max(10 * yd, FLOOR[("iterate", scalar)]))
            ck("x%d_fixed_nonzero@%.0e" % (k, x), np.count_nonzero(xk[fx]), 0)
            ck("x%d_capped@%.0e" % (k, x), 0 if (st["last_iters"] == k and st["last_converged"] == 0) else 1, 0)
            if k in (1, 3) and q == 0:
                quad = quad_rel_residual(O, R.S, xk, R.rhs)
                yr = R.residual_yardstick(O, k)
                ck("residual%d@%.0e(quad %.3e, yardstick %.1e)" % (k, x, quad, yr), abs(st["last_rel_residual"] - quad) / quad,
                   max(10 * yr, FLOOR[("residual", scalar)]))
        if q == 0:
            tol = TOL[scalar]
            s.set_pcg(CAP, tol)
            s.try_step(lam)
            st = s.pcg_stats()
            dx = s.get(ba.GET_DX)
            k_ref = R.k_ref
            print("PCG %s,%s iterations last_iters %d k_ref %d excess %+d allowed %d" % (case, SN[scalar], st["last_iters"], k_ref,
                                                                                      st["last_iters"] - k_ref, allowance(k_ref)))
            ck("iterations(k_ref %d,allowed %d)" % (k_ref, k_ref + allowance(k_ref)), st["last_iters"], k_ref + allowance(k_ref))
            ck("converged", 0 if st["last_converged"] == 1 else 1, 0)
            ck("rel_residual", quad_rel_residual(O, R.S, dx[3 * po.M:], R.rhs), 2 * tol)
            ck("backsub", SC.backsub_errors(po, Jc, Jp, dx, g, lam), BOUND[("backsub", scalar)])
            ck("dx_fixed_nonzero", np.count_nonzero(dx[3 * po.M:][fx]), 0)
            if case == "ragged":
                ck("empty_point_moved", np.count_nonzero(dx[3 * 77:3 * 77 + 3]), 0)
            if case == "longtracks":  # the cost of the self-entries-only B_a: the count with the exact diagonal blocks of S
                Me, ok = PC.invert_blocks(PC.exact_blocks(R.S, po.N))
                assert ok.all()
                ke = PC.pcg(R.S_ld, R.rhs, Me, CAP, tol)["iters"]
                print("PCG %s,%s iterations k_ref with the exact diagonal blocks of S %d (documented B_a: %d)" % (case, SN[scalar], ke, k_ref))
    ck.done()
