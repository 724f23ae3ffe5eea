"""GPU: BA_PRECOND_VISIBILITY_FOREST (ba_solver_set_preconditioner) against tests/visibility_checks.py, in the
pattern of tests/test_gpu_forest_precond.py (its System, Checker and constraints; test_gpu_pcg_stages.py's FLOOR and allowance).

  1. iterates      x_1 (= alpha_0 M^-1 rhs: the edge blocks, the factor and the two sweeps directly), x_2, x_3, x_4, x_7 of a solve capped
                   at k iterations against the long double PCG under the same M on the quad S and rhs of the GPU's own J; bound
                   max(10 x the working-precision CPU PCG under the same M, FLOOR); fixed entries exactly 0; fallback_trees = the
                   yardstick's.  The cases are visibility_checks.GPU_CASES (tests/test_visibility_checks.py shows M positive definite
                   for each of them on the oracle's J).
  2. iterations    problem-39, rel_tol 1e-8: last_iters <= k_ref + allowance(k_ref), converged, the quad residual <= 2 rel_tol
  3. bits          eager = graph = repeated; BLOCK_JACOBI or CONSTRAINT_FOREST behind VISIBILITY_FOREST is the solver that never set the
                   new kind; max_tree = 1 is block Jacobi; preconditioner_info = the plan's counts over L
  4. refusals      leave the solver's bits alone
  5. ba_minimize   problem-21, max_trials = 8: every solve converges at the default cap, no more PCG iterations in all than block Jacobi

Each value is printed as `VIS <case> <metric> <value> <bound>`.
"""
import numpy as np
import pytest

import forest_checks as FC
import pcg_checks as PCG
import relpose_checks as RC
import visibility_checks as VC
from test_gpu_forest_precond import Checker as _ForestChecker
from test_gpu_forest_precond import System, _constraints, _observe, _rounded, _same, gpu_system
from test_gpu_parity import _ragged_problem
from test_gpu_pcg_stages import FLOOR, allowance, quad_rel_residual
from test_gpu_stages import EPS

pytestmark = pytest.mark.gpu
F64, LD = np.float64, np.longdouble
SN = {0: "f64", 1: "f32"}
DT = {0: np.float64, 1: np.float32}
KS = (1, 2, 3, 4, 7)


class Checker(_ForestChecker):
    def __call__(self, metric, value, bound):
        self.rows.append((metric, float(value), float(bound)))
        print("VIS %s %s %.3e %.1e" % (self.case, metric, value, bound))


_PROBLEMS, _SYSTEMS = {}, {}


def _problem(ba, name, prob21):
    if name not in _PROBLEMS:
        _PROBLEMS[name] = {"p21": lambda: prob21, "ragged": lambda: _ragged_problem(ba), "twice": lambda: VC.twice_problem(ba),
                           "syn257": lambda: ba.Problem.synthetic(257, 12 * 257, 60 * 257, 4257)}[name]()
    return _PROBLEMS[name]


def _shared_system(ba, O, prob21, prob, with_cs, scalar, masked):
    """One solver and one System per (problem, constraints, scalar type, mask): the cases differ in max_tree alone."""
    key = (prob, with_cs, scalar, masked)
    if key not in _SYSTEMS:
        pg = _problem(ba, prob, prob21)
        cs = _rounded(_constraints(ba, O, pg, prob), scalar) if with_cs else RC.Constraints()
        cm = pg.gauge_mask(0) if masked else None  # (camera 0, the root of its tree, has its pose fixed)
        _SYSTEMS[key] = gpu_system(ba, O, pg, cs, scalar, cm, VC.LAM_REL, ba.PRECOND_VISIBILITY_FOREST, 0) + (cs, cm, pg.covisibility()[0])
    return _SYSTEMS[key]


def _forest(Y, cs, cov, max_tree):
    pl, L = VC.plan(Y.N, cs.pairs, cov, max_tree)
    return pl, L, VC.cross_blocks(Y.S_ld, L, pl["kept"])


def _reference(Y, pl, L, X, max_iter, rel_tol=0.0, keep=None):
    Dinv, G, ok = VC.factor(Y.B, X, L, pl)
    assert ok.all()
    return FC.pcg(Y.S_ld, Y.rhs, FC.forest(pl, Dinv, G), max_iter, rel_tol, keep=keep)


def _yardstick(Y, pl, L, X, dt, max_iter, keep):
    """(the PCG in dt under the working-precision factor of the same forest or None when it breaks down, trees that fell back)."""
    B, rhs = Y.working_blocks(dt)
    Dw, Gw, bad = VC.working(B, X, L, pl, dt)
    out = FC.pcg(Y.S_ld, rhs, FC.forest(pl, Dw, Gw), max_iter, dtype=dt, keep=keep, V=Y.V)
    if not all(np.all(np.isfinite(v.astype(F64))) for v in out["xs"].values()):
        return None, bad
    return out, bad


def _info_counts(s):
    i = s.preconditioner_info()
    return (i["kind"], i["max_tree"], i["trees"], i["kept"], i["dropped"], i["largest_tree"])


# ---- 1. iterates -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scalar", [0, 1], ids=["f64", "f32"])
@pytest.mark.parametrize("case", list(VC.GPU_CASES))
def test_iterates_under_the_visibility_forest(ba, O, gpu_ok, prob21, case, scalar):
    """x_1, x_2, x_3, x_4, x_7 at lambda = 1e-6 max diag J'J.  syn257 as one tree does not fit the sweeps' LDS; with trees of 64 it has
    several trees and two blocks of per-camera partials; with the constraints set their edges come first in L and H_ab is part of X."""
    prob, max_tree, with_cs, masked = VC.GPU_CASES[case]
    s, Y, lam, cs, cm, cov = _shared_system(ba, O, prob21, prob, with_cs, scalar, masked)
    N = Y.N
    mt = max_tree or N
    s.set_preconditioner(ba.PRECOND_VISIBILITY_FOREST, mt)
    pl, L, X = _forest(Y, cs, cov, mt)
    assert _info_counts(s) == (ba.PRECOND_VISIBILITY_FOREST, mt) + FC.counts(pl)
    ck = Checker("%s,%s" % (case, SN[scalar]))
    ref = _reference(Y, pl, L, X, max(KS), keep=KS)
    dt, scale = DT[scalar], 1.0
    yard, bad = _yardstick(Y, pl, L, X, dt, max(KS), KS)
    if yard is None or bad:  # fp32 broke down: the fp64 yardstick scaled by eps32 / eps64 (test_gpu_stages.py's rule)
        yard, bad64 = _yardstick(Y, pl, L, X, F64, max(KS), KS)
        assert yard is not None and bad64 == 0
        scale = EPS[1] / EPS[0]
    fx = np.zeros(9 * N, bool) if cm is None else ((np.asarray(cm, np.int64)[:, None] >> np.arange(9)[None, :]) & 1 == 1).ravel()
    for k in KS:
        s.set_pcg(k, 1e-30)
        s.try_step(lam)
        st = s.pcg_stats()
        xk = s.get(ba.GET_DX)[-9 * N:]
        yd = scale * PCG.iterate_error(yard["xs"][k], ref["xs"][k], Y.S)
        ck("x%d(yardstick %.1e, worst camera %d)" % (k, yd, PCG.worst_camera(xk, ref["xs"][k], Y.S)), PCG.iterate_error(xk, ref["xs"][k], Y.S),
           max(10 * yd, FLOOR[("iterate", scalar)]))
        ck("x%d_capped" % k, 0 if (st["last_iters"] == k and st["last_converged"] == 0) else 1, 0)
        ck("x%d_fixed_nonzero" % k, np.count_nonzero(xk[fx]), 0)
    fb = s.preconditioner_info()["fallback_trees"]
    ck("fallback_trees(yardstick %d)" % bad, abs(fb - bad), 0)
    ck.done()


# ---- 2. iterations ---------------------------------------------------------------------------------------------------------------------------
def test_iterations_on_problem_39(ba, O, gpu_ok, prob39):
    """problem-39 in one tree at lambda = 1e-6 max diag J'J and rel_tol 1e-8 (fp64; tests/test_visibility_checks.py: the references need 31
    iterations under the forest, 54 under block Jacobi on the oracle's J)."""
    pg, N, tol = prob39, prob39.N, 1e-8
    cs = RC.Constraints()
    s, Y, lam = gpu_system(ba, O, pg, cs, 0, None, VC.LAM_REL, ba.PRECOND_VISIBILITY_FOREST, N)
    pl, L, X = _forest(Y, cs, pg.covisibility()[0], N)
    k_fo, k_bj = _reference(Y, pl, L, X, 2000, tol), Y.block_jacobi_reference(2000, tol)
    assert k_fo["converged"] and k_bj["converged"]
    print("VIS problem-39 k_ref block Jacobi %d forest %d" % (k_bj["iters"], k_fo["iters"]))
    ck = Checker("problem-39,f64")
    s.set_pcg(2000, tol)
    s.try_step(lam)
    st = s.pcg_stats()
    k_ref = k_fo["iters"]
    ck("iterations(k_ref %d)" % k_ref, st["last_iters"], k_ref + allowance(k_ref))
    ck("converged", 0 if st["last_converged"] == 1 else 1, 0)
    ck("rel_residual", quad_rel_residual(O, Y.S, s.get(ba.GET_DX)[-9 * N:], Y.rhs), 2 * tol)
    ck("fallback_trees", s.preconditioner_info()["fallback_trees"], 0)
    s.set_preconditioner(ba.PRECOND_BLOCK_JACOBI)
    s.try_step(lam)
    print("VIS problem-39 device iterations: forest %d, block Jacobi %d" % (st["last_iters"], s.pcg_stats()["last_iters"]))
    ck.done()


# ---- 3. bits ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scalar", [0, 1], ids=["f64", "f32"])
def test_bits(ba, O, gpu_ok, prob21, scalar):
    pg, N = prob21, prob21.N
    cs = _rounded(_constraints(ba, O, pg, "p21"), scalar)
    VIS, CF, BJ = ba.PRECOND_VISIBILITY_FOREST, ba.PRECOND_CONSTRAINT_FOREST, ba.PRECOND_BLOCK_JACOBI

    def solver(kind=None, max_tree=0, with_cs=False):
        s = ba.Solver(pg, ba.ITERSCHUR, scalar)
        if with_cs:
            cs.apply(s)
        if kind is not None:
            s.set_preconditioner(kind, max_tree)
        return s

    # the forest: repeated, a second solver, and the rows of ba_minimize (captured graphs) against an eager host loop
    f1 = solver(VIS, 8)
    a = _observe(ba, f1)
    _same(a, _observe(ba, f1), "repeated")
    _same(a, _observe(ba, solver(VIS, 8)), "second solver")
    g = solver(VIS, 8)
    rows = g.minimize(max_trials=1)["trace"]
    h = solver(VIS, 8)
    e, dmax = h.linearize()
    assert rows[0, 2] == e
    h.try_step(float(DT[scalar](1e-12 * dmax)))
    for w in (ba.GET_DX, ba.GET_CAMS_TEST, ba.GET_POINTS_TEST):
        assert np.array_equal(g.get(w), h.get(w)), ("graph", w)
    sg, sh = g.pcg_stats(), h.pcg_stats()
    assert (sg["last_iters"], sg["last_rel_residual"]) == (sh["last_iters"], sh["last_rel_residual"])
    # preconditioner_info = the plan's counts over L, without and with constraints
    cov = pg.covisibility()[0]
    assert _info_counts(f1) == (VIS, 8) + FC.counts(VC.plan(N, np.zeros((0, 2)), cov, 8)[0])
    fc = solver(VIS, 8, with_cs=True)
    assert _info_counts(fc) == (VIS, 8) + FC.counts(VC.plan(N, cs.pairs, cov, 8)[0])
    late = solver(VIS, 8)
    cs.apply(late)  # (set_relative_poses behind set_preconditioner rebuilds the forest)
    assert _info_counts(late) == _info_counts(fc)
    _same(_observe(ba, fc), _observe(ba, late), "constraints behind the preconditioner")
    # it is another preconditioner
    plain = _observe(ba, solver())
    assert not np.array_equal(a[2], plain[2])
    # BLOCK_JACOBI behind VISIBILITY_FOREST (trials run, graphs captured) is the solver that never set the new kind
    f1.minimize(max_trials=2)
    f1.set_state(solver().get(ba.GET_CAMS), pg.arrays()["pts"])
    f1.set_preconditioner(BJ)
    _same(plain, _observe(ba, f1), "back to block Jacobi")
    # max_tree = 1 gives block Jacobi's bits
    one = solver(VIS, 1)
    assert _info_counts(one) == (VIS, 1, 0, 0, len(cov), 1)
    _same(plain, _observe(ba, one), "max_tree = 1")
    # CONSTRAINT_FOREST behind VISIBILITY_FOREST is the solver that never set the new kind
    want = _observe(ba, solver(CF, 8, with_cs=True))
    fc.minimize(max_trials=2)
    fc.set_state(solver().get(ba.GET_CAMS), pg.arrays()["pts"])
    fc.set_preconditioner(CF, 8)
    _same(want, _observe(ba, fc), "back to the constraint forest")
    # the buffers of the forest are counted and leave with it
    with_forest = late.device_bytes()
    late.set_preconditioner(BJ)
    assert late.device_bytes() < with_forest


# ---- 4. refusals -----------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_solver_unchanged(ba, O, gpu_ok, prob21):
    c = ba.Solver(prob21, ba.CHOLESKY, ba.F64)
    with pytest.raises(ba.BAError) as e:
        c.set_preconditioner(ba.PRECOND_VISIBILITY_FOREST, 8)
    assert e.value.code == ba.ERR_ARG
    s = ba.Solver(prob21, ba.ITERSCHUR, ba.F64)
    s.set_preconditioner(ba.PRECOND_VISIBILITY_FOREST, 8)
    before, info, nbytes = _observe(ba, s, 1), s.preconditioner_info(), s.device_bytes()
    for kind, mt in ((2, 8), (4, 8), (-1, 8), (ba.PRECOND_VISIBILITY_FOREST, -1)):
        with pytest.raises(ba.BAError) as e:
            s.set_preconditioner(kind, mt)
        assert e.value.code == ba.ERR_ARG, (kind, mt)
    assert s.preconditioner_info() == info and s.device_bytes() == nbytes
    _same(before, _observe(ba, s, 1), "behind the refusals")
    s.set_preconditioner(ba.PRECOND_VISIBILITY_FOREST)  # 0: the default
    assert s.preconditioner_info()["max_tree"] > 1


# ---- 5. ba_minimize --------------------------------------------------------------------------------------------------------------------------
def test_minimize_needs_no_more_iterations_than_block_jacobi(ba, O, gpu_ok, prob21):
    """problem-21, the defaults of a new solver (max_iter 100, rel_tol 1e-6, the default max_tree), max_trials = 8: every solve converges
    at the default cap -- a run capped at 200 iterations does the same iterations and leaves the same state -- and the PCG iterations of
    the run are no more than block Jacobi's on the same run."""
    pg = prob21
    runs = []
    for kind, cap in ((ba.PRECOND_VISIBILITY_FOREST, 100), (ba.PRECOND_VISIBILITY_FOREST, 200), (ba.PRECOND_BLOCK_JACOBI, 100)):
        m = ba.Solver(pg, ba.ITERSCHUR, ba.F64)
        m.set_preconditioner(kind)
        if cap != 100:
            m.set_pcg(cap, 1e-6)
        r = m.minimize(max_trials=8)
        st = m.pcg_stats()
        print("VIS minimize: kind %d cap %d solves %d total_iters %d last_iters %d converged %d fallback_trees %d"
              % (kind, cap, st["solves"], st["total_iters"], st["last_iters"], st["last_converged"], m.preconditioner_info()["fallback_trees"]))
        runs.append((st, r["trace"], m.get(ba.GET_CAMS)))
    (s1, t1, c1), (s2, t2, c2), (sb, tb, cb) = runs
    assert s1["solves"] >= 8 and s1["last_converged"] == 1 and s1["total_iters"] < 100 * s1["solves"]
    assert s1["solves"] == s2["solves"] and s1["total_iters"] == s2["total_iters"]  # (no solve of the first run stopped at its cap)
    assert np.array_equal(t1[:, :5], t2[:, :5]) and np.array_equal(c1, c2)
    assert sb["solves"] == s1["solves"] and s1["total_iters"] <= sb["total_iters"], (s1, sb)
