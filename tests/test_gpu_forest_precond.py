"""GPU: BA_PRECOND_CONSTRAINT_FOREST (ba_solver_set_preconditioner) against tests/forest_checks.py.

  1. apply and recurrence   x_1 (= alpha_0 M^-1 rhs: the two sweeps directly), x_2, x_3, x_4, x_7 of a solve capped at k iterations
                            against the long double PCG under the forest M on the quad S and rhs of the GPU's own J plus the
                            constraints' blocks; pcg_checks.iterate_error, bound max(10 x the working-precision CPU PCG with the same M,
                            test_gpu_pcg_stages.py's FLOOR); one tree, several trees at N = 257, cut trees, a star, the root fixed
  2. iterations             a stiff chain on which the CPU references need three times fewer iterations under the forest:
                            last_iters <= k_ref + test_gpu_pcg_stages.py's allowance, converged, the quad residual <= 2 rel_tol
  3. bits                   eager = graph = repeated; BLOCK_JACOBI behind CONSTRAINT_FOREST is a solver that never called it; a forest
                            without a kept edge is block Jacobi; preconditioner_info = forest_plan's counts
  4. refusals               leave the solver's bits alone
  5. ba_minimize            every solve converges at the default max_iter where block Jacobi's reference does not

Each value is printed as `FOREST <case> <metric> <value> <bound>`.
"""
import numpy as np
import pytest

import forest_checks as FC
import pcg_checks as PCG
import relpose_checks as RC
from test_gpu_parity import _ragged_problem
from test_gpu_pcg_stages import FLOOR, allowance, quad_rel_residual
from test_gpu_stages import EPS, sorted_oracle_problem

pytestmark = pytest.mark.gpu
F64, LD = np.float64, np.longdouble
SN = {0: "f64", 1: "f32"}
DT = {0: np.float64, 1: np.float32}
KS = (1, 2, 3, 4, 7)


class Checker:
    def __init__(self, case):
        self.case, self.rows = case, []

    def __call__(self, metric, value, bound):
        self.rows.append((metric, float(value), float(bound)))
        print("FOREST %s %s %.3e %.1e" % (self.case, metric, value, bound))

    def done(self):
        bad = [r for r in self.rows if not (r[1] <= r[2])]
        assert not bad, (self.case, bad)


_PROBLEMS, _CONSTRAINTS, _SYSTEMS = {}, {}, {}


def _problem(ba, name, prob21):
    if name not in _PROBLEMS:
        _PROBLEMS[name] = {"p21": lambda: prob21, "ragged": lambda: _ragged_problem(ba),
                           "syn257": lambda: ba.Problem.synthetic(257, 12 * 257, 60 * 257, 4257)}[name]()
    return _PROBLEMS[name]


def _constraints(ba, O, pg, name):
    """relpose_checks.standard_constraints of a problem (an odometry chain over all cameras + a hub), sized from the fp64 linearisation
    at the start state, once per problem."""
    if name not in _CONSTRAINTS:
        po = sorted_oracle_problem(O, pg)
        s = ba.Solver(pg, ba.ITERSCHUR, ba.F64)
        s.linearize()
        V = np.zeros((pg.N, 9))
        np.add.at(V, po.cam_idx, (s.get(ba.GET_JC).reshape(-1, 2, 9) ** 2).sum(axis=1))
        _CONSTRAINTS[name] = RC.standard_constraints(pg.N, po.cam_idx, po.pt_idx, s.get(ba.GET_CAMS), V)[0]
    return _CONSTRAINTS[name]


def subset(cs, idx, stiff=(1.0, 1.0)):
    """The constraints `idx` of cs with their square-root information scaled: L_t by stiff[0], L_r by stiff[0] stiff[1]."""
    return RC.Constraints(cs.pairs[idx], cs.R0[idx], cs.t0[idx], stiff[0] * stiff[1] * cs.Lr[idx], stiff[0] * cs.Lt[idx])


def variant(cs, N, what, stiff=(1.0, 1.0)):
    n = len(cs)
    if what == "all":
        return subset(cs, np.arange(n), stiff)
    if what == "chain":
        return subset(cs, np.arange(N - 1), stiff)
    if what == "star":  # the hub's constraints alone
        return subset(cs, np.arange(N - 1, n), stiff)
    raise KeyError(what)


def _rounded(cs, scalar):
    return cs.rounded(np.float32) if scalar == 1 else cs


class System:
    """The quad S and rhs of a linearisation (J, residuals and g as the solver returns them) plus the constraints' blocks, the
    documented B_a, the cross blocks H in list order and V_a + lambda I, all in long double."""

    def __init__(self, O, po, Jc, Jp, f, g, cams, cs, cm, lam):
        D = 9 * po.N
        d = RC.direct(cs, po.N, cams, cm)
        R = O.referee_reduced_from_jacobian(O.CHOLESKY, po, Jc, Jp, f, lam)
        self.S_ld, self.rhs_ld = RC.reduced(R["S"].reshape(D, D), R["rhs"], d)
        self.S, self.rhs = self.S_ld.astype(F64), self.rhs_ld.astype(F64)
        self.B = PCG.documented_blocks(po, Jc, Jp, lam, R["S"]) + d["V"]
        self.V = PCG.camera_blocks(po, Jc, lam) + d["V"]
        self.H = np.stack([d["cross"][(int(a), int(b))] for a, b in cs.pairs]) if len(cs) else np.zeros((0, 6, 6), LD)
        self.gc = np.asarray(g)[3 * po.M:]
        self.N, self.pairs = po.N, cs.pairs

    def working_blocks(self, dt):
        """B and rhs as k_pcg_prec_reduce forms them in dt (pcg_checks.yardstick)."""
        B = np.asarray(self.V).astype(dt) - (self.V - self.B).astype(dt)
        rhs = np.asarray(self.gc).astype(dt) - (np.asarray(self.gc, LD) - self.rhs_ld).astype(dt)
        return B, rhs

    def reference(self, pl, max_iter, rel_tol=0.0, keep=None):
        Dinv, G, ok = FC.factor(self.B, self.H, self.pairs, pl)
        assert ok.all()
        return FC.pcg(self.S_ld, self.rhs, FC.forest(pl, Dinv, G), max_iter, rel_tol, keep=keep)

    def block_jacobi_reference(self, max_iter, rel_tol):
        Minv, ok = PCG.invert_blocks(self.B)
        assert ok.all()
        return PCG.pcg(self.S_ld, self.rhs, Minv, max_iter, rel_tol)

    def yardstick(self, pl, dt, max_iter, keep):
        """(the PCG in dt under the working-precision factor of the same forest or None when it breaks down, trees that fell back)."""
        B, rhs = self.working_blocks(dt)
        Dw, Gw, bad = FC.working(B, self.H, self.pairs, pl, dt)
        out = FC.pcg(self.S_ld, rhs, FC.forest(pl, Dw, Gw), max_iter, dtype=dt, keep=keep, V=self.V)
        if not all(np.all(np.isfinite(v.astype(F64))) for v in out["xs"].values()):
            return None, bad
        return out, bad


def gpu_system(ba, O, pg, cs, scalar, cm, lam_rel, kind=1, max_tree=0):
    """(solver at its linearisation with the constraints, the preconditioner and the mask set, System, lambda)."""
    po = sorted_oracle_problem(O, pg)
    s = ba.Solver(pg, ba.ITERSCHUR, scalar)
    cs.apply(s)
    s.set_preconditioner(kind, max_tree)
    if cm is not None:
        s.set_constant(cm, None)
    e, dmax = s.linearize()
    lam = lam_rel * dmax
    Jc, Jp = s.get(ba.GET_JC).reshape(po.K, 2, 9), s.get(ba.GET_JP).reshape(po.K, 2, 3)
    return s, System(O, po, Jc, Jp, s.get(ba.GET_RESIDUALS), s.get(ba.GET_GRAD), s.get(ba.GET_CAMS), cs, cm, lam), lam


def _shared_system(ba, O, prob21, prob, what, scalar, masked):
    """One solver and one System per (problem, constraint set, scalar type, mask): the cases differ in max_tree alone."""
    key = (prob, what, scalar, masked)
    if key not in _SYSTEMS:
        pg = _problem(ba, prob, prob21)
        cs = _rounded(variant(_constraints(ba, O, pg, prob), pg.N, what), scalar)
        cm = pg.gauge_mask(0) if masked else None  # (camera 0, the root of the chain's tree, has its pose fixed)
        _SYSTEMS[key] = gpu_system(ba, O, pg, cs, scalar, cm, 1e-6) + (cs, cm)
    return _SYSTEMS[key]


# ---- 1. apply and recurrence -----------------------------------------------------------------------------------------------------------------
# (problem, constraints, max_tree (0: N), mask)
APPLY_CASES = [("p21", "all", 0, False), ("syn257", "all", 64, False), ("syn257", "all", 0, False), ("p21", "all", 5, False),
               ("ragged", "all", 5, False), ("p21", "star", 0, False), ("p21", "all", 0, True)]


@pytest.mark.parametrize("scalar", [0, 1], ids=["f64", "f32"])
@pytest.mark.parametrize("prob,what,max_tree,masked", APPLY_CASES,
                         ids=["p21-one-tree", "syn257-trees-of-64", "syn257-one-tree", "p21-cut-at-5", "ragged-cut-at-5", "p21-star", "p21-root-fixed"])
def test_iterates_under_the_forest(ba, O, gpu_ok, prob21, prob, what, max_tree, masked, scalar):
    """x_1, x_2, x_3, x_4, x_7 at lambda = 1e-6 max diag J'J.  syn257 with one tree (257 cameras) is the tree that does not fit the
    sweeps' LDS; with trees of 64 it has four trees and a lone camera and two blocks of per-camera partials."""
    s, Y, lam, cs, cm = _shared_system(ba, O, prob21, prob, what, scalar, masked)
    N = Y.N
    mt = max_tree or N
    s.set_preconditioner(ba.PRECOND_CONSTRAINT_FOREST, mt)
    pl = FC.plan(N, cs.pairs, mt)
    info = s.preconditioner_info()
    assert (info["kind"], info["max_tree"], info["trees"], info["kept"], info["dropped"], info["largest_tree"]) == (1, mt) + FC.counts(pl)
    ck = Checker("%s,%s,max_tree=%d%s,%s" % (prob, what, mt, ",root fixed" if masked else "", SN[scalar]))
    ref = Y.reference(pl, max(KS), keep=KS)
    dt, scale = DT[scalar], 1.0
    yard, bad = Y.yardstick(pl, dt, max(KS), KS)
    if yard is None or bad:  # fp32 broke down: the fp64 yardstick scaled by eps32 / eps64 (test_gpu_stages.py's rule)
        yard, bad64 = Y.yardstick(pl, F64, max(KS), KS)
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
    ck("fallback_trees(yardstick %d)" % bad, s.preconditioner_info()["fallback_trees"], bad)
    ck.done()


# ---- 2. iterations ---------------------------------------------------------------------------------------------------------------------------
# The chain of the standard constraints with L_t x 10 and L_r x 3: the chain's cross blocks dominate the cameras' own blocks.  Chosen on
# the CPU with the oracle's J of problem-21 at lambda = 1e-6 max diag J'J: the long double references need 195 iterations under block
# Jacobi and 30 under the forest of two trees (max_tree = 16) at rel_tol 1e-8, 134 and 23 at 1e-4.
STIFF = (10.0, 0.3)
STIFF_MAX_TREE = 16


@pytest.mark.parametrize("scalar", [0, 1], ids=["f64", "f32"])
def test_iterations_on_a_stiff_chain(ba, O, gpu_ok, prob21, scalar):
    pg = prob21
    N = pg.N
    cs = _rounded(variant(_constraints(ba, O, pg, "p21"), N, "chain", STIFF), scalar)
    s, Y, lam = gpu_system(ba, O, pg, cs, scalar, None, 1e-6, ba.PRECOND_CONSTRAINT_FOREST, STIFF_MAX_TREE)
    tol = 1e-8 if scalar == 0 else 1e-4
    pl = FC.plan(N, cs.pairs, STIFF_MAX_TREE)
    k_bj, k_fo = Y.block_jacobi_reference(2000, tol), Y.reference(pl, 2000, tol)
    assert k_bj["converged"] and k_fo["converged"]
    print("FOREST stiff chain,%s k_ref block Jacobi %d forest %d" % (SN[scalar], k_bj["iters"], k_fo["iters"]))
    assert k_bj["iters"] >= 3 * k_fo["iters"], (k_bj["iters"], k_fo["iters"])
    ck = Checker("stiff chain,%s" % SN[scalar])
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
    print("FOREST stiff chain,%s device iterations: forest %d, block Jacobi %d" % (SN[scalar], st["last_iters"], s.pcg_stats()["last_iters"]))
    ck.done()


# ---- 3. bits ---------------------------------------------------------------------------------------------------------------------------------
def _observe(ba, s, trials=3):
    out = [np.array(s.linearize())]
    lam = 1e-9 * out[0][1]
    for _ in range(trials):
        out.append(np.array(s.try_step(lam)))
        out += [s.get(w).copy() for w in (ba.GET_DX, ba.GET_CAMS_TEST, ba.GET_POINTS_TEST)]
        st = s.pcg_stats()
        out.append(np.array([st["last_iters"], st["last_converged"], st["last_rel_residual"]]))
        lam *= 100
    return out


def _same(x, y, what):
    for k, (a, b) in enumerate(zip(x, y)):
        assert np.array_equal(a, b), (what, k)


@pytest.mark.parametrize("scalar", [0, 1], ids=["f64", "f32"])
def test_bits(ba, O, gpu_ok, prob21, scalar):
    pg, N = prob21, prob21.N
    cs = _rounded(_constraints(ba, O, pg, "p21"), scalar)

    def solver(kind=None, max_tree=0, with_cs=True):
        s = ba.Solver(pg, ba.ITERSCHUR, scalar)
        if with_cs:
            cs.apply(s)
        if kind is not None:
            s.set_preconditioner(kind, max_tree)
        return s

    # the forest: repeated, and the rows of ba_minimize (captured graphs) against an eager host loop
    f1 = solver(ba.PRECOND_CONSTRAINT_FOREST, 8)
    a = _observe(ba, f1)
    _same(a, _observe(ba, f1), "repeated")
    _same(a, _observe(ba, solver(ba.PRECOND_CONSTRAINT_FOREST, 8)), "second solver")
    g = solver(ba.PRECOND_CONSTRAINT_FOREST, 8)
    rows = g.minimize(max_trials=1)["trace"]
    h = solver(ba.PRECOND_CONSTRAINT_FOREST, 8)
    e, dmax = h.linearize()
    assert rows[0, 2] == e
    h.try_step(float(DT[scalar](1e-12 * dmax)))
    for w in (ba.GET_DX, ba.GET_CAMS_TEST, ba.GET_POINTS_TEST):
        assert np.array_equal(g.get(w), h.get(w)), ("graph", w)
    sg, sh = g.pcg_stats(), h.pcg_stats()
    assert (sg["last_iters"], sg["last_rel_residual"]) == (sh["last_iters"], sh["last_rel_residual"])
    # it is another preconditioner
    plain = _observe(ba, solver())
    assert not np.array_equal(a[2], plain[2])
    # BLOCK_JACOBI behind CONSTRAINT_FOREST (trials run, graphs captured) is the solver that never called it
    f1.minimize(max_trials=2)
    f1.set_state(solver().get(ba.GET_CAMS), pg.arrays()["pts"])
    f1.set_preconditioner(ba.PRECOND_BLOCK_JACOBI)
    _same(plain, _observe(ba, f1), "back to block Jacobi")
    # a forest without a kept edge is block Jacobi
    _same(plain, _observe(ba, solver(ba.PRECOND_CONSTRAINT_FOREST, 1)), "max_tree = 1")
    none = _observe(ba, solver(with_cs=False))
    _same(none, _observe(ba, solver(ba.PRECOND_CONSTRAINT_FOREST, 8, with_cs=False)), "no constraints")
    # set_relative_poses behind set_preconditioner rebuilds the forest; removing the constraints removes it
    late = ba.Solver(pg, ba.ITERSCHUR, scalar)
    late.set_preconditioner(ba.PRECOND_CONSTRAINT_FOREST, 8)
    assert late.preconditioner_info()["trees"] == 0
    cs.apply(late)
    pl = FC.plan(N, cs.pairs, 8)
    i = late.preconditioner_info()
    assert (i["trees"], i["kept"], i["dropped"], i["largest_tree"]) == FC.counts(pl) and i["trees"] > 1
    _same(a, _observe(ba, late), "constraints behind the preconditioner")
    with_forest = late.device_bytes()
    late.set_preconditioner(ba.PRECOND_BLOCK_JACOBI)
    assert late.device_bytes() < with_forest  # (ba_solver_device_bytes counts the forest's buffers)
    late.set_preconditioner(ba.PRECOND_CONSTRAINT_FOREST, 8)
    RC.Constraints().apply(late)
    assert late.preconditioner_info()["trees"] == 0
    _same(none, _observe(ba, late), "constraints removed")


# ---- 4. refusals -----------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_solver_unchanged(ba, O, gpu_ok, prob21):
    cs = _constraints(ba, O, prob21, "p21")
    c = ba.Solver(prob21, ba.CHOLESKY, ba.F64)
    with pytest.raises(ba.BAError) as e:
        c.set_preconditioner(ba.PRECOND_CONSTRAINT_FOREST, 8)
    assert e.value.code == ba.ERR_ARG
    with pytest.raises(ba.BAError) as e:
        c.preconditioner_info()
    assert e.value.code == ba.ERR_ARG
    s = ba.Solver(prob21, ba.ITERSCHUR, ba.F64)
    cs.apply(s)
    s.set_preconditioner(ba.PRECOND_CONSTRAINT_FOREST, 8)
    before, info, nbytes = _observe(ba, s, 1), s.preconditioner_info(), s.device_bytes()
    for kind, mt in ((2, 8), (-1, 8), (ba.PRECOND_CONSTRAINT_FOREST, -1), (ba.PRECOND_BLOCK_JACOBI, -3)):
        with pytest.raises(ba.BAError) as e:
            s.set_preconditioner(kind, mt)
        assert e.value.code == ba.ERR_ARG, (kind, mt)
    assert s.preconditioner_info() == info and s.device_bytes() == nbytes
    _same(before, _observe(ba, s, 1), "behind the refusals")
    s.set_preconditioner(ba.PRECOND_CONSTRAINT_FOREST)  # 0: the default
    assert s.preconditioner_info()["max_tree"] > 1


# ---- 5. ba_minimize --------------------------------------------------------------------------------------------------------------------------
# L_t x 30, L_r x 3 (an odometry whose translations are the stiff part): with the oracle's J at the first trial's lambda (1e-12 max diag
# J'J) and rel_tol 1e-6 the references need 192 iterations under block Jacobi and 9 under the forest with the chain in one tree.  (With L_r stiffened
# alike block Jacobi's reference stays at 97 ... 99 iterations however stiff the chain: just inside the default cap.)
MINIMIZE_STIFF = (30.0, 0.1)


def test_minimize_converges_where_block_jacobi_does_not(ba, O, gpu_ok, prob21):
    """problem-21 with the stiff chain, the defaults of a new solver (max_iter 100, rel_tol 1e-6).  On the first linearisation at the
    first trial's lambda the CPU reference converges within 100 iterations under the forest and does not under block Jacobi; on the
    device every solve of four LM rows converges: a run capped at 200 iterations does the same iterations, and leaves the same state."""
    pg, N = prob21, prob21.N
    cs = variant(_constraints(ba, O, pg, "p21"), N, "chain", MINIMIZE_STIFF)
    s, Y, lam = gpu_system(ba, O, pg, cs, 0, None, 1e-12, ba.PRECOND_CONSTRAINT_FOREST, 0)
    mt = s.preconditioner_info()["max_tree"]  # (the library's default)
    k_fo, k_bj = Y.reference(FC.plan(N, cs.pairs, mt), 100, 1e-6), Y.block_jacobi_reference(100, 1e-6)
    print("FOREST minimize: reference iterations forest %d (converged %d), block Jacobi %d (converged %d)"
          % (k_fo["iters"], k_fo["converged"], k_bj["iters"], k_bj["converged"]))
    assert k_fo["converged"] and not k_bj["converged"]
    runs = []
    for cap in (100, 200):
        m = ba.Solver(pg, ba.ITERSCHUR, ba.F64)
        cs.apply(m)
        m.set_preconditioner(ba.PRECOND_CONSTRAINT_FOREST)
        if cap != 100:
            m.set_pcg(cap, 1e-6)
        r = m.minimize(max_trials=4)
        st = m.pcg_stats()
        print("FOREST minimize: cap %d solves %d total_iters %d last_iters %d converged %d" % (cap, st["solves"], st["total_iters"], st["last_iters"], st["last_converged"]))
        runs.append((st, r["trace"], m.get(ba.GET_CAMS)))
    (s1, t1, c1), (s2, t2, c2) = runs
    assert s1["solves"] >= 4 and s1["last_converged"] == 1 and s1["total_iters"] < 100 * s1["solves"]
    assert s1["solves"] == s2["solves"] and s1["total_iters"] == s2["total_iters"]  # (no solve of the first run stopped at its cap)
    assert np.array_equal(t1[:, :5], t2[:, :5]) and np.array_equal(c1, c2)
    b = ba.Solver(pg, ba.ITERSCHUR, ba.F64)
    cs.apply(b)
    b.linearize()
    b.try_step(lam)
    sb = b.pcg_stats()
    print("FOREST minimize: block Jacobi's first trial on the device: %d iterations, converged %d" % (sb["last_iters"], sb["last_converged"]))
