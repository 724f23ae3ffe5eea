"""GPU: the model-decrease stopping rule of BA_ITERSCHUR's PCG (ba_solver_set_pcg_model_tol) against
tests/qstop_checks.py on the quad S and rhs of the GPU's OWN J, never against the library itself.

  1. stop and iterate   per case of qstop_checks.CASES and target (2, 4, half the residual rule's count) an eta from the reference's own zeta
                        sequence with clearance >= 1.2 (choose_eta); one try_step with the rule on and rel_tol = 1e-30: last_iters == k*,
                        last_rule == 2, by_model == 1; BA_GET_DX's camera part against the reference's x_k* (pcg_checks.iterate_error, bound
                        max(10 x the working-precision yardstick, test_gpu_pcg_stages.FLOOR))
  2. zeta and s         last_zeta and last_model of the same solves against the reference's zeta_k* and s_k*, relative; bound max(10 x the
                        yardstick's own deviation, floor); the floors by reasoning: 64 eps for s, 64 eps k* s_k / (s_k - s_{k-1}) for zeta
                        (the cancellation in the difference)
  3. rule order, cap    a rel_tol the residual meets first: last_rule == 1 and the count of the same solve with eta = 0; max_iter below k*:
                        last_rule == 0, at_cap == 1, last_zeta = the reference's zeta at the cap
  4. bits               eager = repeated = the replayed graph of ba_minimize with the rule on; eta > 0 then eta = 0 is the solver that
                        never had the rule, apart from the documented buffer
  5. refusals           each one leaves the solver alone; ba_solver_covariance_pcg is the same bits with the rule on and off
  6. end to end         problem-21 in fp64 to the reference's stop with eta = 0.1: the energy bound of DESIGN.md section 9, fewer iterations

1 and 2 are one test function per case and scalar type (they share the solves and the reference).  Every figure is printed as
`QSTOP <case> <metric> <value> <bound>`.
"""
import numpy as np
import pytest

import pcg_checks as PC
import qstop_checks as Q
from test_gpu_pcg_stages import FLOOR, chunk_edge_problem
from test_gpu_shared_intrinsics import equalise
from test_gpu_stages import EPS, sorted_oracle_problem

pytestmark = pytest.mark.gpu

DT = {0: np.float64, 1: np.float32}
SN = {0: "f64", 1: "f32"}
ETA_E2E = 0.1


class Checker:
    def __init__(self, case):
        self.case, self.rows = case, []

    def __call__(self, metric, value, bound):
        self.rows.append((metric, float(value), float(bound)))
        print("QSTOP %s %s %.3e %.1e" % (self.case, metric, value, bound))

    def done(self):
        bad = [r for r in self.rows if not (r[1] <= r[2])]
        assert not bad, (self.case, bad)


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


_PROBLEMS, _GPU_CASES = {}, {}


def _problem(ba, prob, prob21):
    if prob not in _PROBLEMS:
        _PROBLEMS[prob] = {"p21": lambda: prob21, "syn2": lambda: ba.Problem.synthetic(2, 40, 80, 5), "edges": lambda: chunk_edge_problem(ba),
                           "syn257": lambda: ba.Problem.synthetic(257, 12 * 257, 60 * 257, 4257),
                           "syn600": lambda: ba.Problem.synthetic(600, 12 * 600, 60 * 600, 4600)}[prob]()
    return _PROBLEMS[prob]


def gpu_case(ba, O, prob21, name, scalar):
    """(solver at its linearisation with the case's settings, qstop_checks.Case on its own J, lambda, M), built once per case and type."""
    if (name, scalar) in _GPU_CASES:
        return _GPU_CASES[(name, scalar)]
    prob, lam_rel, what, _ = Q.CASES[name]
    pg = _problem(ba, prob, prob21)
    po = sorted_oracle_problem(O, pg)
    s = ba.Solver(pg, ba.ITERSCHUR, scalar)
    lin = dict(po=po)
    if what == "gauge":
        s.set_constant(pg.gauge_mask(0), None)
    elif what == "group":  # one group of all 21 cameras, their intrinsics equalised through set_state first
        lin["groups"] = [np.arange(pg.N)]
        equalise(ba, s, lin["groups"])
        s.set_shared_intrinsics(np.zeros(pg.N, np.int32))
    elif what == "cforest":  # the odometry chain, sized from the fp64 linearisation at the start state; one tree
        t = ba.Solver(pg, ba.ITERSCHUR, ba.F64)
        t.linearize()
        cs = Q.chain(pg.N, po.cam_idx, po.pt_idx, t.get(ba.GET_CAMS), t.get(ba.GET_JC))
        lin["cs"] = cs.rounded(np.float32) if scalar == 1 else cs
        lin["cs"].apply(s)
        s.set_preconditioner(ba.PRECOND_CONSTRAINT_FOREST, pg.N)
    elif what == "vforest":
        lin["cov"] = pg.covisibility()[0]
        s.set_preconditioner(ba.PRECOND_VISIBILITY_FOREST, pg.N)
    elif what == "marquardt":
        s.set_damping(ba.DAMP_MARQUARDT)
    e, dmax = s.linearize()
    lam = lam_rel if what == "marquardt" else lam_rel * dmax
    lin.update(Jc=s.get(ba.GET_JC).reshape(po.K, 2, 9), Jp=s.get(ba.GET_JP).reshape(po.K, 2, 3), f=s.get(ba.GET_RESIDUALS), g=s.get(ba.GET_GRAD),
               cams=s.get(ba.GET_CAMS), lam=lam)
    _GPU_CASES[(name, scalar)] = (s, Q.Case(O, what, lin), lam, po.M)
    return _GPU_CASES[(name, scalar)]


def yardstick(case, scalar, max_iter, eta, keep):
    """(the working-precision run, the factor its errors are scaled by): fp32 that breaks down is replaced by fp64 scaled by eps32 /
    eps64 (test_gpu_stages.py's rule)."""
    out = case.working(DT[scalar], max_iter, eta=eta, keep=keep)
    if out is not None:
        return out, 1.0
    out = case.working(np.float64, max_iter, eta=eta, keep=keep)
    assert out is not None
    return out, EPS[1] / EPS[0]


def rel(a, b):
    return abs(float(a) - float(b)) / abs(float(b))


def floors(ref, k, scalar):
    """(floor of s, floor of zeta), relative: 64 eps of the scalar type; times k s_k / (s_k - s_{k-1}) for the difference in zeta."""
    eps = EPS[scalar]
    return 64 * eps, 64 * eps * k * ref["s"][k] / (ref["s"][k] - ref["s"][k - 1])


def solve(ba, s, lam, cap, rel_tol, eta):
    s.set_pcg(cap, rel_tol)
    s.set_pcg_model_tol(eta)
    s.pcg_stop_stats(reset=True)
    s.try_step(lam)
    return s.pcg_stats(), s.pcg_stop_stats()


# ---- 1 + 2 -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,scalar", [(n, sc) for n in Q.CASES for sc in Q.CASES[n][3]], ids=["%s-%s" % (n, SN[sc]) for n in Q.CASES for sc in Q.CASES[n][3]])
def test_stop_iterate_zeta_and_model(ba, O, gpu_ok, prob21, name, scalar):
    s, case, lam, M = gpu_case(ba, O, prob21, name, scalar)
    ref = case.reference()
    ck = Checker("%s,%s" % (name, SN[scalar]))
    for eta, ks, clear in Q.chosen(case, scalar):
        yard, scale = yardstick(case, scalar, ks + 8, eta, [ks])
        # (the CPU run in the same arithmetic has to agree on the index, or the comparison of this case and type says nothing)
        assert (yard["iters"], yard["rule"]) == (ks, 2), (name, SN[scalar], eta, ks, yard["iters"], yard["rule"], yard["zeta"])
        st, ss = solve(ba, s, lam, ks + 8, 1e-30, eta)
        print("QSTOP %s,%s eta %.4g (clearance %.2f): k* %d, device last_iters %d last_rule %d by_model %d last_rel_residual %.2e"
              % (name, SN[scalar], eta, clear, ks, st["last_iters"], ss["last_rule"], ss["by_model"], st["last_rel_residual"]))
        ck("stop@k%d" % ks, 0 if (st["last_iters"], ss["last_rule"], ss["by_model"], ss["by_residual"], ss["at_cap"], st["last_converged"])
           == (ks, 2, 1, 0, 0, 1) else 1, 0)
        xk = s.get(ba.GET_DX)[3 * M:]
        yd = scale * PC.iterate_error(yard["xs"][ks], ref["xs"][ks], case.S64)
        ck("x%d(yardstick %.1e, worst camera %d)" % (ks, yd, PC.worst_camera(xk, ref["xs"][ks], case.S64)), PC.iterate_error(xk, ref["xs"][ks], case.S64),
           max(10 * yd, FLOOR[("iterate", scalar)]))
        fs, fz = floors(ref, ks, scalar)
        ys, yz = scale * rel(yard["s"][ks], ref["s"][ks]), scale * rel(yard["zeta"][ks], ref["zeta"][ks])
        ck("last_model@k%d(reference %.6e, yardstick %.1e, floor %.1e)" % (ks, ref["s"][ks], ys, fs), rel(ss["last_model"], ref["s"][ks]), max(10 * ys, fs))
        ck("last_zeta@k%d(reference %.6e, yardstick %.1e, floor %.1e)" % (ks, ref["zeta"][ks], yz, fz), rel(ss["last_zeta"], ref["zeta"][ks]), max(10 * yz, fz))
    s.set_pcg_model_tol(0.0)
    ck.done()


# ---- 3 -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scalar", [0, 1], ids=["f64", "f32"])
def test_rule_order_and_the_cap(ba, O, gpu_ok, prob21, scalar):
    name = "p21@1e-6"
    s, case, lam, M = gpu_case(ba, O, prob21, name, scalar)
    ref = case.reference()
    eta, ks, clear = Q.chosen(case, scalar)[-1]
    assert ks >= 8, ks
    ck = Checker("order[%s,%s]" % (name, SN[scalar]))
    # the residual first: a rel_tol halfway (in the logarithm) between the reference's |r_kr| and everything before it
    # (the last k <= k* / 2 that offers a clearance of 1.2 on both sides: |r_k| is not monotone either)
    rr = np.sqrt(ref["rr"])
    kr = max(k for k in range(1, ks // 2 + 1) if rr[k] * 1.2 ** 2 <= rr[:k].min())
    tol = float(np.sqrt(rr[kr] * rr[:kr].min()))
    assert kr >= 2 and rr[kr] * 1.2 <= tol <= rr[:kr].min() / 1.2, (kr, rr[:kr + 1])
    st, ss = solve(ba, s, lam, ks + 8, tol, eta)
    st0, _ = solve(ba, s, lam, ks + 8, tol, 0.0)
    print("QSTOP order,%s residual first: rel_tol %.3e reference k %d, device %d (eta = 0: %d), last_rule %d" % (SN[scalar], tol, kr, st["last_iters"],
                                                                                                             st0["last_iters"], ss["last_rule"]))
    ck("residual_first", 0 if (ss["last_rule"], ss["by_residual"], ss["by_model"], ss["at_cap"], st["last_converged"]) == (1, 1, 0, 0, 1) else 1, 0)
    ck("residual_first_iters(eta = 0: %d, reference %d)" % (st0["last_iters"], kr), abs(st["last_iters"] - st0["last_iters"]), 0)
    if scalar == 0:  # (fp64: the very iterate.  In fp32 k_pcg_update_q's x and r come out with other contractions than k_pcg_update's: DESIGN.md section 20)
        ck("residual_first_residual_bits", 0 if st["last_rel_residual"] == st0["last_rel_residual"] else 1, 0)
    # the cap first
    cap = ks - 2
    yard, scale = yardstick(case, scalar, cap, eta, [cap])
    assert (yard["iters"], yard["rule"]) == (cap, 0)
    st, ss = solve(ba, s, lam, cap, 1e-30, eta)
    ck("cap_first", 0 if (st["last_iters"], ss["last_rule"], ss["at_cap"], ss["by_model"], ss["by_residual"], st["last_converged"]) == (cap, 0, 1, 0, 0, 0) else 1, 0)
    fs, fz = floors(ref, cap, scalar)
    ys, yz = scale * rel(yard["s"][cap], ref["s"][cap]), scale * rel(yard["zeta"][cap], ref["zeta"][cap])
    ck("cap_last_model(yardstick %.1e)" % ys, rel(ss["last_model"], ref["s"][cap]), max(10 * ys, fs))
    ck("cap_last_zeta(reference %.4e, yardstick %.1e)" % (ref["zeta"][cap], yz), rel(ss["last_zeta"], ref["zeta"][cap]), max(10 * yz, fz))
    s.set_pcg_model_tol(0.0)
    ck.done()


# ---- 4 -----------------------------------------------------------------------------------------------------------------------------------------
def _observe(ba, s, lam_rel=1e-9, trials=2):
    out = [np.array(s.linearize())]
    lam = lam_rel * out[0][1]
    for _ in range(trials):
        out.append(np.array(s.try_step(lam)))
        out += [s.get(w).copy() for w in (ba.GET_DX, ba.GET_CAMS_TEST, ba.GET_POINTS_TEST, ba.GET_RHS)]
        st = s.pcg_stats()
        out.append(np.array([st["last_iters"], st["last_converged"], st["last_rel_residual"]]))
        lam *= 1000
    return out


def _same(x, y, what):
    assert len(x) == len(y)
    for k, (a, b) in enumerate(zip(x, y)):
        assert np.array_equal(a, b), (what, k)


@pytest.mark.parametrize("scalar", [0, 1], ids=["f64", "f32"])
def test_bits(ba, gpu_ok, prob21, scalar):
    pg, N = prob21, prob21.N
    eta = 0.1

    def solver(on=True):
        s = ba.Solver(pg, ba.ITERSCHUR, scalar)
        if on:
            s.set_pcg_model_tol(eta)
        return s

    # a solve with the rule on is the same bits run twice, on this solver and on a second one
    a = solver()
    one = _observe(ba, a)
    assert a.pcg_stop_stats()["last_rule"] == 2  # (the rule did end these solves)
    _same(one, _observe(ba, a), "repeated")
    _same(one, _observe(ba, solver()), "second solver")
    # ... in try_step as in the first row of ba_minimize (the captured graph), and over eight rows of two runs
    gsol, h = solver(), solver()
    rows = gsol.minimize(max_trials=1)["trace"]
    e, dmax = h.linearize()
    assert rows[0, 2] == e
    h.try_step(float(DT[scalar](1e-12 * dmax)))
    for what in (ba.GET_DX, ba.GET_CAMS_TEST, ba.GET_POINTS_TEST, ba.GET_RHS):
        assert np.array_equal(bits(gsol.get(what)), bits(h.get(what))), ("graph", what)
    sg, sh = gsol.pcg_stats(), h.pcg_stats()
    assert (sg["last_iters"], sg["last_rel_residual"]) == (sh["last_iters"], sh["last_rel_residual"])
    qg, qh = gsol.pcg_stop_stats(), h.pcg_stop_stats()
    assert (qg["last_rule"], qg["last_zeta"], qg["last_model"]) == (qh["last_rule"], qh["last_zeta"], qh["last_model"]) and qg["last_rule"] == 2
    t1, t2 = solver(), solver()
    r1, r2 = t1.minimize(max_trials=8), t2.minimize(max_trials=8)
    assert len(r1["trace"]) == 8 and np.array_equal(bits(r1["trace"][:, :5]), bits(r2["trace"][:, :5]))
    assert np.array_equal(bits(t1.get(ba.GET_DX)), bits(t2.get(ba.GET_DX)))
    q1 = t1.pcg_stop_stats()
    assert q1 == t2.pcg_stop_stats() and q1["by_model"] + q1["by_residual"] + q1["at_cap"] == t1.pcg_stats()["solves"] == 8
    # eta > 0 and then eta = 0 -- trials run, a graph captured in between -- is the solver that never had the rule
    never = solver(on=False)
    nbytes = never.device_bytes()
    plain = _observe(ba, never)
    assert not np.array_equal(plain[2], one[2])  # (the rule does change the step)
    stats = never.pcg_stats()
    trace = never.minimize(max_trials=8)["trace"]
    b = solver(on=False)
    start_c, start_p = b.get(ba.GET_CAMS), b.get(ba.GET_POINTS)
    b.set_pcg_model_tol(eta)
    assert b.device_bytes() == nbytes + 3 * ((N + 255) // 256) * 8  # (the documented buffer)
    b.minimize(max_trials=2)
    b.set_state(start_c, start_p)
    b.set_pcg_model_tol(0.0)
    b.pcg_stats(reset=True)
    _same(plain, _observe(ba, b), "rule switched off")
    assert b.pcg_stats() == stats
    assert np.array_equal(bits(b.minimize(max_trials=8)["trace"][:, :5]), bits(trace[:, :5]))
    assert b.device_bytes() == nbytes + 3 * ((N + 255) // 256) * 8


# ---- 5 -----------------------------------------------------------------------------------------------------------------------------------------
def _refused(ba, fn, *args):
    with pytest.raises(ba.BAError) as ei:
        fn(*args)
    assert ei.value.code == ba.ERR_ARG, ei.value.code


def test_refusals_leave_the_solver_unchanged(ba, gpu_ok, prob21):
    c = ba.Solver(prob21, ba.CHOLESKY, ba.F64)
    _refused(ba, c.set_pcg_model_tol, 0.1)
    _refused(ba, c.set_pcg_model_tol, 0.0)
    _refused(ba, c.pcg_stop_stats)
    for scalar in (0, 1):
        s = ba.Solver(prob21, ba.ITERSCHUR, scalar)
        nbytes = s.device_bytes()
        before = _observe(ba, s)
        for eta in (-0.1, -0.0 - 1e-300, 1.0, 1.5, float("nan"), float("inf"), float("-inf")):
            _refused(ba, s.set_pcg_model_tol, eta)
        assert s.device_bytes() == nbytes
        _same(before, _observe(ba, s), "refused")
        s.set_pcg_model_tol(0.1)
        on = _observe(ba, s)
        for eta in (1.0, float("nan")):
            _refused(ba, s.set_pcg_model_tol, eta)
        _same(on, _observe(ba, s), "refused with the rule on")
    # a pending step survives the setter
    s = ba.Solver(prob21, ba.ITERSCHUR, ba.F64)
    e, dmax = s.linearize()
    s.try_step(1e-4 * dmax)
    want = s.get(ba.GET_CAMS_TEST)
    s.set_pcg_model_tol(0.1)
    s.accept()
    assert np.array_equal(bits(s.get(ba.GET_CAMS)), bits(want))


def test_covariance_pcg_does_not_use_the_rule(ba, gpu_ok, prob21):
    out = []
    for eta in (0.0, 0.5):
        s = ba.Solver(prob21, ba.ITERSCHUR, ba.F64)
        s.set_pcg_model_tol(eta)
        e, dmax = s.linearize()
        s.try_step(1e-6 * dmax)
        cc, pc, st = s.covariance_pcg(1e-6 * dmax, cams=[0, 5, 20], points=[0, 17])
        out.append((cc, pc, st["total_iters"], st["max_iters"]))
    assert np.array_equal(bits(out[0][0]), bits(out[1][0])) and np.array_equal(bits(out[0][1]), bits(out[1][1])) and out[0][2:] == out[1][2:]


# ---- 6 -----------------------------------------------------------------------------------------------------------------------------------------
def test_end_to_end_problem21(ba, gpu_ok, prob21):
    """problem-21, fp64, to the reference's stop: the defaults, and eta = 0.1 with rel_tol and max_iter left at their defaults.  Final
    energy <= 1.02 x CHOLESKY's (DESIGN.md section 9's bound for this kind), strictly fewer PCG iterations in total."""
    c = ba.Solver(prob21, ba.CHOLESKY, ba.F64).minimize()
    runs = {}
    for eta in (0.0, ETA_E2E):
        s = ba.Solver(prob21, ba.ITERSCHUR, ba.F64)
        s.set_pcg_model_tol(eta)
        r = s.minimize()
        st, ss = s.pcg_stats(), s.pcg_stop_stats()
        runs[eta] = (r, st, ss)
        print("QSTOP e2e eta %.3g: status %s trials %d iterations %d energy %.9g (CHOLESKY %.9g, %d trials) by_residual %d by_model %d at_cap %d"
              % (eta, ba.status_string(r["status"]), r["trials"], st["total_iters"], r["energy"], c["energy"], c["trials"], ss["by_residual"],
                 ss["by_model"], ss["at_cap"]))
    r, st, ss = runs[ETA_E2E]
    assert r["energy"] <= 1.02 * c["energy"], (r["energy"], c["energy"])
    assert runs[0.0][0]["energy"] <= 1.02 * c["energy"]
    assert st["total_iters"] < runs[0.0][1]["total_iters"], (st["total_iters"], runs[0.0][1]["total_iters"])
    assert ss["by_model"] > 0 and ss["by_model"] + ss["by_residual"] + ss["at_cap"] == st["solves"]
