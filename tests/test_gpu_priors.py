"""GPU: Gaussian priors on points, camera centres and intrinsics (ba_solver_set_*_priors) through the C ABI, against
tests/prior_checks.py on top of tests/loss_checks.py (both long double; pinned on the CPU by test_prior_checks.py / test_loss_checks.py).

The prior set is prior_checks.standard_priors: point priors on about 1 % of the points (seeded) plus every point with fewer than 3
observations, centre priors on all cameras, intrinsics priors on f and k1 of every second camera (w = 0 for k2).  Their information is
kappa x the median own diagonal of the block they join, kappa = 1 (points), 10 (centres), 0.1 (f), 1 (k1): inside the band
[1e-2, 1e2]; the sigmas that result are printed per problem (`PRIOR sigmas ...`).

Bounds.  Linearisation: test_gpu_loss.py's TOL for the same quantities (energy, prior energies: TOL energy; gradient: TOL g; max diag
J'J, a sum of products of J's entries like g: TOL g).  Trial: test_gpu_stages.py's BOUND for S, rhs (max(10 x the oracle's error on
the same augmented J, floor), as test_assembly_and_backsub), eta, backsub, e_test, rho_scale.  Every figure is printed as
`PRIOR <case> <metric> <value> <bound>` before it is asserted."""
import numpy as np
import pytest

import cov_checks as CC
import loss_checks as LC
import prior_checks as PC
import stage_checks as SC
from test_gpu_loss import TOL, _weights
from test_gpu_parity import _ragged_problem, relmax
from test_gpu_stages import BOUND, EPS, sorted_oracle_problem

pytestmark = pytest.mark.gpu
F64 = np.float64
LD = np.longdouble


class Checker:
    def __init__(self, case):
        self.case, self.rows = case, []

    def __call__(self, metric, value, bound):
        self.rows.append((metric, float(value), float(bound)))
        print("PRIOR %s %s %.3e %.1e" % (self.case, metric, value, bound))

    def done(self):
        bad = [r for r in self.rows if not (r[1] <= r[2])]
        assert not bad, (self.case, bad)


def _problem(ba, name, prob21, prob39):
    return {"p21": prob21, "p39": prob39}.get(name) or _ragged_problem(ba)


_PRIORS = {}


def _priors(ba, O, pg, name):
    """standard_priors of a problem, sized from the fp64 CHOLESKY linearisation at the start state (plain least squares is not
    needed: the default loss's J'J sets the scale), once per problem."""
    if name not in _PRIORS:
        po = sorted_oracle_problem(O, pg)
        s = ba.Solver(pg, ba.CHOLESKY, ba.F64)
        s.linearize()
        pr, sig = PC.standard_priors(pg.N, pg.M, pg.K, po.pt_idx, s.get(ba.GET_CAMS), s.get(ba.GET_POINTS), s.get(ba.GET_JC).reshape(-1, 2, 9),
                                     s.get(ba.GET_JP).reshape(-1, 2, 3), po.cam_idx)
        print("PRIOR sigmas %s point %.3e centre %.3e f %.3e k1 %.3e (%d point, %d centre, %d intrinsics priors)"
              % (name, sig["point"], sig["centre"], sig["f"], sig["k1"], len(pr.pt_ids), len(pr.c_ids), len(pr.i_ids)))
        _PRIORS[name] = pr
    return _PRIORS[name]


def _solver_priors(pr, scalar):
    return pr.rounded(np.float32) if scalar == 1 else pr


def _yardstick(O, po, pr, cams, pts, kind, scale, w, cm=None, pf=None):
    """Energy, prior energies, g and max diag J'J of observations + priors at the state, long double."""
    Y = LC.model(O, po, cams, pts, kind, scale, w)
    Jc, Jp = Y["Jc"], Y["Jp"]
    if cm is not None or pf is not None:
        fc, fp = CC.free_sets(po, cm, pf)
        Jc = Jc * fc.reshape(po.N, 9)[po.cam_idx][:, None, :]
        Jp = Jp * fp[po.pt_idx][:, None, None]
    U, V, g, e = PC.normal_blocks(po.N, po.M, po.cam_idx, po.pt_idx, Jc, Jp, Y["e"])
    d = PC.direct(pr, po.N, po.M, cams, pts, cm, pf)
    U, V, g = U + d["U"], V + d["V"], g + d["g"]
    dmax = max(np.einsum("nii->ni", U).max(), np.einsum("nii->ni", V).max())
    return dict(energy=e + d["energy"], energies=d["energies"], g=g, dmax=dmax, Jc=Jc, Jp=Jp, e=Y["e"])


MODELS = {"default": (LC.REFERENCE, 0.5, False), "huber_w": (LC.HUBER, 1.0, True)}


def _make(ba, pg, skind, scalar, model, pr):
    kind, scale, weighted = MODELS[model]
    w = _weights(pg.K) if weighted else None
    s = ba.Solver(pg, skind, scalar)
    if model != "default":
        s.set_loss(kind, scale)
        s.set_obs_weights(w)
    if pr is not None:
        _solver_priors(pr, scalar).apply(s)
    order = np.argsort(pg.arrays()["pt_idx"], kind="stable")
    wy = None if w is None else (w.astype(np.float32).astype(F64) if scalar == 1 else w)[order]
    return s, kind, scale, wy


# ---- 1. linearisation --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scalar", [0, 1], ids=["f64", "f32"])
@pytest.mark.parametrize("model", ["default", "huber_w"])
@pytest.mark.parametrize("skind", [2, 5], ids=["cholesky", "iterschur"])
@pytest.mark.parametrize("prob", ["p21", "p39", "ragged"])
def test_linearisation_matches_the_yardstick(ba, O, gpu_ok, prob21, prob39, prob, skind, model, scalar):
    pg = _problem(ba, prob, prob21, prob39)
    po = sorted_oracle_problem(O, pg)
    pr = _priors(ba, O, pg, prob)
    s, kind, scale, wy = _make(ba, pg, skind, scalar, model, pr)
    energy, dmax = s.linearize()
    Y = _yardstick(O, po, _solver_priors(pr, scalar), s.get(ba.GET_CAMS), s.get(ba.GET_POINTS), kind, scale, wy)
    tol = TOL[scalar]
    ck = Checker("lin[%s,%s,%s,%s]" % (prob, ba.KIND_NAMES[skind], model, "f64" if scalar == 0 else "f32"))
    ck("energy", abs(energy - float(Y["energy"])) / float(Y["energy"]), tol["energy"])
    pe = s.prior_energy()
    for q, name in enumerate(("point", "centre", "intrinsics")):
        assert float(Y["energies"][q]) > 0
        ck("prior_energy_%s" % name, abs(pe[q] - float(Y["energies"][q])) / float(Y["energies"][q]), tol["energy"])
    ck("grad", relmax(s.get(ba.GET_GRAD), Y["g"].astype(F64)), tol["g"])
    ck("diag_max", abs(dmax - float(Y["dmax"])) / float(Y["dmax"]), tol["g"])
    # the observation rows stay the observation rows
    ck("residuals", relmax(s.get(ba.GET_RESIDUALS), Y["e"].astype(F64).ravel()), tol["e"])
    ck.done()


# ---- 2. trial ------------------------------------------------------------------------------------------------------------------------------
def _augmented(O, po, pr, s, ba, cm=None, pf=None):
    """The augmented problem at the GPU's own J, residuals and state: (problem, Jc, Jp, f) in doubles."""
    K = po.K
    cams, pts = s.get(ba.GET_CAMS), s.get(ba.GET_POINTS)
    ca, pa, JC, JP, E = PC.augment(pr, po.cam_idx, po.pt_idx, s.get(ba.GET_JC).reshape(K, 2, 9), s.get(ba.GET_JP).reshape(K, 2, 3),
                                   s.get(ba.GET_RESIDUALS).reshape(K, 2), cams, pts, cm, pf)
    pa_ = O.Problem(po.N, po.M, len(ca), ca, pa, np.zeros(2 * len(ca)), po.cams9, po.pts)
    return pa_, JC.astype(F64), JP.astype(F64), E.astype(F64).ravel()


@pytest.mark.parametrize("prob,scalar", [("p21", 0), ("ragged", 0), ("p39", 0), ("p21", 1)], ids=["p21-f64", "ragged-f64", "p39-f64", "p21-f32"])
def test_trial_matches_the_yardstick(ba, O, gpu_ok, prob21, prob39, prob, scalar):
    """CHOLESKY with keep_intermediates, Huber + weights + priors, lambda = 1e-6 and 1e-2 x max diag J'J."""
    pg = _problem(ba, prob, prob21, prob39)
    po = sorted_oracle_problem(O, pg)
    pr = _solver_priors(_priors(ba, O, pg, prob), scalar)
    s, kind, scale, wy = _make(ba, pg, ba.CHOLESKY, scalar, "huber_w", _priors(ba, O, pg, prob))
    s.keep_intermediates(True)
    e0, dmax = s.linearize()
    pa, Jc, Jp, f = _augmented(O, po, pr, s, ba)
    g = s.get(ba.GET_GRAD)
    M = po.M
    ck = Checker("trial[%s,%s]" % (prob, "f64" if scalar == 0 else "f32"))
    ck("grad", SC.grad_errors(pa, Jc, Jp, f, g), BOUND[("grad", scalar)])
    dt = F64 if scalar == 0 else np.float32
    for lam in (1e-6 * dmax, 1e-2 * dmax):
        et, rs, dn = s.try_step(lam)
        S, rhs, dx = s.get(ba.GET_S), s.get(ba.GET_RHS), s.get(ba.GET_DX)
        R = O.referee_reduced_from_jacobian(ba.CHOLESKY, pa, Jc, Jp, f, lam)
        st = O.step(ba.CHOLESKY, pa, Jc.astype(dt), Jp.astype(dt), f.astype(dt), lam)
        got = SC.assembly_errors(pa, Jc, f, lam, S, rhs, R["S"], R["rhs"], Jp)
        orc = SC.assembly_errors(pa, Jc, f, lam, st["S"].astype(F64), st["rhs"].astype(F64), R["S"], R["rhs"], Jp)
        if not all(np.isfinite(v) for v in orc.values()):  # (the fp32 oracle's 3 x 3 LDL^T breaks down: fp64's error x eps32 / eps64, as test_gpu_stages.py)
            s64 = O.step(ba.CHOLESKY, pa, Jc, Jp, f, lam)
            o64 = SC.assembly_errors(pa, Jc, f, lam, s64["S"], s64["rhs"], R["S"], R["rhs"], Jp)
            orc = {k: v * EPS[1] / EPS[0] for k, v in o64.items()}
        for k in ("S", "rhs"):
            ck("%s@%.0e(oracle %.1e)" % (k, lam, orc[k]), got[k], max(10 * orc[k], BOUND[(k, scalar)]))
        ck("eta@%.0e" % lam, SC.eta(S, dx[3 * M:], rhs), BOUND[("eta", scalar)])
        ck("backsub@%.0e" % lam, SC.backsub_errors(pa, Jc, Jp, dx, g, lam), BOUND[("backsub", scalar)])
        ct, pt = s.get(ba.GET_CAMS_TEST), s.get(ba.GET_POINTS_TEST)
        e_ref = float(LC.energy(O, po, ct, pt, kind, scale, wy) + PC.energies(pr, ct, pt).sum())
        ck("e_test@%.0e" % lam, abs(et - e_ref) / e_ref, BOUND[("e_test", scalar)])
        dxl, gl = dx.astype(LD), g.astype(LD)
        rsy = (dxl * (LD(lam) * dxl + gl)).sum()
        ck("rho_scale@%.0e" % lam, float(abs(LD(rs) - rsy) / (np.abs(dxl) * (LD(lam) * np.abs(dxl) + np.abs(gl))).sum()), BOUND[("rho_scale", scalar)])
    ck.done()


# ---- 3. ITERSCHUR --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prob", ["p21", "p39"])
def test_iterschur_solves_the_system_with_priors(ba, O, gpu_ok, prob21, prob39, prob):
    """Same state, same lambda = 1e-4 max diag J'J (test_gpu_iterative_schur.py's setting), set_pcg(1000, 1e-10).  The device's own
    true residual, ba_solver_pcg_stats.last_rel_residual = |rhs - S dx_c| / |rhs|, is <= rel_tol, which shows that the operator and the
    rhs contain the priors -- CHOLESKY's S and rhs do (test_trial_matches_the_yardstick) and the two steps are compared:
    |dx_it - dx_ch| / |dx_ch| <= cond(S) x rel_tol with cond(S) <= |S| / lambda <= 9 max diag / (1e-4 max diag) = 9e4
    (0 <= S - lambda I <= Jc'Jc, block diagonal with 9 x 9 blocks of trace <= 9 max diag), i.e. 9e-6.  Iterations <= those without priors + 2."""
    pg = _problem(ba, prob, prob21, prob39)
    pr = _priors(ba, O, pg, prob)
    ck = Checker("iterschur[%s]" % prob)
    out = {}
    for tag, prs in (("plain", None), ("priors", pr)):
        for skind in (ba.CHOLESKY, ba.ITERSCHUR):
            s, _, _, _ = _make(ba, pg, skind, ba.F64, "huber_w", prs)
            if skind == ba.ITERSCHUR:
                s.set_pcg(1000, 1e-10)
            e, dmax = s.linearize()
            lam = 1e-4 * dmax
            tr = s.try_step(lam)
            out[(tag, skind)] = (e, dmax, np.array(tr), s.get(ba.GET_DX).copy(), s.pcg_stats() if skind == ba.ITERSCHUR else None)
    for tag in ("plain", "priors"):
        ch, it = out[(tag, ba.CHOLESKY)], out[(tag, ba.ITERSCHUR)]
        assert ch[0] == it[0] and ch[1] == it[1]  # (the same linearisation kernels)
        st = it[4]
        ck("%s_converged" % tag, 0 if st["last_converged"] == 1 else 1, 0)
        ck("%s_true_rel_residual" % tag, st["last_rel_residual"], 1e-10)
        ck("%s_dx_vs_cholesky" % tag, np.linalg.norm(it[3] - ch[3]) / np.linalg.norm(ch[3]), 9e-6)
        print("PRIOR iterschur[%s] %s iterations %d" % (prob, tag, st["last_iters"]))
    ck("iterations_with_priors<=plain+2", out[("priors", ba.ITERSCHUR)][4]["last_iters"] - out[("plain", ba.ITERSCHUR)][4]["last_iters"], 2)
    ck.done()


# ---- 4. bit identity ---------------------------------------------------------------------------------------------------------------------
def _observe(ba, s, keep):
    out = [np.array(s.linearize())]
    out.append(s.get(ba.GET_GRAD).copy())
    out.append(np.array(s.try_step(1e-12 * out[0][1])))
    out += [s.get(w).copy() for w in (ba.GET_DX, ba.GET_CAMS_TEST, ba.GET_POINTS_TEST)]
    if keep:
        out += [s.get(ba.GET_S).copy(), s.get(ba.GET_RHS).copy()]
    r = s.minimize(max_trials=20)
    out += [r["trace"][:, :5].copy(), np.array([r["energy"], r["lam"]]), s.get(ba.GET_CAMS).copy(), s.get(ba.GET_POINTS).copy()]
    return out


def _fresh_solver(ba, prob21, skind, scalar):
    s = ba.Solver(prob21, skind, scalar)
    s.keep_intermediates(skind == ba.CHOLESKY)
    return s


@pytest.mark.parametrize("scalar", [0, 1], ids=["f64", "f32"])
@pytest.mark.parametrize("skind", [2, 5], ids=["cholesky", "iterschur"])
def test_removed_priors_are_the_solver_without(ba, O, gpu_ok, prob21, skind, scalar):
    """Setting priors, running with them (the graphs of the prior path are captured) and removing them, against the solver that never
    had any: energy, max diag, gradient, a trial (S and rhs for CHOLESKY), 20 rows of ba_minimize and the state it leaves, bit for bit."""
    pr = _priors(ba, O, prob21, "p21")
    keep = skind == ba.CHOLESKY
    fresh = _observe(ba, _fresh_solver(ba, prob21, skind, scalar), keep)
    cams0 = ba.Solver(prob21, skind, scalar).get(ba.GET_CAMS)
    s = _fresh_solver(ba, prob21, skind, scalar)
    _solver_priors(pr, scalar).apply(s)
    e1, _ = s.linearize()
    assert e1 != fresh[0][0]
    s.minimize(max_trials=3)
    s.set_state(cams0, prob21.arrays()["pts"])
    PC.Priors().apply(s)
    back = _observe(ba, s, keep)
    for k, (x, y) in enumerate(zip(fresh, back)):
        assert np.array_equal(x, y), ("removed", k)


@pytest.mark.parametrize("scalar", [0, 1], ids=["f64", "f32"])
@pytest.mark.parametrize("skind", [2, 5], ids=["cholesky", "iterschur"])
def test_zero_information_priors_are_the_solver_without(ba, O, gpu_ok, prob21, skind, scalar):
    """Priors whose information is all zero (L = 0, w = 0) go through the prior path and give the bits of the solver without priors.
    (The linearisation with priors is the kernel sequence of the solver without, fused kernel included, with the prior kernel behind
    it; the trial's own k_elim_chol replaces the fused pass's records: DESIGN.md section 13.)"""
    pr = _priors(ba, O, prob21, "p21")
    keep = skind == ba.CHOLESKY
    fresh = _observe(ba, _fresh_solver(ba, prob21, skind, scalar), keep)
    z = PC.Priors(pr.pt_ids, pr.pt_x0, 0 * pr.pt_L, pr.c_ids, pr.c_c0, 0 * pr.c_L, pr.i_ids, pr.i_x0, 0 * pr.i_w)
    s = _fresh_solver(ba, prob21, skind, scalar)
    z.apply(s)
    zero = _observe(ba, s, keep)
    for k, (x, y) in enumerate(zip(fresh, zero)):
        assert np.array_equal(x, y), ("zero information", k)


@pytest.mark.parametrize("scalar", [0, 1], ids=["f64", "f32"])
@pytest.mark.parametrize("skind", [2, 5], ids=["cholesky", "iterschur"])
def test_eager_trial_is_the_graph_trial(ba, O, gpu_ok, prob21, skind, scalar):
    """linearize / try_step(lambda0) / accept / linearize on one solver, ba_minimize(max_trials = 1) on another, bit for bit: f of
    row 1, the step and the trial point, rho of row 1 -- (f - e_test) / rho_scale in the solver's scalar type, e_test being the sum the
    graph forms at the head of k_lm_control and try_step in k_reduce_scalars, k_prior<T, false>'s partials included --, and the energy
    the run returns, which is that of the graph's conditional linearisation at xTest (k_prior<T, true> under `go`, its own reduce
    launch) against the eager linearisation behind accept()."""
    sc = np.float32 if scalar == 1 else np.float64
    pr = _solver_priors(_priors(ba, O, prob21, "p21"), scalar)
    s1 = ba.Solver(prob21, skind, scalar)
    pr.apply(s1)
    e, dmax = s1.linearize()
    lam0 = float(sc(1e-12 * dmax))
    et, rs, dn = s1.try_step(lam0)
    dx1, ct1, pt1 = s1.get(ba.GET_DX), s1.get(ba.GET_CAMS_TEST), s1.get(ba.GET_POINTS_TEST)
    s2 = ba.Solver(prob21, skind, scalar)
    pr.apply(s2)
    r = s2.minimize(max_trials=1)
    row = r["trace"][0]
    assert row[1] == 1 and et < e  # (accepted on both sides)
    assert row[2] == e
    assert np.array_equal(ct1, s2.get(ba.GET_CAMS_TEST)) and np.array_equal(pt1, s2.get(ba.GET_POINTS_TEST))
    assert np.array_equal(dx1, s2.get(ba.GET_DX))
    assert row[3] == float((sc(e) - sc(et)) / sc(rs)), (row[3], e, et, rs)
    s1.accept()
    e1, _ = s1.linearize(False)
    assert r["energy"] == e1, (r["energy"], e1, et)
    assert np.array_equal(s1.get(ba.GET_CAMS), s2.get(ba.GET_CAMS)) and np.array_equal(s1.get(ba.GET_POINTS), s2.get(ba.GET_POINTS))
    assert np.array_equal(s1.get(ba.GET_GRAD), s2.get(ba.GET_GRAD)) or scalar == 1  # (fp32: the fused and the eager J differ in bits)


@pytest.mark.parametrize("skind", [2, 5], ids=["cholesky", "iterschur"])
def test_graph_replay_is_the_host_loop_with_priors(ba, O, gpu_ok, prob21, skind):
    """test_gpu_loss.py::test_graph_replay_is_the_host_loop with priors (and Huber + weights), fp64: 12 rows of ba_minimize -- one
    captured graph per trial, step control on the device -- against a host loop of linearize / try_step / accept that takes only the
    lambda column from the table: iteration, accepted, f (bits), rho (1e-12, that test's), the returned energy and state (bits)."""
    pr = _priors(ba, O, prob21, "p21")
    ntr = 12
    g, _, _, _ = _make(ba, prob21, skind, ba.F64, "huber_w", pr)
    r = g.minimize(max_trials=ntr)
    rows = r["trace"]
    assert len(rows) == ntr and (rows[:, 1] == 1).sum() >= 3 and (rows[:, 1] == 0).sum() >= 0
    h, _, _, _ = _make(ba, prob21, skind, ba.F64, "huber_w", pr)
    e, dmax = h.linearize()
    lam, got, it = 1e-12 * dmax, [], 1
    for t in range(ntr):
        et, rs, dn = h.try_step(lam)
        if et < e:
            got.append((it, 1, e, (e - et) / rs))
            h.accept()
            e, _ = h.linearize(False)
            it += 1
        else:
            got.append((it, 0, e, 0.0))
        lam = rows[t, 4]
    got = np.array(got)
    assert np.array_equal(rows[:, 0], got[:, 0]) and np.array_equal(rows[:, 1], got[:, 1])
    assert np.array_equal(rows[:, 2], got[:, 2]), (rows[:, 2], got[:, 2])
    assert np.allclose(rows[:, 3], got[:, 3], rtol=1e-12, atol=0)
    if rows[-1, 1] == 1:
        assert r["energy"] == e
    assert np.array_equal(g.get(ba.GET_CAMS), h.get(ba.GET_CAMS)) and np.array_equal(g.get(ba.GET_POINTS), h.get(ba.GET_POINTS))


# ---- 4b. the Python binding's sigma forms ------------------------------------------------------------------------------------------------
def test_binding_sigma_forms(ba, O, gpu_ok, prob21):
    """Solver.set_point_priors / set_centre_priors with sigma (scalar and (n, 3)) and Solver.set_intrinsics_priors(ids, x0, sigma) with
    sigma = inf for "no row": the same energies, bit for bit, as the lists handed over as L = diag(1 / sigma) and w = 1 / sigma."""
    rng = np.random.default_rng(21)
    pid, cid, iid = np.arange(0, 300, 3, dtype=np.int32), np.arange(prob21.N, dtype=np.int32), np.arange(1, prob21.N, 2, dtype=np.int32)
    s0 = ba.Solver(prob21, ba.CHOLESKY, ba.F64)
    cams, pts = s0.get(ba.GET_CAMS).reshape(-1, 15), s0.get(ba.GET_POINTS).reshape(-1, 3)
    px0, cc0, ix0 = pts[pid] + 0.01, np.asarray(PC.centres(cams), F64) + 1e-4, cams[iid, 12:15] + [1.0, 1e-3, 1e-3]
    sp, sgc = 0.02, rng.uniform(1e-4, 1e-3, (len(cid), 3))
    si = np.tile([2.0, 1e-3, np.inf], (len(iid), 1))
    a = ba.Solver(prob21, ba.CHOLESKY, ba.F64)
    a.set_point_priors(pid, px0, sigma=sp)
    a.set_centre_priors(cid, cc0, sigma=sgc)
    a.set_intrinsics_priors(iid, ix0, si)
    ea, _ = a.linearize()
    Lc = np.zeros((len(cid), 3, 3))
    for q in range(3):
        Lc[:, q, q] = 1.0 / sgc[:, q]
    ref = PC.Priors(pid, px0, np.tile(np.eye(3) / sp, (len(pid), 1, 1)), cid, cc0, Lc, iid, ix0, 1.0 / si)
    assert not ref.i_w[:, 2].any()
    b = ba.Solver(prob21, ba.CHOLESKY, ba.F64)
    ref.apply(b)
    eb, _ = b.linearize()
    assert ea == eb and np.array_equal(a.prior_energy(), b.prior_energy()) and (a.prior_energy() > 0).all()
    y = PC.energies(ref, cams, pts)
    assert np.allclose(a.prior_energy(), y.astype(F64), rtol=TOL[0]["energy"], atol=0)
    with pytest.raises(ValueError):
        a.set_point_priors(pid, px0)  # neither sqrt_info nor sigma
    a.set_intrinsics_priors([], np.zeros((0, 3)), 1.0)
    a.linearize()
    assert a.prior_energy()[2] == 0 and a.prior_energy()[0] > 0


# ---- 4c. points with a prior and no observation (k_prior_lonely) ---------------------------------------------------------------------------
def _lonely_problem(ba):
    pg = _ragged_problem(ba)
    a = pg.arrays()
    keep = ~np.isin(a["pt_idx"], [5, 40, 41, 120, 199, 259])
    return ba.Problem.from_arrays(pg.N, pg.M, int(keep.sum()), a["cam_idx"][keep], a["pt_idx"][keep], a["meas"].reshape(-1, 2)[keep].ravel(),
                                  a["cams9"], a["pts"])


@pytest.mark.parametrize("masked", [False, True], ids=["free", "masked"])
@pytest.mark.parametrize("skind", [2, 5], ids=["cholesky", "iterschur"])
def test_unobserved_points_with_priors(ba, O, gpu_ok, skind, masked):
    """The ragged problem without the observations of six more points (it has one point nobody observes already); standard_priors
    gives each of them a prior (fewer than 3 observations).  A trial: their
    step solves (L'L + lambda I) dx = -L'e (stage_checks.backsub_errors on the augmented problem, its bound), a fixed one does not move
    (masked: every second of them is fixed, and the gauge); 6 and then 30 trials of ba_minimize (graph path): the returned energy is
    the yardstick's at the returned state (TOL energy while the run is `Running`), it never rises, and the free unobserved points have moved while the fixed ones
    keep their bits."""
    pg = _lonely_problem(ba)
    po = sorted_oracle_problem(O, pg)
    pr = _priors(ba, O, pg, "lonely")
    lone = np.flatnonzero(np.bincount(po.pt_idx, minlength=pg.M) == 0)
    assert len(lone) >= 6 and np.isin(lone, pr.pt_ids).all()
    cm = pf = None
    if masked:
        cm = pg.gauge_mask(0)
        pf = np.zeros(pg.M, np.uint8)
        pf[lone[::2]] = 1
    s = ba.Solver(pg, skind, ba.F64)
    pr.apply(s)
    if masked:
        s.set_constant(cm, pf)
    if skind == ba.ITERSCHUR:
        s.set_pcg(1000, 1e-10)
    e0, dmax = s.linearize()
    pts0 = s.get(ba.GET_POINTS).reshape(-1, 3).copy()
    ck = Checker("lonely[%s,%s]" % (ba.KIND_NAMES[skind], "masked" if masked else "free"))
    Y = _yardstick(O, po, pr, s.get(ba.GET_CAMS), s.get(ba.GET_POINTS), LC.REFERENCE, 0.5, None, cm, pf)
    ck("energy", abs(e0 - float(Y["energy"])) / float(Y["energy"]), TOL[0]["energy"])
    pa, Jc, Jp, f = _augmented(O, po, pr, s, ba, cm, pf)
    g = s.get(ba.GET_GRAD)
    lam = 1e-6 * dmax
    et, rs, dn = s.try_step(lam)
    dx = s.get(ba.GET_DX)
    ck("backsub", SC.backsub_errors(pa, Jc, Jp, dx, g, lam), BOUND[("backsub", 0)])
    dxl = dx[:3 * pg.M].reshape(-1, 3)[lone]
    free_lone = np.ones(len(lone), bool) if pf is None else pf[lone] == 0
    assert dxl[free_lone].all(axis=1).any() and np.abs(dxl[free_lone]).max() > 0 and not dxl[~free_lone].any()
    ct, pt = s.get(ba.GET_CAMS_TEST), s.get(ba.GET_POINTS_TEST)
    assert np.array_equal(pt.reshape(-1, 3)[lone][~free_lone], pts0[lone][~free_lone])
    e_ref = float(LC.energy(O, po, ct, pt, LC.REFERENCE, 0.5, None) + PC.energies(pr, ct, pt).sum())
    ck("e_test", abs(et - e_ref) / e_ref, BOUND[("e_test", 0)])
    dxq, gq = dx.astype(LD), g.astype(LD)
    ck("rho_scale", float(abs(LD(rs) - (dxq * (LD(lam) * dxq + gq)).sum()) / (np.abs(dxq) * (LD(lam) * np.abs(dxq) + np.abs(gq))).sum()),
       BOUND[("rho_scale", 0)])
    if skind == ba.ITERSCHUR:
        s.set_pcg(100, 1e-6)
    s.linearize()
    rows = []
    for ntr in (6, 30):  # (6 trials end `Running`: x = xTest has happened and the returned energy is the returned state's)
        r = s.minimize(max_trials=ntr)
        rows.append(r["trace"])
        c1, p1 = s.get(ba.GET_CAMS), s.get(ba.GET_POINTS)
        Ey = float(LC.energy(O, po, c1, p1, LC.REFERENCE, 0.5, None) + PC.energies(pr, c1, p1).sum())
        # a run that ends `Success` leaves BEFORE x = xTest (the reference's quirk, ba_mi355x.h): its energy is xTest's, the state is
        # x, and the flat-line rule that ended it says the two energies differ by less than tol_fun = 1e-8 of them
        running = ba.STATUS[r["status"]] == "Running"
        assert running or ba.STATUS[r["status"]] == "Success", r["status"]
        ck("final_energy@%d(%s)" % (ntr, ba.STATUS[r["status"]]), abs(r["energy"] - Ey) / Ey, TOL[0]["energy"] if running else 1e-8)
    tr = np.concatenate(rows)
    acc = tr[tr[:, 1] == 1]
    ck("accepted_rows>=3", 3 - len(acc), 0)
    ck("energy_rises", float(np.diff(acc[:, 2]).max()) if len(acc) > 1 else 0.0, 0.0)
    p1l = p1.reshape(-1, 3)[lone]
    assert (p1l[free_lone] != pts0[lone][free_lone]).any(axis=1).all() and np.array_equal(p1l[~free_lone], pts0[lone][~free_lone])
    ck.done()


# ---- 5. mask -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("skind", [2, 5], ids=["cholesky", "iterschur"])
def test_mask_and_priors(ba, O, gpu_ok, prob21, skind):
    pg = prob21
    po = sorted_oracle_problem(O, pg)
    pr = _priors(ba, O, pg, "p21")
    cm = pg.gauge_mask(0)
    pf = np.zeros(pg.M, np.uint8)
    pf[np.random.default_rng(1).choice(pg.M, pg.M // 100, replace=False)] = 1
    pf[pr.pt_ids[::2]] = 1  # priors on fixed points too (and camera 0, whose pose is fixed, has a centre prior)
    s = ba.Solver(pg, skind, ba.F64)
    pr.apply(s)
    s.set_constant(cm, pf)
    energy, dmax = s.linearize()
    cams0, pts0 = s.get(ba.GET_CAMS).copy(), s.get(ba.GET_POINTS).copy()
    Y = _yardstick(O, po, pr, cams0, pts0, LC.REFERENCE, 0.5, None, cm, pf)
    ck = Checker("mask[%s]" % ba.KIND_NAMES[skind])
    ck("energy", abs(energy - float(Y["energy"])) / float(Y["energy"]), TOL[0]["energy"])
    g = s.get(ba.GET_GRAD)
    ck("grad", relmax(g, Y["g"].astype(F64)), TOL[0]["g"])
    ck("diag_max", abs(dmax - float(Y["dmax"])) / float(Y["dmax"]), TOL[0]["g"])
    fc, fp = CC.free_sets(po, cm, pf)
    fixed = np.concatenate([np.repeat(~fp, 3), ~fc])
    assert fixed.any() and not g[fixed].any()
    s.try_step(1e-6 * dmax)
    dx = s.get(ba.GET_DX)
    assert not dx[fixed].any() and dx[~fixed].any()
    r = s.minimize(max_trials=10)
    cams1, pts1 = s.get(ba.GET_CAMS).reshape(-1, 15), s.get(ba.GET_POINTS).reshape(-1, 3)
    assert np.array_equal(pts1[pf != 0], pts0.reshape(-1, 3)[pf != 0]) and not np.array_equal(pts1, pts0.reshape(-1, 3))
    assert np.array_equal(cams1[0, :12], cams0.reshape(-1, 15)[0, :12])
    assert np.isfinite(r["energy"])
    ck.done()


# ---- 6. covariance -----------------------------------------------------------------------------------------------------------------------
def test_covariance_with_priors(ba, O, gpu_ok, prob21):
    """problem-21 at its start state, no mask, plain least squares, weights 1: compute(0) is BA_ERR_SINGULAR without priors (the control)
    and BA_OK with them.  test_gpu_covariance.py's metrics and bounds on the augmented problem at the GPU's own J: the camera blocks'
    column errors eta against the quad S (bound max(10 x cov_checks.reference_covariance's numpy inverse, 1e-16)), the point blocks
    against the formula in long double on the refined inverse (bound max(10 x reference_covariance's, 1e-15))."""
    pg = prob21
    po = sorted_oracle_problem(O, pg)
    pr = _priors(ba, O, pg, "p21")
    s = ba.Solver(pg, ba.CHOLESKY, ba.F64)
    s.set_loss(ba.LOSS_TRIVIAL)
    s.linearize()
    with pytest.raises(ba.BAError) as ei:
        s.covariance(0.0, cams=[0])
    assert ei.value.code == ba.ERR_SINGULAR
    pr.apply(s)
    with pytest.raises(ba.BAError) as ei:  # stale: a model set since the last linearisation
        s.covariance(0.0, cams=[0], compute=False)
    assert ei.value.code == ba.ERR_ARG
    s.linearize()
    N = pg.N
    pts_sel = np.unique(np.concatenate([pr.pt_ids[:40], np.random.default_rng(9).choice(pg.M, 60, replace=False)])).astype(np.int32)
    a_, b_ = np.meshgrid(np.arange(N), np.arange(N), indexing="ij")
    cc, pp = s.covariance(0.0, cam_pairs=np.stack([a_.ravel(), b_.ravel()], axis=1).astype(np.int32), points=pts_sel)
    assert np.isfinite(cc).all() and np.isfinite(pp).all()
    Sig = cc.reshape(N, N, 9, 9).transpose(0, 2, 1, 3).reshape(9 * N, 9 * N)
    pa, Jc, Jp, f = _augmented(O, po, pr, s, ba)
    fc, fp = CC.free_sets(pa)
    S = CC.quad_reduced(O, O.CHOLESKY, pa, Jc, Jp, 0.0, fp)
    ck = Checker("cov[p21]")
    cpu = CC.reference_covariance(pa, Jc, Jp, 0.0, points=pts_sel)
    eta_cpu = float(CC.column_errors(O, S, cpu["cc"], fc).max())
    ck("eta_max(cpu %.1e)" % eta_cpu, CC.column_errors(O, S, Sig, fc).max(), max(10 * eta_cpu, 1e-16))
    ref = CC.point_covariance(pa, Jc, Jp, 0.0, fp, CC.refined_inverse(S, fc), pts_sel, np.longdouble)
    e_cpu = float(CC.block_errors(cpu["pp"], ref).max())
    ck("point_blocks(cpu %.1e)" % e_cpu, CC.block_errors(pp, ref).max(), max(10 * e_cpu, 1e-15))
    ck.done()


# ---- 7. minimise ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("skind", [2, 5], ids=["cholesky", "iterschur"])
def test_minimise_with_priors(ba, O, gpu_ok, prob21, skind):
    pg = prob21
    po = sorted_oracle_problem(O, pg)
    pr = _priors(ba, O, pg, "p21")
    cm = np.zeros(pg.N, np.uint16)
    cm[3] = ba.FIX_INTRINSICS
    s = ba.Solver(pg, skind, ba.F64)
    pr.apply(s)
    s.set_constant(cm, None)
    cams0 = s.get(ba.GET_CAMS).reshape(-1, 15).copy()
    Y = _yardstick(O, po, pr, s.get(ba.GET_CAMS), s.get(ba.GET_POINTS), LC.REFERENCE, 0.5, None, cm, None)
    r = s.minimize()
    tr = r["trace"]
    ck = Checker("minimise[%s]" % ba.KIND_NAMES[skind])
    ck("row1_f", abs(tr[0, 2] - float(Y["energy"])) / float(Y["energy"]), TOL[0]["energy"])
    acc = tr[tr[:, 1] == 1]
    ck("accepted_rows>=3", 3 - len(acc), 0)
    ck("energy_rises", float(np.diff(acc[:, 2]).max()), 0.0)
    assert ba.STATUS[r["status"]] == "Success", r["status"]
    s.linearize()
    assert np.isfinite(s.prior_energy()).all() and s.prior_energy().sum() > 0
    assert np.array_equal(s.get(ba.GET_CAMS).reshape(-1, 15)[3, 12:15], cams0[3, 12:15])
    print("PRIOR minimise[%s] rows %d final energy %.9g prior energies %s" % (ba.KIND_NAMES[skind], len(tr), r["energy"], s.prior_energy()))
    ck.done()


# ---- 8. errors -----------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_solver_unchanged(ba, O, gpu_ok, prob21):
    import ctypes as C
    L, _p = ba.lib(), ba._p
    pr = _priors(ba, O, prob21, "p21")
    s = ba.Solver(prob21, ba.CHOLESKY, ba.F64)
    pr.apply(s)

    def observe():
        out = [np.array(s.linearize()), s.prior_energy().copy()]
        out.append(np.array(s.try_step(1e-12 * out[0][1])))
        out.append(s.get(ba.GET_DX).copy())
        return out
    before = observe()
    ids = np.array([0, 1], np.int32)
    x0, Lm, w = np.zeros((2, 3)), np.tile(np.eye(3), (2, 1, 1)), np.ones((2, 3))

    def bad(a, v):
        b = a.copy()
        b.reshape(-1)[-1] = v
        return b
    calls = []
    for fn, lim, info in ((L.ba_solver_set_point_priors, prob21.M, Lm), (L.ba_solver_set_centre_priors, prob21.N, Lm),
                          (L.ba_solver_set_intrinsics_priors, prob21.N, w)):
        calls += [(fn, 2, np.array([0, lim], np.int32), x0, info), (fn, 2, np.array([-1, 0], np.int32), x0, info),
                  (fn, 2, np.array([1, 1], np.int32), x0, info), (fn, 2, ids, bad(x0, np.nan), info), (fn, 2, ids, x0, bad(info, np.inf)),
                  (fn, -1, ids, x0, info), (fn, 2, None, x0, info), (fn, 2, ids, None, info), (fn, 2, ids, x0, None)]
    for fn, n, i, x, info in calls:
        assert fn(s._h, n, _p(i), _p(x), _p(info)) == ba.ERR_ARG, (fn.__name__, n)
    # (a refused call is no change: try_step is still allowed, nothing is stale)
    et = s.try_step(1e-12 * before[0][1])
    assert np.array_equal(np.array(et), before[2])
    after = observe()
    for k, (x, y) in enumerate(zip(before, after)):
        assert np.array_equal(x, y), k
    # another kind, a sharded solver
    for kind in (ba.QRKIT, ba.QRCHOL, ba.MOREQR, ba.QRSPQR):
        q = ba.Solver(prob21, kind, ba.F64)
        for fn, info in ((L.ba_solver_set_point_priors, Lm), (L.ba_solver_set_centre_priors, Lm), (L.ba_solver_set_intrinsics_priors, w)):
            assert fn(q._h, 2, _p(ids), _p(x0), _p(info)) == ba.ERR_ARG, kind
    q = ba.Solver(prob21, ba.CHOLESKY, ba.F64, shard_rank=0, shard_world=2)
    p0 = np.array([q.p0, q.p0 + 1], np.int32)
    assert L.ba_solver_set_point_priors(q._h, 2, _p(p0), _p(x0), _p(Lm)) == ba.ERR_ARG
    assert L.ba_solver_set_centre_priors(q._h, 2, _p(ids), _p(x0), _p(Lm)) == ba.ERR_ARG
    assert L.ba_solver_set_intrinsics_priors(q._h, 2, _p(ids), _p(x0), _p(w)) == ba.ERR_ARG
    # ba_solver_prior_energy: another kind, a sharded solver, no linearisation yet, a model set since the last one
    out3 = np.empty(3)
    assert L.ba_solver_prior_energy(q._h, _p(out3)) == ba.ERR_ARG
    q = ba.Solver(prob21, ba.QRCHOL, ba.F64)
    q.linearize()
    assert L.ba_solver_prior_energy(q._h, _p(out3)) == ba.ERR_ARG
    q = ba.Solver(prob21, ba.ITERSCHUR, ba.F32)
    assert L.ba_solver_prior_energy(q._h, _p(out3)) == ba.ERR_ARG
    q.linearize()
    assert L.ba_solver_prior_energy(q._h, _p(out3)) == 0 and not out3.any()  # (no priors: zeros)
    q.set_loss(ba.LOSS_HUBER, 1.0)
    assert L.ba_solver_prior_energy(q._h, _p(out3)) == ba.ERR_ARG
    # a set call: try_step and covariance_get wait for the next linearisation
    s.set_loss(ba.LOSS_TRIVIAL)
    s.linearize()
    s.covariance(0.0, cams=[0])
    s.set_centre_priors(pr.c_ids, pr.c_c0, sqrt_info=pr.c_L)
    e, r_, n_ = C.c_double(), C.c_double(), C.c_double()
    assert L.ba_solver_try_step(s._h, 1.0, C.byref(e), C.byref(r_), C.byref(n_)) == ba.ERR_ARG
    with pytest.raises(ba.BAError) as ei:
        s.covariance(0.0, cams=[0], compute=False)
    assert ei.value.code == ba.ERR_ARG
    assert L.ba_solver_prior_energy(s._h, _p(out3)) == ba.ERR_ARG
    # device_bytes counts the lists
    b1 = s.device_bytes()
    PC.Priors().apply(s)
    assert s.device_bytes() < b1
