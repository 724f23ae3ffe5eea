"""The model-decrease stopping rule (tests/qstop_checks.py) on the CPU oracle's linearisation alone, and the ABI of the feature.

  the rule       on problem-21 and synthetic(9, 260, 900, 31) at 1e-12, 1e-6 and 1e-2 max diag J'J, in long double: s_k increases and stays
                 below rhs'S^-1 rhs, x_k is orthogonal to r_k (what makes LM's rhoScale the exact model decrease of a truncated step:
                 DESIGN.md section 20), and eta = 0.1 stops no later than the residual rule at 1e-6
  choosing eta   every case of tests/test_gpu_pcg_model_stop.py offers, for each of its targets, an eta with clearance >= 1.2 -- on the
                 oracle's linearisation, which is the GPU's up to rounding
  teeth          each planted defect (zeta without its factor k, s_{k-1} from the slot of s_{k-2}, the last block of 256 cameras left
                 out of s on a 257-camera system) moves the stopping index of a listed case
  the ABI        the built library exports both entry points and the Python wrapper has both methods

No GPU needed.  s_k is checked for the iterates a solve can return, k up to the residual rule's stop at the default rel_tol 1e-6 (behind
it the rounding error of s_k - s_{k-1} is what is left of the difference).  The orthogonality is checked for the truncated steps, k up to
the model rule's stop at eta = 0.01, the smallest eta of DESIGN.md section 20's table: in exact arithmetic it holds at every k, in floating
point CG loses it geometrically with k -- even in long double |x'r| / (|x| |r|) reaches 2e-6 on problem-21 at 1e-12 max diag J'J by k = 81
and 5e-3 on synthetic(9, ...) at 1e-6 by k = 51, while it is at most 3e-17 at every truncated step.  Both ranges' figures are printed, with
|x'r| / s_k, the share of the model decrease that LM's rhoScale then misses."""
import numpy as np
import pytest

import pcg_checks as PC
import qstop_checks as Q
import shared_checks as SH
from conftest import DATA21, to_oracle
from test_pcg_checks import _system

LAMS = (1e-12, 1e-6, 1e-2)


@pytest.fixture(scope="module")
def systems(O):
    import bundleadjustment_benchmarks_amd as ba
    p21 = O.load_bal(DATA21)
    syn = to_oracle(ba.Problem.synthetic(9, 260, 900, 31))
    return {(n, x): _system(O, p, x) for n, p in (("p21", p21), ("syn9", syn)) for x in LAMS}


def _run(sy, **kw):
    return Q.pcg_model(sy["rhs"], Q.dense(sy["S"]), SH.block_prec(sy["Minv"]), Q.K_MAX, **kw)


@pytest.mark.parametrize("x", LAMS)
@pytest.mark.parametrize("name", ["p21", "syn9"])
def test_the_rule(systems, name, x):
    sy = systems[(name, x)]
    res = _run(sy, rel_tol=1e-6)
    k6 = res["iters"]
    assert res["rule"] == 1 and k6 >= 1, (res["rule"], k6)
    s = np.array(res["s_acc"])  # long double
    assert np.all(np.diff(s) > 0), np.diff(s)
    x_inf = SH.dense_solve(sy["S"], sy["rhs"], [])
    s_inf = (np.asarray(sy["rhs"], Q.LD) * x_inf).sum()
    assert np.all(s <= s_inf * (1 + Q.LD(1e-15))), (s[-1], s_inf)
    k01 = Q.stop_index(res["zeta"], 0.01) or k6  # the latest truncated step of DESIGN.md section 20's table (eta = 0.01)
    print("QSTOP %s@%.0e k(1e-6) %d k(eta = 0.01) %d s_k / s_inf at k = 1, 2, 5, 9, 13: %s  zeta_1..8 %s" % (name, x, k6, k01, [float(s[k] / s_inf) for k in (1, 2, 5, 9, 13) if k <= k6], res["zeta"][1:9]))
    print("QSTOP %s@%.0e max |x'r| / (|x| |r|): %.2e up to k(eta = 0.01), %.2e up to k(1e-6); max |x'r| / s_k: %.2e, %.2e"
          % (name, x, res["xr"][:k01].max(), res["xr"].max(), res["xr_model"][:k01].max(), res["xr_model"].max()))
    assert res["xr"][:k01].max() <= 1e-12, res["xr"][:k01]
    assert res["zeta"][1] == 1.0  # (s_0 = 0: the rule cannot fire before k = 2)
    stop = _run(sy, rel_tol=1e-6, eta=0.1)
    assert stop["iters"] <= k6 and (stop["rule"] == 2 or stop["iters"] == k6), (stop["iters"], stop["rule"], k6)
    for k in range(1, stop["iters"]):
        assert not res["zeta"][k] < 0.1, (k, res["zeta"][k])


def test_choose_eta():
    """On problem-21's measured sequence at 1e-12 max diag J'J: 0.1 is a coin toss between k = 3 and 6, and the
    chosen eta is not."""
    zeta = np.array([0, 1.0, 0.181, 0.101, 0.110, 0.104, 0.077, 0.050, 0.050, 0.034, 0.038, 0.038, 0.018, 0.009])
    assert Q.choose_eta(zeta, 2)[1] == 2
    eta, k, clear = Q.choose_eta(zeta, 4)  # (4 and 5 are above zeta_3, 6 is inside 1.2 of it)
    assert k == 7 and clear >= Q.CLEARANCE and Q.stop_index(zeta, eta) == 7
    eta, k, clear = Q.choose_eta(zeta, 10)
    assert k == 12 and abs(eta - 0.0247) < 1e-3 and abs(clear - 1.37) < 0.01 and Q.stop_index(zeta, eta) == 12
    assert Q.choose_eta(np.array([0, 1.0, 0.5, 0.45, 0.44]), 3) is None
    assert (Q.stop_index(zeta, 0.1 * 1.02), Q.stop_index(zeta, 0.1 / 1.02)) == (3, 6)  # (a fixed eta = 0.1: 2 % decide between 3 and 6)


# ---- the GPU cases on the oracle's linearisation -------------------------------------------------------------------------------------------
_CASES = {}


def oracle_case(O, ba, name):
    """qstop_checks.Case of a case of Q.CASES from the oracle's J at the start state (tests/test_gpu_pcg_model_stop.py: from the GPU's),
    built once."""
    if name not in _CASES:
        _CASES[name] = _oracle_case(O, ba, name)
    return _CASES[name]


def _oracle_case(O, ba, name):
    import visibility_checks as VC
    from test_gpu_pcg_stages import chunk_edge_problem
    prob, lam_rel, what, _ = Q.CASES[name]
    pg = {"p21": lambda: ba.Problem.load_bal(DATA21), "syn2": lambda: ba.Problem.synthetic(2, 40, 80, 5), "edges": lambda: chunk_edge_problem(ba),
          "syn257": lambda: ba.Problem.synthetic(257, 12 * 257, 60 * 257, 4257), "syn600": lambda: ba.Problem.synthetic(600, 12 * 600, 60 * 600, 4600)}[prob]()
    p = to_oracle(pg)
    order = np.argsort(p.pt_idx, kind="stable")
    p = O.Problem(p.N, p.M, p.K, p.cam_idx[order], p.pt_idx[order], p.meas.reshape(-1, 2)[order].ravel(), p.cams9, p.pts)
    cam = O.init_cams(p)
    lin = dict(po=p)
    if what == "group":
        lin["groups"] = [np.arange(p.N)]
        cam = np.array(cam).reshape(p.N, 15)
        cam[:, 12:15] = cam[0, 12:15]
        cam = cam.ravel()
    f, e = O.residuals(p, cam, p.pts)
    Jc, Jp = O.jacobian(p, cam, p.pts)
    if what == "gauge":
        Jc = Q.mask_columns(Jc, p.cam_idx, pg.gauge_mask(0))
    dmax = O.step(O.CHOLESKY | O.ASSEMBLE_ONLY, p, Jc, Jp, f, 1.0, want_S=False)["diagmax"]
    lin.update(Jc=np.asarray(Jc).reshape(p.K, 2, 9), Jp=np.asarray(Jp).reshape(p.K, 2, 3), f=f, lam=lam_rel if what == "marquardt" else lam_rel * dmax)
    if what == "cforest":
        lin.update(cams=cam, cs=Q.chain(p.N, p.cam_idx, p.pt_idx, cam, Jc))
    if what == "vforest":
        lin["cov"] = VC.covisibility(p.N, p.cam_idx, p.pt_idx)[0]
    return Q.Case(O, what, lin)


@pytest.mark.parametrize("name", list(Q.CASES))
def test_gpu_cases_offer_an_eta(O, name):
    import bundleadjustment_benchmarks_amd as ba
    c = oracle_case(O, ba, name)
    for scalar in Q.CASES[name][3]:
        for eta, ks, clear in Q.chosen(c, scalar):
            print("QSTOP %s,%s: eta %.4g k* %d clearance %.2f (residual rule at %.0e: k = %d)" % (name, ("f64", "f32")[scalar], eta, ks, clear, Q.RES_TOL[scalar],
                                                                                              c.k_residual(Q.RES_TOL[scalar])))


@pytest.mark.parametrize("name", ["p21@1e-6", "p21-group", "p21-constraint-forest", "p21-visibility-forest", "p21-marquardt"])
def test_working_precision_yardstick_stops_where_the_reference_does(O, name):
    """qstop_checks.Case.working, the yardstick of the GPU tests, on the oracle's linearisation (its own gradient -J'e in place of the
    device's): in fp64 and fp32 it stops at the reference's k* for every chosen eta, and its zeta_k* is off by less than half the
    clearance the eta was chosen with -- what the choice of eta exists to guarantee.  The deviation of s_k is printed: it is what the GPU
    test multiplies by 10 for its bound."""
    import bundleadjustment_benchmarks_amd as ba
    import damping_checks as DC
    import relpose_checks as RC
    c = oracle_case(O, ba, name)
    lin = c.lin
    if lin.get("g") is None:
        g = np.asarray(DC.trial(lin["po"], lin["Jc"], lin["Jp"], lin["f"], lin["lam"], kind=DC.MARQUARDT if c.what == "marquardt" else DC.IDENTITY,
                                want_step=False)["g"], np.float64)
        if c.what == "cforest":
            g[3 * lin["po"].M:] += np.asarray(RC.direct(lin["cs"], c.N, lin["cams"], None)["g"], np.float64)
        lin["g"], c.gc = g, g[3 * lin["po"].M:]
    ref = c.reference()
    for scalar, dt in ((0, np.float64), (1, np.float32)):
        for eta, ks, clear in Q.chosen(c, scalar):
            y = c.working(dt, ks + 8, eta=eta, keep=[ks])
            assert y is not None and (y["iters"], y["rule"]) == (ks, 2), (name, dt, eta, ks, None if y is None else (y["iters"], y["rule"]))
            ds, dz = abs(y["s"][ks] / ref["s"][ks] - 1), abs(y["zeta"][ks] / ref["zeta"][ks] - 1)
            print("QSTOP %s,%s yardstick: eta %.4g k* %d s_k off by %.2e zeta_k off by %.2e" % (name, dt.__name__, eta, ks, ds, dz))
            assert dz <= (clear - 1) / 2, (ds, dz)


def test_planted_defects_move_the_stop(O, systems):
    """zeta without k, and s_{k-1} from two iterations back, on problem-21 at 1e-6 max diag J'J; the last block of partials left out of
    s on synthetic(257, ...): each stops at another k than the reference for an eta chosen with clearance."""
    import bundleadjustment_benchmarks_amd as ba
    sy = systems[("p21", 1e-6)]
    ref = _run(sy, rel_tol=Q.REF_TOL)
    moved = {"no_factor_k": 0, "stale_slot": 0}
    for kt in (2, 4, 17):
        eta, ks, _ = Q.choose_eta(ref["zeta"], kt)
        assert _run(sy, eta=eta)["iters"] == ks
        moved["no_factor_k"] += _run(sy, eta=eta, zeta_k_factor=False)["iters"] != ks
        moved["stale_slot"] += _run(sy, eta=eta, prev_lag=2)["iters"] != ks
    assert all(moved.values()), moved
    c = oracle_case(O, ba, "syn257")
    ref = c.reference()
    rows = np.ones(9 * 257, bool)
    rows[9 * 256:] = False
    eta, ks, _ = Q.chosen(c, 0)[-1]
    bad = Q.pcg_model(c.rhs, Q.dense(c.S), c.prec, ks + 30, eta=eta, s_rows=rows)
    print("QSTOP syn257 block dropped: k* %d stops at %d (rule %d)" % (ks, bad["iters"], bad["rule"]))
    assert bad["iters"] != ks


def test_abi():
    """Fails on a library or a wrapper without the feature."""
    import bundleadjustment_benchmarks_amd as ba
    L = ba.lib()
    for sym in ("ba_solver_set_pcg_model_tol", "ba_solver_pcg_stop_stats"):
        assert sym in ba.EXPORTS and hasattr(L, sym), sym
    assert callable(ba.Solver.set_pcg_model_tol) and callable(ba.Solver.pcg_stop_stats)
    assert [n for n, _ in ba.PCGStopStats._fields_] == ["by_residual", "by_model", "at_cap", "last_rule", "last_zeta", "last_model"]
    with open(__import__("os").path.join(__import__("os").path.dirname(ba.__file__), "..", "include", "ba_mi355x.h")) as fh:
        h = fh.read()
    assert "int ba_solver_set_pcg_model_tol(ba_solver *s, double eta);" in h and "} ba_pcg_stop_stats;" in h
