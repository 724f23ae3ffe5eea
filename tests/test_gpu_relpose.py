"""GPU: relative-pose constraints between camera pairs (ba_solver_set_relative_poses) through the C ABI, against tests/relpose_checks.py
on top of prior_checks.py / loss_checks.py (all long double; pinned on the CPU by test_relpose_checks.py and their own files).

The constraint set is relpose_checks.standard_constraints: an odometry chain over all cameras plus a hub camera tied to 40 others,
R0 / t0 the start state's relative pose moved by 0.05 rad and 1 % of |t_ab|, information kappa x the median own diagonal of the blocks
joined (kappa_t = 10, kappa_r = 1); the sigmas are printed per problem (`RELPOSE sigmas ...`).

Bounds.  Linearisation: test_gpu_loss.py's TOL for the same quantities.  Trial: test_gpu_stages.py's BOUND for S, rhs (max(10 x the
oracle's error on the same system, floor), as test_gpu_priors.py applies it), eta, e_test, rho_scale.  ITERSCHUR: test_gpu_pcg_stages.py's
metric, yardstick and FLOOR / allowance.  Covariance: test_gpu_covariance.py's column metric, max(10 x numpy's own, 1e-16).  Every figure
is printed as `RELPOSE <case> <metric> <value> <bound>` before it is asserted."""
import ctypes as C

import numpy as np
import pytest

import cov_checks as CC
import loss_checks as LC
import pcg_checks as PCG
import prior_checks as PC
import relpose_checks as RC
import stage_checks as SC
from test_gpu_loss import TOL, _weights
from test_gpu_parity import _ragged_problem, relmax
from test_gpu_pcg_stages import FLOOR, allowance, quad_rel_residual
from test_gpu_priors import MODELS, _augmented, _priors, _solver_priors
from test_gpu_stages import BOUND, EPS, sorted_oracle_problem

pytestmark = pytest.mark.gpu
F64 = np.float64
LD = np.longdouble
SN = {0: "f64", 1: "f32"}


class Checker:
    def __init__(self, case):
        self.case, self.rows = case, []

    def __call__(self, metric, value, bound):
        self.rows.append((metric, float(value), float(bound)))
        print("RELPOSE %s %s %.3e %.1e" % (self.case, metric, value, bound))

    def done(self):
        bad = [r for r in self.rows if not (r[1] <= r[2])]
        assert not bad, (self.case, bad)


_PROBLEMS, _CONSTRAINTS = {}, {}


def _problem(ba, name, prob21, prob39):
    if name not in _PROBLEMS:
        _PROBLEMS[name] = {"p21": lambda: prob21, "p39": lambda: prob39, "ragged": lambda: _ragged_problem(ba),
                           "syn2": lambda: ba.Problem.synthetic(2, 40, 80, 5),
                           "syn257": lambda: ba.Problem.synthetic(257, 12 * 257, 60 * 257, 4257)}[name]()
    return _PROBLEMS[name]


WIDE_ANGLES = (1e-9, 5e-4, 1e-2, 1.0, 2.5, float(np.pi) - 1e-3)  # both series, both closed forms, c < 0, the neighbourhood of pi


def _constraints(ba, O, pg, name, wide=False):
    """standard_constraints of a problem, sized from the fp64 CHOLESKY linearisation at the start state, once per problem.  wide: the
    residual rotations cycle through WIDE_ANGLES instead of 0.05 rad."""
    key = (name, wide)
    if key not in _CONSTRAINTS:
        po = sorted_oracle_problem(O, pg)
        s = ba.Solver(pg, ba.CHOLESKY, ba.F64)
        s.linearize()
        V = np.zeros((pg.N, 9))
        np.add.at(V, po.cam_idx, (s.get(ba.GET_JC).reshape(-1, 2, 9) ** 2).sum(axis=1))
        cs, info = RC.standard_constraints(pg.N, po.cam_idx, po.pt_idx, s.get(ba.GET_CAMS), V, **(dict(angle=WIDE_ANGLES) if wide else {}))
        print("RELPOSE sigmas %s trans %.3e rot %.3e (%d constraints, hub %d, %d pairs without a common point, at most %d common points)"
              % (name + ("-wide" if wide else ""), info["sigma_t"], info["sigma_r"], info["n"], info["hub"], info["n_no_common"], info["max_common"]))
        _CONSTRAINTS[key] = (cs, info)
    return _CONSTRAINTS[key]


def _rounded(cs, scalar):
    return cs.rounded(np.float32) if scalar == 1 else cs


def _make(ba, pg, skind, scalar, model, pr, cs):
    kind, scale, weighted = MODELS[model]
    w = _weights(pg.K) if weighted else None
    s = ba.Solver(pg, skind, scalar)
    if model != "default":
        s.set_loss(kind, scale)
        s.set_obs_weights(w)
    if pr is not None:
        _solver_priors(pr, scalar).apply(s)
    if cs is not None:
        _rounded(cs, scalar).apply(s)
    order = np.argsort(pg.arrays()["pt_idx"], kind="stable")
    wy = None if w is None else (w.astype(np.float32).astype(F64) if scalar == 1 else w)[order]
    return s, kind, scale, wy


def _yardstick(O, po, pr, cs, cams, pts, kind, scale, w, cm=None, pf=None):
    """Energy, constraint energies, g and max diag J'J of observations + priors + constraints at the state, long double."""
    Y = LC.model(O, po, cams, pts, kind, scale, w)
    Jc, Jp = Y["Jc"], Y["Jp"]
    if cm is not None or pf is not None:
        fc, fp = CC.free_sets(po, cm, pf)
        Jc = Jc * fc.reshape(po.N, 9)[po.cam_idx][:, None, :]
        Jp = Jp * fp[po.pt_idx][:, None, None]
    U, V, g, e = PC.normal_blocks(po.N, po.M, po.cam_idx, po.pt_idx, Jc, Jp, Y["e"])
    dp = PC.direct(pr if pr is not None else PC.Priors(), po.N, po.M, cams, pts, cm, pf)
    dc = RC.direct(cs, po.N, cams, cm)
    U, V, g = U + dp["U"], V + dp["V"] + dc["V"], g + dp["g"]
    g[3 * po.M:] += dc["g"]
    dmax = max(np.einsum("nii->ni", U).max(), np.einsum("nii->ni", V).max())
    return dict(energy=e + dp["energy"] + dc["energy"], energies=dc["energies"], g=g, dmax=dmax)


# ---- 1. linearisation --------------------------------------------------------------------------------------------------------------------
LIN_CASES = [("p21", "plain"), ("ragged", "plain"), ("p39", "plain"), ("syn2", "plain"), ("syn257", "plain"), ("p21", "priors"), ("p21", "mask")]


@pytest.mark.parametrize("scalar", [0, 1], ids=["f64", "f32"])
@pytest.mark.parametrize("skind", [2, 5], ids=["cholesky", "iterschur"])
@pytest.mark.parametrize("prob,variant", LIN_CASES, ids=["%s-%s" % c for c in LIN_CASES])
def test_linearisation_matches_the_yardstick(ba, O, gpu_ok, prob21, prob39, prob, variant, skind, scalar):
    """Energy, the two constraint energies, BA_GET_GRAD and max diag J'J.  `priors`: Huber + weights + standard_priors on top; `mask`:
    the pose of chain camera 3 and T1 of the hub's first neighbour held constant."""
    _check_linearisation(ba, O, prob21, prob39, prob, variant, skind, scalar, False)


@pytest.mark.parametrize("skind,scalar", [(2, 0), (2, 1), (5, 0)], ids=["cholesky-f64", "cholesky-f32", "iterschur-f64"])
def test_linearisation_matches_the_yardstick_at_wide_angles(ba, O, gpu_ok, prob21, prob39, skind, scalar):
    """The same quantities under the same bounds on problem-21 with the constraints' residual rotations cycling through WIDE_ANGLES:
    every branch of ba_relpose_eval through the C ABI (the standard set holds all of them at 0.05 rad)."""
    _check_linearisation(ba, O, prob21, prob39, "p21", "plain", skind, scalar, True)


def _check_linearisation(ba, O, prob21, prob39, prob, variant, skind, scalar, wide):
    pg = _problem(ba, prob, prob21, prob39)
    po = sorted_oracle_problem(O, pg)
    cs, info = _constraints(ba, O, pg, prob, wide)
    if prob == "syn2":
        assert len(cs) == 1
    if prob == "syn257":
        assert len(cs) > 256  # two workgroups of partials
    pr = _priors(ba, O, pg, prob) if variant == "priors" else None
    s, kind, scale, wy = _make(ba, pg, skind, scalar, "huber_w" if variant == "priors" else "default", pr, cs)
    cm = None
    if variant == "mask":
        cm = np.zeros(pg.N, np.uint16)
        cm[3] = ba.FIX_POSE
        nb = [int(x) for p_ in cs.pairs[pg.N - 1:] for x in p_ if x != info["hub"] and x != 3][0]
        cm[nb] |= 0x002  # T1
        s.set_constant(cm, None)
    energy, dmax = s.linearize()
    Y = _yardstick(O, po, None if pr is None else _solver_priors(pr, scalar), _rounded(cs, scalar), s.get(ba.GET_CAMS), s.get(ba.GET_POINTS),
                   kind, scale, wy, cm, None)
    tol = TOL[scalar]
    ck = Checker("lin[%s,%s,%s,%s]" % (prob, "wide" if wide else variant, ba.KIND_NAMES[skind], SN[scalar]))
    ck("energy", abs(energy - float(Y["energy"])) / float(Y["energy"]), tol["energy"])
    ce = s.relative_pose_energy()
    for q, name in enumerate(("rot", "trans")):
        assert float(Y["energies"][q]) > 0
        ck("constraint_energy_%s" % name, abs(ce[q] - float(Y["energies"][q])) / float(Y["energies"][q]), tol["energy"])
    g = s.get(ba.GET_GRAD)
    ck("grad", relmax(g, Y["g"].astype(F64)), tol["g"])
    ck("diag_max", abs(dmax - float(Y["dmax"])) / float(Y["dmax"]), tol["g"])
    if cm is not None:
        fixed = np.concatenate([np.zeros(3 * pg.M, bool), ~CC.free_sets(po, cm, None)[0]])
        assert fixed.sum() == 7 and not g[fixed].any()
    ck.done()


# ---- 2. trial, CHOLESKY --------------------------------------------------------------------------------------------------------------------
def _system_errors(po, Jc, Jp, f, lam, d, S, rhs, S_ref, rhs_ref):
    """stage_checks.assembly_errors with the constraints in its scales: S entry by entry over sqrt((U_ii + lam)(U_jj + lam)), U the
    diagonal of Jc'Jc + the constraints' V; rhs over sum |J| |r| (observations and constraint rows) + |rhs|."""
    dg = np.sqrt(SC.camera_diag(po, Jc) + np.einsum("nii->ni", d["V"]).astype(F64).ravel() + lam)
    dS = np.abs(np.asarray(S) - np.asarray(S_ref)) / dg[:, None] / dg[None, :]
    sc = SC.abs_grad(po, Jc, Jp, f)[3 * po.M:] + d["absg"] + np.abs(rhs_ref)
    num = np.abs(np.asarray(rhs) - rhs_ref)
    return dict(S=float(dS.max()), rhs=float(np.where(sc > 0, num / np.where(sc > 0, sc, 1), np.where(num > 0, np.inf, 0)).max()))


def _direct(cs, N, cams, cm=None, dt=LD):
    d = RC.direct(cs, N, cams, cm, dt)
    J, e = RC.stacked(cs, N, cams, cm)
    d["absg"] = (np.abs(J).T @ np.abs(e)).astype(F64)
    return d


TRIAL_CASES = [("p21", 0, True), ("ragged", 0, False), ("p39", 0, False), ("p21", 1, False)]


@pytest.mark.parametrize("prob,scalar,priors", TRIAL_CASES, ids=["p21-f64-priors", "ragged-f64", "p39-f64", "p21-f32"])
def test_trial_matches_the_yardstick(ba, O, gpu_ok, prob21, prob39, prob, scalar, priors):
    """CHOLESKY with keep_intermediates at lambda = 1e-6 and 1e-2 x max diag J'J: the kept S and rhs against the quad reduced system of
    the (prior-augmented) observations at the GPU's own J plus relpose_checks.direct; the block of a pair without a common point is
    H_ab alone; eta of the step, e_test and rho_scale."""
    _check_trial(ba, O, prob21, prob39, prob, scalar, priors, False)


@pytest.mark.parametrize("scalar", [0, 1], ids=["f64", "f32"])
def test_trial_matches_the_yardstick_at_wide_angles(ba, O, gpu_ok, prob21, prob39, scalar):
    """The same quantities under the same bounds on problem-21 with the constraints' residual rotations cycling through WIDE_ANGLES."""
    _check_trial(ba, O, prob21, prob39, "p21", scalar, False, True)


def _check_trial(ba, O, prob21, prob39, prob, scalar, priors, wide):
    pg = _problem(ba, prob, prob21, prob39)
    po = sorted_oracle_problem(O, pg)
    cs0, info = _constraints(ba, O, pg, prob, wide)
    cs = _rounded(cs0, scalar)
    pr0 = _priors(ba, O, pg, prob) if priors else PC.Priors()
    pr = _solver_priors(pr0, scalar)
    s, kind, scale, wy = _make(ba, pg, ba.CHOLESKY, scalar, "huber_w" if priors else "default", pr0 if priors else None, cs0)
    s.keep_intermediates(True)
    e0, dmax = s.linearize()
    cams = s.get(ba.GET_CAMS)
    pa, Jc, Jp, f = _augmented(O, po, pr, s, ba)
    d = _direct(cs, po.N, cams)
    g = s.get(ba.GET_GRAD)
    M, N = po.M, po.N
    ck = Checker("trial[%s%s,%s]" % (prob, ",wide" if wide else "", SN[scalar]))
    dt = F64 if scalar == 0 else np.float32
    lone = None
    assert info["n_no_common"] > 0 and info["max_common"] > 1, info  # (problem-21, -39 and the ragged one all have such pairs)
    if info["n_no_common"] > 0:  # the constrained pairs that share no point
        seen, ptc = set(), {}
        for c_, p_ in zip(po.cam_idx, po.pt_idx):
            ptc.setdefault(int(p_), set()).add(int(c_))
        for v in ptc.values():
            for x in v:
                for y in v:
                    seen.add((x, y))
        lone = [(int(a), int(b)) for a, b in cs.pairs if (int(a), int(b)) not in seen]
        assert lone
    for lam in (1e-6 * dmax, 1e-2 * dmax):
        et, rs, dn = s.try_step(lam)
        D = 9 * N
        S, rhs, dx = s.get(ba.GET_S).reshape(D, D), s.get(ba.GET_RHS), s.get(ba.GET_DX)
        R = O.referee_reduced_from_jacobian(ba.CHOLESKY, pa, Jc, Jp, f, lam)
        S_ref, rhs_ref = RC.reduced(R["S"].reshape(D, D), R["rhs"], d)
        S_ref, rhs_ref = S_ref.astype(F64), rhs_ref.astype(F64)
        st = O.step(ba.CHOLESKY, pa, Jc.astype(dt), Jp.astype(dt), f.astype(dt), lam)
        # the oracle has no constraints of its own: its S and rhs plus the same formulas evaluated plainly in the working precision
        dw = RC.direct(cs, po.N, cams, None, dt)
        add = lambda st_: ((st_["S"].reshape(D, D).astype(dt) + dw["S"]).astype(F64), (st_["rhs"].astype(dt) + dw["g"]).astype(F64))
        got = _system_errors(pa, Jc, Jp, f, lam, d, S, rhs, S_ref, rhs_ref)
        orc = _system_errors(pa, Jc, Jp, f, lam, d, *add(st), S_ref, rhs_ref)
        if not all(np.isfinite(v) for v in orc.values()):  # (the fp32 oracle's 3 x 3 LDL^T breaks down: fp64's error x eps32 / eps64)
            s64 = O.step(ba.CHOLESKY, pa, Jc, Jp, f, lam)
            d64 = RC.direct(cs, po.N, cams, None, F64)
            o64 = _system_errors(pa, Jc, Jp, f, lam, d, s64["S"].reshape(D, D) + d64["S"], s64["rhs"] + d64["g"], S_ref, rhs_ref)
            orc = {k: v * EPS[1] / EPS[0] for k, v in o64.items()}
        for k in ("S", "rhs"):
            ck("%s@%.0e(oracle %.1e)" % (k, lam, orc[k]), got[k], max(10 * orc[k], BOUND[(k, scalar)]))
        ck("S_asymmetry@%.0e" % lam, np.abs(S - S.T).max(), 0.0)
        if lone:
            dg = np.sqrt(np.diagonal(S_ref))
            worst = 0.0
            for a, b in lone:
                blk = S[9 * a:9 * a + 9, 9 * b:9 * b + 9]
                H = np.zeros((9, 9))
                H[:6, :6] = d["cross"][(a, b)].astype(F64)
                assert H.any()
                worst = max(worst, float((np.abs(blk - H) / dg[9 * a:9 * a + 9, None] / dg[None, 9 * b:9 * b + 9]).max()))
            ck("no_common_point_blocks@%.0e(%d pairs)" % (lam, len(lone)), worst, max(10 * orc["S"], BOUND[("S", scalar)]))
        ck("eta@%.0e" % lam, SC.eta(S, dx[3 * M:], rhs), BOUND[("eta", scalar)])
        ct, pt = s.get(ba.GET_CAMS_TEST), s.get(ba.GET_POINTS_TEST)
        e_ref = float(LC.energy(O, po, ct, pt, kind, scale, wy) + PC.energies(pr, ct, pt).sum() + RC.energies(cs, ct).sum())
        ck("e_test@%.0e" % lam, abs(et - e_ref) / e_ref, BOUND[("e_test", scalar)])
        dxl, gl = dx.astype(LD), g.astype(LD)
        rsy = (dxl * (LD(lam) * dxl + gl)).sum()
        ck("rho_scale@%.0e" % lam, float(abs(LD(rs) - rsy) / (np.abs(dxl) * (LD(lam) * np.abs(dxl) + np.abs(gl))).sum()), BOUND[("rho_scale", scalar)])
    ck.done()


# ---- 3. ITERSCHUR --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prob,scalar", [("p21", 0), ("ragged", 0), ("p21", 1)], ids=["p21-f64", "ragged-f64", "p21-f32"])
def test_pcg_iterates_with_constraints(ba, O, gpu_ok, prob21, prob39, prob, scalar):
    """test_gpu_pcg_stages.py's prefix iterates x_1 .. x_4, x_7 at lambda = 1e-6 max diag J'J, on the quad S and rhs of the GPU's own J
    plus the constraints' blocks (documented B_a and V_a with the constraints' diagonal blocks added), its iteration count with its
    allowance, and last_rel_residual against the quad residual of the returned step x_1 and x_3."""
    pg = _problem(ba, prob, prob21, prob39)
    po = sorted_oracle_problem(O, pg)
    cs0, _ = _constraints(ba, O, pg, prob)
    cs = _rounded(cs0, scalar)
    s = ba.Solver(pg, ba.ITERSCHUR, scalar)
    cs.apply(s)
    e, dmax = s.linearize()
    Jc, Jp = s.get(ba.GET_JC).reshape(po.K, 2, 9), s.get(ba.GET_JP).reshape(po.K, 2, 3)
    f, g = s.get(ba.GET_RESIDUALS), s.get(ba.GET_GRAD)
    d = RC.direct(cs, po.N, s.get(ba.GET_CAMS))
    lam = 1e-6 * dmax
    D = 9 * po.N
    R = O.referee_reduced_from_jacobian(O.CHOLESKY, po, Jc, Jp, f, lam)
    S_ld, rhs_ld = RC.reduced(R["S"].reshape(D, D), R["rhs"], d)
    S, rhs = S_ld.astype(F64), rhs_ld.astype(F64)
    B = PCG.documented_blocks(po, Jc, Jp, lam, R["S"]) + d["V"]
    Minv, ok = PCG.invert_blocks(B)
    assert ok.all()
    V = PCG.camera_blocks(po, Jc, lam) + d["V"]
    KS = (1, 2, 3, 4, 7)
    ref = PCG.pcg(S_ld, rhs, Minv, max(KS), keep=KS)
    dt = F64 if scalar == 0 else np.float32
    yard, scale_ = PCG.yardstick(S_ld, rhs, B, max(KS), dtype=dt, keep=KS, V=V, g=g[3 * po.M:]), 1.0
    if yard is None:
        yard, scale_ = PCG.yardstick(S_ld, rhs, B, max(KS), dtype=F64, keep=KS, V=V, g=g[3 * po.M:]), EPS[1] / EPS[0]
    ck = Checker("pcg[%s,%s]" % (prob, SN[scalar]))
    for k in KS:
        s.set_pcg(k, 1e-30)
        s.try_step(lam)
        st = s.pcg_stats()
        xk = s.get(ba.GET_DX)[3 * po.M:]
        yd = scale_ * PCG.iterate_error(yard["xs"][k], ref["xs"][k], S)
        ck("x%d(yardstick %.1e)" % (k, yd), PCG.iterate_error(xk, ref["xs"][k], S), max(10 * yd, FLOOR[("iterate", scalar)]))
        ck("x%d_capped" % k, 0 if (st["last_iters"] == k and st["last_converged"] == 0) else 1, 0)
        if k in (1, 3):  # the device's own |rhs - S x_k| / |rhs| against the quad one of the returned x_k (test_gpu_pcg_stages.py: at k = 1, 3)
            quad = quad_rel_residual(O, S, xk, rhs)
            yk = yard["xs"][k].astype(F64)
            yq = quad_rel_residual(O, S, yk, rhs)
            yr = scale_ * abs(PCG.working_residual(S_ld, yk, rhs, dt if scale_ == 1.0 else F64, V=V) - yq) / yq
            ck("residual%d(quad %.3e, yardstick %.1e)" % (k, quad, yr), abs(st["last_rel_residual"] - quad) / quad, max(10 * yr, FLOOR[("residual", scalar)]))
    tol = 1e-8 if scalar == 0 else 1e-4
    full = PCG.pcg(S_ld, rhs, Minv, 1000, tol)
    assert full["converged"]
    s.set_pcg(1000, tol)
    s.try_step(lam)
    st = s.pcg_stats()
    dx = s.get(ba.GET_DX)
    k_ref = full["iters"]
    ck("iterations(k_ref %d)" % k_ref, st["last_iters"], k_ref + allowance(k_ref))
    ck("converged", 0 if st["last_converged"] == 1 else 1, 0)
    quad = quad_rel_residual(O, S, dx[3 * po.M:], rhs)
    ck("rel_residual(quad %.3e)" % quad, quad, 2 * tol)
    # The device's own residual of the converged step.  There |r| is tol |rhs| and the product S x, formed the matrix-free way as
    # V x - (V - S) x in working precision, carries its rounding error in full: first order, row by row,
    #   |fl(rhs - S x) - (rhs - S x)| <= n eps ((|V| + |V - S|) |x| + |rhs|),
    # n the length of the longest sum behind one row (9 entries of V_a, the camera's observations, the longest track, 6 per incident
    # constraint), so the relative residual deviates from the quad one by at most n eps |(|V| + |V - S|) |x| + |rhs|| / (|rhs| quad)
    # relative to it.  (10 x the yardstick's own deviation, the bound at x_1 and x_3, is no bound here: one sample of rounding noise.
    # Measured on an MI355X: 4.9e-7 on the ragged problem, where that sample gave 4.1e-8.)
    xc = np.abs(dx[3 * po.M:])
    Vd = np.zeros((D, D))
    for a in range(po.N):
        Vd[9 * a:9 * a + 9, 9 * a:9 * a + 9] = V[a].astype(F64)
    n_sum = 9 + int(np.bincount(po.cam_idx, minlength=po.N).max()) + int(np.bincount(po.pt_idx, minlength=po.M).max()) \
        + 6 * int(np.bincount(cs.pairs.ravel(), minlength=po.N).max())
    noise = n_sum * EPS[scalar] * float(np.linalg.norm((np.abs(Vd) + np.abs(Vd - S)) @ xc + np.abs(rhs)) / np.linalg.norm(rhs)) / quad
    ck("last_rel_residual_vs_quad(n %d)" % n_sum, abs(st["last_rel_residual"] - quad) / quad, noise)
    ck.done()


# ---- 4. bit identity ---------------------------------------------------------------------------------------------------------------------
def _observe(ba, s, keep):
    out = [np.array(s.linearize())]
    out.append(s.get(ba.GET_GRAD).copy())
    lam = 1e-12 * out[0][1]
    for _ in range(3):
        out.append(np.array(s.try_step(lam)))
        out += [s.get(w).copy() for w in (ba.GET_DX, ba.GET_CAMS_TEST, ba.GET_POINTS_TEST)]
        if keep:
            out += [s.get(ba.GET_S).copy(), s.get(ba.GET_RHS).copy()]
        lam *= 10
    return out


def _fresh(ba, pg, skind, scalar):
    s = ba.Solver(pg, skind, scalar)
    s.keep_intermediates(skind == ba.CHOLESKY)
    return s


@pytest.mark.parametrize("scalar", [0, 1], ids=["f64", "f32"])
@pytest.mark.parametrize("skind", [2, 5], ids=["cholesky", "iterschur"])
def test_removed_and_zero_information_constraints_are_the_solver_without(ba, O, gpu_ok, prob21, skind, scalar):
    """linearize + 3 trials, bit for bit against a fresh solver: (a) constraints set, run (graphs captured) and removed with n = 0;
    (b) constraints whose L_t and L_r are all zero, through the constraint path."""
    cs, _ = _constraints(ba, O, prob21, "p21")
    keep = skind == ba.CHOLESKY
    fresh = _observe(ba, _fresh(ba, prob21, skind, scalar), keep)
    cams0 = ba.Solver(prob21, skind, scalar).get(ba.GET_CAMS)
    s = _fresh(ba, prob21, skind, scalar)
    _rounded(cs, scalar).apply(s)
    e1, _ = s.linearize()
    assert e1 != fresh[0][0]
    s.minimize(max_trials=3)
    s.set_state(cams0, prob21.arrays()["pts"])
    RC.Constraints().apply(s)
    for k, (x, y) in enumerate(zip(fresh, _observe(ba, s, keep))):
        assert np.array_equal(x, y), ("removed", k)
    z = _fresh(ba, prob21, skind, scalar)
    RC.Constraints(cs.pairs, cs.R0, cs.t0, 0 * cs.Lr, 0 * cs.Lt).apply(z)
    for k, (x, y) in enumerate(zip(fresh, _observe(ba, z, keep))):
        assert np.array_equal(x, y), ("zero information", k)
    assert not z.relative_pose_energy().any()


@pytest.mark.parametrize("scalar", [0, 1], ids=["f64", "f32"])
@pytest.mark.parametrize("skind", [2, 5], ids=["cholesky", "iterschur"])
def test_eager_trials_are_the_graph_trials(ba, O, gpu_ok, prob21, skind, scalar):
    """Three rows of ba_minimize (one captured graph per trial) against a host loop of linearize / try_step / accept that takes only the
    lambda column from the table: accepted, f (bits), and the state the run leaves (bits).  fp32: rows 0 and 1 -- row 1's f is the
    energy at the state row 0's step left, which does not depend on J -- and no state: the fused and the eager linearisation differ in
    J's bits there, so the second step and everything behind it do.  Row 0's energy is linearize's."""
    cs = _rounded(_constraints(ba, O, prob21, "p21")[0], scalar)
    g = ba.Solver(prob21, skind, scalar)
    cs.apply(g)
    r = g.minimize(max_trials=3)
    rows = r["trace"]
    h = ba.Solver(prob21, skind, scalar)
    cs.apply(h)
    e, dmax = h.linearize()
    assert rows[0, 2] == e
    sc = np.float32 if scalar == 1 else np.float64
    lam = float(sc(1e-12 * dmax))
    nrow = 3 if scalar == 0 else 2
    for t in range(nrow):
        et, rs, dn = h.try_step(lam)
        acc = et < e
        assert rows[t, 1] == (1 if acc else 0) and rows[t, 2] == e, (t, rows[t], e)
        if t == 0:
            h0 = ba.Solver(prob21, skind, scalar)
            cs.apply(h0)
            r1 = h0.minimize(max_trials=1)
            assert np.array_equal(h.get(ba.GET_DX), h0.get(ba.GET_DX)) and np.array_equal(h.get(ba.GET_CAMS_TEST), h0.get(ba.GET_CAMS_TEST))
            assert np.array_equal(h.get(ba.GET_POINTS_TEST), h0.get(ba.GET_POINTS_TEST))
        if acc:
            h.accept()
            e, _ = h.linearize(False)
        lam = rows[t, 4]
    if scalar == 0:
        if rows[-1, 1] == 1:
            assert r["energy"] == e
        assert np.array_equal(g.get(ba.GET_CAMS), h.get(ba.GET_CAMS)) and np.array_equal(g.get(ba.GET_POINTS), h.get(ba.GET_POINTS))


# ---- 5. covariance -----------------------------------------------------------------------------------------------------------------------
def test_covariance_with_constraints(ba, O, gpu_ok, prob21):
    """problem-21 at its start state, plain least squares: without a mask and without priors compute(0) is BA_ERR_SINGULAR (relative
    poses are invariant under a motion of the world: they fix no gauge); with the gauge mask and the constraints the camera blocks
    (hub-hub, a chain pair, a constrained pair without a common point, all others) against the quad S + the constraints' blocks:
    test_gpu_covariance.py's column errors, bound max(10 x numpy's inverse, 1e-16); a stale result is refused after a set call."""
    pg = prob21
    po = sorted_oracle_problem(O, pg)
    cs, info = _constraints(ba, O, pg, "p21")
    s = ba.Solver(pg, ba.CHOLESKY, ba.F64)
    s.set_loss(ba.LOSS_TRIVIAL)
    cs.apply(s)
    s.linearize()
    with pytest.raises(ba.BAError) as ei:
        s.covariance(0.0, cams=[0])
    assert ei.value.code == ba.ERR_SINGULAR
    cm = pg.gauge_mask(0)
    s.set_constant(cm, None)
    s.linearize()
    N, D = pg.N, 9 * pg.N
    a_, b_ = np.meshgrid(np.arange(N), np.arange(N), indexing="ij")
    cc, pp = s.covariance(0.0, cam_pairs=np.stack([a_.ravel(), b_.ravel()], axis=1).astype(np.int32), points=np.array([0, 7], np.int32))
    assert np.isfinite(cc).all() and np.isfinite(pp).all()
    Sig = cc.reshape(N, N, 9, 9).transpose(0, 2, 1, 3).reshape(D, D)
    Jc, Jp = s.get(ba.GET_JC).reshape(po.K, 2, 9), s.get(ba.GET_JP).reshape(po.K, 2, 3)
    fc, fp = CC.free_sets(po, cm, None)
    d = RC.direct(cs, N, s.get(ba.GET_CAMS), cm)
    S = (CC.quad_reduced(O, O.CHOLESKY, po, Jc, Jp, 0.0, fp).astype(LD) + d["S"]).astype(F64)
    ck = Checker("cov[p21]")
    eta_cpu = float(CC.column_errors(O, S, CC.inv_free(S, fc), fc).max())
    eta = CC.column_errors(O, S, Sig, fc)
    ck("eta_max(cpu %.1e)" % eta_cpu, eta.max(), max(10 * eta_cpu, 1e-16))
    # the point blocks from the formula on the refined inverse of the same S
    ref = CC.point_covariance(po, CC.mask_jacobian(po, Jc, Jp, cm, None)[0], Jp, 0.0, fp, CC.refined_inverse(S, fc), np.array([0, 7]), np.longdouble)
    cpu = CC.point_covariance(po, CC.mask_jacobian(po, Jc, Jp, cm, None)[0], Jp, 0.0, fp, CC.inv_free(S, fc), np.array([0, 7]), F64)
    e_cpu = float(CC.block_errors(cpu, ref).max())
    ck("point_blocks(cpu %.1e)" % e_cpu, CC.block_errors(pp, ref).max(), max(10 * e_cpu, 1e-15))
    cs.apply(s)
    with pytest.raises(ba.BAError) as ei:  # stale: a model set since the last linearisation
        s.covariance(0.0, cams=[0], compute=False)
    assert ei.value.code == ba.ERR_ARG
    ck.done()


# ---- 6. behaviour --------------------------------------------------------------------------------------------------------------------------
def _lm_yardstick(O, po, cs, cams0, pts0):
    """relpose_checks.lm_dense on the dense normal equations of the observation rows of loss_checks (plain least squares) and the
    constraint rows, from the start state: (the state it reaches, its energy)."""
    M, N = po.M, po.N

    def fun(x):
        cam, pts = x
        Y = LC.model(O, po, cam.astype(F64), pts.astype(F64), LC.TRIVIAL, 1.0, None)
        J = np.zeros((2 * po.K, 3 * M + 9 * N), LD)
        for k in range(po.K):
            J[2 * k:2 * k + 2, 3 * po.pt_idx[k]:3 * po.pt_idx[k] + 3] = Y["Jp"][k]
            J[2 * k:2 * k + 2, 3 * M + 9 * po.cam_idx[k]:3 * M + 9 * po.cam_idx[k] + 9] = Y["Jc"][k]
        Jr, er = RC.stacked(cs, N, cam)
        Jr = np.concatenate([np.zeros((len(er), 3 * M), LD), Jr], axis=1)
        return np.concatenate([J, Jr]), np.concatenate([Y["e"].ravel(), er])
    return RC.lm_dense(fun, (np.array(cams0, LD).reshape(-1, 15), np.array(pts0, LD).reshape(-1, 3)), lambda x, dx: PC.retract(x[0], x[1], dx), max_iter=200)


@pytest.mark.parametrize("skind", [2, 5], ids=["cholesky", "iterschur"])
def test_two_cameras_reach_the_constrained_baseline(ba, O, gpu_ok, prob21, prob39, skind):
    """Two cameras, one constraint with t0 = 2 t_ab(start), R0 = R_ab(start) and large information (1e3 x the chain's), plain least
    squares: after ba_minimize |t_ab - t0| / |t0| is below 10 x what the yardstick's own long-double LM (dense normal equations of the
    observation rows of loss_checks and the constraint rows) reaches on the same problem."""
    pg = _problem(ba, "syn2", prob21, prob39)
    po = sorted_oracle_problem(O, pg)
    cs0, _ = _constraints(ba, O, pg, "syn2")
    s = ba.Solver(pg, skind, ba.F64)
    s.set_loss(ba.LOSS_TRIVIAL)
    cams0, pts0 = s.get(ba.GET_CAMS), s.get(ba.GET_POINTS)
    Rab, tab = RC.relative_pose(cams0, 0, 1)
    cs = RC.Constraints([(0, 1)], Rab.astype(F64), 2 * tab.astype(F64), 1e3 * cs0.Lr[0], 1e3 * cs0.Lt[0])
    cs.apply(s)
    if skind == ba.ITERSCHUR:
        s.set_pcg(1000, 1e-10)
    e0, _ = s.linearize()
    r = s.minimize(max_trials=200)
    assert r["trace"][0, 2] == e0
    t1 = RC.relative_pose(s.get(ba.GET_CAMS), 0, 1)[1]
    got = float(np.sqrt(((t1 - cs.t0[0]) ** 2).sum()) / np.linalg.norm(cs.t0[0]))
    x, E = _lm_yardstick(O, po, cs, cams0, pts0)
    t2 = RC.relative_pose(x[0], 0, 1)[1]
    yard = float(np.sqrt(((t2 - cs.t0[0]) ** 2).sum()) / np.linalg.norm(cs.t0[0]))
    print("RELPOSE behaviour[%s] |t_ab - t0| / |t0| start 5.000e-01 gpu %.3e yardstick_lm %.3e energies gpu %.9g lm %.9g" % (ba.KIND_NAMES[skind], got, yard, r["energy"], float(E)))
    ck = Checker("behaviour[%s]" % ba.KIND_NAMES[skind])
    ck("baseline_misfit(yardstick %.1e)" % yard, got, 10 * yard)
    ck.done()


@pytest.mark.parametrize("angle", [0.3, 3.0], ids=["0.3rad", "3.0rad"])
def test_two_cameras_reach_the_constrained_rotation(ba, O, gpu_ok, prob21, prob39, angle):
    """Two cameras, one constraint with t0 = t_ab(start), R0 a rotation of `angle` away from R_ab(start) and stiff rotation information
    (1e3 x the chain's), plain least squares, CHOLESKY fp64: after ba_minimize |phi| = |Log(R_ab R0')| is below 10 x what the yardstick's
    own long-double LM reaches on the same problem, and below 1e-3.  The start lies above both switches of ba_relpose_eval (theta = 0.05,
    sin(theta) = 1e-3; from 3.0 rad also in the quadrant c < 0) and the end state below both; which iterates the run passes on its way
    is not read.  (The yardstick's LM, 200 plain iterations, stops at a higher energy than ba_minimize: its |phi| is a loose target.)"""
    pg = _problem(ba, "syn2", prob21, prob39)
    po = sorted_oracle_problem(O, pg)
    cs0, _ = _constraints(ba, O, pg, "syn2")
    s = ba.Solver(pg, ba.CHOLESKY, ba.F64)
    s.set_loss(ba.LOSS_TRIVIAL)
    cams0, pts0 = s.get(ba.GET_CAMS), s.get(ba.GET_POINTS)
    Rab, tab = RC.relative_pose(cams0, 0, 1)
    ax = np.random.default_rng(23).standard_normal(3)
    R0 = (PC.rodrigues(angle * ax / np.linalg.norm(ax)) @ Rab).astype(F64)
    cs = RC.Constraints([(0, 1)], R0, tab.astype(F64), 1e3 * cs0.Lr[0], cs0.Lt[0])
    cs.apply(s)
    e0, _ = s.linearize()
    r = s.minimize(max_trials=200)
    assert r["trace"][0, 2] == e0
    norm = lambda v: float(np.sqrt((v * v).sum()))
    start = norm(RC.residuals(cs, cams0)[2][0])
    got = norm(RC.residuals(cs, s.get(ba.GET_CAMS))[2][0])
    x, E = _lm_yardstick(O, po, cs, cams0, pts0)
    yard = norm(RC.residuals(cs, x[0])[2][0])
    print("RELPOSE rotation[%s] |phi| start %.3e gpu %.3e yardstick_lm %.3e energies gpu %.9g lm %.9g" % (angle, start, got, yard, r["energy"], float(E)))
    assert abs(start - angle) < 1e-9
    ck = Checker("rotation[%s]" % angle)
    ck("rotation_misfit(yardstick %.1e)" % yard, got, 10 * yard)
    ck("end_state_below_both_switches", got, 1e-3)
    ck.done()


# ---- 7. refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_solver_unchanged(ba, O, gpu_ok, prob21):
    L, _p = ba.lib(), ba._p
    cs, _ = _constraints(ba, O, prob21, "p21")
    s = ba.Solver(prob21, ba.CHOLESKY, ba.F64)
    cs.apply(s)

    def observe():
        out = [np.array(s.linearize()), s.relative_pose_energy().copy()]
        out.append(np.array(s.try_step(1e-12 * out[0][1])))
        out.append(s.get(ba.GET_DX).copy())
        return out
    before = observe()
    N = prob21.N
    pairs = np.array([[0, 1], [2, 3]], np.int32)
    R0, t0, Lm = np.tile(np.eye(3), (2, 1, 1)), np.zeros((2, 3)), np.tile(np.eye(3), (2, 1, 1))

    def bad(a, v):
        b = a.copy()
        b.reshape(-1)[-1] = v
        return b
    refl = R0.copy()
    refl[1, 2, 2] = -1.0  # det = -1
    skew_ = R0.copy()
    skew_[0, 0, 1] = 1e-5  # max |R R' - I| = 1e-5
    fn = L.ba_solver_set_relative_poses
    calls = [(2, np.array([[0, 0], [2, 3]], np.int32), R0, t0, Lm, Lm), (2, np.array([[0, N], [2, 3]], np.int32), R0, t0, Lm, Lm),
             (2, np.array([[-1, 0], [2, 3]], np.int32), R0, t0, Lm, Lm), (2, np.array([[0, 1], [1, 0]], np.int32), R0, t0, Lm, Lm),
             (2, np.array([[0, 1], [0, 1]], np.int32), R0, t0, Lm, Lm), (2, pairs, bad(R0, np.nan), t0, Lm, Lm), (2, pairs, R0, bad(t0, np.inf), Lm, Lm),
             (2, pairs, R0, t0, bad(Lm, np.nan), Lm), (2, pairs, R0, t0, Lm, bad(Lm, np.inf)), (2, pairs, refl, t0, Lm, Lm),
             (2, pairs, skew_, t0, Lm, Lm), (2, pairs, 0 * R0, t0, Lm, Lm), (-1, pairs, R0, t0, Lm, Lm), (2, None, R0, t0, Lm, Lm),
             (2, pairs, None, t0, Lm, Lm), (2, pairs, R0, None, Lm, Lm), (2, pairs, R0, t0, None, Lm), (2, pairs, R0, t0, Lm, None)]
    for k, (n, p, r_, t_, lr, lt) in enumerate(calls):
        assert fn(s._h, n, _p(p), _p(r_), _p(t_), _p(lr), _p(lt)) == ba.ERR_ARG, k
    # (a refused call is no change: try_step is still allowed, nothing is stale)
    assert np.array_equal(np.array(s.try_step(1e-12 * before[0][1])), before[2])
    for k, (x, y) in enumerate(zip(before, observe())):
        assert np.array_equal(x, y), k
    # a value that is finite as a double and not as a float
    q = ba.Solver(prob21, ba.CHOLESKY, ba.F32)
    assert fn(q._h, 2, _p(pairs), _p(R0), _p(bad(t0, 1e39)), _p(Lm), _p(Lm)) == ba.ERR_ARG
    assert fn(q._h, 2, _p(pairs), _p(R0), _p(t0), _p(Lm), _p(Lm)) == 0
    # another kind, a sharded solver
    out2 = np.empty(2)
    for kind in (ba.QRKIT, ba.QRCHOL, ba.MOREQR, ba.QRSPQR):
        q = ba.Solver(prob21, kind, ba.F64)
        assert fn(q._h, 2, _p(pairs), _p(R0), _p(t0), _p(Lm), _p(Lm)) == ba.ERR_ARG, kind
        q.linearize()
        assert L.ba_solver_relative_pose_energy(q._h, _p(out2)) == ba.ERR_ARG
    q = ba.Solver(prob21, ba.CHOLESKY, ba.F64, shard_rank=0, shard_world=2)
    assert fn(q._h, 2, _p(pairs), _p(R0), _p(t0), _p(Lm), _p(Lm)) == ba.ERR_ARG
    q = ba.Solver(prob21, ba.ITERSCHUR, ba.F32)
    assert L.ba_solver_relative_pose_energy(q._h, _p(out2)) == ba.ERR_ARG  # no linearisation yet
    q.linearize()
    assert L.ba_solver_relative_pose_energy(q._h, _p(out2)) == 0 and not out2.any()  # (no constraints: zeros)
    # a set call: try_step and the energy wait for the next linearisation
    cs.apply(s)
    e, r_, n_ = C.c_double(), C.c_double(), C.c_double()
    assert L.ba_solver_try_step(s._h, 1.0, C.byref(e), C.byref(r_), C.byref(n_)) == ba.ERR_ARG
    assert L.ba_solver_relative_pose_energy(s._h, _p(out2)) == ba.ERR_ARG
    s.linearize()
    # device_bytes counts the lists; the binding's sigma form is diag(1 / sigma)
    b1 = s.device_bytes()
    RC.Constraints().apply(s)
    assert s.device_bytes() < b1
    a, b = ba.Solver(prob21, ba.CHOLESKY, ba.F64), ba.Solver(prob21, ba.CHOLESKY, ba.F64)
    a.set_relative_poses(cs.pairs, cs.R0, cs.t0, sigma_rot=0.01, sigma_trans=np.tile([0.1, 0.2, 0.4], (len(cs), 1)))
    b.set_relative_poses(cs.pairs, cs.R0, cs.t0, sqrt_info_rot=np.tile(np.eye(3) / 0.01, (len(cs), 1, 1)),
                         sqrt_info_trans=np.tile(np.diag([10.0, 5.0, 2.5]), (len(cs), 1, 1)))
    assert a.linearize() == b.linearize() and np.array_equal(a.relative_pose_energy(), b.relative_pose_energy()) and a.relative_pose_energy().all()
    with pytest.raises(ValueError):
        a.set_relative_poses(cs.pairs, cs.R0, cs.t0, sigma_rot=0.01, sqrt_info_rot=cs.Lr)
