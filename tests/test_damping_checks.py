"""tests/damping_checks.py on the CPU: the long double restatement of one trial under Marquardt's damping (ba_solver_set_damping), on
the oracle's linearisation of problem-21 and of a small synthetic problem.  It pins the reference tests/test_gpu_damping.py measures
the kernels against, and the property that defines the feature: with lambda diag(J'J) the step does not depend on the units of any
parameter, with lambda I it does.  No GPU needed."""
import numpy as np
import pytest

import damping_checks as DC
import shared_checks as SH
import stage_checks as SC
from conftest import DATA21

LD = np.longdouble
EPS_LD = float(np.finfo(LD).eps)
LAM = 1e-3
OPEN = dict(dmin=1e-300, dmax=1e300)  # clamps that never bite


def _lin(O, p):
    cam = O.init_cams(p)
    f, e = O.residuals(p, cam, p.pts)
    Jc, Jp = O.jacobian(p, cam, p.pts)
    return np.asarray(f).reshape(p.K, 2), np.asarray(Jc).reshape(p.K, 2, 9), np.asarray(Jp).reshape(p.K, 2, 3)


@pytest.fixture(scope="module")
def sub21(O):
    """The first 40 points of problem-21 with all 21 cameras: 3 M + 9 N = 309 unknowns, small enough for the whole J'J."""
    p = O.load_bal(DATA21).subset(40)
    return (p,) + _lin(O, p)


@pytest.fixture(scope="module")
def big21(O):
    """The first 2500 points of problem-21."""
    p = O.load_bal(DATA21).subset(2500)
    return (p,) + _lin(O, p)


@pytest.fixture(scope="module")
def syn(ba, O):
    """synthetic(4, 30, 100): 126 unknowns."""
    pg = ba.Problem.synthetic(4, 30, 100, 7)
    a = pg.arrays()
    order = np.argsort(a["pt_idx"], kind="stable")
    p = O.Problem(pg.N, pg.M, pg.K, a["cam_idx"][order], a["pt_idx"][order], a["meas"].reshape(-1, 2)[order].ravel(), a["cams9"], a["pts"])
    return (p,) + _lin(O, p)


def _scaled_cond(H):
    d = 1 / np.sqrt(np.diagonal(H).astype(np.float64))
    return float(np.linalg.cond(H.astype(np.float64) * d[:, None] * d[None, :]))


def test_identity_damping_is_the_quad_assembly(O, big21):
    """kind 0 of the same code against the quad assembly of oracle/ (referee_reduced_from_jacobian) on 2500 points of problem-21, also at
    lambda = 1e-6, where a distant point's depth is held by lambda alone and its block has a condition number of 1e13: S and rhs in
    stage_checks' scaled metric.  Bound 2^-52: the referee hands its S out in doubles and this one is rounded to doubles for the
    comparison; long double's own 2^-64 per operation is far below that because the elimination goes through L D L' and never inverts
    a block (inverting it loses 2^-64 x its condition number: 6e-9 was measured that way)."""
    p, f, Jc, Jp = big21
    for lam in (1e-6, 1e-2, 1.0):
        t = DC.trial(p, Jc, Jp, f, lam, kind=DC.IDENTITY, want_step=False)
        R = O.referee_reduced_from_jacobian(O.CHOLESKY, p, Jc, Jp, f.ravel(), lam)
        err = SC.assembly_errors(p, Jc, f.ravel(), lam, t["S"].astype(np.float64), t["rhs"].astype(np.float64), R["S"], R["rhs"], Jp)
        print("identity vs quad, lambda %g: %s" % (lam, err))
        assert err["S"] <= 2.0 ** -52 and err["rhs"] <= 2.0 ** -52, err


@pytest.mark.parametrize("which", ["sub21", "syn"])
@pytest.mark.parametrize("kind", [DC.MARQUARDT, DC.IDENTITY])
def test_eliminated_solution_is_the_dense_solution(request, which, kind):
    """dx of the point elimination (S, rhs, back-substitution) equals the solve of the whole (J'J + lambda D) dx = g.  Bound: both are
    long double solves refined to the rounding of their residuals, so each is within about 2^-64 cond of the exact step, cond that of
    the symmetrically scaled matrix; 100 x that for the two together and the sums in between."""
    p, f, Jc, Jp = request.getfixturevalue(which)
    t = DC.trial(p, Jc, Jp, f, LAM, kind=kind)
    H, g, d = DC.dense_system(p, Jc, Jp, f, LAM, kind=kind)
    x = DC.solve(H, g)
    bound = 100 * EPS_LD * _scaled_cond(H)
    err = DC.step_difference(t["dx"], x)
    print("eliminated vs dense (%s, kind %d): %.2e, bound %.2e" % (which, kind, err, bound))
    assert err <= bound, (err, bound)
    assert np.array_equal(d[:3 * p.M], t["d_p"]) or DC.step_difference(t["d_p"], d[:3 * p.M]) <= 4 * EPS_LD
    rs = DC.rho_scale(x, d, g)
    assert abs(float((t["rho_scale"] - rs) / rs)) <= bound


@pytest.mark.parametrize("which", ["sub21", "syn"])
def test_step_is_invariant_under_column_scaling(request, which):
    """The property that defines the feature.  J C for an arbitrary positive diagonal C (each entry log-uniform in [1e-3, 1e3]) is the
    same problem in other units; with the clamps inactive (J C)'(J C) + lambda diag((J C)'(J C)) = C (J'J + lambda D) C, so the step is
    C^-1 times the step of J.  Bound: the long double roundoff of the two solves, 100 x 2^-63 x the condition number of the scaled
    matrix (the same for both: Jacobi scaling removes C).  With lambda I the same comparison misses by orders of magnitude."""
    p, f, Jc, Jp = request.getfixturevalue(which)
    rng = np.random.default_rng(3)
    cp, cc = 10.0 ** rng.uniform(-3, 3, 3 * p.M), 10.0 ** rng.uniform(-3, 3, 9 * p.N)
    Jcs, Jps = DC.scale_columns(p, Jc, Jp, cp, cc)
    c = np.concatenate([cp, cc]).astype(LD)
    H, _, _ = DC.dense_system(p, Jc, Jp, f, LAM, **OPEN)
    bound = 100 * EPS_LD * _scaled_cond(H)
    a = DC.trial(p, Jc, Jp, f, LAM, **OPEN)
    b = DC.trial(p, Jcs, Jps, f, LAM, **OPEN)
    err = DC.step_difference(b["dx"] * c, a["dx"])
    print("Marquardt, scaled columns (%s): %.2e, bound %.2e" % (which, err, bound))
    assert err <= bound, (err, bound)
    assert abs(float((b["rho_scale"] - a["rho_scale"]) / a["rho_scale"])) <= bound  # (the model decrease has no units)
    ai = DC.trial(p, Jc, Jp, f, LAM, kind=DC.IDENTITY)
    bi = DC.trial(p, Jcs, Jps, f, LAM, kind=DC.IDENTITY)
    miss = DC.step_difference(bi["dx"] * c, ai["dx"])
    print("identity, scaled columns (%s): %.2e" % (which, miss))
    assert miss >= 1e-3 and miss >= 1e6 * bound, (miss, bound)


def test_clamps_and_fixed_parameters(sub21):
    """A column with diagonal below diag_min is damped by lambda diag_min, one above diag_max by lambda diag_max, the others by
    lambda diag; a fixed parameter (zero column) has d = lambda diag_min, a row of S that is lambda diag_min alone and a step of exactly 0,
    and a fixed point the same.  The step is the dense solve of J'J + diag(d) with that d written out by hand."""
    p, f, Jc, Jp = sub21
    Jc, Jp = Jc.copy(), Jp.copy()
    fixed_cam_cols = [(0, q) for q in range(6)] + [(5, 7)]  # the pose of camera 0, k1 of camera 5
    for a, q in fixed_cam_cols:
        Jc[p.cam_idx == a, :, q] = 0
    fixed_pts = [3, 17]
    for j in fixed_pts:
        Jp[p.pt_idx == j] = 0
    free = DC.trial(p, Jc, Jp, f, LAM, **OPEN, want_step=False)
    diag = np.concatenate([free["diag_p"], free["diag_c"]]).astype(np.float64)
    pos = np.sort(diag[diag > 0])
    dmin, dmax = float(np.sqrt(pos[len(pos) // 5] * pos[len(pos) // 5 + 1])), float(np.sqrt(pos[-len(pos) // 5 - 1] * pos[-len(pos) // 5]))
    low, high = diag < dmin, diag > dmax
    assert low.sum() > len(fixed_cam_cols) + 3 * len(fixed_pts) and high.sum() > 0 and (~low & ~high).sum() > 0  # both clamps bite
    t = DC.trial(p, Jc, Jp, f, LAM, dmin=dmin, dmax=dmax)
    d = np.concatenate([t["d_p"], t["d_c"]])
    want = np.where(low, LD(LAM) * LD(dmin), np.where(high, LD(LAM) * LD(dmax), LD(LAM) * np.concatenate([free["diag_p"], free["diag_c"]])))
    assert np.array_equal(d, want)
    H, g, _ = DC.dense_system(p, Jc, Jp, f, 0.0, kind=DC.IDENTITY)
    H = H + np.diag(want)
    x = DC.solve(H, g)
    bound = 100 * EPS_LD * _scaled_cond(H)
    assert DC.step_difference(t["dx"], x) <= bound
    for a, q in fixed_cam_cols:
        i = 9 * a + q
        row = t["S"][i].copy()
        assert row[i] == LD(LAM) * LD(dmin) and t["rhs"][i] == 0 and t["dx_c"][i] == 0
        row[i] = 0
        assert not row.any() and not t["S"][:, i][np.arange(p.D) != i].any()
    for j in fixed_pts:
        assert not t["dx_p"][3 * j:3 * j + 3].any() and np.all(t["d_p"][3 * j:3 * j + 3] == LD(LAM) * LD(dmin))


def test_shared_parameter_is_damped_by_the_sum_over_its_group(sub21):
    """With one group of all cameras the step is P y of (P'SP) y = P' rhs, and the damping inside P'SP on the group's parameter q is
    lambda sum_a D_a,q: the reduced matrix of S minus that of S without its camera damping is diagonal, lambda D on an ungrouped row
    and the members' sum on a shared one.  The step's rows 6..8 are bit-equal over the cameras."""
    p, f, Jc, Jp = sub21
    groups = [np.arange(p.N)]
    t = DC.trial(p, Jc, Jp, f, LAM, groups=groups)
    A, c, rep, cols = SH.reduced_system(t["S"], t["rhs"], groups)
    A0, _, _, _ = SH.reduced_system(t["S"] - np.diag(t["d_c"]), t["rhs"], groups)
    dA = A - A0
    dd = np.zeros(p.D, LD)
    np.add.at(dd, rep, t["d_c"])  # lambda P'D P: the members' dampings summed into the representative's row
    scale = np.abs(np.diagonal(A))
    assert np.all(np.abs(np.diagonal(dA) - dd[cols]) <= 8 * EPS_LD * scale)
    off = dA - np.diag(np.diagonal(dA))
    assert np.all(np.abs(off) <= 8 * EPS_LD * np.sqrt(scale[:, None] * scale[None, :]))
    q = np.searchsorted(cols, 6)  # f of the group
    assert abs(float(dd[6] / (LD(LAM) * DC.clamp(t["diag_c"]).reshape(p.N, 9)[:, 6].sum()) - 1)) <= 8 * EPS_LD and dd[cols][q] == dd[6]
    x = t["dx_c"].reshape(p.N, 9)
    assert np.all(x[:, 6:9] == x[0, 6:9])
    y = t["dx_c"][cols]
    r = c - A @ y
    assert float(np.sqrt((r * r).sum() / (c * c).sum())) <= 100 * EPS_LD * _scaled_cond(A)
