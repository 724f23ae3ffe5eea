"""The stage metrics of tests/stage_checks.py on the CPU oracle alone: near zero on consistent data, and at least 100x that on data
with one planted defect of the kind a subtly wrong kernel would leave -- which is what lets tests/test_gpu_stages.py claim that it
would notice one.  No GPU needed."""
import numpy as np
import pytest

import stage_checks as SC
from conftest import DATA21

LAMS = (1e-6, 1.0)


@pytest.fixture(scope="module")
def p21(O):
    return O.load_bal(DATA21)


@pytest.fixture(scope="module")
def sub21(p21):
    """The first 2500 points of problem-21 (all 21 cameras): the quad assembly in well under a second."""
    return p21.subset(2500)


def _lin(O, p):
    cam = O.init_cams(p)
    f, e = O.residuals(p, cam, p.pts)
    Jc, Jp = O.jacobian(p, cam, p.pts)
    return cam, f, e, Jc, Jp


def _weakest_pair(S, N):
    """(a, b), a > b: the camera pair whose off-diagonal 9 x 9 block of S is the smallest non-zero one."""
    best, ab = np.inf, None
    for a in range(N):
        for b in range(a):
            m = np.abs(S[9 * a:9 * a + 9, 9 * b:9 * b + 9]).max()
            if 0 < m < best:
                best, ab = m, (a, b)
    return ab


def _drop_pair(S, a, b):
    S = S.copy()
    S[9 * a:9 * a + 9, 9 * b:9 * b + 9] = 0
    S[9 * b:9 * b + 9, 9 * a:9 * a + 9] = 0
    return S


@pytest.mark.parametrize("lam", LAMS)
def test_eta_of_ldlt_solves_and_of_solves_of_the_wrong_matrix(O, p21, lam):
    """eta of the oracle's unpivoted fp64 LDL^T solve of problem-21's S is at the unit roundoff; solving exactly (LAPACK) a matrix
    that differs from S in one diagonal entry by 1e-6 relative -- the last camera's focal length -- or by one missing camera-pair
    block raises it by far more than 100x, although the step moves by only ~1e-7 relative (the fp64 step tolerance of the
    whole-pipeline tests is 1e-6)."""
    cam, f, e, Jc, Jp = _lin(O, p21)
    st = O.step(O.CHOLESKY, p21, Jc, Jp, f, lam)
    S, rhs, dxc = st["S"], st["rhs"], st["dx"][3 * p21.M:]
    ok = SC.eta(S, dxc, rhs)
    assert ok <= 1e-15, ok
    base = max(ok, SC.eta(S, np.linalg.solve(S, rhs), rhs))
    i = p21.D - 3  # the last camera's f
    Sd = S.copy()
    Sd[i, i] *= 1 + 1e-6
    bad = SC.eta(S, np.linalg.solve(Sd, rhs), rhs)
    assert bad >= 100 * base, (bad, base)
    a, b = _weakest_pair(S, p21.N)
    bad2 = SC.eta(S, np.linalg.solve(_drop_pair(S, a, b), rhs), rhs)
    assert bad2 >= 100 * base, (bad2, base)
    # a NaN step fails every bound
    assert np.isnan(SC.eta(S, np.where(np.arange(p21.D) == 5, np.nan, dxc), rhs))
    # the metric reads the lower triangle only: a defect in the upper one is invisible to it, as to the kernels
    Su = S.copy()
    Su[0, p21.D - 1] += 1.0
    assert SC.eta(Su, dxc, rhs) == ok


def _ldlt_solve(S, b):
    """Unpivoted LDL^T solve in the dtype of S (right-looking, column by column) -- the arithmetic of the GPU's dense factor."""
    A = S.copy()
    n = A.shape[0]
    for k in range(n):
        A[k + 1:, k] /= A[k, k]
        A[k + 1:, k + 1:] -= np.outer(A[k + 1:, k], A[k + 1:, k]) * A[k, k]
    x = b.copy()
    for k in range(n):
        x[k + 1:] -= A[k + 1:, k] * x[k]
    x /= np.diag(A)
    for k in range(n - 1, -1, -1):
        x[:k] -= A[k, :k] * x[k]
    return x


def test_eta_of_an_fp32_ldlt_solve(O, p21):
    """An unpivoted LDL^T solve in fp32 of problem-21's S and rhs (the fp64 oracle's, rounded to fp32) has eta at the fp32 unit
    roundoff -- far below the 1e-5 ceiling of the fp32 GPU tests -- also at small lambda, where some of its pivots come out negative.
    (The fp32 oracle itself cannot serve here: its fp32 point elimination breaks down on problem-21 to NaN.)"""
    cam, f, e, Jc, Jp = _lin(O, p21)
    for lam in (1e-6, 1e-3, 10.0):
        st = O.step(O.CHOLESKY, p21, Jc, Jp, f, lam)
        S32, b32 = st["S"].astype(np.float32), st["rhs"].astype(np.float32)
        x = _ldlt_solve(S32, b32)
        v = SC.eta(S32.astype(np.float64), x.astype(np.float64), b32.astype(np.float64))
        assert v <= 1e-6, (lam, v)


def test_reduced_from_jacobian_is_ref_reduced(O, sub21):
    """ref_reduced_from_jacobian fed the quad J and residuals (rounded to double) is ref_reduced, which linearises itself in quad: the
    same S and rhs up to the rounding of J (measured 1.3e-16 in the assembly metric), and the same step up to that rounding times
    the conditioning of the trial (measured 5e-13)."""
    p = sub21
    cam = O.init_cams(p)
    L = O.referee_linearize(p, cam, p.pts)
    for kind in (O.CHOLESKY, O.QRCHOL):
        S0, r0 = O.referee_reduced(kind, p, cam, p.pts, 1e-3)
        R = O.referee_reduced_from_jacobian(kind, p, L["Jc"], L["Jp"], L["f"], 1e-3)
        err = SC.assembly_errors(p, L["Jc"], L["f"], 1e-3, R["S"], R["rhs"], S0, r0, L["Jp"])
        assert err["S"] < 1e-15 and err["rhs"] < 1e-15, (kind, err)
    R = O.referee_reduced_from_jacobian(O.CHOLESKY, p, L["Jc"], L["Jp"], L["f"], 1e-3, want_S=False, want_dx=True)
    tr = O.referee_trial(O.CHOLESKY, p, cam, p.pts, 1e-3, want_dx=True)
    assert np.abs(R["dx"] - tr["dx"]).max() < 1e-10 * np.abs(tr["dx"]).max()


@pytest.mark.parametrize("kind", [2, 1])
def test_assembly_metric(O, sub21, kind):
    """The fp64 oracle's S and rhs against quad on the same fp64 J: a small scaled error (it grows as lambda shrinks, through the
    3 x 3 point blocks); one diagonal entry x (1 + 1e-6) or one dropped camera-pair block: at least 100x that."""
    p = sub21
    cam, f, e, Jc, Jp = _lin(O, p)
    for lam in LAMS:
        st = O.step(kind, p, Jc, Jp, f, lam)
        R = O.referee_reduced_from_jacobian(kind, p, Jc, Jp, f, lam)
        ok = SC.assembly_errors(p, Jc, f, lam, st["S"], st["rhs"], R["S"], R["rhs"], Jp)
        assert ok["S"] < 1e-10 and ok["rhs"] < 1e-10, ok
        S1 = st["S"].copy()
        S1[p.D - 3, p.D - 3] *= 1 + 1e-6
        bad = SC.assembly_errors(p, Jc, f, lam, S1, st["rhs"], R["S"], R["rhs"], Jp)
        assert bad["S"] >= 100 * ok["S"], (bad, ok)
        a, b = _weakest_pair(st["S"], p.N)
        bad = SC.assembly_errors(p, Jc, f, lam, _drop_pair(st["S"], a, b), st["rhs"], R["S"], R["rhs"], Jp)
        assert bad["S"] >= 100 * ok["S"], (bad, ok, (a, b))
        r1 = st["rhs"].copy()
        r1[p.D - 3] += 1e-6 * abs(r1[p.D - 3])
        bad = SC.assembly_errors(p, Jc, f, lam, None, r1, None, R["rhs"], Jp)
        assert bad["rhs"] >= 100 * ok["rhs"], (bad, ok)


@pytest.mark.parametrize("kind", [2, 1, 3])
def test_backsub_metric(O, sub21, kind):
    """The point steps of the oracle's fp64 trial satisfy their rows of the normal equations to the unit roundoff; one point's step
    off by 1e-6 relative -- the point with the largest step -- shows at least 100x that."""
    p = sub21
    cam, f, e, Jc, Jp = _lin(O, p)
    for lam in LAMS:
        st = O.step(kind, p, Jc, Jp, f, lam)
        ok = SC.backsub_errors(p, Jc, Jp, st["dx"], st["g"], lam)
        assert ok < 1e-13, (lam, ok)
        dx = st["dx"].copy()
        j = int(np.argmax(np.abs(dx[: 3 * p.M]).reshape(p.M, 3).max(axis=1)))
        dx[3 * j: 3 * j + 3] *= 1 + 1e-6
        bad = SC.backsub_errors(p, Jc, Jp, dx, st["g"], lam)
        assert bad >= 100 * ok, (lam, bad, ok)


def test_linearization_and_retraction_metrics(O, sub21):
    """The fp64 oracle's linearisation, trial point and trial scalars against quad at the same inputs: at the level of fp64
    rounding; a retraction entry off by 1e-12 relative, a Jacobian entry or a gradient entry off by 1e-9
    relative: at least 100x that."""
    p = sub21
    cam, f, e, Jc, Jp = _lin(O, p)
    lam = 1e-3
    st = O.step(O.CHOLESKY, p, Jc, Jp, f, lam)
    ref = SC.quad_linearization(p, cam, p.pts)
    lin = SC.linearization_errors(p, cam, p.pts, f, Jc, Jp, e, ref=ref)
    # (measured 1.9e-16 for the Jacobian: per entry, against its own sensitivity -- 4.4e-12 of the block's largest entry, whose
    # formulas cancel)
    assert lin["res"] < 1e-13 and lin["jac"] < 1e-14 and lin["energy"] < 1e-13, lin
    gr = SC.grad_errors(p, Jc, Jp, f, st["g"])
    assert gr < 1e-13, gr
    for k, r, c in ((0, 1, 6), (p.K // 2, 0, 3), (p.K - 1, 1, 8)):  # a focal-length, a rotation, a distortion entry
        Jb = Jc.copy()
        Jb[k, r, c] *= 1 + 1e-9
        assert SC.linearization_errors(p, cam, p.pts, f, Jb, Jp, ref=ref)["jac"] >= 100 * lin["jac"], (k, r, c)
    gb = st["g"].copy()
    gb[3 * p.M + 9 * (p.N - 1) + 6] *= 1 + 1e-9
    assert SC.grad_errors(p, Jc, Jp, f, gb) >= 100 * gr
    co, po = O.retract(p, cam, p.pts, st["dx"])
    ok = SC.retraction_ulps(p, cam, p.pts, st["dx"], co, po, np.finfo(np.float64).eps)
    assert ok <= 4, ok
    for idx in (15 * (p.N - 1) + 4, 15 * (p.N - 1) + 12):  # a rotation entry, the focal length
        c1 = co.copy()
        c1[idx] *= 1 + 1e-12
        bad = SC.retraction_ulps(p, cam, p.pts, st["dx"], c1, po, np.finfo(np.float64).eps)
        assert bad >= 100 * max(ok, 1.0), (idx, bad, ok)
    _, et = O.residuals(p, co, po)
    rs = float(st["dx"] @ (lam * st["dx"] + st["g"]))
    sc = SC.trial_scalar_errors(p, lam, st["dx"], st["g"], et, rs, np.linalg.norm(st["dx"]), co, po)
    assert sc["e_test"] < 1e-13 and sc["rho_scale"] < 1e-14 and sc["dx_norm"] < 1e-14, sc


# ---- dense QR (ba_qr.hip.h): R, Q^T b and the back substitution on their own inputs ------------------------------------------------
def _qr_problem(m, D, seed, grade=0.0):
    """[D + 1 columns, m + 3 rows] (three padding rows, as the kernels' matrices have): Gaussian columns, scaled by 10^U(-grade, grade)."""
    rng = np.random.default_rng(seed)
    Ab = np.zeros((D + 1, m + 3))
    Ab[:, :m] = rng.standard_normal((D + 1, m)) * 10.0 ** rng.uniform(-grade, grade, (D + 1, 1))
    return Ab


def _factored(R_aug, shape, dtype=np.float64):
    """F as the kernels leave it, from R of [A | b]: R on and above the diagonal of the first D rows, Q^T b = (c, rho, 0, ...)."""
    F = np.zeros(shape, dtype)
    n = R_aug.shape[0]
    for c in range(n):
        F[c, : c + 1] = R_aug[: c + 1, c]
    return F


def _backsolve(F, D):
    R = F[:D, :D].T
    c = F[D, :D]
    y = np.zeros(D, F.dtype)
    for i in range(D - 1, -1, -1):
        y[i] = (c[i] - R[i, i + 1:] @ y[i + 1:]) / R[i, i]
    return y


def _householder(Ab, m, D, bad_tau=None, skip_rhs=None):
    """Householder QR of [A | b] column by column (LAPACK's dlarfg convention) in fp64, with one planted defect: bad_tau = (j, s):
    reflector j's tau times s (no longer orthogonal); skip_rhs = j: reflector j not applied to the right-hand side."""
    X = Ab[:, :m].T.copy()
    for j in range(D):
        x = X[j:, j]
        alpha, nx = x[0], np.linalg.norm(x[1:])
        if nx == 0:
            continue
        beta = -np.copysign(np.hypot(alpha, nx), alpha)
        v = x / (alpha - beta)
        v[0] = 1.0
        tau = (beta - alpha) / beta
        if bad_tau is not None and bad_tau[0] == j:
            tau *= bad_tau[1]
        hi = D if skip_rhs == j else D + 1
        X[j:, j + 1: hi] -= tau * np.outer(v, v @ X[j:, j + 1: hi])
        X[j, j], X[j + 1:, j] = beta, 0.0
    F = np.zeros_like(Ab)
    F[:, :m] = X.T
    for c in range(D):
        F[c, c + 1:] = 0.0
    return F


@pytest.mark.parametrize("grade", [0.0, 8.0])
def test_dense_qr_metrics(grade):
    """The dense-QR metrics on an fp64 QR of [A | b] by numpy.linalg.qr (LAPACK): each at the unit roundoff, whatever the column scales
    (grade 8: columns over 1e-8 ... 1e8, the spread of J2bot); an fp32 QR at the fp32 unit roundoff; the probe form of gram likewise.
    Planted defects, each at least 100x the clean value of its metric: one R entry off by 1e-10 relative (gram, full and probe),
    a reflector whose tau is off by 1e-8 relative (orth: no longer orthogonal), one reflector's update of the right-hand side
    dropped (qtb_head), one back-substitution entry off by 1e-10 relative (tri).  A NaN fails every bound."""
    m, D = 700, 45
    Ab = _qr_problem(m, D, 7, grade)
    R_aug = np.linalg.qr(Ab[:, :m].T, mode="r")
    F = _factored(R_aug, Ab.shape)
    y = _backsolve(F, D)
    ok = SC.qr_metrics(Ab, F, m, D, y)
    ok.update({"gram_probe": SC.qr_metrics(Ab, F, m, D, probes=4)["gram"]})
    print(ok)
    assert all(v < 2e-15 for v in ok.values()), ok
    # fp32: numpy's QR in float32 of the same matrix rounded to float32
    A32 = Ab.astype(np.float32)
    F32 = _factored(np.linalg.qr(A32[:, :m].T, mode="r"), Ab.shape, np.float32)
    ok32 = SC.qr_metrics(A32.astype(np.float64), F32.astype(np.float64), m, D, _backsolve(F32, D).astype(np.float64))
    assert all(v < 2e-6 for v in ok32.values()), ok32
    # the defects, against the clean value of a hand-made Householder QR (same convention as the kernels)
    H = _householder(Ab, m, D)
    base = SC.qr_metrics(Ab, H, m, D, _backsolve(H, D))
    base["gram_probe"] = SC.qr_metrics(Ab, H, m, D, probes=4)["gram"]
    assert all(v < 2e-15 for v in base.values()), base
    floor = {k: max(v, ok[k], 1e-17) for k, v in base.items()}
    Fb = H.copy()
    Fb[D - 3, 5] *= 1 + 1e-10  # R_{5, D-3}
    assert SC.qr_metrics(Ab, Fb, m, D)["gram"] >= 100 * floor["gram"]
    assert SC.qr_metrics(Ab, Fb, m, D, probes=4)["gram"] >= 100 * floor["gram_probe"]
    bad = SC.qr_metrics(Ab, _householder(Ab, m, D, bad_tau=(D // 2, 1 + 1e-8)), m, D)
    assert bad["orth"] >= 100 * floor["orth"], (bad, floor)
    bad = SC.qr_metrics(Ab, _householder(Ab, m, D, skip_rhs=D // 3), m, D)
    assert bad["qtb_head"] >= 100 * floor["qtb_head"], (bad, floor)
    yb = _backsolve(H, D)
    yb[D // 2] *= 1 + 1e-10
    assert SC.qr_metrics(Ab, H, m, D, yb)["tri"] >= 100 * floor["tri"]
    # a NaN anywhere in what the kernels return fails every bound
    for where in ("R", "c", "tail", "y"):
        Fn, yn = H.copy(), _backsolve(H, D)
        if where == "R":
            Fn[D - 1, 3] = np.nan
        elif where == "c":
            Fn[D, 2] = np.nan
        elif where == "tail":
            Fn[D, m - 1] = np.nan
        else:
            yn[0] = np.nan
        v = SC.qr_metrics(Ab, Fn, m, D, yn)
        assert {"R": np.isnan(v["gram"]) and np.isnan(v["tri"]), "c": np.isnan(v["qtb_head"]) and np.isnan(v["orth"]),
                "tail": np.isnan(v["orth"]), "y": np.isnan(v["tri"])}[where], (where, v)
        if where == "R":
            assert np.isnan(SC.qr_metrics(Ab, Fn, m, D, probes=2)["gram"])
