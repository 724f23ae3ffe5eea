"""The iterate metric of tests/pcg_checks.py on the CPU oracle's S alone: the fp64 yardstick PCG sits at rounding level against the
long double one at every checked k, and each planted defect of the kind a subtly wrong PCG kernel would leave raises the metric at
some checked k by at least 100x -- which is what lets tests/test_gpu_pcg_stages.py claim that it would notice one.  Likewise for the
iteration count: with the diagonal-only preconditioner the reference needs more iterations than that file's bound can ever allow.
No GPU needed."""
import numpy as np
import pytest

import pcg_checks as PC
from conftest import DATA21

KS = (1, 2, 3, 4, 7)
LAMS = (1e-6, 1e-2)  # x max diag J'J, as in tests/test_gpu_pcg_stages.py


def _system(O, p, x):
    cam = O.init_cams(p)
    f, e = O.residuals(p, cam, p.pts)
    Jc, Jp = O.jacobian(p, cam, p.pts)
    dmax = O.step(O.CHOLESKY | O.ASSEMBLE_ONLY, p, Jc, Jp, f, 1.0, want_S=False)["diagmax"]
    lam = x * dmax
    R = O.referee_reduced_from_jacobian(O.CHOLESKY, p, Jc, Jp, f, lam)
    B = PC.documented_blocks(p, Jc, Jp, lam, R["S"])
    Minv, ok = PC.invert_blocks(B)
    assert ok.all()
    return dict(p=p, S=R["S"], rhs=R["rhs"], B=B, Minv=Minv, lam=lam, Jc=Jc, Jp=Jp)


@pytest.fixture(scope="module")
def systems(O):
    """problem-21 and a small synthetic problem (9 cameras, 260 points) at both lambdas."""
    from conftest import to_oracle
    import bundleadjustment_benchmarks_amd as ba
    p21 = O.load_bal(DATA21)
    syn = to_oracle(ba.Problem.synthetic(9, 260, 900, 31))
    return {(n, x): _system(O, p, x) for n, p in (("p21", p21), ("syn9", syn)) for x in LAMS}


def _errors(sy, ref, **kw):
    Minv = kw.pop("Minv", sy["Minv"])
    out = PC.pcg(sy["S"], sy["rhs"], Minv, max(KS), keep=KS, **kw)
    return np.array([PC.iterate_error(out["xs"][k], ref["xs"][k], sy["S"]) for k in KS])


def _weakest_pair(S, N):
    """(a, b), a > b: the camera pair whose off-diagonal 9 x 9 block of S is the smallest non-zero one."""
    best, ab = np.inf, None
    for a in range(N):
        for b in range(a):
            m = np.abs(S[9 * a:9 * a + 9, 9 * b:9 * b + 9]).max()
            if 0 < m < best:
                best, ab = m, (a, b)
    return ab


@pytest.mark.parametrize("x", LAMS)
@pytest.mark.parametrize("name", ["p21", "syn9"])
def test_iterate_metric_has_teeth(systems, name, x):
    """The fp64 yardstick at rounding level (<= 1e-12; fp32: <= 1e-3) for k = 1, 2, 3, 4, 7, and every planted defect at least 100x the
    fp64 yardstick at some checked k:
      the diagonal-only inverse for one camera (k_pcg_prec_inv's own fallback), for the first, a middle and the last camera;
      the weakest camera pair's off-diagonal block missing from the product S p;
      beta = 0; beta's denominator from the slot one iteration stale;
      one block of partials left out of r'z (the sum split as gc = 2 would split it, the second block -- the last camera -- dropped).
    The beta defects cannot show before x_2 / x_3 (beta_0 = 0, and the stale slot is first read at k = 2): the factor is asked of
    the worst checked k, and which k that was is printed."""
    sy = systems[(name, x)]
    N = sy["p"].N
    ref = PC.pcg(sy["S"], sy["rhs"], sy["Minv"], max(KS), keep=KS)
    y64 = PC.yardstick(sy["S"], sy["rhs"], sy["B"], max(KS), dtype=np.float64, keep=KS)
    base = np.array([PC.iterate_error(y64["xs"][k], ref["xs"][k], sy["S"]) for k in KS])
    print("PCG %s@%.0e yardstick fp64 %s" % (name, x, base))
    assert base.max() <= 1e-12, base
    y32 = PC.yardstick(sy["S"], sy["rhs"], sy["B"], max(KS), dtype=np.float32, keep=KS)
    if y32 is not None:
        b32 = np.array([PC.iterate_error(y32["xs"][k], ref["xs"][k], sy["S"]) for k in KS])
        print("PCG %s@%.0e yardstick fp32 %s" % (name, x, b32))
        assert b32.max() <= 1e-3, b32
    a, b = _weakest_pair(sy["S"], N)
    Sd = sy["S"].copy()
    Sd[9 * a:9 * a + 9, 9 * b:9 * b + 9] = 0
    Sd[9 * b:9 * b + 9, 9 * a:9 * a + 9] = 0
    last = np.ones(9 * N, bool)
    last[9 * (N - 1):] = False
    defects = {"diag_cam0": dict(Minv=PC.diagonal_inverse(sy["B"], [0], sy["Minv"])),
               "diag_cam_mid": dict(Minv=PC.diagonal_inverse(sy["B"], [N // 2], sy["Minv"])),
               "diag_cam_last": dict(Minv=PC.diagonal_inverse(sy["B"], [N - 1], sy["Minv"])),
               "pair_dropped": dict(S_product=Sd), "beta_zero": dict(beta="zero"), "beta_stale": dict(beta="stale"),
               "rz_block_dropped": dict(rz_rows=last)}
    for what, kw in defects.items():
        err = _errors(sy, ref, **kw)
        ratio = err / np.maximum(base, 1e-17)
        print("PCG %s@%.0e %s worst at x_%d: %.2e (%.1e x the yardstick)" % (name, x, what, KS[int(ratio.argmax())], err[ratio.argmax()], ratio.max()))
        assert ratio.max() >= 100, (what, err, base)
    assert np.array_equal(_errors(sy, ref, beta="zero")[:1], [0.0]) and np.array_equal(_errors(sy, ref, beta="stale")[:2], [0.0, 0.0])
    # a NaN anywhere fails every bound
    xn = ref["xs"][3].copy()
    xn[5] = np.nan
    assert np.isnan(PC.iterate_error(xn, ref["xs"][3], sy["S"]))


@pytest.mark.parametrize("name", ["p21", "syn9"])
def test_iteration_bound_excludes_the_diagonal_preconditioner(systems, name):
    """At lambda = 1e-6 max diag J'J and rel_tol = 1e-8 / 1e-4 (tests/test_gpu_pcg_stages.py's): the reference with the inverse of
    the blocks' diagonals on every camera needs more than 1.25 k_ref iterations -- the most that file's allowance can ever be -- and so
    does one with beta = 0; the fp64 yardstick stays inside it."""
    sy = systems[(name, LAMS[0])]
    for tol in (1e-8, 1e-4):
        k_ref = PC.pcg(sy["S"], sy["rhs"], sy["Minv"], 1000, tol)
        assert k_ref["converged"]
        most = k_ref["iters"] + int(0.25 * k_ref["iters"])
        kd = PC.pcg(sy["S"], sy["rhs"], PC.diagonal_inverse(sy["B"]), 1000, tol)["iters"]
        kb = PC.pcg(sy["S"], sy["rhs"], sy["Minv"], 1000, tol, beta="zero")["iters"]
        ky = PC.yardstick(sy["S"], sy["rhs"], sy["B"], 1000, tol, dtype=np.float64)["iters"]
        print("PCG %s tol %.0e k_ref %d, at most %d; diagonal preconditioner %d, beta = 0 %d, fp64 yardstick %d" % (name, tol, k_ref["iters"], most, kd, kb, ky))
        assert kd > most and kb > most and ky <= most


def test_documented_blocks_differ_only_where_a_camera_sees_a_point_twice(O):
    """On a problem with a (camera, point) observed three times: documented_blocks equals the block formed directly from J for every
    camera (long double, to 1e-12 of sqrt(B_ii B_jj)), equals the diagonal block of S for the other cameras bit for bit, and differs from
    it for that camera."""
    from conftest import to_oracle
    import bundleadjustment_benchmarks_amd as ba
    p = to_oracle(ba.Problem.synthetic(5, 60, 200, 3))
    src = np.nonzero(p.pt_idx == 7)[0][0]
    cam_idx = np.concatenate([p.cam_idx, [p.cam_idx[src]] * 2])
    pt_idx = np.concatenate([p.pt_idx, [7, 7]])
    meas = np.concatenate([p.meas.reshape(-1, 2), p.meas.reshape(-1, 2)[src] + [[0.3, -0.2], [-0.1, 0.4]]])
    order = np.argsort(pt_idx, kind="stable")
    p = O.Problem(p.N, p.M, p.K + 2, cam_idx[order], pt_idx[order], meas[order].ravel(), p.cams9, p.pts)
    cam = O.init_cams(p)
    f, e = O.residuals(p, cam, p.pts)
    Jc, Jp = O.jacobian(p, cam, p.pts)
    lam = 1e-3
    S = O.referee_reduced_from_jacobian(O.CHOLESKY, p, Jc, Jp, f, lam)["S"]
    B = PC.documented_blocks(p, Jc, Jp, lam, S)
    LD = np.longdouble
    Jcl, Jpl = Jc.astype(LD), Jp.astype(LD)
    Vp = np.zeros((p.M, 3, 3), LD)
    np.add.at(Vp, p.pt_idx, np.einsum("kri,krj->kij", Jpl, Jpl))
    Vp += LD(lam) * np.eye(3, dtype=LD)
    Ci = PC._inv3(Vp)
    W = np.einsum("kri,krj->kij", Jcl, Jpl)
    direct = np.zeros((p.N, 9, 9), LD)
    np.add.at(direct, p.cam_idx, np.einsum("kri,krj->kij", Jcl, Jcl) - np.einsum("kij,kjl,kml->kim", W, Ci[p.pt_idx], W))
    direct += LD(lam) * np.eye(9, dtype=LD)
    a = int(p.cam_idx[np.nonzero(order == src)[0][0]])
    for c in range(p.N):
        d = np.sqrt(np.diagonal(direct[c]))
        assert float((np.abs(B[c] - direct[c]) / np.outer(d, d)).max()) < 1e-12, c  # (measured 1.6e-14: the cofactor inverses at lambda = 1e-3)
        same = np.array_equal(B[c].astype(np.float64), S[9 * c:9 * c + 9, 9 * c:9 * c + 9])
        assert same == (c != a), (c, a)
    Sa = S[9 * a:9 * a + 9, 9 * a:9 * a + 9]
    d = np.sqrt(np.diagonal(Sa))
    assert float((np.abs(B[a].astype(np.float64) - Sa) / np.outer(d, d)).max()) > 1e-6
