"""CPU: parameters held constant (ba_solver_set_constant, ba_problem_gauge_mask).  The gauge mask's rule against a numpy restatement,
and -- with the CPU oracle on a Jacobian whose fixed columns are zeroed -- that it removes the 7-dimensional similarity null space of
J'J and that the LDL^T step of a fixed parameter is exactly 0.  No GPU: ba_problem_gauge_mask is host-only."""
import numpy as np
import pytest

from conftest import DATA21

BA_ERR_ARG = 4


def rodrigues(om):
    th = np.sqrt(om[0] * om[0] + om[1] * om[1] + om[2] * om[2])
    R = np.eye(3)
    if th > 1e-6:
        J = np.array([[0, -om[2], om[1]], [om[2], 0, -om[0]], [-om[1], om[0], 0]])
        R = R + np.sin(th) / th * J + (1 - np.cos(th)) / (th * th) * (J @ J)
    return R


def gauge_rule(cams9, ref):
    """BA_FIX_POSE on ref; camera b farthest from C_ref (centre C = -R^T T); bit argmax_k |(T_b + R_b C_ref)_k| of b (lowest wins ties)."""
    N = len(cams9) // 9
    c = cams9.reshape(N, 9)
    R = [rodrigues(c[a, 0:3]) for a in range(N)]
    C = np.array([-R[a].T @ c[a, 3:6] for a in range(N)])
    d = ((C - C[ref]) ** 2).sum(1)
    d[ref] = -1
    b = int(np.argmax(d))
    v = np.abs(c[b, 3:6] + R[b] @ C[ref])
    k = int(np.argmax(v))
    m = np.zeros(N, np.uint16)
    m[ref] |= 0x3F
    m[b] |= 1 << k
    return m


@pytest.fixture(scope="module")
def p21(ba):
    return ba.Problem.load_bal(DATA21)


def test_fix_constants(ba):
    assert (ba.FIX_T, ba.FIX_OMEGA, ba.FIX_POSE, ba.FIX_INTRINSICS, ba.FIX_CAMERA) == (0x7, 0x38, 0x3F, 0x1C0, 0x1FF)
    assert ba.FIX_T | ba.FIX_OMEGA == ba.FIX_POSE and ba.FIX_POSE | ba.FIX_INTRINSICS == ba.FIX_CAMERA


def test_gauge_mask_problem21(ba, p21):
    m = p21.gauge_mask(0)
    assert m.dtype == np.uint16 and m.shape == (p21.N,)
    want = np.zeros(p21.N, np.uint16)
    want[0] = ba.FIX_POSE
    # camera 11's centre lies farthest from camera 0's, and T_z dominates dT/ds: |T + R C_0| = (1.005, 0.137, 2.068).  (Camera 6 / T_x
    # is what the rule gives when the oracle's per-camera init_cams array, [N][15], is read parameter-major by mistake.)
    want[11] = 1 << 2
    assert np.array_equal(m, want), np.nonzero(m)
    assert np.array_equal(m, gauge_rule(p21.arrays()["cams9"], 0))


def test_gauge_mask_other_reference_camera(ba, p21):
    m = p21.gauge_mask(3)
    assert np.array_equal(m, gauge_rule(p21.arrays()["cams9"], 3))
    assert m[3] == ba.FIX_POSE and np.count_nonzero(m) == 2


def test_gauge_mask_ors_into_the_callers_words(ba, p21):
    import ctypes as C
    m = np.full(p21.N, ba.FIX_INTRINSICS, np.uint16)
    assert ba.lib().ba_problem_gauge_mask(p21._h, 0, m.ctypes.data_as(C.c_void_p)) == 0
    assert np.array_equal(m, p21.gauge_mask(0) | np.uint16(ba.FIX_INTRINSICS))


def test_gauge_mask_bad_arguments(ba, p21):
    for ref in (-1, p21.N):
        with pytest.raises(ba.BAError) as e:
            p21.gauge_mask(ref)
        assert e.value.code == BA_ERR_ARG
    one = ba.Problem.from_arrays(1, 1, 1, [0], [0], [0.1, 0.2], [0.01, 0.02, 0.03, 0, 0, -5, 500, 0, 0], [0.1, 0.2, 0.3])
    with pytest.raises(ba.BAError) as e:
        one.gauge_mask(0)
    assert e.value.code == BA_ERR_ARG


def _scaled_spectrum(S, lam, free):
    A = S[np.ix_(free, free)] - lam * np.eye(len(free))
    d = 1.0 / np.sqrt(np.diag(A))
    return np.linalg.eigvalsh(A * d[:, None] * d[None, :])


def _fixed_columns(N, cam_mask):
    """Indices (into the D camera unknowns) that cam_mask fixes."""
    return np.array([9 * a + q for a in range(N) for q in range(9) if (int(cam_mask[a]) >> q) & 1], int)


@pytest.mark.parametrize("intrinsics", [False, True], ids=["gauge", "gauge+intrinsics"])
def test_gauge_mask_removes_the_null_space(ba, O, p21, intrinsics):
    po = O.load_bal(DATA21)
    cam = O.init_cams(po)
    f, _ = O.residuals(po, cam, po.pts)
    Jc, Jp = O.jacobian(po, cam, po.pts)
    lam = 1e-10
    S0 = O.step(O.CHOLESKY, po, Jc, Jp, f, lam)["S"]
    ev0 = _scaled_spectrum(S0, lam, np.arange(po.D))
    assert np.sum(ev0 <= 1e-11) >= 7, ev0[:10]

    m = p21.gauge_mask(0)
    if intrinsics:
        m |= np.uint16(ba.FIX_INTRINSICS)
    fixed = _fixed_columns(po.N, m)
    assert len(fixed) == (7 + 3 * po.N if intrinsics else 7)
    # zero column q of every observation of a camera whose bit q is set
    Jcm = Jc.copy()
    cm = m[po.cam_idx].astype(np.int64)
    for q in range(9):
        Jcm[(cm >> q) & 1 == 1, :, q] = 0
    st = O.step(O.CHOLESKY, po, Jcm, Jp, f, lam)
    S = st["S"]
    free = np.setdiff1d(np.arange(po.D), fixed)
    # a fixed row / column of S is lambda alone
    assert np.all(S[fixed][:, free] == 0) and np.allclose(np.diag(S)[fixed], lam, rtol=0, atol=0)
    ev = _scaled_spectrum(S, lam, free)
    assert ev.min() > 1e-8, ev[:5]
    dx_c = st["dx"][3 * po.M:]
    assert np.all(dx_c[fixed] == 0), dx_c[fixed]
    assert np.any(dx_c[free] != 0)
