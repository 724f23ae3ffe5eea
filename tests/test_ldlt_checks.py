"""CPU: tests/ldlt_checks.py, the reference, families and metrics behind tests/test_gpu_ldlt_kernels.py, checked without a GPU.

The long-double reference against numpy.linalg; the integer family's own assertions at every size of the GPU file; a numpy emulation
of the blocked algorithm (ldlt_checks.emulate: panel, W = L11^-1, Y = A21 W^T, trailing update by tiles, sweep in W form) that passes
every metric and returns the integer family bit for bit in fp32 and fp64; and planted defects in that emulation, each of which must
push the metric named beside it over its bound -- the defects that a backward error of the finished step does not see."""
import numpy as np
import pytest

import ldlt_checks as LC
import ldlt_harness as LH
import stage_checks as SC

# the shapes of tests/test_gpu_ldlt_kernels.py
ONE_BLOCK = [9, 15, 16, 17, 31, 32, 33, 47, 48, 49, 62, 63, 64]
FIRST_STEPS = [65, 80, 81, 112, 127, 128, 129, 191, 192, 193]
SCHEDULED = [261, 320, 324, 384, 513, 576, 577, 640, 704]
LARGE = [3008, 3009, 3072, 3136]


def _family(name, D, fp32):
    if name == "spd2":
        return LC.spd(D, 1e2, 0, fp32)
    if name == "spdhi":
        return LC.spd(D, 1e3 if fp32 else 1e8, 0, fp32)
    if name == "sqd":
        return LC.sqd(D, 0, fp32)
    ex = LC.exact_problem(D)
    return ex["A"].astype(LC.dtype(fp32)), ex["b"].astype(LC.dtype(fp32))


@pytest.mark.parametrize("D", [1, 5, 40, 70])
def test_reference_against_numpy(D):
    A, b = LC.spd(D, 1e2, 3, 0)
    E = np.random.default_rng(D).standard_normal((3, D))
    f = LC.factor(A, np.vstack([b, E]))
    L, d = f["L"].astype(np.float64), f["d"].astype(np.float64)
    assert np.all(d > 0) and np.array_equal(np.triu(L, 1), np.zeros((D, D))) and np.array_equal(np.diagonal(L), np.ones(D))
    assert np.allclose(L * np.sqrt(d)[None, :], np.linalg.cholesky(A), rtol=0, atol=1e-13)
    # the rows that ride along: (D^-1 L^-1 R^T)^T, and the solve
    ref = np.linalg.solve(L * d[None, :], np.vstack([b, E]).T).T
    assert np.allclose(f["Z"].astype(np.float64), ref, rtol=0, atol=1e-12 * np.abs(ref).max())
    assert np.allclose(LC.solve(f, LC.LD).astype(np.float64), np.linalg.solve(A, b), rtol=0, atol=1e-11 * np.abs(b).max())
    for W, (p0, nb) in zip(f["W"], LC.blocks(D)):
        assert np.allclose(W.astype(np.float64)[:nb, :nb], np.linalg.inv(L[p0:p0 + nb, p0:p0 + nb]), rtol=0, atol=1e-12)
    # an indefinite matrix: D keeps the sign of a pivot
    A, b = LC.sqd(D, 3, 0)
    f = LC.factor(A, b[None, :])
    L, d = f["L"].astype(np.float64), f["d"].astype(np.float64)
    assert np.allclose((L * d[None, :]) @ L.T, A, rtol=0, atol=1e-13)
    assert int((d < 0).sum()) == int((np.linalg.eigvalsh(A) < 0).sum()) == D // 2


@pytest.mark.parametrize("D", ONE_BLOCK + FIRST_STEPS + SCHEDULED + LARGE)
def test_exact_family_asserts_its_own_exactness(D):
    """exact_problem asserts integrality, the bounds on the sums of absolute values and the non-zero contribution of every panel to
    every tile; here also: b = A x, z = L^T x, and with a zero pivot the same bounds."""
    ex = LC.exact_problem(D)
    assert ex["terms"] < 2 ** 20 and ex["wmax"] < 2 ** 20 and ex["gemm"] < 2 ** 24
    assert np.array_equal(ex["A"] @ ex["x"], ex["b"]) and np.array_equal(ex["L"].T @ ex["x"], ex["z"])
    assert set(np.abs(ex["d"])) <= {1, 2, 4} and set(np.unique(ex["L"] - np.eye(D, dtype=np.int64))) <= {-1, 0, 1}
    assert np.array_equal(ex["A"].astype(np.float32).astype(np.int64), ex["A"])
    if D <= 704:
        z0 = LC.exact_problem(D, zero_at=D // 2)
        assert z0["d"][D // 2] == 0 and z0["x"] is None


@pytest.mark.parametrize("fp32", [0, 1], ids=["f64", "f32"])
@pytest.mark.parametrize("D", [63, 129, 261, 577])
def test_exact_family_is_bit_exact_in_numpy(D, fp32):
    """The unblocked yardstick and the blocked emulation return the integers bit for bit, in fp32 as in fp64, on both routes."""
    ex = LC.exact_problem(D)
    dt = LC.dtype(fp32)
    f = LC.factor(ex["A"].astype(dt), ex["b"].astype(dt)[None, :], dt)
    assert np.array_equal(f["L"], ex["L"]) and np.array_equal(f["d"], ex["d"]) and np.array_equal(f["z"], ex["z"])
    assert np.array_equal(LC.solve(f, dt), ex["x"])
    S = LH.stage(ex["A"], ex["b"], dt, 0xA5)
    for fused in (True, False):
        assert LC.exact_mismatches(LC.emulate(S, D + 1, D, D, fused=fused), ex) == []


@pytest.mark.parametrize("fp32", [0, 1], ids=["f64", "f32"])
@pytest.mark.parametrize("fam", ["spd2", "spdhi", "sqd"])
@pytest.mark.parametrize("D", [63, 129, 261])
def test_emulation_passes_every_metric(D, fam, fp32):
    A, b = _family(fam, D, fp32)
    S = LH.stage(A, b, LC.dtype(fp32), 0xA5)
    for fused in (True, False):
        m = LC.measure(LC.emulate(S, D + 1, D, D, fused=fused), A, b, fp32, signs=True, cls="hi" if fam == "spdhi" else "1e2")
        bad = {k: v for k, v in m.items() if not v[0] <= v[1]}
        assert not bad, (fused, bad)


# (defect, the metric that must fail); D = 261: five block columns, the last one five wide
DEFECTS = [
    (("skip_tile", 3, 2, 0), "fwd_L"),   # one tile's update from one panel skipped
    (("skip_tile", 4, 4, 2), "fwd_z"),   # ... on the last diagonal tile: only the right-hand side row below it
    (("twice", 3, 1, 0), "fwd_L"),       # one panel applied twice
    (("wp_slot", 2), "fwd_L"),           # Wp slot p - 2 used for p - 1
    (("w_row",), "fwd_W"),               # a W row beyond nb left non-zero
    (("w_swap", 1), "sweep"),            # W0 and W1 swapped in a pair
    (("z_group", 1), "sweep"),           # z of the neighbouring group
    (("sign", 37), "signs"),             # the sign of one pivot dropped
]


@pytest.mark.parametrize("fp32", [0, 1], ids=["f64", "f32"])
@pytest.mark.parametrize("defect,metric", DEFECTS, ids=[d[0][0] + "-" + d[1] for d in DEFECTS])
def test_planted_defect_fails_its_metric(defect, metric, fp32):
    D = 261
    A, b = _family("sqd", D, fp32)
    if defect[0] == "sign":
        neg = np.flatnonzero(LC.factor(A, b[None, :])["d"] < 0)
        defect = ("sign", int(neg[neg >= defect[1]][0]))
    S = LH.stage(A, b, LC.dtype(fp32), 0xA5)
    clean = LC.measure(LC.emulate(S, D + 1, D, D), A, b, fp32, signs=True)
    assert clean[metric][0] <= clean[metric][1]
    m = LC.measure(LC.emulate(S, D + 1, D, D, defect=defect), A, b, fp32, signs=True)
    assert not m[metric][0] <= m[metric][1], (defect, m)
    # ... and the integer family is no longer bit-exact
    if defect[0] != "sign":
        ex = LC.exact_problem(D)
        Se = LH.stage(ex["A"], ex["b"], LC.dtype(fp32), 0xA5)
        assert LC.exact_mismatches(LC.emulate(Se, D + 1, D, D, defect=defect), ex) != []


def test_small_coupling_hides_a_skipped_update_from_eta_but_not_from_the_metrics():
    """Why the finished step's backward error is not enough: with off-diagonal blocks of 1e-9 a skipped tile update moves eta by
    1e-18 -- inside the ceiling 1e-14 -- and fwd_L by 1e-9."""
    D = 261
    A, b = LC.spd(D, 1e2, 1, 0)
    blk = np.arange(D) // 64
    A = np.where(blk[:, None] == blk[None, :], A, 1e-9 * A)
    S = LH.stage(A, b, np.float64, 0)
    m = LC.measure(LC.emulate(S, D + 1, D, D, defect=("skip_tile", 3, 2, 0)), A, b, 0)
    assert m["eta"][0] <= m["eta"][1] and not m["fwd_L"][0] <= m["fwd_L"][1], m


@pytest.mark.parametrize("D", [129, 704])
def test_the_references_own_backward_error(D):
    """eta of the unblocked yardstick's solve in the working precision, and of the long-double solve rounded to it: <= 3.6e-17 (fp64)
    and <= 1.6e-8 (fp32) on all three families (measured: 1.4e-17 and 6.5e-9 at most), far inside the ceilings 1e-14 / 1e-5."""
    for fp32, lim in ((0, 3.6e-17), (1, 1.6e-8)):
        dt = LC.dtype(fp32)
        for fam in ("spd2", "spdhi", "sqd", "exact"):
            A, b = _family(fam, D, fp32)
            A64, b64 = A.astype(np.float64), b.astype(np.float64)
            for f, wd in ((LC.factor(A, b[None, :], dt), dt), (LC.factor(A, b[None, :]), LC.LD)):
                e = SC.eta(A64, LC.solve(f, wd).astype(dt).astype(np.float64), b64)
                print("LDLT_REF D=%d %s %s %s eta %.3e" % (D, "f32" if fp32 else "f64", fam, np.dtype(wd).name, e))
                assert e <= lim, (D, fp32, fam, e)
