"""GPU: the dense LDL^T of ba_dense.hip.h (k_ldlt_panel, k_ldlt_step, k_ldlt_step2, k_ldlt_update, k_ldlt_backflow, k_ldlt_backpair,
k_ldlt_backstep) on its own inputs, at every block shape.

test_gpu_stages.py::test_factor_and_sweep_backward_error reaches these kernels only through ba.Solver: reduced camera matrices, and eta
of the finished step.  Here tests/ldlt_harness.hip calls ba_ldlt_make_plan, ba_ldlt_factor and ba_ldlt_backsweep unchanged on matrices
from the host, and tests/ldlt_checks.py measures what they leave -- L below the diagonal blocks, Y = L D in Wp, W = L11^-1 in Winv, the
row z, and x of both sweep routes -- against a long-double factorisation of the same matrix (metrics and families: its docstring).

Shapes: ncols = D, nrows = D + 1, zrow = D, Dp / ld as the solver computes them.
  one block column      D = 9 ... 64: the sub-panel seams; 64: the right-hand side row alone in a second row block
  first fused steps     D = 65 ... 193: last-block widths 1, 16, 17, 48, 63, 0 behind one and two full block columns
  scheduled jobs        D = 261 ... 704: 5, 6, 9, 10, 11 block columns (first depth-2 / -3 jobs, a tile visited twice), widths 5, 0, 1
  k_ldlt_step's last / k_ldlt_step2's first size   D = 3008 (47 full), 3009 (48, the last 1 wide), 3072 (48 full), 3136 (49, odd)
  pair phase            D = 3072, 3136 with BA_LDLT_PAIR_MIN=8: the first odd single-panel step at an even and an odd count
Checks:
  exact      the integer family at every shape, fused (default plan) and safe factor x one-launch and launch-per-pair sweep, fp64 and
             fp32: L, Y (retained slots), W, z, x equal the integers bit for bit.  The only look inside the factor at D >= 3008.
  families   spd (condition 1e2; 1e8 fp64 / 1e3 fp32) and sqd at D <= 704: eta, sweep (both routes), fwd_L, fwd_Y, fwd_W, fwd_z, yld
             on the fused and the safe factor; sqd: the pivots' sign pattern.  spd 1e2 at D >= 3008: eta and sweep only (the long-double
             factor there would take minutes).
  zero pivot exact with one d_k = 0, D = 63, 129, 704, k at the first / last pivot of a sub-panel and of a block column, in the first,
             a middle and the last block column, both factor routes and both sweeps: x holds a non-finite value, no HIP error.
  padding    fill bytes 0x00 and 0xA5 give the same bits in everything the contract defines; guards intact; columns >= Dp untouched
  schedules  D = 261, 324, 513, 576, 704: S, Wp, Winv, x bit-equal under test_gpu_ldlt_schedule.py's BASELINE and VARIANTS
  covariance the form cov_compute factors (safe, nrows = ncols + D stacked rows), fp64, D = 63, 130, 577, 700: exact bit for bit,
             fwd_B and the pivots s_k / B_kk on spd
Bounds: eta the project's ceilings 1e-14 / 1e-5; sweep (ncols + 64) eps; fwd_* and yld max(10 x the unblocked yardstick in the
working precision by the same metric on the same matrix, floor), floors in ldlt_checks.FLOOR beside the worst values measured.
Every value is printed as `LDLT <case> <metric> <value> <bound>`.  A HIP error or a device error word fails the test that met it and
skips every later test of the module: nothing is launched behind a fault.
No case is left out of a metric, with one statement moved: the padding test compares rows <= D of S, not rows < Dp (_defined says why).
Measured worst on an MI355X, fp64 / fp32 (profiles/r18_ldlt_kernels.txt): exact bit for bit on all 38 shapes x 4 routes and in the
covariance form; all 37 zero-pivot placements leave a non-finite x on every route (no kernel change was needed); condition 1e2 and sqd:
eta 6.6e-17 / 2.9e-8, sweep 4.6e-16 / 2.0e-7, fwd_L and fwd_Y 5.2e-13 / 3.5e-4 (bound 2.3e-12 / 1.8e-3 from the yardstick), fwd_W
2.5e-15 / 1.2e-6, fwd_z 7.9e-15 / 4.3e-6, yld 7.7e-15 / 4.2e-6, no pivot sign differs; condition 1e8 / 1e3: fwd_L and fwd_Y 7.9e-8 /
2.1e-3, fwd_W 1.9e-9 / 5.5e-6, fwd_z 2.0e-9 / 2.3e-5, yld 8.9e-10 / 1.4e-5; covariance form fwd_B 1.0e-14 (1e2), 1.3e-9 (1e8), pivots
1.0e-14, 4.1e-10.  The 306 cases take 75 s on an MI355X box, the harness build included; the longest case 4.2 s
(the covariance form at D = 700: two long-double factors with 700 stacked rows).
"""
import numpy as np
import pytest

import ldlt_checks as LC
import ldlt_harness as LH
from test_gpu_ldlt_schedule import BASELINE, VARIANTS
from test_gpu_stages import BOUND as STAGE_BOUND
from test_gpu_stages import Checker

pytestmark = pytest.mark.gpu

ONE_BLOCK = [9, 15, 16, 17, 31, 32, 33, 47, 48, 49, 62, 63, 64]
FIRST_STEPS = [65, 80, 81, 112, 127, 128, 129, 191, 192, 193]
SCHEDULED = [261, 320, 324, 384, 513, 576, 577, 640, 704]
LARGE = [3008, 3009, 3072, 3136, "3072pair8", "3136pair8"]
ROUTES = [(True, "flow"), (True, "launches"), (False, "flow"), (False, "launches")]
TYPES = pytest.mark.parametrize("fp32", [0, 1], ids=["f64", "f32"])

assert LC.ETA == {0: STAGE_BOUND[("eta", 0)], 1: STAGE_BOUND[("eta", 1)]}


class LChecker(Checker):
    def __call__(self, metric, value, bound):
        self.rows.append((metric, float(value), float(bound)))
        print("LDLT %s %s %.3e %.1e" % (self.case, metric, value, bound))


@pytest.fixture(scope="module")
def ldh(tmp_path_factory, gpu_ok):
    return LH.Harness(LH.build(tmp_path_factory.mktemp("ldlt_harness")))


def go(ldh, S, D, fp32, fused=True, sweep="flow", **kw):
    """One harness run of the solver form; fails on a HIP error, a device error word or a broken guard."""
    if ldh.failed:
        pytest.skip("an earlier run of this module failed: " + ldh.failed)
    r = ldh.run(S, D + 1, D, D, fp32, fused=fused, sweep=sweep, **kw)
    assert r["rc"] == 0 and not r["errw"].any(), ldh.failed
    assert r["guards"].all(), dict(zip(LH.GUARDS, r["guards"]))
    return r


def _size(case, monkeypatch):
    if isinstance(case, str):
        monkeypatch.setenv("BA_LDLT_PAIR_MIN", "8")
        return int(case[:4])
    monkeypatch.delenv("BA_LDLT_PAIR_MIN", raising=False)
    return case


def _name(fused, sweep):
    return "%s+%s" % ("fused" if fused else "safe", sweep)


# ---- the integer family: bit for bit on every route ---------------------------------------------------------------------------------------
@TYPES
@pytest.mark.parametrize("case", ONE_BLOCK + FIRST_STEPS + SCHEDULED + LARGE, ids=str)
def test_exact_family_bit_for_bit(ldh, monkeypatch, case, fp32):
    D = _size(case, monkeypatch)
    ex = LC.exact_problem(D, check=D <= 704)  # (the builder's own assertions at the large sizes: tests/test_ldlt_checks.py)
    S = LH.stage(ex["A"], ex["b"], LC.dtype(fp32), 0xA5)
    bad = {}
    for fused, sweep in ROUTES:
        mis = LC.exact_mismatches(go(ldh, S, D, fp32, fused, sweep), ex)
        print("LDLT exact[%s,%s,%s] mismatches %s" % (case, "f32" if fp32 else "f64", _name(fused, sweep), mis))
        if mis:
            bad[_name(fused, sweep)] = mis
    assert not bad, bad


# ---- spd and sqd against the long-double factor ------------------------------------------------------------------------------------------
def _family(fam, D, fp32):
    if fam == "spd2":
        return LC.spd(D, 1e2, 0, fp32)
    if fam == "spdhi":
        return LC.spd(D, 1e3 if fp32 else 1e8, 0, fp32)
    return LC.sqd(D, 0, fp32)


@TYPES
@pytest.mark.parametrize("fam", ["spd2", "spdhi", "sqd"])
@pytest.mark.parametrize("D", ONE_BLOCK + FIRST_STEPS + SCHEDULED)
def test_families_against_long_double(ldh, D, fam, fp32):
    """Fused and safe factor with every metric, the launch-per-pair sweep behind the fused factor with eta and sweep."""
    A, b = _family(fam, D, fp32)
    S = LH.stage(A, b, LC.dtype(fp32), 0xA5)
    ck = LChecker("%s[%d,%s]" % (fam, D, "f32" if fp32 else "f64"))
    for fused, sweep, forward in ((True, "flow", True), (False, "launches", True), (True, "launches", False), (False, "flow", False)):
        r = go(ldh, S, D, fp32, fused, sweep)
        m = LC.measure(r, A, b, fp32, forward=forward, signs=forward and fam == "sqd", cls="hi" if fam == "spdhi" else "1e2")
        for k, (v, bd) in m.items():
            ck("%s:%s" % (_name(fused, sweep), k), v, bd)
    ck.done()


@TYPES
@pytest.mark.parametrize("case", LARGE, ids=str)
def test_large_spd_eta_and_sweep(ldh, monkeypatch, case, fp32):
    """spd, condition 1e2, at k_ldlt_step's last and k_ldlt_step2's first sizes: eta and the sweep metric under both sweep routes (the
    fused factor; the safe one at these sizes is pinned by the integer family)."""
    D = _size(case, monkeypatch)
    A, b = LC.spd(D, 1e2, 0, fp32)
    S = LH.stage(A, b, LC.dtype(fp32), 0xA5)
    ck = LChecker("spd2[%s,%s]" % (case, "f32" if fp32 else "f64"))
    for sweep in ("flow", "launches"):
        r = go(ldh, S, D, fp32, True, sweep)
        for k, (v, bd) in LC.measure(r, A, b, fp32, forward=False).items():
            ck("%s:%s" % (_name(True, sweep), k), v, bd)
    ck.done()


# ---- padding, guards, schedules --------------------------------------------------------------------------------------------------------
def _defined(r, D):
    """What a run leaves for anybody to read: the lower triangle of S in rows <= D (the matrix and the right-hand side row) of the
    columns < D, the rows [64 (p + 1), D] of the retained Wp slots, Winv, x.
    Not the rows D + 1 ... Dp - 1, which the contract zeroes on entry (found by this test's first run): the row GEMM of a panel leaves
    out the 16-row granules past nrows, so Wp keeps whatever it held there, and the trailing update, which works on whole tiles,
    carries that into those rows of S and on into the padding columns.  No pivot, no row of L, z, W or x ever reads them."""
    low = np.tril(np.ones((D + 1, D), bool)).T  # [column, row]: row >= column
    out = [r["S"][:D, :D + 1][low], r["Winv"], r["x"][:D]]
    for p, slot in sorted(LC.retained(D, r["fused"]).items()):
        out.append(r["Wp"][slot][:, 64 * (p + 1):D + 1])
    return out


@TYPES
@pytest.mark.parametrize("D", [63, 129, 577])
def test_padding_and_guards(ldh, D, fp32):
    """Everything the staging contract leaves open -- rows >= Dp, the strictly upper triangle, the Wp, Winv and x storage -- filled with
    0x00 and with 0xA5: the same bits in everything the contract defines, on every route.  Columns >= Dp of S still hold the fill,
    behind the factor and behind the sweep (guards: every run of this file, go())."""
    A, b = LC.spd(D, 1e2, 0, fp32)
    dt = LC.dtype(fp32)
    Dp = LH.layout(D)[0]
    for fused, sweep in ROUTES:
        runs = [go(ldh, LH.stage(A, b, dt, fill), D, fp32, fused, sweep, fill=fill, after=True) for fill in (0x00, 0xA5)]
        for u, v in zip(_defined(runs[0], D), _defined(runs[1], D)):
            assert np.array_equal(u, v, equal_nan=True), (_name(fused, sweep), D)
        assert np.all(np.isfinite(runs[0]["x"][:D]))
        for r in runs:
            for key in ("S", "S2"):
                assert np.all(np.frombuffer(r[key][Dp:].tobytes(), np.uint8) == r["fill"]), (key, r["fill"])


def _plan(ldh, budget, cap):
    b0, c0 = ldh.defaults()
    return (b0 if budget is None else int(budget), c0 if cap is None else int(cap))


@TYPES
@pytest.mark.parametrize("D", [261, 324, 513, 576, 704])
def test_factor_is_bit_equal_under_every_schedule(ldh, D, fp32):
    """test_gpu_ldlt_schedule.py's statement about dx, extended to the factor: the whole S, Wp, Winv and x under the textbook order
    (BASELINE) and under every plan of VARIANTS, the plans made with those numbers."""
    A, b = LC.spd(D, 1e2, 0, fp32)
    S = LH.stage(A, b, LC.dtype(fp32), 0xA5)
    ref = go(ldh, S, D, fp32, True, "flow", plan=_plan(ldh, *BASELINE))
    assert np.all(np.isfinite(ref["x"][:D]))
    bad = []
    for budget, cap in VARIANTS:
        r = go(ldh, S, D, fp32, True, "flow", plan=_plan(ldh, budget, cap))
        same = [np.array_equal(ref[k], r[k], equal_nan=True) for k in ("S", "Wp", "Winv")] + [np.array_equal(ref["x"][:D], r["x"][:D])]
        print("LDLT schedule[%d,%s] budget=%s cap=%s S/Wp/Winv/x equal %s" % (D, "f32" if fp32 else "f64", budget, cap, same))
        if not all(same):
            bad.append((budget, cap, same))
    assert not bad, bad


# ---- the covariance's use of the factor -------------------------------------------------------------------------------------------------
def _cov_run(ldh, A, s):
    if ldh.failed:
        pytest.skip("an earlier run of this module failed: " + ldh.failed)
    D = A.shape[0]
    ncols, nrows, ld, scols = LH.cov_layout(D)
    r = ldh.run(LH.stage_cov(A, s, np.float64), nrows, ncols, ncols, 0, fused=False, sweep=None)
    assert r["rc"] == 0 and not r["errw"].any(), ldh.failed
    assert r["guards"].all(), dict(zip(LH.GUARDS, r["guards"]))
    return r


@pytest.mark.parametrize("D", [63, 130, 577, 700])
def test_covariance_form(ldh, D):
    """ba_ldlt_factor as cov_compute calls it (fp64): ncols = 64 ceil(D / 64) with the padding's unit pivots, D stacked rows s_k e_k^T,
    safe route.  The integer family: L below the diagonal blocks, W and the stacked rows B = E L^-T D^-1 bit for bit.  spd (1e2, 1e8):
    fwd_B and the pivots s_k / B_kk against the long-double factor of the padded matrix with its stacked rows."""
    ncols = LH.cov_layout(D)[0]
    ex = LC.exact_problem(D)
    s = np.random.default_rng(D).integers(1, 4, D)
    r = _cov_run(ldh, ex["A"], s)
    Lh = np.where(LC.below_mask(D), r["S"][:D, :D].T, 0)
    assert np.array_equal(Lh, np.where(LC.below_mask(D), ex["L"], 0))
    assert np.array_equal(r["S"][:D, ncols:ncols + D].T, LC.exact_cov_rows(ex, s))
    for t, W in enumerate(ex["W"]):
        Wx = np.eye(64)
        nb = min(64, D - 64 * t)
        Wx[:nb, :nb] = W[:nb, :nb]  # (the padding's unit pivots)
        assert np.array_equal(r["Winv"][t], Wx), t
    ck = LChecker("cov[%d]" % D)
    for fam, cond in (("spd2", 1e2), ("spdhi", 1e8)):
        A, _ = LC.spd(D, cond, 0, 0)
        s = np.random.default_rng(D + 1).uniform(0.5, 2.0, D)
        r = _cov_run(ldh, A, s)
        Ap = np.eye(ncols)
        Ap[:D, :D] = A
        E = np.zeros((D, ncols))
        E[np.arange(D), np.arange(D)] = s
        ref, yard = LC.factor(Ap, E), LC.factor(Ap, E, np.float64)
        got = LC.cov_metrics(r, ref, D, s)
        yv = LC.cov_metrics(dict(S=np.hstack([np.zeros((D, ncols)), yard["Z"][:, :D].T]), ncols=ncols), ref, D, s)
        for k in ("fwd_B", "pivots"):
            ck("%s:%s" % (fam, k), got[k], LC.bound(k, 0, yv[k], "hi" if fam == "spdhi" else "1e2"))
    ck.done()


# ---- a zero pivot must not leave a finite step ------------------------------------------------------------------------------------------------
def _zero_placements(D):
    """k at the first and the last pivot of a sub-panel, the first and the last of a block column; first, a middle, the last block column"""
    blk = LC.blocks(D)
    out = []
    for p0, nb in sorted({blk[0], blk[len(blk) // 2], blk[-1]}):
        out += [p0, p0 + min(15, nb - 1), p0 + nb - 1]
        if nb > 16:
            out += [p0 + 16, p0 + 16 * ((nb - 1) // 16), p0 + 16 * ((nb - 1) // 16) - 1]
    return sorted(set(out))


@TYPES
@pytest.mark.parametrize("D", [63, 129, 704])
def test_zero_pivot_leaves_a_non_finite_step(ldh, D, fp32):
    """k_lm_control rejects a trial only through non-finite scalars: an exactly zero pivot, wherever it falls, must leave at least one
    non-finite value in x (and no HIP error) -- the defect the dense QR once shipped (ba_qr.hip.h, the zero-diagonal guard of
    k_qr_backsolve).  The integer family with d_k = 0: the pivot is an exact zero on the device as well."""
    finite = []
    for k in _zero_placements(D):
        ex = LC.exact_problem(D, zero_at=k, check=False)
        S = LH.stage(ex["A"], ex["b"], LC.dtype(fp32), 0xA5)
        for fused, sweep in ROUTES:
            x = go(ldh, S, D, fp32, fused, sweep)["x"][:D]
            if np.all(np.isfinite(x)):
                finite.append((k, _name(fused, sweep)))
    print("LDLT zero_pivot[%d,%s] placements %s all-finite %s" % (D, "f32" if fp32 else "f64", _zero_placements(D), finite))
    assert not finite, finite
