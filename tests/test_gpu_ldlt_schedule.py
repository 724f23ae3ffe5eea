"""GPU: the trailing-update schedule of the fused dense LDL^T (ba_ldlt_factor, k_ldlt_step's update jobs) changes WHEN a panel is
applied to a trailing tile, never the order of the operations on any element: the camera + point step of a trial comes out bit for
bit whatever the schedule.  Baseline: the textbook order (an unbounded BA_LDLT_UPD_BUDGET: panel p - 1 on every trailing tile in launch
p, one panel per job).  Against it: budget 0 (only what the deadlines and the depth cap force) with cap 1, 2, 3; mid budgets; the
defaults.  fp64 and fp32, lambda = 1e-10, 1e-3, 10; GET_DX whole, np.array_equal.

Problems (tests/test_gpu_stages.py's synthetic sizes), the smallest shapes where each mechanism first appears:
  N = 29   D = 261, 5 block columns, the last one 5 wide: the first depth-2 and depth-3 jobs
  N = 36   D = 324, 6 block columns: 4 panels pending on the last column, so cap 3 visits a tile twice before its deadline
  N = 57   D = 513, 9 block columns, the last one 1 wide beside the right-hand side row
  N = 64   D = 576 = 9 x 64: the right-hand side row alone in a tenth row block
  N = 240  34 block columns: the size at which a budget of a few hundred units defers as well, and more update jobs per launch
           than CUs"""
import numpy as np
import pytest

from test_gpu_stages import _synthetic

pytestmark = pytest.mark.gpu

LAMBDAS = (1e-10, 1e-3, 10.0)
# (BA_LDLT_UPD_BUDGET, BA_LDLT_UPD_CAP); None = unset (the default)
BASELINE = ("1000000", None)
VARIANTS = [("0", "1"), ("0", "2"), ("0", "3"), ("3", "3"), ("200", "2"), ("300", "4"), (None, None)]

_PROBLEMS = {}


def _steps(ba, monkeypatch, ncams, scalar, budget, cap):
    for name, v in (("BA_LDLT_UPD_BUDGET", budget), ("BA_LDLT_UPD_CAP", cap)):
        if v is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, v)
    if ncams not in _PROBLEMS:
        _PROBLEMS[ncams] = _synthetic(ba, ncams)
    s = ba.Solver(_PROBLEMS[ncams], ba.CHOLESKY, scalar)  # (the schedule is made with the solver)
    s.linearize()
    out = []
    for lam in LAMBDAS:
        s.try_step(lam)
        out.append(s.get(ba.GET_DX).copy())
    return out


@pytest.mark.parametrize("scalar", [0, 1], ids=["f64", "f32"])
@pytest.mark.parametrize("ncams", [29, 36, 57, 64, 240])
def test_step_is_bit_equal_under_every_schedule(ba, gpu_ok, monkeypatch, ncams, scalar):
    ref = _steps(ba, monkeypatch, ncams, scalar, *BASELINE)
    for dx in ref:
        assert np.all(np.isfinite(dx)) and np.any(dx != 0)
    bad = []
    for budget, cap in VARIANTS:
        got = _steps(ba, monkeypatch, ncams, scalar, budget, cap)
        for lam, a, b in zip(LAMBDAS, ref, got):
            same = np.array_equal(a, b)
            print("LDLT_SCHEDULE N=%d %s budget=%s cap=%s lambda=%g equal=%s max|diff|=%.3e" % (ncams, "f64" if scalar == 0 else "f32", budget, cap, lam, same,
                                                                                              float(np.max(np.abs(a - b)))))
            if not same:
                bad.append((budget, cap, lam))
    assert not bad, bad
