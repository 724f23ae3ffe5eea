"""ba_solver_covariance_pcg, the part that needs no GPU: the yardstick of tests/covpcg_checks.py (covariance blocks by per-column PCG on
the reduced system) against the dense inverse of the whole J'J + lam I, a planted defect that the bound must see, the declarations, and
the register report of the new kernels.  Every figure is printed as `COVPCG <case> <metric> <value> <bound>`."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import cov_checks as CC
import covpcg_checks as CP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = float(np.finfo(np.float64).eps)
REL_TOL = 1e-10
_cases = {}


def _case(ba, O, seed, case):
    """(covpcg Case, dense inverse, N, M) of synthetic(6, 40, 160, seed): `damped` = no mask, lam = 1e-3 max diag J'J; `gauge` = gauge mask,
    two points and the rank-2 points fixed, lam = 0 (test_covariance_cpu.py's two cases)."""
    if (seed, case) in _cases:
        return _cases[seed, case]
    pg = ba.Problem.synthetic(6, 40, 160, seed)
    po = CC.sorted_oracle_problem(O, pg)
    Jc, Jp = O.jacobian(po, O.init_cams(po), po.pts.copy())
    if case == "damped":
        cm, pf = None, None
        lam = 1e-3 * max(float((Jc ** 2).sum(axis=1).max()), float((Jp ** 2).sum(axis=1).max()))
    else:
        cm, pf, lam = pg.gauge_mask(0), np.zeros(pg.M, np.uint8), 0.0
        pf[[5, 17]] = 1
        ev = np.linalg.eigvalsh(CC.point_blocks(po, Jc, Jp, 0.0)[0])
        pf[ev[:, 0] <= 1e-10 * ev[:, 2]] = 1  # (rank-2 U_p of twice-seen outlier points: no inverse at lam = 0)
    fc, fp = CC.free_sets(po, cm, pf)
    Jcm, Jpm = CC.mask_jacobian(po, Jc, Jp, cm, pf)
    S = CC.quad_reduced(O, O.CHOLESKY, po, Jcm, Jpm, lam, fp)
    cs = CP.Case(po, Jc, Jp, lam, S, cm, pf)
    dense = CC.dense_covariance(po, Jc, Jp, lam, cm, pf)
    _cases[seed, case] = (cs, dense, pg.N, pg.M)
    return _cases[seed, case]


def _excess(cs, dense, N, M, cc, pp, info, tag):
    """Largest (entry error - bound) / bound over all camera and point entries, bound per entry =
    |S^-1|_2 rel_tol |b_i|_2 |b_j|_2 + 8 cond(H) eps max block (the issue's: test_covariance_cpu.py's bound plus the inexact solve's)."""
    pairs = CP.all_pairs(N)
    ninv = cs.norm_inverse()
    sc_c, sc_p = CP.entry_scales(pairs, info["Ynorm"])
    dc = dense["cc"].reshape(N, 9, N, 9).transpose(0, 2, 1, 3).reshape(-1, 9, 9)
    fro = lambda x: float(np.sqrt((x ** 2).sum(axis=(1, 2))).max())  # noqa: E731
    bc = ninv * REL_TOL * sc_c + 8 * dense["cond"] * EPS * fro(dc)
    bp = ninv * REL_TOL * sc_p + 8 * dense["cond"] * EPS * fro(dense["pp"])
    ec, ep = np.abs(np.asarray(cc, np.float64) - dc), np.abs(np.asarray(pp, np.float64) - dense["pp"])
    print("COVPCG %s camera_entries %.3e %.1e" % (tag, ec.max(), bc.min()))
    print("COVPCG %s point_entries %.3e %.1e" % (tag, ep.max(), bp.min()))
    return max(float((ec / bc).max()), float((ep / bp).max()))


@pytest.mark.parametrize("seed", [3, 11])
@pytest.mark.parametrize("case", ["damped", "gauge"])
def test_yardstick_matches_the_dense_inverse(ba, O, seed, case):
    cs, dense, N, M = _case(ba, O, seed, case)
    cc, pp, info = cs.covariance(CP.all_pairs(N), np.arange(M), 1000, REL_TOL)
    print("COVPCG yardstick[%s,%d] cond(H) %.3e |S^-1| %.3e iterations %d-%d columns %d" %
          (case, seed, dense["cond"], cs.norm_inverse(), min(info["iters"]), max(info["iters"]), info["columns"]))
    assert info["unconverged"] == 0
    assert _excess(cs, dense, N, M, cc, pp, info, "yardstick[%s,%d]" % (case, seed)) <= 1.0
    # fixed parameters: exact zeros; Sigma_ab == Sigma_ba' in bits; diagonal and point blocks symmetric
    Sig = CP.assemble(cc, N)
    assert not Sig[~cs.fc].any() and not Sig[:, ~cs.fc].any() and not pp[~cs.fp].any()
    assert np.array_equal(Sig, Sig.T) and np.array_equal(pp, pp.transpose(0, 2, 1))
    assert info["columns"] == int(cs.fc.sum()) * 1 + 3 * int(cs.fp.sum())


@pytest.mark.parametrize("case", ["damped", "gauge"])
def test_one_alpha_for_the_batch_misses_the_bound(ba, O, case):
    """The planted defect: the columns of a batch share one alpha.  Each column's r is still its true residual, so a run long enough
    could still end inside the bound; the per-column recurrence needs k_ref iterations for its slowest column, and capped there the
    right recurrence is inside the bound while the defective one must be outside."""
    cs, dense, N, M = _case(ba, O, 3, case)
    pairs, pts = CP.all_pairs(N), np.arange(M)
    _, _, info = cs.covariance(pairs, pts, 1000, REL_TOL)
    k_ref = int(max(info["iters"]))
    good = cs.covariance(pairs, pts, k_ref, REL_TOL)
    bad = cs.covariance(pairs, pts, k_ref, REL_TOL, shared_alpha=True)
    e_good = _excess(cs, dense, N, M, *good, "capped[%s]" % case)
    e_bad = _excess(cs, dense, N, M, *bad, "one_alpha[%s]" % case)
    print("COVPCG one_alpha[%s] k_ref %d excess_good %.3e excess_planted %.3e" % (case, k_ref, e_good, e_bad))
    assert e_good <= 1.0 < e_bad


def test_header_and_binding_declare_the_entry_point(ba):
    import ctypes as C
    hdr = open(os.path.join(ROOT, "include", "ba_mi355x.h")).read()
    assert re.search(r"\bint\s+ba_solver_covariance_pcg\s*\(\s*ba_solver\s*\*\s*s\s*,\s*double\s+lambda\s*,\s*int\s+max_iter\s*,\s*double\s+rel_tol\s*,"
                     r"\s*int\s+n_pairs\s*,\s*const\s+int\s*\*\s*cam_pairs\s*,\s*double\s*\*\s*cam_cov\s*,\s*int\s+n_pts\s*,\s*const\s+int\s*\*\s*pt_ids\s*,"
                     r"\s*double\s*\*\s*pt_cov\s*,\s*ba_cov_pcg_stats\s*\*\s*stats", hdr)
    m = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*ba_cov_pcg_stats\s*;", hdr)
    assert m
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    assert re.sub(r"\s+", " ", body).strip() == ("long long columns, batches, total_iters; int max_iters, unconverged; "
                                                  "double worst_rel_residual; double ms;")
    assert "ba_solver_covariance_pcg" in ba.EXPORTS
    assert [f[0] for f in ba.CovPCGStats._fields_] == ["columns", "batches", "total_iters", "max_iters", "unconverged", "worst_rel_residual", "ms"]
    assert [f[1] for f in ba.CovPCGStats._fields_] == [C.c_longlong] * 3 + [C.c_int] * 2 + [C.c_double] * 2
    assert hasattr(ba.Solver, "covariance_pcg")
    assert hasattr(ba.lib(), "ba_solver_covariance_pcg")


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not available")
def test_multi_column_kernels_do_not_spill(tmp_path):
    """Every kernel of csrc/ba_pcg_multi.hip.h cross-compiled for gfx950 with csrc/Makefile's own flags: no spilled VGPR, no scratch."""
    import qr_harness as QH
    hipcc, flags = QH.makefile_flags()
    out = subprocess.run([hipcc] + flags + ["-w", "-I", QH.CSRC, "--cuda-device-only", "-c", os.path.join(ROOT, "tests", "covpcg_resources.hip"), "-o",
                          str(tmp_path / "covpcg.o"), "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    usage = {}
    for m in re.finditer(r"Function Name: (\S+)", out.stderr):
        block = out.stderr[m.end():m.end() + 2500]
        get = lambda pat: int(re.search(pat, block).group(1))  # noqa: E731
        usage[m.group(1)] = dict(vgpr=get(r"VGPRs: (\d+)"), occ=get(r"Occupancy \[waves/SIMD\]: (\d+)"), spill=get(r"VGPRs Spill: (\d+)"),
                                 scratch=get(r"ScratchSize \[bytes/lane\]: (\d+)"))
    mc = {k: v for k, v in usage.items() if "k_mc_" in k}
    for k, v in sorted(mc.items()):
        print("COVPCG resources %s %s" % (k, v))
    # 7 plain kernels + scal, point, cam_chunks, alpha x 2 + cam x 4
    assert len(mc) == 19, sorted(usage)
    for k, v in mc.items():
        assert v["spill"] == 0 and v["scratch"] == 0, (k, v)
