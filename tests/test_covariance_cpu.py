"""Covariance blocks, the part that needs no GPU: the Schur formulas and the fixed-parameter rules of tests/cov_checks.py against the
dense inverse of the whole J'J + lam I (oracle Jacobian, a small synthetic problem), the declarations, and the register report of the
new kernels.  Every figure is printed as `COV <case> <metric> <value> <bound>`."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import cov_checks as CC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = float(np.finfo(np.float64).eps)


def _small(ba, O, seed):
    pg = ba.Problem.synthetic(6, 40, 160, seed)
    po = CC.sorted_oracle_problem(O, pg)
    Jc, Jp = O.jacobian(po, O.init_cams(po), po.pts.copy())
    return pg, po, Jc, Jp


@pytest.mark.parametrize("seed", [3, 11])
@pytest.mark.parametrize("case", ["damped", "gauge"])
def test_schur_formulas_match_the_dense_inverse(ba, O, seed, case):
    """reference_covariance (S^-1, U^-1 + U^-1 (sum W' Sigma W) U^-1) against the inverse of the whole H on the free parameters: no mask
    at lam = 1e-3 max diag J'J, and gauge mask + two fixed points at lam = 0.  Both routes are fp64, each with a norm-wise relative
    error of a modest multiple of cond(H) eps, so the largest block difference relative to the largest block of its kind (a block much
    smaller than the largest inherits the norm-wise error) is bounded by 8 cond(H) eps; cond(H) is computed and printed."""
    pg, po, Jc, Jp = _small(ba, O, seed)
    if case == "damped":
        cm, pf = None, None
        lam = 1e-3 * max(float((Jc ** 2).sum(axis=1).max()), float((Jp ** 2).sum(axis=1).max()))
    else:
        cm, pf, lam = pg.gauge_mask(0), np.zeros(pg.M, np.uint8), 0.0
        pf[[5, 17]] = 1
        # (the robustifier leaves an outlier observation a rank-1 Jacobian: a point seen twice, both times as an outlier, has a rank-2
        # U_p and no covariance at lam = 0 whatever the gauge -- such points are held fixed as well; test_gpu_covariance.py's finding)
        U, _ = CC.point_blocks(po, Jc, Jp, 0.0)
        ev = np.linalg.eigvalsh(U)
        pf[ev[:, 0] <= 1e-10 * ev[:, 2]] = 1
        assert (pf == 0).sum() >= 10
    dense = CC.dense_covariance(po, Jc, Jp, lam, cm, pf)
    ref = CC.reference_covariance(po, Jc, Jp, lam, cm, pf)
    bound = 8 * dense["cond"] * EPS
    N = pg.N
    cc_d = dense["cc"].reshape(N, 9, N, 9).transpose(0, 2, 1, 3).reshape(-1, 9, 9)
    cc_r = ref["cc"].reshape(N, 9, N, 9).transpose(0, 2, 1, 3).reshape(-1, 9, 9)
    e_cc = np.sqrt(((cc_d - cc_r) ** 2).sum(axis=(1, 2))).max() / np.sqrt((cc_d ** 2).sum(axis=(1, 2))).max()
    e_pp = np.sqrt(((dense["pp"] - ref["pp"]) ** 2).sum(axis=(1, 2))).max() / np.sqrt((dense["pp"] ** 2).sum(axis=(1, 2))).max()
    print("COV schur[%s,%d] cond(H) %.3e" % (case, seed, dense["cond"]))
    print("COV schur[%s,%d] camera_blocks %.3e %.1e" % (case, seed, e_cc, bound))
    print("COV schur[%s,%d] point_blocks %.3e %.1e" % (case, seed, e_pp, bound))
    assert e_cc <= bound and e_pp <= bound
    fc, fp = CC.free_sets(po, cm, pf)
    assert not ref["cc"][~fc].any() and not ref["cc"][:, ~fc].any() and not ref["pp"][~fp].any()  # fixed parameters: exactly 0
    assert not dense["cc"][~fc].any() and not dense["pp"][~fp].any()
    for blk in ref["pp"][fp]:
        np.linalg.cholesky((blk + blk.T) / 2)


def test_quad_reduced_handles_fixed_points(ba, O):
    """cov_checks.quad_reduced at lam = 0 with fixed points (their observations ride on one extra point that subtracts nothing) equals
    the numpy S of the formulas to fp64 roundoff, and the plain referee call where no point is fixed."""
    pg, po, Jc, Jp = _small(ba, O, 3)
    cm, pf = pg.gauge_mask(0), np.zeros(pg.M, np.uint8)
    pf[[5, 17]] = 1
    ev = np.linalg.eigvalsh(CC.point_blocks(po, Jc, Jp, 0.0)[0])
    pf[ev[:, 0] <= 1e-10 * ev[:, 2]] = 1  # (rank-2 U_p of twice-seen outlier points: no inverse at lam = 0, held fixed too)
    fc, fp = CC.free_sets(po, cm, pf)
    Jcm, Jpm = CC.mask_jacobian(po, Jc, Jp, cm, pf)
    Sq = CC.quad_reduced(O, O.CHOLESKY, po, Jcm, Jpm, 0.0, fp)
    Sn = CC.reduced_matrix(po, Jcm, Jpm, 0.0, fp)
    assert np.isfinite(Sq).all()
    err = np.abs(Sq - Sn).max() / np.abs(Sn).max()
    print("COV quad_reduced fixed_points %.3e %.1e" % (err, 1e-13))
    assert err <= 1e-13
    assert not Sq[~fc].any() and not Sq[:, ~fc].any()


def test_header_and_binding_declare_the_covariance_entry_points(ba):
    hdr = open(os.path.join(ROOT, "include", "ba_mi355x.h")).read()
    assert re.search(r"\bint\s+ba_solver_covariance_compute\s*\(\s*ba_solver\s*\*\s*s\s*,\s*double\s+lambda\s*\)\s*;", hdr)
    assert re.search(r"\bint\s+ba_solver_covariance_get\s*\(", hdr)
    assert re.search(r"\bBA_ERR_SINGULAR\s*=\s*8\b", hdr)
    assert {"ba_solver_covariance_compute", "ba_solver_covariance_get"} <= set(ba.EXPORTS)
    assert ba.ERR_SINGULAR == 8 and "positive definite" in ba.error_string(8)
    assert hasattr(ba.Solver, "covariance")


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not available")
def test_covariance_kernels_do_not_spill(tmp_path):
    """The new kernels cross-compiled for gfx950 with csrc/Makefile's own flags: no scratch, and the rank-D update keeps at least two
    waves per SIMD."""
    import qr_harness as QH
    hipcc, flags = QH.makefile_flags()
    out = subprocess.run([hipcc] + flags + ["-w", "-I", QH.CSRC, "--cuda-device-only", "-c", os.path.join(ROOT, "tests", "cov_resources.hip"), "-o",
                          str(tmp_path / "cov.o"), "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    usage = {}
    for m in re.finditer(r"Function Name: (\S+)", out.stderr):
        block = out.stderr[m.end():m.end() + 2500]
        get = lambda pat: int(re.search(pat, block).group(1))  # noqa: E731
        usage[m.group(1)] = dict(vgpr=get(r"VGPRs: (\d+)"), agpr=get(r"AGPRs: (\d+)"), occ=get(r"Occupancy \[waves/SIMD\]: (\d+)"),
                                 spill=get(r"VGPRs Spill: (\d+)"), scratch=get(r"ScratchSize \[bytes/lane\]: (\d+)"))
    cov = {k: v for k, v in usage.items() if "k_cov_" in k}
    for k, v in sorted(cov.items()):
        print("COV resources %s %s" % (k, v))
    assert len(cov) == 9, sorted(usage)
    for k, v in cov.items():
        assert v["spill"] == 0 and v["scratch"] == 0, (k, v)
    syrk = [v for k, v in cov.items() if "k_cov_syrk" in k]
    assert syrk and syrk[0]["occ"] >= 2, syrk
