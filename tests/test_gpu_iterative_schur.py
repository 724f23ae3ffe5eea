"""GPU: BA_ITERSCHUR -- CHOLESKY's linearisation and point elimination, then the reduced camera system S dx_c = rhs solved by block-Jacobi
preconditioned conjugate gradients without forming S (csrc/ba_pcg.hip.h).  The kind has no reference counterpart and no parity claim
with any trajectory; what is checked is that it solves the same reduced system CHOLESKY factors, to the stated tolerance, inside the
same LM loop:

  reduced rhs        GET_RHS against the quad assembly from the GPU's own J (and against CHOLESKY's GET_RHS), test_gpu_stages.py's bound
  the step           |S dx_c - rhs| / |rhs| with the quad S and rhs of the GPU's J, the PCG statistics, the back-substitution and the test
                     energy against CHOLESKY's at the same lambda
  iteration cap      max_iter iterations, not converged, finite step
  determinism        two runs, graph and eager (BA_NO_GRAPH) runs, try_step and the first trial of ba_minimize: the same bits
  full run / scale   problem-21 to the reference's stop; a problem with 70 000 cameras, beyond every dense symbol's limit
  executable         Bundle_Adjustment_IterSchur's stdout protocol

Each value is printed as `ITERSCHUR <case> <metric> <value> <bound>`.
"""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import stage_checks as SC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DATA21 = os.path.join(ROOT, "data", "problem-21-11315-pre.txt")

EPS = {0: float(np.finfo(np.float64).eps), 1: float(np.finfo(np.float32).eps)}
BA_ERR_ARG = 4


class Checker:
    """Collects (metric, value, bound), prints every one, asserts them all at the end."""

    def __init__(self, case):
        self.case, self.rows = case, []

    def __call__(self, metric, value, bound):
        self.rows.append((metric, float(value), float(bound)))
        print("ITERSCHUR %s %s %.3e %.1e" % (self.case, metric, value, bound))

    def done(self):
        bad = [r for r in self.rows if not (r[1] <= r[2])]
        assert not bad, (self.case, bad)


def sorted_oracle_problem(O, pg):
    """The oracle's view of a GPU problem in the point-sorted order of the GPU's getters (test_gpu_stages.py)."""
    a = pg.arrays()
    order = np.argsort(a["pt_idx"], kind="stable")
    return O.Problem(pg.N, pg.M, pg.K, a["cam_idx"][order], a["pt_idx"][order], a["meas"].reshape(-1, 2)[order].ravel(), a["cams9"],
                     a["pts"])


def _at_linearization(ba, pg, kind, scalar):
    s = ba.Solver(pg, kind, scalar)
    e, dmax = s.linearize()
    lin = dict(e=e, dmax=dmax, f=s.get(ba.GET_RESIDUALS), Jc=s.get(ba.GET_JC).reshape(-1, 2, 9), Jp=s.get(ba.GET_JP).reshape(-1, 2, 3),
               g=s.get(ba.GET_GRAD))
    return s, lin


def _problem(ba, name, prob21, prob39):
    return {"p21": prob21, "p39": prob39}.get(name) or ba.Problem.synthetic(60, 2400, 9600, 160)


def _rel_residual(O, S, dxc, rhs):
    num, _ = O.referee_sym_residual(S, dxc, rhs)  # |S x - b| per row, in quad
    return float(np.linalg.norm(num) / np.linalg.norm(rhs))


# ---- 1. the reduced rhs ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prob", ["p21", "p39"])
def test_reduced_rhs_matches_cholesky(ba, O, gpu_ok, prob21, prob39, prob):
    """GET_RHS of the new kind (k_pcg_prec_chunks + k_pcg_prec_reduce: the camera-sorted sums) against the quad rhs from the GPU's own J
    and residuals, and against CHOLESKY's GET_RHS (k_schur_pairs' column 9), at lambda0 and 10: the bound of test_gpu_stages.py's
    assembly check, max(10 x the fp64 oracle's error on the same J, 5e-15)."""
    ck = Checker("rhs[%s]" % prob)
    pg = _problem(ba, prob, prob21, prob39)
    po = sorted_oracle_problem(O, pg)
    it, lin = _at_linearization(ba, pg, ba.ITERSCHUR, ba.F64)
    ch, lin_c = _at_linearization(ba, pg, ba.CHOLESKY, ba.F64)
    ch.keep_intermediates(True)
    assert np.array_equal(lin["Jc"], lin_c["Jc"]) and np.array_equal(lin["f"], lin_c["f"])  # the same linearisation kernels
    for lam in (1e-12 * lin["dmax"], 10.0):
        it.try_step(lam)
        ch.try_step(lam)
        rhs_i, rhs_c = it.get(ba.GET_RHS), ch.get(ba.GET_RHS)
        R = O.referee_reduced_from_jacobian(ba.CHOLESKY, po, lin["Jc"], lin["Jp"], lin["f"], lam, want_S=False)
        st = O.step(ba.CHOLESKY, po, lin["Jc"], lin["Jp"], lin["f"], lam)
        orc = SC.assembly_errors(po, lin["Jc"], lin["f"], lam, None, st["rhs"], None, R["rhs"], lin["Jp"])["rhs"]
        bound = max(10 * orc, 5e-15)
        got = SC.assembly_errors(po, lin["Jc"], lin["f"], lam, None, rhs_i, None, R["rhs"], lin["Jp"])["rhs"]
        vs_chol = SC.assembly_errors(po, lin["Jc"], lin["f"], lam, None, rhs_i, None, rhs_c, lin["Jp"])["rhs"]
        ck("rhs@%.0e(oracle %.1e)" % (lam, orc), got, bound)
        ck("rhs_vs_cholesky@%.0e" % lam, vs_chol, bound)
    with pytest.raises(ba.BAError) as ei:
        it.get(ba.GET_S)  # no S exists
    assert ei.value.code == BA_ERR_ARG
    ck.done()


# ---- 2. the step solves the reduced system -------------------------------------------------------------------------------------------------
STEP_CASES = [(p, s) for s in (0, 1) for p in ("p21", "p39", "syn60")]


@pytest.mark.parametrize("prob,scalar", STEP_CASES, ids=["%s-%s" % (p, "f64" if s == 0 else "f32") for p, s in STEP_CASES])
def test_pcg_step_solves_the_reduced_system(ba, O, gpu_ok, prob21, prob39, prob, scalar):
    """try_step(lambda) at lambda = 1e-6, 1e-4, 1e-2 x max diag J'J with set_pcg(1000, 1e-10) (fp32: 1e-4): |S dx_c - rhs| / |rhs| with
    the quad S and rhs assembled from the GPU's own J <= 2 rel_tol; converged; the device's own |rhs - S dx_c| / |rhs| within a factor of
    2 of that; the back-substitution rows of the whole step at test_gpu_stages.py's bound; the test energy within 1e-8 (fp32: 1e-3) of
    CHOLESKY's at the two larger lambdas."""
    tol = 1e-10 if scalar == 0 else 1e-4
    ck = Checker("step[%s,%s]" % (prob, "f64" if scalar == 0 else "f32"))
    pg = _problem(ba, prob, prob21, prob39)
    po = sorted_oracle_problem(O, pg)
    it, lin = _at_linearization(ba, pg, ba.ITERSCHUR, scalar)
    it.set_pcg(1000, tol)
    ch, _ = _at_linearization(ba, pg, ba.CHOLESKY, scalar)
    for q, lam in enumerate(x * lin["dmax"] for x in (1e-6, 1e-4, 1e-2)):
        et, rs, dn = it.try_step(lam)
        st = it.pcg_stats()
        dx = it.get(ba.GET_DX)
        R = O.referee_reduced_from_jacobian(ba.CHOLESKY, po, lin["Jc"], lin["Jp"], lin["f"], lam)
        res = _rel_residual(O, R["S"], dx[3 * po.M:], R["rhs"])
        ck("rel_residual@%.0e(iters %d)" % (lam, st["last_iters"]), res, 2 * tol)
        ck("converged@%.0e" % lam, 0 if st["last_converged"] == 1 else 1, 0)
        ratio = st["last_rel_residual"] / res if res > 0 else np.inf
        ck("device_vs_host_residual@%.0e" % lam, max(ratio, 1 / ratio) if ratio > 0 else np.inf, 2.0)
        ck("backsub@%.0e" % lam, SC.backsub_errors(po, lin["Jc"], lin["Jp"], dx, lin["g"], lam), 2e-14 if scalar == 0 else 1e-5)
        assert np.isfinite(et) and np.isfinite(rs) and np.isfinite(dn)
        if q > 0:
            ec, _, _ = ch.try_step(lam)
            ck("e_test_vs_cholesky@%.0e" % lam, abs(et - ec) / ec, 1e-8 if scalar == 0 else 1e-3)
    ck.done()


# ---- 3. the iteration cap --------------------------------------------------------------------------------------------------------------------
def test_iteration_cap_holds(ba, gpu_ok, prob21):
    s, lin = _at_linearization(ba, prob21, ba.ITERSCHUR, ba.F64)
    s.set_pcg(3, 1e-14)
    et, rs, dn = s.try_step(1e-6 * lin["dmax"])
    st = s.pcg_stats()
    print("ITERSCHUR cap stats", st)
    assert st["last_iters"] == 3 and st["last_converged"] == 0, st
    assert np.isfinite(et) and np.isfinite(rs) and np.isfinite(dn) and np.all(np.isfinite(s.get(ba.GET_DX)))
    for bad in ((0, 1e-6), (10, 0.0), (10, 1.0), (10, float("nan"))):
        with pytest.raises(ba.BAError):
            s.set_pcg(*bad)
    with pytest.raises(ba.BAError):
        ba.Solver(prob21, ba.CHOLESKY, ba.F64).set_pcg(10, 1e-6)


# ---- 4. determinism and one trial sequence --------------------------------------------------------------------------------------------------
_CHILD = r"""
import sys
sys.path.insert(0, %r)
import bundleadjustment_benchmarks_amd as ba
p = ba.Problem.load_bal(%r)
r = ba.Solver(p, ba.ITERSCHUR, ba.F64).minimize(max_trials=20)
for row in r["trace"][:, :5]:
    print(" ".join(float(v).hex() for v in row))
"""


def test_deterministic_and_one_trial_sequence(ba, gpu_ok, prob21):
    """minimize(max_trials=20) twice in one process, and once more in a fresh process with BA_NO_GRAPH=1 (eager launches): the same table
    rows, bit for bit.  try_step(1e-12 max diag) and the first trial of minimize: the same trial point, bit for bit."""
    r1 = ba.Solver(prob21, ba.ITERSCHUR, ba.F64).minimize(max_trials=20)["trace"][:, :5]
    r2 = ba.Solver(prob21, ba.ITERSCHUR, ba.F64).minimize(max_trials=20)["trace"][:, :5]
    assert len(r1) == 20 and np.array_equal(r1, r2)
    env = dict(os.environ, BA_NO_GRAPH="1")
    out = subprocess.run([sys.executable, "-c", _CHILD % (ROOT, DATA21)], capture_output=True, text=True, timeout=600, env=env)
    assert out.returncode == 0, out.stderr[-2000:]
    r3 = np.array([[float.fromhex(v) for v in line.split()] for line in out.stdout.split("\n") if line.strip()])
    assert r3.shape == r1.shape and np.array_equal(r1, r3)
    a = ba.Solver(prob21, ba.ITERSCHUR, ba.F64)
    _, dmax = a.linearize()
    a.try_step(1e-12 * dmax)
    b = ba.Solver(prob21, ba.ITERSCHUR, ba.F64)
    b.minimize(max_trials=1)
    for what in (ba.GET_CAMS_TEST, ba.GET_POINTS_TEST):
        assert np.array_equal(a.get(what), b.get(what)), what


# ---- 5. a full run ----------------------------------------------------------------------------------------------------------------------------
def test_full_run_problem21(ba, gpu_ok, prob21):
    """Default PCG settings, problem-21 in fp64 to the reference's stop: Success, and a final energy within 1.02 x CHOLESKY's (the ~2 %
    spread of the reference algorithm's own final energy, profiles/r04_final_cost_ensembles.json)."""
    s = ba.Solver(prob21, ba.ITERSCHUR, ba.F64)
    r = s.minimize()
    st = s.pcg_stats()
    c = ba.Solver(prob21, ba.CHOLESKY, ba.F64).minimize()
    print("ITERSCHUR full p21: status %s trials %d energy %.9g (CHOLESKY %s, %d trials, %.9g), PCG solves %d iterations %d"
          % (ba.status_string(r["status"]), r["trials"], r["energy"], ba.status_string(c["status"]), c["trials"], c["energy"],
             st["solves"], st["total_iters"]))
    assert r["status"] == 0, r
    assert st["solves"] == r["trials"]
    assert r["energy"] <= 1.02 * c["energy"], (r["energy"], c["energy"])


# ---- 6. beyond the dense limit -------------------------------------------------------------------------------------------------------------
def test_beyond_the_dense_limit(ba, gpu_ok):
    """70 000 cameras: CHOLESKY and QRCHOL refuse on the host (camera pairs beyond 32 bits; a dense S would be 3.2 TB), ITERSCHUR
    runs five trials in under 4 GB of device memory, and every accepted step lowers the energy below the start."""
    t0 = time.time()
    p = ba.Problem.synthetic(70000, 280000, 1120000, 70000)
    for kind in (ba.CHOLESKY, ba.QRCHOL):
        with pytest.raises(ba.BAError) as ei:
            ba.Solver(p, kind, ba.F64)
        assert ei.value.code == BA_ERR_ARG
    s = ba.Solver(p, ba.ITERSCHUR, ba.F64)
    nbytes = s.device_bytes()
    t1 = time.time()
    r = s.minimize(max_trials=5)
    t2 = time.time()
    st = s.pcg_stats()
    tr = r["trace"]
    print("ITERSCHUR N=70000: device %.3f GB, create %.1f s, minimize %.2f s, trials %d, PCG iterations %d, energy %.9g -> %.9g"
          % (nbytes / 1e9, t1 - t0, t2 - t1, r["trials"], st["total_iters"], tr[0, 2], r["energy"]))
    assert nbytes < 4e9, nbytes
    assert len(tr) == 5
    e0 = tr[0, 2]
    after = list(tr[1:, 2]) + [r["energy"]]  # the energy behind each row
    for row, e in zip(tr, after):
        assert np.isfinite(e)
        if row[1]:
            assert e < e0, (row, e, e0)


# ---- 7. the executable -------------------------------------------------------------------------------------------------------------------
def test_executable_protocol(ba, O, gpu_ok):
    """bin/Bundle_Adjustment_IterSchur data/problem-21 with BA_MAX_TRIALS=5: exit 0, the header and progress lines, the statistics before
    (the start is every symbol's start: the oracle's numbers to print precision), the banner, five table rows, the closing lines and
    the statistics after -- test_gpu_configs.py::test_executable_stdout_protocol's format."""
    import re
    exe = os.path.join(ROOT, "bundleadjustment_benchmarks_amd", "bin", "Bundle_Adjustment_IterSchur")
    out = subprocess.run([exe, DATA21], capture_output=True, text=True, timeout=600, env=dict(os.environ, BA_MAX_TRIALS="5"))
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stdout.splitlines()
    po = O.load_bal(DATA21)
    st0 = O.stats(po, O.init_cams(po), po.pts)
    stat0 = ["Mean reprojection error: %g" % st0["mean_err"],
             "Inlier mean reprojection error: %g (%d / %d inliers)" % (st0["inlier_mean_err"], st0["n_inliers"], po.K),
             "True objective: %g" % st0["objective"]]
    bar = "-" * 80
    head = ["N(cameras) = 21, M(points) = 11315, K(measurements) = 36455", "Reading image measurements...", "Done.",
            "Reading cameras params...", "Done.", "Reading 3D points...", "Done."] + stat0 + [
        "############################## Backtrack LevMarq ###############################", bar,
        " Iter%15s%15s%15s%15s%15s" % ("Status", "f", "rho", "lambda", "Elapsed"), bar]
    assert len(lines) == len(head) + 5 + 3 + 3, out.stdout
    assert lines[:len(head)] == head, out.stdout
    rows = lines[len(head):len(head) + 5]
    for row in rows:
        assert re.fullmatch(r"\s+\d+\s+(Accepted|Rejected)\s+\S+\s+\S+\s+\S+\s+[0-9.e+-]+s", row) and len(row) >= 66, row
        assert re.fullmatch(r".{65}\s*[0-9.e+-]+s", row), row
    tail = lines[len(head) + 5:]
    assert tail[0] == bar
    assert re.fullmatch(r"lm\.minimize\(params\) \.\.\. [0-9.e+-]+s", tail[1]), tail[1]
    assert tail[2] == "LM finished with status: Running", tail[2]
    assert re.fullmatch(r"Mean reprojection error: \S+", tail[3]), tail[3]
    assert re.fullmatch(r"Inlier mean reprojection error: \S+ \(\d+ / 36455 inliers\)", tail[4]), tail[4]
    assert re.fullmatch(r"True objective: \S+", tail[5]), tail[5]
