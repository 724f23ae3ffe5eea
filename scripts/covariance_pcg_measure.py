"""Measurements of ba_solver_covariance_pcg (profiles/r16_covariance_pcg_measure.txt).  Not asserted.

    python scripts/covariance_pcg_measure.py [--steps 5] [--problems cfg4,cfg5,n70k] [--package-root DIR]

One MI355X, ITERSCHUR fp64, the stand-ins of config 4 (synthetic(257, 65132, 225911, 1004)) and config 5
(synthetic(1024, 500000, 4000000, 1005)) and n70k = synthetic(70000, 280000, 1120000, 70000), at lambda = 1e-4 max diag J'J.

  one column   a trial's solve: one try_step at rel_tol 1e-10 with a cap of 2000 gives its iterations k; then the cap is set to k and
               ba_timing's factor_ms (the PCG solve) of --steps trials, divided by k: ms per iteration of one column
  nine columns covariance_pcg of one camera block (cams = [N / 2]) at a rel_tol no column can meet, capped at 16 and at 48 iterations:
               (ms(48) - ms(16)) / 32 is the ms per iteration of a 9-column batch without the call's fixed part (elimination, B_a^-1,
               right-hand sides, the product behind the batch); median of --steps pairs; and the fixed part ms(16) - 16 x that
  solves       one camera block, and three points, at rel_tol 1e-6 and 1e-10 (cap 2000): iterations, unconverged, residual, device ms
  dense        at config 4 and config 5 the dense route on BA_CHOLESKY: ba_solver_covariance_compute's three phases and their sum

--package-root DIR imports the package from DIR instead of this tree: the parent commit's library on the same box gives the one-column
baseline (it has no covariance_pcg; its trial kernels are the ones this tree launches).
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CAP, LAM = 2000, 1e-4
PROBLEMS = {"cfg4": (257, 65132, 225911, 1004), "cfg5": (1024, 500000, 4000000, 1005), "n70k": (70000, 280000, 1120000, 70000)}


def one_column(ba, tag, s, lam, steps):
    s.set_pcg(CAP, 1e-10)
    s.try_step(lam)
    k = max(s.pcg_stats()["last_iters"], 1)
    s.set_pcg(k, 1e-10)
    s.try_step(lam)  # (warms the launch sequence of this cap up)
    s.timing(reset=True)
    for _ in range(steps):
        s.try_step(lam)
    t = s.timing()
    solve = t["factor_ms"] / t["n_trials"]
    print("%s one column: a trial's solve %d iterations %.4f ms -> %.4f ms per iteration (trial %.4f ms)"
          % (tag, k, solve, solve / k, t["trial_ms"] / t["n_trials"]), flush=True)
    return solve / k


def nine_columns(ba, tag, s, p, lam, steps, per1):
    cam = [p.N // 2]
    s.covariance_pcg(lam, cams=cam, max_iter=16, rel_tol=1e-30)  # (allocates the work vectors, warms the kernels up)
    per, fixed = [], []
    for _ in range(steps):
        m16 = s.covariance_pcg(lam, cams=cam, max_iter=16, rel_tol=1e-30)[2]["ms"]
        m48 = s.covariance_pcg(lam, cams=cam, max_iter=48, rel_tol=1e-30)[2]["ms"]
        per.append((m48 - m16) / 32)
        fixed.append(m16 - 16 * per[-1])
    it9 = statistics.median(per)
    print("%s nine columns: %.4f ms per iteration of a batch (min %.4f max %.4f over %d pairs), fixed part of a call %.4f ms"
          % (tag, it9, min(per), max(per), steps, statistics.median(fixed)), flush=True)
    print("%s    -> a 9-column iteration costs %.2f one-column iterations (%.4f ms each): %.2f per column"
          % (tag, it9 / per1, per1, it9 / per1 / 9), flush=True)
    pts = [0, p.M // 2, p.M - 1]
    for tol in (1e-6, 1e-10):
        for what, kw in (("one camera block", dict(cams=cam)), ("three points", dict(points=pts))):
            st = s.covariance_pcg(lam, max_iter=CAP, rel_tol=tol, **kw)[2]
            print("%s %-16s rel_tol %.0e: iterations %d (columns %d, unconverged %d) worst |b - S x| / |b| %.2e  %.4f ms"
                  % (tag, what, tol, st["max_iters"], st["columns"], st["unconverged"], st["worst_rel_residual"], st["ms"]), flush=True)
    print("%s device bytes of the solver with the work vectors: %.1f MB" % (tag, s.device_bytes() / 1e6), flush=True)


def dense(ba, tag, p, lam):
    s = ba.Solver(p, ba.CHOLESKY, ba.F64)
    s.linearize()
    s.covariance(lam, cams=[p.N // 2])
    s.covariance(lam, cams=[p.N // 2])
    t = s.covariance_timing()
    print("%s dense route (BA_CHOLESKY) compute: assembly %.4f + factorisation %.4f + inverse %.4f = %.4f ms, %.1f MB"
          % (tag, t[0], t[1], t[2], sum(t[:3]), s.device_bytes() / 1e6), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--problems", default="cfg4,cfg5,n70k")
    ap.add_argument("--package-root", default=ROOT)
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.package_root))
    import bundleadjustment_benchmarks_amd as ba
    have = hasattr(ba.Solver, "covariance_pcg")
    name, cus = ba.device_info()
    print("device %s (%d CUs), %s, package %s, %s" % (name, cus, ba.lib().ba_version().decode(), os.path.dirname(os.path.abspath(ba.__file__)),
                                                     "with covariance_pcg" if have else "one-column baseline alone"), flush=True)
    for tag in a.problems.split(","):
        p = ba.Problem.synthetic(*PROBLEMS[tag])
        t0 = time.perf_counter()
        s = ba.Solver(p, ba.ITERSCHUR, ba.F64)
        _, dmax = s.linearize()
        lam = LAM * dmax
        print("%s: N %d M %d K %d, solver created in %.1f s" % (tag, p.N, p.M, p.K, time.perf_counter() - t0), flush=True)
        per1 = one_column(ba, tag, s, lam, a.steps)
        if have:
            s.linearize()
            nine_columns(ba, tag, s, p, lam, a.steps, per1)
            if tag in ("cfg4", "cfg5"):
                del s
                dense(ba, tag, p, lam)


if __name__ == "__main__":
    main()
