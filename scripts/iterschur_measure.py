"""BA_ITERSCHUR measurements (profiles/r05_iterschur_*.txt): per problem, the first LM trials with the default PCG settings (trial time,
PCG iterations per trial), the time of one PCG iteration and of the launches left behind convergence, ba_solver_time_phase(4), and the
dense CHOLESKY trial at the same size where it exists.

    python scripts/iterschur_measure.py [cfg4|cfg5|n70k ...] [--trials 20]

Problems: cfg4 = synthetic(257, 65132, 225911, 1004) (bench.py's config-4 stand-in), cfg5 = synthetic(1024, 500000, 4000000, 1005),
n70k = synthetic(70000, 280000, 1120000, 70000).  fp64.  Times are device times (ba_timing: HIP events or the device wall clock).
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bundleadjustment_benchmarks_amd as ba  # noqa: E402

PROBLEMS = {"cfg4": (257, 65132, 225911, 1004), "cfg5": (1024, 500000, 4000000, 1005), "n70k": (70000, 280000, 1120000, 70000)}
HBM_TBS = 6.3  # achievable HBM rate (README)


def trial_ms(s):
    t = s.timing()
    return t["trial_ms"] / max(t["n_trials"], 1)


def lm_run(p, kind, trials, pcg=None):
    s = ba.Solver(p, kind, ba.F64)
    if pcg:
        s.set_pcg(*pcg)
    s.timing(reset=True)
    t0 = time.time()
    r = s.minimize(max_trials=trials)
    wall = time.time() - t0
    st = s.pcg_stats() if kind == ba.ITERSCHUR else None
    return s, r, trial_ms(s), wall, st


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("problems", nargs="*", default=["cfg4", "cfg5", "n70k"])
    ap.add_argument("--trials", type=int, default=20)
    a = ap.parse_args()
    name, cus = ba.device_info()
    print("device %s, %d CUs; defaults max_iter %d rel_tol %g" % (name, cus, 100, 1e-6))
    for key in a.problems:
        N, M, K, seed = PROBLEMS[key]
        p = ba.Problem.synthetic(N, M, K, seed)
        print("== %s: synthetic(%d, %d, %d, %d), D = %d" % (key, N, M, K, seed, 9 * N))
        s, r, tms, wall, st = lm_run(p, ba.ITERSCHUR, a.trials)
        print("ITERSCHUR default: %d trials in %.3f s wall, %.3f ms per trial (device), final energy %.9g, status %s" %
              (r["trials"], wall, tms, r["energy"], ba.status_string(r["status"])))
        print("  device bytes %.3f GB; PCG solves %d, iterations %d (%.1f per trial), last: %d iterations, converged %d, |rhs - S dx|/|rhs| %.2e" %
              (s.device_bytes() / 1e9, st["solves"], st["total_iters"], st["total_iters"] / max(st["solves"], 1), st["last_iters"],
               st["last_converged"], st["last_rel_residual"]))
        lam = r["lam"]
        # one trial's state for the phase timings: linearised, eliminated at lambda
        s.try_step(lam)
        t = s.timing(reset=True)
        s.try_step(lam)
        t = s.timing(reset=True)
        print("  try_step at lambda %.3g: eliminate %.3f ms, preconditioner + rhs %.3f ms, PCG %.3f ms (%d iterations), back-sub %.3f ms, test energy %.3f ms" %
              (lam, t["eliminate_ms"], t["schur_ms"], t["factor_ms"], s.pcg_stats()["last_iters"], t["backsub_ms"], t["test_eval_ms"]))
        ph4 = s.time_phase(4, 3, lam)
        print("  time_phase(4) (preconditioner + rhs + PCG, eager launches, defaults): %.3f ms per launch" % ph4)
        # one full iteration: max_iter 40 vs 20 at a tolerance never met
        s.set_pcg(20, 1e-30)
        t20 = s.time_phase(4, 3, lam)
        s.set_pcg(40, 1e-30)
        t40 = s.time_phase(4, 3, lam)
        it_ms = (t40 - t20) / 20
        rec_bytes = 2 * K * 32 * 8
        print("  one PCG iteration (eager): %.4f ms; records read twice %.3f GB -> %.2f TB/s (%.0f %% of %.1f TB/s)" %
              (it_ms, rec_bytes / 1e9, rec_bytes / (it_ms * 1e-3) / 1e12, 100 * rec_bytes / (it_ms * 1e-3) / 1e12 / HBM_TBS, HBM_TBS))
        # the launches behind convergence: rel_tol 0.5 converges within a few iterations; 1000 vs 100 iteration slots, graph replay
        _, r1, t100, _, st1 = lm_run(p, ba.ITERSCHUR, 5, (100, 0.5))
        _, r2, t1000, _, st2 = lm_run(p, ba.ITERSCHUR, 5, (1000, 0.5))
        print("  early-exit tail (graph): %.3f ms per trial with 100 slots, %.3f ms with 1000 (%.1f / %.1f iterations used) -> %.2f us per empty launch" %
              (t100, t1000, st1["total_iters"] / max(st1["solves"], 1), st2["total_iters"] / max(st2["solves"], 1), (t1000 - t100) * 1e3 / (900 * 4)))
        if N <= 65535 and 9 * N <= 9216:
            c, rc, tc, wc, _ = lm_run(p, ba.CHOLESKY, a.trials)
            print("CHOLESKY: %d trials in %.3f s wall, %.3f ms per trial (device), final energy %.9g; device bytes %.3f GB" %
                  (rc["trials"], wc, tc, rc["energy"], c.device_bytes() / 1e9))
        sys.stdout.flush()


if __name__ == "__main__":
    main()
