"""Measurements of shared intrinsics (ba_solver_set_shared_intrinsics; profiles/r17_shared_intrinsics_measure.txt).
Not asserted.

    python scripts/shared_intrinsics_measure.py [--problems cfg4,cfg5,n70k] [--trials 20] [--out profiles/r17_shared_intrinsics_measure.txt]

One MI355X, ITERSCHUR fp64, the stand-ins of config 4 (synthetic(257, 65132, 225911, 1004)) and config 5 (synthetic(1024, 500000,
4000000, 1005)) and n70k = synthetic(70000, 280000, 1120000, 70000), every camera's f, k1, k2 set to camera 0's through set_state, under
three settings: no groups ("free"), one group of all cameras, groups of five consecutive cameras.

  cost of the projection   ms per PCG iteration three ways: (a) replayed graph -- ba_minimize's ms per trial with the cap at 40 iterations
                           against 20, rel_tol never met, / 20; (b) eager -- ba_solver_time_phase(4) at the same two caps, / 20; (c)
                           ba_timing.factor_ms of 20 eager try_steps at the first trial's lambda with the defaults, / their iterations
  cost in iterations       PCG iterations per trial over the first --trials trials of ba_minimize with the defaults (max_iter 100,
                           rel_tol 1e-6), the energy reached, and the iterations of one solve to rel_tol 1e-6 with a cap of 2000 at
                           lambda = 1e-4 max diag J'J
  end to end               tests/shared_checks.end_to_end: 12 frames of one physical camera, f off by 1 % at the start
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import bundleadjustment_benchmarks_amd as ba  # noqa: E402

PROBLEMS = {"cfg4": (257, 65132, 225911, 1004), "cfg5": (1024, 500000, 4000000, 1005), "n70k": (70000, 280000, 1120000, 70000)}
_out = None


def say(line):
    print(line, flush=True)
    if _out:
        _out.write(line + "\n")
        _out.flush()


def labels(N, setting):
    if setting == "free":
        return None
    if setting == "one group":
        return np.zeros(N, np.int32)
    return (np.arange(N) // 5).astype(np.int32)


def solver(p, start, setting):
    s = ba.Solver(p, ba.ITERSCHUR, ba.F64)
    s.set_state(start, None)
    s.set_shared_intrinsics(labels(p.N, setting))
    return s


def graph_trial_ms(s, start, pts, cap):
    s.set_pcg(cap, 1e-30)
    s.set_state(start, pts)
    s.minimize(max_trials=2)  # (captures the graph of this cap)
    s.set_state(start, pts)
    s.timing(reset=True)
    s.minimize(max_trials=6)
    t = s.timing()
    return t["trial_ms"] / max(t["n_trials"], 1)


def measure(tag, p, trials):
    s0 = ba.Solver(p, ba.ITERSCHUR, ba.F64)
    cams = s0.get(ba.GET_CAMS).reshape(-1, 15).copy()
    cams[:, 12:15] = cams[0, 12:15]
    start, pts = cams.ravel(), p.arrays()["pts"]
    del s0
    say("== %s: synthetic(%d, %d, %d), every camera's intrinsics set to camera 0's" % (tag, p.N, p.M, p.K))
    rows = {}
    for setting in ("free", "one group", "groups of five"):
        s = solver(p, start, setting)
        info = s.shared_intrinsics_info()
        # cost in iterations: the first trials of the production loop, defaults
        s.timing(reset=True)
        r = s.minimize(max_trials=trials)
        t, st = s.timing(), s.pcg_stats()
        per_trial, its = t["trial_ms"] / max(t["n_trials"], 1), st["total_iters"] / max(st["solves"], 1)
        # (c) factor_ms of eager try_steps at the first trial's lambda
        s.set_state(start, pts)
        e0, dmax = s.linearize()
        lam = 1e-12 * dmax
        s.try_step(lam)
        s.timing(reset=True)
        k = 0
        for _ in range(20):
            s.try_step(lam)
            k += s.pcg_stats()["last_iters"]
        tc = s.timing()
        c_ms = tc["factor_ms"] / max(k, 1)
        # one solve to 1e-6 at lambda = 1e-4 max diag J'J, cap 2000
        s.set_pcg(2000, 1e-6)
        s.try_step(1e-4 * dmax)
        one = s.pcg_stats()
        # (b) eager, (a) replayed graph: caps 40 against 20, rel_tol never met
        ph = {}
        for cap in (20, 40):
            s.set_pcg(cap, 1e-30)
            ph[cap] = s.time_phase(4, 5, lam)
        b_ms = (ph[40] - ph[20]) / 20
        a_ms = (graph_trial_ms(s, start, pts, 40) - graph_trial_ms(s, start, pts, 20)) / 20
        rows[setting] = (a_ms, b_ms, c_ms, its, one["last_iters"])
        say("%s %-14s groups %6d grouped %6d largest %6d chunks %5d device %.3f GB | ms per iteration: graph %.4f  eager %.4f  factor_ms / iterations %.4f | "
            "first %d trials: %.3f ms per trial, %.1f iterations per trial, energy %.9g -> %.9g | one solve to 1e-6 at 1e-4 max diag: %d iterations "
            "(converged %d, true residual %.1e)"
            % (tag, setting, info["groups"], info["grouped"], info["largest_group"], info["chunks"], s.device_bytes() / 1e9, a_ms, b_ms, c_ms,
               r["trials"], per_trial, its, e0, r["energy"], one["last_iters"], one["last_converged"], one["last_rel_residual"]))
    f = rows["free"]
    for setting in ("one group", "groups of five"):
        g = rows[setting]
        say("%s    -> %s: + %.2f us per iteration in the graph (x %.3f), + %.2f us eager (x %.3f); iterations per trial x %.2f, of the one solve x %.2f"
            % (tag, setting, 1e3 * (g[0] - f[0]), g[0] / f[0], 1e3 * (g[1] - f[1]), g[1] / f[1], g[3] / max(f[3], 1e-9), g[4] / max(f[4], 1)))


def main():
    global _out
    ap = argparse.ArgumentParser()
    ap.add_argument("--problems", default="cfg4,cfg5,n70k")
    ap.add_argument("--trials", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r17_shared_intrinsics_measure.txt"))
    a = ap.parse_args()
    _out = open(a.out, "w")
    name, cus = ba.device_info()
    say("device %s (%d CUs), %s; ITERSCHUR fp64; defaults max_iter 100, rel_tol 1e-6" % (name, cus, ba.lib().ba_version().decode()))
    for tag in [t for t in a.problems.split(",") if t]:
        measure(tag, ba.Problem.synthetic(*PROBLEMS[tag]), a.trials)
    import shared_checks as SH
    r = SH.end_to_end(ba)
    sh, fx = r["shared"], r["fixed"]
    say("== end to end: 12 frames of one physical camera, 400 points, 0.5 px noise (sum of squares %.6f), plain least squares, gauge fixed" % r["noise_energy"])
    say("CHOLESKY, intrinsics fixed at the truth, from the truth: energy %.6f after %d trials (%s)" % (fx["energy"], fx["trials"], ba.STATUS[fx["status"]]))
    say("ITERSCHUR, one group of 12, shared f off by 1 %% at the start: energy %.6f -> %.6f after %d trials (%s), %d PCG iterations in %d solves"
        % (sh["trace"][0, 2], sh["energy"], sh["trials"], ba.STATUS[sh["status"]], r["stats"]["total_iters"], r["stats"]["solves"]))
    say("f: true %.6f, start %.6f, recovered %.6f (relative error %.3e); members bit-equal at the end: %s"
        % (r["f_true"], r["f_start"], r["f_end"], abs(r["f_end"] / r["f_true"] - 1), r["equal"]))
    _out.close()


if __name__ == "__main__":
    main()
