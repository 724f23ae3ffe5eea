"""Measurements of the relative-pose constraints (ba_solver_set_relative_poses; profiles/r11_relpose_measure.txt).
Not asserted.

    python scripts/relpose_measure.py [--reps 200] [--steps 20] [--skip-cfg5]

One MI355X, CHOLESKY fp64, the stand-ins of config 4 (synthetic(257, 65132, 225911, 1004)) and config 5
(synthetic(1024, 500000, 4000000, 1005)) with an odometry chain (N - 1 constraints; targets and information as
tests/relpose_checks.standard_constraints sizes them).  On ONE solver, without and with the constraints:

  1. ba_solver_time_phase 1 (the separate-launch linearisation; with constraints k_relpose<LIN> + k_relpose_gather are its last launches),
     8 (the linearisation as ba_minimize runs it behind an accepted step: fused, its records stay in use) and 3 (the Schur assembly, with
     constraints followed by k_relpose_schur), ms per launch.  The new kernels per linearisation: phase 1 with minus without; per
     trial: phase 3 with minus without plus test_eval_ms of item 2 with minus without (k_relpose<false>).
  2. The device ms of a whole ba_solver_try_step at lambda0 (ba_timing; mean of --steps).
  3. ba_minimize for --steps trials: device ms per trial and per linearisation as the run reports them.
  4. BA_ITERSCHUR on the same problem: PCG iterations of a try_step at lambda = 1e-4 max diag J'J (set_pcg(1000, 1e-10)).
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bundleadjustment_benchmarks_amd as ba  # noqa: E402
import relpose_checks as RC  # noqa: E402


def chain_of(p, s):
    a = p.arrays()
    s.linearize()
    order = np.argsort(a["pt_idx"], kind="stable")
    V = np.zeros((p.N, 9))
    np.add.at(V, a["cam_idx"][order], (s.get(ba.GET_JC).reshape(-1, 2, 9) ** 2).sum(axis=1))
    cs, info = RC.standard_constraints(p.N, a["cam_idx"][order], a["pt_idx"][order], s.get(ba.GET_CAMS), V)
    n = p.N - 1  # the chain alone
    return RC.Constraints(cs.pairs[:n], cs.R0[:n], cs.t0[:n], cs.Lr[:n], cs.Lt[:n]), info


def measure(tag, p, reps, steps):
    s = ba.Solver(p, ba.CHOLESKY, ba.F64)
    cams0, pts0 = s.get(ba.GET_CAMS), p.arrays()["pts"]
    cs, info = chain_of(p, s)
    print("%s constraints: %d (odometry chain); sigma trans %.3e rot %.3e" % (tag, len(cs), info["sigma_t"], info["sigma_r"]), flush=True)
    rows = {}
    for rnd in range(2):  # (round 0 warms every instantiation up; round 1 is kept)
        for name, c in (("without", RC.Constraints()), ("with", cs)):
            c.apply(s)
            _, dmax = s.linearize()
            lam = 1e-12 * dmax
            s.try_step(lam)
            row = {"phase%d" % ph: s.time_phase(ph, reps if rnd else 3, lam) for ph in (1, 8, 3)}
            s.linearize()
            s.timing(reset=True)
            for _ in range(steps if rnd else 1):
                s.try_step(lam)
            t = s.timing()
            for k in ("trial_ms", "schur_ms", "test_eval_ms"):
                row[k] = t[k] / t["n_trials"]
            s.set_state(cams0, pts0)
            r = s.minimize(max_trials=steps)
            row["min_trial_ms"], row["min_linearize_ms"] = r["schur_ms"], r["linearize_ms"]
            s.set_state(cams0, pts0)
            rows[name] = row
    for name, row in rows.items():
        print("%s %-8s " % (tag, name) + "  ".join("%s %.4f ms" % (k, v) for k, v in row.items()), flush=True)
    w, o = rows["with"], rows["without"]
    print("%s new kernels per linearisation (phase 1 with - without): %.2f us; per trial: k_relpose_schur (phase 3) %.2f us + k_relpose<false> "
          "(test_eval) %.2f us" % (tag, 1e3 * (w["phase1"] - o["phase1"]), 1e3 * (w["phase3"] - o["phase3"]), 1e3 * (w["test_eval_ms"] - o["test_eval_ms"])),
          flush=True)
    print("%s fused linearisation behind an accepted step %.2f -> %.2f us; whole trial (try_step) %+.2f us; ba_minimize per trial %+.2f us, per "
          "linearisation %+.2f us" % (tag, 1e3 * o["phase8"], 1e3 * w["phase8"], 1e3 * (w["trial_ms"] - o["trial_ms"]),
                                      1e3 * (w["min_trial_ms"] - o["min_trial_ms"]), 1e3 * (w["min_linearize_ms"] - o["min_linearize_ms"])), flush=True)
    del s
    it = ba.Solver(p, ba.ITERSCHUR, ba.F64)
    it.set_pcg(1000, 1e-10)
    for name, c in (("without", RC.Constraints()), ("with", cs)):
        c.apply(it)
        _, dmax = it.linearize()
        it.try_step(1e-4 * dmax)
        st = it.pcg_stats()
        print("%s ITERSCHUR %-8s iterations %d converged %d true rel residual %.2e" % (tag, name, st["last_iters"], st["last_converged"], st["last_rel_residual"]),
              flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--skip-cfg5", action="store_true")
    a = ap.parse_args()
    name, cus = ba.device_info()
    print("device %s (%d CUs), %s" % (name, cus, ba.lib().ba_version().decode()), flush=True)
    measure("cfg4", ba.Problem.synthetic(257, 65132, 225911, 1004), a.reps, a.steps)
    if not a.skip_cfg5:
        measure("cfg5", ba.Problem.synthetic(1024, 500000, 4000000, 1005), max(3, a.reps // 10), max(3, a.steps // 4))


if __name__ == "__main__":
    main()
