"""Measurements of the measurement model (ba_solver_set_loss / ba_solver_set_obs_weights; profiles/r09_loss_measure.txt, DESIGN.md
section 12).  Not asserted.

    python scripts/loss_measure.py [--reps 200] [--steps 20] [--out FILE.json] [--skip-cfg5]

Every figure is against the default path (the reference's psi at 0.5 px, no weights: the MODEL = false instantiations of k_eval) of the
same tree, on ONE solver whose model is switched between the variants: each loss (REFERENCE at 2 px; TRIVIAL; HUBER 1 px; CAUCHY 1 px) without and with weights in [0.25, 4].

  1. Config 4's stand-in (synthetic(257, 65132, 225911, 1004), CHOLESKY fp64) at the file's state: ba_solver_time_phase 0 (the
     residual-only evaluation of every trial), 1 (linearisation + gradient) and 8 (the fused linearisation behind an accepted step),
     ms per launch, and the device ms of a whole ba_solver_try_step at lambda0 (ba_timing, mean of --steps).
  2. The same at config 5's stand-in (synthetic(1024, 500000, 4000000, 1005)), a tenth of the repetitions.
  3. problem-21, CHOLESKY fp64, run to the reference's stop (at most 3000 trials: `Running` marks a run the cap ended) under each
     variant: trials, status and the final sum rho.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bundleadjustment_benchmarks_amd as ba  # noqa: E402

VARIANTS = [("default", ba.LOSS_REFERENCE, 0.5, False)]
for _name, _kind, _scale in (("reference2", ba.LOSS_REFERENCE, 2.0), ("trivial", ba.LOSS_TRIVIAL, 1.0), ("huber1", ba.LOSS_HUBER, 1.0),
                             ("cauchy1", ba.LOSS_CAUCHY, 1.0)):
    VARIANTS += [(_name, _kind, _scale, False), (_name + "+w", _kind, _scale, True)]
VARIANTS.append(("default+w", ba.LOSS_REFERENCE, 0.5, True))


def weights(K):
    return np.random.default_rng(17).uniform(0.25, 4.0, K)


def timings(p, reps, steps):
    s = ba.Solver(p, ba.CHOLESKY, ba.F64)
    w = weights(p.K)
    out = {}
    for rnd in range(2):  # (round 0 warms every instantiation up; round 1 is kept)
        for name, kind, scale, weighted in VARIANTS:
            s.set_loss(kind, scale)
            s.set_obs_weights(w if weighted else None)
            _, dmax = s.linearize()
            lam = 1e-12 * dmax
            s.try_step(lam)
            row = {"phase%d" % ph: s.time_phase(ph, reps if rnd else 3, lam) for ph in (0, 1, 8)}
            s.linearize()
            s.timing(reset=True)
            for _ in range(steps if rnd else 1):
                s.try_step(lam)
            t = s.timing()
            row["trial_ms"] = t["trial_ms"] / t["n_trials"]
            row["test_eval_ms"] = t["test_eval_ms"] / t["n_trials"]
            out[name] = row
    return out


def report(tag, rows):
    base = rows["default"]
    for name, row in rows.items():
        print("%s %-13s " % (tag, name) + "  ".join("%s %.4f ms (%+.2f %%)" % (k, row[k], 100 * (row[k] / base[k] - 1))
                                                    for k in ("phase0", "phase1", "phase8", "test_eval_ms", "trial_ms")), flush=True)


def to_the_stop(p, cap=3000):
    out = {}
    w = weights(p.K)
    for name, kind, scale, weighted in VARIANTS:
        s = ba.Solver(p, ba.CHOLESKY, ba.F64)
        s.set_loss(kind, scale)
        s.set_obs_weights(w if weighted else None)
        e0, _ = s.linearize()
        r = s.minimize(max_trials=cap)
        out[name] = dict(trials=r["trials"], accepted=int(r["trace"][:, 1].sum()), status=ba.STATUS[r["status"]], energy0=e0, energy=r["energy"],
                         mean_err_px=s.stats()["mean_err"])
        print("problem-21 %-13s trials %4d (accepted %4d) %-18s sum rho %.6f -> %.6f; mean reprojection error %.4f px"
              % (name, r["trials"], out[name]["accepted"], out[name]["status"], e0, r["energy"], out[name]["mean_err_px"]), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip-cfg5", action="store_true")
    a = ap.parse_args()
    out = {"device": ba.device_info()[0]}
    print("device: %s; phases: ba_solver_time_phase, mean of %d launches; trial: ba_timing over %d try_step; (%% against `default`)"
          % (out["device"], a.reps, a.steps), flush=True)
    out["cfg4"] = timings(ba.Problem.synthetic(257, 65132, 225911, 1004), a.reps, a.steps)
    report("cfg4", out["cfg4"])
    if not a.skip_cfg5:
        out["cfg5"] = timings(ba.Problem.synthetic(1024, 500000, 4000000, 1005), max(a.reps // 10, 3), max(a.steps // 10, 2))
        report("cfg5", out["cfg5"])
    out["problem21"] = to_the_stop(ba.Problem.load_bal(os.path.join(ROOT, "data", "problem-21-11315-pre.txt")))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
