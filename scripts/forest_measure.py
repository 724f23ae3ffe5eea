"""Measurements of BA_PRECOND_CONSTRAINT_FOREST (ba_solver_set_preconditioner; profiles/r12_forest_measure.txt).
Not asserted.

    python scripts/forest_measure.py [--steps 5] [--skip-cfg5]

One MI355X, ITERSCHUR fp64, the stand-ins of config 4 (synthetic(257, 65132, 225911, 1004)) and config 5
(synthetic(1024, 500000, 4000000, 1005)) at lambda = 1e-4 max diag J'J and rel_tol 1e-10:

  chain   relpose_measure.py's odometry chain (N - 1 constraints): block Jacobi against the forest at max_tree 16, 64, 256 and N
  rig     N / 4 rigs of 4 cameras, each a star (3 constraints from the rig's first camera): block Jacobi against the forest at max_tree 4

Per setting one try_step with a cap of 2000 iterations gives the PCG iterations k of a trial; the timings are then taken with the cap
set to k (set_pcg(k, 1e-10): the trial converges in its last slot and no empty iteration slot is enqueued), mean of --steps trials
(ba_timing): ms per trial, schur_ms (preconditioner + rhs, the forest's factor included) and factor_ms (the PCG solve, the sweeps
included).  Derived: the factor = schur_ms minus block Jacobi's; one apply (both sweeps) = factor_ms / k minus block Jacobi's
factor_ms / k (the iteration is otherwise the same launches).
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
from relpose_measure import chain_of  # noqa: E402

CAP, TOL, LAM = 2000, 1e-10, 1e-4


def rigs_of(p, s, chain):
    """N / 4 stars of 4 cameras with the chain's information and targets perturbed like relpose_checks.standard_constraints."""
    rng = np.random.default_rng(12)
    cam15 = s.get(ba.GET_CAMS).reshape(p.N, 15)
    pairs = np.array([(4 * g, 4 * g + k) for g in range(p.N // 4) for k in (1, 2, 3)], np.int32)
    n = len(pairs)
    R0, t0 = np.zeros((n, 3, 3)), np.zeros((n, 3))
    for q, (a, b) in enumerate(pairs):
        Rab, tab = RC.relative_pose(cam15, a, b)
        ax, dr = rng.standard_normal(3), rng.standard_normal(3)
        R0[q] = (RC.rodrigues(0.05 * ax / np.linalg.norm(ax)) @ Rab).astype(np.float64)
        t0[q] = (tab + 0.01 * np.sqrt(float((tab * tab).sum())) * dr / np.linalg.norm(dr)).astype(np.float64)
    return RC.Constraints(pairs, R0, t0, np.tile(chain.Lr[0], (n, 1, 1)), np.tile(chain.Lt[0], (n, 1, 1)))


def one(tag, s, kind, max_tree, steps):
    s.set_preconditioner(kind, max_tree)
    _, dmax = s.linearize()
    lam = LAM * dmax
    s.set_pcg(CAP, TOL)
    s.try_step(lam)
    st = s.pcg_stats()
    k, conv = st["last_iters"], st["last_converged"]
    s.set_pcg(max(k, 1), TOL)
    s.try_step(lam)  # (warms the launch sequence of this cap up)
    s.timing(reset=True)
    for _ in range(steps):
        s.try_step(lam)
    t, st2, info = s.timing(), s.pcg_stats(), s.preconditioner_info()
    row = dict(k=k, conv=conv and st2["last_converged"], res=st2["last_rel_residual"], trial=t["trial_ms"] / t["n_trials"],
               schur=t["schur_ms"] / t["n_trials"], solve=t["factor_ms"] / t["n_trials"], info=info)
    name = "block Jacobi" if kind == ba.PRECOND_BLOCK_JACOBI else "forest max_tree %d" % info["max_tree"]
    print("%s %-22s iterations %4d converged %d true rel residual %.1e  trial %9.4f ms  schur %8.4f ms  solve %9.4f ms  (trees %d, kept %d, dropped %d, "
          "largest %d, fell back %d)" % (tag, name, k, row["conv"], row["res"], row["trial"], row["schur"], row["solve"], info["trees"], info["kept"],
                                         info["dropped"], info["largest_tree"], info["fallback_trees"]), flush=True)
    return row


def derived(tag, bj, fo):
    print("%s    -> forest max_tree %d: factor %.4f ms per trial, one apply %.2f us, iterations x %.2f, trial x %.2f of block Jacobi's"
          % (tag, fo["info"]["max_tree"], fo["schur"] - bj["schur"], 1e3 * (fo["solve"] / max(fo["k"], 1) - bj["solve"] / max(bj["k"], 1)),
             fo["k"] / max(bj["k"], 1), fo["trial"] / bj["trial"]), flush=True)


def measure(tag, p, steps):
    s = ba.Solver(p, ba.ITERSCHUR, ba.F64)
    chain, info = chain_of(p, s)
    for name, cs, trees in (("chain", chain, (16, 64, 256, p.N)), ("rig", rigs_of(p, s, chain), (4,))):
        cs.apply(s)
        t = "%s %s" % (tag, name)
        print("%s: %d constraints; sigma trans %.3e rot %.3e" % (t, len(cs), info["sigma_t"], info["sigma_r"]), flush=True)
        bj = one(t, s, ba.PRECOND_BLOCK_JACOBI, 0, steps)
        for mt in trees:
            derived(t, bj, one(t, s, ba.PRECOND_CONSTRAINT_FOREST, mt, steps))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--skip-cfg5", action="store_true")
    a = ap.parse_args()
    name, cus = ba.device_info()
    print("device %s (%d CUs), %s" % (name, cus, ba.lib().ba_version().decode()), flush=True)
    measure("cfg4", ba.Problem.synthetic(257, 65132, 225911, 1004), a.steps)
    if not a.skip_cfg5:
        measure("cfg5", ba.Problem.synthetic(1024, 500000, 4000000, 1005), a.steps)


if __name__ == "__main__":
    main()
