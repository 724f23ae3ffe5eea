"""Measurements of BA_PRECOND_VISIBILITY_FOREST (ba_solver_set_preconditioner; profiles/r13_visibility_measure.txt).
Not asserted.

    python scripts/visibility_measure.py [--steps 5] [--problems cfg4,cfg5,n70k] [--package-root DIR]

One MI355X, ITERSCHUR fp64, the stand-ins of config 4 (synthetic(257, 65132, 225911, 1004)) and config 5
(synthetic(1024, 500000, 4000000, 1005)) and n70k = synthetic(70000, 280000, 1120000, 70000), no constraints, at lambda = 1e-4 max diag
J'J and rel_tol 1e-10: block Jacobi against the visibility forest at max_tree 4, 8, 16, 64 and 256.  At n70k also the defaults of a new
solver (rel_tol 1e-6, at most 100 iterations), at lambda = 1e-4 and at the first trial's 1e-12 max diag J'J.

Per setting one try_step with a cap of 2000 iterations (100 for the defaults) gives the PCG iterations k of a trial; the timings are then
taken with the cap set to k (the trial converges in its last slot and no empty iteration slot is enqueued), mean of --steps trials
(ba_timing): ms per trial, schur_ms (preconditioner + rhs; the forest's edge blocks and factor included) and factor_ms (the PCG solve,
the sweeps included).  The edge kernel and the factor alone: ba_solver_time_phase 9 and 10.  Derived: one apply (both sweeps) =
factor_ms / k minus block Jacobi's factor_ms / k (the iteration is otherwise the same launches).  Host: the seconds of
set_preconditioner (co-visibility, plan, record pairs, uploads) and the growth of the process's peak resident set over that call.

--package-root DIR imports the package from DIR instead of this tree: the parent commit's library on the same box is the baseline
(it knows block Jacobi alone).
"""
import argparse
import os
import resource
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CAP, TOL, LAM = 2000, 1e-10, 1e-4
PROBLEMS = {"cfg4": (257, 65132, 225911, 1004), "cfg5": (1024, 500000, 4000000, 1005), "n70k": (70000, 280000, 1120000, 70000)}
TREES = (4, 8, 16, 64, 256)


def one(ba, tag, s, kind, max_tree, steps, lam_rel=LAM, cap=CAP, tol=TOL):
    rss0, t0 = resource.getrusage(resource.RUSAGE_SELF).ru_maxrss, time.perf_counter()
    s.set_preconditioner(kind, max_tree)
    host_s, rss1 = time.perf_counter() - t0, resource.getrusage(resource.RUSAGE_SELF).ru_maxrss
    _, dmax = s.linearize()
    lam = lam_rel * dmax
    s.set_pcg(cap, tol)
    s.try_step(lam)
    st = s.pcg_stats()
    k, conv = st["last_iters"], st["last_converged"]
    s.set_pcg(max(k, 1), tol)
    s.try_step(lam)  # (warms the launch sequence of this cap up)
    s.timing(reset=True)
    for _ in range(steps):
        s.try_step(lam)
    t, st2, info = s.timing(), s.pcg_stats(), s.preconditioner_info()
    row = dict(k=k, conv=conv, res=st2["last_rel_residual"], trial=t["trial_ms"] / t["n_trials"], schur=t["schur_ms"] / t["n_trials"],
               solve=t["factor_ms"] / t["n_trials"], info=info, edges=0.0, factor=0.0)
    name = "block Jacobi" if kind == 0 else "visibility max_tree %d" % info["max_tree"]
    line = ("%s %-24s iterations %4d converged %d true rel residual %.1e  trial %9.4f ms  schur %8.4f ms  solve %9.4f ms"
            % (tag, name, k, conv, row["res"], row["trial"], row["schur"], row["solve"]))
    if kind != 0 and info["trees"] > 0:
        row["edges"], row["factor"] = s.time_phase(9, 20, lam), s.time_phase(10, 20, lam)
        line += ("  edge kernel %.4f ms  factor %.4f ms  (trees %d, kept %d of %d, largest %d, fell back %d; host %.2f s, peak RSS + %.1f MB)"
                 % (row["edges"], row["factor"], info["trees"], info["kept"], info["kept"] + info["dropped"], info["largest_tree"],
                    info["fallback_trees"], host_s, (rss1 - rss0) / 1024.0))
    print(line, flush=True)
    return row


def derived(tag, bj, fo):
    print("%s    -> max_tree %d: one apply %.2f us, iterations x %.2f, trial x %.2f of block Jacobi's"
          % (tag, fo["info"]["max_tree"], 1e3 * (fo["solve"] / max(fo["k"], 1) - bj["solve"] / max(bj["k"], 1)), fo["k"] / max(bj["k"], 1),
             fo["trial"] / bj["trial"]), flush=True)


def measure(ba, tag, p, steps, vis):
    t0 = time.perf_counter()
    s = ba.Solver(p, ba.ITERSCHUR, ba.F64)
    print("%s: N %d M %d K %d, solver created in %.1f s" % (tag, p.N, p.M, p.K, time.perf_counter() - t0), flush=True)
    if vis is not None:
        t0 = time.perf_counter()
        pairs, w = p.covisibility()
        print("%s: co-visibility %d pairs (weight %d ... %d) in %.2f s" % (tag, len(w), w.max(), w.min(), time.perf_counter() - t0), flush=True)
    settings = [("", LAM, CAP, TOL)]
    if tag == "n70k":
        settings += [(" defaults", LAM, 100, 1e-6), (" defaults lambda0", 1e-12, 100, 1e-6)]
    for sfx, lam_rel, cap, tol in settings:
        t = tag + sfx
        bj = one(ba, t, s, 0, 0, steps, lam_rel, cap, tol)
        if vis is not None:
            for mt in TREES:
                derived(t, bj, one(ba, t, s, vis, mt, steps, lam_rel, cap, tol))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--problems", default="cfg4,cfg5,n70k")
    ap.add_argument("--package-root", default=ROOT)
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.package_root))
    import bundleadjustment_benchmarks_amd as ba
    vis = getattr(ba, "PRECOND_VISIBILITY_FOREST", None)
    name, cus = ba.device_info()
    print("device %s (%d CUs), %s, package %s, %s" % (name, cus, ba.lib().ba_version().decode(), os.path.dirname(os.path.abspath(ba.__file__)),
                                                     "visibility forest" if vis is not None else "block Jacobi alone"), flush=True)
    for tag in a.problems.split(","):
        measure(ba, tag, ba.Problem.synthetic(*PROBLEMS[tag]), a.steps, vis)


if __name__ == "__main__":
    main()
