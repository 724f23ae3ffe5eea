"""Measurements of the PCG's model-decrease stopping rule (ba_solver_set_pcg_model_tol; profiles/r22_pcg_model_stop_measure.txt, DESIGN.md
section 20).  Not asserted.

    python scripts/pcg_model_stop_measure.py [--problems cfg4,cfg5,n70k] [--parent DIR] [--rounds 3] [--out profiles/r22_pcg_model_stop_measure.txt]

One MI355X, ITERSCHUR fp64, the stand-ins of config 4 (synthetic(257, 65132, 225911, 1004)) and config 5 (synthetic(1024, 500000,
4000000, 1005)) and n70k = synthetic(70000, 280000, 1120000, 70000).

  (a) cost per iteration   ms per PCG iteration by DESIGN.md section 18's method -- (ms per trial of ba_minimize's replayed graph with the cap
                           at 40 iterations - at 20) / 20, tolerances never met -- with the rule off (eta = 0), with the rule on and never
                           firing (eta = 1e-300), and of a built checkout of the parent commit (--parent); one process per library,
                           alternated --rounds times, so that the parent's own run-to-run spread stands next to the difference
                           (--caps 10,5 for the two stand-ins: their solves converge to rounding level inside 40 iterations, and zeta_k <= 0
                           then ends them at any eta)
  (b) effect of the rule   ms per trial, PCG iterations per trial and the energy after 20 trials of ba_minimize with the defaults and with
                           eta = 0.1, and which rule ended the solves
"""
import argparse
import json
import os
import subprocess
import sys

PROBLEMS = {"cfg4": (257, 65132, 225911, 1004), "cfg5": (1024, 500000, 4000000, 1005), "n70k": (70000, 280000, 1120000, 70000)}
HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_out = None


def say(line):
    print(line, flush=True)
    if _out:
        _out.write(line + "\n")
        _out.flush()


def load(root):
    sys.path.insert(0, root)
    import bundleadjustment_benchmarks_amd as ba
    return ba


def graph_trial_ms(ba, s, cams, pts, cap):
    s.set_pcg(cap, 1e-30)
    s.set_state(cams, pts)
    s.minimize(max_trials=2)  # (captures the graph of this cap)
    s.set_state(cams, pts)
    s.timing(reset=True)
    s.minimize(max_trials=6)
    t = s.timing()
    return t["trial_ms"] / max(t["n_trials"], 1)


def worker(root, problems, caps):
    """One JSON line per (problem, eta): ms per iteration of the replayed graph and of eager launches (ba_solver_time_phase(4) at the first
    trial's lambda), and how many of the timed solves the rule ended after all (zeta <= 0 fires it at any eta: a solve that has converged to
    rounding level inside the cap).  eta = 1e-300 only where the library has the rule."""
    ba = load(root)
    for tag in problems:
        p = ba.Problem.synthetic(*PROBLEMS[tag])
        s = ba.Solver(p, ba.ITERSCHUR, ba.F64)
        cams, pts = s.get(ba.GET_CAMS), s.get(ba.GET_POINTS)
        for eta in (0.0, 1e-300) if hasattr(s, "set_pcg_model_tol") else (0.0,):
            fired = 0
            if eta:
                s.set_pcg_model_tol(eta)
                s.pcg_stop_stats(reset=True)
            ms = (graph_trial_ms(ba, s, cams, pts, caps[0]) - graph_trial_ms(ba, s, cams, pts, caps[1])) / (caps[0] - caps[1])
            if eta:
                fired = s.pcg_stop_stats()["by_model"]
            s.set_state(cams, pts)
            e, dmax = s.linearize()
            s.try_step(1e-12 * dmax)  # (phase 4 replays the solve on the records of the last elimination: make them this lambda's)
            ph = {}
            for cap in caps:
                s.set_pcg(cap, 1e-30)
                ph[cap] = s.time_phase(4, 5, 1e-12 * dmax)
            print(json.dumps(dict(problem=tag, eta=eta, ms_per_iteration=ms, eager_ms_per_iteration=(ph[caps[0]] - ph[caps[1]]) / (caps[0] - caps[1]),
                                  fired=fired)), flush=True)


def run_worker(root, problems, caps):
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", "--root", root, "--problems", ",".join(problems), "--caps", "%d,%d" % caps], capture_output=True,
                         text=True)
    if out.returncode:
        say(out.stderr[-2000:])
        raise SystemExit("worker of %s failed with status %d" % (root, out.returncode))
    return [json.loads(l) for l in out.stdout.splitlines() if l.startswith("{")]


def cost(problems, parent, rounds, caps):
    say("== (a) ms per PCG iteration, (cap %d - cap %d) / %d, tolerances never met: ba_minimize's replayed graph | eager launches at 1e-12 max diag J'J; "
        "one process per library, alternated" % (caps[0], caps[1], caps[0] - caps[1]))
    rows = {}
    for rnd in range(rounds):
        order = ([("parent", parent)] if parent else []) + [("tree", HERE)]
        for name, root in (order if rnd % 2 == 0 else order[::-1]):
            for r in run_worker(root, problems, caps):
                key = (r["problem"], name if r["eta"] == 0 else "tree, eta = 1e-300")
                rows.setdefault(key, []).append((r["ms_per_iteration"], r["eager_ms_per_iteration"]))
                say("round %d %-5s %-18s graph %.5f  eager %.5f ms per iteration%s" % (rnd + 1, r["problem"], key[1], r["ms_per_iteration"], r["eager_ms_per_iteration"],
                                                                                     "  (the rule ended %d of the graph's solves)" % r["fired"] if r["fired"] else ""))
    med = lambda v: sorted(v)[len(v) // 2]
    for tag in problems:
        for q, how in enumerate(("graph", "eager")):
            base = [v[q] for v in rows.get((tag, "parent"), [])]
            off, on = [v[q] for v in rows[(tag, "tree")]], [v[q] for v in rows[(tag, "tree, eta = 1e-300")]]
            if base:
                say("%-5s %s parent       min %.5f median %.5f max %.5f (spread %.2f us, %.2f %%)" % (tag, how, min(base), med(base), max(base),
                                                                                                     1e3 * (max(base) - min(base)), 100 * (max(base) - min(base)) / med(base)))
            say("%-5s %s eta = 0      min %.5f median %.5f max %.5f%s" % (tag, how, min(off), med(off), max(off),
                                                                         "  (median - parent's: %+.2f us)" % (1e3 * (med(off) - med(base))) if base else ""))
            say("%-5s %s eta = 1e-300 min %.5f median %.5f max %.5f  (median - eta = 0's: %+.2f us, %+.2f %%)" % (tag, how, min(on), med(on), max(on), 1e3 * (med(on) - med(off)),
                                                                                                                 100 * (med(on) - med(off)) / med(off)))


def effect(problems, trials):
    ba = load(HERE)
    say("== (b) %d trials of ba_minimize, the defaults (max_iter 100, rel_tol 1e-6) against eta = 0.1" % trials)
    for tag in problems:
        p = ba.Problem.synthetic(*PROBLEMS[tag])
        for eta in (0.0, 0.1):
            s = ba.Solver(p, ba.ITERSCHUR, ba.F64)
            cams, pts = s.get(ba.GET_CAMS), s.get(ba.GET_POINTS)
            s.set_pcg_model_tol(eta)
            s.minimize(max_trials=2)  # (captures the graph)
            s.set_state(cams, pts)
            s.timing(reset=True)
            s.pcg_stats(reset=True)
            s.pcg_stop_stats(reset=True)
            r = s.minimize(max_trials=trials)
            t, st, ss = s.timing(), s.pcg_stats(), s.pcg_stop_stats()
            say("%-5s eta %-4g %.3f ms per trial, %.1f iterations per trial, energy %.9g -> %.9g after %d trials, last true residual %.1e; ended by the "
                "residual %d, the model %d, the cap %d" % (tag, eta, t["trial_ms"] / max(t["n_trials"], 1), st["total_iters"] / max(st["solves"], 1),
                                                           r["trace"][0, 2], r["energy"], r["trials"], st["last_rel_residual"], ss["by_residual"],
                                                           ss["by_model"], ss["at_cap"]))


def main():
    global _out
    ap = argparse.ArgumentParser()
    ap.add_argument("--problems", default="cfg4,cfg5,n70k")
    ap.add_argument("--parent", help="a built checkout of the parent commit")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--trials", type=int, default=20)
    ap.add_argument("--caps", default="40,20", help="the two iteration caps of (a); smaller ones where the solves converge to rounding level inside 40")
    ap.add_argument("--parts", default="a,b")
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "r22_pcg_model_stop_measure.txt"))
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--root", default=HERE, help=argparse.SUPPRESS)
    a = ap.parse_args()
    problems = [t for t in a.problems.split(",") if t]
    caps = tuple(int(v) for v in a.caps.split(","))
    if a.worker:
        return worker(a.root, problems, caps)
    _out = open(a.out, "w")
    ba = load(HERE)
    name, cus = ba.device_info()
    say("device %s (%d CUs), %s; ITERSCHUR fp64" % (name, cus, ba.lib().ba_version().decode()))
    if "a" in a.parts:
        cost(problems, a.parent, a.rounds, caps)
    if "b" in a.parts:
        effect(problems, a.trials)
    _out.close()


if __name__ == "__main__":
    main()
