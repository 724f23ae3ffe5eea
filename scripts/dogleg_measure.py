"""Measurements of Powell's dogleg (ba_solver_dogleg_prepare / ba_solver_try_dogleg / ba_minimize_dogleg; profiles/r27_dogleg_measure.txt,
DESIGN.md section 21).  Not asserted.

    python scripts/dogleg_measure.py [--parts cost,stop,bench] [--parent DIR] [--problems cfg4,cfg5,p21] [--out profiles/r27_dogleg_measure.txt]

one MI355X, CHOLESKY fp64:
  cost    at the stand-ins of config 4 and config 5 and on problem-21, mu = 1e-12 max diag J'J: ms per call (host clock around the
          synchronous call, 3 warm-up calls, then 20) of try_step(mu), dogleg_prepare(mu) and try_dogleg at a radius of the scaled-gradient
          and of the interpolated branch; device ms of a try_step (its own events); device ms of k_jg alone (ba_solver_time_phase 11,
          50 launches back to back) and its rate against the bytes it has to read: per observation the 20-scalar camera record, 6 scalars
          of the point block and two indices, plus the gradient once (the gathers beyond that are cache hits or they are not: not counted)
  stop    problem-21 and problem-39 to the stop, ba_minimize against ba_minimize_dogleg: trials, factorisations (LM: one per trial;
          dogleg: one per prepare), seconds, final energy, mean reprojection error
  bench   `bench.py --gpus 1 --steps 100 --warmup 10` of this tree and of a built checkout of the parent commit (--parent), alternated
          four times, the order swapped from round to round: headline and final energy
"""
import argparse
import json
import math
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 8.0e12  # MI355X: 8 TB/s
_out = None


def say(line=""):
    print(line, flush=True)
    if _out:
        _out.write(line + "\n")
        _out.flush()


def _wall_ms(call, warm=3, reps=20):
    for _ in range(warm):
        call()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        t.append(1e3 * (time.perf_counter() - t0))
    t.sort()
    return t[len(t) // 2], t[0], t[-1]


def cost(ba, problems):
    say("== cost of a call, CHOLESKY fp64, mu = 1e-12 max diag J'J (ms: median [min, max] of 20 synchronous calls on the host clock)")
    for tag, make in problems.items():
        p = make(ba)
        s = ba.Solver(p, ba.CHOLESKY, ba.F64)
        _, dmax = s.linearize()
        mu = 1e-12 * dmax
        info = s.dogleg_prepare(mu)
        sd, gn = info["alpha"] * math.sqrt(info["g2"]), math.sqrt(info["gn2"])
        rows = [("try_step(mu)", lambda: s.try_step(mu)), ("dogleg_prepare(mu)", lambda: s.dogleg_prepare(mu))]
        rows.append(("try_dogleg, scaled gradient", lambda: s.try_dogleg(0.5 * sd)))
        if sd < 0.9 * gn:
            rows.append(("try_dogleg, interpolated", lambda: s.try_dogleg(math.sqrt(sd * gn))))
        say("%s N %d M %d K %d: |dx_sd| / |dx_gn| = %.3e" % (tag, p.N, p.M, p.K, sd / gn))
        med = {}
        for name, call in rows:
            med[name], lo, hi = _wall_ms(call)
            say("%s   %-30s %8.4f [%8.4f, %8.4f]" % (tag, name, med[name], lo, hi))
        s.timing(reset=True)
        for _ in range(20):
            s.try_step(mu)
        t = s.timing()
        dev_step = t["trial_ms"] / max(t["n_trials"], 1)
        s.dogleg_prepare(mu)
        jg = s.time_phase(11, 50, mu)
        need = p.K * (26 * 8 + 8) + 8 * (3 * p.M + 9 * p.N)
        say("%s   device ms: try_step %.4f (factor %.4f); k_jg %.4f = %.0f GB/s of the %.1f MB it has to read, %.1f %% of 8 TB/s"
            % (tag, dev_step, t["factor_ms"] / max(t["n_trials"], 1), jg, need / (jg * 1e-3) / 1e9, need / 1e6, 100 * need / (jg * 1e-3) / HBM_BYTES_PER_S))
        say("%s   dogleg_prepare - try_step = %+.4f ms; try_step / try_dogleg = %.1f (scaled gradient)%s"
            % (tag, med["dogleg_prepare(mu)"] - med["try_step(mu)"], med["try_step(mu)"] / med["try_dogleg, scaled gradient"],
               ", %.1f (interpolated)" % (med["try_step(mu)"] / med["try_dogleg, interpolated"]) if "try_dogleg, interpolated" in med else ""))
        del s


def stop(ba):
    say("== to the stop, CHOLESKY fp64: ba_minimize (LM) against ba_minimize_dogleg")
    for name in ("problem-21-11315-pre.txt", "problem-39-18060-pre.txt"):
        p = ba.Problem.load_bal(os.path.join(ROOT, "data", name))
        for which in ("LM", "dogleg"):
            for rep in range(2):  # (the first run loads the code objects and, LM, captures the graphs)
                s = ba.Solver(p, ba.CHOLESKY, ba.F64)
                s.timing(reset=True)
                if which == "LM":
                    r = s.minimize(max_trials=5000)
                    trials, acc, fact, final = r["trials"], int(r["trace"][:, 1].sum()), r["trials"], r["energy"]
                    extra = "lambda %.3g" % r["lam"]
                else:
                    r, rows = s.minimize_dogleg(max_trials=5000)
                    trials, acc, fact, final = r["trials"], int(rows[:, 1].sum()), int(s.timing()["n_trials"]), r["energy"]
                    extra = "radius %.3g, %d evaluations" % (r["radius"], r["fun_evals"])
                st = s.stats()
            say("%-26s %-7s %4d trials (%4d accepted), %4d factorisations, status %-26s %.4f s, energy %.9g, mean reprojection error %.6g (%s)"
                % (name, which, trials, acc, fact, ba.STATUS.get(r["status"], r["status"]), r["seconds"], final, st["mean_err"], extra))


def bench(parent, rounds=4):
    say("== bench.py --gpus 1 --steps 100 --warmup 10, tree and parent alternated")
    rows = {"tree": [], "parent": []}
    for rnd in range(rounds):
        order = (("parent", parent), ("tree", ROOT))
        for name, cwd in (order if rnd % 2 == 0 else order[::-1]):  # (who runs first changes from round to round)
            out = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "100", "--warmup", "10"], cwd=cwd, capture_output=True, text=True)
            lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
            if not lines:
                say("round %d %-6s produced no result line (exit %d): %s" % (rnd + 1, name, out.returncode, out.stderr[-300:]))
                return
            r = json.loads(lines[-1])
            rows[name].append(r)
            say("round %d %-6s %.2f %s, final energy %r (%s)" % (rnd + 1, name, r["value"], r["unit"], r["final_energy"], r.get("lm_status")))
    for name in rows:
        v = [r["value"] for r in rows[name]]
        say("%-6s headline min %.2f max %.2f (spread %.2f %%)" % (name, min(v), max(v), 100 * (max(v) - min(v)) / min(v)))
    e = {r["final_energy"] for n in rows for r in rows[n]}
    say("final energies %s" % ("agree to the last bit" if len(e) == 1 else "DIFFER: %r" % sorted(e)))


def main():
    global _out
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="cost,stop,bench")
    ap.add_argument("--parent", help="a built checkout of the parent commit (bench)")
    ap.add_argument("--problems", default="cfg4,cfg5,p21")
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        _out = open(args.out, "w")
    import bundleadjustment_benchmarks_amd as ba
    name, cus = ba.device_info()
    say("device %s (%d CUs)" % (name, cus))
    all_problems = {"cfg4": lambda ba: ba.Problem.synthetic(257, 65132, 225911, 1004),
                    "cfg5": lambda ba: ba.Problem.synthetic(1024, 500000, 4000000, 1005),
                    "p21": lambda ba: ba.Problem.load_bal(os.path.join(ROOT, "data", "problem-21-11315-pre.txt"))}
    problems = {k: all_problems[k] for k in args.problems.split(",") if k}
    parts = args.parts.split(",")
    if "cost" in parts:
        cost(ba, problems)
    if "stop" in parts:
        stop(ba)
    if "bench" in parts:
        if not args.parent:
            ap.error("bench needs --parent")
        bench(args.parent)
    return 0


if __name__ == "__main__":
    sys.exit(main())
