"""Measurements of ba_solver_triangulate_points (profiles/r28_triangulate_measure.txt).  Not asserted.

    python scripts/triangulate_measure.py [--parts cost,long,rescue,start,bench] [--parent DIR] [--problems cfg4,cfg5,p21] [--out FILE]

one MI355X, CHOLESKY fp64:
  cost    device ms of a call over all points (the call's own events; 2 warm-up calls, then the median of 10, the state put back
          before each) at the stand-ins of config 4 and config 5 and on problem-21, refine_iters 0 and 5, beside
          ba_solver_time_phase(0) (the linearisation) on the same solver.  Bytes it has to move: per observation 15 camera scalars and
          2 of the measurement read and 3 fp64 of the ray written and read back (the gathers beyond that are cache hits or they are
          not: not counted), plus per point two offsets, three scalars in and out and the status byte.
  long    what one long track costs: 2048 three-view points alone, and with one more point of 300 and of 1200 observations (the
          largest-chord search is O(t^2) for that point's eight lanes)
  rescue  problem-21 and problem-39 through ba_minimize to the stop, triangulate_points, ba_minimize again: status counts, energy and
          mean reprojection error before and after the call and after the second run
  start   start state of problem-21: the points with a rank-2 block (seen by two outlier observations only) and how many of them the
          call re-seats; whether covariance_compute(0) with the gauge mask succeeds before and after
  bench   `bench.py --gpus 1 --steps 100 --warmup 10` of this tree and of a built checkout of the parent commit (--parent), alternated
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 8.0e12  # MI355X: 8 TB/s
_out = None


def say(line=""):
    print(line, flush=True)
    if _out:
        _out.write(line + "\n")
        _out.flush()


def counts(ba, st):
    return ", ".join("%s %d" % (n, c) for n, c in zip(ba.TRI_NAMES, st["by_status"]) if c)


def cost(ba, problems):
    say("== device ms of triangulate_points over all points, CHOLESKY fp64 (median [min, max] of 10 calls, the state put back before each)")
    for tag, make in problems.items():
        p = make(ba)
        s = ba.Solver(p, ba.CHOLESKY, ba.F64)
        _, dmax = s.linearize()
        lin = s.time_phase(0, 20, 1e-12 * dmax)
        cam, pts = s.get(ba.GET_CAMS), s.get(ba.GET_POINTS)
        need = p.K * (17 * 8 + 4 + 2 * 24) + p.M * (8 + 6 * 8 + 1)
        say("%s N %d M %d K %d (mean track %.2f): linearisation (time_phase 0) %.4f ms; the call has to move %.1f MB" % (tag, p.N, p.M, p.K, p.K / p.M, lin, need / 1e6))
        for it in (0, 5):
            ms = []
            for rep in range(12):
                s.set_state(cam, pts)
                st, _ = s.triangulate_points(None, refine_iters=it)
                if rep >= 2:
                    ms.append(st["ms"])
            ms.sort()
            med = ms[len(ms) // 2]
            say("%s   refine_iters %d: %.4f [%.4f, %.4f] ms = %.0f GB/s, %.2f %% of 8 TB/s, %.2f x the linearisation; %s"
                % (tag, it, med, ms[0], ms[-1], need / (med * 1e-3) / 1e9, 100 * need / (med * 1e-3) / HBM_BYTES_PER_S, med / lin, counts(ba, st)))
        del s


def rescue(ba):
    say("== the case the feature exists for, CHOLESKY fp64: ba_minimize to the stop, triangulate_points (defaults), ba_minimize again")
    for name in ("problem-21-11315-pre.txt", "problem-39-18060-pre.txt"):
        p = ba.Problem.load_bal(os.path.join(ROOT, "data", name))
        for over, label in ((dict(), "defaults"), (dict(only_if_better=False, max_reproj_px=4.0), "only_if_better off, max_reproj_px 4")):
            s = ba.Solver(p, ba.CHOLESKY, ba.F64)
            r1 = s.minimize(max_trials=5000)
            e1 = s.linearize()[0]
            m1 = s.stats()["mean_err"]
            st, status = s.triangulate_points(None, **over)
            e2 = s.linearize()[0]
            m2 = s.stats()["mean_err"]
            r2 = s.minimize(max_trials=5000)
            e3 = s.linearize()[0]
            m3 = s.stats()["mean_err"]
            say("%s (%s)" % (name, label))
            say("   first run : %4d trials, status %s, energy %.9g, mean reprojection error %.6g px" % (r1["trials"], ba.STATUS.get(r1["status"], r1["status"]), e1, m1))
            say("   the call  : %.4f ms; %s" % (st["ms"], counts(ba, st)))
            say("               energy %.9g (cost sums %+.6g), mean reprojection error %.6g px" % (e2, st["cost_after"] - st["cost_before"], m2))
            say("   second run: %4d trials, status %s, energy %.9g, mean reprojection error %.6g px" % (r2["trials"], ba.STATUS.get(r2["status"], r2["status"]), e3, m3))
            del s


def long_track(ba):
    say("== one long track among short ones, CHOLESKY fp64: 2048 points of 3 observations, without and with one more point seen by every camera")
    rng = np.random.default_rng(7)
    for t in (0, 300, 1200):
        N, M = max(t, 1200), 2048 + (1 if t else 0)
        cam_idx = np.concatenate([rng.integers(0, N, 3 * 2048), np.arange(t)]).astype(np.int32)
        pt_idx = np.concatenate([np.repeat(np.arange(2048), 3), np.full(t, 2048)]).astype(np.int32)
        cams9 = np.zeros((N, 9))
        cams9[:, :3] = 0.2 * rng.standard_normal((N, 3))
        cams9[:, 3:6] = rng.standard_normal((N, 3)) + np.array([0.0, 0.0, -6.0])
        cams9[:, 6] = 800.0
        p = ba.Problem.from_arrays(N, M, len(cam_idx), cam_idx, pt_idx, 100 * rng.standard_normal(2 * len(cam_idx)), cams9.reshape(-1),
                                   0.3 * rng.standard_normal(3 * M))
        s = ba.Solver(p, ba.CHOLESKY, ba.F64)
        cam, pts = s.get(ba.GET_CAMS), s.get(ba.GET_POINTS)
        ms = []
        for rep in range(7):
            s.set_state(cam, pts)
            st, status = s.triangulate_points(None)
            if rep >= 2:
                ms.append(st["ms"])
        ms.sort()
        say("longest track %4d: %.4f [%.4f, %.4f] ms%s" % (t, ms[2], ms[0], ms[-1], "; its status: %s" % ba.TRI_NAMES[status[2048]] if t else ""))
        del s


def _outlier_only_pairs(ba, s, a, tau=0.5):
    """The points seen by exactly two observations, both beyond tau: psi gives each a rank-1 Jacobian, the point's block has rank 2."""
    cam = s.get(ba.GET_CAMS).reshape(-1, 15)[a["cam_idx"]]
    X = s.get(ba.GET_POINTS).reshape(-1, 3)[a["pt_idx"]]
    XX = np.einsum("krc,kc->kr", cam[:, :9].reshape(-1, 3, 3), X) + cam[:, 9:12]
    xu = XX[:, :2] / XX[:, 2:3]
    r2 = (xu * xu).sum(-1)
    e = (cam[:, 12] * (1 + cam[:, 13] * r2 + cam[:, 14] * r2 * r2))[:, None] * xu - a["meas"].reshape(-1, 2)
    inl = np.bincount(a["pt_idx"], weights=((e * e).sum(-1) < tau * tau).astype(float), minlength=s.problem.M)
    return (np.bincount(a["pt_idx"], minlength=s.problem.M) == 2) & (inl == 0)


def start(ba):
    say("== start state of problem-21, CHOLESKY fp64: rank-2 points and covariance_compute(0) with the gauge mask")
    p = ba.Problem.load_bal(os.path.join(ROOT, "data", "problem-21-11315-pre.txt"))
    a = p.arrays()
    s = ba.Solver(p, ba.CHOLESKY, ba.F64)
    s.set_constant(p.gauge_mask(0), None)

    def cov_ok():
        s.linearize()
        try:
            s.covariance(lam=0.0, cams=[1])
            return "succeeds"
        except ba.BAError as e:
            return "fails (%s)" % ba.error_string(e.code)

    r0 = _outlier_only_pairs(ba, s, a)
    say("before: %d of %d points are seen by two outlier observations only (rank-2 block); covariance_compute(0) %s" % (int(r0.sum()), p.M, cov_ok()))
    for over, label in ((dict(), "defaults"), (dict(only_if_better=False, max_reproj_px=4.0), "only_if_better off, max_reproj_px 4")):
        s.set_state(None, a["pts"])
        st, status = s.triangulate_points(None, **over)
        r1 = _outlier_only_pairs(ba, s, a)
        say("%s: %s" % (label, counts(ba, st)))
        say("   of the %d rank-2 points %d were re-seated; %d points are rank-2 afterwards" % (int(r0.sum()), int((status[r0] == 0).sum()), int(r1.sum())))
        say("   covariance_compute(0) %s" % cov_ok())


def bench(parent, rounds=3):
    say("== bench.py --gpus 1 --steps 100 --warmup 10, tree and parent alternated")
    rows = {"tree": [], "parent": []}
    for rnd in range(rounds):
        order = (("parent", parent), ("tree", ROOT))
        for name, cwd in (order if rnd % 2 == 0 else order[::-1]):  # (who runs first changes from round to round)
            out = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "100", "--warmup", "10"], cwd=cwd, capture_output=True, text=True)
            lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
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
    ap.add_argument("--parts", default="cost,long,rescue,start,bench")
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
    if "long" in parts:
        long_track(ba)
    if "rescue" in parts:
        rescue(ba)
    if "start" in parts:
        start(ba)
    if "bench" in parts:
        if not args.parent:
            ap.error("bench needs --parent")
        bench(args.parent)
    return 0


if __name__ == "__main__":
    sys.exit(main())
