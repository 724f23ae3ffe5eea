"""Measurements of Marquardt's damping (ba_solver_set_damping; profiles/r20_damping_*.txt).  Not asserted.

    python scripts/damping_measure.py isa OLD.s NEW.s [--out profiles/r20_damping_isa.txt]
    python scripts/damping_measure.py gpu [--parts bench,cost,pcg,buys,n70k,prior] [--parent DIR] [--out profiles/r20_damping_measure.txt]

isa   scripts/kernel_isa_diff.py on two device listings (hipcc ... --cuda-device-only -S) with one step in front: the kernels that
      gained the damping switch carry one more template argument and one more parameter in their symbols, so every identity
      instantiation of NEW is renamed to the symbol it had in OLD before the bodies are compared.  Prints what still differs, line by
      line, for those kernels, and kernel_isa_diff's verdict for all the others.
gpu   one MI355X:
  bench   `bench.py --gpus 1 --steps 100 --warmup 10` of this tree and of a built checkout of the parent commit (--parent), alternated
          four times, the order swapped from round to round: headline and final energy
  cost    CHOLESKY fp64 at the stand-ins of config 4 and config 5: ms per eager try_step and per replayed trial of ba_minimize under
          identity, identity with the elimination as a launch of its own (BA_NO_FUSE=1: the yardstick of the arithmetic) and Marquardt
  pcg     ITERSCHUR fp64, the same problems: ms per PCG iteration under both dampings, cap 40 minus cap 20 (section 18's method)
  buys    problem-21 and problem-39 to the reference's stop under identity (lambda0 = 1e-12 max diag) and Marquardt (lambda_init 1e-3,
          1e-4), CHOLESKY and ITERSCHUR: trials, final energy, PCG iterations
  n70k    synthetic(70 000, 280 000, 1.12 M), ITERSCHUR defaults: iterations and true residual of the first solves under both dampings
  prior   section 18's example: problem-21, three groups, a prior of the group's own information on f of camera 4 three sigma away;
          the part of the way the group's f moves at lambda = 1e-6 and 1e-2 (x max diag under identity)
"""
import argparse
import difflib
import json
import os
import re
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

TOUCHED = ("k_elim_chol", "k_schur_reduce", "k_post_reduce", "k_pcg_prec_reduce", "k_pcg_cam", "k_backsub", "k_retract_cams")
_out = None


def say(line=""):
    print(line, flush=True)
    if _out:
        _out.write(line + "\n")
        _out.flush()


# ---- isa -------------------------------------------------------------------------------------------------------------------------------------
def _base(sym):
    m = re.match(r"_Z(\d+)", sym)
    return sym[2 + len(m.group(1)):2 + len(m.group(1)) + int(m.group(1))]


def isa(old_path, new_path):
    import kernel_isa_diff as K
    old, new = K.kernels(old_path), K.kernels(new_path)
    gone = [s for s in old if s not in new]
    came = [s for s in new if s not in old]
    pairs, marq = {}, []
    for n in came:
        if _base(n) not in TOUCHED:
            if _base(n).endswith("_marq"):  # (k_prior_lonely_marq: a kernel of its own, k_prior_lonely is untouched)
                marq.append(n)
            continue
        # NEW = OLD with one more template argument (Lb0E: the identity instantiation, Lb1E: Marquardt) and more parameters behind OLD's
        as_old = n.replace("Lb0EEv", "Ev", 1)
        cand = [o for o in gone if _base(o) == _base(n) and as_old.startswith(o)] if "Lb0EEv" in n else []
        if cand:
            pairs[cand[0]] = n
        else:
            marq.append(n)
    say("kernels: %d old, %d new; %d symbols unchanged, %d identity instantiations renamed, %d new Marquardt instantiations"
        % (len(old), len(new), len([s for s in old if s in new]), len(pairs), len(marq)))
    unmatched = [o for o in gone if o not in pairs] + [n for n in came if n not in pairs.values() and n not in marq]
    for u in unmatched:
        say("  UNMATCHED %s" % u)
    same = [s for s in old if s in new and old[s] == new[s]]
    differ = [s for s in old if s in new and old[s] != new[s]]
    say("unchanged symbols: %d bodies identical, %d differ" % (len(same), len(differ)))
    for s in differ:
        say("  DIFFERS %s" % s)
    say("renamed identity instantiations (old symbol: what differs in the body, instruction lines and descriptor lines):")
    bad = len(differ) + len(unmatched)
    for o, n in sorted(pairs.items()):
        body = [l.replace(n, o) for l in new[n]]  # (the descriptor names its kernel)
        d = [l for l in difflib.unified_diff(old[o], body, lineterm="", n=0) if l[0] in "+-" and not l.startswith(("---", "+++"))]
        kinds = sorted({re.sub(r"0x[0-9a-f]+|\d+", "#", l[1:]) for l in d})
        only_kernarg = all(re.match(r"(s_load_dword s#, s\[#:#\], #|\.amdhsa_kernarg_size #)$", k) for k in kinds)
        say("  %-100s %s" % (o, "identical" if not d else ("%d lines: %s" % (len(d), "; ".join(l for l in d)))))
        if d and not only_kernarg:
            bad += 1
        if K.fp_histogram(old[o]) != K.fp_histogram(new[n]) or K.resources(old[o]) != K.resources(new[n]):
            say("    floating-point opcodes or resources differ")
            bad += 1
    say("new Marquardt instantiations: " + ", ".join(sorted({_base(m) for m in marq})))
    say("verdict: %s" % ("every existing instantiation's instruction stream is the parent's; the renamed ones differ in the size of the "
                         "kernel-argument segment and in the offset at which the hidden block-count argument behind it is loaded"
                         if bad == 0 else "%d kernels differ beyond that" % bad))
    return 1 if bad else 0


# ---- gpu -------------------------------------------------------------------------------------------------------------------------------------
def bench(parent, rounds=4):
    say("== bench.py --gpus 1 --steps 100 --warmup 10, tree and parent alternated")
    rows = {"tree": [], "parent": []}
    for rnd in range(rounds):
        order = (("parent", parent), ("tree", ROOT))
        for name, cwd in (order if rnd % 2 == 0 else order[::-1]):  # (who runs first changes from round to round)
            out = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "100", "--warmup", "10"], cwd=cwd, capture_output=True, text=True)
            line = [l for l in out.stdout.splitlines() if l.startswith("{")][-1]
            r = json.loads(line)
            rows[name].append(r)
            say("round %d %-6s %.2f %s (ms per step min %.4f, device ms per trial min %.4f), final energy %r (%s)"
                % (rnd + 1, name, r["value"], r["unit"], r.get("ms_per_step_min", float("nan")), r.get("trial_device_ms_min", float("nan")),
                   r["final_energy"], r.get("lm_status")))
    for name in rows:
        v = [r["value"] for r in rows[name]]
        say("%-6s headline min %.2f max %.2f" % (name, min(v), max(v)))
    e = {r["final_energy"] for n in rows for r in rows[n]}
    say("final energies %s" % ("agree to the last bit" if len(e) == 1 else "DIFFER: %r" % sorted(e)))


def _trial_ms(ba, s, cams, pts, eager_lam, trials, **lm):
    """(ms per eager try_step at eager_lam, ms per replayed trial of ba_minimize) from the same start."""
    s.set_state(cams, pts)
    s.linearize()
    s.try_step(eager_lam)
    s.timing(reset=True)
    for _ in range(10):
        s.try_step(eager_lam)
    t = s.timing()
    eager = t["trial_ms"] / max(t["n_trials"], 1)
    s.set_state(cams, pts)
    s.minimize(max_trials=2, **lm)  # (captures the graph)
    s.set_state(cams, pts)
    s.timing(reset=True)
    r = s.minimize(max_trials=trials, **lm)
    t = s.timing()
    return eager, t["trial_ms"] / max(t["n_trials"], 1), r


def cost(ba, problems):
    say("== cost of a trial, CHOLESKY fp64 (ms; eager = ba_solver_try_step, graph = a replayed trial of ba_minimize over 20 trials)")
    for tag, args in problems.items():
        p = ba.Problem.synthetic(*args)
        rows = {}
        for name, nofuse, damp in (("identity", False, 0), ("identity, BA_NO_FUSE=1", True, 0), ("Marquardt", False, 1), ("Marquardt, BA_NO_FUSE=1", True, 1)):
            if nofuse:
                os.environ["BA_NO_FUSE"] = "1"
            else:
                os.environ.pop("BA_NO_FUSE", None)
            s = ba.Solver(p, ba.CHOLESKY, ba.F64)
            cams, pts = s.get(ba.GET_CAMS), s.get(ba.GET_POINTS)
            _, dmax = s.linearize()
            s.set_damping(damp)
            lm = dict(lambda_init=1e-3) if damp else {}
            e, g, r = _trial_ms(ba, s, cams, pts, 1e-3 if damp else 1e-9 * dmax, 20, **lm)
            ph = s.time_phase(2, 20, 1e-3 if damp else 1e-9 * dmax)
            rows[name] = (e, g)
            say("%s %-26s eager %.4f  graph %.4f  elimination alone %.4f | %d trials, %d accepted, energy %.9g"
                % (tag, name, e, g, ph, r["trials"], int(r["trace"][:, 1].sum()), r["energy"]))
            del s
        os.environ.pop("BA_NO_FUSE", None)
        say("%s    Marquardt - identity unfused (the arithmetic): eager %+.4f ms, graph %+.4f ms; identity unfused - identity (the fusion): graph %+.4f ms"
            % (tag, rows["Marquardt"][0] - rows["identity, BA_NO_FUSE=1"][0], rows["Marquardt"][1] - rows["identity, BA_NO_FUSE=1"][1],
               rows["identity, BA_NO_FUSE=1"][1] - rows["identity"][1]))


def pcg(ba, problems):
    say("== ms per PCG iteration, ITERSCHUR fp64: (time at cap 40 - time at cap 20) / 20, rel_tol never met")
    for tag, args in problems.items():
        p = ba.Problem.synthetic(*args)
        s = ba.Solver(p, ba.ITERSCHUR, ba.F64)
        cams, pts = s.get(ba.GET_CAMS), s.get(ba.GET_POINTS)
        _, dmax = s.linearize()
        out = {}
        for damp in (0, 1):
            s.set_damping(damp)
            lam = 1e-3 if damp else 1e-9 * dmax
            ph, gr = {}, {}
            for cap in (20, 40):
                s.set_pcg(cap, 1e-30)
                s.set_state(cams, pts)
                s.linearize()
                ph[cap] = s.time_phase(4, 5, lam)
                lm = dict(lambda_init=1e-3) if damp else {}
                s.set_state(cams, pts)
                s.minimize(max_trials=2, **lm)
                s.set_state(cams, pts)
                s.timing(reset=True)
                s.minimize(max_trials=6, **lm)
                t = s.timing()
                gr[cap] = t["trial_ms"] / max(t["n_trials"], 1)
            out[damp] = ((ph[40] - ph[20]) / 20, (gr[40] - gr[20]) / 20)
        say("%s identity: eager %.4f graph %.4f | Marquardt: eager %.4f graph %.4f | difference eager %+.2f us, graph %+.2f us"
            % (tag, out[0][0], out[0][1], out[1][0], out[1][1], 1e3 * (out[1][0] - out[0][0]), 1e3 * (out[1][1] - out[0][1])))


def buys(ba):
    say("== to the reference's stop: trials (accepted), final energy, PCG iterations")
    for name in ("problem-21-11315-pre.txt", "problem-39-18060-pre.txt"):
        p = ba.Problem.load_bal(os.path.join(ROOT, "data", name))
        for kind_name in ("CHOLESKY", "ITERSCHUR"):
            for label, damp, lm in (("identity, lambda0 = 1e-12 max diag", 0, {}), ("Marquardt, lambda_init 1e-3", 1, dict(lambda_init=1e-3)),
                                    ("Marquardt, lambda_init 1e-4", 1, dict(lambda_init=1e-4))):
                s = ba.Solver(p, getattr(ba, kind_name), ba.F64)
                s.set_damping(damp)
                r = s.minimize(max_trials=2000, **lm)
                it = ""
                if kind_name == "ITERSCHUR":
                    st = s.pcg_stats()
                    it = ", %d PCG iterations in %d solves" % (st["total_iters"], st["solves"])
                say("%-26s %-9s %-36s %4d trials (%3d accepted), status %s, energy %.9g, %.3f s%s"
                    % (name, kind_name, label, r["trials"], int(r["trace"][:, 1].sum()), ba.STATUS.get(r["status"], r["status"]), r["energy"], r["seconds"], it))


def n70k(ba):
    say("== synthetic(70000, 280000, 1120000), ITERSCHUR fp64, defaults (max_iter 100, rel_tol 1e-6): the first three solves")
    p = ba.Problem.synthetic(70000, 280000, 1120000, 70000)
    for label, damp, lam0 in (("identity, lambda0 = 1e-12 max diag", 0, None), ("Marquardt, lambda 1e-3", 1, 1e-3), ("Marquardt, lambda 1e-4", 1, 1e-4)):
        s = ba.Solver(p, ba.ITERSCHUR, ba.F64)
        s.set_damping(damp)
        e, dmax = s.linearize()
        lam = 1e-12 * dmax if lam0 is None else lam0
        for k in range(3):
            et, rs, dn = s.try_step(lam)
            st = s.pcg_stats()
            ok = et < e
            say("%-36s solve %d: lambda %.3e, %3d iterations, converged %d, true residual %.2e, energy %.9g -> %.9g (%s)"
                % (label, k + 1, lam, st["last_iters"], st["last_converged"], st["last_rel_residual"], e, et, "accepted" if ok else "rejected"))
            if ok:
                rho = (e - et) / rs
                lam = max(lam * max(1 - (2 * rho - 1) ** 3, 1 / 3), 1e-10)
                s.accept()
                e, _ = s.linearize()
            else:
                lam *= 2.0
        del s


def prior(ba):
    import prior_checks as PR
    import shared_checks as SH
    say("== section 18's example: problem-21, three groups of 7, 7, 7 less cameras 0 and 7; a prior on f of camera 4, three sigma away, sigma from")
    say("   the group's own information on f (so the undamped step takes the group's f about half of the way); converged solves (rel_tol 1e-13)")
    p = ba.Problem.load_bal(os.path.join(ROOT, "data", "problem-21-11315-pre.txt"))
    g = (np.arange(21) % 3).astype(np.int32)
    g[[0, 7]] = -1
    groups = SH.groups_of(21, g)
    cam = 4
    mine = [m for m in groups if cam in m][0]

    def make(with_prior, damp):
        s = ba.Solver(p, ba.ITERSCHUR, ba.F64)
        cams = s.get(ba.GET_CAMS).reshape(-1, 15).copy()
        for m in groups:
            cams[m, 12:15] = cams[m[0], 12:15]
        s.set_state(cams.ravel(), None)
        s.set_shared_intrinsics(g)
        s.linearize()
        Jc = s.get(ba.GET_JC).reshape(-1, 2, 9)
        a = p.arrays()
        order = np.argsort(a["pt_idx"], kind="stable")
        cidx = a["cam_idx"][order]
        w_f = float(np.sqrt(sum((Jc[cidx == c, :, 6] ** 2).sum() for c in mine)))
        if with_prior:
            x0 = cams[cam, 12:15].copy()
            x0[0] -= 3.0 / w_f
            PR.Priors(i_ids=[cam], i_x0=[x0], i_w=[[w_f, 0.0, 0.0]]).apply(s)
        s.set_damping(damp)
        _, dmax = s.linearize()
        s.set_pcg(20000, 1e-13)
        return s, dmax, w_f
    for label, damp in (("identity", 0), ("Marquardt", 1)):
        a, dmax, w_f = make(True, damp)
        b, _, _ = make(False, damp)
        for x in (1e-6, 1e-2):
            lam = x if damp else x * dmax
            a.try_step(lam)
            b.try_step(lam)
            da = a.get(ba.GET_DX)[3 * p.M:].reshape(-1, 9)[mine[0], 6]
            db = b.get(ba.GET_DX)[3 * p.M:].reshape(-1, 9)[mine[0], 6]
            say("%-10s lambda %.0e%s: the prior moves the group's f by %.4e of the 3 sigma it asks for (dx_f %.6e with, %.6e without; 3 sigma = %.3e; converged %d)"
                % (label, x, "" if damp else " x max diag", (da - db) / (-3.0 / w_f), da, db, 3.0 / w_f, a.pcg_stats()["last_converged"]))


def main():
    global _out
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    a = sub.add_parser("isa")
    a.add_argument("old")
    a.add_argument("new")
    a.add_argument("--out")
    b = sub.add_parser("gpu")
    b.add_argument("--parts", default="bench,cost,pcg,buys,n70k,prior")
    b.add_argument("--parent", help="a built checkout of the parent commit (bench)")
    b.add_argument("--problems", default="cfg4,cfg5")
    b.add_argument("--out")
    args = ap.parse_args()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        _out = open(args.out, "w")
    if args.cmd == "isa":
        return isa(args.old, args.new)
    import bundleadjustment_benchmarks_amd as ba
    name, cus = ba.device_info()
    say("device %s (%d CUs), %s" % (name, cus, ba.version() if hasattr(ba, "version") else ""))
    all_problems = {"cfg4": (257, 65132, 225911, 1004), "cfg5": (1024, 500000, 4000000, 1005)}
    problems = {k: all_problems[k] for k in args.problems.split(",") if k}
    parts = args.parts.split(",")
    if "bench" in parts:
        if not args.parent:
            ap.error("bench needs --parent")
        bench(args.parent)
    if "cost" in parts:
        cost(ba, problems)
    if "pcg" in parts:
        pcg(ba, problems)
    if "buys" in parts:
        buys(ba)
    if "n70k" in parts:
        n70k(ba)
    if "prior" in parts:
        prior(ba)
    return 0


if __name__ == "__main__":
    sys.exit(main())
