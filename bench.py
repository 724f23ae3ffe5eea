#!/usr/bin/env python3
"""bench.py -- LM iterations/sec of the MI355X bundle-adjustment solver on the BASELINE.json workload.

    python bench.py --gpus N --steps K --warmup W            (N > 1: starts its own N rank processes, see launch_ranks)
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N --steps K --warmup W

The timed region -- exactly K trials between two barrier + synchronize pairs -- is run R = --regions (7) times, every time from the
restored initial parameters; `ms_per_step` / `value` are the MEDIAN region's, min / max beside them (`steps` stays the per-region count).
A region whose LM loop reaches its own stop before K trials goes on from the restored initial parameters until it has run exactly K.

--dump-outputs DIR writes, after the timed regions, what the last region's ba_minimize() leaves to its caller, as float64 .npy files:
cams.npy (N x 15, the solver's camera state), points.npy (M x 3; for N > 1 the ranks' shards gathered in point order) and
lm_result.npy ([final energy, lambda, status, iterations, trials] of the last ba_minimize() call).  The inputs are fixed by the
arguments (a BAL file or a seeded synthetic problem), so two builds can be compared output for output.

A plain run does only what the result line's headline needs: set-up, warm-up, the timed regions, the dump, the line.  --full adds, after
all of that, what takes runs of its own (N = 1 only): the per-phase HIP-event replays (`phase_replay_ms`, --phase-reps), the roofline of
the dominant kernel with the algorithmic bytes, and the CPU-oracle baseline (`cpu_baseline`, about 30 s; --no-cpu-baseline drops it).

A "step" is one Levenberg-Marquardt trial = one row of the reference's iteration table
(src/Eigen_ext/BacktrackLevMarqCholesky.h:308,322): point elimination, Schur assembly, dense LDL^T + solve,
back-substitution, retraction, the test-energy evaluation and the step control, plus (once per accepted trial) the residual /
Jacobian / gradient evaluation of the next outer iteration.  Workload (config.workload): BASELINE.json configs[3],
the configuration the metric is quoted on -- CHOLESKY solver, problem-257-65132, fp64.  The BAL file is missing
from the reference checkout (.MISSING_LARGE_BLOBS), so the seeded synthetic stand-in with the same
(N, M, K) = (257, 65132, 225911) is used unless data/problem-257-65132-pre.txt exists.

All inputs are resident in HBM before the timed region; the timed region is exactly K trials of ba_minimize().
For N > 1 the points (and their observations) are sharded over the ranks; the reduced camera system is all-reduced once per
trial by RCCL INSIDE the library (ba_solver_comm_init), enqueued on the solver's stream without a host synchronisation (strong
scaling: the problem is fixed).  torch.distributed (gloo) only carries the communicator id, the barriers and the max of the
timings.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

WORKLOADS = {
    # name: (solver kind, scalar, data file or None, (N, M, K), seed)
    "cfg4": ("CHOLESKY", "f64", "problem-257-65132-pre.txt", (257, 65132, 225911), 1004),
    "cfg2": ("QRCHOL", "f64", "problem-21-11315-pre.txt", (21, 11315, 36455), 1002),
    "cfg3": ("QRKIT", "f32", "problem-39-18060-pre.txt", (39, 18060, 63551), 1003),
    "cfg1": ("CHOLESKY", "f64", "problem-16-22106-pre.txt", (16, 22106, 83718), 1001),
    "cfg5": ("QRCHOL", "f64", None, (1024, 500000, 4000000), 1005),
}
HBM_PEAK_GBS = 8000.0   # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec (6.3 TB/s achievable)
FP64_PEAK_TF = 78.6     # AMD's public MI355X fp64 matrix/vector figure (not in the local guide; 64 cycles per v_mfma_f64_16x16x4, measured)
FP32_PEAK_TF = 157.3    # MI355X_MICROARCH.md: v_mfma_f32_16x16x4_f32, 155 TF measured


def load_problem(ba, name):
    kind, scalar, fname, dims, seed = WORKLOADS[name]
    path = os.path.join(ROOT, "data", fname) if fname else None
    if path and os.path.exists(path):
        return ba.Problem.load_bal(path), "file:data/" + fname
    return ba.Problem.synthetic(dims[0], dims[1], dims[2], seed), "synthetic(seed=%d)" % seed


def algorithmic_bytes(N, M, K, S=8):
    """algorithmic HBM bytes of one outer-iteration evaluation and of one trial's Schur solve."""
    D = 9 * N
    b_evalRJ = K * (8 + 2 * S) + 3 * M * S + 15 * N * S + 26 * K * S
    b_evalR = K * (8 + 2 * S) + 3 * M * S + 15 * N * S
    b_schur = K * (8 + 26 * S) + 2 * 27 * K * S + 2 * 9 * M * S + 3 * D * D * S + 3 * M * S + 2 * D * S
    return b_evalRJ, b_evalR, b_schur


def kernel_source_sha16():
    """sha256 over the HIP / C++ sources of the library: a PMC pass describes the kernels of ONE source state."""
    import glob
    import hashlib
    h = hashlib.sha256()
    for f in sorted(glob.glob(os.path.join(ROOT, "bundleadjustment_benchmarks_amd", "csrc", "*"))):
        if f.endswith((".hip", ".h", ".cpp", ".c")):
            h.update(os.path.basename(f).encode())
            h.update(open(f, "rb").read())
    return h.hexdigest()[:16]


PMC_ROUND = "r04"


def pmc_traffic(workload, kernel_name):
    """HBM bytes per launch of a kernel from the committed PMC passes (profiles/<round>_pmc_<workload>.json: rocprofv3 --pmc FETCH_SIZE /
    WRITE_SIZE in passes of their own -- they cannot ride on this run --, FETCH_SIZE doubled as MI355X_MICROARCH.md prescribes for
    gfx950; profiles/r03_fetch_size_control.txt shows the doubling holds for this repo's gathers too).  None when the file is absent,
    when it was collected from OTHER kernel sources than the ones this run uses (its `source_sha16`), or when it has no entry of
    exactly this kernel name (template arguments behind the name are ignored: 'k_ldlt_step' does not match 'k_ldlt_step2')."""
    try:
        doc = json.load(open(os.path.join(ROOT, "profiles", "%s_pmc_%s.json" % (PMC_ROUND, workload))))
        d = doc[workload]
    except Exception:
        return None
    if doc.get("source_sha16") != kernel_source_sha16():
        return None
    # (several instantiations of one name -- QRKIT's level-1 and upper-level kernels --: the one that moves the most bytes per launch)
    for k, v in sorted(d.items(), key=lambda kv: -kv[1].get("hbm_bytes_per_launch_fetch_x2", 0)):
        if k.split("<")[0] == kernel_name and "hbm_bytes_per_launch_fetch_x2" in v:
            return {"bytes_per_launch": v["hbm_bytes_per_launch_fetch_x2"], "raw_bytes_per_launch": v["hbm_bytes_per_launch_raw"],
                    "source": "profiles/%s_pmc_%s.json (%s, FETCH_SIZE x 2 + WRITE_SIZE; sources %s)" % (PMC_ROUND, workload, k, doc["source_sha16"])}
    return None


def with_traffic(roof, workload, kernel_name):
    """roofline.traffic = HBM bytes per launch (a number, or null without a committed PMC pass of these sources); where it comes from beside it."""
    t = pmc_traffic(workload, kernel_name)
    roof["traffic"] = t["bytes_per_launch"] if t else None
    if t:
        roof["traffic_detail"] = t
    return roof


def host_cores():
    """Cores this process may really use: the affinity mask, cut to the cgroup's CPU quota when there is one (a GPU box hands a
    16-core share of a 256-thread host to each GPU)."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        q, per = open("/sys/fs/cgroup/cpu.max").read().split()
        if q != "max":
            n = min(n, max(1, int(int(q) / int(per))))
    except Exception:
        pass
    return min(n, int(os.environ.get("BA_CPU_BASELINE_CORES", "16")))


def cpu_baseline(name, prob, budget_s=20.0):
    """The CPU oracle timed on a bounded sample of the same workload: ONE thread like the reference (no OpenMP / TBB in its build,
    clock() timing), and -- labelled as not the reference -- the same port with OpenMP on all host cores."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    import oracle_lib as O
    kind, scalar, _, _, _ = WORKLOADS[name]
    if 9 * prob.N > 4000:
        # one oracle trial costs D^3/3 flops in plain C (minutes at D = 9216): outside the 10-30 s budget of this leg
        return {"value": None, "unit": "LM iterations/s", "cores": 1, "kind": "port",
                "sample": "skipped: a single oracle trial at D = %d exceeds the CPU budget; see the cfg4 line" % (9 * prob.N)}
    a = prob.arrays()
    po = O.Problem(prob.N, prob.M, prob.K, a["cam_idx"], a["pt_idx"], a["meas"], a["cams9"], a["pts"])
    dt = np.float64 if scalar == "f64" else np.float32
    okind = {"QRKIT": O.QRKIT, "QRCHOL": O.QRCHOL, "CHOLESKY": O.CHOLESKY}[kind]

    def timed(threads, budget):
        O.set_threads(threads)
        t0 = time.perf_counter()
        O.minimize(okind, po, dtype=dt, max_trials=1)
        t1 = time.perf_counter() - t0
        n = max(2, min(50, int(budget / max(t1, 1e-3))))
        t0 = time.perf_counter()
        r = O.minimize(okind, po, dtype=dt, max_trials=n)
        el = time.perf_counter() - t0
        return len(r["trace"]), el

    ntr, el = timed(1, budget_s)
    out = {"value": ntr / el, "unit": "LM iterations/s", "cores": 1, "kind": "port",
           "sample": "first %d LM trials of the same workload by oracle/ba_oracle.c (gcc -O3, 1 thread, blocked dense LDL^T), %.1f s" % (ntr, el)}
    ncores = host_cores()
    if ncores > 1:
        ntr2, el2 = timed(ncores, budget_s / 2)
        out["all_cores"] = {"value": ntr2 / el2, "cores": ncores, "note": "the same port with OpenMP on every host core -- NOT the reference "
                            "(which is single-threaded); first %d trials, %.1f s" % (ntr2, el2)}
        O.set_threads(1)
    return out


DUMP_LIMIT_BYTES = 64 << 20


def dump_outputs(path, solver, prob, res, rank, world, dist):
    """The state the last timed ba_minimize() left on the device, as float64 .npy files under `path` (rank 0 writes)."""
    import numpy as np
    import bundleadjustment_benchmarks_amd as ba
    pts = solver.get(ba.GET_POINTS).reshape(-1, 3)
    if world > 1:
        shards = [None] * world
        dist.all_gather_object(shards, (solver.p0, pts))
        pts = np.concatenate([p for _, p in sorted(shards, key=lambda sp: sp[0])])
    if rank != 0:
        return
    out = {"cams": solver.get(ba.GET_CAMS).reshape(prob.N, 15), "points": pts,
           "lm_result": np.array([res["energy"], res["lam"], res["status"], res["iterations"], res["trials"]], np.float64)}
    total = sum(a.nbytes for a in out.values())
    if total > DUMP_LIMIT_BYTES:
        raise SystemExit("bench.py: the outputs of this workload (%d bytes) exceed the dump limit of %d" % (total, DUMP_LIMIT_BYTES))
    os.makedirs(path, exist_ok=True)
    for name, a in out.items():
        np.save(os.path.join(path, name + ".npy"), np.ascontiguousarray(a, np.float64))


def free_port():
    import socket
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        return so.getsockname()[1]


def launch_ranks(args):
    """`python bench.py --gpus N` started plain: N fresh rank processes, one per GPU, started BEFORE this process makes any GPU call
    (it never makes one: it only waits).  Rendezvous over 127.0.0.1 (MASTER_ADDR / MASTER_PORT, a free port of this host); rank 0
    prints the JSON line on this process' stdout.  If any rank fails, the others are stopped, the failing rank's stderr is shown and
    the exit code is non-zero.  A rank that does not meet the others within BA_BENCH_RENDEZVOUS_S (default 300) seconds counts as failed
    (torch.distributed's own time-out)."""
    import subprocess
    import tempfile
    n = args.gpus
    port = free_port()
    tmp = tempfile.mkdtemp(prefix="ba_bench_")
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n), MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0", BA_BENCH_CHILD="1")
        err = open(os.path.join(tmp, "rank%d.err" % r), "w+")
        procs.append((subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env,
                                       stdout=None if r == 0 else subprocess.DEVNULL, stderr=err), err))
    failed = None
    alive = set(range(n))
    while alive and failed is None:
        for r in sorted(alive):
            rc = procs[r][0].poll()
            if rc is None:
                continue
            alive.discard(r)
            if rc != 0:
                failed = (r, rc)
                break
        time.sleep(0.05)
    if failed is not None:
        for r in alive:  # the exact processes this function started
            procs[r][0].terminate()
        for r in alive:
            try:
                procs[r][0].wait(timeout=20)
            except Exception:
                procs[r][0].kill()
        r, rc = failed
        procs[r][1].seek(0)
        sys.stderr.write("bench.py: rank %d of %d exited with code %d; its stderr:\n%s\n" % (r, n, rc, procs[r][1].read()[-4000:]))
        raise SystemExit(1)
    procs[0][1].seek(0)
    sys.stderr.write(procs[0][1].read())
    raise SystemExit(0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--regions", type=int, default=7, help="timed regions of --steps trials each (median reported)")
    ap.add_argument("--workload", default="cfg4", choices=sorted(WORKLOADS))
    ap.add_argument("--full", action="store_true",
                    help="also the phase replays, the roofline and the CPU-oracle baseline, after the timed regions (N = 1)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: no CPU-oracle baseline")
    ap.add_argument("--phase-reps", type=int, default=20, help="with --full: replays per phase")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed regions, write the outputs of the last one as DIR/<name>.npy (float64)")
    ap.add_argument("--dry-launch", action="store_true",
                    help="no GPU: start the ranks, let them meet (gloo), print who met -- the launch path of --gpus N without the solver")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        launch_ranks(args)  # (does not return)
    if args.gpus != world:
        raise SystemExit("bench.py: --gpus %d but WORLD_SIZE=%d" % (args.gpus, world))

    dist = None
    if world > 1:
        import datetime
        import torch.distributed as dist
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        # control plane only: id exchange, barriers, max of the timings
        dist.init_process_group(backend="gloo", timeout=datetime.timedelta(seconds=float(os.environ.get("BA_BENCH_RENDEZVOUS_S", "300"))))
    if args.dry_launch:
        met = [None] * world
        if world > 1:
            dist.all_gather_object(met, (rank, os.getpid()))
            dist.barrier()
            dist.destroy_process_group()
        else:
            met = [(rank, os.getpid())]
        if rank == 0:
            print(json.dumps({"dry_launch": True, "n_gpus": world, "ranks_met": [m[0] for m in met], "distinct_processes": len({m[1] for m in met})}))
        return

    import torch
    import bundleadjustment_benchmarks_amd as ba
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X: the solver has no CPU path")
    if torch.cuda.device_count() <= local_rank:
        raise SystemExit("bench.py: rank %d wants GPU %d but only %d are visible" % (rank, local_rank, torch.cuda.device_count()))
    torch.cuda.set_device(local_rank)

    kind_s, scalar_s, _, _, _ = WORKLOADS[args.workload]
    kind = {"QRKIT": ba.QRKIT, "QRCHOL": ba.QRCHOL, "CHOLESKY": ba.CHOLESKY}[kind_s]
    scalar = ba.F64 if scalar_s == "f64" else ba.F32
    prob, source = load_problem(ba, args.workload)
    solver = ba.Solver(prob, kind, scalar, device=local_rank, shard_rank=rank, shard_world=world)
    if world > 1:
        ids = [ba.comm_unique_id() if rank == 0 else None]
        dist.broadcast_object_list(ids, src=0)
        solver.comm_init(ids[0])  # ncclCommInitRank inside the library: the data path's all-reduces are its own
    cam0 = solver.get(ba.GET_CAMS)
    pts0 = solver.get(ba.GET_POINTS)

    def barrier():
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    # warmup: W untimed trials, then restore the initial parameters (inputs stay resident in HBM)
    if args.warmup > 0:
        solver.minimize(max_trials=args.warmup, trace=False)

    def run_steps(k):
        """Exactly k trials from the restored start; an LM loop that stops on its own first starts again from there."""
        done, res = 0, None
        while done < k:
            if done:
                solver.set_state(cam0.reshape(prob.N, 15), pts0)
            res = solver.minimize(max_trials=k - done, trace=False)
            if res["trials"] < 1:
                raise SystemExit("bench.py: ba_minimize ran no trial (status %s)" % ba.STATUS.get(res["status"], res["status"]))
            done += res["trials"]
        return done, res

    regions = []
    for _ in range(max(args.regions, 1)):  # every region: exactly K trials from the restored start, barrier + synchronize on both sides
        solver.set_state(cam0.reshape(prob.N, 15), pts0)
        solver.timing(reset=True)
        barrier()
        t0 = time.perf_counter()
        done, res = run_steps(args.steps)
        barrier()
        el = time.perf_counter() - t0
        if world > 1:
            t = torch.tensor([el], dtype=torch.float64)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            el = float(t.item())
        tmr = solver.timing()
        regions.append((el / done, el, res, tmr, done))
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, solver, prob, res, rank, world, dist)
    order = sorted(range(len(regions)), key=lambda q: regions[q][0])
    _, el, res, tm, steps_done = regions[order[len(order) // 2]]  # the median region (all regions replay the same trials: same res)
    ms_all = [1e3 * w[0] for w in regions]
    dev_all = [w[3]["trial_ms"] / max(w[3]["n_trials"], 1) for w in regions]

    out = None
    if rank == 0:
        N, M, K = prob.N, prob.M, prob.K
        S = 8 if scalar == ba.F64 else 4
        D = 9 * N
        b_evalRJ, b_evalR, b_schur = algorithmic_bytes(N, M, K, S)
        ntr = max(tm["n_trials"], 1)
        label = kind_s + (" solver (per-point QR + dense Householder QR of J2bot; sharded: distributed TSQR, the shards' R factors are all-reduced)" if kind_s == "QRKIT" else " solver")
        out = {
            "metric": "LM iterations/sec", "value": steps_done / el, "unit": "LM iterations/s", "n_gpus": world,
            "steps": steps_done, "warmup": args.warmup, "ms_per_step": 1e3 * el / max(steps_done, 1),
            "regions": len(regions), "ms_per_step_min": min(ms_all), "ms_per_step_max": max(ms_all),
            "trial_device_ms_min": min(dev_all), "trial_device_ms_max": max(dev_all),
            "higher_is_better": True, "scaling": "strong", "vs_baseline": None,  # one fixed problem, its points sharded over the ranks
            "dtype": scalar_s, "data": "synthetic" if source.startswith("synthetic") else source,
            "config": {"workload": "%s, BAL problem-%d-%d (K=%d) %s, %s" % (label, N, M, K, source, scalar_s),
                       "sharding": "points over %d rank(s), RCCL all-reduce (inside the library) of the packed %dx%d reduced camera system per trial" % (world, D, D)
                       if world > 1 else "single GPU"},
            "schur_solve_ms": res["schur_ms"], "linearize_ms": res["linearize_ms"],
            "final_energy": res["energy"], "lm_status": ba.STATUS.get(res["status"], str(res["status"])),
            "accepted_iterations": res["iterations"] - 1,
            "trial_device_ms": tm["trial_ms"] / ntr, "comm_ms_per_trial": tm["comm_ms"] / ntr,
            # what the host adds per step on top of the device time of the trial and of the (conditional) linearisation behind it
            "host_overhead_ms_per_step": 1e3 * el / max(steps_done, 1) - (tm["trial_ms"] + tm["linearize_ms"]) / ntr,
        }
    # --full: roofline of the dominant kernel, measured live with HIP events on the solver's stream (rank 0, N=1 only)
    if args.full and world == 1:
        lam = 1e-4
        solver.set_state(cam0.reshape(prob.N, 15), pts0)
        solver.linearize(True)
        solver.try_step(lam)
        reps = args.phase_reps
        # eval_jacobian_grad: the linearisation as ba_minimize runs it behind an accepted step -- ONE pass that also sums the point part of
        # J'J / J'r and (CHOLESKY) eliminates the points for the next trial (phase 8); eliminate: the stand-alone elimination of a trial
        # behind a REJECTED one (the trial behind an accepted step does not launch it); eval_jacobian_grad_separate: the separate
        # launches of the first, host-synchronous linearisation (phase 1)
        ph = {"eval_residual": solver.time_phase(0, reps, lam), "eval_jacobian_grad": solver.time_phase(8, reps, lam),
              "eval_jacobian_grad_separate": solver.time_phase(1, reps, lam), "eliminate": solver.time_phase(2, reps, lam), "schur_assembly": solver.time_phase(3, reps, lam),
              "dense_factor": solver.time_phase(6, max(reps // 4, 2), lam), "back_sweep": solver.time_phase(7, max(reps // 4, 2), lam),
              "backsub_retract": solver.time_phase(5, reps, lam)}
        nblk = (D + 63) // 64
        flops_factor = D ** 3 / 3.0
        by_hbm = b_schur - 3 * D * D * S
        t_hbm = ph["eliminate"] + ph["schur_assembly"] + ph["backsub_retract"]
        secondary = {"bound": "hbm", "kernel": "k_elim_* + k_schur_pairs + k_schur_reduce + k_backsub", "achieved": by_hbm / (t_hbm * 1e-3) / 1e9,
                     "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": by_hbm / (t_hbm * 1e-3) / 1e9 / HBM_PEAK_GBS, "algorithmic_bytes": by_hbm, "ms": t_hbm}
        with_traffic(secondary, args.workload, "k_schur_pairs")
        if kind_s == "QRKIT":
            # the right block of this symbol is the dense Householder QR of J2bot, (2K + 3M + D) x D: 2 m D^2 flops on the vector /
            # matrix units (fp32: the same rate): per (panel, TSQR level) one k_qr_chunk launch (Householder, T factor) and one k_qr_apply
            # launch (compact-WY trailing update on the matrix cores)
            mrows = 2 * K + 3 * M + D
            flops_qr = 2.0 * mrows * D * D
            peak = FP64_PEAK_TF if S == 8 else FP32_PEAK_TF
            ach = flops_qr / (ph["dense_factor"] * 1e-3) / 1e12
            out["roofline"] = {"bound": "mfma", "kernel": "k_qr_chunk + k_qr_apply<%s> (blocked Householder QR of the dense %dx%d J2bot, TSQR panels; "
                               "peak = the fp%d matrix/vector rate)" % ("double" if S == 8 else "float", mrows, D, 8 * S),
                               "achieved": ach, "peak": peak, "unit": "TFLOP/s", "frac": ach / peak,
                               "algorithmic_flops_per_trial": flops_qr, "ms_per_trial": ph["dense_factor"], "secondary": secondary}
            with_traffic(out["roofline"], args.workload, "k_qr_apply")
        elif ph["dense_factor"] >= t_hbm:
            # k_ldlt_step (fused panel + trailing update; k_ldlt_panel for the first block column): nblk launches per trial,
            # each processing 1/nblk of the D^3/3 flops on average
            peak = FP64_PEAK_TF if S == 8 else FP32_PEAK_TF
            ach = flops_factor / (ph["dense_factor"] * 1e-3) / 1e12
            # traffic: HBM bytes need PMC passes of their own (rocprofv3 --pmc cannot ride on this run): scripts/evidence.sh collects
            # them with this same command; the line quotes the committed per-launch figure and names its file
            out["roofline"] = {"bound": "mfma", "kernel": "%s<%s,64> (fused panel + trailing update of the dense LDL^T of the %dx%d reduced camera matrix; k_ldlt_panel for the first block column)" % ("k_ldlt_step2" if D >= 3072 else "k_ldlt_step", "double" if S == 8 else "float", D, D),
                               "achieved": ach, "peak": peak, "unit": "TFLOP/s", "frac": ach / peak,
                               "launches_per_trial": nblk, "avg_launch_us": 1e3 * ph["dense_factor"] / nblk,
                               "algorithmic_flops_per_launch": flops_factor / nblk, "ms_per_trial": ph["dense_factor"],
                               "secondary": secondary}
            with_traffic(out["roofline"], args.workload, "k_ldlt_step2" if D >= 3072 else "k_ldlt_step")
        else:
            out["roofline"] = secondary
        out["phase_replay_ms"] = ph
        out["algorithmic_bytes"] = {"evalRJ": b_evalRJ, "evalR": b_evalR, "schur": b_schur}
        if not args.no_cpu_baseline:
            out["cpu_baseline"] = cpu_baseline(args.workload, prob)
    if rank == 0:
        print(json.dumps(out))
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
