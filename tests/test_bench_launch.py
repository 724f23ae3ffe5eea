"""bench.py's own launcher for --gpus N: started plain, it must start N rank processes before making any GPU
call, let them meet, print ONE JSON line from rank 0, and fail loudly -- non-zero exit code, the failing rank's stderr -- when a rank
fails.  No GPU here: --dry-launch stops behind the rendezvous; the failure case uses the ranks' own "no MI355X" exit.  The gpu-marked
test at the end pins --steps and --dump-outputs on the solver itself."""
import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT

BENCH = os.path.join(ROOT, "bench.py")


def run(*argv, env=None):
    e = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        e.pop(k, None)
    e.update(env or {})
    return subprocess.run([sys.executable, BENCH] + list(argv), capture_output=True, text=True, timeout=300, env=e)


def test_plain_start_launches_its_own_ranks_and_they_meet():
    out = run("--gpus", "2", "--dry-launch")
    assert out.returncode == 0, out.stderr
    lines = [w for w in out.stdout.splitlines() if w.startswith("{")]
    assert len(lines) == 1, out.stdout  # one JSON line, from rank 0
    d = json.loads(lines[0])
    assert d == {"dry_launch": True, "n_gpus": 2, "ranks_met": [0, 1], "distinct_processes": 2}


def test_three_ranks_meet_under_torch_distributed_run_too():
    e = dict(os.environ)
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "3", "--master-addr", "127.0.0.1",
                          "--master-port", "29533", BENCH, "--gpus", "3", "--dry-launch"], capture_output=True, text=True, timeout=300, env=e)
    assert out.returncode == 0, out.stderr
    d = json.loads([w for w in out.stdout.splitlines() if w.startswith("{")][-1])
    assert d["ranks_met"] == [0, 1, 2] and d["distinct_processes"] == 3


def test_a_failing_rank_fails_the_launch_with_its_stderr():
    import torch
    if torch.cuda.is_available():
        pytest.skip("needs a box without a GPU: the ranks' failure here is their own 'no MI355X' exit")
    out = run("--gpus", "2", "--steps", "2", "--warmup", "0")
    assert out.returncode != 0
    assert "rank" in out.stderr and "exited with code" in out.stderr and "needs an MI355X" in out.stderr, out.stderr
    assert not [w for w in out.stdout.splitlines() if w.startswith("{")]  # no half-measured line


def test_world_size_mismatch_is_refused():
    out = run("--gpus", "2", "--dry-launch", env={"WORLD_SIZE": "3", "RANK": "0", "LOCAL_RANK": "0", "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": "29534"})
    assert out.returncode != 0 and "WORLD_SIZE=3" in out.stderr


@pytest.mark.gpu
def test_steps_are_exact_and_outputs_are_dumped(tmp_path):
    """--steps K times exactly K trials, also past the LM loop's own stop (cfg2 stops after ~220 trials), and --dump-outputs writes the
    last timed run's state; two runs with the same workload and steps dump the same arrays bit for bit (--regions does not matter)."""
    import numpy as np
    dumps = []
    for regions in ("1", "2"):
        d = tmp_path / ("r" + regions)
        out = run("--gpus", "1", "--workload", "cfg2", "--steps", "300", "--warmup", "2", "--regions", regions, "--no-cpu-baseline",
                  "--phase-reps", "2", "--dump-outputs", str(d))
        assert out.returncode == 0, out.stderr[-4000:]
        lines = [w for w in out.stdout.splitlines() if w.startswith("{")]
        assert len(lines) == 1, out.stdout
        r = json.loads(lines[0])
        assert r["steps"] == 300 and r["ms_per_step"] > 0
        a = {n: np.load(d / (n + ".npy")) for n in ("cams", "points", "lm_result")}
        assert all(v.dtype == np.float64 for v in a.values())
        assert a["cams"].shape == (21, 15) and a["points"].shape == (11315, 3) and a["lm_result"].shape == (5,)
        assert sum(v.nbytes for v in a.values()) <= 64 << 20
        assert np.isfinite(a["points"]).all() and a["lm_result"][0] == r["final_energy"]
        assert a["lm_result"][4] < 300, "the LM loop did not stop on its own: the restart path was not exercised"
        dumps.append(a)
    for n in dumps[0]:
        assert np.array_equal(dumps[0][n], dumps[1][n]), n


@pytest.mark.gpu
def test_a_plain_run_prints_the_headline_alone_and_full_adds_the_rest():
    """A plain run stops behind the timed regions: no phase replays, roofline or CPU baseline, which take runs of their own.  --full adds
    the replays and the roofline (the CPU baseline too, unless --no-cpu-baseline) behind the same timed trials."""
    lines = []
    for extra in ((), ("--full", "--no-cpu-baseline", "--phase-reps", "2")):
        out = run("--gpus", "1", "--workload", "cfg2", "--steps", "20", "--warmup", "2", "--regions", "1", *extra)
        assert out.returncode == 0, out.stderr[-4000:]
        got = [w for w in out.stdout.splitlines() if w.startswith("{")]
        assert len(got) == 1, out.stdout
        lines.append(json.loads(got[0]))
    plain, full = lines
    for d in lines:
        assert d["metric"] == "LM iterations/sec" and d["unit"] == "LM iterations/s" and d["higher_is_better"] is True
        assert d["dtype"] == "f64" and d["steps"] == 20 and d["ms_per_step"] > 0 and d["value"] > 0
    assert not {"roofline", "phase_replay_ms", "algorithmic_bytes", "cpu_baseline"} & set(plain), sorted(plain)
    assert {"roofline", "phase_replay_ms", "algorithmic_bytes"} <= set(full) and "cpu_baseline" not in full, sorted(full)
    assert all(v > 0 for v in full["phase_replay_ms"].values()), full["phase_replay_ms"]
    assert plain["final_energy"] == full["final_energy"]  # the same timed trials either way
