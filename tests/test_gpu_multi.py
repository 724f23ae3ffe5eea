"""GPU: the sharded (multi-rank) path end to end on ONE device.

  * two processes, each owning half of the points, all-reducing the packed reduced camera system through the ba_allreduce_fn
    callback (gloo; RCCL refuses two ranks on one device) must reproduce the single-rank LM trajectory -- this is the product's
    sharded code path (segments, pack / unpack, energy tail, device-side step control), only the transport is the test's;
  * the production transport, RCCL inside the library (ba_solver_comm_init), on a one-rank communicator: the same sharded code
    path with ncclAllReduce enqueued on the solver's stream must reproduce the unsharded run bit for bit.
(tests/test_distributed_cpu.py pins the ARITHMETIC of the sharding with the oracle on CPU ranks; it does not touch the product.)"""
import os
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from conftest import ROOT

pytestmark = pytest.mark.gpu

NTR = 8


class DevArray:
    """Zero-copy view of device memory for torch.as_tensor (__cuda_array_interface__)."""

    def __init__(self, ptr, count, scalar):
        self.__cuda_array_interface__ = {"shape": (count,), "typestr": "<f8" if scalar == 0 else "<f4",
                                         "data": (ptr, False), "version": 2, "strides": None}


def _worker(rank, world, port, kind, out_q):
    sys.path.insert(0, ROOT)
    if kind >= 10:  # 13: MOREQR's normal-equations variant (BA_MOREQR_QR=0); 3 is the QR-only default: the shards' R factors meet in the TSQR stack, twice per accepted step
        os.environ["BA_MOREQR_QR"] = "0"
        kind -= 10
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch.distributed as dist
    import bundleadjustment_benchmarks_amd as ba
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.cuda.set_device(0)
        dev = torch.device("cuda", 0)
        p = ba.Problem.synthetic(24, 3000, 10500, 77)
        s = ba.Solver(p, kind, ba.F64, device=0, shard_rank=rank, shard_world=world)
        stream = torch.cuda.current_stream()
        s.set_stream(stream.cuda_stream)

        ops = []

        def collective(ptr, count, scalar, op, strm):
            """The callback ABI of include/ba_mi355x.h with all four op codes (gloo on host copies; RCCL refuses two ranks on one device)."""
            code, root = op & 0xff, op >> 8
            ops.append(code)
            n = count * world if code == 3 else count  # BA_OP_REDUCE_SCATTER: world chunks of `count`
            t = torch.as_tensor(DevArray(ptr, n, scalar), device=dev)
            stream.synchronize()
            c = t.cpu()
            if code in (0, 1):
                dist.all_reduce(c, op=dist.ReduceOp.SUM if code == 0 else dist.ReduceOp.MAX)
                t.copy_(c)
            elif code == 2:  # BA_OP_BCAST | root << 8
                dist.broadcast(c, src=root)
                t.copy_(c)
            elif code == 3:  # the rank's own chunk summed over the ranks; the other chunks are unspecified by the ABI: NaN here
                dist.all_reduce(c, op=dist.ReduceOp.SUM)
                t[rank * count:(rank + 1) * count].copy_(c[rank * count:(rank + 1) * count])
                t[:rank * count].fill_(float("nan"))
                t[(rank + 1) * count:].fill_(float("nan"))
            else:
                return 1
            stream.synchronize()
            return 0
        s.set_allreduce(collective)
        e0, dmax = s.linearize()
        r = s.minimize(max_trials=NTR)
        if rank == 0:
            out_q.put((e0, dmax, r["trace"], r["energy"]))
    finally:
        dist.destroy_process_group()


def _worker_natural_stop(rank, world, port, out_q):
    """Two ranks to the reference's own stop (flat-line), one of them with a slow transport."""
    import time
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch.distributed as dist
    import bundleadjustment_benchmarks_amd as ba
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.cuda.set_device(0)
        dev = torch.device("cuda", 0)
        p = ba.Problem.synthetic(24, 3000, 10500, 77)
        s = ba.Solver(p, ba.CHOLESKY, ba.F64, device=0, shard_rank=rank, shard_world=world)
        stream = torch.cuda.current_stream()
        s.set_stream(stream.cuda_stream)
        calls = [0]

        def allreduce(ptr, count, scalar, op, strm):
            calls[0] += 1
            if rank == 1:
                time.sleep(0.02)  # this rank's host runs behind the other's
            t = torch.as_tensor(DevArray(ptr, count, scalar), device=dev)
            stream.synchronize()
            c = t.cpu()
            dist.all_reduce(c, op=dist.ReduceOp.SUM if op == 0 else dist.ReduceOp.MAX)
            t.copy_(c)
            stream.synchronize()
            return 0
        s.set_allreduce(allreduce)
        r = s.minimize(tol_fun=1e-2)
        out_q.put((rank, calls[0], r["status"], r["trials"], r["energy"]))
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(600)
def test_two_ranks_natural_stop_same_number_of_collectives(ba, gpu_ok):
    """VERDICT r2 item 2 / ADVICE r2 (high): at a NATURAL stop (flat-line, not max_trials) every rank must have enqueued the same
    number of trials -- each carries two all-reduces, and a rank with one more would wait in its collective for ever.  The host
    enqueues trial n iff row n - LM_DEPTH has arrived with its stop mark clear, so the count is s + LM_DEPTH on every rank whatever
    its host's timing (one rank's transport is slowed down here).  Tested once."""
    p = ba.Problem.synthetic(24, 3000, 10500, 77)
    ref = ba.Solver(p, ba.CHOLESKY, ba.F64).minimize(tol_fun=1e-2)
    assert ref["status"] == 0 and 3 <= ref["trials"] < 60  # Success by flat-line after a few iterations
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29300 + os.getpid() % 500
    procs = [ctx.Process(target=_worker_natural_stop, args=(r, 2, port, q)) for r in range(2)]
    for pr in procs:
        pr.start()
    got = sorted(q.get(timeout=500) for _ in range(2))
    for pr in procs:
        pr.join(120)
        assert pr.exitcode == 0
    (_, calls0, st0, tr0, e0), (_, calls1, st1, tr1, e1) = got
    assert calls0 == calls1, (calls0, calls1)
    assert st0 == st1 == 0 and tr0 == tr1 and e0 == e1
    # 3 collectives of the first linearisation (energy, column norms, their maximum) + 2 per enqueued trial; the run ended at row
    # s = trials - 1, so s + LM_DEPTH (3) trials were enqueued
    assert calls0 == 3 + 2 * (tr0 - 1 + 3), (calls0, tr0)
    assert abs(e0 - ref["energy"]) < 3e-2 * ref["energy"]


@pytest.mark.parametrize("kind", [2, 1, 3, 0, 13])  # (0 = QRKIT and 3 = MOREQR: distributed TSQR -- the shards' R factors are what is all-reduced, no normal equations; 13 = MOREQR with BA_MOREQR_QR=0)
@pytest.mark.timeout(600)
def test_two_ranks_match_one_rank(ba, gpu_ok, kind, monkeypatch):
    p = ba.Problem.synthetic(24, 3000, 10500, 77)
    if kind >= 10:
        monkeypatch.setenv("BA_MOREQR_QR", "0")
    s = ba.Solver(p, kind % 10, ba.F64)
    e0, dmax = s.linearize()
    ref = s.minimize(max_trials=NTR)
    del s
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29700 + (os.getpid() + kind) % 1000
    procs = [ctx.Process(target=_worker, args=(r, 2, port, kind, q)) for r in range(2)]
    for pr in procs:
        pr.start()
    e0s, dmaxs, trace, energy = q.get(timeout=500)
    for pr in procs:
        pr.join(120)
        assert pr.exitcode == 0
    assert abs(e0s - e0) < 1e-12 * e0 and abs(dmaxs - dmax) < 1e-12 * dmax
    assert np.array_equal(trace[:, :2], ref["trace"][:, :2])          # iteration numbers and accept / reject
    assert np.allclose(trace[:2, 2], ref["trace"][:2, 2], rtol=1e-9)  # energies: the summation order differs across
    assert np.allclose(trace[:4, 2], ref["trace"][:4, 2], rtol=1e-6)  # shards and the trajectory amplifies it ~10x/iteration
    assert np.allclose(trace[:, 2], ref["trace"][:, 2], rtol=3e-2)


@pytest.mark.parametrize("kind", [2, 1, 0])
@pytest.mark.timeout(300)
def test_rccl_inside_library_one_rank(ba, gpu_ok, kind):
    """ba_comm_unique_id + ba_solver_comm_init (ncclCommInitRank inside the library) on a one-rank communicator switches ba_minimize
    to the sharded path: graph segment A | ncclAllReduce of the packed system + energy tail | segment B | ncclAllReduce of the
    three step scalars | device-side control.  With one rank the sums are identities, so the run must equal the single-GPU path
    (one graph per trial) exactly; the table rows go through the same pinned ring."""
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    p = ba.Problem.synthetic(24, 3000, 10500, 77)
    ref = ba.Solver(p, kind, ba.F64).minimize(max_trials=NTR)
    s = ba.Solver(p, kind, ba.F64)
    s.comm_init(ba.comm_unique_id())
    r = s.minimize(max_trials=NTR)
    assert r["status"] == ref["status"] and r["trials"] == ref["trials"] == NTR
    if kind == 0:  # (QRKIT: the QR of the one-block "stack" re-triangularises R: same step up to rounding, not bit for bit)
        assert np.array_equal(r["trace"][:, :2], ref["trace"][:, :2]) and np.allclose(r["trace"][:, 2:5], ref["trace"][:, 2:5], rtol=1e-6)
    else:
        assert np.array_equal(r["trace"][:, :5], ref["trace"][:, :5])
        assert r["energy"] == ref["energy"]
    tm = s.timing()
    assert tm["n_graph_trials"] == NTR and tm["comm_ms"] > 0
    # the step-level seam goes through the same transport
    e, _ = s.linearize()
    et, _, _ = s.try_step(1e-3)
    assert np.isfinite(et) and et < e


def test_empty_shard_does_not_fault(ba, gpu_ok):
    """More ranks than points: a shard that owns nothing must still walk through a trial (its partial sums are zero)."""
    p = ba.Problem.synthetic(3, 5, 12, 2)
    plans = [p.shard_plan(r, 8) for r in range(8)]
    empty = [r for r, q in enumerate(plans) if q["p1"] == q["p0"]]
    assert empty
    for kind in (ba.CHOLESKY, ba.QRCHOL, ba.MOREQR):
        s = ba.Solver(p, kind, ba.F64, shard_rank=empty[0], shard_world=8)
        s.set_allreduce(lambda ptr, count, scalar, op, stream: 0)  # stands in for the sum over the other (absent) ranks
        e, _ = s.linearize()
        assert e == 0.0
        et, rs, dn = s.try_step(1.0)
        assert et == 0.0
        if kind != ba.MOREQR:  # (MOREQR's exchange is the TSQR stack of the shards' R factors: with every other shard absent -- and
            assert np.isfinite(rs) and np.isfinite(dn)  # shard 0's sqrt(lambda) rows with them -- the stand-in system is 0 y = 0)


def _worker_dist_factor(rank, world, port, out_q, ncams=40):
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ["BA_DIST_FACTOR"] = "1"
    import torch.distributed as dist
    import bundleadjustment_benchmarks_amd as ba
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.cuda.set_device(0)
        dev = torch.device("cuda", 0)
        p = ba.Problem.synthetic(ncams, 1500, 6000, 91)  # D = 360: six block columns, three per rank (405: seven over three ranks)
        s = ba.Solver(p, ba.CHOLESKY, ba.F64, device=0, shard_rank=rank, shard_world=world)
        stream = torch.cuda.current_stream()
        s.set_stream(stream.cuda_stream)

        ops = []

        def collective(ptr, count, scalar, op, strm):
            """The callback ABI of include/ba_mi355x.h with all four op codes (gloo on host copies; RCCL refuses two ranks on one device)."""
            code, root = op & 0xff, op >> 8
            ops.append(code)
            n = count * world if code == 3 else count  # BA_OP_REDUCE_SCATTER: world chunks of `count`
            t = torch.as_tensor(DevArray(ptr, n, scalar), device=dev)
            stream.synchronize()
            c = t.cpu()
            if code in (0, 1):
                dist.all_reduce(c, op=dist.ReduceOp.SUM if code == 0 else dist.ReduceOp.MAX)
                t.copy_(c)
            elif code == 2:  # BA_OP_BCAST | root << 8
                dist.broadcast(c, src=root)
                t.copy_(c)
            elif code == 3:  # the rank's own chunk summed over the ranks; the other chunks are unspecified by the ABI: NaN here
                dist.all_reduce(c, op=dist.ReduceOp.SUM)
                t[rank * count:(rank + 1) * count].copy_(c[rank * count:(rank + 1) * count])
                t[:rank * count].fill_(float("nan"))
                t[(rank + 1) * count:].fill_(float("nan"))
            else:
                return 1
            stream.synchronize()
            return 0
        s.set_allreduce(collective)
        e0, dmax = s.linearize()
        et, rs, dn = s.try_step(1e-4)
        dxc = s.get(ba.GET_DX)[3 * s.Ml:]
        n_step = list(ops)
        r = s.minimize(max_trials=5)
        if rank == 0:
            out_q.put((e0, et, rs, dn, dxc, r["trace"], n_step))
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(600)
@pytest.mark.parametrize("world,ncams", [(2, 40), (3, 45)])
def test_distributed_factor_matches_the_replicated_one(ba, gpu_ok, world, ncams):
    """VERDICT r2 item 9 (SURVEY 8e "consider distributing K6"): BA_DIST_FACTOR=1 factors the reduced camera matrix 1-D block-cyclic
    over the ranks (reduce-scatter of the shards' partial systems to the block-column owners, owner factors a block column, ONE
    broadcast, every rank updates its own columns) instead of redundantly.  FUNCTIONAL
    check only -- two ranks on one GPU over the callback transport against the single-rank (replicated) factor: camera step to 1e-9,
    test energy, rho denominator, the first LM rows.  No speed claim: unmeasured on more than one GPU."""
    p = ba.Problem.synthetic(ncams, 1500, 6000, 91)
    s = ba.Solver(p, ba.CHOLESKY, ba.F64)
    e0, dmax = s.linearize()
    et, rs, dn = s.try_step(1e-4)
    dxc = s.get(ba.GET_DX)[3 * p.M:]
    ref = s.minimize(max_trials=5)
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 30100 + os.getpid() % 500
    procs = [ctx.Process(target=_worker_dist_factor, args=(r, world, port, q, ncams)) for r in range(world)]
    for pr in procs:
        pr.start()
    e0d, etd, rsd, dnd, dxcd, trace, ops = q.get(timeout=500)
    for pr in procs:
        pr.join(120)
        assert pr.exitcode == 0
    assert abs(e0d - e0) < 1e-12 * e0
    assert np.linalg.norm(dxcd - dxc) < 1e-9 * np.linalg.norm(dxc)
    assert abs(etd - et) < 1e-9 * et and abs(rsd - rs) < 1e-7 * abs(rs) and abs(dnd - dn) < 1e-9 * dn
    assert np.array_equal(trace[:, :2], ref["trace"][:, :2]) and np.allclose(trace[:3, 2], ref["trace"][:3, 2], rtol=1e-7)
    # (round 4) the collectives of linearize + ONE step: 3 all-reduces of the first linearisation (energy, column norms, their max), then
    # the exchange as ONE reduce-scatter (op 3: each rank only needs its own block columns summed) + a small all-reduce (g_c, energy),
    # ONE broadcast (op 2) per block column -- round 3 made three sum all-reduces of zeroed copies of each -- and the scalar all-reduce
    nblk = (9 * ncams + 63) // 64
    assert ops == [0, 0, 1] + [3, 0] + [2] * nblk + [0], ops
