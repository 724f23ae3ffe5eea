"""GPU: the failure paths of the in-launch hand-offs are loud (ADVICE r1 / VERDICT r1 item 5).

The dense factorisation and the one-launch backward sweep pass data between workgroups of ONE launch (a flag per row block,
a sentinel per unknown); their waits are bounded.  A wait that runs out must surface as BA_ERR_HIP through the device error
word, not as a silently rejected step.  Tested once, not a stress loop."""
import numpy as np
import pytest

import stage_checks

pytestmark = pytest.mark.gpu


def test_backsweep_without_its_producer_returns_err_hip(ba, gpu_ok, capfd):
    p = ba.Problem.synthetic(40, 480, 2400, 77)  # D = 360: six block columns = three groups in the sweep
    s = ba.Solver(p, ba.CHOLESKY, ba.F64)
    e, _ = s.linearize()
    et0, _, _ = s.try_step(1e-2)
    assert np.isfinite(et0) and et0 < e
    rc = s.selftest(1)  # the group at the head of the chain never publishes; short spin bound
    assert rc == 5, rc  # BA_ERR_HIP
    assert "device error 1024" in capfd.readouterr().err
    # the error word is cleared: the production path works again and reproduces the step
    et1, _, _ = s.try_step(1e-2)
    assert et1 == et0
    assert s.selftest(7) == 4  # unknown self-test: BA_ERR_ARG


def test_row_flag_timeout_is_recovered(ba, gpu_ok, capfd):
    """a hand-off time-out inside the fused factorisation (BA_DEVERR_ROW_FLAG: a row workgroup that was not
    resident in time) must not end the run.  selftest(2) arms the fault -- the row workgroups stay silent, the panel's wait is
    short --, ba_minimize meets it on the first trial, repeats that trial through the launch-per-step factorisation (no workgroup
    waits for another there) and carries on in that mode: same table as a clean solver, one recovery, a notice on stderr."""
    p = ba.Problem.synthetic(40, 480, 2400, 77)  # D = 360: six block columns, five fused steps
    ref = ba.Solver(p, ba.CHOLESKY, ba.F64).minimize(max_trials=6)
    s = ba.Solver(p, ba.CHOLESKY, ba.F64)
    assert s.selftest(2) == 0
    r = s.minimize(max_trials=6)
    err = capfd.readouterr().err
    assert "device error 1" in err and "repeating LM trial 0" in err
    assert s.recoveries() == 1
    assert r["status"] == ref["status"] and r["trials"] == ref["trials"] == 6
    assert np.array_equal(r["trace"][:, :2], ref["trace"][:, :2])
    # (the two factorisations round differently and the trajectory amplifies that: 2e-8 in rho by row 1, 8e-6 by row 5)
    assert np.allclose(r["trace"][:2, 2], ref["trace"][:2, 2], rtol=1e-7) and np.allclose(r["trace"][:, 2:5], ref["trace"][:, 2:5], rtol=1e-4)
    # the solver stays in the launch-per-step mode: a second run needs no recovery and gives the same table from its new start
    r2 = s.minimize(max_trials=3)
    assert s.recoveries() == 1 and r2["trials"] == 3
    # what that mode computes (k_ldlt_panel + k_ldlt_update per block column, k_ldlt_backpair for the three pairs of the six block
    # columns): the backward error of its camera step in its own S and rhs (tests/stage_checks.py), at a small and a large lambda
    # (measured on an MI355X: 5.5e-17).  k_ldlt_backstep (an odd count) is checked by test_gpu_stages.py::test_launch_per_pair_back_sweep.
    s.keep_intermediates(True)
    s.linearize()
    for lam in (1e-10, 1.0):
        s.try_step(lam)
        eta = stage_checks.eta(s.get(ba.GET_S), s.get(ba.GET_DX)[3 * s.Ml:], s.get(ba.GET_RHS))
        print("STAGE launch_per_step eta@%.0e %.3e 1e-15" % (lam, eta))
        assert eta <= 1e-15, (lam, eta)
    assert s.recoveries() == 1
    # a reduced system of one block column has no fused step to fail
    assert ba.Solver(ba.Problem.synthetic(6, 100, 400, 3), ba.QRCHOL, ba.F64).selftest(2) == 4


def test_watchdog_returns_instead_of_hanging(ba, gpu_ok, capfd, monkeypatch):
    """when no LM row appears for BA_WATCHDOG_S seconds ba_minimize must RETURN BA_ERR_HIP -- not fall into a stream
    synchronise behind the launch it has just declared hung.  selftest(3) puts a 4-second kernel in front of the next trial; with
    a one-second watchdog the call comes back after about a second, the handle is dead afterwards and frees nothing."""
    import time
    monkeypatch.setenv("BA_WATCHDOG_S", "1")
    p = ba.Problem.synthetic(8, 400, 1500, 3)
    s = ba.Solver(p, ba.QRCHOL, ba.F64)
    assert s.selftest(3) == 0
    t0 = time.time()
    with pytest.raises(ba.BAError) as ei:
        s.minimize(max_trials=4)
    dt = time.time() - t0
    assert ei.value.code == 5 and 0.9 < dt < 3.5, (ei.value.code, dt)
    assert "giving up on this solver" in capfd.readouterr().err
    with pytest.raises(ba.BAError) as ei2:
        s.linearize()
    assert ei2.value.code == 5
    del s  # (ba_solver_free of a dead handle returns at once)
    time.sleep(3.5)  # let the 4-second kernel end before the next test times anything
    ok = ba.Solver(p, ba.QRCHOL, ba.F64).minimize(max_trials=2)
    assert ok["trials"] == 2


def test_selftest_refuses_a_single_group(ba, gpu_ok):
    p = ba.Problem.synthetic(6, 100, 400, 3)  # D = 54: one block column, nobody to wait for
    s = ba.Solver(p, ba.QRCHOL, ba.F64)
    assert s.selftest(1) == 4


def test_legacy_stream_falls_back_to_direct_launches(ba, O, gpu_ok):
    """ba_solver_set_stream(NULL) hands the solver the legacy default stream, which cannot be captured into a hipGraph:
    ba_minimize must then enqueue the same kernels directly (same device-side control) and give the same run."""
    p = ba.Problem.synthetic(10, 400, 1500, 8)
    ref = ba.Solver(p, ba.QRCHOL, ba.F64).minimize(max_trials=8)
    s = ba.Solver(p, ba.QRCHOL, ba.F64)
    s.set_stream(0)
    r = s.minimize(max_trials=8)
    assert r["status"] == ref["status"] and np.array_equal(r["trace"][:, :5], ref["trace"][:, :5])
    assert s.timing()["n_graph_trials"] == 8  # (counted per device-controlled trial, graph or not)


def test_executable_with_world_of_one_and_max_iter_stop(ba, gpu_ok, tmp_path):
    """The executables' sharding switches with a world of one (RCCL communicator of one rank through the id file), and the LM
    stop conditions other than flat-line reach the caller through the device-side control: max_iter -> MaxItersReached."""
    import os
    import subprocess
    from conftest import DATA21, ROOT
    exe = os.path.join(ROOT, "bundleadjustment_benchmarks_amd", "bin", "Bundle_Adjustment_Cholesky")
    env = dict(os.environ, BA_MAX_TRIALS="4", BA_WORLD="1", BA_RANK="0", BA_COMM_FILE=str(tmp_path / "id"))
    out = subprocess.run([exe, DATA21], capture_output=True, text=True, timeout=600, env=env)
    assert out.returncode == 0 and "LM finished with status: Running" in out.stdout and out.stdout.count("Accepted") == 4
    p = ba.Problem.load_bal(DATA21)
    s = ba.Solver(p, ba.CHOLESKY, ba.F64)
    r = s.minimize(max_iter=3)
    assert r["status"] == 3 and r["iterations"] == 4 and r["trials"] == 3  # the loop top of iteration 4 stops it (:243-248)
    s2 = ba.Solver(p, ba.CHOLESKY, ba.F64)
    r2 = s2.minimize(lambda_max=1e-30, max_trials=50)  # every accepted step leaves lambda > lambda_max: the first rejection ends the run
    assert r2["status"] in (1, -1)
