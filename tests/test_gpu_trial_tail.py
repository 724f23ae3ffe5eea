"""GPU: the tail of an LM iteration that prepares the next trial (csrc/ba_solver.hip, tail_prepares(): behind the step control the
records of the next trial are made and its camera pairs assembled, in one launch with the camera Gram -- k_pairs_gram -- and the trial
that follows starts at k_schur_reduce) against the sequence in which every trial starts with its own elimination and pair assembly
(BA_TRIAL_HEAD=1, read when a solver is created).

Every case runs the same calls on two fresh solvers in this process, one per sequence, and asks for IDENTICAL BYTES: cameras, points,
[energy, lambda], [status, iterations, trials, fun_evals] and every row of the trace (its last column, the host's wall-clock time per
row, left out).  No tolerance: the change moves launches, no addition.

Where the issue's case 2 says "a second minimize continues bit-equal to one uninterrupted run": a second ba_minimize starts, as it always
has, from a host-side linearisation and lambda0 = 1e-12 max diag J'J of the state it finds, so its rows are not those of a longer first
call under either sequence; what is asked here is that the two calls together give the same bytes under both sequences, and that the
energy the first call returns is the energy of the linearisation at the state it returns."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def snapshot(ba, s, r):
    return [("cams", s.get(ba.GET_CAMS)), ("points", s.get(ba.GET_POINTS)), ("result", np.float64([r["energy"], r["lam"]])),
            ("counts", np.int64([r["status"], r["iterations"], r["trials"], r["fun_evals"]])), ("trace", np.ascontiguousarray(r["trace"][:, :5]))]


def both(monkeypatch, body):
    """body() under the default sequence and under BA_TRIAL_HEAD=1: two lists of (name, array), compared byte for byte"""
    monkeypatch.delenv("BA_TRIAL_HEAD", raising=False)
    tail = body()
    monkeypatch.setenv("BA_TRIAL_HEAD", "1")
    head = body()
    monkeypatch.delenv("BA_TRIAL_HEAD", raising=False)
    assert [n for n, _ in tail] == [n for n, _ in head]
    for (name, a), (_, b) in zip(tail, head):
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), (name, a, b)
    return tail


def perturbed(ba, s, p, seed, sigma):
    """the solver's start state with seeded noise on the camera translations and the points"""
    rng = np.random.default_rng(seed)
    cams = s.get(ba.GET_CAMS).reshape(p.N, 15).copy()
    pts = s.get(ba.GET_POINTS).reshape(-1, 3).copy()
    cams[:, 9:12] += rng.normal(0, sigma, (p.N, 3))
    pts += rng.normal(0, sigma, pts.shape)
    return cams.ravel(), pts.ravel()


def patterns(acc):
    a = [int(v) for v in acc]
    two = set(zip(a, a[1:]))
    three = set(zip(a, a[1:], a[2:]))
    return (1, 1) in two, (1, 0, 1) in three, (0, 0) in two


def test_accept_and_reject_sequences(ba, gpu_ok, monkeypatch):
    """accepted -> accepted, accepted -> rejected -> accepted and rejected -> rejected in one run: from a perturbed state, without the
    flat-line stop, and with a small increase base that lets lambda climb slowly (on an MI355X the run reads 11110000110100000000000
    and ends at lambda_max)."""
    p = ba.Problem.synthetic(8, 100, 400, 12)

    def body():
        s = ba.Solver(p, ba.CHOLESKY, ba.F64)
        s.set_state(*perturbed(ba, s, p, 5, 0.01))
        r = s.minimize(max_trials=40, lambda_increase_base=1.5, tol_fun=0.0)
        return snapshot(ba, s, r)

    out = dict(both(monkeypatch, body))
    acc = out["trace"][:, 1]
    print("accepted:", "".join(str(int(v)) for v in acc))
    assert patterns(acc) == (True, True, True), acc


def test_max_trials_behind_an_accepted_step(ba, gpu_ok, monkeypatch):
    p = ba.Problem.synthetic(8, 100, 400, 12)

    def body():
        s = ba.Solver(p, ba.CHOLESKY, ba.F64)
        r1 = s.minimize(max_trials=3)
        assert r1["trials"] == 3 and r1["trace"][-1, 1] == 1 and r1["status"] == -1  # stopped right behind an accepted step
        out = [("first." + n, a) for n, a in snapshot(ba, s, r1)]
        r2 = s.minimize(max_trials=4)  # (its own linearisation first: the energy its first row shows is that of the state r1 left)
        assert r2["trace"][0, 2] == r1["energy"], (r2["trace"][0, 2], r1["energy"])
        return out + [("second." + n, a) for n, a in snapshot(ba, s, r2)]

    both(monkeypatch, body)


def test_set_state_between_two_runs(ba, gpu_ok, monkeypatch):
    p = ba.Problem.synthetic(8, 100, 400, 13)

    def body():
        s = ba.Solver(p, ba.CHOLESKY, ba.F64)
        out = [("first." + n, a) for n, a in snapshot(ba, s, s.minimize(max_trials=4))]
        s.set_state(*perturbed(ba, s, p, 6, 0.01))
        return out + [("second." + n, a) for n, a in snapshot(ba, s, s.minimize(max_trials=6))]

    both(monkeypatch, body)


def test_short_camera_and_single_chunk_pair(ba, gpu_ok, monkeypatch):
    """a camera of fewer than 32 observations (a short chunk of the Gram part) and camera pairs of one chunk (written by the pair
    workgroups straight into S)"""
    p = ba.Problem.synthetic(6, 60, 150, 14)
    a = p.arrays()
    assert 0 < np.bincount(a["cam_idx"], minlength=p.N).min() < 32
    _, weight = p.covisibility()
    assert len(weight) and 1 <= weight.min() and weight.max() <= 64

    def body():
        s = ba.Solver(p, ba.CHOLESKY, ba.F64)
        return snapshot(ba, s, s.minimize(max_trials=8))

    out = dict(both(monkeypatch, body))
    assert out["counts"][2] == 8


def _priors(ba, s, p):
    ids = np.arange(0, 10, dtype=np.int32)
    s.set_point_priors(ids, s.get(ba.GET_POINTS).reshape(-1, 3)[ids] + 0.01, sigma=0.1)


def _relpose(ba, s, p):
    s.set_relative_poses(np.int32([[0, 1]]), np.eye(3)[None], np.zeros((1, 3)), sigma_rot=10.0, sigma_trans=100.0)


def _mask(ba, s, p):
    s.set_constant(p.gauge_mask(), None)


def _marq(ba, s, p):
    s.set_damping(ba.DAMP_MARQUARDT)


OLD_SEQUENCE = dict(priors=("CHOLESKY", "F64", _priors), relpose=("CHOLESKY", "F64", _relpose), mask=("CHOLESKY", "F64", _mask),
                    marquardt=("CHOLESKY", "F64", _marq), qrchol=("QRCHOL", "F64", None), fp32=("CHOLESKY", "F32", None))


@pytest.mark.parametrize("name", sorted(OLD_SEQUENCE))
def test_configurations_that_keep_the_head(ba, gpu_ok, monkeypatch, name):
    kind, scalar, setup = OLD_SEQUENCE[name]
    p = ba.Problem.synthetic(8, 100, 400, 15)

    def body():
        s = ba.Solver(p, getattr(ba, kind), getattr(ba, scalar))
        if setup:
            setup(ba, s, p)
        return snapshot(ba, s, s.minimize(max_trials=6))

    out = dict(both(monkeypatch, body))
    assert out["counts"][2] == 6


def test_point_of_more_than_256_observations(ba, gpu_ok, monkeypatch):
    import shape_problems
    p, facts = shape_problems.get(ba, "tracks257")
    assert facts["kmax"] == 257

    def body():
        s = ba.Solver(p, ba.CHOLESKY, ba.F64)
        return snapshot(ba, s, s.minimize(max_trials=4))

    both(monkeypatch, body)


def test_repeat_behind_a_row_flag_timeout_assembles(ba, gpu_ok, monkeypatch, capfd):
    """selftest(2) arms the row-flag time-out: the first trial fails, the repeat (launch-per-step factorisation) has nobody's tail in
    front of it and must run its own head."""
    p = ba.Problem.synthetic(16, 160, 800, 16)  # D = 144: three block columns, two fused steps

    def body():
        s = ba.Solver(p, ba.CHOLESKY, ba.F64)
        assert s.selftest(2) == 0
        r = s.minimize(max_trials=6)
        assert s.recoveries() == 1 and r["trials"] == 6
        return snapshot(ba, s, r)

    both(monkeypatch, body)
    assert capfd.readouterr().err.count("repeating LM trial 0") == 2
