"""GPU: the per-observation records (rec, JcA) stored through LDS a cache line at a time against the one-thread-per-record stores.

The fused CHOLESKY linearisation (k_eval<T, true, 3>) and k_elim_chol store a wavefront's run of records as the contiguous bytes it is
(ba_store_run); BA_REC_PLAIN=1, read at solver creation, keeps the stores in which every thread walks its own
record.  Only the way the bytes travel differs -- no scalar is computed differently, no sum changes its order -- so the criterion is BIT
EQUALITY of everything a run leaves behind, with no tolerance: the LM tables and final states of whole runs (fused and BA_NO_FUSE=1,
fp64 and fp32), and the intermediates of single steps on the shapes where a cooperative path can go wrong (ragged input, tracks that
fill a point-aligned range, last workgroups and wavefronts that are nearly empty, one camera and one point), with the MASK, MODEL and
MARQ instantiations in force.  (The readers of the records -- k_cam_gram, k_backsub, the Schur assembly -- are the kernels they were:
their cooperative loads measured slower and were dropped, profiles/EXPERIMENTS.md section 7; the cases that were chosen for them stay.)
"""
import numpy as np
import pytest

import shape_problems as SP
from test_gpu_parity import _long_track_problem, _ragged_problem

pytestmark = pytest.mark.gpu

STEP_GETS = ("GET_S", "GET_RHS", "GET_DX", "GET_POINTS_TEST")


def raw(a):
    """the bytes of an array or a tuple of scalars (NaNs compare equal, -0 differs from 0)"""
    return np.ascontiguousarray(a).tobytes()


def both(monkeypatch, run):
    """run() under the default (cooperative) record paths and under BA_REC_PLAIN=1"""
    out = []
    for plain in (False, True):
        if plain:
            monkeypatch.setenv("BA_REC_PLAIN", "1")
        else:
            monkeypatch.delenv("BA_REC_PLAIN", raising=False)
        out.append(run())
    monkeypatch.delenv("BA_REC_PLAIN", raising=False)
    return out


def same(a, b):
    assert a.keys() == b.keys(), (sorted(a), sorted(b))
    bad = [k for k in a if a[k] != b[k]]
    assert not bad, bad


def lm_run(ba, p, kind, scalar, trials, setup=None):
    s = ba.Solver(p, kind, scalar)
    if setup:
        setup(s)
    r = s.minimize(max_trials=trials)
    tr = r["trace"][:, :5].copy()
    return {"rows": len(tr), "rejected": int((tr[:, 1] == 0).sum()), "trace": raw(tr), "cams": raw(s.get(ba.GET_CAMS)),
            "points": raw(s.get(ba.GET_POINTS)), "energy": raw(np.float64(r["energy"]))}


def step_run(ba, p, kind, scalar, setup=None):
    """linearize() and try_step at lambda = 1e-12 dmax and at 10 with the intermediates kept: what the record kernels feed, as bytes.
    (A trial the library refuses -- a singular reduced system -- counts as its error code: the same under both settings.)"""
    s = ba.Solver(p, kind, scalar)
    if setup:
        setup(s)
    s.keep_intermediates(True)
    e, dmax = s.linearize()
    out = {"energy": raw(np.float64(e)), "dmax": raw(np.float64(dmax)), "GET_JC": raw(s.get(ba.GET_JC)), "GET_GRAD": raw(s.get(ba.GET_GRAD))}
    for n, lam in enumerate((1e-12 * dmax, 10.0)):
        try:
            out["trial%d" % n] = raw(np.array(s.try_step(lam), np.float64))
        except ba.BAError as err:
            out["trial%d" % n] = ("refused", err.code)
            continue
        for g in STEP_GETS:
            out["%s@%d" % (g, n)] = raw(s.get(getattr(ba, g)))
    return out


# ---- whole LM runs --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nofuse", [False, True], ids=["fused", "nofuse"])
@pytest.mark.parametrize("scalar", [0, 1], ids=["f64", "f32"])
@pytest.mark.parametrize("kind,trials", [(2, 40), (1, 30)], ids=["CHOLESKY", "QRCHOL"])
def test_lm_runs_are_bit_equal(ba, gpu_ok, prob21, monkeypatch, kind, trials, scalar, nofuse):
    """Problem-21: CHOLESKY over 40 trials (the fp64 run crosses rejected trials, so k_elim_chol really runs behind the fused
    linearisation) and QRCHOL over 30; with BA_NO_FUSE=1 the separate launches (k_elim_chol in front of every trial, k_grad_prep)."""
    if nofuse:
        monkeypatch.setenv("BA_NO_FUSE", "1")
    else:
        monkeypatch.delenv("BA_NO_FUSE", raising=False)
    a, b = both(monkeypatch, lambda: lm_run(ba, prob21, kind, scalar, trials))
    if scalar == 0:
        assert a["rows"] == trials
        if kind == 2:
            assert a["rejected"] > 0, "the comparison is meant to cross rejected trials"
    same(a, b)


# ---- the shapes where a cooperative path can go wrong ---------------------------------------------------------------------------
def _tracks_to_250(ba):
    """Tracks of 250 / 200 / 130 observations next to short ones: point-aligned ranges of k_eval that are nearly full or hold one long
    track and a few lanes more (the fused linearisation's own long-track problem, test_gpu_parity)."""
    p = ba.Problem.synthetic(12, 300, 1200, 78)
    a = p.arrays()
    rng = np.random.default_rng(6)
    cam_idx, pt_idx, meas = list(a["cam_idx"]), list(a["pt_idx"]), [tuple(m) for m in a["meas"].reshape(-1, 2)]
    for j, want in ((7, 250), (8, 200), (150, 130)):
        mine = [i for i in range(p.K) if a["pt_idx"][i] == j]
        for n in range(want - len(mine)):
            src = mine[n % len(mine)]
            cam_idx.append(a["cam_idx"][src]); pt_idx.append(j)
            m = a["meas"].reshape(-1, 2)[src] + rng.normal(0, 0.3, 2)
            meas.append((m[0], m[1]))
    return ba.Problem.from_arrays(p.N, p.M, len(cam_idx), np.array(cam_idx, np.int32), np.array(pt_idx, np.int32),
                                  np.array(meas, np.float64).ravel(), a["cams9"], a["pts"])


def _one_camera_one_point(ba):
    """the first observation of a synthetic problem with its camera and its point: N = M = K = 1"""
    p = ba.Problem.synthetic(5, 40, 131, 9)
    a = p.arrays()
    c, j = int(a["cam_idx"][0]), int(a["pt_idx"][0])
    return ba.Problem.from_arrays(1, 1, 1, np.zeros(1, np.int32), np.zeros(1, np.int32), a["meas"][:2], a["cams9"][9 * c:9 * c + 9],
                                  a["pts"][3 * j:3 * j + 3])


def _large_edges(ba):
    """synthetic(48, 40000, 150000) with the edge shapes in it -- points cut down to one observation and to none, tracks of 250 / 200 /
    130 observations, unsorted input -- so that they meet k_eval<float, true, 3> as well (see LARGE)."""
    p = ba.Problem.synthetic(48, 40000, 150000, 22)
    a = p.arrays()
    cam, pt, meas = a["cam_idx"], a["pt_idx"], a["meas"].reshape(-1, 2)
    keep = np.ones(p.K, bool)
    for j in (3, 40, 41, 20000):
        keep[np.where(pt == j)[0][1:]] = False
    keep[pt == 77] = False
    rng = np.random.default_rng(8)
    add_cam, add_pt, add_meas = [], [], []
    for j, want in ((7, 250), (8, 200), (150, 130), (39999, 250)):
        mine = np.where(pt == j)[0]
        src = mine[np.arange(want - len(mine)) % len(mine)]
        add_cam.append(cam[src]); add_pt.append(pt[src]); add_meas.append(meas[src] + rng.normal(0, 0.3, (len(src), 2)))
    cam = np.concatenate([cam[keep]] + add_cam); pt = np.concatenate([pt[keep]] + add_pt); meas = np.concatenate([meas[keep]] + add_meas)
    perm = rng.permutation(len(cam))
    return ba.Problem.from_arrays(p.N, p.M, len(cam), cam[perm].astype(np.int32), pt[perm].astype(np.int32), meas[perm].ravel(), a["cams9"], a["pts"])


# The fp32 fused linearisation keeps the owners' stores on a problem of one round of workgroups (launch_eval: at most two per CU), which
# every problem of PROBLEMS is: k_eval<float, true, 3> runs only on these -- 150 000 observations are 586 workgroups of k_eval or more,
# beyond two for each of the 256 CUs.
LARGE = {"syn150k": lambda ba: ba.Problem.synthetic(48, 40000, 150000, 21), "edges150k": _large_edges}
PROBLEMS = {
    "ragged": _ragged_problem,                                     # points with no / one observation, a blind camera, unsorted input
    "tracks250": _tracks_to_250,
    "tracks700": _long_track_problem,                              # a track beyond 256: plain ranges of 256, no fused linearisation
    "syn131": lambda ba: ba.Problem.synthetic(5, 40, 131, 9),      # one workgroup; a last wavefront with 3 observations
    "syn1200": lambda ba: ba.Problem.synthetic(12, 300, 1200, 78),  # last workgroup: 176 = 2 wavefronts + 48; camera chunks of 100 % 32
    "one": _one_camera_one_point,
    # tests/shape_problems.py: camera pairs of 1 ... 129 entries; tracks of 1 ... 256 with point-aligned ranges that are exactly full, filled
    # by one track and split; the same with a track of 257 (no point-aligned ranges: plain ranges of 256, no fused linearisation).  Under
    # the tests over PROBLEMS: cooperative against per-thread record stores; fused against BA_NO_FUSE=1:
    # test_designed_shapes_fused_against_the_separate_launches
    "pairs": lambda ba: SP.get(ba, "pairs")[0],
    "tracks256": lambda ba: SP.get(ba, "tracks256")[0],
    "tracks257": lambda ba: SP.get(ba, "tracks257")[0],
}
_CACHE = {}


def problem(ba, name):
    if name not in _CACHE:
        _CACHE[name] = (PROBLEMS.get(name) or LARGE[name])(ba)
    return _CACHE[name]


@pytest.mark.parametrize("scalar", [0, 1], ids=["f64", "f32"])
@pytest.mark.parametrize("kind", [2, 1], ids=["CHOLESKY", "QRCHOL"])
@pytest.mark.parametrize("name", sorted(PROBLEMS))
def test_single_steps_are_bit_equal(ba, gpu_ok, monkeypatch, name, kind, scalar):
    monkeypatch.delenv("BA_NO_FUSE", raising=False)
    p = problem(ba, name)
    a, b = both(monkeypatch, lambda: step_run(ba, p, kind, scalar))
    assert len(a["GET_JC"]) == 18 * p.K * 8 and len(a["GET_GRAD"]) > 0
    same(a, b)


@pytest.mark.parametrize("scalar", [0, 1], ids=["f64", "f32"])
@pytest.mark.parametrize("name", sorted(PROBLEMS))
def test_short_lm_runs_on_the_edge_shapes_are_bit_equal(ba, gpu_ok, monkeypatch, name, scalar):
    """The fused linearisation's cooperative stores (k_eval<T, true, 3>) only run inside ba_minimize: twelve CHOLESKY trials on every
    edge shape, so that point-aligned ranges with empty and nearly empty wavefronts go through them.  In fp32 these small problems stay
    on k_eval<float, true, 2> under both settings (see LARGE): there the cases compare k_elim_chol's stores alone, and the fp32 k_eval
    meets the edge shapes in test_lm_runs_beyond_one_round_of_workgroups_are_bit_equal."""
    monkeypatch.delenv("BA_NO_FUSE", raising=False)
    p = problem(ba, name)
    a, b = both(monkeypatch, lambda: lm_run(ba, p, 2, scalar, 12))
    assert a["rows"] >= 1
    same(a, b)


# ---- the designed shapes: the fused linearisation against the separate launches ------------------------------------------------------
@pytest.mark.parametrize("kind,trials", [(2, 16), (1, 12)], ids=["CHOLESKY", "QRCHOL"])
@pytest.mark.parametrize("name", ["pairs", "tracks256", "tracks257"])
def test_designed_shapes_fused_against_the_separate_launches(ba, gpu_ok, monkeypatch, name, kind, trials):
    """ba_minimize on the designs of tests/shape_problems.py with the fused linearisation (k_eval<T, true, FUSE>: behind an accepted step it
    also sums the point part of J'J and J'r and, CHOLESKY, eliminates the points of the trial that follows) and with BA_NO_FUSE=1 (the
    separate launches: k_point_prep / k_grad_prep, k_elim_chol in front of every trial), cooperative stores in both: the LM table and the
    final state are the same BITS.  tracks256 is the case this is for -- its first point-aligned ranges are 255 + 1 (exactly full), one
    256-track (a range of its own) and 127 + 128 | 2 (split); the run must accept steps, or the fused linearisation never ran.  tracks257:
    a track beyond 256 leaves no point-aligned ranges (ba_plan_eval_ranges; the builder asserts kmax = 257 and the empty plan, and the
    solver's `fuse` is only ever set when that plan is not empty), so both settings take the separate launches and the comparison only shows
    that the switch then changes nothing.  fp64: in fp32 the two sequencings part ways by design ("Fused
    linearisation"), as in tests/test_gpu_parity.py::test_fused_linearisation_is_bit_equal_to_the_separate_launches."""
    monkeypatch.delenv("BA_REC_PLAIN", raising=False)
    p, facts = SP.get(ba, name)
    assert (facts["eval_ranges"] == []) == (name == "tracks257") and (facts["kmax"] > 256) == (name == "tracks257")
    out = []
    for nofuse in (False, True):
        if nofuse:
            monkeypatch.setenv("BA_NO_FUSE", "1")
        else:
            monkeypatch.delenv("BA_NO_FUSE", raising=False)
        out.append(lm_run(ba, p, kind, 0, trials))
    monkeypatch.delenv("BA_NO_FUSE", raising=False)
    a, b = out
    assert a["rows"] == trials and a["rows"] - a["rejected"] >= 3, (a["rows"], a["rejected"])
    same(a, b)


# ---- the MASK, MODEL and MARQ instantiations ------------------------------------------------------------------------------------
def _mask(ba, p):
    cm = np.zeros(p.N, np.uint16)
    cm[0] = ba.FIX_CAMERA; cm[3] = ba.FIX_INTRINSICS; cm[7] = ba.FIX_T
    pf = np.zeros(p.M, np.uint8)
    pf[::17] = 1
    return lambda s: s.set_constant(cm, pf)


def _model(ba, p):
    w = 0.5 + np.random.default_rng(3).random(p.K)

    def setup(s):
        s.set_loss(ba.LOSS_CAUCHY, 1.5)
        s.set_obs_weights(w)
    return setup


def _marq(ba, p):
    return lambda s: s.set_damping(ba.DAMP_MARQUARDT)


FEATURES = {"mask": _mask, "model": _model, "marquardt": _marq}


@pytest.mark.parametrize("scalar", [0, 1], ids=["f64", "f32"])
@pytest.mark.parametrize("feature", sorted(FEATURES))
def test_features_in_force_are_bit_equal(ba, gpu_ok, monkeypatch, feature, scalar):
    """A constant-parameter mask, a Cauchy loss with weights, Marquardt's damping on synthetic(12, 300, 1200): single steps (the
    separate k_elim_chol<T, MARQ, COOP>) and sixteen trials of ba_minimize (fp64: the fused k_eval<double, true, 3, false, MASK, MODEL>;
    fp32 stays on FUSE = 2 at this size and has its k_eval cases below)."""
    monkeypatch.delenv("BA_NO_FUSE", raising=False)
    p = problem(ba, "syn1200")
    setup = FEATURES[feature](ba, p)
    a, b = both(monkeypatch, lambda: step_run(ba, p, 2, scalar, setup))
    same(a, b)
    a, b = both(monkeypatch, lambda: lm_run(ba, p, 2, scalar, 16, setup))
    assert a["rows"] >= 1
    same(a, b)


def _mask_and_model(ba, p):
    m, w = _mask(ba, p), _model(ba, p)

    def setup(s):
        m(s)
        w(s)
    return setup


LARGE_SETUPS = {"plain": lambda ba, p: None, "mask": _mask, "model": _model, "mask+model": _mask_and_model}


@pytest.mark.parametrize("scalar", [0, 1], ids=["f64", "f32"])
@pytest.mark.parametrize("feature", sorted(LARGE_SETUPS))
@pytest.mark.parametrize("name", sorted(LARGE))
def test_lm_runs_beyond_one_round_of_workgroups_are_bit_equal(ba, gpu_ok, monkeypatch, name, feature, scalar):
    """Eight CHOLESKY trials on the problems of LARGE, the only ones on which the fp32 fused linearisation stores cooperatively: all four
    k_eval<T, true, 3, false, MASK, MODEL> of either scalar type (fp32: an image row of 36 scalars, 16 rows filling a wavefront's quarter
    of `cu` exactly), on a plain synthetic problem and on one with the edge shapes in it."""
    monkeypatch.delenv("BA_NO_FUSE", raising=False)
    p = problem(ba, name)
    setup = LARGE_SETUPS[feature](ba, p)
    a, b = both(monkeypatch, lambda: lm_run(ba, p, 2, scalar, 8, setup))
    assert a["rows"] >= 1
    same(a, b)
