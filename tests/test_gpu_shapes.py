"""GPU: the point elimination, the Schur assembly, the camera Gram and the back-substitution at every track and pair shape at which they
switch code path -- the problems of tests/shape_problems.py, each stage against quad precision on the GPU's OWN inputs of that stage with
the metrics and bounds of tests/test_gpu_stages.py (no new tolerance).

  pairs       camera pairs of 1 ... 9, 12, 13, 16, 17, 63, 64, 65, 127, 128, 129 entries: k_schur_pairs' batches of eight from two register
              sets, its masked tail and shadow entry, the direct write of a single-chunk pair against the slab and k_schur_reduce
  tracks256   points of 1, 2, 3, 7, 8, 9 (k_backsub<8>'s stride), 31 ... 256 observations (both sides of every bucket of k_elim_qr<LPP, SL>: the
              last slot of a lane just filled or just empty); point-aligned ranges that are exactly full, filled by one track, split
  tracks257   + a point of 257: the last bucket, and the solver on the separate launches (no point-aligned ranges)
  track1024   a point of 1024 observations: every slot of every lane of k_elim_qr<64, 16>;  track1025: refused by the QR eliminations
  walk        5497 chunks under one workgroup per CU: the persistent walk of k_schur_pairs three chunks deep and more, under four dealings

What a lost observation or entry at these places does to the metrics: tests/test_shape_problems_cpu.py.  Every value is printed as
`STAGE <case> <metric> <value> <bound>`; profiles/r25_shape_stages.txt is the listing of the MI355X run.
"""
import hashlib

import numpy as np
import pytest

import shape_problems as SP
import stage_checks as SC
from test_gpu_parity import _moreqr_default_route, moreqr_route  # noqa: F401 (autouse fixture)
from test_gpu_stages import EPS, Checker, Trial

pytestmark = pytest.mark.gpu

KIND_IDS = {2: "chol", 1: "qrchol", 13: "moreqr_ne", 0: "qrkit", 3: "moreqr"}
_REF = {}


def referee(O, t, lam):
    """The quad S and rhs of the trial's J, residuals and lambda (about 22 us per pair entry on the host), once per (J, f, lambda): the
    kinds share the linearisation kernels, so they hand in the same bytes.  Quad CHOLESKY elimination throughout, as test_dense_qr_step
    does: every kind's reduced system is the same matrix."""
    key = hashlib.sha1(b"".join(np.ascontiguousarray(x).tobytes() for x in (t.Jc, t.Jp, t.f, np.float64(lam)))).hexdigest()
    if key not in _REF:
        _REF[key] = O.referee_reduced_from_jacobian(O.CHOLESKY, t.po, t.Jc, t.Jp, t.f, lam)
    return _REF[key]


def check_trial(ba, O, t, kind_s, has_S, lam):
    """One try_step(lam) of a Trial: eta / back-substitution / retraction / trial scalars (Trial.step, eta under the ordinary bound of BOUND
    in fp32 too: the worst measured is 1.8e-7 of 1e-5), then S and rhs against quad with the
    rule max(10 x the same-precision oracle on the GPU's J, floor) (test_assembly_and_backsub), or for a kind without S qr_eta against
    the quad S and rhs (test_dense_qr_step).  Returns (dx, S, rhs)."""
    ck = t.ck
    dx, S, rhs = t.step(lam, has_S)
    R = referee(O, t, lam)
    if not has_S:
        got = SC.eta(R["S"], dx[3 * t.po.M:], R["rhs"])
        if t.scalar == 0:
            st = t.oracle_step(O.MOREQR, lam, want_S=False)
            orc = SC.eta(R["S"], st["dx"][3 * t.po.M:], R["rhs"])
            ck("qr_eta@%.0e(oracle %.1e)" % (lam, orc), got, max(10 * orc, t.bound("qr_eta")))
        else:
            ck("qr_eta@%.0e" % lam, got, t.bound("qr_eta"))
        return dx, S, rhs
    st = t.oracle_step(kind_s, lam)
    got = SC.assembly_errors(t.po, t.Jc, t.f, lam, S, rhs, R["S"], R["rhs"], t.Jp)
    orc = SC.assembly_errors(t.po, t.Jc, t.f, lam, st["S"].astype(np.float64), st["rhs"].astype(np.float64), R["S"], R["rhs"], t.Jp)
    if not all(np.isfinite(v) for v in orc.values()):
        # (test_assembly_and_backsub's fallback for an fp32 oracle whose CHOLESKY elimination breaks down: the fp64 oracle on the same J,
        # its error scaled by eps32 / eps64)
        s64 = O.step(kind_s, t.po, t.Jc, t.Jp, t.f, lam)
        o64 = SC.assembly_errors(t.po, t.Jc, t.f, lam, s64["S"], s64["rhs"], R["S"], R["rhs"], t.Jp)
        orc = {k: v * EPS[1] / EPS[0] for k, v in o64.items()}
    for k in ("S", "rhs"):
        ck("%s@%.0e(oracle %.1e)" % (k, lam, orc[k]), got[k], max(10 * orc[k], t.bound(k)))
    return dx, S, rhs


def lambdas(ba, t, kind, both=True):
    lam0 = 1e-6 * np.sqrt(t.dmax) if kind == ba.MOREQR else 1e-12 * t.dmax  # (MOREQR's own lambda0: test_dense_qr_step)
    return (lam0, 10.0) if both else (lam0,)


# ---- pairs, tracks256, tracks257: every kind, both scalar types, lambda0 and 10 -----------------------------------------------------------
@pytest.mark.parametrize("scalar", [0, 1], ids=["f64", "f32"])
@pytest.mark.parametrize("kind", [2, 1, 13, 0, 3], ids=[KIND_IDS[k] for k in (2, 1, 13, 0, 3)])
@pytest.mark.parametrize("name", ["pairs", "tracks256", "tracks257"])
def test_elimination_and_assembly_at_every_shape(ba, O, gpu_ok, monkeypatch, name, kind, scalar):
    """The linearisation at the GPU's state, then per lambda eta, back-substitution, retraction and trial scalars, and S and rhs (CHOLESKY:
    k_elim_chol; QRCHOL: k_elim_qr; MOREQR by the normal equations: k_more_trial; then k_schur_pairs / k_schur_reduce and k_cam_gram) or,
    for QRKIT and MOREQR, qr_eta.  Measured worst on an MI355X, GPU (oracle on the same J), fp64 / fp32:
      pairs      S 2.3e-15 (2.7e-15) / 2.9e-6 (2.2e-6), rhs 1.4e-15 / 1.5e-6, eta 3.3e-17 / 1.7e-8, backsub 3.5e-16 / 1.7e-7, qr_eta 2.2e-17 (6.3e-17) / 8.6e-9
      tracks256  S 5.1e-16 (3.1e-15) / 3.5e-7 (1.8e-6), rhs 3.7e-16 / 1.6e-7, eta 4.6e-17 / 1.4e-7, backsub 3.6e-16 / 1.5e-7, qr_eta 1.4e-17 (6.3e-17) / 9.7e-9
      tracks257  S 9.5e-16 (2.8e-15) / 5.6e-7 (1.8e-6), rhs 3.3e-16 / 2.8e-7, eta 1.4e-16 / 1.8e-7, backsub 3.1e-16 / 1.5e-7, qr_eta 2.1e-17 (6.1e-17) / 9.6e-9
    and the energy 1.8e-15 / 2.5e-6.  The largest bound on S that the rule max(10 x oracle, floor) gave is 2.7e-14 / 2.2e-5; one lost
    observation at the designed places is 1.6e-3 and more (tests/test_shape_problems_cpu.py).
    The CPU oracle on its own J (tests/test_shape_problems_cpu.py): fp64 S 4.1e-15, fp32 S 3.3e-6."""
    kind_s, has_S = moreqr_route(kind, monkeypatch, O)
    p, _ = SP.get(ba, name)
    ck = Checker("shapes[%s,%s,%s]" % (name, KIND_IDS[kind], "f64" if scalar == 0 else "f32"))
    t = Trial(ba, O, p, kind_s, scalar, ck)
    t.check_linearization()
    for lam in lambdas(ba, t, kind):
        check_trial(ba, O, t, kind_s, has_S, lam)
    ck.done()


# ---- the 1024 limit ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scalar", [0, 1], ids=["f64", "f32"])
@pytest.mark.parametrize("name,kind", [("track1024", 2), ("track1024", 1), ("track1024", 0), ("track1025", 2)],
                         ids=["1024-chol", "1024-qrchol", "1024-qrkit", "1025-chol"])
def test_a_track_of_1024_observations(ba, O, gpu_ok, monkeypatch, name, kind, scalar):
    """One point of 1024 observations -- 16 slots of each of the 64 lanes of k_elim_qr<64, 16> full -- and of 1025 under CHOLESKY, which has
    no limit: the same checks at lambda0 (540 k pair entries: 12 s of quad assembly on the host per scalar type, shared by the kinds).
    Measured worst, GPU (oracle), fp64 / fp32: S 1.5e-15 (7.6e-15) / 1.2e-6 (1.7e-5), rhs 1.7e-15 / 4.2e-7, eta 4.7e-17 / 2.4e-8, backsub
    3.7e-16 / 1.2e-7, qr_eta 5.6e-18 (4.0e-17) / 1.1e-8, energy 2.5e-14 / 1.7e-6, e_test 1.9e-14 / 2.2e-5 (the closest to a bound in this file: 5e-5)."""
    kind_s, has_S = moreqr_route(kind, monkeypatch, O)
    p, facts = SP.get(ba, name)
    ck = Checker("shapes[%s,%s,%s]" % (name, KIND_IDS[kind], "f64" if scalar == 0 else "f32"))
    t = Trial(ba, O, p, kind_s, scalar, ck)
    t.check_linearization()
    for lam in lambdas(ba, t, kind, both=False):
        check_trial(ba, O, t, kind_s, has_S, lam)
    ck.done()


@pytest.mark.parametrize("scalar", [0, 1], ids=["f64", "f32"])
@pytest.mark.parametrize("kind", ["QRCHOL", "QRKIT", "MOREQR"])
def test_a_track_of_1025_observations_is_refused_by_the_qr_eliminations(ba, gpu_ok, monkeypatch, kind, scalar):
    monkeypatch.delenv("BA_MOREQR_QR", raising=False)
    p, facts = SP.get(ba, "track1025")
    assert facts["kmax"] == 1025
    with pytest.raises(ba.BAError) as err:
        ba.Solver(p, getattr(ba, kind), scalar)
    assert err.value.code == ba.ERR_ARG


# ---- the persistent chunk walk ---------------------------------------------------------------------------------------------------------
DEALINGS = ((("BA_SCHUR_WGS", "1"), ("BA_SCHUR_BANDS", "1"), ("BA_SCHUR_WINDOW", "0")),
            (("BA_SCHUR_WGS", "1"), ("BA_SCHUR_BANDS", "8"), ("BA_SCHUR_WINDOW", "0")),
            (("BA_SCHUR_WGS", "1"), ("BA_SCHUR_BANDS", "8"), ("BA_SCHUR_WINDOW", "1")),
            ())


@pytest.mark.parametrize("scalar", [0, 1], ids=["f64", "f32"])
@pytest.mark.parametrize("kind", [2, 1], ids=["chol", "qrchol"])
def test_walks_of_three_chunks_and_more(ba, O, gpu_ok, monkeypatch, kind, scalar):
    """`walk` under BA_SCHUR_WGS=1: 5497 chunks on at most 4 x CUs wavefronts, so that by pigeonhole some wavefront of k_schur_pairs walks
    three chunks or more (on 256 CUs: 5.4 on average) and the rotation of its prefetched descriptors goes round; the bands and windows
    change which chunks meet in a list.  The first dealing against quad (lambda = 3e-4, as test_schur_assembly_does_not_depend_on_the_dealing);
    S, rhs, the step and the trial's scalars of the other dealings -- the last one the default, about one chunk per wavefront -- are the
    same bits.  Measured worst, GPU (oracle), fp64 / fp32: S 8.3e-15 (7.6e-15) / 6.5e-6 (3.5e-6), rhs 1.2e-14 (1.2e-14) / 9.1e-6 (2.4e-6),
    eta 3.1e-17 / 1.2e-8, backsub 4.3e-16 / 2.1e-7; every dealing the same bits."""
    p, facts = SP.get(ba, "walk")
    assert facts["nchunks"] >= 12 * gpu_ok[1], (facts["nchunks"], gpu_ok)
    lam, ref = 3e-4, None
    for deal in DEALINGS:
        for var in ("BA_SCHUR_WGS", "BA_SCHUR_BANDS", "BA_SCHUR_WINDOW"):
            monkeypatch.delenv(var, raising=False)
        for var, val in deal:
            monkeypatch.setenv(var, val)
        if ref is None:
            ck = Checker("shapes[walk,%s,%s]" % (KIND_IDS[kind], "f64" if scalar == 0 else "f32"))
            t = Trial(ba, O, p, kind, scalar, ck)
            dx, S, rhs = check_trial(ba, O, t, kind, True, lam)
            ck.done()
            # (Trial.step's try_step scalars, read again from a second call: the trial is a function of the linearisation and lambda)
            ref = (S.copy(), rhs.copy(), dx.copy(), t.s.try_step(lam))
            assert np.array_equal(t.s.get(ba.GET_S), ref[0]) and np.array_equal(t.s.get(ba.GET_DX), ref[2])
            del t
        else:
            s = ba.Solver(p, kind, scalar)
            s.keep_intermediates(True)
            s.linearize()
            out = s.try_step(lam)
            got = (s.get(ba.GET_S), s.get(ba.GET_RHS), s.get(ba.GET_DX), out)
            del s
            assert all(np.array_equal(a, b) for a, b in zip(got[:3], ref[:3])) and got[3] == ref[3], deal
