"""The problems of tests/shape_problems.py on the CPU alone: every design holds the shapes it names, the library's structure agrees with the
numpy restatement, the CPU oracle gets through them within the bounds of tests/test_gpu_shapes.py, and the stage metrics report one lost
observation at exactly the places the designs were made for.  No GPU needed."""
import numpy as np
import pytest

import shape_problems as SP
import stage_checks as SC
from conftest import to_oracle
from test_gpu_stages import BOUND, EPS

LAM_HIGH = 10.0


# ---- builders ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(SP.DESIGNS))
def test_builders_hold_their_shapes_and_agree_with_the_library(ba, name):
    """Each builder asserts its own shapes (SP.get raises otherwise); ba_shard_plan -- ba_build_structure with chunks of 64 -- counts the
    same entries, chunks and camera pairs as the numpy restatement; the output is sorted by point."""
    p, facts = SP.get(ba, name)
    plan = p.shard_plan(0, 1)
    assert (plan["entries"], plan["chunks"], plan["pairs"]) == (facts["E"], facts["nchunks"], facts["npairs"])
    assert plan["was_sorted"] == 1 and (plan["p1"], plan["o1"]) == (p.M, p.K)
    if name == "walk":
        assert plan["chunks"] >= 12 * 256
    if name in ("track1024", "track1025"):
        assert facts["E"] < 600000  # (the quad referee's cost goes with E)
    else:
        assert facts["E"] < 150000


def test_structure_restatement_against_the_rule_spelled_out():
    """structure() counts entries as the lower triangle of C'C; here the rule of ba_build_structure observation pair by observation pair, on
    a small list with a camera seen three times by one point."""
    cam = np.array([0, 2, 2, 1, 2, 0, 1, 1, 2])
    pt = np.array([0, 0, 0, 0, 0, 1, 1, 3, 3])
    N, M = 3, 4
    want = np.zeros((N, N), np.int64)
    for j in range(M):
        idx = np.nonzero(pt == j)[0]
        for i in idx:
            for i2 in idx[idx <= i]:
                a, b = max(cam[i], cam[i2]), min(cam[i], cam[i2])
                want[a, b] += 2 if (i != i2 and cam[i] == cam[i2]) else 1
    f = SP.structure(N, M, cam, pt)
    assert np.array_equal(f["entries"], want) and f["E"] == want.sum() and f["kmax"] == 5 and tuple(f["track"]) == (5, 2, 0, 2)
    assert f["nchunks"] == np.count_nonzero(want) and tuple(f["cam_obs"]) == (2, 3, 4) and f["multiplicity_max"] == 3
    assert f["eval_ranges"] == [0, 9]


# ---- the oracle on the designs ---------------------------------------------------------------------------------------------------------
_LIN, _REF = {}, {}


def lin(ba, O, name, dt):
    """(oracle problem, Jc, Jp, f, dmax) of the oracle's own linearisation in dtype dt at the design's start"""
    if (name, dt) not in _LIN:
        po = to_oracle(SP.get(ba, name)[0])
        cam, pts = O.init_cams(po, dt), po.pts.astype(dt)
        f, _ = O.residuals(po, cam, pts)
        Jc, Jp = O.jacobian(po, cam, pts)
        dmax = O.step(O.CHOLESKY | O.ASSEMBLE_ONLY, po, Jc, Jp, f, 1.0)["diagmax"]
        _LIN[(name, dt)] = (po, Jc, Jp, f, dmax)
    return _LIN[(name, dt)]


def referee(ba, O, name, dt, lam):
    if (name, dt, lam) not in _REF:
        po, Jc, Jp, f, _ = lin(ba, O, name, dt)
        _REF[(name, dt, lam)] = O.referee_reduced_from_jacobian(O.CHOLESKY, po, Jc, Jp, f, lam)
    return _REF[(name, dt, lam)]


def oracle_step(O, kind, po, Jc, Jp, f, lam):
    """O.step as float64 arrays; kind 13: MOREQR by the normal equations (tests/test_gpu_parity.py: moreqr_route)"""
    O.set_more_qr(kind != 13)
    try:
        st = O.step(3 if kind == 13 else kind, po, Jc, Jp, f, lam)
    finally:
        O.set_more_qr(True)
    return {k: np.asarray(st[k], np.float64) for k in ("S", "rhs", "dx", "g")}


@pytest.mark.parametrize("scalar", [0, 1], ids=["f64", "f32"])
@pytest.mark.parametrize("name", ["pairs", "tracks256", "tracks257"])
def test_the_oracle_passes_on_the_designs(ba, O, name, scalar):
    """The fp64 and the fp32 oracle on their own J, CHOLESKY / QRCHOL / MOREQR by the normal equations, at lambda0 = 1e-12 dmax and 10:
    eta and the back-substitution within BOUND (the ordinary eta bound in fp32 too), S and rhs against the quad assembly at or below the
    floors of BOUND -- the yardstick max(10 x oracle, floor) of the GPU test then stays within 10 x floor.  Where the fp32 CHOLESKY
    elimination breaks down at lambda0 (a 3 x 3 point block that is singular in fp32) the yardstick is the fp64 oracle on the same J, scaled
    by eps32 / eps64, as in test_gpu_stages.py::test_assembly_and_backsub -- it does not on these designs.  Measured worst: fp64 S 4.1e-15
    and rhs 2.6e-15 (pairs, CHOLESKY, lambda0), eta 7.2e-17, back-substitution 2.2e-15; fp32 S 3.3e-6 and rhs 2.1e-6 (pairs, CHOLESKY,
    lambda0), eta 2.7e-8, back-substitution 6.6e-7."""
    dt = (np.float64, np.float32)[scalar]
    po, Jc, Jp, f, dmax = lin(ba, O, name, dt)
    for lam in (1e-12 * dmax, LAM_HIGH):
        R = referee(ba, O, name, dt, lam)
        for kind in (2, 1, 13):
            st = oracle_step(O, kind, po, Jc, Jp, f, lam)
            asm = SC.assembly_errors(po, Jc, f, lam, st["S"], st["rhs"], R["S"], R["rhs"], Jp)
            print("ORACLE %s %s kind %d lam %.1e S %.2e rhs %.2e" % (name, dt.__name__, kind, lam, asm["S"], asm["rhs"]))
            if not all(np.isfinite(v) for v in asm.values()):
                assert (scalar, kind) == (1, 2) and lam < LAM_HIGH, (kind, lam, asm)
                s64 = O.step(O.CHOLESKY, po, Jc.astype(np.float64), Jp.astype(np.float64), f.astype(np.float64), lam)
                o64 = SC.assembly_errors(po, Jc, f, lam, s64["S"], s64["rhs"], R["S"], R["rhs"], Jp)
                assert all(np.isfinite(v) and v * EPS[1] / EPS[0] < 1 for v in o64.values()), o64
                continue
            # (at or below the floors of BOUND: the GPU rule max(10 x oracle, floor) then never exceeds 10 x floor, 1e-4 in fp32, far
            # below the 1.6e-3 one lost observation shows)
            assert asm["S"] <= BOUND[("S", scalar)] and asm["rhs"] <= BOUND[("rhs", scalar)], asm
            eta = SC.eta(st["S"], st["dx"][3 * po.M:], st["rhs"])
            bs = SC.backsub_errors(po, Jc, Jp, st["dx"], st["g"], lam)
            print("ORACLE %s %s kind %d lam %.1e eta %.2e backsub %.2e" % (name, dt.__name__, kind, lam, eta, bs))
            assert eta <= BOUND[("eta", scalar)], (kind, lam, eta)
            assert bs <= BOUND[("backsub", scalar)], (kind, lam, bs)


# ---- planted defects -------------------------------------------------------------------------------------------------------------------
def _designed_observations(ba):
    """(design, observation, what): the observations the designs were made for -- the last entry of the 65-, 64- and 1-entry pairs, the
    last observation of the 33-track and of the 257-track"""
    out = []
    _, facts = SP.get(ba, "pairs")
    for n in (65, 64, 1):
        q = SP.PAIR_COUNTS.index(n)
        pts = facts["designed"][q]
        assert len(pts) == n
        out.append(("pairs", int(facts["first_obs"][pts[-1]]), "point %d of the %d-entry pair" % (n, n)))
    for name, k in (("tracks256", 33), ("tracks257", 257)):
        _, facts = SP.get(ba, name)
        j = int(np.nonzero(facts["track"] == k)[0][0])
        out.append((name, int(facts["first_obs"][j]) + k - 1, "observation %d of the %d-track" % (k, k)))
    return out


@pytest.mark.parametrize("which", range(5), ids=["pair65", "pair64", "pair1", "track33", "track257"])
def test_one_lost_observation_shows_in_the_assembly_metric(ba, O, which):
    """S assembled (fp64 oracle, CHOLESKY and QRCHOL, lambda0 and 10) with the camera Jacobian of ONE observation zeroed -- what a wrong mask
    at the last slot of a lane, or a lost last entry of a chunk, leaves behind -- against the quad assembly of the intact J: at least 100x
    the clean value of the metric, every time."""
    name, o, what = _designed_observations(ba)[which]
    po, Jc, Jp, f, dmax = lin(ba, O, name, np.float64)
    Jb = Jc.copy()
    Jb[o] = 0
    for lam in (1e-12 * dmax, LAM_HIGH):
        R = referee(ba, O, name, np.float64, lam)
        for kind in (2, 1):
            st = oracle_step(O, kind, po, Jc, Jp, f, lam)
            ok = SC.assembly_errors(po, Jc, f, lam, st["S"], st["rhs"], R["S"], R["rhs"], Jp)
            sb = oracle_step(O, kind, po, Jb, Jp, f, lam)
            bad = SC.assembly_errors(po, Jc, f, lam, sb["S"], sb["rhs"], R["S"], R["rhs"], Jp)
            print("DEFECT %s kind %d lam %.1e S %.2e -> %.2e" % (what, kind, lam, ok["S"], bad["S"]))
            assert bad["S"] >= 100 * ok["S"] and bad["rhs"] >= 100 * ok["rhs"], (what, kind, lam, ok, bad)


def test_a_point_step_without_its_last_observation_shows_in_the_backsub_metric(ba, O):
    """dx_p of the 33-track's point solved from the point's rows of the normal equations WITHOUT its 33rd observation (the camera step
    unchanged): the back-substitution metric rises to at least 100x its clean value."""
    name = "tracks256"
    _, facts = SP.get(ba, name)
    po, Jc, Jp, f, dmax = lin(ba, O, name, np.float64)
    j = int(np.nonzero(facts["track"] == 33)[0][0])
    o0 = int(facts["first_obs"][j])
    obs = np.arange(o0, o0 + 32)
    assert np.all(po.pt_idx[obs] == j) and po.pt_idx[o0 + 32] == j and (o0 + 33 == po.K or po.pt_idx[o0 + 33] != j)
    for lam in (1e-12 * dmax, LAM_HIGH):
        st = oracle_step(O, 2, po, Jc, Jp, f, lam)
        ok = SC.backsub_errors(po, Jc, Jp, st["dx"], st["g"], lam)
        assert ok <= BOUND[("backsub", 0)]
        dxc = st["dx"][3 * po.M:].reshape(po.N, 9)
        V = np.einsum("krc,krd->cd", Jp[obs], Jp[obs]) + lam * np.eye(3)
        gp = -np.einsum("krc,kr->c", Jp[obs], f.reshape(po.K, 2)[obs])
        w = np.einsum("krc,kr->c", Jp[obs], np.einsum("krc,kc->kr", Jc[obs], dxc[po.cam_idx[obs]]))
        dx = st["dx"].copy()
        dx[3 * j:3 * j + 3] = np.linalg.solve(V, gp - w)
        bad = SC.backsub_errors(po, Jc, Jp, dx, st["g"], lam)
        print("DEFECT backsub lam %.1e %.2e -> %.2e" % (lam, ok, bad))
        assert bad >= 100 * ok, (lam, ok, bad)


def test_the_last_observation_of_the_1024_track_shows_in_the_assembly_metric(ba, O):
    """track1024 at lambda0 (the lambda of the GPU test; 540 k entries: one quad assembly): S from the fp64 oracle, QRCHOL and CHOLESKY, with
    the camera Jacobian of the track's 1024th observation zeroed -- the last slot of the last lane of k_elim_qr<64, 16> -- is at least 100x
    the clean value, and above 10 x the fp32 oracle's error on its own J, the most the GPU test's rule allows an fp32 S there."""
    name = "track1024"
    _, facts = SP.get(ba, name)
    po, Jc, Jp, f, dmax = lin(ba, O, name, np.float64)
    j = int(np.nonzero(facts["track"] == 1024)[0][0])
    o = int(facts["first_obs"][j]) + 1023
    assert po.pt_idx[o] == j and (o + 1 == po.K or po.pt_idx[o + 1] != j)
    lam = 1e-12 * dmax
    R = referee(ba, O, name, np.float64, lam)
    Jb = Jc.copy()
    Jb[o] = 0
    po32, Jc32, Jp32, f32, _ = lin(ba, O, name, np.float32)
    R32 = referee(ba, O, name, np.float32, lam)
    for kind in (1, 2):
        ok = SC.assembly_errors(po, Jc, f, lam, *[oracle_step(O, kind, po, Jc, Jp, f, lam)[k] for k in ("S", "rhs")], R["S"], R["rhs"], Jp)
        bad = SC.assembly_errors(po, Jc, f, lam, *[oracle_step(O, kind, po, Jb, Jp, f, lam)[k] for k in ("S", "rhs")], R["S"], R["rhs"], Jp)
        o32 = SC.assembly_errors(po32, Jc32, f32, lam, *[oracle_step(O, kind, po32, Jc32, Jp32, f32, lam)[k] for k in ("S", "rhs")], R32["S"],
                                 R32["rhs"], Jp32)
        print("DEFECT 1024 kind %d S %.2e -> %.2e (fp32 oracle %.2e)" % (kind, ok["S"], bad["S"], o32["S"]))
        assert bad["S"] >= 100 * ok["S"] and bad["S"] > 10 * max(o32["S"], BOUND[("S", 1)]), (kind, ok, bad, o32)
