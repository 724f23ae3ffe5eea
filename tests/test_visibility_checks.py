"""CPU: tests/visibility_checks.py pinned -- ba_problem_covisibility (host only) against the brute-force rule; the 9 x 9 factor and the
two sweeps against a dense long double solve of M on the oracle's S; the inputs of tests/test_gpu_visibility_forest.py's cases (M positive
definite); the iteration gain of the references; the planted defects against that file's bound."""
import numpy as np
import pytest

import forest_checks as FC
import pcg_checks as PC
import relpose_checks as RC
import visibility_checks as VC
from conftest import to_oracle
from test_gpu_forest_precond import System
from test_gpu_parity import _ragged_problem
from test_gpu_stages import sorted_oracle_problem

LD = np.longdouble


# ---- co-visibility -------------------------------------------------------------------------------------------------------------------------
def _same_lists(ba, p, track_max=0):
    a = p.arrays()
    pairs, weight = p.covisibility(track_max)
    want_p, want_w = VC.covisibility(p.N, a["cam_idx"], a["pt_idx"], track_max)
    assert pairs.dtype == np.int32 and pairs.shape == want_p.shape and np.array_equal(pairs, want_p) and np.array_equal(weight, want_w)
    assert (pairs[:, 0] < pairs[:, 1]).all()
    return pairs, weight


def _shuffled(ba, p, seed):
    a = p.arrays()
    perm = np.random.default_rng(seed).permutation(p.K)
    return ba.Problem.from_arrays(p.N, p.M, p.K, a["cam_idx"][perm], a["pt_idx"][perm], a["meas"].reshape(-1, 2)[perm].ravel(), a["cams9"], a["pts"])


def _long_track_problem(ba):
    """synthetic(9, 40, 160, 5) with point 3 seen by seven cameras (one of them twice): longer than track_max = 3."""
    p = ba.Problem.synthetic(9, 40, 160, 5)
    a = p.arrays()
    keep = a["pt_idx"] != 3
    cams = np.array([8, 1, 6, 2, 4, 0, 7, 6], np.int32)
    cam_idx = np.concatenate([a["cam_idx"][keep], cams])
    pt_idx = np.concatenate([a["pt_idx"][keep], np.full(len(cams), 3, np.int32)])
    meas = np.concatenate([a["meas"].reshape(-1, 2)[keep], np.zeros((len(cams), 2))])
    return ba.Problem.from_arrays(p.N, p.M, len(cam_idx), cam_idx, pt_idx, meas.ravel(), a["cams9"], a["pts"])


def test_covisibility_equals_the_rule(ba, prob21, prob39):
    for p in (prob21, prob39, _ragged_problem(ba), VC.twice_problem(ba)):
        pairs, weight = _same_lists(ba, p)
        again, w2 = _shuffled(ba, p, 7).covisibility()
        assert np.array_equal(pairs, again) and np.array_equal(weight, w2)
    n21 = len(prob21.covisibility()[0])
    print("VIS problem-21: %d of %d pairs co-visible; problem-39: %d of %d" % (n21, 21 * 20 // 2, len(prob39.covisibility()[0]), 39 * 38 // 2))
    _same_lists(ba, ba.Problem.synthetic(2100, 3000, 9000, 2))  # (beyond the dense counts: sorted keys)
    lt = _long_track_problem(ba)
    for tm in (3, 6, 7, 0):
        _same_lists(ba, lt, tm)
        a, b = lt.covisibility(tm), _shuffled(ba, lt, 3).covisibility(tm)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    short, full = lt.covisibility(3), lt.covisibility(7)
    assert len(short[0]) < len(full[0])  # (the long track gave its adjacent pairs alone)
    # a camera that sees a point twice counts once: the list of the problem without the two extra observations
    tw = VC.twice_problem(ba)
    a = tw.arrays()
    base = ba.Problem.from_arrays(tw.N, tw.M, tw.K - 2, a["cam_idx"][:-2], a["pt_idx"][:-2], a["meas"][:-4], a["cams9"], a["pts"])
    assert all(np.array_equal(x, y) for x, y in zip(tw.covisibility(), base.covisibility()))
    # refusals
    import ctypes as C
    n = C.c_longlong(0)
    assert ba.lib().ba_problem_covisibility(tw._h, -1, C.byref(n), None, None) == ba.ERR_ARG
    assert ba.lib().ba_problem_covisibility(None, 0, C.byref(n), None, None) == ba.ERR_ARG
    assert ba.lib().ba_problem_covisibility(tw._h, 0, None, None, None) == ba.ERR_ARG


# ---- the systems: the oracle's J at the start state ----------------------------------------------------------------------------------------
_SYS = {}


def _problem(ba, name, prob21, prob39):
    return {"p21": lambda: prob21, "p39": lambda: prob39, "ragged": lambda: _ragged_problem(ba), "twice": lambda: VC.twice_problem(ba),
            "syn257": lambda: ba.Problem.synthetic(257, 12 * 257, 60 * 257, 4257)}[name]()


def _system(ba, O, prob21, prob39, name, with_cs=False, masked=False, lam_rel=VC.LAM_REL):
    """(System of the oracle's linearisation of the problem at its start state -- what the GPU test builds from the device's J --,
    the constraints, the co-visibility pairs)."""
    key = (name, with_cs, masked, lam_rel)
    if key not in _SYS:
        pg = _problem(ba, name, prob21, prob39)
        po = sorted_oracle_problem(O, pg)
        cam = O.init_cams(po)
        f, e = O.residuals(po, cam, po.pts)
        Jc, Jp = O.jacobian(po, cam, po.pts)
        Jc = np.array(Jc).reshape(po.K, 2, 9)
        cm = pg.gauge_mask(0) if masked else None
        if masked:
            free = ((np.asarray(cm, np.int64)[:, None] >> np.arange(9)[None, :]) & 1) == 0
            Jc = Jc * free[po.cam_idx][:, None, :]
        dmax = O.step(O.CHOLESKY | O.ASSEMBLE_ONLY, po, Jc, Jp, f, 1.0, want_S=False)["diagmax"]
        cs = RC.Constraints()
        if with_cs:
            V = np.zeros((po.N, 9))
            np.add.at(V, po.cam_idx, (Jc ** 2).sum(axis=1))
            cs = RC.standard_constraints(po.N, po.cam_idx, po.pt_idx, cam, V)[0]
        Y = System(O, po, Jc, np.array(Jp).reshape(po.K, 2, 3), f, np.zeros(3 * po.M + 9 * po.N), cam, cs, cm, lam_rel * dmax)
        _SYS[key] = (Y, cs, pg.covisibility()[0])
    return _SYS[key]


def _forest(Y, cs, cov, max_tree):
    pl, L = VC.plan(Y.N, cs.pairs, cov, max_tree or Y.N)
    return pl, L, VC.cross_blocks(Y.S_ld, L, pl["kept"])


def test_sweeps_equal_a_dense_solve_of_M(ba, O, prob21, prob39):
    """On the oracle's S of problem-21, one tree and trees of 4: test_forest_checks.py's bound."""
    Y, cs, cov = _system(ba, O, prob21, prob39, "p21")
    for mt in (0, 4):
        pl, L, X = _forest(Y, cs, cov, mt)
        assert max(len(t) for t in pl["trees"]) <= (mt or Y.N) and pl["kept"].sum() == sum(len(t) - 1 for t in pl["trees"])
        M = VC.dense_M(Y.B, X, L, pl["kept"])
        assert np.array_equal(M, M.T) and VC.min_eig(M) > 0
        Dinv, G, ok = VC.factor(Y.B, X, L, pl)
        assert ok.all() and np.abs(G[:, 6:, :]).max() > 0 and np.abs(G[:, :, 6:]).max() > 0
        z = FC.apply(pl, Dinv, G, Y.rhs_ld)
        z_ref = RC._solve(M, Y.rhs_ld)
        err = float(np.abs(z - z_ref).max() / np.abs(z_ref).max())
        print("VIS p21 max_tree %d sweeps vs dense solve %.2e" % (mt or Y.N, err))
        assert err < 1e-15, err
        for dt, bound in ((np.float64, 1e-11), (np.float32, 1e-3)):
            Dw, Gw, bad = VC.working(Y.B, X, L, pl, dt)
            zw = FC.apply(pl, Dw, Gw, Y.rhs_ld.astype(dt))
            assert bad == 0 and float(np.abs(zw - z_ref).max() / np.abs(z_ref).max()) < bound


@pytest.mark.parametrize("case", list(VC.GPU_CASES))
def test_inputs_of_the_gpu_cases(ba, O, prob21, prob39, case):
    """M is positive definite for every case of the GPU test, and its long double factor finds it so."""
    name, mt, with_cs, masked = VC.GPU_CASES[case]
    Y, cs, cov = _system(ba, O, prob21, prob39, name, with_cs, masked)
    pl, L, X = _forest(Y, cs, cov, mt)
    assert pl["kept"].sum() > 0
    lo = VC.min_eig(VC.dense_M(Y.B, X, L, pl["kept"]))
    print("VIS %s: %d trees, %d kept of %d, largest %d, min eig of the scaled M %.2e" % ((case,) + FC.counts(pl)[:2] + (len(L), FC.counts(pl)[3], lo)))
    assert lo > 0
    assert VC.factor(Y.B, X, L, pl)[2].all()
    for dt in (np.float64, np.float32):
        assert VC.working(Y.B, X, L, pl, dt)[2] == 0
    if with_cs:  # the constraint edges come first: every one the constraint forest keeps is kept here, with H_ab inside X
        kept_cs = FC.plan(Y.N, cs.pairs, mt or Y.N)["kept"]
        assert np.array_equal(pl["kept"][:len(cs)], kept_cs) and kept_cs.sum() > 0
        q = int(np.flatnonzero(kept_cs)[0])
        assert np.abs(Y.H[q]).max() > 0


def test_the_forest_reference_needs_fewer_iterations(ba, O, prob21, prob39):
    """problem-39 at lambda = 1e-6 max diag and rel_tol 1e-8, one tree: at most 3 / 4 of block Jacobi's iterations (31 against 54)."""
    Y, cs, cov = _system(ba, O, prob21, prob39, "p39")
    pl, L, X = _forest(Y, cs, cov, 0)
    Dinv, G, ok = VC.factor(Y.B, X, L, pl)
    assert ok.all()
    k_fo = FC.pcg(Y.S_ld, Y.rhs_ld, FC.forest(pl, Dinv, G), 1000, 1e-8)
    k_bj = Y.block_jacobi_reference(1000, 1e-8)
    print("VIS problem-39 reference iterations: block Jacobi %d, forest %d" % (k_bj["iters"], k_fo["iters"]))
    assert k_fo["converged"] and k_bj["converged"] and 4 * k_fo["iters"] <= 3 * k_bj["iters"]


def test_planted_defects_are_caught(ba, O, prob21, prob39):
    """Each defect moves x_1 on problem-21 (one tree) beyond the largest bound the GPU test can have there: max(10 x the fp32 yardstick,
    the fp32 floor)."""
    from test_gpu_pcg_stages import FLOOR
    Y, cs, cov = _system(ba, O, prob21, prob39, "p21")
    pl, L, X = _forest(Y, cs, cov, 0)
    Dinv, G, _ = VC.factor(Y.B, X, L, pl)
    good = FC.pcg(Y.S_ld, Y.rhs_ld, FC.forest(pl, Dinv, G), 1, keep=(1,))["xs"][1]
    Dw, Gw, bad = VC.working(Y.B, X, L, pl, np.float32)
    y32 = FC.pcg(Y.S_ld, Y.rhs_ld.astype(np.float32), FC.forest(pl, Dw, Gw), 1, dtype=np.float32, keep=(1,), V=Y.V)["xs"][1]
    bound = max(10 * PC.iterate_error(y32, good, Y.S), FLOOR[("iterate", 1)])
    leaf = pl["trees"][0][0]
    Dn, Gn, okn = VC.factor(Y.B, X, L, pl, narrow=True)
    if not okn.all():  # (that M is indefinite: a kernel with this defect takes the tree-wide fallback, which the GPU test also counts)
        Dn, Gn = PC.invert_blocks(Y.B)[0], np.zeros_like(Gn)
        print("VIS defect 'the 6-wide cross block' leaves M indefinite: the tree falls back to block Jacobi")
    Ds, Gs, _ = VC.factor(Y.B, X, L, pl, skip_update=leaf)
    defects = {"the 6-wide cross block": FC.forest(pl, Dn, Gn), "a child's update of D_parent skipped": FC.forest(pl, Ds, Gs),
               "backward term dropped": lambda r: FC.apply(pl, Dinv, G, r, drop_backward=True)}
    for what, prec in defects.items():
        err = PC.iterate_error(FC.pcg(Y.S_ld, Y.rhs_ld, prec, 1, keep=(1,))["xs"][1], good, Y.S)
        print("VIS defect '%s': x_1 error %.2e, bound %.2e" % (what, err, bound))
        assert bad == 0 and np.isfinite(err) and err > bound, (what, err, bound)
