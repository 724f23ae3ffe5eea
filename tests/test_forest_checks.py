"""CPU: tests/forest_checks.py pinned -- the forest rule, M, the factor and the two sweeps against a dense long double solve of M; the
planted defects against the metrics tests/test_gpu_forest_precond.py uses; ba_relpose_forest_plan (host only) against the Python rule."""
import numpy as np
import pytest

import forest_checks as FC
import pcg_checks as PC
import relpose_checks as RC

LD = np.longdouble

# name: (N, pairs, max_tree, kept expected)
GRAPHS = {
    "chain": (7, [(a, a + 1) for a in range(6)], 7, [1] * 6),
    "star": (6, [(2, 0), (1, 2), (2, 3), (5, 2), (2, 4)], 6, [1] * 5),
    "cycle": (5, [(0, 1), (1, 2), (2, 3), (3, 4), (4, 0)], 5, [1, 1, 1, 1, 0]),
    "two components": (8, [(0, 1), (5, 6), (1, 2), (6, 7), (4, 5)], 8, [1] * 5),
    "chain cut by max_tree": (10, [(a, a + 1) for a in range(9)], 4, [1, 1, 1, 0, 1, 1, 1, 0, 1]),
}


@pytest.mark.parametrize("name", list(GRAPHS))
def test_sweeps_equal_a_dense_solve_of_M(name):
    N, pairs, max_tree, kept = GRAPHS[name]
    pl = FC.plan(N, pairs, max_tree)
    assert list(pl["kept"].astype(int)) == kept
    assert max(len(t) for t in pl["trees"]) <= max_tree and sorted(pl["order"]) == list(range(N))
    for t in pl["trees"]:  # the root is the lowest camera and comes last; every child comes before its parent
        assert t[-1] == min(t) and pl["parent"][t[-1]] == -1
        where = {c: k for k, c in enumerate(t)}
        assert all(where[c] < where[int(pl["parent"][c])] for c in t[:-1])
    S, rhs, B, H = FC.synthetic(N, pairs, seed=3 + N, stiff=3.0)
    M = FC.dense_M(B, H, pairs, pl["kept"])
    assert np.linalg.eigvalsh(M.astype(np.float64)).min() > 0
    Dinv, G, ok = FC.factor(B, H, pairs, pl)
    assert ok.all()
    z = FC.apply(pl, Dinv, G, rhs)
    z_ref = RC._solve(M, rhs)
    err = float(np.abs(z - z_ref).max() / np.abs(z_ref).max())
    print("FOREST %s sweeps vs dense solve %.2e" % (name, err))
    assert err < 1e-15, err
    # the working-precision restatement is the same operator up to its rounding
    for dt, bound in ((np.float64, 1e-11), (np.float32, 1e-3)):
        Dw, Gw, bad = FC.working(B, H, pairs, pl, dt)
        zw = FC.apply(pl, Dw, Gw, rhs.astype(dt))
        assert bad == 0 and float(np.abs(zw - z_ref).max() / np.abs(z_ref).max()) < bound


def test_working_factor_falls_back_per_tree():
    """A tree whose D loses positive definiteness in the factor's arithmetic runs on the block-Jacobi inverses of its B_a; the other
    trees keep their factor."""
    N, pairs = 6, [(0, 1), (1, 2), (3, 4), (4, 5)]
    pl = FC.plan(N, pairs, 3)
    S, rhs, B, H = FC.synthetic(N, pairs, seed=5)
    H = H.copy()
    H[0] *= 50  # (M is indefinite now: the first tree's root block goes negative)
    Dinv, G, ok = FC.factor(B, H, pairs, pl, np.float64)
    assert not ok[[0, 1, 2]].all() and ok[[3, 4, 5]].all()
    Dw, Gw, bad = FC.working(B, H, pairs, pl, np.float64)
    Bj, _ = PC.invert_blocks(B.astype(np.float64), np.float64)
    assert bad == 1 and not Gw[[0, 1, 2]].any() and Gw[[4, 5]].any()
    assert np.array_equal(Dw[:3], Bj[:3])


def _stiff_chain(N=24, seed=9):
    pairs = [(a, a + 1) for a in range(N - 1)]
    S, rhs, B, H = FC.synthetic(N, pairs, seed=seed, stiff=30.0)
    return N, pairs, S, rhs, B, H


def test_forest_needs_fewer_iterations_on_a_stiff_chain():
    N, pairs, S, rhs, B, H = _stiff_chain()
    Mi, ok = PC.invert_blocks(B)
    k_bj = FC.pcg(S, rhs, FC.block_jacobi(Mi), 2000, 1e-8)
    assert k_bj["converged"] and k_bj["iters"] == PC.pcg(S, rhs, Mi, 2000, 1e-8)["iters"]  # (the callback PCG is pcg_checks')
    its = {}
    for mt in (1, 4, 8, N):
        pl = FC.plan(N, pairs, mt)
        Dinv, G, ok = FC.factor(B, H, pairs, pl)
        out = FC.pcg(S, rhs, FC.forest(pl, Dinv, G), 2000, 1e-8)
        assert out["converged"]
        its[mt] = out["iters"]
    print("FOREST stiff chain iterations: block Jacobi %d, forest %s" % (k_bj["iters"], its))
    assert its[1] == k_bj["iters"] and its[N] * 3 <= k_bj["iters"] and its[N] <= its[8] <= its[4] <= its[1]


def test_planted_defects_are_caught():
    """The three defects a kernel of the sweeps can have, against the bounds of the GPU test: iterate_error of x_1 ... x_4 above
    10 x the fp32 floor of test_gpu_pcg_stages.py (3e-3), and the iteration count above k_ref + its allowance."""
    N, pairs, S, rhs, B, H = _stiff_chain()
    KS = (1, 2, 3, 4)
    pl = FC.plan(N, pairs, 8)
    Dinv, G, _ = FC.factor(B, H, pairs, pl)
    good = FC.pcg(S, rhs, FC.forest(pl, Dinv, G), 2000, 1e-8, keep=KS)
    allowed = good["iters"] + int(np.floor(min(0.44 * good["iters"] + 2, good["iters"] / 4)))
    Dbad, Gbad, _ = FC.factor(B, H, pairs, pl, skip_update=pl["trees"][1][0])
    defects = {
        "backward term dropped": dict(prec=lambda r: FC.apply(pl, Dinv, G, r, drop_backward=True)),
        "child's update of D_p skipped": dict(prec=FC.forest(pl, Dbad, Gbad)),
        "a tree's r'z partial left out": dict(prec=FC.forest(pl, Dinv, G), rz_rows=~np.isin(np.arange(9 * N) // 9, pl["trees"][1])),
    }
    for name, kw in defects.items():
        out = FC.pcg(S, rhs, kw["prec"], 2000, 1e-8, keep=KS, rz_rows=kw.get("rz_rows"))
        errs = [PC.iterate_error(out["xs"][k], good["xs"][k], S) for k in KS]
        print("FOREST defect '%s': x_k errors %s, iterations %d (reference %d, allowed %d)"
              % (name, ["%.1e" % e for e in errs], out["iters"], good["iters"], allowed))
        assert errs[0] > 3e-2, (name, errs)
        assert max(errs) > 3e-2, (name, errs)


def _random_multigraph(seed):
    rng = np.random.default_rng(seed)
    N = int(rng.integers(2, 40))
    n = int(rng.integers(0, 3 * N))
    a = rng.integers(0, N, n)
    b = (a + rng.integers(1, N, n)) % N
    return N, np.stack([a, b], axis=1).astype(np.int32), int(rng.integers(1, N + 2))


def test_library_plan_equals_the_rule(ba):
    cases = [(N, np.array(pairs, np.int32), mt) for N, pairs, mt, _ in GRAPHS.values()] + [_random_multigraph(s) for s in range(50)]
    cases.append((4, np.zeros((0, 2), np.int32), 3))
    for N, pairs, mt in cases:
        got, want = ba.forest_plan(N, pairs, mt), FC.plan(N, pairs, mt)
        for key in ("parent", "via", "order", "kept"):
            assert np.array_equal(got[key], want[key]), (key, N, pairs.tolist(), mt, got[key], want[key])
    for N, pairs, mt in ((3, [(0, 0)], 2), (3, [(0, 3)], 2), (3, [(-1, 1)], 2), (3, [(0, 1)], 0), (3, [(0, 1)], -2)):
        with pytest.raises(ba.BAError) as e:
            ba.forest_plan(N, pairs, mt)
        assert e.value.code == ba.ERR_ARG
