"""The projected PCG of tests/shared_checks.py against the dense solve of (P'SP) y = P' rhs, and ba_intrinsics_group_plan through the
Python binding.  No GPU needed.

On random symmetric positive definite S with random groups the long double projected PCG converges to P y and its iterates stay in
range(Pi) bit for bit; the same comparison fails for a PCG that does not project z and for one that projects by the sum -- which is
what lets tests/test_gpu_shared_intrinsics.py claim that it would notice such a kernel."""
import numpy as np
import pytest

import pcg_checks as PC
import shared_checks as SH

LD = np.longdouble


def _random_system(N, seed):
    """A random SPD S [9N, 9N] with strong 9 x 9 diagonal blocks (what a reduced camera matrix looks like to block Jacobi) and rhs."""
    rng = np.random.default_rng(seed)
    D = 9 * N
    A = rng.standard_normal((D, D)) / np.sqrt(D)
    S = 0.3 * (A @ A.T)
    for a in range(N):
        B = rng.standard_normal((9, 12))
        S[9 * a:9 * a + 9, 9 * a:9 * a + 9] += B @ B.T / 12 + 0.05 * np.eye(9)
    sc = np.tile(10.0 ** rng.uniform(-2, 2, 9), N)  # (columns of very different units, as T, omega, f, k1, k2 are)
    S = S * sc[:, None] * sc[None, :]
    rhs = rng.standard_normal(D) * sc
    Minv, ok = PC.invert_blocks(PC.exact_blocks(S, N))
    assert ok.all()
    return S, rhs, Minv


def _labels(N, what, seed):
    rng = np.random.default_rng(seed + 1)
    g = np.full(N, -1, np.int32)
    if what == "all":
        g[:] = 4
        return g
    size = {"pairs": 2, "triples": 3}[what]
    perm = rng.permutation(N)
    for k in range((N - 2) // size):  # (two cameras at least stay ungrouped)
        g[perm[size * k:size * k + size]] = 100 - k
    return g


@pytest.mark.parametrize("what", ["pairs", "triples", "all"])
@pytest.mark.parametrize("N", [7, 12])
def test_projected_pcg_converges_to_the_dense_solution(N, what):
    S, rhs, Minv = _random_system(N, 10 * N + len(what))
    groups = SH.groups_of(N, _labels(N, what, N))
    assert groups and all(len(m) == {"pairs": 2, "triples": 3, "all": N}[what] for m in groups)
    info = {}
    xd = SH.dense_solve(S, rhs, groups, info)
    assert info["rel_residual"] < 1e-17, info
    # P y against P itself: the residual of the projected system vanishes, and x is in range(P)
    P = SH.lift_matrix(N, groups)
    assert float(np.abs(P.T @ (rhs.astype(LD) - S.astype(LD) @ xd)).max()) < 1e-15 * float(np.abs(P.T @ rhs).max())
    assert np.array_equal(SH.project(xd, groups), xd) or float(np.abs(SH.project(xd, groups) - xd).max()) < 1e-18 * float(np.abs(xd).max())
    good = SH.projected_pcg(S, rhs, SH.block_prec(Minv), groups, 400, 1e-16)
    err = PC.iterate_error(good["x"], xd, S)
    print("SHARED N %d %s: %d groups, %d iterations, error %.2e, range spread %.1e, residual %.2e" %
          (N, what, len(groups), good["iters"], err, good["in_range"], SH.projected_rel_residual(S, good["x"], rhs, groups)))
    assert good["converged"] and err < 1e-13, (good["iters"], err)
    assert good["in_range"] == 0.0  # every iterate holds the same bits in rows 6..8 of a group's members
    assert SH.projected_rel_residual(S, good["x"], rhs, groups) < 1e-15
    # planted defects: the same comparison must fail, by orders of magnitude
    for defect, kw in (("z_not_projected", dict(project_z=False)), ("sum_for_mean", dict(mean=False))):
        bad = SH.projected_pcg(S, rhs, SH.block_prec(Minv), groups, 400, 1e-16, **kw)
        eb = PC.iterate_error(bad["x"], xd, S)
        print("SHARED N %d %s: %s error %.2e" % (N, what, defect, eb))
        assert not (eb < 1e-6), (defect, eb)
    # the sum in all three places reaches the same limit (shared_checks' docstring) through other iterates: the comparison of
    # iterates, which the GPU test makes at k = 1, 2, 3, 4, 7, is the one that notices it
    ks = (1, 2, 3, 4, 7)
    ref = SH.projected_pcg(S, rhs, SH.block_prec(Minv), groups, max(ks), keep=ks)
    y64 = SH.projected_pcg(S, rhs, SH.block_prec(Minv, np.float64), groups, max(ks), dtype=np.float64, keep=ks)
    allsum = SH.projected_pcg(S, rhs, SH.block_prec(Minv), groups, max(ks), keep=ks, mean=False, mean_rhs=False)
    base = max(PC.iterate_error(y64["xs"][k], ref["xs"][k], S) for k in ks)
    worst = max(PC.iterate_error(allsum["xs"][k], ref["xs"][k], S) for k in ks)
    print("SHARED N %d %s: iterates fp64 yardstick %.2e, sum in all three places %.2e" % (N, what, base, worst))
    assert base <= 1e-12 and worst >= 100 * max(base, 1e-17), (base, worst)


def test_projected_pcg_without_groups_is_the_plain_pcg():
    S, rhs, Minv = _random_system(6, 3)
    a = SH.projected_pcg(S, rhs, SH.block_prec(Minv), [], 9, keep=(1, 4, 9))
    b = PC.pcg(S, rhs, Minv, 9, keep=(1, 4, 9))
    for k in (1, 4, 9):
        assert np.array_equal(a["xs"][k], b["xs"][k])


# ---- ba_intrinsics_group_plan ------------------------------------------------------------------------------------------------------------
def _same_plan(got, want):
    for k in ("group_ptr", "members", "chunk_ptr", "chunk_group"):
        assert np.array_equal(got[k], want[k]), (k, got[k], want[k])


def test_plan_canonical_numbering_and_interleaved_membership(ba):
    g = [0, 1, 0, -1, 1, 0]
    pl = ba.intrinsics_group_plan(6, g)
    assert list(pl["group_ptr"]) == [0, 3, 5] and list(pl["members"]) == [0, 2, 5, 1, 4]
    assert list(pl["chunk_ptr"]) == [0, 3, 5] and list(pl["chunk_group"]) == [0, 1]
    _same_plan(pl, SH.plan(6, g))
    # the labels' values play no part: groups are numbered by their lowest member
    pl2 = ba.intrinsics_group_plan(6, [70, 3, 70, -5, 3, 70])
    _same_plan(pl2, pl)
    pl3 = ba.intrinsics_group_plan(6, [3, 70, 3, -1, 70, 3])
    _same_plan(pl3, pl)
    # chunk = 1 and chunk = 2
    assert list(ba.intrinsics_group_plan(6, g, 1)["chunk_ptr"]) == [0, 1, 2, 3, 4, 5]
    assert list(ba.intrinsics_group_plan(6, g, 1)["chunk_group"]) == [0, 0, 0, 1, 1]
    assert list(ba.intrinsics_group_plan(6, g, 2)["chunk_ptr"]) == [0, 2, 3, 5]
    assert list(ba.intrinsics_group_plan(6, g, 2)["chunk_group"]) == [0, 0, 1]


def test_plan_drops_singleton_labels(ba):
    g = [5, 9, 5, 7, -1, 8]
    pl = ba.intrinsics_group_plan(6, g)
    assert list(pl["group_ptr"]) == [0, 2] and list(pl["members"]) == [0, 2] and list(pl["chunk_group"]) == [0]
    for none in ([-1] * 6, [0, 1, 2, 3, 4, 5], [-3, 4, -1, -1, -2, 9]):
        pl = ba.intrinsics_group_plan(6, none)
        assert list(pl["group_ptr"]) == [0] and len(pl["members"]) == 0 and list(pl["chunk_ptr"]) == [0] and len(pl["chunk_group"]) == 0
    pl = ba.intrinsics_group_plan(0, np.zeros(0, np.int32))
    assert list(pl["group_ptr"]) == [0] and list(pl["chunk_ptr"]) == [0]


def test_plan_chunk_boundaries(ba):
    """Groups of 255, 256, 257 and 513 cameras with chunk = 256 (1, 1, 2 and 3 chunks), interleaved over the cameras, plus loners."""
    sizes = (255, 256, 257, 513)
    rng = np.random.default_rng(8)
    N = sum(sizes) + 40
    g = np.full(N, -1, np.int32)
    perm = rng.permutation(N)
    at = 0
    for k, n in enumerate(sizes):
        g[perm[at:at + n]] = 10 + k
        at += n
    pl = ba.intrinsics_group_plan(N, g)
    _same_plan(pl, SH.plan(N, g))
    order = np.argsort([perm[sum(sizes[:k]):sum(sizes[:k + 1])].min() for k in range(4)])  # the groups by their lowest member
    want_sizes = [sizes[k] for k in order]
    assert list(np.diff(pl["group_ptr"])) == want_sizes
    lens = np.diff(pl["chunk_ptr"])
    want = []
    for k, n in enumerate(want_sizes):
        want += [(k, 256)] * (n // 256) + ([(k, n % 256)] if n % 256 else [])
    assert list(zip(pl["chunk_group"], lens)) == want
    assert lens.max() == 256 and len(lens) == 1 + 1 + 2 + 3
    for k in range(4):  # members ascend inside a group and carry one label
        m = pl["members"][pl["group_ptr"][k]:pl["group_ptr"][k + 1]]
        assert np.all(np.diff(m) > 0) and len(set(g[m])) == 1
    pl1 = ba.intrinsics_group_plan(N, g, 1)
    assert np.array_equal(pl1["chunk_ptr"], np.arange(sum(sizes) + 1)) and np.array_equal(pl1["members"], pl["members"])
    _same_plan(pl1, SH.plan(N, g, 1))


def test_plan_refusals(ba):
    g = np.array([0, 0, 1], np.int32)
    for args in ((-1, g, 256), (3, None, 256), (3, g, 0), (3, g, -4)):
        with pytest.raises(ba.BAError) as e:
            ba.intrinsics_group_plan(*args)
        assert e.value.code == ba.ERR_ARG
    assert list(ba.intrinsics_group_plan(0, None)["group_ptr"]) == [0]  # (N = 0 needs no labels)
    # the binding refuses what the C code would misread: fewer labels than cameras, labels that are no integers or do not fit an int
    for bad in ([0, 0], np.zeros((2, 5), np.int32), np.zeros(10), np.array([0, 2 ** 31] * 5)):
        with pytest.raises(ValueError):
            ba.intrinsics_group_plan(10, bad)
    assert list(ba.intrinsics_group_plan(4, np.array([7, 7, -1, 7], np.int64))["members"]) == [0, 1, 3]
