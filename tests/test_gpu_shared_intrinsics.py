"""GPU: shared intrinsics for BA_ITERSCHUR (ba_solver_set_shared_intrinsics) against tests/shared_checks.py.

The quad S and rhs come from the GPU's OWN J and residuals (oracle_lib.referee_reduced_from_jacobian), so what is measured is the solve:

  step        a solve at a tight rel_tol against P y of the dense (P'SP) y = P' rhs in long double, lambda = 1e-6 and 1e-2 x max diag J'J
  iterates    x_k, k = 1, 2, 3, 4, 7 of capped solves against the long double projected PCG
  residual    ba_solver_pcg_stats' last_rel_residual under a cap against |Pi (rhs - S x_k)| / |Pi rhs| of the returned x_k

each within the rule of tests/test_gpu_pcg_stages.py: max(10 x what the working-precision CPU yardstick achieves on the same system --
shared_checks.Working: the product and the blocks formed as the library forms them -- , that file's FLOOR).  Then the invariants bit for
bit, the interplay with masks, priors and the forest preconditioner, the refusals, and one capture of one physical camera end to end.
Every state has its groups' intrinsics equalised through set_state first (the BAL files and `synthetic` give every camera its own).
Each value is printed as `PCG <case> <metric> <value> <bound>` (test_gpu_pcg_stages.Checker).
"""
import numpy as np
import pytest

import pcg_checks as PC
import prior_checks as PR
import relpose_checks as RC
import shared_checks as SH
from test_gpu_pcg_stages import FLOOR, KS, LAMS, Checker
from test_gpu_stages import EPS, sorted_oracle_problem

pytestmark = pytest.mark.gpu

LD = np.longdouble
DT = {0: np.float64, 1: np.float32}
SN = {0: "f64", 1: "f32"}
TIGHT = {0: 1e-13, 1: 1e-6}  # rel_tol of the converged solves (the recurrence's residual goes below the working precision's eps |rhs|)
CAP = 1000


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def equalise(ba, s, groups, cams=None):
    """f, k1, k2 of every member <- those of the group's first member, through set_state (points untouched).  Returns the state."""
    cams = (s.get(ba.GET_CAMS) if cams is None else np.array(cams)).reshape(-1, 15).copy()
    for m in groups:
        cams[m, 12:15] = cams[m[0], 12:15]
    s.set_state(cams.ravel(), None)
    return cams.ravel()


def p21_labels(what, N=21):
    g = np.full(N, -1, np.int32)
    if what == "all":
        g[:] = 0
    elif what == "mod3":  # three groups of 7, 7 and 7 cameras less the cameras 0 and 7, which keep their own
        g[:] = np.arange(N) % 3
        g[[0, 7]] = -1
    elif what == "pair":
        g[[3, 11]] = 5
    elif what == "runs":  # consecutive cameras in a group (an odometry chain fits inside)
        g[4:9] = 0
        g[10:16] = 1
    else:
        raise KeyError(what)
    return g


class System:
    """One linearisation of a grouped solver: the quad S and rhs of the GPU's own J (plus what priors / constraints add: `extra` with
    S [9N, 9N], V [N, 9, 9], g [9N] in long double), the documented blocks B_a, V_a + lambda I, per lambda."""

    def __init__(self, ba, O, s, po, dmax, extra=None):
        self.ba, self.O, self.s, self.po, self.dmax, self.extra = ba, O, s, po, dmax, extra
        K = po.K
        self.Jc, self.Jp = s.get(ba.GET_JC).reshape(K, 2, 9), s.get(ba.GET_JP).reshape(K, 2, 3)
        self.f, self.gc = s.get(ba.GET_RESIDUALS), s.get(ba.GET_GRAD)[3 * po.M:]
        self._at, self._work = {}, {}

    def at(self, lam):
        if lam not in self._at:
            D = 9 * self.po.N
            R = self.O.referee_reduced_from_jacobian(self.O.CHOLESKY, self.po, self.Jc, self.Jp, self.f, lam)
            S64 = R["S"].reshape(D, D)
            S, rhs = S64.astype(LD), R["rhs"].astype(LD)
            B, V = PC.documented_blocks(self.po, self.Jc, self.Jp, lam, S64), PC.camera_blocks(self.po, self.Jc, lam)
            if self.extra is not None:
                S, rhs, B, V = S + self.extra["S"], rhs + self.extra["g"], B + self.extra["V"], V + self.extra["V"]
            self._at[lam] = dict(S=S, rhs=rhs, B=B, V=V, S64=S.astype(np.float64))
        return self._at[lam]

    def working(self, lam, dt):
        if (lam, dt) not in self._work:
            a = self.at(lam)
            self._work[(lam, dt)] = SH.Working(a["S"], a["rhs"], a["B"], a["V"], self.gc, dt)
        return self._work[(lam, dt)]

    def yardstick(self, lam, scalar, groups, max_iter, rel_tol=0.0, keep=None):
        """(the working-precision projected PCG, the factor its errors are scaled by): fp32 that breaks down is replaced by fp64 scaled
        by eps32 / eps64 (tests/test_gpu_stages.py's rule)."""
        out = self.working(lam, DT[scalar]).pcg(groups, max_iter, rel_tol, keep)
        if out is not None:
            return out, 1.0, DT[scalar]
        out = self.working(lam, np.float64).pcg(groups, max_iter, rel_tol, keep)
        assert out is not None
        return out, EPS[1] / EPS[0], np.float64


def grouped(ba, O, pg, scalar, group_of, cm=None, before=None, extra=None):
    """(solver with the groups in force at its linearisation, System, groups)."""
    s = ba.Solver(pg, ba.ITERSCHUR, scalar)
    groups = SH.groups_of(pg.N, group_of)
    equalise(ba, s, groups)
    if cm is not None:
        s.set_constant(cm, None)
    if before is not None:
        before(s)
    s.set_shared_intrinsics(group_of)
    info = s.shared_intrinsics_info()
    assert (info["groups"], info["grouped"], info["largest_group"]) == (len(groups), sum(len(m) for m in groups), max(len(m) for m in groups))
    e, dmax = s.linearize()
    return s, System(ba, O, s, sorted_oracle_problem(O, pg), dmax, extra(s) if extra is not None else None), groups


def check_step(ck, Y, groups, scalar, x, tag=""):
    """A solve at TIGHT against P y; returns (dx_c, P y)."""
    ba, s, M = Y.ba, Y.s, Y.po.M
    lam = x * Y.dmax
    a = Y.at(lam)
    s.set_pcg(CAP, TIGHT[scalar])
    s.try_step(lam)
    st = s.pcg_stats()
    dxc = s.get(ba.GET_DX)[3 * M:]
    info = {}
    xd = SH.dense_solve(a["S"], a["rhs"], groups, info)
    yd, scale, _ = Y.yardstick(lam, scalar, groups, CAP, TIGHT[scalar])
    yerr = scale * PC.iterate_error(yd["x"], xd, a["S64"])
    print("PCG %s%s@%.0e: device iterations %d converged %d residual %.2e; yardstick iterations %d converged %d; dense residual %.1e"
          % (ck.case, tag, x, st["last_iters"], st["last_converged"], st["last_rel_residual"], yd["iters"], yd["converged"], info["rel_residual"]))
    ck("step%s@%.0e(yardstick %.1e, worst camera %d)" % (tag, x, yerr, PC.worst_camera(dxc, xd, a["S64"])), PC.iterate_error(dxc, xd, a["S64"]),
       max(10 * yerr, FLOOR[("iterate", scalar)]))
    w = dxc.reshape(-1, 9)
    ck("dx_rows_differ_in_a_group%s@%.0e" % (tag, x), sum(int(np.any(bits(w[m, 6:9]) != bits(w[m[0], 6:9]))) for m in groups), 0)
    return dxc, xd


# ---- 1. the step against the dense reference ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what,scalar", [("all", 0), ("all", 1), ("mod3", 0), ("mod3", 1), ("pair", 0)],
                         ids=["all-f64", "all-f32", "mod3-f64", "mod3-f32", "pair-f64"])
def test_step_matches_the_dense_reference(ba, O, gpu_ok, prob21, what, scalar):
    s, Y, groups = grouped(ba, O, prob21, scalar, p21_labels(what))
    ck = Checker("shared[p21,%s,%s]" % (what, SN[scalar]))
    for x in LAMS:
        check_step(ck, Y, groups, scalar, x)
    ck.done()


@pytest.fixture(scope="module")
def syn600(ba, O, gpu_ok):
    """synthetic(600, 3600, 18000) with EVERY camera's intrinsics set to camera 0's, linearised once and never stepped from: the group
    settings of the cases below need no other state, set_shared_intrinsics needs no other linearisation, and a case leaves nothing
    behind but its groups, which the next one replaces.  Released with the module."""
    pg = ba.Problem.synthetic(600, 3600, 18000, 4600)
    s = ba.Solver(pg, ba.ITERSCHUR, ba.F64)
    equalise(ba, s, [np.arange(600)])
    e, dmax = s.linearize()
    yield s, System(ba, O, s, sorted_oracle_problem(O, pg), dmax)


@pytest.mark.parametrize("what", ["one-group-of-600", "groups-of-256-and-257"])
def test_step_with_groups_of_several_chunks(ba, O, gpu_ok, syn600, what):
    """One group of 600 is three chunks; 256 is the largest group of one chunk, 257 the smallest of two; the other 87 cameras keep
    their own intrinsics.  The members are spread over the cameras (a stride), not a range."""
    s, Y = syn600
    g = np.full(600, -1, np.int32)
    if what == "one-group-of-600":
        g[:] = 9
        chunks = 3
    else:
        order = (np.arange(600) * 7) % 600  # a permutation: 7 and 600 are coprime
        g[order[:256]] = 1
        g[order[256:513]] = 0
        chunks = 1 + 2
    groups = SH.groups_of(600, g)
    s.set_shared_intrinsics(g)
    info = s.shared_intrinsics_info()
    assert info["chunks"] == chunks and info["groups"] == len(groups) and info["grouped"] == sum(len(m) for m in groups)
    ck = Checker("shared[syn600,%s]" % what)
    for x in LAMS:
        check_step(ck, Y, groups, 0, x)
    ck.done()


def test_projection_of_a_group_above_2048_cameras(ba, gpu_ok):
    """Groups of up to 8 chunks are finished by the launch that sums their chunks; a longer one takes the second launch
    (k_pcg_share_wide), which no case above reaches and no dense reference fits.  What is checked is the projection itself, on the
    reduced rhs: BA_GET_RHS without groups is rhs, with groups Pi rhs, from the same linearisation and lambda -- every other entry
    bit-equal, rows 6..8 of a group's members bit-equal to each other and within the rounding of the sum of the long double mean:
    d eps64 x mean |v|, d = 8 + 5 + ceil(chunks / 32) + 5 additions deep (lane, butterfly, partials, butterfly) + 2 for the division
    and the store.  One group of 2309 cameras (10 chunks: 9 x 256 + 5) spread over the cameras, one of 60, 31 loners.  Then a solve
    at rel_tol 1e-8 under that file's rule for converged solves, |Pi (rhs - S dx_c)| / |Pi rhs| <= 2 rel_tol, by the device's own
    statistic (checked against the quad one in test_iterates_and_residual_under_a_cap), and dx_c bit-equal inside the groups."""
    N = 2400
    pg = ba.Problem.synthetic(N, 14400, 72000, 2400)
    order = (np.arange(N) * 7) % N
    g = np.full(N, -1, np.int32)
    g[order[:2309]] = 3
    g[order[2309:2369]] = 8
    groups = SH.groups_of(N, g)
    assert sorted(len(m) for m in groups) == [60, 2309]
    s = ba.Solver(pg, ba.ITERSCHUR, ba.F64)
    equalise(ba, s, groups)
    e, dmax = s.linearize()
    lam = LAMS[1] * dmax
    s.set_pcg(1, 1e-30)
    s.try_step(lam)
    rhs = s.get(ba.GET_RHS).reshape(N, 9)
    s.set_shared_intrinsics(g)
    info = s.shared_intrinsics_info()
    assert (info["groups"], info["grouped"], info["largest_group"], info["chunks"]) == (2, 2369, 2309, 11)
    s.try_step(lam)
    prhs = s.get(ba.GET_RHS).reshape(N, 9)
    ck = Checker("shared_wide[syn2400]")
    grouped_rows = np.zeros((N, 9), bool)
    for m in groups:
        grouped_rows[m, 6:9] = True
        chunks = -(-len(m) // 256)
        depth = 8 + 5 + -(-chunks // 32) + 5 + 2
        v = rhs[m, 6:9].astype(LD)
        mean = v.sum(axis=0) / len(m)
        bound = depth * EPS[0] * np.abs(v).mean(axis=0)
        ck("members_differ[%d]" % len(m), int(np.any(bits(prhs[m, 6:9]) != bits(prhs[m[0], 6:9]))), 0)
        ck("mean_error_over_bound[%d]" % len(m), float((np.abs(prhs[m[0], 6:9].astype(LD) - mean) / bound).max()), 1.0)
    ck("other_entries_changed", int(np.count_nonzero(bits(prhs[~grouped_rows]) != bits(rhs[~grouped_rows]))), 0)
    tol = 1e-8
    s.set_pcg(CAP, tol)
    s.try_step(lam)
    st = s.pcg_stats()
    print("PCG %s: iterations %d converged %d" % (ck.case, st["last_iters"], st["last_converged"]))
    ck("converged", 0 if st["last_converged"] == 1 else 1, 0)
    ck("rel_residual", st["last_rel_residual"], 2 * tol)
    w = s.get(ba.GET_DX)[3 * pg.M:].reshape(N, 9)
    ck("dx_rows_differ_in_a_group", sum(int(np.any(bits(w[m, 6:9]) != bits(w[m[0], 6:9]))) for m in groups), 0)
    ck("dx_is_zero", 0 if np.all(w[groups[0][0], 6:9] != 0) else 1, 0)
    ck.done()


# ---- 2. iterates, 4. the residual statistic -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scalar", [0, 1], ids=["f64", "f32"])
def test_iterates_and_residual_under_a_cap(ba, O, gpu_ok, prob21, scalar):
    """x_k against the long double projected PCG: x_1 needs Pi rhs and Pi z_0, x_2 the projected S p, the later ones the projection of
    every z and beta through the rotating slots.  At k = 1, 3 and the smaller lambda the device's residual statistic against
    |Pi (rhs - S x_k)| / |Pi rhs| of the x_k it returned (test_gpu_pcg_stages.py's rule for the unshared residual)."""
    s, Y, groups = grouped(ba, O, prob21, scalar, p21_labels("mod3"))
    M = Y.po.M
    ck = Checker("shared_iterates[p21,mod3,%s]" % SN[scalar])
    for q, x in enumerate(LAMS):
        lam = x * Y.dmax
        a = Y.at(lam)
        Minv, ok = PC.invert_blocks(a["B"])
        assert ok.all()
        ref = SH.projected_pcg(a["S"], a["rhs"], SH.block_prec(Minv), groups, max(KS), keep=KS)
        yard, scale, ydt = Y.yardstick(lam, scalar, groups, max(KS), keep=KS)
        assert ref["in_range"] == 0.0
        for k in KS:
            s.set_pcg(k, 1e-30)
            s.try_step(lam)
            st = s.pcg_stats()
            xk = s.get(ba.GET_DX)[3 * M:]
            yd = scale * PC.iterate_error(yard["xs"][k], ref["xs"][k], a["S64"])
            ck("x%d@%.0e(yardstick %.1e, worst camera %d)" % (k, x, yd, PC.worst_camera(xk, ref["xs"][k], a["S64"])),
               PC.iterate_error(xk, ref["xs"][k], a["S64"]), max(10 * yd, FLOOR[("iterate", scalar)]))
            ck("x%d_capped@%.0e" % (k, x), 0 if (st["last_iters"] == k and st["last_converged"] == 0) else 1, 0)
            w = xk.reshape(-1, 9)
            ck("x%d_rows_differ_in_a_group@%.0e" % (k, x), sum(int(np.any(bits(w[m, 6:9]) != bits(w[m[0], 6:9]))) for m in groups), 0)
            if k in (1, 3) and q == 0:
                true = SH.projected_rel_residual(a["S"], xk, a["rhs"], groups)
                yk = yard["xs"][k].astype(np.float64)
                yr = scale * abs(Y.working(lam, ydt).rel_residual(yk, groups) - SH.projected_rel_residual(a["S"], yk, a["rhs"], groups))
                yr /= SH.projected_rel_residual(a["S"], yk, a["rhs"], groups)
                ck("residual%d@%.0e(true %.3e, yardstick %.1e)" % (k, x, true, yr), abs(st["last_rel_residual"] - true) / true,
                   max(10 * yr, FLOOR[("residual", scalar)]))
    # BA_GET_RHS is Pi rhs
    rhs = s.get(ba.GET_RHS)
    w = rhs.reshape(-1, 9)
    ck("rhs_rows_differ_in_a_group", sum(int(np.any(bits(w[m, 6:9]) != bits(w[m[0], 6:9]))) for m in groups), 0)
    ck.done()


# ---- 3. invariants, bit for bit -----------------------------------------------------------------------------------------------------------
def _observe(ba, s, lam_rel=1e-9, trials=2):
    out = [np.array(s.linearize())]
    lam = lam_rel * out[0][1]
    for _ in range(trials):
        out.append(np.array(s.try_step(lam)))
        out += [s.get(w).copy() for w in (ba.GET_DX, ba.GET_CAMS_TEST, ba.GET_POINTS_TEST, ba.GET_RHS)]
        st = s.pcg_stats()
        out.append(np.array([st["last_iters"], st["last_converged"], st["last_rel_residual"]]))
        lam *= 1000
    return out


def _same(x, y, what):
    assert len(x) == len(y)
    for k, (a, b) in enumerate(zip(x, y)):
        assert np.array_equal(a, b), (what, k)


def _equal_in_groups(cams, groups):
    c = np.asarray(cams).reshape(-1, 15)
    return all(np.array_equal(bits(c[m, 12:15]), np.broadcast_to(bits(c[m[0], 12:15]), (len(m), 3))) for m in groups)


@pytest.mark.parametrize("scalar", [0, 1], ids=["f64", "f32"])
def test_bits(ba, O, gpu_ok, prob21, scalar):
    pg, N, M = prob21, prob21.N, prob21.M
    g = p21_labels("mod3")
    groups = SH.groups_of(N, g)

    def solver(with_groups=True):
        s = ba.Solver(pg, ba.ITERSCHUR, scalar)
        equalise(ba, s, groups)
        if with_groups:
            s.set_shared_intrinsics(g)
        return s

    s = solver()
    start = s.get(ba.GET_CAMS)
    e, dmax = s.linearize()
    s.try_step(1e-4 * dmax)
    w = s.get(ba.GET_DX)[3 * M:].reshape(N, 9)
    assert all(np.array_equal(bits(w[m, 6:9]), np.broadcast_to(bits(w[m[0], 6:9]), (len(m), 3))) for m in groups)
    assert np.all(w[groups[0][0], 6:9] != 0) and not np.array_equal(w[0, 6:9], w[7, 6:9])  # (a step was taken; loners keep their own)
    assert _equal_in_groups(s.get(ba.GET_CAMS_TEST), groups)
    s.accept()
    after = s.get(ba.GET_CAMS)
    assert _equal_in_groups(after, groups) and not np.array_equal(after, start)
    r = s.minimize(max_trials=8)
    assert len(r["trace"]) >= 1
    assert _equal_in_groups(s.get(ba.GET_CAMS), groups)
    # a solve is the same bits run twice, on this solver and on a second one
    a = solver()
    one = _observe(ba, a)
    _same(one, _observe(ba, a), "repeated")
    _same(one, _observe(ba, solver()), "second solver")
    # ... and the same bits in try_step as in the first row of ba_minimize (the captured graph)
    gsol, h = solver(), solver()
    rows = gsol.minimize(max_trials=1)["trace"]
    e, dmax = h.linearize()
    assert rows[0, 2] == e
    h.try_step(float(DT[scalar](1e-12 * dmax)))
    for what in (ba.GET_DX, ba.GET_CAMS_TEST, ba.GET_POINTS_TEST, ba.GET_RHS):
        assert np.array_equal(gsol.get(what), h.get(what)), ("graph", what)
    sg, sh = gsol.pcg_stats(), h.pcg_stats()
    assert (sg["last_iters"], sg["last_rel_residual"]) == (sh["last_iters"], sh["last_rel_residual"])
    # groups set and cleared -- trials run, graphs captured in between -- are the solver that never had them
    never = solver(with_groups=False)
    plain = _observe(ba, never)
    assert not np.array_equal(plain[2], one[2])  # (the groups do change the step)
    trace = never.minimize(max_trials=8)["trace"][:, :5]
    for clear in (None, np.full(N, -1, np.int32), np.arange(N, dtype=np.int32)):
        b = solver()
        nbytes = b.device_bytes()
        b.minimize(max_trials=2)
        b.set_state(start, pg.arrays()["pts"])
        b.set_shared_intrinsics(clear)
        assert b.shared_intrinsics_info() == dict(groups=0, grouped=0, largest_group=0, chunks=0)
        assert b.device_bytes() < nbytes  # (ba_solver_device_bytes counts the chunk lists and partials)
        _same(plain, _observe(ba, b), "groups cleared")
        assert np.array_equal(b.minimize(max_trials=8)["trace"][:, :5], trace)


# ---- 5. interplay ---------------------------------------------------------------------------------------------------------------------------
def test_fixed_distortion_of_a_whole_group(ba, O, gpu_ok, prob21):
    """FIX_INTRINSICS & ~f on every member of one group (its shared f free, k1 and k2 fixed): dx of k1, k2 exactly 0 there, and the
    step is the dense reference's without those columns -- the masked J has zero columns there, so their rows of S are lambda alone
    with rhs 0 and the reference's k1, k2 rows are exactly 0 too."""
    g = p21_labels("mod3")
    groups = SH.groups_of(21, g)
    cm = np.zeros(21, np.uint16)
    cm[groups[1]] = ba.FIX_INTRINSICS & ~0x040
    s, Y, groups = grouped(ba, O, prob21, 0, g, cm=cm)
    ck = Checker("shared_fixed_k[p21,mod3,f64]")
    for x in LAMS:
        dxc, xd = check_step(ck, Y, groups, 0, x)
        w, wd = dxc.reshape(-1, 9), xd.reshape(-1, 9)
        ck("fixed_rows_nonzero@%.0e" % x, np.count_nonzero(w[groups[1], 7:9]) + np.count_nonzero(wd[groups[1], 7:9]), 0)
        ck("free_f_is_zero@%.0e" % x, 0 if w[groups[1][0], 6] != 0 else 1, 0)
    ck.done()


def test_a_prior_on_one_member_moves_the_group(ba, O, gpu_ok, prob21):
    """An intrinsics prior on f of camera 4 alone, three of its sigmas away, sigma from the group's own information on f: the whole
    group's f moves with it, by the dense reference's step with the prior's row in S and rhs."""
    g = p21_labels("mod3")
    cam = 4
    probe, Yp, groups = grouped(ba, O, prob21, 0, g)
    mine = [m for m in groups if cam in m][0]
    w_f = float(np.sqrt(sum((Yp.Jc[Yp.po.cam_idx == a, :, 6] ** 2).sum() for a in mine)))
    cams = probe.get(ba.GET_CAMS).reshape(-1, 15)
    x0 = cams[cam, 12:15].copy()
    x0[0] -= 3.0 / w_f
    pr = PR.Priors(i_ids=[cam], i_x0=[x0], i_w=[[w_f, 0.0, 0.0]])

    def extra(s):
        d = PR.direct(pr, 21, prob21.M, s.get(ba.GET_CAMS), s.get(ba.GET_POINTS))
        S = np.zeros((189, 189), LD)
        for a in range(21):
            S[9 * a:9 * a + 9, 9 * a:9 * a + 9] = d["V"][a]
        return dict(S=S, V=d["V"], g=d["g"][3 * prob21.M:])
    s, Y, groups = grouped(ba, O, prob21, 0, g, before=pr.apply, extra=extra)
    assert s.prior_energy()[2] == pytest.approx(9.0, rel=1e-9)
    ck = Checker("shared_prior[p21,mod3,f64]")
    for x in LAMS:
        dxc, xd = check_step(ck, Y, groups, 0, x)
        probe.set_pcg(CAP, TIGHT[0])
        probe.try_step(x * Yp.dmax)
        without = probe.get(ba.GET_DX)[3 * prob21.M:].reshape(-1, 9)
        moved = dxc.reshape(-1, 9)[mine, 6] - without[mine, 6]
        print("PCG %s@%.0e: dx_f of the group with the prior %.6e, without %.6e, 3 sigma = %.3e"
              % (ck.case, x, dxc.reshape(-1, 9)[mine[0], 6], without[mine[0], 6], 3 / w_f))
        ck("members_not_moved_towards_the_prior@%.0e" % x, np.count_nonzero(~(moved < 0)), 0)
    ck.done()


def test_forest_preconditioner_with_a_chain_inside_a_group(ba, O, gpu_ok, prob21):
    """BA_PRECOND_CONSTRAINT_FOREST with the odometry constraints (4, 5), (5, 6) inside the group of cameras 4 .. 8: the projection sits
    behind k_pcg_forest_apply, and the solve converges to the same P y.  The yardstick is the block-Jacobi projected PCG in working
    precision: at convergence the preconditioner decides the path, not what the arithmetic can reach."""
    pg, N = prob21, prob21.N
    g = p21_labels("runs")
    plain = ba.Solver(pg, ba.ITERSCHUR, ba.F64)
    groups = SH.groups_of(N, g)
    state = equalise(ba, plain, groups)
    plain.linearize()
    po = sorted_oracle_problem(O, pg)
    V = np.zeros((N, 9))
    np.add.at(V, po.cam_idx, (plain.get(ba.GET_JC).reshape(-1, 2, 9) ** 2).sum(axis=1))
    full = RC.standard_constraints(N, po.cam_idx, po.pt_idx, state, V)[0]
    idx = [q for q, (a, b) in enumerate(full.pairs) if (int(a), int(b)) in ((4, 5), (5, 6))]
    assert len(idx) == 2
    cs = RC.Constraints(full.pairs[idx], full.R0[idx], full.t0[idx], full.Lr[idx], full.Lt[idx])

    def before(s):
        cs.apply(s)
        s.set_preconditioner(ba.PRECOND_CONSTRAINT_FOREST, 0)

    def extra(s):
        d = RC.direct(cs, N, s.get(ba.GET_CAMS))
        return dict(S=d["S"], V=d["V"], g=d["g"])
    s, Y, groups = grouped(ba, O, pg, 0, g, before=before, extra=extra)
    i = s.preconditioner_info()
    assert (i["trees"], i["kept"], i["largest_tree"]) == (1, 2, 3)
    ck = Checker("shared_forest[p21,runs,f64]")
    for x in LAMS:
        check_step(ck, Y, groups, 0, x)
        ck("fallback_trees@%.0e" % x, s.preconditioner_info()["fallback_trees"], 0)
    ck.done()


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------------------------
def _refused(ba, fn, *args):
    with pytest.raises(ba.BAError) as e:
        fn(*args)
    assert e.value.code == ba.ERR_ARG


def test_refusals_leave_the_solver_unchanged(ba, O, gpu_ok, prob21):
    pg, N = prob21, prob21.N
    g = p21_labels("mod3")
    groups = SH.groups_of(N, g)
    c = ba.Solver(pg, ba.CHOLESKY, ba.F64)
    equalise(ba, c, groups)
    _refused(ba, c.set_shared_intrinsics, g)
    _refused(ba, c.shared_intrinsics_info)
    none = dict(groups=0, grouped=0, largest_group=0, chunks=0)
    # members with intrinsics of their own (problem-21 as loaded); one member one ulp off
    s = ba.Solver(pg, ba.ITERSCHUR, ba.F64)
    before = _observe(ba, s, trials=1)
    _refused(ba, s.set_shared_intrinsics, g)
    cams = equalise(ba, s, groups).reshape(-1, 15)
    cams[groups[2][-1], 13] = np.nextafter(cams[groups[2][-1], 13], np.inf)
    s.set_state(cams.ravel(), None)
    _refused(ba, s.set_shared_intrinsics, g)
    assert s.shared_intrinsics_info() == none
    s.set_state(ba.Solver(pg, ba.ITERSCHUR, ba.F64).get(ba.GET_CAMS), None)
    _same(before, _observe(ba, s, trials=1), "behind the refused groups")
    # members with different intrinsics bits of the mask in force
    cm = np.zeros(N, np.uint16)
    cm[groups[0][1]] = 0x080  # k1 of one member
    equalise(ba, s, groups)
    s.set_constant(cm, None)
    masked = _observe(ba, s, trials=1)
    _refused(ba, s.set_shared_intrinsics, g)
    assert s.shared_intrinsics_info() == none
    _same(masked, _observe(ba, s, trials=1), "behind the refused groups under a mask")
    cm[groups[0]] = 0x080  # the whole group: accepted
    s.set_constant(cm, None)
    s.set_shared_intrinsics(g)
    assert s.shared_intrinsics_info()["groups"] == 3
    # with groups in force
    s = ba.Solver(pg, ba.ITERSCHUR, ba.F64)
    good = equalise(ba, s, groups)
    s.set_shared_intrinsics(g)
    info, nbytes = s.shared_intrinsics_info(), s.device_bytes()
    before = _observe(ba, s, trials=1)
    bad = good.reshape(-1, 15).copy()
    bad[groups[1][2], 12] *= 1.001
    _refused(ba, s.set_state, bad.ravel(), None)
    assert np.array_equal(s.get(ba.GET_CAMS), good)
    cm = np.zeros(N, np.uint16)
    cm[groups[1][0]] = 0x040
    _refused(ba, s.set_constant, cm, None)
    _refused(ba, s.covariance_pcg, 1e-3, None, [0])
    assert s.shared_intrinsics_info() == info and s.device_bytes() == nbytes
    _same(before, _observe(ba, s, trials=1), "behind the refusals")
    # a step that is pending when the group set changes is dropped: its xTest belongs to the other group set
    u = ba.Solver(pg, ba.ITERSCHUR, ba.F64)
    equalise(ba, u, groups)
    e, dmax = u.linearize()
    u.try_step(1e-4 * dmax)
    test = u.get(ba.GET_CAMS_TEST)
    assert not _equal_in_groups(test, groups)  # (the ungrouped step moves every member's intrinsics on its own)
    u.set_shared_intrinsics(g)
    _refused(ba, u.accept)
    assert np.array_equal(u.get(ba.GET_CAMS), good) and u.shared_intrinsics_info()["groups"] == 3
    u.try_step(1e-4 * dmax)  # (no new linearisation needed)
    u.accept()
    assert _equal_in_groups(u.get(ba.GET_CAMS), groups) and not np.array_equal(u.get(ba.GET_CAMS), good)
    u.linearize()
    u.try_step(1e-4 * dmax)
    u.set_shared_intrinsics(None)  # ... and in the other direction
    _refused(ba, u.accept)
    pose = np.zeros(N, np.uint16)
    pose[groups[1][0]] = ba.FIX_POSE  # (bits 0..5 may differ inside a group)
    s.set_constant(pose, None)
    s.set_state(good, None)  # (equal members: accepted)


# ---- 7. end to end ----------------------------------------------------------------------------------------------------------------------------
def test_one_physical_camera_end_to_end(ba, gpu_ok):
    """The truth lies in the shared model's feasible set, so its minimum is no higher than that of the model with the intrinsics held at
    the truth; 1.02 is what this project grants ITERSCHUR's inexact steps against CHOLESKY."""
    r = SH.end_to_end(ba)
    sh, fx = r["shared"], r["fixed"]
    print("SHARED end to end: noise energy %.6f; fixed intrinsics (CHOLESKY) energy %.6f in %d trials (%s); shared (ITERSCHUR) energy %.6f in %d "
          "trials (%s), %d PCG iterations; f true %.6f start %.6f end %.6f (error %.3e relative)"
          % (r["noise_energy"], fx["energy"], fx["trials"], ba.STATUS[fx["status"]], sh["energy"], sh["trials"], ba.STATUS[sh["status"]],
             r["stats"]["total_iters"], r["f_true"], r["f_start"], r["f_end"], abs(r["f_end"] / r["f_true"] - 1)))
    assert sh["trials"] < 500 and fx["trials"] < 500  # (both ran to their own stop)
    assert r["equal"]
    assert sh["energy"] <= 1.02 * fx["energy"], (sh["energy"], fx["energy"])
    t = sh["trace"]
    e_after = np.append(t[1:, 2], sh["energy"])  # (a row's f is the energy before its step)
    acc = t[:, 1] == 1
    assert acc.any() and np.all(e_after[acc] < t[acc, 2]), t[:, :3]
