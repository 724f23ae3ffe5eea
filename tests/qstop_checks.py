"""The model-decrease stopping rule of BA_ITERSCHUR's PCG (ba_solver_set_pcg_model_tol) -- TEST INFRASTRUCTURE ONLY
(tests/test_qstop_checks.py, tests/test_gpu_pcg_model_stop.py).

pcg_model is pcg_checks.pcg's recurrence (with `groups`: shared_checks.projected_pcg's, which is the same one when there are none) with

    s_k = x_k'(rhs + r_k) = -2 Q(x_k),  Q(x) = x'Sx / 2 - x'rhs,  s_0 = 0            (r_k the recurrence's residual)
    zeta_k = k (s_k - s_{k-1}) / s_k                                                  (k >= 1)

formed from the iterate, and the library's order of tests at the head of iteration k:

    |r_k| <= rel_tol |rhs|                      -> rule 1, iters = k
    k == max_iter                               -> rule 0 (the cap)
    k >= 1, s_k > 0 and finite, zeta_k < eta    -> rule 2

The product and the preconditioner are callables (dense, matrix_free, shared_checks.block_prec, forest_checks.forest), so one function is
the reference (long double, products by S) and the working-precision yardstick (everything in float64 / float32, the product in the
matrix-free form V p - (V - S) p; s_k summed in float64 from the rounded x, rhs and r as k_pcg_update_q sums it).

choose_eta picks the eta of a comparison of stopping indices from the reference's own zeta sequence: zeta is not monotone (problem-21
at 1e-12 max diag J'J: zeta_3..5 = 0.101, 0.110, 0.104), and an eta next to a zeta_j decides by rounding.  eta = sqrt(zeta_k* min_{j<k*}
zeta_j) sits a factor `clearance` = sqrt(min_{j<k*} zeta_j / zeta_k*) away from both.

The keyword arguments zeta_k_factor, prev_lag and s_rows of pcg_model plant the defects tests/test_qstop_checks.py uses to show that a
stopping index has teeth; nothing else passes them.
"""
import numpy as np

import pcg_checks as PC
import shared_checks as SH

LD = PC.LD
CLEARANCE = 1.2


def dense(S, dtype=LD):
    Sd = np.asarray(S, dtype)
    return lambda p: Sd @ p


def matrix_free(S, V, dtype):
    """p -> V p - (V - S) p with both terms rounded to dtype (pcg_checks.pcg's V=)."""
    N = len(V)
    Vd = np.asarray(V, dtype)
    E = PC._minus_blocks(np.asarray(S, LD), np.asarray(V, LD)).astype(dtype)
    return lambda p: np.einsum("nij,nj->ni", Vd, p.reshape(N, 9)).reshape(-1) - E @ p


def pcg_model(rhs, matvec, prec, max_iter, rel_tol=0.0, eta=0.0, dtype=LD, groups=(), keep=None, zeta_k_factor=True, prev_lag=1, s_rows=None):
    """The recurrence of the module docstring in `dtype`.  Returns dict(x, iters, rule, xs: {k: x_k for k in keep}, rr: [|r_k|^2 / |rhs|^2],
    s: [s_0 .. s_iters], zeta: [0, zeta_1 .. zeta_iters], xr: [|x_k'r_k| / (|x_k| |r_k|), k = 1 ..], xr_model: [|x_k'r_k| / s_k, k = 1 ..]: the share of the model decrease that
    dx'(lambda dx + g) = x_k'(rhs - r_k) misses).
    Planted defects: zeta_k_factor=False (zeta without its factor k), prev_lag=2 (s_{k-1} taken from the slot of s_{k-2}), s_rows (a bool
    mask: only those rows enter s, a block of partials left out)."""
    acc = LD if dtype is LD else np.float64
    groups = list(groups)
    b = SH.project(np.asarray(rhs, dtype), groups)
    keep = set(keep or ())
    tol2 = dtype(rel_tol) * dtype(rel_tol)
    pz = lambda r: SH.project(np.asarray(prec(r), dtype), groups)

    def model(x, r):
        t = x.astype(acc) * (b.astype(acc) + r.astype(acc))
        return t.sum() if s_rows is None else t[s_rows].sum()

    x, r, p = np.zeros_like(b), b.copy(), np.zeros_like(b)
    z = pz(r)
    bb = (b * b).sum()
    rz, rr, s, zeta, xr, xr_model = [(r * z).sum()], [(r * r).sum()], [acc(0)], [0.0], [], []
    xs, k, rule = {}, 0, 0
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        while True:
            if rr[k] <= tol2 * bb:
                rule = 1
                break
            if k == max_iter:
                break
            if eta > 0 and k >= 1 and s[k] > 0 and np.isfinite(float(s[k])) and zeta[k] < eta:
                rule = 2
                break
            p = z + (dtype(0) if k == 0 else rz[k] / rz[k - 1]) * p
            y = SH.project(np.asarray(matvec(p), dtype), groups)
            alpha = rz[k] / (p * y).sum()
            x = x + alpha * p
            r = r - alpha * y
            z = pz(r)
            rz.append((r * z).sum())
            rr.append((r * r).sum())
            k += 1
            s.append(model(x, r))
            prev = s[k - prev_lag] if k - prev_lag >= 0 else acc(0)
            zeta.append(float((acc(k) if zeta_k_factor else acc(1)) * (s[k] - prev) / s[k]))
            xl, rl = x.astype(LD), r.astype(LD)
            den = np.sqrt((xl * xl).sum() * (rl * rl).sum())
            xr.append(float(abs((xl * rl).sum()) / den) if den > 0 else 0.0)
            xr_model.append(float(abs((xl * rl).sum()) / abs(LD(s[k]))) if s[k] != 0 else 0.0)
            if k in keep:
                xs[k] = x.copy()
    return dict(x=x, iters=k, rule=rule, xs=xs, rr=np.array([float(v / bb) for v in rr]), s=np.array([float(v) for v in s]),
                s_acc=s, zeta=np.array(zeta), xr=np.array(xr), xr_model=np.array(xr_model))


def choose_eta(zeta, k_target, clearance=CLEARANCE):
    """(eta, k*, clearance) for the first k* >= k_target at which eta = sqrt(zeta_k* min_{j<k*} zeta_j) stops the rule at k* and nowhere
    before it with min(eta / zeta_k*, min_{j<k*} zeta_j / eta) >= clearance; None when the sequence offers no such k*.  zeta: [_, zeta_1,
    zeta_2, ...] (entry 0 is not used: the rule starts at k = 1)."""
    zeta = np.asarray(zeta, np.float64)
    for k in range(max(k_target, 1), len(zeta)):
        before = zeta[1:k].min() if k > 1 else 1.0  # (eta < 1: at k* = 1 nothing comes before it)
        if not (0 < zeta[k] < before) or not np.isfinite(zeta[k]):
            continue
        eta = float(np.sqrt(zeta[k] * before))
        clear = float(min(eta / zeta[k], before / eta))
        if clear >= clearance and eta < 1:
            return eta, k, clear
    return None


def stop_index(zeta, eta, s=None):
    """The k >= 1 at which the rule fires on a sequence of zeta (and s > 0 where given); None when it never does."""
    for k in range(1, len(zeta)):
        if (s is None or s[k] > 0) and zeta[k] < eta:
            return k
    return None


# The residual rule whose count the third target halves: the default rel_tol in fp64; in fp32 1e-4, the ratio of
# test_gpu_pcg_stages.TOL -- an fp32 iterate behind it moves by the rounding errors of the product, and zeta_k, a difference of two s, is
# then noise in that arithmetic whatever the reference's sequence offers (measured on the CPU yardstick: synthetic(257, ...) at k* = 43
# stops at 44 in fp32 with zeta off by 118 %).
RES_TOL = {0: 1e-6, 1: 1e-4}


def targets(k_residual):
    """The k_target of the GPU cases: 2 (the earliest stop: zeta_1 = 1), 4 (all three slots have been written and slot 0 overwritten), and
    about half the residual rule's count; none behind that count (there zeta is the rounding error of s_k - s_{k-1})."""
    return [k for k in sorted({2, 4, max(2, k_residual // 2)}) if k <= k_residual]


def chosen(case, scalar):
    """[(eta, k*, clearance)] of a Case's targets for a scalar type, one per k*.  Asserts that the reference's sequence offers each."""
    ref = case.reference()
    out = {}
    for kt in targets(case.k_residual(RES_TOL[scalar])):
        got = choose_eta(ref["zeta"], kt)
        assert got is not None and got[2] >= CLEARANCE and stop_index(ref["zeta"], got[0], ref["s"]) == got[1], (kt, got, ref["zeta"][:kt + 8])
        out[got[1]] = got
    return [out[k] for k in sorted(out)]


# ---- the cases of tests/test_gpu_pcg_model_stop.py, formed from any linearisation (the GPU's own, or the oracle's on the CPU) ---------------
# name: (problem, lambda / max diag J'J (Marquardt: lambda itself), what is special, scalar types)
CASES = {
    "p21@1e-12": ("p21", 1e-12, None, (0,)),  # (fp32's B_a is not trustworthy there: DESIGN.md section 9)
    "p21@1e-6": ("p21", 1e-6, None, (0, 1)),
    "p21@1e-2": ("p21", 1e-2, None, (0, 1)),
    "syn2": ("syn2", 1e-6, None, (0, 1)),
    "edges": ("edges", 1e-6, None, (0, 1)),
    "syn257": ("syn257", 1e-6, None, (0, 1)),
    "syn600": ("syn600", 1e-6, None, (0, 1)),
    "p21-gauge": ("p21", 1e-6, "gauge", (0, 1)),
    "p21-group": ("p21", 1e-6, "group", (0, 1)),
    "p21-constraint-forest": ("p21", 1e-6, "cforest", (0, 1)),
    "p21-visibility-forest": ("p21", 1e-6, "vforest", (0, 1)),
    # (lambda is dimensionless under Marquardt.  At 1e-6 problem-21 with no gauge fixed needs thousands of iterations and its fp32 trial has
    # all but broken down: test_gpu_damping.py's findings)
    "p21-marquardt": ("p21", 1e-2, "marquardt", (0, 1)),
}
K_MAX = 120  # iterations of a reference run at most (problem-21 at 1e-12 max diag J'J meets 1e-6 at k = 81)
REF_TOL = 1e-7


def mask_columns(Jc, cam_idx, cm):
    """Jc with the columns of the parameters a camera mask holds constant zeroed (what BA_GET_JC returns under ba_solver_set_constant)."""
    free = ((np.asarray(cm, np.int64)[:, None] >> np.arange(9)[None, :]) & 1) == 0
    return np.asarray(Jc).reshape(-1, 2, 9) * free[np.asarray(cam_idx)][:, None, :]


def chain(N, cam_idx, pt_idx, cams, Jc):
    """The odometry chain (a, a + 1) of relpose_checks.standard_constraints, sized from this linearisation."""
    import relpose_checks as RC
    V = np.zeros((N, 9))
    np.add.at(V, np.asarray(cam_idx), (np.asarray(Jc, np.float64).reshape(-1, 2, 9) ** 2).sum(axis=1))
    cs = RC.standard_constraints(N, cam_idx, pt_idx, cams, V)[0]
    idx = np.arange(N - 1)
    return RC.Constraints(cs.pairs[idx], cs.R0[idx], cs.t0[idx], cs.Lr[idx], cs.Lt[idx])


class Case:
    """The reference system of one case -- S and rhs in long double, the preconditioner, the groups -- and the working-precision one.
    lin: dict(po: the point-sorted oracle problem, Jc, Jp, f, lam; g: the gradient, points first (the working-precision rhs needs it);
    cams [N, 15] and cs (cforest), cov (vforest), groups (group))."""

    def __init__(self, O, what, lin):
        import damping_checks as DC
        import forest_checks as FC
        import relpose_checks as RC
        import visibility_checks as VC
        self.what, self.lin = what, lin
        po, Jc, Jp, f, lam = (lin[k] for k in ("po", "Jc", "Jp", "f", "lam"))
        N = self.N = po.N
        self.groups = list(lin.get("groups") or [])
        self.gc = None if lin.get("g") is None else np.asarray(lin["g"])[3 * po.M:]
        if what == "marquardt":
            ref = DC.trial(po, Jc, Jp, f, lam, g=lin.get("g"), want_step=False)
            self.S, self.rhs, self.B, self.V = ref["S"], ref["rhs"].astype(LD), ref["B"], ref["Vd"]
        else:
            R = O.referee_reduced_from_jacobian(O.CHOLESKY, po, Jc, Jp, f, lam)
            S64 = R["S"].reshape(9 * N, 9 * N)
            self.S, self.rhs = S64.astype(LD), R["rhs"].astype(LD)
            self.B, self.V = PC.documented_blocks(po, Jc, Jp, lam, S64), PC.camera_blocks(po, Jc, lam)
        self.H, self.pairs, self.adds = np.zeros((0, 6, 6), LD), np.zeros((0, 2), np.int32), {}
        if what == "cforest":
            cs = lin["cs"]
            d = RC.direct(cs, N, lin["cams"], None)
            cross = d["S"].copy()
            for a in range(N):
                cross[9 * a:9 * a + 9, 9 * a:9 * a + 9] = 0
            self.adds = dict(add_V=d["V"], add_cross=cross)  # (the working-precision trial's; its g is the device's own, constraints included)
            self.S, self.rhs = self.S + d["S"], self.rhs + d["g"]
            self.B, self.V = self.B + d["V"], self.V + d["V"]
            self.H, self.pairs = np.stack([d["cross"][(int(a), int(b))] for a, b in cs.pairs]), cs.pairs
            self.pl = FC.plan(N, cs.pairs, N)
            Dinv, G, ok = FC.factor(self.B, self.H, self.pairs, self.pl)
            assert ok.all()
            self.prec = FC.forest(self.pl, Dinv, G)
        elif what == "vforest":
            self.pl, self.L = VC.plan(N, self.pairs, lin["cov"], N)
            self.X = VC.cross_blocks(self.S, self.L, self.pl["kept"])
            Dinv, G, ok = VC.factor(self.B, self.X, self.L, self.pl)
            assert ok.all()
            self.prec = FC.forest(self.pl, Dinv, G)
        else:
            Minv, ok = PC.invert_blocks(self.B)
            assert ok.all()
            self.prec = SH.block_prec(Minv)
        self.S64 = self.S.astype(np.float64)
        self._ref, self._work = None, {}

    def reference(self):
        """The long double run with no model rule on, to a residual of REF_TOL (past every stop the tests ask for) or K_MAX iterations: its
        s and zeta sequences, every iterate kept."""
        if self._ref is None:
            self._ref = pcg_model(self.rhs, dense(self.S), self.prec, K_MAX, REF_TOL, groups=self.groups, keep=range(1, K_MAX + 1))
        return self._ref

    def k_residual(self, rel_tol):
        """The k at which the residual rule at rel_tol ends the reference run; K_MAX where it does not within K_MAX iterations (problem-21
        under Marquardt's damping with no gauge fixed: thousands)."""
        rr = self.reference()["rr"]
        hit = np.nonzero(rr <= rel_tol * rel_tol)[0]
        return int(hit[0]) if len(hit) else len(rr) - 1

    def working_system(self, dt):
        """The working-precision trial of the same J (damping_checks.trial in dt: the normal blocks, the point elimination, S, rhs and B_a
        formed in the solver's scalar type), handed on in long double; None when it is not finite.  The quad assembly has none of the
        elimination's rounding in it, and s_k ~ rhs'S^-1 rhs inherits the relative error of rhs twice over: at 1e-12 max diag J'J, where
        a point block is as badly conditioned as 1 / lambda allows, that is what a working-precision s_k deviates by first
        (test_gpu_damping.Dev.pcg_yardstick found the same for the iterates under Marquardt's damping)."""
        import damping_checks as DC
        if dt not in self._work:
            lin = self.lin
            w = DC.trial(lin["po"], lin["Jc"], lin["Jp"], lin["f"], lin["lam"], kind=DC.MARQUARDT if self.what == "marquardt" else DC.IDENTITY,
                         dtype=dt, g=lin["g"], round_to=dt, want_step=False, **self.adds)
            ok = all(np.all(np.isfinite(np.asarray(w[k], np.float64))) for k in ("S", "rhs", "B"))
            self._work[dt] = tuple(np.asarray(w[k]).astype(LD) for k in ("S", "rhs", "B", "Vd")) if ok else None
        return self._work[dt]

    def working(self, dt, max_iter, rel_tol=0.0, eta=0.0, keep=None):
        """The working-precision yardstick's run in dt on working_system (pcg_checks.yardstick's forms: B = V - (its eliminated part), rhs
        = g - (its eliminated part), the product V p - (V - S) p), or None when a block is not positive definite or an iterate not finite
        in dt."""
        import forest_checks as FC
        import visibility_checks as VC
        w = self.working_system(dt)
        if w is None:
            return None
        S, rhs, B, V = w
        W = SH.Working(S, rhs, B, V, self.gc, dt)
        prec = W.prec
        if self.what in ("cforest", "vforest"):
            Bw = np.asarray(V).astype(dt) - (np.asarray(V, LD) - np.asarray(B, LD)).astype(dt)
            if self.what == "cforest":
                Dw, Gw, bad = FC.working(Bw, self.H, self.pairs, self.pl, dt)
            else:
                Dw, Gw, bad = VC.working(Bw, self.X, self.L, self.pl, dt)
            if bad:
                return None
            prec = FC.forest(self.pl, Dw, Gw)
        elif not W.ok:
            return None
        out = pcg_model(W.rhs, W.matvec, prec, max_iter, rel_tol, eta, dt, self.groups, keep)
        if not all(np.all(np.isfinite(v.astype(np.float64))) for v in list(out["xs"].values()) + [out["x"]]):
            return None
        return out
