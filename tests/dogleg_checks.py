"""Powell's dogleg restated -- TEST INFRASTRUCTURE ONLY (tests/test_dogleg_checks.py, tests/test_gpu_dogleg.py).

ba_solver_dogleg_prepare / ba_solver_try_dogleg / ba_minimize_dogleg (include/ba_mi355x.h).  With g = -J'e,
H = J'J and the model E(x (+) dx) ~ E - 2 g'dx + dx'H dx:

    dx_gn   (H + mu I) dx_gn = g           (damping_checks.trial at lambda = mu, identity damping: the existing reference trial)
    dx_sd   alpha g, alpha = |g|^2 / q, q = |J g|^2
    dx      a g + c dx_gn for a radius: Gauss-Newton (0) if |dx_gn| <= radius, else the scaled gradient (1) if alpha |g| >= radius,
            else the point of the segment dx_sd .. dx_gn on the sphere (2)
    pred    2 g'dx - dx'H dx = 2 (a g2 + c d) - (a^2 q + 2 a c (g2 - mu d) + c^2 (d - mu gn2)),  d = g'dx_gn,  H dx_gn = g - mu dx_gn

`Reference` does this in np.longdouble on a given (J, e, g); `working_scalars` forms the four sums the way a CPU implementation in the
solver's scalar type with fp64 accumulation does (the yardstick of the GPU's sums).  `drive` is the driver's control rule on any
implementation of the four calls; `OracleCalls` implements them on the fp64 oracle.
"""
import math

import numpy as np

import damping_checks as DC

LD = np.longdouble


def coefficients(g2, q, gn2, d, mu, radius, dtype=LD):
    """(a, c, branch, pred) by the rule of include/ba_mi355x.h in `dtype`; ValueError for what ba_dogleg_coefficients refuses."""
    t = np.dtype(dtype).type
    vals = [t(v) for v in (g2, q, gn2, d)]
    if not all(np.isfinite(v) and v >= 0 for v in vals):
        raise ValueError("a scalar is negative or not finite")
    mu, radius = t(mu), t(radius)
    if not (mu > 0 and np.isfinite(mu)) or not radius > 0:
        raise ValueError("mu or radius")
    g2, q, gn2, d = vals
    if g2 == 0:
        return t(0), t(0), 0, t(0)
    if not q > 0:
        raise ValueError("q <= 0 with g2 > 0")
    alpha, ng = g2 / q, np.sqrt(g2)
    if np.sqrt(gn2) <= radius:
        a, c, br = t(0), t(1), 0
    elif alpha * ng >= radius:
        a, c, br = radius / ng, t(0), 1
    else:
        A, B, C = gn2 - 2 * alpha * d + alpha * alpha * g2, alpha * d - alpha * alpha * g2, alpha * alpha * g2 - radius * radius
        disc = max(B * B - A * C, t(0))
        beta = (-B + np.sqrt(disc)) / A if B <= 0 else -C / (B + np.sqrt(disc))
        beta = min(max(beta, t(0)), t(1))
        a, c, br = alpha * (1 - beta), beta, 2
    with np.errstate(over="ignore", invalid="ignore"):  # (scalars near the top of the range: pred is then not finite, as the library's)
        pred = 2 * (a * g2 + c * d) - (a * a * q + 2 * a * c * (g2 - mu * d) + c * c * (d - mu * gn2))
    return a, c, br, pred


def j_times(p, Jc, Jp, v, dtype=LD):
    """J v [K, 2] for v in the order of BA_GET_DX (points first), products and sums in dtype."""
    Jc = np.asarray(Jc).reshape(p.K, 2, 9).astype(dtype)
    Jp = np.asarray(Jp).reshape(p.K, 2, 3).astype(dtype)
    v = np.asarray(v).astype(dtype)
    vp, vc = v[:3 * p.M].reshape(p.M, 3), v[3 * p.M:].reshape(p.N, 9)
    return np.einsum("krc,kc->kr", Jc, vc[p.cam_idx]) + np.einsum("krc,kc->kr", Jp, vp[p.pt_idx])


def working_scalars(p, Jc, Jp, g, dx_gn, scalar_dtype):
    """dict(g2, q, gn2, d): the arrays as the solver's scalar type holds them, every product and sum in float64 (np.sum's pairwise order) --
    what a CPU implementation of the same sums achieves; the yardstick for the device's."""
    r = np.dtype(scalar_dtype).type
    g64, x64 = np.asarray(g, np.float64).astype(r).astype(np.float64), np.asarray(dx_gn, np.float64).astype(r).astype(np.float64)
    y = j_times(p, np.asarray(Jc, np.float64).astype(r), np.asarray(Jp, np.float64).astype(r), g64, np.float64)
    return dict(g2=float((g64 * g64).sum()), q=float((y * y).sum()), gn2=float((x64 * x64).sum()), d=float((g64 * x64).sum()))


class Reference:
    """The dogleg of one linearisation in long double.  g: the gradient to use (a device's own BA_GET_GRAD; default -J'e); dx_gn: the
    Gauss-Newton step to use instead of the reference trial's (a device's kept step, for the checks of a step formed from it)."""

    def __init__(self, p, Jc, Jp, f, g, mu, dx_gn=None):
        self.p, self.Jc, self.Jp, self.mu = p, Jc, Jp, LD(mu)
        if g is None:
            g = DC.normal_blocks(p, Jc, Jp, f)[2]
        self.g = np.asarray(g).astype(LD)
        if dx_gn is None:
            dx_gn = DC.trial(p, Jc, Jp, f, mu, kind=DC.IDENTITY, g=np.asarray(g, np.float64))["dx"]
        self.dx_gn = np.asarray(dx_gn).astype(LD)
        y = j_times(p, Jc, Jp, self.g)
        self.q = (y * y).sum()
        self.g2, self.gn2, self.d = (self.g * self.g).sum(), (self.dx_gn * self.dx_gn).sum(), (self.g * self.dx_gn).sum()
        self.alpha = self.g2 / self.q if self.g2 > 0 else LD(0)
        self.sd_norm, self.gn_norm = self.alpha * np.sqrt(self.g2), np.sqrt(self.gn2)

    def scalars(self):
        return dict(g2=self.g2, q=self.q, gn2=self.gn2, d=self.d)

    def pred_direct(self, dx):
        """2 g'dx - |J dx|^2 in long double."""
        dx = np.asarray(dx).astype(LD)
        y = j_times(self.p, self.Jc, self.Jp, dx)
        return 2 * (self.g * dx).sum() - (y * y).sum()

    def step(self, radius):
        """(a, c, branch, dx, pred from the scalars)."""
        a, c, br, pred = coefficients(self.g2, self.q, self.gn2, self.d, self.mu, radius)
        return a, c, br, a * self.g + c * self.dx_gn, pred


# ---- the driver's control rule (ba_minimize_dogleg) -------------------------------------------------------------------------------------
SUCCESS, EXCEEDED, TOO_MANY_FUN_EVALS, MAX_ITERS, RUNNING = 0, 1, 2, 3, -1
DEFAULTS = dict(radius_init=0.0, radius_min=1e-32, radius_max=1e16, mu_rel=1e-12, mu_rel_max=1.0, tol_fun=1e-8, max_iter=1000000,
                max_fun_ev=1000000)


def drive(calls, max_trials=0, **over):
    """calls: linearize() -> (E, max diag J'J); prepare(mu) -> dict(g2, q, gn2, g_dot_gn, mu, energy_gn); try_dogleg(radius) ->
    (e_test, pred, dx_norm, branch); accept(); coefficients(g2, q, gn2, d, mu, radius) -> (a, c, branch, pred).  Every operation on
    doubles in the order of the library's driver, so that a loop over the library's own calls reproduces its rows bit for bit.
    Returns dict(status, iterations, trials, fun_evals, energy, radius, rows [n, 6]: iter, accepted, f, rho, radius, e_test)."""
    P = dict(DEFAULTS, **over)
    status, it, trials, m, radius, rows, done = RUNNING, 0, 0, 1.0, float(P["radius_init"]), [], False
    E, dmax = calls.linearize()
    fun_evals = 1
    while status == RUNNING and not done:
        it += 1
        if it > P["max_iter"]:
            status = MAX_ITERS
            break
        ready = False
        while not ready:
            if P["mu_rel"] * m > P["mu_rel_max"]:
                status = EXCEEDED
                break
            if fun_evals >= P["max_fun_ev"]:
                status = TOO_MANY_FUN_EVALS
                break
            info = calls.prepare(P["mu_rel"] * m * dmax)
            fun_evals += 1
            if info["g2"] == 0:
                status = SUCCESS
                break
            try:
                pred_gn = float(calls.coefficients(info["g2"], info["q"], info["gn2"], info["g_dot_gn"], info["mu"], math.inf)[3])
            except (ValueError, RuntimeError):  # (scalars the rule refuses -- a step that is not finite -- count as a pred that is not finite)
                pred_gn = math.nan
            if pred_gn > 0 and math.isfinite(pred_gn):
                ready = True
            else:
                m *= 10
        if not ready:
            break
        m = max(1.0, m / 5)
        gn_norm = math.sqrt(info["gn2"])
        if it == 1 and radius == 0:
            radius = gn_norm
        first = True
        while status == RUNNING:
            if radius < P["radius_min"]:
                status = EXCEEDED
                break
            e_test, pred, dxn = info["energy_gn"], pred_gn, gn_norm
            if not (first and gn_norm <= radius):
                if fun_evals >= P["max_fun_ev"]:
                    status = TOO_MANY_FUN_EVALS
                    break
                e_test, pred, dxn, _ = calls.try_dogleg(radius)
                fun_evals += 1
            first = False
            trials += 1
            done = max_trials > 0 and trials >= max_trials  # (this row is the last: what it decides is still carried out)
            accepted = pred > 0 and e_test < E
            with np.errstate(all="ignore"):
                rho = float(np.float64(E - e_test) / np.float64(pred))  # (IEEE division, as the library's: no exception at pred = 0)
            rows.append((it, int(accepted), E, rho, radius, e_test))
            if not accepted:
                radius /= 2
                if done:
                    break
                continue
            flat = (E - e_test) / E < P["tol_fun"]
            if rho > 0.75:
                radius = min(P["radius_max"], max(radius, 3 * dxn))
            elif rho < 0.25:
                radius /= 2
            calls.accept()
            if flat:
                E, status = e_test, SUCCESS
                break
            E, dmax = calls.linearize()
            break
    return dict(status=status, iterations=it, trials=trials, fun_evals=fun_evals, energy=E, radius=radius,
                rows=np.array(rows, np.float64).reshape(-1, 6))


class OracleCalls:
    """The four calls on the fp64 oracle (oracle_lib): residuals, Jacobian, the CHOLESKY step at lambda = mu and the retraction."""

    def __init__(self, O, po):
        self.O, self.po = O, po
        self.cam, self.pts = O.init_cams(po), po.pts.copy()
        self.test = None

    def linearize(self):
        O, po = self.O, self.po
        self.f, e = O.residuals(po, self.cam, self.pts)
        self.Jc, self.Jp = O.jacobian(po, self.cam, self.pts)
        U, V, _ = DC.normal_blocks(po, self.Jc, self.Jp, self.f, np.float64)
        dp, dc = DC.diagonals(U, V)
        return e, float(max(dp.max(), dc.max()))

    def _trial(self, dx):
        self.test = self.O.retract(self.po, self.cam, self.pts, dx)
        return self.O.residuals(self.po, self.test[0], self.test[1])[1]

    def prepare(self, mu):
        st = self.O.step(2, self.po, self.Jc, self.Jp, self.f, mu, want_S=False)  # (2: CHOLESKY)
        self.g, self.gn, self.mu = st["g"], st["dx"], mu
        y = j_times(self.po, self.Jc, self.Jp, self.g, np.float64)
        self.sc = dict(g2=float(self.g @ self.g), q=float((y * y).sum()), gn2=float(self.gn @ self.gn), g_dot_gn=float(self.g @ self.gn), mu=mu)
        return dict(self.sc, energy_gn=self._trial(self.gn))

    def coefficients(self, g2, q, gn2, d, mu, radius):
        return tuple(float(v) for v in coefficients(g2, q, gn2, d, mu, radius, np.float64))

    def try_dogleg(self, radius):
        a, c, br, pred = self.coefficients(self.sc["g2"], self.sc["q"], self.sc["gn2"], self.sc["g_dot_gn"], self.mu, radius)
        dx = a * self.g + c * self.gn
        return self._trial(dx), pred, float(np.linalg.norm(dx)), br

    def accept(self):
        self.cam, self.pts = self.test
