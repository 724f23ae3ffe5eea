"""Powell's dogleg on the CPU: ba_dogleg_coefficients (host only) against the long double rule of tests/dogleg_checks.py on designed
scalars, the step's length and predicted decrease on the oracle's linearisation of problem-21, the reachability of the interpolated
branch that tests/test_gpu_dogleg.py relies on, and the driver's control rule on a scripted problem.  No GPU needed."""
import math

import numpy as np
import pytest

import dogleg_checks as DG
from conftest import DATA21, DATA39

LD = np.longdouble
MU = 1e-3


def _lin(O, p):
    cam = O.init_cams(p)
    f, e = O.residuals(p, cam, p.pts)
    Jc, Jp = O.jacobian(p, cam, p.pts)
    return np.asarray(f).reshape(p.K, 2), np.asarray(Jc).reshape(p.K, 2, 9), np.asarray(Jp).reshape(p.K, 2, 3)


def _dmax(p, Jc, Jp, f):
    U, V, _ = DG.DC.normal_blocks(p, Jc, Jp, f, np.float64)
    dp, dc = DG.DC.diagonals(U, V)
    return float(max(dp.max(), dc.max()))


@pytest.fixture(scope="module")
def full(O):
    """problem-21 and problem-39 whole, at the oracle's linearisation."""
    out = {}
    for name, path in (("p21", DATA21), ("p39", DATA39)):
        p = O.load_bal(path)
        out[name] = (p,) + _lin(O, p)
    return out


@pytest.fixture(scope="module")
def ref21(full):
    p, f, Jc, Jp = full["p21"]
    return DG.Reference(p, Jc, Jp, f, None, 1e-6 * _dmax(p, Jc, Jp, f))


# designed scalars: g = (2, 0), H = diag(2, 1/2)-like numbers chosen by hand; alpha = g2 / q = 0.5, |dx_sd| = 1, |dx_gn| = 3
G2, Q, GN2, D = 4.0, 8.0, 9.0, 3.0
DESIGNED = [
    ("gn_inside", (G2, Q, GN2, D, MU, 3.5), 0),
    ("gn_radius_exactly_its_norm", (G2, Q, GN2, D, MU, 3.0), 0),          # sqrt(gn2) <= radius: the <= side
    ("gn_just_outside", (G2, Q, GN2, D, MU, math.nextafter(3.0, 0.0)), 2),
    ("inf", (G2, Q, GN2, D, MU, math.inf), 0),
    ("gradient", (G2, Q, GN2, D, MU, 0.25), 1),
    ("gradient_radius_exactly_cauchy", (G2, Q, GN2, D, MU, 1.0), 1),      # alpha sqrt(g2) >= radius: the >= side
    ("interpolated_just_past_cauchy", (G2, Q, GN2, D, MU, math.nextafter(1.0, 2.0)), 2),
    ("interpolated_B_positive", (G2, Q, GN2, D, MU, 2.0), 2),             # B = alpha d - alpha^2 g2 = 0.5 > 0
    ("interpolated_B_negative", (G2, Q, GN2, 1.5, MU, 2.0), 2),           # B = -0.25 <= 0
    ("interpolated_B_zero", (G2, Q, GN2, 2.0, MU, 2.0), 2),
    ("tiny_radius", (G2, Q, GN2, D, MU, 1e-300), 1),
    ("flat_gradient", (0.0, 0.0, 0.0, 0.0, MU, 1.0), 0),                  # g2 = 0: a = c = 0, pred = 0
    ("flat_gradient_q_positive", (0.0, 1.0, 2.0, 0.0, MU, 1.0), 0),
]


@pytest.mark.parametrize("name,args,branch", DESIGNED, ids=[d[0] for d in DESIGNED])
def test_coefficients_against_long_double(ba, name, args, branch):
    """a, c, pred to 16 eps64 of the long double rule, the branch exactly; |a g + c dx_gn| = min(radius, |dx_gn|) for the vectors the
    scalars were made from.  The scales: beta is a number in (0, 1] whose root form does not cancel, but C = alpha^2 g2 - radius^2 does
    at the Cauchy end and 1 - beta at the Gauss-Newton end, each leaving an ABSOLUTE error of a few eps64: c is held relative to 1, a
    relative to alpha (the error of the step is then eps64 of the Cauchy and the Gauss-Newton step), pred relative to the sum of the
    magnitudes of its terms."""
    a, c, br, pred = ba.dogleg_coefficients(*args)
    ra, rc, rbr, rpred = DG.coefficients(*args)
    assert br == rbr == branch
    tol = 16 * np.finfo(np.float64).eps
    g2, q, gn2, d, mu, radius = args
    alpha = g2 / q if g2 > 0 else 0.0
    terms = 2 * (abs(ra) * g2 + rc * d) + ra * ra * q + 2 * abs(ra) * rc * g2 + rc * rc * d
    for got, want, scale in ((a, ra, max(abs(ra), alpha)), (c, rc, 1.0), (pred, rpred, terms)):
        assert abs(LD(got) - want) <= tol * scale, (name, got, want)
    if g2 == 0:
        assert (a, c, pred) == (0.0, 0.0, 0.0)
        return
    # |a g + c dx_gn|^2 = a^2 g2 + 2 a c d + c^2 gn2
    n = float(np.sqrt(LD(a) * LD(a) * g2 + 2 * LD(a) * c * d + LD(c) * c * gn2))  # (long double's range: a^2 underflows a double at 1e-300)
    want = min(radius, math.sqrt(gn2))
    assert abs(n - want) <= 16 * np.finfo(np.float64).eps * want, (name, n, want)
    if br == 0:
        assert (a, c) == (0.0, 1.0)
    if br == 1:
        assert c == 0.0
    if br == 2:
        assert 0 < c <= 1 and a >= 0


REFUSED = [
    (-1.0, Q, GN2, D, MU, 1.0), (G2, -1.0, GN2, D, MU, 1.0), (G2, Q, -1.0, D, MU, 1.0), (G2, Q, GN2, -1.0, MU, 1.0),
    (math.nan, Q, GN2, D, MU, 1.0), (G2, math.inf, GN2, D, MU, 1.0), (G2, Q, math.nan, D, MU, 1.0), (G2, Q, GN2, math.inf, MU, 1.0),
    (G2, Q, GN2, D, 0.0, 1.0), (G2, Q, GN2, D, -1.0, 1.0), (G2, Q, GN2, D, math.inf, 1.0), (G2, Q, GN2, D, math.nan, 1.0),
    (G2, Q, GN2, D, MU, 0.0), (G2, Q, GN2, D, MU, -1.0), (G2, Q, GN2, D, MU, math.nan), (G2, Q, GN2, D, MU, -math.inf),
    (G2, 0.0, GN2, D, MU, 1.0),
]


@pytest.mark.parametrize("args", REFUSED, ids=[str(i) for i in range(len(REFUSED))])
def test_coefficients_refusals(ba, args):
    with pytest.raises(ba.BAError) as ei:
        ba.dogleg_coefficients(*args)
    assert ei.value.code == ba.ERR_ARG
    with pytest.raises(ValueError):
        DG.coefficients(*args)


def test_params_default(ba):
    p = ba.DoglegParams.default()
    lm = ba.LMParams()
    ba.lib().ba_lm_params_default(__import__("ctypes").byref(lm))
    assert (p.radius_init, p.radius_min, p.radius_max, p.mu_rel, p.mu_rel_max, p.tol_fun) == (0.0, 1e-32, 1e16, 1e-12, 1.0, 1e-8)
    assert (p.max_iter, p.max_fun_ev, p.max_trials, p.verbose) == (lm.max_iter, lm.max_fun_ev, 0, 0)


def test_step_length_and_pred_on_problem21(ba, ref21):
    """On the oracle's J of problem-21 at mu = 1e-6 max diag J'J, in each branch: |dx| = min(radius, |dx_gn|) to rounding, and the
    predicted decrease from the six scalars against 2 g'dx - |J dx|^2 in long double.  The two differ by the residual of the reference
    trial, (H + mu I) dx_gn - g, times the step: the long double solve refines to 2^-53 of the scaled system (damping_checks.solve
    stops when the double-precision corrections stop shrinking), so 1e-9 of the sum of the magnitudes of pred's terms is the bound;
    the library's doubles are then held to 64 eps64 of the long double rule on the same scalars."""
    r = ref21
    eps = np.finfo(np.float64).eps
    radii = (2 * r.gn_norm, LD(math.inf), r.sd_norm / 2, np.sqrt(r.sd_norm * r.gn_norm))
    for radius, branch in zip(radii, (0, 0, 1, 2)):
        a, c, br, dx, pred = r.step(radius)
        assert br == branch
        n = np.sqrt((dx * dx).sum())
        want = min(radius, r.gn_norm)
        assert abs(n - want) <= 1e-12 * want, (branch, float(n), float(want))
        direct = r.pred_direct(dx)
        y = DG.j_times(r.p, r.Jc, r.Jp, dx)
        scale = 2 * (np.abs(r.g) * np.abs(dx)).sum() + (y * y).sum()
        print("DOGLEG cpu21 pred[branch %d] %.3e vs %.3e rel %.2e" % (branch, float(pred), float(direct), float(abs(pred - direct) / scale)))
        assert abs(pred - direct) <= 1e-9 * scale, (branch, float(pred), float(direct))
        assert pred > 0
        ga, gc, gbr, gpred = ba.dogleg_coefficients(float(r.g2), float(r.q), float(r.gn2), float(r.d), float(r.mu), float(radius))
        assert gbr == branch
        # (the scalars were rounded to doubles on the way in: 4 eps64 of input error besides the rule's own)
        assert abs(LD(gpred) - pred) <= 64 * eps * scale and abs(LD(ga) - a) <= 64 * eps * max(abs(a), LD(1e-300)) and abs(LD(gc) - c) <= 64 * eps


def test_interpolated_branch_is_reachable(full):
    """The self-consistency tests/test_gpu_dogleg.py relies on: on problem-21 and problem-39 at mu = 1e-6 and 1e-2 max diag J'J the Cauchy
    step is less than half as long as the Gauss-Newton step (measured: 4.1e-4 and 0.149 on problem-21, 4.2e-4 and 0.144 on problem-39),
    so a radius between the two exists and the interpolated branch is reached."""
    for name in ("p21", "p39"):
        p, f, Jc, Jp = full[name]
        dmax = _dmax(p, Jc, Jp, f)
        for rel in (1e-6, 1e-2):
            r = DG.Reference(p, Jc, Jp, f, None, rel * dmax)
            ratio = float(r.sd_norm / r.gn_norm)
            print("DOGLEG cpu %s@%.0e cauchy/gn %.3e" % (name, rel, ratio))
            assert ratio < 0.5
            assert r.step(np.sqrt(r.sd_norm * r.gn_norm))[2] == 2


class _Scripted:
    """The four calls on a script: a quadratic in one unknown, E(x) = h (x - 1)^2 + 1, from x = 0, so every number can be followed by hand."""

    def __init__(self, h=2.0, bad_prepares=0):
        self.h, self.x, self.bad, self.log = h, 0.0, bad_prepares, []

    def E(self, x):
        return self.h * (x - 1) ** 2 + 1

    def linearize(self):
        self.log.append("lin")
        return self.E(self.x), self.h

    def prepare(self, mu):
        self.log.append("prep")
        g = -self.h * (self.x - 1)  # g = -J'e with J = sqrt(h), e = sqrt(h) (x - 1)
        gn = g / (self.h + mu)
        self.info = dict(g2=g * g, q=self.h * g * g, gn2=gn * gn, g_dot_gn=g * gn, mu=mu)
        self.g, self.gn = g, gn
        self.test = self.x + gn
        if self.bad > 0:  # a model that does not decrease: the driver must raise mu and not count a trial
            self.bad -= 1
            if self.bad % 2:
                return dict(self.info, gn2=math.nan, energy_gn=self.E(self.test))  # (a step that is not finite: the rule refuses the scalars)
            return dict(self.info, g_dot_gn=1e308, energy_gn=self.E(self.test))  # (2 g'dx_gn overflows: pred is not finite)
        return dict(self.info, energy_gn=self.E(self.test))

    def coefficients(self, *a):
        return tuple(float(v) for v in DG.coefficients(*a, dtype=np.float64))

    def try_dogleg(self, radius):
        self.log.append("try")
        a, c, br, pred = self.coefficients(self.info["g2"], self.info["q"], self.info["gn2"], self.info["g_dot_gn"], self.info["mu"], radius)
        dx = a * self.g + c * self.gn
        self.test = self.x + dx
        return self.E(self.test), pred, abs(dx), br

    def accept(self):
        self.log.append("acc")
        self.x = self.test


def test_control_rule_on_a_quadratic():
    """A quadratic is its own model: rho = 1 on every trial.  With radius_init = 0 the first radius is |dx_gn| and the first trial is the
    prepare's own Gauss-Newton step, not evaluated again; the radius triples; with mu = 0.1 max diag J'J the error shrinks elevenfold
    per iteration until a step is flat: BA_SUCCESS with the step taken, and not one dogleg evaluation on the way.  With radius_init
    below the Cauchy length the first trial is a scaled-gradient step of exactly that length."""
    s = _Scripted()
    out = DG.drive(s, mu_rel=0.1)
    rows = out["rows"]
    assert out["status"] == DG.SUCCESS and out["trials"] == len(rows) == out["iterations"] and 3 <= len(rows) <= 12
    assert "try" not in s.log and s.log[:4] == ["lin", "prep", "acc", "lin"] and s.log[-1] == "acc"
    assert np.all(rows[:, 1] == 1) and np.all(np.abs(rows[:-1, 3] - 1) < 1e-6) and rows[0, 2] == 3.0
    assert rows[0, 4] == abs(2.0 / 2.2) and rows[1, 4] == 3 * rows[0, 4] and abs(s.x - 1) < 1e-3
    assert out["energy"] == rows[-1, 5] and out["fun_evals"] == 1 + len(rows)
    s = _Scripted()
    out = DG.drive(s, radius_init=0.25, max_trials=2)
    assert s.log[:6] == ["lin", "prep", "try", "acc", "lin", "prep"] and out["status"] == DG.RUNNING and out["trials"] == 2
    assert list(out["rows"][:, 4]) == [0.25, 0.75] and np.all(out["rows"][:, 1] == 1) and "try" not in s.log[6:]


def test_control_rule_retries_and_limits():
    """A prepare whose Gauss-Newton pred is not positive is repeated with ten times the regularisation and is no trial; mu_rel m beyond
    mu_rel_max, a radius below radius_min, max_iter and max_fun_ev end the run with their status."""
    s = _Scripted(bad_prepares=2)
    out = DG.drive(s, max_trials=1)
    assert s.log[:4] == ["lin", "prep", "prep", "prep"] and out["trials"] == 1 and out["fun_evals"] == 4
    assert DG.drive(_Scripted(bad_prepares=50), mu_rel_max=1e-3)["status"] == DG.EXCEEDED
    assert DG.drive(_Scripted(), max_iter=1)["status"] == DG.MAX_ITERS
    assert DG.drive(_Scripted(), max_fun_ev=2)["status"] == DG.TOO_MANY_FUN_EVALS
    assert DG.drive(_Scripted(), radius_init=1e-3, radius_min=1e-2)["status"] == DG.EXCEEDED
