"""GPU: the kernels of ba_relpose.hip.h on their own inputs (tests/relpose_harness.hip, compiled with the library's flags), against
tests/relpose_checks.py in long double on the inputs as the kernel holds them (for float: the lists and cam rounded to fp32 and widened).

  (a) k_relpose over an angle sweep of the residual rotation, 256 constraints per angle (one workgroup, so one pair of energy
      partials, per angle) and a last group of 37: the five blocks of every record and the two partials of every workgroup.
  (b) bits on the same inputs: trial against linearisation, an all-zero mask against no mask, masked columns, the mirrored halves of
      H_aa / H_bb, a go word of 0.
  (c) k_relpose_gather, (d) k_relpose_schur: one addition per entry in a fixed order, so numpy in T gives the same bits.
  (e) ba_relpose_matvec_row against the long-double sum.

Metric of a record block X (H_aa, H_bb, H_ab, g_a, g_b): max |X - X_ref| / max |X_ref| over the block (its entries are six-term sums of
mixed sign), the worst constraint of the group; of a partial: relative to the long-double sum.  Yardstick: the same formulas of
relpose_checks evaluated plainly in fp64 (dt = float64) on the same inputs, for float rounded once to fp32.  Bound: max(10 x the
yardstick's error by the same metric on the same group, floor).  The geometry is fp64 for both scalar types and a record entry is rounded
to T once, so the floors are a few roundings of the format: 8 eps64 (1.8e-15) for fp64, 1 eps32 (1.2e-7) for fp32.  Every figure is
printed as `RPK <case> <metric> <value> <bound>` before it is asserted.

One partial has a second term in its bound: the rotation energy where min(theta, pi - theta) < 1 / 128, theta = 0 excepted.  There
Log is ill-conditioned (an absolute 1e-16 in R_ab R0' is 1e-16 / theta of phi; next to pi, eps / (pi - theta) of phi's direction,
which the full L_r turns into |e_r|^2), so one constraint's energy carries a relative error of eps64 / min(theta, pi - theta) in any
fp64 evaluation; the 256 errors of a partial have random signs and leave 1 / 16 of that in the sum, which passes the floor 8 eps64
below 1 / 128.  The error of the yardstick's own sum is then one sample of that noise and no measure of it: another order of the same
operations (the kernel's (x + y) + z without fma against numpy's products) draws another sample.  What the yardstick does measure is
the size of the noise, rss = sqrt(sum of the squared errors of its terms) / sum, the standard deviation of a sum of errors with
random signs; the bound there is max(10 x yardstick, 10 x rss, floor).  The translation partial and the rotation partial at every
other angle keep the rule as it stands.  scripts/relpose_kernel_order.py evaluates the partials in the kernel's order of operations
in numpy, without a GPU: it gives the device's figures of the series groups digit for digit, 0.2 .. 2.8 rss.

Which branch of ba_relpose_eval an angle takes (fp64 inputs; `asin` = the series of theta / sin(theta) where s < 1e-3 and c > 0, `div` =
theta / s; `cot` = the series of Jl^-1's coefficient below theta = 0.05, `closed` = the closed form; the run prints the counts and asserts them):
  0, 1e-12, 1e-9, 1e-6, 1e-4, 9.9e-4   asin, cot          0.0501, 0.3, 1, pi/2 (c about 0), 2, 3 (c < 0), the tail (0.7)   div, closed
  1.01e-3, 1e-2, 0.0499                div, cot           pi - 1e-2 (s = 1e-2, c < 0)                                      div, closed
                                                          pi - 1e-3, pi - 1e-4, pi - 1e-6 (s < 1e-3, only c < 0 decides)   div, closed
For float the inputs are rounded to fp32, which turns the angles 0 < theta <= 1e-9 into 3e-9 .. 5e-8 and 1e-6 into 0.96e-6 .. 1.04e-6;
every angle keeps its branch.

Measured on an MI355X (profiles/r15_relpose_kernels.txt): see MEASURED below the imports."""
import numpy as np
import pytest

import prior_checks as PC
import relpose_checks as RC
import relpose_harness as RH

pytestmark = pytest.mark.gpu
F64, F32, LD = np.float64, np.float32, np.longdouble
DT = {0: F64, 1: F32}
SN = {0: "f64", 1: "f32"}
EPS = {0: float(np.finfo(F64).eps), 1: float(np.finfo(F32).eps)}
FLOOR = {0: 8 * EPS[0], 1: EPS[1]}
BITS = {0: np.uint64, 1: np.uint32}
PI = float(np.pi)
THETAS = [("0", 0.0), ("1e-12", 1e-12), ("1e-9", 1e-9), ("1e-6", 1e-6), ("1e-4", 1e-4), ("9.9e-4", 9.9e-4), ("1.01e-3", 1.01e-3),
          ("1e-2", 1e-2), ("0.0499", 0.0499), ("0.0501", 0.0501), ("0.3", 0.3), ("1", 1.0), ("pi/2", PI / 2), ("2", 2.0), ("3", 3.0),
          ("pi-1e-2", PI - 1e-2), ("pi-1e-3", PI - 1e-3), ("pi-1e-4", PI - 1e-4), ("pi-1e-6", PI - 1e-6)]
GROUP, TAIL, TAIL_THETA = 256, 37, 0.7
ILL = 1.0 / 128  # min(theta, pi - theta) below which the noise of a rotation partial passes its floor (module docstring)
BLOCKS = ("H_aa", "H_bb", "H_ab", "g_a", "g_b")

# MEASURED on an MI355X (profiles/r15_relpose_kernels.txt), the worst value of each kind, by value and by its ratio to the bound:
#   fp64 H blocks        away from pi 1.06e-15 (H_bb at 1e-9, bound 6.2e-15; by ratio H_aa of the tail, 5.8e-16 against 3.0e-15);
#                        next to pi 1.8e-10 (H_aa at pi - 1e-6, bound 9.3e-10)
#   fp64 g blocks        away from pi 1.4e-12 (g_a at 1.01e-3, yardstick 1.4e-12, bound 1.4e-11), then 3.7e-13 at 1e-12, 2.9e-13 at 1e-4,
#                        2.6e-13 at 1e-9, about 1e-13 elsewhere: t_ab - t0 cancels and the worst of 256 blocks is one whose g is small; by
#                        ratio g_a at 0.0499, 1.04e-13 against 4.8e-13.  Next to pi 8.9e-10 (g_b at pi - 1e-6, bound 5.9e-9); by ratio g_b at
#                        pi - 1e-4, 2.8e-11 against 1.2e-10.  The worst block next to pi is 3.9 .. 12.5 x eps64 / (pi - theta)
#   fp64 partials        translation 1.06e-15 (pi - 1e-2, bound 4.5e-15), by ratio 6.8e-16 against the floor 1.8e-15 (1e-6); rotation under
#                        the plain rule 6.9e-16 against 2.1e-15 (1e-2); rotation where Log is ill-conditioned 1.0e-14 at 1e-4 (yardstick
#                        9.4e-16, rss 5.1e-14), 9.6e-15 at pi - 1e-3 (3.5e-16, 3.8e-15: the largest ratio, 0.25), up to 7.3e-6 at 1e-12
#   fp32 record blocks   5.9e-8 at every angle (yardstick 5.9e-8, bound 5.9e-7): one rounding to float
#   fp32 partials        9.4e-8 (translation, theta = 0.3) against the floor 1.2e-7: 256 float terms in a tree of nine additions
#   matvec               fp64 2.3e-16, fp32 9.1e-8 (the yardstick's own 2.3e-16 / 9.1e-8) against 64 eps = 1.4e-14 / 7.6e-6

class Checker:
    def __init__(self, case):
        self.case, self.rows = case, []

    def __call__(self, metric, value, bound):
        self.rows.append((metric, float(value), float(bound)))
        print("RPK %s %s %.3e %.1e" % (self.case, metric, value, bound))

    def done(self):
        bad = [r for r in self.rows if not (r[1] <= r[2])]
        assert not bad, (self.case, bad)


def bits(a, scalar):
    return np.ascontiguousarray(a).view(BITS[scalar])


def same_bits(a, b, scalar):
    return a.shape == b.shape and np.array_equal(bits(a, scalar), bits(b, scalar))


@pytest.fixture(scope="module")
def rph(tmp_path_factory):
    return RH.Harness(RH.build(tmp_path_factory.mktemp("relpose_harness")))


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------
def _unit(rng):
    v = rng.standard_normal(3)
    return v / np.linalg.norm(v)


def _constraint(rng, theta):
    """Two cameras (doubles) and the lists of one constraint whose residual rotation has the angle theta (test_relpose_checks._pose_pair:
    exactly 0 for theta = 0, R_a = I and R0 = R_b, so that R_ab R0' = R_b R_b' is symmetric in every bit)."""
    cam = np.zeros((2, 15))
    cam[0, :9] = np.eye(3).reshape(-1) if theta == 0 else PC.rodrigues(_unit(rng) * rng.uniform(0.3, 2.5)).astype(F64).reshape(-1)
    cam[1, :9] = PC.rodrigues(_unit(rng) * rng.uniform(0.3, 2.5)).astype(F64).reshape(-1)
    cam[:, 9:12] = rng.standard_normal((2, 3)) * 3
    cam[:, 12:15] = [-500.0, 0.1, 0.01]
    Rab, tab = RC.relative_pose(cam, 0, 1)
    R0 = cam[1, :9].reshape(3, 3) if theta == 0 else (PC.rodrigues(_unit(rng) * LD(theta)).T @ Rab).astype(F64)
    return cam, R0, (tab + 0.1 * rng.standard_normal(3)).astype(F64), rng.standard_normal((3, 3)) * 2, rng.standard_normal((3, 3)) * 2


def _sweep_inputs():
    """19 angles x 256 constraints and a tail of 37 at theta = 0.7 (constraint 1 of the tail: L_r = 0, constraint 2: L_t = 0), each
    constraint on two cameras of its own; odd constraints list the pair as (b, a)'s slots swapped in the camera array, so that a > b
    occurs.  Returns (cam15 [2 n, 15], Constraints, group slices, names)."""
    rng = np.random.default_rng(1905)
    angles = [(nm, th, GROUP) for nm, th in THETAS] + [("tail", TAIL_THETA, TAIL)]
    cams, pairs, R0, t0, Lr, Lt, groups = [], [], [], [], [], [], []
    q = 0
    for nm, th, cnt in angles:
        groups.append((nm, th, slice(q, q + cnt)))
        for k in range(cnt):
            cam, r0, t_, lr, lt = _constraint(rng, th)
            if nm == "tail" and k == 1:
                lr = 0 * lr
            if nm == "tail" and k == 2:
                lt = 0 * lt
            a, b = (2 * q, 2 * q + 1) if q % 2 == 0 else (2 * q + 1, 2 * q)
            cams.append(cam if a < b else cam[::-1])
            pairs.append((a, b))
            R0.append(r0); t0.append(t_); Lr.append(lr); Lt.append(lt)
            q += 1
    return np.concatenate(cams), RC.Constraints(pairs, R0, t0, Lr, Lt), groups


def _held(cam15, cs, scalar):
    """The inputs as a kernel of that scalar type holds them, widened to double."""
    if scalar == 0:
        return np.asarray(cam15, F64), cs
    return np.asarray(cam15, F64).astype(F32).astype(F64), cs.rounded(F32)


def records(cs, cam15, dt, cmask=None):
    """The record blocks and the per-constraint energies of relpose_checks' residuals and Jacobians, all in dt."""
    et, er, ph = RC.residuals(cs, cam15, dt)
    J = RC.jacobians(cs, cam15, cmask, dt)
    e = np.concatenate([et, er], axis=1)
    Ja, Jb = J[:, :, :6], J[:, :, 6:]
    return dict(H_aa=np.einsum("nki,nkj->nij", Ja, Ja), H_bb=np.einsum("nki,nkj->nij", Jb, Jb), H_ab=np.einsum("nki,nkj->nij", Ja, Jb),
                g_a=-np.einsum("nki,nk->ni", Ja, e), g_b=-np.einsum("nki,nk->ni", Jb, e), er2=(er * er).sum(axis=1), et2=(et * et).sum(axis=1), phi=ph)


def split(rec, rph):
    """The blocks of an [n, BA_RP_REC] array of records."""
    n = len(rec)
    return dict(H_aa=rec[:, :36].reshape(n, 6, 6), H_bb=rec[:, 36:72].reshape(n, 6, 6), H_ab=rec[:, rph.HAB:rph.HAB + 36].reshape(n, 6, 6),
                g_a=rec[:, rph.G:rph.G + 6], g_b=rec[:, rph.G + 6:rph.G + 12])


def block_errors(X, ref):
    """max |X - X_ref| / max |X_ref| per constraint."""
    n = len(ref)
    d = np.abs(np.asarray(X).astype(LD) - ref).reshape(n, -1).max(axis=1)
    s = np.abs(ref).reshape(n, -1).max(axis=1)
    assert (s > 0).all()
    return (d / s).astype(F64)


def rel(x, ref):
    """|x - ref| / ref; against an exact 0: 0 where x is 0 too."""
    if ref == 0:
        return 0.0 if x == 0 else np.inf
    return float(abs(LD(x) - ref) / abs(ref))


_SWEEP = {}


def _sweep(rph, scalar):
    """Inputs, the long-double reference, the fp64 yardstick (rounded once to T) and the device's LIN run, once per scalar type."""
    if "in" not in _SWEEP:
        _SWEEP["in"] = _sweep_inputs()
    if scalar not in _SWEEP:
        cam15, cs, groups = _SWEEP["in"]
        cam, csr = _held(cam15, cs, scalar)
        ref = records(csr, cam, LD)
        y64 = records(csr, cam, F64)
        yard = {k: v.astype(DT[scalar]) for k, v in y64.items()}
        _SWEEP[scalar] = dict(cam=cam, cs=csr, groups=groups, ref=ref, y64=y64, yard=yard, lin=rph.relpose(scalar, RH.LIN, cam, csr))
    return _SWEEP[scalar]


# ---- (a) the angle sweep -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scalar", [0, 1], ids=["f64", "f32"])
def test_records_and_energies_over_the_angle_sweep(gpu_ok, rph, scalar):
    """k_relpose<T, true, false>: per angle the worst block error of the 256 records and the two energy partials of that workgroup."""
    W = _sweep(rph, scalar)
    ref, yard, out, dt = W["ref"], W["yard"], W["lin"], DT[scalar]
    n = len(W["cs"])
    assert n == len(THETAS) * GROUP + TAIL and out["part_e"].shape == (2, len(THETAS) + 1) and out["guards"].all()
    got = split(out["rec"], rph)
    assert np.isfinite(out["rec"]).all() and np.isfinite(out["part_e"]).all()
    err = {k: block_errors(got[k], ref[k]) for k in BLOCKS}
    yer = {k: block_errors(yard[k], ref[k]) for k in BLOCKS}
    ck = Checker("sweep[%s]" % SN[scalar])
    for g, (nm, th, sl) in enumerate(W["groups"]):
        ph = ref["phi"][sl]
        tha = np.sqrt((ph * ph).sum(axis=1)).astype(F64)
        asin, cot = (np.sin(tha) < 1e-3) & (np.cos(tha) > 0), tha < 0.05
        print("RPK sweep[%s] theta=%s held angle %.6e .. %.6e asin-series %d/%d cot-series %d/%d"
              % (SN[scalar], nm, tha.min(), tha.max(), asin.sum(), len(tha), cot.sum(), len(tha)))
        # the whole group on the side of both switches that the module docstring names, for the inputs as this scalar type holds them
        assert (asin == (th < 1e-3)).all() and (cot == (th < 0.05)).all(), (nm, int(asin.sum()), int(cot.sum()))
        worst = 0.0
        for k in BLOCKS:
            y = float(yer[k][sl].max())
            worst = max(worst, float(err[k][sl].max()))
            ck("theta=%s/%s(yardstick %.1e)" % (nm, k, y), err[k][sl].max(), max(10 * y, FLOOR[scalar]))
        en = []
        for row, key in ((0, "er2"), (1, "et2")):
            r = ref[key][sl]
            s_ref = r.sum()
            y = rel(dt(W["y64"][key][sl].sum()), s_ref)  # the plain fp64 sum of the fp64 terms, rounded once to T
            en.append(rel(out["part_e"][row, g], s_ref))
            name, bound = "theta=%s/%s(yardstick %.1e" % (nm, ("energy_rot", "energy_trans")[row], y), max(10 * y, FLOOR[scalar])
            if row == 0 and 0 < min(th, PI - th) < ILL:  # (module docstring: the rotation partial where Log is ill-conditioned)
                d = yard[key][sl].astype(LD) - r
                rss = float(np.sqrt((d * d).sum()) / s_ref)
                name, bound = name + ", rss of its terms %.1e" % rss, max(bound, 10 * rss)
            ck(name + ")", en[-1], bound)
        if scalar == 0 and th > 3.05:  # the header of ba_relpose.hip.h: accuracy degrades like eps / (pi - |phi|)
            gap = EPS[0] / (PI - th)
            print("RPK sweep[%s] theta=%s near_pi eps64/(pi-theta) %.3e worst_block %.3e (x %.2f) energy_rot %.3e (x %.2f)"
                  % (SN[scalar], nm, gap, worst, worst / gap, en[0], en[0] / gap))
    # the constraint without rotation information and the one without translation information (tail 1, 2)
    t0 = W["groups"][-1][2].start
    a_ = got["H_aa"][t0 + 2], got["H_bb"][t0 + 2], got["H_ab"][t0 + 2]
    zeros = [x[:3, :] for x in a_] + [x[:, :3] for x in a_] + [got["g_a"][t0 + 2][:3], got["g_b"][t0 + 2][:3]]
    ck("no_translation_information_rows_nonzero", sum(int(np.count_nonzero(z)) for z in zeros), 0)
    cam, cs = W["cam"], W["cs"]
    for q, row, name in ((t0 + 1, 0, "no_rotation_information_energy_rot"), (t0 + 2, 1, "no_translation_information_energy_trans")):
        a, b = cs.pairs[q]
        one = RC.Constraints([(0, 1)], cs.R0[q], cs.t0[q], cs.Lr[q], cs.Lt[q])
        o1 = rph.relpose(scalar, RH.LIN, cam[[a, b]], one)
        assert o1["guards"].all() and o1["part_e"][1 - row, 0] > 0
        ck(name, abs(float(o1["part_e"][row, 0])), 0)
        ck(name + "_record_bits_differ", 0 if same_bits(o1["rec"][0], out["rec"][q], scalar) else 1, 0)
    # L_r = 0 takes phi and Jl^-1 out of the record: the same constraint with another R0 (2.9 rad further) gives the same bits
    q = t0 + 1
    a, b = cs.pairs[q]
    R0x = (PC.rodrigues(np.array([0.0, 2.9, 0.0])) @ cs.R0[q]).astype(DT[scalar]).astype(F64)
    o2 = rph.relpose(scalar, RH.LIN, cam[[a, b]], RC.Constraints([(0, 1)], R0x, cs.t0[q], cs.Lr[q], cs.Lt[q]))
    assert o2["guards"].all() and not cs.Lr[q].any() and np.abs(R0x - cs.R0[q]).max() > 0.5
    ck("no_rotation_information_record_depends_on_R0", 0 if same_bits(o2["rec"][0], out["rec"][q], scalar) else 1, 0)
    ck("no_rotation_information_energy_rot_other_R0", abs(float(o2["part_e"][0, 0])), 0)
    ck.done()


# ---- (b) bits ----------------------------------------------------------------------------------------------------------------------------
MASKS = (0x03F, 0x007, 0x038)


@pytest.mark.parametrize("scalar", [0, 1], ids=["f64", "f32"])
def test_bits_on_the_same_inputs(gpu_ok, rph, scalar):
    """The contract above ba_relpose_eval and k_relpose: the trial's partials are the linearisation's, bit for bit; an all-zero mask
    changes nothing; a masked parameter's rows, columns and g entries are exactly 0 and every other entry keeps its bits; H_aa and
    H_bb are symmetric in bits; with a go word of 0 nothing is written."""
    W = _sweep(rph, scalar)
    cam, cs, lin = W["cam"], W["cs"], W["lin"]
    n, N = len(cs), len(W["cam"])
    assert same_bits(lin["part_e"], lin["part_keep"], scalar)
    tr = rph.relpose(scalar, RH.TRIAL, cam, cs)
    assert tr["guards"].all() and same_bits(tr["part_e"], lin["part_e"], scalar)
    assert RH.untouched(tr["rec"]) and RH.untouched(tr["part_keep"])
    go1 = rph.relpose(scalar, RH.LIN, cam, cs, go=1)
    assert go1["guards"].all() and all(same_bits(go1[k], lin[k], scalar) for k in ("rec", "part_e", "part_keep"))
    go0 = rph.relpose(scalar, RH.LIN, cam, cs, go=0)
    assert go0["guards"].all() and all(RH.untouched(go0[k]) for k in ("rec", "part_e", "part_keep"))
    m0 = rph.relpose(scalar, RH.LIN_MASK, cam, cs, cmask=np.zeros(N, np.uint16))
    assert m0["guards"].all() and all(same_bits(m0[k], lin[k], scalar) for k in ("rec", "part_e", "part_keep"))
    free = split(lin["rec"], rph)
    for k in ("H_aa", "H_bb"):
        assert same_bits(free[k], np.ascontiguousarray(free[k].transpose(0, 2, 1)), scalar), k
    # constraint q: mask MASKS[q % 3] on a (q // 3 % 3 == 0), on b (1), on both (2)
    cm = np.zeros(N, np.uint16)
    ma, mb = np.zeros(n, np.int64), np.zeros(n, np.int64)
    for q, (a, b) in enumerate(cs.pairs):
        where = q // 3 % 3
        if where != 1:
            cm[a] = ma[q] = MASKS[q % 3]
        if where != 0:
            cm[b] = mb[q] = MASKS[q % 3]
    mk = rph.relpose(scalar, RH.LIN_MASK, cam, cs, cmask=cm)
    assert mk["guards"].all() and same_bits(mk["part_e"], lin["part_e"], scalar) and same_bits(mk["part_keep"], lin["part_e"], scalar)
    got = split(mk["rec"], rph)
    fa = ((ma[:, None] >> np.arange(6)[None, :]) & 1) == 0  # [n, 6] free columns of a
    fb = ((mb[:, None] >> np.arange(6)[None, :]) & 1) == 0
    keep = dict(H_aa=fa[:, :, None] & fa[:, None, :], H_bb=fb[:, :, None] & fb[:, None, :], H_ab=fa[:, :, None] & fb[:, None, :], g_a=fa, g_b=fb)
    for k in BLOCKS:
        assert not keep[k].all() and keep[k].any()
        assert not np.count_nonzero(got[k][~keep[k]]), k
        assert np.array_equal(bits(got[k], scalar)[keep[k]], bits(free[k], scalar)[keep[k]]), k
        assert np.count_nonzero(free[k][~keep[k]]) > 0.99 * (~keep[k]).sum(), k  # (what the mask clears was not zero before)


# ---- (c) - (e): a hub, a chain, cameras without a constraint ---------------------------------------------------------------------------------
def _graph_inputs(N, pairs, seed):
    rng = np.random.default_rng(seed)
    cam = np.zeros((N, 15))
    for a in range(N):
        cam[a, :9] = PC.rodrigues(_unit(rng) * rng.uniform(0.3, 2.5)).astype(F64).reshape(-1)
    cam[:, 9:12] = rng.standard_normal((N, 3)) * 3
    cam[:, 12:15] = [-500.0, 0.1, 0.01]
    R0, t0 = [], []
    for a, b in pairs:
        Rab, tab = RC.relative_pose(cam, a, b)
        R0.append((PC.rodrigues(_unit(rng) * LD(rng.uniform(0.01, 2.8))).T @ Rab).astype(F64))
        t0.append((tab + 0.1 * rng.standard_normal(3)).astype(F64))
    n = len(pairs)
    return cam, RC.Constraints(pairs, R0, t0, rng.standard_normal((n, 3, 3)) * 2, rng.standard_normal((n, 3, 3)) * 2)


HUB_N = 40


def _hub_pairs():
    """360 constraints on 40 cameras: camera 0 in 300 of them (as a and as b in turn, with cameras 1 .. 29), a chain over 1 .. 29 in
    both orientations and four skips; cameras 30 .. 39 in none."""
    pairs = [(0, 1 + k % 29) if k % 2 == 0 else (1 + k % 29, 0) for k in range(300)]
    pairs += [(k, k + 1) for k in range(1, 29)] + [(k + 1, k) for k in range(1, 29)] + [(1, 3), (5, 3), (5, 7), (9, 7)]
    assert len(pairs) == 360
    return pairs


_HUB = {}


def _hub(rph, scalar):
    if scalar not in _HUB:
        cam, cs = _held(*_graph_inputs(HUB_N, _hub_pairs(), 77), scalar)
        out = rph.relpose(scalar, RH.LIN, cam, cs)
        assert out["guards"].all() and np.isfinite(out["rec"]).all()
        _HUB[scalar] = (cs.pairs, out["rec"])
    return _HUB[scalar]


@pytest.mark.parametrize("scalar", [0, 1], ids=["f64", "f32"])
def test_gather_adds_the_records_in_csr_order(gpu_ok, rph, scalar):
    """k_relpose_gather on the device's own records: V's 6 x 6 corners and gc[0..5] are the pre-filled values plus the camera's records
    in CSR order, added one by one in T (the same bits as numpy); everything else keeps its bits; V's corner stays symmetric in bits."""
    pairs, rec = _hub(rph, scalar)
    dt, N = DT[scalar], HUB_N
    rng = np.random.default_rng(5)
    V0 = rng.standard_normal((N, 9, 9))
    V0 = (V0 + V0.transpose(0, 2, 1)).astype(dt)
    gc0 = rng.standard_normal(9 * N).astype(dt)
    V, gc, guards = rph.gather(scalar, N, pairs, rec, V0, gc0)
    assert guards.all()
    ptr, inc = RH.csr(N, pairs)
    assert ptr[1] == 300 and (np.diff(ptr)[30:] == 0).all() and ptr[-1] == 2 * len(pairs)
    blk = split(rec, rph)
    Ve, ge = V0.copy(), gc0.copy().reshape(N, 9)
    for a in range(N):
        for w in inc[ptr[a]:ptr[a + 1]]:
            t, side = w >> 1, w & 1
            assert pairs[t][side] == a
            Ve[a, :6, :6] = Ve[a, :6, :6] + (blk["H_bb"] if side else blk["H_aa"])[t]
            ge[a, :6] = ge[a, :6] + (blk["g_b"] if side else blk["g_a"])[t]
    assert Ve.dtype == dt and ge.dtype == dt
    V = V.reshape(N, 9, 9)
    assert same_bits(V, Ve, scalar) and same_bits(gc, ge.reshape(-1), scalar)
    assert not same_bits(V[:30, :6, :6], V0[:30, :6, :6], scalar)
    corner = np.zeros((N, 9, 9), bool)
    corner[:30, :6, :6] = True
    assert np.array_equal(bits(V, scalar)[~corner], bits(V0, scalar)[~corner])
    assert same_bits(gc.reshape(N, 9)[:, 6:], gc0.reshape(N, 9)[:, 6:], scalar) and same_bits(gc[270:], gc0[270:], scalar)
    assert same_bits(V, np.ascontiguousarray(V.transpose(0, 2, 1)), scalar)
    Vn, gn, guards = rph.gather(scalar, N, pairs, rec, V0, gc0, go=0)
    assert guards.all() and same_bits(Vn.reshape(N, 9, 9), V0, scalar) and same_bits(gn, gc0, scalar)


@pytest.mark.parametrize("scalar", [0, 1], ids=["f64", "f32"])
def test_schur_adds_the_cross_blocks_into_the_lower_block_triangle(gpu_ok, rph, scalar):
    """k_relpose_schur, N = 9, ld = 128 > D = 81, every unordered pair once in a mix of a < b and a > b: S[(9 lo + c) ld + 9 hi + r] is
    the pre-filled value plus (J_hi' J_lo)[r][c] of the device's own record, one addition in T, and nothing else changes."""
    N, ld, dt = 9, 128, DT[scalar]
    rng = np.random.default_rng(9)
    pairs = [(a, b) if rng.integers(2) else (b, a) for a in range(N) for b in range(a + 1, N)]
    assert len(pairs) == 36 and 8 < sum(a > b for a, b in pairs) < 28
    cam, cs = _held(*_graph_inputs(N, pairs, 78), scalar)
    out = rph.relpose(scalar, RH.LIN, cam, cs)
    assert out["guards"].all() and np.isfinite(out["rec"]).all()
    Hab = split(out["rec"], rph)["H_ab"]
    S0 = rng.standard_normal((9 * N, ld)).astype(dt)
    S, guards = rph.schur(scalar, N, pairs, out["rec"], ld, S0)
    assert guards.all()
    Se, hit = S0.copy(), np.zeros(S0.shape, bool)
    for t, (a, b) in enumerate(pairs):
        hi, lo = max(a, b), min(a, b)
        blk = Hab[t] if a == hi else Hab[t].T  # J_hi' J_lo, [r][c]
        assert not np.array_equal(blk, blk.T)
        Se[9 * lo:9 * lo + 6, 9 * hi:9 * hi + 6] = Se[9 * lo:9 * lo + 6, 9 * hi:9 * hi + 6] + blk.T
        hit[9 * lo:9 * lo + 6, 9 * hi:9 * hi + 6] = True
    assert Se.dtype == dt and same_bits(S, Se, scalar)
    assert hit.sum() == 36 * 36 and not (bits(S, scalar)[hit] == bits(S0, scalar)[hit]).all()
    assert np.array_equal(bits(S, scalar)[~hit], bits(S0, scalar)[~hit])  # the upper block triangle, the intrinsics, the padding


@pytest.mark.parametrize("scalar", [0, 1], ids=["f64", "f32"])
def test_matvec_row_against_the_long_double_sum(gpu_ok, rph, scalar):
    """ba_relpose_matvec_row on the hub's records and a random v: y_a = sum over the incident constraints H_ab v_b (H_ba = H_ab') in
    long double, the error of a row relative to sum |H_ab| |v_b| of that row.  Yardstick: the same sums in numpy in T; floor 64 eps_T
    (the hub's rows sum 300 x 6 products)."""
    pairs, rec = _hub(rph, scalar)
    dt, N = DT[scalar], HUB_N
    v = np.random.default_rng(6).standard_normal(9 * N).astype(dt)
    y, guards = rph.matvec(scalar, N, pairs, rec, v)
    assert guards.all() and np.isfinite(y).all()
    Hab = split(rec, rph)["H_ab"]
    ref, mag, yard = np.zeros((N, 9), LD), np.zeros((N, 9), LD), np.zeros((N, 9), dt)
    for t, (a, b) in enumerate(pairs):
        H, va, vb = Hab[t], v[9 * a:9 * a + 6], v[9 * b:9 * b + 6]
        ref[a, :6] += H.astype(LD) @ vb.astype(LD)
        ref[b, :6] += H.astype(LD).T @ va.astype(LD)
        mag[a, :6] += np.abs(H).astype(LD) @ np.abs(vb).astype(LD)
        mag[b, :6] += np.abs(H).astype(LD).T @ np.abs(va).astype(LD)
        yard[a, :6] = yard[a, :6] + (H * vb[None, :]).sum(axis=1, dtype=dt)
        yard[b, :6] = yard[b, :6] + (H.T * va[None, :]).sum(axis=1, dtype=dt)
    y = y.reshape(N, 9)
    live = mag[:, :6] > 0
    assert live[:30].all() and not live[30:].any()
    e_gpu = float((np.abs(y[:, :6].astype(LD) - ref[:, :6])[live] / mag[:, :6][live]).max())
    e_yard = float((np.abs(yard[:, :6].astype(LD) - ref[:, :6])[live] / mag[:, :6][live]).max())
    ck = Checker("matvec[%s]" % SN[scalar])
    ck("rows(yardstick %.1e)" % e_yard, e_gpu, max(10 * e_yard, 64 * EPS[scalar]))
    ck("intrinsics_rows_nonzero", np.count_nonzero(y[:, 6:]), 0)
    ck("unconstrained_cameras_nonzero", np.count_nonzero(y[30:]), 0)
    ck.done()
