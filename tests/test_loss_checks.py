"""CPU: the yardstick of the measurement model (tests/loss_checks.py) pinned on its own, the contract's declarations, and the register
report of the new k_eval instantiations (hipcc cross-compiles gfx950).  No GPU needed.

Bounds, from the number formats: the yardstick starts from quad results rounded ONCE to double (2^-53 = 1.1e-16 relative per
entry) and works in long double (2^-64) from there.
  * against referee_linearize(tau = 0.5): both sides carry one double rounding of their inputs / outputs and the chain rule multiplies
    entries of comparable size: 1e-13 of the largest entry of each array leaves three decimal digits over 2^-53 for the cancellation in
    (nr - rr00) of the reference's own form (oracle_impl: c2 (nr - rr00)) near r0 = 0 or r1 = 0;
  * sum e^2 = sum rho: long double throughout, K = 1e4 terms of one sign: 1e-16;
  * finite differences: the moved states are rounded to double, which moves a pixel by 2^-53 |x| |dr/dx| ~ 1e-13 px, and the steps
    move it by 1e-3 px: 1e-10 of the quotient; the Richardson step removes the h^2 term and leaves (1e-3 px / scale)^4 = 1e-12.
    1e-7 of the largest entry of the observation's 2 x 12 block leaves three digits for columns whose entries are small next to it."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import loss_checks as LC
from conftest import DATA21, ROOT

LD = np.longdouble
CASES = [(LC.REFERENCE, 2.0), (LC.TRIVIAL, 1.0), (LC.HUBER, 1.0), (LC.CAUCHY, 1.0)]


def relmax(a, b):
    return float(np.abs(np.asarray(a, LD) - np.asarray(b, LD)).max() / max(np.abs(np.asarray(b, LD)).max(), LD(1e-300)))


@pytest.fixture(scope="module")
def excerpt(O):
    po = O.load_bal(DATA21).subset(1500)
    return po, O.init_cams(po)


def test_psi_at_half_a_pixel_is_the_referee(O, excerpt):
    po, cam = excerpt
    R = O.referee_linearize(po, cam, po.pts, 0.5)
    Y = LC.model(O, po, cam, po.pts, LC.REFERENCE, 0.5)
    got = dict(f=Y["e"].ravel(), Jc=Y["Jc"], Jp=Y["Jp"], g=Y["g"])
    for k in ("f", "Jc", "Jp", "g"):
        err = relmax(got[k], R[k])
        print("LOSS yardstick_vs_referee %s %.3e %.1e" % (k, err, 1e-13))
        assert err <= 1e-13, k
    assert abs(float(Y["energy"]) - R["energy"]) <= 1e-13 * R["energy"]
    share = float((Y["s"] < 0.25).mean())
    assert 0.05 < share < 0.95, share  # both branches of psi were compared


@pytest.mark.parametrize("kind,scale", CASES, ids=[LC.KIND_NAMES[k] for k, _ in CASES])
def test_sum_of_squares_is_sum_of_rho(O, excerpt, kind, scale):
    po, cam = excerpt
    w = np.random.default_rng(3).uniform(0.25, 4.0, po.K)
    for ww in (None, w):
        Y = LC.model(O, po, cam, po.pts, kind, scale, ww)
        assert abs(Y["energy"] - Y["rho"].sum()) <= LD(1e-16) * Y["rho"].sum()
        assert abs(LC.energy(O, po, cam, po.pts, kind, scale, ww) - Y["rho"].sum()) <= LD(1e-16) * Y["rho"].sum()
        assert np.isfinite(Y["Jc"].astype(np.float64)).all() and np.isfinite(Y["Jp"].astype(np.float64)).all()


STEP = [1e-6, 1e-6, 1e-6, 1e-7, 1e-7, 1e-7, 1e-3, 1e-5, 1e-4, 1e-6, 1e-6, 1e-6]  # T, omega, f, k1, k2 | X: each moves a pixel by ~1e-3 px


def _moved_state(cam15, pts, N, q, step):
    """x (+) step e_q for every camera (q < 9: T, omega, f, k1, k2 -- the camera block of BA_GET_JC) or every point (q >= 9), as the
    reference's update_params moves it (BAFunctor.h:299-342): additive, the rotation by left-multiplication with the Rodrigues matrix
    of the increment -- in long double, rounded to the double state the referee takes."""
    c = cam15.reshape(N, 15).astype(LD).copy()
    x = pts.reshape(-1, 3).astype(LD).copy()
    if q >= 9:
        x[:, q - 9] += LD(step)
    elif q < 3:
        c[:, 9 + q] += LD(step)
    elif q >= 6:
        c[:, 6 + q] += LD(step)
    else:
        om = np.zeros(3, LD)
        om[q - 3] = LD(step)
        th = abs(LD(step))
        Jx = np.array([[0, -om[2], om[1]], [om[2], 0, -om[0]], [-om[1], om[0], 0]], LD)
        dR = np.eye(3, dtype=LD) + np.sin(th) / th * Jx + (1 - np.cos(th)) / (th * th) * (Jx @ Jx)
        c[:, :9] = np.einsum("ij,njk->nik", dR, c[:, :9].reshape(N, 3, 3)).reshape(N, 9)
    return c.astype(np.float64).ravel(), x.astype(np.float64).ravel()


def test_jacobian_is_the_finite_difference_of_the_residual(O):
    """Every column of the tangent space moved at once for all cameras (all points): an observation sees its own camera and point
    only.  Central differences at h and h / 2 (STEP: a pixel moves by ~1e-3 px, far inside the losses' scales of 1 - 2 px),
    Richardson-extrapolated; the raw residuals of the 48 moved states are shared by the four kinds.  The moved states are rounded to
    double (2^-53 |x| |dr/dx| ~ 1e-13 px against a difference of 2e-3 px: 1e-10 relative).  Observations within 2 % of a kink (in
    sqrt(s)) are left out of THIS test: rho is C1 there, a difference quotient across the kink carries the jump of rho''."""
    po = O.load_bal(DATA21).subset(40)
    cam = O.init_cams(po)
    w = np.random.default_rng(5).uniform(0.25, 4.0, po.K)
    K = po.K
    moved = {}
    for q in range(12):
        for sgn in (1, -1):
            for div in (1, 2):
                co, pt = _moved_state(cam, po.pts, po.N, q, sgn * STEP[q] / div)
                moved[(q, sgn, div)] = LC.raw(O, po, co, pt)
    r0, Jc0, Jp0 = LC.raw(O, po, cam, po.pts)
    checked = 0
    for kind, scale in CASES:
        for ww in (None, w):
            Y = LC.apply_model(po, r0, Jc0, Jp0, kind, scale, ww)
            fd = np.zeros((K, 2, 12), LD)
            for q in range(12):
                d = {}
                for div in (1, 2):
                    ep = LC.apply_model(po, *moved[(q, 1, div)], kind, scale, ww)["e"]
                    em = LC.apply_model(po, *moved[(q, -1, div)], kind, scale, ww)["e"]
                    d[div] = (ep - em) / (2 * LD(STEP[q]) / div)
                fd[:, :, q] = (4 * d[2] - d[1]) / 3
            J = np.concatenate([Y["Jc"], Y["Jp"]], axis=2)
            far = np.abs(np.sqrt(Y["s"].astype(np.float64)) / scale - 1) > 0.02 if kind in (LC.REFERENCE, LC.HUBER) else np.ones(K, bool)
            assert far.sum() >= K // 2
            sc = np.abs(J).max(axis=(1, 2))
            err = float((np.abs(J - fd).max(axis=(1, 2)) / sc)[far].max())
            print("LOSS yardstick_fd %s weights=%s %.3e %.1e (%d observations)" % (LC.KIND_NAMES[kind], ww is not None, err, 1e-7, far.sum()))
            assert err <= 1e-7, (kind, ww is not None)
            checked += int(far.sum())
    assert checked > 0


def test_tiny_residuals_are_rebuilt_from_a_moved_measurement(O, excerpt):
    """The referee's clamps (module docstring of loss_checks): with the measurements of every tenth observation replaced by the
    yardstick's own projection the raw residual there is rounding (< 1e-12 px), dr/dx is what it was to 2^-53-level changes of the
    inputs -- the measurement does not enter it -- and every kind's e and J stay finite, J = sqrt(rho'(0)) dr/dx."""
    po, cam = excerpt
    r, Jc, Jp = LC.raw(O, po, cam, po.pts)
    m = po.meas.reshape(-1, 2).copy()
    sel = np.arange(0, po.K, 10)
    m[sel] = (m[sel].astype(LD) + r[sel]).astype(np.float64)
    p2 = O.Problem(po.N, po.M, po.K, po.cam_idx, po.pt_idx, m.ravel(), po.cams9, po.pts)
    r2, Jc2, Jp2 = LC.raw(O, p2, cam, po.pts)
    assert float(np.abs(r2[sel]).max()) < 1e-12
    assert relmax(Jc2, Jc) <= 1e-15 and relmax(Jp2, Jp) <= 1e-15
    for kind, scale in CASES:
        Y = LC.apply_model(p2, r2, Jc2, Jp2, kind, scale)
        g0 = np.sqrt(0.5) if kind == LC.REFERENCE else 1.0
        assert np.isfinite(Y["e"].astype(np.float64)).all()
        assert relmax(Y["Jc"][sel], g0 * Jc2[sel]) <= 1e-15 and relmax(Y["Jp"][sel], g0 * Jp2[sel]) <= 1e-15


def test_header_and_binding_declare_the_measurement_model(ba):
    hdr = open(os.path.join(ROOT, "include", "ba_mi355x.h")).read()
    assert re.search(r"BA_LOSS_REFERENCE\s*=\s*0\s*,\s*BA_LOSS_TRIVIAL\s*=\s*1\s*,\s*BA_LOSS_HUBER\s*=\s*2\s*,\s*BA_LOSS_CAUCHY\s*=\s*3\s*}\s*ba_loss_kind\s*;", hdr)
    assert re.search(r"\bint\s+ba_solver_set_loss\s*\(\s*ba_solver\s*\*\s*s\s*,\s*int\s+kind\s*,\s*double\s+scale\s*\)\s*;", hdr)
    assert re.search(r"\bint\s+ba_solver_set_obs_weights\s*\(\s*ba_solver\s*\*\s*s\s*,\s*const\s+double\s*\*\s*w\b", hdr)
    assert {"ba_solver_set_loss", "ba_solver_set_obs_weights"} <= set(ba.EXPORTS)
    assert (ba.LOSS_REFERENCE, ba.LOSS_TRIVIAL, ba.LOSS_HUBER, ba.LOSS_CAUCHY) == (0, 1, 2, 3)
    assert (LC.REFERENCE, LC.TRIVIAL, LC.HUBER, LC.CAUCHY) == (0, 1, 2, 3)
    assert hasattr(ba.Solver, "set_loss") and hasattr(ba.Solver, "set_obs_weights")
    L = ba.lib()
    assert hasattr(L, "ba_solver_set_loss") and hasattr(L, "ba_solver_set_obs_weights")


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not available")
def test_model_instantiations_of_k_eval_keep_their_registers(tmp_path):
    """tests/loss_resources.hip instantiates launch_eval's nine MODEL instantiations of k_eval per scalar type next to the five unmasked
    defaults, compiled with csrc/Makefile's own flags: no spills, no scratch, and the fused fp64 linearisation of the model
    (k_eval<double, true, 2, false, *, true>: CHOLESKY behind an accepted step) keeps at least the waves per SIMD of the default's."""
    import qr_harness as QH
    hipcc, flags = QH.makefile_flags()
    out = subprocess.run([hipcc] + flags + ["-w", "-I", QH.CSRC, "--cuda-device-only", "-c", os.path.join(ROOT, "tests", "loss_resources.hip"), "-o",
                          str(tmp_path / "loss.o"), "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    usage = {}
    for m in re.finditer(r"Function Name: (\S+)", out.stderr):
        block = out.stderr[m.end():m.end() + 2500]
        get = lambda pat: int(re.search(pat, block).group(1))  # noqa: E731
        usage[m.group(1)] = dict(vgpr=get(r"VGPRs: (\d+)"), occ=get(r"Occupancy \[waves/SIMD\]: (\d+)"), spill=get(r"VGPRs Spill: (\d+)"),
                                 sspill=get(r"SGPRs Spill: (\d+)"), scratch=get(r"ScratchSize \[bytes/lane\]: (\d+)"))
    # _Z6k_evalI<T>Lb<JAC>ELi<FUSE>ELb<SOA>ELb<MASK>ELb<MODEL>EE...
    pat = re.compile(r"^_Z6k_evalI([df])Lb([01])ELi([012])ELb([01])ELb([01])ELb([01])EE")
    ev = {}
    for k, v in usage.items():
        m = pat.match(k)
        if m:
            ev[(m.group(1),) + tuple(int(x) for x in m.groups()[1:])] = v
    for k, v in sorted(ev.items()):
        print("LOSS resources k_eval%s %s" % (k, v))
    model = {k: v for k, v in ev.items() if k[5] == 1}
    assert len(model) == 18 and len(ev) == 28, sorted(ev)
    for k, v in model.items():
        assert v["spill"] == 0 and v["sspill"] == 0 and v["scratch"] == 0, (k, v)
    default = ev[("d", 1, 2, 0, 0, 0)]
    for mask in (0, 1):
        assert model[("d", 1, 2, 0, mask, 1)]["occ"] >= default["occ"], (mask, model[("d", 1, 2, 0, mask, 1)], default)
