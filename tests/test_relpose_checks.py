"""CPU: the yardstick of the relative-pose constraints (tests/relpose_checks.py) pinned on its own, and the contract's declarations.
No GPU needed.

Bounds, from the number formats.  Everything is long double (eps = 2^-64 = 5.4e-20); poses are O(1) .. O(10).
  * finite differences: central differences with step h = 1e-6 through `retract` leave a truncation term h^2 |e'''| / 6 = 2e-13 x O(10)
    and a roundoff term eps |e| / h = 5e-14 x O(10), both relative to entries of J of size O(1) .. O(10): bound 1e-7 of the largest
    entry of the constraint's Jacobian, as the issue sets it;
  * invariance under a rigid motion of the world: R_b Q (R_a Q)' and T + R c pass through a dozen long-double operations on O(10)
    values: 1e-15 relative to the residual's largest entry (the issue's bound) leaves four digits;
  * Jl^-1 Jl = I: both from closed forms above their series thresholds, where the cancellation in 1 - cos th and in
    1 / th^2 - (1 + cos th) / (2 th sin th) costs eps / th^2 <= 2.5e3 eps relative to terms that enter with a factor th .. th^2: a few
    hundred eps absolute, bound 1e-17;
  * `direct` against the dense J'J of the stacked rows: the same products in another order: 1e-17."""
import os
import re
import subprocess

import numpy as np
import pytest

import prior_checks as PC
import relpose_checks as RC
from conftest import ROOT

LD = np.longdouble


def relmax(a, b):
    return float(np.abs(np.asarray(a, LD) - np.asarray(b, LD)).max() / max(np.abs(np.asarray(b, LD)).max(), LD(1e-300)))


def _unit(rng):
    v = rng.standard_normal(3)
    return v / np.linalg.norm(v)


def _pose_pair(rng, theta):
    """Two cameras (doubles) and a constraint whose residual rotation has the angle theta (exactly 0 for theta = 0: R_a = I and
    R0 = R_b, so that R_ab R0' = R_b R_b' is symmetric in every bit)."""
    cam = np.zeros((2, 15))
    if theta == 0:
        cam[0, :9] = np.eye(3).reshape(-1)
    else:
        cam[0, :9] = PC.rodrigues(_unit(rng) * rng.uniform(0.3, 2.5)).astype(np.float64).reshape(-1)
    cam[1, :9] = PC.rodrigues(_unit(rng) * rng.uniform(0.3, 2.5)).astype(np.float64).reshape(-1)
    cam[:, 9:12] = rng.standard_normal((2, 3)) * 3
    cam[:, 12:15] = [-500.0, 0.1, 0.01]
    Rab, tab = RC.relative_pose(cam, 0, 1)
    R0 = cam[1, :9].reshape(3, 3) if theta == 0 else (PC.rodrigues(_unit(rng) * theta).T @ Rab).astype(np.float64)
    t0 = (tab + 0.1 * rng.standard_normal(3)).astype(np.float64)
    cs = RC.Constraints([(0, 1)], R0, t0, rng.standard_normal((3, 3)) * 2, rng.standard_normal((3, 3)) * 2)
    return cam, cs


THETAS = [0.0, 1e-9, 1e-3, 2.0] + [None] * 16


def test_analytic_jacobian_matches_central_differences():
    rng = np.random.default_rng(14)
    h = LD(1e-6)
    worst = 0.0
    for k, theta in enumerate(THETAS):
        th = rng.uniform(0.01, 2.8) if theta is None else theta
        cam, cs = _pose_pair(rng, th)
        _, _, ph = RC.residuals(cs, cam)
        got_th = float(np.sqrt((ph[0] * ph[0]).sum()))
        assert (got_th == 0.0) if th == 0 else abs(got_th - th) <= 1e-12 + 1e-6 * th, (k, th, got_th)
        J = RC.jacobians(cs, cam)[0]
        fd = np.zeros((6, 12), LD)
        for col in range(12):
            dx = np.zeros(18, LD)
            dx[9 * (col // 6) + col % 6] = h
            ep, em = [np.concatenate(RC.residuals(cs, PC.retract(cam, np.zeros((0, 3)), s * dx)[0])[:2], axis=1)[0] for s in (1, -1)]
            fd[:, col] = (ep - em) / (2 * h)
        err = relmax(fd, J)
        worst = max(worst, err)
        print("RELPOSE fd[%d] theta %.3e rel_error %.3e 1.0e-07" % (k, th, err))
        assert err <= 1e-7, (k, th, err)
    assert worst > 0


def test_residuals_are_invariant_under_a_world_motion():
    rng = np.random.default_rng(15)
    for k in range(10):
        cam, cs = _pose_pair(rng, rng.uniform(0.01, 2.5))
        cam = np.array(cam, LD)  # rotations orthogonal to long-double roundoff (doubles are rotations only to 1e-16, and so is the invariance)
        for a in range(2):
            cam[a, :9] = PC.rodrigues(_unit(rng) * rng.uniform(0.3, 2.5)).reshape(-1)
        et, er, _ = RC.residuals(cs, cam)
        Q, c = PC.rodrigues(_unit(rng) * rng.uniform(0.1, 3.0)), rng.standard_normal(3).astype(LD) * 5
        moved = np.array(cam, LD)
        for a in range(2):
            R = np.asarray(cam[a, :9], LD).reshape(3, 3)
            moved[a, :9] = (R @ Q).reshape(-1)
            moved[a, 9:12] = np.asarray(cam[a, 9:12], LD) + R @ c
        et2, er2, _ = RC.residuals(cs, moved)
        for name, x, y in (("e_t", et2, et), ("e_r", er2, er)):
            err = relmax(x, y)
            print("RELPOSE invariance[%d] %s %.3e 1.0e-15" % (k, name, err))
            assert err <= 1e-15, (k, name, err)


@pytest.mark.parametrize("masked", [False, True], ids=["free", "masked"])
def test_direct_is_the_dense_normal_equations(masked):
    rng = np.random.default_rng(16)
    N = 6
    cam = np.zeros((N, 15))
    for a in range(N):
        cam[a, :9] = PC.rodrigues(_unit(rng) * rng.uniform(0.3, 2.0)).astype(np.float64).reshape(-1)
        cam[a, 9:12] = rng.standard_normal(3) * 2
    pairs = [(0, 1), (1, 2), (2, 3), (3, 4), (4, 5), (5, 2), (0, 4)]
    n = len(pairs)
    R0, t0 = np.zeros((n, 3, 3)), np.zeros((n, 3))
    for q, (a, b) in enumerate(pairs):
        Rab, tab = RC.relative_pose(cam, a, b)
        R0[q] = (PC.rodrigues(_unit(rng) * 0.2) @ Rab).astype(np.float64)
        t0[q] = (tab + 0.05 * rng.standard_normal(3)).astype(np.float64)
    cs = RC.Constraints(pairs, R0, t0, rng.standard_normal((n, 3, 3)), rng.standard_normal((n, 3, 3)))
    cm = np.array([0x03F, 0, 0x007, 0, 0x1C0, 0], np.uint16) if masked else None
    d = RC.direct(cs, N, cam, cm)
    J, e = RC.stacked(cs, N, cam, cm)
    H = J.T @ J
    assert relmax(d["S"], H) <= 1e-17
    assert relmax(d["g"], -J.T @ e) <= 1e-17
    assert abs(d["energy"] - (e * e).sum()) <= 1e-17 * d["energy"]
    assert relmax(d["energies"], RC.energies(cs, cam)) <= 1e-17
    for (a, b), Hab in d["cross"].items():
        assert relmax(Hab, H[9 * a:9 * a + 6, 9 * b:9 * b + 6]) <= 1e-17
    for a in range(N):
        assert relmax(d["V"][a], H[9 * a:9 * a + 9, 9 * a:9 * a + 9]) <= 1e-17 or not H[9 * a:9 * a + 9, 9 * a:9 * a + 9].any()
        assert not d["V"][a, 6:, :].any() and not d["V"][a, :, 6:].any()  # the intrinsics columns are zero
    if masked:
        assert not d["V"][0].any() and not d["g"][:9].any() and not d["V"][2, :3, :].any() and d["V"][2, 3:6, 3:6].any()
        assert d["V"][4, :6, :6].any()  # (only the intrinsics of camera 4 are fixed)
        assert d["energy"] == RC.direct(cs, N, cam)["energy"]
    S, rhs = RC.reduced(np.eye(9 * N), np.ones(9 * N), d)
    assert relmax(S, np.eye(9 * N, dtype=LD) + H) <= 1e-17 and relmax(rhs, 1 - J.T @ e) <= 1e-17


def test_inverse_left_jacobian():
    rng = np.random.default_rng(17)
    for th in (0.0, 1e-9, 1e-3, 0.019, 0.021, 0.5, 2.0, 3.0):
        phi = (_unit(rng) * th).astype(LD)
        err = float(np.abs(RC.jl_inv(phi) @ RC.jl(phi) - np.eye(3)).max())
        print("RELPOSE jl_inv theta %.3e |Jl^-1 Jl - I| %.3e 1.0e-17" % (th, err))
        assert err <= 1e-17, (th, err)
        # Log and Exp are inverse to each other
        if th < 3.0:
            assert float(np.abs(RC.log_so3(PC.rodrigues(phi)) - phi).max()) <= 1e-17 * max(th, 1.0)


def test_standard_constraints_and_the_long_double_lm():
    """A ring of 45 cameras, each point seen by three neighbours: the chain, a hub with 40 ties, pairs without a common point; and the
    yardstick's LM reaches the constraint's target on a two-camera problem of constraint rows alone."""
    rng = np.random.default_rng(18)
    N, M = 45, 200
    cam = np.zeros((N, 15))
    for a in range(N):
        cam[a, :9] = PC.rodrigues(_unit(rng) * 0.3).astype(np.float64).reshape(-1)
        cam[a, 9:12] = rng.standard_normal(3)
    pt = np.repeat(np.arange(M), 3).astype(np.int32)
    ci = ((np.repeat(np.arange(M), 3) % N) + np.tile(np.arange(3), M)).astype(np.int32) % N
    cs, info = RC.standard_constraints(N, ci, pt, cam, np.ones((N, 9)))
    assert info["n"] == N - 1 + 40 == len(cs) and info["n_no_common"] >= 1 and info["max_common"] >= 2
    assert len({frozenset(p) for p in cs.pairs.tolist()}) == len(cs) and (cs.pairs[:, 0] != cs.pairs[:, 1]).all()
    _, _, ph = RC.residuals(cs, cam)
    assert np.allclose(np.sqrt((ph * ph).sum(axis=1)).astype(np.float64), 0.05, rtol=1e-9)
    assert 1e-2 <= 1 / info["sigma_t"] ** 2 <= 1e2 and 1e-2 <= 1 / info["sigma_r"] ** 2 <= 1e2
    two = RC.Constraints([(0, 1)], cs.R0[0], 2 * RC.relative_pose(cam, 0, 1)[1].astype(np.float64), np.eye(3), np.eye(3))

    def fun(x):
        J, e = RC.stacked(two, 2, x)
        return J, e
    x, E = RC.lm_dense(fun, np.array(cam[:2], LD), lambda x, dx: PC.retract(x, np.zeros((0, 3)), dx)[0])
    assert float(E) <= 1e-30, float(E)


def test_standard_constraints_take_the_angle_per_constraint():
    """angle = 0.05 written out is the default in every bit; a list of angles is cycled over the constraints and each one is the
    residual rotation's angle (pi - 1e-3 to 1e-12 relative: Log's eps / (pi - theta) in long double is 5e-17)."""
    rng = np.random.default_rng(19)
    N = 12
    cam = np.zeros((N, 15))
    for a in range(N):
        cam[a, :9] = PC.rodrigues(_unit(rng) * rng.uniform(0.3, 2.5)).astype(np.float64).reshape(-1)
        cam[a, 9:12] = rng.standard_normal(3)
    pt = np.repeat(np.arange(30), 2).astype(np.int32)
    ci = (np.arange(60) % N).astype(np.int32)
    base, _ = RC.standard_constraints(N, ci, pt, cam, np.ones((N, 9)))
    same, _ = RC.standard_constraints(N, ci, pt, cam, np.ones((N, 9)), angle=0.05)
    for k in ("pairs", "R0", "t0", "Lr", "Lt"):
        assert np.array_equal(getattr(base, k), getattr(same, k)), k
    angles = [1e-9, 5e-4, 1e-2, 1.0, 2.5, np.pi - 1e-3]
    wide, _ = RC.standard_constraints(N, ci, pt, cam, np.ones((N, 9)), angle=angles)
    assert np.array_equal(wide.pairs, base.pairs) and np.array_equal(wide.t0, base.t0) and len(wide) > len(angles)
    _, _, ph = RC.residuals(wide, cam)
    th = np.sqrt((ph * ph).sum(axis=1)).astype(np.float64)
    # R0 is rounded to double: an absolute 1e-16 in the rotation, 1e-7 of the angle 1e-9
    assert np.allclose(th, np.resize(angles, len(wide)), rtol=1e-9, atol=1e-15)
    one, _ = RC.standard_constraints(N, ci, pt, cam, np.ones((N, 9)), angle=np.full(len(base), 0.05))
    assert np.array_equal(one.R0, base.R0)


def test_header_binding_and_library_declare_the_constraints(ba):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ba_mi355x.h")).read(), flags=re.S)  # (without the comments)
    dbl = r"const\s+double\s*\*\s*"
    for name, args in (("ba_solver_set_relative_poses",
                        r"int\s+n\s*,\s*const\s+int\s*\*\s*cam_pairs[^,]*,\s*%sR0[^,]*,\s*%st0[^,]*,\s*%ssqrt_info_rot[^,]*,\s*%ssqrt_info_trans[^,)]*"
                        % (dbl, dbl, dbl, dbl)),
                       ("ba_solver_relative_pose_energy", r"double\s*\*\s*out2")):
        assert re.search(r"\bint\s+%s\s*\(\s*ba_solver\s*\*\s*s\s*,\s*%s\s*\)\s*;" % (name, args), hdr), name
        assert name in ba.EXPORTS
        assert hasattr(ba.lib(), name), name
        assert getattr(ba.lib(), name).argtypes is not None, name
    out = subprocess.run(["nm", "-D", "--defined-only", ba.LIB_PATH], capture_output=True, text=True)
    if out.returncode == 0:
        syms = set(line.split()[-1] for line in out.stdout.splitlines() if line.strip())
        assert {"ba_solver_set_relative_poses", "ba_solver_relative_pose_energy"} <= syms
    for m in ("set_relative_poses", "relative_pose_energy"):
        assert hasattr(ba.Solver, m), m
    # the host-only helper against the yardstick
    rng = np.random.default_rng(19)
    cam, _ = _pose_pair(rng, 0.3)
    R, t = ba.relative_pose(cam, 0, 1)
    Ry, ty = RC.relative_pose(cam, 0, 1)
    assert relmax(R, Ry) <= 1e-15 and relmax(t, ty) <= 1e-15
