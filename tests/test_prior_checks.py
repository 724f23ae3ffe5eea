"""CPU: the yardstick of the Gaussian priors (tests/prior_checks.py) pinned on its own, the contract's declarations and the register
report of the prior kernel (hipcc cross-compiles gfx950).  No GPU needed.

Bounds, from the number formats.  Everything is long double (2^-64 = 5.4e-20); entries are O(1) .. O(1e3).
  * finite differences: central differences at steps h and h / 2, Richardson-combined, leave an O(h^4) term of the third-order
    derivatives: h = 1e-3 on parameters of size O(1) gives 1e-12 of the block's largest entry, and the subtraction of two long-double
    values of e costs 2^-64 |e| / h = 1e-16.  Bound: 1e-9 of the largest entry of the prior's Jacobian (three digits over the O(h^4) term);
  * sum e^2 against the energy, and the pseudo-observation form against the direct form: the same products summed in another order,
    a few hundred terms: 1e-17 relative to the largest entry."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import prior_checks as PC
from conftest import ROOT

LD = np.longdouble


def relmax(a, b):
    return float(np.abs(np.asarray(a, LD) - np.asarray(b, LD)).max() / max(np.abs(np.asarray(b, LD)).max(), LD(1e-300)))


@pytest.fixture(scope="module")
def scene():
    """5 cameras with rotations of 0.3 .. 2 rad, 12 points; priors of every type with full (not triangular, not symmetric) L."""
    rng = np.random.default_rng(11)
    N, M = 5, 12
    cam = np.zeros((N, 15), LD)
    for a in range(N):
        w = rng.standard_normal(3)
        cam[a, :9] = PC.rodrigues(w / np.linalg.norm(w) * rng.uniform(0.3, 2.0)).reshape(-1)
        cam[a, 9:12] = rng.standard_normal(3) * 2
        cam[a, 12:15] = [-500 + 30 * rng.standard_normal(), 0.1 * rng.standard_normal(), 0.01 * rng.standard_normal()]
    pts = rng.standard_normal((M, 3)).astype(LD) * 3
    pr = PC.Priors([1, 4, 7, 11], rng.standard_normal((4, 3)), rng.standard_normal((4, 3, 3)) * 2,
                   [0, 2, 3, 4], rng.standard_normal((4, 3)), rng.standard_normal((4, 3, 3)) * 3,
                   [0, 1, 4], rng.standard_normal((3, 3)), np.array([[2.0, 0.5, 0.0], [0.0, 3.0, 1.0], [1.5, 0.0, 0.0]]))
    return N, M, cam, pts, pr


def _fd(pr, cam, pts, N, M, col, h):
    def e_at(step):
        dx = np.zeros(3 * M + 9 * N, LD)
        dx[col] = step
        c, x = PC.retract(cam, pts, dx)
        return PC.rows(pr, c, x)
    d1 = [(p - m) / (2 * h) for p, m in zip(e_at(h), e_at(-h))]
    d2 = [(p - m) / h for p, m in zip(e_at(h / 2), e_at(-h / 2))]
    return [(4 * b - a) / 3 for a, b in zip(d1, d2)]


def test_every_prior_jacobian_is_the_finite_difference_of_its_rows(scene):
    """Column by column of [3M points | 9N cameras] through the documented retraction (T + dT, R <- Rodrigues(d omega) R, additive f,
    k1, k2 and points), restated in prior_checks.retract.  The centre prior's sign and side (-R' [T]x) are decided here."""
    N, M, cam, pts, pr = scene
    Jp, Jc, Ji = PC.jacobians(pr, cam)
    Fp, Fc, Fi = np.zeros_like(Jp), np.zeros_like(Jc), np.zeros_like(Ji)
    h = LD(1e-3)
    for n, j in enumerate(pr.pt_ids):
        for q in range(3):
            Fp[n, :, q] = _fd(pr, cam, pts, N, M, 3 * j + q, h)[0][n]
    for ids, F, which in ((pr.c_ids, Fc, 1), (pr.i_ids, Fi, 2)):
        for n, a in enumerate(ids):
            for q in range(9):
                F[n, :, q] = _fd(pr, cam, pts, N, M, 3 * M + 9 * a + q, h)[which][n]
    for name, J, F in (("point", Jp, Fp), ("centre", Jc, Fc), ("intrinsics", Ji, Fi)):
        err = relmax(F, J)
        print("PRIOR fd %s %.3e 1.0e-09" % (name, err))
        assert err <= 1e-9, name
    assert np.abs(Jc[:, :, 3:6]).max() > 0.1  # (the omega columns are there to be tested)
    # a column of another block does not move a prior's rows
    other = _fd(pr, cam, pts, N, M, 3 * 0 + 1, h)  # point 0 carries no prior
    assert all(not np.asarray(o).any() for o in other)


def test_sum_of_squares_is_the_energy(scene):
    N, M, cam, pts, pr = scene
    d = PC.direct(pr, N, M, cam, pts)
    tot = sum((e * e).sum() for e in PC.rows(pr, cam, pts))
    assert abs(d["energy"] - tot) <= 1e-17 * tot and d["energy"] > 0
    assert relmax(d["energies"], PC.energies(pr, cam, pts)) <= 1e-17
    # g = -J'e: the gradient of energy / 2, by the finite difference of the energy
    h = LD(1e-3)
    for col in (3 * 4 + 1, 3 * M + 9 * 2 + 4, 3 * M + 9 * 4 + 6):
        def en(step):
            dx = np.zeros(3 * M + 9 * N, LD)
            dx[col] = step
            return PC.energies(pr, *PC.retract(cam, pts, dx)).sum()
        fd = (4 * (en(h / 2) - en(-h / 2)) / h - (en(h) - en(-h)) / (2 * h)) / 3
        assert abs(-d["g"][col] - fd / 2) <= 1e-9 * abs(fd), col


@pytest.mark.parametrize("masked", [False, True], ids=["free", "masked"])
def test_pseudo_observations_are_the_direct_form(scene, masked):
    """A few observations with random blocks + the priors: U, V, g and the energy of the augmented problem are the observations' own
    plus prior_checks.direct; under a mask the fixed columns are zero in both forms."""
    N, M, cam, pts, pr = scene
    rng = np.random.default_rng(3)
    K = 40
    ci, pi = rng.integers(0, N, K).astype(np.int32), np.sort(rng.integers(0, M, K)).astype(np.int32)
    Jc, Jp, e = rng.standard_normal((K, 2, 9)).astype(LD), rng.standard_normal((K, 2, 3)).astype(LD), rng.standard_normal((K, 2)).astype(LD)
    cm = pf = None
    if masked:
        cm = np.array([0x03F, 0, 0x1C0, 0x004, 0], np.uint16)
        pf = np.zeros(M, np.uint8)
        pf[[4, 5]] = 1
        free = ((cm.astype(np.uint32)[:, None] >> np.arange(9)[None, :]) & 1) == 0
        Jc = Jc * free[ci][:, None, :]
        Jp = Jp * (pf[pi] == 0)[:, None, None]
    U0, V0, g0, e0 = PC.normal_blocks(N, M, ci, pi, Jc, Jp, e)
    d = PC.direct(pr, N, M, cam, pts, cm, pf)
    ca, pa, JC, JP, E = PC.augment(pr, ci, pi, Jc, Jp, e, cam, pts, cm, pf)
    assert len(ca) == K + 2 * (len(pr.pt_ids) + len(pr.c_ids) + len(pr.i_ids)) and np.all(np.diff(pa) >= 0)
    U1, V1, g1, e1 = PC.normal_blocks(N, M, ca, pa, JC, JP, E)
    for name, got, ref in (("U", U1, U0 + d["U"]), ("V", V1, V0 + d["V"]), ("g", g1, g0 + d["g"])):
        assert relmax(got, ref) <= 1e-17, name
    assert abs(e1 - (e0 + d["energy"])) <= 1e-17 * e1
    if masked:
        assert not d["U"][4].any() and d["U"][1].any() and not d["V"][0, :6, :].any() and not d["V"][2, 6:, 6:].any()
        assert not d["g"][3 * 4:3 * 4 + 3].any() and not d["g"][3 * M:3 * M + 6].any()
        assert d["energy"] == PC.direct(pr, N, M, cam, pts)["energy"]  # a fixed parameter's prior is a constant in the energy


def test_header_binding_and_library_declare_the_priors(ba):
    hdr = open(os.path.join(ROOT, "include", "ba_mi355x.h")).read()
    for name, args in (("ba_solver_set_point_priors", r"int\s+n\s*,\s*const\s+int\s*\*\s*pt_ids\s*,\s*const\s+double\s*\*\s*x0\s*,\s*const\s+double\s*\*\s*sqrt_info"),
                       ("ba_solver_set_centre_priors", r"int\s+n\s*,\s*const\s+int\s*\*\s*cam_ids\s*,\s*const\s+double\s*\*\s*c0\s*,\s*const\s+double\s*\*\s*sqrt_info"),
                       ("ba_solver_set_intrinsics_priors", r"int\s+n\s*,\s*const\s+int\s*\*\s*cam_ids\s*,\s*const\s+double\s*\*\s*x0\s*,\s*const\s+double\s*\*\s*w"),
                       ("ba_solver_prior_energy", r"double\s*\*\s*out3")):
        assert re.search(r"\bint\s+%s\s*\(\s*ba_solver\s*\*\s*s\s*,\s*%s\s*\)\s*;" % (name, args), hdr), name
        assert name in ba.EXPORTS
        assert hasattr(ba.lib(), name), name
        assert getattr(ba.lib(), name).argtypes is not None, name
    out = subprocess.run(["nm", "-D", "--defined-only", ba.LIB_PATH], capture_output=True, text=True)
    if out.returncode == 0:
        syms = set(line.split()[-1] for line in out.stdout.splitlines() if line.strip())
        assert {"ba_solver_set_point_priors", "ba_solver_set_centre_priors", "ba_solver_set_intrinsics_priors", "ba_solver_prior_energy"} <= syms
    for m in ("set_point_priors", "set_centre_priors", "set_intrinsics_priors", "prior_energy"):
        assert hasattr(ba.Solver, m), m


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not available")
def test_prior_kernel_uses_no_scratch(tmp_path):
    """tests/prior_resources.hip instantiates launch_prior's three instantiations of k_prior and the two of k_prior_lonely per scalar type, compiled with
    csrc/Makefile's own flags: no spills, no scratch."""
    import qr_harness as QH
    hipcc, flags = QH.makefile_flags()
    out = subprocess.run([hipcc] + flags + ["-w", "-I", QH.CSRC, "--cuda-device-only", "-c", os.path.join(ROOT, "tests", "prior_resources.hip"), "-o",
                          str(tmp_path / "prior.o"), "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    usage = {}
    for m in re.finditer(r"Function Name: (\S+)", out.stderr):
        block = out.stderr[m.end():m.end() + 2500]
        get = lambda pat: int(re.search(pat, block).group(1))  # noqa: E731
        usage[m.group(1)] = dict(vgpr=get(r"VGPRs: (\d+)"), occ=get(r"Occupancy \[waves/SIMD\]: (\d+)"), spill=get(r"VGPRs Spill: (\d+)"),
                                 sspill=get(r"SGPRs Spill: (\d+)"), scratch=get(r"ScratchSize \[bytes/lane\]: (\d+)"))
    pr = {k: v for k, v in usage.items() if k.startswith("_Z7k_priorI") or k.startswith("_Z14k_prior_lonelyI")}
    for k, v in sorted(pr.items()):
        print("PRIOR resources %s %s" % (k, v))
    assert len(pr) == 10, sorted(usage)
    for k, v in pr.items():
        assert v["spill"] == 0 and v["sspill"] == 0 and v["scratch"] == 0, (k, v)
