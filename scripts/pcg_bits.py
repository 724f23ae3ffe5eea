#!/usr/bin/env python3
"""The bits of BA_ITERSCHUR's PCG and of the covariance routes, for comparing two builds of the library on one GPU.

    python scripts/pcg_bits.py DIR      (DIR: the directory to import bundleadjustment_benchmarks_amd from; this tree's data/ is read)

Prints one line per item, `name sha256-of-the-raw-bytes`; two builds compute the same when their outputs are equal line for line.

Inputs: data/problem-21-11315-pre.txt (every camera has more than 16 chunks: the 16-wide loops of the chunk sums run) and
Problem.synthetic(300, 3000, 15000, 19) (the camera kernels run past one workgroup, at 256 and at 28 cameras per workgroup).
Per input and scalar type, ITERSCHUR under five setups -- block Jacobi; the constraint forest over a chain of relative poses; the
visibility forest; a constant mask; shared intrinsics -- each hashed behind try_step at two lambda (GET_RHS, GET_DX, GET_CAMS_TEST,
GET_POINTS_TEST, pcg_stats) and over the trial rows of a five-trial minimize.  In fp64 also covariance_pcg for two camera pairs and
four points (two point batches), plain and under the mask, and the dense covariance under CHOLESKY for the same request.  Every
solver's device_bytes closes its lines, as a number.
"""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAMS = (1e-4, 1e-8)  # relative to max diag J'J


def line(name, *arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    print("%s %s" % (name, h.hexdigest()), flush=True)


def chain(ba, s, N):
    """relative poses along the chain 0 - 1 - ... - N-1: the pose at the start, the translation off by a fixed amount"""
    cams = s.get(ba.GET_CAMS)
    pairs = np.stack([np.arange(N - 1), np.arange(1, N)], axis=1).astype(np.int32)
    R0, t0 = zip(*(ba.relative_pose(cams, a, b) for a, b in pairs))
    u, _, vt = np.linalg.svd(np.array(R0))  # (an fp32 solver's state is orthonormal to fp32 only: the library wants 1e-6)
    s.set_relative_poses(pairs, u @ vt, np.array(t0) + 1e-3, sigma_rot=0.01, sigma_trans=0.1)


def mask(ba, p):
    """camera 0's pose and every seventh camera's intrinsics fixed, every fifth point fixed"""
    cm = np.zeros(p.N, np.uint16)
    cm |= p.gauge_mask(0)
    cm[3::7] |= np.uint16(ba.FIX_INTRINSICS)
    return cm, (np.arange(p.M) % 5 == 2)


def shared(ba, s, p):
    """groups of four cameras with one f, k1, k2 (the members' values made equal first)"""
    cams = s.get(ba.GET_CAMS).reshape(p.N, 15).copy()
    g = np.arange(p.N) // 4
    cams[:, 12:15] = cams[4 * g, 12:15]
    s.set_state(cams, None)
    s.set_shared_intrinsics(g.astype(np.int32))


SETUPS = {
    "jacobi": lambda ba, s, p: None,
    "constraint_forest": lambda ba, s, p: (chain(ba, s, p.N), s.set_preconditioner(ba.PRECOND_CONSTRAINT_FOREST, 64)),
    "visibility_forest": lambda ba, s, p: s.set_preconditioner(ba.PRECOND_VISIBILITY_FOREST),
    "mask": lambda ba, s, p: s.set_constant(*mask(ba, p)),
    "shared": shared,
}


def trials(ba, tag, p, scalar):
    for name, setup in SETUPS.items():
        s = ba.Solver(p, ba.ITERSCHUR, scalar)
        setup(ba, s, p)
        _, dmax = s.linearize()
        for lam in LAMS:
            s.try_step(lam * dmax)
            st = s.pcg_stats()
            for what in ("GET_RHS", "GET_DX", "GET_CAMS_TEST", "GET_POINTS_TEST"):
                line("%s %s lam=%g %s" % (tag, name, lam, what), s.get(getattr(ba, what)))
            line("%s %s lam=%g pcg_stats" % (tag, name, lam),
                 np.array([st["solves"], st["total_iters"], st["last_iters"], st["last_converged"]], np.int64), np.float64(st["last_rel_residual"]))
        line("%s %s minimize rows" % (tag, name), s.minimize(max_trials=5)["trace"][:, :5])  # (the last column is a wall-clock time)
        print("%s %s device_bytes %d" % (tag, name, s.device_bytes()), flush=True)


def covariances(ba, tag, p):
    pairs = np.array([[1, 1], [2, p.N - 1]], np.int32)
    pts = np.array([0, 1, p.M // 2, p.M - 1], np.int32)
    for name, masked in (("plain", False), ("mask", True)):
        s = ba.Solver(p, ba.ITERSCHUR, ba.F64)
        if masked:
            s.set_constant(*mask(ba, p))
        _, dmax = s.linearize()
        cc, pc, st = s.covariance_pcg(1e-4 * dmax, cam_pairs=pairs, points=pts)
        line("%s covariance_pcg %s cameras" % (tag, name), cc)
        line("%s covariance_pcg %s points" % (tag, name), pc)
        line("%s covariance_pcg %s stats" % (tag, name), np.array([st[k] for k in ("columns", "batches", "total_iters", "max_iters", "unconverged")], np.int64),
             np.float64(st["worst_rel_residual"]))
        print("%s covariance_pcg %s device_bytes %d" % (tag, name, s.device_bytes()), flush=True)
        d = ba.Solver(p, ba.CHOLESKY, ba.F64)
        if masked:
            d.set_constant(*mask(ba, p))
        _, dmax = d.linearize()
        cc, pc = d.covariance(1e-4 * dmax, cam_pairs=pairs, points=pts)
        line("%s covariance dense %s cameras" % (tag, name), cc)
        line("%s covariance dense %s points" % (tag, name), pc)
        print("%s covariance dense %s device_bytes %d" % (tag, name, d.device_bytes()), flush=True)


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    sys.path.insert(0, os.path.abspath(sys.argv[1]))
    import bundleadjustment_benchmarks_amd as ba
    problems = (("p21", ba.Problem.load_bal(os.path.join(ROOT, "data", "problem-21-11315-pre.txt"))), ("syn300", ba.Problem.synthetic(300, 3000, 15000, 19)))
    for tag, p in problems:
        for scalar, sn in ((ba.F64, "f64"), (ba.F32, "f32")):
            trials(ba, "%s %s" % (tag, sn), p, scalar)
        covariances(ba, tag, p)


if __name__ == "__main__":
    main()
