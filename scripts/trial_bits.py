#!/usr/bin/env python3
"""The bits of one LM trial and of a linearisation under every option of the direct kinds, for comparing two builds of the library
on one GPU (scripts/pcg_bits.py does the same for BA_ITERSCHUR's PCG and the covariance routes).

    python scripts/trial_bits.py DIR      (DIR: the directory to import bundleadjustment_benchmarks_amd from; this tree's data/ is read)

Prints one line per item, `name sha256-of-the-raw-bytes`; two builds compute the same when their outputs are equal line for line.

Input: data/problem-21-11315-pre.txt in fp64 and fp32, one process, one solver at a time.  Behind an accepted step of ba_minimize fp32
runs the fused linearisation that leaves its records by the owners' stores (k_eval's FUSE = 2) there, fp64 the one that stores a
wavefront's run at a time (FUSE = 3).  The cases with priors run on that problem without the observations of points 7 and 8, which
both get a prior (k_prior_lonely; the mask fixes point 7).

Per case (CASES: the fewest that reach every branch of the solver's launch statements):
  linearize              energy, max diag J'J, the prior and constraint energies where there are any
  try_step               at the two lambda of pcg_bits.LAMS (x max diag J'J; under Marquardt's damping lambda itself): the three returned
                         scalars, GET_DX, GET_CAMS_TEST, GET_POINTS_TEST
  time_phase(1), (8)     one linearisation by the separate launches, one by the fused pass: GET_RESIDUALS, GET_JC, GET_JP, GET_GRAD
  minimize(max_trials=5) the trial rows, the result and the final state (the graph path: fused linearisation, x = xTest on k_eval)
  device_bytes           at the end, as a number
The plain CHOLESKY case also: dogleg_prepare at LAMS[1] x max diag J'J (its scalars), try_dogleg at half and at twice the Gauss-Newton
norm (the scalars and GET_DX) behind the try_steps, and at the end triangulate_points on all points (status bytes, the stats without
the time, GET_POINTS).  "priors+relpose" has both optional terms in the partial buffers; "priors_resize" sets the priors, then a point
list of another block count (k_prior has one workgroup per 256 priors), then none at all, with a linearisation behind each, and goes
on as the plain case.
"""
import os
import sys

import numpy as np

from pcg_bits import LAMS, chain, line, mask

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LONELY = (7, 8)

# (solver kind, options, environment of the solver's creation)
CASES = (
    ("CHOLESKY", (), {}),
    ("CHOLESKY", ("mask",), {}),
    ("CHOLESKY", ("model",), {}),
    ("CHOLESKY", ("mask", "model"), {}),
    ("CHOLESKY", ("marq",), {}),
    ("CHOLESKY", ("marq", "mask"), {}),
    ("CHOLESKY", ("priors",), {}),
    ("CHOLESKY", ("priors", "marq", "mask"), {}),
    ("CHOLESKY", ("relpose",), {}),
    ("CHOLESKY", ("relpose", "mask"), {}),
    ("CHOLESKY", ("priors", "relpose"), {}),
    ("CHOLESKY", ("priors_resize",), {}),
    ("CHOLESKY", ("marq",), {"BA_NO_FOLD": "1"}),  # the only route to the stand-alone k_post_reduce<T, true>
    ("ITERSCHUR", ("marq",), {}),
    ("ITERSCHUR", ("marq", "mask"), {}),
    ("ITERSCHUR", ("model",), {}),
    ("QRCHOL", (), {}),
    ("QRCHOL", ("mask",), {}),
    ("QRCHOL", ("model",), {}),
    ("QRCHOL", ("mask", "model"), {}),
    ("MOREQR", ("mask",), {}),
)


def without_observations(ba, p, points):
    """the problem without the observations of `points` (as tests/test_gpu_priors.py builds its unobserved points)"""
    a = p.arrays()
    keep = ~np.isin(a["pt_idx"], points)
    return ba.Problem.from_arrays(p.N, p.M, int(keep.sum()), a["cam_idx"][keep], a["pt_idx"][keep], a["meas"].reshape(-1, 2)[keep].ravel(),
                                  a["cams9"], a["pts"])


def priors(ba, s, p):
    """point priors (the two unobserved points among them), centre priors on every third camera, intrinsics priors on every second:
    each a fixed offset away from the start state"""
    cams, pts = s.get(ba.GET_CAMS).reshape(p.N, 15), s.get(ba.GET_POINTS).reshape(p.M, 3)
    ids = np.array([3, *LONELY, 100, 5000, p.M - 1], np.int32)
    s.set_point_priors(ids, pts[ids] + 0.01, sigma=0.1)
    cids = np.arange(0, p.N, 3, dtype=np.int32)
    R, T = cams[cids, :9].reshape(-1, 3, 3), cams[cids, 9:12]
    s.set_centre_priors(cids, -np.einsum("nji,nj->ni", R, T) + 0.02, sigma=0.5)
    iids = np.arange(1, p.N, 2, dtype=np.int32)
    s.set_intrinsics_priors(iids, cams[iids, 12:15] * 1.001, sigma=np.abs(cams[iids, 12:15]) * 0.01 + 1e-9)


def priors_resize(ba, s, p, tag):
    none = np.zeros(0, np.int32)
    priors(ba, s, p)
    for name, ids in (("set", None), ("700 points", np.arange(0, 2100, 3, dtype=np.int32)), ("no points", none), ("none", none)):
        if ids is not None:
            s.set_point_priors(ids, s.get(ba.GET_POINTS).reshape(p.M, 3)[ids] + 0.01, sigma=0.1)
        if name == "none":
            s.set_centre_priors(none, np.zeros((0, 3)), sigma=1.0)
            s.set_intrinsics_priors(none, np.zeros((0, 3)), sigma=1.0)
        line("%s priors %s linearize" % (tag, name), np.float64(s.linearize()), s.prior_energy())
        print("%s priors %s device_bytes %d" % (tag, name, s.device_bytes()), flush=True)


def dogleg(ba, s, tag, mu):
    info = s.dogleg_prepare(mu)
    line("%s dogleg_prepare" % tag, np.float64([info[k] for k in ("mu", "g2", "q", "gn2", "g_dot_gn", "alpha", "energy_gn", "rho_scale_gn")]))
    for f in (0.5, 2.0):  # inside the Gauss-Newton norm (the interpolated or the gradient step), outside it (the Gauss-Newton step)
        e, pred, dxn, branch = s.try_dogleg(f * np.sqrt(info["gn2"]))
        line("%s try_dogleg %g |gn|" % (tag, f), np.float64([e, pred, dxn]), np.int64(branch))
        line("%s try_dogleg %g |gn| GET_DX" % (tag, f), s.get(ba.GET_DX))


def setup(ba, s, p, opts):
    if "model" in opts:  # Huber away from the default scale, weights that are exact in fp32
        s.set_loss(ba.LOSS_HUBER, 1.0)
        s.set_obs_weights(0.5 + (np.arange(p.K) % 7) / 8.0)
    if "priors" in opts:
        priors(ba, s, p)
    if "relpose" in opts:
        chain(ba, s, p.N)
    if "mask" in opts:
        s.set_constant(*mask(ba, p))
    if "marq" in opts:
        s.set_damping(ba.DAMP_MARQUARDT)


def case(ba, tag, p, kind, opts, env):
    os.environ.update(env)
    try:
        s = ba.Solver(p, getattr(ba, kind), ba.F64 if tag.endswith("f64") else ba.F32)
    finally:
        for k in env:
            del os.environ[k]
    tag = " ".join([tag, kind, "+".join(opts) or "plain"] + ["%s=%s" % kv for kv in env.items()])
    plain = kind == "CHOLESKY" and not opts and not env
    if "priors_resize" in opts:
        priors_resize(ba, s, p, tag)
    setup(ba, s, p, opts)
    e, dmax = s.linearize()
    line("%s linearize" % tag, np.float64([e, dmax]))
    if "priors" in opts:
        line("%s prior_energy" % tag, s.prior_energy())
    if "relpose" in opts:
        line("%s relative_pose_energy" % tag, s.relative_pose_energy())
    scale = 1.0 if "marq" in opts else dmax
    for lam in LAMS:
        line("%s lam=%g try_step" % (tag, lam), np.float64(s.try_step(lam * scale)))
        for what in ("GET_DX", "GET_CAMS_TEST", "GET_POINTS_TEST"):
            line("%s lam=%g %s" % (tag, lam, what), s.get(getattr(ba, what)))
    if plain:
        dogleg(ba, s, tag, LAMS[1] * dmax)
    for phase in (1, 8):
        s.time_phase(phase, 1, LAMS[0] * scale)
        for what in ("GET_RESIDUALS", "GET_JC", "GET_JP", "GET_GRAD"):
            line("%s time_phase(%d) %s" % (tag, phase, what), s.get(getattr(ba, what)))
    r = s.minimize(max_trials=5)
    line("%s minimize rows" % tag, r["trace"][:, :5])  # (the last column is a wall-clock time)
    line("%s minimize result" % tag, np.int64([r["status"], r["iterations"], r["trials"], r["fun_evals"]]), np.float64([r["energy"], r["lam"]]))
    line("%s minimize state" % tag, s.get(ba.GET_CAMS), s.get(ba.GET_POINTS))
    if plain:
        ts, status = s.triangulate_points()
        line("%s triangulate_points" % tag, status, np.int64(ts["asked"]), ts["by_status"], np.float64([ts["cost_before"], ts["cost_after"]]))
        line("%s triangulate_points GET_POINTS" % tag, s.get(ba.GET_POINTS))
    print("%s device_bytes %d" % (tag, s.device_bytes()), flush=True)


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    sys.path.insert(0, os.path.abspath(sys.argv[1]))
    import bundleadjustment_benchmarks_amd as ba
    p = ba.Problem.load_bal(os.path.join(ROOT, "data", "problem-21-11315-pre.txt"))
    lonely = without_observations(ba, p, LONELY)
    for sn in ("f64", "f32"):
        for kind, opts, env in CASES:
            case(ba, "p21 " + sn, lonely if "priors" in opts else p, kind, opts, env)


if __name__ == "__main__":
    main()
