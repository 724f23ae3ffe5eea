"""Measurements of the covariance blocks (ba_solver_covariance_compute / _get; profiles/r07_covariance_measure.*).
Not asserted.

    python scripts/covariance_measure.py [--reps 7] [--out FILE.json] [--skip-cfg5]

At config 4's stand-in (synthetic(257, 65132, 225911, 1004), D = 2313), config 5's (synthetic(1024, 500000, 4000000, 1005), D = 9216)
and problem-39, CHOLESKY fp64, lambda = 1e-6 max diag J'J, median of --reps: device ms of compute split into assembly / factorisation /
inverse (HIP events, ba_solver_covariance_timing), the inverse's TFLOP/s from 2 D^3 / 3 against the 78.6 TF fp64 peak, beside
ba_solver_time_phase(6) (the LM trial's fused factorisation of S alone) of the same build; wall ms of get for all camera diagonal blocks
and (problem-39) for all points, with the device ms of the point kernel for all points and for the point of the longest track alone.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bundleadjustment_benchmarks_amd as ba  # noqa: E402


def measure(name, p, reps, all_points):
    s = ba.Solver(p, ba.CHOLESKY, ba.F64)
    _, dmax = s.linearize()
    lam = 1e-6 * dmax
    b0 = s.device_bytes()
    s.covariance(lam, cams=[0])  # (warm-up: code objects, the buffer)
    ms, get_c, get_p, dev_p, dev_long = [], [], [], [], []
    track = np.bincount(p.arrays()["pt_idx"], minlength=p.M)
    longest = int(np.argmax(track))
    for _ in range(reps):
        s.covariance(lam)
        ms.append(s.covariance_timing())
        t0 = time.time()
        s.covariance(cams=np.arange(p.N), compute=False)
        get_c.append(1e3 * (time.time() - t0))
        if all_points:
            t0 = time.time()
            s.covariance(points=np.arange(p.M), compute=False)
            get_p.append(1e3 * (time.time() - t0))
            dev_p.append(s.covariance_timing()[3])
            s.covariance(points=[longest], compute=False)
            dev_long.append(s.covariance_timing()[3])
    asm, fac, inv = [float(np.median([m[q] for m in ms])) for q in range(3)]
    D = p.D
    out = dict(N=p.N, M=p.M, K=p.K, D=D, lam=lam, assembly_ms=asm, factor_ms=fac, inverse_ms=inv,
               inverse_tflops=2 * D ** 3 / 3 / (inv * 1e-3) / 1e12, trial_factor_ms=s.time_phase(6, 5, lam),
               get_cam_diag_ms=float(np.median(get_c)), get_all_points_ms=float(np.median(get_p)) if get_p else None,
               buffer_bytes=s.device_bytes() - b0, points_kernel_ms=float(np.median(dev_p)) if dev_p else None,
               longest_track=int(track[longest]), longest_track_point_kernel_ms=float(np.median(dev_long)) if dev_long else None)
    print("%s D=%d: compute %.3f ms = assembly %.3f + factor %.3f + inverse %.3f (%.2f TF, %.1f %% of 78.6); trial's own factor %.3f ms; "
          "get: camera diagonals %.3f ms%s; buffer %.1f MB"
          % (name, D, asm + fac + inv, asm, fac, inv, out["inverse_tflops"], 100 * out["inverse_tflops"] / 78.6, out["trial_factor_ms"],
             out["get_cam_diag_ms"], "" if not get_p else ", all %d points %.3f ms wall (point kernel %.4f ms; the point of the longest track, %d observations, alone %.4f ms)"
             % (p.M, out["get_all_points_ms"], out["points_kernel_ms"], out["longest_track"], out["longest_track_point_kernel_ms"]),
             out["buffer_bytes"] / 1e6), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip-cfg5", action="store_true")
    a = ap.parse_args()
    out = {"device": ba.device_info()[0]}
    out["problem39"] = measure("problem-39", ba.Problem.load_bal(os.path.join(ROOT, "data", "problem-39-18060-pre.txt")), a.reps, True)
    out["cfg4"] = measure("cfg4", ba.Problem.synthetic(257, 65132, 225911, 1004), a.reps, False)
    if not a.skip_cfg5:
        out["cfg5"] = measure("cfg5", ba.Problem.synthetic(1024, 500000, 4000000, 1005), a.reps, False)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1, default=float)


if __name__ == "__main__":
    main()
