"""The rotation-energy partials of tests/test_gpu_relpose_kernels.py's angle sweep in numpy fp64 in k_relpose's own order of operations
(R_ab and E as (x + y) + z, no fma, the workgroup's reduction tree), beside relpose_checks evaluated plainly in fp64: per angle the
relative error of the partial against the long-double sum (`sum`), of the worst single constraint (`worst term`), and the root sum of
squares of the term errors over the sum (`rss`: the standard deviation of the partial's error if the term errors had random signs).
No GPU needed.  An MI355X gives the `kernel order` sums of the groups that take the series of theta / sin(theta) digit for digit
(profiles/r15_relpose_kernels.txt); where theta / s is formed, atan2 of the device's library may differ in the last place.

    python scripts/relpose_kernel_order.py"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import test_gpu_relpose_kernels as T  # noqa: E402

LD = np.longdouble


def block_sum(v):
    """block_reduce<double, false> of one workgroup of 256 threads: a shuffle tree inside each wave, then the waves in index order."""
    v = np.concatenate([v, np.zeros(256 - len(v))]).reshape(4, 64)
    for off in (32, 16, 8, 4, 2, 1):
        w = v.copy()
        w[:, :64 - off] = v[:, :64 - off] + v[:, off:]
        v = w
    return ((v[0, 0] + v[1, 0]) + v[2, 0]) + v[3, 0]


def main():
    cam15, cs, groups = T._sweep_inputs()
    ref, y64 = T.records(cs, cam15, LD), T.records(cs, cam15, np.float64)
    Ra, Rb = cam15[cs.pairs[:, 0], :9], cam15[cs.pairs[:, 1], :9]
    R0, Lr = cs.R0.reshape(-1, 9), cs.Lr.reshape(-1, 9)
    Rab, E = np.zeros_like(Ra), np.zeros_like(Ra)
    for i in range(3):
        for j in range(3):
            Rab[:, 3 * i + j] = (Rb[:, 3 * i] * Ra[:, 3 * j] + Rb[:, 3 * i + 1] * Ra[:, 3 * j + 1]) + Rb[:, 3 * i + 2] * Ra[:, 3 * j + 2]
    for i in range(3):
        for j in range(3):
            E[:, 3 * i + j] = (Rab[:, 3 * i] * R0[:, 3 * j] + Rab[:, 3 * i + 1] * R0[:, 3 * j + 1]) + Rab[:, 3 * i + 2] * R0[:, 3 * j + 2]
    v0, v1, v2 = 0.5 * (E[:, 7] - E[:, 5]), 0.5 * (E[:, 2] - E[:, 6]), 0.5 * (E[:, 3] - E[:, 1])
    s2 = (v0 * v0 + v1 * v1) + v2 * v2
    s, c = np.sqrt(s2), 0.5 * (((E[:, 0] + E[:, 4]) + E[:, 8]) - 1.0)
    with np.errstate(all="ignore"):
        f = np.where((s < 1e-3) & (c > 0), 1.0 + s2 * (1.0 / 6.0 + s2 * (3.0 / 40.0)), np.arctan2(s, c) / s)
    phi = [f * v0, f * v1, f * v2]
    er = [(Lr[:, 3 * k] * phi[0] + Lr[:, 3 * k + 1] * phi[1]) + Lr[:, 3 * k + 2] * phi[2] for k in range(3)]
    er2 = (er[0] * er[0] + er[1] * er[1]) + er[2] * er[2]
    print("%-8s | %-33s | %-33s" % ("theta", "kernel order: sum, worst term, rss", "relpose_checks fp64: the same"))
    for nm, _, sl in groups:
        r = ref["er2"][sl]
        if not r.sum() > 0:
            continue
        cols = []
        for terms, total in ((er2[sl], block_sum(er2[sl])), (y64["er2"][sl], y64["er2"][sl].sum())):
            d = terms.astype(LD) - r
            cols += [abs(LD(total) - r.sum()) / r.sum(), (np.abs(d)[r > 0] / r[r > 0]).max(), np.sqrt((d * d).sum()) / r.sum()]
        print("%-8s | %.3e  %.3e  %.3e   | %.3e  %.3e  %.3e" % ((nm,) + tuple(float(x) for x in cols)))


if __name__ == "__main__":
    main()
