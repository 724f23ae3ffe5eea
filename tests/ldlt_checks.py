"""The dense LDL^T (ba_dense.hip.h) on its own inputs: reference, yardstick, matrix families and metrics -- TEST INFRASTRUCTURE ONLY
(tests/test_ldlt_checks.py on the CPU, tests/test_gpu_ldlt_kernels.py on the GPU through tests/ldlt_harness.*).

Reference   LDL^T without pivoting, right-looking and unblocked, in numpy.longdouble (64-bit significand) of the matrix in the
            kernels' dtype, with extra rows riding along (the right-hand side, or the covariance form's stacked rows): L, d, Y = L d,
            W = L11^-1 per 64-block, z = D^-1 L^-1 b.  Cached per matrix.
Yardstick   the same unblocked algorithm in the working precision, measured by the same metrics: a bound is
            max(10 x yardstick, floor) (FLOOR below).
Families    spd   Q diag(logspace) Q^T scaled to a unit diagonal;
            sqd   a symmetrically permuted quasi-definite [[H, B], [B^T, -C]]: half the pivots negative, at every sub-panel position;
            exact an integer A = L D L^T whose every intermediate in ANY evaluation order is an integer below 2^24 in magnitude, so
                  fp32 and fp64 must return L, Y, W, z and x bit for bit (exact_problem's docstring says why); also with one d_k = 0.
Metrics     (long double, on what the kernels left: `run`, the dict of ldlt_harness.Harness.run or of emulate())
            eta     stage_checks.eta(A, x, b), the backward error of the solve
            sweep   the back sweep on its own inputs, per block p |x_p - W_p^T (z_p - sum_{q>p} L_qp^T x_q)| over
                    |W_p^T| (|z_p| + sum |L_qp^T| |x_q|), W, L, z from the copies taken behind the factor; bound (ncols + 64) eps
            fwd_L, fwd_Y  the stored entries below the diagonal blocks, per column relative to the reference column's largest entry
                    (Y's right-hand side row, z d, relative to max |z* d*| like fwd_z)
            fwd_W   |W L11* - I| per block over the whole 64 x 64 image (rows past the last pivot must be zero)
            fwd_z   max |z - z*| / max |z*|
            fwd_B   the covariance form's stacked rows, per column like fwd_L
            yld     Y_ij against L_ij d*_j, per column relative to the reference Y column's largest entry
            signs   the number of pivots whose sign differs from the reference's (read off Y / L where the panel's Y is retained
                    and the column has rows below, off z against L*^-1 b otherwise)
What S holds behind the factor: below the diagonal blocks L, in row zrow z; a diagonal block is written back only by a panel step of
one workgroup, so the metrics never read one.
"""
import hashlib

import numpy as np

NB = 64
LD = np.longdouble
EPS = {0: float(np.finfo(np.float64).eps), 1: float(np.finfo(np.float32).eps)}
# Floors under 10 x the yardstick, per metric, dtype and conditioning class of the family ("1e2": spd at condition 1e2 and sqd; "hi":
# spd at 1e8 in fp64 / 1e3 in fp32), from the first MI355X run with at least 10x headroom over the worst value measured where the
# floor is the bound that holds (the worst values beside them, fp64 / fp32; profiles/r18_ldlt_kernels.txt).  Ceilings of the 1e2
# class: 1e-12 / 1e-4.  fwd_L and fwd_Y stand AT that ceiling and not 10x over their worst values (5.2e-13 / 3.5e-4 both):
# an entry's error relative to its column's largest entry grows with the conditioning of the leading submatrix in front of the column
# and with the column's length, the unblocked yardstick itself reaches 2.3e-13 / 1.8e-4 there, and on every such case the bound
# that holds is 10 x the yardstick (the kernels stay below 0.8 of it), not the floor.  The hi class scales the ceilings with the
# condition number (x 1e6 in fp64; the kernels reach 13 x the yardstick there: Y = X W^T with the explicit inverse, 1 / d by Newton
# steps), fp32 fwd_L / fwd_Y by measurement (2.6e-4 at D = 128 where the floor holds).
FLOOR = {
    ("fwd_L", 0, "1e2"): 1e-12, ("fwd_L", 1, "1e2"): 1e-4,    # 5.2e-13 / 3.5e-4 (D = 577; the yardstick's bound holds there: 2.3e-12 / 1.8e-3)
    ("fwd_Y", 0, "1e2"): 1e-12, ("fwd_Y", 1, "1e2"): 1e-4,    # 5.2e-13 / 3.5e-4 (the same)
    ("fwd_W", 0, "1e2"): 3e-14, ("fwd_W", 1, "1e2"): 2e-5,    # 2.5e-15 / 1.2e-6
    ("fwd_z", 0, "1e2"): 1e-13, ("fwd_z", 1, "1e2"): 5e-5,    # 7.9e-15 / 4.3e-6
    ("yld", 0, "1e2"): 1e-13, ("yld", 1, "1e2"): 5e-5,        # 7.7e-15 / 4.2e-6
    ("fwd_L", 0, "hi"): 1e-6, ("fwd_L", 1, "hi"): 3e-3,       # 7.9e-8 / 2.0e-3 (fp32: the yardstick's bound holds there, 3.5e-2)
    ("fwd_Y", 0, "hi"): 1e-6, ("fwd_Y", 1, "hi"): 3e-3,       # 7.9e-8 / 2.1e-3 (the same)
    ("fwd_W", 0, "hi"): 3e-8, ("fwd_W", 1, "hi"): 2e-4,       # 1.9e-9 / 5.5e-6
    ("fwd_z", 0, "hi"): 1e-7, ("fwd_z", 1, "hi"): 5e-4,       # 2.0e-9 / 2.3e-5
    ("yld", 0, "hi"): 1e-7, ("yld", 1, "hi"): 5e-4,           # 8.9e-10 / 1.4e-5
    # the covariance form (fp64), condition 1e2 / 1e8: fwd_B 1.0e-14 / 1.3e-9, the pivots s_k / B_kk 1.0e-14 / 4.1e-10 (D = 700, 130)
    ("fwd_B", 0, "1e2"): 1e-13, ("fwd_B", 0, "hi"): 2e-8, ("pivots", 0, "1e2"): 1e-13, ("pivots", 0, "hi"): 1e-8,
}
FWD = ("fwd_L", "fwd_Y", "fwd_W", "fwd_z", "yld")


def bound(metric, fp32, yard, cls="1e2"):
    return max(10.0 * yard, FLOOR[(metric, int(fp32), cls)])


def sweep_bound(ncols, fp32):
    """the componentwise bound of a dot product of ncols + 64 terms"""
    return (ncols + 64) * EPS[int(fp32)]


def dtype(fp32):
    return np.float32 if fp32 else np.float64


def blocks(n):
    return [(p0, min(NB, n - p0)) for p0 in range(0, n, NB)]


# ---- reference and yardstick ---------------------------------------------------------------------------------------------------------
def unblocked(A, R, dt):
    """Right-looking LDL^T without pivoting in dtype dt of the symmetric A (lower triangle read) with the rows R riding along.
    Returns L (unit lower), d, Z = (D^-1 L^-1 R^T)^T."""
    n = A.shape[0]
    M = np.vstack([np.tril(A), np.atleast_2d(R)]).astype(dt)
    d = np.zeros(n, dt)
    with np.errstate(all="ignore"):  # (a zero pivot: the non-finite values are the result)
        for k in range(n):
            d[k] = M[k, k]
            y = M[k + 1:, k].copy()
            l = y / d[k]
            M[k + 1:, k] = l
            if k + 1 < n:
                M[k + 1:, k + 1:] -= np.outer(l, y[:n - k - 1])
            M[k, k] = 1
    return np.tril(M[:n]), d, M[n:]


def winv_blocks(L, dt):
    """W = L11^-1 of every 64-block, in its 64 x 64 image (zero past the last pivot)."""
    out = []
    for p0, nb in blocks(L.shape[0]):
        L11 = L[p0:p0 + nb, p0:p0 + nb].astype(dt)
        W = np.eye(nb, dtype=dt)
        with np.errstate(all="ignore"):
            for k in range(nb):  # forward substitution, row by row
                W[k] -= L11[k, :k] @ W[:k]
        Wf = np.zeros((NB, NB), dt)
        Wf[:nb, :nb] = W
        out.append(Wf)
    return out


_REF = {}


def factor(A, R, dt=LD):
    """dict(L, d, Y, W, Z) of unblocked() in dt (long double: the reference; the kernels' dtype: the yardstick), cached."""
    A, R = np.ascontiguousarray(A), np.ascontiguousarray(np.atleast_2d(R))
    key = (hashlib.sha1(A.tobytes() + R.tobytes()).hexdigest(), np.dtype(dt).name)
    if key not in _REF:
        L, d, Z = unblocked(A, R, dt)
        _REF[key] = dict(L=L, d=d, Y=L * d[None, :], W=winv_blocks(L, dt), Z=Z, z=Z[0])
    return _REF[key]


def solve(f, dt):
    """x of L^T x = z by back substitution in dt"""
    L, x = f["L"].astype(dt), f["z"].astype(dt).copy()
    for k in range(len(x) - 1, 0, -1):
        x[:k] -= L[k, :k] * x[k]
    return x


# ---- matrix families -----------------------------------------------------------------------------------------------------------------
def spd(D, cond, seed, fp32):
    """(A, b) in the kernels' dtype: Q diag(logspace(0, -log10 cond)) Q^T scaled to a unit diagonal."""
    rng = np.random.default_rng([seed, D, 1])
    Q = np.linalg.qr(rng.standard_normal((D, D)))[0]
    A = (Q * np.logspace(0, -np.log10(cond), D)[None, :]) @ Q.T
    s = 1 / np.sqrt(np.diagonal(A))
    A = A * s[:, None] * s[None, :]
    A = ((A + A.T) / 2).astype(dtype(fp32))
    np.fill_diagonal(A, 1)
    return A, rng.standard_normal(D).astype(dtype(fp32))


def sqd(D, seed, fp32):
    """(A, b): P [[H, B], [B^T, -C]] P^T with H, C of the spd family (condition 1e2), |B|_2 ~ 0.1 -- every principal minor is
    non-singular, the LDL^T exists without pivoting and is stable (|B^T H^-1 B| <= 1), half of its pivots are negative."""
    rng = np.random.default_rng([seed, D, 2])
    n1 = (D + 1) // 2
    n2 = D - n1
    K = np.zeros((D, D))
    K[:n1, :n1] = spd(n1, 1e2, seed + 1, 0)[0]
    if n2:
        K[n1:, n1:] = -spd(n2, 1e2, seed + 2, 0)[0]
        B = rng.standard_normal((n1, n2)) * (0.05 / np.sqrt(D))
        K[:n1, n1:] = B
        K[n1:, :n1] = B.T
    perm = rng.permutation(D)
    A = K[np.ix_(perm, perm)].astype(dtype(fp32))
    return A, rng.standard_normal(D).astype(dtype(fp32))


_EXACT = {}


def exact_problem(D, seed=0, zero_at=None, check=True):
    """The integer family: dict(A, b, L, d, Y, W, z, x) in int64 with A = L diag(d) L^T, b = A x.

    L = I + N, N in {-1, 0, 1}, N_ij != 0 only where j < i and level(i) > level(j) with levels in {0, 1, 2}: N^3 = 0 and so
    L^-1 = I - N + N^2 is an integer matrix, and so is every block's W = L11^-1.  d_k in {+-1, +-2, +-4}: the reciprocal of a power
    of two is exact after ba_rcp's Newton step whatever the last bit of the hardware estimate, so L = Y d^-1 is exact.  Every
    quantity the blocked algorithm forms -- a partly updated Schur complement, Y = X W^T, a W tile, a partial sum of the sweep -- is
    a sum of integer products whose absolute values add up to less than 2^24 (asserted here: below 2^20 for the Schur terms and W),
    so every partial sum, in any order, fused or not, is an integer that fp32 holds: the result is bit for bit the integer one.
    Planted: row i(t) of every block t has level 2 and N[i(t), k(p)] = +-1 in the level-0 column k(p) of EVERY earlier block p, so
    that each panel's product Y(ti, p) L(tj, p)^T is non-zero on every tile ti >= tj > p: a tile or a panel left out shows.  Every
    other row has three random entries.  zero_at: d at that index is 0 (z and x are then undefined and returned as None)."""
    key = (D, seed, zero_at)
    if key in _EXACT:
        return _EXACT[key]
    rng = np.random.default_rng([seed, D, 3])
    blk = blocks(D)
    level = rng.integers(0, 3, D)
    rows, cols = [], []
    for t, (p0, nb) in enumerate(blk):
        rows.append(p0 + (7 * t + 13) % nb)
        cols.append(p0 + (7 * t + 14 + t % 5) % nb)
    for t, (p0, nb) in enumerate(blk):
        if t + 1 < len(blk):
            level[cols[t]] = 0
        if t > 0:
            level[rows[t]] = 2
    N = np.zeros((D, D), np.int64)
    for i in range(1, D):
        if i in rows[1:]:
            continue  # (a planted row holds its planted entries alone: one term per panel, nothing to cancel it)
        for j in rng.integers(0, i, 3):
            if level[j] < level[i]:
                N[i, j] = rng.choice((-1, 1))
    for t in range(1, len(blk)):
        N[rows[t], [cols[p] for p in range(t)]] = rng.choice((-1, 1), t)
    L = np.eye(D, dtype=np.int64) + N
    d = rng.choice((1, 2, 4), D) * rng.choice((-1, 1), D)
    if zero_at is not None:
        d[zero_at] = 0
    x = rng.integers(-3, 4, D)
    x[x == 0] = 1
    Y = L * d[None, :]
    Lf, Yf = L.astype(np.float64), Y.astype(np.float64)  # (float64 BLAS products of small integers are exact)
    A = np.zeros((D, D))
    absA = np.zeros((D, D))
    zf = Lf.T @ x  # z = L^T x
    zy = np.abs(zf)[None, :] * np.abs(d)[None, :]
    absz = np.zeros(D)
    missing = []
    for p, (p0, nb) in enumerate(blk):
        P = Yf[p0:, p0:p0 + nb] @ Lf[p0:, p0:p0 + nb].T  # (rows and columns in front of the panel: L is lower triangular)
        A[p0:, p0:] += P
        absA[p0:, p0:] += np.abs(Yf[p0:, p0:p0 + nb]) @ np.abs(Lf[p0:, p0:p0 + nb]).T
        absz += (zy[:, p0:p0 + nb] @ np.abs(Lf[:, p0:p0 + nb]).T)[0]
        if check and zero_at is None:
            nz = np.zeros((D, D), bool)
            nz[p0:, p0:] = P != 0
            for ti in range(p + 1, len(blk)):
                for tj in range(p + 1, ti + 1):
                    if not nz[blk[ti][0]:blk[ti][0] + blk[ti][1], blk[tj][0]:blk[tj][0] + blk[tj][1]].any():
                        missing.append((ti, tj, p))
    assert not missing, missing[:5]
    A = np.rint(A).astype(np.int64)
    Linv = np.eye(D, dtype=np.int64) - N + (N.astype(np.float64) @ N.astype(np.float64)).astype(np.int64)
    W = []
    wmax = gemm = 0.0
    for p0, nb in blk:
        Wf = np.zeros((NB, NB), np.int64)
        n11 = N[p0:p0 + nb, p0:p0 + nb]
        Wf[:nb, :nb] = np.eye(nb, dtype=np.int64) - n11 + n11 @ n11
        assert np.array_equal(Wf[:nb, :nb] @ L[p0:p0 + nb, p0:p0 + nb], np.eye(nb, dtype=np.int64))
        W.append(Wf)
        wmax = max(wmax, float(np.abs(Wf).max()))
        # Y = X W^T with X = L21 D L11^T (the updated rows below, the right-hand side row among them)
        below = np.vstack([np.abs(Yf[p0 + nb:, p0:p0 + nb]), zy[:, p0:p0 + nb]])
        gemm = max(gemm, float((below @ np.abs(Lf[p0:p0 + nb, p0:p0 + nb]).T @ np.abs(Wf[:nb, :nb]).T.astype(np.float64)).max()))
    b = A @ x
    z = zf.astype(np.int64)
    # the sweep's sums: |W_p^T| (|z_p| + sum_q |L_qp^T| |x_q|) <= wmax * 64 * max(...)
    swp = wmax * NB * float((np.abs(z) + np.abs(Lf).T @ np.abs(x)).max())
    terms = max(float(absA.max()), float(absz.max()))
    assert terms < 2 ** 20 and wmax < 2 ** 20 and gemm < 2 ** 24 and swp < 2 ** 24, (terms, wmax, gemm, swp)
    if check:
        assert np.array_equal(Lf @ Linv.astype(np.float64), np.eye(D)) and np.array_equal(A, A.T)
    ex = dict(A=A, b=b, L=L, d=d, Y=Y, W=W, z=z, x=x, Linv=Linv, terms=terms, wmax=wmax, gemm=gemm, D=D)
    if zero_at is not None:
        ex["z"] = ex["x"] = None
    _EXACT[key] = ex
    if len(_EXACT) > 3:
        _EXACT.pop(next(iter(_EXACT)))
    return ex


def exact_cov_rows(ex, s):
    """The stacked rows of the covariance form, B = E L^-T D^-1 with E = diag(s): dyadic rationals, exact in fp64."""
    Yr = np.abs(s)[:, None] * np.abs(ex["Linv"]).T.astype(np.float64)  # |Y| of the stacked rows: s_k |L^-1|_jk
    # their partly updated rows are sums of the terms Y_kj L_ij, and Y = X W^T sums at most 64 products with |W| <= wmax
    assert float((Yr @ np.abs(ex["L"]).T.astype(np.float64)).max()) * 64 * ex["wmax"] < 2 ** 24
    return (s[:, None] * ex["Linv"].T) / ex["d"][None, :].astype(np.float64)


# ---- what a run left -----------------------------------------------------------------------------------------------------------------
def retained(ncols, fused):
    """{panel: Wp slot} of the panels whose Y is still in Wp behind the factor (ba_ldlt_factor: slot p below 48 block columns on the
    fused route, p % 4 beyond, slot 0 otherwise).  Only a full block column has rows below it, so only such a panel writes."""
    nblk = -(-ncols // NB)
    writers = [p for p, (p0, nb) in enumerate(blocks(ncols)) if nb == NB]
    if not writers:
        return {}
    if nblk >= 48 and fused:
        return {p: p % 4 for p in writers[-4:]}
    if nblk >= 2 and fused:
        return {p: p for p in writers}
    return {writers[-1]: 0}


def below_mask(D):
    """[row, column]: strictly below the column's diagonal block"""
    i = np.arange(D)
    return i[:, None] >= (i[None, :] // NB + 1) * NB


def parts(run, D=None):
    """L (entries below the diagonal blocks, zero elsewhere), z, {panel: Y below the diagonal block as [rows, 64]}, W, x of a run."""
    D = run["ncols"] if D is None else D
    S = run["S"]
    L = np.where(below_mask(D), S[:D, :D].T, 0)
    Y = {p: run["Wp"][slot][:, NB * (p + 1):run["nrows"]].T for p, slot in retained(run["ncols"], run["fused"]).items()}
    return dict(L=L, z=S[:D, run["zrow"]].copy(), Y=Y, W=run["Winv"], x=run["x"][:D])


def _colrel(err, ref):
    """max over the columns of max |err| / max |ref| of the column (columns without entries left out)"""
    if err.size == 0:
        return 0.0
    e, r = np.abs(err).max(axis=0), np.abs(ref).max(axis=0)
    ok = r > 0
    if np.isnan(e).any():
        return float("nan")
    out = float((e[ok] / r[ok]).max()) if ok.any() else 0.0
    return float("inf") if (e[~ok] > 0).any() else out


def forward_metrics(pr, ref):
    """fwd_L, fwd_Y, fwd_W, fwd_z, yld of parts `pr` (of a run or of the yardstick: yard_parts) against the reference factor."""
    D = len(ref["d"])
    m = below_mask(D)
    Lh, Ls = pr["L"].astype(LD), ref["L"].astype(LD)
    out = dict(fwd_L=_colrel(np.where(m, Lh - Ls, 0), np.where(m, Ls, 0)))
    # Y's rows of the matrix per column like L; its right-hand side row (z d) on its own scale, max |z* d*|, like fwd_z: inside one
    # column it would be measured against the column's L entries, which are no scale for it
    fy = yl = 0.0
    zd = (ref["Z"][0] * ref["d"]).astype(LD)
    for p, Yh in pr["Y"].items():
        r0, c = NB * (p + 1), slice(NB * p, NB * p + NB)
        n = D - r0  # rows of the matrix below the diagonal block; row n of Yh is the right-hand side row
        Yh = Yh.astype(LD)
        dc = ref["d"][None, c].astype(LD)
        fy = max(fy, _colrel(Yh[:n] - ref["Y"][r0:, c], ref["Y"][r0:, c]), float(np.abs(Yh[n] - zd[c]).max() / np.abs(zd).max()))
        yl = max(yl, _colrel(Yh[:n] - Lh[r0:, c] * dc, ref["Y"][r0:, c]),
                 float(np.abs(Yh[n] - pr["z"].astype(LD)[c] * dc[0]).max() / np.abs(zd).max()))
    out["fwd_Y"], out["yld"] = float(fy), float(yl)
    fw = 0.0
    for t, (p0, nb) in enumerate(blocks(D)):
        Lx = np.eye(NB, dtype=LD)
        Lx[:nb, :nb] = Ls[p0:p0 + nb, p0:p0 + nb]
        Ix = np.zeros((NB, NB), LD)
        Ix[:nb, :nb] = np.eye(nb)
        fw = max(fw, float(np.abs(np.asarray(pr["W"][t]).astype(LD) @ Lx - Ix).max()))
    out["fwd_W"] = fw
    zs = ref["z"].astype(LD)
    out["fwd_z"] = float(np.abs(pr["z"].astype(LD) - zs).max() / np.abs(zs).max())
    return out


def yard_parts(yard, ncols, fused, nrows):
    """The yardstick's factor in the shape of parts(): what the same storage would hold."""
    D = len(yard["d"])
    Y = {}
    for p in retained(ncols, fused):
        c = slice(NB * p, NB * p + NB)
        Y[p] = np.vstack([yard["Y"][NB * (p + 1):, c], (yard["Z"] * yard["d"][None, :])[:, c]])[:nrows - NB * (p + 1)]
    return dict(L=np.where(below_mask(D), yard["L"], 0), z=yard["z"], Y=Y, W=yard["W"], x=None)


def sweep_metric(pr, x=None):
    """The back sweep on its own inputs (module docstring), W, L, z of `pr`, x of the sweep."""
    x = (pr["x"] if x is None else x).astype(LD)
    D = len(x)
    L, z = pr["L"].astype(LD), pr["z"].astype(LD)
    r = z - L.T @ x
    ra = np.abs(z) + np.abs(L).T @ np.abs(x)
    worst = 0.0
    for t, (p0, nb) in enumerate(blocks(D)):
        W = np.asarray(pr["W"][t]).astype(LD)[:nb, :nb]
        num = np.abs(x[p0:p0 + nb] - W.T @ r[p0:p0 + nb])
        den = np.abs(W).T @ ra[p0:p0 + nb]
        if np.isnan(num).any():
            return float("nan")
        q = np.where(den > 0, num / np.where(den > 0, den, 1), np.where(num > 0, np.inf, 0))
        worst = max(worst, float(q.max()))
    return worst


def pivot_signs(pr, ref):
    """The sign of every pivot as the run's storage shows it."""
    D = len(ref["d"])
    sg = np.zeros(D)
    lib = ref["z"] * ref["d"]  # L^-1 b = D z
    for k in range(D):
        p = k // NB
        if p in pr["Y"]:
            Lc = np.concatenate([pr["L"][NB * (p + 1):, k], pr["z"][k:k + 1]])[:pr["Y"][p].shape[0]]
            i = int(np.argmax(np.abs(Lc)))
            sg[k] = np.sign(float(pr["Y"][p][i, k - NB * p]) * float(Lc[i]))
        else:
            sg[k] = np.sign(float(pr["z"][k]) * float(lib[k]))
    return sg


def sign_mismatches(pr, ref):
    return int(np.sum(pivot_signs(pr, ref) != np.sign(ref["d"].astype(np.float64))))


def cov_metrics(run, ref, D, s):
    """fwd_B (the stacked rows against the reference's, per column) and the pivots s_k / B_kk against d*, relative."""
    ncols = run["ncols"]
    Bh = run["S"][:D, ncols:ncols + D].T.astype(LD)  # [stacked row, column]
    Bs = ref["Z"].astype(LD)[:, :D]
    dh = s.astype(LD) / np.diagonal(Bh)
    return dict(fwd_B=_colrel(Bh - Bs, Bs), pivots=float(np.abs(dh / ref["d"][:D].astype(LD) - 1).max()))


def exact_mismatches(run, ex, sweep=True, x=None):
    """Names of the stored quantities that are not bit for bit the integers of exact_problem."""
    pr = parts(run, ex["D"])
    D = ex["D"]
    bad = []
    if not np.array_equal(pr["L"], np.where(below_mask(D), ex["L"], 0)):
        bad.append("L")
    Zy = (ex["z"] * ex["d"])[None, :]
    for p, Yh in pr["Y"].items():
        c = slice(NB * p, NB * p + NB)
        if not np.array_equal(Yh[:D + 1 - NB * (p + 1)], np.vstack([ex["Y"][NB * (p + 1):, c], Zy[:, c]])):
            bad.append("Y%d" % p)
    for t in range(len(ex["W"])):
        if not np.array_equal(pr["W"][t], ex["W"][t]):
            bad.append("W%d" % t)
    if not np.array_equal(pr["z"], ex["z"]):
        bad.append("z")
    if sweep and not np.array_equal(pr["x"] if x is None else x, ex["x"]):
        bad.append("x")
    return bad


# ---- a numpy emulation of the blocked algorithm, with planted defects ----------------------------------------------------------------------
def emulate(S, nrows, ncols, zrow, fused=True, defect=None):
    with np.errstate(all="ignore"):
        return _emulate(S, nrows, ncols, zrow, fused, defect)


def _emulate(S, nrows, ncols, zrow, fused, defect):
    """The blocked algorithm of ba_dense.hip.h in numpy, in S's dtype, leaving what the kernels leave (the dict of Harness.run): panel
    (unblocked LDL^T of the diagonal block, W = L11^-1), Y = A21 W^T, L = Y d^-1, trailing update tile by tile, the sweep in W form
    over pairs of block columns.  defect: (name, ...) plants one of the defects of tests/test_ldlt_checks.py."""
    dt = S.dtype
    scols, ld = S.shape
    blk = blocks(ncols)
    nblk = len(blk)
    name = defect[0] if defect else None
    M = np.tril(S[:r64(ncols), :nrows].T)  # [row, column], the padding columns included
    So = S.copy()
    slots = max(nblk, 4) if 2 <= nblk < 48 else 4
    Wp = np.zeros((slots, NB, ld), dt)
    Winv = np.zeros((nblk, NB, NB), dt)
    ret = retained(ncols, fused)
    Yhist = {}
    for p, (p0, nb) in enumerate(blk):
        A11 = M[p0:p0 + nb, p0:p0 + nb]
        L11, d, _ = unblocked(A11, np.zeros((0, nb), dt), dt)
        if name == "sign" and defect[1] // NB == p:
            d[defect[1] - p0] = abs(d[defect[1] - p0])
        W = winv_blocks(L11, dt)[0]
        if name == "w_row" and p == nblk - 1 and nb < NB:
            W[nb, :nb] = 1
        Winv[p] = W
        X = M[p0 + nb:, p0:p0 + nb]
        Y = (X @ W[:nb, :nb].T).astype(dt)
        Lb = (Y / d[None, :]).astype(dt)
        So[p0:p0 + nb, p0 + nb:nrows] = Lb.T
        Yhist[p] = Y
        if p in ret:
            Wp[ret[p], :, p0 + NB:nrows] = Y.T
        Yu = Yhist[p - 1][NB:] if name == "wp_slot" and p == defect[1] else Y
        for ti in range(p + 1, -(-nrows // NB)):
            for tj in range(p + 1, min(ti, nblk - 1) + 1):
                reps = 1
                if defect and defect[1:] == (ti, tj, p):
                    reps = 0 if name == "skip_tile" else 2 if name == "twice" else 1
                r = slice(NB * ti, min(NB * ti + NB, nrows))
                c = slice(NB * tj, NB * tj + NB)
                for _ in range(reps):
                    M[r, c] -= (Yu[r.start - p0 - nb:r.stop - p0 - nb] @ _pad(Lb, NB * tj - p0 - nb, NB).T).astype(dt)
    # the sweep: x_p = W_p^T (z_p - sum_{q > p} L_qp^T x_q), L_qp below the diagonal blocks
    x = np.zeros(r64(ncols), dt)
    z = np.zeros(r64(ncols), dt)
    z[:ncols] = So[:ncols, zrow]
    Lm = np.where(below_mask(ncols), So[:ncols, :ncols].T, 0)
    Wuse = list(Winv)
    if name == "w_swap":
        Wuse[defect[1]], Wuse[defect[1] + 1] = Wuse[defect[1] + 1], Wuse[defect[1]]
    for p in range(nblk - 1, -1, -1):
        p0, nb = blk[p]
        zp = z[p0:p0 + NB].copy()
        if name == "z_group" and p == defect[1]:
            zp = z[p0 + 2 * NB:p0 + 3 * NB].copy()
        zp[:nb] -= Lm[:, p0:p0 + nb].T @ x[:ncols]
        x[p0:p0 + nb] = (Wuse[p].T @ zp)[:nb]
    xs = np.zeros(2 * (ld - 64) + 2 * NB, dt)
    xs[:ncols] = x[:ncols]
    return dict(S=So, Wp=Wp, Winv=Winv, x=xs, S2=None, errw=np.zeros(2), guards=np.ones(5, np.int32), rc=0, nrows=nrows, ncols=ncols,
                zrow=zrow, fused=fused, fill=0)


def r64(n):
    return -(-n // NB) * NB


def _pad(Lb, r0, n):
    """rows r0 ... r0 + n - 1 of Lb, zero rows past its end (the padding columns take part in a whole tile's update)"""
    out = np.zeros((n, Lb.shape[1]), Lb.dtype)
    got = Lb[r0:r0 + n]
    out[:got.shape[0]] = got
    return out


ETA = {0: 1e-14, 1: 1e-5}  # the project's ceilings (tests/test_gpu_stages.py: BOUND[("eta", .)])


def measure(run, A, b, fp32, forward=True, sweep=True, signs=False, x=None, cls="1e2"):
    """{metric: (value, bound)} of a run on the matrix (A, b) in the kernels' dtype.  forward: the fwd_* metrics and yld against the
    long-double factor, bounds from the yardstick; sweep: eta and the sweep metric (x: another sweep's result on the same factor)."""
    import stage_checks as SC
    D = A.shape[0]
    pr = parts(run)
    out = {}
    if forward or signs:
        ref = factor(A, b[None, :])
    if forward:
        yard = factor(A, b[None, :], dtype(fp32))
        got = forward_metrics(pr, ref)
        yv = forward_metrics(yard_parts(yard, run["ncols"], run["fused"], run["nrows"]), ref)
        for k in FWD:
            out[k] = (got[k], bound(k, fp32, yv[k], cls))
    if signs:
        out["signs"] = (sign_mismatches(pr, ref), 0)
    if sweep:
        xs = pr["x"] if x is None else x[:D]
        out["eta"] = (SC.eta(np.asarray(A, np.float64), np.asarray(xs, np.float64), np.asarray(b, np.float64)), ETA[int(fp32)])
        out["sweep"] = (sweep_metric(pr, xs), sweep_bound(run["ncols"], fp32))
    return out
