"""Host yardstick of ba_solver_covariance_pcg (csrc/ba_pcg_multi.hip.h) -- TEST INFRASTRUCTURE ONLY.

Covariance blocks as solutions of S X = B, column by column, by the recurrence of pcg_checks.pcg:

    Sigma_ab = rows a of S^-1 E_b   (served from column block max(a, b); (X + X') / 2 on the diagonal)
    Sigma_pp = U_p^-1 + Y_p' S^-1 Y_p,  Y_p = W_p U_p^-1  (rows of camera c: sum over the point's observations o by c of Jc_o'Jp_o U_p^-1)

on a DENSE S (the quad assembly from the GPU's own J, cov_checks.quad_reduced) whose rows and columns of fixed parameters are the
identity, preconditioned by the documented B_a (pcg_checks.documented_blocks) with a unit diagonal on the fixed rows.  In np.longdouble
with products by S it is the reference; in float64 with the matrix-free product (V p - (V - S) p, pcg's V=) it is the working-precision
yardstick.  Every column is a recurrence of its own: own alpha, beta, stopping test and iteration count.  shared_alpha=True plants the
defect of a batch whose columns share one alpha (tests/test_covariance_pcg_cpu.py shows that the bound sees it).

Jc [K, 2, 9], Jp [K, 2, 3] in the order of p.cam_idx / p.pt_idx (point-sorted), as cov_checks takes them.
"""
import numpy as np

import cov_checks as CC
import pcg_checks as PC

LD = np.longdouble
NR = 9


def identity_rows(A, fixed):
    """A copy of the square matrix A with the rows and columns `fixed` (bool) replaced by the identity's."""
    A = np.array(A)
    fx = np.flatnonzero(fixed)
    A[fx, :] = 0
    A[:, fx] = 0
    A[fx, fx] = 1
    return A


def identity_rows_blocks(B, fixed):
    """The same per 9 x 9 block [N, 9, 9]."""
    B = np.array(B)
    for a, r in zip(*np.nonzero(np.asarray(fixed).reshape(-1, 9))):
        B[a, r, :] = 0
        B[a, :, r] = 0
        B[a, r, r] = 1
    return B


class Case:
    """One linearisation: (p, Jc, Jp) of the solver, lam, the quad S at lam, the mask.  S_extra_blocks: nothing here knows priors or
    constraints -- hand in an S (and V, U) that already holds them (S=, V=, U=)."""

    def __init__(self, p, Jc, Jp, lam, S, cam_mask=None, pt_fixed=None, V=None, U=None):
        self.p, self.lam = p, float(lam)
        self.fc, self.fp = CC.free_sets(p, cam_mask, pt_fixed)
        self.Jc, self.Jp = CC.mask_jacobian(p, Jc, Jp, cam_mask, pt_fixed)
        self.D = 9 * p.N
        self.S = identity_rows(np.asarray(S, LD), ~self.fc)
        B = PC.documented_blocks(p, self.Jc, self.Jp, lam, np.asarray(S, LD))
        self.B = identity_rows_blocks(B, ~self.fc)
        self.V = identity_rows_blocks(PC.camera_blocks(p, self.Jc, lam) if V is None else np.asarray(V, LD), ~self.fc)
        Ul, self.G = CC.point_blocks(p, self.Jc.astype(LD), self.Jp.astype(LD), LD(lam), LD)
        self.U = Ul if U is None else np.asarray(U, LD)
        order = np.argsort(p.pt_idx, kind="stable")
        self.order, self.ptr = order, np.searchsorted(p.pt_idx[order], np.arange(p.M + 1))
        self.Minv, ok = PC.invert_blocks(self.B, LD)
        assert ok.all(), "a documented block B_a is not positive definite"
        self._cache = {}

    # ---- right-hand sides ------------------------------------------------------------------------------------------------------------
    def rhs_cam(self, b):
        """E_b [D, 9]; the column of a fixed parameter is zero."""
        E = np.zeros((self.D, NR), LD)
        for c in range(9):
            if self.fc[9 * b + c]:
                E[9 * b + c, c] = 1
        return E

    def point_inverse(self, j, dtype=LD):
        return CC._inv3(np.asarray(self.U[j], dtype))

    def rhs_point(self, j, dtype=LD):
        """Y_p [D, 3] in dtype; zero for a fixed point or one nobody observes."""
        Y = np.zeros((self.D, 3), dtype)
        if not self.fp[j]:
            return Y
        obs = self.order[self.ptr[j]:self.ptr[j + 1]]
        if len(obs) == 0:
            return Y
        Ui = self.point_inverse(j, dtype)
        for o in obs:
            a = int(self.p.cam_idx[o])
            Y[9 * a:9 * a + 9] += np.asarray(self.G[o], dtype) @ Ui
        return Y

    # ---- solves ------------------------------------------------------------------------------------------------------------------------
    def solve(self, Bm, max_iter, rel_tol, dtype=LD, keep=None, matrix_free=False):
        """Every column of Bm [D, n] by its own recurrence.  dict(X [D, n] (the last iterate), iters [n], conv [n] bool, live [n] bool,
        xs {k: [D, n]} for k in keep (a column that stopped before k keeps its last iterate)); None when the working-precision yardstick
        does not exist (pcg_checks.yardstick)."""
        n = Bm.shape[1]
        X = np.zeros((self.D, n), dtype)
        iters, conv, live = np.zeros(n, int), np.ones(n, bool), np.zeros(n, bool)
        keep = sorted(keep or ())
        xs = {k: np.zeros((self.D, n), dtype) for k in keep}
        for c in range(n):
            b = Bm[:, c]
            if not np.any(b):
                continue
            live[c] = True
            if dtype == LD:
                out = PC.pcg(self.S, b, self.Minv, max_iter, rel_tol, LD, keep)
            else:
                out = PC.yardstick(self.S, np.asarray(b, LD), self.B, max_iter, rel_tol, dtype, keep, V=self.V if matrix_free else None)
                if out is None:
                    return None
            X[:, c], iters[c], conv[c] = out["x"], out["iters"], out["converged"]
            for k in keep:
                xs[k][:, c] = out["xs"].get(k, out["x"])
        return dict(X=X, iters=iters, conv=conv, live=live, xs=xs)

    def solve_shared_alpha(self, Bm, max_iter, rel_tol):
        """THE PLANTED DEFECT: the recurrence on all columns of a batch at once with ONE alpha = sum_c r'z / sum_c p'Sp for the batch
        (own beta and own stopping test per column), long double."""
        n = Bm.shape[1]
        N = self.p.N
        prec = lambda R: np.einsum("nij,njc->nic", self.Minv, R.reshape(N, 9, n)).reshape(-1, n)  # noqa: E731
        X, R = np.zeros((self.D, n), LD), np.array(Bm, LD)
        Z, P = prec(R), np.zeros((self.D, n), LD)
        bb = (R * R).sum(axis=0)
        rz = (R * Z).sum(axis=0)
        rz_old = np.ones(n, LD)
        tol2 = LD(rel_tol) ** 2
        done = ~(bb > 0)
        iters = np.zeros(n, int)
        for k in range(max_iter):
            done |= (R * R).sum(axis=0) <= tol2 * bb
            if done.all():
                break
            act = ~done
            beta = np.where(act, rz / rz_old, 0) if k else np.zeros(n, LD)
            Pk = Z + beta * P
            Y = self.S @ Pk
            alpha = rz[act].sum() / (Pk[:, act] * Y[:, act]).sum()
            X[:, act] += alpha * Pk[:, act]
            R[:, act] -= alpha * Y[:, act]
            P[:, act] = Pk[:, act]
            Z[:, act] = prec(R)[:, act]
            rz_old = np.where(act, rz, rz_old)
            rz = np.where(act, (R * Z).sum(axis=0), rz)
            iters[act] += 1
        return dict(X=X, iters=iters, conv=done, live=bb > 0, xs={})

    # ---- the blocks ----------------------------------------------------------------------------------------------------------------------
    def covariance(self, pairs=(), points=(), max_iter=1000, rel_tol=1e-10, dtype=LD, matrix_free=False, shared_alpha=False, at=None):
        """(cc [n, 9, 9], pp [m, 3, 3], info) as ba_solver_covariance_pcg assembles them; None where the working-precision yardstick
        does not exist.  at = k: from the iterates x_k instead of the last ones (prefix tests).  info: iters (per live column, in the
        order solved), unconverged, columns, Ynorm [m, 3] = |Y_p e_i|_2, X {('c', b) | ('p', j): the columns}."""
        pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
        points = np.asarray(points, np.int64).reshape(-1)
        keep = None if at is None else [at]
        cc = np.zeros((len(pairs), 9, 9), dtype)
        pp = np.zeros((len(points), 3, 3), dtype)
        info = dict(iters=[], unconverged=0, columns=0, Ynorm=np.zeros((len(points), 3)), X={})

        def run(key, Bm):
            ck = (key, max_iter, rel_tol, np.dtype(dtype).name, matrix_free, shared_alpha, at)
            if ck not in self._cache:
                if shared_alpha:
                    out = self.solve_shared_alpha(Bm, max_iter, rel_tol)
                else:
                    out = self.solve(np.asarray(Bm, dtype if dtype != LD else LD), max_iter, rel_tol, dtype, keep, matrix_free)
                self._cache[ck] = out
            out = self._cache[ck]
            if out is None:
                return None
            lv = out["live"]
            info["iters"] += list(out["iters"][lv])
            info["unconverged"] += int((~out["conv"][lv]).sum())
            info["columns"] += int(lv.sum())
            return out["X"] if at is None else out["xs"][at]

        for b in sorted(set(int(max(q)) for q in pairs)):
            if not self.fc[9 * b:9 * b + 9].any():
                continue
            X = run(("c", b), self.rhs_cam(b))
            if X is None:
                return None
            info["X"][("c", b)] = X
            for q, (pa, pb) in enumerate(pairs):
                if max(pa, pb) != b:
                    continue
                if pa == pb:
                    blk = X[9 * b:9 * b + 9]
                    cc[q] = (blk + blk.T) / 2
                elif pb == b:
                    cc[q] = X[9 * pa:9 * pa + 9]
                else:
                    cc[q] = X[9 * pb:9 * pb + 9].T
        solved = [q for q, j in enumerate(points) if self.fp[j] and self.ptr[j + 1] > self.ptr[j]]
        for q, j in enumerate(points):
            if self.fp[j] and self.ptr[j + 1] == self.ptr[j]:
                pp[q] = np.eye(3) / dtype(self.lam)
        for s0 in range(0, len(solved), 3):
            batch = solved[s0:s0 + 3]
            Ys = [self.rhs_point(int(points[q]), dtype) for q in batch]
            if shared_alpha:
                X = run(("p", tuple(int(points[q]) for q in batch)), np.concatenate(Ys, axis=1))
                Xs = [X[:, 3 * i:3 * i + 3] for i in range(len(batch))]
            else:
                Xs = [run(("p", int(points[q])), Y) for q, Y in zip(batch, Ys)]
            for q, Y, X in zip(batch, Ys, Xs):
                if X is None:
                    return None
                j = int(points[q])
                info["X"][("p", j)] = X
                info["Ynorm"][q] = np.sqrt((np.asarray(Y, LD) ** 2).sum(axis=0)).astype(np.float64)
                m = Y.T @ X
                pp[q] = self.point_inverse(j, dtype) + (m + m.T) / 2
        return cc, pp, info

    def norm_inverse(self):
        """|S^-1|_2 on the free parameters (= |Sigma_cc|_2)."""
        idx = np.flatnonzero(self.fc)
        ev = np.linalg.eigvalsh(np.asarray(self.S, np.float64)[np.ix_(idx, idx)])
        return float(1 / ev[0])

    def true_residuals(self, b, Xb):
        """|E_b - S X_b|_2 per column, long double (the columns' |b| is 1)."""
        R = self.rhs_cam(b) - self.S @ np.asarray(Xb, LD)
        return np.sqrt((R * R).sum(axis=0)).astype(np.float64)


def all_pairs(N):
    a, b = np.meshgrid(np.arange(N), np.arange(N), indexing="ij")
    return np.stack([a.ravel(), b.ravel()], axis=1).astype(np.int32)


def assemble(cc, N):
    """[N * N, 9, 9] in all_pairs' order -> [9 N, 9 N]."""
    return np.asarray(cc).reshape(N, N, 9, 9).transpose(0, 2, 1, 3).reshape(9 * N, 9 * N)


def entry_scales(pairs, Ynorm):
    """|b_i| |b_j| per entry: ones [n, 9, 9] for camera blocks, |Y_p e_i| |Y_p e_j| [m, 3, 3] for point blocks."""
    return np.ones((len(pairs), 9, 9)), Ynorm[:, :, None] * Ynorm[:, None, :]


def work_bytes(N, M, chunks):
    """Bytes ba_solver_device_bytes grows by at the first ba_solver_covariance_pcg (include/ba_mi355x.h), the state struct aside."""
    return 8 * (6 * 81 * N + 27 * max(M, 1) + 81 * max(chunks, 1) + 81 * N + 27 * ((N + 27) // 28))
