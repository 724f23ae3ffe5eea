"""ctypes driver of tests/ldlt_harness.hip, the dense LDL^T of ba_dense.hip.h on a matrix from the host -- TEST INFRASTRUCTURE ONLY.

The harness is compiled with the library's own hipcc flags (qr_harness.makefile_flags: csrc/Makefile), so that it runs the code the
library runs.  This module stages the matrix (the contract in ldlt_harness.hip's header: everything it leaves open holds the fill
byte), sizes the buffers as ba_solver.hip does and hands back what the kernels left."""
import ctypes as C
import os
import subprocess

import numpy as np

import qr_harness as QH

ROOT = QH.ROOT
CSRC = QH.CSRC
SRC = os.path.join(ROOT, "tests", "ldlt_harness.hip")
NB = 64
NAUG = 3  # ba_solver.hip: augmented rows behind the matrix
GUARDS = ("S", "Wp", "Winv", "x", "flags")


def build(outdir):
    hipcc, flags = QH.makefile_flags()
    out = os.path.join(str(outdir), "ldlt_harness.so")
    subprocess.run([hipcc] + flags + ["-shared", "-I", CSRC, SRC, "-o", out], check=True, capture_output=True, timeout=900)
    return out


def r64(n):
    return -(-n // NB) * NB


def layout(D):
    """(Dp, ld, columns of S) as ba_solver.hip computes them for D unknowns."""
    Dp = r64(D + NAUG)
    return Dp, Dp + 64, Dp + 64


def cov_layout(D):
    """(ncols, nrows, ld, columns) of the covariance form: the last block column padded, D stacked rows behind it."""
    ncols = r64(D)
    return ncols, ncols + D, r64(ncols + D + NAUG) + 64, ncols + 64


def filled(shape, dt, fill):
    return np.frombuffer(bytes([fill]) * (int(np.prod(shape)) * np.dtype(dt).itemsize), dt).reshape(shape).copy()


def stage(A, b, dt, fill):
    """S[column, row] of the solver form: lower triangle of A, b in row D, the contract's zeros and unit diagonal, `fill` elsewhere."""
    D = A.shape[0]
    Dp, ld, scols = layout(D)
    S = filled((scols, ld), dt, fill)
    for c in range(D):
        S[c, c:D] = A[c:, c]
        S[c, D] = b[c]
        S[c, D + 1:Dp] = 0
    for c in range(D, Dp):
        S[c, c] = 1
        S[c, c + 1:Dp] = 0
    return S


def stage_cov(A, s, dt):
    """The covariance form as k_cov_stage leaves it in a zeroed buffer: lower triangle of A (already scaled), unit diagonal of the
    padding, s_k e_k^T in row ncols + k."""
    D = A.shape[0]
    ncols, nrows, ld, scols = cov_layout(D)
    S = np.zeros((scols, ld), dt)
    for c in range(D):
        S[c, c:D] = A[c:, c]
        S[c, ncols + c] = s[c]
    for c in range(D, ncols):
        S[c, c] = 1
    return S


class _Args(C.Structure):
    _fields_ = [("fp32", C.c_int), ("nrows", C.c_int), ("ncols", C.c_int), ("ld", C.c_int), ("zrow", C.c_int), ("scols", C.c_int),
                ("fused", C.c_int), ("budget", C.c_longlong), ("cap", C.c_int), ("sweep", C.c_int), ("fill", C.c_int),
                ("n_wp", C.c_longlong), ("n_winv", C.c_longlong), ("n_x", C.c_longlong), ("zh_off", C.c_int)]


SWEEP = {None: 0, "flow": 1, "launches": 2}


class Harness:
    def __init__(self, path):
        L = self.L = C.CDLL(path)
        L.ldh_run.argtypes = [C.POINTER(_Args)] + [C.c_void_p] * 7
        L.ldh_wp_panels.argtypes = [C.c_int]
        self.failed = None  # the first HIP error / device error word: nothing more is launched behind it

    def defaults(self):
        """(budget, cap) of ba_ldlt_make_plan when the environment sets none"""
        b, c = C.c_longlong(), C.c_int()
        self.L.ldh_defaults(C.byref(b), C.byref(c))
        return b.value, c.value

    def cus(self):
        n = C.c_int()
        rc = self.L.ldh_cus(C.byref(n))
        assert rc == 0, rc
        return n.value

    def run(self, S, nrows, ncols, zrow, fp32, fused=True, plan=None, sweep="flow", fill=0xA5, after=False):
        """S: the staged matrix [columns, ld] in the kernels' dtype (not modified).  plan: (budget, cap), None = the defaults.
        Returns S (after the factor), Wp [slots, 64, ld], Winv [block columns, 64, 64], x (the whole vector, zh behind it), S2 (after
        the sweep, when asked for), errw (after factor, after sweep), guards, rc."""
        assert self.failed is None, self.failed
        dt = np.float32 if fp32 else np.float64
        assert S.dtype == dt and S.flags.c_contiguous
        scols, ld = S.shape
        nblk = -(-ncols // NB)
        budget, cap = self.defaults() if plan is None else plan
        S = S.copy()
        Wp = np.empty((self.L.ldh_wp_panels(ncols), NB, ld), dt)
        Winv = np.empty((nblk, NB, NB), dt)
        xoff = ld - 64  # (the solver: Dp; x is 2 Dp + 128 scalars, zh = x + Dp)
        x = np.empty(2 * xoff + 2 * NB, dt)
        S2 = np.empty_like(S) if after and sweep else None
        errw = np.zeros(2)
        guards = np.zeros(5, np.int32)
        a = _Args(int(fp32), nrows, ncols, ld, zrow, scols, int(bool(fused)), int(budget), int(cap), SWEEP[sweep], fill, Wp.size, Winv.size,
                  x.size, xoff)
        p = lambda v: None if v is None else v.ctypes.data_as(C.c_void_p)  # noqa: E731
        rc = self.L.ldh_run(C.byref(a), p(S), p(Wp), p(Winv), p(x), p(S2), p(errw), p(guards))
        if rc != 0 or errw.any():
            self.failed = "ldh_run rc=%d errw=%s (nrows=%d ncols=%d fp32=%d fused=%d sweep=%s)" % (rc, errw, nrows, ncols, fp32, fused, sweep)
        return dict(S=S, Wp=Wp, Winv=Winv, x=x, S2=S2, errw=errw, guards=guards, rc=rc, nrows=nrows, ncols=ncols, zrow=zrow, fused=bool(fused),
                    fill=fill)
