"""ctypes driver of tests/relpose_harness.hip, the kernels of ba_relpose.hip.h on lists from the host -- TEST INFRASTRUCTURE ONLY.

The harness is compiled with the library's own hipcc flags, read from csrc/Makefile (qr_harness.makefile_flags), so that it runs the
code the library runs.  Arrays go in and come back in the kernels' scalar type; a buffer the kernel did not write holds FILL bytes."""
import ctypes as C
import os
import subprocess

import numpy as np

from qr_harness import CSRC, ROOT, makefile_flags

SRC = os.path.join(ROOT, "tests", "relpose_harness.hip")
FILL = 0xA5  # relpose_harness.hip: RPH_BYTE
LIN, LIN_MASK, TRIAL = 0, 1, 2  # rph_relpose's mode: k_relpose<T, true, false>, <T, true, true>, <T, false, false>


def build(outdir):
    hipcc, flags = makefile_flags()
    out = os.path.join(str(outdir), "relpose_harness.so")
    subprocess.run([hipcc] + flags + ["-shared", "-I", CSRC, SRC, "-o", out], check=True, capture_output=True, timeout=600)
    return out


def csr(N, pairs):
    """(ptr [N + 1], inc [2 n]) of the cameras' incident constraints in list order, inc = 2 * constraint + side, as
    ba_solver_set_relative_poses builds it."""
    lists = [[] for _ in range(N)]
    for t, (a, b) in enumerate(np.asarray(pairs).reshape(-1, 2)):
        lists[int(a)].append(2 * t)
        lists[int(b)].append(2 * t + 1)
    ptr = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int32)
    return ptr, np.array([w for x in lists for w in x], np.int32)


def untouched(a):
    """True where every byte of the array still holds the harness's fill."""
    return bool(np.all(np.frombuffer(np.ascontiguousarray(a).tobytes(), np.uint8) == FILL))


_p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731


class Harness:
    def __init__(self, path):
        L = self.L = C.CDLL(path)
        v, i = C.c_void_p, C.c_int
        L.rph_relpose.argtypes = [i, i, i, i, v, v, v, v, v, v, v, i, v, v, v, v]
        L.rph_gather.argtypes = [i, i, i, v, v, v, v, i, v, v, v]
        L.rph_schur.argtypes = [i, i, i, v, v, i, v, v]
        L.rph_matvec.argtypes = [i, i, i, v, v, v, v, v, v, v]
        c = [C.c_int() for _ in range(4)]
        L.rph_cfg(*[C.byref(x) for x in c])
        self.REC, self.HAB, self.G, self.ENT = [x.value for x in c]

    def relpose(self, fp32, mode, cam15, cs, cmask=None, go=-1):
        """cam15 [N, 15] and the lists of cs (relpose_checks.Constraints), rounded to the scalar type here.  Returns dict(rec [n, REC],
        part_e [2, grid], part_keep [2, grid]) as the kernel left them, guards (3)."""
        dt = np.float32 if fp32 else np.float64
        cam15 = np.asarray(cam15, np.float64).reshape(-1, 15)
        N, n = len(cam15), len(cs)
        cam = np.ascontiguousarray(cam15.T.astype(dt))  # [15][N]
        pair = np.ascontiguousarray(cs.pairs, np.int32)
        lists = [np.ascontiguousarray(a.astype(dt)) for a in (cs.R0, cs.t0, cs.Lr, cs.Lt)]
        cm = np.zeros(N, np.uint16) if cmask is None else np.ascontiguousarray(cmask, np.uint16)
        assert len(cm) == N
        grid = (n + 255) // 256
        rec, pe, pk = np.empty((n, self.REC), dt), np.empty((2, grid), dt), np.empty((2, grid), dt)
        guards = np.zeros(3, np.int32)
        rc = self.L.rph_relpose(int(fp32), mode, n, N, _p(cam), _p(pair), *[_p(a) for a in lists], _p(cm), go, _p(rec), _p(pe), _p(pk), _p(guards))
        assert rc == 0, "HIP error %d" % rc
        return dict(rec=rec, part_e=pe, part_keep=pk, guards=guards)

    def gather(self, fp32, N, pairs, rec, V, gc, go=-1):
        """V [N, 81], gc [9 N] pre-filled; returns (V, gc) behind k_relpose_gather, guards (2)."""
        dt = np.float32 if fp32 else np.float64
        pair = np.ascontiguousarray(pairs, np.int32)
        ptr, inc = csr(N, pair)
        rec, V, gc = np.ascontiguousarray(rec, dt), np.array(V, dt).reshape(N, 81), np.array(gc, dt).reshape(9 * N)
        guards = np.zeros(2, np.int32)
        rc = self.L.rph_gather(int(fp32), N, len(pair), _p(ptr), _p(inc), _p(pair), _p(rec), go, _p(V), _p(gc), _p(guards))
        assert rc == 0, "HIP error %d" % rc
        return V, gc, guards

    def schur(self, fp32, N, pairs, rec, ld, S):
        """S [9 N, ld] pre-filled (column 9 lo + c of the lower block triangle is row 9 lo + c here); returns S behind k_relpose_schur,
        guards (1)."""
        dt = np.float32 if fp32 else np.float64
        pair = np.ascontiguousarray(pairs, np.int32)
        rec, S = np.ascontiguousarray(rec, dt), np.array(S, dt).reshape(9 * N, ld)
        guards = np.zeros(1, np.int32)
        rc = self.L.rph_schur(int(fp32), len(pair), N, _p(pair), _p(rec), ld, _p(S), _p(guards))
        assert rc == 0, "HIP error %d" % rc
        return S, guards

    def matvec(self, fp32, N, pairs, rec, v):
        """y [9 N] of ba_relpose_matvec_row, one thread per (camera, row), guards (1)."""
        dt = np.float32 if fp32 else np.float64
        pair = np.ascontiguousarray(pairs, np.int32)
        ptr, inc = csr(N, pair)
        rec, v = np.ascontiguousarray(rec, dt), np.ascontiguousarray(v, dt).reshape(9 * N)
        y = np.empty(9 * N, dt)
        guards = np.zeros(1, np.int32)
        rc = self.L.rph_matvec(int(fp32), N, len(pair), _p(ptr), _p(inc), _p(pair), _p(rec), _p(v), _p(y), _p(guards))
        assert rc == 0, "HIP error %d" % rc
        return y, guards
