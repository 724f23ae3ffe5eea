"""GPU: the dense Householder QR of ba_qr.hip.h (k_qr_chunk, k_qr_apply, k_qr_backsolve) on its own inputs, at every TSQR shape.

test_gpu_stages.py::test_dense_qr_step checks the QR only through the camera step, whose bound includes the point elimination.  Here
the metrics of tests/stage_checks.py (qr_metrics) measure the QR alone, against sums in long double / quad over the matrix the QR was
handed:
  gram      max |R'R - A'A|_ij / (|a_i| |a_j|), the backward error of the factor (probe form for large m D^2)
  qtb_head  max |R'c - A'b|_i / (|a_i| |b|), the head of Q^T b
  orth      | |Q^T b|^2 - |b|^2 | / |b|^2 -- Q^T b is all of column D: the right-hand side rides along through every level
  tri       max |R y - c|_i / (|R| |y| + |c|)_i, k_qr_backsolve alone
Two sources of matrices:
  harness   tests/qr_harness.hip (compiled with the library's flags): ba_qr_factor + ba_qr_backsolve on a host matrix, with guard
            words behind A, the T storage and y, the padding rows checked, one or two streams, a go word, BA_QR_HW_SQRT's flag
  solver    the matrix a trial really factors (getter 15, BA_DBG_QRCHECK) and what the factorisation left (getter 16), y = the camera
            step (GET_DX): QRKIT, MOREQR's inner QR, QRSPQR
Each value is printed as `STAGE <case> <metric> <value> <bound>`.  Measured worst on an MI355X (two runs, the same values), fp64 / fp32:
  gram      1.4e-15 / 8.2e-7 (solver: MOREQR's inner matrix, problem-21); harness 5.7e-16 / 4.0e-7
  qtb_head  2.9e-16 / 1.8e-7 (harness, square matrices)
  orth      4.2e-16 / 2.7e-7 (harness, square, D = 100); solver 3.5e-17 / 1.9e-9
  tri       4.9e-16 (D = 16 320) / 2.8e-7 (D = 351)
Four-level trees: the harness at 131 073 (fp64) and 262 145 (fp32) rows, problem-39's J2bot in fp64 (181 633 rows); five levels at
2 097 153 rows (fp64).  k_qr_backsolve's dynamic LDS: requests up to the device's limit of 160 KiB run (fp64 D = 16 320, 0.5 s for
the whole QR).  The 117 cases take 35 s on an MI355X.
"""
import ctypes as C

import numpy as np
import pytest

import qr_harness as QH
import stage_checks as SC
from test_gpu_parity import _moreqr_default_route, _ragged_problem  # noqa: F401 (autouse fixture)
from test_gpu_stages import Checker

pytestmark = pytest.mark.gpu

# Bounds, set from the first MI355X run with 10x headroom over the worst value of every case of this file (in the comment), within
# the ceilings 1e-14 (fp64) and 1e-5 (fp32).  fp64 gram: the ceiling, 7x over MOREQR's inner matrix on problem-21 (68 268 rows).
BOUND = {
    ("gram", 0): 1e-14, ("gram", 1): 1e-5,            # 1.4e-15 (solver, MOREQR p21) / 8.2e-7 (the same in fp32)
    ("qtb_head", 0): 3e-15, ("qtb_head", 1): 2e-6,    # 2.9e-16 (square, D = 64) / 1.8e-7 (square, D = 20)
    ("orth", 0): 5e-15, ("orth", 1): 3e-6,            # 4.2e-16 / 2.7e-7 (square, D = 100)
    ("tri", 0): 5e-15, ("tri", 1): 3e-6,              # 4.9e-16 (D = 16 320) / 2.8e-7 (D = 351)
}
PROBE_ABOVE = 5e9  # m D^2 beyond which gram takes the probe form


@pytest.fixture(scope="module")
def qrh(tmp_path_factory):
    return QH.Harness(QH.build(tmp_path_factory.mktemp("qr_harness")))


def _dt(fp32):
    return np.float32 if fp32 else np.float64


def _depth(m, c0, ch):
    """TSQR levels of the panel at c0 (ba_qr_factor): level 1 chunks of CH rows, 16 R's per chunk above."""
    nsb, fan, lv = -(-(m - c0) // 32), ch // 32, 1
    while True:
        nch = -(-nsb // fan)
        if nch == 1:
            return lv
        nsb, fan, lv = nch, 16, lv + 1


def _chunks(m, ch):
    """chunks per level of panel 0 (the most of every panel)"""
    nsb, fan, out = -(-m // 32), ch // 32, []
    while True:
        nch = -(-nsb // fan)
        out.append(nch)
        if nch == 1:
            return out
        nsb, fan = nch, 16


def make(kind, m, D, fp32, ch, seed=0):
    """[D + 1, m] in the kernels' dtype: b in column D.  kind: gauss | graded (columns over 1e-8 ... 1e8) | blocksparse (every
    column zero in whole level-1 chunks) | tiny (column D // 2 in the scale-up range of k_qr_chunk) | huge (fp32: column D // 3 of
    1e19 with an outlier of 1e25, the scale-down range) | zerobelow (columns 0 ... 4 zero below the diagonal: identity reflectors) |
    lowrank (the second level-1 chunk's rows of panel 0 of rank 8) | dupcol / zerocol (exact rank deficiency)."""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((D + 1, m))
    if kind == "graded":
        X[:D] *= 10.0 ** rng.uniform(-8, 8, (D, 1))
    elif kind == "blocksparse":
        seen = np.zeros(D, bool)
        for r0 in range(0, m, ch):
            off = rng.random(D) < 0.5
            if r0 + ch >= m:
                off &= seen  # (every column keeps a chunk: full rank)
            seen |= ~off
            X[:D][off, r0:r0 + ch] = 0.0
    elif kind == "tiny":
        X[D // 2] *= 1e-21 if fp32 else 1e-150
    elif kind == "huge":
        X[D // 3] *= 1e19
        X[D // 3, m // 2] = 1e25
    elif kind == "zerobelow":
        for c in range(min(5, D)):
            X[c, c + 1:] = 0.0
    elif kind == "lowrank":
        r0, r1 = min(ch, m), min(2 * ch, m)
        k = min(32, D)
        X[:k, r0:r1] = rng.standard_normal((k, 8)) @ rng.standard_normal((8, r1 - r0))
    elif kind == "dupcol":
        X[D - 2] = X[1]
    elif kind == "zerocol":
        X[D // 2] = 0.0
    return X.astype(_dt(fp32))


def check_harness_run(qrh, name, Ab, m, D, fp32, ck, rank_deficient=False, probes=None, **kw):
    """Runs the harness and asserts: no HIP error, guards and padding rows intact, T storage written only where the chunks of the
    tree are, and the four metrics (the factor's three alone when rank_deficient).  Returns the run."""
    ch, levels = qrh.cfg(fp32)
    r = qrh.run(Ab, m, D, fp32, **kw)
    assert r["rc"] == 0, (name, r["rc"])
    assert r["guards"].all(), (name, r["guards"])
    F = r["F"]
    assert not np.any(F[:, m:]), name  # rows >= m stay zero
    nch = _chunks(m, ch)
    assert len(nch) <= levels, (name, nch)
    for lv in range(levels):
        used = nch[lv] * 1024 if lv < len(nch) else 0
        assert QH.untouched(r["tau"][lv, used:]), (name, lv)
    if probes is None:
        probes = 4 if m * D * D > PROBE_ABOVE else 0
    met = SC.qr_metrics(np.asarray(Ab, np.float64), np.asarray(F, np.float64), m, D,
                        None if rank_deficient else np.asarray(r["y"], np.float64), probes=probes)
    for k, v in met.items():
        ck("%s:%s" % (name, k), v, BOUND[(k, int(fp32))])
    return r


# ---- shapes ---------------------------------------------------------------------------------------------------------------------
def shape_cases():
    out = []
    for fp32 in (0, 1):
        ch = 1024 if fp32 else 512
        p = "f32" if fp32 else "f64"
        # depth: one level up to CH rows, two up to 16 CH, three up to 256 CH, four beyond
        for m in (ch - 1, ch, ch + 1, 16 * ch, 16 * ch + 1, 256 * ch + 1):
            out.append(("depth-%s-m%d" % (p, m), fp32, m, 40, "gauss"))
        out.append(("depthdrop-%s" % p, fp32, ch + 40, 96, "gauss"))          # 2 levels in panels 0, 1; 1 from panel 2
        out.append(("depthdrop3-%s" % p, fp32, 16 * ch + 20, 64, "gauss"))   # 3 levels in panel 0 (a one-sub-block chunk), 2 in panel 1
        # the last panel's width D mod 32 (0: none partial) and the right-hand side alone in the last strip (D = 32 k)
        for D in (1, 9, 31, 32, 33, 63, 64, 65, 288, 351):
            out.append(("width-%s-D%d" % (p, D), fp32, 2 * ch + 37, D, "gauss"))
        out.append(("onesub-%s" % p, fp32, 3 * ch + 20, 40, "gauss"))      # the last level-1 chunk: one sub-block of 20 rows
        for r in (1, 31):                                                 # the last sub-block: 1 / 31 valid rows
            out.append(("tail%d-%s" % (r, p), fp32, 2 * ch + r, 33, "gauss"))
        for D in (20, 64, 100):                                           # square: chunks with fewer rows than 32
            out.append(("square-%s-D%d" % (p, D), fp32, D, D, "gauss"))
    out.append(("depth5-f64", 0, 2097153, 9, "gauss"))                     # 4097 -> 257 -> 17 -> 2 -> 1 chunks
    return out


SHAPES = shape_cases()


@pytest.mark.parametrize("name,fp32,m,D,kind", SHAPES, ids=[c[0] for c in SHAPES])
def test_qr_shapes(qrh, gpu_ok, name, fp32, m, D, kind):
    """Every TSQR depth of both precisions (fp64: 1 level up to 512 rows, 2 up to 8192, 3 up to 131 072, 4 beyond, 5 at 2 097 153;
    fp32: 1024, 16 384, 262 144), panels whose depth differs, every partial piece (last panel width D mod 32, last chunk of one
    sub-block, last sub-block of 1 / 31 rows, the right-hand side alone in the last 32-column strip, square matrices).  Measured worst
    on an MI355X: fp64 gram 5.7e-16, qtb_head 2.9e-16, orth 4.2e-16, tri 4.7e-16; fp32 4.0e-7, 1.8e-7, 2.7e-7, 2.8e-7."""
    ch, _ = qrh.cfg(fp32)
    ck = Checker("qr[%s]" % name)
    print("STAGE qr[%s] levels %d (panel 0), %d (last panel)" % (name, _depth(m, 0, ch), _depth(m, 32 * ((D - 1) // 32), ch)))
    check_harness_run(qrh, name, make(kind, m, D, fp32, ch), m, D, fp32, ck)
    ck.done()


# ---- values ---------------------------------------------------------------------------------------------------------------------
VALUES = [(k, fp32) for fp32 in (0, 1) for k in ("graded", "blocksparse", "tiny", "zerobelow", "lowrank", "dupcol", "zerocol")] + \
    [("huge", 1)]


@pytest.mark.parametrize("kind,fp32", VALUES, ids=["%s-%s" % (k, "f32" if f else "f64") for k, f in VALUES])
def test_qr_values(qrh, gpu_ok, kind, fp32):
    """The value branches of k_qr_chunk's reflector on planted data (make()): graded and block-sparse columns (J2bot's), the scale-up
    branch (fp64 entries of 1e-150, fp32 1e-21: squares below the normal range), the scale-down branch (fp32 entries of 1e19 and an
    outlier of 1e25: the squared norm overflows), identity reflectors (columns exactly zero below the pivot), a level-1 chunk of
    rank 8, exact rank deficiency (a repeated or zero column: the factor's metrics only).  Three levels in fp64 (m = 16 CH + 37).
    Measured worst on an MI355X: fp64 5.5e-16 (graded, gram), fp32 4.0e-7 (repeated column, gram)."""
    ch, _ = qrh.cfg(fp32)
    m, D = (2 * ch + 37, 70) if fp32 else (16 * ch + 37, 70)
    ck = Checker("qrval[%s,%s]" % (kind, "f32" if fp32 else "f64"))
    check_harness_run(qrh, kind, make(kind, m, D, fp32, ch, seed=3), m, D, fp32, ck, rank_deficient=kind in ("dupcol", "zerocol"))
    ck.done()


@pytest.mark.parametrize("hw", [0, 1, 2])
def test_qr_scale_up_under_every_sqrt_flavour(qrh, gpu_ok, hw):
    """The fp32 scale-up case under each BA_QR_HW_SQRT flavour of the reflector's square root (ba_qr_sqrt: 0 the default, v_sqrt_f32
    + one Newton step; 1 the bare instruction; 2 IEEE sqrtf)."""
    ch, _ = qrh.cfg(1)
    m, D = 2 * ch + 37, 70
    ck = Checker("qrsqrt[%d]" % hw)
    check_harness_run(qrh, "tiny-hw%d" % hw, make("tiny", m, D, 1, ch, seed=3), m, D, 1, ck, hw_sqrt=hw)
    ck.done()


# ---- non-finite input -----------------------------------------------------------------------------------------------------------
NONFINITE = [(fp32, v, where) for fp32 in (0, 1) for v in ("nan", "inf")
             for where in ("A:0,0", "A:alone,0", "A:chunk2,5", "A:last", "A:deep,35", "A:above,20", "b:0", "b:last", "b:chunk2")]


@pytest.mark.parametrize("fp32,val,where", NONFINITE, ids=["%s-%s-%s" % ("f32" if f else "f64", v, w) for f, v, w in NONFINITE])
def test_qr_nonfinite_input_gives_nonfinite_step(qrh, gpu_ok, fp32, val, where):
    """A NaN or an Inf anywhere in A or b -- pivot, below a pivot in another chunk, the last row of the last column, a deep row of the
    second panel, above the diagonal, the right-hand side -- must leave y non-finite: the LM control rejects a trial only through
    non-finite scalars, and a finite step from such input would be accepted.  (k_qr_chunk: a non-finite column norm takes the identity
    reflector; a NaN or an Inf below the pivot reaches y through the 0 x NaN / 0 x Inf of the stored reflector and its T factor.  An
    Inf pivot left R_jj = Inf and y_j = 0 with every other entry finite, in both precisions, until k_qr_backsolve turned an infinite
    R_jj into a NaN.)"""
    ch, _ = qrh.cfg(fp32)
    m, D = 2 * ch + 37, 40
    Ab = make("gauss", m, D, fp32, ch, seed=5)
    x = np.nan if val == "nan" else np.inf
    col, row = {"A:0,0": (0, 0), "A:chunk2,5": (5, ch + 3), "A:last": (D - 1, m - 1), "A:deep,35": (35, ch + 100),
                "A:above,20": (20, 2), "A:alone,0": (0, 0), "b:0": (D, 0), "b:last": (D, m - 1), "b:chunk2": (D, ch + 7)}[where]
    if where == "A:alone,0":  # column 0 zero below its pivot: no norm is formed at all
        Ab[0, 1:] = 0
        col, row = 0, 0
    Ab[col, row] = x
    r = qrh.run(Ab, m, D, fp32)
    assert r["rc"] == 0 and r["guards"].all(), r["rc"]
    print("STAGE qrnan[%s,%s,%s] finite_y %d of %d" % ("f32" if fp32 else "f64", val, where, np.isfinite(r["y"]).sum(), D))
    assert not np.all(np.isfinite(r["y"])), (fp32, val, where, r["y"])


# ---- side paths -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fp32", [0, 1], ids=["f64", "f32"])
def test_qr_streams_repeat_and_go(qrh, gpu_ok, fp32):
    """On a three-level tree (m = 16 CH + 1): one stream and two (the trailing updates beside the chunk chain) give the same bits, and
    so do two runs; ba_qr_factor behind a go word of 1 followed by the back substitution gives the same bits; behind a go word of 0
    (MOREQR's outer QR behind a rejected trial) every kernel returns at once: A, the T storage and y are left bit for bit."""
    ch, _ = qrh.cfg(fp32)
    m, D = 16 * ch + 1, 72
    Ab = make("graded", m, D, fp32, ch, seed=9)
    two = qrh.run(Ab, m, D, fp32, streams=2)
    for kw in (dict(streams=1), dict(streams=2), dict(streams=2, go=1), dict(streams=1, go=1)):
        r = qrh.run(Ab, m, D, fp32, **kw)
        assert r["rc"] == 0 and r["guards"].all(), kw
        for k in ("F", "y", "tau"):
            assert np.array_equal(r[k].view(np.uint8), two[k].view(np.uint8)), (kw, k)
    for streams in (1, 2):
        r = qrh.run(Ab, m, D, fp32, streams=streams, go=0)
        assert r["rc"] == 0 and r["guards"].all()
        assert np.array_equal(r["F"][:, :m].view(np.uint8), Ab.view(np.uint8)) and not np.any(r["F"][:, m:])
        assert QH.untouched(r["tau"]) and QH.untouched(r["y"])


# ---- k_qr_backsolve's dynamic LDS -----------------------------------------------------------------------------------------------
def backsolve_cases():
    return [(0, 4032), (0, 4033), (1, 12224), (1, 12225), (0, "max")]


@pytest.mark.parametrize("fp32,D", backsolve_cases(), ids=["%s-D%s" % ("f32" if f else "f64", d) for f, d in backsolve_cases()])
def test_qr_backsolve_lds(qrh, gpu_ok, fp32, D):
    """k_qr_backsolve requests sizeof(T) (D + 64 + 4096) bytes of dynamic LDS: D = 4032 / 4033 (fp64) and 12 224 / 12 225 (fp32) lie
    either side of 64 KiB; 'max' is the largest fp64 D whose request fits the device's limit per workgroup.  m = D + 40, gram in
    the probe form.  Every launch runs and is right on an MI355X (limit 160 KiB: 'max' = 16 320): tri fp64 4.9e-16, fp32 2.4e-7.
    Beyond the limit the solver refuses the symbol (test_cabi.py::test_dense_qr_refuses_a_D_beyond_the_backsolve_lds)."""
    if D == "max":
        _, lim = qrh.lds(fp32, 0)
        D = lim // 8 - 64 - 4096
    req, lim = qrh.lds(fp32, D)
    print("STAGE qrlds[%s,%d] request %d limit %d" % ("f32" if fp32 else "f64", D, req, lim))
    m = D + 40
    ck = Checker("qrlds[%s,%d]" % ("f32" if fp32 else "f64", D))
    Ab = make("gauss", m, D, fp32, qrh.cfg(fp32)[0], seed=11)
    r = check_harness_run(qrh, "D%d" % D, Ab, m, D, fp32, ck, probes=4)
    print("STAGE qrlds[%s,%d] ms %.1f" % ("f32" if fp32 else "f64", D, r["ms"]))
    ck.done()


# ---- the matrices the solver factors --------------------------------------------------------------------------------------------
def _getter(ba, s, what, n):
    out = np.empty(n)
    ba._chk(ba.lib().ba_solver_get(s._h, what, out.ctypes.data_as(C.c_void_p), n), "ba_solver_get(%d)" % what)
    return out


SOLVER_CASES = [("p21", 0, 0, "lam0"), ("p21", 0, 0, "10"), ("p39", 0, 0, "lam0"), ("p39", 0, 1, "lam0"),
                ("p21", 3, 0, "lam0"), ("p21", 3, 1, "lam0"), ("ragged", 4, 0, "lam0")]


@pytest.mark.parametrize("prob,kind,scalar,lam", SOLVER_CASES,
                         ids=["%s-%s-%s-%s" % (p, {0: "qrkit", 3: "moreqr", 4: "qrspqr"}[k], "f64" if s == 0 else "f32", l)
                              for p, k, s, l in SOLVER_CASES])
def test_solver_dense_qr(ba, gpu_ok, prob21, prob39, monkeypatch, prob, kind, scalar, lam):
    """The four metrics on the matrix a trial really factors: getter 15 (BA_DBG_QRCHECK: the copy taken in front of the solve),
    getter 16 (what the factorisation left), y = the camera step.  QRKIT (J2bot, 2K + 3M + D rows: problem-21 3 levels in both
    precisions, problem-39 4 levels in fp64 -- config 3's input through Bundle_Adjustment_QRKit -- and 3 in fp32), MOREQR's inner
    matrix (6M + 2D rows), QRSPQR on the ragged problem.  lambda0 = 1e-12 max diag J'J (MOREQR: 1e-6 sqrt of it), and 10."""
    monkeypatch.setenv("BA_DBG_QRCHECK", "1")
    monkeypatch.delenv("BA_MOREQR_QR", raising=False)
    pg = prob21 if prob == "p21" else prob39 if prob == "p39" else _ragged_problem(ba)
    s = ba.Solver(pg, kind, scalar)
    _, dmax = s.linearize()
    lv = 10.0 if lam == "10" else (1e-6 * np.sqrt(dmax) if kind == ba.MOREQR else 1e-12 * dmax)
    s.try_step(lv)
    D = pg.D
    m = 6 * s.Ml + 2 * D if kind == ba.MOREQR else 2 * s.Kl + 3 * s.Ml + D
    A = _getter(ba, s, 15, m * (D + 1)).reshape(D + 1, m)
    F = _getter(ba, s, 16, m * (D + 1)).reshape(D + 1, m)
    y = s.get(ba.GET_DX)[3 * s.Ml:]
    del s
    ch = 1024 if scalar else 512
    name = "%s,%d,%s,%s" % (prob, kind, "f64" if scalar == 0 else "f32", lam)
    print("STAGE solverqr[%s] rows %d D %d levels %d" % (name, m, D, _depth(m, 0, ch)))
    ck = Checker("solverqr[%s]" % name)
    met = SC.qr_metrics(A, F, m, D, y, probes=4 if m * D * D > PROBE_ABOVE else 0)
    for k, v in met.items():
        ck(k, v, BOUND[(k, scalar)])
    ck.done()
