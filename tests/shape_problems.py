"""Problems whose tracks and camera pairs have chosen sizes -- TEST INFRASTRUCTURE ONLY (tests/test_shape_problems_cpu.py,
tests/test_gpu_shapes.py, tests/test_gpu_record_paths.py).

The kernels between the linearisation and the dense solve switch code path on two integers per item: the observations of a point
(k_elim_chol, k_elim_qr<LPP, SL> per track-length bucket, k_more_trial, k_backsub<8>, the point-aligned ranges of the fused
linearisation) and the entries of a camera pair (k_schur_pairs: batches of eight from two register sets, the direct write of a
single-chunk pair against the slab and k_schur_reduce).  A design here names those integers; build() makes the problem and structure()
recounts them from the arrays that were emitted, under the rule of ba_build_structure (csrc/ba_structure.cpp), so that every design
asserts that its shapes are really there.

Geometry and measurements come from ba.Problem.synthetic(N, M, M N, seed): every camera sees every point there, a pool with one valid
measurement per (camera, point).  A design is a list of tracks -- per point, in point order, the cameras that observe it; a camera named
again in a track is a copy of its observation with seeded pixel noise (as test_gpu_parity._long_track_problem does).  Every measurement is
then pulled to within 0.7 ... 0.95 tau of the start state's projection (_pull_in says why: beyond the robust kernel's tau = 0.5 px an
observation's block has rank one, and a lost entry of a designed pair could not be seen).  Output is sorted by point.
"""
import numpy as np

import oracle_lib as O

CHUNK, DCHUNK = 64, 32            # entries per chunk of a camera pair, observations per chunk of a camera (ba_shard_plan)
QR_BUCKETS = (32, 64, 128, 256)   # k_elim_qr: <= 32, <= 64, <= 128, <= 256, the rest (<= 1024)
RANGE = 256                       # a point-aligned range of the fused linearisation (ba_plan_eval_ranges)

PAIR_COUNTS = (1, 2, 3, 4, 5, 6, 7, 8, 9, 12, 13, 16, 17, 63, 64, 65, 127, 128, 129)
TRACK_LENGTHS = (1, 2, 3, 7, 8, 9, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256)


# ---- the structure rule, restated ----------------------------------------------------------------------------------------------------
def structure(N, M, cam_idx, pt_idx):
    """What ba_build_structure counts, from the arrays alone (observations sorted by point).

    A point's observations i' <= i give one entry to the pair (max cam, min cam); two different observations of one camera give two
    entries on the diagonal pair.  With n_jc = the observations of point j by camera c that is n_ja n_jb entries of point j on a pair
    a > b, and n_jc self entries + 2 n_jc (n_jc - 1) / 2 = n_jc^2 on the diagonal pair of c: entries = the lower triangle of C'C,
    C = (n_jc).  Returns a dict:
      entries [N, N] (lower triangle, a >= b), E, pair_chunks [N, N], nchunks, npairs = N (N + 1) / 2,
      cam_obs [N], cam_chunks [N], track [M], bucket [M] (0 ... 4), kmax, eval_ranges (the boundaries of ba_plan_eval_ranges, [] beyond
      256 observations of one point), multiplicity_max (the most observations of one point by one camera)."""
    cam_idx, pt_idx = np.asarray(cam_idx), np.asarray(pt_idx)
    assert np.all(np.diff(pt_idx) >= 0), "observations must be sorted by point"
    C = np.zeros((M, N))
    np.add.at(C, (pt_idx, cam_idx), 1.0)
    G = np.rint(C.T @ C).astype(np.int64)  # (exact: every sum is far below 2^53)
    entries = np.tril(G)
    pair_chunks = (entries + CHUNK - 1) // CHUNK
    cam_obs = np.bincount(cam_idx, minlength=N)
    track = np.bincount(pt_idx, minlength=M)
    kmax = int(track.max()) if M else 0
    ranges = []
    if kmax <= RANGE and len(cam_idx):
        ranges, fill, start = [0], 0, np.concatenate([[0], np.cumsum(track)])
        for j in range(M):
            if fill + track[j] > RANGE:
                ranges.append(int(start[j]))
                fill = 0
            fill += int(track[j])
        ranges.append(len(cam_idx))
    return dict(entries=entries, E=int(entries.sum()), pair_chunks=pair_chunks, nchunks=int(pair_chunks.sum()), npairs=N * (N + 1) // 2,
                cam_obs=cam_obs, cam_chunks=(cam_obs + DCHUNK - 1) // DCHUNK, track=track,
                bucket=np.searchsorted(np.array(QR_BUCKETS), track, side="left"), kmax=kmax, eval_ranges=ranges,
                multiplicity_max=int(C.max()) if C.size else 0)


def bucket_lengths(facts, b):
    """the sorted track lengths in k_elim_qr's bucket b"""
    return sorted(int(k) for k in facts["track"][facts["bucket"] == b])


def connected(entries):
    """whether the cameras form one component under 'share a point'"""
    A = (entries + entries.T) > 0
    seen = np.zeros(len(A), bool)
    seen[0] = True
    todo = [0]
    while todo:
        nxt = np.nonzero(A[todo.pop()] & ~seen)[0]
        seen[nxt] = True
        todo.extend(int(c) for c in nxt)
    return bool(seen.all())


# ---- the builder -------------------------------------------------------------------------------------------------------------------
TAU = 0.5              # pixels: the reference's robust kernel (oracle_lib.residuals)
PULL = (0.70, 0.95)    # of tau


def _pull_in(N, M, cam_idx, pt_idx, meas, cams9, pts, rng):
    """The measurements pulled towards the projection q of the start state until they are within tau x U(PULL) pixels of it (the
    direction of meas - q kept).  At the pool's own start nine observations in ten lie beyond tau = 0.5 px of the reference's robust kernel,
    and after sixteen LM trials still more than half (measured with the oracle): there the kernel's weight is zero and the observation's
    2 x 12 Jacobian block has rank one.  A point seen by two such observations constrains no camera -- its entries of S are of order
    lambda / V, 1e-12 of the diagonal at lambda0 -- so an entry of a designed pair could be lost without any metric moving.  Within 0.95 tau the weight 1 - r^2 / tau^2 is >= 0.0975: the block's radial row weighs
    1 / 7 of its tangential row at the worst, 0.8 at 0.7 tau -- full rank, and every entry of a pair carries its share of the pair's block.
    Not closer than 0.7 tau where it can be helped: a residual is the difference of pixel coordinates of ~1e3, so the energy of small
    residuals is a cancelling sum, relative error ~ (1 - x) / (r (2 - x)) eps |q|, x = r^2 / tau^2, per observation, and the energy bounds
    of BOUND (tests/test_gpu_stages.py) were set on problems whose observations mostly lie beyond tau, where an observation's energy is
    the constant tau^2 / 4; at 0.7 ... 0.95 tau that factor is eight times smaller than within 0.2 px.  q comes from the oracle's own projection: its residual with zero measurements
    and tau out of reach is q / sqrt(2)."""
    po = O.Problem(N, M, len(cam_idx), cam_idx, pt_idx, np.zeros(2 * len(cam_idx)), cams9, pts)
    f, _ = O.residuals(po, O.init_cams(po), po.pts, tau=1e12)
    q = np.sqrt(2.0) * f.reshape(-1, 2)
    r = meas - q
    nr = np.linalg.norm(r, axis=1)
    want = np.minimum(nr, TAU * rng.uniform(PULL[0], PULL[1], len(nr)))
    return q + r * (want / np.where(nr > 0, nr, 1.0))[:, None]


def build(ba, N, tracks, seed):
    """(problem, facts, obs_of): the problem of the tracks (a list of camera lists, one per point), structure() of what was emitted, and
    obs_of[j] = the index of point j's first observation in the output."""
    M = len(tracks)
    pool = ba.Problem.synthetic(N, M, M * N, seed)
    a = pool.arrays()
    assert np.array_equal(a["pt_idx"], np.repeat(np.arange(M), N)) and np.array_equal(a["cam_idx"], np.tile(np.arange(N), M))
    meas = a["meas"].reshape(M, N, 2)
    rng = np.random.default_rng(seed)
    length = np.array([len(t) for t in tracks])
    pt_idx = np.repeat(np.arange(M), length).astype(np.int32)
    cam_idx = np.concatenate([np.asarray(t, np.int32) for t in tracks])
    out = meas[pt_idx, cam_idx].copy()
    # a camera named again in a track: its observation + seeded pixel noise
    again = np.zeros(len(cam_idx), bool)
    key = pt_idx.astype(np.int64) * N + cam_idx
    _, first = np.unique(key, return_index=True)
    again[:] = True
    again[first] = False
    out[again] += rng.normal(0, 0.3, (int(again.sum()), 2))
    out = _pull_in(N, M, cam_idx, pt_idx, out, a["cams9"], a["pts"], rng)
    p = ba.Problem.from_arrays(N, M, len(cam_idx), cam_idx, pt_idx, out.ravel(), a["cams9"], a["pts"])
    e = p.arrays()
    po = O.Problem(N, M, p.K, e["cam_idx"], e["pt_idx"], e["meas"], e["cams9"], e["pts"])
    f, _ = O.residuals(po, O.init_cams(po), po.pts)
    f = np.linalg.norm(f.reshape(-1, 2), axis=1)  # sqrt(psi(r^2)), psi = r^2 (2 - r^2 / tau^2) / 4: 0.2488 at 0.95 tau, 0.25 from tau on
    assert 0 < f.min() and f.max() < 0.2489, (f.min(), f.max())
    facts = structure(N, M, e["cam_idx"], e["pt_idx"])
    assert tuple(facts["track"]) == tuple(length)
    assert connected(facts["entries"]) and facts["cam_obs"].min() >= 8, facts["cam_obs"]
    return p, facts, np.concatenate([[0], np.cumsum(length)])[:-1]


def _background(rng, cams, n):
    """n tracks of 3 ... 5 different cameras of `cams`"""
    return [sorted(int(c) for c in rng.choice(cams, int(rng.integers(3, 6)), replace=False)) for _ in range(n)]


def _long_track(rng, N, k):
    """k observations over N cameras: every camera before any is named again"""
    return [int(c) for c in np.concatenate([rng.permutation(N) for _ in range((k + N - 1) // N)])[:k]]


def _shuffled(rng, tracks):
    return [tracks[i] for i in rng.permutation(len(tracks))]


# ---- the designs ---------------------------------------------------------------------------------------------------------------------
def pairs(ba):
    """38 cameras; pair (2 q + 1, 2 q) shares exactly PAIR_COUNTS[q] points, each seen by these two cameras only: one batch of k_schur_pairs
    (n = 1 ... 8), a second batch of one entry (9), 12 / 13 and 16 / 17 (the shadow entry n - 1 at n = 1 mod 4 and mod 8), 63 / 64 / 65 (the
    pair stops being a single chunk: direct write against slab + k_schur_reduce), 127 / 128 / 129 (two full chunks, a third of one
    entry).  Background tracks of 3 ... 5 cameras of equal parity connect the cameras and never hold both cameras of a designed pair; one
    of the form (a, a, b) puts a non-self entry on a diagonal pair.  facts["designed"][q] = the points of pair q, in point order."""
    N, seed = 38, 3801
    rng = np.random.default_rng(seed)
    tracks = [[2 * q + 1, 2 * q] for q, n in enumerate(PAIR_COUNTS) for _ in range(n)]
    tracks += _background(rng, np.arange(0, N, 2), 260) + _background(rng, np.arange(1, N, 2), 260)
    tracks = _shuffled(rng, tracks) + [[4, 4, 10]]
    p, facts, first = build(ba, N, tracks, seed)
    ent, chunks = facts["entries"], facts["pair_chunks"]
    assert tuple(int(ent[2 * q + 1, 2 * q]) for q in range(len(PAIR_COUNTS))) == PAIR_COUNTS
    assert all(int(chunks[2 * q + 1, 2 * q]) == (1 if n <= 64 else 2 if n <= 128 else 3) for q, n in enumerate(PAIR_COUNTS))
    odd_even = ent[1::2, 0::2]  # (row 2 q + 1, column 2 q'): only q = q' is designed, q' <= q in the lower triangle
    assert np.count_nonzero(odd_even) == len(PAIR_COUNTS) and int((np.tril(np.ones_like(ent)) * (ent == 0)).sum()) > 0
    assert facts["multiplicity_max"] == 2 and ent[4, 4] == facts["cam_obs"][4] + 2  # the two non-self entries of (a, a, b)
    assert facts["kmax"] == 5
    facts["designed"] = {q: [j for j, t in enumerate(tracks) if t == [2 * q + 1, 2 * q]] for q in range(len(PAIR_COUNTS))}
    facts["first_obs"] = first
    return p, facts


def _tracks256(rng, N):
    t = {k: _long_track(rng, N, k) for k in TRACK_LENGTHS}
    bg = _background(rng, np.arange(N), 300)
    # a range of exactly 256 observations from two tracks; a track that fills a range alone; 127 + 128 + 2 = 257: the range splits
    # in front of the 2-track
    head = [t[255], t[1], t[256], t[127], t[128], t[2]]
    rest = _shuffled(rng, [t[k] for k in TRACK_LENGTHS if k not in (255, 1, 256, 127, 128, 2)] + bg)
    return head + rest


def _assert_tracks(facts, extra=()):
    track = facts["track"]
    want = sorted(k for k in TRACK_LENGTHS + tuple(extra) if k != 3)  # (3: the designed point and background tracks)
    assert sorted(int(k) for k in track if k > 5 or k < 3) == want and np.count_nonzero(track == 3) >= 1, sorted(track)
    assert bucket_lengths(facts, 1) == [33, 63, 64] and bucket_lengths(facts, 2) == [65, 127, 128]
    assert bucket_lengths(facts, 3) == [129, 255, 256] and bucket_lengths(facts, 4) == sorted(extra)
    assert [k for k in bucket_lengths(facts, 0) if k > 5 or k < 3] == [1, 2, 7, 8, 9, 31, 32]
    assert tuple(track[:6]) == (255, 1, 256, 127, 128, 2)


def tracks256(ba):
    """40 cameras; one point each of TRACK_LENGTHS observations (a camera again and again beyond 40) next to background tracks of 3 ... 5:
    1, 2, 3, 7, 8, 9 the edges of k_backsub<8>'s stride; 31 ... 257 the last slot of a lane of k_elim_qr just filled or just empty on both
    sides of every bucket boundary.  Points 0 - 1 (255 + 1) fill a point-aligned range of 256 exactly, point 2 (256) fills one alone,
    points 3 - 5 (127 + 128 + 2 = 257) split one."""
    N, seed = 40, 4001
    p, facts, first = build(ba, N, _tracks256(np.random.default_rng(seed), N), seed)
    _assert_tracks(facts)
    assert facts["kmax"] == 256 and facts["eval_ranges"][:4] == [0, 256, 512, 767], facts["eval_ranges"][:5]
    facts["first_obs"] = first
    return p, facts


def tracks257(ba):
    """tracks256 and one point of 257 observations: kmax = 257, no point-aligned ranges (the separate launches), k_elim_qr's last bucket."""
    N, seed = 40, 4001
    rng = np.random.default_rng(seed)
    tracks = _tracks256(rng, N)
    tracks.append(_long_track(rng, N, 257))
    p, facts, first = build(ba, N, tracks, seed)
    _assert_tracks(facts, extra=(257,))
    assert facts["kmax"] == 257 and facts["eval_ranges"] == []
    facts["first_obs"] = first
    return p, facts


def _one_long(ba, k, seed):
    N = 40
    rng = np.random.default_rng(seed)
    tracks = _shuffled(rng, _background(rng, np.arange(N), 300) + [_long_track(rng, N, k)])
    p, facts, first = build(ba, N, tracks, seed)
    assert facts["kmax"] == k and bucket_lengths(facts, 4) == [k] and sum(len(bucket_lengths(facts, b)) for b in (1, 2, 3)) == 0
    facts["first_obs"] = first
    return p, facts


def track1024(ba):
    """one point of 1024 observations (the most k_elim_qr<64, 16> takes: every slot of every lane full) next to background tracks"""
    return _one_long(ba, 1024, 1024)


def track1025(ba):
    """one point of 1025 observations: refused by the QR eliminations, accepted by CHOLESKY"""
    return _one_long(ba, 1025, 1025)


def walk(ba):
    """96 cameras; every camera pair shares at least one point of its own (seen by these two cameras only), every seventh pair 2 ... 70 of
    them: >= 4560 off-diagonal chunks of mixed size next to the diagonal pairs' -- more than 12 per workgroup of a grid of one workgroup
    per CU, so that wavefronts of the persistent pair kernel walk lists of three chunks and more."""
    N, seed = 96, 9601
    rng = np.random.default_rng(seed)
    tracks, q = [], 0
    for a in range(N):
        for b in range(a):
            n = 2 + (q // 7) % 69 if q % 7 == 0 else 1
            tracks += [[b, a]] * n
            q += 1
    p, facts, first = build(ba, N, _shuffled(rng, tracks), seed)
    off = np.tril(facts["pair_chunks"], -1)
    ent = np.tril(facts["entries"], -1)
    assert np.count_nonzero(np.tril(np.ones((N, N)), -1) * (ent == 0)) == 0 and ent.max() == 70 and int(off.sum()) >= 4560
    assert sorted(set(int(v) for v in ent[np.tril_indices(N, -1)])) == list(range(1, 71))
    assert facts["nchunks"] >= 12 * 256
    facts["first_obs"] = first
    return p, facts


DESIGNS = dict(pairs=pairs, tracks256=tracks256, tracks257=tracks257, track1024=track1024, track1025=track1025, walk=walk)
_BUILT = {}


def get(ba, name):
    """(problem, facts) of a design, built once per process"""
    if name not in _BUILT:
        _BUILT[name] = DESIGNS[name](ba)
    return _BUILT[name]
