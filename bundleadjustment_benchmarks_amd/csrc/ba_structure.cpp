// ba_structure.cpp -- static (iteration-independent) structure of one shard: point-sorted observation order,
// shard boundaries, camera-pair entry lists and their chunking.  Host code, runs once per solver.
//
// What it replaces in the reference: the sparsity bookkeeping Eigen does on every call -- setFromTriplets of 24K
// triplets per outer iteration (src/Optimization/BAFunctor.cpp:95-98), the per-trial row permutation of
// [J; sqrt(lambda) I] (src/Eigen_ext/BacktrackLevMarqQRChol.h:291-315) and the symbolic analysis inside
// SimplicialLDLT::compute (src/Eigen_ext/BacktrackLevMarqCholesky.h:278).  The pattern never changes, so it is
// built once.
#include "ba_internal.h"

#include <algorithm>
#include <new>
#include <numeric>
#include <utility>

int ba_build_structure(const ba_problem *p, int shard_rank, int shard_world, int chunk_len, int dchunk_len, ba_structure *s, bool pairs)
{
    if (!p || !s || shard_world < 1 || shard_rank < 0 || shard_rank >= shard_world || chunk_len < 1 || dchunk_len < 1) return BA_ERR_ARG;
    const int N = p->N, M = p->M, K = p->K;
    s->N = N; s->M = M; s->K = K; s->chunk_len = chunk_len;

    // 1. stable sort of the observations by point (counting sort); BAL files are already sorted.
    s->was_sorted = true;
    for (int i = 1; i < K; i++)
        if (p->pt_idx[i] < p->pt_idx[i - 1]) { s->was_sorted = false; break; }
    std::vector<int> gptr((size_t)M + 1, 0);
    for (int i = 0; i < K; i++) gptr[(size_t)p->pt_idx[i] + 1]++;
    for (int j = 0; j < M; j++) gptr[j + 1] += gptr[j];
    s->perm.resize(K);
    if (s->was_sorted) {
        std::iota(s->perm.begin(), s->perm.end(), 0);
    } else {
        std::vector<int> cur(gptr.begin(), gptr.end() - 1);
        for (int i = 0; i < K; i++) s->perm[cur[p->pt_idx[i]]++] = i;
    }

    // 2. shard boundaries: contiguous point ranges balanced by observation count.
    auto boundary = [&](int r) -> int {
        if (r <= 0) return 0;
        if (r >= shard_world) return M;
        const long long target = (long long)K * r / shard_world;
        int j = (int)(std::lower_bound(gptr.begin(), gptr.end(), (int)target) - gptr.begin());
        return std::min(j, M);
    };
    s->p0 = boundary(shard_rank);
    s->p1 = boundary(shard_rank + 1);
    s->o0 = gptr[s->p0];
    s->o1 = gptr[s->p1];
    s->Ml = s->p1 - s->p0;
    s->Kl = s->o1 - s->o0;
    const int Ml = s->Ml, Kl = s->Kl;
    s->obs_cam.resize(Kl);
    s->obs_pt.resize(Kl);
    s->pt_ptr.resize((size_t)Ml + 1);
    for (int j = 0; j <= Ml; j++) s->pt_ptr[j] = gptr[s->p0 + j] - s->o0;
    s->kmax = 0;
    for (int j = 0; j < Ml; j++) s->kmax = std::max(s->kmax, s->pt_ptr[j + 1] - s->pt_ptr[j]);
    {
        auto bucket = [](int k) { return k <= 32 ? 0 : k <= 64 ? 1 : k <= 128 ? 2 : k <= 256 ? 3 : 4; };
        int cnt[5] = {0, 0, 0, 0, 0};
        for (int j = 0; j < Ml; j++) cnt[bucket(s->pt_ptr[j + 1] - s->pt_ptr[j])]++;
        s->qr_bucket_ptr[0] = 0;
        for (int b = 0; b < 5; b++) s->qr_bucket_ptr[b + 1] = s->qr_bucket_ptr[b] + cnt[b];
        int cur[5];
        for (int b = 0; b < 5; b++) cur[b] = s->qr_bucket_ptr[b];
        s->qr_pts.resize(Ml);
        for (int j = 0; j < Ml; j++) s->qr_pts[cur[bucket(s->pt_ptr[j + 1] - s->pt_ptr[j])]++] = j;
    }
    for (int i = 0; i < Kl; i++) {
        const int src = s->perm[s->o0 + i];
        s->obs_cam[i] = p->cam_idx[src];
        s->obs_pt[i] = p->pt_idx[src] - s->p0;
    }

    // 3. camera pairs (hi >= lo), pair id = hi (hi + 1) / 2 + lo.
    if (pairs) {
        const long long np = (long long)N * (N + 1) / 2;
        if (np > 0x7fffffffLL) return BA_ERR_ARG;
        s->npairs = (int)np;
        s->pair_hi.resize(np);
        s->pair_lo.resize(np);
        for (int hi = 0, q = 0; hi < N; hi++)
            for (int lo = 0; lo <= hi; lo++, q++) { s->pair_hi[q] = hi; s->pair_lo[q] = lo; }
        auto pid = [](int a, int b) -> long long {
            const int hi = std::max(a, b), lo = std::min(a, b);
            return (long long)hi * (hi + 1) / 2 + lo;
        };
        // count entries per pair.  For one point with observations i < i': entry (row = the one with the larger camera).
        // Two observations of the SAME camera in one point (not in BAL data, allowed) give both orders on the diagonal pair.
        std::vector<long long> pcount((size_t)np + 1, 0);
        for (int j = 0; j < Ml; j++) {
            const int b = s->pt_ptr[j], e = s->pt_ptr[j + 1];
            for (int i = b; i < e; i++)
                for (int i2 = b; i2 <= i; i2++) {
                    const long long q = pid(s->obs_cam[i], s->obs_cam[i2]);
                    pcount[q + 1] += (i != i2 && s->obs_cam[i] == s->obs_cam[i2]) ? 2 : 1;
                }
        }
        for (long long q = 0; q < np; q++) pcount[q + 1] += pcount[q];
        s->E = pcount[np];
        if (s->E > 0x7fffffffLL) return BA_ERR_NOMEM;
        s->ent_r.resize((size_t)s->E);
        s->ent_c.resize((size_t)s->E);
        {
            std::vector<long long> cur(pcount.begin(), pcount.end() - 1);
            for (int j = 0; j < Ml; j++) { // increasing point order inside each pair: fixed summation order
                const int b = s->pt_ptr[j], e = s->pt_ptr[j + 1];
                for (int i = b; i < e; i++)
                    for (int i2 = b; i2 <= i; i2++) {
                        const int ca = s->obs_cam[i], cb = s->obs_cam[i2];
                        const long long q = pid(ca, cb);
                        if (ca >= cb) { s->ent_r[cur[q]] = i; s->ent_c[cur[q]] = i2; cur[q]++; }
                        else { s->ent_r[cur[q]] = i2; s->ent_c[cur[q]] = i; cur[q]++; }
                        if (i != i2 && ca == cb) { s->ent_r[cur[q]] = i2; s->ent_c[cur[q]] = i; cur[q]++; }
                    }
            }
        }
        // 4. chunks
        s->pair_chunk_ptr.assign((size_t)np + 1, 0);
        s->chunk_ptr.clear();
        s->chunk_pair.clear();
        for (long long q = 0; q < np; q++) {
            for (long long b = pcount[q]; b < pcount[q + 1]; b += chunk_len) {
                s->chunk_ptr.push_back((int)b);
                s->chunk_pair.push_back((int)q);
            }
            s->pair_chunk_ptr[q + 1] = (int)s->chunk_ptr.size();
        }
        s->nchunks = (int)s->chunk_pair.size();
        s->chunk_ptr.push_back((int)s->E);
    } // pairs

    // 5. camera-sorted view of the observations (= self entries of the diagonal pairs), in chunks of dchunk_len.
    std::vector<int> cptr((size_t)N + 1, 0);
    for (int i = 0; i < Kl; i++) cptr[(size_t)s->obs_cam[i] + 1]++;
    for (int c = 0; c < N; c++) cptr[c + 1] += cptr[c];
    s->cam_obs.resize(Kl);
    {
        std::vector<int> cur(cptr.begin(), cptr.end() - 1);
        for (int i = 0; i < Kl; i++) s->cam_obs[cur[s->obs_cam[i]]++] = i;
    }
    s->cam_dchunk_ptr.assign((size_t)N + 1, 0);
    s->dchunk_ptr.clear();
    s->dchunk_cam.clear();
    for (int c = 0; c < N; c++) {
        for (int b = cptr[c]; b < cptr[c + 1]; b += dchunk_len) {
            s->dchunk_ptr.push_back(b);
            s->dchunk_cam.push_back(c);
        }
        s->cam_dchunk_ptr[c + 1] = (int)s->dchunk_cam.size();
    }
    s->ndchunks = (int)s->dchunk_cam.size();
    s->dchunk_ptr.push_back(Kl);
    return BA_OK;
}

extern "C" int ba_shard_plan(const ba_problem *p, int shard_rank, int shard_world, long long *out8)
{
    if (!p || !out8) return BA_ERR_ARG;
    ba_structure s;
    int rc = ba_build_structure(p, shard_rank, shard_world, 64, 32, &s);
    if (rc) return rc;
    out8[0] = s.p0; out8[1] = s.p1; out8[2] = s.o0; out8[3] = s.o1; out8[4] = s.E; out8[5] = s.nchunks; out8[6] = s.npairs;
    out8[7] = s.was_sorted ? 1 : 0;
    return BA_OK;
}

// The spanning forest of the constraint graph behind BA_PRECOND_CONSTRAINT_FOREST (ba_mi355x.h states the rule; the solver builds its
// device lists from these four arrays, tests/forest_checks.py restates it).
extern "C" int ba_relpose_forest_plan(int N, int n, const int *cam_pairs, int max_tree, int *parent, int *via, int *order, unsigned char *kept)
{
    if (N < 0 || n < 0 || max_tree < 1 || (N > 0 && (!parent || !via || !order)) || (n > 0 && (!cam_pairs || !kept))) return BA_ERR_ARG;
    for (int q = 0; q < n; q++) {
        const int a = cam_pairs[2 * q], b = cam_pairs[2 * q + 1];
        if (a < 0 || b < 0 || a >= N || b >= N || a == b) return BA_ERR_ARG;
    }
    std::vector<int> uf((size_t)N), size((size_t)N, 1), deg((size_t)N + 1, 0);
    std::iota(uf.begin(), uf.end(), 0);
    auto find = [&](int x) {
        while (uf[x] != x) { uf[x] = uf[uf[x]]; x = uf[x]; }
        return x;
    };
    for (int q = 0; q < n; q++) {
        const int ra = find(cam_pairs[2 * q]), rb = find(cam_pairs[2 * q + 1]);
        kept[q] = ra != rb && size[ra] + size[rb] <= max_tree;
        if (!kept[q]) continue;
        const int lo = std::min(ra, rb), hi = std::max(ra, rb); // (the representative is the component's lowest camera: its root)
        uf[hi] = lo;
        size[lo] += size[hi];
        deg[cam_pairs[2 * q] + 1]++; deg[cam_pairs[2 * q + 1] + 1]++;
    }
    // adjacency of the kept edges, list order per camera
    for (int a = 0; a < N; a++) deg[a + 1] += deg[a];
    std::vector<int> adj((size_t)deg[N]), fill(deg.begin(), deg.end() - 1);
    for (int q = 0; q < n; q++)
        if (kept[q]) { adj[fill[cam_pairs[2 * q]]++] = q; adj[fill[cam_pairs[2 * q + 1]]++] = q; }
    for (int a = 0; a < N; a++) { parent[a] = -1; via[a] = -1; }
    std::vector<int> bfs;
    std::vector<unsigned char> seen((size_t)N, 0);
    int pos = 0;
    for (int root = 0; root < N; root++) { // ascending root: a camera not seen yet is the lowest of its component
        if (seen[root] || deg[root] == deg[root + 1]) continue;
        bfs.assign(1, root);
        seen[root] = 1;
        for (size_t h = 0; h < bfs.size(); h++) {
            const int c = bfs[h];
            for (int k = deg[c]; k < deg[c + 1]; k++) {
                const int q = adj[k], o = cam_pairs[2 * q] == c ? cam_pairs[2 * q + 1] : cam_pairs[2 * q];
                if (seen[o]) continue;
                seen[o] = 1; parent[o] = c; via[o] = q;
                bfs.push_back(o);
            }
        }
        for (size_t h = bfs.size(); h-- > 0;) order[pos++] = bfs[h];
    }
    for (int a = 0; a < N; a++)
        if (!seen[a]) order[pos++] = a;
    return BA_OK;
}

// The groups and chunks behind ba_solver_set_shared_intrinsics (ba_mi355x.h states the rule; the solver builds its device lists from
// these arrays, tests/shared_checks.py restates it).
extern "C" int ba_intrinsics_group_plan(int N, const int *group_of, int chunk, int *n_groups, int *group_ptr, int *members, int *n_chunks,
                                        int *chunk_ptr, int *chunk_group)
{
    if (N < 0 || (N > 0 && !group_of) || chunk < 1) return BA_ERR_ARG;
    try {
        // cameras by (label, index); a run of one label with two or more cameras is a group, the groups then by their lowest member
        std::vector<int> by((size_t)0);
        for (int a = 0; a < N; a++)
            if (group_of[a] >= 0) by.push_back(a);
        std::stable_sort(by.begin(), by.end(), [&](int u, int v) { return group_of[u] < group_of[v]; });
        std::vector<std::pair<int, int>> runs; // (first position in `by`, length), lowest member first inside a run
        for (size_t i = 0; i < by.size();) {
            size_t j = i;
            while (j < by.size() && group_of[by[j]] == group_of[by[i]]) j++;
            if (j - i >= 2) runs.emplace_back((int)i, (int)(j - i));
            i = j;
        }
        std::sort(runs.begin(), runs.end(), [&](const std::pair<int, int> &u, const std::pair<int, int> &v) { return by[u.first] < by[v.first]; });
        int ng = 0, nm = 0, nc = 0;
        for (const auto &r : runs) {
            if (group_ptr) group_ptr[ng] = nm;
            for (int k = 0; k < r.second; k += chunk) {
                if (chunk_ptr) chunk_ptr[nc] = nm + k;
                if (chunk_group) chunk_group[nc] = ng;
                nc++;
            }
            for (int k = 0; k < r.second; k++)
                if (members) members[nm + k] = by[(size_t)r.first + k];
            nm += r.second;
            ng++;
        }
        if (group_ptr) group_ptr[ng] = nm;
        if (chunk_ptr) chunk_ptr[nc] = nm;
        if (n_groups) *n_groups = ng;
        if (n_chunks) *n_chunks = nc;
    } catch (const std::bad_alloc &) {
        return BA_ERR_NOMEM;
    }
    return BA_OK;
}

// The co-visibility graph behind BA_PRECOND_VISIBILITY_FOREST (ba_mi355x.h states the rule, tests/visibility_checks.py restates it).
// Counts: dense N x N up to 2048 cameras; beyond that packed keys a N + b, sorted and run-length counted whenever 16 M of them have
// gathered, the runs merged into the sorted list so far -- memory follows the number of distinct pairs, not the number of points.
int ba_covisibility(int N, int M, const int *pt_ptr, const int *obs_cam, int track_max, std::vector<int> &pairs, std::vector<int> &weight)
{
    if (track_max == 0) track_max = BA_VIS_TRACK_MAX_DEFAULT;
    if (N < 0 || M < 0 || track_max < 0 || (M > 0 && (!pt_ptr || !obs_cam))) return BA_ERR_ARG;
    pairs.clear();
    weight.clear();
    const bool dense = N <= 2048;
    std::vector<int> cnt(dense ? (size_t)N * N : 0, 0);
    std::vector<long long> keys;
    std::vector<std::pair<long long, int>> acc, run, merged; // (key, count), key ascending
    auto flush = [&]() {
        std::sort(keys.begin(), keys.end());
        run.clear();
        for (size_t i = 0; i < keys.size();) {
            size_t j = i;
            while (j < keys.size() && keys[j] == keys[i]) j++;
            run.emplace_back(keys[i], (int)(j - i));
            i = j;
        }
        keys.clear();
        merged.clear();
        merged.reserve(acc.size() + run.size());
        size_t x = 0, y = 0;
        while (x < acc.size() || y < run.size()) {
            if (y == run.size() || (x < acc.size() && acc[x].first < run[y].first)) merged.push_back(acc[x++]);
            else if (x == acc.size() || run[y].first < acc[x].first) merged.push_back(run[y++]);
            else { merged.emplace_back(acc[x].first, acc[x].second + run[y].second); x++; y++; }
        }
        acc.swap(merged);
    };
    std::vector<int> cams;
    for (int j = 0; j < M; j++) {
        cams.assign(obs_cam + pt_ptr[j], obs_cam + pt_ptr[j + 1]);
        std::sort(cams.begin(), cams.end());
        cams.erase(std::unique(cams.begin(), cams.end()), cams.end());
        const int t = (int)cams.size();
        for (int i = 0; i + 1 < t; i++) {
            const int last = t <= track_max ? t - 1 : i + 1; // (a long track: the next camera alone)
            for (int k = i + 1; k <= last; k++) {
                if (dense) cnt[(size_t)cams[i] * N + cams[k]]++;
                else keys.push_back((long long)cams[i] * N + cams[k]);
            }
        }
        if (keys.size() >= ((size_t)1 << 24)) flush();
    }
    if (dense) {
        for (size_t q = 0; q < cnt.size(); q++)
            if (cnt[q]) acc.emplace_back((long long)q, cnt[q]);
    } else
        flush();
    std::stable_sort(acc.begin(), acc.end(), [](const std::pair<long long, int> &u, const std::pair<long long, int> &v) { return u.second > v.second; });
    pairs.reserve(2 * acc.size());
    weight.reserve(acc.size());
    for (const auto &kv : acc) {
        pairs.push_back((int)(kv.first / N));
        pairs.push_back((int)(kv.first % N));
        weight.push_back(kv.second);
    }
    return BA_OK;
}

extern "C" int ba_problem_covisibility(const ba_problem *p, int track_max, long long *n_pairs, int *pairs, int *weight)
{
    if (!p || !n_pairs || track_max < 0 || (pairs == nullptr) != (weight == nullptr)) return BA_ERR_ARG;
    try {
        std::vector<int> ptr((size_t)p->M + 1, 0), cam((size_t)p->K), hp, hw;
        for (int i = 0; i < p->K; i++) ptr[(size_t)p->pt_idx[i] + 1]++;
        for (int j = 0; j < p->M; j++) ptr[j + 1] += ptr[j];
        std::vector<int> cur(ptr.begin(), ptr.end() - 1);
        for (int i = 0; i < p->K; i++) cam[cur[p->pt_idx[i]]++] = p->cam_idx[i];
        const int rc = ba_covisibility(p->N, p->M, ptr.data(), cam.data(), track_max, hp, hw);
        if (rc) return rc;
        *n_pairs = (long long)hw.size();
        if (pairs) {
            std::copy(hp.begin(), hp.end(), pairs);
            std::copy(hw.begin(), hw.end(), weight);
        }
    } catch (const std::bad_alloc &) {
        return BA_ERR_NOMEM;
    }
    return BA_OK;
}
