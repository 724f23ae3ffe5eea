// ba_structure.cpp -- static (iteration-independent) structure of one shard: point-sorted observation order,
// shard boundaries, camera-pair entry lists and their chunking, and the plans of the index lists the kernels walk (ba_plan_*: the
// solver uploads them).  Host code without a HIP call, runs once per solver or setter; tests/plans_check.cpp checks the plans.
//
// What it replaces in the reference: the sparsity bookkeeping Eigen does on every call -- setFromTriplets of 24K
// triplets per outer iteration (src/Optimization/BAFunctor.cpp:95-98), the per-trial row permutation of
// [J; sqrt(lambda) I] (src/Eigen_ext/BacktrackLevMarqQRChol.h:291-315) and the symbolic analysis inside
// SimplicialLDLT::compute (src/Eigen_ext/BacktrackLevMarqCholesky.h:278).  The pattern never changes, so it is
// built once.
#include "ba_internal.h"

#include <algorithm>
#include <functional>
#include <new>
#include <numeric>
#include <queue>
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

// ---- the plans of the solver's device lists (ba_internal.h) ------------------------------------------------------------------------

void ba_plan_eval_ranges(const ba_structure &s, std::vector<int> &eb)
{
    eb.clear();
    if (s.kmax > 256 || s.Kl <= 0) return;
    eb.push_back(0);
    int fill = 0; // observations in the current range
    for (int j = 0; j < s.Ml; j++) {
        const int k = s.pt_ptr[j + 1] - s.pt_ptr[j];
        if (fill + k > 256) { eb.push_back(s.pt_ptr[j]); fill = 0; }
        fill += k;
    }
    eb.push_back(s.Kl);
}

// Chunks dealt to the wavefronts of the persistent pair kernel, longest first, always to the least loaded wavefront
// (cost = batches of eight entries + a constant per chunk); a wavefront's list is then walked in chunk order.
// Every wavefront of the persistent grid must be resident at once (the dealing assumes they run side by side): wgs_per_cu is the
// occupancy's answer.
void ba_plan_schur(const ba_structure &sx, int wgs_per_cu, int num_cus, int bands, int window, ba_schur_plan &out)
{
    out.grid = std::max(1, std::min((sx.nchunks + 3) / 4, wgs_per_cu * num_cus));
    const int nband = (bands > 1 && out.grid >= 8 * bands) ? bands : 1;
    out.grid = out.grid / nband * nband;
    out.nband = nband;
    const int W = 4 * out.grid, Wb = W / nband;
    std::vector<int> order((size_t)sx.nchunks), owner((size_t)sx.nchunks);
    std::vector<int> &wptr = out.wave_ptr;
    wptr.assign((size_t)W + 1, 0);
    auto cost = [&](int c) { return 2 * ((sx.chunk_ptr[c + 1] - sx.chunk_ptr[c] + 7) / 8) + 1; };
    // bands: the chunk list (sorted by row camera, column camera) cut into nband ranges of equal cost; the workgroups with
    // blockIdx % nband == b (one XCD under the observed round-robin placement) own range b.  Wavefront index: see k_schur_pairs.
    std::vector<int> bptr((size_t)nband + 1, sx.nchunks);
    {
        long long tot = 0, acc = 0;
        for (int c = 0; c < sx.nchunks; c++) tot += cost(c);
        bptr[0] = 0;
        for (int c = 0, b = 1; c < sx.nchunks && b < nband; c++) {
            acc += cost(c);
            while (b < nband && acc >= tot * b / nband) bptr[b++] = c + 1;
        }
    }
    // The dealing goes window by window through the band (`window` chunks per wavefront and window; 0 = the whole band
    // is one window): the loads carry over, so the balance is the same, but a wavefront's list now holds a few chunks of
    // EVERY window, i.e. all wavefronts of the band walk through the (row camera, column camera) order side by side and the
    // records of one row camera (its observations: ~1 MB at config 5) are in the XCD's L2 when the next column camera's
    // chunk asks for them.
    for (int b = 0; b < nband; b++) {
        typedef std::pair<long long, int> load_t; // (load, wavefront): min-heap
        std::priority_queue<load_t, std::vector<load_t>, std::greater<load_t>> heap;
        for (int w = 0; w < Wb; w++) heap.push(load_t(0, b * Wb + w));
        const int nb_ = bptr[b + 1] - bptr[b];
        const long long win = window > 0 ? (long long)window * Wb : (long long)std::max(nb_, 1);
        for (long long w0 = bptr[b]; w0 < bptr[b + 1]; w0 += win) {
            const int w1 = (int)std::min<long long>(w0 + win, bptr[b + 1]);
            order.assign(w1 - (int)w0, 0);
            std::iota(order.begin(), order.end(), (int)w0);
            std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return cost(x) > cost(y); });
            for (int c : order) {
                load_t t = heap.top();
                heap.pop();
                owner[c] = t.second;
                wptr[t.second + 1]++;
                heap.push(load_t(t.first + cost(c), t.second));
            }
        }
    }
    for (int w = 0; w < W; w++) wptr[w + 1] += wptr[w];
    out.chunk_info.assign(4 * (size_t)sx.nchunks, 0);
    {
        std::vector<int> cur(wptr.begin(), wptr.end() - 1);
        for (int c = 0; c < sx.nchunks; c++) { // increasing chunk id inside every wavefront's list
            const int q = sx.chunk_pair[c];
            // (a diagonal pair always goes through k_schur_reduce, which puts lambda on the diagonal when k_post_reduce is folded away)
            const bool single = sx.pair_chunk_ptr[q + 1] - sx.pair_chunk_ptr[q] == 1 && sx.pair_hi[q] != sx.pair_lo[q];
            int *ci = &out.chunk_info[4 * (size_t)cur[owner[c]]++];
            ci[0] = sx.chunk_ptr[c];
            ci[1] = (sx.chunk_ptr[c + 1] - sx.chunk_ptr[c]) | (single ? BA_CHUNK_SINGLE : 0);
            ci[2] = sx.pair_hi[q] | (sx.pair_lo[q] << 16);
            ci[3] = c;
        }
    }
    out.red_pairs.clear();
    for (int q = 0; q < sx.npairs; q++)
        if (sx.pair_chunk_ptr[q + 1] - sx.pair_chunk_ptr[q] != 1 || sx.pair_hi[q] == sx.pair_lo[q]) out.red_pairs.push_back(q);
    out.ent.resize(2 * (size_t)sx.E);
    for (long long e = 0; e < sx.E; e++) { // a self entry carries ~point in place of its column observation (k_schur_pairs)
        const int r_ = sx.ent_r[(size_t)e], c_ = sx.ent_c[(size_t)e];
        out.ent[2 * (size_t)e] = r_;
        out.ent[2 * (size_t)e + 1] = r_ == c_ ? ~sx.obs_pt[r_] : c_;
    }
}

int ba_plan_forest(const ba_structure &sx, const std::vector<int> &rp_pairs, int kind, int max_tree, ba_forest_plan &out)
{
    const int N = sx.N;
    const bool vis = kind == BA_PRECOND_VISIBILITY_FOREST;
    out = ba_forest_plan();
    std::vector<int> pairs(rp_pairs); // L
    if (vis) {
        std::vector<int> cp, cw;
        const int rc = ba_covisibility(N, sx.Ml, sx.pt_ptr.data(), sx.obs_cam.data(), 0, cp, cw);
        if (rc) return rc;
        if (pairs.size() / 2 + cp.size() / 2 > (size_t)0x7fffffff) return BA_ERR_NOMEM;
        pairs.insert(pairs.end(), cp.begin(), cp.end());
        out.width = 9;
    }
    const int n = (int)(pairs.size() / 2);
    out.dropped = n;
    out.largest = N > 0 ? 1 : 0;
    if (kind == BA_PRECOND_BLOCK_JACOBI || n == 0 || max_tree < 2) return BA_OK;
    std::vector<int> parent((size_t)N), via((size_t)N), order((size_t)N);
    std::vector<unsigned char> kept((size_t)n);
    const int rc = ba_relpose_forest_plan(N, n, pairs.data(), max_tree, parent.data(), via.data(), order.data(), kept.data());
    if (rc) return rc;
    for (int q = 0; q < n; q++) out.kept += kept[q];
    out.dropped = n - out.kept;
    if (out.kept == 0) return BA_OK;
    std::vector<unsigned char> &in_tree = out.in_tree;
    in_tree.assign((size_t)N, 0);
    for (int a = 0; a < N; a++)
        if (parent[a] >= 0) { in_tree[a] = 1; in_tree[parent[a]] = 1; }
    std::vector<int> pos((size_t)N, -1);
    std::vector<int> &tree_ptr = out.tree_ptr, &node_cam = out.node_cam, &node_par = out.node_par, &node_rec = out.node_rec;
    tree_ptr.assign(1, 0);
    for (int k = 0; k < N && in_tree[order[k]]; k++) pos[order[k]] = k; // (the lone cameras are last)
    for (int k = 0; k < N && in_tree[order[k]]; k++) {
        const int c = order[k];
        node_cam.push_back(c);
        node_par.push_back(parent[c] >= 0 ? pos[parent[c]] : -1);
        // (a kept co-visibility edge has no constraint on its pair: that one came first in L and would have been kept instead)
        node_rec.push_back(parent[c] >= 0 && 2 * (size_t)via[c] < rp_pairs.size() ? 2 * via[c] + (pairs[2 * (size_t)via[c]] == c ? 0 : 1) : -1);
        if (parent[c] < 0) { // the root ends its tree
            out.largest = std::max(out.largest, k + 1 - tree_ptr.back());
            tree_ptr.push_back(k + 1);
        }
    }
    out.ntrees = (int)tree_ptr.size() - 1;
    out.nodes = (int)node_cam.size();
    if (vis) { // per node the record pairs (o of the node, o' of its parent) of their common points: ascending point, then observation order
        std::vector<int> cptr((size_t)N + 1, 0);
        std::vector<int> &edge_ptr = out.edge_ptr, &edge_oo = out.edge_oo;
        edge_ptr.assign(1, 0);
        for (int i = 0; i < sx.Kl; i++) cptr[(size_t)sx.obs_cam[i] + 1]++;
        for (int a = 0; a < N; a++) cptr[a + 1] += cptr[a];
        const std::vector<int> &co = sx.cam_obs, &op = sx.obs_pt; // (a camera's observations ascend, and with them their points)
        for (int k = 0; k < out.nodes; k++) {
            if (node_par[k] >= 0) {
                const int a = node_cam[k], b = node_cam[node_par[k]];
                int ia = cptr[a], ib = cptr[b];
                const int ea = cptr[a + 1], eb = cptr[b + 1];
                while (ia < ea && ib < eb) {
                    const int pa = op[co[ia]], pb = op[co[ib]];
                    if (pa < pb) ia++;
                    else if (pb < pa) ib++;
                    else {
                        int ra = ia, rb = ib;
                        while (ra < ea && op[co[ra]] == pa) ra++;
                        while (rb < eb && op[co[rb]] == pa) rb++;
                        for (int x = ia; x < ra; x++)
                            for (int y = ib; y < rb; y++) { edge_oo.push_back(co[x]); edge_oo.push_back(co[y]); }
                        ia = ra; ib = rb;
                    }
                }
                if (edge_oo.size() / 2 > (size_t)0x3fffffff) return BA_ERR_NOMEM;
            }
            edge_ptr.push_back((int)(edge_oo.size() / 2));
        }
    }
    return BA_OK;
}

// A group of 2 .. BA_SHARE_LOCAL chunks never crosses a workgroup's 8 slots (empty slots in front of it where it would).
void ba_plan_share_slots(int ngroups, int nchunks, const int *gptr, const int *cptr, const int *cgrp, ba_share_plan &out)
{
    out = ba_share_plan();
    std::vector<int> &desc = out.desc;
    auto slot = [&](int m0, int len, int c0, int nc, int ng) { desc.insert(desc.end(), {m0, len, c0, nc, ng}); };
    for (int g = 0, c = 0; g < ngroups; g++) {
        int nc = 0;
        while (c + nc < nchunks && cgrp[c + nc] == g) nc++;
        if (nc > 1 && nc <= BA_SHARE_LOCAL)
            while (desc.size() / 5 % 8 + (size_t)nc > 8) slot(0, 0, 0, 1, 1); // (an empty slot)
        const int c0 = (int)(desc.size() / 5), ng = gptr[g + 1] - gptr[g];
        for (int k = 0; k < nc; k++) {
            if (nc > BA_SHARE_LOCAL) out.wide.push_back((int)(desc.size() / 5));
            slot(cptr[c + k], cptr[c + k + 1] - cptr[c + k], c0, nc, ng);
        }
        out.largest = std::max(out.largest, ng);
        c += nc;
    }
    out.nslots = (int)(desc.size() / 5);
    out.nwide = (int)out.wide.size();
}

void ba_plan_relpose_csr(int N, int n, const int *pairs, std::vector<int> &ptr, std::vector<int> &inc)
{
    ptr.assign((size_t)N + 1, 0);
    inc.resize(2 * (size_t)n);
    for (int q = 0; q < 2 * n; q++) ptr[pairs[q] + 1]++;
    for (int a = 0; a < N; a++) ptr[a + 1] += ptr[a];
    std::vector<int> fill(ptr.begin(), ptr.end() - 1);
    for (int q = 0; q < n; q++) { inc[fill[pairs[2 * q]]++] = 2 * q; inc[fill[pairs[2 * q + 1]]++] = 2 * q + 1; }
}

size_t ba_plan_owner_offsets(int Dp, int nb, int world, std::vector<int> &off)
{
    const int nbc = Dp / nb;
    std::vector<size_t> fill((size_t)world, 0);
    off.resize((size_t)nbc);
    for (int p = 0; p < nbc; p++) { off[p] = (int)(fill[p % world] / nb); fill[p % world] += (size_t)nb * (size_t)(Dp - nb * p); }
    size_t own_chunk = 0;
    for (size_t f : fill) own_chunk = std::max(own_chunk, f);
    for (int p = 0; p < nbc; p++) off[p] += (int)((size_t)(p % world) * own_chunk / nb);
    return own_chunk;
}
