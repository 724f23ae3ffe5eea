// Stand-alone check of the host plans behind the solver's device lists (csrc/ba_structure.cpp, declared in csrc/ba_internal.h):
// tests/test_plans_cpu.py builds it from this file, ba_structure.cpp and ba_problem.cpp with the host compiler and
// -fsanitize=address,undefined and runs it with the data directory as its argument.  Every plan is checked against the invariants
// the kernels rely on -- none of them a measured number, none a second copy of the plan's algorithm:
//   eval ranges     start at 0, end at Kl, increase strictly, every boundary a pt_ptr value, at most 256 observations, greedy-maximal
//                   (the next point would not fit); none when a point has more than 256 observations or the shard has none
//   dealing         grid >= 1, a multiple of nband, 4 grid + 1 wave_ptr entries, monotone from 0 to nchunks; every chunk once, ids
//                   ascending inside a wavefront's list; the wavefronts of band b hold one contiguous range of the chunk list and the
//                   ranges ascend with b; descriptor = first entry, count, hi | lo << 16, id of the structure; BA_CHUNK_SINGLE iff the
//                   pair has one chunk and hi != lo; entry = (r, c), (r, ~point) for a self entry; red_pairs = ascending, the pairs with
//                   a chunk count other than 1 or hi == lo; inside a band largest load - smallest <= largest chunk cost, and no
//                   wavefront's load without the chunk it got last exceeds the smallest final load (that chunk went to the then
//                   emptiest wavefront; the loads carry over the windows, or a later window would break this)
//   forest          trees partition the nodes, tree_ptr ascends, a non-root's parent sits later in the same tree, the root is last
//                   with parent -1, largest <= max_tree, kept + dropped = |L|, in_tree = the nodes' cameras, node_rec = the constraint
//                   and side whose camera is the node (-1: roots, co-visibility edges); visibility: edge_ptr monotone, empty at roots,
//                   every pair (o, o') of the node's camera, its parent's camera and one point, ascending, as many as brute force counts
//   share slots     every chunk once, in order, c0 / nc / ng right, no group of 2 .. BA_SHARE_LOCAL chunks across a multiple of 8,
//                   padding {0, 0, 0, 1, 1}, wide = the slots of longer groups, largest = the largest group
//   CSR             ptr monotone, camera a's list = 2 q / 2 q + 1 of the constraints whose first / second camera is a, in list order
//   owner offsets   column p in the chunk of rank p % world, no overlap, own_chunk = the largest fill
// At the end five planted defects, each of which must be reported.
#include "ba_internal.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <string>

static int failures = 0, cases = 0;
static bool quiet = false; // planted defects: count, do not print
#define CHECK(cond, ...) do { if (!(cond)) { if (failures++ < 20 && !quiet) { printf("FAIL %s:%d %s | ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } } } while (0)

// ---- inputs ---------------------------------------------------------------------------------------------------------------------
static ba_problem *load(const std::string &path)
{
    ba_problem *p = nullptr;
    const int rc = ba_problem_load_bal(path.c_str(), &p);
    if (rc) { printf("cannot load %s (%d)\n", path.c_str(), rc); exit(2); }
    return p;
}
// cams[j]: the cameras of point j's observations, in file order
static ba_problem *hand_built(int N, const std::vector<std::vector<int>> &cams)
{
    std::vector<int> ci, pi;
    for (size_t j = 0; j < cams.size(); j++)
        for (int c : cams[j]) { ci.push_back(c); pi.push_back((int)j); }
    const int K = (int)ci.size(), M = (int)cams.size();
    std::vector<double> meas(2 * (size_t)K, 0.0), cams9(9 * (size_t)N, 0.0), pts(3 * (size_t)M, 0.0);
    ba_problem *p = nullptr;
    const int rc = ba_problem_create(N, M, K, ci.data(), pi.data(), meas.data(), cams9.data(), pts.data(), &p);
    if (rc) { printf("ba_problem_create failed (%d)\n", rc); exit(2); }
    return p;
}
static std::vector<int> run_of(int first, int count)
{
    std::vector<int> v((size_t)count);
    for (int i = 0; i < count; i++) v[i] = first + i;
    return v;
}
static ba_structure structure(const ba_problem *p, int rank, int world)
{
    ba_structure s;
    const int rc = ba_build_structure(p, rank, world, BA_CHUNK, 32, &s);
    if (rc) { printf("ba_build_structure failed (%d)\n", rc); exit(2); }
    return s;
}

// ---- eval ranges ----------------------------------------------------------------------------------------------------------------
static void verify_eval(const ba_structure &s, const std::vector<int> &eb)
{
    if (s.kmax > 256 || s.Kl == 0) { CHECK(eb.empty(), "kmax %d Kl %d: %zu boundaries", s.kmax, s.Kl, eb.size()); return; }
    CHECK(eb.size() >= 2 && eb.front() == 0 && eb.back() == s.Kl, "%zu boundaries", eb.size());
    for (size_t i = 0; i + 1 < eb.size(); i++) {
        CHECK(eb[i] < eb[i + 1] && eb[i + 1] - eb[i] <= 256, "range %zu: %d .. %d", i, eb[i], eb[i + 1]);
        CHECK(std::binary_search(s.pt_ptr.begin(), s.pt_ptr.end(), eb[i + 1]), "boundary %d is no point's", eb[i + 1]);
        if (i + 2 == eb.size()) break;
        // the point that starts the next range (behind the points without observations that share its offset) would not have fitted
        const size_t j = (size_t)(std::upper_bound(s.pt_ptr.begin(), s.pt_ptr.end(), eb[i + 1]) - s.pt_ptr.begin()) - 1;
        CHECK(j + 1 < s.pt_ptr.size() && eb[i + 1] - eb[i] + s.pt_ptr[j + 1] - s.pt_ptr[j] > 256, "range %zu: %d .. %d could take point %zu", i, eb[i],
              eb[i + 1], j);
    }
}
static std::vector<int> check_eval(const ba_structure &s)
{
    std::vector<int> eb;
    ba_plan_eval_ranges(s, eb);
    verify_eval(s, eb);
    cases++;
    return eb;
}

// ---- dealing --------------------------------------------------------------------------------------------------------------------
static void verify_schur(const ba_structure &s, int cap, int bands, int window, const ba_schur_plan &pl)
{
    const int nch = s.nchunks;
    CHECK(pl.grid >= 1 && pl.grid <= std::max(cap, 1) && pl.nband >= 1 && (pl.nband == 1 || pl.nband == bands) && pl.grid % pl.nband == 0, "grid %d nband %d",
          pl.grid, pl.nband);
    CHECK(pl.wave_ptr.size() == 4 * (size_t)pl.grid + 1 && pl.chunk_info.size() == 4 * (size_t)nch && pl.ent.size() == 2 * (size_t)s.E, "sizes");
    if (pl.wave_ptr.size() != 4 * (size_t)pl.grid + 1 || pl.chunk_info.size() != 4 * (size_t)nch || pl.ent.size() != 2 * (size_t)s.E || pl.grid < 1 ||
        pl.nband < 1 || pl.grid % pl.nband)
        return;
    const int W = 4 * pl.grid, Wb = W / pl.nband;
    CHECK(pl.wave_ptr[0] == 0 && pl.wave_ptr[W] == nch, "wave_ptr %d .. %d, %d chunks", pl.wave_ptr[0], pl.wave_ptr[W], nch);
    for (int w = 0; w < W; w++) CHECK(pl.wave_ptr[w] <= pl.wave_ptr[w + 1], "wave_ptr at %d", w);
    if (pl.wave_ptr[0] != 0 || pl.wave_ptr[W] != nch || !std::is_sorted(pl.wave_ptr.begin(), pl.wave_ptr.end())) return;
    auto cost = [&](int c) { return (long long)2 * ((s.chunk_ptr[c + 1] - s.chunk_ptr[c] + 7) / 8) + 1; }; // batches of eight entries + a constant
    std::vector<int> seen((size_t)nch, 0);
    int next_lo = 0; // the chunk list's position behind the bands so far
    for (int b = 0; b < pl.nband; b++) {
        int lo = nch, hi = -1, count = 0;
        long long cmax = 0;
        std::vector<long long> load((size_t)Wb, 0);
        for (int w = b * Wb; w < (b + 1) * Wb; w++)
            for (int k = pl.wave_ptr[w]; k < pl.wave_ptr[w + 1]; k++) {
                const int *ci = &pl.chunk_info[4 * (size_t)k], c = ci[3];
                CHECK(c >= 0 && c < nch, "descriptor %d: chunk %d", k, c);
                if (c < 0 || c >= nch) continue;
                CHECK(seen[c]++ == 0, "chunk %d twice", c);
                if (k > pl.wave_ptr[w]) CHECK(ci[-1] < c, "wavefront %d: chunk %d behind %d", w, c, ci[-1]);
                const int q = s.chunk_pair[c];
                const bool single = s.pair_chunk_ptr[q + 1] - s.pair_chunk_ptr[q] == 1 && s.pair_hi[q] != s.pair_lo[q];
                CHECK(ci[0] == s.chunk_ptr[c] && (ci[1] & ~BA_CHUNK_SINGLE) == s.chunk_ptr[c + 1] - s.chunk_ptr[c] && ci[2] == (s.pair_hi[q] | (s.pair_lo[q] << 16)),
                      "chunk %d: descriptor %d %d %d", c, ci[0], ci[1], ci[2]);
                CHECK(((ci[1] & BA_CHUNK_SINGLE) != 0) == single, "chunk %d of pair (%d, %d): single flag %d", c, s.pair_hi[q], s.pair_lo[q], ci[1] & BA_CHUNK_SINGLE);
                lo = std::min(lo, c); hi = std::max(hi, c); count++;
                load[w - b * Wb] += cost(c);
                cmax = std::max(cmax, cost(c));
            }
        if (count == 0) continue;
        CHECK(lo == next_lo && hi - lo + 1 == count, "band %d holds %d chunks of %d .. %d, the bands before end at %d", b, count, lo, hi, next_lo);
        next_lo = hi + 1;
        const long long lmin = *std::min_element(load.begin(), load.end()), lmax = *std::max_element(load.begin(), load.end());
        CHECK(lmax - lmin <= cmax, "band %d: loads %lld .. %lld, largest chunk cost %lld", b, lmin, lmax, cmax);
        // the chunk a wavefront got last: of its chunks in the latest window the cheapest, of equal ones the last
        const long long win = window > 0 ? (long long)window * Wb : (long long)nch + 1;
        for (int w = b * Wb; w < (b + 1) * Wb; w++) {
            if (pl.wave_ptr[w] == pl.wave_ptr[w + 1]) continue;
            int last = -1;
            for (int k = pl.wave_ptr[w]; k < pl.wave_ptr[w + 1]; k++) {
                const int c = pl.chunk_info[4 * (size_t)k + 3];
                if (c < lo || c > hi) continue;
                if (last < 0 || (c - lo) / win > (last - lo) / win || ((c - lo) / win == (last - lo) / win && cost(c) <= cost(last))) last = c;
            }
            if (last >= 0) CHECK(load[w - b * Wb] - cost(last) <= lmin, "band %d wavefront %d: load %lld, last chunk %d (cost %lld), smallest load %lld", b, w,
                                 load[w - b * Wb], last, cost(last), lmin);
        }
    }
    for (int c = 0; c < nch; c++) CHECK(seen[c] == 1, "chunk %d: %d times", c, seen[c]);
    for (long long e = 0; e < s.E; e++) {
        const int r = s.ent_r[(size_t)e], c = s.ent_c[(size_t)e];
        CHECK(pl.ent[2 * (size_t)e] == r && pl.ent[2 * (size_t)e + 1] == (r == c ? ~s.obs_pt[r] : c), "entry %lld", e);
    }
    std::vector<int> red;
    for (int q = 0; q < s.npairs; q++)
        if (s.pair_chunk_ptr[q + 1] - s.pair_chunk_ptr[q] != 1 || s.pair_hi[q] == s.pair_lo[q]) red.push_back(q);
    CHECK(red == pl.red_pairs, "red_pairs: %zu, expected %zu", pl.red_pairs.size(), red.size());
}
static ba_schur_plan check_schur(const ba_structure &s, int wgs, int cus, int bands, int window)
{
    ba_schur_plan pl;
    ba_plan_schur(s, wgs, cus, bands, window, pl);
    verify_schur(s, wgs * cus, bands, window, pl);
    cases++;
    return pl;
}

// ---- forest ---------------------------------------------------------------------------------------------------------------------
static void verify_forest(const ba_structure &s, const std::vector<int> &rp, int kind, int max_tree, const ba_forest_plan &fp)
{
    const int N = s.N;
    const bool vis = kind == BA_PRECOND_VISIBILITY_FOREST;
    size_t n = rp.size() / 2;
    if (vis) {
        std::vector<int> cp, cw;
        CHECK(ba_covisibility(N, s.Ml, s.pt_ptr.data(), s.obs_cam.data(), 0, cp, cw) == BA_OK, "ba_covisibility");
        n += cw.size();
    }
    CHECK(fp.width == (vis ? 9 : 6) && fp.kept >= 0 && (size_t)fp.kept + (size_t)fp.dropped == n, "kept %d + dropped %d, list of %zu", fp.kept, fp.dropped, n);
    if (fp.kept == 0) {
        CHECK(fp.ntrees == 0 && fp.nodes == 0 && fp.tree_ptr.empty() && fp.node_cam.empty() && fp.edge_oo.empty() && fp.largest == (N > 0 ? 1 : 0), "no kept edge");
        return;
    }
    const int nodes = fp.nodes, nt = fp.ntrees;
    CHECK(nt >= 1 && (int)fp.tree_ptr.size() == nt + 1 && (int)fp.node_cam.size() == nodes && (int)fp.node_par.size() == nodes && (int)fp.node_rec.size() == nodes &&
              (int)fp.in_tree.size() == N && fp.kept == nodes - nt,
          "sizes: %d trees, %d nodes, %d kept", nt, nodes, fp.kept);
    if ((int)fp.tree_ptr.size() != nt + 1 || (int)fp.node_cam.size() != nodes || (int)fp.node_par.size() != nodes || (int)fp.node_rec.size() != nodes ||
        (int)fp.in_tree.size() != N)
        return;
    CHECK(fp.tree_ptr[0] == 0 && fp.tree_ptr[nt] == nodes, "tree_ptr %d .. %d", fp.tree_ptr[0], fp.tree_ptr[nt]);
    int largest = 0;
    for (int t = 0; t < nt; t++) {
        const int t0 = fp.tree_ptr[t], t1 = fp.tree_ptr[t + 1];
        CHECK(t0 < t1 && t1 <= nodes, "tree %d: %d .. %d", t, t0, t1);
        if (!(t0 < t1 && t1 <= nodes && t0 >= 0)) return;
        largest = std::max(largest, t1 - t0);
        for (int k = t0; k < t1; k++) {
            if (k == t1 - 1) CHECK(fp.node_par[k] == -1 && fp.node_rec[k] == -1, "tree %d: root %d has parent %d, record %d", t, k, fp.node_par[k], fp.node_rec[k]);
            else CHECK(fp.node_par[k] > k && fp.node_par[k] < t1, "tree %d (%d .. %d): node %d has parent %d", t, t0, t1, k, fp.node_par[k]);
        }
    }
    CHECK(fp.largest == largest && largest <= max_tree, "largest %d, trees' %d, max_tree %d", fp.largest, largest, max_tree);
    std::vector<unsigned char> mark((size_t)N, 0);
    for (int k = 0; k < nodes; k++) {
        const int c = fp.node_cam[k];
        CHECK(c >= 0 && c < N && !mark[c], "node %d: camera %d", k, c);
        if (c >= 0 && c < N) mark[c] = 1;
    }
    CHECK(mark == fp.in_tree, "in_tree");
    for (int k = 0; k < nodes; k++) {
        const int par = fp.node_par[k], r = fp.node_rec[k];
        if (par <= k || par >= nodes) continue; // (a root, or reported above)
        const int a = fp.node_cam[k], b = fp.node_cam[par];
        if (r >= 0) {
            CHECK((size_t)r < rp.size() && rp[r] == a && rp[r ^ 1] == b, "node %d (camera %d, parent's %d): record %d", k, a, b, r);
        } else {
            bool constrained = false;
            for (size_t q = 0; q < rp.size() / 2; q++) constrained |= (rp[2 * q] == a && rp[2 * q + 1] == b) || (rp[2 * q] == b && rp[2 * q + 1] == a);
            CHECK(r == -1 && vis && !constrained, "node %d (camera %d, parent's %d): record %d", k, a, b, r);
        }
    }
    if (!vis) { CHECK(fp.edge_ptr.empty() && fp.edge_oo.empty(), "edge lists without visibility"); return; }
    CHECK((int)fp.edge_ptr.size() == nodes + 1 && fp.edge_ptr[0] == 0 && std::is_sorted(fp.edge_ptr.begin(), fp.edge_ptr.end()) &&
              (size_t)fp.edge_ptr.back() * 2 == fp.edge_oo.size(),
          "edge_ptr");
    if ((int)fp.edge_ptr.size() != nodes + 1 || fp.edge_ptr[0] != 0 || !std::is_sorted(fp.edge_ptr.begin(), fp.edge_ptr.end()) ||
        (size_t)fp.edge_ptr.back() * 2 != fp.edge_oo.size())
        return;
    std::vector<int> na((size_t)s.Ml), nb((size_t)s.Ml);
    for (int k = 0; k < nodes; k++) {
        const int par = fp.node_par[k], e0 = fp.edge_ptr[k], e1 = fp.edge_ptr[k + 1];
        if (par < 0) { CHECK(e0 == e1, "root %d has %d pairs", k, e1 - e0); continue; }
        if (par >= nodes) continue;
        const int a = fp.node_cam[k], b = fp.node_cam[par];
        for (int e = e0; e < e1; e++) {
            const int o = fp.edge_oo[2 * (size_t)e], o2 = fp.edge_oo[2 * (size_t)e + 1];
            const bool inside = o >= 0 && o < s.Kl && o2 >= 0 && o2 < s.Kl;
            CHECK(inside, "node %d pair %d: (%d, %d)", k, e, o, o2);
            if (!inside) continue;
            CHECK(s.obs_cam[o] == a && s.obs_cam[o2] == b && s.obs_pt[o] == s.obs_pt[o2], "node %d pair (%d, %d): cameras %d %d (node's %d, parent's %d), points %d %d", k, o,
                  o2, s.obs_cam[o], s.obs_cam[o2], a, b, s.obs_pt[o], s.obs_pt[o2]);
            if (e > e0) { // ascending point, then the node's observation, then the parent's: no pair twice
                const int po = fp.edge_oo[2 * (size_t)e - 2], po2 = fp.edge_oo[2 * (size_t)e - 1];
                const bool in2 = po >= 0 && po < s.Kl;
                CHECK(in2 && (s.obs_pt[po] < s.obs_pt[o] || (s.obs_pt[po] == s.obs_pt[o] && (po < o || (po == o && po2 < o2)))), "node %d pair %d out of order", k, e);
            }
        }
        // brute force: per point (observations of a) x (observations of b)
        std::fill(na.begin(), na.end(), 0);
        std::fill(nb.begin(), nb.end(), 0);
        for (int i = 0; i < s.Kl; i++) {
            if (s.obs_cam[i] == a) na[s.obs_pt[i]]++;
            if (s.obs_cam[i] == b) nb[s.obs_pt[i]]++;
        }
        long long want = 0;
        for (int j = 0; j < s.Ml; j++) want += (long long)na[j] * nb[j];
        CHECK(e1 - e0 == want, "node %d (cameras %d, %d): %d pairs, %lld common-point observation pairs", k, a, b, e1 - e0, want);
    }
}
static ba_forest_plan check_forest(const ba_structure &s, const std::vector<int> &rp, int kind, int max_tree)
{
    ba_forest_plan fp;
    CHECK(ba_plan_forest(s, rp, kind, max_tree, fp) == BA_OK, "ba_plan_forest");
    verify_forest(s, rp, kind, max_tree, fp);
    cases++;
    return fp;
}

// ---- share slots ----------------------------------------------------------------------------------------------------------------
struct groups { int ngroups = 0, nchunks = 0; std::vector<int> gptr, members, cptr, cgrp; };
static groups group_plan(const std::vector<int> &group_of)
{
    const int N = (int)group_of.size();
    groups g;
    g.gptr.resize((size_t)N / 2 + 2); g.members.resize((size_t)N + 1); g.cptr.resize((size_t)N + 2); g.cgrp.resize((size_t)N + 1);
    const int rc = ba_intrinsics_group_plan(N, group_of.data(), BA_SHARE_CHUNK, &g.ngroups, g.gptr.data(), g.members.data(), &g.nchunks, g.cptr.data(), g.cgrp.data());
    if (rc) { printf("ba_intrinsics_group_plan failed (%d)\n", rc); exit(2); }
    return g;
}
static void verify_share(const groups &g, const ba_share_plan &pl)
{
    CHECK(pl.desc.size() == 5 * (size_t)pl.nslots && pl.wide.size() == (size_t)pl.nwide, "sizes");
    if (pl.desc.size() != 5 * (size_t)pl.nslots) return;
    std::vector<int> wide;
    int c = 0, largest = 0; // the next chunk of the group plan
    for (int sl = 0; sl < pl.nslots; sl++) {
        const int *d = &pl.desc[5 * (size_t)sl];
        if (d[1] == 0) { CHECK(d[0] == 0 && d[2] == 0 && d[3] == 1 && d[4] == 1, "padding slot %d: %d %d %d %d %d", sl, d[0], d[1], d[2], d[3], d[4]); continue; }
        CHECK(c < g.nchunks, "slot %d: a chunk too many", sl);
        if (c >= g.nchunks) return;
        const int gr = g.cgrp[c];
        int first = c, nc = 0; // the group's first chunk and chunk count
        while (first > 0 && g.cgrp[first - 1] == gr) first--;
        while (first + nc < g.nchunks && g.cgrp[first + nc] == gr) nc++;
        const int ng = g.gptr[gr + 1] - g.gptr[gr];
        CHECK(d[0] == g.cptr[c] && d[1] == g.cptr[c + 1] - g.cptr[c] && d[2] == sl - (c - first) && d[3] == nc && d[4] == ng,
              "slot %d (chunk %d, the %d-th of %d of group %d with %d cameras): %d %d %d %d %d", sl, c, c - first, nc, gr, ng, d[0], d[1], d[2], d[3], d[4]);
        if (nc > 1 && nc <= BA_SHARE_LOCAL && c == first) CHECK(sl / 8 == (sl + nc - 1) / 8, "group %d: %d chunks from slot %d cross a block of 8", gr, nc, sl);
        if (nc > BA_SHARE_LOCAL) wide.push_back(sl);
        largest = std::max(largest, ng);
        c++;
    }
    CHECK(c == g.nchunks, "%d chunks in the slots, %d in the plan", c, g.nchunks);
    CHECK(wide == pl.wide, "wide: %zu slots, expected %zu", pl.wide.size(), wide.size());
    CHECK(largest == pl.largest, "largest %d, expected %d", pl.largest, largest);
}
static ba_share_plan check_share(const groups &g)
{
    ba_share_plan pl;
    ba_plan_share_slots(g.ngroups, g.nchunks, g.gptr.data(), g.cptr.data(), g.cgrp.data(), pl);
    verify_share(g, pl);
    cases++;
    return pl;
}

// ---- CSR of the constraints, owner offsets ----------------------------------------------------------------------------------------
static void check_csr(int N, const std::vector<int> &pairs)
{
    const int n = (int)(pairs.size() / 2);
    std::vector<int> ptr, inc;
    ba_plan_relpose_csr(N, n, pairs.data(), ptr, inc);
    cases++;
    CHECK((int)ptr.size() == N + 1 && (int)inc.size() == 2 * n && ptr[0] == 0 && ptr[N] == 2 * n && std::is_sorted(ptr.begin(), ptr.end()), "ptr");
    if ((int)ptr.size() != N + 1 || (int)inc.size() != 2 * n || ptr[0] != 0 || ptr[N] != 2 * n || !std::is_sorted(ptr.begin(), ptr.end())) return;
    for (int a = 0; a < N; a++) {
        std::vector<int> want;
        for (int q = 0; q < 2 * n; q++) // (q = 2 constraint + side, which is the list order)
            if (pairs[q] == a) want.push_back(q);
        CHECK(want == std::vector<int>(inc.begin() + ptr[a], inc.begin() + ptr[a + 1]), "camera %d", a);
    }
}
static void check_owner(int Dp, int nb, int world)
{
    std::vector<int> off;
    const size_t own_chunk = ba_plan_owner_offsets(Dp, nb, world, off);
    cases++;
    const int nbc = Dp / nb;
    CHECK((int)off.size() == nbc, "%zu offsets, %d block columns", off.size(), nbc);
    if ((int)off.size() != nbc) return;
    std::vector<size_t> fill((size_t)world, 0);
    std::vector<std::pair<size_t, size_t>> ranges;
    for (int p = 0; p < nbc; p++) {
        const size_t r = (size_t)(p % world), b = (size_t)off[p] * nb, len = (size_t)nb * (size_t)(Dp - nb * p);
        CHECK(off[p] >= 0 && b >= r * own_chunk && b + len <= (r + 1) * own_chunk, "Dp %d world %d: column %d at %zu + %zu, chunk of %zu", Dp, world, p, b, len, own_chunk);
        fill[r] += len;
        ranges.emplace_back(b, b + len);
    }
    std::sort(ranges.begin(), ranges.end());
    for (size_t i = 0; i + 1 < ranges.size(); i++) CHECK(ranges[i].second <= ranges[i + 1].first, "Dp %d world %d: ranges overlap at %zu", Dp, world, ranges[i + 1].first);
    CHECK(own_chunk == *std::max_element(fill.begin(), fill.end()), "Dp %d world %d: own_chunk %zu", Dp, world, own_chunk);
}

// a planted defect must be reported
static void planted(const char *what, const std::function<void()> &verify)
{
    const int before = failures;
    quiet = true;
    verify();
    quiet = false;
    const bool caught = failures > before;
    failures = before;
    printf("planted: %s: %s\n", what, caught ? "reported" : "NOT REPORTED");
    if (!caught) failures++;
}

int main(int argc, char **argv)
{
    if (argc != 2) { printf("usage: plans_check <directory of problem-21-11315-pre.txt and problem-39-18060-pre.txt>\n"); return 2; }
    const std::string data = argv[1];
    ba_problem *p21 = load(data + "/problem-21-11315-pre.txt"), *p39 = load(data + "/problem-39-18060-pre.txt"), *tiny = nullptr;
    if (ba_problem_synthetic(2, 40, 80, 5, &tiny)) { printf("ba_problem_synthetic failed\n"); return 2; }
    // hand-built: a point of exactly 256 observations | points that fill a range to exactly 256 | a point of 257 | a point seen twice
    std::vector<std::vector<int>> c256 = {run_of(0, 3), run_of(0, 256), run_of(5, 200), run_of(2, 57), run_of(0, 2)};
    std::vector<std::vector<int>> cfill = {run_of(0, 100), run_of(0, 100), run_of(0, 56), run_of(0, 10), run_of(0, 100), run_of(0, 100), run_of(0, 57), run_of(1, 2)};
    std::vector<std::vector<int>> c257 = {run_of(0, 3), run_of(0, 257), run_of(1, 4)};
    std::vector<std::vector<int>> ctwice = {{0, 0, 1}, {1, 2}, {0, 2, 2, 3}, {3, 1, 0}, {2, 3}};
    ba_problem *h256 = hand_built(300, c256), *hfill = hand_built(100, cfill), *h257 = hand_built(300, c257), *htwice = hand_built(4, ctwice);
    ba_problem *two = hand_built(2, {{0, 1}, {0, 1}}); // of eight shards, the first owns no observation

    struct named { const char *name; ba_structure s; };
    std::vector<named> all;
    all.push_back({"problem-21", structure(p21, 0, 1)});
    all.push_back({"problem-39", structure(p39, 0, 1)});
    all.push_back({"problem-21 shard 0/2", structure(p21, 0, 2)});
    all.push_back({"problem-21 shard 1/2", structure(p21, 1, 2)});
    all.push_back({"synthetic(2, 40, 80, 5)", structure(tiny, 0, 1)});
    all.push_back({"a point of 256", structure(h256, 0, 1)});
    all.push_back({"a range filled to 256", structure(hfill, 0, 1)});
    all.push_back({"a point of 257", structure(h257, 0, 1)});
    all.push_back({"a point seen twice", structure(htwice, 0, 1)});
    all.push_back({"a shard without observations", structure(two, 0, 8)});
    const ba_structure &s21 = all[0].s, &stiny = all[4].s, &s256 = all[5].s, &sfill = all[6].s, &s257 = all[7].s, &stwice = all[8].s, &sempty = all[9].s;
    CHECK(sempty.Kl == 0 && sempty.Ml == 0, "the first of eight shards of two points owns %d observations", sempty.Kl);

    // eval ranges
    for (const named &x : all) check_eval(x.s);
    CHECK(check_eval(s256) == std::vector<int>({0, 3, 259, 459, 518}), "a point of 256 is a range of its own");
    CHECK(check_eval(sfill) == std::vector<int>({0, 256, 466, 525}), "100 + 100 + 56 observations are one range");
    CHECK(s257.kmax == 257 && check_eval(s257).empty() && check_eval(sempty).empty(), "no ranges");

    // dealing: one band (a grid below 8 bands), eight bands, a grid cut down to a multiple of the bands; windows 0, 1, longer than a band
    const int caps[3][2] = {{1, 32}, {1, 64}, {4, 256}}, windows[3] = {0, 1, 100000};
    ba_schur_plan swap_me, flag_me;
    for (const named &x : all)
        for (const auto &cap : caps)
            for (int window : windows) {
                const ba_schur_plan pl = check_schur(x.s, cap[0], cap[1], 8, window);
                if (&x.s != &s21) continue;
                CHECK(s21.nchunks == 1610, "problem-21: %d chunks", s21.nchunks);
                if (cap[1] == 32) CHECK(pl.grid == 32 && pl.nband == 1, "cap 32: grid %d, %d bands", pl.grid, pl.nband);
                if (cap[1] == 64) CHECK(pl.grid == 64 && pl.nband == 8, "cap 64: grid %d, %d bands", pl.grid, pl.nband);
                if (cap[1] == 256) CHECK(pl.grid == 400 && pl.nband == 8, "cap 1024: grid %d (403 cut to a multiple of 8), %d bands", pl.grid, pl.nband);
                if (cap[1] == 64 && window == 1) swap_me = flag_me = pl;
            }
    {
        const ba_schur_plan pl = check_schur(stiny, 4, 256, 8, 0); // 3 chunks on the 4 wavefronts of one workgroup
        CHECK(stiny.nchunks == 3 && pl.grid == 1 && pl.wave_ptr.size() == 5, "synthetic(2, 40, 80, 5): %d chunks, grid %d", stiny.nchunks, pl.grid);
        check_schur(s21, 4, 256, 1, 0); // BA_SCHUR_BANDS=1
        check_schur(s21, 4, 256, 4, 3);
    }

    // forests: a chain and a star of constraints at max_tree 2, 3, 64, under both kinds; visibility forests without constraints
    std::vector<int> chain, star;
    for (int a = 0; a + 1 < 21; a++) { chain.push_back(a + 1); chain.push_back(a); }
    for (int a = 0; a < 21; a++)
        if (a != 7) { star.push_back(a % 2 ? 7 : a); star.push_back(a % 2 ? a : 7); }
    ba_forest_plan chain_plan, vis_plan;
    for (int max_tree : {2, 3, 64})
        for (int kind : {(int)BA_PRECOND_CONSTRAINT_FOREST, (int)BA_PRECOND_VISIBILITY_FOREST}) {
            const ba_forest_plan fc = check_forest(s21, chain, kind, max_tree), fs = check_forest(s21, star, kind, max_tree);
            CHECK(fc.kept > 0 && fs.kept > 0 && fc.largest == std::min(max_tree, 21) && fs.largest == std::min(max_tree, 21), "chain / star at max_tree %d", max_tree);
            if (max_tree == 64 && kind == BA_PRECOND_CONSTRAINT_FOREST) chain_plan = fc;
        }
    vis_plan = check_forest(s21, {}, BA_PRECOND_VISIBILITY_FOREST, BA_PCG_VIS_MAX_TREE_DEFAULT);
    CHECK(vis_plan.kept > 0 && !vis_plan.edge_oo.empty(), "problem-21's visibility forest");
    check_forest(s21, {}, BA_PRECOND_CONSTRAINT_FOREST, BA_PCG_MAX_TREE_DEFAULT); // no constraint: no forest
    check_forest(s21, chain, BA_PRECOND_BLOCK_JACOBI, 64);
    check_forest(s21, chain, BA_PRECOND_CONSTRAINT_FOREST, 1);
    for (int max_tree : {2, 4}) {
        CHECK(check_forest(stwice, {}, BA_PRECOND_VISIBILITY_FOREST, max_tree).kept > 0, "the point seen twice: no kept edge");
        check_forest(stwice, {3, 0, 1, 2}, BA_PRECOND_VISIBILITY_FOREST, max_tree);
    }
    check_forest(all[2].s, chain, BA_PRECOND_VISIBILITY_FOREST, BA_PCG_VIS_MAX_TREE_DEFAULT);
    check_forest(sempty, {}, BA_PRECOND_VISIBILITY_FOREST, BA_PCG_VIS_MAX_TREE_DEFAULT);

    // share slots: groups of exactly BA_SHARE_LOCAL chunks and one more, groups of 3 chunks of which the third would straddle a block
    // of 8 slots, groups of one chunk, singletons (a label used once) and negatives mixed in
    std::vector<int> group_of;
    auto add = [&](int label, int count) { group_of.insert(group_of.end(), (size_t)count, label); };
    add(100, 600); add(-1, 3); add(101, 600); add(7, 1); add(102, 600); add(103, 2); add(-5, 1); add(104, BA_SHARE_LOCAL * BA_SHARE_CHUNK);
    add(8, 1); add(105, BA_SHARE_LOCAL * BA_SHARE_CHUNK + 1); add(106, 300); add(107, 2); add(108, 7 * BA_SHARE_CHUNK); add(103, 1); add(109, BA_SHARE_CHUNK + 1);
    const groups g = group_plan(group_of);
    const ba_share_plan share = check_share(g);
    CHECK(g.ngroups == 10 && share.nwide == BA_SHARE_LOCAL + 1 && share.nslots > g.nchunks && share.largest == BA_SHARE_LOCAL * BA_SHARE_CHUNK + 1,
          "%d groups, %d chunks, %d slots, %d wide", g.ngroups, g.nchunks, share.nslots, share.nwide);
    check_share(group_plan({-1, 0, 1, 2, -1})); // no group
    check_share(group_plan({4, 4, 4}));

    // CSR of the constraints; owner offsets at block-column counts that are no multiple of the world
    check_csr(21, chain); check_csr(21, star); check_csr(21, {}); check_csr(4, {3, 0, 1, 2, 0, 1, 2, 3, 3, 1});
    for (int world : {1, 2, 3})
        for (int nbc : {1, 7, 10, 37}) check_owner(64 * nbc, 64, world);

    // planted defects
    {
        const int W = 4 * swap_me.grid;
        int wa = 0, wb = W - 1;
        while (wa < W && swap_me.wave_ptr[wa] == swap_me.wave_ptr[wa + 1]) wa++;
        while (wb > wa && swap_me.wave_ptr[wb] == swap_me.wave_ptr[wb + 1]) wb--;
        CHECK(wa < wb, "problem-21 at cap 64 fills one wavefront alone");
        if (wa < wb)
            for (int q = 0; q < 4; q++) std::swap(swap_me.chunk_info[4 * (size_t)swap_me.wave_ptr[wa] + q], swap_me.chunk_info[4 * (size_t)swap_me.wave_ptr[wb + 1] - 4 + q]);
        planted("two chunks swapped between wavefronts", [&] { verify_schur(s21, 64, 8, 1, swap_me); });
        size_t k = 0;
        while (k < (size_t)s21.nchunks && !(flag_me.chunk_info[4 * k + 1] & BA_CHUNK_SINGLE)) k++;
        CHECK(k < (size_t)s21.nchunks, "problem-21 has no single chunk");
        if (k < (size_t)s21.nchunks) flag_me.chunk_info[4 * k + 1] &= ~BA_CHUNK_SINGLE;
        planted("a cleared SINGLE flag", [&] { verify_schur(s21, 64, 8, 1, flag_me); });
        CHECK(chain_plan.nodes == 21 && chain_plan.ntrees == 1, "the chain is one tree");
        if (chain_plan.nodes == 21) chain_plan.node_par[5] = 2;
        planted("a child placed behind its parent", [&] { verify_forest(s21, chain, BA_PRECOND_CONSTRAINT_FOREST, 64, chain_plan); });
        // the padding in front of a group taken out: every slot behind it moves up
        ba_share_plan crossed = share;
        std::vector<int> moved((size_t)share.nslots, -1);
        crossed.desc.clear();
        for (int sl = 0; sl < share.nslots; sl++)
            if (share.desc[5 * (size_t)sl + 1] != 0) {
                moved[sl] = (int)(crossed.desc.size() / 5);
                crossed.desc.insert(crossed.desc.end(), share.desc.begin() + 5 * (size_t)sl, share.desc.begin() + 5 * (size_t)sl + 5);
            }
        for (size_t sl = 0; sl < crossed.desc.size() / 5; sl++) crossed.desc[5 * sl + 2] = moved[crossed.desc[5 * sl + 2]];
        for (int &w : crossed.wide) w = moved[w];
        crossed.nslots = (int)(crossed.desc.size() / 5);
        planted("a group laid across a slot block", [&] { verify_share(g, crossed); });
        // the parent's observation of the first pair replaced by one of the same camera at another point
        bool done = false;
        for (int k2 = 0; k2 < vis_plan.nodes && !done; k2++)
            if (vis_plan.edge_ptr[k2] < vis_plan.edge_ptr[k2 + 1]) {
                int &o2 = vis_plan.edge_oo[2 * (size_t)vis_plan.edge_ptr[k2] + 1];
                for (int i = 0; i < s21.Kl && !done; i++)
                    if (s21.obs_cam[i] == s21.obs_cam[o2] && s21.obs_pt[i] != s21.obs_pt[o2]) { o2 = i; done = true; }
            }
        CHECK(done, "no pair to spoil");
        planted("an edge_oo pair of different points", [&] { verify_forest(s21, {}, BA_PRECOND_VISIBILITY_FOREST, BA_PCG_VIS_MAX_TREE_DEFAULT, vis_plan); });
    }
    for (ba_problem *p : {p21, p39, tiny, h256, hfill, h257, htwice, two}) ba_problem_free(p);
    printf("%d cases, %d failures\n", cases, failures);
    return failures ? 1 : 0;
}
