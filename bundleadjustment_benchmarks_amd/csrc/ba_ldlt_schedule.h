// ba_ldlt_schedule.h -- host side only: which trailing tiles every fused step of the dense LDL^T updates, and with which panels.
//
// The right-looking factorisation (ba_dense.hip.h) owes tile (ti, tj) of the trailing matrix, tj >= 2, the panels 0 ... tj - 2 in
// ascending order; panel tj - 1 is applied by launch tj itself (its row workgroups and the diagonal look-ahead).  Applying panel
// p - 1 to every trailing tile in launch p -- the textbook order -- front-loads the work: 630 tiles in launch 1 of a 37-column
// matrix, 15 in launch 30, beside a panel chain that takes the same time in every launch.  Nothing needs the far columns early:
// block column j must only hold panels 0 ... j - 2 when launch j STARTS.  This generator spreads the (tile, panel) units evenly:
// launch p gets a list of jobs (ti, tj, a, n) = "apply panels a ... a + n - 1 to tile (ti, tj)", such that
//   1. every (tile, panel) unit of the textbook order is applied exactly once,
//   2. on every tile the panels come in ascending order,
//   3. panel q is used in launches > q only (its Y and L exist from the end of launch q),
//   4. no tile appears twice in one launch,
//   5. before launch j starts every tile of block column j holds panels 0 ... j - 2,
//   6. n <= cap.
// A tile of column j that has `done` panels after launch p can still make its deadline iff j - 1 - done <= cap (j - 1 - p): the
// generator forces a job (at full depth, min(cap, pending): a visit costs a pass over the tile) on every tile that would break
// that otherwise -- by induction the forced depth never exceeds the cap or what is pending, so no deadline is ever missed,
// whatever the budget: a launch's effective budget is max(budget, forced units).  What is left of the budget goes to the other
// pending tiles, nearest column first.  cap = 1 forces everything at once, and so does a budget past the number of tiles: the
// textbook order, one depth-1 job per trailing tile and launch, tiles in row order.
#ifndef BA_LDLT_SCHEDULE_H
#define BA_LDLT_SCHEDULE_H

#include <algorithm>
#include <vector>

struct ba_ldlt_job { int ti, tj, a, n; }; // tile (block row, block column), first panel, number of panels

struct ba_ldlt_schedule {
    std::vector<ba_ldlt_job> jobs; // launch p: jobs[first[p]] ... jobs[first[p + 1] - 1], deepest first
    std::vector<int> first;        // ncb + 1 entries (launches 0 and ncb - 1 have no jobs)
    std::vector<long long> budget; // per launch: the effective budget, max(requested, forced units)
    std::vector<long long> forced; // per launch: units of the forced jobs
};

#define BA_LDLT_BUDGET_UNBOUNDED (1ll << 40)

// nrb row blocks (the right-hand side row included), ncb block columns; budget + slope * (p - 1) units in launch p.
inline ba_ldlt_schedule ba_ldlt_make_schedule(int nrb, int ncb, long long budget, int cap, long long slope = 0)
{
    ba_ldlt_schedule s;
    if (ncb < 0) ncb = 0;
    if (nrb < ncb) nrb = ncb;
    if (cap < 1) cap = 1;
    if (budget < 0) budget = 0;
    s.first.assign((size_t)ncb + 1, 0);
    s.budget.assign((size_t)ncb, 0);
    s.forced.assign((size_t)ncb, 0);
    std::vector<int> done((size_t)nrb * ncb, 0), seen((size_t)nrb * ncb, 0); // panels applied; last launch that visited the tile
    std::vector<ba_ldlt_job> cur;
    for (int p = 1; p < ncb; p++) {
        s.first[p] = (int)s.jobs.size();
        cur.clear();
        long long units = 0;
        for (int j = p + 1; j < ncb; j++) // forced: the deadline (column p + 1) and the tiles that the cap leaves no slack
            for (int i = j; i < nrb; i++) {
                const size_t t = (size_t)i * ncb + j;
                const int pend = p - done[t];
                if (pend <= 0 || (long long)(j - 1 - done[t]) <= (long long)cap * (j - 1 - p)) continue;
                const int n = std::min(cap, pend);
                cur.push_back({i, j, done[t], n});
                done[t] += n; seen[t] = p; units += n;
            }
        s.forced[p] = units;
        const long long want = std::min(budget + slope * (p - 1), BA_LDLT_BUDGET_UNBOUNDED);
        s.budget[p] = std::max(want, units);
        for (int j = p + 2; j < ncb && units < want; j++) // the rest of the budget, nearest column first
            for (int i = j; i < nrb && units < want; i++) {
                const size_t t = (size_t)i * ncb + j;
                const int pend = p - done[t];
                if (pend <= 0 || seen[t] == p) continue;
                const int n = (int)std::min<long long>(std::min(cap, pend), want - units);
                cur.push_back({i, j, done[t], n});
                done[t] += n; seen[t] = p; units += n;
            }
        // deepest first (they end last), then the textbook order of the tiles: rows, and a row's tiles next to each other
        std::sort(cur.begin(), cur.end(), [](const ba_ldlt_job &x, const ba_ldlt_job &y) {
            return x.n != y.n ? x.n > y.n : x.ti != y.ti ? x.ti < y.ti : x.tj < y.tj;
        });
        s.jobs.insert(s.jobs.end(), cur.begin(), cur.end());
    }
    s.first[ncb] = (int)s.jobs.size();
    return s;
}

#endif
