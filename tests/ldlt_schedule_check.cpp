// Stand-alone check of csrc/ba_ldlt_schedule.h (tests/test_ldlt_schedule_cpu.py builds it with the host compiler and
// -fsanitize=address,undefined and runs it).  For every block-column count 2 ... 47, row blocks = columns and columns + 1 (the
// right-hand side row in a row block of its own), budgets {0, 1, 50, 300, unbounded} and caps {1, 2, 3, 4} it replays the
// schedule launch by launch against the six invariants in the header, checks that the units of a launch stay within the
// effective budget plus that launch's forced work, and that the unbounded budget gives the textbook order.
#include "ba_ldlt_schedule.h"

#include <cstdio>
#include <cstdlib>

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (failures++ < 20) { printf("FAIL %s:%d %s | ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } } } while (0)

static long long check(int nrb, int ncb, long long budget, int cap, bool textbook)
{
    const ba_ldlt_schedule s = ba_ldlt_make_schedule(nrb, ncb, budget, cap);
    CHECK((int)s.first.size() == ncb + 1 && s.first[0] == 0 && s.first[ncb] == (int)s.jobs.size(), "ncb %d", ncb);
    std::vector<int> applied((size_t)nrb * ncb, 0), seen((size_t)nrb * ncb, 0);
    long long worst = 0;
    for (int p = 1; p < ncb; p++) {
        CHECK(s.first[p] <= s.first[p + 1], "p %d", p);
        // 5: before launch p starts, block column p holds panels 0 ... p - 2
        for (int i = p; i < nrb; i++) CHECK(applied[(size_t)i * ncb + p] == p - 1, "deadline: ncb %d nrb %d budget %lld cap %d p %d row %d has %d", ncb, nrb, budget, cap, p, i, applied[(size_t)i * ncb + p]);
        // this launch's forced work, from the state alone: the tiles that could not make their deadline within the cap otherwise
        long long forced = 0;
        for (int j = p + 1; j < ncb; j++)
            for (int i = j; i < nrb; i++) {
                const int d = applied[(size_t)i * ncb + j], pend = p - d;
                if (pend > 0 && (long long)(j - 1 - d) > (long long)cap * (j - 1 - p)) forced += std::min(cap, pend);
            }
        long long units = 0;
        for (int k = s.first[p]; k < s.first[p + 1]; k++) {
            const ba_ldlt_job &jb = s.jobs[k];
            const bool inside = jb.tj >= p + 1 && jb.tj < ncb && jb.ti >= jb.tj && jb.ti < nrb;
            CHECK(inside, "p %d job (%d, %d)", p, jb.ti, jb.tj);
            if (!inside) continue;
            const size_t t = (size_t)jb.ti * ncb + jb.tj;
            CHECK(jb.n >= 1 && jb.n <= cap, "6: depth %d cap %d", jb.n, cap);
            CHECK(jb.a == applied[t], "1, 2: tile (%d, %d) holds %d panels, job starts at %d", jb.ti, jb.tj, applied[t], jb.a);
            CHECK(jb.a + jb.n - 1 <= p - 1, "3: panel %d in launch %d", jb.a + jb.n - 1, p);
            CHECK(jb.a + jb.n - 1 <= jb.tj - 2, "1: panel %d on column %d", jb.a + jb.n - 1, jb.tj);
            CHECK(seen[t] != p, "4: tile (%d, %d) twice in launch %d", jb.ti, jb.tj, p);
            if (k > s.first[p]) CHECK(s.jobs[k - 1].n >= jb.n, "deepest first, p %d", p);
            if (textbook) {
                CHECK(jb.n == 1 && jb.a == p - 1, "textbook: p %d job (%d, %d, %d, %d)", p, jb.ti, jb.tj, jb.a, jb.n);
                if (k > s.first[p]) CHECK(s.jobs[k - 1].ti < jb.ti || (s.jobs[k - 1].ti == jb.ti && s.jobs[k - 1].tj < jb.tj), "textbook order, p %d", p);
            }
            applied[t] = jb.a + jb.n; seen[t] = p; units += jb.n;
        }
        if (textbook) { // every trailing tile, once
            long long tiles = 0;
            for (int j = p + 1; j < ncb; j++) tiles += nrb - j;
            CHECK(units == tiles && s.first[p + 1] - s.first[p] == tiles, "textbook: p %d units %lld tiles %lld", p, units, tiles);
        }
        const long long effective = std::max(std::min(budget, BA_LDLT_BUDGET_UNBOUNDED), forced);
        CHECK(s.forced[p] == forced && s.budget[p] == effective, "p %d forced %lld / %lld budget %lld / %lld", p, s.forced[p], forced, s.budget[p], effective);
        CHECK(units >= forced && units <= effective + forced, "budget: ncb %d cap %d budget %lld p %d units %lld forced %lld", ncb, cap, budget, p, units, forced);
        worst = std::max(worst, units);
    }
    for (int j = 0; j < ncb; j++) // 1: complete
        for (int i = j; i < nrb; i++) CHECK(applied[(size_t)i * ncb + j] == std::max(j - 1, 0), "complete: tile (%d, %d) holds %d", i, j, applied[(size_t)i * ncb + j]);
    return worst;
}

int main()
{
    const long long budgets[5] = {0, 1, 50, 300, BA_LDLT_BUDGET_UNBOUNDED};
    int cases = 0;
    for (int ncb = 2; ncb <= 47; ncb++)
        for (int extra = 0; extra < 2; extra++)
            for (int b = 0; b < 5; b++)
                for (int cap = 1; cap <= 4; cap++, cases++) check(ncb + extra, ncb, budgets[b], cap, b == 4 || cap == 1);
    // a budget in units past the tile count is the textbook order as well; a p-dependent budget keeps the invariants
    check(38, 37, 37 * 38, 3, true);
    { const ba_ldlt_schedule s = ba_ldlt_make_schedule(38, 37, 200, 3, 8); CHECK(!s.jobs.empty(), "slope"); }
    // degenerate sizes
    CHECK(ba_ldlt_make_schedule(1, 1, 0, 3).jobs.empty() && ba_ldlt_make_schedule(2, 1, 300, 3).first.size() == 2, "one block column");
    CHECK(ba_ldlt_make_schedule(0, 0, 0, 0).first.size() == 1, "empty");
    for (int cap = 2; cap <= 4; cap++) printf("37 block columns, 38 row blocks, budget 0, cap %d: at most %lld units per launch\n", cap, check(38, 37, 0, cap, false));
    printf("%d cases, %d failures\n", cases, failures);
    return failures ? 1 : 0;
}
