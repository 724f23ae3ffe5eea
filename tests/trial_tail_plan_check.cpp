// The grid of k_pairs_gram (csrc/ba_internal.h, ba_plan_tail_grid) against the plans it joins: the pair workgroups of ba_plan_schur come
// first and keep their count -- a multiple of the band count, so that a block index means the same band as in k_schur_pairs --, one
// workgroup per eight chunks of the camera-sorted view follows, none when there is no such chunk.  A stand-alone program
// (tests/test_trial_tail_plan_cpu.py builds and runs it); argv[1]: the data directory.
#include "ba_internal.h"

#include <cstdio>
#include <string>

static int failures = 0, cases = 0;
#define CHECK(c) do { if (!(c)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); failures++; } } while (0)

static void check(const ba_problem *p, int wgs, int cus, int bands)
{
    cases++;
    ba_structure s;
    if (ba_build_structure(p, 0, 1, BA_CHUNK, 32, &s)) { printf("ba_build_structure failed\n"); failures++; return; }
    ba_schur_plan pl;
    ba_plan_schur(s, wgs, cus, bands, 0, pl);
    const ba_tail_grid tg = ba_plan_tail_grid(pl.grid, s.ndchunks);
    CHECK(tg.pair_wgs == pl.grid && pl.nband >= 1 && tg.pair_wgs % pl.nband == 0);
    CHECK((int)pl.wave_ptr.size() == 4 * tg.pair_wgs + 1); // every wavefront of the front part has its range, nobody behind it reads one
    CHECK(s.ndchunks > 0 && tg.gram_wgs == (s.ndchunks + 7) / 8);
    CHECK(8 * tg.gram_wgs >= s.ndchunks && 8 * (tg.gram_wgs - 1) < s.ndchunks); // every chunk has its 32-lane group, no workgroup is idle
    CHECK((int)s.dchunk_ptr.size() == s.ndchunks + 1);
}

int main(int argc, char **argv)
{
    if (argc < 2) { printf("usage: trial_tail_plan_check DATA_DIR\n"); return 2; }
    ba_problem *p = nullptr;
    for (const char *name : {"problem-21-11315-pre.txt", "problem-39-18060-pre.txt"}) {
        if (ba_problem_load_bal((std::string(argv[1]) + "/" + name).c_str(), &p)) { printf("cannot load %s\n", name); return 2; }
        for (int wgs : {1, 3, 4})
            for (int bands : {1, 8}) check(p, wgs, 256, bands);
        ba_problem_free(p);
    }
    // small: 6 cameras of fewer than 32 observations (one short chunk each), and a count of chunks that is no multiple of 8
    for (int N : {6, 9, 17}) {
        if (ba_problem_synthetic(N, 60, 150, 14, &p)) { printf("ba_problem_synthetic failed\n"); return 2; }
        check(p, 4, 256, 8);
        check(p, 3, 8, 1);
        ba_problem_free(p);
    }
    // no chunk of the camera-sorted view: no Gram workgroup, whatever the pair part
    cases++;
    CHECK(ba_plan_tail_grid(1024, 0).gram_wgs == 0 && ba_plan_tail_grid(1024, 0).pair_wgs == 1024);
    CHECK(ba_plan_tail_grid(8, 1).gram_wgs == 1 && ba_plan_tail_grid(8, 8).gram_wgs == 1 && ba_plan_tail_grid(8, 9).gram_wgs == 2);
    printf("%d cases, %d failures\n", cases, failures);
    return failures ? 1 : 0;
}
