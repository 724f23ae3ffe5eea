// Dev tool: times the dense LDL^T kernels of ba_dense.hip.h on a random SPD matrix (not part of the product).
// hipcc --offload-arch=gfx950 -O3 -std=c++17 -mllvm -amdgpu-mfma-vgpr-form [-DBA_STAMP] -I bundleadjustment_benchmarks_amd/csrc scripts/bench_dense.hip -o scripts/bench_dense.bin
// (the library's flags, csrc/Makefile; scripts/dense_trace.sh <tag> bench_dense.bin <D> lists the per-launch times of a factorisation)
#ifndef BENCH_NB
#define BENCH_NB 64
#endif
#include "ba_dense.hip.h"
#include <cstdio>
#include <cstdlib>
#include <vector>
#include <cmath>
#include <cstring>
#include <algorithm>
#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e)); exit(1);} } while (0)
int main(int argc, char **argv)
{
    int D = argc > 1 ? atoi(argv[1]) : 2313;
    constexpr int NB = BENCH_NB; const int Dp = ((D + 3 + NB - 1) / NB) * NB, ld = Dp + 64;
    std::vector<double> h((size_t)ld * (Dp + 64), 0.0);
    srand(1);
    // SPD: A = B B^T / n + I with B random (use a cheap banded + random low-rank construction)
    std::vector<double> v((size_t)D * 8);
    for (auto &x : v) x = rand() / (double)RAND_MAX - 0.5;
    for (int c = 0; c < D; c++)
        for (int r = c; r < D; r++) {
            double a = (r == c) ? 4.0 : 0.0;
            for (int k = 0; k < 8; k++) a += v[(size_t)r * 8 + k] * v[(size_t)c * 8 + k];
            h[(size_t)c * ld + r] = a;
        }
    for (int c = 0; c < D; c++) h[(size_t)c * ld + D] = rand() / (double)RAND_MAX; // rhs row
    for (int c = D; c < Dp; c++) h[(size_t)c * ld + c] = 1.0;
    double *S, *Wp, *Winv, *x, *S0; int *flags;
    long long *stamps;
    CK(hipMalloc(&S, sizeof(double) * h.size())); CK(hipMalloc(&S0, sizeof(double) * h.size()));
    const size_t wpn = (size_t)ba_ldlt_wp_panels(D, NB) * ld * NB; // the Y history of the fused steps
    CK(hipMalloc(&Wp, sizeof(double) * wpn)); CK(hipMalloc(&Winv, sizeof(double) * (size_t)(Dp / NB) * NB * NB));
    CK(hipMalloc(&x, sizeof(double) * (2 * Dp + 128))); CK(hipMalloc(&stamps, 8 * 64));
    CK(hipMemcpy(S0, h.data(), sizeof(double) * h.size(), hipMemcpyHostToDevice));
    CK(hipMemset(Wp, 0, sizeof(double) * wpn));
    const int nflags = Dp / NB + 2; CK(hipMalloc(&flags, sizeof(int) * nflags)); CK(hipMemset(flags, 0, sizeof(int) * nflags));
    hipStream_t st; CK(hipStreamCreate(&st));
    hipEvent_t e0, e1, e2, e3; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1)); CK(hipEventCreate(&e2)); CK(hipEventCreate(&e3));
    const int nrows = D + 1, ncols = D, nblk = (ncols + NB - 1) / NB;
    // the trailing-update schedule of the fused steps (BA_LDLT_UPD_BUDGET / BA_LDLT_UPD_CAP), uploaded once like the solver does
    auto upload_plan = [&](ba_ldlt_plan pl) { int *d; CK(hipMalloc(&d, sizeof(int) * pl.jobs.size())); CK(hipMemcpy(d, pl.jobs.data(), sizeof(int) * pl.jobs.size(), hipMemcpyHostToDevice)); pl.d_jobs = d; return pl; };
    const ba_ldlt_plan plan = upload_plan(ba_ldlt_make_plan(nrows, ncols, NB));
    float tp = 0, tu = 0, tb = 0, tot = 0;
    std::vector<double> xs_h(D);
    const int reps = 5;
    for (int fused = 0; fused < 2; fused++) {
    tot = 0; tb = 0;
    for (int rep = 0; rep < reps + 1; rep++) {
        CK(hipMemcpyAsync(S, S0, sizeof(double) * h.size(), hipMemcpyDeviceToDevice, st));
        CK(hipEventRecord(e0, st));
        if (fused) ba_ldlt_factor<double, NB>(st, nrows, ncols, ld, S, Wp, Winv, flags, nflags, nullptr, false, 0, &plan); // the product's launch sequence
        else for (int p = 0; p < nblk; p++) {
            const int p0 = p * NB, below = nrows - (p0 + NB), g = below > 0 ? (below + 63) / 64 : 1;
            hipLaunchKernelGGL((k_ldlt_panel<double, NB>), dim3(g), dim3(256), 0, st, nrows, ncols, ld, p0, S, Wp, Winv + (size_t)p * NB * NB, flags, nflags);
            const int p1 = p0 + NB;
            if (p1 < ncols) {
                const int nti = (nrows - p1 + 63) / 64, ntj = (ncols - p1 + 63) / 64;
                hipLaunchKernelGGL((k_ldlt_update<double, NB>), dim3(ntj, nti), dim3(256), 0, st, nrows, ncols, ld, p0, S, Wp);
            }
        }
        CK(hipEventRecord(e1, st));
        if (fused) ba_ldlt_backsweep<double, NB>(st, ncols, ld, D, S, Winv, x, x + Dp);
        else for (int p = nblk - 1; p >= 0; p--) { // one block column per launch
            const int p0 = p * NB;
            int g = (p0 + 63) / 64; if (g < 1) g = 1;
            hipLaunchKernelGGL((k_ldlt_backstep<double, NB>), dim3(g), dim3(256), 0, st, ncols, ld, D, p0, S, Winv + (size_t)p * NB * NB, x);
        }
        CK(hipEventRecord(e2, st));
        CK(hipStreamSynchronize(st));
        float a, b; CK(hipEventElapsedTime(&a, e0, e1)); CK(hipEventElapsedTime(&b, e1, e2));
        if (rep) { tot += a; tb += b; }
    }
    CK(hipMemcpy(xs_h.data(), x, sizeof(double) * D, hipMemcpyDeviceToHost));
    { double rn = 0, bn = 0; for (int r = 0; r < D; r++) { double a = 0; for (int c = 0; c < D; c++) a += (c <= r ? h[(size_t)c * ld + r] : h[(size_t)r * ld + c]) * xs_h[c]; const double b = h[(size_t)r * ld + D]; rn += (a - b) * (a - b); bn += b * b; }
      printf("%s: D=%d factor %.3f ms  backsweep %.3f ms  residual %.2e\n", fused ? "fused look-ahead" : "separate launches", D, tot / reps, tb / reps, std::sqrt(rn / bn)); }
    }
    if (argc > 2 && atoi(argv[2]) == -2) {
        // Sweep of the trailing-update schedule (bench_dense.bin <D> -2 [rounds]): budget (+ slope per launch) x cap, variants interleaved round by round, median over the rounds of the mean of `reps` factorisations; every variant's factor is
        // compared bit for bit with the textbook order's (variant 0).
        struct V { long long budget; int cap; long long slope; };
        std::vector<V> vs = {{BA_LDLT_BUDGET_UNBOUNDED, 1, 0}};
        for (int cap : {2, 3, 4}) for (long long b : {0, 100, 250, 300, 350, 400, 450}) vs.push_back({b, cap, 0});
        for (int cap : {2, 3, 4}) { vs.push_back({200, cap, 8}); vs.push_back({250, cap, 6}); vs.push_back({400, cap, -6}); }
        std::vector<ba_ldlt_plan> pls;
        for (const V &v : vs) pls.push_back(upload_plan(ba_ldlt_make_plan(nrows, ncols, NB, v.budget, v.cap, v.slope)));
        const int rounds = argc > 3 ? atoi(argv[3]) : 7;
        std::vector<std::vector<float>> ms(vs.size());
        std::vector<double> ref(h.size()), got(h.size());
        std::vector<int> equal(vs.size(), -1);
        for (int round = 0; round < rounds; round++)
            for (size_t k = 0; k < vs.size(); k++) {
                float acc = 0;
                for (int rep = 0; rep < reps + 1; rep++) {
                    CK(hipMemcpyAsync(S, S0, sizeof(double) * h.size(), hipMemcpyDeviceToDevice, st));
                    CK(hipEventRecord(e0, st));
                    ba_ldlt_factor<double, NB>(st, nrows, ncols, ld, S, Wp, Winv, flags, nflags, nullptr, false, 0, &pls[k]);
                    CK(hipEventRecord(e1, st));
                    CK(hipStreamSynchronize(st));
                    float a; CK(hipEventElapsedTime(&a, e0, e1));
                    if (rep) acc += a;
                }
                ms[k].push_back(acc / reps);
                if (round == 0) {
                    CK(hipMemcpy(k ? got.data() : ref.data(), S, sizeof(double) * h.size(), hipMemcpyDeviceToHost));
                    equal[k] = k ? memcmp(got.data(), ref.data(), sizeof(double) * h.size()) == 0 : 1;
                }
            }
        for (size_t k = 0; k < vs.size(); k++) {
            std::sort(ms[k].begin(), ms[k].end());
            size_t nj = pls[k].jobs.size() / 4 - 1; int mx = 0;
            for (int p = 1; p < nblk; p++) mx = std::max(mx, pls[k].first[p + 1] - pls[k].first[p]);
            printf("sweep D=%d budget %lld slope %lld cap %d: jobs %zu (most per launch %d)  factor median %.4f ms  min %.4f  max %.4f  bit-equal %d\n", D,
                   vs[k].budget >= BA_LDLT_BUDGET_UNBOUNDED ? -1ll : vs[k].budget, vs[k].slope, vs[k].cap, nj, mx, ms[k][ms[k].size() / 2], ms[k].front(), ms[k].back(), equal[k]);
        }
        return 0;
    }
    // panel-only and update-only timings at p0 = 0
    CK(hipMemcpy(S, S0, sizeof(double) * h.size(), hipMemcpyDeviceToDevice));
    CK(hipEventRecord(e0, st));
    for (int r = 0; r < 20; r++) hipLaunchKernelGGL((k_ldlt_panel<double, NB>), dim3((nrows - NB + 63) / 64), dim3(256), 0, st, nrows, ncols, ld, 0, S, Wp, Winv);
    CK(hipEventRecord(e1, st));
    for (int r = 0; r < 20; r++) hipLaunchKernelGGL((k_ldlt_panel<double, NB>), dim3(1), dim3(256), 0, st, nrows, ncols, ld, 0, S, Wp, Winv);
    CK(hipEventRecord(e2, st));
    for (int r = 0; r < 20; r++) { const int nti = (nrows - NB + 63) / 64, ntj = (ncols - NB + 63) / 64; hipLaunchKernelGGL((k_ldlt_update<double, NB>), dim3(ntj, nti), dim3(256), 0, st, nrows, ncols, ld, 0, S, Wp); }
    CK(hipEventRecord(e3, st));
    CK(hipStreamSynchronize(st));
    CK(hipEventElapsedTime(&tp, e0, e1)); float tp1; CK(hipEventElapsedTime(&tp1, e1, e2)); CK(hipEventElapsedTime(&tu, e2, e3));
    printf("D=%d factor %.3f ms  backsweep %.3f ms | panel(p0=0, full grid) %.2f us, panel(1 WG) %.2f us, update(p0=0) %.2f us\n", D, tot / reps, tb / reps,
           tp / 20 * 1e3, tp1 / 20 * 1e3, tu / 20 * 1e3);
    // correctness: solve residual
    CK(hipMemcpy(S, S0, sizeof(double) * h.size(), hipMemcpyDeviceToDevice));
    // (factor once more, cleanly)
    for (int p = 0; p < nblk; p++) {
        const int p0 = p * NB, below = nrows - (p0 + NB), g = below > 0 ? (below + 63) / 64 : 1;
        hipLaunchKernelGGL((k_ldlt_panel<double, NB>), dim3(g), dim3(256), 0, st, nrows, ncols, ld, p0, S, Wp, Winv + (size_t)p * NB * NB);
        const int p1 = p0 + NB;
        if (p1 < ncols) { const int nti = (nrows - p1 + 63) / 64, ntj = (ncols - p1 + 63) / 64; hipLaunchKernelGGL((k_ldlt_update<double, NB>), dim3(ntj, nti), dim3(256), 0, st, nrows, ncols, ld, p0, S, Wp); }
    }
    for (int p = nblk - 1; p >= 0; p--) { const int p0 = p * NB; int g = (p0 + 63) / 64; if (g < 1) g = 1; hipLaunchKernelGGL((k_ldlt_backstep<double, NB>), dim3(g), dim3(256), 0, st, ncols, ld, D, p0, S, Winv + (size_t)p * NB * NB, x); }
    CK(hipStreamSynchronize(st));
    std::vector<double> xs(D);
    CK(hipMemcpy(xs.data(), x, sizeof(double) * D, hipMemcpyDeviceToHost));
    double rn = 0, bn = 0;
    for (int r = 0; r < D; r++) {
        double a = 0;
        for (int c = 0; c < D; c++) a += (c <= r ? h[(size_t)c * ld + r] : h[(size_t)r * ld + c]) * xs[c];
        const double b = h[(size_t)r * ld + D];
        rn += (a - b) * (a - b); bn += b * b;
    }
    printf("relative residual |Sx-b|/|b| = %.3e\n", std::sqrt(rn / bn));
#ifdef BA_STAMP
    CK(hipMemcpy(S, S0, sizeof(double) * h.size(), hipMemcpyDeviceToDevice));
    for (int r = 0; r < (argc > 2 ? atoi(argv[2]) : 1); r++) // (argv[2] > 1: is the instruction cache still warm in the next launch?)
        hipLaunchKernelGGL((k_ldlt_panel<double, NB>), dim3(1), dim3(256), 0, st, nrows, ncols, ld, 0, S, Wp, Winv);
    CK(hipStreamSynchronize(st));
    long long hs[64]; CK(hipMemcpyFromSymbol(hs, HIP_SYMBOL(ba_stamp_acc), sizeof(hs)));
    for (int w = 0; w < 4; w++) printf("classic panel wave %d: preamble %lld\n", w, hs[8 * w + 7]);
    { long long ho[16]; CK(hipMemcpyFromSymbol(ho, HIP_SYMBOL(ba_stamp_own), sizeof(ho)));
      for (int w = 0; w < 2; w++) printf("classic panel (no look-ahead work): wave %d own work per pivot-loop phase: %lld %lld %lld %lld\n", w, ho[4 * w], ho[4 * w + 1], ho[4 * w + 2], ho[4 * w + 3]);
      long long hp[16]; CK(hipMemcpyFromSymbol(hp, HIP_SYMBOL(ba_stamp_piv), sizeof(hp)));
      for (int ph = 0; ph < 4; ph++) printf("classic panel: factor wave, phase %d: tile in registers at %lld, fifteen pivots done at %lld\n", ph, hp[4 * ph], hp[4 * ph + 1]); }
    { // stamps of a fused step in the middle of the factorisation (block column 8) and its duration
        CK(hipMemcpy(S, S0, sizeof(double) * h.size(), hipMemcpyDeviceToDevice));
        hipEvent_t f0, f1; CK(hipEventCreate(&f0)); CK(hipEventCreate(&f1));
        for (int p = 0; p <= 8 && p < nblk; p++) {
            const int p0 = p * NB, below = nrows - (p0 + NB), g = below > 0 ? (below + 63) / 64 : 1;
            double *wcur = Wp + (size_t)p * ld * NB, *wprev = Wp + (size_t)(p ? p - 1 : 0) * ld * NB;
            if (p == 0) { hipLaunchKernelGGL((k_ldlt_panel<double, NB>), dim3(g), dim3(256), 0, st, nrows, ncols, ld, p0, S, wcur, Winv, flags, nflags); continue; }
            const int nt = (nrows - p0 + 63) / 64, ntc = (ncols - p0 + 63) / 64;
            const int nupd = plan.first[p + 1] - plan.first[p]; (void)nt; (void)ntc;
            if (p == 8) CK(hipEventRecord(f0, st));
            hipLaunchKernelGGL((k_ldlt_step<double, NB, true>), dim3(3 * g + nupd), dim3(256), 8192, st, nrows, ncols, ld, p0, 2 * g, S, wcur, wprev, Winv + (size_t)p * NB * NB, g, flags, (double *)nullptr, 0, (const int4 *)plan.d_jobs + plan.first[p], (const double *)Wp);
            if (p == 8) CK(hipEventRecord(f1, st));
        }
        CK(hipStreamSynchronize(st));
        float fms = 0; CK(hipEventElapsedTime(&fms, f0, f1));
        long long hf[64]; CK(hipMemcpyFromSymbol(hf, HIP_SYMBOL(ba_stamp_acc), sizeof(hf)));
        printf("fused step p=8: %.2f us (event to event); workgroup 0, wave 0: preamble %lld  A1 %lld  A2 %lld  A3 %lld  Wassembly %lld  publish+phaseB %lld  (sum %lld cycles)\n",
               fms * 1e3, hf[7], hf[0], hf[1], hf[3], hf[4], hf[5], hf[7] + hf[0] + hf[1] + hf[2] + hf[3] + hf[4] + hf[5]);
        printf("fused step p=8: own work inside the four A1 phases (before their barriers), waves 0..3: %lld %lld %lld %lld\n", hf[6], hf[14], hf[22], hf[30]);
        long long ho[16]; CK(hipMemcpyFromSymbol(ho, HIP_SYMBOL(ba_stamp_own), sizeof(ho)));
        { long long hp[16]; CK(hipMemcpyFromSymbol(hp, HIP_SYMBOL(ba_stamp_piv), sizeof(hp)));
          for (int ph = 0; ph < 4; ph++) printf("fused step p=8: factor wave, phase %d: tile in registers at %lld, fifteen pivots done at %lld\n", ph, hp[4 * ph], hp[4 * ph + 1]); }
        for (int w = 0; w < 4; w++) printf("fused step p=8: wave %d own work per pivot-loop phase: %lld %lld %lld %lld\n", w, ho[4 * w], ho[4 * w + 1], ho[4 * w + 2], ho[4 * w + 3]);
    }
    for (int w = 0; w < 4; w++)
        printf("wave %d cycles: A1 %lld (own work %lld)  A2 %lld  scale %lld  A3 %lld  Wassembly %lld  publish+phaseB %lld\n", w, hs[8 * w], hs[8 * w + 6], hs[8 * w + 1],
               hs[8 * w + 2], hs[8 * w + 3], hs[8 * w + 4], hs[8 * w + 5]);
#endif
    return 0;
}
