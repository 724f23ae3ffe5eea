// Test harness of the relative-pose kernels (bundleadjustment_benchmarks_amd/csrc/ba_relpose.hip.h) -- TEST INFRASTRUCTURE ONLY.
// tests/test_gpu_relpose_kernels.py compiles it with the library's flags (csrc/Makefile) into a shared object of its own: the library's
// kernels, unchanged, in the grids the solver launches them in, on lists from the host; everything they leave comes back.
// Every output buffer is filled with RPH_BYTE before the launch (or holds what the caller passed in) and has RPH_GUARD scalars of
// RPH_BYTE behind it: "not written" is a byte comparison on the host, and guards[] is 1 where the words behind a buffer are intact.
#include "ba_relpose.hip.h"
#include <cstdlib>
#include <cstring>

#define RPH_GUARD 1024 /* guard scalars behind every output buffer */
#define RPH_BYTE 0xA5  /* fill byte of the guards and of the outputs */

static bool guard_intact(const void *dev, size_t bytes, hipError_t *e)
{
    unsigned char *g = (unsigned char *)malloc(bytes);
    if (!g) { *e = hipErrorOutOfMemory; return false; }
    bool ok = (*e = hipMemcpy(g, dev, bytes, hipMemcpyDeviceToHost)) == hipSuccess;
    for (size_t i = 0; ok && i < bytes; i++) ok = g[i] == RPH_BYTE;
    free(g);
    return ok;
}

// a device buffer of `bytes` with the guard behind it; src: its contents (nullptr: RPH_BYTE)
static hipError_t dev_out(void **d, size_t bytes, size_t guard, const void *src)
{
    hipError_t e = hipMalloc(d, bytes + guard);
    if (e != hipSuccess) return e;
    if ((e = hipMemset(*d, RPH_BYTE, bytes + guard)) != hipSuccess) return e;
    return src && bytes ? hipMemcpy(*d, src, bytes, hipMemcpyHostToDevice) : hipSuccess;
}

static hipError_t dev_in(void **d, size_t bytes, const void *src)
{
    hipError_t e = hipMalloc(d, bytes ? bytes : 1);
    if (e != hipSuccess || !bytes) return e;
    return hipMemcpy(*d, src, bytes, hipMemcpyHostToDevice);
}

#define RCK(x) do { if ((e = (x)) != hipSuccess) goto out; } while (0)

// k_relpose<T, LIN, MASK> in launch_relpose's grid.  mode: 0 LIN, 1 LIN + MASK, 2 the trial part.  go: < 0 no go word, else its value.
// rec [n][BA_RP_REC], part_e and part_keep [2][grid] come back as the kernel left them.  guards[3]: behind rec, part_e, part_keep.
template <typename T>
static int run_relpose(int mode, int n, int N, const T *cam, const int *pair, const T *R0, const T *t0, const T *Lr, const T *Lt,
                       const unsigned short *cmask, int go, T *rec, T *part_e, T *part_keep, int *guards)
{
    const unsigned grid = (unsigned)((n + 255) / 256);
    const size_t bR = sizeof(T) * (size_t)n * BA_RP_REC, bP = sizeof(T) * 2 * (size_t)grid, bG = sizeof(T) * RPH_GUARD;
    void *dcam = nullptr, *dpair = nullptr, *dR0 = nullptr, *dt0 = nullptr, *dLr = nullptr, *dLt = nullptr, *dmask = nullptr, *dgo = nullptr;
    void *drec = nullptr, *dpe = nullptr, *dpk = nullptr;
    hipError_t e = hipSuccess;
    RCK(dev_in(&dcam, sizeof(T) * 15 * (size_t)N, cam));
    RCK(dev_in(&dpair, sizeof(int) * 2 * (size_t)n, pair));
    RCK(dev_in(&dR0, sizeof(T) * 9 * (size_t)n, R0));
    RCK(dev_in(&dt0, sizeof(T) * 3 * (size_t)n, t0));
    RCK(dev_in(&dLr, sizeof(T) * 9 * (size_t)n, Lr));
    RCK(dev_in(&dLt, sizeof(T) * 9 * (size_t)n, Lt));
    RCK(dev_in(&dmask, sizeof(unsigned short) * (size_t)N, cmask));
    if (go >= 0) RCK(dev_in(&dgo, sizeof(int), &go));
    RCK(dev_out(&drec, bR, bG, nullptr));
    RCK(dev_out(&dpe, bP, bG, nullptr));
    RCK(dev_out(&dpk, bP, bG, nullptr));
    {
        ba_relpose_args<T> ra{n, (const int *)dpair, (const T *)dR0, (const T *)dt0, (const T *)dLr, (const T *)dLt};
#define RPH_LAUNCH(L, M) hipLaunchKernelGGL((k_relpose<T, L, M>), dim3(grid), dim3(256), 0, 0, ra, N, (const T *)dcam, (T *)drec, (T *)dpe, \
                                            (T *)dpk, (const int *)dgo, (const unsigned short *)dmask)
        if (mode == 0) RPH_LAUNCH(true, false);
        else if (mode == 1) RPH_LAUNCH(true, true);
        else RPH_LAUNCH(false, false);
#undef RPH_LAUNCH
    }
    RCK(hipGetLastError());
    RCK(hipDeviceSynchronize());
    RCK(hipMemcpy(rec, drec, bR, hipMemcpyDeviceToHost));
    RCK(hipMemcpy(part_e, dpe, bP, hipMemcpyDeviceToHost));
    RCK(hipMemcpy(part_keep, dpk, bP, hipMemcpyDeviceToHost));
    guards[0] = guard_intact((char *)drec + bR, bG, &e);
    if (e == hipSuccess) guards[1] = guard_intact((char *)dpe + bP, bG, &e);
    if (e == hipSuccess) guards[2] = guard_intact((char *)dpk + bP, bG, &e);
out:
    (void)hipDeviceSynchronize();
    (void)hipFree(dcam); (void)hipFree(dpair); (void)hipFree(dR0); (void)hipFree(dt0); (void)hipFree(dLr); (void)hipFree(dLt);
    (void)hipFree(dmask); (void)hipFree(dgo); (void)hipFree(drec); (void)hipFree(dpe); (void)hipFree(dpk);
    return (int)e;
}

extern "C" int rph_relpose(int fp32, int mode, int n, int N, const void *cam, const int *pair, const void *R0, const void *t0, const void *Lr,
                           const void *Lt, const unsigned short *cmask, int go, void *rec, void *part_e, void *part_keep, int *guards)
{
    if (n < 1 || N < 1 || mode < 0 || mode > 2) return -1;
    for (int k = 0; k < 2 * n; k++)
        if (pair[k] < 0 || pair[k] >= N) return -1;
    return fp32 ? run_relpose<float>(mode, n, N, (const float *)cam, pair, (const float *)R0, (const float *)t0, (const float *)Lr,
                                     (const float *)Lt, cmask, go, (float *)rec, (float *)part_e, (float *)part_keep, guards)
                : run_relpose<double>(mode, n, N, (const double *)cam, pair, (const double *)R0, (const double *)t0, (const double *)Lr,
                                      (const double *)Lt, cmask, go, (double *)rec, (double *)part_e, (double *)part_keep, guards);
}

// the CSR of the cameras' incident constraints on the device; false: an entry out of range
static bool csr_in_range(int N, int n, const int *ptr, const int *inc, const int *pair)
{
    if (N < 1 || n < 1 || ptr[0] != 0 || ptr[N] < 0 || ptr[N] > 2 * n) return false;
    for (int a = 0; a < N; a++)
        if (ptr[a + 1] < ptr[a]) return false;
    for (int k = 0; k < ptr[N]; k++)
        if (inc[k] < 0 || inc[k] >= 2 * n) return false;
    for (int k = 0; k < 2 * n; k++)
        if (pair[k] < 0 || pair[k] >= N) return false;
    return true;
}

// k_relpose_gather<T> in launch_relpose's grid: V [N][81] and gc [9 N] go in and come back.  guards[2]: behind V, gc.
template <typename T>
static int run_gather(int N, int n, const int *ptr, const int *inc, const int *pair, const T *rec, int go, T *V, T *gc, int *guards)
{
    const size_t bV = sizeof(T) * 81 * (size_t)N, bg = sizeof(T) * 9 * (size_t)N, bG = sizeof(T) * RPH_GUARD;
    void *dptr = nullptr, *dinc = nullptr, *dpair = nullptr, *drec = nullptr, *dgo = nullptr, *dV = nullptr, *dgc = nullptr;
    hipError_t e = hipSuccess;
    RCK(dev_in(&dptr, sizeof(int) * ((size_t)N + 1), ptr));
    RCK(dev_in(&dinc, sizeof(int) * 2 * (size_t)n, inc));
    RCK(dev_in(&dpair, sizeof(int) * 2 * (size_t)n, pair));
    RCK(dev_in(&drec, sizeof(T) * (size_t)n * BA_RP_REC, rec));
    if (go >= 0) RCK(dev_in(&dgo, sizeof(int), &go));
    RCK(dev_out(&dV, bV, bG, V));
    RCK(dev_out(&dgc, bg, bG, gc));
    {
        ba_relpose_csr<T> cs{(const int *)dptr, (const int *)dinc, (const int *)dpair, (const T *)drec};
        hipLaunchKernelGGL((k_relpose_gather<T>), dim3((unsigned)(((size_t)N * BA_RP_ENT + 255) / 256)), dim3(256), 0, 0, N, cs, (T *)dV, (T *)dgc,
                           (const int *)dgo);
    }
    RCK(hipGetLastError());
    RCK(hipDeviceSynchronize());
    RCK(hipMemcpy(V, dV, bV, hipMemcpyDeviceToHost));
    RCK(hipMemcpy(gc, dgc, bg, hipMemcpyDeviceToHost));
    guards[0] = guard_intact((char *)dV + bV, bG, &e);
    if (e == hipSuccess) guards[1] = guard_intact((char *)dgc + bg, bG, &e);
out:
    (void)hipDeviceSynchronize();
    (void)hipFree(dptr); (void)hipFree(dinc); (void)hipFree(dpair); (void)hipFree(drec); (void)hipFree(dgo); (void)hipFree(dV); (void)hipFree(dgc);
    return (int)e;
}

// inc holds 2 n entries (ptr[N] of them are read)
extern "C" int rph_gather(int fp32, int N, int n, const int *ptr, const int *inc, const int *pair, const void *rec, int go, void *V, void *gc,
                          int *guards)
{
    if (!csr_in_range(N, n, ptr, inc, pair)) return -1;
    return fp32 ? run_gather<float>(N, n, ptr, inc, pair, (const float *)rec, go, (float *)V, (float *)gc, guards)
                : run_gather<double>(N, n, ptr, inc, pair, (const double *)rec, go, (double *)V, (double *)gc, guards);
}

// k_relpose_schur<T> in launch_schur's grid: S [9 N][ld] goes in and comes back.  guards[1]: behind S.
template <typename T> static int run_schur(int n, int N, const int *pair, const T *rec, int ld, T *S, int *guards)
{
    const size_t bS = sizeof(T) * (size_t)ld * 9 * (size_t)N, bG = sizeof(T) * RPH_GUARD;
    void *dpair = nullptr, *drec = nullptr, *dS = nullptr;
    hipError_t e = hipSuccess;
    RCK(dev_in(&dpair, sizeof(int) * 2 * (size_t)n, pair));
    RCK(dev_in(&drec, sizeof(T) * (size_t)n * BA_RP_REC, rec));
    RCK(dev_out(&dS, bS, bG, S));
    hipLaunchKernelGGL((k_relpose_schur<T>), dim3((unsigned)(((size_t)n * 36 + 255) / 256)), dim3(256), 0, 0, n, (const int *)dpair, (const T *)drec, ld,
                       (T *)dS);
    RCK(hipGetLastError());
    RCK(hipDeviceSynchronize());
    RCK(hipMemcpy(S, dS, bS, hipMemcpyDeviceToHost));
    guards[0] = guard_intact((char *)dS + bS, bG, &e);
out:
    (void)hipDeviceSynchronize();
    (void)hipFree(dpair); (void)hipFree(drec); (void)hipFree(dS);
    return (int)e;
}

extern "C" int rph_schur(int fp32, int n, int N, const int *pair, const void *rec, int ld, void *S, int *guards)
{
    if (n < 1 || N < 1 || ld < 9 * N) return -1;
    for (int k = 0; k < 2 * n; k++)
        if (pair[k] < 0 || pair[k] >= N) return -1;
    return fp32 ? run_schur<float>(n, N, pair, (const float *)rec, ld, (float *)S, guards)
                : run_schur<double>(n, N, pair, (const double *)rec, ld, (double *)S, guards);
}

// ba_relpose_matvec_row as k_pcg_relpose calls it: one thread per (camera, row 0..8), `val` a plain read of v
template <typename T> __global__ __launch_bounds__(256) void k_rph_matvec(int N, ba_relpose_csr<T> cs, const T *__restrict__ v, T *__restrict__ y)
{
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t a = idx / 9;
    const int r = (int)(idx - 9 * a);
    if (a < (size_t)N) y[9 * a + r] = ba_relpose_matvec_row<T>(cs, (int)a, r, [&](size_t o) { return v[o]; });
}

// y [9 N] comes back.  guards[1]: behind y.
template <typename T> static int run_matvec(int N, int n, const int *ptr, const int *inc, const int *pair, const T *rec, const T *v, T *y, int *guards)
{
    const size_t by = sizeof(T) * 9 * (size_t)N, bG = sizeof(T) * RPH_GUARD;
    void *dptr = nullptr, *dinc = nullptr, *dpair = nullptr, *drec = nullptr, *dv = nullptr, *dy = nullptr;
    hipError_t e = hipSuccess;
    RCK(dev_in(&dptr, sizeof(int) * ((size_t)N + 1), ptr));
    RCK(dev_in(&dinc, sizeof(int) * 2 * (size_t)n, inc));
    RCK(dev_in(&dpair, sizeof(int) * 2 * (size_t)n, pair));
    RCK(dev_in(&drec, sizeof(T) * (size_t)n * BA_RP_REC, rec));
    RCK(dev_in(&dv, by, v));
    RCK(dev_out(&dy, by, bG, nullptr));
    {
        ba_relpose_csr<T> cs{(const int *)dptr, (const int *)dinc, (const int *)dpair, (const T *)drec};
        hipLaunchKernelGGL((k_rph_matvec<T>), dim3((unsigned)((9 * (size_t)N + 255) / 256)), dim3(256), 0, 0, N, cs, (const T *)dv, (T *)dy);
    }
    RCK(hipGetLastError());
    RCK(hipDeviceSynchronize());
    RCK(hipMemcpy(y, dy, by, hipMemcpyDeviceToHost));
    guards[0] = guard_intact((char *)dy + by, bG, &e);
out:
    (void)hipDeviceSynchronize();
    (void)hipFree(dptr); (void)hipFree(dinc); (void)hipFree(dpair); (void)hipFree(drec); (void)hipFree(dv); (void)hipFree(dy);
    return (int)e;
}

extern "C" int rph_matvec(int fp32, int N, int n, const int *ptr, const int *inc, const int *pair, const void *rec, const void *v, void *y, int *guards)
{
    if (!csr_in_range(N, n, ptr, inc, pair)) return -1;
    return fp32 ? run_matvec<float>(N, n, ptr, inc, pair, (const float *)rec, (const float *)v, (float *)y, guards)
                : run_matvec<double>(N, n, ptr, inc, pair, (const double *)rec, (const double *)v, (double *)y, guards);
}

extern "C" int rph_cfg(int *rec, int *hab, int *g, int *ent)
{
    *rec = BA_RP_REC; *hab = BA_RP_HAB; *g = BA_RP_G; *ent = BA_RP_ENT;
    return 0;
}
