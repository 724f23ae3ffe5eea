// Test harness of the dense Householder QR (bundleadjustment_benchmarks_amd/csrc/ba_qr.hip.h) -- TEST INFRASTRUCTURE ONLY.
// tests/test_gpu_dense_qr.py compiles it with the library's flags (csrc/Makefile) into a shared object of its own: the kernels run as
// the solver runs them (ba_qr_factor, then ba_qr_backsolve), on a matrix from the host, and everything they leave comes back.
#include "ba_mfma.hip.h"
#define BA_REC 32 /* (ba_kernels.hip.h: scalars per observation record; only k_qrkit_build, unused here, needs it) */
#include "ba_qr.hip.h"
#include <cstring>

#define QRH_GUARD 4096 /* guard words behind every buffer */
#define QRH_BYTE 0xA5  /* fill byte of the guards, of the T storage and of y */

extern "C" int qrh_cfg(int fp32, int *ch, int *tau_levels)
{
    *ch = fp32 ? ba_qr_cfg<float>::CH : ba_qr_cfg<double>::CH;
    *tau_levels = BA_QR_TAU_LEVELS;
    return 0;
}

// the T storage of one level, as the solver sizes it: (ceil(m / CH) + 2) 32 x 32 factors
template <typename T> static size_t tau_stride(int m) { return (size_t)((m + ba_qr_cfg<T>::CH - 1) / ba_qr_cfg<T>::CH + 2) * BA_QR_PB * BA_QR_PB; }

extern "C" size_t qrh_tau_stride(int fp32, int m) { return fp32 ? tau_stride<float>(m) : tau_stride<double>(m); }

static bool guard_intact(const unsigned char *g, size_t bytes)
{
    for (size_t i = 0; i < bytes; i++)
        if (g[i] != QRH_BYTE) return false;
    return true;
}

// A: (m + 64) x (D + 1) column-major in T, rows >= m zero, b in column D; overwritten with the factored matrix.  tau: room for
// BA_QR_TAU_LEVELS * qrh_tau_stride(m) scalars, y: D scalars -- both come back as the kernels left them (QRH_BYTE where not written).
// streams: 1 or 2 (the trailing updates on a second stream, the solver's default); go: < 0 no go word, else its value (with a go
// word ba_qr_factor runs alone, as MOREQR's outer QR does, and the back substitution follows only when go != 0); hw_sqrt: the value of
// ba_qr_hw_sqrt_flag.  guards[3]: 1 where the words behind A, tau and y are intact.  Returns 0, or the first HIP error.
template <typename T>
static int run(int m, int D, T *A, int streams, int go, int hw_sqrt, T *tau, T *y, int *guards, float *ms)
{
    const size_t lda = (size_t)m + 64, nA = lda * (size_t)(D + 1), nT = (size_t)BA_QR_TAU_LEVELS * tau_stride<T>(m);
    const size_t bA = sizeof(T) * nA, bT = sizeof(T) * nT, bY = sizeof(T) * (size_t)D, bG = sizeof(T) * QRH_GUARD;
    T *dA = nullptr, *dT = nullptr, *dY = nullptr;
    int *dgo = nullptr;
    hipStream_t st = nullptr, st2 = nullptr;
    hipEvent_t ea = nullptr, eb = nullptr, t0 = nullptr, t1 = nullptr;
    unsigned char *g = nullptr;
    hipError_t e = hipSuccess;
#define QCK(x) do { if ((e = (x)) != hipSuccess) goto out; } while (0)
    QCK(hipMalloc(&dA, bA + bG));
    QCK(hipMalloc(&dT, bT + bG));
    QCK(hipMalloc(&dY, bY + bG));
    QCK(hipMemset((char *)dA + bA, QRH_BYTE, bG));
    QCK(hipMemset(dT, QRH_BYTE, bT + bG));
    QCK(hipMemset(dY, QRH_BYTE, bY + bG));
    QCK(hipMemcpy(dA, A, bA, hipMemcpyHostToDevice));
    QCK(hipMemcpyToSymbol(HIP_SYMBOL(ba_qr_hw_sqrt_flag), &hw_sqrt, sizeof(int)));
    QCK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    QCK(hipEventCreate(&t0));
    QCK(hipEventCreate(&t1));
    {
        ba_qr_side sd;
        if (streams == 2) {
            QCK(hipStreamCreateWithFlags(&st2, hipStreamNonBlocking));
            QCK(hipEventCreateWithFlags(&ea, hipEventDisableTiming));
            QCK(hipEventCreateWithFlags(&eb, hipEventDisableTiming));
            sd.st2 = st2;
            sd.ev_chunk = ea;
            sd.ev_apply = eb;
        }
        if (go >= 0) {
            QCK(hipMalloc(&dgo, sizeof(int)));
            QCK(hipMemcpy(dgo, &go, sizeof(int), hipMemcpyHostToDevice));
            sd.go = dgo;
        }
        QCK(hipDeviceSynchronize());
        QCK(hipEventRecord(t0, st));
        if (go < 0) ba_qr_solve<T>(st, dA, lda, m, D, dT, tau_stride<T>(m), dY, sd);
        else {
            ba_qr_factor<T>(st, dA, lda, m, D, dT, tau_stride<T>(m), sd);
            if (go != 0) ba_qr_backsolve<T>(st, dA, lda, D, dY);
        }
        QCK(hipGetLastError()); // (a launch the runtime refused, e.g. for its dynamic LDS)
        QCK(hipEventRecord(t1, st));
        QCK(hipStreamSynchronize(st));
        QCK(hipEventElapsedTime(ms, t0, t1));
    }
    QCK(hipMemcpy(A, dA, bA, hipMemcpyDeviceToHost));
    QCK(hipMemcpy(tau, dT, bT, hipMemcpyDeviceToHost));
    QCK(hipMemcpy(y, dY, bY, hipMemcpyDeviceToHost));
    g = (unsigned char *)malloc(bG);
    if (!g) { e = hipErrorOutOfMemory; goto out; }
    QCK(hipMemcpy(g, (char *)dA + bA, bG, hipMemcpyDeviceToHost));
    guards[0] = guard_intact(g, bG);
    QCK(hipMemcpy(g, (char *)dT + bT, bG, hipMemcpyDeviceToHost));
    guards[1] = guard_intact(g, bG);
    QCK(hipMemcpy(g, (char *)dY + bY, bG, hipMemcpyDeviceToHost));
    guards[2] = guard_intact(g, bG);
#undef QCK
out:
    free(g);
    if (st) (void)hipStreamSynchronize(st);
    if (st2) (void)hipStreamSynchronize(st2);
    (void)hipFree(dA); (void)hipFree(dT); (void)hipFree(dY); (void)hipFree(dgo);
    if (ea) (void)hipEventDestroy(ea);
    if (eb) (void)hipEventDestroy(eb);
    if (t0) (void)hipEventDestroy(t0);
    if (t1) (void)hipEventDestroy(t1);
    if (st2) (void)hipStreamDestroy(st2);
    if (st) (void)hipStreamDestroy(st);
    return (int)e;
}

extern "C" int qrh_run(int fp32, int m, int D, void *A, int streams, int go, int hw_sqrt, void *tau, void *y, int *guards, float *ms)
{
    if (m < D || D < 1 || (streams != 1 && streams != 2)) return -1;
    return fp32 ? run<float>(m, D, (float *)A, streams, go, hw_sqrt, (float *)tau, (float *)y, guards, ms)
                : run<double>(m, D, (double *)A, streams, go, hw_sqrt, (double *)tau, (double *)y, guards, ms);
}

// the dynamic LDS the back substitution requests for D unknowns, and the device's limit per workgroup
extern "C" int qrh_lds(int fp32, int D, size_t *request, size_t *limit)
{
    *request = (fp32 ? sizeof(float) : sizeof(double)) * (size_t)(D + 64 + 64 * 64);
    int dev = 0, v = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e == hipSuccess) e = hipDeviceGetAttribute(&v, hipDeviceAttributeMaxSharedMemoryPerBlock, dev);
    *limit = (size_t)v;
    return (int)e;
}
