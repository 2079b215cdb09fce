// api_pcr.hip -- the principal-component regression entry of the C ABI (R/PCR.R).
#include <hip/hip_runtime.h>

#include <cstring>
#include <vector>

#include "host_runtime.h"
#include "pcr.h"

namespace ldsr_host {

static int pcr_fail(int code, const std::string &msg) { return fail(code, "ldsr_pcr_batch: " + msg); }

extern "C" int ldsr_pcr_batch(int device, int n_members, int n, const int *k, const double *X, const double *y,
                              int n_folds, const unsigned char *heldout, int N, const double *Xpred,
                              double *pred, double *lev, double *coef, double *sigma, int *df, int *status) {
    // every check before any HIP call
    if (n_members < 1) return pcr_fail(LDSR_EINVAL, "n_members must be >= 1");
    if (n < 2) return pcr_fail(LDSR_EINVAL, "n must be >= 2");
    if (n_folds < 1) return pcr_fail(LDSR_EINVAL, "n_folds must be >= 1");
    if (!k) return pcr_fail(LDSR_EINVAL, "k must not be NULL");
    if (!X) return pcr_fail(LDSR_EINVAL, "X must not be NULL");
    if (!y) return pcr_fail(LDSR_EINVAL, "y must not be NULL");
    if (!heldout) return pcr_fail(LDSR_EINVAL, "heldout must not be NULL (an all-zero row is the plain fit)");
    if (!pred || !status) return pcr_fail(LDSR_EINVAL, "pred and status must not be NULL");
    if (Xpred ? N < 1 : N != n) return pcr_fail(LDSR_EINVAL, Xpred ? "N must be >= 1" : "N must equal n when Xpred is NULL");
    int kmax = 0;
    size_t ktot = 0;
    std::vector<long long> coff((size_t)n_members);
    for (int m = 0; m < n_members; m++) {
        if (k[m] < 1) return pcr_fail(LDSR_EINVAL, "k[" + std::to_string(m) + "] must be >= 1");
        if (k[m] > PCR_MAXK)
            return pcr_fail(LDSR_EUNSUPPORTED, "k[" + std::to_string(m) + "] = " + std::to_string(k[m]) +
                                                   " is above the compiled limit of " + std::to_string(PCR_MAXK));
        coff[m] = (long long)ktot;
        ktot += (size_t)k[m];
        if (k[m] > kmax) kmax = k[m];
    }
    if ((size_t)n * (kmax + 2) > PCR_MAX_WORK)
        return pcr_fail(LDSR_EUNSUPPORTED, "n * (max k + 2) = " + std::to_string((size_t)n * (kmax + 2)) +
                                               " is above " + std::to_string(PCR_MAX_WORK) + ", what one cell's design may take in LDS");
    const size_t cells = (size_t)n_members * n_folds;
    if (cells > 0x7fffffffull) return pcr_fail(LDSR_EINVAL, "n_members * n_folds must be below 2^31");
    for (size_t i = 0; i < (size_t)n_folds * n; i++)
        if (heldout[i] > 1) return pcr_fail(LDSR_EINVAL, "heldout must hold 0 / 1 only (byte " + std::to_string(i) + ")");

    ArenaLease lease;
    int rc = arena_acquire(device, &lease.a);
    if (rc) return rc;
    Arena *A = lease.a;
    Carver c;
    const size_t b_k = sizeof(int) * (size_t)n_members, b_off = sizeof(long long) * (size_t)n_members;
    const size_t b_X = sizeof(double) * ktot * n, b_y = sizeof(double) * (size_t)n, b_ho = (size_t)n_folds * n;
    const size_t b_Xp = Xpred ? sizeof(double) * ktot * N : 0;
    const size_t o_k = c.take(b_k), o_off = c.take(b_off), o_X = c.take(b_X), o_y = c.take(b_y);
    const size_t o_ho = c.take(b_ho), o_Xp = c.take(b_Xp);
    const size_t in_bytes = c.o;
    const size_t b_pred = sizeof(double) * cells * N;
    const size_t o_pred = c.take(b_pred), o_lev = c.take(lev ? b_pred : 0);
    const size_t o_coef = c.take(coef ? sizeof(double) * cells * PCR_COEF_STRIDE : 0);
    const size_t o_sig = c.take(sigma ? sizeof(double) * cells : 0);
    const size_t o_df = c.take(df ? sizeof(int) * cells : 0), o_st = c.take(sizeof(int) * cells);
    rc = arena_reserve(A, c, in_bytes, "ldsr_pcr_batch");
    if (rc) return rc;
    char *dev = A->dev, *pin = A->pin;
    memcpy(pin + o_k, k, b_k);
    memcpy(pin + o_off, coff.data(), b_off);
    memcpy(pin + o_X, X, b_X);
    memcpy(pin + o_y, y, b_y);
    memcpy(pin + o_ho, heldout, b_ho);
    if (Xpred) memcpy(pin + o_Xp, Xpred, b_Xp);
    HIPCHK(hipMemcpyAsync(dev, pin, in_bytes, hipMemcpyHostToDevice, A->stream));
    PcrParams p;
    p.n_members = n_members; p.n = n; p.n_folds = n_folds; p.N = N; p.kmax = kmax;
    p.k = (const int *)(dev + o_k);
    p.coff = (const long long *)(dev + o_off);
    p.X = (const double *)(dev + o_X);
    p.y = (const double *)(dev + o_y);
    p.heldout = (const unsigned char *)(dev + o_ho);
    p.Xpred = Xpred ? (const double *)(dev + o_Xp) : nullptr;
    p.pred = (double *)(dev + o_pred);
    p.lev = lev ? (double *)(dev + o_lev) : nullptr;
    p.coef = coef ? (double *)(dev + o_coef) : nullptr;
    p.sigma = sigma ? (double *)(dev + o_sig) : nullptr;
    p.df = df ? (int *)(dev + o_df) : nullptr;
    p.status = (int *)(dev + o_st);
    HIPCHK(launch_pcr(p, A->stream));
    HIPCHK(hipMemcpyAsync(pred, dev + o_pred, b_pred, hipMemcpyDeviceToHost, A->stream));
    if (lev) HIPCHK(hipMemcpyAsync(lev, dev + o_lev, b_pred, hipMemcpyDeviceToHost, A->stream));
    if (coef) HIPCHK(hipMemcpyAsync(coef, dev + o_coef, sizeof(double) * cells * PCR_COEF_STRIDE, hipMemcpyDeviceToHost, A->stream));
    if (sigma) HIPCHK(hipMemcpyAsync(sigma, dev + o_sig, sizeof(double) * cells, hipMemcpyDeviceToHost, A->stream));
    if (df) HIPCHK(hipMemcpyAsync(df, dev + o_df, sizeof(int) * cells, hipMemcpyDeviceToHost, A->stream));
    HIPCHK(hipMemcpyAsync(status, dev + o_st, sizeof(int) * cells, hipMemcpyDeviceToHost, A->stream));
    HIPCHK(hipStreamSynchronize(A->stream));
    return LDSR_OK;
}

}  // namespace ldsr_host
