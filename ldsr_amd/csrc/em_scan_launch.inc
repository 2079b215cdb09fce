// em_scan_launch.inc -- the translation unit of one scan member (em_members.h), compiled with -DSCAN_L=<L>
// -DSCAN_W=<W>: instantiates the scan kernel for every padded (PP, QQ) at that chunk length / wave count in
// the variants scan_variant() names (em_scan_impl.h) and defines the member's launcher.
#include "em_scan_impl.h"
#include "ldsr_kernels.h"

template <int PP, int QQ, bool QUEUE, bool GIMG, bool FIT>
static hipError_t launch_v(const EmParams &prm, int n_blocks, int cpb, hipStream_t stream) {
    constexpr int L = SCAN_L, W = SCAN_W;
    if constexpr (scan_variant(PP, QQ, L, W, QUEUE, GIMG, FIT)) {
        const size_t lds = ((GIMG ? 0 : (size_t)scan_image_doubles(L, W, PP, QQ)) + scan_xch_doubles(W)) * sizeof(double);
        auto kern = em_scan_kernel<PP, QQ, L, W, QUEUE, GIMG, FIT>;
        if (lds > 64 * 1024) {
            hipError_t e = hipFuncSetAttribute((const void *)kern,
                                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            if (e != hipSuccess) return e;
        }
        hipLaunchKernelGGL(kern, dim3(n_blocks), dim3(64 * W * cpb), lds, stream, prm);
        return hipGetLastError();
    }
    return hipErrorInvalidValue;
}

// (launch_em_scan hands over a schedule the image form has: FIT without the queue, the global image with it)
template <int PP, int QQ>
static hipError_t launch_one(const EmParams &prm, int n_blocks, int cpb, bool queue, bool gimg,
                             bool fit, hipStream_t stream) {
    if (fit) return gimg ? launch_v<PP, QQ, false, true, true>(prm, n_blocks, cpb, stream)
                         : launch_v<PP, QQ, false, false, true>(prm, n_blocks, cpb, stream);
    if (gimg) return launch_v<PP, QQ, true, true, false>(prm, n_blocks, cpb, stream);
    return queue ? launch_v<PP, QQ, true, false, false>(prm, n_blocks, cpb, stream)
                 : launch_v<PP, QQ, false, false, false>(prm, n_blocks, cpb, stream);
}

template <>
hipError_t launch_em_scan_LW<SCAN_L, SCAN_W>(const EmParams &prm, int PPv, int QQv, int n_blocks,
                                             int cpb, bool queue, bool gimg, bool fit,
                                             hipStream_t stream) {
    switch (PPv * 16 + QQv) {
#define CASE_PQ(a, b) case a * 16 + b: return launch_one<a, b>(prm, n_blocks, cpb, queue, gimg, fit, stream);
        CASE_PQ(1, 1) CASE_PQ(1, 2) CASE_PQ(1, 4) CASE_PQ(1, 8)
        CASE_PQ(2, 1) CASE_PQ(2, 2) CASE_PQ(2, 4) CASE_PQ(2, 8)
        CASE_PQ(4, 1) CASE_PQ(4, 2) CASE_PQ(4, 4) CASE_PQ(4, 8)
        CASE_PQ(8, 1) CASE_PQ(8, 2) CASE_PQ(8, 4) CASE_PQ(8, 8)
#undef CASE_PQ
        default: return hipErrorInvalidValue;
    }
}
