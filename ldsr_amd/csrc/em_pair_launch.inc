// em_pair_launch.inc -- the translation unit of one pair member (em_members.h), compiled with -DPAIR_L=<L>
// -DPAIR_LPC=<32: two cells per wave | 16: four>: instantiates the kernel of em_pair_impl.h for every padded
// (PP, QQ) at that chunk length in the variants pair_variant() names and defines the member's launcher (which
// exists for every member, even where no (PP, QQ) has a variant: it then returns hipErrorInvalidValue).
#include "em_pair_impl.h"
#include "ldsr_kernels.h"

template <int PP, int QQ, bool QUEUE, bool LEAD>
static hipError_t pair_launch_v(const EmParams &prm, int n_blocks, int wpb, hipStream_t stream) {
    constexpr int L = PAIR_L;
    if constexpr (pair_variant(PP, QQ, L, PAIR_LPC, QUEUE, LEAD)) {
        const size_t lds = ((size_t)pair_image_doubles(L, PP, QQ, PAIR_LPC) + (size_t)wpb * pair_strip_doubles(L) +
                            (LEAD ? (size_t)pair_lead_doubles(prm.lead, PAIR_LPC, PP) : 0) +
                            (!LEAD && pair_steady(L, PAIR_LPC, PP, QQ) ? (size_t)pair_tri_doubles(PP, QQ, PAIR_LPC) : 0)) * sizeof(double);
        if (lds > 160 * 1024) return hipErrorInvalidValue;
        auto kern = em_pair_kernel<PP, QQ, L, PAIR_LPC, QUEUE, LEAD>;
        if (lds > 64 * 1024) {
            hipError_t e = hipFuncSetAttribute((const void *)kern,
                                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            if (e != hipSuccess) return e;
        }
        hipLaunchKernelGGL(kern, dim3(n_blocks), dim3(64 * wpb), lds, stream, prm);
        return hipGetLastError();
    }
    return hipErrorInvalidValue;
}

template <>
hipError_t launch_em_pair_L<PAIR_L, PAIR_LPC>(const EmParams &prm, int PPv, int QQv, int n_blocks, int wpb,
                                    bool queue, hipStream_t stream) {
    const bool lead = prm.lead > 0;     // LEAD form: closed form for an all-missing lead
    switch (PPv * 16 + QQv) {
#define CASE_PQ(a, b)                                                                                  \
    case a * 16 + b:                                                                                   \
        return lead ? (queue ? pair_launch_v<a, b, true, true>(prm, n_blocks, wpb, stream)             \
                             : pair_launch_v<a, b, false, true>(prm, n_blocks, wpb, stream))           \
                    : (queue ? pair_launch_v<a, b, true, false>(prm, n_blocks, wpb, stream)            \
                             : pair_launch_v<a, b, false, false>(prm, n_blocks, wpb, stream));
        CASE_PQ(1, 1) CASE_PQ(1, 2) CASE_PQ(1, 4) CASE_PQ(1, 8)
        CASE_PQ(2, 1) CASE_PQ(2, 2) CASE_PQ(2, 4) CASE_PQ(2, 8)
        CASE_PQ(4, 1) CASE_PQ(4, 2) CASE_PQ(4, 4) CASE_PQ(4, 8)
        CASE_PQ(8, 1) CASE_PQ(8, 2) CASE_PQ(8, 4) CASE_PQ(8, 8)
#undef CASE_PQ
        default: return hipErrorInvalidValue;
    }
}
