// model_rd.h — model_rd_from_sse (EbInterPrediction.c:3402-3438), the Laplacian rate / distortion model of a block's SSE, once for the
// kernels that cost a prediction by it: fast_pick_kernel (kernel_fast_pick.h) and interp_decide_kernel (kernel_interp_search.h).
#pragma once
#include "dev_common.h"

namespace svtdev {

// model_rd_norm's tables (EbInterPrediction.c:3324-3352); xsq_iq_q10[xq] is ((((xq & 7) + 8) << (xq >> 3)) - 8) << 2
static __device__ const int32_t kFpRateTabQ10[104] = {
    65536, 6086, 5574, 5275, 5063, 4899, 4764, 4651, 4553, 4389, 4255, 4142, 4044, 3958, 3881, 3811, 3748, 3635, 3538, 3453, 3376, 3307,
    3244, 3186, 3133, 3037, 2952, 2877, 2809, 2747, 2690, 2638, 2589, 2501, 2423, 2353, 2290, 2232, 2179, 2130, 2084, 2001, 1928, 1862,
    1802, 1748, 1698, 1651, 1608, 1530, 1460, 1398, 1342, 1290, 1243, 1199, 1159, 1086, 1021, 963, 911, 864, 821, 781, 745, 680, 623,
    574, 530, 490, 455, 424, 395, 345, 304, 269, 239, 213, 190, 171, 154, 126, 104, 87, 73, 61, 52, 44, 38, 28, 21, 16, 12, 10, 8, 6,
    5, 3, 2, 1, 1, 1, 0, 0};
static __device__ const int32_t kFpDistTabQ10[104] = {
    0, 0, 1, 1, 1, 2, 2, 2, 3, 3, 4, 5, 5, 6, 7, 7, 8, 9, 11, 12, 13, 15, 16, 17, 18, 21, 24, 26, 29, 31, 34, 36, 39, 44, 49, 54, 59, 64,
    69, 73, 78, 88, 97, 106, 115, 124, 133, 142, 151, 167, 184, 200, 215, 231, 245, 260, 274, 301, 327, 351, 375, 397, 418, 439, 458,
    495, 528, 559, 587, 613, 637, 659, 680, 717, 749, 777, 801, 823, 842, 859, 874, 899, 919, 936, 949, 960, 969, 977, 983, 994, 1001,
    1006, 1010, 1013, 1015, 1017, 1018, 1020, 1022, 1022, 1023, 1023, 1023, 1024};

// model_rd_from_sse (EbInterPrediction.c:3402-3438) -> av1_model_rd_from_var_lapndz (:3377-3400) -> model_rd_norm (:3311-3375)
__device__ __forceinline__ void fp_model_rd(unsigned long long sse, uint32_t n_log2, uint32_t qstep, uint32_t& rate, unsigned long long& dist) {
    rate = 0; dist = 0;
    if (sse == 0) return;
    const unsigned long long x64 = ((((unsigned long long)qstep * qstep) << (n_log2 + 10)) + (sse >> 1)) / sse;
    const int32_t xsq = (int32_t)(x64 < 245727ull ? x64 : 245727ull);           // MAX_XSQ_Q10
    const int32_t tmp = (xsq >> 2) + 8;
    const int32_t k = (31 - __clz(tmp)) - 3;
    const int32_t xq = (k << 3) + ((tmp >> k) & 7);                              // 0 .. 102
    const int32_t iq = ((((xq & 7) + 8) << (xq >> 3)) - 8) << 2;
    const int32_t a = ((xsq - iq) << 10) >> (2 + k), b = 1024 - a;
    const int32_t r_q10 = (kFpRateTabQ10[xq] * b + kFpRateTabQ10[xq + 1] * a) >> 10;
    const int32_t d_q10 = (kFpDistTabQ10[xq] * b + kFpDistTabQ10[xq + 1] * a) >> 10;
    rate = (uint32_t)(((r_q10 << n_log2) + 1) >> 1);
    dist = (unsigned long long)(((long long)sse * (long long)d_q10 + 512) >> 10) << 4;
}

}  // namespace svtdev
