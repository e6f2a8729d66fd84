// quant_params.h — the quantiser scalars of one launch and their derivation from the reference's tables.  Plain C++17, no HIP header:
// dev_common.h includes it for the struct, svt_hip_txfm.hip and md_plan.h for the function (pure host arithmetic).
#pragma once
#include <stdint.h>

namespace svtdev {
// Quantizer scalars for one launch: index 0 = DC (coefficient 0), 1 = AC.
// Derived on the host from the reference's five int16[8] tables
// (EbFullLoop.c:239-296): zbin/round already ROUND_POWER_OF_TWO'ed by
// log_scale; quant_m = quant + 65536 (so ((t*quant)>>16)+t == (t*quant_m)>>16).
struct QParams {
    int32_t zbin[2];
    int32_t round[2];
    uint32_t quant_m[2];
    int32_t quant_shift[2];
    int32_t dequant[2];
    int32_t log_scale;
    // POW2 fast path (host-checked): quant_shift = 2^k, so the two-step reference
    // formula collapses to  aq = (t1 * quant_m) >> fast_sh  with fast_sh = 32 - log_scale - k
    int32_t fast_sh[2];
    int32_t fast_ok;
    // the same collapse as ONE multiply: with quant_hi = quant_m << (31 - fast_sh) (fits 32 bits: quant_m < 2^17, fast_sh >= 16),
    // aq = mulhi_u32(2 * t1, quant_hi) = floor(t1 * quant_m / 2^fast_sh) exactly; zbin2 / round2 are the doubled thresholds
    uint32_t quant_hi[2];
    int32_t zbin2[2];
    int32_t round2[2];
};
inline int rpot(int v, int n) { return n == 0 ? v : ((v + (1 << (n - 1))) >> n); }

inline QParams make_qparams(const int16_t* zbin, const int16_t* round, const int16_t* quant,
                            const int16_t* quant_shift, const int16_t* dequant, int log_scale) {
    QParams qp;
    for (int i = 0; i < 2; i++) {
        qp.zbin[i] = rpot(zbin[i], log_scale);       // EbFullLoop.c:248-249
        qp.round[i] = rpot(round[i], log_scale);     // :277
        qp.quant_m[i] = (uint32_t)((int)quant[i] + 65536);
        qp.quant_shift[i] = quant_shift[i];
        qp.dequant[i] = dequant[i];
    }
    qp.log_scale = log_scale;
    qp.fast_ok = 1;
    for (int i = 0; i < 2; i++) {
        const int qs = quant_shift[i];
        int k = -1;
        if (qs > 0 && (qs & (qs - 1)) == 0) { k = 0; while ((1 << k) != qs) k++; }
        const int sh = 32 - log_scale - k;
        qp.fast_sh[i] = sh;
        if (k < 0 || sh < 16 || sh > 31 || dequant[i] < 0 || qp.round[i] < 0 || qp.quant_m[i] >= (1u << 17)) qp.fast_ok = 0;
        qp.quant_hi[i] = (sh >= 16 && sh <= 31) ? qp.quant_m[i] << (31 - sh) : 0u;
        qp.zbin2[i] = 2 * qp.zbin[i];
        qp.round2[i] = 2 * qp.round[i];
    }
    return qp;
}
}  // namespace svtdev
