// lr_search.cpp — the Wiener filter derivation, the refinement walk and the picture-level finish of loop restoration on the host
// (lr_search.h), mirrored line for line from EbRestorationPick.c:860-1126, :1278-1387 and :1508-1580, :1724-1756, :1842-2058.
// No HIP header.  Products the reference forms in a signed type are formed with wmul / wadd / wsub below: the same value where
// nothing overflows, and the two's-complement result the compiled reference leaves where something does.
#include "lr_search.h"

#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "host_err.h"
#include "lr_plan.h"
#include "lr_sgr_solve.h"

namespace svthost {

namespace {
constexpr int kWin = LR_WIN, kHalfWin = 3, kHalfWin1 = 4, kFiltStep = 128;      // WIENER_WIN, WIENER_HALFWIN, WIENER_HALFWIN1, WIENER_FILT_STEP
constexpr int64_t kTapScale = (int64_t)1 << 16;                                  // WIENER_TAP_SCALE_FACTOR
constexpr int kIters = 5;                                                        // NUM_WIENER_ITERS
constexpr int kInitFilt[kWin] = {3, -7, 15, 106, 15, -7, 3};                     // WIENER_FILT_TAP{0,1,2,3}_MIDV: the centre is 128 - 2 * (3 - 7 + 15)

inline int64_t wmul(int64_t a, int64_t b) { return (int64_t)((uint64_t)a * (uint64_t)b); }
inline int64_t wadd(int64_t a, int64_t b) { return (int64_t)((uint64_t)a + (uint64_t)b); }
inline int64_t wsub(int64_t a, int64_t b) { return (int64_t)((uint64_t)a - (uint64_t)b); }
inline int64_t wabs(int64_t a) { return a < 0 ? wsub(0, a) : a; }
// the reference's divisions never divide INT64_MIN by -1 on a path a zero pivot has not already left
inline int64_t wdiv(int64_t a, int64_t b) { return (b == -1) ? wsub(0, a) : a / b; }

inline int wrap_index(int i, int win) { const int h1 = (win >> 1) + 1; return i >= h1 ? win - 1 - i : i; }

// linsolve_wiener (:867-907)
int linsolve_wiener(int n, int64_t* A, int stride, int64_t* b, int32_t* x) {
    for (int k = 0; k < n - 1; k++) {
        for (int i = n - 1; i > k; i--) {
            if (wabs(A[(i - 1) * stride + k]) < wabs(A[i * stride + k])) {
                for (int j = 0; j < n; j++) {
                    const int64_t c = A[i * stride + j];
                    A[i * stride + j] = A[(i - 1) * stride + j];
                    A[(i - 1) * stride + j] = c;
                }
                const int64_t c = b[i];
                b[i] = b[i - 1];
                b[i - 1] = c;
            }
        }
        for (int i = k; i < n - 1; i++) {
            if (A[k * stride + k] == 0) return 0;
            const int64_t c = A[(i + 1) * stride + k];
            const int64_t cd = A[k * stride + k];
            for (int j = 0; j < n; j++) A[(i + 1) * stride + j] = wsub(A[(i + 1) * stride + j], wmul(wdiv(wmul(c / 256, A[k * stride + j]), cd), 256));
            b[i + 1] = wsub(b[i + 1], wdiv(wmul(c, b[k]), cd));
        }
    }
    for (int i = n - 1; i >= 0; i--) {
        if (A[i * stride + i] == 0) return 0;
        int64_t c = 0;
        for (int j = i + 1; j <= n - 1; j++) c = wadd(c, wmul(A[i * stride + j], x[j]) / kTapScale);
        x[i] = (int32_t)wdiv(wmul(kTapScale, wsub(b[i], c)), A[i * stride + i]);
    }
    return 1;
}

// the normalisation both updates end with (:938-962, :995-1019)
void normalise_and_solve(int win, int64_t* A, int64_t* B, int32_t* out) {
    const int h1 = (win >> 1) + 1;
    int32_t S[kWin];
    for (int i = 0; i < h1 - 1; ++i)
        A[i] = wsub(A[i], wsub(wadd(wmul(A[h1 - 1], 2), B[i * h1 + h1 - 1]), wmul(2, B[(h1 - 1) * h1 + (h1 - 1)])));
    for (int i = 0; i < h1 - 1; ++i)
        for (int j = 0; j < h1 - 1; ++j)
            B[i * h1 + j] = wsub(B[i * h1 + j], wmul(2, wsub(wadd(B[i * h1 + (h1 - 1)], B[(h1 - 1) * h1 + j]), wmul(2, B[(h1 - 1) * h1 + (h1 - 1)]))));
    if (linsolve_wiener(h1 - 1, B, h1, A, S)) {
        S[h1 - 1] = (int32_t)kTapScale;
        for (int i = h1; i < win; ++i) {
            S[i] = S[win - 1 - i];
            S[h1 - 1] = (int32_t)((uint32_t)S[h1 - 1] - 2u * (uint32_t)S[i]);
        }
        memcpy(out, S, (size_t)win * sizeof(*out));
    }
}

// update_a_sep_sym (:909-962): fix b, update a.  Mc[i][j] = M[i * win + j]; Hc[i * win + j] = H + i * win * win2 + j * win
void update_a_sep_sym(int win, const int64_t* M, const int64_t* H, int32_t* a, const int32_t* b) {
    int64_t A[kHalfWin1], B[kHalfWin1 * kHalfWin1];
    const int win2 = win * win, h1 = (win >> 1) + 1;
    memset(A, 0, sizeof(A));
    memset(B, 0, sizeof(B));
    for (int i = 0; i < win; i++)
        for (int j = 0; j < win; ++j) A[wrap_index(j, win)] = wadd(A[wrap_index(j, win)], wmul(M[i * win + j], b[i]) / kTapScale);
    for (int i = 0; i < win; i++)
        for (int j = 0; j < win; j++) {
            const int64_t* Hc = H + (size_t)j * win * win2 + (size_t)i * win;      // Hc[j * win + i]
            for (int k = 0; k < win; ++k)
                for (int l = 0; l < win; ++l) {
                    const int kk = wrap_index(k, win), ll = wrap_index(l, win);
                    B[ll * h1 + kk] = wadd(B[ll * h1 + kk], wmul(wmul(Hc[k * win2 + l], b[i]) / kTapScale, b[j]) / kTapScale);
                }
        }
    normalise_and_solve(win, A, B, a);
}

// update_b_sep_sym (:965-1019): fix a, update b
void update_b_sep_sym(int win, const int64_t* M, const int64_t* H, const int32_t* a, int32_t* b) {
    int64_t A[kHalfWin1], B[kHalfWin1 * kHalfWin1];
    const int win2 = win * win, h1 = (win >> 1) + 1;
    memset(A, 0, sizeof(A));
    memset(B, 0, sizeof(B));
    for (int i = 0; i < win; i++) {
        const int ii = wrap_index(i, win);
        for (int j = 0; j < win; j++) A[ii] = wadd(A[ii], wmul(M[i * win + j], a[j]) / kTapScale);
    }
    for (int i = 0; i < win; i++)
        for (int j = 0; j < win; j++) {
            const int ii = wrap_index(i, win), jj = wrap_index(j, win);
            const int64_t* Hc = H + (size_t)i * win * win2 + (size_t)j * win;      // Hc[i * win + j]
            for (int k = 0; k < win; ++k)
                for (int l = 0; l < win; ++l)
                    B[jj * h1 + ii] = wadd(B[jj * h1 + ii], wmul(wmul(Hc[k * win2 + l], a[k]) / kTapScale, a[l]) / kTapScale);
        }
    normalise_and_solve(win, A, B, b);
}

// finalize_sym_filter (:1094-1126) -> the seven taps
void finalize_sym_filter(int win, const int32_t* f, int16_t fi[8]) {
    const int half = win >> 1;
    for (int i = 0; i < half; ++i) {
        const int64_t dividend = (int32_t)((uint32_t)f[i] * (uint32_t)kFiltStep);      // an int product in the reference
        const int64_t divisor = kTapScale;
        fi[i] = dividend < 0 ? (int16_t)((dividend - (divisor / 2)) / divisor) : (int16_t)((dividend + (divisor / 2)) / divisor);
    }
    if (win == kWin) {
        fi[0] = (int16_t)lr_clamp(fi[0], kLrTapMin[0], kLrTapMax[0]);
        fi[1] = (int16_t)lr_clamp(fi[1], kLrTapMin[1], kLrTapMax[1]);
        fi[2] = (int16_t)lr_clamp(fi[2], kLrTapMin[2], kLrTapMax[2]);
    } else {
        fi[2] = (int16_t)lr_clamp(fi[1], kLrTapMin[2], kLrTapMax[2]);
        fi[1] = (int16_t)lr_clamp(fi[0], kLrTapMin[1], kLrTapMax[1]);
        fi[0] = 0;
    }
    fi[kWin - 1] = fi[0];
    fi[kWin - 2] = fi[1];
    fi[kWin - 3] = fi[2];
    fi[3] = (int16_t)(-2 * (fi[0] + fi[1] + fi[2]));
}

// compute_score (:1053-1092)
int64_t compute_score(int win, const int64_t* M, const int64_t* H, const int16_t* vfilt, const int16_t* hfilt) {
    int32_t ab[kWin * kWin];
    int16_t a[kWin], b[kWin];
    int64_t P = 0, Q = 0;
    const int plane_off = (kWin - win) >> 1, win2 = win * win;
    a[kHalfWin] = b[kHalfWin] = kFiltStep;
    for (int i = 0; i < kHalfWin; ++i) {
        a[i] = a[kWin - i - 1] = vfilt[i];
        b[i] = b[kWin - i - 1] = hfilt[i];
        a[kHalfWin] = (int16_t)(a[kHalfWin] - 2 * a[i]);
        b[kHalfWin] = (int16_t)(b[kHalfWin] - 2 * b[i]);
    }
    memset(ab, 0, sizeof(ab));
    for (int k = 0; k < win; ++k)
        for (int l = 0; l < win; ++l) ab[k * win + l] = a[l + plane_off] * b[k + plane_off];
    for (int k = 0; k < win2; ++k) {
        P = wadd(P, wmul(ab[k], M[k]) / kFiltStep / kFiltStep);
        for (int l = 0; l < win2; ++l) Q = wadd(Q, wmul(wmul(ab[k], H[k * win2 + l]), ab[l]) / kFiltStep / kFiltStep / kFiltStep / kFiltStep);
    }
    const int64_t score = wsub(Q, wmul(2, P));
    const int64_t iP = M[win2 >> 1], iQ = H[(win2 >> 1) * win2 + (win2 >> 1)];
    return wsub(score, wsub(iQ, wmul(2, iP)));
}
}  // namespace

int lr_wiener_solve(int win, const int64_t* M, const int64_t* H, int16_t vfilter[3], int16_t hfilter[3], int* accepted) {
    if ((win != 7 && win != 5 && win != 3) || !M || !H || !vfilter || !hfilter || !accepted)
        return set_err(SVT_HIP_ERR_INVALID, "window %d (7, 5 or 3) or a NULL argument", win);
    // wiener_decompose_sep_sym (:1021-1052)
    int32_t a[kWin], b[kWin];
    const int plane_off = (kWin - win) >> 1;
    for (int i = 0; i < win; i++) a[i] = b[i] = (int32_t)(kTapScale / kFiltStep * kInitFilt[i + plane_off]);
    for (int iter = 1; iter < kIters; iter++) {
        update_a_sep_sym(win, M, H, a, b);
        update_b_sep_sym(win, M, H, a, b);
    }
    // search_wiener_seg (:1811-1825): a is the vertical filter, b the horizontal one
    int16_t vf[8] = {}, hf[8] = {};
    finalize_sym_filter(win, a, vf);
    finalize_sym_filter(win, b, hf);
    for (int i = 0; i < 3; i++) { vfilter[i] = vf[i]; hfilter[i] = hf[i]; }
    *accepted = compute_score(win, M, H, vf, hf) > 0 ? 0 : 1;
    return SVT_HIP_OK;
}

// ---- finer_tile_search_wiener_seg (:1278-1387) as a state machine ----------------------------------------------------------------
namespace {
enum { WALK_FIRST = 0, WALK_TRIAL = 1, WALK_DONE = 2 };
constexpr int kStartStep = 4;

void next_dir(svt_hip_lr_walk* w) {
    w->p = (kWin - w->win) >> 1; w->phase = 0; w->skip = 0;
    if (++w->dir > 1) { w->dir = 0; w->step >>= 1; }
}
void next_tap(svt_hip_lr_walk* w) {
    w->phase = 0; w->skip = 0;
    if (++w->p >= kHalfWin) next_dir(w);
}
// from the walk's position: the next trial the reference would make, or the end
int advance(svt_hip_lr_walk* w) {
    for (;;) {
        if (w->step < 1) { w->state = WALK_DONE; return SVT_HIP_LR_WALK_DONE; }
        int16_t* tap = &(w->dir ? w->vfilter : w->hfilter)[w->p];      // horizontal taps first, then vertical, per step
        if (w->phase == 0) {
            if (*tap - w->step >= kLrTapMin[w->p]) { *tap = (int16_t)(*tap - w->step); w->state = WALK_TRIAL; return SVT_HIP_LR_WALK_TRY; }
            if (w->skip) next_dir(w);        // `if (skip) break;` ends the tap loop after a successful downward move
            else w->phase = 1;
        } else {
            if (*tap + w->step <= kLrTapMax[w->p]) { *tap = (int16_t)(*tap + w->step); w->state = WALK_TRIAL; return SVT_HIP_LR_WALK_TRY; }
            next_tap(w);
        }
    }
}
}  // namespace

int lr_walk_start(svt_hip_lr_walk* w, int win, const int16_t vfilter[3], const int16_t hfilter[3]) {
    if (!w || !vfilter || !hfilter || (win != 7 && win != 5 && win != 3)) return set_err(SVT_HIP_ERR_INVALID, "window %d (7, 5 or 3) or a NULL argument", win);
    memset(w, 0, sizeof(*w));
    for (int i = 0; i < 3; i++) {
        if (vfilter[i] < kLrTapMin[i] || vfilter[i] > kLrTapMax[i] || hfilter[i] < kLrTapMin[i] || hfilter[i] > kLrTapMax[i])
            return set_err(SVT_HIP_ERR_INVALID, "tap %d: %d / %d (%d .. %d)", i, vfilter[i], hfilter[i], kLrTapMin[i], kLrTapMax[i]);
        w->vfilter[i] = vfilter[i]; w->hfilter[i] = hfilter[i];
    }
    w->win = win; w->step = kStartStep; w->dir = 0; w->p = (kWin - win) >> 1; w->state = WALK_FIRST;
    return SVT_HIP_LR_WALK_TRY;          // err = try_restoration_unit_seg(rui) with the solve's taps
}

int lr_walk_next(svt_hip_lr_walk* w, int64_t sse) {
    if (!w || w->state == WALK_DONE || (w->win != 7 && w->win != 5 && w->win != 3) || w->p < 0 || w->p >= kHalfWin || w->step < 1 || w->step > kStartStep)
        return set_err(SVT_HIP_ERR_INVALID, "NULL, finished or damaged walk");
    if (w->state == WALK_FIRST) {
        w->err = sse;
        return advance(w);
    }
    int16_t* tap = &(w->dir ? w->vfilter : w->hfilter)[w->p];
    if (sse > w->err) {                  // err2 > err rejects: a tie is accepted
        *tap = (int16_t)(w->phase == 0 ? *tap + w->step : *tap - w->step);
        if (w->phase == 0) { if (w->skip) next_dir(w); else w->phase = 1; }
        else next_tap(w);
    } else {
        w->err = sse;
        if (w->phase == 0) {
            w->skip = 1;
            if (w->step != kStartStep) next_dir(w);      // at the highest step keep moving in the same direction
        } else if (w->step != kStartStep) next_tap(w);
    }
    return advance(w);
}

}  // namespace svthost

// ---- rest_finish_search (:1989-2058) for one plane -------------------------------------------------------------------------------
namespace svthost {
namespace {
constexpr int kProbCostShift = 9;                               // AV1_PROB_COST_SHIFT
constexpr int RESTORE_NONE = 0, RESTORE_WIENER = 1, RESTORE_SGRPROJ = 2, RESTORE_SWITCHABLE = 3, RESTORE_TYPES = 4;
constexpr int8_t kSgrR0[16] = {2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 0, 0, 0, 0, 2, 2}, kSgrR1[16] = {1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0};

// aom_count_primitive_refsubexpfin with recenter_finite_nonneg, aom_count_primitive_subexpfin and aom_count_primitive_quniform
// (EbEntropyCoding.c:3293-3460)
uint16_t recenter_nonneg(uint16_t r, uint16_t v) {
    if (v > (r << 1)) return v;
    if (v >= r) return (uint16_t)((v - r) << 1);
    return (uint16_t)(((r - v) << 1) - 1);
}
uint16_t recenter_finite_nonneg(uint16_t n, uint16_t r, uint16_t v) {
    return (r << 1) <= n ? recenter_nonneg(r, v) : recenter_nonneg((uint16_t)(n - 1 - r), (uint16_t)(n - 1 - v));
}
int count_quniform(uint16_t n, uint16_t v) {
    if (n <= 1) return 0;
    int l = 0;
    while (((n - 1) >> l) != 0) l++;                           // get_msb(n - 1) + 1
    const int m = (1 << l) - n;
    return v < m ? l - 1 : l;
}
int count_subexpfin(uint16_t n, uint16_t k, uint16_t v) {
    int count = 0, i = 0, mk = 0;
    for (;;) {
        const int b = i ? k + i - 1 : k, a = 1 << b;
        if (n <= mk + 3 * a) return count + count_quniform((uint16_t)(n - mk), (uint16_t)(v - mk));
        count++;
        if (v >= mk + a) { i++; mk += a; }
        else return count + b;
    }
}
int count_refsubexpfin(int n, int k, int ref, int v) { return count_subexpfin((uint16_t)n, (uint16_t)k, recenter_finite_nonneg((uint16_t)n, (uint16_t)ref, (uint16_t)v)); }

struct Wiener { int16_t v[3], h[3]; };
struct Sgr { int ep, xqd[2]; };
constexpr int kSubexpK[3] = {1, 2, 3};                          // WIENER_FILT_TAP{0,1,2}_SUBEXP_K

// count_wiener_bits (:1129-1165): tap 0 only at the full window
int count_wiener_bits(int win, const Wiener& w, const Wiener& ref) {
    int bits = 0;
    for (int t = win == kWin ? 0 : 1; t < 3; t++) bits += count_refsubexpfin(kLrTapMax[t] - kLrTapMin[t] + 1, kSubexpK[t], ref.v[t] - kLrTapMin[t], w.v[t] - kLrTapMin[t]);
    for (int t = win == kWin ? 0 : 1; t < 3; t++) bits += count_refsubexpfin(kLrTapMax[t] - kLrTapMin[t] + 1, kSubexpK[t], ref.h[t] - kLrTapMin[t], w.h[t] - kLrTapMin[t]);
    return bits;
}
// count_sgrproj_bits (:664-679)
int count_sgrproj_bits(const Sgr& s, const Sgr& ref) {
    int bits = 4;                                               // SGRPROJ_PARAMS_BITS
    if (kSgrR0[s.ep] > 0) bits += count_refsubexpfin(kLrXqdMax[0] - kLrXqdMin[0] + 1, 4, ref.xqd[0] - kLrXqdMin[0], s.xqd[0] - kLrXqdMin[0]);
    if (kSgrR1[s.ep] > 0) bits += count_refsubexpfin(kLrXqdMax[1] - kLrXqdMin[1] + 1, 4, ref.xqd[1] - kLrXqdMin[1], s.xqd[1] - kLrXqdMin[1]);
    return bits;
}
// RDCOST_DBL (EbRestoration.h:394): binary64, no product feeds a sum that could be contracted to another value (both products are exact
// scalings by powers of two or are divided first)
double rdcost_dbl(int rdmult, int64_t rate, int64_t dist) {
    const double r = ((double)rate * rdmult) / (double)(1 << kProbCostShift);
    const double d = (double)dist * (1 << 7);                   // RDDIV_BITS
    return r + d;
}

struct Rusi { Wiener wiener; Sgr sgrproj; int64_t sse[3]; int best_rtype[3]; };
struct Rsc { int64_t sse, bits; Sgr sgrproj; Wiener wiener; };
}  // namespace

int lr_finish(int plane, int wn_filter_mode, const svt_hip_lr_costs* x, const svt_hip_lr_result* res, uint32_t nunits, int32_t* frame_type, svt_hip_lr_unit* out) {
    if (plane < 0 || plane > 2 || wn_filter_mode < 0 || wn_filter_mode > 3 || !x || !res || nunits == 0 || nunits > (1u << 20) || !frame_type || !out)
        return set_err(SVT_HIP_ERR_INVALID, "plane %d (0 .. 2), wn_filter_mode %d (0 .. 3), %u units or a NULL argument", plane, wn_filter_mode, nunits);
    for (uint32_t u = 0; u < nunits; u++) {
        const svt_hip_lr_result& r = res[u];
        if (r.ep < 0 || r.ep > 15 || r.sse[0] < 0 || r.sse[1] < 0 || r.sse[2] < 0) return set_err(SVT_HIP_ERR_INVALID, "unit %u: ep %d (0 .. 15) or a negative SSE", u, r.ep);
        for (int t = 0; t < 3; t++)
            if (r.vfilter[t] < kLrTapMin[t] || r.vfilter[t] > kLrTapMax[t] || r.hfilter[t] < kLrTapMin[t] || r.hfilter[t] > kLrTapMax[t])
                return set_err(SVT_HIP_ERR_INVALID, "unit %u: Wiener tap %d out of range", u, t);
        for (int t = 0; t < 2; t++)
            if (r.xqd[t] < kLrXqdMin[t] || r.xqd[t] > kLrXqdMax[t]) return set_err(SVT_HIP_ERR_INVALID, "unit %u: xqd[%d] out of range", u, t);
    }
    Rusi* rusi = (Rusi*)calloc(nunits, sizeof(Rusi));
    if (!rusi) return set_err(SVT_HIP_ERR_INVALID, "out of host memory");
    const int force = wn_filter_mode ? RESTORE_TYPES : RESTORE_SGRPROJ;      // force_restore_type_d
    const int num_rtypes = nunits > 1 ? RESTORE_TYPES : RESTORE_SWITCHABLE;   // a plane of one unit never goes switchable
    // search_wiener_finish's window (:1850-1852); search_switchable's is WIENER_WIN for luma whatever the mode (:1518-1519)
    const int wn_luma = wn_filter_mode == 1 ? 3 : (wn_filter_mode == 2 ? 5 : 7);
    const int win_wiener = wn_filter_mode == 1 ? 3 : (plane == 0 ? wn_luma : 5), win_switch = plane == 0 ? 7 : 5;
    double best_cost = 0;
    int best_rtype = RESTORE_NONE;
    for (int r = 0; r < num_rtypes; ++r) {
        if (force != RESTORE_TYPES && r != RESTORE_NONE && r != force) continue;
        // search_rest_type_finish (:1927-1939): reset_rsc, rsc_on_tile, then the visitor of type r over the units
        Rsc rsc{};
        rsc.sgrproj.xqd[0] = (kLrXqdMin[0] + kLrXqdMax[0]) / 2; rsc.sgrproj.xqd[1] = (kLrXqdMin[1] + kLrXqdMax[1]) / 2;      // set_default_sgrproj
        rsc.wiener = Wiener{{3, -7, 15}, {3, -7, 15}};                                                                        // set_default_wiener
        for (uint32_t u = 0; u < nunits; u++) {
            Rusi& ru = rusi[u];
            const svt_hip_lr_result& in = res[u];
            if (r == RESTORE_NONE) {                       // search_norestore_finish
                ru.sse[RESTORE_NONE] = in.sse[RESTORE_NONE];
                rsc.sse += ru.sse[RESTORE_NONE];
            } else if (r == RESTORE_WIENER) {              // search_wiener_finish (:1842-1900)
                const int64_t bits_none = x->wiener_restore_cost[0];
                ru.sse[RESTORE_WIENER] = in.sse[RESTORE_WIENER];
                if (ru.sse[RESTORE_WIENER] == INT64_MAX) {
                    rsc.bits += bits_none;
                    rsc.sse += ru.sse[RESTORE_NONE];
                    ru.best_rtype[RESTORE_WIENER - 1] = RESTORE_NONE;
                    continue;
                }
                for (int t = 0; t < 3; t++) { ru.wiener.v[t] = in.vfilter[t]; ru.wiener.h[t] = in.hfilter[t]; }
                const int64_t bits_wiener = x->wiener_restore_cost[1] + ((int64_t)count_wiener_bits(win_wiener, ru.wiener, rsc.wiener) << kProbCostShift);
                const double cost_none = rdcost_dbl(x->rdmult, bits_none >> 4, ru.sse[RESTORE_NONE]);
                const double cost_wiener = rdcost_dbl(x->rdmult, bits_wiener >> 4, ru.sse[RESTORE_WIENER]);
                const int rtype = cost_wiener < cost_none ? RESTORE_WIENER : RESTORE_NONE;
                ru.best_rtype[RESTORE_WIENER - 1] = rtype;
                rsc.sse += ru.sse[rtype];
                rsc.bits += cost_wiener < cost_none ? bits_wiener : bits_none;
                if (cost_wiener < cost_none) rsc.wiener = ru.wiener;
            } else if (r == RESTORE_SGRPROJ) {             // search_sgrproj_finish (:1724-1756)
                ru.sse[RESTORE_SGRPROJ] = in.sse[RESTORE_SGRPROJ];
                ru.sgrproj = Sgr{in.ep, {in.xqd[0], in.xqd[1]}};
                const int64_t bits_none = x->sgrproj_restore_cost[0];
                const int64_t bits_sgr = x->sgrproj_restore_cost[1] + ((int64_t)count_sgrproj_bits(ru.sgrproj, rsc.sgrproj) << kProbCostShift);
                const double cost_none = rdcost_dbl(x->rdmult, bits_none >> 4, ru.sse[RESTORE_NONE]);
                const double cost_sgr = rdcost_dbl(x->rdmult, bits_sgr >> 4, ru.sse[RESTORE_SGRPROJ]);
                const int rtype = cost_sgr < cost_none ? RESTORE_SGRPROJ : RESTORE_NONE;
                ru.best_rtype[RESTORE_SGRPROJ - 1] = rtype;
                rsc.sse += ru.sse[rtype];
                rsc.bits += cost_sgr < cost_none ? bits_sgr : bits_none;
                if (cost_sgr < cost_none) rsc.sgrproj = ru.sgrproj;
            } else {                                       // search_switchable (:1508-1569)
                double best_c = 0;
                int64_t best_bits = 0;
                int best_r = RESTORE_NONE;
                for (int rr = 0; rr < RESTORE_SWITCHABLE; ++rr) {
                    if (rr > RESTORE_NONE && ru.best_rtype[rr - 1] == RESTORE_NONE) continue;
                    const int64_t coeff_pcost = rr == RESTORE_WIENER ? count_wiener_bits(win_switch, ru.wiener, rsc.wiener)
                                                                     : (rr == RESTORE_SGRPROJ ? count_sgrproj_bits(ru.sgrproj, rsc.sgrproj) : 0);
                    const int64_t bits = x->switchable_restore_cost[rr] + (coeff_pcost << kProbCostShift);
                    const double cost = rdcost_dbl(x->rdmult, bits >> 4, ru.sse[rr]);
                    if (rr == 0 || cost < best_c) { best_c = cost; best_bits = bits; best_r = rr; }
                }
                ru.best_rtype[RESTORE_SWITCHABLE - 1] = best_r;
                rsc.sse += ru.sse[best_r];
                rsc.bits += best_bits;
                if (best_r == RESTORE_WIENER) rsc.wiener = ru.wiener;
                if (best_r == RESTORE_SGRPROJ) rsc.sgrproj = ru.sgrproj;
            }
        }
        const double cost = rdcost_dbl(x->rdmult, rsc.bits >> 4, rsc.sse);
        if (r == 0 || cost < best_cost) { best_cost = cost; best_rtype = r; }
    }
    *frame_type = best_rtype;
    memset(out, 0, (size_t)nunits * sizeof(*out));
    if (best_rtype != RESTORE_NONE)
        for (uint32_t u = 0; u < nunits; u++) {            // copy_unit_info (:1571-1580)
            out[u].type = rusi[u].best_rtype[best_rtype - 1];
            if (out[u].type == RESTORE_WIENER) {
                for (int t = 0; t < 3; t++) { out[u].vfilter[t] = rusi[u].wiener.v[t]; out[u].hfilter[t] = rusi[u].wiener.h[t]; }
            } else {
                out[u].ep = rusi[u].sgrproj.ep; out[u].xqd[0] = (int16_t)rusi[u].sgrproj.xqd[0]; out[u].xqd[1] = (int16_t)rusi[u].sgrproj.xqd[1];
            }
        }
    free(rusi);
    return SVT_HIP_OK;
}
}  // namespace svthost

extern "C" int svt_hip_lr_finish(int plane, int wn_filter_mode, const svt_hip_lr_costs* costs, const svt_hip_lr_result* results, uint32_t nunits,
                                 int32_t* frame_restoration_type, svt_hip_lr_unit* units) {
    return svthost::lr_finish(plane, wn_filter_mode, costs, results, nunits, frame_restoration_type, units);
}
extern "C" int svt_hip_lr_wiener_solve(int win, const int64_t* M, const int64_t* H, int16_t vfilter[3], int16_t hfilter[3], int* accepted) {
    return svthost::lr_wiener_solve(win, M, H, vfilter, hfilter, accepted);
}
extern "C" int svt_hip_lr_walk_start(svt_hip_lr_walk* w, int win, const int16_t vfilter[3], const int16_t hfilter[3]) {
    return svthost::lr_walk_start(w, win, vfilter, hfilter);
}
extern "C" int svt_hip_lr_walk_next(svt_hip_lr_walk* w, int64_t sse) { return svthost::lr_walk_next(w, sse); }

// ---- the self-guided parameter search's host side: lr_sgr_solve.h's text behind the C ABI -------------------------------------------
extern "C" int svt_hip_lr_sgr_solve(const int64_t stats[5], uint32_t npix, int ep, int16_t xqd[2]) {
    using namespace svthost;
    if (!stats || !xqd || ep < 0 || ep >= LR_SGR_PARAMS || npix == 0 || npix > 0x7fffffffu)
        return set_err(SVT_HIP_ERR_INVALID, "ep %d (0 .. 15), %u samples or a NULL argument", ep, npix);
    int v[2];
    lr_sgr_solve(stats, npix, ep, v);
    xqd[0] = (int16_t)v[0]; xqd[1] = (int16_t)v[1];
    return SVT_HIP_OK;
}

extern "C" int svt_hip_lr_sgr_walk_host(const int16_t* f1, const int16_t* f2, const int16_t* sd, uint32_t n, int ep, int16_t xqd[2], int64_t* err,
                                        int64_t* trials, int max_trials) {
    using namespace svthost;
    if (!f1 || !f2 || !sd || !xqd || !err || n == 0 || ep < 0 || ep >= LR_SGR_PARAMS || (trials && max_trials < 0))
        return set_err(SVT_HIP_ERR_INVALID, "ep %d (0 .. 15), %u samples or a NULL argument", ep, n);
    int v[2] = {xqd[0], xqd[1]};
    for (int p = 0; p < 2; p++)
        if (v[p] < lr_sgr_xqd_min(p) || v[p] > lr_sgr_xqd_max(p)) return set_err(SVT_HIP_ERR_INVALID, "xqd[%d] = %d (%d .. %d)", p, v[p], lr_sgr_xqd_min(p), lr_sgr_xqd_max(p));
    int made = 0, evals = 0;
    const auto eval = [&](int xq0, int xq1) -> int64_t {
        int64_t e = 0;
        for (uint32_t i = 0; i < n; i++) e += lr_sgr_sample_err(xq0, xq1, f1[i], f2[i], sd[i]);
        if (trials && made < max_trials) { trials[3 * made] = xq0; trials[3 * made + 1] = xq1; trials[3 * made + 2] = e; }
        made++;
        return e;
    };
    *err = lr_sgr_walk(ep, v, eval, LR_SGR_MAX_EVALS, &evals);
    xqd[0] = (int16_t)v[0]; xqd[1] = (int16_t)v[1];
    return evals;
}

extern "C" int svt_hip_lr_sgr_ep_range(const int8_t sg_ref_frame_ep[2], int sg_filter_mode, int32_t out[2]) {
    using namespace svthost;
    if (!sg_ref_frame_ep || !out || sg_ref_frame_ep[0] >= LR_SGR_PARAMS || sg_ref_frame_ep[1] >= LR_SGR_PARAMS)
        return set_err(SVT_HIP_ERR_INVALID, "a NULL argument or a reference ep above 15");
    lr_sgr_ep_range(sg_ref_frame_ep[0], sg_ref_frame_ep[1], sg_filter_mode, out);
    return SVT_HIP_OK;
}
