// lr_search.h — the host side of the search of loop restoration: the Wiener filter derivation from the statistics
// (wiener_decompose_sep_sym with update_a_sep_sym / update_b_sep_sym / linsolve_wiener, finalize_sym_filter and compute_score,
// EbRestorationPick.c:860-1126), finer_tile_search_wiener_seg (:1278-1387) as a resumable walk that asks for one trial at a time, and
// the picture-level finish rest_finish_search (:1989-2058) for one plane.
// Host only (no HIP header, no device call): tests/c/lr_plan_host.cpp drives it under the sanitizers.  The derivation and the walk are
// integer arithmetic, as in the reference; where the reference's own expression can overflow a signed type the same two's-complement
// result is produced through unsigned arithmetic.  The finish's only binary64 is RDCOST_DBL.
#pragma once
#include <stdint.h>

#include "../../include/svt_hip_dsp.h"

namespace svthost {

// wiener_decompose_sep_sym -> finalize_sym_filter -> compute_score for one unit.  M [win2], H [win2 * win2] as
// svt_hip_lr_wiener_stats_frame packs them.  vfilter / hfilter: taps 0 .. 2.  accepted: 0 when compute_score is above 0 (the unit's
// Wiener SSE is INT64_MAX and nothing is tried), else 1.
int lr_wiener_solve(int win, const int64_t* M, const int64_t* H, int16_t vfilter[3], int16_t hfilter[3], int* accepted);

// The walk.  lr_walk_start takes the solve's taps and asks for the first trial (those taps); every lr_walk_next takes the SSE of the
// trial asked for last and either asks for the next (SVT_HIP_LR_WALK_TRY, taps in w->vfilter / w->hfilter) or ends
// (SVT_HIP_LR_WALK_DONE, the final taps in the same place and their SSE in w->err).
int lr_walk_start(svt_hip_lr_walk* w, int win, const int16_t vfilter[3], const int16_t hfilter[3]);
int lr_walk_next(svt_hip_lr_walk* w, int64_t sse);

// rest_finish_search (:1989-2058) for one plane: see svt_hip_lr_finish in include/svt_hip_dsp.h
int lr_finish(int plane, int wn_filter_mode, const svt_hip_lr_costs* costs, const svt_hip_lr_result* results, uint32_t nunits, int32_t* frame_restoration_type,
              svt_hip_lr_unit* units);

}  // namespace svthost
