"""Every ctypes record and numpy dtype that mirrors a struct of include/svt_hip_dsp.h, stated once, and the one filler that turns a
dict of tensors and numbers into such a record.

RECORDS maps the C struct's name to its ctypes twin; tests/test_mirror_cpu.py compiles one program against the header and compares
sizeof and every offsetof.  RULES holds, per record, what fill() cannot read off the record's own _fields_."""
import collections
import ctypes
from ctypes import c_int8 as i8, c_int16 as i16, c_int32 as i32, c_int64 as i64, c_size_t, c_uint8 as u8, c_uint16 as u16, c_uint32 as u32, \
    c_uint64 as u64, c_void_p

Structure = ctypes.Structure
RECORDS = {}                                        # C struct name -> ctypes record
C_FIELD = {"lambda_": "lambda"}                     # ctypes field -> C field, where the C name is a Python keyword


def record(c_name):
    """class decorator: enter the record into RECORDS under its C struct's name"""
    def enter(cls):
        cls.c_name = c_name
        RECORDS[c_name] = cls
        return cls
    return enter


def _all(t, *names):
    return [(n, t) for n in names]


# -- motion estimation, picture statistics -------------------------------------------------------------------------------------------
@record("svt_hip_me_frame_params")
class MeFrameParams(Structure):
    """svt_hip_me_frame_params: what MotionEstimateLcu reads of its picture, sequence and ME context (include/svt_hip_dsp.h)"""
    _fields_ = _all(i32, "picture_width", "picture_height", "slice_type", "temporal_layer_index", "hierarchical_levels", "enable_hme_flag",
                    "enable_hme_level0_flag", "enable_hme_level1_flag", "enable_hme_level2_flag", "number_hme_search_region_in_width",
                    "number_hme_search_region_in_height", "hme_level0_total_search_area_width", "hme_level0_total_search_area_height") + \
               [("hme_search_area_in_width_array", (u16 * 2) * 3), ("hme_search_area_in_height_array", (u16 * 2) * 3)] + \
               _all(i32, "search_area_width", "search_area_height") + [("ref_pic_poc", i32 * 2)] + \
               _all(i32, "is_used_as_reference_flag", "max_number_of_pus_per_sb", "nsq_search_level", "cu8x8_mode", "fractional_search_method", "flavour")

    @classmethod
    def from_lcu_prm(cls, prm):
        """from the int32 parameter block of oracle/ref_me.c's ref_motion_estimate_lcu (its slots 2 / 3, the SB origin, and 27 .. 41,
        the picture geometry, are not parameters of a picture call)"""
        p = cls()
        (p.picture_width, p.picture_height, p.slice_type, p.temporal_layer_index, p.hierarchical_levels) = (int(prm[i]) for i in (0, 1, 4, 6, 7))
        (p.enable_hme_flag, p.enable_hme_level0_flag, p.enable_hme_level1_flag, p.enable_hme_level2_flag) = (int(prm[i]) for i in (8, 9, 10, 11))
        p.is_used_as_reference_flag, p.search_area_width, p.search_area_height = int(prm[12]), int(prm[13]), int(prm[14])
        p.number_hme_search_region_in_width, p.number_hme_search_region_in_height = int(prm[15]), int(prm[16])
        p.hme_level0_total_search_area_width, p.hme_level0_total_search_area_height = int(prm[17]), int(prm[18])
        p.ref_pic_poc[0], p.ref_pic_poc[1], p.flavour = int(prm[19]), int(prm[20]), int(prm[21])
        p.cu8x8_mode, p.fractional_search_method, p.max_number_of_pus_per_sb, p.nsq_search_level = (int(prm[i]) for i in (23, 24, 25, 26))
        for lv in range(3):
            for i in range(2):
                p.hme_search_area_in_width_array[lv][i] = int(prm[42 + 4 * lv + i])
                p.hme_search_area_in_height_array[lv][i] = int(prm[44 + 4 * lv + i])
        return p


@record("svt_hip_me_subpel_params")
class MeSubpelParams(Structure):
    """svt_hip_me_subpel_params: the enables of the half- / quarter-pel refinement (the reference sets all of them to 1)"""
    _fields_ = _all(i32, "fractional_search64x64", "enable_half_pel32x32", "enable_half_pel16x16", "enable_half_pel8x8", "enable_quarter_pel")


@record("svt_hip_me_pyramid")
class MePyramid(Structure):
    """svt_hip_me_pyramid: the padded full / quarter / sixteenth luma buffers of one picture (or of a stack of pictures)"""
    _fields_ = [("d_plane", c_void_p * 3), ("stride", u32 * 3), ("origin_x", u32 * 3), ("origin_y", u32 * 3), ("pitch", u64 * 3)]


@record("svt_hip_hme_params")
class HmeParams(Structure):
    _fields_ = _all(i32, "search_area_width", "search_area_height", "x_origin_offset", "y_origin_offset", "pad_width", "pad_height", "ref_width",
                    "ref_height", "round_down", "mv_shift")


@record("svt_hip_me_setup_params")
class MeSetupParams(Structure):
    _fields_ = _all(i32, "picture_width", "picture_height", "ref_width", "ref_height", "search_area_width", "search_area_height", "regions_w",
                    "regions_h", "second_best", "zz_check")


@record("svt_hip_me_result")
class MeResult(Structure):
    _fields_ = _all(i16, "x_mv_l0", "y_mv_l0", "x_mv_l1", "y_mv_l1") + [("distortion", u32 * 3), ("direction", u8 * 3), ("total_me_candidate_index", u8)]


@record("svt_hip_pic_stats_planes")
class PicStatsPlanes(Structure):
    """svt_hip_pic_stats_planes: the padded luma, Cb, Cr and 1/16 luma buffers of one picture (or of a stack of pictures)"""
    _fields_ = [("d_plane", c_void_p * 4), ("stride", u32 * 4), ("origin_x", u32 * 4), ("origin_y", u32 * 4), ("pitch", u64 * 4)]


@record("svt_hip_pic_stats_params")
class PicStatsParams(Structure):
    """svt_hip_pic_stats_params"""
    _fields_ = _all(i32, "picture_width", "picture_height", "block_mean_calc_prec", "regions_per_width", "regions_per_height")


@record("svt_hip_pic_stats_out")
class PicStatsOut(Structure):
    """svt_hip_pic_stats_out: the eight device outputs of svt_hip_picture_stats_frame"""
    _fields_ = _all(c_void_p, "d_y_mean", "d_variance", "d_cb_mean", "d_cr_mean", "d_pic_avg_variance", "d_histogram", "d_avg_intensity_region",
                    "d_avg_intensity")


PicStatsResult = collections.namedtuple("PicStatsResult", ("y_mean", "variance", "cb_mean", "cr_mean", "pic_avg_variance", "histogram",
                                                           "avg_intensity_region", "avg_intensity"))


@record("svt_hip_y4m_info")
class Y4mInfo(Structure):
    """svt_hip_y4m_info: what read_y4m_header (Source/App/EncApp/EbAppInputy4m.c:35) takes from the header line"""
    _fields_ = _all(u32, "width", "height", "fr_n", "fr_d", "bit_depth", "interlaced") + [("chroma", ctypes.c_char * 8), ("scan_type", ctypes.c_char)]


# -- intra prediction, open-loop intra search, the frame-level encode pass ---------------------------------------------------------------
@record("svt_hip_ois_group")
class OisGroup(Structure):
    """svt_hip_ois_group"""
    _fields_ = [("d_xy", c_void_p), ("bsize", u32), ("modes", c_void_p), ("angle_deltas", c_void_p), ("ncand", i32), ("d_distortion", c_void_p),
                ("d_best_index", c_void_p), ("d_work", c_void_p), ("work_bytes", c_size_t), ("nblocks", c_size_t)]


@record("svt_hip_intra_pos")
class IntraPos(Structure):
    """svt_hip_intra_pos: where one prediction block sits (the arguments of av1_predict_intra_block, EbIntraPrediction.c:4078)"""
    _fields_ = _all(i32, "is_16bit", "sb_size_mi", "mi_rows", "mi_cols", "tile_mi_row_start", "tile_mi_row_end", "tile_mi_col_start",
                    "tile_mi_col_end", "partition", "bsize", "tx_size", "plane", "bl_org_x_pict", "bl_org_y_pict", "col_off", "row_off", "wpx", "hpx")


@record("svt_hip_intra_blk")
class IntraBlk(Structure):
    """svt_hip_intra_blk: per-block descriptor of svt_hip_build_intra_predictors_batch"""
    _fields_ = [("mode", u8), ("angle_delta", i8)] + _all(u8, "filt_type", "disable_edge_filter", "n_top_px", "n_topright_px", "n_left_px",
                                                          "n_bottomleft_px")


@record("svt_hip_frame_group")
class FrameGroup(Structure):
    _fields_ = [("d_src", c_void_p), ("src_stride", u32), ("d_pred", c_void_p), ("pred_stride", u32), ("d_recon", c_void_p), ("recon_stride", u32),
                ("d_xy", c_void_p), ("d_offsets", c_void_p), ("nblocks", u32), ("tx_size", i32), ("tx_type", i32)] + \
               _all(c_void_p, "d_iscan", "d_qcoeff", "d_eob", "d_coeff", "d_dqcoeff")


@record("svt_hip_frame_cfl_group")
class FrameCflGroup(Structure):
    _fields_ = [("d_luma_recon", c_void_p), ("luma_stride", u32), ("d_pred_cb", c_void_p), ("pred_stride_cb", u32), ("d_pred_cr", c_void_p),
                ("pred_stride_cr", u32), ("d_xy", c_void_p), ("d_alpha_q3_cb", c_void_p), ("d_alpha_q3_cr", c_void_p), ("width", u32), ("height", u32),
                ("nblocks", u32)]


@record("svt_hip_frame_levels")
class FrameLevels(Structure):
    _fields_ = [("d_levels_buf", c_void_p), ("levels_block_pitch", c_size_t)]


# -- mode decision: full loop, coefficient rate, transform-type decision, CfL ----------------------------------------------------------------
@record("svt_hip_full_loop_group")
class FullLoopGroup(Structure):
    _fields_ = [("d_src", c_void_p), ("src_stride", u32), ("d_src_xy", c_void_p), ("d_pred", c_void_p), ("pred_stride", u32), ("d_pred_xy", c_void_p),
                ("nblocks", u32), ("tx_size", i32), ("ntypes", i32), ("tx_types", u8 * 16)] + _all(c_void_p, "d_iscan", "d_dist", "d_eob", "d_qcoeff", "d_dqcoeff")


@record("svt_hip_coeff_rate_group")
class CoeffRateGroup(Structure):
    _fields_ = [("tx_size", i32), ("ntypes", i32), ("tx_types", u8 * 16), ("nblocks", u32)] + \
               _all(c_void_p, "d_qcoeff", "d_eob", "d_iscan", "d_txb_skip_ctx", "d_dc_sign_ctx", "d_type_bits", "d_coeff_cost", "d_eob_cost", "d_bits")


@record("svt_hip_tx_decision")
class TxDecision(Structure):
    _fields_ = [("cost", u64), ("dist", u64 * 2), ("bits", u64), ("eob", u16), ("tx_type", u8), ("type_index", u8), ("has_coeff", u8), ("pad", u8 * 3)]


@record("svt_hip_tx_decide_group")
class TxDecideGroup(Structure):
    _fields_ = [("tx_size", i32), ("ntypes", i32), ("tx_types", u8 * 16), ("nblocks", u32), ("lambda_", u32)] + \
               _all(c_void_p, "d_dist", "d_eob", "d_bits", "d_qcoeff", "d_dqcoeff", "d_decision", "d_best_qcoeff", "d_best_dqcoeff")


@record("svt_hip_tx_search_group")
class TxSearchGroup(Structure):
    _fields_ = [("fl", FullLoopGroup)] + _all(c_void_p, "d_txb_skip_ctx", "d_dc_sign_ctx", "d_type_bits", "d_coeff_cost", "d_eob_cost") + \
               [("lambda_", u32)] + _all(c_void_p, "d_decision", "d_best_qcoeff", "d_best_dqcoeff")


TX_DECISION_DTYPE = [("cost", "<u8"), ("dist", "<u8", (2,)), ("bits", "<u8"), ("eob", "<u2"), ("tx_type", "u1"), ("type_index", "u1"),
                     ("has_coeff", "u1"), ("pad", "u1", (3,))]        # numpy view of a downloaded uint8 [n, 40] decision tensor


@record("svt_hip_qrows")
class QRows(Structure):
    _fields_ = _all(c_void_p, "zbin", "round", "quant", "quant_shift", "dequant")


@record("svt_hip_cfl_search_group")
class CflSearchGroup(Structure):
    _fields_ = [("d_luma_recon", c_void_p), ("luma_stride", u32), ("d_src", c_void_p * 2), ("src_stride", u32 * 2), ("d_pred", c_void_p * 2),
                ("pred_stride", u32 * 2), ("d_xy", c_void_p), ("nblocks", u32), ("tx_size", i32), ("tx_type", i32), ("d_iscan", c_void_p),
                ("d_txb_skip_ctx", c_void_p * 2), ("d_dc_sign_ctx", c_void_p * 2)] + _all(c_void_p, "d_coeff_cost", "d_eob_cost", "d_dist", "d_bits", "d_eob")


@record("svt_hip_cfl_decision")
class CflDecision(Structure):
    _fields_ = [("best_rd", i64), ("dc_rd", i64), ("alpha_q3", i32 * 2), ("uv_mode", u8), ("cfl_alpha_idx", u8), ("cfl_alpha_signs", u8), ("pad", u8 * 5)]


@record("svt_hip_cfl_decide_group")
class CflDecideGroup(Structure):
    _fields_ = [("nblocks", u32), ("lambda_", u32)] + _all(c_void_p, "d_dist", "d_bits", "d_alpha_rate", "d_cfl_mode_bits", "d_dc_mode_bits",
                                                         "d_decision", "d_alpha_q3_cb", "d_alpha_q3_cr")


@record("svt_hip_cfl_pick_group")
class CflPickGroup(Structure):
    _fields_ = [("search", CflSearchGroup), ("lambda_", u32)] + _all(c_void_p, "d_alpha_rate", "d_cfl_mode_bits", "d_dc_mode_bits", "d_decision",
                                                                   "d_alpha_q3_cb", "d_alpha_q3_cr")


CFL_DECISION_DTYPE = [("best_rd", "<i8"), ("dc_rd", "<i8"), ("alpha_q3", "<i4", (2,)), ("uv_mode", "u1"), ("cfl_alpha_idx", "u1"),
                      ("cfl_alpha_signs", "u1"), ("pad", "u1", (5,))]    # numpy view of a downloaded uint8 [n, 32] decision tensor


# -- mode decision: the intra fast loop and its end ------------------------------------------------------------------------------------------
@record("svt_hip_fast_loop_group")
class FastLoopGroup(Structure):
    _fields_ = [("d_src", c_void_p), ("src_stride", u32), ("d_src_xy", c_void_p), ("d_top_neigh", c_void_p), ("d_left_neigh", c_void_p),
                ("neigh_pitch", i32), ("d_blocks", c_void_p), ("nblocks", u32), ("tx_size", i32), ("ncand", i32), ("modes", u8 * 64),
                ("angle_deltas", i8 * 64), ("d_dist", c_void_p), ("d_pred", c_void_p)]


FAST_RATE_TABLES = (("yModeFacBits", (5, 5, 14)), ("mbModeFacBits", (4, 14)), ("intraUVmodeFacBits", (2, 13, 15)),
                    ("angleDeltaFacBits", (8, 8)), ("skipModeFacBits", (3, 3)), ("intraInterFacBits", (4, 2)))       # svt_hip_fast_rates
FAST_RATE_WORDS = 877
FAST_PICK_BLK_DTYPE = [("top_mode", "u1"), ("left_mode", "u1"), ("skip_mode_ctx", "u1"), ("is_inter_ctx", "u1"), ("has_chroma", "u1"),
                       ("pad", "u1", (3,))]                              # svt_hip_fast_pick_blk


@record("svt_hip_fast_pick_group")
class FastPickGroup(Structure):
    _fields_ = [("tx_size", i32), ("bsize", i32), ("bsize_uv", i32), ("nblocks", u32), ("ncand", i32), ("modes", u8 * 64), ("angle_deltas", i8 * 64),
                ("uv_modes", u8 * 64), ("uv_angle_deltas", i8 * 64), ("use_angle_delta", i32), ("nfl", i32), ("slice_is_intra", i32), ("lambda_", u32),
                ("ac_dequant_q3", i16), ("intrabc_bits", u32)] + \
               _all(c_void_p, "d_dist", "d_dist_cb", "d_dist_cr", "d_blk", "d_rates", "d_pred", "d_src_xy", "d_cand", "d_sorted", "d_cost", "d_rate",
                    "d_ref_fast_cost", "d_all_cost", "d_pred_out", "d_src_xy_out")


@record("svt_hip_intra_fast_search_group")
class IntraFastSearchGroup(Structure):
    _fields_ = [("luma", FastLoopGroup), ("use_chroma", i32), ("cb", FastLoopGroup), ("cr", FastLoopGroup), ("pick", FastPickGroup)]


# -- inter prediction, warped motion, interpolation filter search ----------------------------------------------------------------------------
@record("svt_hip_inter_blk")
class InterBlk(Structure):
    """svt_hip_inter_blk: one (block, candidate) of svt_hip_inter_pred_frame (16 bytes; inter_blk_dtype() is its numpy twin)"""
    _fields_ = [("x", u16), ("y", u16), ("mv", (i16 * 2) * 2), ("pred_direction", u8), ("filter_x", u8), ("filter_y", u8), ("pad", u8)]


@record("svt_hip_inter_pred_group")
class InterPredGroup(Structure):
    """svt_hip_inter_pred_group"""
    _fields_ = [("d_ref", c_void_p * 2), ("ref_stride", u32), ("ss", i32), ("bwidth", i32), ("bheight", i32), ("nblocks", u32), ("d_blk", c_void_p),
                ("d_pred", c_void_p), ("pred_stride", u32), ("d_src", c_void_p), ("src_stride", u32), ("d_dist", c_void_p)]


@record("svt_hip_warp_samples")
class WarpSamples(Structure):
    """svt_hip_warp_samples: what av1_find_samples returns for a block (132 bytes; warp_samples_dtype() is its numpy twin)"""
    _fields_ = [("nsamples", i32), ("pts", i32 * 16), ("pts_inref", i32 * 16)]


@record("svt_hip_warp_model")
class WarpModel(Structure):
    """svt_hip_warp_model: the local warp model of one (block, candidate) (36 bytes; warp_model_dtype() is its numpy twin)"""
    _fields_ = [("mat", i32 * 6)] + _all(i16, "alpha", "beta", "gamma", "delta") + [("valid", u8), ("num_proj_ref", u8), ("pad", u8 * 2)]


@record("svt_hip_warp_fit_group")
class WarpFitGroup(Structure):
    """svt_hip_warp_fit_group"""
    _fields_ = [("bsize", i32), ("nblocks", u32), ("ncand", i32)] + _all(c_void_p, "d_samples", "d_blk", "d_model", "d_nvalid")


@record("svt_hip_warp_pred_group")
class WarpPredGroup(Structure):
    """svt_hip_warp_pred_group"""
    _fields_ = [("d_ref", c_void_p), ("ref_stride", u32), ("ss", i32), ("bwidth", i32), ("bheight", i32), ("nblocks", u32), ("ncand", i32),
                ("d_blk", c_void_p), ("d_model", c_void_p), ("d_sel", c_void_p), ("n", i32), ("sel_first", i32), ("d_pred", c_void_p),
                ("pred_stride", u32), ("d_src", c_void_p), ("src_stride", u32), ("d_dist", c_void_p)]


UNI_PRED_LIST_0, UNI_PRED_LIST_1, BI_PRED = 0, 1, 2
INTER_PRED_MAX_GROUPS = 48


@record("svt_hip_interp_sse_group")
class InterpSseGroup(Structure):
    """svt_hip_interp_sse_group"""
    _fields_ = [("d_ref", (c_void_p * 3) * 2), ("ref_stride", u32 * 3), ("d_src", c_void_p * 3), ("src_stride", u32 * 3), ("bwidth", i32),
                ("bheight", i32), ("nblocks", u32), ("d_blk", c_void_p), ("d_sse", c_void_p)]


@record("svt_hip_interp_decision")
class InterpDecision(Structure):
    """svt_hip_interp_decision (32 bytes; interp_decision_dtype() is its numpy twin)"""
    _fields_ = [("interp_filters", u32), ("switchable_rate", i32), ("rd", i64), ("skip_sse_sb", i64), ("skip_txfm_sb", i32), ("pad", u32)]


@record("svt_hip_interp_params")
class InterpParams(Structure):
    """svt_hip_interp_params"""
    _fields_ = [("full_lambda", u32), ("ac_dequant_q3", i32), ("d_rates", c_void_p), ("use_uv", i32), ("mode", i32)]


@record("svt_hip_interp_decide_group")
class InterpDecideGroup(Structure):
    """svt_hip_interp_decide_group"""
    _fields_ = [("bwidth", i32), ("bheight", i32), ("nblocks", u32)] + _all(c_void_p, "d_sse", "d_ctx", "d_searchable", "d_decision", "d_blk", "d_blk_out")


@record("svt_hip_interp_search_group")
class InterpSearchGroup(Structure):
    """svt_hip_interp_search_group"""
    _fields_ = [("sse", InterpSseGroup)] + _all(c_void_p, "d_ctx", "d_searchable", "d_decision", "d_blk_out")


INTERP_DUAL_FAST, INTERP_FULL, INTERP_SINGLE = 0, 1, 2


# -- mode decision: inter candidates in the fast loop, the join, the partition decision ---------------------------------------------------------
@record("svt_hip_inter_cand")
class InterCand(Structure):
    """svt_hip_inter_cand: what only the fast cost reads of an inter candidate (16 bytes; inter_cand_dtype() is its numpy twin)"""
    _fields_ = [("pred_mv", (i16 * 2) * 2), ("mode_ctx", i16)] + _all(u8, "pred_mode", "ref_frame_type", "drl_index", "ref_mv_count", "drl_ctx", "flags")


@record("svt_hip_inter_fast_blk")
class InterFastBlk(Structure):
    """svt_hip_inter_fast_blk: the block's context bytes (16 bytes; inter_fast_blk_dtype() is its numpy twin)"""
    _fields_ = _all(u8, "skip_flag_context", "is_inter_ctx", "reference_mode_context", "compoud_reference_type_context", "comp_ref_p", "comp_ref_p1",
                    "comp_ref_p2", "comp_bwdref_p", "comp_bwdref_p1") + [("single_ref_p", u8 * 6), ("has_uv", u8)]


INTER_FAST_RATE_TABLES = (("skipModeFacBits", (3, 3)), ("newMvModeFacBits", (6, 3)), ("zeroMvModeFacBits", (2, 3)), ("refMvModeFacBits", (6, 3)),
                          ("drlModeFacBits", (3, 3)), ("interCompoundModeFacBits", (8, 9)), ("singleRefFacBits", (3, 6, 3)),
                          ("compRefTypeFacBits", (5, 3)), ("compRefFacBits", (3, 3, 3)), ("compBwdRefFacBits", (3, 2, 3)),
                          ("compInterFacBits", (5, 3)), ("motionModeFacBits", (22, 3)), ("motionModeFacBits1", (22, 2)),
                          ("intraInterFacBits", (4, 2)), ("nmv_vec_cost", (4,)))      # svt_hip_inter_fast_rates
INTER_FAST_RATE_WORDS = 383
MV_VALS = 32767


def _table(shape):
    t = i32
    for n in reversed(shape):
        t = t * n
    return t


@record("svt_hip_inter_fast_rates")
class InterFastRates(Structure):
    """svt_hip_inter_fast_rates"""
    _fields_ = [(name, _table(shape)) for name, shape in INTER_FAST_RATE_TABLES]


@record("svt_hip_inter_fast_pick_group")
class InterFastPickGroup(Structure):
    """svt_hip_inter_fast_pick_group"""
    _fields_ = [("bsize", i32), ("bsize_uv", i32), ("nblocks", u32), ("ninter", i32), ("nintra", i32), ("nfl", i32), ("lambda_", u32),
                ("ac_dequant_q3", i16), ("reference_mode_select", i32), ("switchable_motion_mode", i32)] + \
               _all(c_void_p, "d_blk", "d_cand_in", "d_ctx", "d_rates", "d_mv_cost", "d_dist", "d_dist_cb", "d_dist_cr", "d_intra_cost", "d_intra_rate",
                    "d_cand", "d_sorted", "d_cost", "d_rate", "d_ref_fast_cost", "d_all_cost", "d_blk_out", "d_cand_out", "d_src_xy_out")


@record("svt_hip_inter_fast_search_group")
class InterFastSearchGroup(Structure):
    """svt_hip_inter_fast_search_group"""
    _fields_ = [("pick", InterFastPickGroup), ("bwidth", i32), ("bheight", i32), ("use_chroma", i32), ("d_ref", (c_void_p * 3) * 2),
                ("ref_stride", u32 * 3), ("d_src", c_void_p * 3), ("src_stride", u32 * 3), ("d_pred_out", c_void_p * 3), ("d_intra_pred", c_void_p)]


@record("svt_hip_md_blk")
class MdBlk(Structure):
    """svt_hip_md_blk: the block's bytes the full cost reads (4 bytes; md_blk_dtype() is its numpy twin)"""
    _fields_ = [("skip_flag_context", u8), ("has_uv", u8), ("pad", u8 * 2)]


MD_RATE_TABLES = (("skipModeFacBits", (3, 3)), ("intraUVmodeFacBits", (2, 13, 15)), ("cflAlphaFacBits", (8, 2, 16)))      # svt_hip_md_rates
MD_RATE_WORDS = 655
MD_NO_INTRA = 0xFF


@record("svt_hip_md_rates")
class MdRates(Structure):
    """svt_hip_md_rates"""
    _fields_ = [(name, _table(shape)) for name, shape in MD_RATE_TABLES]


@record("svt_hip_md_decision")
class MdDecision(Structure):
    """svt_hip_md_decision (72 bytes; md_decision_dtype() is its numpy twin)"""
    _fields_ = _all(u64, "cost", "cost_luma", "merge_cost", "skip_cost", "full_lambda_rate") + [("full_distortion", u32), ("eob", u16 * 3)] + \
               _all(u8, "slot", "cand", "count", "is_intra", "skip_flag", "merge_flag", "y_has_coeff", "u_has_coeff", "v_has_coeff", "block_has_coeff",
                    "tx_type", "best_intra_mode", "uv_mode", "cfl_alpha_idx", "cfl_alpha_signs") + [("pad", u8 * 7)]


MD_GATHERS = ("pred", "best_pred", "qcoeff", "dqcoeff", "best_qcoeff", "best_dqcoeff")


@record("svt_hip_md_decide_group")
class MdDecideGroup(Structure):
    """svt_hip_md_decide_group"""
    _fields_ = [("bsize", i32), ("nblocks", u32), ("n", i32), ("ninter", i32), ("nintra", i32), ("lambda_", u32), ("slice_is_intra", i32),
                ("full_loop_escape", i32), ("modes", u8 * 64)] + \
               _all(c_void_p, "d_luma", "d_dist_cb", "d_dist_cr", "d_bits_cb", "d_bits_cr", "d_eob_cb", "d_eob_cr", "d_rate", "d_cand", "d_cand_out",
                    "d_cfl", "d_blk", "d_rates", "d_decision", "d_full_cost") + \
               [("d_" + n, c_void_p * 3) for n in MD_GATHERS] + [("d_inter_blk", c_void_p), ("d_best_inter_blk", c_void_p)]


@record("svt_hip_md_search_group")
class MdSearchGroup(Structure):
    """svt_hip_md_search_group"""
    _fields_ = [("md", MdDecideGroup), ("luma", TxSearchGroup), ("use_chroma", i32), ("cb", FullLoopGroup), ("cr", FullLoopGroup),
                ("d_txb_skip_ctx_c", c_void_p * 2), ("d_dc_sign_ctx_c", c_void_p * 2), ("d_coeff_cost_uv", c_void_p), ("d_eob_cost_uv", c_void_p),
                ("d_bits_c", c_void_p * 2)]


SB_BLOCKS, SB_SQUARES, SB_MAX_FINAL = 1101, 341, 256      # a 64x64 superblock: blocks in md scan, squares, the most blocks it can code
PART_NO_SRC = 0xFFFFFFFF
PARTITION_SPLIT = 3
PARTITION_BITS_SHAPE = (20, 11)                            # partitionFacBits


@record("svt_hip_blk_geom")
class BlkGeom(Structure):
    """svt_hip_blk_geom (16 bytes)"""
    _fields_ = [("sqi_mds", u16)] + _all(u8, "bsize", "shape", "depth", "nsi", "totns", "d1i", "origin_x", "origin_y", "bwidth", "bheight", "sq_size",
                                         "is_last_quadrant", "has_uv", "pad")


@record("svt_hip_partition_args")
class PartitionArgs(Structure):
    """svt_hip_partition_args"""
    _fields_ = _all(u32, "nsb", "nleaves", "nsrc", "lambda_", "pic_width", "pic_height") + [("slice_is_intra", i32), ("pad", i32)] + \
               _all(c_void_p, "d_sb", "d_leaf", "d_decision", "d_cost", "d_partition_bits", "d_sq", "d_final_count", "d_final", "d_final_decision")


# -- the back end: final reconstruction, intra encode pass, CDEF, deblocking, loop restoration ---------------------------------------------------
RECON_FINAL_MAX_GROUPS = 32
RECON_OK, RECON_NO_SRC, RECON_BSIZE, RECON_OUTSIDE, RECON_TX_TYPE = 0, 1, 2, 3, 4      # d_status of svt_hip_recon_final_frame
SB_QCOEFF_LUMA = 4096                                      # int32 per superblock of the luma coefficient stream; chroma a quarter


@record("svt_hip_recon_final_group")
class ReconFinalGroup(Structure):
    """svt_hip_recon_final_group"""
    _fields_ = [("src_first", u32), ("nblocks", u32), ("bsize", i32), ("tx_type_uv", i32), ("d_best_pred", c_void_p * 3),
                ("d_best_dqcoeff", c_void_p * 3), ("d_best_qcoeff", c_void_p * 3)]


@record("svt_hip_recon_final_args")
class ReconFinalArgs(Structure):
    """svt_hip_recon_final_args"""
    _fields_ = [("nsb", u32), ("nsrc", u32), ("ngroups", i32), ("planes", i32)] + _all(c_void_p, "d_final", "d_final_count", "d_decision", "groups") + \
               [("d_recon", c_void_p * 3), ("stride", u32 * 3), ("width", u32 * 3), ("height", u32 * 3), ("d_status", c_void_p),
                ("d_sb_qcoeff", c_void_p * 3), ("d_coeff_offset", c_void_p), ("d_scratch", c_void_p), ("scratch_bytes", c_size_t)]


# d_status of svt_hip_intra_encode_frame
INTRA_ENC_OK, INTRA_ENC_NO_SRC, INTRA_ENC_OUTSIDE, INTRA_ENC_TX_TYPE, INTRA_ENC_NOT_INTRA, INTRA_ENC_MODE, INTRA_ENC_CFL_SIZE, INTRA_ENC_SCHEDULE = 0, 1, 3, 4, 5, 6, 7, 8


@record("svt_hip_intra_encode_args")
class IntraEncodeArgs(Structure):
    """svt_hip_intra_encode_args"""
    _fields_ = _all(u32, "npics", "sb_cols", "sb_rows", "sb_pitch", "nsrc", "blk_pitch") + _all(c_void_p, "d_final", "d_final_count", "d_blk") + \
               [("d_src", c_void_p * 3), ("d_recon", c_void_p * 3)] + _all(u32 * 3, "src_stride", "stride", "width", "height") + \
               [("src_pic_pitch", c_size_t * 3), ("recon_pic_pitch", c_size_t * 3)] + _all(c_void_p, "q_luma", "q_chroma", "d_tables", "d_status", "d_result") + \
               [("d_sb_qcoeff", c_void_p * 3), ("d_coeff_offset", c_void_p), ("d_scratch", c_void_p), ("scratch_bytes", c_size_t)]


@record("svt_hip_cdef_pic")
class CdefPic(Structure):
    """svt_hip_cdef_pic"""
    _fields_ = [("d_rec", c_void_p * 3), ("rec_stride", u32 * 3), ("d_src", c_void_p * 3), ("src_stride", u32 * 3), ("d_dst", c_void_p * 3),
                ("dst_stride", u32 * 3), ("d_skip", c_void_p), ("skip_stride", u32), ("width", u32), ("height", u32), ("bit_depth", i32),
                ("base_qindex", i32), ("npics", u32), ("rec_pitch", u64 * 3), ("src_pitch", u64 * 3), ("dst_pitch", u64 * 3), ("skip_pitch", u64)]


@record("svt_hip_dlf_pic")
class DlfPic(Structure):
    """svt_hip_dlf_pic"""
    _fields_ = [("d_rec", c_void_p * 3), ("rec_stride", u32 * 3), ("d_src", c_void_p * 3), ("src_stride", u32 * 3), ("d_dst", c_void_p * 3),
                ("dst_stride", u32 * 3), ("d_mi", c_void_p), ("mi_stride", u32), ("width", u32), ("height", u32), ("bit_depth", i32), ("npics", u32),
                ("rec_pitch", u64 * 3), ("src_pitch", u64 * 3), ("dst_pitch", u64 * 3), ("mi_pitch", u64), ("filter_level", i32 * 2),
                ("filter_level_u", i32), ("filter_level_v", i32), ("sharpness_level", i32), ("mode_ref_delta_enabled", i32), ("ref_deltas", i8 * 8),
                ("mode_deltas", i8 * 2), ("pad", u8 * 6)]


@record("svt_hip_dlf_mi_args")
class DlfMiArgs(Structure):
    """svt_hip_dlf_mi_args"""
    _fields_ = _all(c_void_p, "d_final", "d_final_count", "d_info", "d_mi") + \
               _all(u32, "npics", "nsb", "sb_pitch", "nsrc", "mi_cols", "mi_rows", "mi_stride", "pad") + [("mi_pitch", u64)]


@record("svt_hip_lr_pic")
class LrPic(Structure):
    """svt_hip_lr_pic"""
    _fields_ = [("d_cdef", c_void_p * 3), ("cdef_stride", u32 * 3), ("pad0", u32), ("d_dblk", c_void_p * 3), ("dblk_stride", u32 * 3), ("pad1", u32),
                ("d_src", c_void_p * 3), ("src_stride", u32 * 3), ("pad2", u32), ("d_dst", c_void_p * 3), ("dst_stride", u32 * 3), ("pad3", u32),
                ("width", u32), ("height", u32), ("bit_depth", i32), ("unit_size", u32 * 3), ("npics", u32), ("pad4", u32), ("cdef_pitch", u64 * 3),
                ("dblk_pitch", u64 * 3), ("src_pitch", u64 * 3), ("dst_pitch", u64 * 3)]


@record("svt_hip_lr_walk")
class LrWalk(Structure):
    """svt_hip_lr_walk"""
    _fields_ = [("vfilter", i16 * 3), ("hfilter", i16 * 3)] + _all(i32, "win", "step", "dir", "p", "phase", "skip", "state") + [("err", i64)]


LR_UNIT_DTYPE = [("type", "<i4"), ("vfilter", "<i2", 3), ("hfilter", "<i2", 3), ("xqd", "<i2", 2), ("ep", "<i4")]              # svt_hip_lr_unit
LR_CAND_DTYPE = [("pic", "<u4"), ("plane", "<u4"), ("unit", "<u4"), ("u", LR_UNIT_DTYPE)]                                       # svt_hip_lr_cand
LR_RESULT_DTYPE = [("sse", "<i8", 3), ("vfilter", "<i2", 3), ("hfilter", "<i2", 3), ("xqd", "<i2", 2), ("ep", "<i4"), ("pad", "<i4")]      # svt_hip_lr_result
LR_COSTS_DTYPE = [("rdmult", "<i4"), ("wiener_restore_cost", "<i4", 2), ("sgrproj_restore_cost", "<i4", 2), ("switchable_restore_cost", "<i4", 3)]
LR_SGR_WALK_DTYPE = [("err", "<i8"), ("xqd", "<i2", 2), ("start", "<i2", 2), ("evals", "<i4"), ("pad", "<i4")]                         # svt_hip_lr_sgr_walk
LR_SGR_BEST_DTYPE = [("sse", "<i8"), ("proj_err", "<i8"), ("ep", "<i4"), ("xqd", "<i2", 2)]        # svt_hip_lr_sgr_best

# the records that are also attributes of SvtHipDsp (the names tests and tools have used since each was added)
DSP_ATTRIBUTES = ("OisGroup", "FrameGroup", "FrameCflGroup", "FrameLevels", "HmeParams", "IntraPos", "IntraBlk", "MeSetupParams", "MeResult", "MeFrameParams",
                  "MePyramid", "MeSubpelParams", "PicStatsPlanes", "PicStatsParams", "PicStatsOut", "PicStatsResult", "FullLoopGroup", "CoeffRateGroup",
                  "TxDecision", "TxDecideGroup", "TxSearchGroup", "TX_DECISION_DTYPE", "QRows", "CflSearchGroup", "CflDecision", "CflDecideGroup",
                  "CflPickGroup", "CFL_DECISION_DTYPE", "FastLoopGroup", "FAST_RATE_TABLES", "FAST_RATE_WORDS", "FAST_PICK_BLK_DTYPE", "FastPickGroup",
                  "IntraFastSearchGroup", "MD_GATHERS", "CdefPic", "DlfPic", "DlfMiArgs", "LrPic", "LrWalk", "LR_UNIT_DTYPE", "LR_CAND_DTYPE",
                  "LR_RESULT_DTYPE", "LR_COSTS_DTYPE", "LR_SGR_WALK_DTYPE", "LR_SGR_BEST_DTYPE")


# -- numpy twins of the records that live in device tensors --------------------------------------------------------------------------------
def _dtype(fields):
    import numpy as np
    return np.dtype(fields)


def md_blk_dtype():
    """numpy dtype of svt_hip_md_blk"""
    return _dtype([("skip_flag_context", "u1"), ("has_uv", "u1"), ("pad", "u1", (2,))])


def md_decision_dtype():
    """numpy dtype of svt_hip_md_decision"""
    return _dtype([("cost", "<u8"), ("cost_luma", "<u8"), ("merge_cost", "<u8"), ("skip_cost", "<u8"), ("full_lambda_rate", "<u8"),
                   ("full_distortion", "<u4"), ("eob", "<u2", (3,))] +
                  [(n, "u1") for n in ("slot", "cand", "count", "is_intra", "skip_flag", "merge_flag", "y_has_coeff", "u_has_coeff", "v_has_coeff",
                                       "block_has_coeff", "tx_type", "best_intra_mode", "uv_mode", "cfl_alpha_idx", "cfl_alpha_signs")] + [("pad", "u1", (7,))])


def intra_enc_blk_dtype():
    """numpy dtype of svt_hip_intra_enc_blk (8 bytes)"""
    return _dtype([("is_intra", "u1"), ("mode", "u1"), ("angle_delta", "i1"), ("uv_mode", "u1"), ("cfl_alpha_idx", "u1"), ("cfl_alpha_signs", "u1"),
                   ("tx_type", "u1"), ("tx_type_uv", "u1")])


def intra_enc_result_dtype():
    """numpy dtype of svt_hip_intra_enc_result (8 bytes)"""
    return _dtype([("eob", "<u2", (3,)), ("tx_type", "u1"), ("pad", "u1")])


def part_leaf_dtype():
    """numpy dtype of svt_hip_part_leaf (12 bytes)"""
    return _dtype([("mds_idx", "<u2"), ("split_flag", "u1"), ("tot_d1_blocks", "u1"), ("left_partition", "i1"), ("above_partition", "i1"),
                   ("pad", "u1", (2,)), ("src", "<u4")])


def part_sb_dtype():
    """numpy dtype of svt_hip_part_sb (12 bytes)"""
    return _dtype([("leaf_first", "<u4"), ("leaf_count", "<u2"), ("origin_x", "<u2"), ("origin_y", "<u2"), ("pad", "<u2")])


def part_sq_dtype():
    """numpy dtype of svt_hip_part_sq (16 bytes)"""
    return _dtype([("cost", "<u8"), ("best_d1_blk", "<u2"), ("part", "u1"), ("split_flag", "u1"), ("tested", "u1"), ("pad", "u1", (3,))])


def part_final_dtype():
    """numpy dtype of svt_hip_part_final (12 bytes)"""
    return _dtype([("mds_idx", "<u2"), ("x", "<u2"), ("y", "<u2"), ("bsize", "u1"), ("part", "u1"), ("src", "<u4")])


def inter_cand_dtype():
    """numpy dtype of svt_hip_inter_cand"""
    return _dtype([("pred_mv", "<i2", (2, 2)), ("mode_ctx", "<i2"), ("pred_mode", "u1"), ("ref_frame_type", "u1"), ("drl_index", "u1"),
                   ("ref_mv_count", "u1"), ("drl_ctx", "u1"), ("flags", "u1")])


def inter_fast_blk_dtype():
    """numpy dtype of svt_hip_inter_fast_blk"""
    return _dtype([(n, "u1") for n in ("skip_flag_context", "is_inter_ctx", "reference_mode_context", "compoud_reference_type_context", "comp_ref_p",
                                       "comp_ref_p1", "comp_ref_p2", "comp_bwdref_p", "comp_bwdref_p1")] + [("single_ref_p", "u1", (6,)), ("has_uv", "u1")])


def interp_decision_dtype():
    """numpy dtype of svt_hip_interp_decision"""
    return _dtype([("interp_filters", "<u4"), ("switchable_rate", "<i4"), ("rd", "<i8"), ("skip_sse_sb", "<i8"), ("skip_txfm_sb", "<i4"), ("pad", "<u4")])


def inter_blk_dtype():
    """numpy dtype of svt_hip_inter_blk"""
    return _dtype([("x", "<u2"), ("y", "<u2"), ("mv", "<i2", (2, 2)), ("pred_direction", "u1"), ("filter_x", "u1"), ("filter_y", "u1"), ("pad", "u1")])


def warp_samples_dtype():
    """numpy dtype of svt_hip_warp_samples"""
    return _dtype([("nsamples", "<i4"), ("pts", "<i4", (16,)), ("pts_inref", "<i4", (16,))])


def warp_model_dtype():
    """numpy dtype of svt_hip_warp_model"""
    return _dtype([("mat", "<i4", (6,)), ("alpha", "<i2"), ("beta", "<i2"), ("gamma", "<i2"), ("delta", "<i2"), ("valid", "u1"), ("num_proj_ref", "u1"),
                   ("pad", "u1", (2,))])


def _pack_rates(tables, layout):
    import numpy as np
    parts = []
    for name, shape in layout:
        a = np.asarray(tables[name], np.int32)
        assert a.shape == shape, (name, a.shape)
        parts.append(a.reshape(-1))
    return np.concatenate(parts)


def pack_md_rates(tables):
    """dict of the three int32 tables (MD_RATE_TABLES shapes) -> int32 [655] in svt_hip_md_rates order"""
    return _pack_rates(tables, MD_RATE_TABLES)


def pack_inter_fast_rates(tables):
    """dict of the fifteen int32 tables (INTER_FAST_RATE_TABLES shapes) -> int32 [383] in svt_hip_inter_fast_rates order"""
    return _pack_rates(tables, INTER_FAST_RATE_TABLES)


def pack_fast_rates(tables):
    """dict of the six int32 tables (FAST_RATE_TABLES shapes) -> int32 [877] in svt_hip_fast_rates order"""
    return _pack_rates(tables, FAST_RATE_TABLES)


# -- the filler --------------------------------------------------------------------------------------------------------------------------------
# fill(record, g) walks the record's _fields_ and reads each from the dict g by the field's type:
#   void *d_X               the pointer of g["X"], NULL where the key is absent or None
#   a number                g.get(key, 0)
#   uint8 / int8 / uint32 [N]   the list g[key], cut to N and padded with 0
#   void *[N]               up to N planes of the list g[key] (a None in the list is NULL)
#   void *[2][3]            key ("ref0", "ref1"): one plane list per row
#   a nested record         filled from the same dict
# where key is the C field's name without its "d_".  RULES[record] states what differs:
#   keys      field -> key (or a tuple of keys, one per element of an array field)
#   defaults  field -> function of g, used where the key is absent
#   required  keys read with g[key]: a missing one is a KeyError
#   manual    fields the builder sets itself
Rules = collections.namedtuple("Rules", ("keys", "defaults", "required", "manual"), defaults=({}, {}, (), ()))


def _rows(key, alt=None):
    """default of a count: the first dimension of the tensor g[key] (or g[alt]), 0 without it"""
    def rows(g):
        t = g.get(key) if g.get(key) is not None or alt is None else g.get(alt)
        return t.shape[0] if t is not None else 0
    return rows


def _nbytes(key):
    return lambda g: g[key].numel() * g[key].element_size() if g.get(key) is not None else 0


_NTYPES = {"ntypes": lambda g: len(list(g["tx_types"]))}
_TX = ("nblocks", "tx_size", "tx_types")
_REFS = {"d_ref": ("ref0", "ref1")}
RULES = {
    FrameGroup: Rules(defaults={"nblocks": lambda g: g["xy"].numel()}, required=("src_stride", "pred_stride", "recon_stride", "xy", "tx_size", "tx_type")),
    FrameCflGroup: Rules(keys={"pred_stride_cb": "cb_stride", "pred_stride_cr": "cr_stride", "d_alpha_q3_cb": "alpha_cb", "d_alpha_q3_cr": "alpha_cr"},
                         defaults={"nblocks": lambda g: g["xy"].numel()},
                         required=("luma_recon", "luma_stride", "pred_cb", "cb_stride", "pred_cr", "cr_stride", "xy", "alpha_cb", "alpha_cr", "width", "height")),
    FullLoopGroup: Rules(defaults=_NTYPES, required=_TX),
    CoeffRateGroup: Rules(defaults=_NTYPES, required=_TX),
    TxDecideGroup: Rules(defaults=_NTYPES, required=_TX),
    CflSearchGroup: Rules(keys={"d_luma_recon": "luma"}, required=("nblocks", "tx_size")),
    CflDecideGroup: Rules(required=("nblocks",)),
    FastLoopGroup: Rules(keys={"d_top_neigh": "top", "d_left_neigh": "left", "angle_deltas": "deltas"},
                         defaults={"neigh_pitch": lambda g: g["top"].shape[1] if g.get("top") is not None else 0, "ncand": lambda g: len(list(g["modes"])[:64])},
                         required=("nblocks", "tx_size", "modes", "deltas")),
    FastPickGroup: Rules(keys={"angle_deltas": "deltas", "uv_angle_deltas": "uv_deltas"}, defaults={"ncand": lambda g: len(list(g.get("modes", [])))}),
    InterPredGroup: Rules(keys=_REFS, defaults={"nblocks": _rows("blk")}),
    WarpFitGroup: Rules(defaults={"nblocks": _rows("samples")}),
    WarpPredGroup: Rules(defaults={"nblocks": _rows("blk"), "n": lambda g: g["sel"].shape[1] if g.get("sel") is not None else 0}),
    InterpSseGroup: Rules(keys=_REFS, defaults={"nblocks": _rows("blk")}),
    InterpDecideGroup: Rules(defaults={"nblocks": _rows("decision")}),
    InterFastPickGroup: Rules(defaults={"nblocks": _rows("ctx")}),
    InterFastSearchGroup: Rules(keys=_REFS),
    MdDecideGroup: Rules(required=("bsize", "nblocks", "n")),
    PartitionArgs: Rules(defaults={"nsb": lambda g: g["sb"].shape[0], "nleaves": _rows("leaf"), "nsrc": _rows("decision", "cost")}),
    ReconFinalGroup: Rules(required=("src_first", "nblocks", "bsize")),
    ReconFinalArgs: Rules(defaults={"nsb": lambda g: g["final_count"].shape[0], "nsrc": lambda g: g["decision"].shape[0],
                                    "ngroups": lambda g: len(g.get("groups") or []), "planes": lambda g: len(g.get("recon") or ()),
                                    "scratch_bytes": _nbytes("scratch")}, manual=("groups", "stride", "width", "height")),
    IntraEncodeArgs: Rules(defaults={"npics": lambda g: 1, "nsrc": _rows("blk"), "scratch_bytes": _nbytes("scratch")}, required=("sb_cols", "sb_rows"),
                           manual=("q_luma", "q_chroma", "src_stride", "stride", "width", "height")),
}
_NO_RULES = Rules()


def _ptr(t):
    return t.data_ptr() if t is not None else None


def _planes(dst, planes):
    planes = planes or ()
    for p in range(len(dst)):
        dst[p] = _ptr(planes[p]) if p < len(planes) else None


def fill(rec, g):
    """fill the ctypes record from the dict g (the rules stand above RULES) -> rec"""
    rules = RULES.get(type(rec), _NO_RULES)
    for name, ctype in rec._fields_:
        if name in rules.manual:
            continue
        if issubclass(ctype, Structure):
            fill(getattr(rec, name), g)
            continue
        c_name = C_FIELD.get(name, name)
        key = rules.keys.get(name, c_name[2:] if c_name.startswith("d_") else c_name)
        if ctype is c_void_p:
            setattr(rec, name, _ptr(g[key] if key in rules.required else g.get(key)))
        elif not issubclass(ctype, ctypes.Array):
            if key in rules.required:
                v = g[key]
            elif name in rules.defaults and key not in g:
                v = rules.defaults[name](g)
            else:
                v = g.get(key, 0)
            setattr(rec, name, int(v))
        elif isinstance(key, tuple):                                    # one key per element: pointers, or plane lists
            for i, k in enumerate(key):
                if ctype._type_ is c_void_p:
                    getattr(rec, name)[i] = _ptr(g.get(k))
                else:
                    _planes(getattr(rec, name)[i], g.get(k))
        elif ctype._type_ is c_void_p:
            _planes(getattr(rec, name), g.get(key))
        else:
            v = g[key] if key in rules.required else g.get(key)             # a list, a tuple or a numpy array
            v = [int(x) for x in list(() if v is None else v)[:ctype._length_]]
            setattr(rec, name, ctype(*(v + [0] * (ctype._length_ - len(v)))))
    return rec


def build(Record, groups, at_least=1):
    """the ctypes array of a list of dicts, one filled Record each (at_least: the length of the array of an empty list)"""
    arr = (Record * max(len(groups), at_least))()
    for i, g in enumerate(groups):
        fill(arr[i], g)
    return arr


# what the package re-exports (fill and build stay records.fill / records.build: the package has a submodule named build)
__all__ = [n for n in dir() if not n.startswith("_") and n not in ("collections", "ctypes", "i8", "i16", "i32", "i64", "u8", "u16", "u32", "u64",
                                                                    "c_size_t", "c_void_p", "Structure", "record", "fill", "build")]
