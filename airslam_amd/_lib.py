"""ctypes binding of libairfe.so (include/airfe.h).  No fallback: if the HIP library is missing or no GPU is
visible the product path raises — there is no CPU implementation behind this package."""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libairfe.so")


class Tuning(C.Structure):
    """airfe_tuning (include/airfe.h): kernel-selection overrides, -1 = the library's choice"""
    _fields_ = [(n, C.c_int) for n in (
        "fuse_lg_block", "gemm_small_max_m", "gemm8_min_m", "gemmr_min_m", "gemmr_wgs", "qkv_pair", "block_min_m", "lgb_tokens", "sg_kenc_gemm",
        "fold_qkv", "overlap_lines", "kf_graph", "kf_spec_rows", "fuse_dec", "assign_fused", "fold_out_proj", "desc_gather_stream", "copy_wgs")] + [("reserved", C.c_int * 5)]


class Cfg(C.Structure):
    _fields_ = [
        ("device", C.c_int), ("precision", C.c_int), ("max_batch", C.c_int), ("enc_chunk", C.c_int),
        ("max_keypoints", C.c_int), ("keypoint_threshold", C.c_float), ("remove_borders", C.c_int),
        ("nms_radius", C.c_int), ("line_threshold", C.c_float), ("line_length_threshold", C.c_float),
        ("matcher", C.c_int), ("image_width", C.c_int), ("image_height", C.c_int), ("sinkhorn_iters", C.c_int),
        ("superpoint_pack", C.c_char_p), ("plnet_s1_pack", C.c_char_p), ("lightglue_pack", C.c_char_p),
        ("superglue_pack", C.c_char_p), ("matcher_precision", C.c_int), ("line_precision", C.c_int), ("check_launches", C.c_int),
        ("tuning", C.POINTER(Tuning)),
    ]


class Stage0(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in (
        "juncs_pred", "lines_pred", "iskeep", "idx_junc_to_end_min", "idx_junc_to_end_max",
        "loi_features", "loi_features_thin", "loi_features_aux")]


class BowdbFilter(C.Structure):
    """airfe_bowdb_filter (include/airfe.h)"""
    _fields_ = [("ratio", C.c_float), ("min_words", C.c_int), ("d_max_index", C.c_void_p), ("d_exclude", C.c_void_p), ("exclude_words", C.c_int)]


class RelocCfg(C.Structure):
    """airfe_reloc_cfg (include/airfe.h)"""
    _fields_ = [("ratio", C.c_float), ("min_words", C.c_int), ("K", C.c_int), ("outlier_rejection", C.c_int), ("min_inlier", C.c_int),
                ("pose_refinement", C.c_int), ("cam", C.c_double * 5), ("thr", C.c_double * 2)]


class LoopCfg(C.Structure):
    """airfe_loop_cfg (include/airfe.h)"""
    _fields_ = [("ratio", C.c_float), ("min_words", C.c_int), ("K", C.c_int), ("outlier_rejection", C.c_int), ("distance_rate", C.c_double),
                ("min_matches", C.c_int), ("min_points", C.c_int), ("min_inliers", C.c_int), ("cam", C.c_double * 5), ("thr", C.c_double * 2)]


class SeqPolicy(C.Structure):
    """airfe_seq_policy (include/airfe_seq.h)"""
    _fields_ = [("min_init_stereo_feature", C.c_int), ("min_num_match", C.c_int), ("max_num_match", C.c_int), ("tracking_point_rate", C.c_float),
                ("tracking_parallax_rate", C.c_float), ("min_x_diff", C.c_double), ("max_x_diff", C.c_double), ("max_y_diff", C.c_double),
                ("image_width", C.c_int), ("image_height", C.c_int)]


class SeqFrame(C.Structure):
    """airfe_seq_frame (include/airfe_seq.h)"""
    _fields_ = ([(n, C.c_int) for n in ("frame_type", "candidate", "promoted", "dropped", "enough_match", "good_stereo_point", "n_left", "n_right", "n_lines_left",
                                        "n_lines_right", "n_junctions", "n_stereo", "n_matches")] + [("_pad", C.c_int)]
                + [(n, C.c_void_p) for n in ("features_left", "features_right", "lines_left", "lines_right", "junctions", "stereo_idx", "stereo_score", "matches_idx",
                                             "matches_score")])


class DebugLinearArgs(C.Structure):
    """airfe_debug_linear_args (include/airfe_debug.h)"""
    _fields_ = ([(n, C.c_int) for n in ("prec", "M", "K", "K1", "N")] + [(n, C.c_void_p) for n in ("x1", "x2", "w", "b")]
                + [("epi", C.c_int), ("act", C.c_int), ("rowidx", C.c_void_p), ("src_rows", C.c_int), ("rot_cos", C.c_void_p), ("rot_sin", C.c_void_p),
                   ("Np", C.c_int), ("H", C.c_int), ("x32", C.c_void_p), ("d2s_hc", C.c_int), ("d2s_wc", C.c_int), ("flag", C.c_void_p),
                   ("kernel", C.c_int), ("gr_wgs", C.c_int), ("out", C.c_void_p), ("out2", C.c_void_p)])


class DebugLgBlockArgs(C.Structure):
    """airfe_debug_lg_block_args (include/airfe_debug.h)"""
    _fields_ = ([("prec", C.c_int), ("M", C.c_int)] + [(n, C.c_void_p) for n in ("attn", "x32", "xb", "wo", "bo", "w1", "b1", "gamma", "beta", "w2", "b2")]
                + [(n, C.c_int) for n in ("relu", "tokens_per_wg", "mixed", "nqk_n")]
                + [(n, C.c_void_p) for n in ("nqk_w", "nqk_b", "nv_w", "nv_b", "rot_cos", "rot_sin")]
                + [("Np", C.c_int)] + [(n, C.c_void_p) for n in ("q", "k", "vt")] + [("rows_past", C.c_int * 5)])


class DebugWgPrimsArgs(C.Structure):
    """airfe_debug_wg_prims_args (include/airfe_debug.h)"""
    _fields_ = [("v", C.c_void_p), ("keep", C.c_void_p), ("n", C.c_int), ("threads", C.c_int), ("keys", C.c_void_p), ("P", C.c_int), ("key_bytes", C.c_int),
                ("scan", C.c_void_p), ("pos", C.c_void_p), ("totals", C.c_void_p), ("wave", C.c_void_p), ("sorted", C.c_void_p)]


class DebugConvArgs(C.Structure):
    """airfe_debug_conv_args (include/airfe_debug.h)"""
    _fields_ = ([(n, C.c_void_p) for n in ("x", "img", "w1a", "b1a", "w", "b")] + [(n, C.c_int) for n in ("cin", "cout", "B", "H", "W", "pool", "out_pad", "relu", "wgs")]
                + [("y_words", C.c_size_t), ("y_raw", C.c_void_p)])


class DebugLgPrepareArgs(C.Structure):
    """airfe_debug_lg_prepare_args (include/airfe_debug.h)"""
    _fields_ = ([(n, C.c_int) for n in ("prec", "B", "cap", "ld", "kp_off", "normalize")] + [(n, C.c_float) for n in ("cx", "cy", "linv")]
                + [(n, C.c_void_p) for n in ("f0", "f1", "n0", "n1", "wr", "f0x", "f1x")] + [(n, C.c_int) for n in ("n0x", "n1x", "slack_rows", "rows")]
                + [(n, C.c_void_p) for n in ("x32", "xb", "rot_cos", "rot_sin", "lens")] + [("rows_past", C.c_int)])


class DebugLgAssignArgs(C.Structure):
    """airfe_debug_lg_assign_args (include/airfe_debug.h)"""
    _fields_ = ([(n, C.c_int) for n in ("prec", "B", "n")] + [(n, C.c_void_p) for n in ("md", "x32", "w")] + [("b", C.c_float), ("lens", C.c_void_p), ("cap", C.c_int),
                ("thr", C.c_float), ("form", C.c_int)]
                + [(n, C.c_void_p) for n in ("pad", "z", "sim", "scores", "rowlse", "collse", "rowval", "rowarg", "colarg", "idx", "score", "nmatch")])


class DebugSgFrontArgs(C.Structure):
    """airfe_debug_sg_front_args (include/airfe_debug.h)"""
    _fields_ = ([(n, C.c_int) for n in ("prec", "split", "B", "cap", "normalize")] + [(n, C.c_void_p) for n in ("f0", "f1", "n0", "n1")] + [("rows", C.c_int)]
                + [(n, C.c_void_p) for n in ("lens", "x32", "xb", "h128", "hb")] + [("rows_past", C.c_int)])


class DebugAttentionArgs(C.Structure):
    """airfe_debug_attn_args (include/airfe_debug.h)"""
    _fields_ = ([(n, C.c_int) for n in ("prec", "S", "H", "n", "cross")] + [(n, C.c_void_p) for n in ("q", "k", "v", "lens")]
                + [("canary", C.c_int), ("raw", C.c_int), ("out", C.c_void_p), ("Np", C.c_int), ("rows_past", C.c_int)])


class DebugDetectorTailArgs(C.Structure):
    """airfe_debug_detector_tail_args (include/airfe_debug.h)"""
    _fields_ = ([(n, C.c_int) for n in ("B", "Bs", "h", "w", "cap")] + [(n, C.c_void_p) for n in ("heat", "act", "feat", "feat1", "n", "n1", "nms_map", "keep", "cand_cnt")]
                + [("nms_map_written", C.c_int)])


class DebugLinePostArgs(C.Structure):
    """airfe_debug_line_post_args (include/airfe_debug.h)"""
    _fields_ = ([(n, C.c_int) for n in ("B", "nj", "ld", "h", "w", "capL", "capJ", "from_plane")]
                + [(n, C.c_void_p) for n in ("la", "sc", "m2", "heat", "lines", "nlines", "nfound", "junc", "njunc", "jfound", "jmap")])


class DebugJunctionTailArgs(C.Structure):
    """airfe_debug_junction_tail_args (include/airfe_debug.h)"""
    _fields_ = ([(n, C.c_int) for n in ("B", "nj", "ld", "h", "w", "capL", "capJ")]
                + [(n, C.c_void_p) for n in ("la", "sc", "m2", "heat", "act", "lines", "nlines", "nfound", "junc", "njunc", "jfound")] + [("fused", C.c_int)])


class DebugLineMidArgs(C.Structure):
    """airfe_debug_line_mid_args (include/airfe_debug.h)"""
    _fields_ = ([(n, C.c_int) for n in ("B", "j2l", "s1_form", "wgs")]
                + [(n, C.c_void_p) for n in ("juncs_pred", "lines_pred", "thin", "aux", "loi", "iskeep_in", "idx_min_in", "idx_max_in", "iskeep", "idx_min", "idx_max", "counts",
                                             "keep", "pairs", "rep", "head4", "prop4", "ridx", "proj", "lines_adjusted", "scores_line", "table_dirty")])


class DebugS0DecodeArgs(C.Structure):
    """airfe_debug_s0_decode_args (include/airfe_debug.h)"""
    _fields_ = ([(n, C.c_int) for n in ("B", "mode", "ld", "off", "want_ta8", "want_loi", "want_jnms", "prec", "wgs")] + [(n, C.c_void_p) for n in ("rows", "x", "w", "b")]
                + [("stage_floats", C.c_size_t)] + [(n, C.c_void_p) for n in ("stage", "jloc", "joff", "jnms", "ta8", "loi", "head_rows")])


# name -> (restype, argtypes); every symbol include/*.h declares
SIGNATURES = {
    "airfe_copy_rows_dev": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "airfe_pack_rows_dev": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "airfe_seq_default_policy": (None, [C.POINTER(SeqPolicy)]),
    "airfe_seq_add_keyframe_check": (C.c_int, [C.POINTER(SeqPolicy), C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int]),
    "airfe_seq_good_stereo_points": (C.c_int, [C.POINTER(SeqPolicy), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]),
    "airfe_seq_create": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(SeqPolicy), C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)]),
    "airfe_seq_destroy": (None, [C.c_void_p]),
    "airfe_seq_last_error": (C.c_char_p, [C.c_void_p]),
    "airfe_seq_begin": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_size_t]),
    "airfe_seq_end": (C.c_int, [C.c_void_p, C.POINTER(SeqFrame)]),
    "airfe_seq_step": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_size_t, C.POINTER(SeqFrame)]),
    "airfe_seq_stream": (C.c_void_p, [C.c_void_p]),
    "airfe_seq_set_outlier_rejection": (C.c_int, [C.c_void_p, C.c_int]),
    "airfe_seq_wall_split": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "airfe_default_cfg": (None, [C.POINTER(Cfg)]),
    "airfe_default_tuning": (None, [C.POINTER(Tuning)]),
    "airfe_debug_fail_next_launch": (C.c_int, [C.c_void_p, C.c_int]),
    "airfe_create": (C.c_int, [C.POINTER(Cfg), C.POINTER(C.c_void_p)]),
    "airfe_destroy": (None, [C.c_void_p]),
    "airfe_last_error": (C.c_char_p, [C.c_void_p]),
    "airfe_detect_points": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int,
                                      C.POINTER(C.c_int)]),
    "airfe_has_line_branch": (C.c_int, [C.c_void_p]),
    "airfe_detect_plnet": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(Stage0), C.c_void_p,
                                     C.c_int, C.POINTER(C.c_int), C.c_void_p, C.c_int, C.POINTER(C.c_int), C.c_void_p,
                                     C.c_int, C.POINTER(C.c_int), C.c_int]),
    "airfe_stereo_keyframe": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                        C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int),
                                        C.POINTER(C.c_int), C.c_void_p, C.c_int, C.POINTER(C.c_int), C.c_void_p, C.c_void_p, C.c_int,
                                        C.POINTER(C.c_int)]),
    "airfe_stereo_keyframe_tracked": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                                C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int),
                                                C.POINTER(C.c_int), C.c_void_p, C.c_int, C.POINTER(C.c_int), C.c_void_p, C.c_void_p, C.c_int,
                                                C.POINTER(C.c_int), C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_int)]),
    "airfe_track_frame": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_int),
                                    C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int)]),
    "airfe_promote_frame": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_int), C.c_void_p, C.c_void_p, C.c_int,
                                      C.POINTER(C.c_int)]),
    "airfe_adopt_reference": (C.c_int, [C.c_void_p]),
    "airfe_match_lightglue": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                        C.c_int, C.POINTER(C.c_int)]),
    "airfe_match_superglue": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_void_p]),
    "airfe_assign_points_to_lines": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                               C.c_void_p, C.c_int, C.c_void_p]),
    "airfe_match_lines": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                    C.c_void_p, C.c_int, C.c_void_p]),
    "airfe_bow_load": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]),
    "airfe_bow_transform": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "airfe_bow_transform_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "airfe_bow_vector": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_int), C.c_void_p]),
    "airfe_bow_vector_batch_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 5),
    "airfe_bowdb_create": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    "airfe_bowdb_destroy": (C.c_int, [C.c_void_p]),
    "airfe_bowdb_clear": (C.c_int, [C.c_void_p]),
    "airfe_bowdb_size": (C.c_int, [C.c_void_p]),
    "airfe_bowdb_add_batch_dev": (C.c_int, [C.c_void_p] * 6 + [C.c_int, C.c_int, C.c_void_p]),
    "airfe_bowdb_add": (C.c_int, [C.c_void_p] * 6 + [C.c_int, C.c_int]),
    "airfe_bowdb_query_batch_dev": (C.c_int, [C.c_void_p] * 4 + [C.c_int, C.c_int, C.POINTER(BowdbFilter)] + [C.c_void_p] * 3 + [C.c_int] + [C.c_void_p] * 4),
    "airfe_bowdb_topk_dev": (C.c_int, [C.c_void_p] * 4 + [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "airfe_bowdb_match_candidates_batch_dev": (C.c_int, [C.c_void_p] * 4 + [C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 3 + [C.c_int] + [C.c_void_p] * 3),
    "airfe_bowdb_attach_map": (C.c_int, [C.c_void_p, C.c_int]),
    "airfe_bowdb_set_points_dev": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "airfe_bowdb_set_points": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "airfe_bowdb_get_points": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "airfe_bowdb_set_covisibility": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]),
    "airfe_bowdb_get_covisibility": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int)]),
    "airfe_bowdb_set_positions": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "airfe_bowdb_group_dev": (C.c_int, [C.c_void_p, C.c_int] + [C.c_void_p] * 3 + [C.c_int] * 3 + [C.c_void_p] * 8),
    "airfe_relocalize_batch_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(RelocCfg), C.c_void_p, C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 9 +
                                   [C.c_int] + [C.c_void_p] * 3),
    "airfe_bowdb_set_poses": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "airfe_bowdb_get_poses": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "airfe_bowdb_set_u_right_dev": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "airfe_bowdb_set_u_right": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "airfe_bowdb_get_u_right": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "airfe_bowdb_attach_point_ids": (C.c_int, [C.c_void_p, C.c_int]),
    "airfe_bowdb_set_point_ids_dev": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "airfe_bowdb_set_point_ids": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "airfe_bowdb_get_point_ids": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "airfe_bowdb_build_covisibility_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "airfe_bowdb_build_covisibility": (C.c_int, [C.c_void_p, C.POINTER(C.c_int)]),
    "airfe_bowdb_attach_triangulation": (C.c_int, [C.c_void_p]),
    "airfe_bowdb_triangulate_points_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 5),
    "airfe_bowdb_triangulate_points": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int)]),
    "airfe_bowdb_fill_points_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "airfe_triangulate_point": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_int)]),
    "airfe_bowdb_attach_merge": (C.c_int, [C.c_void_p]),
    "airfe_bowdb_merge_points_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "airfe_bowdb_merge_points": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "airfe_bowdb_loop_merge_batch_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 6 + [C.c_int] + [C.c_void_p] * 4),
    "airfe_junction_connections_batch_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p] + [C.c_int] * 4 + [C.c_void_p, C.c_int] +
                                             [C.c_void_p] * 4),
    "airfe_junction_connections": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_int),
                                             C.c_void_p]),
    "airfe_bowdb_attach_junctions": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "airfe_bowdb_set_junctions_dev": (C.c_int, [C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 6),
    "airfe_bowdb_set_junctions": (C.c_int, [C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 5),
    "airfe_bowdb_get_junctions": (C.c_int, [C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 10),
    "airfe_bowdb_junction_term_batch_dev": (C.c_int, [C.c_void_p] * 9 + [C.c_int] + [C.c_void_p] * 4),
    "airfe_bowdb_junction_extra_batch_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p] + [C.c_int] * 4 + [C.c_void_p] * 4),
    "airfe_bowdb_add_junction_frames_batch_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p] + [C.c_int] * 4 + [C.c_void_p]),
    "airfe_bowdb_query_stored_batch_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_int, C.c_int] + [C.c_void_p] * 3 + [C.c_int] +
                                           [C.c_void_p] * 4),
    "airfe_loop_detect_batch_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(LoopCfg), C.c_void_p, C.c_int] + [C.c_void_p] * 10 + [C.c_int] +
                                    [C.c_void_p] * 3),
    "airfe_set_rectify_maps": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int]),
    "airfe_rectify_detect_points": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                              C.POINTER(C.c_int)]),
    "airfe_rectify_batch_dev": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_size_t, C.c_void_p,
                                          C.c_int, C.c_size_t, C.c_void_p]),
    "airfe_detect_points_batch_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_size_t,
                                                C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "airfe_match_lightglue_batch_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                                  C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "airfe_match_superglue_batch_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                                  C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "airfe_stereo_batch_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                         C.c_size_t, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "airfe_detect_plnet_batch_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_size_t, C.c_void_p,
                                               C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                               C.c_int, C.c_void_p, C.c_void_p]),
    "airfe_stereo_plnet_batch_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_size_t,
                                               C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                               C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                               C.c_void_p]),
    "airfe_debug_plnet_j2l": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "airfe_assign_points_to_lines_batch_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                                         C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "airfe_match_lines_batch_dev": (C.c_int, [C.c_void_p] + [C.c_void_p] * 8 + [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                              C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "airfe_fundamental_ransac": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int)]),
    "airfe_fundamental_ransac_batch_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                                     C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "airfe_set_outlier_rejection": (C.c_int, [C.c_void_p, C.c_int]),
    "airfe_pnp_ransac": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int)]),
    "airfe_pnp_ransac_batch_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                             C.c_void_p, C.c_void_p, C.c_void_p]),
    "airfe_stereo_points": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.POINTER(C.c_int)]),
    "airfe_stereo_points_batch_dev": (C.c_int, [C.c_void_p] * 6 + [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 5),
    "airfe_stereo_lines": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int] + [C.c_void_p] * 8),
    "airfe_stereo_lines_batch_dev": (C.c_int, [C.c_void_p] * 6 + [C.c_int, C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 7),
    "airfe_stereo_line_landmarks_batch_dev": (C.c_int, [C.c_void_p] * 6 + [C.c_int] + [C.c_void_p] * 4 + [C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                                        C.c_void_p, C.c_int] + [C.c_void_p] * 8 + [C.c_int] + [C.c_void_p] * 8),
    "airfe_track_pose_batch_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                             C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "airfe_frame_optimize": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 7 + [C.POINTER(C.c_int)]),
    "airfe_frame_optimize_batch_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 9),
    "airfe_track_pose_opt_batch_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p,
                                                 C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 9),
    "airfe_sync": (C.c_int, [C.c_void_p]),
    "airfe_superglue_status": (C.c_int, [C.c_void_p, C.c_void_p]),
    "airfe_profile_enable": (C.c_int, [C.c_void_p, C.c_int]),
    "airfe_profile_stages": (C.c_int, []),
    "airfe_profile_stage_name": (C.c_char_p, [C.c_int]),
    "airfe_profile_read": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "airfe_debug_detector_maps": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "airfe_debug_lightglue_scores": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    "airfe_debug_superglue_scores": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    "airfe_debug_lg_filter": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int)]),
    "airfe_debug_sg_decode": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "airfe_debug_sg_sinkhorn": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_int)]),
    "airfe_debug_detector_tail": (C.c_int, [C.c_void_p, C.POINTER(DebugDetectorTailArgs)]),
    "airfe_debug_line_post": (C.c_int, [C.c_void_p, C.POINTER(DebugLinePostArgs)]),
    "airfe_debug_junction_tail": (C.c_int, [C.c_void_p, C.POINTER(DebugJunctionTailArgs)]),
    "airfe_debug_junctions_topk": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "airfe_debug_line_mid": (C.c_int, [C.c_void_p, C.POINTER(DebugLineMidArgs)]),
    "airfe_debug_s0_decode": (C.c_int, [C.c_void_p, C.POINTER(DebugS0DecodeArgs)]),
    "airfe_debug_lg_prepare": (C.c_int, [C.c_void_p, C.POINTER(DebugLgPrepareArgs)]),
    "airfe_debug_lg_assign": (C.c_int, [C.c_void_p, C.POINTER(DebugLgAssignArgs)]),
    "airfe_debug_sg_front": (C.c_int, [C.c_void_p, C.POINTER(DebugSgFrontArgs)]),
    "airfe_debug_plnet_stage0": (C.c_int, [C.c_void_p] + [C.c_void_p] * 10),
    "airfe_debug_plnet_s1": (C.c_int, [C.c_void_p, C.POINTER(Stage0), C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int)]),
    "airfe_debug_plnet_s1_last": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int)]),
    "airfe_debug_preprocess": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "airfe_debug_conv3x3": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                      C.c_int, C.c_int, C.c_void_p]),
    "airfe_debug_conv": (C.c_int, [C.c_void_p, C.POINTER(DebugConvArgs)]),
    "airfe_debug_trace": (C.c_int, [C.c_void_p, C.c_int]),
    "airfe_debug_trace_stop": (C.c_int, [C.c_void_p, C.c_int]),
    "airfe_debug_trace_buffer": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t]),
    "airfe_debug_trace_slots": (C.c_int, [C.c_void_p]),
    "airfe_debug_conv_order": (C.c_int, [C.c_int, C.POINTER(C.c_int)]),
    "airfe_debug_wg_prims": (C.c_int, [C.c_void_p, C.POINTER(DebugWgPrimsArgs)]),
    "airfe_debug_trace_slot": (C.c_int, [C.c_void_p, C.c_int, C.c_char_p, C.c_int, C.POINTER(C.c_uint), C.POINTER(C.c_uint), C.POINTER(C.c_uint)]),
    "airfe_debug_trace_read": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "airfe_debug_gemm": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                   C.c_void_p]),
    "airfe_debug_linear": (C.c_int, [C.c_void_p, C.POINTER(DebugLinearArgs)]),
    "airfe_debug_qkv": (C.c_int, [C.c_void_p] + [C.c_int] * 3 + [C.c_void_p] * 3 + [C.c_int] + [C.c_void_p] * 4 + [C.c_int] * 2 + [C.c_void_p] * 3),
    "airfe_debug_lg_block": (C.c_int, [C.c_void_p, C.POINTER(DebugLgBlockArgs)]),
    "airfe_debug_ln_gelu": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]),
    "airfe_debug_attention_args": (C.c_int, [C.c_void_p, C.POINTER(DebugAttentionArgs)]),
    "airfe_debug_attention": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
}

_lib = None


def lib() -> C.CDLL:
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} is missing: build it with `python -m airslam_amd.build` "
                "(hipcc, gfx950).  airslam_amd has no CPU fallback.")
        # PyTorch-ROCm ships its own libamdhip64; with two HIP runtimes in one process the one that initialises second sees no
        # device.  Importing torch BEFORE the dlopen makes libairfe.so bind to the runtime torch uses (same soname), whatever order
        # the caller imports things in (__graft_entry__.build() loads the library before smoke() imports torch).
        try:
            import torch  # noqa: F401
        except Exception:
            pass
        l = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(l, name)      # AttributeError if the library does not export it
            fn.restype = res
            fn.argtypes = args
        _lib = l
    return _lib
