"""ctypes binding of libw2l_hip.so (the C ABI declared in include/w2l_hip.h).

There is no fallback: if the shared library is missing or a call fails, a RuntimeError is raised
(the exception type the reference's callers already expect from a failing GPU op, inference.py:79).
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# W2L_HIP_LIB selects an alternative build of the same ABI (kernel A/B experiments); default = the in-tree build
LIB_PATH = os.environ.get("W2L_HIP_LIB") or os.path.join(_HERE, "lib", "libw2l_hip.so")

ACT_NONE, ACT_RELU, ACT_SIGMOID, ACT_LEAKY = 0, 1, 2, 3
PREC_F32, PREC_BF16 = 0, 1


class ConvGeom(C.Structure):
    _fields_ = [(n, C.c_int) for n in
                ("transposed", "cin", "cout", "kh", "kw", "sh", "sw", "ph", "pw", "oph", "opw", "act")]


class AdamTensor(C.Structure):
    """w2l_adam_tensor: device pointers + element count of one parameter"""
    _fields_ = [("param", C.c_void_p), ("grad", C.c_void_p), ("exp_avg", C.c_void_p), ("exp_avg_sq", C.c_void_p),
                ("n", C.c_longlong)]


class WgradInfo(C.Structure):
    """w2l_wgrad_info: what w2l_conv_wgrad_prec would run (w2l_conv_wgrad_resolve)"""
    _fields_ = [(n, C.c_int) for n in ("family", "cfg", "ksplit", "chunk", "K", "kstep", "reduce_blocks")]


class WgradBf16Info(C.Structure):
    """w2l_wgrad_bf16_info: the plan of w2l_conv_wgrad_bf16 (w2l_conv_wgrad_bf16_resolve)"""
    _fields_ = [(n, C.c_int) for n in ("ni", "bh", "bw", "nboxes", "splits", "boxes_per_split", "ntg", "tg", "ncq", "mt", "qp")]


# The table structs of the packed paths.  The typedef in include/w2l_hip.h is the authority, the class here mirrors it
# (tests/test_struct_mirrors_cpu.py holds every pair together), and the numpy dtype the modules fill their tables through is
# derived from the class, so a layout is typed once on this side.
class FrameRow(C.Structure):
    """w2l_frame_row (include/w2l_hip.h): one face row of the row-table kernels, 48 bytes"""
    _fields_ = [("src", C.c_uint64), ("dst", C.c_uint64), ("H", C.c_int32), ("W", C.c_int32), ("y1", C.c_int32),
                ("y2", C.c_int32), ("x1", C.c_int32), ("x2", C.c_int32), ("pad", C.c_int32 * 2)]


FRAME_ROW = np.dtype(FrameRow)


class ResizeRow(C.Structure):
    """w2l_resize_row: one frame of the whole-frame row-table resize, 32 bytes"""
    _fields_ = [("src", C.c_uint64), ("dst", C.c_uint64), ("Hs", C.c_int32), ("Ws", C.c_int32), ("Hd", C.c_int32),
                ("Wd", C.c_int32)]


RESIZE_ROW = np.dtype(ResizeRow)


class JpegInfo(C.Structure):
    """w2l_jpeg_info: what w2l_jpeg_parse reads from one file's markers"""
    _fields_ = [("H", C.c_int32), ("W", C.c_int32), ("ecs_offset", C.c_int32), ("ecs_bytes", C.c_int32), ("eoi", C.c_int32),
                ("nvals", C.c_int32 * 4), ("quant", (C.c_uint8 * 64) * 2), ("bits", (C.c_uint8 * 16) * 4),
                ("vals", (C.c_uint8 * 256) * 4)]


class JpegRow(C.Structure):
    """w2l_jpeg_row: one file of w2l_jpeg_decode_rows, 32 bytes"""
    _fields_ = [("src", C.c_uint64), ("dst", C.c_uint64), ("nbytes", C.c_int32), ("H", C.c_int32), ("W", C.c_int32),
                ("table", C.c_int32)]


JPEG_ROW = np.dtype(JpegRow)


class JpegSegment(C.Structure):
    """w2l_jpeg_segment: one restart interval of w2l_jpeg_decode_rows_rst, 32 bytes"""
    _fields_ = [(n, C.c_int32) for n in ("row", "offset", "nbytes", "first_mcu", "n_mcus")] + [("pad", C.c_int32 * 3)]


JPEG_SEGMENT = np.dtype(JpegSegment)


class MelRow(C.Structure):
    """w2l_mel_row: one mel window of the row-table gather, 16 bytes"""
    _fields_ = [("mel", C.c_uint64), ("T", C.c_int32), ("start", C.c_int32)]


MEL_ROW = np.dtype(MelRow)


class SyncRow(C.Structure):
    """w2l_sync_row: one scorer window of w2l_sync_window_rows, 32 bytes"""
    _fields_ = [("frames", C.c_uint64), ("mel", C.c_uint64), ("T", C.c_int32), ("start", C.c_int32), ("pad", C.c_int32 * 2)]


SYNC_ROW = np.dtype(SyncRow)


class LseSegment(C.Structure):
    """w2l_lse_segment: one clip's rows of w2l_lse_score_segments, 8 bytes"""
    _fields_ = [("row0", C.c_int32), ("n", C.c_int32)]


LSE_SEGMENT = np.dtype(LseSegment)


class BoxSegment(C.Structure):
    """w2l_box_segment: one clip's rows of w2l_face_boxes_segments, 16 bytes"""
    _fields_ = [("row0", C.c_int32), ("n", C.c_int32), ("H", C.c_int32), ("W", C.c_int32)]


BOX_SEGMENT = np.dtype(BoxSegment)


class BoxStreamSegment(C.Structure):
    """w2l_box_stream_segment: one live stream's rows of a tick of w2l_face_boxes_stream, 32 bytes"""
    _fields_ = [(n, C.c_int32) for n in ("row0", "n_new", "H", "W", "slot", "seen", "closed", "out0")]


BOX_STREAM_SEGMENT = np.dtype(BoxStreamSegment)


class TrackSegment(C.Structure):
    """w2l_track_segment: one clip's (or one live stream's new) rows of w2l_face_track_segments, 16 bytes"""
    _fields_ = [(n, C.c_int32) for n in ("row0", "n", "slot", "seen")]


TRACK_SEGMENT = np.dtype(TrackSegment)


class StrideSegment(C.Structure):
    """w2l_stride_segment: one clip's (or shot's) key rows and full rows of w2l_face_rects_expand_segments, 16 bytes"""
    _fields_ = [(n, C.c_int32) for n in ("key_row0", "row0", "n", "zero")]


STRIDE_SEGMENT = np.dtype(StrideSegment)


class MelStream(C.Structure):
    """w2l_mel_stream: one stream of w2l_mel_stream_cols, 48 bytes"""
    _fields_ = [("samples", C.c_uint64), ("first", C.c_int64), ("total", C.c_int64), ("window", C.c_uint64), ("held", C.c_int32),
                ("cap", C.c_int32), ("col0", C.c_int64)]


MEL_STREAM = np.dtype(MelStream)


class MelCol(C.Structure):
    """w2l_mel_col: one (stream, column) entry of w2l_mel_stream_cols, 16 bytes"""
    _fields_ = [("stream", C.c_int32), ("rsv", C.c_int32), ("col", C.c_int64)]


MEL_COL = np.dtype(MelCol)


class ResampleStreamEntry(C.Structure):
    """w2l_resample_stream_entry: one stream of w2l_resample_stream, 128 bytes"""
    _fields_ = [("src", C.c_uint64), ("src_first", C.c_int64), ("src_total", C.c_int64), ("n_res", C.c_int64), ("dst16", C.c_uint64),
                ("dst_first", C.c_int64), ("win", C.c_uint64), ("delta", C.c_uint64), ("carry", C.c_uint64), ("carry_first", C.c_int64),
                ("scale", C.c_double), ("inc", C.c_double), ("src_held", C.c_int32), ("dst_cap", C.c_int32), ("index_step", C.c_int32),
                ("nwin", C.c_int32), ("carry_held", C.c_int32), ("unused", C.c_int32 * 3)]


RESAMPLE_STREAM = np.dtype(ResampleStreamEntry)


class ResampleBlock(C.Structure):
    """w2l_resample_block: up to 128 consecutive outputs of one stream of w2l_resample_stream, 32 bytes"""
    _fields_ = [("stream", C.c_int32), ("count", C.c_int32), ("t0", C.c_int64), ("tr0", C.c_double), ("copy", C.c_int32),
                ("unused", C.c_int32)]


RESAMPLE_BLOCKS = np.dtype(ResampleBlock)


WGRAD_WINO, WGRAD_DIRECT, WGRAD_SMALL = 0, 1, 2

_vp, _i, _ll, _f = C.c_void_p, C.c_int, C.c_longlong, C.c_float

# name -> (restype, argtypes); must list every symbol of include/w2l_hip.h (tests/test_abi.py checks it)
SIGNATURES = {
    "w2l_last_error": (C.c_char_p, []),
    "w2l_abi_version": (_i, []),
    "w2l_device_count": (_i, []),
    "w2l_device_arch": (_i, [_i, C.c_char_p, C.c_size_t]),
    "w2l_conv_create": (_i, [C.POINTER(ConvGeom), _vp, _vp, _vp, _vp, C.POINTER(_vp)]),
    "w2l_conv_destroy": (_i, [_vp]),
    "w2l_conv_block_plan": (_i, [_i, _i, _i, _i, C.POINTER(_i)]),
    "w2l_conv_cin_padded": (_i, [_i]),
    "w2l_conv_out_hw": (_i, [C.POINTER(ConvGeom), _i, _i, C.POINTER(_i), C.POINTER(_i)]),
    "w2l_conv_forward": (_i, [_vp, _vp, _i, _i, _i, _vp, _i, _vp, _i, _vp, _i]),
    "w2l_conv_attach_head": (_i, [_vp, _vp, _vp, _i, _i, _vp]),
    "w2l_conv_macs": (_ll, [C.POINTER(ConvGeom), _i, _i, _i]),
    "w2l_conv_set_precision": (_i, [_vp, _i]),
    "w2l_conv_set_tile": (_i, [_vp, _i]),
    "w2l_conv_num_tiles": (_i, []),
    "w2l_bn_fold": (_i, [_vp, _i, _vp, _vp, _vp, _vp, _vp, _f, _vp, _vp]),
    "w2l_nchw_to_nhwc": (_i, [_vp, _i, _i, _i, _i, _vp, _vp, _i, _i]),
    "w2l_nhwc_to_nchw": (_i, [_vp, _i, _i, _i, _i, _vp, _i, _vp]),
    "w2l_datagen_pack": (_i, [_vp, _i, _i, _vp, _vp, _i, _i]),
    "w2l_datagen_pack_bf16": (_i, [_vp, _i, _i, _vp, _vp, _i, _i]),
    "w2l_frames_to_u8": (_i, [_vp, _i, _i, _i, _vp, _i, _vp]),
    "w2l_crop_resize_u8": (_i, [_vp, _i, _vp, _i, _i, _vp, _vp, _i, _vp]),
    "w2l_resize_u8": (_i, [_vp, _i, _vp, _i, _i, _vp, _i, _i]),
    "w2l_resize_paste_u8": (_i, [_vp, _i, _vp, _i, _vp, _vp, _vp, _i, _i, _i]),
    "w2l_crop_resize_rows_u8": (_i, [_vp, _i, _vp, _i, _vp]),
    "w2l_compose_rows_u8": (_i, [_vp, _i, _vp, _i, _vp, _i]),
    "w2l_resize_blend_u8": (_i, [_vp, _i, _vp, _i, _vp, _vp, _vp, _i, _i, _i, _i, _i]),
    "w2l_compose_blend_rows_u8": (_i, [_vp, _i, _vp, _i, _vp, _i, _i, _i]),
    "w2l_color_match_u8": (_i, [_vp, _i, _vp, _vp, _i, _i, _vp]),
    "w2l_resize_rows_u8": (_i, [_vp, _i, _vp, _i]),
    "w2l_jpeg_encode_rows": (_i, [_vp, _i, _vp, _vp, _i, _i, _vp, _vp, C.c_size_t]),
    "w2l_jpeg_workspace_bytes": (C.c_size_t, [_i, _i]),
    "w2l_jpeg_header": (_i, [_i, _i, _i, _vp]),
    "w2l_jpeg_parse": (_i, [C.c_char_p, C.c_size_t, C.POINTER(JpegInfo)]),
    "w2l_jpeg_table_bytes": (C.c_size_t, []),
    "w2l_jpeg_build_tables": (_i, [C.POINTER(JpegInfo), _vp]),
    "w2l_jpeg_decode_rows": (_i, [_vp, _i, _vp, _vp, _i, _i, _vp, _vp, C.c_size_t]),
    "w2l_jpeg_decode_workspace_bytes": (C.c_size_t, [_i, _i]),
    "w2l_jpeg_encode_rows_rst": (_i, [_vp, _i, _vp, _vp, _i, _i, _i, _vp, _vp, C.c_size_t]),
    "w2l_jpeg_workspace_bytes_rst": (C.c_size_t, [_i, _i]),
    "w2l_jpeg_capacity_rst": (C.c_size_t, [_i, _i, _i]),
    "w2l_jpeg_header_rst": (_i, [_i, _i, _i, _i, _vp]),
    "w2l_jpeg_parse_rst": (_i, [C.c_char_p, C.c_size_t, C.POINTER(JpegInfo), C.POINTER(C.c_int32)]),
    "w2l_jpeg_restart_segments": (_i, [_vp, C.c_size_t, _i, _i, _vp, _i]),
    "w2l_jpeg_decode_rows_rst": (_i, [_vp, _i, _vp, _vp, _i, _i, _vp, _i, _vp, _vp, C.c_size_t]),
    "w2l_jpeg_decode_workspace_bytes_rst": (C.c_size_t, [_i, _i]),
    "w2l_s3fd_pack": (_i, [_vp, _ll, _vp, _vp, _i]),
    "w2l_s3fd_pack_rows": (_i, [_vp, _i, _i, _i, _vp, _vp, _i]),
    "w2l_s3fd_pack_rows_scaled": (_i, [_vp, _i, _i, _i, _i, _i, _vp, _vp, _i]),
    "w2l_maxpool2x2": (_i, [_vp, _i, _i, _i, _i, _vp, _i, _vp, _i]),
    "w2l_l2norm_scale": (_i, [_vp, _ll, _i, _vp, _i, _vp, _vp, _i]),
    "w2l_s3fd_decode": (_i, [_vp, _i, _i, _i, _i, _vp, _i, _i, _vp, _i, _vp]),
    "w2l_s3fd_nms": (_i, [_vp, _i, _i, _vp, _f, _f, _vp, _vp, _vp, _ll]),
    "w2l_s3fd_first_rect": (_i, [_vp, _i, _i, _vp, _vp, _vp, _f, _vp, _vp]),
    "w2l_s3fd_first_rect_scaled": (_i, [_vp, _i, _i, _vp, _vp, _vp, _f, _f, _f, _vp, _vp]),
    "w2l_s3fd_top_rects": (_i, [_vp, _i, _i, _vp, _vp, _vp, _f, _f, _f, _i, _vp, _vp, _vp]),
    "w2l_face_track_segments": (_i, [_vp, _i, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, _i, _vp, _vp, _vp]),
    "w2l_face_boxes_segments": (_i, [_vp, _i, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, _vp]),
    "w2l_face_boxes_stream": (_i, [_vp, _i, _vp, _vp, _vp, _vp, _i, _vp, _i, _i, _i, _i, _i, _i, _vp, _i, _vp]),
    "w2l_face_boxes_runs": (_i, [_vp, _i, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp]),
    "w2l_face_spans_segments": (_i, [_vp, _i, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp]),
    "w2l_face_tracks_all_segments": (_i, [_vp, _i, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, _vp]),
    "w2l_face_rects_expand_segments": (_i, [_vp, _i, _vp, _i, _vp, _vp, _i, _vp, _vp, _i, _vp]),
    "w2l_face_boxes_stream_runs": (_i, [_vp, _i, _vp, _vp, _vp, _vp, _i, _vp, _i, _i, _i, _i, _i, _i, _i, _vp, _vp, _i, _vp]),
    "w2l_frame_hist_rows": (_i, [_vp, _i, _i, _i, _vp, _vp]),
    "w2l_scene_cuts": (_i, [_vp, _i, _vp, _vp, _i, _i, _vp, _vp, _vp]),
    "w2l_s3fd_pack_bf16": (_i, [_vp, _ll, _vp, _vp, _i]),
    "w2l_s3fd_pack_rows_bf16": (_i, [_vp, _i, _i, _i, _vp, _vp, _i]),
    "w2l_s3fd_pack_rows_scaled_bf16": (_i, [_vp, _i, _i, _i, _i, _i, _vp, _vp, _i]),
    "w2l_maxpool2x2_bf16": (_i, [_vp, _i, _i, _i, _i, _vp, _i, _vp, _i]),
    "w2l_l2norm_scale_bf16": (_i, [_vp, _ll, _i, _vp, _i, _vp, _vp, _i]),
    "w2l_s3fd_headb_create": (_i, [_i, _i, _vp, _vp, _vp, _vp, _vp, C.POINTER(_vp)]),
    "w2l_s3fd_headb_update": (_i, [_vp, _vp, _vp, _vp, _vp, _vp]),
    "w2l_s3fd_headb_destroy": (_i, [_vp]),
    "w2l_s3fd_headb_decode": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _i, _vp]),
    "w2l_mel_create": (_i, [_vp, _vp, C.POINTER(_vp)]),
    "w2l_mel_destroy": (_i, [_vp]),
    "w2l_mel_num_frames": (_i, [_ll]),
    "w2l_melspectrogram": (_i, [_vp, _vp, _vp, _ll, _vp]),
    "w2l_mel_stream_cols": (_i, [_vp, _vp, _vp, _i, _vp, _i]),
    "w2l_mel_gather": (_i, [_vp, _vp, _i, _vp, _i, _vp, _i, _i]),
    "w2l_mel_gather_bf16": (_i, [_vp, _vp, _i, _vp, _i, _vp, _i, _i]),
    "w2l_mel_gather_rows": (_i, [_vp, _vp, _i, _vp, _i, _i]),
    "w2l_mel_gather_rows_bf16": (_i, [_vp, _vp, _i, _vp, _i, _i]),
    "w2l_resample_sinc": (_i, [_vp, _vp, _i, _vp, _i, C.c_double, _vp, _vp, _i, _i, _vp]),
    "w2l_resample_stream": (_i, [_vp, _vp, _vp, _i, _vp, _i, _i]),
    "w2l_l2norm_rows": (_i, [_vp, _i, _i, _vp, _i, _vp]),
    "w2l_cosine_bce": (_i, [_vp, _i, _i, _vp, _vp, _vp, _vp, _vp]),
    "w2l_bce_mean": (_i, [_vp, _i, _vp, _vp, _vp]),
    "w2l_conv_update": (_i, [_vp, _vp, _vp, _vp, _vp]),
    "w2l_conv_wgrad": (_i, [C.POINTER(ConvGeom), _vp, _i, _i, _i, _vp, _i, _vp, _i, _vp]),
    "w2l_conv_wgrad_prec": (_i, [C.POINTER(ConvGeom), _vp, _i, _i, _i, _vp, _i, _vp, _i, _vp, _i]),
    "w2l_conv_wgrad_resolve": (_i, [C.POINTER(ConvGeom), _i, _i, _i, _i, _i, _i, C.POINTER(WgradInfo)]),
    "w2l_conv_wgrad_set_cfg": (_i, [_i, _i]),
    "w2l_wgrad_divmod_host": (_i, [_i, _i, _vp, _vp, _vp, _vp]),
    "w2l_convb_create": (_i, [C.POINTER(ConvGeom), _vp, _vp, C.POINTER(_vp)]),
    "w2l_convb_update": (_i, [_vp, _vp, _vp]),
    "w2l_convb_update_many": (_i, [_i, _vp, _vp, _vp]),
    "w2l_convb_destroy": (_i, [_vp]),
    "w2l_convb_forward": (_i, [_vp, _vp, _i, _i, _i, _vp, _i, _vp, _i, _vp, _i, _vp, _vp, _i]),
    "w2l_convb_attach_head": (_i, [_vp, _vp, _vp, _vp, _i, _i, _vp]),
    "w2l_convb_forward_head": (_i, [_vp, _vp, _i, _i, _i, _vp, _i, _vp, _vp, _i, _vp, _vp]),
    "w2l_convb_forward_bn": (_i, [_vp, _vp, _i, _i, _i, _vp, _i, _vp, _i, _vp, _vp, _vp, _f, _f, _vp, _vp, _vp, _vp, _vp, _vp]),
    "w2l_convb_forward_bnbwd": (_i, [_vp, _vp, _i, _i, _i, _vp, _i, _vp, _i, _vp, _i, _vp, _i, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp,
                                     C.POINTER(C.c_int)]),
    "w2l_convb_forward_actbwd": (_i, [_vp, _vp, _i, _i, _i, _vp, _i, _vp, _i, _vp, _i, _vp, _i, _i, _vp, C.POINTER(C.c_int)]),
    "w2l_convb_set_tile": (_i, [_vp, _i]),
    "w2l_convb_num_tiles": (_i, []),
    "w2l_convb_resolve": (_i, [_vp, _i, _i, _i, _i, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "w2l_convb_resolve_geom": (_i, [C.POINTER(ConvGeom), _i, _i, _i, _i, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int),
                                    C.POINTER(_ll)]),
    "w2l_conv_wgrad_bf16": (_i, [C.POINTER(ConvGeom), _vp, _i, _i, _i, _vp, _i, _vp, _i, _vp]),
    "w2l_conv_wgrad_bf16_resolve": (_i, [C.POINTER(ConvGeom), _i, _i, _i, _i, _i, C.POINTER(WgradBf16Info)]),
    "w2l_bn_train_stats_bf16": (_i, [_vp, _ll, _i, _i, _vp, _i, _vp, _vp, _f, _f, _vp, _vp, _vp, _vp, _vp, _vp]),
    "w2l_affine_act_bf16": (_i, [_vp, _ll, _i, _vp, _i, _vp, _vp, _vp, _i, _i, _vp, _i]),
    "w2l_bn_train_bwd_bf16": (_i, [_vp, _ll, _i, _i, _vp, _i, _vp, _i, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp, _i]),
    "w2l_bn_train_bwd_apply_bf16": (_i, [_vp, _ll, _i, _vp, _i, _vp, _i, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp, _i]),
    "w2l_act_bwd_bf16": (_i, [_vp, _ll, _i, _vp, _i, _vp, _i, _i, _vp, _vp, _i, _vp, _i]),
    "w2l_add_rows_bf16": (_i, [_vp, _ll, _i, _vp, _i, _vp, _i, _vp, _i]),
    "w2l_col_sum_bf16": (_i, [_vp, _ll, _i, _vp, _i, _vp]),
    "w2l_thin1x1_forward_bf16": (_i, [_vp, _ll, _i, _i, _vp, _i, _vp, _vp, _i, _vp, _i]),
    "w2l_thin1x1_dgrad_bf16": (_i, [_vp, _ll, _i, _i, _vp, _i, _vp, _vp, _i, _vp, _i]),
    "w2l_thin1x1_wgrad_bf16": (_i, [_vp, _ll, _i, _i, _vp, _i, _vp, _i, _vp, _vp]),
    "w2l_thin1x1_wgrad_blocks": (_i, [_ll]),
    "w2l_nchw_to_nhwc_bf16": (_i, [_vp, _i, _i, _i, _i, _vp, _vp, _i, _i]),
    "w2l_nhwc_bf16_to_nchw": (_i, [_vp, _i, _i, _i, _i, _vp, _i, _vp]),
    "w2l_bn_train_stats": (_i, [_vp, _ll, _i, _vp, _i, _vp, _vp, _f, _f, _vp, _vp, _vp, _vp, _vp, _vp]),
    "w2l_affine_act": (_i, [_vp, _ll, _i, _vp, _i, _vp, _vp, _vp, _i, _i, _vp, _i]),
    "w2l_bn_train_bwd": (_i, [_vp, _ll, _i, _vp, _i, _vp, _i, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp, _i]),
    "w2l_act_bwd": (_i, [_vp, _ll, _i, _vp, _i, _vp, _i, _i, _vp, _vp, _i, _vp, _i]),
    "w2l_add_rows": (_i, [_vp, _ll, _i, _vp, _i, _vp, _i, _vp, _i]),
    "w2l_col_sum": (_i, [_vp, _ll, _i, _vp, _i, _vp]),
    "w2l_l1_mean": (_i, [_vp, _ll, _vp, _vp, _vp]),
    "w2l_l1_bwd": (_i, [_vp, _ll, _vp, _vp, _vp, _vp]),
    "w2l_cosine_bce_bwd": (_i, [_vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "w2l_l2norm_bwd": (_i, [_vp, _i, _i, _vp, _i, _vp, _vp, _i]),
    "w2l_bce_bwd": (_i, [_vp, _i, _vp, _vp, _vp, _vp]),
    "w2l_shifted_pdist": (_i, [_vp, _i, _i, _i, _vp, _vp, _vp]),
    "w2l_sync_window_rows": (_i, [_vp, _i, _vp, _i, _vp, _i, _vp, _i]),
    "w2l_sync_window_rows_bf16": (_i, [_vp, _i, _vp, _i, _vp, _i, _vp, _i]),
    "w2l_sync_embeddings_bf16": (_i, [_vp, _i, _i, _vp, _i, _vp, _i, _vp, _vp]),
    "w2l_lse_score_segments": (_i, [_vp, _i, _vp, _i, _i, _vp, _vp, _vp, _vp]),
    "w2l_adam_create": (_i, [_i, C.POINTER(_ll), C.POINTER(_vp)]),
    "w2l_adam_destroy": (_i, [_vp]),
    "w2l_adam_step": (_i, [_vp, _vp, C.POINTER(AdamTensor), _f, _f, _f, _f, _f, _i]),
    "w2l_plan_create": (_i, [C.POINTER(_vp)]),
    "w2l_plan_destroy": (_i, [_vp]),
    "w2l_plan_add_conv": (_i, [_vp, _vp, _i, _i, _i, _vp, _i, _vp, _i, _vp, _i]),
    "w2l_plan_add_convb": (_i, [_vp, _vp, _i, _i, _i, _vp, _i, _vp, _i, _vp, _i, _vp, _vp]),
    "w2l_plan_add_convb_head": (_i, [_vp, _vp, _i, _i, _i, _vp, _i, _vp, _vp, _i, _vp, _vp]),
    "w2l_plan_copy_item": (_i, [_vp, _vp, _i]),
    "w2l_plan_run": (_i, [_vp, _vp]),
    "w2l_plan_size": (_i, [_vp]),
    "w2l_plan_autotune": (_i, [_vp, _vp, _i]),
    "w2l_plan_get_config": (_i, [_vp, _i, C.POINTER(_i), C.POINTER(_i)]),
    "w2l_plan_set_config": (_i, [_vp, _i, _i, _i]),
    "w2l_plan_profile": (_i, [_vp, _vp, _i, _vp]),
    "w2l_plan_executed_flops": (_i, [_vp, C.POINTER(_ll), C.POINTER(_i)]),
    "w2l_conv_num_igemm_tiles": (_i, []),
    "w2l_flops_begin": (_i, []),
    "w2l_flops_end": (_ll, [C.POINTER(_ll)]),
    "w2l_clock_probe": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    "w2l_igemm_block_order": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "w2l_wino4_block_plan": (_i, [_i, _i, _i, _vp]),
    "w2l_conv_config_family": (_i, [_i]),
    "w2l_conv_exclude_families": (_i, [_i]),
    "w2l_tune_key_ints": (_i, []),
    "w2l_tune_set": (_i, [C.POINTER(_i), _i, _i]),
    "w2l_tune_entry_applicable": (_i, [C.POINTER(_i), _i]),
    "w2l_tune_clear": (_i, []),
    "w2l_tune_count": (_i, []),
    "w2l_tune_export": (_i, [C.POINTER(_i), _i]),
}

_lib = None

# Shape-keyed launch configurations (include/w2l_hip.h, "tune table"): the committed file is loaded into the library once per
# process, so that a layer's (tile, split-K) - and with it its summation order and every bit of its output - is a function of
# its shape alone.  W2L_TUNE_TABLE=<path> selects another file, W2L_TUNE_TABLE=0 none (heuristic configurations only).
TUNE_TABLE_PATH = os.path.join(_HERE, "tune_table.json")
# W2L_EXACT=1 (bench.py --exact): the launch table tuned WITHOUT the F(4x4,3x3) Winograd kernel, and that family switched off
# in the library: F(2x2) / implicit-GEMM launches only, about half the rounding error of the default table at a measured cost
# in frames/s.  Both tables are functions of the shape: either mode is bit-reproducible on its own.
EXACT = os.environ.get("W2L_EXACT", "0") == "1"
EXACT_TABLE_PATH = os.path.join(_HERE, "tune_table_exact.json")
# The kernel family of a configuration id (w2l_conv_config_family) names FAMILY_NAMES[family]: the implicit GEMM, F(2x2,3x3)
# Winograd and its second form (conv_wino2, wino2q included), the fused-phase stride-2 transposed kernel, F(4x4,3x3) Winograd; then
# the split-operand families, whose fp32 operands enter the bf16 matrix cores as three bf16 pieces: the implicit GEMM, F(2x2)
# Winograd, the transposed kernel, the 7x7 first layer and the direct 3x3 for 32-cout layers (+ fused 1x1 head).
FAMILY_NAMES = ("igemm", "wino", "wino2", "tp2", "wino4", "split", "wino2s", "tp2s", "stem7s", "k3s")
SPLIT_FAMILIES = frozenset(FAMILY_NAMES.index(n) for n in ("split", "wino2s", "tp2s", "stem7s", "k3s"))
# family numbers by name, for callers that name one family
FAMILY_WINO4, FAMILY_SPLIT, FAMILY_WINO2S, FAMILY_TP2S, FAMILY_STEM7S, FAMILY_K3S = (
    FAMILY_NAMES.index(n) for n in ("wino4", "split", "wino2s", "tp2s", "stem7s", "k3s"))


def config_ids(lib, family):
    """configuration ids of the kernel family named `family` (FAMILY_NAMES), in id order"""
    f = FAMILY_NAMES.index(family)
    return [i for i in range(lib.w2l_conv_num_tiles()) if lib.w2l_conv_config_family(i) == f]


# W2L_SPLIT=0 switches the split-operand families (fp32-accurate results on the bf16 matrix cores) off AND
# puts the tuned fp32-pipe entries back for the launches the committed table gives to that family (tune_table_nosplit.json), so
# that the switch is an A/B against the tuned fp32 kernels, not against the heuristic.
NO_SPLIT = os.environ.get("W2L_SPLIT", "1") == "0"
NOSPLIT_TABLE_PATH = os.path.join(_HERE, "tune_table_nosplit.json")


def load_tune_table(lib, path=None):
    """push the entries of a tune-table JSON file into the library; returns the number of entries loaded"""
    import json
    if path is None and NO_SPLIT and not EXACT and not os.environ.get("W2L_TUNE_TABLE"):
        return load_tune_table(lib, TUNE_TABLE_PATH) + load_tune_table(lib, NOSPLIT_TABLE_PATH)
    path = path or os.environ.get("W2L_TUNE_TABLE") or (EXACT_TABLE_PATH if EXACT else TUNE_TABLE_PATH)
    if path == "0" or not os.path.exists(path):
        return 0
    with open(path) as fh:
        doc = json.load(fh)
    nk = lib.w2l_tune_key_ints()
    if doc.get("key_ints") != nk or doc.get("num_configs", 0) > lib.w2l_conv_num_tiles():
        raise RuntimeError("tune table %s was written for another library build (key_ints %s / configs %s)"
                           % (path, doc.get("key_ints"), doc.get("num_configs")))
    n = 0
    for e in doc["entries"]:
        key = (C.c_int * nk)(*e[:nk])
        check_rc = lib.w2l_tune_set(key, int(e[nk]), int(e[nk + 1]))
        if check_rc != 0:
            raise RuntimeError("tune table %s: bad entry %s" % (path, e))
        n += 1
    return n


def export_tune_table(lib):
    """entries currently in the library's tune table as lists of ints (key..., tile, ksplit), sorted"""
    nk = lib.w2l_tune_key_ints()
    n = lib.w2l_tune_count()
    buf = (C.c_int * (max(n, 1) * (nk + 2)))()
    n = lib.w2l_tune_export(buf, n)
    return sorted([int(buf[i * (nk + 2) + j]) for j in range(nk + 2)] for i in range(n))


def save_tune_table(lib, path, note=""):
    import json
    nk = lib.w2l_tune_key_ints()
    for e in export_tune_table(lib):
        if not lib.w2l_tune_entry_applicable((C.c_int * nk)(*e[:nk]), e[nk]):
            raise RuntimeError("tune table entry %s names a configuration its shape cannot run" % e)
    doc = {"key_ints": lib.w2l_tune_key_ints(), "num_configs": lib.w2l_conv_num_tiles(),
           "key": "transposed cin cout kh kw sh sw ph pw oph opw precision has_residual head_c N H W -> config ksplit",
           "note": note, "entries": export_tune_table(lib)}
    with open(path, "w") as fh:
        fh.write(json.dumps(doc, indent=None, separators=(",", ":")).replace("],[", "],\n[") + "\n")
    return len(doc["entries"])


def load():
    """Load libw2l_hip.so (built in-tree by __graft_entry__.build() / `make -C wav2lip_amd/csrc`)."""
    global _lib
    if _lib is not None:
        return _lib
    import torch  # noqa: F401  -- torch's bundled HIP runtime (libamdhip64.so.7) must be the one this process binds:
    # the library shares streams and device pointers with torch, so both must sit on the same runtime instance
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            "wav2lip_amd: HIP library %s is missing; build it with `make -C wav2lip_amd/csrc` "
            "(there is no CPU fallback)" % LIB_PATH)
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    # W2L_EXACT=1: no F(4x4) Winograd.  W2L_SPLIT=0: no split-operand implicit GEMM (see NO_SPLIT above).
    mask = ((1 << FAMILY_WINO4) if EXACT else 0) | (sum(1 << f for f in SPLIT_FAMILIES) if NO_SPLIT else 0)
    if mask and lib.w2l_conv_exclude_families(mask) != 0:
        raise RuntimeError("wav2lip_amd: could not switch kernel families off (mask %d)" % mask)
    load_tune_table(lib)
    _lib = lib
    return lib


def check(rc, what=""):
    if rc != 0:
        msg = load().w2l_last_error()
        raise RuntimeError("libw2l_hip %s failed (%d): %s" % (what, rc, msg.decode() if msg else "?"))


def ptr(t):
    """device pointer of a torch tensor (or None)"""
    return None if t is None else C.c_void_p(t.data_ptr())


def current_stream():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)
