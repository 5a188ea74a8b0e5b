"""ctypes binding of libapse_hip.so (include/apse_hip.h).

PyTorch-ROCm is used only for device memory and streams: every call passes raw
``data_ptr()`` values and ``torch.cuda.current_stream().cuda_stream``.  There is
no CPU fallback: if the library is missing or no GPU is visible the product path
raises (the oracle under ``oracle/`` is test infrastructure and is never imported
from here).
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# APSE_HIP_LIB: another build of the same sources (A/B measurements of a compile-time switch, tools/gpu_ab.sh); the
# default is the in-tree library
_TREE_LIB = os.path.join(_HERE, "libapse_hip.so")
LIB_PATH = os.environ.get("APSE_HIP_LIB") or _TREE_LIB
# entries that only tools/ and the operator tests use: a build from before they existed may still be loaded through
# APSE_HIP_LIB (load())
TOOL_ENTRIES = ("apse_conv2d_ex", "apse_winograd_pack_filter", "apse_winograd_conv2d", "apse_winograd_conv2d_split", "apse_conv_pointwise_launches", "apse_lane_stats", "apse_rpn_select", "apse_box_inference",
                "apse_c4_rpn_select", "apse_rpn_select_train", "apse_rpn_train_proposals_workspace_bytes", "apse_rpn_train_proposals",
                "apse_set_rpn_head", "apse_roi_features_windows", "apse_set_crop_features", "apse_preprocess_frames_yuv", "apse_yuv_to_bgr", "apse_yuv_matrix_host", "apse_resize_normalize_yuv")

APSE_OK = 0


class ApseError(RuntimeError):
    pass


class Config(C.Structure):
    _fields_ = [
        ("struct_size", C.c_int), ("device", C.c_int), ("max_batch", C.c_int),
        ("frame_h", C.c_int), ("frame_w", C.c_int), ("image_h", C.c_int), ("image_w", C.c_int),
        ("blocks", C.c_int * 4), ("num_classes", C.c_int),
        ("score_thresh", C.c_float), ("box_nms", C.c_float), ("rpn_nms", C.c_float), ("mask_thresh", C.c_float),
        ("rpn_pre_topk", C.c_int), ("rpn_post_topk", C.c_int), ("dets_per_image", C.c_int),
        ("pixel_mean", C.c_float * 3), ("assoc_roi", C.c_int), ("embed_dim", C.c_int), ("assoc_scale", C.c_float),
        ("compute_dtype", C.c_int), ("storage16", C.c_int),
    ]


class ConfigArch(Config):
    """apse_config with the appended ``arch`` field (0 FPN, 1 C4).  ``Config`` keeps the earlier layout: a caller that passes its
    size gets FPN."""
    _fields_ = [("arch", C.c_int)]


class ConfigLane(ConfigArch):
    """apse_config with the appended ``tail_lane`` field (0 default = on, < 0 off)."""
    _fields_ = [("tail_lane", C.c_int)]


class ResultsLayout(C.Structure):
    _fields_ = [("bytes", C.c_size_t), ("n_max", C.c_int), ("dets_per_image", C.c_int), ("embed_dim", C.c_int),
                ("max_batch", C.c_int)] + [(k, C.c_size_t) for k in (
                    "total", "offset", "prop_count", "img", "cls", "roi", "score", "box_resized", "box", "valid", "rect",
                    "mass", "centroid", "closest", "embedding")]


class RenderItem(C.Structure):
    """apse_render_item (include/apse_hip.h)."""
    _fields_ = [("image", C.c_int), ("rect", C.c_int * 4), ("words_per_row", C.c_int), ("bits", C.c_void_p),
                ("box", C.c_float * 4), ("rgb", C.c_uint8 * 4), ("label_off", C.c_int), ("label_len", C.c_int)]


class MotsWindow(C.Structure):
    """apse_mots_window (include/apse_hip.h)."""
    _fields_ = [("rect", C.c_int * 4), ("words_per_row", C.c_int), ("area", C.c_int), ("bits", C.c_void_p)]


class MotsObject(C.Structure):
    """apse_mots_object (include/apse_hip.h)."""
    _fields_ = [("rect", C.c_int * 4), ("words_per_row", C.c_int), ("score", C.c_float), ("bits", C.c_void_p)]


class ConvDesc(C.Structure):
    _fields_ = [(k, C.c_int) for k in ("B", "H", "W", "Cin", "Cout", "KH", "KW", "stride", "pad", "relu", "res_mode",
                                       "cfg", "splitk", "prec", "fuse_reduce", "x_st", "res_st", "y_st")]


vp, i, f, sz = C.c_void_p, C.c_int, C.c_float, C.c_size_t
# every entry of include/apse_hip.h: name -> (argtypes, restype)
SIGNATURES = {
    "apse_create": ([C.POINTER(Config), C.POINTER(vp)], i),
    "apse_destroy": ([vp], None),
    "apse_last_error": ([vp], C.c_char_p),
    "apse_version": ([], C.c_char_p),
    "apse_set_weight": ([vp, C.c_char_p, vp, C.POINTER(C.c_int64), i], i),
    "apse_finalize_weights": ([vp], i),
    "apse_set_resize_tables": ([vp, vp, vp, i, vp, vp, i], i),
    "apse_set_camera": ([vp, C.POINTER(C.c_double), C.POINTER(C.c_double), i, vp, i, i], i),
    "apse_preprocess_frames": ([vp, vp, i, vp], i),
    "apse_preprocess_images": ([vp, vp, i, vp], i),
    "apse_backbone": ([vp, i, vp], i),
    "apse_rpn": ([vp, i, vp], i),
    "apse_rpn_levels": ([vp, i, i, vp], i),
    "apse_box_head": ([vp, i, vp], i),
    "apse_set_detections": ([vp, vp, vp, vp, vp, i, vp], i),
    "apse_mask_tail": ([vp, i, vp], i),
    "apse_embed": ([vp, i, vp], i),
    "apse_forward": ([vp, i, vp], i),
    "apse_results_describe": ([vp, C.POINTER(ResultsLayout)], i),
    "apse_read_results": ([vp, vp, sz, vp], i),
    "apse_read_results_begin": ([vp, vp, sz, vp], i),
    "apse_read_results_end": ([vp, vp], i),
    "apse_lane_stats": ([vp, C.POINTER(C.c_longlong * 4)], i),
    "apse_copy_mask_window": ([vp, i, i, i, i, i, vp, vp], i),
    "apse_copy_mask_windows": ([vp, i, vp, vp, vp, vp, vp], i),
    "apse_host_copy": ([vp, vp, sz, i], i),
    "apse_feature_shape": ([vp, C.c_char_p, C.POINTER(C.c_int * 3)], i),
    "apse_export_feature": ([vp, C.c_char_p, vp, i, vp], i),
    "apse_debug_tensor": ([vp, C.c_char_p, vp, sz, C.POINTER(sz), vp], i),
    "apse_flops": ([vp, i, C.c_double, C.c_double], C.c_double),
    "apse_profile": ([vp, i], i),
    "apse_profile_read": ([vp, C.POINTER(C.c_double * 42), i], i),
    "apse_conv_packed_elems": ([C.POINTER(ConvDesc)], sz),
    "apse_conv_pack_weight": ([C.POINTER(ConvDesc), vp, i, vp, vp], i),
    "apse_conv2d": ([C.POINTER(ConvDesc), vp, vp, vp, vp, vp, vp, sz, vp], i),
    "apse_conv2d_ex": ([C.POINTER(ConvDesc), vp, vp, vp, vp, vp, vp, sz, vp, i, i, i, vp], i),
    "apse_winograd_pack_filter": ([vp, i, i, vp], i),
    "apse_winograd_conv2d": ([C.POINTER(ConvDesc), vp, vp, vp, vp, vp], i),
    "apse_winograd_conv2d_split": ([C.POINTER(ConvDesc), vp, vp, vp, vp, vp, C.c_size_t, i, vp], i),
    "apse_conv_pointwise_launches": ([], C.c_uint),
    "apse_maxpool3x3s2": ([vp, vp, i, i, i, i, vp], i),
    "apse_maxpool3x3s2_typed": ([vp, vp, i, i, i, i, i, vp], i),
    "apse_roi_align": ([C.POINTER(vp), C.POINTER(i), C.POINTER(i), vp, i, i, i, vp, vp], i),
    "apse_roi_align_typed": ([C.POINTER(vp), C.POINTER(i), C.POINTER(i), vp, i, i, i, i, vp, vp], i),
    "apse_roi_pool": ([vp, i, i, vp, vp, i, i, f, vp, vp], i),
    "apse_roi_features": ([vp, i, vp, vp, i, i, vp, vp], i),
    "apse_roi_features_windows": ([vp, i, vp, vp, i, i, vp, vp], i),
    "apse_set_crop_features": ([vp, i], i),
    "apse_nms_rank": ([vp, vp, vp, i, i, i, i, f, i, vp, vp, vp, vp, vp], i),
    "apse_rpn_select": ([C.POINTER(vp), C.POINTER(i), C.POINTER(i), i, i, i, i, i, i, f, i, vp, vp, vp, vp, vp, vp, vp, vp, vp], i),
    "apse_box_inference": ([vp, i, i, vp, vp, i, i, i, i, f, f, i, i] + [vp] * 16, i),
    "apse_c4_rpn_select": ([vp, i, i, i, i, i, i, i, f, vp, vp, vp, vp, vp, vp, vp, vp], i),
    "apse_mask_centroid_dense": ([vp, i, i, C.POINTER(C.c_int * 3), vp], i),
    "apse_mask_closest_dense": ([vp, i, i, f, f, C.POINTER(C.c_int * 2), vp], i),
    "apse_l2_normalize": ([vp, vp, i, i, vp], i),
    "apse_sqdist": ([vp, vp, i, i, i, vp, vp], i),
    "apse_undistort_gamma": ([vp, vp, i, i, i, C.POINTER(C.c_double), C.POINTER(C.c_double), i, vp, i, i, vp], i),
    "apse_lab_tables_host": ([vp, vp, C.c_size_t], C.c_size_t),
    "apse_replay_create": ([i, i, f, i], vp),
    "apse_replay_destroy": ([vp], None),
    "apse_replay_step": ([vp, i, i, vp, vp, vp, C.c_char_p, i, vp], i),
    "apse_replay_packed": ([vp, vp, C.c_longlong, i, i, i, vp, C.c_longlong], C.c_longlong),
    "apse_replay_max_id": ([vp], i),
    "apse_replay_next_id": ([vp], i),
    "apse_render_workspace_bytes": ([i, i, i], sz),
    "apse_render_instances": ([vp, vp, i, i, i, i, vp, i, vp, sz, vp, i, vp, sz, vp], i),
    "apse_render_pack_mask": ([vp, i, i, vp, vp], i),
    "apse_render_font_host": ([vp, sz], sz),
    "apse_mots_split_workspace_bytes": ([], sz),
    "apse_mots_split_idmap": ([vp, i, i, i, vp, sz, vp, vp, vp, vp, sz, vp], i),
    "apse_mots_rle_to_bits": ([vp, vp, i, i, i, vp, vp], i),
    "apse_mots_overlaps": ([vp, i, vp, i, vp, i, vp, vp], i),
    "apse_mots_shift_overlaps": ([vp, i, vp, i, i, i, vp, vp], i),
    "apse_mots_render_idmap": ([vp, vp, i, i, i, vp, vp], i),
    "apse_mots_crop_overlaps": ([vp, vp, i, i, i, vp, sz, vp, vp, vp], i),
    "apse_mots_rle_workspace_bytes": ([vp, i, i, i], sz),
    "apse_mots_bits_to_rle": ([vp, vp, i, i, i, vp, i, vp, vp, vp, sz, vp], i),
    "apse_mots_rle_pack_workspace_bytes": ([i], sz),
    "apse_mots_rle_pack": ([vp, vp, i, i, vp, i, vp, vp, vp, sz, vp], i),
    "apse_resize_normalize": ([vp, vp, vp, vp, vp, vp, i, vp, vp, i, i, i, i, i, i, i, i, C.POINTER(f * 3), vp], i),
    "apse_assoc_fc_workspace_bytes": ([i, i, i], sz),
    "apse_assoc_fc_forward": ([vp, vp, vp, i, i, i, vp, vp, vp, sz, vp], i),
    "apse_assoc_fc_backward": ([vp, vp, vp, vp, i, i, i, vp, vp, vp, sz, vp], i),
    "apse_triplet_workspace_bytes": ([i], sz),
    "apse_triplet_hard_forward": ([vp, vp, i, i, f, i, vp, vp, sz, vp], i),
    "apse_triplet_all_forward": ([vp, vp, i, i, f, i, vp, vp, sz, vp], i),
    "apse_triplet_hard_backward": ([vp, i, i, i, vp, vp, vp, vp], i),
    "apse_triplet_all_backward": ([vp, i, i, i, vp, vp, vp, vp], i),
    "apse_sgd_step": ([vp, vp, vp, C.c_longlong, f, f, f, f, i, i, vp], i),
    "apse_coco_box_iou": ([vp, vp, vp, i, i, i, vp, vp, vp, vp, vp], i),
    "apse_coco_poly_to_bits": ([vp, vp, i, vp, i, vp, vp, vp, i, vp, vp, vp, vp], i),
    "apse_coco_match": ([vp, vp, vp, i, i, i, vp, vp, vp, i, vp, vp, vp, i, vp, i, vp, i, vp, vp, vp, vp, vp], i),
    "apse_coco_accumulate_workspace_bytes": ([C.c_longlong], sz),
    "apse_coco_sort_lists": ([vp, vp, i, vp, C.c_longlong, i, vp, vp, sz, vp], i),
    "apse_coco_accumulate": ([vp, vp, vp, i, vp, i, vp, vp, vp, C.c_longlong, i, vp, i, i, i, i, i, vp, vp, vp, vp, sz,
                              vp], i),
    "apse_mask_roi_features": ([vp, i, vp, i, vp, vp], i),
    "apse_mask_train_workspace_bytes": ([i, i], sz),
    "apse_mask_pack_elems": ([i, i, i, i], sz),
    "apse_mask_pack_weight": ([vp, vp, i, i, i, i, i, vp, vp, vp], i),
    "apse_mask_conv_forward": ([vp, vp, vp, i, i, i, i, i, i, i, i, i, i, i, vp, vp, sz, vp], i),
    "apse_mask_conv3x3": ([vp, vp, vp, i, i, vp, vp], i),
    "apse_mask_relu_grad": ([vp, vp, C.c_longlong, vp, vp], i),
    "apse_mask_bias_grad": ([vp, C.c_longlong, vp, vp, sz, vp], i),
    "apse_mask_wgrad": ([vp, vp, i, i, vp, vp, sz, vp], i),
    "apse_mask_loss_forward": ([vp, i, vp, vp, i, vp, vp, sz, vp], i),
    "apse_mask_loss_backward": ([vp, i, vp, vp, i, vp, vp, vp], i),
    "apse_mask_predictor_backward": ([vp, vp, vp, vp, i, i, vp, vp, vp, vp, sz, vp], i),
    "apse_coco_mask_targets": ([vp, vp, i, vp, i, i, vp, vp, i, i, vp, vp, vp], i),
    "apse_mots_remap_windows": ([vp, i, i, i, vp, vp, i, i, vp, vp, vp], i),
    "apse_bitmask_targets": ([vp, i, i, i, vp, vp, i, i, vp, vp], i),
    "apse_box_roi_features": ([vp, i, vp, i, vp, vp], i),
    "apse_proposals": ([vp, i, vp, vp, vp], i),
    "apse_box_train_workspace_bytes": ([i, i], sz),
    "apse_box_match": ([vp, i, vp, vp, i, i, f, vp, vp, vp, vp], i),
    "apse_box_permute_features": ([vp, i, vp, vp], i),
    "apse_box_fc_forward": ([vp, vp, vp, i, i, i, i, vp, vp, sz, vp], i),
    "apse_box_fc_dgrad": ([vp, vp, i, i, i, i, vp, vp], i),
    "apse_box_fc_wgrad": ([vp, vp, i, i, i, vp, vp], i),
    "apse_box_bias_grad": ([vp, i, i, vp, vp, sz, vp], i),
    "apse_box_loss_forward": ([vp, vp, vp, vp, vp, i, i, C.POINTER(f * 4), f, vp, vp, sz, vp], i),
    "apse_box_loss_backward": ([vp, vp, vp, vp, vp, i, i, C.POINTER(f * 4), f, vp, vp, vp, vp, vp], i),
    "apse_rpn_train_workspace_bytes": ([i, i, i], sz),
    "apse_rpn_anchor_labels": ([C.POINTER(i * 5), C.POINTER(i * 5), vp, i, f, f, vp, vp, vp, vp, sz, vp], i),
    "apse_rpn_patches": ([vp, i, vp, i, vp, vp, vp, vp, vp], i),
    "apse_rpn_loss_forward": ([vp, vp, vp, vp, vp, vp, i, i, f, vp, vp, sz, vp], i),
    "apse_rpn_loss_backward": ([vp, vp, vp, vp, vp, vp, i, i, f, vp, vp, vp, vp, vp], i),
    "apse_augment_u8": ([vp, i, i, i, vp, vp, vp, vp, vp], i),
    "apse_rpn_select_train": ([C.POINTER(vp), C.POINTER(i), C.POINTER(i), i, i, i, i, i, i, f, i, vp, vp, vp, vp, vp, vp, vp, vp, vp], i),
    "apse_rpn_train_proposals_workspace_bytes": ([i, i], sz),
    "apse_rpn_train_proposals": ([vp, i, i, i, vp, vp, vp, vp, sz, vp], i),
    "apse_set_rpn_head": ([vp, vp, vp, vp, vp, vp, vp, vp], i),
    "apse_preprocess_frames_yuv": ([vp, vp, i, i, i, i, vp], i),
    "apse_yuv_to_bgr": ([vp, vp, i, i, i, i, i, i, vp], i),
    "apse_yuv_matrix_host": ([i, C.POINTER(C.c_int * 6)], i),
    "apse_resize_normalize_yuv": ([vp, i, i, i, vp, vp, vp, vp, vp, i, vp, vp, i, i, i, i, i, i, i, i, C.POINTER(f * 3), vp], i),
}
del vp, i, f, sz
EXPORTS = list(SIGNATURES)


_lib = None


def load():
    """Loads the shared library (raises ApseError when it has not been built)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ApseError("libapse_hip.so not found at %s: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                        "or `make -C apse_uav_amd/csrc` (there is no CPU fallback)" % LIB_PATH)
    # One HIP runtime per process: PyTorch-ROCm ships its own libamdhip64 and the library links the system one.  Whichever is
    # loaded first serves both, and with the system copy first the library found no device on the GPU box once torch had come up
    # on its own copy afterwards (build() followed by smoke() in one process).  torch first, always.
    import torch  # noqa: F401
    lib = C.CDLL(LIB_PATH)
    for name, (args, ret) in SIGNATURES.items():
        if name in TOOL_ENTRIES and LIB_PATH != _TREE_LIB and not hasattr(lib, name):
            continue                       # an older build loaded through APSE_HIP_LIB for an A/B run
        fn = getattr(lib, name)            # AttributeError here = ABI drift between header and library
        fn.argtypes = args
        fn.restype = ret
    _lib = lib
    return lib


def stream_ptr():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def check(rc, ctx=None, what=""):
    if rc != APSE_OK:
        msg = load().apse_last_error(ctx).decode() if ctx is not None else ""
        raise ApseError("%s failed (code %d) %s" % (what, rc, msg))


def ptr(t):
    """Device (or host) pointer of a contiguous torch tensor / numpy array, or NULL."""
    if t is None:
        return C.c_void_p(0)
    if isinstance(t, np.ndarray):
        assert t.flags["C_CONTIGUOUS"]
        return C.c_void_p(t.ctypes.data)
    assert t.is_contiguous()
    return C.c_void_p(t.data_ptr())
