"""ctypes binding of libupsnet_hip.so (the C ABI declared in include/upsnet_hip.h).

The HIP library IS the product: there is no CPU / eager fallback. If the shared library is missing
(or a kernel launch fails) the ops raise RuntimeError.
"""
import ctypes
import os
import threading

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("UPSNET_LIB_PATH") or os.path.join(_HERE, "csrc", "libupsnet_hip.so")   # (the override: same-box A/B of two builds)

c_int, c_float, c_double, c_void_p, c_size_t, c_long = ctypes.c_int, ctypes.c_float, ctypes.c_double, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_long
P = c_void_p

_SIGNATURES = {
    "upsnet_last_error": (ctypes.c_char_p, []),
    "upsnet_last_kernel_form": (ctypes.c_char_p, []),
    "upsnet_abi_version": (c_int, []),
    "upsnet_zero_fill": (c_int, [P, P, c_size_t]),
    "upsnet_roi_align_forward": (c_int, [P, P, c_float, c_int, c_int, c_int, c_int, c_int, c_int, c_int, P, P]),
    "upsnet_roi_align_forward_nhwc": (c_int, [P, P, c_int, c_int, c_int, c_int, c_float, P, c_int, c_int, c_int, c_int, P]),
    "upsnet_fpn_roi_align_forward": (c_int, [P, P, P, P, P, c_int, P, c_int, P, c_int, c_int, c_int, P, P]),
    "upsnet_fpn_roi_order": (c_int, [P, P, c_int, P, c_int, c_int, P]),
    "upsnet_fpn_roi_align_forward_ordered": (c_int, [P, P, P, P, P, c_int, P, c_int, P, c_int, c_int, c_int, P, P, P]),
    "upsnet_roi_tuning": (None, [c_int]),
    "upsnet_roi_geometry": (None, [c_int, c_int]),
    "upsnet_deform_im2col": (c_int, [P, P, P] + [c_int] * 13 + [P]),
    "upsnet_mod_deform_im2col": (c_int, [P, P, P, P] + [c_int] * 15 + [P]),
    "upsnet_roi_align_backward": (c_int, [P, P, c_float] + [c_int] * 8 + [P, P]),
    "upsnet_deform_col2im": (c_int, [P, P, P] + [c_int] * 13 + [P]),
    "upsnet_deform_col2im_coord": (c_int, [P, P, P, P] + [c_int] * 13 + [P]),
    "upsnet_mod_deform_col2im": (c_int, [P, P, P, P] + [c_int] * 15 + [P]),
    "upsnet_mod_deform_col2im_coord": (c_int, [P, P, P, P, P] + [c_int] * 15 + [P, P]),
    "upsnet_deform_conv_forward_nhwc": (c_int, [P, c_int, P, P, P, P, P, P] + [c_int] * 11 + [P, c_int, P, c_int]),
    "upsnet_dcn_packed_weight_floats": (c_size_t, [c_int, c_int, c_int, c_int]),
    "upsnet_dcn_pack_weight": (c_int, [P, P, c_int, c_int, c_int, c_int, P]),
    "upsnet_deform_conv_fused_nhwc": (c_int, [P, c_int, P, P, P, P, P, P] + [c_int] * 7 + [P, P, c_int]),
    "upsnet_deform_conv_fused_splitk_workspace_bytes": (c_size_t, [c_int] * 9),
    "upsnet_deform_conv_fused_nhwc_splitk": (c_int, [P, P, P, P, P] + [c_int] * 9 + [P, P, c_int, c_int, P]),
    "upsnet_dcn_tuning": (None, [c_int]),
    "upsnet_dcn_packed_weight_bf16_elems": (c_size_t, [c_int, c_int, c_int, c_int]),
    "upsnet_dcn_pack_weight_bf16": (c_int, [P, P, c_int, c_int, c_int, c_int, P]),
    "upsnet_deform_conv_fused_nhwc_bf16": (c_int, [P, c_int, P, P, P, P, P, P] + [c_int] * 7 + [P, P, c_int]),
    "upsnet_conv1x1_frag_nhwc_f32": (c_int, [P, P, P, P, c_int, c_int, c_int, c_int, P, P, c_int, c_int, c_int, c_int]),
    "upsnet_conv1x1_tuning": (None, [c_int]),
    "upsnet_conv1x1_siblings_nhwc_f32": (c_int, [P, P, P, P, c_int, c_int, c_int, c_int, P, P, c_int, c_int, c_int, c_int, c_int]),
    "upsnet_conv1x1_pair32_tuning": (None, [c_int]),
    "upsnet_residency_tuning": (c_int, [c_int, c_int]),
    "upsnet_residency_pad_bytes": (c_size_t, [c_int, c_size_t, c_size_t]),
    "upsnet_residency_last_dynamic_lds": (c_int, []),
    "upsnet_conv1x1_splitk_workspace_bytes": (ctypes.c_size_t, [c_int, c_int, c_int, c_int, c_int]),
    "upsnet_conv1x1_frag_nhwc_f32_splitk": (c_int, [P, P, P, P, c_int, c_int, c_int, c_int, P, P, c_int, c_int, c_int, c_int, P]),
    "upsnet_conv1x1_ksw_packed_weight_floats": (ctypes.c_size_t, [c_int, c_int]),
    "upsnet_conv1x1_ksw_pack_weight": (c_int, [P, P, c_int, c_int, P]),
    "upsnet_conv1x1_ksw_nhwc_f32": (c_int, [P, P, P, P, c_int, c_int, c_int, c_int, P, P, c_int, c_int, c_int, c_int, c_int, c_int]),
    "upsnet_conv1x1_ksw_tuning": (None, [c_int]),
    "upsnet_conv3x3_ksw_packed_weight_floats": (ctypes.c_size_t, [c_int]),
    "upsnet_conv3x3_ksw_pack_weight": (c_int, [P, P, c_int, c_int, P]),
    "upsnet_conv3x3_ksw_nhwc_f32": (c_int, [P, P, P, c_int, c_int, c_int, c_int, P, P, c_int, c_int]),
    "upsnet_conv2d_winograd36_splitk_workspace_bytes": (ctypes.c_size_t, [c_int, c_int, c_int, c_int, c_int]),
    "upsnet_conv2d_winograd36_nhwc_f32_splitk": (c_int, [P, P, P, c_int, c_int, c_int, c_int, P, c_int, P, c_int, c_int, c_int, P]),
    "upsnet_conv1x1_pair_nhwc_f32": (c_int, [P, P, P, P, P, c_long, c_int, P, P, c_int, P, P, c_int]),
    "upsnet_conv2d_nhwc_f32": (c_int, [P, c_int, P, P, P, P, P, P, c_int, P, c_int, P, c_int, c_int, c_int, c_int, c_int, c_int, c_int]),
    "upsnet_conv2d_nhwc_f32_multiw": (c_int, [P, c_int, P, P, P, P, P, c_int, P, c_int, c_int, c_int, c_int, c_int, c_int, c_int]),
    "upsnet_conv_tuning": (None, [c_int, c_int]),
    "upsnet_conv_pack_weight": (c_int, [P, P, c_int, c_int, c_int, c_int, c_int, P]),
    "upsnet_nms_host": (c_int, [P, P, P, c_int, c_int, c_float, c_int]),
    "upsnet_nms_workspace_bytes": (c_size_t, [c_int, c_int]),
    "upsnet_nms_batched": (c_int, [P, P, P, P, P, c_int, c_int, c_float, P, P, P]),
    "upsnet_nms_tuning": (None, [c_int]),
    "upsnet_cpu_nms_batched": (c_int, [P, P, P, P, c_int, c_int, c_double, P, P, P]),
    "upsnet_soft_nms_batched_workspace_bytes": (c_size_t, [c_int, c_int]),
    "upsnet_soft_nms_batched": (c_int, [P, P, P, P, c_int, c_int, c_float, c_float, c_float, c_int, P, P]),
    "upsnet_soft_nms_workspace_bytes": (c_size_t, [c_int]),
    "upsnet_soft_nms": (c_int, [P, P, P, c_int, c_float, c_float, c_float, c_int, P, P]),
    "upsnet_proposal_workspace_bytes": (c_size_t, [c_int, P, P, c_int, c_int, c_int]),
    "upsnet_pyramid_proposals_strided": (c_int, [P, c_int, P, P, P, P, P, P, P, P, P, P, c_int, P, c_int, c_int, c_float, c_float, P, P, P, P]),
    "upsnet_pyramid_proposals_strided_ordered": (c_int, [P, c_int, P, P, P, P, P, P, P, P, P, P, c_int, P, c_int, c_int, c_float, c_float, P, P, P, P, P]),
    "upsnet_pyramid_proposals_joint_strided": (c_int, [P, c_int, P, P, P, P, P, P, P, P, P, P, c_int, P, c_int, c_int, c_float, c_float, P, P, P, P]),
    "upsnet_pyramid_proposals": (c_int, [P, c_int, P, P, P, P, P, P, c_int, P, c_int, c_int, c_float, c_float, P, P, P, P]),
    "upsnet_mask_roi_capacity": (c_int, [c_int, c_int, c_int]),
    "upsnet_mask_roi_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "upsnet_mask_roi": (c_int, [P, P, P, P, c_int, P, c_int, P, c_int, c_float, c_float, c_int, P, P, P, P, P, P, P]),
    "upsnet_mask_roi_ex": (c_int, [P, P, P, P, c_int, P, c_int, P, c_int, c_int, c_float, c_float, c_int, P, P, P, P, P, P, P]),
    "upsnet_mask_logit_gather": (c_int, [P, P, c_int, c_int, c_int, c_long, c_long, c_long, P, P, c_int, P]),
    "upsnet_mask_removal_workspace_bytes": (c_size_t, [c_int, c_int, c_int, c_int]),
    "upsnet_mask_removal": (c_int, [P, P, P, P, P, c_int, P, c_int, c_int, c_int, c_int, c_double, P, P, P, P]),
    "upsnet_panoptic_tail_pack": (c_int, [P, P, P, c_int, P, P, P, P, P, P, P, P]),
    "upsnet_mask_paste": (c_int, [P, P, P, P, P, P, c_int, c_int, c_int, c_int, P]),
    "upsnet_seg_term": (c_int, [P, P, c_int, c_int, c_int, P, P, P, c_int, P]),
    "upsnet_panoptic_fuse": (c_int, [P, P, c_int, c_int, c_int, c_int, P, P, P, P, P, P, c_int, c_int, P, c_int, P, P]),
    "upsnet_panoptic_fuse_up": (c_int, [P, P, c_int, c_int, c_int, c_int, c_int, c_int, P, P, P, P, P, P, c_int, c_int, P, P, P]),
    "upsnet_panoptic_fuse_up_conf": (c_int, [P, P, c_int, c_int, c_int, c_int, c_int, c_int, P, P, P, P, P, P, c_int, c_int, P, P, P, P]),
    "upsnet_conv2d_stem_nhwc4_f32": (c_int, [P, P, c_int, c_int, c_int, P, c_int, P, c_int, c_int, c_int, c_int, c_int, c_int, P]),
    "upsnet_conv_pack_weight_stem": (c_int, [P, P, c_int, c_int, c_int, c_int, c_int, P]),
    "upsnet_deconv2x2_nhwc_f32": (c_int, [P, P, c_int, c_int, c_int, c_int, P, c_int, P, c_int, c_int, P]),
    "upsnet_deconv2x2_pack_weight": (c_int, [P, P, c_int, c_int, c_int, P]),
    "upsnet_deconv2x2_frag_nhwc_f32": (c_int, [P, P, P, c_int, c_int, c_int, c_int, P, P, c_int, c_int]),
    "upsnet_prep_image_u8": (c_int, [P, P, c_int, c_int, P, c_double, c_int, c_int, c_int, c_int, c_int, P]),
    "upsnet_image_to_nhwc4": (c_int, [P, P, c_int, c_int, c_int, c_int, P]),
    "upsnet_unified_pan_workspace_bytes": (c_size_t, []),
    "upsnet_unified_pan_result": (c_int, [P, P, P, P, c_int, c_int, c_int, c_int, c_int, c_int, P, P]),
    "upsnet_combined_pan_workspace_bytes": (c_size_t, [c_int, c_long]),
    "upsnet_combined_pan_result": (c_int, [P, c_int, P, c_int, c_int, c_long, P, P, c_int, c_int, c_int, c_double, P]),
    "upsnet_mask_roi_dedup": (c_int, [P, P, P, P, c_int, P, P, P, P, c_int, P, P, P]),
    "upsnet_conv2d_winograd_nhwc_f32": (c_int, [P, c_int, P, P, P, P, P, P, c_int, P, c_int, P, c_int, c_int]),
    "upsnet_conv2d_winograd_nhwc_f32_splitk": (c_int, [P, P, P, P, c_int, c_int, c_int, c_int, P, c_int, P, c_int, c_int, c_int, P]),
    "upsnet_conv_pack_weight_winograd": (c_int, [P, P, c_int, c_int, c_int, P]),
    "upsnet_conv_pack_weight_winograd_tn32": (c_int, [P, P, c_int, c_int, c_int, P]),
    "upsnet_conv2d_winograd_nhwc_f32_tn32": (c_int, [P, c_int, P, P, P, P, P, P, c_int, P, c_int, P, c_int, c_int]),
    "upsnet_conv2d_winograd_nhwc_f32_tail": (c_int, [P, P, P, c_int, c_int, c_int, c_int, c_int, P, c_int, P, c_int, P, c_int, c_int]),
    "upsnet_conv2d_winograd36_nhwc_f32": (c_int, [P, c_int, P, P, P, P, P, c_int, P, c_int, P, c_int, c_int]),
    "upsnet_conv_pack_weight_winograd36": (c_int, [P, P, c_int, c_int, c_int, P]),
    "upsnet_conv2d_nhwc_bf16": (c_int, [P, c_int, P, P, P, P, P, P, c_int, P, P, c_int, P, c_int, c_int, c_int, c_int, c_int, c_int]),
    "upsnet_bottleneck_proj_bf16": (c_int, [P, P, P, c_int, c_int, c_int, c_int, c_int, c_int, P, P, P, P, P, P]),
    "upsnet_conv_bf16_tuning": (c_int, [c_int, c_int]),
    "upsnet_conv1x1_bf16_tuning": (c_int, [c_int]),
    "upsnet_stem_pool_pack_weight_f32": (c_int, [P, P, c_int, P]),
    "upsnet_stem_pool_f32": (c_int, [P, P, c_int, c_int, c_int, P, P, P]),
    "upsnet_stem_pool_pack_weight_bf16": (c_int, [P, P, c_int, P]),
    "upsnet_stem_pool_bf16": (c_int, [P, P, c_int, c_int, c_int, P, P, P]),
    "upsnet_deconv2x2_nhwc_bf16": (c_int, [P, P, c_int, c_int, c_int, c_int, P, c_int, P, c_int, c_int, P, c_int]),
    "upsnet_bottleneck_bf16": (c_int, [P, P, P, c_int, c_int, c_int, c_int, P, P, P, P, P, P]),
    "upsnet_conv_pack_weight_bf16": (c_int, [P, P, c_int, c_int, c_int, c_int, c_int, P, P]),
    "upsnet_conv2d_splitk_workspace_bytes": (c_size_t, [c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int]),
    "upsnet_conv2d_nhwc_f32_splitk": (c_int, [P, P, P, P, c_int, c_int, c_int, c_int, P, c_int, P, c_int, c_int, c_int, c_int, c_int, c_int, c_int, P]),
    "upsnet_im_post_rle": (c_int, [P, P, P, P, c_int, c_int, c_int, c_int, c_int, c_int, P, P]),
    "upsnet_fcn_score_combine": (c_int, [P, c_int, P, c_int, c_int, c_int, P, P]),
    "upsnet_panoptic_argmax": (c_int, [P, P, c_int, c_int, c_int, c_int, P, P, c_int, c_int, P]),
    "upsnet_pq_workspace_bytes": (c_size_t, [c_int]),
    "upsnet_pq_accumulate": (c_int, [P, P, P, c_int, c_int, P, c_int, P, c_int, c_int, P, P, P, P, P, P]),
    "upsnet_pan_boundary_workspace_bytes": (c_size_t, [c_int, c_int]),
    "upsnet_pan_boundary_map": (c_int, [P, c_int, P, P, c_int, c_int, P, P]),
    "upsnet_pq_boundary_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "upsnet_pq_boundary_accumulate": (c_int, [P, c_int, P, P, c_int, c_int, P, c_int, P, c_int, c_int, P, P, P, P, P, P]),
    "upsnet_restore_label_maps": (c_int, [P, P, P, c_long, c_int, c_int, P, c_int, P, c_int, P, P]),
    "upsnet_restore_plane_u8": (c_int, [P, P, c_long, c_int, c_int, P, c_int, P, c_int, P]),
    "upsnet_confusion_accumulate": (c_int, [P, P, P, c_long, c_int, c_int, P]),
    "upsnet_det_eval_image_workspace_bytes": (c_size_t, [c_int] * 6),
    "upsnet_det_eval_image": (c_int, [P, c_int, c_int, c_int, c_int, c_int, P, P, P, P, c_int, P, P, c_int, c_int, P, P, c_int, P, P, P, P,
                                      P, P, P, c_int, P, P, c_int, P, c_int, P, c_int, P, P, P, P, P, P, P]),
    "upsnet_det_eval_accumulate_workspace_bytes": (c_size_t, [c_long, c_int]),
    "upsnet_det_eval_accumulate": (c_int, [P, c_long, P, P, P, P, P, P, c_int, P, P, P, P, P, P]),
    "upsnet_det_eval_boundary_image_workspace_bytes": (c_size_t, [c_int] * 5),
    "upsnet_det_eval_boundary_image": (c_int, [P, c_int, c_int, c_int, c_int, c_int, P, P, P, c_int, P, P, c_int, c_int, P, P, c_int, P, P, P,
                                               P, P, P, c_int, P, P, c_int, P, c_int, P, c_int, P, P, P, P, P, P, P]),
    "upsnet_boundary_dilation_fits": (c_int, [c_int, c_int, c_int]),
    "upsnet_boundary_masks_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "upsnet_boundary_masks": (c_int, [P, c_int, c_int, c_int, c_int, P, P, P, P, P, P]),
    "upsnet_poly_raster_workspace_bytes": (c_size_t, [c_long, c_long]),
    "upsnet_poly_raster": (c_int, [P, P, P, P, P, P, c_int, c_int, c_long, c_int, c_int, P, P, P]),
    "upsnet_proposal_recall_workspace_bytes": (c_size_t, [c_int, c_long]),
    "upsnet_proposal_recall": (c_int, [P, c_int, P, P, P, c_int, c_long, P, P]),
    "upsnet_cs_inst_counts_ints": (c_size_t, [c_int]),
    "upsnet_cs_inst_workspace_bytes": (c_size_t, [c_int]),
    "upsnet_cs_inst_state_words": (c_int, []),
    "upsnet_cs_inst_image": (c_int, [P, P, c_int, c_int, c_int, P, P, P, P, P, c_int, P, P, c_int, P, P, P, P, P, P]),
    "upsnet_cs_pixel_inst_ints": (c_size_t, []),
    "upsnet_cs_pixel_image": (c_int, [P, P, P, P, P, c_int, c_int, P, P, P, P, P]),
    "upsnet_pan_format_workspace_bytes": (c_size_t, []),
    "upsnet_pan_format_table_ints": (c_size_t, []),
    "upsnet_pan_format": (c_int, [P, P, c_int, c_int, P, P, P, P]),
    "upsnet_pan_relabel": (c_int, [P, P, c_int, c_int, P, c_int, c_int, P, P, P]),
    "upsnet_gt_prepare_workspace_bytes": (c_size_t, [c_int]),
    "upsnet_gt_prepare": (c_int, [P, P, P, c_int, c_int, P, P, P, c_int, c_int, P, P, P, P, P, P, P]),
    "upsnet_vis_max_detections": (c_int, []),
    "upsnet_vis_max_label": (c_int, []),
    "upsnet_vis_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "upsnet_vis_font": (c_int, [P]),
    "upsnet_vis_render": (c_int, [P, P, c_int, c_int, c_int, P, P, P, P, P, P, c_int, P, P]),
    "upsnet_pan_vis_workspace_bytes": (c_size_t, []),
    "upsnet_pan_vis_workspace_zeroed_bytes": (c_size_t, []),
    "upsnet_pan_vis_max_labels": (c_int, []),
    "upsnet_pan_vis": (c_int, [P, c_int, P, P, P, P, c_int, c_int, P, P, P, c_int, P, P, P]),
    "upsnet_group_norm_chunk_pixels": (c_int, []),
    "upsnet_group_norm_workspace_bytes": (c_size_t, [c_int, P, P, P]),
    "upsnet_group_norm_nhwc_f32": (c_int, [P, c_int, P, P, P, P, P, c_int, P, P, c_float, c_int, P, P, P, c_int, P]),
    "upsnet_group_norm_small_nhwc_f32": (c_int, [P, P, P, c_int, c_int, c_int, c_int, P, P, c_float, c_int]),
    "upsnet_cs_inst_expand": (c_int, [P, P, P, c_int, c_int, c_int, c_int, P]),
    "upsnet_tta_seg_merge": (c_int, [P, c_int, P, P, P, P, P, P, c_int, c_int, c_int, c_int, P]),
    "upsnet_tta_roi_union": (c_int, [P, c_int, P, P, P, P, P, P, P, c_int, c_int, c_int, P, P, P, P]),
    "upsnet_tta_boxes_to_aug": (c_int, [P, c_int, P, P, P, P, c_int, P]),
    "upsnet_tta_mask_merge": (c_int, [P, c_int, P, P, c_int, c_int, c_int, c_int, P]),
    "upsnet_box_vote": (c_int, [P, P, P, P, c_int, P, c_int, P, c_int, P, c_float, c_float, P, P, P, c_int, P]),
    "upsnet_mask_roi_soft_workspace_bytes": (c_size_t, [c_int, c_int]),
    "upsnet_mask_roi_soft": (c_int, [P, P, P, P, c_int, P, c_int, P, c_int, c_float, c_float, c_int, P, c_int, c_float, c_float, P, P, P, P, P, P]),
    "upsnet_pan_track_workspace_bytes": (c_size_t, [c_int, c_int]),
    "upsnet_pan_track_stamp_offset": (c_size_t, []),
    "upsnet_pan_track_table_ints": (c_size_t, [c_int, c_int]),
    "upsnet_pan_track_table_offset": (c_size_t, []),
    "upsnet_pan_track_step": (c_int, [P, P, c_int, c_int, c_double, c_int, c_int, P, P, P, P, c_int]),
    "upsnet_pan_track_motion_workspace_bytes": (c_size_t, [c_int, c_int]),
    "upsnet_pan_track_motion_count_offset": (c_size_t, []),
    "upsnet_pan_track_motion_pred_offset": (c_size_t, []),
    "upsnet_pan_track_step_motion": (c_int, [P, P, c_int, c_int, c_double, c_int, c_int, P, P, P, P, c_int, P]),
    "upsnet_pan_stable_colors": (c_int, [P, P, c_int, c_int, P, c_int, P]),
    "upsnet_pan_components_workspace_bytes": (c_size_t, [c_int, c_int]),
    "upsnet_pan_components": (c_int, [P, P, c_int, c_int, c_int, c_int, c_int, P, P, P, P]),
    "upsnet_pan_absorb_workspace_bytes": (c_size_t, [c_int, c_int]),
    "upsnet_pan_absorb": (c_int, [P, P, c_int, c_int, c_int, c_int, c_int, P, P, P, P]),
    "upsnet_pan_segment_scores_workspace_bytes": (c_size_t, []),
    "upsnet_pan_segment_scores_table_ints": (c_size_t, []),
    "upsnet_pan_segment_scores": (c_int, [P, P, P, c_int, c_int, P, P]),
    "upsnet_pan_score_filter": (c_int, [P, P, c_int, c_int, P, c_double, P]),
    "upsnet_video_eval_workspace_bytes": (c_size_t, [c_int, c_int, c_int, c_int]),
    "upsnet_video_eval_sequence_ints": (c_size_t, []),
    "upsnet_video_eval_frame": (c_int, [P, P, P, c_int, c_int, P, c_int, c_int, c_int, P, c_int, c_int, c_int, c_int, P, P, P, P, P, P, P]),
    "upsnet_video_eval_end": (c_int, [P, c_int, c_int, c_int, c_int, P, P, P]),
    "upsnet_mots_eval_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "upsnet_mots_eval_frame": (c_int, [P, P, P, c_int, c_int, P, c_int, c_int, c_int, c_int, P, P, P, P, P]),
    "upsnet_mots_eval_end": (c_int, [P, c_int, c_int, P, c_int, c_int, P, P]),
    "upsnet_pan_rle_transitions": (c_int, [P, P, c_int, c_int, c_int, P, P]),
}

_lib = None


def exported_symbols():
    """Names declared in include/upsnet_hip.h (used by the CPU-side ABI test)."""
    return sorted(_SIGNATURES)


def lib():
    """Load libupsnet_hip.so; raise loudly if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError("upsnet_amd: %s is missing -- build it with `python -m upsnet_amd.build` "
                               "(there is no CPU fallback)" % LIB_PATH)
        l = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in _SIGNATURES.items():
            fn = getattr(l, name)  # AttributeError if a declared symbol is not exported
            fn.restype = res
            fn.argtypes = args
        _lib = l
    return _lib


def check(rc, what):
    if rc != 0:
        raise RuntimeError("upsnet_amd.%s failed: %s" % (what, lib().upsnet_last_error().decode()))


_ELEMENT = threading.local()      # depth of ptr_unaligned / ptr_array_unaligned calls in flight on this thread

ALIGN = 16      # bytes: every address handed to an entry point is a multiple of this (include/upsnet_hip.h, "Alignment")


def _address(t, unaligned, what):
    """t.data_ptr(), refused unless it is a multiple of ALIGN. unaligned=True: one of the few parameters the header promises to read at
    element width only (tests/abiguard.py: UNALIGNED); the wrapper says so where it takes the address."""
    a = t.data_ptr()
    if a % ALIGN and not unaligned and not getattr(_ELEMENT, 'depth', 0):
        raise ValueError("%s: the %s tensor of shape %s at 0x%x is not %d-byte aligned (a view that starts inside an allocation?): read-only "
                         "inputs go through f32c / i32c / i64c / nhwc / dense, which copy, written ones through written(), which refuses"
                         % (what, str(t.dtype).replace('torch.', ''), tuple(t.shape), a, ALIGN))
    return a


def ptr(t, unaligned=False):
    """Device pointer of a tensor (None -> NULL). An address that is not 16-byte aligned is a ValueError unless unaligned=True."""
    return None if t is None else c_void_p(_address(t, unaligned, 'ptr'))


def ptr_unaligned(t):
    """ptr(t, unaligned=True) as the wrappers spell it: through the module's `ptr` of the moment with one argument, so that whatever
    stands in for `ptr` (tests/abiguard.py, this tree's or an earlier one's, which knows no second argument) sees the tensor."""
    _ELEMENT.depth = getattr(_ELEMENT, 'depth', 0) + 1
    try:
        return ptr(t)
    finally:
        _ELEMENT.depth -= 1


def stream():
    return c_void_p(torch.cuda.current_stream().cuda_stream)


def require_cuda(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise Exception("not implemented")  # same behaviour as functions/deform_conv.py:40-41


def aligned(t):
    """t itself if its address is a multiple of 16, else a copy of equal values, strides and attached attributes in a fresh allocation
    (the allocator's blocks are aligned far beyond 16 bytes). For READ-ONLY inputs: a copy would swallow a kernel's writes."""
    if t is None or t.data_ptr() % ALIGN == 0:
        return t
    c = t.clone()                       # (preserve_format: a dense view keeps its strides, channels_last stays channels_last)
    c.__dict__.update(t.__dict__)       # (rois._ups_roi_order and its like travel with the values)
    return c


def dense(t):
    """contiguous + aligned, the element type kept: a read-only input whose type the wrapper has checked or converted already (bf16
    packs, uint8 maps, converted counts); None passes through."""
    return None if t is None else aligned(t.contiguous())


def f32c(t):
    """fp32 + contiguous (plumbing); None passes through."""
    if t is None:
        return None
    if t.dtype != torch.float32:
        t = t.float()
    return aligned(t.contiguous())


def i32c(t):
    """int32 + contiguous: a read-only index / count input (a tensor the kernel writes is never converted: a copy would swallow the writes)."""
    if t is None:
        return None
    if t.dtype != torch.int32:
        t = t.to(torch.int32)
    return aligned(t.contiguous())


def i64c(t):
    """int64 + contiguous: a read-only index input (see i32c)."""
    if t is None:
        return None
    if t.dtype != torch.int64:
        t = t.to(torch.int64)
    return aligned(t.contiguous())


def written(t, dtype, what):
    """A tensor the kernel writes (an output, a workspace, a device counter) is taken as it is or refused: `dtype` (None: any, a
    workspace of bytes), contiguous and 16-byte aligned."""
    if t is not None and ((dtype is not None and t.dtype != dtype) or not t.is_contiguous()):
        raise ValueError("%s must be a contiguous %s tensor (got %s, strides %s): the kernel writes it, a converted copy would swallow the writes"
                         % (what, 'any-type' if dtype is None else str(dtype).replace('torch.', ''), str(t.dtype).replace('torch.', ''),
                            tuple(t.stride())))
    if t is not None and t.data_ptr() % ALIGN:
        raise ValueError("%s must be %d-byte aligned (got a view %d bytes past a multiple of %d): the kernel writes it, an aligned copy would "
                         "swallow the writes" % (what, ALIGN, t.data_ptr() % ALIGN, ALIGN))
    return t


def nhwc(t):
    """Physical NHWC view of a logical NCHW tensor (plumbing; no copy if already channels_last)."""
    return aligned(t.contiguous(memory_format=torch.channels_last))


def int_array(vals):
    return (c_int * len(vals))(*[int(v) for v in vals])


def float_array(vals):
    return (c_float * len(vals))(*[float(v) for v in vals])


def ptr_array(tensors, unaligned=False):
    """Host array of device pointers (None -> NULL); every element is held to 16-byte alignment like ptr()'s."""
    return (c_void_p * len(tensors))(*[None if t is None else _address(t, unaligned, 'ptr_array') for t in tensors])


def ptr_array_unaligned(tensors):
    """ptr_array(tensors, unaligned=True) as the wrappers spell it (see ptr_unaligned)."""
    _ELEMENT.depth = getattr(_ELEMENT, 'depth', 0) + 1
    try:
        return ptr_array(tensors)
    finally:
        _ELEMENT.depth -= 1


def addr(t, unaligned=False):
    """Device address of a tensor as a plain int, for a table of addresses that a kernel reads (the caller keeps `t` alive); held to
    16-byte alignment like ptr()'s."""
    return _address(t, unaligned, 'addr')
