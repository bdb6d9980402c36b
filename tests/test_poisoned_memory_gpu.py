"""GPU: every allocating HIP entry point on poisoned, guard-banded memory (tests/memguard.py), and the whole fused forward of both
models on it, eager and as HIP-graph replays.

Each CASES entry runs an op's existing test body -- its edge-shape inputs, its float64 / oracle / golden reference and bound, its zero
contracts ("assert not out[6:].any()", which on poisoned memory now means something) -- twice: under pattern A and under pattern B.
Meanwhile
  * every allocation of the package (outputs, split-K workspaces, weight packs) is poison with guard bands around it,
  * every dense tensor argument of the case's entry points is passed through banded_copy (poison bands around the input),
  * every tensor an entry point returns is recorded, and every numpy array, number and string with it (the evaluators' summaries, the
    writers' pixels); the records of the two patterns must be bitwise equal (only the region DEFINED_REGION names, where a header
    contract leaves the rest undefined),
  * every entry point the case lists must have been called,
  * every band must be intact afterwards.
The entry points are the functions that allocate, in whichever module of the package (memguard.scan_package finds them); for an object
that keeps state, also the method that yields its result, so that what it accumulated reaches the comparison. A body that poisons its
own allocations joins this file's guard and runs wholly under its pattern (memguard.poisoned(adopt=True)).
The table is plain data (test module, test function, arguments, entry points): importable without a GPU, so that
tests/test_memguard_cpu.py can check that no allocating entry point is left out.
"""
import collections
import collections.abc
import contextlib
import importlib
import inspect
import os
import sys
import tempfile

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import memguard  # noqa: E402

pytestmark = pytest.mark.gpu

Case = collections.namedtuple('Case', 'id module test kwargs entries')

_CONV = 'test_conv_gpu'
_OPS = 'test_ops_gpu'


def _c(id, module, test, entries, **kwargs):
    return Case(id, module, test, kwargs, tuple(entries))


W = ('ops.conv2d_winograd_multi', 'ops.pack_winograd_weight')
W36 = ('ops.conv2d_winograd36_multi', 'ops.pack_winograd36_weight')
F1 = ('ops.conv1x1_frag', 'ops.pack_conv1x1_weight')
BF = ('ops.conv2d_nhwc_bf16_multi', 'ops.pack_conv_weight_bf16')
DCN = ('ops.deform_conv_fused', 'ops.pack_dcn_weight')

# the entry points of the later features: every function that allocates, and for a stateful object the method that yields its result
TRACK = ('pan_track.PanopticTracker._start', 'pan_track.PanopticTracker.update', 'pan_track.PanopticTracker.state')
VPQ = ('video_pq.VideoPanopticEvaluator._dev_state', 'video_pq.VideoPanopticEvaluator.add_frame', 'video_pq.VideoPanopticEvaluator.end_sequence',
       'video_pq.VideoPanopticEvaluator.raw')
MOTS = ('mots.MOTSEvaluator._dev_state', 'mots.MOTSEvaluator.add_frame', 'mots.MOTSEvaluator.end_sequence', 'mots.MOTSEvaluator.raw')
CS_INST = ('cityscapes_eval.InstanceEvaluator._reserve', 'cityscapes_eval.InstanceEvaluator._launch', 'cityscapes_eval.InstanceEvaluator.summary')
GTP = ('gt_prepare.gt_prepare_workspace', 'gt_prepare.gt_prepare_launch')
GN = ('group_norm.group_norm_multi', 'group_norm._out_like', 'group_norm.group_norm_small')

CASES = [
    # ---------------------------------------------------------------- direct / implicit-GEMM convolution (+ split-K)
    _c('igemm_ragged_stride2_res', _CONV, 'test_conv2d_nhwc_vs_torch', ('ops.conv2d_nhwc_multi', 'ops.pack_conv_weight'),
       N=2, Cin=32, Cout=96, H=9, W=9, k=3, stride=2, pad=1, relu=True, res=True, bias=True),
    _c('igemm_cout18', _CONV, 'test_conv2d_nhwc_vs_torch', ('ops.conv2d_nhwc_multi', 'ops.pack_conv_weight'),
       N=1, Cin=256, Cout=18, H=17, W=23, k=3, stride=1, pad=1, relu=False, res=False, bias=True),
    _c('igemm_multiw', _CONV, 'test_conv_multi_map_launch_with_per_map_weights', ('ops.conv2d_nhwc_multiw',)),
    _c('igemm_splitk_4_over_3', _CONV, 'test_conv_splitk_vs_unsplit', ('ops.conv2d_nhwc_splitk',),
       N=1, Cin=1024, Cout=256, H=17, W=23, k=1, stride=1, ksplit=3, relu=False, res=True),
    _c('igemm_splitk_cout12', _CONV, 'test_conv_splitk_vs_unsplit', ('ops.conv2d_nhwc_splitk',),
       N=2, Cin=64, Cout=12, H=9, W=10, k=1, stride=1, ksplit=2, relu=True, res=False),
    _c('igemm_splitk_3x3_small', _CONV, 'test_conv_splitk_vs_unsplit', ('ops.conv2d_nhwc_splitk',),
       N=1, Cin=128, Cout=18, H=13, W=11, k=3, stride=1, ksplit=4, relu=False, res=True),
    # ---------------------------------------------------------------- 1x1: frag (both tiles), split-K, pair, siblings, ksw
    _c('frag_one_kstep_small_map', _CONV, 'test_conv1x1_gemm_kernel_vs_torch', F1,
       N=1, Cin=32, Cout=96, H=7, W=5, stride=1, relu=True, res='same', bias=True, bn=0),
    _c('frag_bn128_stride2', _CONV, 'test_conv1x1_gemm_kernel_vs_torch', F1,
       N=3, Cin=96, Cout=160, H=9, W=9, stride=2, relu=True, res=None, bias=True, bn=128),
    _c('frag_up_residual', _CONV, 'test_conv1x1_gemm_kernel_vs_torch', F1,
       N=2, Cin=1024, Cout=256, H=16, W=24, stride=1, relu=False, res='up', bias=True, bn=0),
    _c('frag_splitk_odd', _CONV, 'test_conv1x1_frag_splitk', F1, N=1, Cin=96, Cout=64, H=7, W=5, ks=3, relu=False, res=True),
    _c('frag_splitk_two_images', _CONV, 'test_conv1x1_frag_splitk', F1, N=2, Cin=256, Cout=1024, H=13, W=9, ks=2, relu=True, res=True),
    _c('frag_splitk_11', _CONV, 'test_conv1x1_frag_splitk', F1, N=1, Cin=1024, Cout=256, H=5, W=21, ks=11, relu=True, res=False),
    _c('frag_balanced_main_plus_tail', _CONV, 'test_conv1x1_balanced_main_plus_tail', ('hipconv._conv1x1_balanced',) + F1),
    _c('pair_res2', _CONV, 'test_conv1x1_pair_kernel', ('ops.conv1x1_pair',) + F1, N=1, H=9, W=7, C1=128),
    _c('pair_res3', _CONV, 'test_conv1x1_pair_kernel_res3', ('ops.conv1x1_pair',) + F1, N=2, H=37, W=41, C1=512),
    _c('pair_res4_w8', _CONV, 'test_conv1x1_pair_kernel_res4', ('ops.conv1x1_pair',) + F1, N=1, H=5, W=3, C1=256, waves=8),
    _c('pair_res4_w4', _CONV, 'test_conv1x1_pair_kernel_res4', ('ops.conv1x1_pair',) + F1, N=2, H=19, W=21, C1=1024, waves=4),
    _c('siblings_ragged', _CONV, 'test_conv1x1_sibling_launch', ('ops.conv1x1_siblings',) + F1,
       N=1, Cin=32, H=33, W=17, ca=96, cb=40, stride=1),
    _c('siblings_stride2', _CONV, 'test_conv1x1_sibling_launch', ('ops.conv1x1_siblings',) + F1,
       N=1, Cin=512, H=9, W=7, ca=256, cb=1024, stride=2),
    _c('ksw_cin80_cout36', _CONV, 'test_conv1x1_ksw_vs_fp64', ('ops.conv1x1_ksw', 'ops.pack_conv1x1_ksw_weight'),
       N=1, Cin=80, Cout=36, H=6, W=6, stride=1, relu=True, res=True, bias=True),
    _c('ksw_two_images', _CONV, 'test_conv1x1_ksw_vs_fp64', ('ops.conv1x1_ksw', 'ops.pack_conv1x1_ksw_weight'),
       N=2, Cin=128, Cout=512, H=13, W=9, stride=1, relu=False, res=True, bias=False),
    _c('ksw_stride2_odd', _CONV, 'test_conv1x1_ksw_vs_fp64', ('ops.conv1x1_ksw', 'ops.pack_conv1x1_ksw_weight'),
       N=1, Cin=512, Cout=256, H=27, W=43, stride=2, relu=True, res=False, bias=True),
    _c('ksw3_h1', _CONV, 'test_conv3x3_ksw_vs_fp64', ('ops.conv3x3_ksw', 'ops.pack_conv3x3_ksw_weight'),
       N=3, Cin=16, Cout=27, H=1, W=5, relu=False, bias=True),
    _c('ksw3_two_images', _CONV, 'test_conv3x3_ksw_vs_fp64', ('ops.conv3x3_ksw', 'ops.pack_conv3x3_ksw_weight'),
       N=2, Cin=64, Cout=32, H=9, W=7, relu=False, bias=False),
    _c('ksw3_cout5', _CONV, 'test_conv3x3_ksw_vs_fp64', ('ops.conv3x3_ksw', 'ops.pack_conv3x3_ksw_weight'),
       N=1, Cin=48, Cout=5, H=3, W=3, relu=True, bias=True),
    # ---------------------------------------------------------------- F(2x2): 64- and 32-tile forms, tail entry point, split-K
    _c('wino_ragged', _CONV, 'test_winograd_conv_vs_torch', W, shapes=[(1, 33, 47)], Cin=32, Cout=96, relu=False, res=False, bias=True),
    _c('wino_cout18_32tile', _CONV, 'test_winograd_conv_vs_torch', W, shapes=[(1, 17, 9)], Cin=64, Cout=18, relu=False, res=False, bias=False),
    _c('wino_batch_res', _CONV, 'test_winograd_conv_vs_torch', W, shapes=[(2, 9, 11)], Cin=32, Cout=32, relu=True, res=True, bias=True),
    _c('wino_forms_1x1_map', _CONV, 'test_winograd_tile_forms_agree_bit_for_bit', W, shapes=[(1, 1, 1)], Cin=32, Cout=5),
    _c('wino_forms_ragged_batch', _CONV, 'test_winograd_tile_forms_agree_bit_for_bit', W, shapes=[(1, 2, 3), (3, 5, 7)], Cin=64, Cout=70),
    _c('wino_32ch_form', _CONV, 'test_winograd_32_channel_form_is_bit_identical', W, N=3, Cin=64, Cout=96, H=9, W=11, relu=False),
    _c('wino_tail', _CONV, 'test_winograd_tail_entry_point', W + ('ops.conv2d_winograd_tail',),
       N=5, n_main=4, C=64, Cout=192, H=9, W=11, relu=False),
    _c('wino_tail_split_fused', _CONV, 'test_winograd_tail_split_of_a_batched_launch', W + ('ops.conv2d_winograd_tail',), fused=True),
    _c('wino_tail_split_two_launches', _CONV, 'test_winograd_tail_split_of_a_batched_launch', W + ('hipconv._wino_split_launch',), fused=False),
    _c('wino_splitk_odd', _CONV, 'test_winograd_splitk_vs_torch', W + ('ops.conv2d_winograd_splitk',),
       N=1, H=33, W=47, Cin=64, Cout=96, ksplit=2, relu=False, res=True),
    _c('wino_splitk_6_over_3', _CONV, 'test_winograd_splitk_vs_torch', W + ('ops.conv2d_winograd_splitk',),
       N=1, H=9, W=7, Cin=96, Cout=32, ksplit=3, relu=False, res=False),
    _c('wino_splitk_cout20', _CONV, 'test_winograd_splitk_vs_torch', W + ('ops.conv2d_winograd_splitk',),
       N=1, H=20, W=12, Cin=128, Cout=20, ksplit=2, relu=True, res=True),
    # ---------------------------------------------------------------- F(4x4): multi, split-K, ROI batches; W = 1 and 2
    _c('wino36_smaller_than_tile', _CONV, 'test_winograd36_vs_fp64', W36 + W, segs=[(1, 3, 5)], Cin=32, Cout=64, relu=False, bias=True),
    _c('wino36_h1', _CONV, 'test_winograd36_vs_fp64', W36 + W, segs=[(5, 1, 9)], Cin=32, Cout=64, relu=False, bias=True),
    _c('wino36_w2_h130', _CONV, 'test_winograd36_vs_fp64', W36 + W, segs=[(1, 130, 2)], Cin=32, Cout=64, relu=True, bias=True),
    _c('wino36_w1', _CONV, 'test_winograd36_vs_fp64', W36 + W, segs=[(3, 5, 1)], Cin=32, Cout=64, relu=False, bias=True),
    _c('wino36_w2', _CONV, 'test_winograd36_vs_fp64', W36 + W, segs=[(2, 9, 2)], Cin=32, Cout=64, relu=True, bias=False),
    _c('wino36_cout100', _CONV, 'test_winograd36_vs_fp64', W36 + W, segs=[(1, 20, 20)], Cin=256, Cout=100, relu=True, bias=True),
    _c('wino36_roi_maps', _CONV, 'test_winograd36_vs_fp64', W36 + W, segs=[(7, 14, 14)], Cin=256, Cout=256, relu=True, bias=True),
    _c('wino36_splitk_4_over_3', _CONV, 'test_winograd36_splitk_vs_fp64_and_unsplit', W36 + ('ops.conv2d_winograd36_splitk',),
       N=1, H=33, W=47, Cin=64, Cout=100, ks=3, relu=False, bias=True),
    _c('wino36_splitk_two_images', _CONV, 'test_winograd36_splitk_vs_fp64_and_unsplit', W36 + ('ops.conv2d_winograd36_splitk',),
       N=2, H=9, W=13, Cin=32, Cout=64, ks=2, relu=True, bias=False),
    _c('wino36_roi_batches', _CONV, 'test_winograd36_roi_batches_do_not_depend_on_the_batch', W36),
    # ---------------------------------------------------------------- bf16 convolutions, wreg forms, deconvolutions, score combine
    _c('bf16_mc_3x3_ragged', _CONV, 'test_conv_bf16_matrix_cores_vs_torch', BF,
       N=1, Cin=128, Cout=160, H=37, W=45, k=3, stride=1, pad=1, relu=True, res=True, split=True),
    _c('bf16_mc_batch_small', _CONV, 'test_conv_bf16_matrix_cores_vs_torch', BF,
       N=3, Cin=32, Cout=128, H=9, W=17, k=3, stride=1, pad=1, relu=False, res=False, split=False),
    _c('bf16_act_cout19', _CONV, 'test_conv_bf16_matrix_cores_vs_torch', BF,
       N=1, Cin=512, Cout=19, H=24, W=40, k=1, stride=1, pad=0, relu=False, res=False, split=True),
    _c('bf16_act_io', _CONV, 'test_conv_bf16_activations', BF,
       N=1, Cin=128, Cout=160, H=37, W=45, k=3, stride=1, pad=1, relu=False, res='bf16', in16=True, out16=True),
    _c('bf16_lateral_up', _CONV, 'test_conv_bf16_lateral_with_upsampled_residual', BF, N=1, Cin=64, Cout=96, H=6, W=10, split=False),
    _c('wreg3_ragged', _CONV, 'test_conv3x3_wreg_bf16_kernel', BF, shapes=[(1, 37, 53)], Cin=256, Cout=256, relu=False, bias=True, io=3),
    _c('wreg3_kslabs', _CONV, 'test_conv3x3_wreg_bf16_kernel', BF, shapes=[(1, 40, 24)], Cin=96, Cout=256, relu=True, bias=False, io=1),
    _c('wreg1_small_map', _CONV, 'test_conv1x1_wreg_bf16_kernel', BF,
       N=1, Cin=2048, Cout=512, H=7, W=9, stride=1, relu=True, res='fp32', bias=True, out16=True),
    _c('wreg1_384', _CONV, 'test_conv1x1_wreg_bf16_kernel', BF, N=3, Cin=128, Cout=384, H=5, W=5, stride=1, relu=True, res=None, bias=True,
       out16=False),
    _c('wreg1_stride2', _CONV, 'test_conv1x1_wreg_bf16_kernel', BF, N=2, Cin=256, Cout=128, H=41, W=57, stride=2, relu=True, res=None,
       bias=True, out16=True),
    _c('deconv_bf16_narrow', _CONV, 'test_deconv2x2_bf16_vs_torch', ('ops.deconv2x2_bf16',),
       N=1, Cin=64, Cout=32, H=5, W=9, relu=False, bias=False, out16=True),
    _c('deconv_bf16_f32out', _CONV, 'test_deconv2x2_bf16_vs_torch', ('ops.deconv2x2_bf16',),
       N=3, Cin=128, Cout=96, H=6, W=6, relu=True, bias=True, out16=False),
    _c('deconv_frag_ragged', _CONV, 'test_deconv2x2_frag_vs_torch', ('ops.deconv2x2_frag',),
       N=7, Cin=256, Cout=256, H=14, W=14, relu=True, bias=True),
    _c('deconv_frag_tiny', _CONV, 'test_deconv2x2_frag_vs_torch', ('ops.deconv2x2_frag',), N=1, Cin=96, Cout=64, H=3, W=3, relu=True, bias=True),
    _c('deconv_f32', 'test_preprocess_gpu', 'test_deconv2x2_vs_torch', ('ops.deconv2x2', 'ops.pack_deconv2x2_weight'),
       N=1, H=5, W=9, Cin=64, Cout=32),
    _c('fcn_combine_2lev', _CONV, 'test_fcn_score_combine_vs_oracle', ('ops.fcn_score_combine',), S=5, H=8, W=8, nlev=2, bias=False),
    _c('fcn_combine_133', _CONV, 'test_fcn_score_combine_vs_oracle', ('ops.fcn_score_combine',), S=133, H=24, W=40, nlev=4, bias=True),
    # ---------------------------------------------------------------- stem, stem + pool, preprocess, bottleneck blocks
    _c('stem_conv', 'test_preprocess_gpu', 'test_stem_conv_vs_torch', ('ops.conv2d_stem', 'ops.pack_stem_weight', 'ops.image_to_nhwc4'),
       N=2, H=33, W=47, Cout=64, k=7, stride=2, pad=3),
    _c('stem_pool_f32_small', 'test_stem_pool_gpu', 'test_stem_pool_f32_vs_float64',
       ('ops.stem_pool_f32', 'ops.pack_stem_pool_weight_f32', 'ops.image_to_nhwc4'), N=1, H=9, W=7, bias=True),
    _c('stem_pool_f32_batch', 'test_stem_pool_gpu', 'test_stem_pool_f32_vs_float64',
       ('ops.stem_pool_f32', 'ops.pack_stem_pool_weight_f32', 'ops.image_to_nhwc4'), N=2, H=37, W=53, bias=True),
    _c('stem_pool_bf16_small', 'test_stem_pool_gpu', 'test_stem_pool_bf16_vs_float64',
       ('ops.stem_pool_bf16', 'ops.pack_stem_pool_weight_bf16', 'ops.image_to_nhwc4'), N=1, H=9, W=7, bias=True),
    _c('stem_pool_bf16_batch', 'test_stem_pool_gpu', 'test_stem_pool_bf16_vs_float64',
       ('ops.stem_pool_bf16', 'ops.pack_stem_pool_weight_bf16', 'ops.image_to_nhwc4'), N=2, H=37, W=53, bias=True),
    _c('prep_u8_nhwc4', 'test_preprocess_gpu', 'test_prep_image_u8_vs_oracle', ('ops.prep_image_u8',),
       H=37, W=53, target=64, max_size=96, nhwc4=True),
    _c('prep_u8_nchw', 'test_preprocess_gpu', 'test_prep_image_u8_vs_oracle', ('ops.prep_image_u8',),
       H=60, W=45, target=30, max_size=1000, nhwc4=False),
    _c('bottleneck_small_map', 'test_bottleneck_bf16_gpu', 'test_bottleneck_bf16_vs_float64', ('ops.bottleneck_bf16',), cm=256, N=1, H=3, W=5),
    _c('bottleneck_ragged_batch', 'test_bottleneck_bf16_gpu', 'test_bottleneck_bf16_vs_float64', ('ops.bottleneck_bf16',), cm=64, N=2, H=37, W=53),
    _c('bottleneck_three_launch', 'test_bottleneck_bf16_gpu', 'test_bottleneck_bf16_equals_the_three_launch_path', ('ops.bottleneck_bf16',) + BF,
       cm=512, N=1, H=9, W=12),
    _c('bottleneck_proj_odd', 'test_bottleneck_bf16_gpu', 'test_bottleneck_proj_bf16_vs_float64', ('ops.bottleneck_proj_bf16',),
       cm=128, cin=256, stride=2, N=1, H=37, W=53),
    _c('bottleneck_proj_batch', 'test_bottleneck_bf16_gpu', 'test_bottleneck_proj_bf16_vs_float64', ('ops.bottleneck_proj_bf16',),
       cm=256, cin=512, stride=2, N=2, H=9, W=15),
    # ---------------------------------------------------------------- DCN: fused frag / igemm / split-K / bf16, im2col / col2im drop-ins
    _c('dcn_frag_4maps', _OPS, 'test_deform_conv_fused_vs_oracle', DCN,
       cin=64, cout=128, sizes=[(16, 24), (8, 12), (4, 6), (2, 3)], mod=False, relu=True, kind='frag'),
    _c('dcn_frag_cout19_mod', _OPS, 'test_deform_conv_fused_vs_oracle', DCN, cin=64, cout=19, sizes=[(11, 13)], mod=True, relu=False, kind='frag'),
    _c('dcn_igemm_ragged', _OPS, 'test_deform_conv_fused_vs_oracle', DCN, cin=128, cout=160, sizes=[(33, 17)], mod=False, relu=False,
       kind='igemm'),
    _c('dcn_igemm_2maps', _OPS, 'test_deform_conv_fused_vs_oracle', DCN, cin=32, cout=256, sizes=[(7, 19), (3, 5)], mod=False, relu=False,
       kind='igemm'),
    _c('dcn_splitk', _OPS, 'test_deform_conv_fused_splitk_small_maps', DCN, cin=512, cout=512, H=13, W=21),
    _c('dcn_bf16_4maps', _OPS, 'test_deform_conv_fused_bf16_matrix_cores', DCN,
       cin=64, cout=128, sizes=[(16, 24), (8, 12), (4, 6), (2, 3)], mod=False, relu=True, k=3, pad=1, dil=1),
    _c('dcn_bf16_dil_cout19', _OPS, 'test_deform_conv_fused_bf16_matrix_cores', DCN,
       cin=64, cout=19, sizes=[(11, 13)], mod=True, relu=False, k=3, pad=2, dil=2),
    _c('dcn_geometry_stride2', _OPS, 'test_deform_conv_fused_geometries', DCN, k=3, pad=1, stride=2, dil=1),
    _c('dcn_im2col_dg2', _OPS, 'test_deform_im2col_bitexact', ('ops.deform_im2col', 'ops.mod_deform_im2col'),
       C=12, H=9, W=9, k=3, pad=2, stride=1, dil=2, dg=2),
    _c('dcn_function_module', _OPS, 'test_deform_conv_function_and_module', DCN),
    # ---------------------------------------------------------------- ROIAlign (natural and dealt order, device counts 0 / < N / = N)
    _c('roi_align_nchw_nhwc', _OPS, 'test_roi_align_nchw_bitexact', ('ops.roi_align_nchw', 'ops.roi_align_nhwc'),
       C=4, H=5, W=7, ph=7, scale=1.0 / 32),
    _c('fpn_roi_align_c320', _OPS, 'test_fpn_roi_align_bitexact', ('ops.fpn_roi_align',), N=9, ph=14, C=320, variant=0),
    _c('fpn_roi_align_32x32_bins', _OPS, 'test_fpn_roi_align_bitexact', ('ops.fpn_roi_align',), N=33, ph=32, C=8, variant=3),
    _c('fpn_roi_align_one', _OPS, 'test_fpn_roi_align_bitexact', ('ops.fpn_roi_align',), N=1, ph=7, C=32, variant=4),
    _c('fpn_roi_align_padded_tail', _OPS, 'test_fpn_roi_align_padded_tail', ('ops.fpn_roi_align',)),
    _c('fpn_roi_order_count_lt_n', _OPS, 'test_fpn_roi_align_xcd_order_is_a_permutation_and_changes_no_bit',
       ('ops.fpn_roi_order', 'ops.fpn_roi_align'), N=37, ph=7, nvalid=21),
    _c('fpn_roi_order_count_0', _OPS, 'test_fpn_roi_align_xcd_order_is_a_permutation_and_changes_no_bit',
       ('ops.fpn_roi_order', 'ops.fpn_roi_align'), N=9, ph=14, nvalid=0),
    _c('fpn_roi_order_count_n', _OPS, 'test_fpn_roi_align_xcd_order_is_a_permutation_and_changes_no_bit',
       ('ops.fpn_roi_order', 'ops.fpn_roi_align'), N=300, ph=7, nvalid=None),
    # ---------------------------------------------------------------- proposals, NMS, detection
    _c('proposals_small', _OPS, 'test_pyramid_proposals_bitexact', ('ops.pyramid_proposals',), H=32, W=32, pre=50, post=20),
    _c('proposals_table', _OPS, 'test_pyramid_proposals_write_the_roi_xcd_table_of_the_box_head', ('ops.pyramid_proposals', 'ops.fpn_roi_align')),
    _c('proposals_joint', _OPS, 'test_pyramid_proposals_joint_bitexact', ('ops.pyramid_proposals',),
       H=96, W=160, pre=300, post=250, thr=0.3, min_size=8),
    _c('nms_device_65', _OPS, 'test_gpu_nms_bitexact', ('ops.gpu_nms', 'ops.nms_batched'), n=65, thresh=0.5),
    _c('nms_device_1', _OPS, 'test_gpu_nms_bitexact', ('ops.gpu_nms', 'ops.nms_batched'), n=1, thresh=0.7),
    _c('nms_wrappers_empty', _OPS, 'test_nms_wrappers_and_empty', ('ops.gpu_nms', 'ops.nms_batched')),
    _c('nms_batched_counts', _OPS, 'test_nms_batched_with_counts_and_preremoved', ('ops.nms_batched',)),
    _c('nms_host_compatible', _OPS, 'test_cpu_nms_ge_bitexact', ('ops.cpu_nms',), n=65, thresh=0.3),
    _c('soft_nms_uneven', _OPS, 'test_soft_nms_batched_bitexact', ('ops.soft_nms_batched',), method=1, nmax=64, P=3),
    _c('soft_nms_1', _OPS, 'test_soft_nms_bitexact', ('ops.soft_nms_batched',), method=2, n=5),
    _c('mask_roi_small', _OPS, 'test_mask_roi_bitexact', ('ops.mask_roi',), N=7, C=9, agn=False, thresh=0.05, peaky=1.0),
    _c('mask_roi_agnostic_none', _OPS, 'test_mask_roi_bitexact', ('ops.mask_roi',), N=50, C=9, agn=True, thresh=0.999, peaky=0.1),
    _c('mask_roi_dedup', 'test_model_gpu', 'test_mask_head_dedup_is_bit_identical_to_two_passes',
       ('ops.mask_roi_dedup', 'ops.mask_roi')),
    _c('mask_logit_gather_nhwc', _OPS, 'test_mask_logit_gather_bitexact', ('ops.mask_logit_gather',), n=5, C=9, ms=28, K=7, layout='nhwc'),
    _c('mask_logit_gather_more_than_rows', _OPS, 'test_mask_logit_gather_bitexact', ('ops.mask_logit_gather',), n=37, C=81, ms=7, K=300,
       layout='nhwc'),
    _c('mask_logit_gather_bf16', _OPS, 'test_mask_logit_gather_bitexact', ('ops.mask_logit_gather',), n=4, C=3, ms=28, K=5, layout='bf16'),
    _c('nms_chain_1025', 'test_selection_structured_gpu', 'test_nms_structured', ('ops.gpu_nms', 'ops.nms_batched'), name='chain-1025-0.5'),
    _c('proposals_tail_pass', 'test_selection_structured_gpu', 'test_proposals_structured', ('ops.pyramid_proposals',),
       name='decided_in-tail2-60', individual=True),
    _c('mask_roi_cut_in_tie', 'test_selection_structured_gpu', 'test_mask_roi_structured', ('ops.mask_roi',),
       name='cut_in_tie', agn=False, clip=True),
    # ---------------------------------------------------------------- panoptic head / fuse / argmax / tail, post-processing
    _c('panoptic_head_one', _OPS, 'test_panoptic_head_bitexact',
       ('ops.panoptic_fuse', 'ops.mask_paste', 'ops.seg_term', 'ops.panoptic_argmax', 'ops.mask_removal'), m=1, S=19, C=9, H=64, W=64, void=True),
    _c('panoptic_head_coco', _OPS, 'test_panoptic_head_bitexact',
       ('ops.panoptic_fuse', 'ops.mask_paste', 'ops.seg_term', 'ops.panoptic_argmax', 'ops.mask_removal'),
       m=12, S=133, C=81, H=96, W=100, void=False),
    _c('mask_removal_dummy', _OPS, 'test_mask_removal_modules_and_dummy', ('ops.mask_removal',)),
    _c('panoptic_fuse_up_one', _OPS, 'test_panoptic_fuse_with_fused_upsample_bitexact', ('ops.panoptic_fuse_up', 'ops.panoptic_fuse'),
       m=1, S=19, C=9, Hs=16, Ws=16, nhwc=True),
    _c('panoptic_fuse_up_nchw', _OPS, 'test_panoptic_fuse_with_fused_upsample_bitexact', ('ops.panoptic_fuse_up', 'ops.panoptic_fuse'),
       m=60, S=19, C=9, Hs=64, Ws=128, nhwc=False),
    _c('panoptic_tail_pack', _OPS, 'test_panoptic_tail_pack_and_keep_zero_fill', ('ops.panoptic_tail_pack', 'ops.mask_removal')),
    _c('panoptic_crowd_dropped', 'test_panoptic_structured_gpu', 'test_mask_removal_structured', ('ops.mask_removal',), name='crowd-dropped'),
    _c('panoptic_1024_one_class', 'test_panoptic_structured_gpu', 'test_mask_removal_structured', ('ops.mask_removal',),
       name='many-1024-True'),
    _c('panoptic_odd_width_101', 'test_panoptic_structured_gpu', 'test_panoptic_fuse_structured',
       ('ops.panoptic_fuse', 'ops.mask_paste', 'ops.seg_term', 'ops.panoptic_argmax', 'ops.mask_removal'), name='odd_width-101', void=True),
    _c('panoptic_golden', 'test_golden_gpu', 'test_panoptic_head_golden', ('ops.panoptic_fuse', 'ops.panoptic_argmax')),
    _c('unified_pan_odd', 'test_postprocess_gpu', 'test_unified_pan_vs_oracle', ('ops.unified_pan_result',), H=33, W=47, k=3, limit=50, seed=2),
    _c('unified_pan_no_inst', 'test_postprocess_gpu', 'test_unified_pan_vs_oracle', ('ops.unified_pan_result',), H=64, W=64, k=0,
       limit=10 ** 9, seed=3),
    _c('rle_transitions', 'test_postprocess_gpu', 'test_im_post_rle_vs_oracle', ('rle.mask_transitions',), H=120, W=75, n=20, seed=1),
    _c('combined_pan_ragged', 'test_pan_combined_gpu', 'test_ragged_empty_and_input_kinds', ('ops.combined_pan_result',)),
    _c('combined_pan_hand', 'test_pan_combined_gpu', 'test_hand_derived_cases', ('ops.combined_pan_result',)),
    # ---------------------------------------------------------------- evaluation
    _c('pq_odd_sizes', 'test_pq_gpu', 'test_unaligned_and_odd_sizes', ('ops.pq_accumulate',)),
    _c('pq_single_segment', 'test_pq_gpu', 'test_single_segment_and_all_void', ('ops.pq_accumulate',)),
    _c('confusion_golden', 'test_pq_gpu', 'test_confusion_matrix_golden_and_miou', ('ops.confusion_accumulate',)),
    _c('coco_bbox_scene', 'test_coco_eval_gpu', 'test_bbox_random_scenes_bitwise',
       ('coco_eval.DetectionEvaluator._alloc_records', 'coco_eval.DetectionEvaluator._launch_on_device',
        'coco_eval.DetectionEvaluator.accumulate'), seed=1),
    _c('coco_segm_rle', 'test_coco_eval_gpu', 'test_segm_model_tensors_and_rle_strings_bitwise',
       ('coco_eval.DetectionEvaluator._launch_on_device', 'coco_eval.DetectionEvaluator.accumulate', 'rle.mask_transitions')),
    _c('restore_pil_shrink', 'test_dataset_run_gpu', 'test_restore_pil_rule_matches_pil', ('ops.restore_label_maps',), src=(7, 9), dst=(3, 5)),
    _c('restore_cv2_1x1', 'test_dataset_run_gpu', 'test_restore_cv2_rule_matches_numpy', ('ops.restore_label_maps',),
       im_info=(1, 1, 3.0), pad=0),
    # ---------------------------------------------------------------- sequences: tracker, VPQ / STQ, MOTS (dataset/pan_track.py, video_pq.py, mots.py)
    _c('track_reset_four_frames', 'test_pan_track_gpu', 'test_reset_gives_a_fresh_tracker', TRACK),
    _c('track_hand_three_frames', 'test_pan_track_gpu', 'test_hand_cases_equal_the_restatement', TRACK, name='three_frames'),
    _c('track_blobs_37x53', 'test_pan_track_gpu', 'test_few_things', TRACK, things=1),
    _c('vpq_two_sequences_37x53', 'test_video_pq_gpu', 'test_workspace_is_zero_again_and_a_second_sequence_scores_as_on_a_fresh_evaluator', VPQ),
    _c('vpq_three_sizes_one_evaluator', 'test_video_pq_gpu', 'test_a_used_evaluator_takes_sequences_of_other_sizes_like_a_fresh_one', VPQ),
    _c('vpq_hand_short_window', 'test_video_pq_gpu', 'test_hand_cases_equal_the_restatement', VPQ, name='short'),
    _c('mots_two_sequences_37x53', 'test_mots_gpu', 'test_workspace_is_zero_again_and_a_second_sequence_scores_as_on_a_fresh_evaluator', MOTS),
    _c('mots_three_sizes_one_evaluator', 'test_mots_gpu', 'test_a_used_evaluator_takes_sequences_of_other_sizes_like_a_fresh_one', MOTS),
    _c('mots_zero_scored_frames', 'test_mots_gpu', 'test_sequence_with_zero_scored_frames', MOTS),
    _c('mots_rle_retry_edge', 'test_mots_gpu', 'test_rle_transitions_equal_numpy', ('mots.segment_transitions',), name='edge'),
    _c('mots_rle_retry_blob', 'test_mots_gpu', 'test_rle_transitions_equal_numpy', ('mots.segment_transitions',), name='blob0'),
    _c('mots_rle_no_thing', 'test_mots_gpu', 'test_rle_transitions_equal_numpy', ('mots.segment_transitions',), name='no_thing'),
    # ---------------------------------------------------------------- Cityscapes instance AP / pixel IoU / instance files
    _c('cs_inst_rle_odd', 'test_cityscapes_inst_gpu', 'test_poisoned_guard_banded_memory', CS_INST, feed='rle'),
    _c('cs_inst_masks_odd', 'test_cityscapes_inst_gpu', 'test_poisoned_guard_banded_memory', CS_INST, feed='masks'),
    _c('cs_inst_no_predictions', 'test_cityscapes_inst_gpu', 'test_images_without_predictions_and_empty_evaluator', CS_INST),
    _c('cs_pixel_odd', 'test_cityscapes_pixel_gpu', 'test_poisoned_guard_banded_memory',
       ('cityscapes_pixel_eval.PixelEvaluator._launch', 'cityscapes_pixel_eval.PixelEvaluator.summary')),
    _c('cs_expand_65x129_8bit', 'test_cityscapes_inst_format_gpu', 'test_poisoned_guard_banded_memory', ('cityscapes_inst_format.expand_masks',),
       size=(65, 129), one_bit=False),
    _c('cs_expand_65x129_1bit', 'test_cityscapes_inst_format_gpu', 'test_poisoned_guard_banded_memory', ('cityscapes_inst_format.expand_masks',),
       size=(65, 129), one_bit=True),
    _c('cs_expand_37x53_1bit', 'test_cityscapes_inst_format_gpu', 'test_poisoned_guard_banded_memory', ('cityscapes_inst_format.expand_masks',),
       size=(37, 53), one_bit=True),
    _c('cs_files_write_and_score', 'test_cityscapes_inst_format_gpu', 'test_written_folders_score_like_the_lists_in_memory',
       ('cityscapes_inst_format.InstanceMaskFormatter.submit', 'cityscapes_inst_format.InstanceMaskFormatter.finish',
        'cityscapes_inst_format.score_instance_files', 'cityscapes_eval.InstanceEvaluator.last_counts') + CS_INST),
    # ---------------------------------------------------------------- panoptic PNG format, pictures (dataset/pan_format.py, pan_vis.py, vis.py)
    _c('pan_format_101x77', 'test_pan_format_gpu', 'test_poisoned_memory_panoptic_format',
       ('pan_format.PanopticFormatter.submit', 'pan_format.PanopticFormatter.finish')),
    _c('pan_format_stable_37x53', 'test_pan_track_gpu', 'test_stable_colours_equal_the_host_statement',
       ('pan_format.PanopticFormatter.submit', 'pan_format.PanopticFormatter.finish'), H=37, W=53),
    _c('pan_relabel_add_png', 'test_pan_format_gpu', 'test_poisoned_memory_relabel_and_add_png', ('pan_format.relabel',)),
    _c('pan_vis_three_sizes', 'test_pan_vis_gpu', 'test_poisoned_output_and_workspace_over_images_of_different_size',
       ('pan_vis.PanopticRenderer._dev_state', 'pan_vis.PanopticRenderer.submit')),
    _c('pan_vis_used_workspace', 'test_pan_vis_gpu', 'test_used_workspace_gives_the_bytes_of_a_fresh_one',
       ('pan_vis.PanopticRenderer._dev_state', 'pan_vis.PanopticRenderer.submit')),
    _c('vis_three_sizes', 'test_vis_gpu', 'test_poisoned_output_and_workspace_two_images_of_different_size', ('vis.render_detections',)),
    _c('vis_33x65', 'test_vis_gpu', 'test_odd_sizes_and_detection_counts_match_restatement', ('vis.render_detections',), H=33, W=65, n=9),
    _c('vis_no_detections', 'test_vis_gpu', 'test_odd_sizes_and_detection_counts_match_restatement', ('vis.render_detections',), H=97, W=130, n=0),
    # ---------------------------------------------------------------- boundaries, polygons, ground truth, proposal recall
    _c('boundary_masks_65x130', 'test_boundary_gpu', 'test_mask_to_boundary_bitwise', ('boundary.mask_to_boundary',), H=65, W=130, ratio=.02),
    _c('boundary_masks_64x33', 'test_boundary_gpu', 'test_mask_to_boundary_bitwise', ('boundary.mask_to_boundary',), H=64, W=33, ratio=.02),
    _c('boundary_ap_rect_planes', 'test_boundary_gpu', 'test_rect_limited_det_planes',
       ('coco_eval.DetectionEvaluator._launch_on_device', 'coco_eval.DetectionEvaluator.accumulate')),
    _c('boundary_pan_17x33_d2', 'test_boundary_pq_gpu', 'test_panoptic_boundary_bits', ('boundary.panoptic_boundary',), H=17, W=33, d=2),
    _c('boundary_pan_64x65_d7', 'test_boundary_pq_gpu', 'test_panoptic_boundary_bits', ('boundary.panoptic_boundary',), H=64, W=65, d=7),
    _c('boundary_pan_window_gt_image', 'test_boundary_pq_gpu', 'test_panoptic_boundary_bits', ('boundary.panoptic_boundary',), H=5, W=7, d=3),
    _c('polygon_four_sizes', 'test_polygon_gpu', 'test_on_poisoned_guard_banded_memory',
       ('polygon.rasterize_polygons', 'polygon.PolygonRasters.transitions'), pattern='A'),
    _c('gt_prepare_37x53', 'test_gt_prepare_gpu', 'test_guard_bands_and_every_byte_written', GTP, name='37x53', pattern='A'),
    _c('gt_prepare_ignored_only', 'test_gt_prepare_gpu', 'test_guard_bands_and_every_byte_written', GTP, name='ignored_only', pattern='B'),
    _c('gt_prepare_transition_overflow', 'test_gt_prepare_gpu', 'test_transition_overflow_raises_and_leaves_the_workspace_clean', GTP),
    _c('gt_prepare_regrow', 'test_gt_prepare_gpu', 'test_preparer_runs_an_image_that_outgrows_the_default_transitions_again', GTP),
    _c('gt_semantic_37x53', 'test_gt_prepare_gpu', 'test_semantic_converter_equals_restatement', ('gt_prepare.panoptic_semantic', 'pan_format.relabel')),
    _c('proposal_recall_four_images', 'test_proposal_recall_gpu', 'test_poisoned_memory',
       ('proposal_eval.ProposalRecallEvaluator._add', 'proposal_eval.ProposalRecallEvaluator.summary')),
    _c('proposal_recall_image_without_gt', 'test_proposal_recall_gpu', 'test_device_equals_restatement_all_areas_and_limits',
       ('proposal_eval.ProposalRecallEvaluator._add', 'proposal_eval.ProposalRecallEvaluator.summary'),
       seed=12, sizes=[(2000, 300), (5, 5), (1, 1), (1000, 0)]),
    # ---------------------------------------------------------------- test-time augmentation, voting, soft selection (tta.py)
    _c('tta_seg_merge_scalar_19', 'test_tta_gpu', 'test_seg_merge_equals_the_restatement', ('tta.seg_merge',), S=19, cell=4),
    _c('tta_seg_merge_vector_20', 'test_tta_gpu', 'test_seg_merge_equals_the_restatement', ('tta.seg_merge',), S=20, cell=1),
    _c('tta_seg_merge_unaligned', 'test_tta_gpu', 'test_seg_merge_unaligned_bases_take_the_scalar_form', ('tta.seg_merge',)),
    _c('tta_union_8_rows', 'test_tta_gpu', 'test_roi_union_equals_the_restatement', ('tta.roi_union',), R=8, C=9),
    _c('tta_union_clamped_counts', 'test_tta_gpu', 'test_roi_union_clamps_counts_to_the_capacity', ('tta.roi_union',)),
    _c('tta_boxes_100', 'test_tta_gpu', 'test_boxes_to_aug_equals_the_restatement', ('tta.boxes_to_aug',), n=100),
    _c('tta_boxes_1', 'test_tta_gpu', 'test_boxes_to_aug_equals_the_restatement', ('tta.boxes_to_aug',), n=1),
    _c('tta_mask_merge_nchw', 'test_tta_gpu', 'test_mask_merge_equals_the_restatement', ('tta.mask_merge',), n=100, channels_last=False),
    _c('tta_mask_merge_nhwc_one', 'test_tta_gpu', 'test_mask_merge_equals_the_restatement', ('tta.mask_merge',), n=1, channels_last=True),
    _c('box_vote_65', 'test_box_vote_gpu', 'test_box_vote_equals_the_restatement', ('tta.box_vote',), N=65, C=9),
    _c('box_vote_overflow_marker', 'test_box_vote_gpu', 'test_overflow_marker_copies_every_row_and_a_count_past_the_capacity_is_clamped',
       ('tta.box_vote',), num=-1),
    _c('soft_select_65', 'test_soft_select_gpu', 'test_soft_selection_equals_the_restatement', ('tta.mask_roi_soft',), N=65, C=9),
    _c('soft_select_dummy_row', 'test_soft_select_gpu', 'test_nothing_above_the_threshold_and_no_rows_give_the_dummy_row', ('tta.mask_roi_soft',)),
    # ---------------------------------------------------------------- GroupNorm heads (group_norm.py)
    _c('gn_groups_of_3_lanes', 'test_group_norm_gpu', 'test_poisoned_memory_op', GN, shape=(2, 384, 5, 7)),
    _c('gn_groups_of_5_lanes', 'test_group_norm_gpu', 'test_poisoned_memory_op', GN, shape=(1, 640, 3, 3)),
    _c('gn_fc_rows_67', 'test_group_norm_gpu', 'test_poisoned_memory_op', GN, shape=(67, 1024, 1, 1)),
    _c('gn_ragged_last_chunk', 'test_group_norm_gpu', 'test_poisoned_memory_op', GN[:2], shape='3P+7'),
    _c('gn_relu_upsampled_residual', 'test_group_norm_gpu', 'test_poisoned_memory_epilogues', GN[:2], case=dict(relu=True, res='up')),
    _c('gn_pyramid_one_launch', 'test_group_norm_gpu', 'test_multi_map_launch_equals_single_launches', GN[:2]),
]

# allocating entry points without a case of their own here, and why
EXCLUDED = {
    'deform_conv._DeformLayer.__init__':
        "(module not guarded: memguard.UNGUARDED) module construction: the two torch.empty are nn.Parameter storage that reset_parameters() fills entirely (uniform_) in the same "
        "constructor, before any kernel can see it; the kernels that read it are the DCN cases above",
    'resnet_upsnet.resnet_upsnet._phase1_graphed':
        "its one torch.empty is the 4-word host buffer (CPU, then .pin_memory()) that a captured copy fills with the tail counters; no "
        "kernel is given it, and the function itself runs under both patterns in test_fused_forward_on_poisoned_memory_eager_and_graph_replay",
    'upsnet_end2end_test.ResultGatherer.__init__':
        "the benchmark script's multi-process gatherer: its send buffers are written by Tensor.copy_ / fill_ (ResultGatherer._write) and read "
        "by torch.distributed collectives only, never by a HIP kernel of the package; it needs a process group (tests/test_dist_cpu.py runs it)",
    'upsnet_end2end_test.ResultGatherer._alloc_store':
        "the receive store of the same gatherer: filled by dist.gather and read back row by row up to each rank's record count; no HIP "
        "kernel of the package touches it, and it needs a process group (tests/test_dist_cpu.py runs it)",
}

# entry point -> (function of (the returned tensors, the positional arguments) -> the tensors whose every bit is defined): where include/upsnet_hip.h leaves part
# of an output undefined, only the defined part is compared between the patterns
def _rows(t, n):
    return [t[p, :int(n[p])] for p in range(t.shape[0])]


def _pan_vis_zeroed():
    from upsnet_amd._lib import lib
    return int(lib().upsnet_pan_vis_workspace_zeroed_bytes())


def _gt_prepare_defined(r, a):
    """include/upsnet_hip.h, upsnet_gt_prepare: "table ...; rows past the count are not written", "trans_off int [seg_capacity + 1]:
    [0 .. instances] are written", trans holds the lists up to trans_off[instances], status flag 1 "more segments than seg_capacity (no
    instance list is made", flag 2 "(trans is not written)", flag 4 "the outputs are not to be used"; of both maps "every byte ... is
    written"."""
    train_map, rgb, table, trans_off, trans, status = r
    n_seg, n_inst, n_trans, flags = (int(v) for v in status[:4].tolist())
    if flags & 4:
        return [status]
    out = [train_map, rgb, status, table[:min(n_seg, table.shape[0])]]
    if not flags & 1:
        out.append(trans_off[:n_inst + 1])
        if not flags & 2:
            out.append(trans[:n_trans])
    return out


DEFINED_REGION = {
    # (train_map, rgb, table, trans_off, trans, status) at their capacities: see _gt_prepare_defined
    'gt_prepare.gt_prepare_launch': _gt_prepare_defined,
    # the output buffer before the launch that fills it (its contents at return are the allocator's); what the launch writes is
    # compared through group_norm_multi / group_norm_small, which return it
    'group_norm._out_like': lambda ret, a: [],
    # the renderer's state dict: of its workspace "its first upsnet_pan_vis_workspace_zeroed_bytes() bytes ZEROED ONCE before the first
    # use, every call leaves them zeroed again; the rest needs no zeroing" (include/upsnet_hip.h, upsnet_pan_vis): the rest is scratch
    'pan_vis.PanopticRenderer._dev_state': lambda st, a: [st['ws'][:_pan_vis_zeroed()], st['names'], st['lens']],
    # the evaluator's state dict, handed out again at every frame. Its seq_out is written by end_sequence alone (the allocator's until
    # then), and then holds "pairs (cell + 1, count), in arbitrary order; ... [1] and the ints past the last pair are unspecified"
    # (include/upsnet_hip.h, upsnet_video_eval_end): what it delivers is compared through raw(), which resolves the cells in a fixed order
    'video_pq.VideoPanopticEvaluator._dev_state': lambda st, a: [st[k] for k in sorted(st) if k != 'seq_out'],
    # "Of the four outputs the rows below max(|*num_out|, min(cap, max(max_det, 256))) are defined -- the selection, the dummy row, zero
    # rows --, the rows from there on are unspecified" (include/upsnet_hip.h, upsnet_mask_roi_soft); a[6] is max_det
    'tta.mask_roi_soft': lambda r, a: [t[:max(abs(int(r[4][0])), min(t.shape[0], max(int(a[6]), 256)))] for t in r[:4]] + [r[4]],
    # the record buffers the per-image launches fill later (their contents at return are the allocator's)
    'coco_eval.DetectionEvaluator._alloc_records': lambda ret, a: [],
    # a permutation; the order of the ROIs inside one (level, stripe, cell) bucket is unspecified (include/upsnet_hip.h)
    'ops.fpn_roi_order': lambda order, a: [order.sort().values],
    # keep_idx rows past keep_cnt[p] unspecified (include/upsnet_hip.h)
    'ops.nms_batched': lambda r, a: _rows(r[0], r[1]) + [r[1]],
    # boxes / inds rows past n_out[p] unspecified (include/upsnet_hip.h)
    'ops.soft_nms_batched': lambda r, a: _rows(r[0], r[2]) + _rows(r[1], r[2]) + [r[2]],
    # rows past num unspecified (include/upsnet_hip.h)
    'ops.mask_roi': lambda r, a: [t[:int(r[4][0])] for t in r[:4]] + [r[4]],
    # map_out rows past *num_b and extra_boxes rows past *num_extra unspecified (include/upsnet_hip.h)
    'ops.mask_roi_dedup': lambda r, a: [r[0][:int(a[6][0])], r[1][:int(r[2][0])], r[2]],
}

# arguments that an entry point writes (never passed through banded_copy)
INPLACE_ARGS = {'out', 'outs', 'workspace', 'data_col', 'tp', 'fp', 'fn', 'iou', 'status', 'confusion', 'grad_im', 'grad_offset',
                'grad_mask', 'bottom_grad'}
INPLACE_ENTRIES = {'ops.pq_accumulate', 'ops.confusion_accumulate', 'ops.deform_im2col', 'ops.mod_deform_im2col'}


# returned objects that are handles, not results: what they stand for reaches the comparison through the method named
HANDLES = {
    '_Pending': "PanopticFormatter.submit / InstanceMaskFormatter.submit: the pictures come out of finish(), an entry point of the same cases",
    'PolygonRasters': "rasterize_polygons: the lists come out of PolygonRasters.transitions(), an entry point of the same case",
    'InstanceEvaluator': "score_instance_files: the numbers come out of InstanceEvaluator.last_counts() / summary(), entry points of the same case",
}


def _tensors(obj):
    """Every tensor in what an entry point returned; numpy arrays, numbers, strings and bytes (the summaries and tables of the
    evaluators, the writers' pixels) as tensors too, so that they reach the bitwise comparison of the two patterns."""
    if isinstance(obj, torch.Tensor):
        yield obj
    elif isinstance(obj, np.ndarray):
        if obj.dtype.kind in 'biuf':
            yield torch.from_numpy(np.array(obj, order='C', copy=True).reshape(obj.shape if obj.ndim else (1,)))
        elif obj.dtype.kind == 'O':
            yield from _tensors(obj.tolist())
    elif isinstance(obj, (bool, int, np.integer)):
        yield torch.tensor([int(obj)], dtype=torch.int64)
    elif isinstance(obj, (float, np.floating)):
        yield torch.tensor([float(obj)], dtype=torch.float64)
    elif isinstance(obj, (str, bytes)):
        yield torch.tensor(list(obj.encode() if isinstance(obj, str) else obj), dtype=torch.uint8)
    elif isinstance(obj, collections.abc.Mapping):
        for k in sorted(obj, key=str):
            yield from _tensors(obj[k])
    elif isinstance(obj, collections.abc.Sequence):     # (lists, tuples, the tracker's TrackSegments: looking at them resolves them)
        for o in obj:
            yield from _tensors(o)
    elif obj is not None and type(obj).__name__ not in HANDLES:
        raise TypeError("an entry point returned a %s, which the sweep cannot compare: teach _tensors the type or list it in HANDLES" % type(obj))


def _band(a, pattern):
    if isinstance(a, torch.Tensor) and a.is_cuda and memguard.is_dense(a) and not a.requires_grad:
        b = memguard.banded_copy(a, pattern)
        b.__dict__.update(a.__dict__)          # (e.g. the ROI -> XCD table pyramid_proposals attaches to its rois)
        return b
    if isinstance(a, list) and a and all(isinstance(t, torch.Tensor) for t in a):
        return [_band(t, pattern) for t in a]
    return a


def _recorder(name, fn, pattern, log, calls):
    inplace = name in INPLACE_ENTRIES
    params = [p.name for p in inspect.signature(fn).parameters.values() if p.kind in (p.POSITIONAL_ONLY, p.POSITIONAL_OR_KEYWORD)]

    def wrapped(*args, **kw):
        calls.append(name)
        if not inplace:    # (a written argument is one by its name, passed by keyword or by position)
            args = tuple(a if i < len(params) and params[i] in INPLACE_ARGS else _band(a, pattern) for i, a in enumerate(args))
            kw = {k: (v if k in INPLACE_ARGS else _band(v, pattern)) for k, v in kw.items()}
        ret = fn(*args, **kw)
        region = DEFINED_REGION.get(name)
        for t in _tensors(region(ret, args) if region is not None else ret):
            log.append((name, t.detach().clone()))
        return ret
    return wrapped


_ENTRY_MODULES = {m.rsplit('.', 1)[-1]: m for m in memguard.MODULES}      # 'ops' -> 'upsnet_amd.ops', 'mots' -> 'upsnet_amd.dataset.mots', ...


def _owner(entry):
    """(object holding the entry point, attribute name): the module, or the class of a method."""
    mod, *path = entry.split('.')
    obj = importlib.import_module(_ENTRY_MODULES[mod])
    for p in path[:-1]:
        obj = getattr(obj, p)
    return obj, path[-1]


@contextlib.contextmanager
def _cityscapes_config(tmod):
    """tests/test_pan_combined_gpu.py's fixture of the same name."""
    import copy
    from upsnet_amd.config.config import config
    saved = copy.deepcopy(dict(config))
    config.dataset.num_classes, config.dataset.num_seg_classes = tmod.NUM_CLASSES, tmod.ID_LAST_STUFF + tmod.NUM_CLASSES
    try:
        yield config
    finally:
        config.clear()
        config.update(saved)


@contextlib.contextmanager
def _saved_config():
    """The `saved_config` fixture of the feature test files: the configuration is put back afterwards."""
    import copy
    from upsnet_amd.config.config import config
    saved = copy.deepcopy(dict(config))
    try:
        yield config
    finally:
        config.clear()
        config.update(saved)


_MODEL = {}


def _model_setup():
    """tests/test_model_gpu.py's `setup` fixture (built once, outside any poison)."""
    if 'setup' not in _MODEL:
        from upsnet_amd.config.config import update_config_dict, CITYSCAPES_R50
        update_config_dict(CITYSCAPES_R50)
        from upsnet_amd.synthetic import build_model, make_image
        model, data = build_model(), make_image(256, 512, seed=0, device='cuda')
        graph, model.use_graph = model.use_graph, False
        with torch.no_grad():    # (the first forward of each pipeline packs and caches weights: both patterns then allocate alike)
            for pipeline in ('modules', 'fused'):
                model.pipeline = pipeline
                model(data)
        model.use_graph = graph
        _MODEL['setup'] = (model, data)
    return _MODEL['setup']


def case_call(case, stack, mp):
    """(the case's test function, stand-ins for the fixtures it asks for): `stack` is an ExitStack that the stand-ins live on, `mp`
    a MonkeyPatch on it. Shared with tests/test_abi_contract_gpu.py, which runs the same bodies under another instrument."""
    import pathlib
    from upsnet_amd import ops
    tmod = importlib.import_module(case.module)
    fn = getattr(tmod, case.test)
    args = {}
    for p in inspect.signature(fn).parameters:
        if p in case.kwargs:
            continue
        if p == 'U':
            args[p] = ops
        elif p == 'monkeypatch':
            args[p] = mp
        elif p == 'tmp_path':
            args[p] = pathlib.Path(stack.enter_context(tempfile.TemporaryDirectory()))
        elif p == 'saved_config':
            args[p] = stack.enter_context(_saved_config())
        elif p == 'cityscapes_config':
            args[p] = stack.enter_context(_cityscapes_config(tmod))
        elif p == 'setup':        # (eager: the graph path on poisoned memory is test_fused_forward_on_poisoned_memory_...)
            args[p] = _model_setup()
            args[p][0]._graphs.clear()
            mp.setattr(args[p][0], 'use_graph', False)
        else:
            raise RuntimeError("%s: no stand-in for the fixture %r" % (case.id, p))
    return fn, args


def run_case(case, pattern):
    """The case's test body under `pattern`: returns [(entry point, returned tensor)] and [entry point] in call order, and the number
    of allocations."""
    log, calls = [], []
    with contextlib.ExitStack() as stack:
        mp = stack.enter_context(pytest.MonkeyPatch.context())
        fn, args = case_call(case, stack, mp)
        for e in case.entries:
            owner, name = _owner(e)
            mp.setattr(owner, name, _recorder(e, getattr(owner, name), pattern, log, calls))
        with memguard.poisoned(pattern, adopt=True) as g:      # (a body that poisons its own allocations joins this guard)
            fn(**args, **case.kwargs)
    return log, calls, g.count


@pytest.mark.parametrize('case', CASES, ids=[c.id for c in CASES])
def test_entry_point_on_poisoned_memory(case):
    """The case's own assertions (reference, bound, zero contracts) under patterns A and B, bitwise-equal returned tensors, intact
    bands (memguard.poisoned raises on a written band)."""
    log_a, calls_a, n_a = run_case(case, 'A')
    log_b, calls_b, n_b = run_case(case, 'B')
    assert calls_a, "no entry point of %s was called" % (case.entries,)
    assert set(calls_a) == set(case.entries), "entry points listed but never called: %s" % sorted(set(case.entries) - set(calls_a))
    assert calls_a == calls_b and n_a == n_b, (n_a, n_b)
    assert n_a > 0 or set(calls_a) <= INPLACE_ENTRIES, "nothing was allocated"
    assert [e for e, _ in log_a] == [e for e, _ in log_b]
    for i, ((e, a), (_, b)) in enumerate(zip(log_a, log_b)):
        if not memguard.bit_equal(a, b):
            diff = (memguard.bits(a) != memguard.bits(b)).nonzero().flatten()
            pytest.fail("%s: returned tensor %d (%s %s) differs between poison patterns at bytes %d..%d of %d"
                        % (e, i, tuple(a.shape), a.dtype, int(diff[0]), int(diff[-1]), memguard.bits(a).numel()))


# ------------------------------------------------------------------------------------------------ model-level differential
MODEL_KEYS = ('panoptic_outputs', 'pred_boxes', 'cls_probs', 'cls_inds', 'mask_probs', 'panoptic_cls_inds', 'fcn_outputs')


@pytest.mark.parametrize('preset,h,w', [('CITYSCAPES_R50', 256, 512), ('COCO_R101_DCN', 200, 333)])
def test_fused_forward_on_poisoned_memory_eager_and_graph_replay(preset, h, w):
    """The full fused forward, eager on ordinary memory, then under pattern A and under pattern B through the HIP-graph path (two
    eager visits, the capture, one more replay): every output bitwise equal to the ordinary run, every band intact. The capture
    under poison takes the fill kernels along, so each replay re-poisons its intermediates; model._graphs is cleared around each
    pattern, so that no graph outlives its pattern."""
    cfg = importlib.import_module('upsnet_amd.config.config')
    update_config_dict = cfg.update_config_dict
    update_config_dict(getattr(cfg, preset))
    try:
        from upsnet_amd.synthetic import build_model, make_image
        model = build_model()
        data = make_image(h, w, seed=3, device='cuda')
        with torch.no_grad():
            model.use_graph = False
            model._graphs.clear()
            ref = {k: v.clone() for k, v in model(data).items() if k in MODEL_KEYS}
            assert set(ref) == set(MODEL_KEYS)
            model.use_graph = True
            for pattern in ('A', 'B'):
                model._graphs.clear()
                try:
                    with memguard.poisoned(pattern) as g:
                        # every graph instance: two eager visits, the capture (+ replay), one more replay
                        outs = [{k: v.clone() for k, v in model(data).items() if k in MODEL_KEYS} for _ in range(4 * model.graph_slots)]
                        torch.cuda.synchronize()
                        graphs = sum(1 for e in model._graphs.values() for sl in e['slots'] if 'graph' in sl)
                finally:
                    model._graphs.clear()
                assert graphs == model.graph_slots, "not every HIP graph instance was captured under pattern %s" % pattern
                assert g.count > 100, g.count
                for i, out in enumerate(outs):
                    for k in MODEL_KEYS:
                        assert memguard.bit_equal(out[k], ref[k]), (pattern, i, k)
    finally:
        update_config_dict(cfg.CITYSCAPES_R50)
