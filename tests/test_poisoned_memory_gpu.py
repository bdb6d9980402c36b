"""GPU: every allocating HIP entry point on poisoned, guard-banded memory (tests/memguard.py), and the whole fused forward of both
models on it, eager and as HIP-graph replays.

Each CASES entry runs an op's existing test body -- its edge-shape inputs, its float64 / oracle / golden reference and bound, its zero
contracts ("assert not out[6:].any()", which on poisoned memory now means something) -- twice: under pattern A and under pattern B.
Meanwhile
  * every allocation of the package (outputs, split-K workspaces, weight packs) is poison with guard bands around it,
  * every dense tensor argument of the case's entry points is passed through banded_copy (poison bands around the input),
  * every tensor an entry point returns is recorded; the records of the two patterns must be bitwise equal (only the region
    DEFINED_REGION names, where a header contract leaves the rest undefined),
  * every band must be intact afterwards.
The table is plain data (test module, test function, arguments, entry points): importable without a GPU, so that
tests/test_memguard_cpu.py can check that no allocating entry point is left out.
"""
import collections
import contextlib
import importlib
import os
import sys
import tempfile

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
       ('ops.mask_roi_dedup', 'ops.mask_roi', 'ops.mask_logit_gather')),
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
]

# allocating entry points without a case of their own here, and why
EXCLUDED = {}

# entry point -> (function of (the returned tensors, the positional arguments) -> the tensors whose every bit is defined): where include/upsnet_hip.h leaves part
# of an output undefined, only the defined part is compared between the patterns
def _rows(t, n):
    return [t[p, :int(n[p])] for p in range(t.shape[0])]


DEFINED_REGION = {
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


def _tensors(obj):
    if isinstance(obj, torch.Tensor):
        yield obj
    elif isinstance(obj, (list, tuple)):
        for o in obj:
            yield from _tensors(o)
    elif isinstance(obj, dict):
        for k in sorted(obj, key=str):
            yield from _tensors(obj[k])


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

    def wrapped(*args, **kw):
        calls.append(name)
        if not inplace:
            args = tuple(_band(a, pattern) for a in args)
            kw = {k: (v if k in INPLACE_ARGS else _band(v, pattern)) for k, v in kw.items()}
        ret = fn(*args, **kw)
        region = DEFINED_REGION.get(name)
        for t in _tensors(region(ret, args) if region is not None else ret):
            log.append((name, t.detach().clone()))
        return ret
    return wrapped


_ENTRY_MODULES = {'ops': 'upsnet_amd.ops', 'rle': 'upsnet_amd.dataset.rle', 'coco_eval': 'upsnet_amd.dataset.coco_eval'}


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


def run_case(case, pattern):
    """The case's test body under `pattern`: returns [(entry point, returned tensor)] and [entry point] in call order, and the number
    of allocations."""
    import inspect
    import pathlib
    from upsnet_amd import ops
    tmod = importlib.import_module(case.module)
    fn = getattr(tmod, case.test)
    log, calls = [], []
    with contextlib.ExitStack() as stack:
        mp = stack.enter_context(pytest.MonkeyPatch.context())
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
            elif p == 'cityscapes_config':
                args[p] = stack.enter_context(_cityscapes_config(tmod))
            elif p == 'setup':        # (eager: the graph path on poisoned memory is test_fused_forward_on_poisoned_memory_...)
                args[p] = _model_setup()
                args[p][0]._graphs.clear()
                mp.setattr(args[p][0], 'use_graph', False)
            else:
                raise RuntimeError("%s: no stand-in for the fixture %r" % (case.id, p))
        for e in case.entries:
            owner, name = _owner(e)
            mp.setattr(owner, name, _recorder(e, getattr(owner, name), pattern, log, calls))
        with memguard.poisoned(pattern) as g:
            fn(**args, **case.kwargs)
    return log, calls, g.count


@pytest.mark.parametrize('case', CASES, ids=[c.id for c in CASES])
def test_entry_point_on_poisoned_memory(case):
    """The case's own assertions (reference, bound, zero contracts) under patterns A and B, bitwise-equal returned tensors, intact
    bands (memguard.poisoned raises on a written band)."""
    log_a, calls_a, n_a = run_case(case, 'A')
    log_b, calls_b, n_b = run_case(case, 'B')
    assert calls_a, "no entry point of %s was called" % (case.entries,)
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
