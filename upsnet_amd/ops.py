"""Functional wrappers over the C ABI (tensor plumbing only: allocation, layout views, stream).

Every function here launches hand-written HIP kernels from libupsnet_hip.so on the current torch
stream. Nothing falls back to PyTorch/CPU; non-CUDA inputs raise (as the reference's Functions do,
functions/deform_conv.py:40-41, functions/roialign.py:34-35).
"""
import os

import numpy as np
import torch

from . import _lib
from ._lib import addr, aligned, check, dense, f32c, float_array, i32c, i64c, int_array, lib, nhwc, ptr, ptr_array, ptr_array_unaligned, ptr_unaligned, require_cuda, stream, written


# bench.py sets PROFILE['enabled'] to bracket the dominant kernel with events on the launch stream
PROFILE = {'enabled': False, 'events': []}


def _prof_begin():
    """Start event of one profiled launch, recorded on the launch stream; None (and nothing else done) while profiling is off."""
    if not PROFILE['enabled']:
        return None
    ev0 = torch.cuda.Event(enable_timing=True)
    ev0.record()
    return ev0


def _prof_end(ev0, kind, flops, nbytes, label=None):
    """Record the end event and append (kind, ev0, ev1, algorithmic flops, algorithmic bytes[, label]) to PROFILE['events']."""
    ev1 = torch.cuda.Event(enable_timing=True)
    ev1.record()
    PROFILE['events'].append((kind, ev0, ev1, flops, nbytes) if label is None else (kind, ev0, ev1, flops, nbytes, label))


def cached_pack(owner, slot, tensors, build, *extra):
    """build() cached in owner.__dict__['_hip_plans'][slot], rebuilt when the key changes: (data_ptr, _version, shape) of every tensor
    in `tensors` that is not None, then `extra`. The cache lives on its owner (a module, or the weight tensor itself), never in a
    process-wide dict keyed by id(): the id -- and with the caching allocator even the weight's address -- of a freed model's layer can
    be reused by a different layer of a later model, and a stale pack of another shape makes the kernel read out of bounds. Captured
    HIP graphs hold the addresses of the packs of capture time, so a key must never change between warm-up and replay."""
    key = tuple((t.data_ptr(), t._version, tuple(t.shape)) for t in tensors if t is not None) + extra
    plans = owner.__dict__.setdefault('_hip_plans', {})
    ent = plans.get(slot)
    if ent is None or ent[0] != key:
        ent = plans[slot] = (key, build())
    return ent[1]


def last_kernel_form():
    """Test introspection (include/upsnet_hip.h: upsnet_last_kernel_form): the kernel instance this thread's last library-dispatched
    convolution launch took."""
    return lib().upsnet_last_kernel_form().decode()


def _ws(nbytes, device):
    return torch.empty((int(nbytes),), dtype=torch.uint8, device=device)


# ----------------------------------------------------------------------------- ROIAlign
def roi_align_nchw(features, rois, pooled_h, pooled_w, spatial_scale, sampling_ratio=2):
    """Drop-in for roi_align_cuda.roi_align_forward (NCHW in, [N,C,PH,PW] out)."""
    require_cuda(features, rois)
    features, rois = f32c(features), f32c(rois)
    if rois.dim() != 2 or rois.shape[1] != 5:
        raise RuntimeError("rois must be [N,5]")
    B, C, H, W = features.shape
    N = rois.shape[0]
    out = torch.empty((N, C, pooled_h, pooled_w), dtype=torch.float32, device=features.device)
    check(lib().upsnet_roi_align_forward(stream(), ptr(features), float(spatial_scale), N, H, W, C, int(pooled_h),
                                         int(pooled_w), int(sampling_ratio), ptr(rois), ptr(out)), "roi_align_forward")
    return out


def roi_align_nhwc(features, rois, pooled_h, pooled_w, spatial_scale, sampling_ratio=2):
    """ROIAlign on channels-last features; returns a channels_last [N,C,PH,PW] tensor."""
    require_cuda(features, rois)
    features, rois = nhwc(features.float()), f32c(rois)
    B, C, H, W = features.shape
    N = rois.shape[0]
    out = torch.empty((N, C, pooled_h, pooled_w), dtype=torch.float32, device=features.device,
                      memory_format=torch.channels_last)
    check(lib().upsnet_roi_align_forward_nhwc(stream(), ptr(features), B, H, W, C, float(spatial_scale), ptr(rois), N,
                                              int(pooled_h), int(pooled_w), int(sampling_ratio), ptr(out)),
          "roi_align_forward_nhwc")
    return out


def roi_align_algorithmic_bytes(feats, n, C, ph, pw):
    """the pooled output written once + the ROI records + the feature pixels the ROIs can touch read once (per ROI the
    (2 ph + 1) x (2 pw + 1) sample neighbourhood of its level, capped at the whole pyramid)."""
    feat_bytes = 4 * C * sum(f.shape[2] * f.shape[3] for f in feats)
    return 4.0 * n * C * ph * pw + 20.0 * n + min(feat_bytes, 4.0 * n * C * (2 * ph + 1) * (2 * pw + 1))


# r13: deal the ROIs to the XCDs by image neighbourhood (csrc/roi_order.h). 'auto': launches of >= ROI_XCD_ORDER_MIN ROIs whose rois tensor carries
# the table pyramid_proposals wrote for it (the box head's 1000 proposals). Results are bit-identical either way.
ROI_XCD_ORDER = os.environ.get('UPSNET_ROI_XCD_ORDER', '1') != '0'
ROI_XCD_ORDER_MIN = int(os.environ.get('UPSNET_ROI_XCD_ORDER_MIN', '512'))
# a ROI set that does not come with a table (not straight from pyramid_proposals) gets one from a launch of its own only if this is set: measured
# (profiles/r13_bench.log, random ROIs) the extra launch costs what the dealing saves cold -- 1000 ROIs 63.6 vs 62.7 us, 300 ROIs 28.3 vs 25.2
ROI_XCD_ORDER_STANDALONE = os.environ.get('UPSNET_ROI_XCD_ORDER_STANDALONE', '0') != '0'


def fpn_roi_order(rois, image_hw, num_rois_dev=None):
    """int32 [N]: the workgroup -> ROI table of fpn_roi_align(order=...) that gives every XCD one contiguous range of the ROIs sorted by
    (pyramid level, image stripe, column cell). image_hw: extent of the image the ROIs live in. N <= 2048."""
    require_cuda(rois)
    rois, num_rois_dev = f32c(rois), i32c(num_rois_dev)
    order = torch.empty((max(rois.shape[0], 1),), dtype=torch.int32, device=rois.device)
    check(lib().upsnet_fpn_roi_order(stream(), ptr(rois), int(rois.shape[0]), ptr(num_rois_dev), int(image_hw[0]), int(image_hw[1]), ptr(order)),
          "fpn_roi_order")
    return order[:rois.shape[0]]


def fpn_roi_align(feats, rois, pooled_h, pooled_w, spatial_scale, sampling_ratio=2, num_rois_dev=None,
                  return_levels=False, order='auto'):
    """FPNRoIAlign.forward on device: feats = 4 logical-NCHW tensors (batch 1), rois [N,5].
    order: None = workgroup b takes ROI b; an int32 [N] table from fpn_roi_order; 'auto' = build the table when the launch has at least
    ROI_XCD_ORDER_MIN ROIs (UPSNET_ROI_XCD_ORDER=0 switches it off). Same bits in every case.

    Returns a channels_last [N,C,PH,PW] tensor in the original ROI order."""
    require_cuda(rois, *feats)
    assert len(feats) == 4 and len(spatial_scale) == 4
    feats = [nhwc(f.float()) for f in feats]
    rois, num_rois_dev = f32c(rois), i32c(num_rois_dev)
    C = feats[0].shape[1]
    for f in feats:
        if f.shape[0] != 1 or f.shape[1] != C:
            raise RuntimeError("fpn_roi_align: batch 1 and equal channel counts required")
    N = rois.shape[0]
    dev = rois.device
    out = torch.empty((N, C, pooled_h, pooled_w), dtype=torch.float32, device=dev, memory_format=torch.channels_last)
    levels = torch.empty((max(N, 1),), dtype=torch.int32, device=dev) if return_levels else None
    if isinstance(order, str):
        given = getattr(rois, '_ups_roi_order', None)          # the proposals' own table (pyramid_proposals wrote it: no launch here)
        eligible = ROI_XCD_ORDER and sampling_ratio == 2 and ROI_XCD_ORDER_MIN <= N <= 2048 and max(pooled_h, pooled_w) <= 32
        if eligible and given is not None and given.numel() == N and given.device == rois.device:
            order = given
        elif eligible and ROI_XCD_ORDER_STANDALONE:
            order = fpn_roi_order(rois, (int(round(feats[0].shape[2] / spatial_scale[0])), int(round(feats[0].shape[3] / spatial_scale[0]))), num_rois_dev)
        else:
            order = None
    elif order is not None:
        # (the kernel trusts the table: a table that is not a permutation of 0..N-1 would leave output rows unwritten)
        if not (isinstance(order, torch.Tensor) and order.dtype == torch.int32 and order.numel() == N and order.device == rois.device and order.is_contiguous()):
            raise RuntimeError("fpn_roi_align: order must be a contiguous int32 tensor of %d entries on %s (from fpn_roi_order / pyramid_proposals)" % (N, rois.device))
    ev0 = _prof_begin()
    check(lib().upsnet_fpn_roi_align_forward_ordered(stream(), ptr_array(feats), int_array([f.shape[2] for f in feats]),
                                                     int_array([f.shape[3] for f in feats]), float_array(spatial_scale), C,
                                                     ptr(rois), N, ptr(num_rois_dev), int(pooled_h), int(pooled_w),
                                                     int(sampling_ratio), ptr(out), ptr(levels), ptr(order)), "fpn_roi_align_forward_ordered")
    if ev0 is not None:
        _prof_end(ev0, 'roialign', 0.0, roi_align_algorithmic_bytes(feats, N, C, pooled_h, pooled_w),
                  'roialign %dx%dx%dx%d' % (N, C, pooled_h, pooled_w))
    return (out, levels[:N]) if return_levels else out


# ----------------------------------------------------------------------------- deformable conv
def out_hw(H, W, k, pad, stride, dil):
    return ((H + 2 * pad[0] - dil[0] * (k[0] - 1) - 1) // stride[0] + 1,
            (W + 2 * pad[1] - dil[1] * (k[1] - 1) - 1) // stride[1] + 1)


def deform_im2col(data_im, data_offset, im_shape, col_shape, kernel_shape, pad, stride, dilation, parallel_imgs,
                  deformable_group, data_col):
    """Drop-in for deform_conv_cuda.deform_im2col (deform_conv_cuda.cpp:49-68); fills data_col in place."""
    require_cuda(data_im, data_offset, data_col)
    data_im, data_offset = f32c(data_im), f32c(data_offset)
    written(data_col, torch.float32, "deform_im2col: data_col")
    check(lib().upsnet_deform_im2col(stream(), ptr(data_im), ptr(data_offset), int(im_shape[1]), int(im_shape[2]),
                                     int(im_shape[3]), int(kernel_shape[0]), int(kernel_shape[1]), int(pad[0]), int(pad[1]),
                                     int(stride[0]), int(stride[1]), int(dilation[0]), int(dilation[1]), int(parallel_imgs),
                                     int(deformable_group), ptr(data_col)), "deform_im2col")
    return 1


def mod_deform_im2col(data_im, data_offset, data_mask, im_shape, col_shape, kernel_shape, pad, stride, dilation,
                      deformable_group, data_col):
    """Drop-in for mod_deform_conv_cuda.mod_deform_im2col (mod_deform_conv_cuda.cpp:51-74), batch 1."""
    require_cuda(data_im, data_offset, data_mask, data_col)
    data_im, data_offset, data_mask = f32c(data_im), f32c(data_offset), f32c(data_mask)
    written(data_col, torch.float32, "mod_deform_im2col: data_col")
    check(lib().upsnet_mod_deform_im2col(stream(), ptr(data_im), ptr(data_offset), ptr(data_mask), 1, int(im_shape[1]),
                                         int(im_shape[2]), int(im_shape[3]), int(col_shape[1]), int(col_shape[2]),
                                         int(kernel_shape[0]), int(kernel_shape[1]), int(pad[0]), int(pad[1]),
                                         int(stride[0]), int(stride[1]), int(dilation[0]), int(dilation[1]),
                                         int(deformable_group), ptr(data_col)), "mod_deform_im2col")
    return 1


def _shape_args(im_shape, kernel_shape, pad, stride, dilation):
    return (int(im_shape[1]), int(im_shape[2]), int(im_shape[3]), int(kernel_shape[0]), int(kernel_shape[1]), int(pad[0]),
            int(pad[1]), int(stride[0]), int(stride[1]), int(dilation[0]), int(dilation[1]))


def deform_col2im(data_col, data_offset, im_shape, col_shape, kernel_shape, pad, stride, dilation, parallel_imgs,
                  deformable_group, grad_im):
    """Drop-in for deform_conv_cuda.deform_col2im (deform_conv_cuda.cpp:70-86); accumulates into grad_im."""
    require_cuda(data_col, data_offset, grad_im)
    data_col, data_offset = f32c(data_col), f32c(data_offset)
    written(grad_im, torch.float32, "deform_col2im: grad_im")
    check(lib().upsnet_deform_col2im(stream(), ptr(data_col), ptr(data_offset), *_shape_args(im_shape, kernel_shape, pad, stride,
                                                                                            dilation),
                                     int(parallel_imgs), int(deformable_group), ptr(grad_im)), "deform_col2im")
    return 1


def deform_col2im_coord(data_col, data_im, data_offset, im_shape, col_shape, kernel_shape, pad, stride, dilation,
                        parallel_imgs, deformable_group, grad_offset):
    """Drop-in for deform_conv_cuda.deform_col2im_coord (deform_conv_cuda.cpp:88-105); overwrites grad_offset."""
    require_cuda(data_col, data_im, data_offset, grad_offset)
    data_col, data_im, data_offset = f32c(data_col), f32c(data_im), f32c(data_offset)
    written(grad_offset, torch.float32, "deform_col2im_coord: grad_offset")
    check(lib().upsnet_deform_col2im_coord(stream(), ptr(data_col), ptr(data_im), ptr(data_offset),
                                           *_shape_args(im_shape, kernel_shape, pad, stride, dilation), int(parallel_imgs),
                                           int(deformable_group), ptr(grad_offset)), "deform_col2im_coord")
    return 1


def mod_deform_col2im(data_col, data_offset, data_mask, im_shape, col_shape, kernel_shape, pad, stride, dilation,
                      deformable_group, grad_im):
    """Drop-in for mod_deform_conv_cuda.mod_deform_col2im (mod_deform_conv_cuda.cpp:76-92), batch 1."""
    require_cuda(data_col, data_offset, data_mask, grad_im)
    data_col, data_offset, data_mask = f32c(data_col), f32c(data_offset), f32c(data_mask)
    written(grad_im, torch.float32, "mod_deform_col2im: grad_im")
    a = _shape_args(im_shape, kernel_shape, pad, stride, dilation)
    check(lib().upsnet_mod_deform_col2im(stream(), ptr(data_col), ptr(data_offset), ptr(data_mask), 1, a[0], a[1], a[2],
                                         int(col_shape[1]), int(col_shape[2]), *a[3:], int(deformable_group), ptr(grad_im)),
          "mod_deform_col2im")
    return 1


def mod_deform_col2im_coord(data_col, data_im, data_offset, data_mask, im_shape, col_shape, kernel_shape, pad, stride,
                            dilation, deformable_group, grad_offset, grad_mask):
    """Drop-in for mod_deform_conv_cuda.mod_deform_col2im_coord (mod_deform_conv_cuda.cpp:94-114), batch 1."""
    require_cuda(data_col, data_im, data_offset, data_mask, grad_offset, grad_mask)
    data_col, data_im, data_offset, data_mask = f32c(data_col), f32c(data_im), f32c(data_offset), f32c(data_mask)
    written(grad_offset, torch.float32, "mod_deform_col2im_coord: grad_offset")
    written(grad_mask, torch.float32, "mod_deform_col2im_coord: grad_mask")
    a = _shape_args(im_shape, kernel_shape, pad, stride, dilation)
    check(lib().upsnet_mod_deform_col2im_coord(stream(), ptr(data_col), ptr(data_im), ptr(data_offset), ptr(data_mask), 1, a[0],
                                               a[1], a[2], int(col_shape[1]), int(col_shape[2]), *a[3:], int(deformable_group),
                                               ptr(grad_offset), ptr(grad_mask)), "mod_deform_col2im_coord")
    return 1


def roi_align_backward(pooled_h, pooled_w, sampling_ratio, spatial_scale, top_grad, rois, bottom_grad):
    """Drop-in for roi_align_cuda.roi_align_backward (roi_align_cuda.cpp:77-112); accumulates into bottom_grad [B,C,H,W]."""
    require_cuda(top_grad, rois, bottom_grad)
    if rois.dim() != 2 or rois.shape[1] != 5:
        return 0
    top_grad, rois = f32c(top_grad), f32c(rois)
    written(bottom_grad, torch.float32, "roi_align_backward: bottom_grad")
    B, C, H, W = bottom_grad.shape
    check(lib().upsnet_roi_align_backward(stream(), ptr(top_grad), float(spatial_scale), B, rois.shape[0], H, W, C, int(pooled_h),
                                          int(pooled_w), int(sampling_ratio), ptr(rois), ptr(bottom_grad)), "roi_align_backward")
    return 1


# Deformable-convolution kernel generation: 'frag' = csrc/deform_fused.hip (default), 'igemm' = the first-generation loader mode of
# the dense kernel (csrc/conv.hip), kept for A/B measurements and for geometries the new kernel does not take.
DCN_KERNEL = os.environ.get('UPSNET_DCN_KERNEL', 'frag')


def dcn_precision():
    """'bf16' when the dense convolutions run on the bf16 matrix cores (hipconv.PRECISION == 'bf16', BASELINE configs[2]): the fused
    deformable convolutions then do too (csrc/deform_fused_bf16.hip). 'bf16x3' and 'fp32' keep the exact fp32 kernel."""
    from .models import hipconv
    return 'bf16' if hipconv.PRECISION == 'bf16' and os.environ.get('UPSNET_DCN_BF16', '1') != '0' else 'fp32'


def dcn_square(pad, stride, dil):
    """The fused kernels (both generations) take one pad / stride / dilation for both axes; other geometries run the reference's own
    structure (im2col into a caller-allocated column buffer + one GEMM) through the NCHW drop-in entry point."""
    return pad[0] == pad[1] and stride[0] == stride[1] and dil[0] == dil[1]


def pack_dcn_weight(weight, kind=None):
    """[Cout,Cin,kh,kw] -> packed weight for deform_conv_fused: ('frag', wp) in MFMA fragment order for csrc/deform_fused.hip
    (('frag_bf16', wp) for csrc/deform_fused_bf16.hip: kind 'frag_bf16', or 'frag' while dcn_precision() is 'bf16'), or
    (wpack [kh*kw*Cin, ldw], ldw) -- the dense convolution's packing -- for the first-generation kernel."""
    kind = kind or DCN_KERNEL
    cout, cin, kh, kw = weight.shape
    if kind == 'frag' and dcn_precision() == 'bf16':
        kind = 'frag_bf16'
    if kind == 'frag_bf16' and cin % 32 == 0 and kh * kw <= 25:
        w = f32c(weight)
        wp = torch.empty((lib().upsnet_dcn_packed_weight_bf16_elems(cout, cin, kh, kw),), dtype=torch.bfloat16, device=w.device)
        check(lib().upsnet_dcn_pack_weight_bf16(stream(), ptr(w), cout, cin, kh, kw, ptr(wp)), "dcn_pack_weight_bf16")
        return ('frag_bf16', wp)
    if kind == 'frag' and cin % 32 == 0 and kh * kw <= 25:
        w = f32c(weight)
        wp = torch.empty((lib().upsnet_dcn_packed_weight_floats(cout, cin, kh, kw),), dtype=torch.float32, device=w.device)
        check(lib().upsnet_dcn_pack_weight(stream(), ptr(w), cout, cin, kh, kw, ptr(wp)), "dcn_pack_weight")
        return ('frag', wp)
    return pack_conv_weight(weight)


def cached_dcn_pack(weight):
    """Packed deformable-convolution weight cached ON the weight tensor (re-packed when it changes or moves)."""
    return cached_pack(weight, 'dcn', (weight,), lambda: pack_dcn_weight(weight.detach()), DCN_KERNEL, dcn_precision())


def fused_dcn_supported(cin, cout, deformable_groups, groups, pad=(0, 0), stride=(1, 1), dil=(1, 1)):
    return groups == 1 and deformable_groups == 1 and cin % 32 == 0 and dcn_square(pad, stride, dil)


def _nhwc_out(n, c, h, w, device):
    """channels_last [n,c,h,w] output whose memory is NHWC-dense even for degenerate dims."""
    return torch.empty((n, h, w, c), dtype=torch.float32, device=device).permute(0, 3, 1, 2)


DCN_SPLITK = os.environ.get('UPSNET_DCN_SPLITK', '1') != '0'


def dcn_ksplit(outs, cin, cout, taps):
    """Split-K factor of the fused deformable kernel for one small map: enough workgroups for ~2 per CU (~3 for the smallest maps), >= 9 K steps each."""
    if not DCN_SPLITK or cout % 4:
        return 1
    o = outs[0]
    wgs = o.shape[0] * -(-o.shape[2] // 8) * -(-o.shape[3] // 8) * -(-cout // 128)
    nsl = cin // 32 * taps
    # (r13) maps of <= 128 tiles (res5 of UPSNet-101-DCN: 96 at 800x1333, 128 at 1024x2048) split until ~3 workgroups per CU: 512 -> 512 on 25 x 42
    # x4 86.8, x6 84.3, x8 68.6 us (tools/bench_c3_layers.py); larger maps are flat beyond 384 workgroups (256 -> 256 on 50 x 84: x3 64.0, x4 68.3, x6 64.0)
    target = 768 if wgs <= 128 else 384
    ks = 1
    while ks < 8 and wgs * ks < target and nsl // (ks + 1) >= 9:
        ks += 1
    while ks > 1 and -(-nsl // ks) * (ks - 1) >= nsl:
        ks -= 1
    return ks


def deform_conv_fused(xs, offsets, wpack, bias, cin, cout, ksize, stride, pad, dil, masks=None, relu=False):
    """Fused deformable conv over up to 4 maps sharing weights. xs/offsets/masks: lists of logical NCHW
    tensors with batch 1; wpack = (packed weight, ldw) from pack_dcn_weight; returns channels_last outputs."""
    wp, ldw = wpack     # ('frag', packed) or (packed, ldw)
    require_cuda(ldw if isinstance(wp, str) else wp, *xs)
    if isinstance(wp, str):
        ldw = dense(ldw) if wp == 'frag_bf16' else f32c(ldw)
    else:
        wp = f32c(wp)
    n = len(xs)
    assert 1 <= n <= 4 and len(offsets) == n
    xs = [nhwc(x.float()) for x in xs]
    offsets = [nhwc(o.float()) for o in offsets]
    if masks is not None:
        masks = [nhwc(m.float()) for m in masks]
    outs = []
    for x, o in zip(xs, offsets):
        if x.shape[0] != 1 or x.shape[1] != cin:
            raise RuntimeError("deform_conv_fused: batch 1 / Cin mismatch")
        Ho, Wo = out_hw(x.shape[2], x.shape[3], ksize, pad, stride, dil)
        if tuple(o.shape) != (1, 2 * ksize[0] * ksize[1], Ho, Wo):
            raise RuntimeError("deform_conv_fused: offset shape %s != %s" % (tuple(o.shape), (1, 2 * ksize[0] * ksize[1], Ho, Wo)))
        outs.append(_nhwc_out(1, cout, Ho, Wo, x.device))
    b = None if bias is None else f32c(bias)
    ev0 = _prof_begin()
    if wp == 'frag_bf16':   # bf16 matrix cores (BASELINE configs[2])
        if not (pad[0] == pad[1] and stride[0] == stride[1] and dil[0] == dil[1]):
            raise RuntimeError("deform_conv_fused: square pad / stride / dilation only")
        check(lib().upsnet_deform_conv_fused_nhwc_bf16(stream(), n, ptr_array(xs), ptr_array(offsets),
                                                       ptr_array(masks) if masks is not None else None, ptr_array(outs),
                                                       int_array([x.shape[2] for x in xs]), int_array([x.shape[3] for x in xs]),
                                                       int(cin), int(cout), ksize[0], ksize[1], pad[0], stride[0], dil[0], ptr(ldw), ptr(b),
                                                       int(bool(relu))), "deform_conv_fused_nhwc_bf16")
    elif wp == 'frag':   # (kind, packed) from pack_dcn_weight: second-generation kernel
        if not (pad[0] == pad[1] and stride[0] == stride[1] and dil[0] == dil[1]):
            raise RuntimeError("deform_conv_fused: square pad / stride / dilation only")
        ks = dcn_ksplit(outs, cin, cout, ksize[0] * ksize[1]) if n == 1 else 1
        if ks > 1:
            wsb = lib().upsnet_deform_conv_fused_splitk_workspace_bytes(xs[0].shape[2], xs[0].shape[3], int(cout), ksize[0], ksize[1], pad[0],
                                                                        stride[0], dil[0], ks)
            ws = _ws(wsb, xs[0].device)
            check(lib().upsnet_deform_conv_fused_nhwc_splitk(stream(), ptr(xs[0]), ptr(offsets[0]), ptr(masks[0]) if masks is not None else None,
                                                             ptr(outs[0]), xs[0].shape[2], xs[0].shape[3], int(cin), int(cout), ksize[0],
                                                             ksize[1], pad[0], stride[0], dil[0], ptr(ldw), ptr(b), int(bool(relu)), ks, ptr(ws)),
                  "deform_conv_fused_nhwc_splitk")
        else:
            check(lib().upsnet_deform_conv_fused_nhwc(stream(), n, ptr_array(xs), ptr_array(offsets),
                                                      ptr_array(masks) if masks is not None else None, ptr_array(outs),
                                                      int_array([x.shape[2] for x in xs]), int_array([x.shape[3] for x in xs]),
                                                      int(cin), int(cout), ksize[0], ksize[1], pad[0], stride[0], dil[0], ptr(ldw), ptr(b),
                                                      int(bool(relu))), "deform_conv_fused_nhwc")
    else:
        check(lib().upsnet_deform_conv_forward_nhwc(stream(), n, ptr_array(xs), ptr_array(offsets),
                                                    ptr_array(masks) if masks is not None else None, ptr_array(outs),
                                                    int_array([x.shape[2] for x in xs]), int_array([x.shape[3] for x in xs]),
                                                    int(cin), int(cout), ksize[0], ksize[1], pad[0], pad[1], stride[0], stride[1],
                                                    dil[0], dil[1], 1, ptr(wp), int(ldw), ptr(b), int(bool(relu))),
              "deform_conv_forward_nhwc")
    if ev0 is not None:
        npix = sum(o.shape[2] * o.shape[3] for o in outs)
        taps = ksize[0] * ksize[1]
        _prof_end(ev0, 'dcn_fused_bf16' if wp == 'frag_bf16' else 'dcn_fused', 2.0 * cout * cin * taps * npix,
                  4.0 * (sum(x.shape[2] * x.shape[3] for x in xs) * cin + npix * (2 * taps + cout) + cout * cin * taps),
                  "dcn %d->%d %s" % (cin, cout, [tuple(x.shape[2:]) for x in xs]))
    return outs


# ----------------------------------------------------------------------------- NMS
def nms_host(sorted_dets, thresh, device_id=0):
    """`_nms` drop-in: numpy float32 [N,>=4] sorted by score -> kept indices (numpy int32)."""
    d = np.ascontiguousarray(sorted_dets, dtype=np.float32)
    n = d.shape[0]
    keep = np.zeros((max(n, 1),), np.int32)
    num = np.zeros((1,), np.int32)
    check(lib().upsnet_nms_host(keep.ctypes.data_as(_lib.c_void_p), num.ctypes.data_as(_lib.c_void_p),
                                d.ctypes.data_as(_lib.c_void_p), n, d.shape[1] if d.ndim == 2 else 5, float(thresh),
                                int(device_id)), "nms_host")
    return keep[:int(num[0])]


def nms_batched(boxes, scores, counts, thresh, pre_removed=None):
    """boxes [P,nmax,4], scores [P,nmax], counts [P] int32 (device) -> keep_idx [P,nmax] int32, keep_cnt [P]."""
    require_cuda(boxes, scores, counts)
    boxes, scores = f32c(boxes), f32c(scores)
    counts = i32c(counts)
    Pn, nmax = scores.shape
    dev = boxes.device
    keep = torch.empty((Pn, nmax), dtype=torch.int32, device=dev)
    cnt = torch.empty((Pn,), dtype=torch.int32, device=dev)
    ws = _ws(lib().upsnet_nms_workspace_bytes(Pn, nmax), dev)
    pr = None if pre_removed is None else dense(pre_removed.to(torch.uint8))
    check(lib().upsnet_nms_batched(stream(), ptr(boxes), ptr(scores), ptr(counts), ptr(pr), Pn, nmax, float(thresh),
                                   ptr(keep), ptr(cnt), ptr(ws)), "nms_batched")
    return keep, cnt


def gpu_nms(dets, thresh):
    """gpu_nms (gpu_nms.pyx:23-38) on a device tensor [N,5]; returns a device int64 tensor of kept indices
    (visiting order). One tiny D2H (the count) to size the result."""
    require_cuda(dets)
    dets = f32c(dets)
    n = dets.shape[0]
    if n == 0:
        return torch.zeros((0,), dtype=torch.int64, device=dets.device)
    counts = torch.full((1,), n, dtype=torch.int32, device=dets.device)
    keep, cnt = nms_batched(dets[None, :, :4], dets[None, :, 4], counts, thresh)
    return keep[0, :int(cnt.item())].long()


def cpu_nms(dets, thresh):
    """cpu_nms (cpu_nms.pyx:29-80) on a device tensor [N,5]: like gpu_nms but suppression at `overlap >= thresh` (double compare)."""
    require_cuda(dets)
    dets = f32c(dets)
    n = dets.shape[0]
    if n == 0:
        return torch.zeros((0,), dtype=torch.int64, device=dets.device)
    counts = torch.full((1,), n, dtype=torch.int32, device=dets.device)
    boxes, scores = f32c(dets[None, :, :4]), f32c(dets[None, :, 4])
    keep = torch.empty((1, n), dtype=torch.int32, device=dets.device)
    cnt = torch.empty((1,), dtype=torch.int32, device=dets.device)
    ws = _ws(lib().upsnet_nms_workspace_bytes(1, n), dets.device)
    check(lib().upsnet_cpu_nms_batched(stream(), ptr(boxes), ptr(scores), ptr(counts), 1, n, float(thresh), ptr(keep), ptr(cnt),
                                       ptr(ws)), "cpu_nms_batched")
    return keep[0, :int(cnt.item())].long()


def soft_nms_batched(boxes, counts=None, sigma=0.5, Nt=0.3, threshold=0.001, method=0):
    """P soft-NMS problems in one launch (one workgroup each): boxes [P,nmax,5] (x1,y1,x2,y2,score), counts [P] int32 device or
    None. Returns (boxes' [P,nmax,5], inds [P,nmax] int64, n_out [P] int32), all on the device: rows [0, n_out[p]) of problem p are
    cpu_soft_nms's result (cpu_nms.pyx:91-196), the rest is unspecified."""
    require_cuda(boxes)
    b = f32c(boxes).clone()
    Pn, nmax = b.shape[0], b.shape[1]
    inds = torch.empty((Pn, max(nmax, 1)), dtype=torch.int64, device=b.device)
    n_out = torch.zeros((max(Pn, 1),), dtype=torch.int32, device=b.device)
    if Pn and nmax:
        cnt = None if counts is None else i32c(counts.to(device=b.device))
        ws = _ws(lib().upsnet_soft_nms_batched_workspace_bytes(Pn, nmax), b.device)
        check(lib().upsnet_soft_nms_batched(stream(), ptr(b), ptr(inds), ptr(cnt), Pn, nmax, float(sigma), float(Nt), float(threshold),
                                            int(method), ptr(n_out), ptr(ws)), "soft_nms_batched")
    return b, inds[:, :nmax], n_out[:Pn]


def soft_nms(boxes, sigma=0.5, Nt=0.3, threshold=0.001, method=0):
    """cpu_soft_nms semantics on device: returns (boxes', inds[:N'])."""
    require_cuda(boxes)
    b, inds, n_out = soft_nms_batched(f32c(boxes)[None], None, sigma, Nt, threshold, method)
    return b[0], inds[0, :int(n_out[0].item())] if boxes.shape[0] else inds[0, :0]


# ----------------------------------------------------------------------------- proposals
def pyramid_proposals(cls_probs, bbox_preds, im_info, anchors, strides, pre_nms_top_n, post_nms_top_n, nms_thresh,
                      min_size, joint=False):
    """Device-side PyramidProposal. cls_probs[l] [1,A,H,W], bbox_preds[l] [1,4A,H,W]; im_info device [3].
    Returns fixed-size (rois [post,5], scores [post], num device int32). joint = the individual_proposals=False branch
    (functions/pyramid_proposal.py:181-208): kept boxes in NMS order, before the reference's random padding.
    A channel slice of a wider map is read in place, wherever it starts (element-aligned: the kernels read one float per access)."""
    require_cuda(im_info, *cls_probs)
    L = len(cls_probs)

    def pixel_linear(t):
        """(tensor, channel stride, pixel stride) if (c, h, w) -> c*cs + (h*W + w)*ps addresses t in place (NCHW, or a channel
        slice of an NHWC map), else a contiguous NCHW copy."""
        if t.dtype == torch.float32 and t.shape[0] == 1 and (t.shape[2] == 1 or t.stride(2) == t.shape[3] * t.stride(3)):
            return t, t.stride(1), t.stride(3)
        t = f32c(t)
        return t, t.stride(1), t.stride(3)
    cls_probs, cls_cs, cls_ps = zip(*[pixel_linear(c) for c in cls_probs])
    bbox_preds, box_cs, box_ps = zip(*[pixel_linear(b) for b in bbox_preds])
    A = cls_probs[0].shape[1]
    Hs = [c.shape[2] for c in cls_probs]
    Ws = [c.shape[3] for c in cls_probs]
    for c, b in zip(cls_probs, bbox_preds):
        if c.shape[0] != 1 or b.shape[1] != 4 * A:
            raise ValueError("Sorry, multiple images each device is not implemented")  # pyramid_proposal.py:47-49
    dev = im_info.device
    hs, ws_ = int_array(Hs), int_array(Ws)
    nbytes = lib().upsnet_proposal_workspace_bytes(L, hs, ws_, A, int(pre_nms_top_n), int(post_nms_top_n))
    if nbytes == 0:
        raise RuntimeError("pyramid_proposals: unsupported level count")
    ws = _ws(nbytes, dev)
    rois = torch.empty((post_nms_top_n, 5), dtype=torch.float32, device=dev)
    scores = torch.empty((post_nms_top_n,), dtype=torch.float32, device=dev)
    num = torch.empty((1,), dtype=torch.int32, device=dev)
    anc = float_array(np.asarray(anchors, np.float32).reshape(-1).tolist())
    long_array = lambda v: (_lib.c_long * len(v))(*[int(x) for x in v])
    im_info = f32c(im_info)
    args = (stream(), L, ptr_array_unaligned(cls_probs), ptr_array_unaligned(bbox_preds), long_array(cls_cs), long_array(cls_ps), long_array(box_cs), long_array(box_ps),
            hs, ws_, int_array(strides), anc, A, ptr(im_info), int(pre_nms_top_n), int(post_nms_top_n), float(nms_thresh), float(min_size),
            ptr(rois), ptr(scores), ptr(num), ptr(ws))
    if joint:
        check(lib().upsnet_pyramid_proposals_joint_strided(*args), "pyramid_proposals")
    else:
        # r13: the launch that ranks the proposals also writes the ROI -> XCD dealing table of the box head's ROIAlign launch (csrc/roi_order.h);
        # it travels with the rois tensor (fpn_roi_align(order='auto') picks it up when it is handed this very tensor)
        order = torch.empty((post_nms_top_n,), dtype=torch.int32, device=dev) if (ROI_XCD_ORDER and ROI_XCD_ORDER_MIN <= post_nms_top_n <= 2048) else None
        check(lib().upsnet_pyramid_proposals_strided_ordered(*args, ptr(order)), "pyramid_proposals")
        if order is not None:
            rois._ups_roi_order = order
    return rois, scores, num


# ----------------------------------------------------------------------------- detection selection
def mask_roi(rois, bbox_delta, cls_prob, im_info, class_agnostic, score_thresh, nms_thresh, max_det, reg_weights,
             num_rois_dev=None, clip_boxes=True):
    """Device-side MaskROI: returns fixed-capacity (boxes [cap,5], scores [cap], cls [cap] int64, src [cap] int32,
    num device int32)."""
    require_cuda(rois, bbox_delta, cls_prob, im_info)
    rois, bbox_delta, cls_prob = f32c(rois), f32c(bbox_delta), f32c(cls_prob)
    N, C = cls_prob.shape
    dev = rois.device
    cap = lib().upsnet_mask_roi_capacity(N, C, int(class_agnostic))
    boxes = torch.empty((cap, 5), dtype=torch.float32, device=dev)
    scores = torch.empty((cap,), dtype=torch.float32, device=dev)
    cls = torch.empty((cap,), dtype=torch.int64, device=dev)
    src = torch.empty((cap,), dtype=torch.int32, device=dev)
    num = torch.empty((1,), dtype=torch.int32, device=dev)
    ws = _ws(lib().upsnet_mask_roi_workspace_bytes(N, C, int(class_agnostic)), dev)
    im_info, num_rois_dev = f32c(im_info.reshape(-1)), i32c(num_rois_dev)
    check(lib().upsnet_mask_roi_ex(stream(), ptr(rois), ptr(bbox_delta), ptr(cls_prob), N, ptr(num_rois_dev), C,
                                ptr(im_info), int(class_agnostic), int(bool(clip_boxes)), float(score_thresh), float(nms_thresh),
                                int(max_det), float_array(reg_weights), ptr(boxes), ptr(scores), ptr(cls), ptr(src),
                                ptr(num), ptr(ws)), "mask_roi")
    return boxes, scores, cls, src, num


def mask_logit_gather(mask_logit, row, cls, K=None):
    """pan_logit [K,1,ms,ms] with pan_logit[k] = mask_logit[row[k], cls[k]] (rows / classes clamped): one gather kernel instead of
    clamp + index_select + expand + gather. mask_logit: [n,C,ms,ms] in any dense layout (NCHW or channels_last); it may start anywhere
    in an allocation (element-aligned: the kernel reads one float per access), every other tensor is held to 16 bytes."""
    require_cuda(mask_logit, row, cls)
    n, C, mh, mw = mask_logit.shape
    t = mask_logit if mask_logit.dtype == torch.float32 else mask_logit.float()
    if not (t.stride(2) == mw * t.stride(3)):
        t = dense(t)
    K = row.shape[0] if K is None else int(K)
    out = torch.empty((K, 1, mh, mw), dtype=torch.float32, device=t.device)
    row, cls = i32c(row), i64c(cls)      # (bound before the call: a temporary's block is free again once ptr() returns)
    check(lib().upsnet_mask_logit_gather(stream(), ptr_unaligned(t), n, C, mh * mw, t.stride(0), t.stride(1), t.stride(3),
                                         ptr(row), ptr(cls), K, ptr(out)),
          "mask_logit_gather")
    return out


# ----------------------------------------------------------------------------- panoptic head
def mask_removal(mask_rois4, cls_prob, mask_logit, cls_idx, num_thing_classes, im_shape, fraction_threshold=0.3, m_dev=None):
    """Device-side MaskRemoval selection. Returns (keep_inds [m] int64, num_keep, real_keep) device tensors.
    m_dev: optional device int32 count of valid rows (the arrays then have fixed capacity m)."""
    require_cuda(mask_rois4, cls_prob, mask_logit, cls_idx)
    mask_rois4, cls_prob = f32c(mask_rois4), f32c(cls_prob).reshape(-1)
    m = mask_rois4.shape[0]
    mask_logit = f32c(mask_logit).reshape(m, -1)
    ms = int(round(mask_logit.shape[1] ** 0.5))
    cls_idx, m_dev = i64c(cls_idx).reshape(-1), i32c(m_dev)
    H, W = int(im_shape[0]), int(im_shape[1])
    dev = mask_rois4.device
    keep = torch.empty((m,), dtype=torch.int64, device=dev)   # (the finalize kernel zero-fills the rows past the count)
    num = torch.empty((1,), dtype=torch.int32, device=dev)
    real = torch.empty((1,), dtype=torch.int32, device=dev)
    ws = _ws(lib().upsnet_mask_removal_workspace_bytes(m, num_thing_classes, H, W), dev)
    check(lib().upsnet_mask_removal(stream(), ptr(mask_rois4), ptr(cls_prob), ptr(mask_logit), ptr(cls_idx), m, ptr(m_dev), ms,
                                    int(num_thing_classes), H, W, float(fraction_threshold), ptr(keep), ptr(num), ptr(real),
                                    ptr(ws)), "mask_removal")
    return keep, num, real


def panoptic_tail_pack(keep, num_keep, cls, scores, det_num, pan_num, extra_num):
    """(kept_cls, kept_scores, counters[4] int32) of the fixed-capacity tail in one launch: cls / scores gathered at the kept rows
    (rows past num_keep read row 0) and {det_num, pan_num, extra_num, num_keep} packed for the single host read."""
    require_cuda(keep, cls, scores)
    K = int(cls.shape[0])
    cls, scores = i64c(cls).reshape(-1), f32c(scores).reshape(-1)
    keep, num_keep, det_num, pan_num, extra_num = i64c(keep), i32c(num_keep), i32c(det_num), i32c(pan_num), i32c(extra_num)
    kept_cls = torch.empty((K,), dtype=torch.int64, device=cls.device)
    kept_scores = torch.empty((K,), dtype=torch.float32, device=cls.device)
    counters = torch.empty((4,), dtype=torch.int32, device=cls.device)
    check(lib().upsnet_panoptic_tail_pack(stream(), ptr(keep), ptr(num_keep), K, ptr(cls), ptr(scores), ptr(det_num), ptr(pan_num),
                                          ptr(extra_num), ptr(kept_cls), ptr(kept_scores), ptr(counters)), "panoptic_tail_pack")
    return kept_cls, kept_scores, counters


def mask_paste(mask_rois4, mask_logit, keep, num, real, k, im_shape):
    require_cuda(mask_rois4, mask_logit)
    mask_rois4 = f32c(mask_rois4)
    m = mask_rois4.shape[0]
    mask_logit = f32c(mask_logit).reshape(m, -1)
    ms = int(round(mask_logit.shape[1] ** 0.5))
    H, W = int(im_shape[0]), int(im_shape[1])
    out = torch.empty((1, k, H, W), dtype=torch.float32, device=mask_rois4.device)
    keep, num, real = i64c(keep), i32c(num), i32c(real)
    check(lib().upsnet_mask_paste(stream(), ptr(mask_rois4), ptr(mask_logit), ptr(keep), ptr(num), ptr(real), int(k), ms, H, W,
                                  ptr(out)), "mask_paste")
    return out


def seg_term(fcn_output, boxes4, cls, class_map):
    require_cuda(fcn_output, boxes4, cls, class_map)
    fcn = f32c(fcn_output)
    _, S, H, W = fcn.shape
    boxes4 = f32c(boxes4)
    k = boxes4.shape[0]
    out = torch.empty((1, k, H, W), dtype=torch.float32, device=fcn.device)
    cls, class_map = i64c(cls), i64c(class_map)
    check(lib().upsnet_seg_term(stream(), ptr(fcn), S, H, W, ptr(boxes4), ptr(cls), ptr(class_map), k, ptr(out)), "seg_term")
    return out


def panoptic_argmax(fcn_output, num_stuff, seg_inst, mask_energy, enable_void=True):
    require_cuda(fcn_output, seg_inst, mask_energy)
    fcn, seg_inst, mask_energy = f32c(fcn_output), f32c(seg_inst), f32c(mask_energy)
    _, S, H, W = fcn.shape
    k = seg_inst.shape[1]
    pan = torch.empty((1, H, W), dtype=torch.int64, device=fcn.device)
    check(lib().upsnet_panoptic_argmax(stream(), ptr(fcn), S, H, W, int(num_stuff), ptr(seg_inst), ptr(mask_energy), k,
                                       int(bool(enable_void)), ptr(pan)), "panoptic_argmax")
    return pan


def panoptic_fuse(fcn_output, num_stuff, mask_rois5, mask_logit, cls_idx, keep, num, real, class_map, enable_void=True,
                  want_sem=True):
    """Fused head: returns (panoptic [1,H,W] int64, semantic argmax [1,H,W] int64 or None)."""
    require_cuda(fcn_output, mask_rois5, mask_logit, cls_idx)
    fcn = f32c(fcn_output)
    _, S, H, W = fcn.shape
    mask_rois5 = f32c(mask_rois5)
    m = mask_rois5.shape[0]
    if m > 256:   # the kernels keep their instance table in LDS (FUSE_MAXK); more rows would be dropped silently
        raise RuntimeError("panoptic_fuse: at most 256 instance rows (got %d); use mask_paste + seg_term + panoptic_argmax" % m)
    mask_logit = f32c(mask_logit).reshape(m, -1)
    ms = int(round(mask_logit.shape[1] ** 0.5))
    pan = torch.empty((1, H, W), dtype=torch.int64, device=fcn.device)
    sem = torch.empty((1, H, W), dtype=torch.int64, device=fcn.device) if want_sem else None
    cls_idx, keep, num, real, class_map = i64c(cls_idx), i64c(keep), i32c(num), i32c(real), i64c(class_map)
    check(lib().upsnet_panoptic_fuse(stream(), ptr(fcn), S, H, W, int(num_stuff), ptr(mask_rois5), ptr(mask_logit),
                                     ptr(cls_idx), ptr(keep), ptr(num), ptr(real), int(min(m, 256)),
                                     ms, ptr(class_map), int(bool(enable_void)), ptr(pan), ptr(sem)), "panoptic_fuse")
    return pan, sem


# ----------------------------------------------------------------------------- dense convolution (fp32 MFMA implicit GEMM)
def conv_supported(cin, kh, kw, groups=1, dilation=(1, 1)):
    return groups == 1 and tuple(dilation) == (1, 1) and cin % 32 == 0 and kh == kw and kh * kw <= 49


def pack_conv_weight(weight):
    """[Cout,Cin,kh,kw] -> ([kh*kw*Cin, ldw], ldw) with ldw = Cout rounded up to 32 (zero padded columns)."""
    require_cuda(weight)
    weight = f32c(weight)
    Cout, Cin, kh, kw = weight.shape
    ldw = (Cout + 31) // 32 * 32
    wp = torch.empty((kh * kw * Cin, ldw), dtype=torch.float32, device=weight.device)
    check(lib().upsnet_conv_pack_weight(stream(), ptr(weight), Cout, Cin, kh, kw, ldw, ptr(wp)), "conv_pack_weight")
    return wp, ldw


def conv2d_nhwc_multi(xs, wpack, ldw, bias, cout, ksize, stride, pad, relu=False, residuals=None, residual_up=False):
    """Up to 5 logical-NCHW tensors through the SAME convolution in one launch; returns channels_last outputs.
    out_i = relu?(conv(x_i) + bias + residual_i); residual_up: residual_i is at half resolution and is added through
    a nearest x2 upsampling (FPN top-down path)."""
    require_cuda(wpack, *xs)
    wpack = f32c(wpack)
    assert 1 <= len(xs) <= 5
    xs = [nhwc(x.float()) for x in xs]
    cin = xs[0].shape[1]
    outs, ress = [], None
    shapes = []
    for x in xs:
        N, C, H, W = x.shape
        if C != cin:
            raise RuntimeError("conv2d_nhwc_multi: channel mismatch")
        shapes.append((N, (H + 2 * pad - ksize) // stride + 1, (W + 2 * pad - ksize) // stride + 1, cout))
    # the outputs of a multi-map launch are carved from ONE allocation (outs[0]._ups_flat), so that a following elementwise op over
    # all maps (the RPN's sigmoid over 5 levels) is one launch over the flat buffer instead of one per map
    # (every map starts on a 256-byte boundary of the flat buffer, whatever its channel count: 15-channel RPN heads, 18 / 27-channel
    # offset maps -- a later 16-byte-per-lane consumer must not see a 4-byte-aligned base)
    sizes = [n * h * w * c for n, h, w, c in shapes]
    starts, off = [], 0
    for sz in sizes:
        starts.append(off)
        off += (sz + 63) // 64 * 64
    flat = torch.empty((off,), dtype=torch.float32, device=xs[0].device)
    for (n, h, w, c), sz, st in zip(shapes, sizes, starts):
        outs.append(flat[st:st + sz].view(n, h, w, c).permute(0, 3, 1, 2))
    outs[0]._ups_flat = flat
    if residuals is not None:
        ress = [nhwc(r.float()) for r in residuals]
        for r, o in zip(ress, outs):
            want = (o.shape[0], o.shape[1], o.shape[2] // 2, o.shape[3] // 2) if residual_up else tuple(o.shape)
            if tuple(r.shape) != want or (residual_up and (o.shape[2] % 2 or o.shape[3] % 2)):
                raise RuntimeError("conv2d_nhwc: residual shape %s != %s" % (tuple(r.shape), want))
    ev0 = _prof_begin()
    bias = None if bias is None else f32c(bias)
    check(lib().upsnet_conv2d_nhwc_f32(stream(), len(xs), ptr_array(xs), ptr_array(ress) if ress is not None else None,
                                       ptr_array(outs), int_array([x.shape[0] for x in xs]), int_array([x.shape[2] for x in xs]),
                                       int_array([x.shape[3] for x in xs]), int(cin), ptr(wpack), int(ldw),
                                       ptr(bias), int(cout), int(ksize), int(ksize), int(stride),
                                       int(pad), int(bool(relu)), int(bool(residual_up and ress is not None))), "conv2d_nhwc_f32")
    if ev0 is not None:
        npix = sum(o.shape[0] * o.shape[2] * o.shape[3] for o in outs)
        nin = sum(x.shape[0] * x.shape[2] * x.shape[3] for x in xs)
        _prof_end(ev0, 'conv', 2.0 * cout * cin * ksize * ksize * npix,
                  4.0 * (cin * nin + cout * npix * (2 if ress is not None else 1) + cout * cin * ksize * ksize),
                  "direct %dx%d/%d %d->%d %s%s" % (ksize, ksize, stride, cin, cout, [tuple(x.shape[0:1] + x.shape[2:]) for x in xs],
                                                    " +res" if ress is not None else ""))
    return outs


def conv2d_nhwc_multiw(xs, wpacks, ldw, cout, ksize, stride, pad, relu=False):
    """Up to 5 maps through the same convolution GEOMETRY, each with its own packed weights, in one launch (no bias / residual)."""
    require_cuda(*xs, *wpacks)
    wpacks = [f32c(w) for w in wpacks]
    assert 1 <= len(xs) <= 5 and len(wpacks) == len(xs)
    xs = [nhwc(x.float()) for x in xs]
    cin = xs[0].shape[1]
    outs = [_nhwc_out(x.shape[0], cout, (x.shape[2] + 2 * pad - ksize) // stride + 1, (x.shape[3] + 2 * pad - ksize) // stride + 1, x.device)
            for x in xs]
    ev0 = _prof_begin()
    check(lib().upsnet_conv2d_nhwc_f32_multiw(stream(), len(xs), ptr_array(xs), ptr_array(outs), int_array([x.shape[0] for x in xs]),
                                              int_array([x.shape[2] for x in xs]), int_array([x.shape[3] for x in xs]), int(cin),
                                              ptr_array(wpacks), int(ldw), int(cout), int(ksize), int(ksize), int(stride), int(pad),
                                              int(bool(relu))), "conv2d_nhwc_f32_multiw")
    if ev0 is not None:
        npix = sum(o.shape[0] * o.shape[2] * o.shape[3] for o in outs)
        nin = sum(x.shape[0] * x.shape[2] * x.shape[3] for x in xs)
        _prof_end(ev0, 'conv', 2.0 * cout * cin * ksize * ksize * npix, 4.0 * (cin * nin + cout * npix + len(xs) * cout * cin * ksize * ksize),
                  "direct %dx%d/%d %d->%d %s per-map weights" % (ksize, ksize, stride, cin, cout, [tuple(x.shape[2:]) for x in xs]))
    return outs


def conv2d_nhwc(x, wpack, ldw, bias, cout, ksize, stride, pad, relu=False, residual=None, residual_up=False):
    """x: logical NCHW tensor (any batch); returns a channels_last [N,Cout,Ho,Wo] tensor.
    out = relu?(conv(x) + bias + residual) in one kernel."""
    return conv2d_nhwc_multi([x], wpack, ldw, bias, cout, ksize, stride, pad, relu, None if residual is None else [residual],
                             residual_up)[0]


def pack_conv1x1_weight(weight):
    """[Cout,Cin,1,1] -> fragment-order pack for conv1x1_frag (csrc/conv1x1.hip; the layout of csrc/deform_fused.hip with one tap)."""
    require_cuda(weight)
    w = f32c(weight)
    cout, cin = w.shape[0], w.shape[1]
    wp = torch.empty((lib().upsnet_dcn_packed_weight_floats(cout, cin, 1, 1),), dtype=torch.float32, device=w.device)
    check(lib().upsnet_dcn_pack_weight(stream(), ptr(w), cout, cin, 1, 1, ptr(wp)), "dcn_pack_weight")
    return wp


def conv1x1_frag(x, wpack, bias, cout, stride=1, relu=False, residual=None, residual_up=False, out=None, ksplit=1):
    """1x1 convolution (stride 1 / 2) on the lean fp32 MFMA GEMM kernel of csrc/conv1x1.hip: out = relu?(conv(x) + bias + residual),
    residual_up: the residual is at half resolution and is added through a nearest x2 upsampling (FPN top-down path).
    x: logical NCHW (any batch), returns channels_last [N,Cout,Ho,Wo]. out: caller-provided channels_last output (a view of a larger
    tensor); ksplit > 1: the K walk of every tile split over ksplit workgroups + the reduce kernel (no residual_up)."""
    require_cuda(wpack, x)
    wpack = f32c(wpack)
    x = nhwc(x.float())
    N, cin, H, W = x.shape
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    if out is None:
        out = _nhwc_out(N, cout, Ho, Wo, x.device)
    elif tuple(out.shape) != (N, cout, Ho, Wo) or out.dtype != torch.float32 or not out.permute(0, 2, 3, 1).is_contiguous():
        raise RuntimeError("conv1x1_frag: out must be a channels_last fp32 [%d,%d,%d,%d]" % (N, cout, Ho, Wo))
    res = None
    if residual is not None:
        res = nhwc(residual.float())
        want = (N, cout, out.shape[2] // 2, out.shape[3] // 2) if residual_up else tuple(out.shape)
        if tuple(res.shape) != want or (residual_up and (out.shape[2] % 2 or out.shape[3] % 2)):
            raise RuntimeError("conv1x1_frag: residual shape %s != %s" % (tuple(res.shape), want))
    ev0 = _prof_begin()
    if ksplit > 1:
        if residual_up:
            raise RuntimeError("conv1x1_frag: split-K has no upsampled-residual epilogue")
        ws = _ws(lib().upsnet_conv1x1_splitk_workspace_bytes(N, Ho, Wo, int(cout), int(ksplit)), x.device)
        bias = None if bias is None else f32c(bias)
        check(lib().upsnet_conv1x1_frag_nhwc_f32_splitk(stream(), ptr(x), ptr(res), ptr(out), N, H, W, int(cin), ptr(wpack),
                                                        ptr(bias), int(cout), int(stride), int(bool(relu)),
                                                        int(ksplit), ptr(ws)), "conv1x1_frag_nhwc_f32_splitk")
    else:
        bias = None if bias is None else f32c(bias)
        check(lib().upsnet_conv1x1_frag_nhwc_f32(stream(), ptr(x), ptr(res), ptr(out), N, H, W, int(cin), ptr(wpack),
                                                 ptr(bias), int(cout), int(stride), int(bool(relu)),
                                                 int(bool(residual_up and res is not None))), "conv1x1_frag_nhwc_f32")
    if ev0 is not None:
        npix = out.shape[0] * out.shape[2] * out.shape[3]
        _prof_end(ev0, 'conv', 2.0 * cout * cin * npix, 4.0 * (cin * npix + cout * npix * (2 if res is not None else 1) + cout * cin),
                  "direct 1x1/%d %d->%d [%s]%s%s (gemm)" % (stride, cin, cout, tuple(x.shape[0:1] + x.shape[2:]), " +res" if res is not None else "",
                                                            " split-K x%d" % ksplit if ksplit > 1 else ""))
    return out


def pack_conv1x1_ksw_weight(weight):
    """[Cout,Cin,1,1] -> 16x16x4 fragment-order pack for conv1x1_ksw (csrc/conv1x1_ksw.hip)."""
    require_cuda(weight)
    w = f32c(weight)
    cout, cin = w.shape[0], w.shape[1]
    wp = torch.empty((lib().upsnet_conv1x1_ksw_packed_weight_floats(cout, cin),), dtype=torch.float32, device=w.device)
    check(lib().upsnet_conv1x1_ksw_pack_weight(stream(), ptr(w), cout, cin, ptr(wp)), "conv1x1_ksw_pack_weight")
    return wp


def conv1x1_ksw(x, wpack, bias, cout, tile, stride=1, relu=False, residual=None, out=None, split_n=False):
    """1x1 convolution (stride 1 / 2) on the small-tile kernel of csrc/conv1x1_ksw.hip (16x16x4 MFMA fragments, K split over the waves):
    out = relu?(conv(x) + bias + residual). tile = (pixels, channels) of a workgroup: {(16, 64), (32, 32), (32, 64), (64, 64)} with the waves
    splitting K, {(16, 256), (32, 128), (32, 256)} with split_n (the waves split the channels, each walks all of K).
    x: logical NCHW (any batch), returns channels_last [N,Cout,Ho,Wo]."""
    require_cuda(wpack, x)
    wpack = f32c(wpack)
    x = nhwc(x.float())
    N, cin, H, W = x.shape
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    if out is None:
        out = _nhwc_out(N, cout, Ho, Wo, x.device)
    elif tuple(out.shape) != (N, cout, Ho, Wo) or out.dtype != torch.float32 or not out.permute(0, 2, 3, 1).is_contiguous():
        raise RuntimeError("conv1x1_ksw: out must be a channels_last fp32 [%d,%d,%d,%d]" % (N, cout, Ho, Wo))
    res = None
    if residual is not None:
        res = nhwc(residual.float())
        if tuple(res.shape) != tuple(out.shape):
            raise RuntimeError("conv1x1_ksw: residual shape %s != %s" % (tuple(res.shape), tuple(out.shape)))
    ev0 = _prof_begin()
    bias = None if bias is None else f32c(bias)
    check(lib().upsnet_conv1x1_ksw_nhwc_f32(stream(), ptr(x), ptr(res), ptr(out), N, H, W, int(cin), ptr(wpack),
                                            ptr(bias), int(cout), int(stride), int(bool(relu)),
                                            int(tile[0]), int(tile[1]), int(bool(split_n))), "conv1x1_ksw_nhwc_f32")
    if ev0 is not None:
        npix = out.shape[0] * out.shape[2] * out.shape[3]
        _prof_end(ev0, 'conv', 2.0 * cout * cin * npix, 4.0 * (cin * npix + cout * npix * (2 if res is not None else 1) + cout * cin),
                  "direct 1x1/%d %d->%d [%s]%s (gemm ksw %dx%d%s)" % (stride, cin, cout, tuple(x.shape[0:1] + x.shape[2:]),
                                                                     " +res" if res is not None else "", tile[0], tile[1], "n" if split_n else "k"))
    return out


def pack_conv3x3_ksw_weight(weight):
    """[Cout <= 32, Cin, 3, 3] -> 16x16x4 fragment-order pack for conv3x3_ksw (csrc/conv1x1_ksw.hip)."""
    require_cuda(weight)
    w = f32c(weight)
    cout, cin = w.shape[0], w.shape[1]
    wp = torch.empty((lib().upsnet_conv3x3_ksw_packed_weight_floats(cin),), dtype=torch.float32, device=w.device)
    check(lib().upsnet_conv3x3_ksw_pack_weight(stream(), ptr(w), cout, cin, ptr(wp)), "conv3x3_ksw_pack_weight")
    return wp


def conv3x3_ksw(x, wpack, bias, cout, relu=False):
    """3x3 / stride 1 / pad 1 convolution into cout <= 32 channels on the small-tile kernel (csrc/conv1x1_ksw.hip, conv3x3_ksw_f32_kernel):
    the offset predictors of the deformable bottlenecks on small maps. x: logical NCHW, returns channels_last [N,cout,H,W]."""
    require_cuda(wpack, x)
    wpack = f32c(wpack)
    x = nhwc(x.float())
    N, cin, H, W = x.shape
    out = _nhwc_out(N, cout, H, W, x.device)
    ev0 = _prof_begin()
    bias = None if bias is None else f32c(bias)
    check(lib().upsnet_conv3x3_ksw_nhwc_f32(stream(), ptr(x), ptr(out), N, H, W, int(cin), ptr(wpack), ptr(bias),
                                            int(cout), int(bool(relu))), "conv3x3_ksw_nhwc_f32")
    if ev0 is not None:
        npix = N * H * W
        _prof_end(ev0, 'conv', 2.0 * cout * cin * 9 * npix, 4.0 * (cin * npix + cout * npix + cout * cin * 9),
                  "direct 3x3/1 %d->%d [%s] (ksw 16x32)" % (cin, cout, (N, H, W)))
    return out


def conv1x1_siblings(x, wpack, bias, cout_a, cout_b, stride=1, relu_a=True, relu_b=False):
    """Two 1x1 convolutions of the same input in one launch (csrc/conv1x1.hip, sibling mode): rows [0, cout_a) of the concatenated weight
    -> out_a (ReLU flag relu_a), the remaining cout_b rows -> out_b. wpack: pack_conv1x1_weight(torch.cat([w_a, w_b])); bias: both biases
    concatenated or None. Bit-identical to two conv1x1_frag calls. Returns two channels_last tensors."""
    require_cuda(wpack, x)
    wpack = f32c(wpack)
    x = nhwc(x.float())
    N, cin, H, W = x.shape
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    out_a, out_b = _nhwc_out(N, cout_a, Ho, Wo, x.device), _nhwc_out(N, cout_b, Ho, Wo, x.device)
    ev0 = _prof_begin()
    bias = None if bias is None else f32c(bias)
    check(lib().upsnet_conv1x1_siblings_nhwc_f32(stream(), ptr(x), ptr(out_a), ptr(out_b), N, H, W, int(cin), ptr(wpack),
                                                 ptr(bias), int(cout_a), int(cout_b), int(stride),
                                                 int(bool(relu_a)), int(bool(relu_b))), "conv1x1_siblings_nhwc_f32")
    if ev0 is not None:
        npix, cout = N * Ho * Wo, cout_a + cout_b
        _prof_end(ev0, 'conv', 2.0 * cout * cin * npix, 4.0 * (cin * npix + cout * npix + cout * cin),
                  "direct 1x1/%d siblings %d->%d+%d [%s] (gemm)" % (stride, cin, cout_a, cout_b, (N, H, W)))
    return out_a, out_b


PAIR32_WAVES = int(os.environ.get('UPSNET_CONV1X1_PAIR32_WAVES', '8'))   # waves per workgroup of the 32-pixel pair kernel (res4): 8 (two per SIMD) or 4
_pair32_waves_set = [None]


def conv1x1_pair(x, residual, w3pack, bias3, c1, w1pack, bias1, c2):
    """Tail of one bottleneck and head of the next in one launch (csrc/conv1x1_pair.hip):
    out1 = relu(conv1x1(x; w3) + bias3 + residual), out2 = relu(conv1x1(out1; w1) + bias1); both bit-identical to two
    conv1x1_frag calls. x: logical NCHW; returns two channels_last tensors."""
    require_cuda(w3pack, w1pack, x, residual)
    w3pack, w1pack = f32c(w3pack), f32c(w1pack)
    x, res = nhwc(x.float()), nhwc(residual.float())
    N, c0, H, W = x.shape
    if tuple(res.shape) != (N, c1, H, W):
        raise RuntimeError("conv1x1_pair: residual shape %s != %s" % (tuple(res.shape), (N, c1, H, W)))
    out1, out2 = _nhwc_out(N, c1, H, W, x.device), _nhwc_out(N, c2, H, W, x.device)
    if _pair32_waves_set[0] != PAIR32_WAVES:
        lib().upsnet_conv1x1_pair32_tuning(PAIR32_WAVES)
        _pair32_waves_set[0] = PAIR32_WAVES
    ev0 = _prof_begin()
    bias3 = None if bias3 is None else f32c(bias3)
    bias1 = None if bias1 is None else f32c(bias1)
    check(lib().upsnet_conv1x1_pair_nhwc_f32(stream(), ptr(x), ptr(res), ptr(out1), ptr(out2), N * H * W, int(c0), ptr(w3pack),
                                             ptr(bias3), int(c1), ptr(w1pack),
                                             ptr(bias1), int(c2)), "conv1x1_pair_nhwc_f32")
    if ev0 is not None:
        npix = N * H * W
        _prof_end(ev0, 'conv', 2.0 * (c1 * c0 + c2 * c1) * npix, 4.0 * (c0 * npix + 2 * c1 * npix + c2 * npix + c1 * c0 + c2 * c1),
                  "direct 1x1 pair %d->%d->%d [%s] +res (gemm)" % (c0, c1, c2, (N, H, W)))
    return out1, out2


def fcn_score_combine(parts, bias=None):
    """score = bias + parts[0] + sum_l bilinear_up_{2^l}(parts[l]); parts[l]: logical NCHW [1,S,H>>l,W>>l] (channels_last
    memory). Returns a channels_last [1,S,H,W] tensor (fcn.py:94-100 with the 1x1 conv commuted below the upsampling)."""
    require_cuda(*parts)
    parts = [nhwc(t.float()) for t in parts]
    _, S, H, W = parts[0].shape
    for l, t in enumerate(parts):
        if tuple(t.shape) != (1, S, H >> l, W >> l):
            raise RuntimeError("fcn_score_combine: level %d has shape %s, expected %s" % (l, tuple(t.shape), (1, S, H >> l, W >> l)))
    out = _nhwc_out(1, S, H, W, parts[0].device)
    bias = None if bias is None else f32c(bias)
    check(lib().upsnet_fcn_score_combine(stream(), len(parts), ptr_array(parts), S, H, W, ptr(bias),
                                         ptr(out)), "fcn_score_combine")
    return out


def panoptic_fuse_up(fcn_score, scale, num_stuff, mask_rois5, mask_logit, cls_idx, keep, num, real, class_map, want_sem=True, want_conf=False):
    """Fused head INCLUDING FCNHead's x4 bilinear upsampling: takes the low-resolution fcn_score [1,S,Hs,Ws]
    (logical NCHW; channels_last memory is consumed as is) and returns (panoptic, semantic) [1,Hs*scale,Ws*scale] int64.
    want_conf: the sibling kernel with the confidence plane (panoptic_fuse_up_conf); returns (panoptic, semantic, conf)."""
    require_cuda(fcn_score, mask_rois5, mask_logit, cls_idx)
    sc = fcn_score.float()
    _, S, Hs, Ws = sc.shape
    is_nhwc = (not sc.is_contiguous()) and sc.is_contiguous(memory_format=torch.channels_last)
    sc = aligned(sc) if is_nhwc else dense(sc)
    mask_rois5 = f32c(mask_rois5)
    m = mask_rois5.shape[0]
    if m > 256:   # the kernels keep their instance table in LDS (FUSE_MAXK); more rows would be dropped silently
        raise RuntimeError("panoptic_fuse: at most 256 instance rows (got %d); use mask_paste + seg_term + panoptic_argmax" % m)
    mask_logit = f32c(mask_logit).reshape(m, -1)
    ms = int(round(mask_logit.shape[1] ** 0.5))
    H, W = Hs * scale, Ws * scale
    pan = torch.empty((1, H, W), dtype=torch.int64, device=sc.device)
    sem = torch.empty((1, H, W), dtype=torch.int64, device=sc.device) if want_sem else None
    cls_idx, keep, num, real, class_map = i64c(cls_idx), i64c(keep), i32c(num), i32c(real), i64c(class_map)
    args = (stream(), ptr(sc), int(is_nhwc), S, Hs, Ws, int(scale), int(num_stuff), ptr(mask_rois5), ptr(mask_logit),
            ptr(cls_idx), ptr(keep), ptr(num), ptr(real), int(min(m, 256)), ms, ptr(class_map), ptr(pan), ptr(sem))
    if not want_conf:
        check(lib().upsnet_panoptic_fuse_up(*args), "panoptic_fuse_up")
        return pan, sem
    conf = torch.empty((1, H, W), dtype=torch.uint8, device=sc.device)
    check(lib().upsnet_panoptic_fuse_up_conf(*args, ptr(conf)), "panoptic_fuse_up_conf")
    return pan, sem, conf


def panoptic_fuse_up_conf(fcn_score, scale, num_stuff, mask_rois5, mask_logit, cls_idx, keep, num, real, class_map, want_sem=True):
    """panoptic_fuse_up with the confidence plane (include/upsnet_hip.h: upsnet_panoptic_fuse_up_conf): returns
    (panoptic, semantic, conf); conf uint8 [1,Hs*scale,Ws*scale] = (uint8)(255 * P[winner] + 0.5), P the softmax over the panoptic
    logits of the pixel. The two label maps are bit-equal to panoptic_fuse_up's; all three come out of one launch."""
    return panoptic_fuse_up(fcn_score, scale, num_stuff, mask_rois5, mask_logit, cls_idx, keep, num, real, class_map, want_sem, True)


def panoptic_conf_planes(fcn_output, num_stuff, seg_inst, mask_energy, enable_void=True):
    """The confidence plane from materialised planes, in plain torch: for the paths the fused-upsample kernel does not serve (more than
    256 panoptic instances, fuse_up off, the module-level forward). fcn_output [1,S,H,W], seg_inst / mask_energy [1,k,H,W] fp32 ->
    uint8 [1,H,W] by the rule of upsnet_panoptic_fuse_up_conf: the softmax over stuff | instance | void logits (no void channel without
    enable_void) at its maximum, which is the label panoptic_argmax emits. torch's exp and summation order are not the kernel's: the two
    agree within one step of the byte."""
    f = fcn_output.float()
    z = [f[:, :num_stuff], seg_inst + mask_energy]
    if enable_void:
        z.append(f[:, num_stuff:].max(1, keepdim=True)[0] - seg_inst.max(1, keepdim=True)[0])
    conf = torch.softmax(torch.cat(z, 1), 1).max(1)[0]
    return (conf * 255.0 + 0.5).to(torch.uint8)


# ----------------------------------------------------------------------------- stem / deconvolution / input blob
def pack_stem_weight(weight):
    """[Cout,Cin<=4,KH,KW<=8] -> ([KH*32, ldw], ldw): one K slab = one kernel row of 8 pixels x 4 channels."""
    require_cuda(weight)
    weight = f32c(weight)
    Cout, Cin, kh, kw = weight.shape
    ldw = (Cout + 31) // 32 * 32
    wp = torch.empty((kh * 32, ldw), dtype=torch.float32, device=weight.device)
    check(lib().upsnet_conv_pack_weight_stem(stream(), ptr(weight), Cout, Cin, kh, kw, ldw, ptr(wp)), "conv_pack_weight_stem")
    return wp, ldw


def pack_stem_pool_weight_f32(weight):
    """[64, Cin <= 3, 7, 7] fp32 -> the operand pack of stem_pool_f32 (2 x 75 x 64 floats)."""
    require_cuda(weight)
    weight = f32c(weight)
    if tuple(weight.shape[0:1] + weight.shape[2:]) != (64, 7, 7) or weight.shape[1] > 3:
        raise RuntimeError("pack_stem_pool_weight_f32: weight must be [64, Cin <= 3, 7, 7]")
    wp = torch.empty(2 * 75 * 64, dtype=torch.float32, device=weight.device)
    check(lib().upsnet_stem_pool_pack_weight_f32(stream(), ptr(weight), int(weight.shape[1]), ptr(wp)), "stem_pool_pack_weight_f32")
    return wp


def stem_pool_f32(x4, wpack, bias):
    """max_pool2d(relu(conv7x7/2/3(x) + bias), 3, 2, 1) in one launch; x4: logical [N,4,H,W] channels_last fp32 (image_to_nhwc4 /
    prep_image_u8). Returns channels_last fp32 [N,64,Hp,Wp]."""
    require_cuda(x4, wpack)
    wpack = f32c(wpack)
    x4 = nhwc(x4.float())
    N, C, H, W = x4.shape
    if C != 4:
        raise RuntimeError("stem_pool_f32: input must have 4 channels (RGB + zero), got %d" % C)
    Hc, Wc = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    Hp, Wp = (Hc - 1) // 2 + 1, (Wc - 1) // 2 + 1
    out = _nhwc_out(N, 64, Hp, Wp, x4.device)
    ev0 = _prof_begin()
    bias = None if bias is None else f32c(bias)
    check(lib().upsnet_stem_pool_f32(stream(), ptr(x4), N, H, W, ptr(wpack), ptr(bias), ptr(out)), "stem_pool_f32")
    if ev0 is not None:
        _prof_end(ev0, 'conv', 2.0 * 64 * 147 * N * Hc * Wc, 16.0 * N * H * W + 4.0 * 64 * N * Hp * Wp + 4.0 * 64 * 147, 'stem + pool')
    return out


def pack_stem_pool_weight_bf16(weight):
    """[64, Cin <= 4, 7, 7] fp32 -> the bf16 fragment pack of stem_pool_bf16 (2 x 14 x 64 x 8 elements)."""
    require_cuda(weight)
    weight = f32c(weight)
    if tuple(weight.shape[0:1] + weight.shape[2:]) != (64, 7, 7) or weight.shape[1] > 4:
        raise RuntimeError("pack_stem_pool_weight_bf16: weight must be [64, Cin <= 4, 7, 7]")
    wp = torch.empty(2 * 14 * 64 * 8, dtype=torch.bfloat16, device=weight.device)
    check(lib().upsnet_stem_pool_pack_weight_bf16(stream(), ptr(weight), int(weight.shape[1]), ptr(wp)), "stem_pool_pack_weight_bf16")
    return wp


def stem_pool_bf16(x4, wpack, bias):
    """relu(conv7x7/2/3(x) + bias) -> max_pool 3x3/2/1 in one launch; x4: logical [N,4,H,W] channels_last fp32 (image_to_nhwc4 /
    prep_image_u8). Returns a bf16 channels_last [N,64,Hp,Wp]."""
    require_cuda(x4, wpack)
    wpack = dense(wpack)
    x4 = nhwc(x4.float())
    N, C, H, W = x4.shape
    if C != 4:
        raise RuntimeError("stem_pool_bf16: input must have 4 channels (RGB + zero), got %d" % C)
    Hc, Wc = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    Hp, Wp = (Hc - 1) // 2 + 1, (Wc - 1) // 2 + 1
    out = torch.empty((N, Hp, Wp, 64), dtype=torch.bfloat16, device=x4.device).permute(0, 3, 1, 2)
    ev0 = _prof_begin()
    bias = None if bias is None else f32c(bias)
    check(lib().upsnet_stem_pool_bf16(stream(), ptr(x4), N, H, W, ptr(wpack), ptr(bias), ptr(out)), "stem_pool_bf16")
    if ev0 is not None:
        _prof_end(ev0, 'conv_bf16', 2.0 * 64 * 147 * N * Hc * Wc, 16.0 * N * H * W + 2.0 * 64 * N * Hp * Wp)
    return out


def image_to_nhwc4(x):
    """fp32 [N,C<=4,H,W] -> physical [N,H,W,4] (returned as a logical [N,4,H,W] channels_last tensor)."""
    require_cuda(x)
    x = f32c(x)
    N, C, H, W = x.shape
    out = _nhwc_out(N, 4, H, W, x.device)
    check(lib().upsnet_image_to_nhwc4(stream(), ptr(x), N, C, H, W, ptr(out)), "image_to_nhwc4")
    return out


def conv2d_stem(x4, wpack, ldw, bias, cout, kh, kw, stride, pad, relu=False):
    """x4: logical [N,4,H,W] channels_last (from image_to_nhwc4 / prep_image_u8). Returns channels_last [N,Cout,Ho,Wo]."""
    require_cuda(x4, wpack)
    wpack = f32c(wpack)
    x4 = nhwc(x4.float())
    N, C, H, W = x4.shape
    if C != 4:
        raise RuntimeError("conv2d_stem: input must have 4 channels (RGB + zero), got %d" % C)
    Ho, Wo = (H + 2 * pad - kh) // stride + 1, (W + 2 * pad - kw) // stride + 1
    out = _nhwc_out(N, cout, Ho, Wo, x4.device)
    ev0 = _prof_begin()
    bias = None if bias is None else f32c(bias)
    check(lib().upsnet_conv2d_stem_nhwc4_f32(stream(), ptr(x4), N, H, W, ptr(wpack), int(ldw), ptr(bias),
                                             int(cout), int(kh), int(kw), int(stride), int(pad), int(bool(relu)), ptr(out)),
          "conv2d_stem_nhwc4_f32")
    if ev0 is not None:
        _prof_end(ev0, 'conv', 2.0 * cout * 3 * kh * kw * N * Ho * Wo, 4.0 * (4 * N * H * W + cout * N * Ho * Wo + cout * 3 * kh * kw))
    return out


def pack_deconv2x2_weight(weight):
    """ConvTranspose2d weight [Cin,Cout,2,2] -> ([Cin, ldw], ldw) with columns (dy,dx,co)."""
    require_cuda(weight)
    weight = f32c(weight)
    Cin, Cout, kh, kw = weight.shape
    if (kh, kw) != (2, 2):
        raise RuntimeError("pack_deconv2x2_weight: kernel must be 2x2")
    ldw = (4 * Cout + 31) // 32 * 32
    wp = torch.empty((Cin, ldw), dtype=torch.float32, device=weight.device)
    check(lib().upsnet_deconv2x2_pack_weight(stream(), ptr(weight), Cin, Cout, ldw, ptr(wp)), "deconv2x2_pack_weight")
    return wp, ldw


def deconv2x2(x, wpack, ldw, bias, cout, relu=False):
    """ConvTranspose2d(k=2, s=2, p=0) (+bias, +ReLU) on a logical NCHW tensor; returns channels_last [N,Cout,2H,2W]."""
    require_cuda(x, wpack)
    wpack = f32c(wpack)
    x = nhwc(x.float())
    N, C, H, W = x.shape
    out = _nhwc_out(N, cout, 2 * H, 2 * W, x.device)
    ev0 = _prof_begin()
    bias = None if bias is None else f32c(bias)
    check(lib().upsnet_deconv2x2_nhwc_f32(stream(), ptr(x), N, H, W, C, ptr(wpack), int(ldw), ptr(bias),
                                          int(cout), int(bool(relu)), ptr(out)), "deconv2x2_nhwc_f32")
    if ev0 is not None:
        _prof_end(ev0, 'conv', 2.0 * 4 * cout * C * N * H * W, 4.0 * (C * N * H * W + 4 * cout * N * H * W + 4 * cout * C))
    return out


def pack_deconv2x2_weight_frag(weight, bias):
    """ConvTranspose2d weight [Cin,Cout,2,2] (+ bias [Cout]) -> (fragment-order pack of the [4 Cout, Cin] matrix with rows (dy, dx, co),
    bias repeated per (dy, dx)) for deconv2x2_frag (csrc/conv1x1.hip, scatter epilogue)."""
    require_cuda(weight)
    Cin, Cout, kh, kw = weight.shape
    if (kh, kw) != (2, 2) or Cin % 32 or Cout % 32:
        raise RuntimeError("pack_deconv2x2_weight_frag: kernel 2x2, Cin % 32 == 0, Cout % 32 == 0")
    w = weight.detach().float().permute(2, 3, 1, 0).reshape(4 * Cout, Cin, 1, 1).contiguous()
    return pack_conv1x1_weight(w), (None if bias is None else bias.detach().float().repeat(4).contiguous())


def deconv2x2_frag(x, wpack, bias4, cout, relu=False):
    """ConvTranspose2d(k=2, s=2, p=0) (+bias, +ReLU) on the lean GEMM kernel; returns channels_last [N,Cout,2H,2W]."""
    require_cuda(x, wpack)
    wpack, bias4 = f32c(wpack), f32c(bias4)
    x = nhwc(x.float())
    N, C, H, W = x.shape
    out = _nhwc_out(N, cout, 2 * H, 2 * W, x.device)
    ev0 = _prof_begin()
    check(lib().upsnet_deconv2x2_frag_nhwc_f32(stream(), ptr(x), ptr(out), N, H, W, C, ptr(wpack), ptr(bias4), int(cout), int(bool(relu))),
          "deconv2x2_frag_nhwc_f32")
    if ev0 is not None:
        _prof_end(ev0, 'conv', 2.0 * 4 * cout * C * N * H * W, 4.0 * (C * N * H * W + 4 * cout * N * H * W + 4 * cout * C),
                  "deconv 2x2/2 %d->%d [%s] (gemm)" % (C, cout, (N, H, W)))
    return out


def pack_deconv2x2_weight_bf16(weight):
    """ConvTranspose2d weight [Cin,Cout,2,2] -> (bf16 pack, ldw) of the [4 Cout, Cin] matrix with rows (ky, kx, co) for deconv2x2_bf16."""
    require_cuda(weight)
    Cin, Cout, kh, kw = weight.shape
    if (kh, kw) != (2, 2) or Cin % 64 or Cout % 32:
        raise RuntimeError("pack_deconv2x2_weight_bf16: kernel 2x2, Cin % 64 == 0, Cout % 32 == 0")
    w = weight.detach().float().permute(2, 3, 1, 0).reshape(4 * Cout, Cin, 1, 1).contiguous()
    hi, _, ldw = pack_conv_weight_bf16(w, split=False)
    return hi, ldw


def deconv2x2_bf16(x, whi, ldw, bias, cout, relu=False, out_dtype=torch.float32):
    """ConvTranspose2d(k=2, s=2, p=0) (+bias, +ReLU) of a bf16 map on the bf16 matrix cores; channels_last [N,Cout,2H,2W]."""
    require_cuda(x, whi)
    whi = dense(whi)
    if x.dtype != torch.bfloat16:
        raise RuntimeError("deconv2x2_bf16: expects a bf16 map")
    x = nhwc(x)
    N, C, H, W = x.shape
    out16 = out_dtype == torch.bfloat16
    out = (torch.empty((N, 2 * H, 2 * W, cout), dtype=torch.bfloat16, device=x.device).permute(0, 3, 1, 2) if out16
           else _nhwc_out(N, cout, 2 * H, 2 * W, x.device))
    ev0 = _prof_begin()
    bias = None if bias is None else f32c(bias)
    check(lib().upsnet_deconv2x2_nhwc_bf16(stream(), ptr(x), N, H, W, C, ptr(whi), int(ldw), ptr(bias),
                                           int(cout), int(bool(relu)), ptr(out), int(out16)), "deconv2x2_nhwc_bf16")
    if ev0 is not None:
        _prof_end(ev0, 'conv_bf16', 2.0 * 4 * cout * C * N * H * W,
                  2.0 * C * N * H * W + (2.0 if out16 else 4.0) * 4 * cout * N * H * W + 2.0 * 4 * cout * C)
    return out


def prep_image_u8(image_hwc, pixel_means, im_scale, resized_hw, padded_hw, nhwc4=True):
    """uint8 [H,W,3] device image -> padded fp32 blob: logical [1,4,Hp,Wp] channels_last (nhwc4) or [1,3,Hp,Wp] NCHW."""
    import ctypes
    require_cuda(image_hwc)
    if image_hwc.dtype != torch.uint8 or image_hwc.dim() != 3 or image_hwc.shape[2] != 3:
        raise RuntimeError("prep_image_u8: expected a uint8 [H,W,3] image")
    im = dense(image_hwc)
    H, W = im.shape[:2]
    (Hr, Wr), (Hp, Wp) = resized_hw, padded_hw
    means = (ctypes.c_double * 3)(*[float(m) for m in pixel_means])
    out = _nhwc_out(1, 4, Hp, Wp, im.device) if nhwc4 else torch.empty((1, 3, Hp, Wp), dtype=torch.float32, device=im.device)
    check(lib().upsnet_prep_image_u8(stream(), ptr(im), H, W, means, float(im_scale), int(Hr), int(Wr),
                                     int(Hp), int(Wp), int(bool(nhwc4)), ptr(out)), "prep_image_u8")
    return out


def restore_label_maps(sseg, pano, y_ofs, x_ofs):
    """Nearest-neighbour gather of one image's label maps (include/upsnet_hip.h: upsnet_restore_label_maps): sseg / pano int64 [H,W]
    or [1,H,W] device tensors (pano may be None; rows may be strided, columns contiguous; a crop may start at any element of the padded
    map), y_ofs / x_ofs int32 index tables (host or device; dataset/restore.py builds them). Returns (uint8 [len(y_ofs), len(x_ofs)] for sseg, the same for pano or None);
    out[y, x] = low byte of src[y_ofs[y], x_ofs[x]]. Both maps come out of one launch."""
    require_cuda(sseg, pano)
    maps = [m.reshape(m.shape[-2], m.shape[-1]) if m is not None else None for m in (sseg, pano)]
    for m in maps:
        if m is not None and (m.dtype != torch.int64 or m.stride(1) != 1):
            raise ValueError("restore_label_maps: int64 maps with contiguous rows required, got %s stride %s" % (m.dtype, m.stride()))
    s, p = maps
    if p is not None and (p.shape != s.shape or p.stride() != s.stride()):
        s, p = dense(s), dense(p)
    H, W = s.shape
    ys = torch.as_tensor(y_ofs, dtype=torch.int32).reshape(-1)
    xs = torch.as_tensor(x_ofs, dtype=torch.int32).reshape(-1)
    for name, t, n in (("y_ofs", ys, H), ("x_ofs", xs, W)):
        if t.numel() and (int(t.min()) < 0 or int(t.max()) >= n):
            raise ValueError("restore_label_maps: %s outside 0..%d" % (name, n - 1))
    ys, xs = dense(ys.to(s.device)), dense(xs.to(s.device))
    H0, W0 = ys.numel(), xs.numel()
    out_s = torch.empty((H0, W0), dtype=torch.uint8, device=s.device)
    out_p = torch.empty((H0, W0), dtype=torch.uint8, device=s.device) if p is not None else None
    if H0 == 0 or W0 == 0:
        return out_s, out_p
    check(lib().upsnet_restore_label_maps(stream(), ptr_unaligned(s), ptr_unaligned(p), int(s.stride(0)), H, W, ptr(ys), H0, ptr(xs), W0, ptr(out_s),
                                          ptr(out_p)), "restore_label_maps")
    return out_s, out_p


def restore_plane_u8(plane, y_ofs, x_ofs, *, out=None):
    """restore_label_maps' gather for one uint8 plane (include/upsnet_hip.h: upsnet_restore_plane_u8): plane uint8 [H,W] or [1,H,W]
    device tensor (rows may be strided, columns contiguous; a crop may start at any byte of the padded plane), the same index tables. Returns uint8 [len(y_ofs), len(x_ofs)] =
    plane[y_ofs[y], x_ofs[x]]: the panoptic confidence at the original image size, by the rule of the label maps. out= is taken
    instead of being allocated."""
    require_cuda(plane)
    s = plane.reshape(plane.shape[-2], plane.shape[-1])
    if s.dtype != torch.uint8 or s.stride(1) != 1:
        raise ValueError("restore_plane_u8: a uint8 plane with contiguous rows required, got %s stride %s" % (s.dtype, s.stride()))
    H, W = s.shape
    ys = torch.as_tensor(y_ofs, dtype=torch.int32).reshape(-1)
    xs = torch.as_tensor(x_ofs, dtype=torch.int32).reshape(-1)
    for name, t, n in (("y_ofs", ys, H), ("x_ofs", xs, W)):
        if t.numel() and (int(t.min()) < 0 or int(t.max()) >= n):
            raise ValueError("restore_plane_u8: %s outside 0..%d" % (name, n - 1))
    ys, xs = dense(ys.to(s.device)), dense(xs.to(s.device))
    H0, W0 = ys.numel(), xs.numel()
    if out is None:
        out = torch.zeros((H0, W0), dtype=torch.uint8, device=s.device)
    elif out.dtype != torch.uint8 or tuple(out.shape) != (H0, W0) or not out.is_contiguous() or out.device != s.device:
        raise ValueError("restore_plane_u8: out must be a contiguous uint8 [%d,%d] tensor on the plane's device" % (H0, W0))
    if H0 == 0 or W0 == 0:
        return out
    check(lib().upsnet_restore_plane_u8(stream(), ptr_unaligned(s), int(s.stride(0)), H, W, ptr(ys), H0, ptr(xs), W0, ptr(out)), "restore_plane_u8")
    return out


def unified_pan_result(pan, seg, cls_inds, id_last_stuff, num_seg_classes, stuff_area_limit=4 * 64 * 64):
    """get_unified_pan_result of ONE image on the device: pan / seg int64 [H,W] (or [1,H,W]), cls_inds int64 [k] -> uint8 [H,W,3]."""
    require_cuda(pan, seg)
    pan = i64c(pan.reshape(pan.shape[-2], pan.shape[-1]))
    seg = i64c(seg.reshape(seg.shape[-2], seg.shape[-1]))
    if pan.shape != seg.shape:
        raise RuntimeError("unified_pan_result: pan %s and seg %s differ in shape" % (tuple(pan.shape), tuple(seg.shape)))
    cls_inds = i64c(cls_inds.to(device=pan.device)).reshape(-1)
    H, W = pan.shape
    ws = torch.empty((int(lib().upsnet_unified_pan_workspace_bytes()),), dtype=torch.uint8, device=pan.device)
    out = torch.empty((H, W, 3), dtype=torch.uint8, device=pan.device)
    check(lib().upsnet_unified_pan_result(stream(), ptr(pan), ptr(seg), ptr(cls_inds) if cls_inds.numel() else None, int(cls_inds.numel()),
                                          H, W, int(id_last_stuff), int(num_seg_classes), int(stuff_area_limit), ptr(ws), ptr(out)),
          "unified_pan_result")
    return out


COMBINED_PAN_CHUNK_IMAGES = 256          # images per launch (one workgroup each in the greedy kernel)
COMBINED_PAN_CHUNK_PIXELS = 1 << 28      # pixels per launch: bounds the workspace (2.1 bytes per pixel)
_SEG_BLOCK = 4096                        # segments of a run never cross a multiple of this (csrc/pan_combine.hip)


def _combined_seg_u8(seg, dev):
    """One semantic map -> (uint8 [H,W] tensor on dev, or None with a pending (min, max) range check); never modifies the input."""
    if isinstance(seg, torch.Tensor):
        t = seg
    else:
        a = np.asarray(seg)
        if a.ndim == 2 and a.dtype != np.uint8 and a.size:
            if not np.issubdtype(a.dtype, np.integer) or int(a.min()) < 0 or int(a.max()) > 255:
                raise ValueError("combined_pan_result: semantic labels must be integers in 0..255")
            a = a.astype(np.uint8)
        t = torch.from_numpy(np.ascontiguousarray(a))
    if t.dim() != 2:
        raise ValueError("combined_pan_result: semantic maps must be [H,W], got %s" % (tuple(t.shape),))
    if t.dtype != torch.uint8 and (t.dtype.is_floating_point or t.dtype.is_complex or t.dtype == torch.bool):
        raise ValueError("combined_pan_result: semantic maps must be uint8 or int64, got %s" % t.dtype)
    return t.to(dev)


def combined_pan_result(segs, boxes, masks, id_last_stuff, score_threshold=0.6, fraction_threshold=0.7, stuff_area_limit=4 * 64 * 64):
    """BaseDataset.get_combined_pan_result on the device (csrc/pan_combine.hip; DESIGN 4.7 for the pinned semantics).

    segs: per-image semantic maps [H,W] (numpy or tensor, uint8 or int64 with values 0..255); boxes[c][i]: [n,5] (x1 y1 x2 y2 score)
    and masks[c][i]: n RLE dicts {'size': [H, W], 'counts': str | bytes} for classes c = 1..len(boxes)-1 (entry 0 is ignored).
    Candidates: classes concatenated in order, np.argsort(score, kind='stable')[::-1], those with float(score) < score_threshold
    dropped. Returns a list of uint8 [H,W,3] device tensors. Every ValueError is raised before the first launch; inputs are never
    modified."""
    from .dataset.rle import _segmented_cumsum, decode_rle_strings
    n = len(segs)
    if len(boxes) != len(masks):
        raise ValueError("combined_pan_result: %d classes of boxes, %d of masks" % (len(boxes), len(masks)))
    num_classes = len(boxes)
    if num_classes < 2 or id_last_stuff < 0 or id_last_stuff + num_classes - 1 >= 255:
        raise ValueError("combined_pan_result: %d classes after id_last_stuff %d do not fit the uint8 labels" % (num_classes, id_last_stuff))
    for c in range(1, num_classes):
        if len(boxes[c]) != n or len(masks[c]) != n:
            raise ValueError("combined_pan_result: class %d has boxes for %d and masks for %d of %d images" % (c, len(boxes[c]), len(masks[c]), n))
    if n == 0:
        return []
    dev = next((s.device for s in segs if isinstance(s, torch.Tensor) and s.is_cuda), None) or torch.device('cuda', torch.cuda.current_device())
    seg_t = [_combined_seg_u8(s, dev) for s in segs]
    wide = [t for t in seg_t if t.dtype != torch.uint8 and t.numel()]
    if wide:   # one host synchronisation for all non-uint8 maps of the call
        r = torch.stack([torch.stack([t.min(), t.max()]).to(torch.int64) for t in wide]).cpu()
        if int(r[:, 0].min()) < 0 or int(r[:, 1].max()) > 255:
            raise ValueError("combined_pan_result: semantic labels must be integers in 0..255")
    seg_t = [dense(t.to(torch.uint8)) for t in seg_t]
    thr = float(score_threshold)
    strings, cls_of, npix_of, img_ncand = [], [], [], []
    for i, t in enumerate(seg_t):
        H, W = int(t.shape[0]), int(t.shape[1])
        if H * W > (1 << 24):
            raise ValueError("combined_pan_result: image %d has %d x %d pixels; the pixel counts are exact only up to 2^24" % (i, H, W))
        sc, cl, rl = [], [], []
        for c in range(1, num_classes):
            b, m = boxes[c][i], masks[c][i]
            b = np.asarray(b)
            nb = b.shape[0] if b.size else 0
            if nb != len(m):
                raise ValueError("combined_pan_result: image %d class %d: %d boxes, %d masks" % (i, c, nb, len(m)))
            if nb:
                if b.ndim != 2 or b.shape[1] < 5:
                    raise ValueError("combined_pan_result: image %d class %d: boxes must be [n,5], got %s" % (i, c, b.shape))
                sc.append(b[:, 4].astype(np.float64))
                cl.append(np.full(nb, c, np.int32))
                rl.extend(m)
        for r in rl:
            if not isinstance(r, dict) or [int(v) for v in r.get('size', ())] != [H, W]:
                raise ValueError("combined_pan_result: image %d: mask size %s differs from the semantic map's %s" %
                                 (i, r.get('size') if isinstance(r, dict) else type(r), [H, W]))
        if sc:
            s = np.concatenate(sc)
            order = np.argsort(s, kind='stable')[::-1]
            order = order[~(s[order] < thr)]
            cls = np.concatenate(cl)[order]
            per = np.bincount(cls, minlength=num_classes)
            if per.max(initial=0) > 255:
                raise ValueError("combined_pan_result: image %d class %d has %d candidates at or above the score threshold; the "
                                 "instance ids are uint8" % (i, int(per.argmax()), int(per.max())))
            for k in order:
                cnt = rl[k]['counts']
                if not isinstance(cnt, (str, bytes)):
                    raise ValueError("combined_pan_result: image %d: RLE counts must be a compressed string" % i)
                strings.append(cnt)
            cls_of.append(cls)
        npix_of.append(np.full(len(order) if sc else 0, H * W, np.int64))
        img_ncand.append(len(order) if sc else 0)
    cls_all = np.concatenate(cls_of) if cls_of else np.zeros(0, np.int32)
    npix_all = np.concatenate(npix_of)
    counts, off = decode_rle_strings(strings)
    ncodes = np.diff(off)
    str_of = np.repeat(np.arange(len(strings)), ncodes)
    if counts.size and counts.min() < 0:
        raise ValueError("combined_pan_result: negative RLE count (string %d)" % int(str_of[np.argmax(counts < 0)]))
    total = np.bincount(str_of, weights=counts.astype(np.float64), minlength=len(strings))   # exact: sums below 2^53
    bad = np.flatnonzero(total != npix_all)
    if bad.size:
        raise ValueError("combined_pan_result: RLE counts of candidate %d sum to %d, not H * W = %d" %
                         (int(bad[0]), int(total[bad[0]]), int(npix_all[bad[0]])))
    # runs of ones: [end of count j-1, end of count j) for odd j in each string
    first = np.zeros(counts.size, bool)
    first[off[:-1][ncodes > 0]] = True
    pos = _segmented_cumsum(counts, first) if counts.size else counts
    j = np.arange(counts.size) - np.repeat(off[:-1], ncodes)
    odd = np.flatnonzero(((j & 1) == 1) & (counts > 0))
    run_b = pos[odd]
    run_a = run_b - counts[odd]
    run_str = str_of[odd]
    area = np.bincount(run_str, weights=(run_b - run_a).astype(np.float64), minlength=len(strings)).astype(np.int64)
    # cut runs at multiples of _SEG_BLOCK
    blk_a, blk_b = run_a // _SEG_BLOCK, (run_b - 1) // _SEG_BLOCK
    nseg = blk_b - blk_a + 1
    run_idx = np.repeat(np.arange(run_a.size), nseg)
    blk = blk_a[run_idx] + (np.arange(run_idx.size) - np.repeat(np.cumsum(nseg) - nseg, nseg))
    seg_a = np.maximum(run_a[run_idx], blk * _SEG_BLOCK)
    seg_b = np.minimum(run_b[run_idx], (blk + 1) * _SEG_BLOCK)
    seg_str = run_str[run_idx]
    seg_cnt = np.bincount(seg_str, minlength=len(strings))
    keep = area > 0                          # zero-area candidates are skipped and use no instance number
    cand_img = np.repeat(np.arange(n), img_ncand)
    out = [torch.empty((int(t.shape[0]), int(t.shape[1]), 3), dtype=torch.uint8, device=dev) for t in seg_t]
    # chunks of images (all with pixels): one workspace, four launches per chunk
    live = [i for i in range(n) if seg_t[i].numel()]
    chunks, cur, cur_pix = [], [], 0
    for i in live:
        p = seg_t[i].numel()
        if cur and (len(cur) >= COMBINED_PAN_CHUNK_IMAGES or cur_pix + p > COMBINED_PAN_CHUNK_PIXELS):
            chunks.append(cur)
            cur, cur_pix = [], 0
        cur.append(i)
        cur_pix += p
    if cur:
        chunks.append(cur)
    for ch in chunks:
        in_chunk = keep & np.isin(cand_img, ch)
        sel = np.flatnonzero(in_chunk)                          # candidates of the chunk, in image then merge order
        cbeg = np.concatenate([[0], np.cumsum(np.bincount(np.searchsorted(ch, cand_img[sel]), minlength=len(ch)))])
        segs_sel = np.flatnonzero(in_chunk[seg_str])           # their segments, in the same order
        c_seg_end = np.cumsum(seg_cnt[sel])
        cand = np.stack([cls_all[sel], area[sel], c_seg_end - seg_cnt[sel], c_seg_end], 1).astype(np.int32) if sel.size else None
        segs_np = np.stack([seg_a[segs_sel], seg_b[segs_sel]], 1).astype(np.int32) if segs_sel.size else None
        hw = np.array([[int(seg_t[i].shape[0]), int(seg_t[i].shape[1])] for i in ch], np.int64)
        npx = hw[:, 0] * hw[:, 1]
        img = np.zeros((len(ch), 8), np.int64)
        img[:, 0:2] = hw
        img[:, 2] = [addr(seg_t[i]) for i in ch]
        img[:, 3] = [addr(out[i]) for i in ch]
        img[:, 4], img[:, 5] = cbeg[:-1], cbeg[1:]
        img[:, 6] = np.concatenate([[0], np.cumsum((npx + 63) // 64)[:-1]])
        img[:, 7] = np.concatenate([[0], np.cumsum(npx)[:-1]])
        total_pix = int(npx.sum())
        img_d = torch.from_numpy(img).to(dev)
        cand_d = torch.from_numpy(cand).to(dev) if cand is not None else None
        segs_d = torch.from_numpy(segs_np).to(dev) if segs_np is not None else None
        ws = torch.empty((int(lib().upsnet_combined_pan_workspace_bytes(len(ch), total_pix)),), dtype=torch.uint8, device=dev)
        check(lib().upsnet_combined_pan_result(stream(), len(ch), ptr(img_d), int(hw[:, 0].max()), int(hw[:, 1].max()), total_pix,
                                               ptr(cand_d), ptr(segs_d), int(id_last_stuff), num_classes, int(stuff_area_limit),
                                               float(fraction_threshold), ptr(ws)), "combined_pan_result")
    return out


def pq_workspace(max_gt, device):
    """Zeroed workspace of pq_accumulate for images of at most max_gt GT segments (0..4096); every call leaves it zeroed again."""
    nbytes = int(lib().upsnet_pq_workspace_bytes(int(max_gt)))
    if nbytes == 0:
        raise ValueError("pq_workspace: max_gt %d outside 0..4096" % max_gt)
    return torch.zeros((nbytes,), dtype=torch.uint8, device=device)


def pq_accumulate(pred_2ch, gt_rgb, segments, cat_known, image_index, max_gt, workspace, tp, fp, fn, iou, status):
    """_pq_compute_single_core of ONE image on the device, added into the running accumulators (include/upsnet_hip.h):
    pred_2ch / gt_rgb uint8 [H,W,3]; segments int64 [n,4] = (id, category_id, iscrowd, area) in segments_info order; cat_known uint8
    [256]; tp / fp / fn int64 [256], iou float64 [256], status int64 [1] (first error). No host synchronisation."""
    require_cuda(pred_2ch, gt_rgb, segments, cat_known, workspace, tp, fp, fn, iou, status)
    if pred_2ch.dtype != torch.uint8 or gt_rgb.dtype != torch.uint8 or pred_2ch.dim() != 3 or pred_2ch.shape[2] != 3 \
            or tuple(pred_2ch.shape) != tuple(gt_rgb.shape):
        raise ValueError("pq_accumulate: pred_2ch %s %s and gt_rgb %s %s must both be uint8 [H,W,3]"
                         % (tuple(pred_2ch.shape), pred_2ch.dtype, tuple(gt_rgb.shape), gt_rgb.dtype))
    if segments.dtype != torch.int64 or segments.dim() != 2 or segments.shape[1] != 4:
        raise ValueError("pq_accumulate: segments must be int64 [n,4]")
    for t, dt, n in ((cat_known, torch.uint8, 256), (tp, torch.int64, 256), (fp, torch.int64, 256), (fn, torch.int64, 256),
                     (iou, torch.float64, 256), (status, torch.int64, 1)):
        if t.dtype != dt or t.numel() != n or not t.is_contiguous():
            raise ValueError("pq_accumulate: accumulator / table of %d %s expected, got %s %s" % (n, dt, tuple(t.shape), t.dtype))
        written(t, dt, "pq_accumulate: accumulator / table")
    written(workspace, None, "pq_accumulate: workspace")
    pred_2ch, gt_rgb, segments = dense(pred_2ch), dense(gt_rgb), dense(segments)
    H, W = pred_2ch.shape[:2]
    check(lib().upsnet_pq_accumulate(stream(), ptr(pred_2ch), ptr(gt_rgb), H, W, ptr(segments) if segments.numel() else None,
                                     int(segments.shape[0]), ptr(cat_known), int(image_index), int(max_gt), ptr(workspace), ptr(tp), ptr(fp),
                                     ptr(fn), ptr(iou), ptr(status)), "pq_accumulate")


def pq_boundary_workspace(max_gt, height, width, device):
    """Zeroed workspace of pq_boundary_accumulate for images of at most max_gt GT segments (0..4096) and height x width pixels (a
    smaller image fits too); every call leaves its count areas zeroed again."""
    nbytes = int(lib().upsnet_pq_boundary_workspace_bytes(int(max_gt), int(height), int(width)))
    if nbytes == 0:
        raise ValueError("pq_boundary_workspace: max_gt %d outside 0..4096 or image size %dx%d out of range" % (max_gt, height, width))
    return torch.zeros((nbytes,), dtype=torch.uint8, device=device)


def pq_boundary_accumulate(dilation, pred_2ch, gt_rgb, segments, cat_known, image_index, max_gt, workspace, tp, fp, fn, iou, status):
    """pq_accumulate with every pair scored by min(mask IoU, boundary IoU) (Boundary PQ, csrc/pq_boundary.hip): `dilation` >= 1 is the
    boundary width d of this image (dataset.boundary.boundary_dilation); workspace from pq_boundary_workspace, at least as large as
    this image needs. All other arguments as pq_accumulate. No host synchronisation, no allocation."""
    require_cuda(pred_2ch, gt_rgb, segments, cat_known, workspace, tp, fp, fn, iou, status)
    if pred_2ch.dtype != torch.uint8 or gt_rgb.dtype != torch.uint8 or pred_2ch.dim() != 3 or pred_2ch.shape[2] != 3 \
            or tuple(pred_2ch.shape) != tuple(gt_rgb.shape):
        raise ValueError("pq_boundary_accumulate: pred_2ch %s %s and gt_rgb %s %s must both be uint8 [H,W,3]"
                         % (tuple(pred_2ch.shape), pred_2ch.dtype, tuple(gt_rgb.shape), gt_rgb.dtype))
    if segments.dtype != torch.int64 or segments.dim() != 2 or segments.shape[1] != 4:
        raise ValueError("pq_boundary_accumulate: segments must be int64 [n,4]")
    for t, dt, n in ((cat_known, torch.uint8, 256), (tp, torch.int64, 256), (fp, torch.int64, 256), (fn, torch.int64, 256),
                     (iou, torch.float64, 256), (status, torch.int64, 1)):
        if t.dtype != dt or t.numel() != n or not t.is_contiguous():
            raise ValueError("pq_boundary_accumulate: accumulator / table of %d %s expected, got %s %s" % (n, dt, tuple(t.shape), t.dtype))
        written(t, dt, "pq_boundary_accumulate: accumulator / table")
    if int(dilation) < 1:
        raise ValueError("pq_boundary_accumulate: dilation %d < 1" % dilation)
    H, W = pred_2ch.shape[:2]
    need = int(lib().upsnet_pq_boundary_workspace_bytes(int(max_gt), H, W))
    if need == 0 or workspace.dtype != torch.uint8 or not workspace.is_contiguous() or workspace.numel() < need:
        raise ValueError("pq_boundary_accumulate: a uint8 workspace of at least %d bytes expected for max_gt %d and %dx%d, got %s %s"
                         % (need, max_gt, H, W, tuple(workspace.shape), workspace.dtype))
    written(workspace, torch.uint8, "pq_boundary_accumulate: workspace")     # (64-bit counters are carved from it at 16-byte steps)
    pred_2ch, gt_rgb, segments = dense(pred_2ch), dense(gt_rgb), dense(segments)
    check(lib().upsnet_pq_boundary_accumulate(stream(), int(dilation), ptr(pred_2ch), ptr(gt_rgb), H, W,
                                              ptr(segments) if segments.numel() else None, int(segments.shape[0]), ptr(cat_known),
                                              int(image_index), int(max_gt), ptr(workspace), ptr(tp), ptr(fp), ptr(fn), ptr(iou), ptr(status)),
          "pq_boundary_accumulate")


def pan_boundary_workspace_bytes(height, width):
    """Bytes of pan_boundary_map's workspace for a height x width image (no zeroing needed); ValueError for a size out of range."""
    nbytes = int(lib().upsnet_pan_boundary_workspace_bytes(int(height), int(width)))
    if nbytes == 0:
        raise ValueError("pan_boundary_map: image size %dx%d out of range" % (height, width))
    return nbytes


def pan_boundary_map(dilation, pred_2ch, gt_rgb, workspace, out):
    """The boundary bits of a panoptic label map pair (csrc/pq_boundary.hip) into out uint8 [H,W] (every byte written): bit 0 = GT
    boundary, bit 1 = pred boundary. A pixel is boundary unless the (2 * dilation + 1)^2 window centred on it lies inside the image and
    holds the pixel's own label (GT: the PNG id; pred: cat * 256 + inst, all cat == 255 pixels one VOID label). Either map, not both,
    may be None (its bit stays 0); workspace: uint8, at least pan_boundary_workspace_bytes(H, W). A non-contiguous map is copied.
    No host synchronisation; dataset.boundary.panoptic_boundary allocates and calls this."""
    maps = [m for m in (pred_2ch, gt_rgb) if m is not None]
    if not maps:
        raise ValueError("pan_boundary_map: neither pred_2ch nor gt_rgb given")
    require_cuda(workspace, out, *maps)
    for m in maps:
        if m.dtype != torch.uint8 or m.dim() != 3 or m.shape[2] != 3 or tuple(m.shape) != tuple(maps[0].shape):
            raise ValueError("pan_boundary_map: maps must be uint8 [H,W,3] of one shape, got %s %s" % (tuple(m.shape), m.dtype))
    if int(dilation) < 1:
        raise ValueError("pan_boundary_map: dilation %d < 1" % dilation)
    H, W = maps[0].shape[:2]
    nbytes = pan_boundary_workspace_bytes(H, W)
    if workspace.dtype != torch.uint8 or not workspace.is_contiguous() or workspace.numel() < nbytes:
        raise ValueError("pan_boundary_map: a uint8 workspace of at least %d bytes expected, got %s %s"
                         % (nbytes, tuple(workspace.shape), workspace.dtype))
    written(workspace, torch.uint8, "pan_boundary_map: workspace")
    if out.dtype != torch.uint8 or tuple(out.shape) != (H, W) or not out.is_contiguous():
        raise ValueError("pan_boundary_map: out must be a contiguous uint8 [%d,%d], got %s %s" % (H, W, tuple(out.shape), out.dtype))
    written(out, torch.uint8, "pan_boundary_map: out")
    pred_2ch, gt_rgb = dense(pred_2ch), dense(gt_rgb)
    with torch.cuda.device(out.device):
        check(lib().upsnet_pan_boundary_map(stream(), int(dilation), ptr(pred_2ch) if pred_2ch is not None else None,
                                            ptr(gt_rgb) if gt_rgb is not None else None, H, W, ptr(workspace), ptr(out)), "pan_boundary_map")
    return out


def confusion_accumulate(gt_label, pred_label, class_num, ignore_label, confusion):
    """get_confusion_matrix on the device, added into confusion int64 [class_num, class_num]: gt_label / pred_label uint8 of one
    shape; pixels with gt == ignore_label dropped (-1: none); index gt * C + pred counted iff < C^2 (pred >= C aliases, as
    np.bincount does in the reference)."""
    require_cuda(gt_label, pred_label, confusion)
    if gt_label.dtype != torch.uint8 or pred_label.dtype != torch.uint8 or gt_label.shape != pred_label.shape:
        raise ValueError("confusion_accumulate: gt %s %s and pred %s %s must both be uint8 of one shape"
                         % (tuple(gt_label.shape), gt_label.dtype, tuple(pred_label.shape), pred_label.dtype))
    if confusion.dtype != torch.int64 or tuple(confusion.shape) != (class_num, class_num) or not confusion.is_contiguous():
        raise ValueError("confusion_accumulate: confusion must be a contiguous int64 [%d,%d] tensor" % (class_num, class_num))
    written(confusion, torch.int64, "confusion_accumulate: confusion")
    gt_label, pred_label = dense(gt_label), dense(pred_label)
    check(lib().upsnet_confusion_accumulate(stream(), ptr(gt_label), ptr(pred_label), int(gt_label.numel()), int(class_num),
                                            int(ignore_label), ptr(confusion)), "confusion_accumulate")
    return confusion


def mask_roi_dedup(a_src, a_cls, a_num, b_src, b_cls, b_boxes, b_num):
    """Rows of the B detections inside [A ; unmatched of B] (matching on (source ROI, class)). Returns (map int32 [capB],
    extra_boxes [capB,5], num_extra device int32 [1])."""
    require_cuda(a_src, b_src, b_boxes)
    cap_a, cap_b = a_src.shape[0], b_src.shape[0]
    dev = b_boxes.device
    mp = torch.empty((cap_b,), dtype=torch.int32, device=dev)
    extra = torch.empty((cap_b, 5), dtype=torch.float32, device=dev)
    n_extra = torch.empty((1,), dtype=torch.int32, device=dev)
    a_src, a_cls, a_num = i32c(a_src), i64c(a_cls), i32c(a_num)
    b_src, b_cls, b_boxes, b_num = i32c(b_src), i64c(b_cls), f32c(b_boxes), i32c(b_num)
    check(lib().upsnet_mask_roi_dedup(stream(), ptr(a_src), ptr(a_cls), ptr(a_num), cap_a, ptr(b_src), ptr(b_cls), ptr(b_boxes),
                                      ptr(b_num), cap_b, ptr(mp), ptr(extra), ptr(n_extra)), "mask_roi_dedup")
    return mp, extra, n_extra


# ----------------------------------------------------------------------------- Winograd F(2x2,3x3)
def pack_winograd_weight(weight, tn32=False):
    """[Cout,Cin,3,3] -> (U = G g G^T in the kernel's fragment order, 16*Cin*ldw floats, ldw). tn32: the order of the 32-channel
    workgroup form for any Cout (conv2d_winograd_multi(..., tn32=True))."""
    require_cuda(weight)
    weight = f32c(weight)
    Cout, Cin, kh, kw = weight.shape
    if (kh, kw) != (3, 3):
        raise RuntimeError("pack_winograd_weight: kernel must be 3x3")
    if tn32:
        ldw = (Cout + 31) // 32 * 32
        wp = torch.empty((16 * Cin, ldw), dtype=torch.float32, device=weight.device)
        check(lib().upsnet_conv_pack_weight_winograd_tn32(stream(), ptr(weight), Cout, Cin, ldw, ptr(wp)), "conv_pack_weight_winograd_tn32")
        return wp, ldw
    ldw = 32 if Cout <= 32 else (Cout + 63) // 64 * 64   # 64 output channels per workgroup; narrow heads: the 32-channel form
    wp = torch.empty((16 * Cin, ldw), dtype=torch.float32, device=weight.device)
    check(lib().upsnet_conv_pack_weight_winograd(stream(), ptr(weight), Cout, Cin, ldw, ptr(wp)), "conv_pack_weight_winograd")
    return wp, ldw


def conv2d_winograd_splitk(x, wpack, ldw, bias, cout, ksplit, relu=False, residual=None):
    """conv2d_winograd for one small map with the K walk split over `ksplit` workgroups per tile (+ the shared reduce kernel)."""
    require_cuda(x, wpack)
    wpack = f32c(wpack)
    x = nhwc(x.float())
    N, C, H, W = x.shape
    out = _nhwc_out(N, cout, H, W, x.device)
    res = None
    if residual is not None:
        res = nhwc(residual.float())
        if tuple(res.shape) != tuple(out.shape):
            raise RuntimeError("conv2d_winograd_splitk: residual shape %s != %s" % (tuple(res.shape), tuple(out.shape)))
    ws = _ws(lib().upsnet_conv2d_splitk_workspace_bytes(N, H, W, int(cout), 3, 3, 1, 1, int(ksplit)), x.device)
    ev0 = _prof_begin()
    bias = None if bias is None else f32c(bias)
    check(lib().upsnet_conv2d_winograd_nhwc_f32_splitk(stream(), ptr(x), ptr(res), ptr(out), N, H, W, C, ptr(wpack), int(ldw),
                                                       ptr(bias), int(cout), int(bool(relu)), int(ksplit),
                                                       ptr(ws)), "conv2d_winograd_nhwc_f32_splitk")
    if ev0 is not None:
        npix = N * H * W
        _prof_end(ev0, 'conv', 2.0 * cout * C * 9 * npix, 4.0 * (C * npix + cout * npix * (2 if res is not None else 1) + cout * C * 9),
                  "winograd split-K x%d 3x3/1 %d->%d %s" % (ksplit, C, cout, (N, H, W)))
    return out


def conv2d_winograd_tail(x, wpack, ldw, wpack32, ldw32, bias, cout, n_main, relu=False):
    """3x3 / stride 1 / pad 1 Winograd convolution of a batch in ONE launch of two workgroup forms (csrc/conv_wino.hip,
    conv_wino16_tail_f32_kernel): images [0, n_main) on 32 x 64 tiles, the rest on 32 x 32 tiles (wpack32 from
    pack_winograd_weight(w, tn32=True)). Bit-identical to conv2d_winograd_multi([x], ...)."""
    require_cuda(wpack, wpack32, x)
    wpack, wpack32 = f32c(wpack), f32c(wpack32)
    x = nhwc(x.float())
    N, C, H, W = x.shape
    out = _nhwc_out(N, cout, H, W, x.device)
    ev0 = _prof_begin()
    bias = None if bias is None else f32c(bias)
    check(lib().upsnet_conv2d_winograd_nhwc_f32_tail(stream(), ptr(x), ptr(out), int(N), int(n_main), int(H), int(W), int(C), ptr(wpack), int(ldw),
                                                     ptr(wpack32), int(ldw32), ptr(bias), int(cout),
                                                     int(bool(relu))), "conv2d_winograd_nhwc_f32_tail")
    if ev0 is not None:
        npix = N * H * W
        _prof_end(ev0, 'conv', 2.0 * cout * C * 9 * npix, 4.0 * (C * npix + cout * npix + cout * C * 9),
                  "winograd 3x3/1 %d->%d [%s] tail %d" % (C, cout, (N, H, W), N - n_main))
    return out


def conv2d_winograd_multi(xs, wpack, ldw, bias, cout, relu=False, residuals=None, outs=None, tn32=False):
    """3x3 / stride 1 / pad 1 convolution of up to 5 maps (shared weights) by fused Winograd F(2x2,3x3); same contract as
    conv2d_nhwc_multi. outs: caller-provided channels_last outputs (e.g. batch slices of one tensor); tn32: the 32-channel workgroup
    form (wpack from pack_winograd_weight(w, tn32=True))."""
    require_cuda(wpack, *xs)
    wpack = f32c(wpack)
    assert 1 <= len(xs) <= 5
    xs = [nhwc(x.float()) for x in xs]
    cin = xs[0].shape[1]
    given, outs, ress = outs, [], None
    for i, x in enumerate(xs):
        N, C, H, W = x.shape
        if C != cin:
            raise RuntimeError("conv2d_winograd_multi: channel mismatch")
        if given is not None:
            o = given[i]
            if tuple(o.shape) != (N, cout, H, W) or o.dtype != torch.float32 or not o.permute(0, 2, 3, 1).is_contiguous():
                raise RuntimeError("conv2d_winograd_multi: outs[%d] must be a channels_last fp32 [%d,%d,%d,%d]" % (i, N, cout, H, W))
            outs.append(o)
        else:
            outs.append(_nhwc_out(N, cout, H, W, x.device))
    if residuals is not None:
        ress = [nhwc(r.float()) for r in residuals]
        for r, o in zip(ress, outs):
            if tuple(r.shape) != tuple(o.shape):
                raise RuntimeError("conv2d_winograd: residual shape %s != %s" % (tuple(r.shape), tuple(o.shape)))
    ev0 = _prof_begin()
    fn = lib().upsnet_conv2d_winograd_nhwc_f32_tn32 if tn32 else lib().upsnet_conv2d_winograd_nhwc_f32
    bias = None if bias is None else f32c(bias)
    check(fn(stream(), len(xs), ptr_array(xs), ptr_array(ress) if ress is not None else None,
             ptr_array(outs), int_array([x.shape[0] for x in xs]), int_array([x.shape[2] for x in xs]),
             int_array([x.shape[3] for x in xs]), int(cin), ptr(wpack), int(ldw),
             ptr(bias), int(cout), int(bool(relu))),
          "conv2d_winograd_nhwc_f32")
    if ev0 is not None:
        npix = sum(o.shape[0] * o.shape[2] * o.shape[3] for o in outs)
        # algorithmic work of the convolution (direct-form flops), as for the direct kernel
        _prof_end(ev0, 'conv', 2.0 * cout * cin * 9 * npix, 4.0 * (cin * npix + cout * npix * (2 if ress is not None else 1) + cout * cin * 9),
                  "winograd 3x3/1 %d->%d %s%s%s" % (cin, cout, [tuple(x.shape[0:1] + x.shape[2:]) for x in xs],
                                                    " +res" if ress is not None else "", " tn32" if tn32 else ""))
    return outs


def pack_winograd36_weight(weight):
    """[Cout,Cin,3,3] -> (U = G g G^T of Winograd F(4x4,3x3) in the fragment order of csrc/conv_wino36.hip, 36*Cin*ldw floats, ldw)."""
    require_cuda(weight)
    weight = f32c(weight)
    Cout, Cin, kh, kw = weight.shape
    if (kh, kw) != (3, 3) or Cin % 32:
        raise RuntimeError("pack_winograd36_weight: 3x3 kernel and Cin %% 32 == 0")
    ldw = (Cout + 63) // 64 * 64
    wp = torch.empty((36 * Cin, ldw), dtype=torch.float32, device=weight.device)
    check(lib().upsnet_conv_pack_weight_winograd36(stream(), ptr(weight), Cout, Cin, ldw, ptr(wp)), "conv_pack_weight_winograd36")
    return wp, ldw


def conv2d_winograd36_multi(xs, wpack, ldw, bias, cout, relu=False, outs=None):
    """3x3 / stride 1 / pad 1 convolution (+ bias, ReLU) of up to 5 maps (shared weights) by Winograd F(4x4,3x3): the contract of
    conv2d_winograd_multi without residuals (csrc/conv_wino36.hip)."""
    require_cuda(wpack, *xs)
    wpack = f32c(wpack)
    assert 1 <= len(xs) <= 5
    xs = [nhwc(x.float()) for x in xs]
    cin = xs[0].shape[1]
    given, outs = outs, []
    for i, x in enumerate(xs):
        N, C, H, W = x.shape
        if C != cin:
            raise RuntimeError("conv2d_winograd36_multi: channel mismatch")
        if given is not None:
            o = given[i]
            if tuple(o.shape) != (N, cout, H, W) or o.dtype != torch.float32 or not o.permute(0, 2, 3, 1).is_contiguous():
                raise RuntimeError("conv2d_winograd36_multi: outs[%d] must be a channels_last fp32 [%d,%d,%d,%d]" % (i, N, cout, H, W))
            outs.append(o)
        else:
            outs.append(_nhwc_out(N, cout, H, W, x.device))
    ev0 = _prof_begin()
    bias = None if bias is None else f32c(bias)
    check(lib().upsnet_conv2d_winograd36_nhwc_f32(stream(), len(xs), ptr_array(xs), ptr_array(outs), int_array([x.shape[0] for x in xs]),
                                                  int_array([x.shape[2] for x in xs]), int_array([x.shape[3] for x in xs]), int(cin), ptr(wpack),
                                                  int(ldw), ptr(bias), int(cout), int(bool(relu))),
          "conv2d_winograd36_nhwc_f32")
    if ev0 is not None:
        npix = sum(o.shape[0] * o.shape[2] * o.shape[3] for o in outs)
        _prof_end(ev0, 'conv', 2.0 * cout * cin * 9 * npix, 4.0 * (cin * npix + cout * npix + cout * cin * 9),
                  "winograd36 3x3/1 %d->%d %s" % (cin, cout, [tuple(x.shape[0:1] + x.shape[2:]) for x in xs]))
    return outs


def conv2d_winograd36_splitk(x, wpack, ldw, bias, cout, ksplit, relu=False):
    """conv2d_winograd36_multi for ONE map with the channel walk of every tile split over `ksplit` workgroups + the reduce / epilogue kernel
    (csrc/conv_wino36.hip, r13): maps with fewer 32-tile x 64-channel workgroups than CUs."""
    require_cuda(wpack, x)
    wpack = f32c(wpack)
    x = nhwc(x.float())
    N, cin, H, W = x.shape
    out = _nhwc_out(N, cout, H, W, x.device)
    ws = _ws(lib().upsnet_conv2d_winograd36_splitk_workspace_bytes(N, H, W, int(cout), int(ksplit)), x.device)
    ev0 = _prof_begin()
    bias = None if bias is None else f32c(bias)
    check(lib().upsnet_conv2d_winograd36_nhwc_f32_splitk(stream(), ptr(x), ptr(out), N, H, W, int(cin), ptr(wpack), int(ldw),
                                                         ptr(bias), int(cout), int(bool(relu)), int(ksplit), ptr(ws)),
          "conv2d_winograd36_nhwc_f32_splitk")
    if ev0 is not None:
        npix = N * H * W
        _prof_end(ev0, 'conv', 2.0 * cout * cin * 9 * npix, 4.0 * (cin * npix + cout * npix + cout * cin * 9),
                  "winograd36 split-K x%d 3x3/1 %d->%d %s" % (ksplit, cin, cout, (N, H, W)))
    return out


# ----------------------------------------------------------------------------- bf16 matrix-core convolution (opt-in)
def pack_conv_weight_bf16(weight, split=True):
    """[Cout,Cin,kh,kw] fp32 -> (hi, lo, ldw): bf16 [kh*kw*Cin/32, ldw, 32] (as int16 storage), ldw = Cout rounded up to 64.
    split=False ("bf16" mode) leaves lo = None."""
    require_cuda(weight)
    weight = f32c(weight)
    Cout, Cin, kh, kw = weight.shape
    ldw = (Cout + 127) // 128 * 128
    shape = (kh * kw * Cin // 32, ldw, 32)
    hi = torch.empty(shape, dtype=torch.bfloat16, device=weight.device)
    lo = torch.empty(shape, dtype=torch.bfloat16, device=weight.device) if split else None
    check(lib().upsnet_conv_pack_weight_bf16(stream(), ptr(weight), Cout, Cin, kh, kw, ldw, ptr(hi), ptr(lo)), "conv_pack_weight_bf16")
    return hi, lo, ldw


def conv2d_nhwc_bf16_multi(xs, whi, wlo, ldw, bias, cout, ksize, stride, pad, relu=False, residuals=None, residual_up=False,
                           out_dtype=torch.float32):
    """conv2d_nhwc_multi on the bf16 matrix cores: wlo None -> plain bf16 products, else the 3-term split (fp32-equivalent).
    residual_up (1x1 kernels): the residuals are at half resolution, added through a nearest x2 upsampling.
    Plain bf16 mode only: inputs / residuals may be torch.bfloat16 tensors (all maps of a launch alike) and out_dtype may be
    torch.bfloat16 -- bf16 activations between layers (the kernels then load / store 2-byte elements, no conversion pass)."""
    require_cuda(whi, *xs)
    whi, wlo = dense(whi), dense(wlo)
    assert 1 <= len(xs) <= 5
    in16 = xs[0].dtype == torch.bfloat16
    out16 = out_dtype == torch.bfloat16
    if (in16 or out16) and wlo is not None:
        raise RuntimeError("conv2d_nhwc_bf16_multi: bf16 tensors only in the plain bf16 mode")
    xs = [nhwc(x if (in16 and x.dtype == torch.bfloat16) else x.float()) for x in xs]
    if in16 and any(x.dtype != torch.bfloat16 for x in xs):
        raise RuntimeError("conv2d_nhwc_bf16_multi: mixed input dtypes in one launch")
    cin = xs[0].shape[1]
    outs, ress = [], None
    for x in xs:
        N, C, H, W = x.shape
        if C != cin:
            raise RuntimeError("conv2d_nhwc_bf16_multi: channel mismatch")
        Ho, Wo = (H + 2 * pad - ksize) // stride + 1, (W + 2 * pad - ksize) // stride + 1
        outs.append(torch.empty((N, Ho, Wo, cout), dtype=torch.bfloat16, device=x.device).permute(0, 3, 1, 2) if out16
                    else _nhwc_out(N, cout, Ho, Wo, x.device))
    res16 = False
    if residuals is not None:
        res16 = residuals[0].dtype == torch.bfloat16 and wlo is None
        ress = [nhwc(r if (res16 and r.dtype == torch.bfloat16) else r.float()) for r in residuals]
        if res16 and any(r.dtype != torch.bfloat16 for r in ress):
            raise RuntimeError("conv2d_nhwc_bf16_multi: mixed residual dtypes in one launch")
        for r, o in zip(ress, outs):
            want = (o.shape[0], o.shape[1], o.shape[2] // 2, o.shape[3] // 2) if residual_up else tuple(o.shape)
            if tuple(r.shape) != want:
                raise RuntimeError("conv2d_nhwc_bf16: residual shape %s != %s" % (tuple(r.shape), want))
    ev0 = _prof_begin()
    bias = None if bias is None else f32c(bias)
    check(lib().upsnet_conv2d_nhwc_bf16(stream(), len(xs), ptr_array(xs), ptr_array(ress) if ress is not None else None, ptr_array(outs),
                                        int_array([x.shape[0] for x in xs]), int_array([x.shape[2] for x in xs]),
                                        int_array([x.shape[3] for x in xs]), int(cin), ptr(whi), ptr(wlo), int(ldw),
                                        ptr(bias), int(cout), int(ksize), int(ksize), int(stride), int(pad),
                                        int(bool(relu)) | (2 if (residual_up and ress is not None) else 0) | (4 if in16 else 0) |
                                        (8 if out16 else 0) | (16 if res16 else 0)), "conv2d_nhwc_bf16")
    if ev0 is not None:
        npix = sum(o.shape[0] * o.shape[2] * o.shape[3] for o in outs)
        nin = sum(x.shape[0] * x.shape[2] * x.shape[3] for x in xs)
        _prof_end(ev0, 'conv_bf16', 2.0 * cout * cin * ksize * ksize * npix,
                  (2.0 if in16 else 4.0) * cin * nin + (2.0 if out16 else 4.0) * cout * npix +
                  ((2.0 if res16 else 4.0) * cout * npix * (0.25 if residual_up else 1.0) if ress is not None else 0.0) +
                  2.0 * cout * cin * ksize * ksize)
    return outs


def _bf16_fragments(w2d):
    """[Cout, K] fp32 -> bf16 in MFMA-fragment order [Cout/32][K/16][64 lanes][8] (lane = (k half) * 32 + row; see
    csrc/bottleneck_bf16.hip): one 16-byte load per lane and MFMA, straight from L2 into the A operand."""
    cout, k = w2d.shape
    return w2d.to(torch.bfloat16).view(cout // 32, 32, k // 16, 2, 8).permute(0, 2, 3, 1, 4).contiguous()


def pack_bottleneck_bf16(w1, w2, w3, b1, b2, b3):
    """Folded weights of an identity bottleneck ([Cm,C,1,1], [Cm,Cm,3,3], [C,Cm,1,1], biases) -> the operand pack of bottleneck_bf16."""
    require_cuda(w1, w2, w3)
    cm, c = w1.shape[0], w1.shape[1]
    if not (c == 4 * cm and tuple(w2.shape) == (cm, cm, 3, 3) and tuple(w3.shape) == (c, cm, 1, 1) and cm in (64, 128, 256, 512)):
        raise RuntimeError("pack_bottleneck_bf16: not an identity bottleneck of width 64/128/256/512")
    zeros = lambda n: torch.zeros(n, dtype=torch.float32, device=w1.device)
    return (_bf16_fragments(w1.detach().float().reshape(cm, c)),
            _bf16_fragments(w2.detach().float().permute(0, 2, 3, 1).reshape(cm, 9 * cm)),
            _bf16_fragments(w3.detach().float().reshape(c, cm)),
            zeros(cm) if b1 is None else f32c(b1.detach()), zeros(cm) if b2 is None else f32c(b2.detach()),
            zeros(c) if b3 is None else f32c(b3.detach()), cm)


def pack_bottleneck_proj_bf16(w1, w2, w3, wd, b1, b2, b3, bd):
    """Folded weights of a projection bottleneck ([Cm,Cin,1,1], [Cm,Cm,3,3], [C,Cm,1,1], projection [C,Cin,1,1], biases) -> the operand
    pack of bottleneck_proj_bf16: conv3 and the projection as one weight matrix [C, Cm + Cin], one bias b3 + bd."""
    require_cuda(w1, w2, w3, wd)
    cm, cin = w1.shape[0], w1.shape[1]
    c = 4 * cm
    if not (tuple(w2.shape) == (cm, cm, 3, 3) and tuple(w3.shape) == (c, cm, 1, 1) and tuple(wd.shape) == (c, cin, 1, 1) and
            (cm, cin) in ((64, 64), (128, 256), (256, 512))):
        raise RuntimeError("pack_bottleneck_proj_bf16: not the first bottleneck of res2 / res3 / res4")
    z = lambda b, n: torch.zeros(n, dtype=torch.float32, device=w1.device) if b is None else f32c(b.detach())
    w3d = torch.cat([w3.detach().float().reshape(c, cm), wd.detach().float().reshape(c, cin)], 1)
    return (_bf16_fragments(w1.detach().float().reshape(cm, cin)),
            _bf16_fragments(w2.detach().float().permute(0, 2, 3, 1).reshape(cm, 9 * cm)),
            _bf16_fragments(w3d), z(b1, cm), z(b2, cm), (z(b3, c) + z(bd, c)).contiguous(), cm, cin)


def bottleneck_proj_bf16(x, pack, stride):
    """relu(conv3(relu(conv2(relu(conv1_s(x))))) + proj_s(x)) of a stage's first bottleneck in one launch; x, result: bf16 channels_last."""
    w1, w2, w3d, b1, b2, b3d, cm, cin = pack
    require_cuda(x, w1)
    w1, w2, w3d, b1, b2, b3d = dense(w1), dense(w2), dense(w3d), f32c(b1), f32c(b2), f32c(b3d)
    if x.dtype != torch.bfloat16 or x.shape[1] != cin:
        raise RuntimeError("bottleneck_proj_bf16: expects a bf16 map of %d channels" % cin)
    x = nhwc(x)
    N, C, H, W = x.shape
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    out = torch.empty((N, Ho, Wo, 4 * cm), dtype=torch.bfloat16, device=x.device).permute(0, 3, 1, 2)
    ev0 = _prof_begin()
    check(lib().upsnet_bottleneck_proj_bf16(stream(), ptr(x), ptr(out), N, H, W, int(cin), int(cm), int(stride), ptr(w1), ptr(w2), ptr(w3d),
                                            ptr(b1), ptr(b2), ptr(b3d)), "bottleneck_proj_bf16")
    if ev0 is not None:
        k = cm * cin + 9 * cm * cm + 4 * cm * (cm + cin)
        _prof_end(ev0, 'bottleneck_bf16', 2.0 * k * N * Ho * Wo, 2.0 * C * N * Ho * Wo + 2.0 * 4 * cm * N * Ho * Wo + 2.0 * k)
    return out


def bottleneck_bf16(x, pack):
    """relu(conv3(relu(conv2(relu(conv1(x))))) + x) of an identity bottleneck in one launch; x, result: bf16 NHWC-strided NCHW."""
    w1, w2, w3, b1, b2, b3, cm = pack
    require_cuda(x, w1)
    w1, w2, w3, b1, b2, b3 = dense(w1), dense(w2), dense(w3), f32c(b1), f32c(b2), f32c(b3)
    if x.dtype != torch.bfloat16 or x.shape[1] != 4 * cm:
        raise RuntimeError("bottleneck_bf16: expects a bf16 map of %d channels" % (4 * cm))
    x = nhwc(x)
    N, C, H, W = x.shape
    out = torch.empty((N, H, W, C), dtype=torch.bfloat16, device=x.device).permute(0, 3, 1, 2)
    ev0 = _prof_begin()
    check(lib().upsnet_bottleneck_bf16(stream(), ptr(x), ptr(out), N, H, W, cm, ptr(w1), ptr(w2), ptr(w3), ptr(b1), ptr(b2), ptr(b3)),
          "bottleneck_bf16")
    if ev0 is not None:
        _prof_end(ev0, 'bottleneck_bf16', 2.0 * 17 * cm * cm * N * H * W, 2.0 * 2 * C * N * H * W + 2.0 * 17 * cm * cm)
    return out


def conv2d_nhwc_splitk(x, wpack, ldw, bias, cout, ksize, stride, pad, ksplit, relu=False, residual=None):
    """conv2d_nhwc for one small map with the K walk split over `ksplit` workgroups per tile (+ a reduce/epilogue kernel)."""
    require_cuda(x, wpack)
    wpack = f32c(wpack)
    x = nhwc(x.float())
    N, C, H, W = x.shape
    Ho, Wo = (H + 2 * pad - ksize) // stride + 1, (W + 2 * pad - ksize) // stride + 1
    out = _nhwc_out(N, cout, Ho, Wo, x.device)
    res = None
    if residual is not None:
        res = nhwc(residual.float())
        if tuple(res.shape) != tuple(out.shape):
            raise RuntimeError("conv2d_nhwc_splitk: residual shape %s != %s" % (tuple(res.shape), tuple(out.shape)))
    ws = _ws(lib().upsnet_conv2d_splitk_workspace_bytes(N, H, W, int(cout), int(ksize), int(ksize), int(stride), int(pad), int(ksplit)), x.device)
    ev0 = _prof_begin()
    bias = None if bias is None else f32c(bias)
    check(lib().upsnet_conv2d_nhwc_f32_splitk(stream(), ptr(x), ptr(res), ptr(out), N, H, W, C, ptr(wpack), int(ldw),
                                              ptr(bias), int(cout), int(ksize), int(ksize), int(stride),
                                              int(pad), int(bool(relu)), int(ksplit), ptr(ws)), "conv2d_nhwc_f32_splitk")
    if ev0 is not None:
        npix = N * Ho * Wo
        _prof_end(ev0, 'conv', 2.0 * cout * C * ksize * ksize * npix,
                  4.0 * (C * N * H * W + cout * npix * (2 if res is not None else 1) + cout * C * ksize * ksize),
                  "split-K x%d %dx%d/%d %d->%d %s" % (ksplit, ksize, ksize, stride, C, cout, (N, H, W)))
    return out


# ----------------------------------------------------------------------------- proposal recall (evaluate_box_proposals)
PROPOSAL_RECALL_MAX_GT = 4096   # GT boxes per problem (csrc/prop_eval.hip keeps one LDS key per GT column)


def proposal_recall_workspace_bytes(num_problems, total_proposals):
    return int(lib().upsnet_proposal_recall_workspace_bytes(int(num_problems), int(total_proposals)))


def proposal_recall(problems, proposals, gt_boxes, max_gt, total_proposals, workspace, out):
    """The greedy matching of evaluate_box_proposals for a batch of (image, area, limit) problems, one launch (csrc/prop_eval.hip;
    include/upsnet_hip.h: upsnet_proposal_recall for the table layout). problems int64 [n, 6], proposals / gt_boxes float32 [., 4],
    workspace uint8 of proposal_recall_workspace_bytes(n, total_proposals) bytes and out float32: caller-owned device tensors (the
    evaluator, dataset/proposal_eval.py, sizes and owns them); out is fully written. No host synchronisation."""
    require_cuda(problems, proposals, gt_boxes, workspace, out)
    if problems.dtype != torch.int64 or problems.dim() != 2 or problems.shape[1] != 6 or not problems.is_contiguous():
        raise ValueError("proposal_recall: problems must be a contiguous int64 [n, 6] table, got %s %s" % (problems.dtype, tuple(problems.shape)))
    for name, b in (('proposals', proposals), ('gt_boxes', gt_boxes)):
        if b.dtype != torch.float32 or b.dim() != 2 or b.shape[1] != 4 or not b.is_contiguous():
            raise ValueError("proposal_recall: %s must be contiguous float32 [., 4], got %s %s" % (name, b.dtype, tuple(b.shape)))
    if not 0 <= int(max_gt) <= PROPOSAL_RECALL_MAX_GT:
        raise ValueError("proposal_recall: %d GT boxes in a problem (at most %d)" % (int(max_gt), PROPOSAL_RECALL_MAX_GT))
    n = int(problems.shape[0])
    problems, proposals, gt_boxes = aligned(problems), aligned(proposals), aligned(gt_boxes)
    written(workspace, None, "proposal_recall: workspace")
    if workspace.numel() * workspace.element_size() < proposal_recall_workspace_bytes(n, total_proposals):
        raise ValueError("proposal_recall: workspace of %d bytes, %d needed" % (workspace.numel() * workspace.element_size(),
                                                                             proposal_recall_workspace_bytes(n, total_proposals)))
    written(out, torch.float32, "proposal_recall: out")
    check(lib().upsnet_proposal_recall(stream(), n, ptr(problems), ptr(proposals), ptr(gt_boxes), int(max_gt), int(total_proposals),
                                       ptr(workspace), ptr(out)), "proposal_recall")
    return out


# ----------------------------------------------------------------------------- evaluation ground truth from the raw downloads
def gt_prepare_workspace(device, seg_capacity=4096):
    """dataset/gt_prepare.py: the zeroed workspace of gt_prepare / gt_prepare_launch."""
    from .dataset import gt_prepare as impl
    return impl.gt_prepare_workspace(device, seg_capacity)


def gt_prepare_launch(ids, tables, label_ids=None, seg_capacity=4096, trans_capacity=None, workspace=None):
    """dataset/gt_prepare.py: one Cityscapes instanceIds map -> train-id map, panoptic RGB, segment table, run lists and status words
    on the device (csrc/gt_prepare.hip), without synchronising."""
    from .dataset import gt_prepare as impl
    return impl.gt_prepare_launch(ids, tables, label_ids, seg_capacity, trans_capacity, workspace)


def gt_prepare(ids, tables, label_ids=None, seg_capacity=4096, trans_capacity=None, workspace=None):
    """dataset/gt_prepare.py: gt_prepare_launch, synchronised, cut to its counts; ValueError for an overflow, a value beyond 16 bits
    or a labelIds map that disagrees."""
    from .dataset import gt_prepare as impl
    return impl.gt_prepare(ids, tables, label_ids, seg_capacity, trans_capacity, workspace)


def panoptic_semantic(rgb, segments_info):
    """dataset/gt_prepare.py: COCO panoptic PNG content -> semantic map of category ids (255: id 0 and ids without a segment),
    channel 0 of csrc/pan_format.hip's relabel kernel."""
    from .dataset import gt_prepare as impl
    return impl.panoptic_semantic(rgb, segments_info)


# ----------------------------------------------------------------------------- test-time augmentation: the merge step (csrc/tta.hip)
TTA_MAX_AUG = 8


def tta_seg_merge(maps, q, resized_w, flip, cell):
    """tta.py: the semantic score maps of the augmentations resampled into the frame of maps[0] and averaged."""
    from . import tta as impl
    return impl.seg_merge(maps, q, resized_w, flip, cell)


def tta_roi_union(rois, delta, prob, num_rois_dev, r, resized_w, flip):
    """tta.py: every augmentation's valid proposal rows, mapped to the base frame and packed behind each other."""
    from . import tta as impl
    return impl.roi_union(rois, delta, prob, num_rois_dev, r, resized_w, flip)


def tta_boxes_to_aug(boxes, q, resized_w, flip):
    """tta.py: boxes of the base frame mapped into every augmentation's frame, [A,n,5]."""
    from . import tta as impl
    return impl.boxes_to_aug(boxes, q, resized_w, flip)


def tta_mask_merge(logits, flip):
    """tta.py: the augmentations' mask logits averaged, flipped ones mirrored left to right."""
    from . import tta as impl
    return impl.mask_merge(logits, flip)


def box_vote(rois, bbox_delta, cls_prob, im_info, boxes, cls, num, vote_score_thresh, vote_iou_thresh, reg_weights,
             num_rois_dev=None, clip_boxes=True):
    """tta.py: score-weighted box voting on the output of mask_roi, voted [cap,5] (csrc/box_vote.hip)."""
    from . import tta as impl
    return impl.box_vote(rois, bbox_delta, cls_prob, im_info, boxes, cls, num, vote_score_thresh, vote_iou_thresh, reg_weights,
                         num_rois_dev, clip_boxes)


def mask_roi_soft(rois, bbox_delta, cls_prob, im_info, score_thresh, nms_thresh, max_det, reg_weights, method, sigma, floor,
                  num_rois_dev=None, clip_boxes=True):
    """tta.py: the class-wise detection selection with soft-NMS, (boxes [cap,5], scores [cap] decayed, cls [cap] int64, src [cap] int32,
    num device int32) like mask_roi (csrc/detect.hip mroi_soft_kernel)."""
    from . import tta as impl
    return impl.mask_roi_soft(rois, bbox_delta, cls_prob, im_info, score_thresh, nms_thresh, max_det, reg_weights, method, sigma, floor,
                              num_rois_dev, clip_boxes)


def pan_track_step(pan_2ch, iou_thresh, max_age, frame, workspace, memory, out, host_table=None):
    """One tracker step on the device (include/upsnet_hip.h, csrc/pan_track.hip): pan_2ch uint8 [H,W,3]; memory int16 [H,W] holding
    the uint16 track keys (c << 8 | j, 0 = none), updated in place; workspace: upsnet_pan_track_workspace_bytes(H, W) bytes, zeroed
    once; out: uint8 [H,W,3], the tracked map; host_table: pinned int32 host memory that takes the table's head (8 ints) and its first
    rows (8 ints each), as many as fit, by an asynchronous copy (None: no copy). Three launches, no host synchronisation, no allocation
    (dataset/pan_track.PanopticTracker owns the buffers)."""
    return _pan_track_step("pan_track_step", pan_2ch, iou_thresh, max_age, frame, workspace, memory, out, host_table, None)


def pan_track_step_motion(pan_2ch, iou_thresh, max_age, frame, workspace, memory, out, motion_workspace, host_table=None):
    """pan_track_step with constant-velocity motion prediction: motion_workspace is a contiguous uint8 device tensor of
    upsnet_pan_track_motion_workspace_bytes(H, W) bytes, 16-byte aligned and zeroed once; it holds the tracks' centroids and velocities
    and the step's predicted memory. Seven launches, no host synchronisation, no allocation."""
    require_cuda(motion_workspace)
    if motion_workspace.dtype != torch.uint8 or not motion_workspace.is_contiguous() or motion_workspace.data_ptr() % 16:
        raise ValueError("pan_track_step_motion: motion_workspace must be a contiguous, 16-byte aligned uint8 tensor")
    return _pan_track_step("pan_track_step_motion", pan_2ch, iou_thresh, max_age, frame, workspace, memory, out, host_table, motion_workspace)


def _pan_track_step(what, pan_2ch, iou_thresh, max_age, frame, workspace, memory, out, host_table, motion_workspace):
    require_cuda(pan_2ch, workspace, memory, out)
    if pan_2ch.dtype != torch.uint8 or pan_2ch.dim() != 3 or pan_2ch.shape[2] != 3 or not pan_2ch.is_contiguous():
        raise ValueError("pan_track_step: pan_2ch must be contiguous uint8 [H,W,3], got %s %s" % (tuple(pan_2ch.shape), pan_2ch.dtype))
    H, W = int(pan_2ch.shape[0]), int(pan_2ch.shape[1])
    if out.dtype != torch.uint8 or tuple(out.shape) != (H, W, 3) or not out.is_contiguous():
        raise ValueError("pan_track_step: out must be contiguous uint8 [%d,%d,3], got %s %s" % (H, W, tuple(out.shape), out.dtype))
    if memory.dtype != torch.int16 or tuple(memory.shape) != (H, W) or not memory.is_contiguous():
        raise ValueError("pan_track_step: memory must be a contiguous int16 [%d,%d] tensor, got %s %s" % (H, W, tuple(memory.shape), memory.dtype))
    written(workspace, None, "pan_track_step: workspace")
    written(motion_workspace, None, "pan_track_step: motion_workspace")
    need = int(lib().upsnet_pan_track_workspace_bytes(H, W))
    if need == 0 or workspace.numel() * workspace.element_size() < need:
        raise ValueError("pan_track_step: workspace too small for (or no workspace exists for) a frame of %d x %d" % (H, W))
    host_rows = 0
    if host_table is not None:
        if host_table.is_cuda or not host_table.is_pinned() or host_table.dtype != torch.int32 or host_table.numel() < 8 \
                or not host_table.is_contiguous():
            raise ValueError("pan_track_step: host_table must be contiguous pinned int32 host memory of at least 8 ints")
        host_rows = (host_table.numel() - 8) // 8
    pan_2ch = aligned(pan_2ch)
    args = (stream(), ptr(pan_2ch), H, W, float(iou_thresh), int(max_age), int(frame), ptr(workspace), ptr(memory), ptr(out),
            ptr(host_table), host_rows)
    if motion_workspace is None:
        check(lib().upsnet_pan_track_step(*args), what)
    else:
        if motion_workspace.numel() < int(lib().upsnet_pan_track_motion_workspace_bytes(H, W)):
            raise ValueError("pan_track_step_motion: motion_workspace too small for a frame of %d x %d" % (H, W))
        check(lib().upsnet_pan_track_step_motion(*(args + (ptr(motion_workspace),))), what)
    return out


def pan_stable_colors(pred_2ch, cat_table, mode, out):
    """Frame-stable colours of a 2-channel map (csrc/pan_track.hip): mode 0 the PNG colour (category, instance, 1), mode 1 the picture
    colour of (category, instance) from cat_table (int32 [256] device tensor, pan_format.category_table; None in mode 0), painted into
    out, H * W * 3 contiguous uint8."""
    require_cuda(pred_2ch, cat_table, out)
    if pred_2ch.dtype != torch.uint8 or pred_2ch.dim() != 3 or pred_2ch.shape[2] != 3 or not pred_2ch.is_contiguous():
        raise ValueError("pan_stable_colors: pred_2ch must be contiguous uint8 [H,W,3], got %s %s" % (tuple(pred_2ch.shape), pred_2ch.dtype))
    H, W = int(pred_2ch.shape[0]), int(pred_2ch.shape[1])
    if out.dtype != torch.uint8 or out.numel() != H * W * 3 or not out.is_contiguous():
        raise ValueError("pan_stable_colors: out must be a contiguous uint8 tensor of %d bytes" % (H * W * 3))
    cat_table, pred_2ch = i32c(cat_table), aligned(pred_2ch)
    check(lib().upsnet_pan_stable_colors(stream(), ptr(pred_2ch), H, W, ptr(cat_table), int(mode), ptr(out)), "pan_stable_colors")
    return out


def pan_components_workspace(height, width, device):
    """Workspace of pan_components for maps of height x width pixels. The kernels initialise what they read: its contents never
    matter, and one workspace serves every map of that size (or a smaller one)."""
    nbytes = int(lib().upsnet_pan_components_workspace_bytes(int(height), int(width)))
    if nbytes == 0:
        raise ValueError("pan_components: a map of %d x %d pixels has no workspace: H * W must lie in 1..2^24" % (height, width))
    return torch.zeros((nbytes,), dtype=torch.uint8, device=device)


def pan_components(pan_2ch, min_area=0, connectivity=8, keep_largest=True, *, want_labels=False, workspace=None, out=None, labels=None):
    """Connected components of a 2-channel map and the removal of small fragments (include/upsnet_hip.h states the rule;
    csrc/pan_components.hip). pan_2ch: contiguous uint8 [H,W,3] device tensor. A component (pixels of one (category,
    instance) key connected under `connectivity`, 4 or 8; category 255 is VOID and in none) of fewer than min_area pixels becomes VOID
    (255, 0, byte 2 kept) unless keep_largest and it is the largest of its key (ties: the one that starts first). min_area = 0 only
    labels.

    Returns (out, stats, labels): out uint8 [H,W,3]; stats int32 [4] = distinct keys, components, components removed, pixels removed;
    labels int32 [H,W] with want_labels (or labels=), else None: the smallest linear index y * W + x of the pixel's component in the
    INPUT map, -1 for VOID. All device tensors; five launches, nothing waits for the host. workspace= (pan_components_workspace; any
    contents), out= (may be pan_2ch itself) and labels= are taken instead of being allocated.
    ValueError before any launch: a wrong dtype, shape or size, connectivity other than 4 or 8, a negative or non-integer min_area."""
    return _pan_clean("pan_components", lib().upsnet_pan_components_workspace_bytes, lib().upsnet_pan_components, 4, pan_2ch,
                      min_area, connectivity, keep_largest, want_labels, workspace, out, labels)


def pan_absorb_workspace(height, width, device):
    """Workspace of pan_absorb for maps of height x width pixels: that of pan_components, one winner cell per pixel and the vote table
    of 2 * H * W slots. The kernels initialise what they read: its contents never matter, and one workspace serves every map of that
    size (or a smaller one)."""
    nbytes = int(lib().upsnet_pan_absorb_workspace_bytes(int(height), int(width)))
    if nbytes == 0:
        raise ValueError("pan_absorb: a map of %d x %d pixels has no workspace: H * W must lie in 1..2^24" % (height, width))
    return torch.zeros((nbytes,), dtype=torch.uint8, device=device)


def pan_absorb(pan_2ch, min_area=0, connectivity=8, keep_largest=True, *, want_labels=False, workspace=None, out=None, labels=None):
    """pan_components with the removed components (fragments) absorbed instead of voided (include/upsnet_hip.h states the rule;
    csrc/pan_components.hip): a fragment takes the (category, instance) of the kept segment it shares the longest border
    with -- one vote per pixel edge between a fragment pixel and a kept pixel, the most votes win, ties to the smaller key -- and
    becomes VOID (255, 0, byte 2 kept) only where it has no such border. One round: a fragment that touches only other fragments, VOID,
    the image border or kept pixels across a corner becomes VOID. Which components are fragments is pan_components' rule on the same
    arguments; min_area = 0 only labels.

    Returns (out, stats, labels): out uint8 [H,W,3]; stats int32 [8] = distinct keys, components, fragments, fragment pixels (the four
    of pan_components), fragments absorbed, pixels absorbed, distinct (fragment, donor key) pairs voted for, vote table overflow (0: the
    table is sized so that it cannot fill; were it ever 1, out is a copy of pan_2ch, and the caller that reads stats must raise);
    labels as pan_components. All device tensors; eight launches, nothing waits for the host. workspace= (pan_absorb_workspace; any
    contents), out= (may be pan_2ch itself) and labels= are taken instead of being allocated.
    ValueError before any launch: a wrong dtype, shape or size, connectivity other than 4 or 8, a negative or non-integer min_area."""
    return _pan_clean("pan_absorb", lib().upsnet_pan_absorb_workspace_bytes, lib().upsnet_pan_absorb, 8, pan_2ch, min_area,
                      connectivity, keep_largest, want_labels, workspace, out, labels)


def _pan_clean(name, workspace_bytes, entry, nstats, pan_2ch, min_area, connectivity, keep_largest, want_labels, workspace, out, labels):
    """pan_components and pan_absorb: one set of argument checks and allocations, worded with the caller's name; `entry` (the C entry
    point, `workspace_bytes` its workspace size) fills int32 [nstats]."""
    if pan_2ch.dtype != torch.uint8 or pan_2ch.dim() != 3 or pan_2ch.shape[2] != 3 or not pan_2ch.is_contiguous():
        raise ValueError("%s: pan_2ch must be contiguous uint8 [H,W,3], got %s %s" % (name, tuple(pan_2ch.shape), pan_2ch.dtype))
    if connectivity not in (4, 8):
        raise ValueError("%s: connectivity must be 4 or 8, got %r" % (name, connectivity))
    if isinstance(min_area, bool) or int(min_area) != min_area or min_area < 0 or min_area > 0x7fffffff:
        raise ValueError("%s: min_area must be an integer >= 0, got %r" % (name, min_area))
    H, W = int(pan_2ch.shape[0]), int(pan_2ch.shape[1])
    if H * W == 0 or H * W > (1 << 24):
        raise ValueError("%s: a map of %d x %d pixels: H * W must lie in 1..2^24" % (name, H, W))
    if out is not None and (out.dtype != torch.uint8 or tuple(out.shape) != (H, W, 3) or not out.is_contiguous()):
        raise ValueError("%s: out must be contiguous uint8 [%d,%d,3], got %s %s" % (name, H, W, tuple(out.shape), out.dtype))
    if labels is not None and (labels.dtype != torch.int32 or tuple(labels.shape) != (H, W) or not labels.is_contiguous()
                               or labels.data_ptr() % 16):
        raise ValueError("%s: labels must be a contiguous, 16-byte aligned int32 [%d,%d] tensor, got %s %s"
                         % (name, H, W, tuple(labels.shape), labels.dtype))
    require_cuda(pan_2ch, workspace, out, labels)      # (after the checks that need no device)
    need = int(workspace_bytes(H, W))
    if workspace is not None and (workspace.dtype != torch.uint8 or not workspace.is_contiguous() or workspace.numel() < need
                                  or workspace.data_ptr() % 16):
        raise ValueError("%s: workspace must be a contiguous, 16-byte aligned uint8 tensor of at least %d bytes for a map "
                         "of %d x %d" % (name, need, H, W))
    dev = pan_2ch.device
    with torch.cuda.device(dev):
        if workspace is None:
            workspace = torch.zeros((need,), dtype=torch.uint8, device=dev)
        if out is None:
            out = pan_2ch.clone()
        if labels is None and want_labels:
            labels = torch.zeros((H, W), dtype=torch.int32, device=dev)
        stats = torch.zeros((nstats,), dtype=torch.int32, device=dev)
        pan_2ch = aligned(pan_2ch)
        check(entry(stream(), ptr(pan_2ch), H, W, int(connectivity), int(min_area), int(bool(keep_largest)), ptr(workspace), ptr(out),
                    ptr(labels), ptr(stats)), name)
    return out, stats, labels


def _pan_conf_check(name, pan_2ch, conf=None):
    if pan_2ch.dtype != torch.uint8 or pan_2ch.dim() != 3 or pan_2ch.shape[2] != 3 or not pan_2ch.is_contiguous():
        raise ValueError("%s: pan_2ch must be contiguous uint8 [H,W,3], got %s %s" % (name, tuple(pan_2ch.shape), pan_2ch.dtype))
    H, W = int(pan_2ch.shape[0]), int(pan_2ch.shape[1])
    if H * W == 0 or H * W > (1 << 24):
        raise ValueError("%s: a map of %d x %d pixels: H * W must lie in 1..2^24" % (name, H, W))
    if conf is not None and (conf.dtype != torch.uint8 or tuple(conf.shape) != (H, W) or not conf.is_contiguous()):
        raise ValueError("%s: conf must be contiguous uint8 [%d,%d], got %s %s" % (name, H, W, tuple(conf.shape), conf.dtype))
    return H, W


def pan_segment_scores(pan_2ch, conf, *, workspace=None, table=None):
    """Area and confidence sum of every segment of a 2-channel map (include/upsnet_hip.h: upsnet_pan_segment_scores).
    pan_2ch contiguous uint8 [H,W,3], conf contiguous uint8 [H,W] (the panoptic confidence at the map's size). Returns the device
    table, an int32 tensor [4 + 3 * 65280] whose words are unsigned (sum_q can pass 2^31: read it through numpy's .view(np.uint32)):
    [0] = number of rows n, then n rows (key = category << 8 | instance, area, sum_q) from word 4 on, in ascending key; VOID (category
    255) has no row. The score of a row is sum_q / (255 * area)
    (dataset/pan_confidence.py forms it in double on the host). Three launches, nothing waits for the host. workspace= (uint8, at
    least upsnet_pan_segment_scores_workspace_bytes() bytes, any contents) and table= (any contents) are taken instead of being
    allocated."""
    H, W = _pan_conf_check("pan_segment_scores", pan_2ch, conf)
    require_cuda(pan_2ch, conf, workspace)
    need = int(lib().upsnet_pan_segment_scores_workspace_bytes())
    if workspace is not None and (workspace.dtype != torch.uint8 or not workspace.is_contiguous() or workspace.numel() < need
                                  or workspace.data_ptr() % 4):
        raise ValueError("pan_segment_scores: workspace must be a contiguous, 4-byte aligned uint8 tensor of at least %d bytes" % need)
    nints = int(lib().upsnet_pan_segment_scores_table_ints())
    if table is not None and (table.dtype != torch.int32 or not table.is_contiguous() or table.numel() < nints):
        raise ValueError("pan_segment_scores: table must be a contiguous int32 tensor of at least %d words" % nints)
    require_cuda(table)
    dev = pan_2ch.device
    with torch.cuda.device(dev):
        if workspace is None:
            workspace = torch.zeros((need,), dtype=torch.uint8, device=dev)
        if table is None:
            table = torch.zeros((nints,), dtype=torch.int32, device=dev)
        pan_2ch, conf = aligned(pan_2ch), aligned(conf)
        check(lib().upsnet_pan_segment_scores(stream(), ptr(pan_2ch), ptr(conf), H, W, ptr(workspace), ptr(table)), "pan_segment_scores")
    return table


def pan_score_filter(pan_2ch, table, min_score, *, out=None):
    """Removes the doubtful segments of a 2-channel map (include/upsnet_hip.h: upsnet_pan_score_filter): every pixel of a non-VOID key
    whose row of `table` (pan_segment_scores of the same map) has sum_q < min_score * 255 * area, compared in double, becomes
    (255, 0, 0). 0 <= min_score <= 1; 0 removes nothing. Returns the filtered map; out= may be pan_2ch itself. One launch."""
    H, W = _pan_conf_check("pan_score_filter", pan_2ch)
    if not (0.0 <= float(min_score) <= 1.0):
        raise ValueError("pan_score_filter: min_score must lie in 0..1, got %r" % (min_score,))
    if table.dtype != torch.int32 or not table.is_contiguous() or table.numel() < int(lib().upsnet_pan_segment_scores_table_ints()):
        raise ValueError("pan_score_filter: table must be the int32 table of pan_segment_scores")
    if out is not None and (out.dtype != torch.uint8 or tuple(out.shape) != (H, W, 3) or not out.is_contiguous()):
        raise ValueError("pan_score_filter: out must be contiguous uint8 [%d,%d,3], got %s %s" % (H, W, tuple(out.shape), out.dtype))
    require_cuda(pan_2ch, table, out)
    with torch.cuda.device(pan_2ch.device):
        if out is None:
            out = pan_2ch.clone()
        pan_2ch, table = aligned(pan_2ch), aligned(table)
        check(lib().upsnet_pan_score_filter(stream(), ptr(pan_2ch), H, W, ptr(table), float(min_score), ptr(out)), "pan_score_filter")
    return out


def video_eval_workspace(max_gt, height, width, max_window, device):
    """Zeroed workspace of video_eval_frame / video_eval_end for sequences of height x width frames, at most max_gt (0..4096) rows in the
    sequence table and windows of at most max_window (1..8) frames; video_eval_end leaves all of it zero again."""
    nbytes = int(lib().upsnet_video_eval_workspace_bytes(int(max_gt), int(height), int(width), int(max_window)))
    if nbytes == 0:
        raise ValueError("video_eval_workspace: max_gt %d outside 0..4096, frame size %dx%d outside 1..2^24 pixels or max_window %d outside 1..8"
                         % (max_gt, height, width, max_window))
    return torch.zeros((nbytes,), dtype=torch.uint8, device=device)


def _video_eval_check_workspace(what, workspace, max_gt, H, W, max_window):
    need = int(lib().upsnet_video_eval_workspace_bytes(int(max_gt), H, W, int(max_window)))
    if need == 0 or workspace.dtype != torch.uint8 or not workspace.is_contiguous() or workspace.numel() < need:
        raise ValueError("%s: workspace too small for (or no workspace exists for) max_gt %d, a frame of %d x %d and max_window %d"
                         % (what, max_gt, H, W, max_window))
    written(workspace, torch.uint8, what + ": workspace")


def video_eval_frame(pred_2ch, gt_rgb, table, num_rows, num_crowd, max_gt, windows, frame, sequence, cat_known, workspace, tp, fp, fn,
                     iou, status):
    """One frame of a tracked sequence into the VPQ / STQ counts (include/upsnet_hip.h, csrc/video_eval.hip): pred_2ch / gt_rgb uint8
    [H,W,3]; table int32 [2 * num_rows + num_crowd] (per row in ascending id: id, category | iscrowd << 8; then the crowd rows);
    windows: ascending host ints in 1..8; tp / fp / fn int64 [len(windows), 256], iou float64 [len(windows), 256], status int64 [2].
    Three launches, no host synchronisation, no allocation."""
    require_cuda(pred_2ch, gt_rgb, table, cat_known, workspace, tp, fp, fn, iou, status)
    if pred_2ch.dtype != torch.uint8 or gt_rgb.dtype != torch.uint8 or pred_2ch.dim() != 3 or pred_2ch.shape[2] != 3 \
            or tuple(pred_2ch.shape) != tuple(gt_rgb.shape):
        raise ValueError("video_eval_frame: pred_2ch %s %s and gt_rgb %s %s must both be uint8 [H,W,3]"
                         % (tuple(pred_2ch.shape), pred_2ch.dtype, tuple(gt_rgb.shape), gt_rgb.dtype))
    windows = [int(n) for n in windows]
    nw = len(windows)
    if not 1 <= nw <= 8 or any(not 1 <= n <= 8 for n in windows) or any(b <= a for a, b in zip(windows, windows[1:])):
        raise ValueError("video_eval_frame: windows must be ascending, unique and in 1..8, got %s" % (windows,))
    num_rows, num_crowd = int(num_rows), int(num_crowd)
    if table.dtype != torch.int32 or not table.is_contiguous() or table.numel() != 2 * num_rows + num_crowd or not 0 <= num_crowd <= num_rows:
        raise ValueError("video_eval_frame: table must be contiguous int32 of 2 * %d + %d ints, got %s %s"
                         % (num_rows, num_crowd, tuple(table.shape), table.dtype))
    for t, dt, n in ((cat_known, torch.uint8, 256), (tp, torch.int64, nw * 256), (fp, torch.int64, nw * 256), (fn, torch.int64, nw * 256),
                     (iou, torch.float64, nw * 256), (status, torch.int64, 2)):
        if t.dtype != dt or t.numel() != n or not t.is_contiguous():
            raise ValueError("video_eval_frame: accumulator / table of %d %s expected, got %s %s" % (n, dt, tuple(t.shape), t.dtype))
        written(t, dt, "video_eval_frame: accumulator / table")
    pred_2ch, gt_rgb = dense(pred_2ch), dense(gt_rgb)
    H, W = int(pred_2ch.shape[0]), int(pred_2ch.shape[1])
    _video_eval_check_workspace("video_eval_frame", workspace, max_gt, H, W, windows[-1])
    check(lib().upsnet_video_eval_frame(stream(), ptr(pred_2ch), ptr(gt_rgb), H, W, ptr(table) if table.numel() else None, num_rows, num_crowd,
                                        int(max_gt), int_array(windows), nw, windows[-1], int(frame), int(sequence), ptr(cat_known),
                                        ptr(workspace), ptr(tp), ptr(fp), ptr(fn), ptr(iou), ptr(status)), "video_eval_frame")


def video_eval_end(height, width, max_gt, max_window, workspace, sequence_out, host_out=None):
    """The end of a sequence (csrc/video_eval.hip): the sequence-level cells into sequence_out (device int32,
    upsnet_video_eval_sequence_ints() ints: [0] their number, pairs (cell + 1, count) from [2] on), copied asynchronously into
    host_out (pinned int32 of the same size; None: no copy); the workspace is all zero afterwards. Two launches and the copy."""
    require_cuda(workspace, sequence_out)
    ints = int(lib().upsnet_video_eval_sequence_ints())
    if sequence_out.dtype != torch.int32 or sequence_out.numel() != ints or not sequence_out.is_contiguous():
        raise ValueError("video_eval_end: sequence_out must be contiguous int32 of %d ints, got %s %s" % (ints, tuple(sequence_out.shape), sequence_out.dtype))
    written(sequence_out, torch.int32, "video_eval_end: sequence_out")
    if host_out is not None and (host_out.is_cuda or not host_out.is_pinned() or host_out.dtype != torch.int32 or host_out.numel() != ints
                                 or not host_out.is_contiguous()):
        raise ValueError("video_eval_end: host_out must be contiguous pinned int32 host memory of %d ints" % ints)
    _video_eval_check_workspace("video_eval_end", workspace, max_gt, int(height), int(width), max_window)
    check(lib().upsnet_video_eval_end(stream(), int(height), int(width), int(max_gt), int(max_window), ptr(workspace), ptr(sequence_out),
                                      ptr(host_out)), "video_eval_end")


def mots_eval_workspace_bytes(max_gt, height, width):
    """Bytes of the workspace of mots_eval_frame / mots_eval_end for sequences of height x width frames and at most max_gt (0..4096)
    rows in the sequence table: a uint8 tensor of the caller's (dataset/mots.py), zeroed once; mots_eval_end leaves all of it zero again."""
    nbytes = int(lib().upsnet_mots_eval_workspace_bytes(int(max_gt), int(height), int(width)))
    if nbytes == 0:
        raise ValueError("mots_eval_workspace_bytes: max_gt %d outside 0..4096 or frame size %dx%d outside 1..2^24 pixels" % (max_gt, height, width))
    return nbytes


def _mots_eval_check(what, workspace, table, num_rows, max_gt, H, W):
    need = int(lib().upsnet_mots_eval_workspace_bytes(int(max_gt), H, W))
    if need == 0 or workspace.dtype != torch.uint8 or not workspace.is_contiguous() or workspace.numel() < need:
        raise ValueError("%s: workspace too small for (or no workspace exists for) max_gt %d and a frame of %d x %d" % (what, max_gt, H, W))
    written(workspace, torch.uint8, what + ": workspace")
    if table.dtype != torch.int32 or not table.is_contiguous() or table.numel() != 2 * num_rows or not 0 <= num_rows <= max_gt:
        raise ValueError("%s: table must be contiguous int32 of 2 * %d ints with at most max_gt %d rows, got %s %s"
                         % (what, num_rows, max_gt, tuple(table.shape), table.dtype))


def mots_eval_frame(pred_2ch, gt_rgb, table, num_rows, max_gt, frame, sequence, cat_info, workspace, counts, soft, status):
    """One frame of a tracked sequence into the MOTS counts (include/upsnet_hip.h, csrc/mots_eval.hip): pred_2ch / gt_rgb uint8 [H,W,3];
    table int32 [2 * num_rows] (per row in ascending id: id, category | iscrowd << 8 | isthing << 9); cat_info uint8 [256] (bit 0 known,
    bit 1 thing); counts int64 [7, 256] (tp, fp, fn, gt_masks, ids, frag, fp_ignored), soft float64 [256], status int64 [2].
    Three launches, no host synchronisation, no allocation."""
    require_cuda(pred_2ch, gt_rgb, table, cat_info, workspace, counts, soft, status)
    if pred_2ch.dtype != torch.uint8 or gt_rgb.dtype != torch.uint8 or pred_2ch.dim() != 3 or pred_2ch.shape[2] != 3 \
            or tuple(pred_2ch.shape) != tuple(gt_rgb.shape):
        raise ValueError("mots_eval_frame: pred_2ch %s %s and gt_rgb %s %s must both be uint8 [H,W,3]"
                         % (tuple(pred_2ch.shape), pred_2ch.dtype, tuple(gt_rgb.shape), gt_rgb.dtype))
    num_rows = int(num_rows)
    for t, dt, n in ((cat_info, torch.uint8, 256), (counts, torch.int64, 7 * 256), (soft, torch.float64, 256), (status, torch.int64, 2)):
        if t.dtype != dt or t.numel() != n or not t.is_contiguous():
            raise ValueError("mots_eval_frame: accumulator / table of %d %s expected, got %s %s" % (n, dt, tuple(t.shape), t.dtype))
        written(t, dt, "mots_eval_frame: accumulator / table")
    pred_2ch, gt_rgb = dense(pred_2ch), dense(gt_rgb)
    H, W = int(pred_2ch.shape[0]), int(pred_2ch.shape[1])
    _mots_eval_check("mots_eval_frame", workspace, table, num_rows, max_gt, H, W)
    check(lib().upsnet_mots_eval_frame(stream(), ptr(pred_2ch), ptr(gt_rgb), H, W, ptr(table) if table.numel() else None, num_rows, int(max_gt),
                                       int(frame), int(sequence), ptr(cat_info), ptr(workspace), ptr(counts), ptr(soft), ptr(status)),
          "mots_eval_frame")


def mots_eval_end(height, width, table, num_rows, max_gt, workspace, mtl):
    """The end of a sequence (csrc/mots_eval.hip): MT / PT / ML of its rows added into mtl (int64 [3, 256]); the workspace is all zero
    afterwards. One launch."""
    require_cuda(table, workspace, mtl)
    if mtl.dtype != torch.int64 or mtl.numel() != 3 * 256 or not mtl.is_contiguous():
        raise ValueError("mots_eval_end: mtl must be contiguous int64 of 768 words, got %s %s" % (tuple(mtl.shape), mtl.dtype))
    written(mtl, torch.int64, "mots_eval_end: mtl")
    num_rows = int(num_rows)
    _mots_eval_check("mots_eval_end", workspace, table, num_rows, max_gt, int(height), int(width))
    check(lib().upsnet_mots_eval_end(stream(), int(height), int(width), ptr(table) if table.numel() else None, num_rows, int(max_gt),
                                     ptr(workspace), ptr(mtl)), "mots_eval_end")


def pan_rle_transitions(pan_2ch, pairs, count):
    """COCO RLE of every thing segment (category != 255, instance >= 1) of one 2-channel map (csrc/mots_eval.hip): pairs (int64
    [cap], the caller's) takes the words key << 24 | p in arbitrary order, p the column-major positions at which the key's membership
    changes; count (int32 [1]) takes their number, even when it exceeds cap -- the caller then grows pairs and calls again
    (dataset/mots.py: segment_transitions). A memset and one launch, no host synchronisation, no allocation."""
    require_cuda(pan_2ch, pairs, count)
    if pan_2ch.dtype != torch.uint8 or pan_2ch.dim() != 3 or pan_2ch.shape[2] != 3 or not pan_2ch.is_contiguous():
        raise ValueError("pan_rle_transitions: pan_2ch must be contiguous uint8 [H,W,3], got %s %s" % (tuple(pan_2ch.shape), pan_2ch.dtype))
    H, W = int(pan_2ch.shape[0]), int(pan_2ch.shape[1])
    if not 0 < H * W <= (1 << 24):
        raise ValueError("pan_rle_transitions: a map of %d x %d pixels: H * W must lie in 1..2^24" % (H, W))
    if pairs.dtype != torch.int64 or pairs.dim() != 1 or not pairs.is_contiguous() or count.dtype != torch.int32 or count.numel() != 1:
        raise ValueError("pan_rle_transitions: pairs must be contiguous int64 [cap] and count int32 [1], got %s %s and %s %s"
                         % (tuple(pairs.shape), pairs.dtype, tuple(count.shape), count.dtype))
    cap = int(pairs.numel())
    pan_2ch = aligned(pan_2ch)
    check(lib().upsnet_pan_rle_transitions(stream(), ptr(pan_2ch), H, W, cap, ptr(pairs) if cap else None, ptr(count)), "pan_rle_transitions")
