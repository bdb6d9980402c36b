"""Mask boundaries on the device: `mask_to_boundary` of the Boundary IoU API (Cheng et al., Boundary IoU, CVPR 2021), the rule behind
COCOeval's iouType 'boundary' and LVIS' Boundary AP, restated in csrc/det_eval.hip (bnd_erode_kernel).

    d = int(round(dilation_ratio * sqrt(H ** 2 + W ** 2))), at least 1 (float64, Python's round: halves go to even)
    eroded = d rounds of a 3x3 erosion of the zero-padded mask = the AND over the (2d+1) x (2d+1) window, outside the image read as 0
    boundary = mask & ~eroded

so a mask cut by the image edge has boundary along that edge. `mask_to_boundary` here runs the kernel the evaluator
(DetectionEvaluator(..., 'boundary'), dataset/coco_eval.py) runs on its bit planes. Neither the Boundary IoU API nor cv2 is a
dependency: the rule is restated from their published sources.

Refused with ValueError before any launch: a dilation_ratio that is not a finite number > 0, wrong shapes or dtypes, RLE sizes that
differ, and a dilation whose window exceeds the kernel's tile (d > 3056 on an image larger than 2d+1 both ways)."""
import math

import numpy as np
import torch

from .._lib import check, dense, lib, ptr, stream


def check_dilation_ratio(dilation_ratio):
    r = float(dilation_ratio)
    if not math.isfinite(r) or r <= 0:
        raise ValueError("dilation_ratio must be a finite number > 0, got %r" % (dilation_ratio,))
    return r


def boundary_dilation(h, w, dilation_ratio=0.02):
    """The erosion depth d of an h x w image (host): int(round(ratio * image diagonal)), at least 1."""
    r = check_dilation_ratio(dilation_ratio)
    h, w = int(h), int(w)
    if h < 1 or w < 1:
        raise ValueError("image size %dx%d out of range" % (h, w))
    d = int(round(r * math.sqrt(h ** 2 + w ** 2)))
    return max(d, 1)


def checked_dilation(h, w, dilation_ratio):
    """boundary_dilation, refused when the kernel's window tile cannot hold it."""
    d = boundary_dilation(h, w, dilation_ratio)
    if d >= 1 << 30 or not lib().upsnet_boundary_dilation_fits(h, w, d):
        raise ValueError("dilation %d (ratio %g on %dx%d) exceeds what the boundary kernel's window holds" % (d, dilation_ratio, h, w))
    return d


def mask_to_boundary(masks, dilation_ratio=0.02, size=None, device=None):
    """masks: a uint8 / bool [n,H,W] device tensor (non-zero = set), or a list of RLE dicts ({'size': [H, W], 'counts': ...}) of one
    size (`size`, when given, must be it; required for an empty list). Returns the boundaries as a uint8 [n,H,W] device tensor of
    0 / 1. Nothing is synchronised."""
    from .coco_eval import counts_to_transitions, rle_counts
    check_dilation_ratio(dilation_ratio)
    trans = off = None
    if isinstance(masks, (list, tuple)):
        ts, o = [], [0]
        for s in masks:
            counts, hw = rle_counts(s)
            if size is None:
                size = hw
            if hw != tuple(int(v) for v in size):
                raise ValueError("RLE mask size %s differs from %s" % (hw, tuple(size)))
            t = counts_to_transitions(counts)
            ts.append(t)
            o.append(o[-1] + len(t))
        if size is None:
            raise ValueError("an empty RLE list needs size = (H, W)")
        H, W = (int(v) for v in size)
        n = len(masks)
        dev = torch.device(device) if device is not None else torch.device('cuda', torch.cuda.current_device())
        trans = torch.from_numpy(np.concatenate(ts + [np.zeros(1, np.int64)]).astype(np.int32)).to(dev)   # (one spare entry: never empty)
        off = torch.from_numpy(np.asarray(o, np.int64)).to(dev)
        src = None
    else:
        if not isinstance(masks, torch.Tensor) or masks.dim() != 3 or masks.dtype not in (torch.uint8, torch.bool):
            raise ValueError("masks must be a uint8 / bool [n,H,W] tensor or a list of RLE dicts, got %r"
                             % ((tuple(masks.shape), masks.dtype) if isinstance(masks, torch.Tensor) else type(masks),))
        if not masks.is_cuda:
            raise ValueError("masks must be a device tensor (there is no CPU path)")
        n, H, W = masks.shape
        if size is not None and tuple(int(v) for v in size) != (H, W):
            raise ValueError("size %s differs from the masks' %s" % (tuple(size), (H, W)))
        dev = masks.device
        src = dense(masks)
        src = src.view(torch.uint8) if src.dtype == torch.bool else src
    if H < 1 or W < 1 or H * W >= 1 << 31:
        raise ValueError("image size %dx%d out of range" % (H, W))
    if n > 65535:
        raise ValueError("%d masks in one call (at most 65535)" % n)
    d = checked_dilation(H, W, dilation_ratio)
    out = torch.empty((n, H, W), dtype=torch.uint8, device=dev)
    if n == 0:
        return out
    area = torch.empty(n, dtype=torch.int32, device=dev)
    ws = torch.empty(max(int(lib().upsnet_boundary_masks_workspace_bytes(n, H, W)), 1), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        check(lib().upsnet_boundary_masks(stream(), d, H, W, n, ptr(src), ptr(trans), ptr(off), ptr(ws), ptr(out), ptr(area)),
              "boundary_masks")
    return out


def panoptic_boundary(pred_2ch=None, gt_rgb=None, ratio=0.02):
    """The boundary bits of panoptic label maps (csrc/pq_boundary.hip; the bits Boundary PQ counts, dataset/pq.py): pred_2ch and / or
    gt_rgb uint8 [H,W,3] device tensors of one shape -> uint8 [H,W], bit 0 = GT boundary, bit 1 = pred boundary (0 for a map not given).
    d = boundary_dilation(H, W, ratio); a pixel is boundary unless the (2d+1) x (2d+1) window centred on it lies inside the image and
    holds the pixel's own label (GT: R + 256 G + 65536 B; pred: cat * 256 + inst, every cat == 255 pixel one VOID label), so that
    boundary & (label == s) is mask_to_boundary(label == s) for every segment s. Any d >= 1 is accepted. ValueError before any launch:
    a bad ratio, no map, wrong shapes or dtypes, host tensors. A non-contiguous view is copied."""
    from .. import ops
    check_dilation_ratio(ratio)
    maps = [m for m in (pred_2ch, gt_rgb) if m is not None]
    if not maps:
        raise ValueError("panoptic_boundary: neither pred_2ch nor gt_rgb given")
    for m in maps:
        if not isinstance(m, torch.Tensor) or m.dtype != torch.uint8 or m.dim() != 3 or m.shape[2] != 3:
            raise ValueError("panoptic_boundary: maps must be uint8 [H,W,3] tensors, got %r"
                             % ((tuple(m.shape), m.dtype) if isinstance(m, torch.Tensor) else type(m),))
        if not m.is_cuda:
            raise ValueError("panoptic_boundary: maps must be device tensors (there is no CPU path)")
        if tuple(m.shape) != tuple(maps[0].shape):
            raise ValueError("panoptic_boundary: pred_2ch %s and gt_rgb %s differ in shape" % (tuple(maps[0].shape), tuple(m.shape)))
    H, W = maps[0].shape[:2]
    d = boundary_dilation(H, W, ratio)
    dev = maps[0].device
    ws = torch.empty((ops.pan_boundary_workspace_bytes(H, W),), dtype=torch.uint8, device=dev)
    out = torch.empty((H, W), dtype=torch.uint8, device=dev)
    return ops.pan_boundary_map(d, pred_2ch, gt_rgb, ws, out)
