"""MaskROI (upsnet/operators/modules/mask_roi.py:23-146): detection selection on the device.

forward(rois, bbox_delta, cls_prob, im_info) -> (scores [n], boxes [n,5], cls_idx [n] int64).

MaskROI(..., soft_nms=(method, sigma, floor)) selects with soft-NMS instead (class-wise only): method 1 linear or
2 gaussian in cpu_soft_nms's numbering, floor the score below which a decayed candidate is dropped; the scores returned are decayed.
"""
import numpy as np
import torch
import torch.nn as nn

from ... import ops
from ...config.config import config


def check_count(n):
    """The device selection reports a candidate overflow (more (ROI, class) pairs above score_thresh than its fixed capacity of
    8192 in class-agnostic mode) as a negative count: the result would differ from the reference, so fail loudly."""
    if n < 0:
        raise RuntimeError("MaskROI: more than 8192 class-agnostic candidates above score_thresh; raise the threshold or lower the "
                           "number of proposals (the reference has no such limit, the device selection does)")
    return n


def check_count_soft(n):
    """The soft selection keeps a class's candidates in LDS: a class with more than 4096 above score_thresh is reported as a negative
    count (nothing is clamped silently)."""
    if n < 0:
        raise RuntimeError("MaskROI: soft-NMS holds at most 4096 candidates per class and a class has more above score_thresh; raise "
                           "the threshold or lower the number of proposals (the 4096-per-class limit is the device selection's)")
    return n


class MaskROI(nn.Module):

    def __init__(self, clip_boxes, bbox_class_agnostic, top_n, num_classes, nms_thresh=None, class_agnostic=False,
                 score_thresh=None, soft_nms=None):
        super(MaskROI, self).__init__()
        if soft_nms is not None and class_agnostic:
            raise ValueError("MaskROI: soft_nms goes with the class-wise selection only (class_agnostic=True keeps hard NMS: the "
                             "panoptic head wants a non-overlapping instance set)")
        self.soft_nms = None if soft_nms is None else tuple(soft_nms)
        self.clip_boxes = clip_boxes
        self.bbox_class_agnostic = bbox_class_agnostic
        self.top_n = top_n
        self.num_classes = num_classes
        self.nms_thresh = nms_thresh if nms_thresh is not None else config.test.nms_thresh
        self.class_agnostic = class_agnostic
        self.nms_classes = num_classes if not class_agnostic else 2
        self.score_thresh = score_thresh if score_thresh is not None else config.test.score_thresh

    def forward_padded(self, bottom_rois, bbox_delta, cls_prob, im_info, num_rois_dev=None, soft_nms=None):
        """Sync-free variant: fixed-capacity (boxes, scores, cls_idx, src_roi, num) device tensors. soft_nms: a (method, sigma, floor)
        tuple for this call (default: the constructor's)."""
        soft = self.soft_nms if soft_nms is None else tuple(soft_nms)
        if soft is not None and self.class_agnostic:
            raise ValueError("MaskROI: soft_nms goes with the class-wise selection only")
        dev = bottom_rois.device
        if isinstance(im_info, torch.Tensor):
            im = im_info.float().reshape(-1)[:3].to(dev)
        else:
            im = torch.from_numpy(np.asarray(im_info, dtype=np.float32).reshape(-1)[:3].copy()).to(dev, non_blocking=True)
        if soft is not None:
            return ops.mask_roi_soft(bottom_rois.detach(), bbox_delta.detach(), cls_prob.detach(), im, self.score_thresh, self.nms_thresh,
                                     config.test.max_det, config.network.bbox_reg_weights, soft[0], soft[1], soft[2], num_rois_dev,
                                     clip_boxes=bool(self.clip_boxes))
        return ops.mask_roi(bottom_rois.detach(), bbox_delta.detach(), cls_prob.detach(), im, self.class_agnostic,
                            self.score_thresh, self.nms_thresh, config.test.max_det, config.network.bbox_reg_weights,
                            num_rois_dev, clip_boxes=bool(self.clip_boxes))

    def forward(self, bottom_rois, bbox_delta, cls_prob, im_info, nms=True, cls_score=None, cls_label=None):
        if cls_score is not None or cls_label is not None:
            raise NotImplementedError("cls_score / cls_label are training-time inputs")
        boxes, scores, cls, src, num = self.forward_padded(bottom_rois, bbox_delta, cls_prob, im_info)
        n = (check_count if self.soft_nms is None else check_count_soft)(int(num.item()))
        return scores[:n], boxes[:n], cls[:n]
