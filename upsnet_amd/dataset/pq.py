"""Panoptic quality on the device: the scoring of BaseDataset.evaluate_panoptic (upsnet/dataset/base_dataset.py:209-330), whose core
_pq_compute_single_core (:514-610) runs here as csrc/pq_eval.hip, one image per `add`, into running per-category accumulators.

Semantics are the reference's, summed in the order of a single-worker reference run (images in the order added; within an image and
category, matches in ascending GT id), so that wherever the JSON areas equal the pixel counts the accumulated IoU sums are
bit-identical to it. Deliberate deviations:
  * invalid input raises ValueError on the host before any launch (duplicate GT ids, a GT id 0, category ids outside 0..254, more
    segments than max_gt_segments, shape mismatch); a pred category that is not in `categories` raises KeyError at the first
    synchronisation (pq_stat / summary), naming the image and the category. The reference's own error path raises NameError
    (`gt_ann` is undefined there);
  * the prediction must already be at GT resolution: resizing for im_scale != 1 stays with the caller;
  * scoring produces no pred PNG / JSON (the reference's IdGenerator colours only relabel the pred segments and PQ does not depend on
    them); dataset/pan_format.write_panoptic writes them, and add_png scores such files -- or any COCO-panoptic prediction -- again.
"""
import logging

import numpy as np
import torch

from .. import ops

logger = logging.getLogger(__name__)

MAX_CATEGORY = 254   # 255 is the VOID label of the 2-channel prediction


def segments_array(segments_info, max_gt_segments):
    """segments_info (the GT JSON's list of dicts) -> int64 [n,4] (id, category_id, iscrowd, area), validated; raises ValueError."""
    n = len(segments_info)
    if n > max_gt_segments:
        raise ValueError("%d GT segments, more than max_gt_segments=%d" % (n, max_gt_segments))
    segs = np.array([(el['id'], el['category_id'], el.get('iscrowd', 0), el['area']) for el in segments_info], np.int64).reshape(n, 4)
    ids, cats = segs[:, 0], segs[:, 1]
    if np.any(ids == 0):
        raise ValueError("GT segment with id 0 (the VOID id of the panoptic PNG)")
    if np.any((ids < 0) | (ids >= 1 << 31)):
        raise ValueError("GT segment ids must lie in 1..2^31-1")
    uniq, counts = np.unique(ids, return_counts=True)
    if np.any(counts > 1):
        raise ValueError("duplicate GT segment ids %s" % uniq[counts > 1].tolist())
    if np.any((cats < 0) | (cats > MAX_CATEGORY)):
        raise ValueError("GT category ids must lie in 0..%d, got %s" % (MAX_CATEGORY, sorted(set(cats[(cats < 0) | (cats > MAX_CATEGORY)].tolist()))))
    return segs


def _check_image(name, t, shape=None, other='pred_2ch'):
    if t.dtype not in (np.uint8, torch.uint8) or len(t.shape) != 3 or t.shape[2] != 3:
        raise ValueError("%s must be uint8 [H,W,3], got %s %s" % (name, tuple(t.shape), t.dtype))
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError("%s %s and %s %s differ in shape (resize the prediction to GT resolution first)"
                         % (name, tuple(t.shape), other, tuple(shape)))


class PanopticEvaluator(object):
    """Running PQ statistics of a sequence of images on one device.

    categories: the dataset's category table, {id: {'isthing': 0/1, ...}} or the JSON's list of dicts with 'id'.
    add() queues one image on the current stream (no synchronisation, no allocation after the first call); pq_stat() / summary()
    synchronise once. `a += b` merges the evaluator of another rank (PQStat.__iadd__ semantics: a's sums plus b's).

    boundary=True scores Boundary PQ (Cheng et al., Boundary IoU, CVPR 2021; csrc/pq_boundary.hip): every pair's IoU is
    min(mask IoU, boundary IoU), the boundary bits those of dataset.boundary.panoptic_boundary at d = boundary_dilation(H, W,
    dilation_ratio) per image, iou_b = inter_b / (area_bp + area_bg - inter_b - void_b) over pixel counts (0 when that union is empty).
    FP absorption, FN, summation order and the result dicts are unchanged. The workspace then also holds two byte maps of the image: it
    is allocated for the first image and again only when a larger image arrives. ValueError before any launch: a dilation_ratio that
    is not a finite number > 0; `a += b` across different ratios or across a boundary and a plain evaluator."""

    def __init__(self, categories, device=None, max_gt_segments=4096, boundary=False, dilation_ratio=0.02):
        if not isinstance(categories, dict):
            categories = {el['id']: el for el in categories}
        bad = [c for c in categories if not 0 <= int(c) <= MAX_CATEGORY]
        if bad:
            raise ValueError("category ids must lie in 0..%d, got %s" % (MAX_CATEGORY, bad))
        if not 0 <= int(max_gt_segments) <= 4096:
            raise ValueError("max_gt_segments %d outside 0..4096" % max_gt_segments)
        self.categories = categories
        self.device = torch.device(device) if device is not None else None
        self.max_gt_segments = int(max_gt_segments)
        self.boundary = bool(boundary)
        self.dilation_ratio = None
        if self.boundary:
            from .boundary import check_dilation_ratio
            self.dilation_ratio = check_dilation_ratio(dilation_ratio)
        self._ws_pixels = 0  # boundary: the image size (pixels) the workspace holds
        self.num_images = 0
        self._state = None   # device tensors, allocated at the first add

    def _dev_state(self):
        if self._state is None:
            dev = self.device if self.device is not None else torch.device('cuda', torch.cuda.current_device())
            self.device = dev
            known = np.zeros(256, np.uint8)
            known[[int(c) for c in self.categories]] = 1
            self._state = dict(known=torch.from_numpy(known).to(dev),
                               ws=None if self.boundary else ops.pq_workspace(self.max_gt_segments, dev),
                               tp=torch.zeros(256, dtype=torch.int64, device=dev), fp=torch.zeros(256, dtype=torch.int64, device=dev),
                               fn=torch.zeros(256, dtype=torch.int64, device=dev), iou=torch.zeros(256, dtype=torch.float64, device=dev),
                               status=torch.zeros(1, dtype=torch.int64, device=dev),
                               png_status=torch.zeros(2, dtype=torch.int64, device=dev))
        return self._state

    def _accumulate(self, pred_2ch, gt_rgb, segs):
        st = self._state
        segs = torch.from_numpy(segs)
        if torch.cuda.is_available():
            segs = segs.pin_memory()
        segs = segs.to(self.device, non_blocking=True)
        if not self.boundary:
            ops.pq_accumulate(pred_2ch, gt_rgb, segs, st['known'], self.num_images, self.max_gt_segments, st['ws'], st['tp'], st['fp'],
                              st['fn'], st['iou'], st['status'])
        else:
            from .boundary import boundary_dilation
            H, W = pred_2ch.shape[:2]
            if H * W > self._ws_pixels:   # (the old workspace's count areas are zero by contract: nothing to carry over)
                st['ws'] = ops.pq_boundary_workspace(self.max_gt_segments, H, W, self.device)
                self._ws_pixels = H * W
            ops.pq_boundary_accumulate(boundary_dilation(H, W, self.dilation_ratio), pred_2ch, gt_rgb, segs, st['known'], self.num_images,
                                       self.max_gt_segments, st['ws'], st['tp'], st['fp'], st['fn'], st['iou'], st['status'])
        self.num_images += 1

    def _upload(self, t):
        if isinstance(t, np.ndarray):
            return torch.from_numpy(np.ascontiguousarray(t)).to(self.device, non_blocking=True)
        return t

    def add(self, pred_2ch, gt_rgb, segments_info):
        """pred_2ch: uint8 [H,W,3] (ops.unified_pan_result's output); gt_rgb: uint8 [H,W,3] GT panoptic PNG (id = R + 256 G + 65536 B);
        segments_info: the image's GT segments (dicts with id, category_id, iscrowd, area). Device tensors or numpy arrays (uploaded)."""
        _check_image('pred_2ch', pred_2ch)
        _check_image('gt_rgb', gt_rgb, pred_2ch.shape)
        segs = segments_array(segments_info, self.max_gt_segments)
        self._dev_state()
        pred_2ch, gt_rgb = self._upload(pred_2ch), self._upload(gt_rgb)
        self._accumulate(pred_2ch, gt_rgb, segs)

    def add_png(self, pred_rgb, pred_segments_info, gt_rgb, gt_segments_info):
        """One image of a prediction in COCO panoptic format: pred_rgb uint8 [H,W,3] PNG of arbitrary ids (id = R + 256 G + 65536 B,
        0 = VOID) with the JSON's pred_segments_info (id, category_id; its area is ignored, the reference overwrites it with the pixel
        count). The PNG is relabelled to a 2-channel map on the device (csrc/pan_format.hip; instance slots per category in ascending
        pred id, the order in which the reference adds several matches of one GT segment), then scored exactly like add().
        ValueError before any launch: an id 0, outside 1..2^24-1 or used twice, a category outside 0..254, more than 256 segments of
        one category, a shape mismatch. KeyError at the first synchronisation, naming the image index and the id: a segment that is
        in the PNG and not in the JSON, or in the JSON without a pixel in the PNG (the reference's sanity checks, :531-542)."""
        from .pan_format import relabel, segments_table
        _check_image('pred_rgb', pred_rgb)
        _check_image('gt_rgb', gt_rgb, pred_rgb.shape, 'pred_rgb')
        table = segments_table(pred_segments_info)
        segs = segments_array(gt_segments_info, self.max_gt_segments)
        st = self._dev_state()
        pred_rgb, gt_rgb = self._upload(pred_rgb), self._upload(gt_rgb)
        pred_2ch, _ = relabel(pred_rgb, table, self.num_images, st['png_status'])
        self._accumulate(pred_2ch, gt_rgb, segs)

    def __iadd__(self, other):
        if (self.boundary, self.dilation_ratio) != (other.boundary, other.dilation_ratio):
            raise ValueError("cannot merge evaluators of different rules: boundary=%s dilation_ratio=%s and boundary=%s dilation_ratio=%s"
                             % (self.boundary, self.dilation_ratio, other.boundary, other.dilation_ratio))
        if other._state is None:
            self.num_images += other.num_images
            return self
        st, ot = self._dev_state(), {k: v.to(self.device) for k, v in other._state.items() if k != 'ws'}
        for k in ('tp', 'fp', 'fn', 'iou'):
            st[k] += ot[k]
        # the first error stays first: other's image indices follow this evaluator's
        shifted = torch.where(ot['status'] != 0, ot['status'] + (self.num_images << 8), ot['status'])
        st['status'].copy_(torch.where(st['status'] != 0, st['status'], shifted))
        # (add_png's words hold 2^62 - ((index + 1) << 24 | id): the earliest image is the maximum)
        shifted = torch.where(ot['png_status'] != 0, ot['png_status'] - (self.num_images << 24), ot['png_status'])
        st['png_status'].copy_(torch.maximum(st['png_status'], shifted))
        self.num_images += other.num_images
        return self

    def pq_stat(self):
        """Synchronise once; return a host PQStat of everything added. KeyError if a pred category was not in `categories`, or if an
        image added with add_png failed one of the PNG / JSON sanity checks (the earliest image's error)."""
        from .base_dataset import PQStat
        stat = PQStat()
        if self._state is None:
            return stat
        st = self._state
        host = torch.cat([st['tp'], st['fp'], st['fn'], st['iou'].view(torch.int64), st['status'], st['png_status']]).cpu().numpy()
        tp, fp, fn = host[0:256], host[256:512], host[512:768]
        iou, status = host[768:1024].view(np.float64), int(host[1024])
        errors = []   # (image index, the reference's order of checks, message)
        for k, text in ((0, 'presented in PNG and not presented in JSON'), (1, 'presented in JSON and not presented in PNG')):
            if int(host[1025 + k]):
                v = (1 << 62) - int(host[1025 + k])
                errors.append(((v >> 24) - 1, 2 * k, 'In the image with index {} (in the order added) segment with ID {} is {}.'.format(
                    (v >> 24) - 1, v & 0xffffff, text)))
        if status:
            errors.append(((status >> 8) - 1, 1, 'In the image with index {} (in the order added) a segment has unknown category_id {}.'.format(
                (status >> 8) - 1, status & 255)))
        if errors:
            raise KeyError(min(errors)[2])
        for c in np.nonzero(tp + fp + fn)[0]:
            cat = stat[int(c)]
            cat.tp, cat.fp, cat.fn, cat.iou = int(tp[c]), int(fp[c]), int(fn[c]), float(iou[c])
        return stat

    def summary(self):
        """The reference's result dict {'All', 'Things', 'Stuff': {'pq', 'sq', 'rq', 'n'}, 'per_class': {...}}; logs its two tables."""
        return pq_summary(self.pq_stat(), self.categories)


def pq_summary(pq_stat, categories):
    """pq_compute's tail (base_dataset.py:291-313): PQStat.pq_average for All / Things / Stuff, and the two logged tables."""
    metrics = [("All", None), ("Things", True), ("Stuff", False)]
    results = {}
    for name, isthing in metrics:
        results[name], per_class = pq_stat.pq_average(categories, isthing=isthing)
        if name == 'All':
            results['per_class'] = per_class
    logger.info("{:10s}| {:>5s}  {:>5s}  {:>5s} {:>5s}".format("", "PQ", "SQ", "RQ", "N"))
    logger.info("-" * (10 + 7 * 4))
    for name, _ in metrics:
        r = results[name]
        logger.info("{:10s}| {:5.1f}  {:5.1f}  {:5.1f} {:5d}".format(name, 100 * r['pq'], 100 * r['sq'], 100 * r['rq'], r['n']))
    logger.info("{:4s}| {:>5s} {:>5s} {:>5s} {:>6s} {:>7s} {:>7s} {:>7s}".format("IDX", "PQ", "SQ", "RQ", "IoU", "TP", "FP", "FN"))
    for idx, r in results['per_class'].items():
        if 'tp' not in r:
            continue   # a category with no tp / fp / fn has no counts to print
        logger.info("{:4d} | {:5.1f} {:5.1f} {:5.1f} {:6.1f} {:7d} {:7d} {:7d}".format(idx, 100 * r['pq'], 100 * r['sq'], 100 * r['rq'], r['iou'],
                                                                                 r['tp'], r['fp'], r['fn']))
    return results
