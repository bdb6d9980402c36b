"""RPN proposal recall on the device: Detectron's average recall (AR) as the reference's BaseDataset.evaluate_box_proposals computes
it (upsnet/dataset/base_dataset.py:723-805), the greedy matching restated in csrc/prop_eval.hip.

The host does every selection with the reference's numpy expressions: GT = rows with gt_classes > 0 and is_crowd == 0, the area
filter (inclusive on both ends, in the given area dtype), proposals = rows with gt_classes == 0 in order, cut to `limit`, cast to
float32. `add` queues one image: all (area, limit) problems of the evaluator in one launch, no host synchronisation. `summary`
copies the recorded IoUs back once and does the sort, the `>= t` counts in float64, `/ float(num_pos)` and `recalls.mean()` as the
reference does; every field equals the reference's bit for bit.

Rules of the reference kept on purpose: an image with no proposals adds to num_pos and appends nothing (its `continue` comes
before the limit cut); limit = 0 therefore appends zeros; num_pos == 0 gives NaN recalls. Refused with ValueError before any
launch: non-finite boxes, an unknown area, a negative limit, inconsistent lengths, more than 4096 GT boxes of one area in an image.
"""
import numpy as np
import torch

from .. import ops

AREAS = {'all': 0, 'small': 1, 'medium': 2, 'large': 3, '96-128': 4, '128-256': 5, '256-512': 6, '512-inf': 7}
AREA_RANGES = [
    [0 ** 2, 1e5 ** 2],  # all
    [0 ** 2, 32 ** 2],  # small
    [32 ** 2, 96 ** 2],  # medium
    [96 ** 2, 1e5 ** 2],  # large
    [96 ** 2, 128 ** 2],  # 96-128
    [128 ** 2, 256 ** 2],  # 128-256
    [256 ** 2, 512 ** 2],  # 256-512
    [512 ** 2, 1e5 ** 2]]  # 512-inf
AR_LIMITS = (100, 300, 1000)
AR_AREAS = (('all', ''), ('small', 's'), ('medium', 'm'), ('large', 'l'))


def default_thresholds():
    step = 0.05
    return np.arange(0.5, 0.95 + 1e-5, step)


def recall_summary(gt_overlaps, num_pos, thresholds=None):
    """The tail of evaluate_box_proposals: gt_overlaps (the float64 recorded IoUs of all images) -> the reference's dict."""
    gt_overlaps = np.sort(gt_overlaps)
    if thresholds is None:
        thresholds = default_thresholds()
    recalls = np.zeros_like(thresholds)
    with np.errstate(divide='ignore', invalid='ignore'):   # num_pos == 0: NaN, as the reference (which warns)
        for i, t in enumerate(thresholds):
            recalls[i] = (gt_overlaps >= t).sum() / float(num_pos)
    ar = recalls.mean()
    return {'ar': ar, 'recalls': recalls, 'thresholds': thresholds, 'gt_overlaps': gt_overlaps, 'num_pos': num_pos}


def gt_entry(anns, size, cls_of, min_area=-1):
    """One image's GT in roidb form from its instances-JSON annotations, by the rules of the reference's
    JsonDataset._add_gt_annotations (json_dataset.py:164-230; xywh_to_xyxy / clip_xyxy_to_image of bbox_transform.py): size =
    (height, width); cls_of = {category_id: 1-based class}; an unknown category_id raises ValueError."""
    height, width = size
    boxes, classes, areas, crowd = [], [], [], []
    for obj in anns:
        if obj['area'] < min_area:
            continue
        if 'ignore' in obj and obj['ignore'] == 1:
            continue
        if int(obj['category_id']) not in cls_of:
            raise ValueError("annotation %s: category_id %s is not among the JSON's categories" % (obj.get('id'), obj['category_id']))
        xywh = obj['bbox']
        x1, y1 = xywh[0], xywh[1]
        x2 = x1 + np.maximum(0., xywh[2] - 1.)
        y2 = y1 + np.maximum(0., xywh[3] - 1.)
        x1 = np.minimum(width - 1., np.maximum(0., x1))
        y1 = np.minimum(height - 1., np.maximum(0., y1))
        x2 = np.minimum(width - 1., np.maximum(0., x2))
        y2 = np.minimum(height - 1., np.maximum(0., y2))
        if obj['area'] > 0 and x2 > x1 and y2 > y1:
            boxes.append([x1, y1, x2, y2])
            classes.append(cls_of[int(obj['category_id'])])
            areas.append(obj['area'])
            crowd.append(obj['iscrowd'])
    n = len(boxes)
    entry = {'boxes': np.zeros((n, 4), np.float32), 'gt_classes': np.zeros((n,), np.int32), 'seg_areas': np.zeros((n,), np.float32),
             'is_crowd': np.zeros((n,), bool)}
    for ix in range(n):
        entry['boxes'][ix, :] = boxes[ix]
        entry['gt_classes'][ix] = classes[ix]
        entry['seg_areas'][ix] = areas[ix]
        entry['is_crowd'][ix] = crowd[ix]
    return entry


def _boxes(a, name):
    a = np.asarray(a)
    if a.ndim != 2 or a.shape[1] != 4:
        if a.size == 0:
            return np.zeros((0, 4), a.dtype if a.dtype.kind == 'f' else np.float32)
        raise ValueError("%s must be [n, 4], got %s" % (name, a.shape))
    return a


def _vector(a, n, name):
    a = np.asarray(a)
    if a.ndim != 1 or a.shape[0] != n:
        raise ValueError("%s must have one entry per box (%d), got shape %s" % (name, n, a.shape))
    return a


class ProposalRecallEvaluator(object):
    """Running proposal recall of a sequence of images on one device, for every (area, limit) pair of `areas` x `limits` at once.

    areas: names of the reference's 8 area ranges ('all', 'small', 'medium', 'large', '96-128', '128-256', '256-512', '512-inf');
    limits: proposal limits (None = all proposals, else an int >= 0). add() / add_entry() queue one image each (no synchronisation);
    summary() synchronises once. `a += b` merges the evaluator of another rank or chunk (same areas and limits); the recorded IoUs are
    sorted before they are counted, so the order of the images does not change the summary."""

    def __init__(self, areas=('all',), limits=(None,), device=None):
        areas, limits = list(areas), list(limits)
        for a in areas:
            if a not in AREAS:
                raise ValueError('Unknown area range: {}'.format(a))
        for lim in limits:
            if lim is not None and (int(lim) != lim or int(lim) < 0):
                raise ValueError("limit must be None or an int >= 0, got %r" % (lim,))
        if not areas or not limits or len(set(areas)) != len(areas) or len(set(limits)) != len(limits):
            raise ValueError("areas and limits must be non-empty and distinct, got %s x %s" % (areas, limits))
        self.areas = areas
        self.limits = [None if lim is None else int(lim) for lim in limits]
        self.keys = [(a, lim) for a in self.areas for lim in self.limits]
        self.device = torch.device(device) if device is not None else None
        self.num_pos = {k: 0 for k in self.keys}
        self.num_images = 0
        self._bufs = []                          # per-image device outputs (float32)
        self._parts = {k: [] for k in self.keys}  # (buffer index, offset, length) of each appended _gt_overlaps

    def _dev(self):
        if self.device is None or (self.device.type == 'cuda' and self.device.index is None):
            self.device = torch.device('cuda', torch.cuda.current_device())
        return self.device

    # ---------------------------------------------------------------------------------------------------------- add
    def add_entry(self, entry):
        """One roidb entry as the reference reads it: 'boxes' [n, 4] (GT rows and proposal rows, gt_classes == 0 marks a proposal),
        'gt_classes' [n], 'is_crowd' [n], 'seg_areas' [n]."""
        boxes = _boxes(entry['boxes'], "entry['boxes']")
        n = boxes.shape[0]
        gt_classes = _vector(entry['gt_classes'], n, "entry['gt_classes']")
        is_crowd = _vector(entry['is_crowd'], n, "entry['is_crowd']")
        seg_areas = _vector(entry['seg_areas'], n, "entry['seg_areas']")
        gt_inds = np.where((gt_classes > 0) & (is_crowd == 0))[0]
        non_gt_inds = np.where(gt_classes == 0)[0]
        self._add(boxes[non_gt_inds, :], boxes[gt_inds, :], seg_areas[gt_inds])

    def add(self, proposals, gt_boxes, gt_classes, is_crowd, gt_areas):
        """One image: proposals [N, 4] x1 y1 x2 y2 in rank order; gt_boxes [G, 4] with gt_classes [G] (> 0 for objects), is_crowd [G]
        and gt_areas [G] (the segment areas the area ranges test). Host arrays (numpy or CPU tensors)."""
        def host(a):
            return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a
        proposals = _boxes(host(proposals), 'proposals')
        gt_boxes = _boxes(host(gt_boxes), 'gt_boxes')
        G = gt_boxes.shape[0]
        gt_classes = _vector(host(gt_classes), G, 'gt_classes')
        is_crowd = _vector(host(is_crowd), G, 'is_crowd')
        gt_areas = _vector(host(gt_areas), G, 'gt_areas')
        gt_inds = np.where((gt_classes > 0) & (is_crowd == 0))[0]
        self._add(proposals, gt_boxes[gt_inds, :], gt_areas[gt_inds])

    def _add(self, boxes, gt_boxes, gt_areas):
        boxes = boxes.astype(dtype=np.float32, copy=False)
        gts, gt_off = [], [0]
        for a in self.areas:
            area_range = AREA_RANGES[AREAS[a]]
            valid_gt_inds = np.where((gt_areas >= area_range[0]) & (gt_areas <= area_range[1]))[0]
            g = gt_boxes[valid_gt_inds, :].astype(dtype=np.float32, copy=False)
            if g.shape[0] > ops.PROPOSAL_RECALL_MAX_GT:
                raise ValueError("%d GT boxes in area %r of one image: at most %d are supported" % (g.shape[0], a, ops.PROPOSAL_RECALL_MAX_GT))
            gts.append(g)
            gt_off.append(gt_off[-1] + g.shape[0])
        if not np.all(np.isfinite(boxes)) or not all(np.all(np.isfinite(g)) for g in gts):
            raise ValueError("proposal and GT boxes must be finite")
        P = boxes.shape[0]
        rows, out_len, words = [], 0, 0
        keys = []
        for ai, a in enumerate(self.areas):
            G = gts[ai].shape[0]
            for lim in self.limits:
                self.num_pos[(a, lim)] += G
                if P == 0:
                    continue
                p = P if (lim is None or P <= lim) else lim
                rows.append((0, p, gt_off[ai], G, out_len, words))
                keys.append(((a, lim), out_len, G))
                out_len += G
                words += (p + 31) // 32
        self.num_images += 1
        if not rows:
            return
        dev = self._dev()
        table = np.asarray(rows, np.int64).reshape(-1, 6)
        gt_all = np.concatenate(gts) if gt_off[-1] else np.zeros((0, 4), np.float32)
        total = int(table[:, 1].sum())
        # one pinned host buffer, one upload: table | proposals | GT boxes (16-byte aligned sections)
        nb_t, nb_p, nb_g = table.nbytes, boxes.size * 4, gt_all.size * 4
        host = torch.empty((nb_t + nb_p + nb_g + 16,), dtype=torch.uint8, pin_memory=torch.cuda.is_available())
        hn = host.numpy()
        hn[:nb_t] = table.view(np.uint8).reshape(-1)
        hn[nb_t:nb_t + nb_p] = np.ascontiguousarray(boxes).view(np.uint8).reshape(-1)
        hn[nb_t + nb_p:nb_t + nb_p + nb_g] = np.ascontiguousarray(gt_all).view(np.uint8).reshape(-1)
        with torch.cuda.device(dev):
            d = host.to(dev, non_blocking=True)
            d_table = d[:nb_t].view(torch.int64).view(-1, 6)
            d_props = d[nb_t:nb_t + nb_p].view(torch.float32).view(-1, 4)
            d_gts = d[nb_t + nb_p:nb_t + nb_p + max(nb_g, 16)].view(torch.float32).view(-1, 4)   # never empty (a valid address)
            ws = torch.empty((max(ops.proposal_recall_workspace_bytes(len(rows), total), 1),), dtype=torch.uint8, device=dev)
            out = torch.empty((max(out_len, 1),), dtype=torch.float32, device=dev)
            ops.proposal_recall(d_table, d_props, d_gts, max(g.shape[0] for g in gts), total, ws, out)
        b = len(self._bufs)
        self._bufs.append(out[:out_len])
        for k, off, G in keys:
            self._parts[k].append((b, off, G))

    # ---------------------------------------------------------------------------------------------------------- merge / summary
    def __iadd__(self, other):
        if not isinstance(other, ProposalRecallEvaluator) or other.keys != self.keys:
            raise ValueError("can only merge a ProposalRecallEvaluator of the same areas and limits")
        base = len(self._bufs)
        dev = self._dev() if other._bufs else None
        self._bufs.extend(t.to(dev) for t in other._bufs)
        for k in self.keys:
            self.num_pos[k] += other.num_pos[k]
            self._parts[k].extend((base + b, off, n) for b, off, n in other._parts[k])
        self.num_images += other.num_images
        return self

    def gt_overlaps(self):
        """{(area, limit): float64 recorded IoUs, images in the order added} (one device -> host copy)."""
        if self._bufs:
            lens = [t.numel() for t in self._bufs]
            flat = torch.cat(self._bufs).cpu().numpy()
            starts = np.concatenate([[0], np.cumsum(lens)])
        res = {}
        for k in self.keys:
            parts = [flat[starts[b] + off:starts[b] + off + n] for b, off, n in self._parts[k]]
            gt_overlaps = np.zeros(0)
            if parts:
                gt_overlaps = np.hstack([gt_overlaps] + [p.astype(np.float64) for p in parts])
            res[k] = gt_overlaps
        return res

    def summary(self, thresholds=None):
        """{(area, limit): {'ar', 'recalls', 'thresholds', 'gt_overlaps' (sorted float64), 'num_pos'}}, the reference's dict."""
        ov = self.gt_overlaps()
        return {k: recall_summary(ov[k], self.num_pos[k], thresholds) for k in self.keys}


def ar_metrics(summary, limits=AR_LIMITS):
    """Detectron's proposal metric names: AR@100, ARs@100, ARm@100, ARl@100, ... ARl@1000 (a summary of areas all/small/medium/large
    x limits)."""
    out = {}
    for lim in limits:
        for area, suffix in AR_AREAS:
            out['AR%s@%d' % (suffix, lim)] = summary[(area, lim)]['ar']
    return out
