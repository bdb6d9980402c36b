"""Cityscapes instance-level AP on the device: the region AP of the Cityscapes devkit's evalInstanceLevelSemanticLabeling with its
default arguments, which the reference's Cityscapes.evaluate_masks reports (upsnet/dataset/cityscapes.py:347-397). The devkit is not
part of the reference tree, so its rules are restated here; the per-image part runs in csrc/cs_inst_eval.hip.

Rules. GT of an image = its uint16 gtFine_instanceIds map: every distinct raw value v is a region with labelID = v // 1000 if
v >= 1000 else v, instID = v and pixelCount = its pixel count; regions whose labelID is one of CLASS_LABEL_IDS belong to that class,
instID < 1000 there is a group region. Void pixels are those whose RAW value is in VOID_VALUES (29003 is not void, 29 is). For a
prediction p of class c: pixelCount = mask area, voidIntersection, and the intersection with every region of c. Per (class c,
threshold t of OVERLAPS), over all images:
  * valid GT = regions of c with instID >= 1000 and pixelCount >= MIN_REGION_SIZE;
  * overlap(p, g) = intersection / (g.pixelCount + p.pixelCount - intersection) in float64, a match needs overlap > t;
  * a valid GT with matchers gives the entry (1, its largest matcher score) and (0, score) for every other matcher; one without
    adds a hard false negative;
  * a prediction that overlaps no region of c (valid or not) above t gives (0, score) unless (voidIntersection + intersections with
    group regions + intersections with regions below MIN_REGION_SIZE) / pixelCount > t (a small group region counts twice), in which
    case it is ignored; one whose only overlap above t is a group or a small region gives nothing;
  * AP: NaN without a valid GT of c in any image, 0.0 with GT and no prediction of c, else average_precision().
`summary` = nanmean over classes x thresholds (AP), over the t == 0.5 column (AP50), per class mean / the 0.5 entry.

`add_rle` / `add_masks` queue one image (counts and match on the device, one record per prediction: score, class, a code per
threshold; no host synchronisation after the upload). `accumulate` copies the records back once and runs the devkit's numpy curve in
float64. Entries enter the curve only through sorted scores, np.unique and integer sums, so the order of the images and of merged
evaluators does not change a bit of the result.

Deliberate deviations: a prediction of zero area is dropped (the devkit divides by zero); a class with valid GT and predictions of
which every one is ignored has AP 0.0 (the devkit indexes an empty array); the score is the float32 of the results widened to double
(the reference prints a float32 into pred.txt and the devkit parses it: order and ties are the same); no mask PNGs or pred.txt files
(dataset/cityscapes_inst_format.py writes and reads them).
Refused with ValueError before any launch: wrong dtypes or shapes, a mask or RLE whose size differs from the map's, RLE counts that
do not sum to H * W, a class outside 1..8, more than 65535 predictions in one image. Scores must not be NaN (device data in
add_masks, not inspected). Nothing has a capacity beyond that: the tables are indexed by (class, raw id) directly.
"""
import ctypes
import logging
import warnings

import numpy as np
import torch

from .._lib import aligned, check, lib, ptr, stream
from .coco_eval import rle_counts
from .rle import decode_rle_strings

logger = logging.getLogger(__name__)

CLASS_NAMES = ('person', 'rider', 'car', 'truck', 'bus', 'train', 'motorcycle', 'bicycle')
CLASS_LABEL_IDS = (24, 25, 26, 27, 28, 31, 32, 33)                     # Cityscapes label ids of the dataset's classes 1..8
VOID_VALUES = (0, 1, 2, 3, 4, 5, 6, 9, 10, 14, 15, 16, 18, 29, 30)       # labels with ignoreInEval
OVERLAPS = np.arange(0.5, 1.0, 0.05)                                     # as numpy yields them: 0.6000000000000001, ...
MIN_REGION_SIZE = 100
NUM_CLASSES = len(CLASS_NAMES)
SLOTS = 1001            # regions a class can hold: the group region + instances 0..999
ROW = SLOTS + 2         # per prediction: area, void intersection, intersection per slot
MAX_PREDS = 65535
_THR_STRIDE = 16        # state layout of csrc/cs_inst_eval.hip: hard FN [8][16] | images with valid GT [8] | predictions [8]


def average_precision(y_true, y_score, hard_false_negatives):
    """The devkit's precision / recall curve and its step-wise integral for one (class, threshold), float64 throughout."""
    score_arg_sort = np.argsort(y_score)
    y_score_sorted = y_score[score_arg_sort]
    y_true_sorted = y_true[score_arg_sort]
    y_true_sorted_cumsum = np.cumsum(y_true_sorted)
    _, unique_indices = np.unique(y_score_sorted, return_index=True)
    nb_prec_recall = len(unique_indices) + 1
    nb_examples = len(y_score_sorted)
    nb_true_examples = y_true_sorted_cumsum[-1] if nb_examples else 0.0      # (deviation: no entries -> AP 0.0)
    precision = np.zeros(nb_prec_recall)
    recall = np.zeros(nb_prec_recall)
    y_true_sorted_cumsum = np.append(y_true_sorted_cumsum, 0)
    for idx_res, idx_scores in enumerate(unique_indices):
        cum_sum = y_true_sorted_cumsum[idx_scores - 1]
        tp = nb_true_examples - cum_sum
        fp = nb_examples - idx_scores - tp
        fn = cum_sum + hard_false_negatives
        precision[idx_res] = float(tp) / (tp + fp)
        recall[idx_res] = float(tp) / (tp + fn)
    precision[-1] = 1.
    recall[-1] = 0.
    recall_for_conv = np.copy(recall)
    recall_for_conv = np.append(recall_for_conv[0], recall_for_conv)
    recall_for_conv = np.append(recall_for_conv, 0.)
    step_widths = np.convolve(recall_for_conv, [-0.5, 0, 0.5], 'valid')
    return np.dot(precision, step_widths)


def summarize(aps):
    """aps float64 [8, 10] -> the devkit's averages (computeAverages): NaN cells (classes without GT) are left out of the means."""
    d50 = np.flatnonzero(np.isclose(OVERLAPS, 0.5))
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)      # (a mean over NaNs only is NaN, as in the devkit, which warns)
        res = {'AP': np.nanmean(aps), 'AP50': np.nanmean(aps[:, d50]), 'per_class': {}, 'aps': aps}
        for c, name in enumerate(CLASS_NAMES):
            res['per_class'][name] = {'ap': np.average(aps[c, :]), 'ap50': np.average(aps[c, d50])}
    return res


def results_lines(res):
    """The devkit's table (printResults, no colours): one row per class, then the average row."""
    lines = ['#' * 50, '{:<15}'.format('what') + ':' + '{:>15}'.format('AP') + '{:>15}'.format('AP_50%'), '#' * 50]
    for name in CLASS_NAMES:
        r = res['per_class'][name]
        lines.append('{:<15}'.format(name) + ':' + '{:>15.3f}'.format(r['ap']) + '{:>15.3f}'.format(r['ap50']))
    lines.append('-' * 50)
    lines.append('{:<15}'.format('average') + ':' + '{:>15.3f}'.format(res['AP']) + '{:>15.3f}'.format(res['AP50']))
    return lines


def _gt_map(gt_ids):
    """The id map as (int16-viewed tensor, H, W): numpy uint16 [H, W] or a tensor of dtype uint16."""
    if isinstance(gt_ids, np.ndarray):
        if gt_ids.dtype != np.uint16 or gt_ids.ndim != 2:
            raise ValueError("gt_ids must be a uint16 [H, W] map, got %s %s" % (gt_ids.shape, gt_ids.dtype))
        t = torch.from_numpy(np.ascontiguousarray(gt_ids).view(np.int16))
    elif isinstance(gt_ids, torch.Tensor):
        if gt_ids.dtype != torch.uint16 or gt_ids.dim() != 2:
            raise ValueError("gt_ids must be a uint16 [H, W] map, got %s %s" % (tuple(gt_ids.shape), gt_ids.dtype))
        t = gt_ids.contiguous().view(torch.int16)
    else:
        raise ValueError("gt_ids must be a numpy array or a tensor, got %r" % type(gt_ids))
    H, W = int(t.shape[0]), int(t.shape[1])
    if H <= 0 or W <= 0 or H * W > (1 << 30):
        raise ValueError("gt_ids of %d x %d: H * W must be in 1..2^30" % (H, W))
    return t, H, W


def _transitions(rles, H, W):
    """im_post's RLE dicts of one class -> (transitions int32, lengths int64 [n]): the column-major change positions of every mask,
    the last (= H * W) dropped. ValueError on a size other than (H, W) or counts that do not sum to H * W."""
    n = len(rles)
    for r in rles:
        if not isinstance(r, dict) or 'counts' not in r or 'size' not in r:
            raise ValueError("a mask must be an RLE dict with 'size' and 'counts', got %r" % type(r))
        if tuple(int(v) for v in r['size']) != (H, W):
            raise ValueError("RLE of size %s on an instance-id map of %d x %d" % (list(r['size']), H, W))
    if all(isinstance(r['counts'], (str, bytes)) for r in rles):
        counts, off = decode_rle_strings([r['counts'] for r in rles])
    else:
        parts = [rle_counts(r)[0] for r in rles]
        counts = np.concatenate(parts) if parts else np.zeros(0, np.int64)
        off = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int64)
    lens = np.diff(off)
    if np.any(lens == 0) or np.any(counts < 0):
        raise ValueError("RLE counts must be non-negative and sum to %d x %d" % (H, W))
    cs = np.cumsum(counts)
    ends = cs[off[1:] - 1]
    sums = ends - np.concatenate([[0], ends[:-1]])
    if np.any(sums != H * W):
        k = int(np.flatnonzero(sums != H * W)[0])
        raise ValueError("RLE counts sum to %d, not %d x %d" % (int(sums[k]), H, W))
    pos = cs - np.repeat(np.concatenate([[0], ends[:-1]]), lens)
    keep = np.ones(cs.size, bool)
    keep[off[1:] - 1] = False
    assert n == lens.size
    return pos[keep].astype(np.int32), lens - 1


class InstanceEvaluator(object):
    """Running Cityscapes instance-level AP of a sequence of images on one device. add_rle() / add_masks() queue one image each;
    accumulate() synchronises once; `a += b` merges the evaluator of another chunk of the image list. walk: 'strided' (the column-major
    run lists are walked over the row-major id map itself: the default, the faster of the two) or 'transposed' (over a transposed copy
    of the map made once per image); the results are the same (DESIGN 4.10 has the timings)."""

    def __init__(self, device=None, walk='strided'):
        if walk not in ('transposed', 'strided'):
            raise ValueError("walk must be 'transposed' or 'strided', got %r" % (walk,))
        self.walk = walk
        self.device = torch.device(device) if device is not None else None
        self.num_images = 0
        self._n = 0             # records in use
        self._cap = 0
        self._score = self._cls = self._code = self._state = None
        self._thr = (ctypes.c_double * len(OVERLAPS))(*[float(t) for t in OVERLAPS])
        self._last = None
        self.aps = None

    def _dev(self):
        if self.device is None or (self.device.type == 'cuda' and self.device.index is None):
            self.device = torch.device('cuda', torch.cuda.current_device())
        return self.device

    def _reserve(self, n):
        """Room for n more records (the arrays double; a prefix copy on the device, nothing synchronised)."""
        dev = self._dev()
        if self._state is None:
            self._state = torch.zeros((lib().upsnet_cs_inst_state_words(),), dtype=torch.int64, device=dev)
        if self._n + n <= self._cap:
            return
        cap = max(1024, 2 * self._cap, self._n + n)
        score = torch.empty((cap,), dtype=torch.float32, device=dev)
        cls = torch.empty((cap,), dtype=torch.uint8, device=dev)
        code = torch.empty((cap, len(OVERLAPS)), dtype=torch.uint8, device=dev)
        if self._n:
            score[:self._n].copy_(self._score[:self._n])
            cls[:self._n].copy_(self._cls[:self._n])
            code[:self._n].copy_(self._code[:self._n])
        self._score, self._cls, self._code, self._cap = score, cls, code, cap

    # ---------------------------------------------------------------------------------------------------------- add
    def add_rle(self, gt_ids, dets_per_class, rles_per_class):
        """One image as it sits in results_list.pkl: dets_per_class[c] [n_c, 5] rows (x1 y1 x2 y2 score) and rles_per_class[c]
        im_post's RLE dicts for c = 1..8 (index 0, the background, is ignored; an empty list stands for no detections)."""
        gt, H, W = _gt_map(gt_ids)
        if len(dets_per_class) != len(rles_per_class):
            raise ValueError("%d classes of detections, %d of masks" % (len(dets_per_class), len(rles_per_class)))
        cls, scores, trans, lens = [], [], [], []
        for c in range(1, len(dets_per_class)):
            dets, rles = dets_per_class[c], rles_per_class[c]
            if isinstance(dets, (list, tuple)) and len(dets) == 0:
                dets = np.zeros((0, 5), np.float32)
            dets = np.asarray(dets)
            if dets.ndim != 2 or dets.shape[1] != 5 or dets.dtype.kind != 'f':
                raise ValueError("class %d: detections must be a float [n, 5] array, got %s %s" % (c, dets.shape, dets.dtype))
            if len(rles) != dets.shape[0]:
                raise ValueError("class %d: %d detections with %d masks" % (c, dets.shape[0], len(rles)))
            if dets.shape[0] == 0:
                continue
            if c > NUM_CLASSES:
                raise ValueError("detections of class %d: the instance classes are 1..%d" % (c, NUM_CLASSES))
            t, ln = _transitions(rles, H, W)
            cls.append(np.full((dets.shape[0],), c, np.int32))
            scores.append(dets[:, 4].astype(np.float32))
            trans.append(t)
            lens.append(ln)
        n = int(sum(a.size for a in cls))
        if n > MAX_PREDS:
            raise ValueError("%d predictions in one image: at most %d are supported" % (n, MAX_PREDS))
        cls = np.concatenate(cls) if cls else np.zeros(0, np.int32)
        scores = np.concatenate(scores) if scores else np.zeros(0, np.float32)
        trans = np.concatenate(trans) if trans else np.zeros(0, np.int32)
        off = np.concatenate([[0], np.cumsum(np.concatenate(lens))]) if lens else np.zeros(1, np.int64)
        if int(off[-1]) > 0x7FFFFFFF:
            raise ValueError("%d run boundaries in one image: at most 2^31 - 1" % int(off[-1]))
        off = off.astype(np.int32)
        dev = self._dev()
        # one pinned host buffer, one upload: classes | scores | offsets | transitions (all 4-byte items)
        parts = [cls.view(np.uint8), scores.view(np.uint8), off.view(np.uint8), trans.view(np.uint8)]
        host = torch.empty((sum((p.size + 15) // 16 * 16 for p in parts) + 16,), dtype=torch.uint8, pin_memory=torch.cuda.is_available())
        hn, o, views = host.numpy(), 0, []
        for p in parts:
            hn[o:o + p.size] = p
            views.append((o, p.size))
            o += (p.size + 15) // 16 * 16       # (every part starts on a 16-byte boundary of the upload)
        with torch.cuda.device(dev):
            d = host.to(dev, non_blocking=True)
            d_cls, d_score, d_off = (d[a:a + max(b, 4)].view(dt) for (a, b), dt in zip(views[:3], (torch.int32, torch.float32, torch.int32)))
            d_trans = d[views[3][0]:views[3][0] + max(views[3][1], 4)].view(torch.int32)     # never empty (a valid address)
            self._launch(gt.to(dev, non_blocking=True), H, W, n, d_cls, d_score, d_trans, d_off, None)

    def add_masks(self, gt_ids, masks, scores, classes):
        """One image with dense masks on the device: masks uint8 / bool [n, H, W] (non-zero = inside), scores float32 [n], classes
        integer [n] in 1..8 (scores and classes: host arrays or tensors; device classes are copied back to be checked)."""
        gt, H, W = _gt_map(gt_ids)
        if not isinstance(masks, torch.Tensor) or masks.dtype not in (torch.uint8, torch.bool) or masks.dim() != 3:
            raise ValueError("masks must be a uint8 / bool [n, H, W] tensor, got %r %s" % (type(masks), getattr(masks, 'dtype', None)))
        n = int(masks.shape[0])
        if tuple(masks.shape[1:]) != (H, W):
            raise ValueError("masks of %d x %d on an instance-id map of %d x %d" % (masks.shape[1], masks.shape[2], H, W))
        if n > MAX_PREDS:
            raise ValueError("%d predictions in one image: at most %d are supported" % (n, MAX_PREDS))
        scores = torch.as_tensor(scores)
        classes = torch.as_tensor(classes)
        if scores.dtype != torch.float32 or tuple(scores.shape) != (n,):
            raise ValueError("scores must be float32 [%d], got %s %s" % (n, tuple(scores.shape), scores.dtype))
        if classes.dtype not in (torch.int32, torch.int64, torch.uint8, torch.int16) or tuple(classes.shape) != (n,):
            raise ValueError("classes must be an integer [%d] array, got %s %s" % (n, tuple(classes.shape), classes.dtype))
        cls_np = classes.detach().cpu().numpy().astype(np.int64)
        if np.any((cls_np < 1) | (cls_np > NUM_CLASSES)):
            raise ValueError("class %d: the instance classes are 1..%d" % (int(cls_np[(cls_np < 1) | (cls_np > NUM_CLASSES)][0]), NUM_CLASSES))
        dev = self._dev()
        if not masks.is_cuda:
            raise ValueError("masks must be on the device (%s)" % dev)
        with torch.cuda.device(dev):
            m = masks.contiguous()
            m = m.view(torch.uint8) if m.dtype == torch.bool else m
            d_cls = torch.from_numpy(cls_np.astype(np.int32)).to(dev) if n else torch.zeros((1,), dtype=torch.int32, device=dev)
            d_score = scores.to(dev).contiguous() if n else torch.zeros((1,), dtype=torch.float32, device=dev)
            self._launch(gt.to(dev, non_blocking=True), H, W, n, d_cls, d_score, None, None, m)

    def _launch(self, gt, H, W, n, d_cls, d_score, d_trans, d_off, masks):
        dev = self._dev()
        self._reserve(n)
        l = lib()
        counts = torch.empty((l.upsnet_cs_inst_counts_ints(n),), dtype=torch.int32, device=dev)
        ws = torch.empty((l.upsnet_cs_inst_workspace_bytes(n),), dtype=torch.uint8, device=dev)
        transposed = masks is None and n > 0 and self.walk == 'transposed'
        gt_t = torch.empty((W, H), dtype=torch.int16, device=dev) if transposed else None
        b = self._n
        # the image's records land behind those of the images before it: a part that starts off 16 bytes is written into an aligned
        # buffer of its own and copied into place
        dst = [t[b:b + n] if n else t for t in (self._score, self._cls, self._code)]
        r_score, r_cls, r_code = land = [aligned(d) for d in dst]
        check(l.upsnet_cs_inst_image(stream(), ptr(gt), H, W, n, ptr(d_cls) if n else None, ptr(d_score) if n else None,
                                     ptr(d_trans) if n else None, ptr(d_off) if n else None, ptr(masks) if n else None,
                                     int(self.walk == 'strided'), ptr(gt_t), self._thr, len(OVERLAPS), ptr(counts), ptr(ws),
                                     ptr(r_score) if n else None, ptr(r_cls) if n else None,
                                     ptr(r_code) if n else None, ptr(self._state)), "cs_inst_image")
        for d, t in zip(dst, land):
            if t is not d:
                d.copy_(t)
        self._n += n
        self.num_images += 1
        self._last = (counts, n)

    def last_counts(self):
        """The integer counts of the image added last, on the device: {'area' [n], 'void' [n], 'inter' [n, 1001] (per slot of the
        prediction's class: 0 = the group region, 1 + k = raw value 1000 * label id + k), 'gt' [8, 1001] (pixel counts)}; the
        predictions in the order given (add_rle: classes ascending)."""
        counts, n = self._last
        rows = counts[:n * ROW].view(n, ROW)
        return {'area': rows[:, 0], 'void': rows[:, 1], 'inter': rows[:, 2:], 'gt': counts[n * ROW:].view(NUM_CLASSES, SLOTS)}

    # ---------------------------------------------------------------------------------------------------------- merge / summary
    def __iadd__(self, other):
        if not isinstance(other, InstanceEvaluator):
            raise ValueError("can only merge an InstanceEvaluator")
        if other._state is None:
            return self
        m = other._n
        self._reserve(m)
        dev = self._dev()
        if m:
            self._score[self._n:self._n + m].copy_(other._score[:m].to(dev))
            self._cls[self._n:self._n + m].copy_(other._cls[:m].to(dev))
            self._code[self._n:self._n + m].copy_(other._code[:m].to(dev))
        self._state += other._state.to(dev)
        self._n += m
        self.num_images += other.num_images
        return self

    def accumulate(self):
        """aps float64 [8, 10] (class, threshold): one device -> host copy of the records, then the devkit's curve per cell."""
        T = len(OVERLAPS)
        aps = np.full((NUM_CLASSES, T), np.nan)
        if self._state is not None:
            n = self._n
            state = self._state.cpu().numpy()
            score = self._score[:n].cpu().numpy().astype(np.float64) if n else np.zeros(0)
            cls = self._cls[:n].cpu().numpy() if n else np.zeros(0, np.uint8)
            code = self._code[:n].cpu().numpy() if n else np.zeros((0, T), np.uint8)
            for c in range(NUM_CLASSES):
                have_gt = state[NUM_CLASSES * _THR_STRIDE + c] > 0
                have_pred = state[NUM_CLASSES * _THR_STRIDE + NUM_CLASSES + c] > 0
                of_c = cls == c + 1
                for ti in range(T):
                    if have_gt and have_pred:
                        sel = of_c & (code[:, ti] != 0)
                        aps[c, ti] = average_precision((code[sel, ti] == 1).astype(np.float64), score[sel],
                                                       int(state[c * _THR_STRIDE + ti]))
                    elif have_gt:
                        aps[c, ti] = 0.0
        self.aps = aps
        return aps

    def summary(self):
        """{'AP', 'AP50', 'per_class': {name: {'ap', 'ap50'}}, 'aps': float64 [8, 10]}."""
        return summarize(self.accumulate())
