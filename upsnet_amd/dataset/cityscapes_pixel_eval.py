"""Cityscapes pixel-level semantic labelling on the device: IoU and instance-weighted iIoU per class and per category, the metric of
the Cityscapes devkit's evalPixelLevelSemanticLabeling. The devkit is not part of the reference tree, so its rules are restated
here; the per-image part runs in csrc/cs_pixel_eval.hip.

Rules. Ground truth of an image = its gtFine_labelIds map (label ids 0..33) and, for iIoU, its gtFine_instanceIds map; a prediction
is a map of label ids. conf[g][p] counts every pixel. With E = the labels that are not ignore-in-eval (EVAL_LABEL_IDS):
  * class IoU of label l: NaN if l is ignored; tp = conf[l][l], fn = sum(conf[l, :]) - tp, fp = sum(conf[g][l] for g in E, g != l)
    -- ground truth of an ignored label makes no false positive, a prediction of an ignored label is a false negative;
    tp + fp + fn == 0 -> NaN, else float(tp) / (tp + fp + fn);
  * category IoU: L = the labels of the category in E (none -> NaN); tp = sum(conf[L][:, L]), fn = sum(conf[L, :]) - tp,
    fp = sum(conf[G][:, L]) over the G in E of other categories;
  * instances of an image: the distinct raw values v > 1000 of the id map, ascending; label v // 1000, skipped unless it is one of
    CLASS_LABEL_IDS (caravan and trailer are ignore-in-eval). size = pixels of v, tp = those with pred == label, category tp = those
    whose pred is a label of the label's category in E. weight = avg_class_size[class] / float(size); the class and the category
    get tpWeighted += float(tp) * weight and fnWeighted += float(size - tp) * weight (float64, in this order, image after image);
  * class / category iIoU: the same formulas with the weighted tp and fn, and the unweighted fp; NaN for labels without instances
    and for the categories other than human and vehicle;
  * the four averages are means over the non-NaN scores: 'IoU_class' (the devkit's averageScoreClasses), 'iIoU_class'
    (averageScoreInstClasses), 'IoU_category' (averageScoreCategories), 'iIoU_category' (averageScoreInstCategories).

`add` queues one image (no host synchronisation); `accumulate` copies the sums back once and forms the scores in Python floats.
Integer sums do not depend on the order of the images; the weighted sums are float64 sums in the order of the calls, so the same
images in the same order give the same bits, and another order or a merge (`a += b`) agrees to rounding.

Deliberate deviations: an image added without its instance-id map counts towards IoU only, and then every iIoU of the evaluator is
NaN (the devkit needs both files). Refused with ValueError before any launch: wrong dtypes or shapes, maps of different sizes,
H * W > 2^30, an average class size that is not positive. After the run (`accumulate`): a prediction pixel whose value is not a label
(train id 19..254 or 255 of a network output, a label id above 33), or a ground-truth label above 33, raises ValueError naming the
first such image -- the devkit aborts on an unknown label; nothing is dropped silently."""
import ctypes
import logging
import math

import numpy as np
import torch

from .._lib import aligned, check, lib, ptr, stream
from .cityscapes_eval import CLASS_LABEL_IDS, CLASS_NAMES, VOID_VALUES

logger = logging.getLogger(__name__)

NUM_LABELS = 34
# id -> (name, category); ignoreInEval = id in VOID_VALUES, hasInstances = id >= 24
LABELS = (('unlabeled', 'void'), ('ego vehicle', 'void'), ('rectification border', 'void'), ('out of roi', 'void'), ('static', 'void'),
          ('dynamic', 'void'), ('ground', 'void'), ('road', 'flat'), ('sidewalk', 'flat'), ('parking', 'flat'), ('rail track', 'flat'),
          ('building', 'construction'), ('wall', 'construction'), ('fence', 'construction'), ('guard rail', 'construction'),
          ('bridge', 'construction'), ('tunnel', 'construction'), ('pole', 'object'), ('polegroup', 'object'),
          ('traffic light', 'object'), ('traffic sign', 'object'), ('vegetation', 'nature'), ('terrain', 'nature'), ('sky', 'sky'),
          ('person', 'human'), ('rider', 'human'), ('car', 'vehicle'), ('truck', 'vehicle'), ('bus', 'vehicle'), ('caravan', 'vehicle'),
          ('trailer', 'vehicle'), ('train', 'vehicle'), ('motorcycle', 'vehicle'), ('bicycle', 'vehicle'))
CATEGORIES = ('flat', 'construction', 'object', 'nature', 'sky', 'human', 'vehicle')     # (void has no evaluated label)
EVAL_LABEL_IDS = tuple(i for i in range(NUM_LABELS) if i not in VOID_VALUES)
TRAIN_TO_LABEL_ID = (7, 8, 11, 12, 13, 17, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 31, 32, 33)   # the reference's train2regular
NOT_A_LABEL = 255
# the colours of train ids 0..18 (the Cityscapes label colours of TRAIN_TO_LABEL_ID), entries 0..18 of the reference's get_pallete
TRAIN_ID_COLOURS = ((128, 64, 128), (244, 35, 232), (70, 70, 70), (102, 102, 156), (190, 153, 153), (153, 153, 153), (250, 170, 30),
                    (220, 220, 0), (107, 142, 35), (152, 251, 152), (70, 130, 180), (220, 20, 60), (255, 0, 0), (0, 0, 142), (0, 0, 70),
                    (0, 60, 100), (0, 80, 100), (0, 0, 230), (119, 11, 32))
# Average instance sizes of the devkit's evalPixelLevelSemanticLabeling (args.avgClassSize), in the order of CLASS_NAMES. UNVERIFIED:
# recalled from the devkit's published source, which is not available to this project's tests; a wrong digit is a one-line fix here,
# and PixelEvaluator(avg_class_size=...) overrides them.
AVG_CLASS_SIZE = (3462.4756337644, 3930.4788056518, 12794.0202738185, 27855.1264367816, 35732.1511111111, 67583.7075812274,
                  6298.7200839748, 4672.3249222261)
INST_K = 1000           # instance numbers of a class: the per-image table is int32 [8][1000][3]
WSUM_ROWS = ('person', 'rider', 'car', 'truck', 'bus', 'train', 'motorcycle', 'bicycle', 'human', 'vehicle')
_BAD_BLOCK = 1024       # images per block of the per-image error counters

assert EVAL_LABEL_IDS == TRAIN_TO_LABEL_ID and LABELS[24][0] == CLASS_NAMES[0]


def lookup_table(train_ids):
    """uint8 [256]: prediction value -> label id, NOT_A_LABEL for a value that is none (train ids: 0..18; label ids: 0..33)."""
    lut = np.full(256, NOT_A_LABEL, np.uint8)
    if train_ids:
        lut[:len(TRAIN_TO_LABEL_ID)] = TRAIN_TO_LABEL_ID
    else:
        lut[:NUM_LABELS] = np.arange(NUM_LABELS)
    return lut


def _map(a, what, np_dtype, torch_dtype, view=None):
    """A [H, W] map as a contiguous tensor (host or device) of torch_dtype (uint16: viewed as int16)."""
    if isinstance(a, np.ndarray):
        if a.dtype != np_dtype or a.ndim != 2:
            raise ValueError("%s must be a %s [H, W] map, got %s %s" % (what, np.dtype(np_dtype).name, a.shape, a.dtype))
        a = np.ascontiguousarray(a)
        return torch.from_numpy(a.view(view) if view is not None else a)
    if isinstance(a, torch.Tensor):
        if a.dtype != torch_dtype or a.dim() != 2:
            raise ValueError("%s must be a %s [H, W] map, got %s %s" % (what, np.dtype(np_dtype).name, tuple(a.shape), a.dtype))
        a = a.contiguous()
        return a.view(torch.int16) if view is not None else a
    raise ValueError("%s must be a numpy array or a tensor, got %r" % (what, type(a)))


def _iou(tp, fp, fn):
    denom = tp + fp + fn
    if denom == 0:
        return float('nan')
    return float(tp) / denom


def _mean(scores):
    """The devkit's getScoreAverage: the mean of the entries that are not NaN, summed in the order given; NaN if there is none."""
    n, s = 0, 0.0
    for v in scores:
        if not math.isnan(v):
            n += 1
            s += v
    return s / n if n else float('nan')


def scores(conf, wsum, with_instances=True):
    """conf int64 [34, 34] and wsum float64 [10, 4] (None or with_instances False: no iIoU) -> the result dict of `summary`."""
    conf = np.asarray(conf)
    E = list(EVAL_LABEL_IDS)
    per_class, per_category = {}, {}
    for l in E:
        tp = int(conf[l, l])
        fn = int(conf[l, :].sum()) - tp
        fp = int(conf[[g for g in E if g != l], l].sum())
        iiou = float('nan')
        if with_instances and wsum is not None and l in CLASS_LABEL_IDS:
            row = CLASS_LABEL_IDS.index(l)
            iiou = _iou(float(wsum[row, 1]), fp, float(wsum[row, 3]))
        per_class[LABELS[l][0]] = {'iou': _iou(tp, fp, fn), 'iiou': iiou}
    for cat in CATEGORIES:
        L = [l for l in E if LABELS[l][1] == cat]
        G = [g for g in E if LABELS[g][1] != cat]
        tp = int(conf[L][:, L].sum())
        fn = int(conf[L, :].sum()) - tp
        fp = int(conf[G][:, L].sum())
        iiou = float('nan')
        if with_instances and wsum is not None and cat in WSUM_ROWS:
            row = WSUM_ROWS.index(cat)
            iiou = _iou(float(wsum[row, 1]), fp, float(wsum[row, 3]))
        per_category[cat] = {'iou': _iou(tp, fp, fn), 'iiou': iiou}
    return {'IoU_class': _mean(per_class[LABELS[l][0]]['iou'] for l in E),
            'iIoU_class': _mean(per_class[LABELS[l][0]]['iiou'] for l in E),
            'IoU_category': _mean(per_category[c]['iou'] for c in CATEGORIES),
            'iIoU_category': _mean(per_category[c]['iiou'] for c in CATEGORIES),
            'per_class': per_class, 'per_category': per_category, 'conf': conf.copy(),
            'wsum': None if wsum is None else np.array(wsum, np.float64)}


def results_lines(res):
    """The devkit's tables (printClassScores / printCategoryScores, no colours): classes, their averages, categories, theirs."""
    def row(name, r):
        return '{:<14}'.format(name) + ': ' + '{:>5.3f}'.format(r['iou']) + '    ' + '{:>5.3f}'.format(r['iiou'])
    lines = ['classes          IoU      nIoU', '-' * 32]
    lines += [row(LABELS[l][0], res['per_class'][LABELS[l][0]]) for l in EVAL_LABEL_IDS]
    lines += ['-' * 32, row('Score Average', {'iou': res['IoU_class'], 'iiou': res['iIoU_class']}), '-' * 32, '',
              'categories       IoU      nIoU', '-' * 32]
    lines += [row(c, res['per_category'][c]) for c in CATEGORIES]
    lines += ['-' * 32, row('Score Average', {'iou': res['IoU_category'], 'iiou': res['iIoU_category']}), '-' * 32]
    return lines


class PixelEvaluator(object):
    """Running Cityscapes pixel-level IoU / iIoU of a sequence of images on one device. add() queues one image; accumulate()
    synchronises once; `a += b` merges the evaluator of another chunk of the image list."""

    def __init__(self, device=None, avg_class_size=None):
        avg = AVG_CLASS_SIZE if avg_class_size is None else avg_class_size
        if isinstance(avg, dict):
            avg = [avg[n] for n in CLASS_NAMES]
        avg = [float(v) for v in avg]
        if len(avg) != len(CLASS_NAMES) or not all(0.0 < v < 1e300 for v in avg):
            raise ValueError("avg_class_size must be %d positive sizes (%s), got %r" % (len(CLASS_NAMES), ', '.join(CLASS_NAMES), avg))
        self.avg_class_size = tuple(avg)
        self._avg = (ctypes.c_double * len(avg))(*avg)
        self.device = torch.device(device) if device is not None else None
        self.num_images = 0
        self.images_without_ids = 0
        self.names = []
        self._conf = self._wsum = None
        self._bad = []          # blocks of int32 [_BAD_BLOCK][4], one row per image: two counters, padded so every row starts on 16 bytes
        self._luts = {}
        self._last = None

    def _dev(self):
        if self.device is None or (self.device.type == 'cuda' and self.device.index is None):
            self.device = torch.device('cuda', torch.cuda.current_device())
        return self.device

    def _state(self):
        dev = self._dev()
        if self._conf is None:
            self._conf = torch.zeros((NUM_LABELS, NUM_LABELS), dtype=torch.int64, device=dev)
            self._wsum = torch.zeros((len(WSUM_ROWS), 4), dtype=torch.float64, device=dev)
        if self.num_images == len(self._bad) * _BAD_BLOCK:
            self._bad.append(torch.zeros((_BAD_BLOCK, 4), dtype=torch.int32, device=dev))
        return self._bad[-1][self.num_images % _BAD_BLOCK][:2]

    def add(self, gt_labels, gt_ids, pred, train_ids=True, name=None):
        """One image: gt_labels uint8 [H, W] (label ids), gt_ids uint16 [H, W] (the instance-id map) or None (IoU only), pred uint8
        [H, W]: train ids 0..18 (the network's output; train_ids=True) or label ids 0..33. Host arrays or tensors."""
        gl = _map(gt_labels, 'gt_labels', np.uint8, torch.uint8)
        pr = _map(pred, 'pred', np.uint8, torch.uint8)
        gi = None if gt_ids is None else _map(gt_ids, 'gt_ids', np.uint16, torch.uint16, np.int16)
        H, W = int(gl.shape[0]), int(gl.shape[1])
        for what, m in (('pred', pr), ('gt_ids', gi)):
            if m is not None and tuple(m.shape) != (H, W):
                raise ValueError("%s of %d x %d on a label map of %d x %d" % (what, m.shape[0], m.shape[1], H, W))
        if H <= 0 or W <= 0 or H * W > (1 << 30):
            raise ValueError("maps of %d x %d: H * W must be in 1..2^30" % (H, W))
        self._launch(gl, gi, pr, H, W, bool(train_ids), name)

    def _launch(self, gl, gi, pr, H, W, train_ids, name):
        dev = self._dev()
        with torch.cuda.device(dev):
            bad = self._state()
            if train_ids not in self._luts:
                self._luts[train_ids] = torch.from_numpy(lookup_table(train_ids)).to(dev)
            gl, pr = gl.to(dev, non_blocking=True), pr.to(dev, non_blocking=True)
            gi = None if gi is None else gi.to(dev, non_blocking=True)
            gl, pr, gi = aligned(gl), aligned(pr), aligned(gi)
            inst = None if gi is None else torch.empty((lib().upsnet_cs_pixel_inst_ints(),), dtype=torch.int32, device=dev)
            check(lib().upsnet_cs_pixel_image(stream(), ptr(gl), ptr(gi), ptr(pr), ptr(self._luts[train_ids]), H, W, self._avg,
                                              ptr(self._conf), ptr(inst), ptr(self._wsum), ptr(bad)), "cs_pixel_image")
        self.names.append(name if name is not None else 'image %d' % self.num_images)
        self.num_images += 1
        self.images_without_ids += int(gi is None)
        self._last = inst

    def last_counts(self):
        """The instance table of the image added last, on the device: int32 [8, 1000, 3] = (class, instance number k of the raw
        value 1000 * label id + k) -> size | pixels with pred == label | pixels with pred in the label's category; None for an
        image added without its instance-id map."""
        return None if self._last is None else self._last.view(len(CLASS_NAMES), INST_K, 3)

    def __iadd__(self, other):
        if not isinstance(other, PixelEvaluator):
            raise ValueError("can only merge a PixelEvaluator")
        if other.avg_class_size != self.avg_class_size:
            raise ValueError("cannot merge evaluators of different average class sizes")
        if other._conf is None:
            return self
        dev = self._dev()
        if self._conf is None:
            self._state()
            self._bad = []
        self._conf += other._conf.to(dev)
        self._wsum += other._wsum.to(dev)
        # (the error counters stay one row per image: this evaluator's rows, then the other's)
        mine = torch.cat(self._bad)[:self.num_images] if self._bad else torch.zeros((0, 4), dtype=torch.int32, device=dev)
        rows = torch.cat([mine, torch.cat(other._bad)[:other.num_images].to(dev)])
        pad = (-rows.shape[0]) % _BAD_BLOCK
        rows = torch.cat([rows, torch.zeros((pad, 4), dtype=torch.int32, device=dev)])
        self._bad = list(rows.split(_BAD_BLOCK))
        self.names += other.names
        self.num_images += other.num_images
        self.images_without_ids += other.images_without_ids
        return self

    def state(self):
        """(conf int64 [34, 34], wsum float64 [10, 4]) on the host, after the error check of accumulate()."""
        if self._conf is None:
            return np.zeros((NUM_LABELS, NUM_LABELS), np.int64), np.zeros((len(WSUM_ROWS), 4), np.float64)
        bad = torch.cat(self._bad)[:self.num_images].cpu().numpy()
        hit = np.flatnonzero(bad.any(axis=1))
        if hit.size:
            k = int(hit[0])
            raise ValueError("%s: %d prediction pixels are not a label id (after the look-up), %d ground-truth pixels have a label "
                             "above %d; %d images in all" % (self.names[k], bad[k, 0], bad[k, 1], NUM_LABELS - 1, hit.size))
        return self._conf.cpu().numpy(), self._wsum.cpu().numpy()

    def accumulate(self):
        conf, wsum = self.state()
        return scores(conf, wsum, with_instances=self.images_without_ids == 0)

    def summary(self):
        """{'IoU_class', 'iIoU_class', 'IoU_category', 'iIoU_category', 'per_class': {name: {'iou', 'iiou'}}, 'per_category': {name:
        {'iou', 'iiou'}}, 'conf' int64 [34, 34], 'wsum' float64 [10, 4]}."""
        return self.accumulate()
