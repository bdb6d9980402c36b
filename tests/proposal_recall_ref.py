"""Test-side numpy restatement of the reference's BaseDataset.evaluate_box_proposals (upsnet/dataset/base_dataset.py:723-805) with
bbox_overlaps_c of upsnet/bbox/bbox.pyx restated in float32 numpy, in the same operation order (numpy float32 arithmetic is IEEE
single, no contraction, correctly rounded division). tests/golden/proposal_recall.npz pins it to the reference's own code."""
import numpy as np

AREAS = {'all': 0, 'small': 1, 'medium': 2, 'large': 3, '96-128': 4, '128-256': 5, '256-512': 6, '512-inf': 7}
AREA_RANGES = [[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2], [96 ** 2, 128 ** 2],
               [128 ** 2, 256 ** 2], [256 ** 2, 512 ** 2], [512 ** 2, 1e5 ** 2]]


def bbox_overlaps(boxes, query_boxes):
    """bbox_overlaps_c: float32 [N, K]."""
    b = np.asarray(boxes, np.float32)
    q = np.asarray(query_boxes, np.float32)
    one = np.float32(1)
    box_area = (q[:, 2] - q[:, 0] + one) * (q[:, 3] - q[:, 1] + one)
    iw = np.minimum(b[:, None, 2], q[None, :, 2]) - np.maximum(b[:, None, 0], q[None, :, 0]) + one
    ih = np.minimum(b[:, None, 3], q[None, :, 3]) - np.maximum(b[:, None, 1], q[None, :, 1]) + one
    barea = (b[:, 2] - b[:, 0] + one) * (b[:, 3] - b[:, 1] + one)
    with np.errstate(all='ignore'):
        ua = barea[:, None] + box_area[None, :] - iw * ih
        ov = iw * ih / ua
    return np.where((iw > 0) & (ih > 0), ov, np.float32(0)).astype(np.float32)


def greedy(boxes, gt_boxes):
    """The per-image loop of evaluate_box_proposals: float64 [G] recorded IoUs."""
    overlaps = bbox_overlaps(boxes.astype(dtype=np.float32, copy=False), gt_boxes.astype(dtype=np.float32, copy=False))
    _gt_overlaps = np.zeros((gt_boxes.shape[0]))
    for j in range(min(boxes.shape[0], gt_boxes.shape[0])):
        argmax_overlaps = overlaps.argmax(axis=0)
        max_overlaps = overlaps.max(axis=0)
        gt_ind = max_overlaps.argmax()
        gt_ovr = max_overlaps.max()
        assert gt_ovr >= 0
        box_ind = argmax_overlaps[gt_ind]
        _gt_overlaps[j] = overlaps[box_ind, gt_ind]
        assert _gt_overlaps[j] == gt_ovr
        overlaps[box_ind, :] = -1
        overlaps[:, gt_ind] = -1
    return _gt_overlaps


def greedy_fast(boxes, gt_boxes):
    """greedy() for large P x G: the same matrix with -1 in deleted rows and columns and the same argmax choices, but the column
    maxima are kept and only the columns whose argmax row was just deleted are rescanned (tested against greedy())."""
    overlaps = bbox_overlaps(boxes.astype(dtype=np.float32, copy=False), gt_boxes.astype(dtype=np.float32, copy=False))
    G = gt_boxes.shape[0]
    _gt_overlaps = np.zeros((G))
    if min(boxes.shape[0], G) == 0:
        return _gt_overlaps
    argmax_overlaps = overlaps.argmax(axis=0)
    max_overlaps = overlaps.max(axis=0)
    for j in range(min(boxes.shape[0], G)):
        gt_ind = max_overlaps.argmax()
        box_ind = argmax_overlaps[gt_ind]
        _gt_overlaps[j] = overlaps[box_ind, gt_ind]
        overlaps[box_ind, :] = -1
        overlaps[:, gt_ind] = -1
        max_overlaps[gt_ind] = -1
        redo = np.where((argmax_overlaps == box_ind) & (max_overlaps >= 0))[0]
        if len(redo):
            sub = overlaps[:, redo]
            argmax_overlaps[redo] = sub.argmax(axis=0)
            max_overlaps[redo] = sub.max(axis=0)
    return _gt_overlaps


def evaluate_box_proposals(roidb, thresholds=None, area='all', limit=None, fast=False):
    assert area in AREAS, 'Unknown area range: {}'.format(area)
    area_range = AREA_RANGES[AREAS[area]]
    gt_overlaps = np.zeros(0)
    num_pos = 0
    for entry in roidb:
        gt_inds = np.where((entry['gt_classes'] > 0) & (entry['is_crowd'] == 0))[0]
        gt_boxes = entry['boxes'][gt_inds, :]
        gt_areas = entry['seg_areas'][gt_inds]
        valid_gt_inds = np.where((gt_areas >= area_range[0]) & (gt_areas <= area_range[1]))[0]
        gt_boxes = gt_boxes[valid_gt_inds, :]
        num_pos += len(valid_gt_inds)
        non_gt_inds = np.where(entry['gt_classes'] == 0)[0]
        boxes = entry['boxes'][non_gt_inds, :]
        if boxes.shape[0] == 0:
            continue
        if limit is not None and boxes.shape[0] > limit:
            boxes = boxes[:limit, :]
        gt_overlaps = np.hstack((gt_overlaps, (greedy_fast if fast else greedy)(boxes, gt_boxes)))
    gt_overlaps = np.sort(gt_overlaps)
    if thresholds is None:
        step = 0.05
        thresholds = np.arange(0.5, 0.95 + 1e-5, step)
    recalls = np.zeros_like(thresholds)
    with np.errstate(divide='ignore', invalid='ignore'):
        for i, t in enumerate(thresholds):
            recalls[i] = (gt_overlaps >= t).sum() / float(num_pos)
    ar = recalls.mean()
    return {'ar': ar, 'recalls': recalls, 'thresholds': thresholds, 'gt_overlaps': gt_overlaps, 'num_pos': num_pos}


def roidb_entry(proposals, gt_boxes, gt_classes, is_crowd, gt_areas, interleave=None):
    """A roidb entry of one image: GT rows and proposal rows (gt_classes 0) in one 'boxes' array; `interleave` = a random generator
    that shuffles the GT rows among the proposal rows (the proposals' own order is kept)."""
    P, G = len(proposals), len(gt_boxes)
    n = P + G
    is_gt = np.zeros(n, bool)
    if interleave is not None and n:
        is_gt[interleave.choice(n, G, replace=False)] = True
    else:
        is_gt[:G] = True
    boxes = np.zeros((n, 4), np.float32)
    boxes[is_gt] = gt_boxes
    boxes[~is_gt] = proposals
    cls = np.zeros(n, np.int32)
    cls[is_gt] = gt_classes
    crowd = np.zeros(n, bool)
    crowd[is_gt] = is_crowd
    areas = np.zeros(n, np.asarray(gt_areas).dtype if G else np.float32)
    areas[is_gt] = gt_areas
    return {'boxes': boxes, 'gt_classes': cls, 'is_crowd': crowd, 'seg_areas': areas}


def random_scene(rng, P, G, W=1024, H=800, crowd_frac=0.1, dup_frac=0.0):
    """Proposals near GT boxes and random ones (gen_rois-like), float32, with integer-ish coordinates so that ties occur."""
    def boxes(n, lo=4, hi=400):
        x1 = rng.uniform(0, W - 8, n)
        y1 = rng.uniform(0, H - 8, n)
        w = np.exp(rng.uniform(np.log(lo), np.log(hi), n))
        h = w * np.exp(rng.uniform(-0.7, 0.7, n))
        return np.stack([x1, y1, np.minimum(x1 + w, W - 1), np.minimum(y1 + h, H - 1)], 1)
    gt = np.round(boxes(G)).astype(np.float32)
    near = []
    if G:
        idx = rng.integers(0, G, P // 2)
        jit = rng.normal(0, 6, (len(idx), 4))
        near = gt[idx] + np.round(jit)
    props = np.concatenate([np.asarray(near).reshape(-1, 4), np.round(boxes(P - len(near)))]).astype(np.float32)
    props = props[rng.permutation(P)]
    if dup_frac and P > 1:
        k = int(P * dup_frac)
        props[rng.integers(0, P, k)] = props[rng.integers(0, P, k)]
    cls = rng.integers(1, 9, G).astype(np.int32)
    crowd = rng.random(G) < crowd_frac
    areas = ((gt[:, 2] - gt[:, 0] + 1) * (gt[:, 3] - gt[:, 1] + 1) * rng.uniform(0.5, 1.0, G)).astype(np.float32)
    return props, gt, cls, crowd, areas
