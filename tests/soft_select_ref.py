"""The soft detection selection restated in numpy, written from the rule and not from the kernel (csrc/detect.hip
mroi_soft_kernel): what tests/test_soft_select_cpu.py checks by hand and what tests/test_soft_select_gpu.py holds the device to bit for
bit. The candidates are box_vote_ref.decode (oracle.ops.bbox_transform / clip_boxes, the bit-exact twins of ups_decode_clip), the
per-class soft-NMS is oracle.soft_nms (pinned against the reference's compiled cpu_nms.pyx), the flat list and the max_det rule are
plain numpy."""
import numpy as np

import oracle

import box_vote_ref as bref

F = np.float32
CLASS_LIMIT = 4096        # candidates a class holds (its state is LDS-resident)
FILL = 256                # rows always defined (zero rows past the count), with max_det: max(max_det, FILL)


def candidates(rois, delta, prob, n, im_info, weights, clip, score_thresh):
    """{c: (dets [k,5] float32 (box, score), rows [k] int64)} for c = 1..C-1: the rows r < n with prob[r,c] > score_thresh, ascending."""
    rois, delta, prob = (np.asarray(a, F) for a in (rois, delta, prob))
    N, C = prob.shape
    n = min(max(int(n), 0), N)
    out = {}
    for c in range(1, C):
        rows = np.where(prob[:n, c] > F(score_thresh))[0]
        boxes = bref.decode(rois, delta, c, n, im_info, weights, clip)[rows]
        out[c] = (np.concatenate([boxes, prob[rows, c][:, None]], 1).astype(F).reshape(-1, 5), rows.astype(np.int64))
    return out


def soft_select(rois, delta, prob, n, im_info, weights, clip, score_thresh, nms_thresh, max_det, method, sigma, floor, cands=None):
    """dict(boxes [d,5], scores [d], cls [d] int64, src [d] int32, num, T, per_class): the d = max(|num|, min(cap, max(max_det, 256)))
    rows the device defines (the selection, then zero rows), num as the device reports it (negative: a class held more than
    CLASS_LIMIT candidates and kept its first CLASS_LIMIT), T the length of the flat list before the max_det rule and per_class the
    candidate count of every class."""
    prob = np.asarray(prob, F)
    N, C = prob.shape
    cap = (C - 1) * N
    if cands is None:
        cands = candidates(rois, delta, prob, n, im_info, weights, clip, score_thresh)
    boxes, scores, cls, src, per_class = [], [], [], [], []
    overflow = False
    for c in range(1, C):
        dets, rows = cands[c]
        per_class.append(len(rows))
        if len(rows) > CLASS_LIMIT:
            overflow, dets, rows = True, dets[:CLASS_LIMIT], rows[:CLASS_LIMIT]
        res, inds = oracle.soft_nms(dets, sigma=sigma, Nt=nms_thresh, threshold=floor, method=method)
        k = len(inds)
        boxes.append(res[:k, :4]), scores.append(res[:k, 4]), src.append(rows[inds]), cls.append(np.full(k, c, np.int64))
    boxes = np.concatenate(boxes).astype(F).reshape(-1, 4)
    scores, cls, src = np.concatenate(scores).astype(F), np.concatenate(cls).astype(np.int64), np.concatenate(src).astype(np.int32)
    T = len(scores)
    if max_det > 0 and T > max_det:
        thr = np.sort(scores)[-max_det]
        keep = np.where(scores >= thr)[0]
        boxes, scores, cls, src = boxes[keep], scores[keep], cls[keep], src[keep]
    cnt = len(scores)
    if cnt == 0:      # the reference's dummy row (mask_roi.py:135-141)
        boxes, scores, cls, src, cnt = np.zeros((1, 4), F), np.ones(1, F), np.zeros(1, np.int64), np.zeros(1, np.int32), 1
    d = max(cnt, min(cap, max(max_det, FILL)))
    out = dict(boxes=np.zeros((d, 5), F), scores=np.zeros(d, F), cls=np.zeros(d, np.int64), src=np.full(d, -1, np.int32),
               num=-cnt if overflow else cnt, T=T, per_class=per_class)
    out['boxes'][:cnt, 1:], out['scores'][:cnt], out['cls'][:cnt], out['src'][:cnt] = boxes, scores, cls, src
    return out


def cluster_inputs(rng, N, C, distinct=True):
    """box_vote_ref.cluster_case's rois / delta / prob (jittered clusters: the candidates of a cluster overlap each other with IoU >
    0.8). distinct: every probability of a class column is redrawn until the column holds no value twice (935 float32 draws in a
    column collide now and then), so that the visiting order does not depend on how ties are broken."""
    case = bref.cluster_case(rng, N, C, 0)
    prob = case['prob']
    while distinct:
        distinct = False
        for c in range(C):
            _, first = np.unique(prob[:, c], return_index=True)
            dup = np.setdiff1d(np.arange(N), first)
            if len(dup):
                prob[dup, c] = rng.uniform(0.0, 1.0, len(dup)).astype(F)
                distinct = True
    return case['rois'], case['delta'], prob


def decayed(res, prob):
    """Boolean per selected row: its score is no longer prob[src, cls]."""
    k = abs(res['num'])
    if k == 1 and res['cls'][0] == 0:
        return np.zeros(1, bool)
    return res['scores'][:k] != np.asarray(prob, F)[res['src'][:k], res['cls'][:k]]
