"""The box voting rule restated in numpy float32, written from the rule and not from the kernel (csrc/box_vote.hip):
what tests/test_box_vote_cpu.py checks by hand and against float64, and what tests/test_box_vote_gpu.py holds the device to bit for
bit. The decode goes through oracle.ops.bbox_transform / clip_boxes, the bit-exact twins of ups_decode_clip; every other operation is
one float32 numpy operation in the order the rule writes it (numpy never contracts a product and a sum).

Also here: the jittered-cluster inputs both test files use (cluster_case)."""
import math

import numpy as np

from oracle import ops as oops

F = np.float32
STRIPES = 64


def decode(rois, delta, c, n, im_info, weights, clip):
    """The class-c candidate boxes of rows 0..n-1, [n,4] float32, as the detection selection builds them."""
    d = oops.bbox_transform(rois[:n, 1:5], delta[:n, 4 * c:4 * c + 4], weights)
    if clip and n:
        d = oops.clip_boxes(d, (im_info[0], im_info[1]))
    return d.astype(F).reshape(n, 4)


def iou(b, d):
    """The "+1" IoU of box b (4 float32) with every row of d [n,4], float32, operation by operation as ups_iou."""
    one, zero = F(1), F(0)
    left, right = np.maximum(b[0], d[:, 0]), np.minimum(b[2], d[:, 2])
    top, bottom = np.maximum(b[1], d[:, 1]), np.minimum(b[3], d[:, 3])
    width, height = np.maximum(right - left + one, zero), np.maximum(bottom - top + one, zero)
    inter = width * height
    sa = (b[2] - b[0] + one) * (b[3] - b[1] + one)
    sb = (d[:, 2] - d[:, 0] + one) * (d[:, 3] - d[:, 1] + one)
    with np.errstate(divide='ignore', invalid='ignore'):
        return inter / (sa + sb - inter)


def voters(b, w, d, score_thresh, iou_thresh):
    """Boolean [n]: w > score_thresh (strict) and iou(b, d) >= iou_thresh (a NaN IoU is no voter)."""
    with np.errstate(invalid='ignore'):
        return (w > F(score_thresh)) & (iou(b, d) >= F(iou_thresh))


def striped_sums(v, w, d):
    """The five sums (S_w, S_x1, S_y1, S_x2, S_y2) over the voters v: partial j of 64 starts at +0 and adds the terms of the voters
    r with r % 64 == j in ascending r; then p[j] = p[j] + p[j+s] for s = 32 .. 1. float32."""
    n = len(w)
    p = np.zeros((5, STRIPES), F)
    for base in range(0, n, STRIPES):                 # one step of every stripe: rows base .. base + 63
        m = min(STRIPES, n - base)
        rows = slice(base, base + m)
        t = np.empty((5, m), F)
        t[0] = w[rows]
        for i in range(4):
            t[1 + i] = w[rows] * d[rows, i]           # one rounded multiply
        p[:, :m] = np.where(v[rows][None], p[:, :m] + t, p[:, :m])
    s = STRIPES // 2
    while s >= 1:
        p[:, :s] = p[:, :s] + p[:, s:2 * s]
        s //= 2
    return p[:, 0].copy()


def box_vote(rois, delta, prob, n, im_info, weights, clip, boxes, cls, num, score_thresh, iou_thresh, want_counts=False):
    """voted [cap,5] float32 (and with want_counts the voter count of every row k < max(num, 0))."""
    rois, delta, prob, boxes = (np.asarray(a, F) for a in (rois, delta, prob, boxes))
    N, C = prob.shape
    cap = boxes.shape[0]
    n = min(max(int(n), 0), N)
    kn = min(max(int(num), 0), cap)
    voted = boxes.copy()
    decoded, counts = {}, []
    hi = (F(im_info[1]) - F(1), F(im_info[0]) - F(1))        # x, y
    for k in range(kn):
        c = min(max(int(cls[k]), 0), C - 1)
        if c not in decoded:
            decoded[c] = decode(rois, delta, c, n, im_info, weights, clip)
        d, w, b = decoded[c], prob[:n, c], boxes[k, 1:5]
        v = voters(b, w, d, score_thresh, iou_thresh)
        counts.append(int(v.sum()))
        s = striped_sums(v, w, d)
        if s[0] > 0:
            with np.errstate(invalid='ignore', over='ignore'):
                out = s[1:] / s[0]
            if clip:
                for i in range(4):
                    out[i] = np.fmax(np.fmin(out[i], hi[i % 2]), F(0))
            voted[k, 1:5] = out
    return (voted, counts) if want_counts else voted


def box_vote_f64(rois, delta, prob, n, im_info, weights, clip, boxes, cls, num, score_thresh, iou_thresh):
    """The same formula with the sums and the division in float64 (plain sums: the order does not matter at this precision), over the
    same float32 voters, weights and candidate boxes. Returns (voted [kn,4] float64, voter counts, max |candidate coordinate| per row)."""
    rois, delta, prob, boxes = (np.asarray(a, F) for a in (rois, delta, prob, boxes))
    N, C = prob.shape
    n = min(max(int(n), 0), N)
    kn = min(max(int(num), 0), boxes.shape[0])
    out, counts, mags = np.zeros((kn, 4)), [], []
    for k in range(kn):
        c = min(max(int(cls[k]), 0), C - 1)
        d, w, b = decode(rois, delta, c, n, im_info, weights, clip), prob[:n, c], boxes[k, 1:5]
        v = voters(b, w, d, score_thresh, iou_thresh)
        counts.append(int(v.sum()))
        w64, d64 = w[v].astype(np.float64), d[v].astype(np.float64)
        if w64.sum() > 0:
            res = (w64[:, None] * d64).sum(0) / w64.sum()
            if clip:
                res[0::2] = np.clip(res[0::2], 0, float(F(im_info[1]) - F(1)))
                res[1::2] = np.clip(res[1::2], 0, float(F(im_info[0]) - F(1)))
            out[k] = res
            mags.append(float(np.abs(d64).max()))
        else:
            out[k] = b
            mags.append(0.0)
    return out, counts, mags


def bound(max_coord, V):
    """First-order bound on |float32 rule - float64 formula| for a row with V voters: one rounding per term, a stripe of
    ceil(V/64) sequential adds, six tree levels, for the numerator and the denominator each, and one division."""
    return max_coord * (2 * math.ceil(V / STRIPES) + 16) * 2.0 ** -24


# ------------------------------------------------------------------------------------------------ inputs
REG_WEIGHTS = (10.0, 10.0, 5.0, 5.0)
IM_INFO = np.array([600.0, 900.0, 1.0], F)


def cluster_case(rng, N, C, kept, clip=True, big=0, pad=37, low_prob=False):
    """Proposals as jittered clusters: rows are a few pixels of jitter around a handful of centres (boxes of ~200 px, so that the
    jittered boxes of a cluster overlap each other with IoU > 0.8), small deltas, random probabilities. `big` rows go to the first
    cluster (more than 128 voters need several terms per stripe). The first cluster hangs over the image's top left corner and the
    last over its bottom right one (IM_INFO), so the clip and the second clamp matter. The kept list: `kept` rows, each the exact
    class-c candidate of a random (row, class) -- what the selection would have kept -- followed by `pad` rows of arbitrary values
    (cap = kept + pad).
    Returns dict(rois, delta, prob, boxes, cls, num, src)."""
    centres = np.array([[60, 70], [420, 160], [700, 150], [250, 420], [830, 520]], np.float64)
    which = rng.integers(0, len(centres), N)
    which[:min(big, N)] = 0
    half = rng.uniform(90, 110, (len(centres), 2))
    c = centres[which] + rng.uniform(-1.5, 1.5, (N, 2))
    h = half[which] + rng.uniform(-1.5, 1.5, (N, 2))
    rois = np.concatenate([np.zeros((N, 1)), c - h, c + h], 1).astype(F)
    delta = rng.normal(0, 0.05, (N, 4 * C)).astype(F)
    prob = rng.uniform(0.0, 0.04 if low_prob else 1.0, (N, C)).astype(F)
    src = rng.integers(0, N, kept)
    cls = rng.integers(1, C, kept).astype(np.int64)
    if big and kept:
        src[0], cls[0] = 0, 1                      # a kept row inside the large cluster
    boxes = np.zeros((kept + pad, 5), F)
    for k in range(kept):
        boxes[k, 1:] = decode(rois[src[k]:src[k] + 1], delta[src[k]:src[k] + 1], int(cls[k]), 1, IM_INFO, REG_WEIGHTS, clip)[0]
    boxes[kept:] = rng.normal(0, 300, (pad, 5)).astype(F)
    cls_all = np.concatenate([cls, rng.integers(0, C, pad)]).astype(np.int64)
    return dict(rois=rois, delta=delta, prob=prob, boxes=boxes, cls=cls_all, num=kept, src=src)
