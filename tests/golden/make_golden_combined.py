#!/usr/bin/env python
"""Golden vectors for the combined panoptic merge, made by the REFERENCE's own Python: BaseDataset._merge_pred_single_core
(upsnet/dataset/base_dataset.py:404-449) on one worker, imported from the reference checkout with the in-process shims of
make_golden_blob.py plus a `pycocotools.mask.decode` stand-in (rleFrString + rleDecode of maskApi.c, restated). The candidates are
ordered as get_combined_pan_result (:373-385) orders them (classes concatenated, np.argsort(score)[::-1]).

The scenes avoid the two places where the reference is ambiguous: no two scores are equal (its argsort is unstable) and no quotient
remain / area equals fl32(fraction_threshold) (numpy 1.x and 2.x compare it differently). tests/test_pan_combined_cpu.py pins those
by hand-derived cases.

Run in the build container:  python tests/golden/make_golden_combined.py   (writes tests/golden/pan_combined.npz)
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_blob as mgb  # noqa: E402  (shims, the reference checkout on sys.path, the reference's BaseDataset)

BaseDataset, config = mgb.BaseDataset, mgb.config

NUM_CLASSES, NUM_SEG = 9, 19          # Cityscapes: id_last_stuff = 10
SCORE_THR, FRAC_THR = 0.6, 0.7


def rle_string(counts):
    """rleToString of maskApi.c."""
    out = []
    for i, c in enumerate(counts):
        x = int(c) - (int(counts[i - 2]) if i > 2 else 0)
        more = True
        while more:
            ch = x & 0x1f
            x >>= 5
            more = (x != -1) if (ch & 0x10) else (x != 0)
            out.append(chr((ch | (0x20 if more else 0)) + 48))
    return ''.join(out)


def rle_counts(s):
    """rleFrString of maskApi.c."""
    counts, p = [], 0
    while p < len(s):
        x, k, more = 0, 0, True
        while more:
            c = ord(s[p]) - 48
            x |= (c & 0x1f) << 5 * k
            more = bool(c & 0x20)
            p += 1
            k += 1
            if not more and (c & 0x10):
                x |= -1 << 5 * k
        if len(counts) > 2:
            x += counts[-2]
        counts.append(x)
    return counts


def encode(mask):
    h, w = mask.shape
    flat = mask.T.reshape(-1).astype(np.int8)
    pos = np.concatenate([[0], np.flatnonzero(np.diff(flat)) + 1, [flat.size]])
    counts = np.diff(pos).tolist()
    if flat[0]:
        counts = [0] + counts
    return {'size': [h, w], 'counts': rle_string(counts)}


def decode(rle):
    """pycocotools.mask.decode of one RLE dict: uint8 [h, w] (column-major runs)."""
    h, w = rle['size']
    counts = rle_counts(rle['counts'])
    return np.repeat(np.arange(len(counts)) % 2, counts).astype(np.uint8).reshape(w, h).T.copy()


sys.modules['pycocotools.mask'].decode = decode


def scene(rng, h, w, n):
    """Semantic map with stuff blocks of assorted sizes and thing blobs; n detections: boxes with masks (rectangles and ellipses,
    some overlapping heavily, some full-width), scores spread across the threshold, all distinct."""
    sem = rng.integers(0, 11, (h // 8 + 1, w // 8 + 1)).repeat(8, 0).repeat(8, 1)[:h, :w]
    for _ in range(6):
        y, x = rng.integers(0, h), rng.integers(0, w)
        sem[y:y + rng.integers(4, h // 2), x:x + rng.integers(4, w // 2)] = rng.integers(11, 19)
    sem[rng.random((h, w)) < 0.01] = rng.integers(0, 19)
    sem[0:3, 0:5] = 255 if rng.random() < 0.5 else 7
    yy, xx = np.mgrid[0:h, 0:w]
    boxes, cls, rles = [], [], []
    scores = rng.permutation(np.linspace(0.3, 0.99, n) + 0.0017).astype(np.float32)
    base = None
    for d in range(n):
        if d % 11 == 3:
            m = np.zeros((h, w), bool)
            y0 = int(rng.integers(0, h - h // 5))
            m[y0:y0 + h // 5, :] = True                             # full width
        elif d % 5 == 2 and base is not None:
            m = np.roll(base, (int(rng.integers(-2, 3)), int(rng.integers(-3, 4))), (0, 1))   # heavy overlap with an earlier mask
        elif d % 2:
            cy, cx, ry, rx = rng.uniform(0, h), rng.uniform(0, w), rng.uniform(2, h / 3), rng.uniform(2, w / 3)
            m = ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1
        else:
            y0, x0 = rng.integers(0, h - 2), rng.integers(0, w - 2)
            m = np.zeros((h, w), bool)
            m[y0:y0 + rng.integers(1, h // 2), x0:x0 + rng.integers(1, w // 2)] = True
        if d == 1:
            m[:] = False                                            # an empty mask
        base = m if d % 3 == 0 else base
        ys, xs = np.nonzero(m)
        box = [xs.min(), ys.min(), xs.max(), ys.max()] if ys.size else [0, 0, 0, 0]
        boxes.append(list(np.float32(box)) + [scores[d]])
        cls.append(int(rng.integers(1, NUM_CLASSES)))
        rles.append(encode(m))
    return sem.astype(np.uint8), np.array(boxes, np.float32), np.array(cls, np.int32), rles


def check_unambiguous(boxes, rles):
    """No score ties; no quotient equal to fl32(FRAC_THR) along the reference's own greedy (recomputed here)."""
    s = boxes[:, 4]
    assert np.unique(s).size == s.size and not np.any(s == np.float32(SCORE_THR))
    occ = None
    for k in np.argsort(s)[::-1]:
        if s[k] < SCORE_THR:
            continue
        m = decode(rles[k]).astype(bool)
        occ = np.zeros(m.shape, bool) if occ is None else occ
        a = int(m.sum())
        if a == 0:
            continue
        q = np.float32(np.float32((m & ~occ).sum()) / np.float32(a))
        assert q != np.float32(FRAC_THR), "ambiguous quotient"
        if float(q) >= FRAC_THR:
            occ |= m


def main():
    config.dataset = mgb.mg.EasyDict(num_classes=NUM_CLASSES, num_seg_classes=NUM_SEG)
    out = {'num_classes': np.int64(NUM_CLASSES), 'num_seg_classes': np.int64(NUM_SEG), 'score_threshold': np.float64(SCORE_THR),
           'fraction_threshold': np.float64(FRAC_THR)}
    specs = [(48, 80, 24, 150), (37, 53, 30, 60), (64, 64, 40, 200), (20, 90, 12, 40)]
    out['stuff_area_limit'] = np.array([s[3] for s in specs], np.int64)
    for i, (h, w, n, limit) in enumerate(specs):
        rng = np.random.default_rng(500 + i)
        sem, boxes, cls, rles = scene(rng, h, w, n)
        check_unambiguous(boxes, rles)
        order = np.argsort(boxes[:, 4])[::-1]                      # get_combined_pan_result's ordering (:381)
        masks = np.array(rles)
        pan = BaseDataset._merge_pred_single_core(0, [boxes[order]], [cls[order]], [masks[order]], [sem.copy()], SCORE_THR, FRAC_THR,
                                                  int(limit))[0]
        assert pan.dtype == np.uint8 and pan.shape == (h, w, 3)
        out['seg_%d' % i] = sem
        out['boxes_%d' % i] = boxes
        out['cls_%d' % i] = cls
        out['rle_%d' % i] = np.array([r['counts'] for r in rles])
        out['pan_%d' % i] = pan
        key = pan[:, :, 0].astype(np.int64) * 256 + pan[:, :, 1]
        print('scene %d: %dx%d, %d dets, %d instances' % (i, h, w, n, np.unique(key[pan[:, :, 1] > 0]).size))
    out['num_scenes'] = np.int64(len(specs))
    np.savez_compressed(os.path.join(HERE, 'pan_combined.npz'), **out)


if __name__ == '__main__':
    main()
