"""Instance masks -> COCO RLE: host mirror of im_post (upsnet/upsnet_end2end_test.py:95-152).

The reference resizes / thresholds / pastes every detection's mask over the whole image on the host and calls
pycocotools.mask.encode. Here the device kernel (csrc/postprocess.hip: im_post_rle_kernel) evaluates only the box region and
returns the run-length encoding as the list of column-major pixel indices where the mask value changes; this module turns
that into pycocotools' `counts` (differences) and its compressed string (rleToString of pycocotools' maskApi.c -- a third-party
format, restated from the published algorithm).
"""

import numpy as np
import torch

from .._lib import check, f32c, i64c, lib, ptr, stream


def counts_from_transitions(positions, num_pixels):
    """Sorted change positions -> pycocotools counts (alternating zeros / ones, starting with zeros)."""
    p = np.concatenate([[0], np.asarray(positions, np.int64), [int(num_pixels)]])
    return np.diff(p).tolist()


def rle_to_string(counts):
    out = []
    for i, c in enumerate(counts):
        x = int(c)
        if i > 2:
            x -= int(counts[i - 2])
        more = True
        while more:
            ch = x & 0x1f
            x >>= 5
            more = (x != -1) if (ch & 0x10) else (x != 0)
            if more:
                ch |= 0x20
            out.append(chr(ch + 48))
    return ''.join(out)


def mask_transitions(pred_boxes, pred_masks, cls_inds, im_h, im_w, cap=4096):
    """Device part: pred_boxes [n,4] (image coordinates), pred_masks [n,C,M,M] (or [n,1,M,M]), cls_inds [n] ->
    list of n int64 arrays of change positions. Grows `cap` and retries when a mask has more transitions."""
    n = pred_boxes.shape[0]
    if n == 0:
        return []
    boxes, masks, cls = f32c(pred_boxes), f32c(pred_masks), i64c(cls_inds)
    if not (boxes.is_cuda and masks.is_cuda and cls.is_cuda):
        raise RuntimeError("mask_transitions: CUDA tensors required")
    C, M = masks.shape[1], masks.shape[-1]
    while True:
        trans = torch.empty((n, cap), dtype=torch.int32, device=boxes.device)
        cnt = torch.empty((n,), dtype=torch.int32, device=boxes.device)
        check(lib().upsnet_im_post_rle(stream(), ptr(boxes), ptr(masks), ptr(cls), n, C, M, int(im_h), int(im_w), int(cap), ptr(trans), ptr(cnt)),
              "im_post_rle")
        c = cnt.cpu().numpy()
        if int(c.max()) <= cap:
            break
        cap = int(c.max())
    t = trans.cpu().numpy().view(np.uint32)
    return [t[d, :c[d]].astype(np.int64) for d in range(n)]


def im_post(boxes_all, masks_all, scores, pred_boxes, pred_masks, cls_inds, num_classes, im_info):
    """Same contract as the reference's im_post: appends per-class [boxes|score] arrays to boxes_all[cls] and lists of
    {'size': [h, w], 'counts': str} to masks_all[cls]. pred_* are device tensors of ONE image; im_info = (height, width)."""
    im_h, im_w = int(im_info[0]), int(im_info[1])
    trans = mask_transitions(pred_boxes, pred_masks, cls_inds, im_h, im_w)
    cls_np = cls_inds.cpu().numpy()
    boxes_np = pred_boxes.float().cpu().numpy()
    scores_np = np.asarray(scores.cpu().numpy() if isinstance(scores, torch.Tensor) else scores).reshape(-1, 1)
    for idx in range(1, num_classes):
        sel = np.nonzero(cls_np == idx)[0]
        segms = [{'size': [im_h, im_w], 'counts': rle_to_string(counts_from_transitions(trans[d], im_h * im_w))} for d in sel]
        boxes_all[idx].append(np.hstack([boxes_np[sel], scores_np[sel]]))
        masks_all[idx].append(segms)


def _segmented_cumsum(v, starts):
    """Cumulative sums of v restarted at every index where `starts` is set (starts[0] must be set)."""
    cs = np.cumsum(v)
    first = np.flatnonzero(starts)
    return cs - (cs[first] - v[first])[np.cumsum(starts) - 1]


def decode_rle_strings(strings):
    """pycocotools' compressed RLE strings -> (counts int64, code offsets int64 [n + 1]): counts[off[j]:off[j+1]] are the counts of
    strings[j], as dataset.coco_eval.rle_from_string returns them (rleFrString of maskApi.c), decoded for all strings at once with
    array operations. A string whose last character continues a code raises ValueError."""
    enc = [s if isinstance(s, bytes) else s.encode('ascii') for s in strings]
    n = len(enc)
    lens = np.fromiter((len(s) for s in enc), np.int64, n)
    c = np.frombuffer(b''.join(enc), np.uint8).astype(np.int64) - 48
    end = (c & 0x20) == 0                                   # the character ends a code
    char_end = np.cumsum(lens)
    if np.any(lens > 0) and not np.all(end[char_end[lens > 0] - 1]):
        raise ValueError("RLE string ends inside a code")
    code_first = np.flatnonzero(np.concatenate([[True], end[:-1]])) if c.size else np.zeros(0, np.int64)
    code_of = np.cumsum(end) - end                          # code index of every character
    k = np.arange(c.size) - code_first[code_of]             # position of the character in its code
    x = np.add.reduceat((c & 0x1f) << (5 * k), code_first) if c.size else np.zeros(0, np.int64)
    ln = np.diff(np.concatenate([code_first, [c.size]]))
    neg = (c[code_first + ln - 1] & 0x10) != 0
    x[neg] -= np.left_shift(1, 5 * ln[neg])                 # x |= -1 << 5 k on the (non-negative) value
    off = np.concatenate([[0], np.cumsum(end)])[np.concatenate([[0], char_end])].astype(np.int64)
    codes_per = np.diff(off)
    j = np.arange(x.size) - np.repeat(off[:-1], codes_per)  # index of the code in its string
    counts = x.copy()
    # counts[j] = x[j] + counts[j - 2] for j > 2: per string, cumulative sums over j = 1, 3, 5, ... and over j = 2, 4, 6, ...
    for sel, starts in (((j & 1) == 1, j == 1), ((j & 1) == 0, (j == 0) | (j == 2))):
        idx = np.flatnonzero(sel)
        if idx.size:
            counts[idx] = _segmented_cumsum(x[idx], starts[idx])
    return counts, off
