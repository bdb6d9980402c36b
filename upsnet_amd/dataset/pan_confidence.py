"""Scores of panoptic segments from the confidence plane, and the removal of the doubtful ones, on the device (csrc/pan_confidence.hip;
DESIGN.md section 4.29).

With config.test.pan_confidence the model returns, beside the panoptic label map, one byte per pixel: 255 x the softmax over the panoptic
logits (stuff channels, one channel per kept instance, the void channel) at the winning label -- how sure the head was of the label it
gave. The score of a segment of the unified 2-channel map is the mean of that over its pixels. The reference keeps the arg-max only;
the rules are this project's own, stated in include/upsnet_hip.h and restated in plain numpy in tests/pan_confidence_ref.py. The
posterior is not calibrated, and nothing here claims that filtering by it improves PQ.

    scores = segment_scores(pan_2ch, conf)            # {(category, instance): (area, sum_q, score)}
    kept = filter_by_score(pans, confs, 0.5)           # segments of score < 0.5 become VOID
"""
import numpy as np
import torch

from .. import ops
from .pq import _check_image

MAX_PIXELS = 1 << 24
HEAD, ROW = 4, 3              # the table of ops.pan_segment_scores: [0] = rows, then (key, area, sum_q) from word 4
FAST_ROWS = 256               # rows that travel with the header; a map with more segments costs a second copy


def check_min_score(min_score):
    """ValueError unless 0 <= min_score <= 1."""
    if isinstance(min_score, bool) or not isinstance(min_score, (int, float)) or not (0.0 <= float(min_score) <= 1.0):
        raise ValueError("min_score must be a number in 0..1, got %r" % (min_score,))


def _on_device(pan_2ch, conf):
    _check_image('pan_2ch', pan_2ch)
    H, W = int(pan_2ch.shape[0]), int(pan_2ch.shape[1])
    if H * W == 0 or H * W > MAX_PIXELS:
        raise ValueError("a map of %d x %d pixels cannot be scored: H * W must lie in 1..2^24" % (H, W))
    if tuple(conf.shape) != (H, W) or str(conf.dtype).split('.')[-1] != 'uint8':
        raise ValueError("the confidence plane of a %d x %d map must be uint8 [%d,%d], got %s %s" % (H, W, H, W, tuple(conf.shape), conf.dtype))
    dev = pan_2ch.device if isinstance(pan_2ch, torch.Tensor) else (conf.device if isinstance(conf, torch.Tensor) else
                                                                   torch.device('cuda', torch.cuda.current_device()))
    put = [torch.from_numpy(np.ascontiguousarray(t)).to(dev, non_blocking=True) if isinstance(t, np.ndarray) else t for t in (pan_2ch, conf)]
    if not all(t.is_cuda for t in put):
        raise RuntimeError("pan_confidence: map and plane must be on the device (there is no CPU fallback)")
    return put[0].contiguous(), put[1].contiguous()


def score_rows(table):
    """The rows of an ops.pan_segment_scores table on the host: uint32 [n,3] (key, area, sum_q) in ascending key. One small copy, and
    a second one for a map of more than FAST_ROWS segments."""
    head = table[:HEAD + ROW * FAST_ROWS].cpu().numpy().view(np.uint32)
    n = int(head[0])
    if n > FAST_ROWS:
        head = table[:HEAD + ROW * n].cpu().numpy().view(np.uint32)
    return head[HEAD:HEAD + ROW * n].reshape(n, ROW)


def segment_scores(pan_2ch, conf):
    """{(category, instance): (area, sum_q, score)} of one 2-channel map (uint8 [H,W,3]) and its confidence plane (uint8 [H,W]), device
    tensors or numpy arrays (uploaded): area pixels whose confidence bytes sum to sum_q, score = sum_q / (255.0 * area) in float64 on
    the host. VOID (category 255) has no entry; the dictionary is in ascending (category, instance)."""
    pan_2ch, conf = _on_device(pan_2ch, conf)
    rows = score_rows(ops.pan_segment_scores(pan_2ch, conf))
    return {(int(k) >> 8, int(k) & 255): (int(a), int(s), int(s) / (255.0 * int(a))) for k, a, s in rows.tolist()}


def filter_by_score(pans, confs, min_score, return_stats=False):
    """The maps of `pans` with every segment whose score (segment_scores) is below min_score turned into VOID (255, 0, 0): the test is
    float(sum_q) < min_score * float(255 * area), one double product, so the host decides as the device does. A list of new uint8
    [H,W,3] device tensors; the inputs are untouched. Four launches per map, nothing waits for the host. return_stats: also
    (segments before, segments after) summed over the maps, which costs two small copies per map. ValueError before any launch: counts
    that differ, a map or plane of the wrong shape or type, min_score outside 0..1."""
    check_min_score(min_score)
    pans, confs = list(pans), list(confs)
    if len(pans) != len(confs):
        raise ValueError("%d maps and %d confidence planes" % (len(pans), len(confs)))
    out, before, after = [], 0, 0
    for pan, conf in zip(pans, confs):
        pan, conf = _on_device(pan, conf)
        table = ops.pan_segment_scores(pan, conf)
        kept = ops.pan_score_filter(pan, table, float(min_score))
        out.append(kept)
        if return_stats:
            rows = score_rows(table)
            before += len(rows)
            after += int((rows[:, 2].astype(np.float64) >= float(min_score) * (255.0 * rows[:, 1].astype(np.float64))).sum())
    return (out, (before, after)) if return_stats else out
