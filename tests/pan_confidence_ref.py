"""Panoptic confidence restated in numpy (include/upsnet_hip.h: upsnet_panoptic_fuse_up_conf, upsnet_pan_segment_scores,
upsnet_pan_score_filter). The softmax is taken in float64 over the oracle's own fp32 planes (oracle.upsample_bilinear,
oracle.ops.mask_removal, oracle.ops.seg_term; the void plane formed as in oracle.ops.panoptic_fuse_numpy); the segment sums and the
filter are plain loops. tests/test_pan_confidence_cpu.py holds this file to hand-derived literals; tests/test_pan_confidence_gpu.py
holds the device to this file.
"""
import os
import sys

import numpy as np

import oracle
from oracle import ops as oops

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import panoptic_cases as pc  # noqa: E402

F32 = np.float32
TOL = 1e-4                     # |conf - conf_ref64|: derived in test_pan_confidence_gpu.py's docstring
TILE_H, TILE_W = 8, 128        # the fused kernel's output tile


def quantize(conf):
    """The byte of a confidence, in fp32 as the device forms it: (unsigned)(conf * 255.0f + 0.5f)."""
    c = np.asarray(conf, F32)
    return (c * F32(255.0) + F32(0.5)).astype(np.uint32).astype(np.uint8)


def panoptic_logits(fcn_output, seg_inst, mask_energy, s_stuff):
    """[s_stuff + k + 1, H, W] fp32: stuff | seg_inst + mask_energy | void, the planes oracle.ops.panoptic_fuse_numpy compares."""
    fcn_output, seg_inst, mask_energy = [np.asarray(a, F32) for a in (fcn_output, seg_inst, mask_energy)]
    void = fcn_output[s_stuff:].max(0, keepdims=True) - seg_inst.max(0, keepdims=True)
    return np.concatenate([fcn_output[:s_stuff], seg_inst + mask_energy, void], 0)


def confidence(fcn_output, seg_inst, mask_energy, s_stuff, first_zero_only=False):
    """(conf float64 [H,W], winner int64 [H,W] with 255 for void): conf = P[winner] = 1 / sum_c exp(z_c - z_max) in float64.
    first_zero_only restates the MISTAKE the kernel must not make: of the instances that touch a pixel's 8 x 128 tile nowhere (both
    planes 0 all over it) only the first enters the sum, as in the arg-max."""
    z = panoptic_logits(fcn_output, seg_inst, mask_energy, s_stuff).astype(np.float64)
    k = np.asarray(seg_inst).shape[0]
    zmax = z.max(0)
    e = np.exp(z - zmax[None])
    if first_zero_only:
        si, me = np.asarray(seg_inst, F32), np.asarray(mask_energy, F32)
        H, W = zmax.shape
        for y0 in range(0, H, TILE_H):
            for x0 in range(0, W, TILE_W):
                sl = (slice(y0, y0 + TILE_H), slice(x0, x0 + TILE_W))
                untouched = [j for j in range(k) if not si[j][sl].any() and not me[j][sl].any()]
                for j in untouched[1:]:
                    e[s_stuff + j][sl] = 0.0
    conf = 1.0 / e.sum(0)
    win = np.argmax(z, 0).astype(np.int64)
    win[win == z.shape[0] - 1] = 255
    return conf, win


def head_confidence(score, rois5, prob, logit, cls, S, C, first_zero_only=False):
    """The head of oracle.ops.panoptic_head on the oracle's x4 upsampling of `score` [1,S,Hs,Ws], with the confidence:
    dict(keep_inds, panoptic, sem, conf (float64 [H,W]))."""
    fcn = oracle.upsample_bilinear(np.asarray(score, F32)[0], 4)[None]
    H, W = fcn.shape[2:]
    keep, energy = oops.mask_removal(np.asarray(rois5, F32)[:, 1:], prob, logit, cls, (H, W))
    mr = np.asarray(rois5, F32)[keep]
    ci = np.asarray(cls, np.int64)[keep]
    _, inst = oops.seg_term(ci, fcn, mr * F32(4.0), S, C)
    s_stuff = S - (C - 1)
    pan, sem = oracle.panoptic_fuse(fcn[0], s_stuff, inst[0], energy[0], True)
    conf, win = confidence(fcn[0], inst[0], energy[0], s_stuff, first_zero_only)
    assert np.array_equal(win, pan), "the softmax's maximum is not the oracle's label"
    return dict(keep_inds=keep, panoptic=pan, sem=sem, conf=conf)


def conf_crowd():
    """64 small all-positive boxes of 6 x 6 pixels on an 8 x 8 grid (pitch 32 x 16) of a 128 x 256 map, classes by turns, all kept; stuff
    and thing scores uniform in [-1, 1]. Far from every box z_max <= 1 and 63 or 64 instance logits are exactly 0: their terms sum to
    at least 63 / e. Returns ((score [1,S,32,64], rois5, prob, logit, cls, S, C, H, W), tag) like panoptic_cases.up_tiny."""
    rng = np.random.default_rng(6464)
    H, W, C, S = 128, 256, 5, 9
    rois = np.asarray([[32 * c + 12, 16 * r + 5, 32 * c + 17, 16 * r + 10] for r in range(8) for c in range(8)], F32)
    rois = rois[rng.permutation(64)]
    cls = (1 + np.arange(64) % (C - 1)).astype(np.int64)
    prob = np.linspace(0.99, 0.5, 64).astype(F32)
    score = rng.uniform(-1, 1, size=(1, S, H // 4, W // 4)).astype(F32)
    rois5 = np.hstack([np.zeros((64, 1), F32), rois]).astype(F32)
    return (score, rois5, prob, np.full((64, 1, pc.MS, pc.MS), 2.0, F32), cls, S, C, H, W), 'conf_crowd'


# ---------------------------------------------------------------------------------------------------- segment scores and the filter
def segment_sums(pan_2ch, conf):
    """{key = category << 8 | instance: [area, sum_q]} over the non-VOID pixels, one pixel at a time."""
    pan_2ch, conf = np.asarray(pan_2ch), np.asarray(conf)
    out = {}
    H, W = conf.shape
    for y in range(H):
        row, crow = pan_2ch[y], conf[y]
        for x in range(W):
            c = int(row[x, 0])
            if c == 255:
                continue
            cell = out.setdefault(c << 8 | int(row[x, 1]), [0, 0])
            cell[0] += 1
            cell[1] += int(crow[x])
    return out


def score_table(pan_2ch, conf):
    """uint32 [n, 3] rows (key, area, sum_q) in ascending key: the rows of upsnet_pan_segment_scores."""
    sums = segment_sums(pan_2ch, conf)
    return np.asarray([[k, sums[k][0], sums[k][1]] for k in sorted(sums)], np.uint32).reshape(-1, 3)


def segment_scores(pan_2ch, conf):
    """{(category, instance): (area, sum_q, score)}, score = sum_q / (255.0 * area) in float64."""
    return {(k >> 8, k & 255): (a, s, s / (255.0 * a)) for k, (a, s) in segment_sums(pan_2ch, conf).items()}


def score_filter(pan_2ch, conf, min_score):
    """Every pixel of a non-VOID key with float(sum_q) < min_score * float(255 * area) becomes (255, 0, 0)."""
    sums = segment_sums(pan_2ch, conf)
    drop = {k for k, (a, s) in sums.items() if float(s) < float(min_score) * float(255 * a)}
    out = np.array(pan_2ch, copy=True)
    H, W = out.shape[:2]
    for y in range(H):
        for x in range(W):
            c = int(out[y, x, 0])
            if c != 255 and (c << 8 | int(out[y, x, 1])) in drop:
                out[y, x] = (255, 0, 0)
    return out
