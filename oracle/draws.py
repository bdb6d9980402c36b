"""oracle.draws -- TEST INFRASTRUCTURE ONLY: the weight / image draws of the multi-draw parity tests and the classifier-gain rule
they are built with.

synthetic.DEFAULT_CLS_GAIN was fitted to weight seed 235 alone (tools/calib_gain_cpu.py); under it other seeds keep 1-4 panoptic
instances of UPSNet-50. fit_cls_gain is the same criterion for ANY seed: the proposals of one seeded calibration image (FIT_SIZE,
image seed = weight seed + 3) go through the box head on the host, and the gain is the smallest one at which FIT_CLS_SHARE of them
have a best foreground probability above the panoptic threshold -- the share seed 235 has under DEFAULT_CLS_GAIN on its own
calibration image (60 of 1000 proposals for UPSNet-50, 94 of 300 for UPSNet-101-DCN). A function of (model, weight seed) alone: it
never looks at a parity result. On seed 235 it returns 5.39 / 21.9 against the hand-fitted 5.4 / 22.0.

Usage: synthetic.build_model(seed=weight_seed, cls_gain=fit_cls_gain); make_image(h, w, seed=image_seed)."""
import math

import numpy as np
import torch
import torch.nn.functional as F

# (weight seed, image seed), fixed before any of them was run on a GPU; tests/test_trunk_gpu.py, test_layerwise_gpu.py and
# test_model_gpu.py run each one with cls_gain=fit_cls_gain
DRAWS = [(236, 11), (237, 12), (238, 13), (1, 15)]

FIT_CLS_SHARE = {9: 0.06, 81: 0.313}
FIT_SIZE = (256, 512)
FIT_GAIN_RANGE = (1.0, 64.0)


def _fg_share(logits, gain, thresh):
    """share of the rows of `logits` whose best foreground (class >= 1) softmax probability at `gain` exceeds `thresh` (float64)."""
    p = torch.softmax(logits.double() * gain, dim=1)
    return float((p[:, 1:].max(dim=1)[0] > thresh).double().mean())


def fit_cls_gain(model, seed):
    """The gain rule (module docstring) for a calibrated, UNSCALED model on the CPU (synthetic.build_unprepared calls it before it
    scales rcnn.cls_score): host forward of trunk, FPN, RPN, proposals and box head on make_image(*FIT_SIZE, seed=seed + 3), then
    bisection on log(gain) inside FIT_GAIN_RANGE (40 steps) for the smallest gain at which the share of proposals with a best
    foreground probability above config.test.panoptic_score_thresh reaches FIT_CLS_SHARE; rounded to 0.01. Deterministic."""
    from upsnet_amd.config.config import config as cfg
    from upsnet_amd.synthetic import make_image
    from . import ops as oops
    from .forward import _backbone_cpu, _fpn_pool_cpu, _np
    target = FIT_CLS_SHARE[cfg.dataset.num_classes]
    data = make_image(FIT_SIZE[0], FIT_SIZE[1], seed=seed + 3)
    was_training = model.training
    model.eval()
    try:
        with torch.no_grad():
            pyr = model.fpn(*_backbone_cpu(model.resnet_backbone, data['data']))
            probs, boxes = [], []
            for f in pyr:
                _, b, p = model.rpn(f)
                probs.append(_np(p))
                boxes.append(_np(b))
            im_info = np.asarray(data['im_info'], np.float32)
            rois, _ = oops.pyramid_proposal(probs, boxes, im_info[0], cfg.network.rpn_feat_stride, cfg.network.anchor_scales,
                                            cfg.network.anchor_ratios, cfg.test.rpn_pre_nms_top_n, cfg.test.rpn_post_nms_top_n,
                                            cfg.test.rpn_nms_thresh, cfg.test.rpn_min_size)
            pool = _fpn_pool_cpu(list(pyr[:4]), rois, 7)
            fc7 = model.rcnn.fc7(F.relu(model.rcnn.fc6[0](pool.reshape(pool.shape[0], -1))))
            logits = model.rcnn.cls_score(fc7)
    finally:
        model.train(was_training)
    thresh = cfg.test.panoptic_score_thresh
    if _fg_share(logits, FIT_GAIN_RANGE[1], thresh) < target:
        return FIT_GAIN_RANGE[1]
    lo, hi = math.log(FIT_GAIN_RANGE[0]), math.log(FIT_GAIN_RANGE[1])
    for _ in range(40):
        mid = 0.5 * (lo + hi)
        if _fg_share(logits, math.exp(mid), thresh) >= target:
            hi = mid
        else:
            lo = mid
    return min(max(round(math.exp(hi), 2), FIT_GAIN_RANGE[0]), FIT_GAIN_RANGE[1])
