"""The detection-count regimes of the whole forward (plain data + one context manager): the synthetic model of the whole-model tests
runs one regime only -- about 100 per-class detections, a few dozen panoptic ones, every one of them also a per-class detection. The
code that strings the ops together by their device-side counts (resnet_upsnet._phase1 / _forward_fused / _forward_modules, tta._tail,
evaluate.post_image) has more: the reference's dummy detection on either side, a single real row, both selections at max_det, more
than 256 panoptic rows, "nothing kept" after mask removal, fewer proposals than the ROI buffer holds.

Every regime is reached on the seed-235 CITYSCAPES_R50 model with the knobs named here only. REGIMES[name]:
  image      key of IMAGES (height, width, seed of synthetic.make_image)
  test       fields of config.test to set; score_thresh / panoptic_score_thresh also go to model.mask_roi / model.mask_roi_panoptic
             (the modules read their attribute, oracle.forward.check_taps reads the configuration or its thresholds= argument)
  mask_bias  value the mask head's last bias is filled with, or None
  is_regime  predicate on the counts of check_taps / counts_of: dict(n_rois, n_det, n_pan, n_inst, classes) -- classes are the thing
             classes of the kept panoptic rows -- and the regime's max_det
tests/test_count_regimes_cpu.py asserts, with the oracle alone, that each case is in the regime it is named for.
"""
import contextlib

import numpy as np

IMAGES = {'wide': (256, 512, 0), 'small': (64, 64, 0)}
ROI_CAPACITY = 1000          # config.test.rpn_post_nms_top_n of CITYSCAPES_R50: rows of the padded ROI buffer
DEFAULT_MAX_DET = 100
NEVER = 2.0                  # a score threshold no probability exceeds


def _things(c):
    return len(c['classes']) == c['n_inst'] and all(k >= 1 for k in c['classes'])


def _dummy_pan(c):
    return c['n_pan'] == 1 and c['n_inst'] == 1 and c['classes'] == [0]


REGIMES = {
    # the regime of every other whole-model test: both selections real, the panoptic one below every cap
    'default': dict(image='wide', test={}, mask_bias=None,
                    is_regime=lambda c, max_det: 2 <= c['n_det'] <= max_det and 2 <= c['n_pan'] < max_det and c['n_inst'] >= 2 and _things(c)),
    # no detection on either side: both selections return the reference's dummy (mask_roi.py:135-141)
    'none': dict(image='wide', test=dict(score_thresh=NEVER, panoptic_score_thresh=NEVER), mask_bias=None,
                 is_regime=lambda c, max_det: c['n_det'] == 1 and _dummy_pan(c)),
    # per-class detections, panoptic dummy: mask_removal.py:55-57
    'det-only': dict(image='wide', test=dict(panoptic_score_thresh=NEVER), mask_bias=None,
                     is_regime=lambda c, max_det: c['n_det'] >= 2 and _dummy_pan(c)),
    # per-class dummy, real panoptic detections: every panoptic row is an "extra" row of the mask head
    'pan-only': dict(image='wide', test=dict(score_thresh=NEVER), mask_bias=None,
                     is_regime=lambda c, max_det: c['n_det'] == 1 and c['n_pan'] >= 2 and c['n_inst'] >= 2 and _things(c)),
    # one panoptic row that is NOT the dummy; panoptic_score_thresh = ONE (below), from the default run's scores
    'one': dict(image='wide', test=dict(panoptic_score_thresh='ONE'), mask_bias=None,
                is_regime=lambda c, max_det: c['n_det'] >= 2 and c['n_pan'] == 1 and c['n_inst'] == 1 and c['classes'][0] >= 1),
    # both selections cut at max_det
    'saturated': dict(image='wide', test=dict(score_thresh=0.0, panoptic_score_thresh=0.0), mask_bias=None,
                      is_regime=lambda c, max_det: c['n_det'] == max_det == DEFAULT_MAX_DET and c['n_pan'] == max_det and c['n_inst'] >= 2 and _things(c)),
    # more panoptic rows than the fused kernels' instance table: the materialising head
    'over-256': dict(image='wide', test=dict(score_thresh=0.0, panoptic_score_thresh=0.0, max_det=400), mask_bias=None,
                     is_regime=lambda c, max_det: c['n_det'] > 256 and 256 < c['n_pan'] <= max_det and c['n_inst'] >= 2 and _things(c)),
    # every mask logit negative: no panoptic row survives mask removal, row 0 is kept without an instance pixel (mask_removal.py:90-92)
    'nothing-kept': dict(image='wide', test={}, mask_bias=-50.0,
                         is_regime=lambda c, max_det: c['n_pan'] >= 2 and c['n_inst'] == 1 and c['classes'][0] >= 1),
    # fewer proposals than the ROI buffer holds: a device count below the capacity
    'short': dict(image='small', test={}, mask_bias=None,
                  is_regime=lambda c, max_det: 1 <= c['n_rois'] < ROI_CAPACITY),
}
DUMMY_DET = ('none', 'pan-only')        # regimes whose per-class side is the dummy
DUMMY_PAN = ('none', 'det-only')        # regimes whose panoptic side is the dummy
NO_INSTANCE_PIXEL = ('none', 'det-only', 'nothing-kept')   # no label in [num_stuff, 255) in the panoptic map
TTA_REGIMES = ('none', 'pan-only', 'one', 'over-256')
NAMES = list(REGIMES)


def top_two_midpoint(pan_scores):
    """The 'one' regime's panoptic_score_thresh: the midpoint of the two largest panoptic scores of the default regime, as the float32
    the kernel and the oracle compare against (`score > thresh`). Fails loudly unless exactly one score exceeds it."""
    s = np.sort(np.asarray(pan_scores, np.float32).reshape(-1))[::-1]
    assert s.size >= 2, "the 'one' regime needs two panoptic detections in the default regime, got %d" % s.size
    mid = np.float32((np.float64(s[0]) + np.float64(s[1])) / 2)
    assert s[0] > mid >= s[1], "the two largest panoptic scores (%r, %r) leave no float32 threshold between them" % (s[0], s[1])
    return float(mid)


def thresholds(name, one=None):
    """The regime's knobs as check_taps(thresholds=...) / head_stage_cpu(thresholds=...) take them. one: top_two_midpoint(...)."""
    th = dict(REGIMES[name]['test'])
    if th.get('panoptic_score_thresh') == 'ONE':
        assert one is not None, "the 'one' regime takes its threshold from the default run: pass one=top_two_midpoint(pan_scores)"
        th['panoptic_score_thresh'] = float(one)
    return th


def max_det_of(name):
    return REGIMES[name]['test'].get('max_det', DEFAULT_MAX_DET)


def check_regime(name, counts):
    assert REGIMES[name]['is_regime'](counts, max_det_of(name)), "not the %r regime: %s" % (name, counts)


def counts_of(out):
    """dict(n_rois, n_det, n_pan, n_inst, classes) from oracle.forward.forward_cpu's result."""
    return dict(n_rois=int(out['n_rois']), n_det=int(out['n_det']), n_pan=int(out['pan_boxes'].shape[0]), n_inst=int(out['n_inst']),
                classes=[int(c) for c in out['panoptic_cls_inds']])


@contextlib.contextmanager
def regime(model, name, one=None):
    """Put `model` (product model on any device, or its CPU copy) and the configuration into the regime; everything is restored on
    exit, also after an exception.

    The thresholds are kernel arguments and max_det sizes the early mask head, all baked into a captured HIP graph, so the graphs are
    dropped on entry and on exit. mask_bias edits mask_branch.mask_score.bias in place: the packed weights of a layer are keyed on
    (data_ptr, _version, shape) of its weight and bias (ops.cached_pack), an in-place fill bumps _version, so the next launch re-packs
    and no pack cache has to be dropped by hand; the bias itself is handed to the kernels by address."""
    import torch
    from upsnet_amd.config.config import config
    spec = REGIMES[name]
    th = thresholds(name, one)
    saved_cfg = {k: config.test[k] for k in th}
    saved_mod = (model.mask_roi.score_thresh, model.mask_roi_panoptic.score_thresh, model.mask_roi.top_n, model.mask_roi_panoptic.top_n)
    bias = model.mask_branch.mask_score.bias
    saved_bias = bias.detach().clone() if spec['mask_bias'] is not None else None
    try:
        for k, v in th.items():
            config.test[k] = v
        model.mask_roi.score_thresh = config.test.score_thresh
        model.mask_roi_panoptic.score_thresh = config.test.panoptic_score_thresh
        model.mask_roi.top_n = model.mask_roi_panoptic.top_n = config.test.max_det
        if saved_bias is not None:
            with torch.no_grad():
                bias.fill_(spec['mask_bias'])
        model.invalidate_graphs()
        yield th
    finally:
        for k, v in saved_cfg.items():
            config.test[k] = v
        (model.mask_roi.score_thresh, model.mask_roi_panoptic.score_thresh, model.mask_roi.top_n, model.mask_roi_panoptic.top_n) = saved_mod
        if saved_bias is not None:
            with torch.no_grad():
                bias.copy_(saved_bias)
        model.invalidate_graphs()
