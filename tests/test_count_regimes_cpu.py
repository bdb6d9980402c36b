"""CPU: every case of tests/count_regimes.py is in the regime it is named for, judged by the oracle alone (oracle.forward.forward_cpu
on the unprepared seed-235 model) -- no GPU code runs here. The trunk and the box head are evaluated once per image; only the
selections, the mask head and the panoptic head are re-run per regime."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import count_regimes as cr  # noqa: E402


@pytest.fixture(scope='module')
def host():
    from upsnet_amd.config.config import update_config_dict, CITYSCAPES_R50
    update_config_dict(CITYSCAPES_R50)
    from oracle.forward import box_stage_cpu
    from upsnet_amd.synthetic import build_unprepared, make_image
    model = build_unprepared()
    model.eval()
    stages = {}

    def stage(image):
        if image not in stages:
            h, w, seed = cr.IMAGES[image]
            stages[image] = box_stage_cpu(model, make_image(h, w, seed=seed))
        return stages[image]
    return model, stage, {}


def _run(host, name):
    """head_stage_cpu's result of the regime (cached: 'one' needs the default regime's scores)."""
    from oracle.forward import head_stage_cpu
    model, stage, done = host
    if name not in done:
        one = cr.top_two_midpoint(_run(host, 'default')['pan_scores']) if name == 'one' else None
        with cr.regime(model, name, one=one) as th:
            # the oracle takes the knobs as an argument; the context manager is needed for the bias edit only
            done[name] = head_stage_cpu(model, stage(cr.REGIMES[name]['image']), thresholds=th)
    return done[name]


@pytest.mark.parametrize('name', cr.NAMES)
def test_the_oracle_is_in_the_regime(host, name):
    from upsnet_amd.config.config import config
    out = _run(host, name)
    counts = cr.counts_of(out)
    print(name, counts)
    cr.check_regime(name, counts)
    num_stuff = config.dataset.num_seg_classes - (config.dataset.num_classes - 1)
    pan = out['panoptic_outputs']
    if name in cr.DUMMY_DET:
        assert np.array_equal(out['cls_probs'], np.ones((1,), np.float32)) and np.array_equal(out['pred_boxes'], np.zeros((1, 5), np.float32))
        assert np.array_equal(out['cls_inds'], np.zeros((1,), np.int64)) and out['mask_probs'].shape == (1, config.dataset.num_classes, 28, 28)
    if name in cr.DUMMY_PAN:
        assert np.array_equal(out['pan_scores'], np.ones((1,), np.float32)) and np.array_equal(out['pan_boxes'], np.zeros((1, 5), np.float32))
        assert np.array_equal(out['panoptic_cls_inds'], np.zeros((1,), np.int64))
    inst_pixels = int(((pan >= num_stuff) & (pan != 255)).sum())
    if name in cr.NO_INSTANCE_PIXEL:
        assert inst_pixels == 0 and np.array_equal(out['keep_inds'], [0])
    elif name != 'short':
        assert inst_pixels > 0


def test_regime_restores_the_configuration_and_the_model(host):
    from upsnet_amd.config.config import config
    model = host[0]
    bias = model.mask_branch.mask_score.bias
    before = (config.test.score_thresh, config.test.panoptic_score_thresh, config.test.max_det, model.mask_roi.score_thresh,
              model.mask_roi_panoptic.score_thresh, bias.detach().clone())
    model._graphs['stale'] = None
    with pytest.raises(ZeroDivisionError):
        with cr.regime(model, 'over-256'):
            assert config.test.max_det == 400 and model.mask_roi.score_thresh == 0.0 and model.mask_roi_panoptic.score_thresh == 0.0
            assert model._graphs == {}
            1 / 0
    with cr.regime(model, 'nothing-kept'):
        assert float(bias.detach().max()) == -50.0
    with cr.regime(model, 'one', one=0.75) as th:
        assert th == {'panoptic_score_thresh': 0.75} and model.mask_roi_panoptic.score_thresh == 0.75
    after = (config.test.score_thresh, config.test.panoptic_score_thresh, config.test.max_det, model.mask_roi.score_thresh,
             model.mask_roi_panoptic.score_thresh)
    assert after == before[:5] and torch.equal(bias, before[5])


def test_top_two_midpoint_fails_loudly_on_a_tie():
    assert cr.top_two_midpoint([0.5, 0.75, 0.25]) == 0.625
    with pytest.raises(AssertionError):
        cr.top_two_midpoint([0.75, 0.75, 0.25])
    with pytest.raises(AssertionError):
        cr.top_two_midpoint([0.75])


def test_check_taps_thresholds_argument_rejects_unknown_keys():
    from oracle.forward import _thresholds
    from upsnet_amd.config.config import config
    assert _thresholds(None) == {'score_thresh': config.test.score_thresh, 'panoptic_score_thresh': config.test.panoptic_score_thresh,
                                 'max_det': config.test.max_det}
    assert _thresholds({'max_det': 400})['max_det'] == 400
    with pytest.raises(KeyError):
        _thresholds({'nms_thresh': 0.3})
