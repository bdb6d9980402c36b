"""CPU: the seed-independent classifier gain of the synthetic model (oracle.draws.fit_cls_gain) the multi-draw parity tests build
their networks with: deterministic, finite, inside the range the rule states, and on seed 235 the gain DEFAULT_CLS_GAIN was
hand-fitted to."""
import math

import pytest
import torch


@pytest.mark.parametrize("preset", ["CITYSCAPES_R50", "COCO_R101_DCN"])
def test_fit_cls_gain_is_deterministic_finite_and_in_range(preset):
    from upsnet_amd.config import config as cfgmod
    from upsnet_amd.config.config import update_config_dict, CITYSCAPES_R50, config
    from upsnet_amd import synthetic
    from oracle import draws
    update_config_dict(getattr(cfgmod, preset))
    try:
        seed = draws.DRAWS[0][0]
        a = synthetic.build_unprepared(seed=seed, cls_gain=draws.fit_cls_gain)
        b = synthetic.build_unprepared(seed=seed, cls_gain=draws.fit_cls_gain)
        assert isinstance(a.cls_gain, float) and math.isfinite(a.cls_gain) and a.cls_gain == b.cls_gain
        lo, hi = draws.FIT_GAIN_RANGE
        # strictly inside: a result at the upper end would mean the share is not reachable (the rule's fallback), not a fit
        assert lo <= a.cls_gain < hi, a.cls_gain
        sa, sb = a.state_dict(), b.state_dict()
        assert sa.keys() == sb.keys() and all(torch.equal(sa[k], sb[k]) for k in sa)
        # the scaled classifier is the unscaled one times the gain
        raw = synthetic.build_unprepared(seed=seed, cls_gain=None)
        assert torch.equal(sa['rcnn.cls_score.weight'], raw.state_dict()['rcnn.cls_score.weight'] * a.cls_gain)
        # the rule reproduces the hand-fitted gain of seed 235 (tools/calib_gain_cpu.py) to within 2 %
        ref = synthetic.build_unprepared(seed=235, cls_gain=draws.fit_cls_gain).cls_gain
        default = synthetic.DEFAULT_CLS_GAIN[config.dataset.num_classes]
        assert abs(ref / default - 1.0) < 0.02, (ref, default)
    finally:
        update_config_dict(CITYSCAPES_R50)
