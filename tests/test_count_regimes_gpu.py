"""GPU: the whole forward at the detection-count extremes of tests/count_regimes.py, against the oracle.

The whole-model tests elsewhere run one regime. Here every regime runs through both pipelines stage-wise against the oracle
(oracle.forward.check_taps), through the HIP-graph path (in-graph fixed-capacity tail or eager continuation, whichever the counters
select), through evaluate.post_image and through test-time augmentation. Every comparison is bit-exact; each regime's predicate is a
hard assertion on the counts of that very run, so a test cannot pass by running the default regime."""
import copy
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import count_regimes as cr  # noqa: E402

pytestmark = pytest.mark.gpu

KEYS = ('panoptic_outputs', 'pred_boxes', 'cls_probs', 'cls_inds', 'mask_probs', 'panoptic_cls_inds', 'fcn_outputs')
OUT_KEYS = KEYS + ('panoptic_cls_probs',)


def _bits(a, b):
    """same shape, dtype and bits (NaN-safe, layout-free)."""
    a, b = a.contiguous(), b.contiguous()
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(torch.uint8), b.view(torch.uint8))


def _same(got, want, keys, what):
    for k in keys:
        assert _bits(got[k], want[k]), (what, k, tuple(got[k].shape), tuple(want[k].shape))


class Ctx(object):
    def __init__(self, model, make_image):
        self.model = model
        self.images = {k: make_image(h, w, seed=s, device='cuda') for k, (h, w, s) in cr.IMAGES.items()}
        self.runs = {}

    def image(self, name):
        return self.images[cr.REGIMES[name]['image']]

    def one(self, name):
        """The 'one' regime's threshold from the DEVICE's default-regime panoptic scores."""
        return cr.top_two_midpoint(self.eager('default')['fused'][1]['pan_scores'].cpu().numpy()) if name == 'one' else None

    def regime(self, name):
        return cr.regime(self.model, name, one=self.one(name))

    def eager(self, name):
        """{'fused' / 'modules': (out, taps)} of one eager forward per pipeline inside the regime, and 'th' (its knobs); computed once."""
        if name not in self.runs:
            model, res = self.model, {}
            with self.regime(name) as th, torch.no_grad():
                res['th'] = dict(th)
                for pipeline in ('fused', 'modules'):
                    model.pipeline, model.taps = pipeline, {}
                    try:
                        out = model(self.image(name))
                        res[pipeline] = ({k: v.clone() for k, v in out.items()}, model.taps)
                    finally:
                        model.pipeline, model.taps = 'fused', None
            self.runs[name] = res
        return self.runs[name]


@pytest.fixture(scope='module')
def ctx():
    from upsnet_amd.config.config import update_config_dict, CITYSCAPES_R50
    update_config_dict(CITYSCAPES_R50)
    from upsnet_amd.synthetic import build_model, make_image
    c = Ctx(build_model(), make_image)
    yield c
    c.model.invalidate_graphs()
    c.runs.clear()
    torch.cuda.empty_cache()


@pytest.mark.parametrize('name', cr.NAMES)
def test_stagewise_parity_in_both_pipelines(ctx, name):
    """Every custom-op stage of both pipelines == the oracle on the recorded inputs, the label map included; the two pipelines' output
    dicts are bit-equal; the run is in the regime it is named for."""
    from oracle.forward import check_taps
    from upsnet_amd.config.config import config
    run = ctx.eager(name)
    for pipeline in ('fused', 'modules'):
        out, taps = run[pipeline]
        res = check_taps(taps, enable_void=ctx.model.enable_void, thresholds=run['th'])
        counts = res.pop('counts')
        print('%s / %s: %s' % (name, pipeline, {k: v for k, v in counts.items() if k != 'classes'}), 'classes', sorted(set(counts['classes'])))
        assert all(res.values()), (name, pipeline, res, counts)
        assert counts['label_mismatch'] == 0, (name, pipeline, counts)
        cr.check_regime(name, counts)
        # the output dict is the recorded stages
        assert out['cls_inds'].numel() == counts['n_det'] and out['panoptic_cls_inds'].numel() == counts['n_inst']
        assert _bits(out['pred_boxes'], taps['det_boxes']) and _bits(out['panoptic_outputs'], taps['panoptic'])
        assert _bits(out['panoptic_cls_inds'], taps['pan_cls'][taps['keep']]) and _bits(out['panoptic_cls_probs'], taps['pan_scores'][taps['keep']])
        assert out['panoptic_cls_inds'].tolist() == counts['classes']
        num_stuff = config.dataset.num_seg_classes - (config.dataset.num_classes - 1)
        pan = out['panoptic_outputs']
        inst_pixels = int(((pan >= num_stuff) & (pan != 255)).sum())
        if name in cr.NO_INSTANCE_PIXEL:
            assert inst_pixels == 0 and taps['keep'].tolist() == [0], (name, inst_pixels, taps['keep'].tolist())
        elif name != 'short':
            assert inst_pixels > 0
    assert set(run['fused'][0]) == set(run['modules'][0]) == set(OUT_KEYS)
    _same(run['fused'][0], run['modules'][0], OUT_KEYS, name)


@pytest.mark.parametrize('name', cr.NAMES)
def test_mask_logits_are_those_of_a_separate_pass(ctx, name):
    """What check_taps takes as given: the panoptic mask logits (early mask head on the padded per-class rows, reused through pan_row /
    mask_roi_dedup, extra rows, the dummy's zero box, the 400-row batch) == a mask-head pass of their own over the panoptic boxes
    gathered at the panoptic classes, and mask_probs == sigmoid of a pass over the per-class boxes."""
    from upsnet_amd.config.config import config
    model = ctx.model
    out, taps = ctx.eager(name)['fused']
    ms = config.network.mask_size
    with ctx.regime(name), torch.no_grad():      # (nothing-kept: the pass of its own needs the regime's bias)
        pan = model.mask_branch(taps['feats'], taps['pan_boxes'])
        det = model.mask_branch(taps['feats'], taps['det_boxes'])
    want = pan.gather(1, taps['pan_cls'].view(-1, 1, 1, 1).expand(-1, -1, ms, ms))
    assert taps['pan_logit'].shape == (taps['pan_boxes'].shape[0], 1, ms, ms)
    assert _bits(taps['pan_logit'], want), name
    assert _bits(out['mask_probs'], torch.sigmoid(det)), name
    _, taps_m = ctx.eager(name)['modules']
    assert _bits(taps_m['pan_logit'], want), name


@pytest.mark.parametrize('name', sorted(set(cr.DUMMY_DET + cr.DUMMY_PAN)))
def test_dummy_detection_contract(ctx, name):
    """The reference's dummy (mask_roi.py:135-141): scores [1.], a zero [1,5] box, class [0]; mask_probs [1,C,28,28]; the dtypes of the
    default regime."""
    from upsnet_amd.config.config import config
    default = ctx.eager('default')['fused'][0]
    for pipeline in ('fused', 'modules'):
        out, taps = ctx.eager(name)[pipeline]
        for k in OUT_KEYS:
            assert out[k].dtype == default[k].dtype and out[k].dim() == default[k].dim(), (name, pipeline, k, out[k].dtype, out[k].shape)
        if name in cr.DUMMY_DET:
            assert out['cls_probs'].tolist() == [1.0] and out['cls_inds'].tolist() == [0]
            assert tuple(out['pred_boxes'].shape) == (1, 5) and not out['pred_boxes'].any()
            assert tuple(out['mask_probs'].shape) == (1, config.dataset.num_classes, 28, 28)
        if name in cr.DUMMY_PAN:
            assert taps['pan_scores'].tolist() == [1.0] and taps['pan_cls'].tolist() == [0]
            assert tuple(taps['pan_boxes'].shape) == (1, 5) and not taps['pan_boxes'].any()
            assert out['panoptic_cls_inds'].tolist() == [0] and out['panoptic_cls_probs'].tolist() == [1.0]


@pytest.mark.parametrize('name', cr.NAMES)
def test_graph_replay_equals_eager(ctx, name):
    """HIP-graph path in the regime, one and two graph instances, synchronous and forward_async: every output (the seven keys of
    test_model_gpu.py::test_hip_graph_replay_equals_eager and the kept rows' scores, which unlike their classes are all distinct) == the
    eager forward (itself == the oracle, test_stagewise_parity_in_both_pipelines). The slot's counters say which continuation served
    it. A second image of the shape (other counts wherever the knobs leave any) then goes through the same captured instances and
    back, so a row that one replay leaves behind shows in the next. Afterwards the default regime replays on the same model with
    nothing of the extreme regime left."""
    from upsnet_amd.synthetic import make_image
    model = ctx.model
    want = ctx.eager(name)['fused'][0]
    img = ctx.image(name)
    h, w, seed = cr.IMAGES[cr.REGIMES[name]['image']]
    other = make_image(h, w, seed=seed + 7, device='cuda')
    was = (model.use_graph, model.graph_slots)
    try:
        with ctx.regime(name), torch.no_grad():
            model.use_graph = False
            want_other = {k: v.clone() for k, v in model(other).items()}
            model.use_graph = True
            for slots in (1, 2):
                model.invalidate_graphs()
                model.graph_slots = slots
                for step in range(5):
                    _same(model(img), want, OUT_KEYS, (name, slots, step))
                for step in range(3):
                    _same(model.forward_async(img).result(), want, OUT_KEYS, (name, slots, 'async', step))
                ents = [e for sl in model._graphs.values() for e in sl['slots']]
                assert len(ents) == slots and all('graph' in e for e in ents), (name, slots, [sorted(e) for e in ents])
                for e in ents:
                    torch.cuda.synchronize()
                    n_det, n_pan, n_extra, k = e['out']['tail']['counters'].tolist()
                    max_det = e['out']['max_det']
                    assert max_det == cr.max_det_of(name)
                    in_graph = n_extra == 0 and n_det <= max_det and n_pan <= 256
                    print('%s, %d graph instance(s), instance %d: n_det %d n_pan %d n_extra %d k %d -> %s'
                          % (name, slots, e['idx'], n_det, n_pan, n_extra, k, 'in-graph tail' if in_graph else 'eager continuation'))
                    assert (n_det, n_pan) == (want['cls_inds'].numel(), ctx.eager(name)['fused'][1]['pan_cls'].numel())
                    if name == 'pan-only':
                        assert n_extra == n_pan > 0, (n_det, n_pan, n_extra)
                    if name == 'over-256':
                        assert n_pan > 256, (n_det, n_pan, n_extra)
                    if name in ('none', 'one'):
                        # no extra row by construction (dummy == dummy; the best panoptic row is a per-class detection): in-graph tail
                        assert in_graph and k == 1, (n_det, n_pan, n_extra, k)
                for step, j in enumerate((1, 0, 1, 1, 0)):
                    _same(model(other if j else img), want_other if j else want, OUT_KEYS, (name, slots, 'two images', step))
        # (the context has dropped the regime's graphs) the default regime on the same model
        default = ctx.eager('default')['fused'][0]
        with torch.no_grad():
            model.graph_slots = 1
            for step in range(4):    # eager, eager, capture + replay, replay
                _same(model(ctx.image('default')), default, OUT_KEYS, (name, 'default afterwards', step))
            ent, = [e for sl in model._graphs.values() for e in sl['slots']]
            assert 'graph' in ent
    finally:
        model.use_graph, model.graph_slots = was
        model.invalidate_graphs()


@pytest.mark.parametrize('name', cr.NAMES)
def test_after_the_network(ctx, name):
    """evaluate.post_image on the regime's outputs: per-class [box | score] arrays and RLE strings == the oracle's im_post / rle_counts
    / rle_to_string on the same detections (for the dummy: an empty (0, 5) array and an empty list for every class, as in
    upsnet_end2end_test.py:109-152); get_unified_pan_result on the restored maps == the oracle's."""
    from oracle import ops as oops
    from upsnet_amd.config.config import config
    from upsnet_amd.dataset.base_dataset import BaseDataset
    from upsnet_amd.evaluate import post_image
    out = ctx.eager(name)['fused'][0]
    h, w, _ = cr.IMAGES[cr.REGIMES[name]['image']]
    C, S = config.dataset.num_classes, config.dataset.num_seg_classes
    all_boxes, all_masks = [[] for _ in range(C)], [[] for _ in range(C)]
    ssegs, panos, pano_cls = [], [], []
    post_image(out, np.array([h, w, 1.0], np.float32), C, all_boxes, all_masks, ssegs, panos, pano_cls)
    boxes = out['pred_boxes'][:, 1:].cpu().numpy() / np.float32(1.0)
    scores, cls = out['cls_probs'].cpu().numpy(), out['cls_inds'].cpu().numpy()
    ref = oops.im_post(boxes, out['mask_probs'].cpu().numpy(), cls, h, w)
    assert all_boxes[0] == [] and all_masks[0] == []
    seen = 0
    for idx in range(1, C):
        sel = np.nonzero(cls == idx)[0]
        assert len(all_boxes[idx]) == 1 and len(all_masks[idx]) == 1
        got = all_boxes[idx][0]
        assert got.shape == (len(sel), 5) and got.dtype == np.float32
        np.testing.assert_array_equal(got, np.hstack([boxes[sel], scores[sel].reshape(-1, 1)]))
        assert len(all_masks[idx][0]) == len(sel)
        for d, seg in zip(sel, all_masks[idx][0]):
            assert seg['size'] == [h, w] and seg['counts'] == oops.rle_to_string(oops.rle_counts(ref[d])), (name, idx, d)
            seen += 1
    if name in cr.DUMMY_DET:
        assert seen == 0 and all(len(all_masks[idx][0]) == 0 for idx in range(1, C))
    else:
        assert seen == cls.size
    # the restored maps (scale 1: the unpadded region) and the panoptic result built from them
    assert len(ssegs) == len(panos) == len(pano_cls) == 1
    np.testing.assert_array_equal(ssegs[0], out['fcn_outputs'][0, :h, :w].cpu().numpy().astype(ssegs[0].dtype))
    np.testing.assert_array_equal(panos[0], out['panoptic_outputs'][0, :h, :w].cpu().numpy().astype(panos[0].dtype))
    np.testing.assert_array_equal(pano_cls[0], out['panoptic_cls_inds'].cpu().numpy())
    for limit in (4 * 64 * 64, 50):
        got = BaseDataset().get_unified_pan_result(ssegs, panos, pano_cls, stuff_area_limit=limit)[0].cpu().numpy()
        np.testing.assert_array_equal(got, oops.get_unified_pan_result(ssegs[0], panos[0], pano_cls[0], S, C, limit))


# ------------------------------------------------------------------------------------------------ test-time augmentation
@pytest.fixture(scope='module')
def tta_model():
    """The model of tests/test_tta_gpu.py: base augmentation only, scale 256 / max size 512 (a 256 x 512 image keeps its size)."""
    from upsnet_amd.config.config import config, update_config_dict, CITYSCAPES_R50
    from upsnet_amd.synthetic import build_model
    saved = copy.deepcopy(dict(config))
    update_config_dict(CITYSCAPES_R50)
    update_config_dict(dict(test=dict(scales=[256], max_size=512, aug_scales=[], aug_flip=False)))
    model = build_model(device='cuda')
    model.use_graph = False
    yield model
    del model
    config.clear()
    config.update(saved)
    torch.cuda.empty_cache()


@pytest.mark.parametrize('name', cr.TTA_REGIMES)
def test_tta_base_augmentation_equals_the_plain_forward(tta_model, name):
    """tta.forward_tta holds a copy of the eager continuation: with the base augmentation alone it must equal the plain forward on
    every key in the regimes that take its other branches (dummy on both sides, extra rows only, a single row, the materialising
    head)."""
    from oracle.forward import check_taps
    from upsnet_amd.dataset.blob import get_image_blob
    from upsnet_amd.synthetic import make_image_u8
    from upsnet_amd.tta import augmentation_list
    assert augmentation_list() == [(256, 512, False)]
    h, w, seed = cr.IMAGES['wide']
    img = make_image_u8(h, w, seed=seed, device='cuda')
    blob = get_image_blob(img)
    data = {'data': blob['data'], 'im_info': blob['im_info']}
    assert tuple(np.asarray(data['im_info']).reshape(-1)[:3]) == (float(h), float(w), 1.0)
    one = None
    with torch.no_grad():
        if name == 'one':
            tta_model.taps = {}
            try:
                tta_model(data)
                one = cr.top_two_midpoint(tta_model.taps['pan_scores'].cpu().numpy())
            finally:
                tta_model.taps = None
        with cr.regime(tta_model, name, one=one) as th:
            tta_model.taps = {}
            try:
                want = tta_model(data)
                taps = tta_model.taps
            finally:
                tta_model.taps = None
            got = tta_model.forward_tta(img)
    res = check_taps(taps, enable_void=tta_model.enable_void, thresholds=th)
    counts = res.pop('counts')
    assert all(res.values()) and counts['label_mismatch'] == 0, (name, res, counts)
    cr.check_regime(name, counts)
    assert set(got) == set(want)
    _same(got, want, sorted(want), name)
