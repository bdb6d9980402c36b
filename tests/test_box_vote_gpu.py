"""GPU: box voting (csrc/box_vote.hip). ops.box_vote against the numpy restatement of the rule (tests/box_vote_ref.py),
bit for bit, on poisoned and guard-banded memory (tests/memguard.py, patterns A and B); the voted augmented forward against the
restatement applied to its own parts; the evaluation run with --bbox_vote."""
import copy
import os
import pickle
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import memguard       # noqa: E402
import box_vote_ref as ref   # noqa: E402

pytestmark = pytest.mark.gpu

F = np.float32
GUARDED = memguard.MODULES + ('upsnet_amd.tta',)


def dev(x):
    return torch.from_numpy(np.array(x, order='C', copy=True)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def bits_equal(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def both_patterns(run):
    """run(pattern) under poisoned allocations and checked guard bands, once per pattern; the results must agree bitwise."""
    res = []
    for pattern in 'AB':
        with memguard.poisoned(pattern, modules=GUARDED):
            out = run(pattern)
            torch.cuda.synchronize()
        res.append(np.ascontiguousarray(host(out)))
    assert bits_equal(res[0], res[1]), 'result depends on the poison pattern'
    return res[0]


def device_vote(case, n, clip, thr, num=None, score_thresh=0.05):
    """ops.box_vote on banded copies of the case's tensors, under both poison patterns."""
    from upsnet_amd import ops

    def run(p):
        b = lambda x: memguard.banded_copy(dev(x), p)
        nd = b(np.array([n], np.int32))
        kd = b(np.array([case['num'] if num is None else num], np.int32))
        return ops.box_vote(b(case['rois']), b(case['delta']), b(case['prob']), b(ref.IM_INFO), b(case['boxes']), b(case['cls']), kd,
                            score_thresh, thr, ref.REG_WEIGHTS, num_rois_dev=nd, clip_boxes=clip)
    return both_patterns(run)


def ref_vote(case, n, clip, thr, num=None, score_thresh=0.05):
    return ref.box_vote(case['rois'], case['delta'], case['prob'], n, ref.IM_INFO, ref.REG_WEIGHTS, clip, case['boxes'], case['cls'],
                        case['num'] if num is None else num, score_thresh, thr, want_counts=True)


# ------------------------------------------------------------------------------------------------ the kernel against the rule
@pytest.mark.parametrize('C', [2, 9, 81])
@pytest.mark.parametrize('N', [1, 63, 64, 65, 200, 1000])
def test_box_vote_equals_the_restatement(N, C):
    """Kept rows 0, 1, 5, 100 with cap = kept + 37, a device row count below N (rows past it are good candidates that must not vote),
    clip on and off, IoU thresholds 0.5 and 0.8. At N = 1 there is one candidate row, so no kept row can have two voters; from N = 63
    on at least half the kept rows have two or more, and from N = 200 on one kept row has more than 128 (170 rows share a cluster)."""
    rng = np.random.default_rng(1000 * N + C)
    n = N if N == 1 else N - 7
    for i, kept in enumerate((0, 1, 5, 100)):
        for clip, thr in (((True, 0.5), (False, 0.8)) if i % 2 == 0 else ((True, 0.8), (False, 0.5))):
            case = ref.cluster_case(rng, N, C, kept, clip=clip, big=170 if N >= 200 else 0)
            want, counts = ref_vote(case, n, clip, thr)
            got = device_vote(case, n, clip, thr)
            assert got.shape == (kept + 37, 5) and got.dtype == np.float32
            assert bits_equal(got, want), (kept, clip, thr, counts)
            assert bits_equal(got[kept:], case['boxes'][kept:])
            if N == 1:
                assert all(c <= 1 for c in counts)
            elif kept:
                assert sum(c >= 2 for c in counts) * 2 >= kept, counts
                assert not bits_equal(got[:kept], case['boxes'][:kept])
            if N >= 200 and kept:
                assert counts[0] > 128, counts[0]


def test_nothing_above_the_score_threshold_moves_nothing():
    rng = np.random.default_rng(7)
    case = ref.cluster_case(rng, 200, 9, 20, big=170, low_prob=True)
    want, counts = ref_vote(case, 200, True, 0.5)
    assert counts == [0] * 20 and bits_equal(want, case['boxes'])
    assert bits_equal(device_vote(case, 200, True, 0.5), case['boxes'])
    # ... and the same rows vote once the threshold is below their probabilities
    want, counts = ref_vote(case, 200, True, 0.5, score_thresh=0.01)
    assert max(counts) > 64
    assert bits_equal(device_vote(case, 200, True, 0.5, score_thresh=0.01), want)


@pytest.mark.parametrize('num', [-1, 1000])
def test_overflow_marker_copies_every_row_and_a_count_past_the_capacity_is_clamped(num):
    rng = np.random.default_rng(8)
    case = ref.cluster_case(rng, 200, 9, 20, big=170, pad=0)
    want, _ = ref_vote(case, 200, True, 0.5, num=num)
    got = device_vote(case, 200, True, 0.5, num=num)
    assert bits_equal(got, want)
    assert bits_equal(got, case['boxes']) == (num < 0)


def test_iou_threshold_above_one_returns_the_input():
    rng = np.random.default_rng(9)
    case = ref.cluster_case(rng, 200, 9, 20, big=170)
    assert bits_equal(device_vote(case, 200, True, 1.5), case['boxes'])


def test_out_of_range_classes_and_row_counts_are_clamped():
    rng = np.random.default_rng(10)
    case = ref.cluster_case(rng, 65, 9, 5)
    case['cls'][1], case['cls'][3] = -4, 4000
    for n in (-3, 65 + 1000):
        want, _ = ref_vote(case, n, True, 0.5)
        assert bits_equal(device_vote(case, n, True, 0.5), want)


def test_same_source_and_class_gives_the_same_bits_in_two_kept_lists():
    """What keeps ops.mask_roi_dedup valid: it pairs rows of the two selections by (source ROI, class), and such rows get the same
    voted box whatever list, position and capacity they come in."""
    rng = np.random.default_rng(11)
    case = ref.cluster_case(rng, 300, 9, 30, big=170)
    a = device_vote(case, 300, True, 0.8)
    order = rng.permutation(30)[:11]
    other = dict(case, boxes=np.concatenate([case['boxes'][order], np.zeros((300, 5), F)]),
                 cls=np.concatenate([case['cls'][order], np.zeros(300, np.int64)]), num=11)
    b = device_vote(other, 300, True, 0.8)
    assert bits_equal(b[:11], a[order]) and not bits_equal(a[order], case['boxes'][order])


def test_wrapper_refuses_bad_arguments():
    from upsnet_amd import ops
    rng = np.random.default_rng(12)
    case = ref.cluster_case(rng, 20, 3, 2)
    t = {k: dev(v) for k, v in case.items() if k != 'num'}
    num, im = torch.tensor([2], dtype=torch.int32, device='cuda'), dev(ref.IM_INFO)
    args = lambda **kw: [kw.get(k, t[k]) for k in ('rois', 'delta', 'prob')] + [im] + [kw.get(k, t[k]) for k in ('boxes', 'cls')]
    with pytest.raises(RuntimeError, match='IoU threshold'):
        ops.box_vote(*args(), num, 0.05, 0.0, ref.REG_WEIGHTS)
    with pytest.raises(ValueError):
        ops.box_vote(*args(delta=t['delta'][:, :4]), num, 0.05, 0.5, ref.REG_WEIGHTS)
    with pytest.raises(ValueError):
        ops.box_vote(*args(cls=t['cls'].int()), num, 0.05, 0.5, ref.REG_WEIGHTS)
    with pytest.raises(ValueError):
        ops.box_vote(*args(), num.long(), 0.05, 0.5, ref.REG_WEIGHTS)
    with pytest.raises(Exception):
        ops.box_vote(*args(rois=t['rois'].cpu()), num, 0.05, 0.5, ref.REG_WEIGHTS)
    empty = ops.box_vote(*args(boxes=t['boxes'][:0], cls=t['cls'][:0]), num, 0.05, 0.5, ref.REG_WEIGHTS)
    assert tuple(empty.shape) == (0, 5)


# ------------------------------------------------------------------------------------------------ the model
IMAGE_HW = (250, 470)       # under scales 256 / max size 512: resized 256 x 481 (padded to 512), im_scale 1.024
# The synthetic weights' box head gives the candidates of one object little overlap. Measured on this model and image: at the default
# 0.8 no kept row of the base augmentation alone has a second voter (8 of 100 with the three augmentations); at 0.5, 85 and 91 of
# the 100 class-wise rows have two or more (at most 10 and 24). So the model tests vote at IoU >= 0.5, and assert that boxes move.
MODEL_VOTE_THRESH = 0.5


@pytest.fixture(scope='module')
def vote_model():
    from upsnet_amd.config.config import config, update_config_dict, CITYSCAPES_R50
    from upsnet_amd.synthetic import build_model
    saved = copy.deepcopy(dict(config))
    update_config_dict(CITYSCAPES_R50)
    update_config_dict(dict(test=dict(scales=[256], max_size=512, aug_scales=[], aug_flip=False, bbox_vote=False,
                                      bbox_vote_thresh=MODEL_VOTE_THRESH)))
    model = build_model(device='cuda')
    yield model
    del model
    config.clear()
    config.update(saved)
    torch.cuda.empty_cache()


AUG_LISTS = {'base': [(256, 512, False)], 'three': [(256, 512, False), (256, 512, True), (192, 384, False)]}


def _voted_by_the_rule(parts, which, clip):
    from upsnet_amd.config.config import config
    st, it = parts['bbox_vote']
    pre, cls = host(parts[which + '_boxes_prevote']), host(parts[which + '_cls'])
    return ref.box_vote(host(parts['merged_rois']), host(parts['merged_delta']), host(parts['merged_prob']),
                        int(parts['merged_n_rois'].item()), parts['im_info'][0], config.network.bbox_reg_weights, clip, pre, cls,
                        pre.shape[0], st, it, want_counts=True)


@pytest.mark.parametrize('augs', ['base', 'three'])
def test_voted_forward_equals_the_restatement_on_its_parts(vote_model, monkeypatch, augs):
    from upsnet_amd import ops, tta
    from upsnet_amd.config.config import config
    from upsnet_amd.synthetic import make_image_u8
    monkeypatch.setattr(tta, 'augmentation_list', lambda cfg=None: list(AUG_LISTS[augs]))
    img = make_image_u8(*IMAGE_HW, seed=5, device='cuda')

    # voting off: not one voting launch, the parts carry the selections' own boxes, and (base augmentation alone) the plain forward
    monkeypatch.setitem(config.test, 'bbox_vote', False)
    calls = []
    real = ops.box_vote
    monkeypatch.setattr(ops, 'box_vote', lambda *a, **kw: calls.append(1) or real(*a, **kw))
    off, off_parts = vote_model.forward_tta(img, return_parts=True)
    assert not calls and off_parts['bbox_vote'] is None
    assert memguard.bit_equal(off_parts['det_boxes'], off_parts['det_boxes_prevote'])
    assert memguard.bit_equal(off_parts['pan_boxes'], off_parts['pan_boxes_prevote'])
    if augs == 'base':
        from upsnet_amd.dataset.blob import get_image_blob
        data = get_image_blob(img)
        with torch.no_grad():
            plain = vote_model({'data': data['data'], 'im_info': data['im_info']})
        assert set(off) == set(plain)
        for k in plain:
            assert memguard.bit_equal(off[k].contiguous(), plain[k].contiguous()), k

    # voting on
    monkeypatch.setitem(config.test, 'bbox_vote', True)
    with memguard.poisoned('A', modules=GUARDED):
        out, parts = vote_model.forward_tta(img, return_parts=True)
        torch.cuda.synchronize()
    assert len(calls) == 2
    assert parts['bbox_vote'] == (float(config.test.score_thresh), MODEL_VOTE_THRESH)
    n_det, n_pan, n_extra = parts['n_det'], parts['n_pan'], parts['n_extra']
    assert n_det > 0 and n_pan > 0
    # the selections themselves are what they were without voting
    assert (n_det, n_pan, n_extra) == (off_parts['n_det'], off_parts['n_pan'], off_parts['n_extra'])
    for k in ('det_boxes_prevote', 'pan_boxes_prevote', 'det_scores', 'det_cls', 'pan_scores', 'pan_cls'):
        assert memguard.bit_equal(parts[k], off_parts[k]), k
    assert memguard.bit_equal(parts['pan_row'][:n_pan], off_parts['pan_row'][:n_pan])
    # 1. both kept lists are the rule applied to the selections' boxes and the merged union (test.score_thresh for both)
    want_det, det_counts = _voted_by_the_rule(parts, 'det', bool(vote_model.mask_roi.clip_boxes))
    want_pan, pan_counts = _voted_by_the_rule(parts, 'pan', bool(vote_model.mask_roi_panoptic.clip_boxes))
    assert bits_equal(host(parts['det_boxes']), want_det) and bits_equal(host(parts['pan_boxes']), want_pan)
    assert max(det_counts) >= 2, det_counts
    # 2. the mask head's rows: the voted detections, then the voted panoptic rows the dedup did not pair; paired rows carry equal boxes
    boxes, pan_row = host(parts['boxes']), host(parts['pan_row'])[:n_pan]
    assert boxes.shape == (n_det + n_extra, 5)
    assert bits_equal(boxes[:n_det], want_det) and bits_equal(boxes[pan_row], want_pan)
    # 3. the outputs are the tail on the merged tensors and the voted boxes
    with torch.no_grad():
        want_out = tta._tail(vote_model, parts['merged_score'], parts['cell'] == 4, parts['merged_mask_logits'], n_det, n_pan,
                             parts['det_boxes'], parts['det_scores'], parts['det_cls'], parts['pan_boxes'], parts['pan_scores'],
                             parts['pan_cls'], parts['pan_row'])
    assert set(out) == set(want_out) == set(off)
    for k in out:
        assert memguard.bit_equal(out[k].contiguous(), want_out[k].contiguous()), k
    assert bits_equal(host(out['pred_boxes']), want_det)
    # 4. voting moved at least one detection; scores, classes and order did not change
    assert out['pred_boxes'].shape == off['pred_boxes'].shape
    moved = (host(out['pred_boxes']) != host(off['pred_boxes'])).any(1)
    assert moved.any()
    assert memguard.bit_equal(out['cls_probs'], off['cls_probs']) and memguard.bit_equal(out['cls_inds'], off['cls_inds'])


# ------------------------------------------------------------------------------------------------ the evaluation run
def test_evaluate_main_with_box_voting(vote_model, tmp_path):
    from test_dataset_run_cpu import make_dataset, write_cfg
    from test_dataset_run_gpu import _direct_chain, _write_gt
    from upsnet_amd.config.config import config, update_config
    from upsnet_amd.dataset import Cityscapes
    from upsnet_amd.evaluate import main
    saved = copy.deepcopy(dict(config))
    try:
        sizes = [(256, 512), (128, 256)]
        root = str(tmp_path / 'Cityscapes')
        make_dataset(root, 'Cityscapes', sizes, seed=11)
        cfg = write_cfg(tmp_path, 'Cityscapes', root, 'val')
        update_config(cfg)
        ds = Cityscapes(image_sets=['val'], phase='test')
        chains = [_direct_chain(vote_model, e['image'], ds.num_classes) for e in ds.roidb]
        _write_gt(ds, chains, list(range(len(sizes))), ['img_%d' % e['id'] for e in ds.roidb])

        # voting alone: the eager path with the base augmentation
        res = main(['--cfg', cfg, '--synthetic_weights', '--bbox_vote', '--bbox_vote_thresh', '0.7'])
        with open(res['results_file'], 'rb') as f:
            got = pickle.load(f)
        assert got['bbox_vote'] == [float(config.test.score_thresh), 0.7]
        assert got['test_aug'] == [[config.test.scales[0], config.test.max_size, False]]
        assert set(got) == {'all_boxes', 'all_masks', 'all_ssegs', 'all_panos', 'all_pano_cls_inds', 'test_aug', 'bbox_vote'}
        n = len(sizes)
        assert len(got['all_ssegs']) == len(got['all_panos']) == len(got['all_pano_cls_inds']) == n
        assert all(len(got['all_boxes'][c]) == n for c in range(1, ds.num_classes))
        m = res['metrics']
        assert {'box_ap', 'mask_ap', 'panoptic', 'sseg'} <= set(m)
        assert 0.0 <= m['sseg']['meanIU'] <= 1.0 and np.isfinite(m['sseg']['meanIU'])
        assert len(res['times']['net_time']) == n
    finally:
        config.clear()
        config.update(saved)
