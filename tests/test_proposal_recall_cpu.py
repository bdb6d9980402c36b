"""CPU: the numpy restatement of evaluate_box_proposals (tests/proposal_recall_ref.py) against the reference's own results
(tests/golden/proposal_recall.npz), hand-derived cases for the tie rules, limit = 0, images with no proposals, num_pos == 0 and the
inclusive area edges, the instances-JSON GT builder (JsonDataset._add_gt_annotations rules), the host summary, and the evaluator's
refusals, which come before any launch."""
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import proposal_recall_ref as prr  # noqa: E402

from upsnet_amd.dataset import proposal_eval as pe  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'proposal_recall.npz')


def golden():
    z = np.load(GOLDEN)
    spec = json.loads(str(z['spec']))
    imgs = [{f: z['img%d_%s' % (i, f)] for f in ('boxes', 'gt_classes', 'is_crowd', 'seg_areas')} for i in range(spec['num_images'])]
    thr = {k: (None if v is None else np.asarray(v)) for k, v in spec['thresholds'].items()}
    calls = []
    for k, (inds, area, limit, t) in enumerate(spec['calls']):
        want = {f: z['call%d_%s' % (k, f)] for f in ('recalls', 'thresholds', 'gt_overlaps', 'ar', 'num_pos')}
        calls.append(([imgs[i] for i in inds], area, limit, thr[t], want))
    return calls


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True)


def check_result(res, want):
    assert same(res['gt_overlaps'], want['gt_overlaps'])
    assert same(res['recalls'], want['recalls'])
    assert same(np.asarray(res['thresholds']), want['thresholds'])
    assert same(np.float64(res['ar']), want['ar'])
    assert int(res['num_pos']) == int(want['num_pos'])


def test_golden_covers_the_issue_cases():
    calls = golden()
    areas = {c[1] for c in calls}
    assert areas == set(prr.AREAS)
    assert any(int(c[4]['num_pos']) == 0 and np.isnan(c[4]['ar']) for c in calls)
    assert {c[2] for c in calls} >= {None, 0, 5}
    assert any(c[3] is not None for c in calls) and any(c[3] is None for c in calls)
    imgs = calls[0][0]
    assert any(not np.any(e['gt_classes'] == 0) for e in imgs)                                    # no proposals
    assert any(not np.any((e['gt_classes'] > 0) & (e['is_crowd'] == 0)) for e in imgs)           # no valid GT
    assert any(np.any(e['is_crowd'][e['gt_classes'] > 0]) for e in imgs)                          # crowd GT
    areas = np.concatenate([e['seg_areas'][e['gt_classes'] > 0] for e in imgs])
    assert all(np.any(areas == e) for e in (32 ** 2, 96 ** 2, 128 ** 2, 256 ** 2, 512 ** 2))


@pytest.mark.parametrize("k", range(len(golden())))
def test_restatement_equals_reference_bitwise(k):
    roidb, area, limit, thr, want = golden()[k]
    check_result(prr.evaluate_box_proposals(roidb, thr, area, limit), want)


def test_host_summary_equals_reference_tail():
    """recall_summary (the evaluator's host tail) on the restated per-image IoUs gives the reference's dict."""
    for roidb, area, limit, thr, want in golden():
        ov = prr.evaluate_box_proposals(roidb, thr, area, limit)['gt_overlaps']
        rng = np.random.default_rng(0)
        check_result(pe.recall_summary(rng.permutation(ov), int(want['num_pos']), thr), want)


def test_iou_restatement_matches_hand_values():
    ov = prr.bbox_overlaps(np.array([[0, 0, 9, 9], [5, 0, 14, 9], [20, 20, 30, 30], [10, 0, 19, 9]], np.float32),
                           np.array([[0, 0, 9, 9]], np.float32))
    assert ov.dtype == np.float32
    assert ov[0, 0] == 1 and ov[1, 0] == np.float32(50) / np.float32(150) and ov[2, 0] == 0
    assert ov[3, 0] == 0      # iw = 9 - 10 + 1 = 0: not > 0


def test_tie_rules_first_column_then_first_row():
    # GT 0 and GT 1 identical; proposals 0 and 1 identical: every IoU 1. Step 0 takes (row 0, col 0), step 1 (row 1, col 1).
    gt = np.array([[0, 0, 9, 9], [0, 0, 9, 9]], np.float32)
    props = np.array([[0, 0, 9, 9], [0, 0, 9, 9]], np.float32)
    assert list(prr.greedy(props, gt)) == [1.0, 1.0]
    # mirror shifts: proposals 0 and 1 have the same IoU with GT 0; GT 1 is covered only by proposal 0 (less well). The first
    # step takes GT 0 (best covered, the first among equal column maxima) with proposal 0 (first row), so GT 1 is left with
    # proposal 1's IoU of 0.
    gt = np.array([[10, 0, 19, 9], [0, 0, 11, 9]], np.float32)
    props = np.array([[8, 0, 17, 9], [12, 0, 21, 9]], np.float32)
    ov = prr.bbox_overlaps(props, gt)
    assert ov[0, 0] == ov[1, 0] and ov[0, 1] > 0 and ov[1, 1] == 0 and ov[0, 0] > ov[0, 1]
    assert list(prr.greedy(props, gt)) == [ov[0, 0], 0.0]


def test_limit_zero_no_proposals_and_num_pos_zero():
    gt = np.array([[0, 0, 9, 9], [20, 20, 39, 39]], np.float32)
    props = np.array([[0, 0, 9, 9]], np.float32)
    e = prr.roidb_entry(props, gt, [1, 1], [0, 0], [100, 400])
    r = prr.evaluate_box_proposals([e], area='all', limit=0)
    assert same(r['gt_overlaps'], np.zeros(2)) and r['num_pos'] == 2 and r['ar'] == 0
    e_none = prr.roidb_entry(np.zeros((0, 4), np.float32), gt, [1, 1], [0, 0], [100, 400])
    r = prr.evaluate_box_proposals([e_none, e], area='all')
    assert r['num_pos'] == 4 and same(r['gt_overlaps'], np.array([0.0, 1.0]))        # the empty image appends nothing
    r = prr.evaluate_box_proposals([e], area='512-inf')
    assert r['num_pos'] == 0 and np.all(np.isnan(r['recalls'])) and np.isnan(r['ar'])
    assert same(r['gt_overlaps'], np.zeros(0))


@pytest.mark.parametrize("area,lo,hi", [('small', 0, 32 ** 2), ('medium', 32 ** 2, 96 ** 2), ('96-128', 96 ** 2, 128 ** 2),
                                        ('128-256', 128 ** 2, 256 ** 2), ('256-512', 256 ** 2, 512 ** 2)])
def test_area_edges_are_inclusive(area, lo, hi):
    areas = np.array([lo - 1, lo, lo + 1, hi - 1, hi, hi + 1], np.float32)
    gt = np.tile(np.array([[0, 0, 9, 9]], np.float32), (len(areas), 1))
    e = prr.roidb_entry(gt.copy(), gt, np.ones(len(areas)), np.zeros(len(areas)), areas)
    r = prr.evaluate_box_proposals([e], area=area)
    assert r['num_pos'] == 4          # lo, lo + 1, hi - 1, hi


def test_gt_builder_rules():
    cls_of = {7: 1, 3: 2}
    anns = [
        {'id': 1, 'area': 50.0, 'bbox': [-5.0, 2.0, 20.0, 10.0], 'category_id': 7, 'iscrowd': 0},   # clipped at x = 0
        {'id': 2, 'area': 50.0, 'bbox': [90.0, 40.0, 30.0, 30.0], 'category_id': 3, 'iscrowd': 1},  # clipped at W-1, H-1; crowd
        {'id': 3, 'area': 0.0, 'bbox': [1.0, 1.0, 5.0, 5.0], 'category_id': 7, 'iscrowd': 0},       # area 0
        {'id': 4, 'area': 9.0, 'bbox': [1.0, 1.0, 1.0, 5.0], 'category_id': 7, 'iscrowd': 0},       # w = 1: x2 == x1
        {'id': 5, 'area': 9.0, 'bbox': [1.0, 1.0, 4.0, 4.0], 'category_id': 7, 'iscrowd': 0, 'ignore': 1},
        {'id': 6, 'area': 2.5, 'bbox': [1.0, 1.0, 0.5, 4.0], 'category_id': 3, 'iscrowd': 0},       # w < 1: max(0, w - 1) = 0
        {'id': 7, 'area': 12.0, 'bbox': [3.0, 4.0, 2.5, 3.0], 'category_id': 3, 'iscrowd': 0},
    ]
    e = pe.gt_entry(anns, (60, 100), cls_of)
    assert e['boxes'].dtype == np.float32 and e['seg_areas'].dtype == np.float32 and e['is_crowd'].dtype == bool
    assert e['boxes'].tolist() == [[0.0, 2.0, 14.0, 11.0], [90.0, 40.0, 99.0, 59.0], [3.0, 4.0, 4.5, 6.0]]
    assert e['gt_classes'].tolist() == [1, 2, 2] and e['is_crowd'].tolist() == [False, True, False]
    assert e['seg_areas'].tolist() == [50.0, 50.0, 12.0]
    e = pe.gt_entry(anns, (60, 100), cls_of, min_area=20)
    assert e['gt_classes'].tolist() == [1, 2]
    with pytest.raises(ValueError, match="category_id"):
        pe.gt_entry([dict(anns[0], category_id=99)], (60, 100), cls_of)


def test_ar_metric_names():
    summ = {(a, lim): {'ar': float(i)} for i, (a, lim) in enumerate((a, lim) for a, _ in pe.AR_AREAS for lim in pe.AR_LIMITS)}
    m = pe.ar_metrics(summ)
    assert list(m) == ['AR@100', 'ARs@100', 'ARm@100', 'ARl@100', 'AR@300', 'ARs@300', 'ARm@300', 'ARl@300',
                       'AR@1000', 'ARs@1000', 'ARm@1000', 'ARl@1000']


def test_refusals_before_any_launch():
    with pytest.raises(ValueError, match="Unknown area"):
        pe.ProposalRecallEvaluator(areas=('tiny',))
    with pytest.raises(ValueError, match="limit"):
        pe.ProposalRecallEvaluator(limits=(-1,))
    ev = pe.ProposalRecallEvaluator(areas=('all',), limits=(None,))
    gt = np.array([[0, 0, 9, 9]], np.float32)
    with pytest.raises(ValueError, match="finite"):
        ev.add(np.array([[0, 0, np.nan, 9]], np.float32), gt, [1], [0], [100])
    with pytest.raises(ValueError, match="finite"):
        ev.add(np.array([[0, 0, 9, 9]], np.float32), np.array([[0, 0, np.inf, 9]]), [1], [0], [100])
    with pytest.raises(ValueError, match="one entry per box"):
        ev.add(np.zeros((1, 4), np.float32), gt, [1, 1], [0], [100])
    with pytest.raises(ValueError, match=r"\[n, 4\]"):
        ev.add(np.zeros((3, 5), np.float32), gt, [1], [0], [100])
    big = np.tile(gt, (4097, 1))
    with pytest.raises(ValueError, match="4096"):
        ev.add(np.zeros((1, 4), np.float32), big, np.ones(4097), np.zeros(4097), np.full(4097, 100.0))
    assert ev.num_images == 0 and ev._bufs == []
    with pytest.raises(ValueError):
        ev += pe.ProposalRecallEvaluator(areas=('small',))


@pytest.mark.parametrize("seed,P,G,dup", [(1, 200, 30, 0.0), (2, 50, 80, 0.2), (3, 400, 120, 0.3), (4, 7, 7, 0.5)])
def test_fast_restatement_equals_plain(seed, P, G, dup):
    """greedy_fast (used by the GPU tests at P = 10 000, G = 4096) makes the plain loop's choices."""
    rng = np.random.default_rng(seed)
    p, g, _, _, _ = prr.random_scene(rng, P, G, dup_frac=dup)
    g[: G // 4] = g[0]                   # identical GT boxes
    assert np.array_equal(prr.greedy_fast(p, g), prr.greedy(p, g))
    for lim in (0, 5, P // 2):
        assert np.array_equal(prr.greedy_fast(p[:lim], g), prr.greedy(p[:lim], g))


# ------------------------------------------------------------------------------------------------ evaluate.py --eval_proposals
def test_eval_proposals_flag():
    from upsnet_amd.config.parse_args import parse_args
    assert parse_args('', ['--eval_proposals']).eval_proposals is True
    assert parse_args('', []).eval_proposals is False


def test_eval_only_without_proposals_in_the_pickle_exits(tmp_path):
    """--eval_only --eval_proposals on a pickle written without --eval_proposals: SystemExit naming the flag, before the dataset
    or any launch."""
    import copy
    import pickle
    from upsnet_amd.config.config import config
    from upsnet_amd.evaluate import main
    saved = copy.deepcopy(dict(config))
    try:
        cfg = tmp_path / 'exp.yaml'
        cfg.write_text('output_path: "%s"\ndataset:\n  dataset: NoSuchDataset\n  test_image_set: val\n' % tmp_path)
        res_dir = tmp_path / 'exp' / 'val' / 'results'
        res_dir.mkdir(parents=True)
        with open(res_dir / 'results_list.pkl', 'wb') as f:
            pickle.dump({'all_boxes': [[]], 'all_masks': None, 'all_ssegs': None, 'all_panos': None, 'all_pano_cls_inds': None}, f)
        with pytest.raises(SystemExit, match='--eval_proposals'):
            main(['--cfg', str(cfg), '--eval_only', '--eval_proposals'])
    finally:
        config.clear()
        config.update(saved)


def test_post_image_stores_scaled_proposals():
    """post_image's proposal rule: rois[:n, 1:5] / float32(im_info[2]) as float32 [n, 4]; nothing else is needed from `out` when
    every head is off."""
    import copy
    import torch
    from upsnet_amd.config.config import config
    from upsnet_amd.evaluate import post_image
    saved = copy.deepcopy(dict(config))
    try:
        for k in ('has_rcnn', 'has_mask_head', 'has_fcn_head', 'has_panoptic_head'):
            config.network[k] = False
        rois = torch.tensor([[0, 10.5, 20.25, 30, 40], [0, 1, 2, 3, 4]], dtype=torch.float32)
        im_info = np.array([800, 1333, 1.3], np.float32)
        props = []
        post_image({'proposals': rois}, im_info, 9, [], None, None, None, None, props)
        assert len(props) == 1 and props[0].dtype == np.float32 and props[0].shape == (2, 4)
        assert np.array_equal(props[0], rois[:, 1:].numpy() / np.float32(1.3))
        post_image({}, im_info, 9, [], None, None, None, None)      # without the list: proposals are not read
    finally:
        config.clear()
        config.update(saved)
