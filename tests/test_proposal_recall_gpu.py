"""GPU: proposal recall on the device (csrc/prop_eval.hip, dataset/proposal_eval.py) against the reference's own results
(tests/golden/proposal_recall.npz) and the numpy restatement (tests/proposal_recall_ref.py), bit for bit: every field of
BaseDataset.evaluate_box_proposals, seeded random scenes up to P = 10 000 and G = 4096, merged and permuted evaluators, and one
poisoned, guard-banded run (tests/memguard.py)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import memguard  # noqa: E402
import proposal_recall_ref as prr  # noqa: E402
from test_proposal_recall_cpu import check_result, golden, same  # noqa: E402

pytestmark = pytest.mark.gpu

ALL_AREAS = list(prr.AREAS)


def dataset():
    from upsnet_amd.dataset.base_dataset import BaseDataset
    return BaseDataset.__new__(BaseDataset)


@pytest.mark.parametrize("k", range(len(golden())))
def test_evaluate_box_proposals_equals_reference(k):
    roidb, area, limit, thr, want = golden()[k]
    check_result(dataset().evaluate_box_proposals(roidb, thresholds=thr, area=area, limit=limit), want)


def scenes(seed, sizes, dup=0.1):
    rng = np.random.default_rng(seed)
    out = []
    for P, G in sizes:
        p, g, c, cr, a = prr.random_scene(rng, P, G, W=2048, H=1024, dup_frac=dup)
        if G >= 8:
            g[1] = g[0]                  # identical GT boxes
            a[1] = a[0]
        out.append(prr.roidb_entry(p, g, c, cr, a, interleave=rng))
    return out


def evaluator_summary(roidb, areas, limits, thresholds=None, order=None):
    from upsnet_amd.dataset.proposal_eval import ProposalRecallEvaluator
    ev = ProposalRecallEvaluator(areas=areas, limits=limits)
    for i in (order if order is not None else range(len(roidb))):
        ev.add_entry(roidb[i])
    return ev.summary(thresholds)


@pytest.mark.parametrize("seed,sizes", [
    (11, [(1000, 7), (1000, 90), (1000, 23), (300, 1), (0, 4), (12, 40)]),
    (12, [(2000, 300), (5, 5), (1, 1), (1000, 0)]),
])
def test_device_equals_restatement_all_areas_and_limits(seed, sizes):
    roidb = scenes(seed, sizes)
    limits = [None, 0, 1, 100, 300, 1000]
    summ = evaluator_summary(roidb, ALL_AREAS, limits)
    for area in ALL_AREAS:
        for lim in limits:
            want = prr.evaluate_box_proposals(roidb, None, area, lim, fast=True)
            check_result(summ[(area, lim)], want)


@pytest.mark.parametrize("P,G", [(10000, 4096), (10000, 64), (300, 4096)])
def test_device_equals_restatement_large(P, G):
    roidb = scenes(100 + G, [(P, G)], dup=0.05)
    limits = [None, 1000, 3]
    summ = evaluator_summary(roidb, ['all', 'large'], limits)
    for area in ('all', 'large'):
        for lim in limits:
            check_result(summ[(area, lim)], prr.evaluate_box_proposals(roidb, None, area, lim, fast=True))


def test_ties_duplicates_and_no_overlap():
    """Integer boxes on a small grid: many exactly equal IoUs of different pairs, duplicated proposals and GT boxes, proposals that
    overlap nothing."""
    rng = np.random.default_rng(5)
    roidb = []
    for _ in range(6):
        P, G = int(rng.integers(1, 60)), int(rng.integers(1, 40))
        gt = rng.integers(0, 6, (G, 2)) * 10
        gt = np.concatenate([gt, gt + 9], 1).astype(np.float32)
        pr = np.concatenate([rng.integers(0, 6, (P, 2)) * 10 + rng.integers(-2, 3, (P, 2)), np.zeros((P, 2))], 1)
        pr[:, 2:] = pr[:, :2] + 9
        pr[::7] += 1000                  # overlaps nothing
        roidb.append(prr.roidb_entry(pr.astype(np.float32), gt, np.ones(G), np.zeros(G), np.full(G, 100.0, np.float32), rng))
    thr = np.array([0.0, 0.3, 0.5, 0.9])
    summ = evaluator_summary(roidb, ['all', 'small'], [None, 2, 10], thr)
    for area in ('all', 'small'):
        for lim in (None, 2, 10):
            check_result(summ[(area, lim)], prr.evaluate_box_proposals(roidb, thr, area, lim))


def test_merged_and_permuted_evaluators_are_identical():
    from upsnet_amd.dataset.proposal_eval import ProposalRecallEvaluator
    roidb = scenes(21, [(800, 30), (500, 12), (0, 3), (1000, 60), (40, 90), (200, 5)])
    areas, limits = ['all', 'small', 'medium', 'large'], [100, 300, 1000]
    whole = evaluator_summary(roidb, areas, limits)
    perm = evaluator_summary(roidb, areas, limits, order=[5, 2, 0, 4, 1, 3])
    a, b = ProposalRecallEvaluator(areas, limits), ProposalRecallEvaluator(areas, limits)
    for i, e in enumerate(roidb):
        (a if i % 2 else b).add_entry(e)
    b += a
    merged = b.summary()
    assert b.num_images == len(roidb)
    for k in whole:
        for other in (perm, merged):
            assert same(other[k]['gt_overlaps'], whole[k]['gt_overlaps']) and same(other[k]['recalls'], whole[k]['recalls'])
            assert same(np.float64(other[k]['ar']), np.float64(whole[k]['ar'])) and other[k]['num_pos'] == whole[k]['num_pos']


def test_add_form_equals_roidb_form():
    from upsnet_amd.dataset.proposal_eval import ProposalRecallEvaluator
    rng = np.random.default_rng(8)
    p, g, c, cr, a = prr.random_scene(rng, 700, 50)
    ev = ProposalRecallEvaluator(ALL_AREAS, [None, 100])
    ev.add(torch.from_numpy(p), g, c, cr, a)
    s = ev.summary()
    e = prr.roidb_entry(p, g, c, cr, a, rng)
    for k in s:
        check_result(s[k], prr.evaluate_box_proposals([e], None, k[0], k[1]))


def test_poisoned_memory():
    """Outputs and workspace of the evaluator come from poisoned, guard-banded torch.empty (its inputs are host arrays, uploaded
    into one staging copy). The summaries equal an ordinary run and the raw device outputs are bitwise equal under both patterns;
    every band stays intact (checked on exit)."""
    from upsnet_amd.dataset import proposal_eval
    roidb = scenes(31, [(1000, 40), (70, 90), (0, 5), (33, 1)])
    areas, limits = ['all', 'small', 'large'], [None, 0, 50]
    plain = evaluator_summary(roidb, areas, limits)
    got = []
    for pattern in 'AB':
        with memguard.poisoned(pattern, modules=memguard.MODULES + ('upsnet_amd.dataset.proposal_eval',)) as guard:
            ev = proposal_eval.ProposalRecallEvaluator(areas, limits)
            for e in roidb:
                ev.add_entry(e)
            s = ev.summary()
            raw = torch.cat(ev._bufs)
        assert guard.count >= 2 * 3           # workspace + output per image with proposals
        got.append((s, raw))
    for k in plain:
        for s, _ in got:
            assert same(s[k]['gt_overlaps'], plain[k]['gt_overlaps']) and same(s[k]['recalls'], plain[k]['recalls'])
            assert same(np.float64(s[k]['ar']), np.float64(plain[k]['ar'])) and s[k]['num_pos'] == plain[k]['num_pos']
    assert memguard.bit_equal(got[0][1], got[1][1])


def test_evaluate_proposals_from_instances_json(tmp_path):
    """BaseDataset.evaluate_proposals: GT from an instances JSON (_add_gt_annotations rules), AR@{100,300,1000} x {all,s,m,l}
    equal to the restatement on the same GT, proposal_recall.txt written."""
    import json
    from upsnet_amd.dataset.proposal_eval import gt_entry
    rng = np.random.default_rng(44)
    images, anns, props = [], [], []
    for i, image_id in enumerate((7, 3, 12)):
        images.append({'id': image_id, 'height': 480, 'width': 640})
        p, g, c, cr, a = prr.random_scene(rng, 1200, 25, W=640, H=480)
        for k in range(len(g)):
            x1, y1, x2, y2 = (float(v) for v in g[k])
            anns.append({'id': len(anns) + 1, 'image_id': image_id, 'category_id': [5, 9][k % 2], 'iscrowd': int(cr[k]),
                         'area': float(a[k]) * (100 if k == 3 else 1), 'bbox': [x1 - 3, y1, x2 - x1 + 1, y2 - y1 + 1]})
        props.append(p)
    path = tmp_path / 'instances.json'
    path.write_text(json.dumps({'images': images, 'annotations': anns, 'categories': [{'id': 5}, {'id': 9}]}))
    ds = dataset()
    ds.instances_json_file = str(path)
    order = sorted(im['id'] for im in images)
    by_id = {im['id']: p for im, p in zip(images, props)}
    all_props = [by_id[i] for i in order]
    m = ds.evaluate_proposals(all_props, str(tmp_path))
    assert (tmp_path / 'proposal_recall.txt').exists() and len(m) == 12
    roidb = []
    for image_id, p in zip(order, all_props):
        g = gt_entry([a for a in anns if a['image_id'] == image_id], (480, 640), {5: 1, 9: 2})
        roidb.append(prr.roidb_entry(p, g['boxes'], g['gt_classes'], g['is_crowd'], g['seg_areas']))
    for lim in (100, 300, 1000):
        for area, sfx in (('all', ''), ('small', 's'), ('medium', 'm'), ('large', 'l')):
            want = prr.evaluate_box_proposals(roidb, None, area, lim, fast=True)['ar']
            assert same(np.float64(m['AR%s@%d' % (sfx, lim)]), np.float64(want))


# ------------------------------------------------------------------------------------------------ proposals out of a run
@pytest.fixture()
def cityscapes_model_config():
    import copy
    from upsnet_amd.config.config import CITYSCAPES_R50, config, update_config_dict
    saved = copy.deepcopy(dict(config))
    update_config_dict(CITYSCAPES_R50)
    yield config
    config.clear()
    config.update(saved)


def test_keep_proposals_fused(cityscapes_model_config):
    """keep_proposals: proposals == rois[:n_rois] of an eager forward with taps, identical through graph replay with one and two
    images in flight; off: the output keys are unchanged."""
    from upsnet_amd.synthetic import build_model, make_image
    model = build_model(device='cuda')
    data = make_image(256, 512, seed=3, device='cuda')
    with torch.no_grad():
        keys = set(model(data))
        model.taps = {}
        model.keep_proposals = True
        out = model(data)
        torch.cuda.synchronize()
        n = int(model.taps['n_rois'].reshape(-1)[0])
        want = model.taps['rois'][:n].clone()
        assert n > 0 and set(out) == keys | {'rois', 'n_rois', 'proposals'}
        assert memguard.bit_equal(out['proposals'], want) and int(out['n_rois'].reshape(-1)[0]) == n
        assert memguard.bit_equal(out['rois'][:n], want)
        model.taps = None
        for _ in range(5):                     # in flight 1: eager warm-up, capture, replays
            o = model(data)
            assert memguard.bit_equal(o['proposals'], want)
        pending, seen = [], 0
        for _ in range(7):                     # in flight 2: forward_async, each result read before its slot replays again
            pending.append(model.forward_async(data))
            if len(pending) >= 2:
                o = pending.pop(0).result()
                assert memguard.bit_equal(o['proposals'], want)
                seen += 1
        while pending:
            assert memguard.bit_equal(pending.pop(0).result()['proposals'], want)
            seen += 1
        assert seen == 7
        model.keep_proposals = False
        assert set(model(data)) == keys
        assert set(model.forward_async(data).result()) == keys


def test_keep_proposals_modules(cityscapes_model_config):
    from upsnet_amd.synthetic import build_model, make_image
    model = build_model(device='cuda', pipeline='modules')
    data = make_image(256, 512, seed=3, device='cuda')
    with torch.no_grad():
        keys = set(model(data))
        model.taps = {}
        model.keep_proposals = True
        out = model(data)
    assert set(out) == keys | {'rois', 'n_rois', 'proposals'}
    assert memguard.bit_equal(out['proposals'], model.taps['rois'])
    assert int(out['n_rois'].reshape(-1)[0]) == model.taps['rois'].shape[0] > 0


def test_evaluate_eval_proposals_end_to_end(tmp_path):
    """evaluate --synthetic_weights --eval_proposals on a generated COCO set whose GT is the network's own detections:
    metrics['proposal_ar'] equals the restatement on the pickled all_proposals and the JSON GT; --eval_only --eval_proposals
    reproduces it; a run without the flag writes the old pickle keys and metrics."""
    import copy
    import json
    import pickle
    from test_dataset_run_cpu import make_dataset, write_cfg
    from test_dataset_run_gpu import CASES, _direct_chain, _write_gt
    from upsnet_amd.config.config import config, update_config
    from upsnet_amd.dataset import coco
    from upsnet_amd.dataset.proposal_eval import gt_entry
    from upsnet_amd.evaluate import main
    from upsnet_amd.synthetic import build_model
    saved = copy.deepcopy(dict(config))
    try:
        image_set, sizes = CASES['coco']
        root = str(tmp_path / 'coco')
        make_dataset(root, 'coco', sizes, seed=11)
        cfg = write_cfg(tmp_path, 'coco', root, image_set)
        update_config(cfg)
        ds = coco(image_sets=[image_set], phase='test')
        model = build_model(device='cuda')
        model.use_graph = False
        chains = [_direct_chain(model, e['image'], ds.num_classes) for e in ds.roidb]
        _write_gt(ds, chains, [2, 0, 3, 1], [e['id'] for e in ds.roidb])
        del model
        torch.cuda.empty_cache()

        first = main(['--cfg', cfg, '--synthetic_weights', '--in-flight', '2', '--eval_proposals'])
        with open(first['results_file'], 'rb') as f:
            res = pickle.load(f)
        assert set(res) == {'all_boxes', 'all_masks', 'all_ssegs', 'all_panos', 'all_pano_cls_inds', 'all_proposals'}
        props = res['all_proposals']
        assert len(props) == len(ds.roidb) and all(p.dtype == np.float32 and p.ndim == 2 and p.shape[1] == 4 and len(p) > 0
                                                    for p in props)
        with open(ds.instances_json_file) as f:
            js = json.load(f)
        cls_of = {int(c['id']): i + 1 for i, c in enumerate(js['categories'])}
        roidb = []
        for e, p in zip(ds.roidb, props):
            g = gt_entry([a for a in js['annotations'] if a['image_id'] == e['id']], (e['height'], e['width']), cls_of)
            roidb.append(prr.roidb_entry(p, g['boxes'], g['gt_classes'], g['is_crowd'], g['seg_areas']))
        assert sum(int(r['gt_classes'].astype(bool).sum()) for r in roidb) > 0
        m = first['metrics']['proposal_ar']
        for lim in (100, 300, 1000):
            for area, sfx in (('all', ''), ('small', 's'), ('medium', 'm'), ('large', 'l')):
                want = prr.evaluate_box_proposals(roidb, None, area, lim, fast=True)['ar']
                assert same(np.float64(m['AR%s@%d' % (sfx, lim)]), np.float64(want)), (area, lim)
        assert m['AR@1000'] > 0
        again = main(['--cfg', cfg, '--eval_only', '--eval_proposals'])
        assert again['metrics']['proposal_ar'] == m

        plain = main(['--cfg', cfg, '--synthetic_weights', '--in-flight', '2'])
        with open(plain['results_file'], 'rb') as f:
            res2 = pickle.load(f)
        assert set(res2) == {'all_boxes', 'all_masks', 'all_ssegs', 'all_panos', 'all_pano_cls_inds'}
        assert 'proposal_ar' not in plain['metrics'] and set(plain['metrics']) == set(first['metrics']) - {'proposal_ar'}
        with pytest.raises(SystemExit, match='--eval_proposals'):
            main(['--cfg', cfg, '--eval_only', '--eval_proposals'])
    finally:
        config.clear()
        config.update(saved)
