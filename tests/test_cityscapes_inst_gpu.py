"""GPU: the device Cityscapes instance-level AP (dataset/cityscapes_eval.py, csrc/cs_inst_eval.hip) against the numpy restatement on
full boolean masks (tests/cityscapes_inst_ref.py): the integer counts of every prediction, and aps / AP / AP50 bit for bit, on the
seeded scenes that tests/test_cityscapes_inst_cpu.py shows to reach every branch -- through add_rle (compressed strings and plain
count lists, both walks of the id map) and add_masks (uint8 and bool), merged and permuted, on poisoned guard-banded memory, and end
to end through `python -m upsnet_amd.evaluate --eval_instances`. Every comparison is equality; nothing is sampled."""
import copy
import functools
import os
import pickle

import numpy as np
import pytest
import torch

from conftest import ROOT  # noqa: F401  (puts the repo root on sys.path)

import cityscapes_inst_cases as cases
import cityscapes_inst_ref as ref
import memguard

pytestmark = pytest.mark.gpu

MODULES = memguard.MODULES + ('upsnet_amd.dataset.cityscapes_eval',)


@functools.lru_cache(maxsize=None)
def scene_and_reference(name):
    seed, sizes, n_regions = cases.GPU_SCENES[name]
    scene = cases.make_scene(seed, sizes, n_regions)
    aps, avg, counts = ref.evaluate(scene)
    return scene, aps, avg, counts


def same_bits(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a.view(np.uint64)[~np.isnan(a)],
                                                                                            b.view(np.uint64)[~np.isnan(b)])


def check_summary(got, aps, avg):
    assert got['aps'].dtype == np.float64 and got['aps'].shape == (8, 10)
    assert same_bits(got['aps'], aps), (got['aps'], aps)
    assert same_bits(got['AP'], avg['AP']) and same_bits(got['AP50'], avg['AP50'])
    for name, r in avg['per_class'].items():
        assert same_bits(got['per_class'][name]['ap'], r['ap']) and same_bits(got['per_class'][name]['ap50'], r['ap50']), name


def check_counts(ev, gt, preds, order, want):
    """The device's integers of the image added last against the restatement's: area, void, every intersection, GT pixel counts."""
    c = {k: v.cpu().numpy() for k, v in ev.last_counts().items()}
    assert c['area'].shape == (len(order),) and c['inter'].shape == (len(order), 1001) and c['gt'].shape == (8, 1001)
    for row, i in enumerate(order):
        w = want[i]
        label = ref.CLASSES[preds[i]['cls'] - 1][1]
        inter = {(label if s == 0 else label * 1000 + s - 1): int(n) for s, n in enumerate(c['inter'][row]) if n}
        if w is None:
            assert c['area'][row] == 0 and c['void'][row] == 0 and not inter
        else:
            assert (int(c['area'][row]), int(c['void'][row]), inter) == (w['area'], w['void'], w['inter']), (row, i)
    values, pixels = np.unique(gt, return_counts=True)
    gt_want = np.zeros((8, 1001), np.int64)
    for v, n in zip(values.tolist(), pixels.tolist()):
        label = v // 1000 if v >= 1000 else v
        for k, (_, lid) in enumerate(ref.CLASSES):
            if lid == label:
                gt_want[k, 0 if v < 1000 else 1 + v - 1000 * label] = n
    assert np.array_equal(c['gt'], gt_want)


def feed_rle(ev, scene, want_counts=None, images=None):
    from upsnet_amd.dataset.rle import rle_to_string
    for k in (range(len(scene)) if images is None else images):
        gt, preds = scene[k]
        dets, rles, order = cases.per_class_results(preds, rle_to_string if k % 2 == 0 else None)
        ev.add_rle(torch.from_numpy(gt).cuda() if k % 3 == 1 else gt, dets, rles)
        if want_counts is not None:
            check_counts(ev, gt, preds, order, want_counts[k])


def feed_masks(ev, scene, want_counts=None, images=None, wrap=lambda t: t):
    for k in (range(len(scene)) if images is None else images):
        gt, preds = scene[k]
        masks = np.stack([p['mask'] for p in preds])
        masks = torch.from_numpy(masks if k % 2 else masks.astype(np.uint8) * 255).cuda()
        scores = np.array([p['conf'] for p in preds], np.float32)
        classes = np.array([p['cls'] for p in preds], np.int64)
        ev.add_masks(wrap(torch.from_numpy(gt).cuda()) if k % 2 else gt, wrap(masks), torch.from_numpy(scores).cuda() if k % 2 else scores,
                     classes)
        if want_counts is not None:
            check_counts(ev, gt, preds, list(range(len(preds))), want_counts[k])


@pytest.mark.parametrize('walk', ['transposed', 'strided'])
@pytest.mark.parametrize('name', sorted(cases.GPU_SCENES))
def test_add_rle_equals_the_restatement(name, walk):
    from upsnet_amd.dataset.cityscapes_eval import InstanceEvaluator
    scene, aps, avg, counts = scene_and_reference(name)
    ev = InstanceEvaluator(walk=walk)
    feed_rle(ev, scene, counts)
    check_summary(ev.summary(), aps, avg)
    assert ev.num_images == len(scene)


@pytest.mark.parametrize('name', sorted(cases.GPU_SCENES))
def test_add_masks_equals_the_restatement(name):
    from upsnet_amd.dataset.cityscapes_eval import InstanceEvaluator
    scene, aps, avg, counts = scene_and_reference(name)
    ev = InstanceEvaluator()
    feed_masks(ev, scene, counts)
    check_summary(ev.summary(), aps, avg)


def test_hand_cases_on_the_device():
    """Two of the CPU file's hand-derived cases through the device: overlap exactly 300 / 500, and a prediction 80 % on void."""
    from upsnet_amd.dataset.cityscapes_eval import InstanceEvaluator
    from test_cityscapes_inst_cpu import car_with_tp, pred, rect, road
    gt = road()
    car_with_tp(gt)
    ev = InstanceEvaluator()
    ev.add_masks(gt, torch.from_numpy(rect(60, 80, 2, 7, 20, 20)[None]).cuda(), np.array([0.9], np.float32), np.array([3]))
    assert ev.summary()['aps'][2].tolist() == [1.0, 1.0] + [0.0] * 8
    gt = road()
    tp = car_with_tp(gt)
    gt[40:50, 30:38] = 0
    preds = [tp, pred(3, 0.9, rect(60, 80, 40, 30, 10, 10))]
    ev = InstanceEvaluator()
    dets, rles, _ = cases.per_class_results(preds)
    ev.add_rle(gt, dets, rles)
    assert ev.summary()['aps'][2].tolist() == [1.0] * 6 + [0.25] * 4


def test_images_without_predictions_and_empty_evaluator():
    from upsnet_amd.dataset.cityscapes_eval import InstanceEvaluator
    ev = InstanceEvaluator()
    assert np.all(np.isnan(ev.summary()['aps']))
    scene, _, _, _ = scene_and_reference('odd')
    images = [(gt, []) for gt, _ in scene]
    aps, avg, _ = ref.evaluate(images)
    for gt, _ in images:
        ev.add_rle(gt, [[]] * 9, [[]] * 9)
    check_summary(ev.summary(), aps, avg)
    ev2 = InstanceEvaluator()
    for gt, _ in images:
        ev2.add_masks(gt, torch.zeros((0,) + gt.shape, dtype=torch.uint8, device='cuda'), np.zeros(0, np.float32), np.zeros(0, np.int64))
    check_summary(ev2.summary(), aps, avg)


def test_merged_and_permuted_evaluators_give_the_same_bits():
    from upsnet_amd.dataset.cityscapes_eval import InstanceEvaluator
    scene, aps, avg, _ = scene_and_reference('odd')
    n = len(scene)
    a, b, c = InstanceEvaluator(), InstanceEvaluator(), InstanceEvaluator()
    feed_rle(a, scene, images=range(0, 2))
    feed_masks(b, scene, images=range(2, n))
    a += b
    a += c                       # an evaluator that saw nothing
    check_summary(a.summary(), aps, avg)
    assert a.num_images == n
    p = InstanceEvaluator()
    feed_rle(p, scene, images=[4, 2, 5, 0, 3, 1][:n])
    check_summary(p.summary(), aps, avg)
    with pytest.raises(ValueError):
        a += 3


def test_value_errors_come_before_any_launch(monkeypatch):
    from upsnet_amd.dataset import cityscapes_eval as ce
    from upsnet_amd.dataset.rle import rle_to_string

    def no_launch(*a, **k):
        raise AssertionError("a launch was reached")
    monkeypatch.setattr(ce.InstanceEvaluator, '_launch', no_launch)
    H, W = 6, 5
    gt = np.full((H, W), 26001, np.uint16)
    ev = ce.InstanceEvaluator()
    ok_rle = {'size': [H, W], 'counts': rle_to_string([3, 4, 23])}
    det = np.array([[0, 0, 1, 1, 0.5]], np.float32)

    def rle_call(c, dets, rles, n_cls=9, g=gt):
        d, r = [[] for _ in range(n_cls)], [[] for _ in range(n_cls)]
        d[c], r[c] = dets, rles
        return lambda: ev.add_rle(g, d, r)

    def mask_call(masks, scores, classes, g=gt):
        return lambda: ev.add_masks(g, masks, scores, classes)
    one = torch.ones((1, H, W), dtype=torch.uint8, device='cuda')
    s1, c1 = np.array([0.5], np.float32), np.array([3])
    bad = {
        'rle size': rle_call(3, det, [{'size': [H, W + 1], 'counts': rle_to_string([3, 4, 29])}]),
        'rle sum': rle_call(3, det, [{'size': [H, W], 'counts': rle_to_string([3, 4, 22])}]),
        'rle list sum': rle_call(3, det, [{'size': [H, W], 'counts': [3, 4, 24]}]),
        'rle negative': rle_call(3, det, [{'size': [H, W], 'counts': [33, -3]}]),
        'rle polygon': rle_call(3, det, [[0.0, 0.0, 1.0, 1.0, 2.0, 0.0]]),
        'dets shape': rle_call(3, det[:, :4], [ok_rle]),
        'dets dtype': rle_call(3, det.astype(np.int64), [ok_rle]),
        'dets / masks': rle_call(3, det, [ok_rle, ok_rle]),
        'class 9': rle_call(9, det, [ok_rle], n_cls=10),
        'gt dtype': rle_call(3, det, [ok_rle], g=gt.astype(np.int32)),
        'gt dims': rle_call(3, det, [ok_rle], g=gt[None]),
        'gt tensor dtype': rle_call(3, det, [ok_rle], g=torch.zeros((H, W), dtype=torch.int32)),
        'gt type': rle_call(3, det, [ok_rle], g=gt.tolist()),
        'mask size': mask_call(torch.ones((1, H + 1, W), dtype=torch.uint8, device='cuda'), s1, c1),
        'mask dtype': mask_call(one.float(), s1, c1),
        'mask dims': mask_call(one[0], s1, c1),
        'mask host': mask_call(one.cpu(), s1, c1),
        'score dtype': mask_call(one, s1.astype(np.float64), c1),
        'score shape': mask_call(one, np.zeros(2, np.float32), c1),
        'class dtype': mask_call(one, s1, np.array([3.0])),
        'class shape': mask_call(one, s1, np.array([3, 3])),
        'class 0': mask_call(one, s1, np.array([0])),
        'class 9 dense': mask_call(one, s1, torch.tensor([9], device='cuda')),
    }
    for what, call in bad.items():
        with pytest.raises(ValueError):
            call()
            pytest.fail("%s: no ValueError" % what)
    with pytest.raises(AssertionError, match='a launch was reached'):       # and the valid calls do reach the launch
        rle_call(3, det, [ok_rle])()
    with pytest.raises(AssertionError, match='a launch was reached'):
        mask_call(one, s1, c1)()
    with pytest.raises(ValueError):
        ce.InstanceEvaluator(walk='diagonal')


@pytest.mark.parametrize('feed', ['rle', 'masks'])
def test_poisoned_guard_banded_memory(feed):
    """Every torch.empty of the new module poisoned and fenced: the same bits under both patterns as without, every band intact."""
    from upsnet_amd.dataset.cityscapes_eval import InstanceEvaluator
    scene, aps, avg, counts = scene_and_reference('odd')

    def run(pattern):
        ev = InstanceEvaluator()
        last = []
        for k in range(len(scene)):
            if feed == 'rle':
                feed_rle(ev, scene, images=[k])
            else:
                feed_masks(ev, scene, images=[k], wrap=(lambda t: memguard.banded_copy(t, pattern)) if pattern else (lambda t: t))
            last.append(ev._last[0].clone())
        res = ev.summary()
        rec = (ev._score[:ev._n].clone(), ev._cls[:ev._n].clone(), ev._code[:ev._n].clone(), ev._state.clone())
        return res, last, rec

    plain = run(None)
    check_summary(plain[0], aps, avg)
    for pattern in ('A', 'B'):
        with memguard.poisoned(pattern, modules=MODULES) as g:
            got = run(pattern)
        assert g.count >= 2 * len(scene)
        check_summary(got[0], aps, avg)
        for x, y in zip(got[1] + list(got[2]), plain[1] + list(plain[2])):
            assert memguard.bit_equal(x, y)


# ------------------------------------------------------------------------------------------------ end to end
@pytest.fixture()
def saved_config():
    from upsnet_amd.config.config import config
    saved = copy.deepcopy(dict(config))
    yield config
    config.clear()
    config.update(saved)


def _decode(rle):
    """A compressed COCO RLE dict -> bool [H, W] (pycocotools' rleFrString restated; column-major runs)."""
    s, counts, p = rle['counts'], [], 0
    while p < len(s):
        x, k, more = 0, 0, True
        while more:
            c = ord(s[p]) - 48
            x |= (c & 0x1f) << (5 * k)
            more = bool(c & 0x20)
            p += 1
            k += 1
            if not more and (c & 0x10):
                x |= -1 << (5 * k)
        if len(counts) > 2:
            x += counts[-2]
        counts.append(x)
    h, w = rle['size']
    return np.repeat(np.arange(len(counts)) % 2, counts).astype(bool).reshape(w, h).T


def test_evaluate_end_to_end_with_eval_instances(tmp_path, saved_config):
    """A generated Cityscapes tree whose instance-id maps are painted from the network's own masks (later masks over earlier ones),
    plus a car group region and a void band: --eval_instances equals the restatement on the pickled results, --eval_only reproduces
    it, and a run without the flag has the metrics it had before."""
    from PIL import Image
    from test_dataset_run_cpu import make_dataset, write_cfg
    from test_dataset_run_gpu import _direct_chain, _write_gt
    from upsnet_amd.config.config import update_config
    from upsnet_amd.dataset import Cityscapes
    from upsnet_amd.evaluate import main
    from upsnet_amd.synthetic import build_model
    root = str(tmp_path / 'Cityscapes')
    make_dataset(root, 'Cityscapes', [(256, 512)] * 2 + [(128, 256)], seed=11)
    cfg = write_cfg(tmp_path, 'Cityscapes', root, 'val')
    update_config(cfg)
    ds = Cityscapes(image_sets=['val'], phase='test')
    model = build_model(device='cuda')
    model.use_graph = False
    chains = [_direct_chain(model, e['image'], ds.num_classes) for e in ds.roidb]
    n = len(ds.roidb)
    _write_gt(ds, chains, list(range(n)), ['img_%d' % e['id'] for e in ds.roidb])
    del model
    torch.cuda.empty_cache()
    maps = []
    for k, entry in enumerate(ds.roidb):
        H, W = entry['height'], entry['width']
        ids = np.full((H, W), 7, np.uint16)
        for c in range(1, 9):
            for j, rle in enumerate(chains[k]['masks'][c - 1]):
                ids[_decode(rle)] = ref.CLASSES[c - 1][1] * 1000 + j
        ids[H // 2:H // 2 + H // 8, W // 4:W // 2] = 26      # a car group region
        ids[:, :W // 8] = 0                                   # a void band
        path = ds.instance_gt_path(entry)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        Image.fromarray(ids).save(path)
        maps.append(ids)

    res = main(['--cfg', cfg, '--synthetic_weights', '--eval_instances'])
    with open(res['results_file'], 'rb') as f:
        got = pickle.load(f)
    images = []
    for k in range(n):
        preds = [{'cls': c, 'conf': got['all_boxes'][c][k][j, 4], 'mask': _decode(rle)}
                 for c in range(1, 9) for j, rle in enumerate(got['all_masks'][c][k])]
        images.append((maps[k], preds))
    assert sum(len(p) for _, p in images) > 0
    stats = {}
    aps, avg, _ = ref.evaluate(images, stats)
    assert stats.get('ap_curve', 0) > 0, stats
    m = res['metrics']
    assert set(m) == {'box_ap', 'mask_ap', 'panoptic', 'sseg', 'instance_ap'}
    check_summary(m['instance_ap'], aps, avg)
    with open(os.path.join(os.path.dirname(res['results_file']), 'instance_results.txt')) as f:
        lines = f.read().splitlines()
    assert [l.split(':')[0].strip() for l in lines[3:11]] == [name for name, _ in ref.CLASSES]
    assert lines[-1].startswith('average') and lines[-1].split()[-2:] == ['%.3f' % avg['AP'], '%.3f' % avg['AP50']]

    again = main(['--cfg', cfg, '--eval_only', '--eval_instances'])
    assert again['times'] is None
    check_summary(again['metrics']['instance_ap'], aps, avg)
    assert np.array_equal(again['metrics']['mask_ap'], m['mask_ap'])

    plain = main(['--cfg', cfg, '--eval_only'])
    assert set(plain['metrics']) == {'box_ap', 'mask_ap', 'panoptic', 'sseg'}
    assert np.array_equal(plain['metrics']['mask_ap'], m['mask_ap']) and np.array_equal(plain['metrics']['box_ap'], m['box_ap'])
    assert plain['metrics']['panoptic'] == m['panoptic']

    os.remove(ds.instance_gt_path(ds.roidb[1]))
    with pytest.raises(FileNotFoundError, match='gtFine_instanceIds.png'):
        main(['--cfg', cfg, '--eval_only', '--eval_instances'])
