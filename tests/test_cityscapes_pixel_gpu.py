"""GPU: the device Cityscapes pixel-level IoU / iIoU (dataset/cityscapes_pixel_eval.py, csrc/cs_pixel_eval.hip) against the numpy
restatement on full maps (tests/cityscapes_pixel_ref.py): the confusion matrix and every image's instance table with ==, and the four
averages and every per-class / per-category score bit for bit when the images are added in the restatement's order -- on the seeded
scenes that tests/test_cityscapes_pixel_cpu.py shows to reach every branch, at 1024 x 2048 and odd sizes down to one-pixel-wide maps,
with both look-up tables, host arrays and device tensors, on poisoned guard-banded memory, merged and permuted (integers equal, the
weighted sums within the bound derived below), and end to end through `python -m upsnet_amd.evaluate`. Nothing is sampled."""
import copy
import functools
import math
import os
import pickle

import numpy as np
import pytest
import torch

from conftest import ROOT  # noqa: F401  (puts the repo root on sys.path)

import cityscapes_pixel_cases as cases
import cityscapes_pixel_ref as ref
import memguard

pytestmark = pytest.mark.gpu

MODULES = memguard.MODULES + ('upsnet_amd.dataset.cityscapes_pixel_eval',)
CLASS_LABELS = (24, 25, 26, 27, 28, 31, 32, 33)
AVERAGES = (('IoU_class', 'averageScoreClasses'), ('iIoU_class', 'averageScoreInstClasses'), ('IoU_category', 'averageScoreCategories'),
            ('iIoU_category', 'averageScoreInstCategories'))


def special_scene():
    return [cases.no_instance_image(), cases.many_instances_image(), cases.all_labels_image(), cases.many_instances_image(40, 33, 64, 512, 2)]


@functools.lru_cache(maxsize=None)
def scene_and_reference(name, avg_name='AVG'):
    if name == 'special':
        scene = special_scene()
    else:
        seed, sizes, n_inst = cases.GPU_SCENES[name]
        scene = cases.make_scene(seed, sizes, n_inst)
    res = ref.evaluate([(g, i, cases.as_label_ids(p, t)) for g, i, p, t in scene], getattr(ref, avg_name))
    return scene, res


def same_bits(a, b):
    a, b = float(a), float(b)
    return (math.isnan(a) and math.isnan(b)) or np.float64(a).view(np.uint64) == np.float64(b).view(np.uint64)


def check_scores(got, res):
    """Every score and average with the restatement's bits, NaNs in the same places."""
    for key, want in AVERAGES:
        assert same_bits(got[key], res[want]), (key, got[key], res[want])
    assert len(got['per_class']) == 19 and len(got['per_category']) == 7
    for name, r in got['per_class'].items():
        assert same_bits(r['iou'], res['classScores'][name]) and same_bits(r['iiou'], res['classInstScores'][name]), (name, r)
    for name, r in got['per_category'].items():
        assert same_bits(r['iou'], res['categoryScores'][name]) and same_bits(r['iiou'], res['categoryInstScores'][name]), (name, r)


def ref_wsum(res):
    rows = [res['inst_stats']['classes'][n] for n in ref.INSTANCE_CLASSES] + [res['inst_stats']['categories'][c] for c in ('human', 'vehicle')]
    return np.array([[r['tp'], r['tpWeighted'], r['fn'], r['fnWeighted']] for r in rows], np.float64)


def check_state(got, res):
    assert got['conf'].dtype == np.int64 and np.array_equal(got['conf'], res['conf'])
    w, want = got['wsum'], ref_wsum(res)
    assert w.dtype == np.float64 and np.array_equal(w.view(np.uint64), want.view(np.uint64)), (w, want)


def check_table(ev, want):
    """The device's instance table of the image added last against the restatement's {raw value: (size, tp, category tp)}."""
    t = ev.last_counts()
    if want is None:
        assert t is None
        return
    t = t.cpu().numpy()
    assert t.shape == (8, 1000, 3) and t.dtype == np.int32
    full = np.zeros((8, 1000, 3), np.int64)
    for v, cell in want.items():
        full[CLASS_LABELS.index(v // 1000), v % 1000] = cell
    assert np.array_equal(t, full)


def off_by_one(a):
    """A contiguous device copy that starts one element into its buffer: not 16-byte aligned (the kernel's scalar loads)."""
    buf = np.zeros(a.size + 1, a.dtype)
    buf[1:] = a.reshape(-1)
    t = torch.from_numpy(buf).cuda()[1:].view(a.shape)
    assert t.data_ptr() % 16 != 0 and t.is_contiguous()
    return t


def feed(ev, scene, tables=None, images=None, wrap=None):
    """Images k = 0, 1, ...: host arrays, device tensors (k % 3 == 1), device tensors off the 16-byte grid (k % 3 == 2), or banded
    device copies (wrap)."""
    for k in (range(len(scene)) if images is None else images):
        gl, gi, pr, train = scene[k]
        if wrap is not None:
            gl, gi, pr = (wrap(torch.from_numpy(a).cuda()) for a in (gl, gi, pr))
        elif k % 3 == 1:
            gl, gi, pr = (torch.from_numpy(a).cuda() for a in (gl, gi, pr))
        elif k % 3 == 2:
            gl, gi, pr = (off_by_one(a) for a in (gl, gi, pr))
        ev.add(gl, gi, pr, train_ids=train, name='img%d' % k)
        if tables is not None:
            check_table(ev, tables[k])


@pytest.mark.parametrize('name', ['full', 'odd', 'special'])
def test_add_equals_the_restatement(name):
    from upsnet_amd.dataset.cityscapes_pixel_eval import PixelEvaluator
    scene, res = scene_and_reference(name)
    ev = PixelEvaluator(avg_class_size=ref.AVG)
    feed(ev, scene, res['inst'])
    got = ev.summary()
    check_state(got, res)
    check_scores(got, res)
    assert ev.num_images == len(scene)


def test_default_and_other_average_sizes():
    """The default table (equal to the tests' own copy of the recalled values) and a table of the tests' own."""
    from upsnet_amd.dataset.cityscapes_pixel_eval import PixelEvaluator
    scene, res = scene_and_reference('odd')
    ev = PixelEvaluator()
    feed(ev, scene)
    check_scores(ev.summary(), res)
    scene, res = scene_and_reference('odd', 'OTHER_AVG')
    ev = PixelEvaluator(avg_class_size=ref.OTHER_AVG)
    feed(ev, scene)
    got = ev.summary()
    check_state(got, res)
    check_scores(got, res)


def test_hand_case_on_the_device():
    """The CPU file's two-instance case through the device: IoU 0.62, iIoU 0.425 with every average size 100."""
    from upsnet_amd.dataset.cityscapes_pixel_eval import PixelEvaluator
    gi = np.full((10, 10), 7, np.uint16)
    gi[0:4, :] = 24001
    gi[5, :] = 24002
    pr = np.full((10, 10), 7, np.uint8)
    pr[0:3, :] = 24
    pr[5, 0] = 24
    ev = PixelEvaluator(avg_class_size=[100.0] * 8)
    ev.add(cases.labels_of(gi), gi, pr, train_ids=False)
    got = ev.summary()
    assert got['per_class']['person'] == {'iou': 0.62, 'iiou': 0.425} and got['iIoU_class'] == 0.425
    assert got['wsum'][0].tolist() == [31.0, 85.0, 19.0, 115.0] and got['wsum'][8].tolist() == [31.0, 85.0, 19.0, 115.0]


def test_without_instance_maps_and_empty_evaluator():
    from upsnet_amd.dataset.cityscapes_pixel_eval import PixelEvaluator
    ev = PixelEvaluator()
    got = ev.summary()
    assert all(math.isnan(got[k]) for k, _ in AVERAGES) and not got['conf'].any()
    scene, _ = scene_and_reference('odd')
    res = ref.evaluate([(g, None, cases.as_label_ids(p, t)) for g, _, p, t in scene])
    for gl, _, pr, train in scene:
        ev.add(gl, None, pr, train_ids=train)
        assert ev.last_counts() is None
    got = ev.summary()
    assert np.array_equal(got['conf'], res['conf']) and not got['wsum'].any()
    check_scores(got, res)
    assert math.isnan(got['iIoU_class']) and not math.isnan(got['IoU_class'])


def test_merged_and_permuted_evaluators():
    """Integer state equal; the weighted sums within a derived bound: a float64 sum of N non-negative terms differs between any two
    orders by at most (N - 1) * 2^-53 relative to the sum (each of the N - 1 additions rounds by at most 2^-53 relative to a partial
    sum that is at most the total), so tpWeighted / fnWeighted are compared at N * 2^-53 relative, N = the instances added."""
    from upsnet_amd.dataset.cityscapes_pixel_eval import PixelEvaluator
    scene, res = scene_and_reference('odd')
    n = len(scene)
    n_inst = sum(len(t) for t in res['inst'])
    assert n_inst > 20
    want = ref_wsum(res)

    def check(ev):
        got = ev.summary()
        assert np.array_equal(got['conf'], res['conf'])
        assert np.array_equal(got['wsum'][:, [0, 2]], want[:, [0, 2]])
        assert np.all(np.abs(got['wsum'][:, [1, 3]] - want[:, [1, 3]]) <= n_inst * 2.0 ** -53 * want[:, [1, 3]])
        return got
    a, b, c = PixelEvaluator(avg_class_size=ref.AVG), PixelEvaluator(avg_class_size=ref.AVG), PixelEvaluator(avg_class_size=ref.AVG)
    feed(a, scene, images=range(0, 3))
    feed(b, scene, images=range(3, n))
    a += b
    a += c                       # an evaluator that saw nothing
    check(a)
    assert a.num_images == n and a.names == ['img%d' % k for k in range(n)]
    c += a                       # into an evaluator that saw nothing
    check(c)
    p = PixelEvaluator(avg_class_size=ref.AVG)
    feed(p, scene, images=[4, 2, 6, 0, 3, 1, 5][:n])
    check(p)
    with pytest.raises(ValueError):
        a += 3
    with pytest.raises(ValueError, match='average class sizes'):
        a += PixelEvaluator(avg_class_size=ref.OTHER_AVG)


def test_unknown_labels_raise_after_the_run_naming_the_image():
    from upsnet_amd.dataset.cityscapes_pixel_eval import PixelEvaluator
    scene, _ = scene_and_reference('odd')
    for what, k_bad in (('train id', 2), ('label id', 1), ('gt', 3)):
        ev = PixelEvaluator()
        for k, (gl, gi, pr, train) in enumerate(scene):
            gl, pr = gl.copy(), pr.copy()
            if k == k_bad and what == 'gt':
                gl[-1, -1] = 34
            elif k == k_bad:
                assert train == (what == 'train id')
                pr[0, :2] = 19 if train else 34
            ev.add(gl, gi, pr, train_ids=train, name='img%d' % k)
        with pytest.raises(ValueError, match='img%d: %s' % (k_bad, '0 prediction pixels .*, 1 ground' if what == 'gt' else '2 prediction pixels')):
            ev.summary()
    b = PixelEvaluator()
    b.add(scene[0][0], scene[0][1], scene[0][2], train_ids=True, name='fine')
    b += ev                          # the error survives a merge, with its image's name
    with pytest.raises(ValueError, match='img3: '):
        b.summary()


def test_value_errors_come_before_any_launch(monkeypatch):
    from upsnet_amd.dataset import cityscapes_pixel_eval as pe

    def no_launch(*a, **k):
        raise AssertionError("a launch was reached")
    monkeypatch.setattr(pe.PixelEvaluator, '_launch', no_launch)
    H, W = 6, 5
    gl, gi, pr = np.full((H, W), 7, np.uint8), np.full((H, W), 7, np.uint16), np.zeros((H, W), np.uint8)
    ev = pe.PixelEvaluator()
    bad = {
        'label dtype': (gl.astype(np.int32), gi, pr), 'label dims': (gl[None], gi, pr), 'label type': (gl.tolist(), gi, pr),
        'ids dtype': (gl, gi.astype(np.int32), pr), 'ids size': (gl, gi[:, :4], pr), 'ids tensor dtype': (gl, torch.zeros((H, W), dtype=torch.int32), pr),
        'pred dtype': (gl, gi, pr.astype(np.int64)), 'pred size': (gl, gi, pr[:5]), 'pred tensor dtype': (gl, gi, torch.zeros((H, W), dtype=torch.int64)),
        'pred dims': (gl, gi, pr[None]), 'empty': (gl[:0], gi[:0], pr[:0]),
    }
    for what, (a, b, c) in bad.items():
        with pytest.raises(ValueError):
            ev.add(a, b, c)
            pytest.fail("%s: no ValueError" % what)
    with pytest.raises(AssertionError, match='a launch was reached'):       # and the valid calls do reach the launch
        ev.add(gl, gi, pr)
    with pytest.raises(AssertionError, match='a launch was reached'):
        ev.add(torch.from_numpy(gl), None, torch.from_numpy(pr).cuda(), train_ids=False)


def test_poisoned_guard_banded_memory():
    """Every torch.empty of the new module poisoned and fenced, the inputs inside bands of poison (odd sizes: the 16-byte loads end
    exactly where the maps end): the same bits under both patterns as without, every band intact."""
    from upsnet_amd.dataset.cityscapes_pixel_eval import PixelEvaluator
    scene, res = scene_and_reference('odd')

    def run(pattern):
        ev = PixelEvaluator(avg_class_size=ref.AVG)
        last = []
        for k in range(len(scene)):
            feed(ev, scene, images=[k], wrap=(lambda t: memguard.banded_copy(t, pattern)) if pattern else None)
            last.append(ev._last.clone())
        got = ev.summary()
        return got, last

    plain = run(None)
    check_state(plain[0], res)
    check_scores(plain[0], res)
    for pattern in ('A', 'B'):
        with memguard.poisoned(pattern, modules=MODULES) as g:
            got = run(pattern)
        assert g.count >= len(scene)
        check_state(got[0], res)
        check_scores(got[0], res)
        for x, y in zip(got[1], plain[1]):
            assert memguard.bit_equal(x, y)


# ------------------------------------------------------------------------------------------------ end to end
@pytest.fixture()
def saved_config():
    from upsnet_amd.config.config import config
    saved = copy.deepcopy(dict(config))
    yield config
    config.clear()
    config.update(saved)


def test_evaluate_end_to_end_with_eval_pixels(tmp_path, saved_config):
    """A generated Cityscapes tree whose label-id maps are the network's own semantic output with a shifted band of other labels, a
    void band and an ignored label, and whose instance-id maps cut the thing regions into instances: --eval_pixels equals the
    restatement on the pickled predictions, --eval_only reproduces it, --write_ssegs then --score_ssegs gives the same bits for both
    PNG kinds, a run without the flags has the metrics it had before, and a missing map is named before anything runs."""
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
    t2l = np.array(ref.TRAIN2LABEL, np.uint8)
    gts = []
    for k, entry in enumerate(ds.roidb):
        H, W = entry['height'], entry['width']
        labels = np.roll(t2l[chains[k]['sseg']], 5, 1)           # the prediction's own labels, five columns off
        labels[:, :W // 8] = 0                                    # a void band
        labels[H // 2:H // 2 + H // 8, W // 4:W // 2] = 9         # an ignored label
        labels[:H // 4, W // 2:] = 24 + (np.arange(W - W // 2) // 16 % 4)[None, :].astype(np.uint8)     # persons .. trucks
        ids = labels.astype(np.uint16)
        things = labels >= 24
        cell = (np.arange(H)[:, None] // 32 * 16 + np.arange(W)[None, :] // 32) % 1000
        ids[things] = (labels[things].astype(np.uint16) * 1000 + cell[things]).astype(np.uint16)
        ids[H // 8:H // 4, W // 2:W // 2 + 16] = 24              # a person group region
        for path, arr in ((ds.label_gt_path(entry), labels), (ds.instance_gt_path(entry), ids)):
            os.makedirs(os.path.dirname(path), exist_ok=True)
            Image.fromarray(arr).save(path)
        gts.append((labels, ids))

    res = main(['--cfg', cfg, '--synthetic_weights', '--eval_pixels', '--write_ssegs'])
    with open(res['results_file'], 'rb') as f:
        got = pickle.load(f)
    want = ref.evaluate([(gl, gi, t2l[np.asarray(got['all_ssegs'][k]).reshape(gl.shape)]) for k, (gl, gi) in enumerate(gts)])
    assert sum(len(t) for t in want['inst']) > 10 and 0.0 < want['averageScoreInstClasses'] < 1.0
    m = res['metrics']
    assert set(m) == {'box_ap', 'mask_ap', 'panoptic', 'sseg', 'pixel_iou'}
    check_state(m['pixel_iou'], want)
    check_scores(m['pixel_iou'], want)
    results_dir = os.path.dirname(res['results_file'])
    with open(os.path.join(results_dir, 'pixel_results.txt')) as f:
        text = f.read()
    assert 'road' in text and 'vehicle' in text and '%5.3f' % want['averageScoreClasses'] in text

    scored = main(['--cfg', cfg, '--score_ssegs', os.path.join(results_dir, 'ssegs')])
    assert scored['results_file'] is None and set(scored['metrics']) == {'pixel_iou'}
    check_state(scored['metrics']['pixel_iou'], want)
    check_scores(scored['metrics']['pixel_iou'], want)

    again = main(['--cfg', cfg, '--eval_only', '--eval_pixels', '--write_ssegs', '--ssegs_label_ids'])
    assert again['times'] is None
    check_state(again['metrics']['pixel_iou'], want)
    check_scores(again['metrics']['pixel_iou'], want)
    with Image.open(os.path.join(results_dir, 'ssegs_label_ids', os.path.basename(ds.roidb[0]['image'])[:-len('_leftImg8bit.png')] + '.png')) as im:
        assert im.mode == 'L'
    scored = main(['--cfg', cfg, '--score_ssegs', os.path.join(results_dir, 'ssegs_label_ids')])
    check_state(scored['metrics']['pixel_iou'], want)
    check_scores(scored['metrics']['pixel_iou'], want)

    plain = main(['--cfg', cfg, '--eval_only'])
    assert set(plain['metrics']) == {'box_ap', 'mask_ap', 'panoptic', 'sseg'}
    assert np.array_equal(plain['metrics']['mask_ap'], m['mask_ap']) and np.array_equal(plain['metrics']['box_ap'], m['box_ap'])
    assert plain['metrics']['panoptic'] == m['panoptic'] and plain['metrics']['sseg']['meanIU'] == m['sseg']['meanIU']

    os.remove(os.path.join(results_dir, 'ssegs', os.path.basename(ds.roidb[1]['image'])[:-len('_leftImg8bit.png')] + '.png'))
    with pytest.raises(FileNotFoundError, match='no prediction for'):
        main(['--cfg', cfg, '--score_ssegs', os.path.join(results_dir, 'ssegs')])
    os.remove(ds.label_gt_path(ds.roidb[1]))
    with pytest.raises(FileNotFoundError, match='gtFine_labelIds.png'):
        main(['--cfg', cfg, '--eval_only', '--eval_pixels'])
