"""GPU: csrc/gt_prepare.hip against its numpy restatement (tests/gt_prepare_ref.py), bit for bit -- both maps, the segment table, the
run lists, their counts and order -- on the shapes of tests/gt_prepare_cases.py; determinism, guard bands, the overflow flags, the
labelIds cross-check, the panoptic-to-semantic converter; and the round trip: a raw Cityscapes tree / COCO panoptic download is
prepared, the dataset classes load it, and predictions derived from the ground truth score exactly 1 through every public scorer."""
import copy
import json
import os

import numpy as np
import pytest
import torch

import memguard
from gt_prepare_cases import CASES, case, e2e_scene
from gt_prepare_ref import semantic_reference
from test_dataset_run_cpu import make_dataset, write_cfg
from test_gt_prepare_cpu import make_raw_cityscapes

pytestmark = pytest.mark.gpu

GUARDED = memguard.MODULES + ('upsnet_amd.dataset.gt_prepare', 'upsnet_amd.dataset.pan_format')   # the modules that allocate here


@pytest.fixture()
def saved_config():
    from upsnet_amd.config.config import config
    saved = copy.deepcopy(dict(config))
    yield config
    config.clear()
    config.update(saved)


def _tables():
    from upsnet_amd.dataset.prepare import label_tables
    return torch.from_numpy(label_tables()).cuda()


def _run(ids, **kw):
    from upsnet_amd import ops
    out = ops.gt_prepare(torch.from_numpy(np.ascontiguousarray(ids)).cuda(), _tables(), **kw)
    torch.cuda.synchronize()
    return out


def _assert_equal(got, want, name):
    for g, w, what in zip(got, want, ('train_map', 'rgb', 'table', 'trans_off', 'trans')):
        g = g.cpu().numpy()
        assert g.dtype == w.dtype and g.shape == w.shape, (name, what, g.dtype, g.shape, w.dtype, w.shape)
        assert np.array_equal(g, w), (name, what)


@pytest.mark.parametrize('name', sorted(CASES))
def test_kernel_equals_restatement(name):
    ids, want = case(name)
    _assert_equal(_run(ids), want, name)


def test_more_values_than_the_pixel_pass_holds_in_lds():
    """64 x 64 = one workgroup of the pixel pass, 8 thing labels x 160 instance numbers = 1280 distinct live values on its 4096
    pixels: more than the 1024 slots of the workgroup's LDS table, so whatever the hash does with them at least 256 values take the
    global fallback. Capacities that refuse nothing."""
    from gt_prepare_cases import THING_LABELS
    from gt_prepare_ref import reference
    from upsnet_amd.dataset.prepare import label_tables
    values = np.array([lab * 1000 + k for lab in THING_LABELS for k in range(160)], np.int32)
    flat = values[np.arange(64 * 64) % len(values)]
    np.random.default_rng(1024).shuffle(flat)
    ids = np.ascontiguousarray(flat.reshape(64, 64))
    assert len(np.unique(ids)) == 1280 > 1024
    want = reference(ids, label_tables())
    assert want[2].shape[0] == 1280
    _assert_equal(_run(ids, seg_capacity=2048, trans_capacity=4 * 64 * 64), want, '1280 values in one workgroup')


def test_two_runs_give_identical_bytes():
    for name in ('many_instances', 'checkerboard', '37x53'):
        ids, _ = case(name)
        a, b = _run(ids), _run(ids)
        for x, y in zip(a, b):
            assert memguard.bit_equal(x, y), name


@pytest.mark.parametrize('pattern', ['A', 'B'])
@pytest.mark.parametrize('name', ['37x53', 'checkerboard', 'border_frame', 'many_instances', 'ignored_only'])
def test_guard_bands_and_every_byte_written(name, pattern):
    """Outputs and workspace come poisoned out of guard bands: equal to the restatement under both poison bytes means every byte of
    the maps, of the counted rows and of the counted lists was written; the bands must be intact on exit."""
    from upsnet_amd import ops
    ids, want = case(name)
    with memguard.poisoned(pattern, modules=GUARDED) as guard:
        dev_ids = memguard.banded_copy(torch.from_numpy(ids).cuda(), pattern)
        tables = memguard.banded_copy(_tables(), pattern)
        got = ops.gt_prepare(dev_ids, tables)
        torch.cuda.synchronize()
        assert guard.count >= 7          # workspace, two maps, table, trans_off, trans, status
        _assert_equal(got, want, name)


def test_transition_overflow_raises_and_leaves_the_workspace_clean():
    from upsnet_amd import ops
    ids, want = case('checkerboard')
    small, small_want = case('37x53')
    with memguard.poisoned('A', modules=GUARDED):
        ws = ops.gt_prepare_workspace(torch.device('cuda'))
        with pytest.raises(ValueError) as e:
            _run(ids, trans_capacity=100, workspace=ws)
        assert '%d mask transitions' % len(want[4]) in str(e.value)
        with pytest.raises(ValueError):
            _run(ids, trans_capacity=len(want[4]) - 1, workspace=ws)
        _assert_equal(_run(ids, trans_capacity=len(want[4]), workspace=ws), want, 'checkerboard at the exact capacity')
        _assert_equal(_run(small, workspace=ws), small_want, '37x53 after the overflow')


def test_segment_overflow_raises_and_leaves_the_workspace_clean():
    from upsnet_amd import ops
    ids, want = case('many_instances')
    small, small_want = case('37x53')
    assert want[2].shape[0] > 1200
    with memguard.poisoned('B', modules=GUARDED):
        ws = ops.gt_prepare_workspace(torch.device('cuda'), 1024)
        with pytest.raises(ValueError) as e:
            _run(ids, seg_capacity=1024, workspace=ws)
        assert '%d segments' % want[2].shape[0] in str(e.value)
        _assert_equal(_run(small, seg_capacity=1024, workspace=ws), small_want, '37x53 after the overflow')
        ws = ops.gt_prepare_workspace(torch.device('cuda'), want[2].shape[0])
        _assert_equal(_run(ids, seg_capacity=want[2].shape[0], workspace=ws), want, 'many_instances at the exact capacity')


def test_label_ids_cross_check():
    ids, want = case('37x53')
    labels = np.where(ids < 1000, ids, ids // 1000).astype(np.uint8)
    _assert_equal(_run(ids, label_ids=torch.from_numpy(labels).cuda()), want, 'matching labelIds')
    labels[20, 31] ^= 1
    with pytest.raises(ValueError) as e:
        _run(ids, label_ids=torch.from_numpy(labels).cuda())
    assert '1 pixels of the labelIds map' in str(e.value)


def test_values_beyond_16_bits_raise():
    ids = case('37x53')[0].copy()
    ids[3, 3] = 70000
    with pytest.raises(ValueError):
        _run(ids)
    with pytest.raises(ValueError):
        _run(ids.astype(np.int64))


@pytest.mark.parametrize('value', [256, 300, 999, -1])
def test_values_that_encode_no_label_raise(value):
    """The label tables have 256 entries: 256..999 (and a negative value) name no label, must not index them, and raise as 70000
    does -- with and without a labelIds map, as the restatement does; the next call on the same workspace is correct."""
    from upsnet_amd import ops
    from upsnet_amd.dataset.prepare import label_tables
    from gt_prepare_ref import reference
    ids, want = case('37x53')
    bad = ids.copy()
    bad[0, 0] = bad[20, 31] = bad[36, 52] = value          # a vector-path thread, the middle, the scalar tail
    with pytest.raises(ValueError):
        reference(bad, label_tables())
    labels = np.where(ids < 1000, ids, ids // 1000).astype(np.uint8)
    with memguard.poisoned('A', modules=GUARDED):
        ws = ops.gt_prepare_workspace(torch.device('cuda'))
        with pytest.raises(ValueError) as e:
            _run(bad, workspace=ws)
        assert 'encode no label' in str(e.value)
        with pytest.raises(ValueError) as e:
            _run(bad, label_ids=torch.from_numpy(labels).cuda(), workspace=ws)
        assert 'encode no label' in str(e.value)
        _assert_equal(_run(ids, workspace=ws), want, '37x53 after the refusal')


def test_preparer_runs_an_image_that_outgrows_the_default_transitions_again():
    """many_instances has more transitions than the default capacity of its size: CityscapesPreparer.finish must run it again at
    the counted size (the helper ops.gt_prepare shares), with the next image already queued on the same workspace."""
    from upsnet_amd.dataset.gt_prepare import gt_prepare_default_transitions
    from upsnet_amd.dataset.prepare import CityscapesPreparer
    ids, want = case('many_instances')
    small, small_want = case('37x53')
    assert len(want[4]) > gt_prepare_default_transitions(*ids.shape)
    with memguard.poisoned('B', modules=GUARDED):
        prep = CityscapesPreparer()
        first = prep.submit(np.ascontiguousarray(ids))
        second = prep.submit(np.ascontiguousarray(small))
        third = prep.submit(np.ascontiguousarray(ids))
        for p, w, name in ((first, want, 'many_instances'), (second, small_want, '37x53'), (third, want, 'many_instances again')):
            got = prep.finish(p)
            for g, x, what in zip(got, w, ('train_map', 'rgb', 'table', 'trans_off', 'trans')):
                assert g.dtype == x.dtype and g.shape == x.shape and np.array_equal(g, x), (name, what)


def test_semantic_converter_equals_restatement():
    from upsnet_amd import ops
    rng = np.random.default_rng(9)
    H, W = 37, 53
    seg_ids = [0, 5, 256, 65543, 1 << 20, 77]          # 0 = VOID; 65543 is not listed below
    pick = rng.integers(0, len(seg_ids), (H // 4 + 1, W // 4 + 1))
    ids = np.array(seg_ids)[np.repeat(np.repeat(pick, 4, 0), 4, 1)[:H, :W]]
    rgb = np.stack([ids % 256, ids // 256 % 256, ids // 65536], 2).astype(np.uint8)
    segments = [{'id': 1 << 20, 'category_id': 132, 'iscrowd': 0}, {'id': 5, 'category_id': 0, 'iscrowd': 0},
                {'id': 256, 'category_id': 60, 'iscrowd': 1}, {'id': 77, 'category_id': 60, 'iscrowd': 0},
                {'id': 9999, 'category_id': 3, 'iscrowd': 0}]                                          # (9999 has no pixel)
    want = semantic_reference(rgb, segments)
    assert {0, 60, 132, 255} <= set(np.unique(want).tolist())
    for pattern in ('A', 'B'):
        with memguard.poisoned(pattern, modules=GUARDED):
            got = ops.panoptic_semantic(memguard.banded_copy(torch.from_numpy(rgb).cuda(), pattern), segments)
            torch.cuda.synchronize()
            assert got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), want)
    with pytest.raises(ValueError):
        ops.panoptic_semantic(torch.from_numpy(rgb).cuda(), segments + [{'id': 5, 'category_id': 1}])


# ------------------------------------------------------------------------------------------------ round trips
def _pred_2ch(ids, tables):
    """The prediction that IS the ground truth: channel 0 the train id (VOID for ignored labels and for groups, which are crowd
    regions), channel 1 the instance number + 1 of a thing instance."""
    label = np.where(ids < 1000, ids, ids // 1000)
    cat = tables[0][label].astype(np.int64)
    group = (ids < 1000) & (tables[1][label] != 0)
    cat[group] = 255
    inst = np.where((ids >= 1000) & (cat != 255), ids % 1000 + 1, 0)
    return np.stack([cat, inst, np.zeros_like(cat)], 2).astype(np.uint8)


def test_cityscapes_round_trip(tmp_path, saved_config):
    from upsnet_amd.config.config import update_config
    from upsnet_amd.dataset import Cityscapes
    from upsnet_amd.dataset.prepare import label_tables
    from upsnet_amd.prepare import main
    root = str(tmp_path / 'cityscapes')
    scenes = [e2e_scene(k) for k in range(3)]
    bases = make_raw_cityscapes(root, scenes)
    raw = sorted(os.path.join(d, f) for d, _, fs in os.walk(root) for f in fs)
    assert main(['--dataset', 'cityscapes', '--root', root]) == {'val': 3}
    assert [p for p in raw if not os.path.isfile(p)] == []                      # the download is untouched ...
    assert sorted(os.listdir(root)) == ['annotations', 'gtFine', 'images', 'labels', 'leftImg8bit', 'panoptic']
    with pytest.raises(FileExistsError):
        main(['--dataset', 'cityscapes', '--root', root])
    update_config(write_cfg(tmp_path, 'Cityscapes', root, 'val'))
    ds = Cityscapes(image_sets=['val'], phase='test')
    ds.check_files()
    ds.check_instance_files()
    order = sorted(range(3), key=lambda k: bases[k])                            # image ids 1..3 follow the sorted base names
    assert [e['file_name'] for e in ds.roidb] == [bases[k] + '_leftImg8bit.png' for k in order]
    assert [e['id'] for e in ds.roidb] == [1, 2, 3] and os.path.islink(ds.roidb[0]['image'])
    scenes = [scenes[k] for k in order]
    tables = label_tables()
    out = str(tmp_path / 'out')
    os.makedirs(out)

    assert ds.panoptic_order() == [0, 1, 2]
    pq = ds.evaluate_panoptic([torch.from_numpy(_pred_2ch(s, tables)).cuda() for s in scenes], out)
    scored = [c for c, r in pq['per_class'].items() if 'tp' in r]
    assert set(scored) == {0, 1, 2, 8, 10, 11, 13, 15, 18}
    for c in scored:
        r = pq['per_class'][c]
        assert r['pq'] == 1.0 and r['sq'] == 1.0 and r['rq'] == 1.0 and r['fp'] == 0 and r['fn'] == 0, (c, r)

    train = [tables[0][np.where(s < 1000, s, s // 1000)].astype(np.uint8) for s in scenes]
    ss = ds.evaluate_ssegs(train, out)
    present = sorted(set(np.concatenate([t.ravel() for t in train]).tolist()) - {255})
    assert present == scored and all(ss['IU_array'][c] == 1.0 for c in present)

    with open(ds.instances_json_file) as f:
        inst = json.load(f)
    assert [c['id'] for c in inst['categories']] == list(range(1, 9))
    all_boxes = [[]] + [[np.zeros((0, 5), np.float32) for _ in range(3)] for _ in range(8)]
    all_segms = [[]] + [[[] for _ in range(3)] for _ in range(8)]
    for a in inst['annotations']:
        x, y, w, h = a['bbox']
        i, c = a['image_id'] - 1, a['category_id']
        all_boxes[c][i] = np.vstack([all_boxes[c][i], np.array([[x, y, x + w - 1, y + h - 1, 1.0]], np.float32)])
        all_segms[c][i].append(a['segmentation'])
    assert len(inst['annotations']) == 13 and sorted(set(a['category_id'] for a in inst['annotations'])) == [1, 3, 5, 8]
    box = ds.evaluate_boxes(all_boxes, out)
    assert box[0] == 1.0 and box[1] == 1.0
    mask = ds.evaluate_masks(all_boxes, all_segms, out)
    assert mask.stats[0] == 1.0 and mask.stats[1] == 1.0
    res = ds.evaluate_instances(all_boxes, all_segms, out)
    for name in ('person', 'car', 'bus', 'bicycle'):
        assert res['per_class'][name] == {'ap': 1.0, 'ap50': 1.0}, (name, res['per_class'][name])
    assert res['AP'] == 1.0 and res['AP50'] == 1.0


def test_coco_round_trip(tmp_path, saved_config):
    from PIL import Image
    from upsnet_amd.config.config import update_config
    from upsnet_amd.dataset import coco
    from upsnet_amd.prepare import main
    root = str(tmp_path / 'coco')
    sizes, image_ids = [(40, 60), (37, 53), (48, 64)], [139, 5, 77]
    make_dataset(root, 'coco', sizes, ids=image_ids)
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'coco_stff.json')) as f:
        cats = json.load(f)['inputs']['val']['categories']
    rng = np.random.default_rng(4)
    os.makedirs(os.path.join(root, 'annotations', 'panoptic_val2017'))
    images, anns, truth = [], [], {}
    for (H, W), i in zip(sizes, image_ids):
        n = 9
        pick = rng.integers(0, n, (H // 8 + 1, W // 8 + 1))
        seg_map = np.repeat(np.repeat(pick, 8, 0), 8, 1)[:H, :W]                  # value 0 = VOID
        seg_ids = np.concatenate([[0], rng.choice(np.arange(1, 1 << 24), n - 1, replace=False)])
        positions = rng.choice(133, n - 1, replace=False)                           # things and stuff, by list position
        ids = seg_ids[seg_map]
        Image.fromarray(np.stack([ids % 256, ids // 256 % 256, ids // 65536], 2).astype(np.uint8)).save(
            os.path.join(root, 'annotations', 'panoptic_val2017', '%012d.png' % i))
        segs = [{'id': int(seg_ids[k]), 'category_id': cats[positions[k - 1]]['id'], 'iscrowd': int(k == 3), 'area': int((seg_map == k).sum()),
                 'bbox': [0, 0, 1, 1]} for k in range(1, n) if (seg_map == k).any()]
        images.append({'id': i, 'file_name': '%012d.jpg' % i, 'height': H, 'width': W})
        anns.append({'image_id': i, 'file_name': '%012d.png' % i, 'segments_info': segs})
        new_cat = np.array([255] + [p + 53 if p < 80 else p - 80 for p in positions])
        truth[i] = (seg_map, new_cat, np.array([0] + [int(k == 3) for k in range(1, n)]))
    anns.sort(key=lambda a: a['image_id'])      # (as in the download: annotations by ascending id, which the sorted image list meets)
    with open(os.path.join(root, 'annotations', 'panoptic_val2017.json'), 'w') as f:
        json.dump({'images': images, 'annotations': anns, 'categories': cats}, f)
    assert main(['--dataset', 'coco', '--root', root]) == {'val2017': 3}
    with pytest.raises(FileExistsError):
        main(['--dataset', 'coco', '--root', root])
    update_config(write_cfg(tmp_path, 'coco', root, 'val2017'))
    saved_config.dataset.num_seg_classes = 133
    ds = coco(image_sets=['val2017'], phase='test')
    ds.check_files()
    assert [e['id'] for e in ds.roidb] == sorted(image_ids)
    with open(ds.panoptic_json_file) as f:
        stff = json.load(f)
    assert [im['id'] for im in stff['images']] == sorted(image_ids) and [a['image_id'] for a in stff['annotations']] == sorted(image_ids)
    sem = [truth[e['id']][1][truth[e['id']][0]].astype(np.uint8) for e in ds.roidb]
    for e, want in zip(ds.roidb, sem):
        assert np.array_equal(np.array(Image.open(ds.seg_gt_path(e))), want)
    ss = ds.evaluate_ssegs(sem, str(tmp_path))
    present = sorted(set(np.concatenate([s.ravel() for s in sem]).tolist()) - {255})
    assert len(present) > 10 and all(ss['IU_array'][c] == 1.0 for c in present)
    preds = []
    for k in ds.panoptic_order():                                                   # one prediction per annotation, in its order
        seg_map, new_cat, crowd = truth[ds.roidb[k]['id']]
        cat = np.where(crowd[seg_map] == 1, 255, new_cat[seg_map])
        inst = np.where(cat == 255, 0, seg_map)                                     # segments of one category stay apart
        preds.append(torch.from_numpy(np.stack([cat, inst, np.zeros_like(cat)], 2).astype(np.uint8)).cuda())
    assert ds.panoptic_order() == [0, 1, 2]
    pq = ds.evaluate_panoptic(preds, str(tmp_path))
    scored = [c for c, r in pq['per_class'].items() if 'tp' in r]
    assert len(scored) > 10
    for c in scored:
        r = pq['per_class'][c]
        assert r['pq'] == 1.0 and r['sq'] == 1.0 and r['rq'] == 1.0, (c, r)
