"""CPU: the ground-truth preparation (dataset/prepare.py) without a device -- the numpy restatement against
hand-written expectations for one literal map, the JSON writers fed with restatement output, the command line's refusals (all made
before any launch), and the COCO stuff-first remap against what the reference's own init_coco.py wrote (tests/golden/coco_stff.json,
made by tests/golden/make_golden_coco_stff.py)."""
import copy
import json
import os

import numpy as np
import pytest

from conftest import ROOT  # noqa: F401  (puts the repo root on sys.path)
from gt_prepare_cases import LITERAL, case
from gt_prepare_ref import reference, semantic_reference


def test_label_tables():
    from upsnet_amd.dataset.prepare import label_tables
    t = label_tables()
    assert t.shape == (3, 256) and t.dtype == np.int32
    assert [int(t[0, l]) for l in (7, 8, 11, 23, 24, 26, 33)] == [0, 1, 2, 10, 11, 13, 18]
    assert all(t[0, l] == 255 for l in (0, 1, 2, 3, 4, 5, 6, 9, 10, 14, 15, 16, 18, 29, 30)) and (t[0, 34:] == 255).all()
    assert np.flatnonzero(t[0] != 255).size == 19
    assert np.flatnonzero(t[1]).tolist() == list(range(24, 34))
    assert [int(t[2, l]) for l in (24, 25, 26, 27, 28, 31, 32, 33)] == list(range(8)) and np.flatnonzero(t[2] >= 0).size == 8


def test_restatement_on_the_literal_map():
    """4 x 6: road (7), unlabeled (0), a car group (v = 26), the cars 26000 and 26001 (with a hole of road), a caravan (29000)."""
    from upsnet_amd.dataset.prepare import label_tables
    train, rgb, rows, trans_off, trans = reference(LITERAL, label_tables())
    assert train.dtype == np.uint8 and train.tolist() == [[0, 0, 13, 13, 13, 255],
                                                           [0, 13, 13, 0, 13, 255],
                                                           [13, 13, 13, 13, 13, 255],
                                                           [13, 0, 0, 0, 0, 255]]
    road, grp, car0, car1, void = [7, 0, 0], [26, 0, 0], [144, 101, 0], [145, 101, 0], [0, 0, 0]     # 26000 = 144 + 256 * 101
    assert rgb.dtype == np.uint8 and rgb.tolist() == [[road, road, car1, car1, car1, void],
                                                       [road, car0, car1, road, car1, void],
                                                       [grp, car0, car1, car1, car1, void],
                                                       [grp, road, road, road, road, void]]
    # v, label, train id, iscrowd, area, x_min, y_min, x_max, y_max -- ascending v; 0 and the caravan are no segments
    assert rows.dtype == np.int32 and rows.tolist() == [[7, 7, 0, 0, 8, 0, 0, 4, 3],
                                                         [26, 26, 13, 1, 2, 0, 2, 0, 3],
                                                         [26000, 26, 13, 0, 2, 1, 1, 1, 2],
                                                         [26001, 26, 13, 0, 8, 2, 0, 4, 2]]
    # column-major positions x * 4 + y: 26000 covers 5..6; 26001 covers 8..10, 12, 14, 16..18
    assert trans_off.tolist() == [0, 2, 10]
    assert trans.tolist() == [5, 7, 8, 11, 12, 13, 14, 15, 16, 19]


@pytest.mark.parametrize('name', ['literal', '37x53', 'border_frame', 'hole_two_components', 'groups_and_caravans', '1xW', 'Hx1'])
def test_json_writers(name):
    from upsnet_amd.dataset.prepare import (instance_annotations, instance_categories, instance_rows, label_tables, panoptic_categories,
                                            panoptic_segments)
    from upsnet_amd.dataset.cityscapes_eval import CLASS_LABEL_IDS, CLASS_NAMES
    from upsnet_amd.dataset.rle import decode_rle_strings
    ids, (train, rgb, rows, trans_off, trans) = case(name)
    H, W = ids.shape
    segs = panoptic_segments(rows)
    assert [s['id'] for s in segs] == sorted(set(v for v in ids.ravel().tolist() if label_tables()[0][v if v < 1000 else v // 1000] != 255))
    for s, r in zip(segs, rows.tolist()):
        assert list(s) == ['id', 'category_id', 'area', 'bbox', 'iscrowd']
        m = ids == s['id']
        ys, xs = np.nonzero(m)
        assert s['area'] == int(m.sum()) and s['category_id'] == r[2] and s['iscrowd'] == int(s['id'] < 1000 and r[1] >= 24)
        assert s['bbox'] == [xs.min(), ys.min(), xs.max() - xs.min() + 1, ys.max() - ys.min() + 1]
        assert all(type(v) is int for v in s['bbox'] + [s['id'], s['area'], s['category_id'], s['iscrowd']])
    anns = instance_annotations(5, rows, trans_off, trans, H, W, first_id=11)
    inst = instance_rows(rows)
    assert [r[0] for r in inst] == [v for v in sorted(set(ids.ravel().tolist())) if v >= 1000 and v // 1000 in CLASS_LABEL_IDS]
    assert [a['id'] for a in anns] == list(range(11, 11 + len(inst)))
    if anns:
        counts, off = decode_rle_strings([a['segmentation']['counts'] for a in anns])
    for j, (a, r) in enumerate(zip(anns, inst)):
        assert list(a) == ['id', 'image_id', 'category_id', 'iscrowd', 'area', 'bbox', 'segmentation']
        m = ids == r[0]
        ys, xs = np.nonzero(m)
        assert a['image_id'] == 5 and a['iscrowd'] == 0 and a['area'] == int(m.sum())
        assert a['category_id'] == CLASS_LABEL_IDS.index(r[1]) + 1
        assert a['bbox'] == [float(xs.min()), float(ys.min()), float(xs.max() - xs.min() + 1), float(ys.max() - ys.min() + 1)]
        assert all(type(v) is float for v in a['bbox'])
        assert a['segmentation']['size'] == [H, W]
        c = counts[off[j]:off[j + 1]]
        assert c.sum() == H * W
        decoded = np.repeat(np.arange(len(c)) % 2, c).astype(bool).reshape(W, H).T       # column-major runs, starting with zeros
        assert np.array_equal(decoded, m)
    json.dumps({'a': anns, 's': segs})                                                    # plain Python numbers throughout
    cats = panoptic_categories()
    assert [c['id'] for c in cats] == list(range(19)) and [c['isthing'] for c in cats] == [0] * 11 + [1] * 8
    assert cats[0] == {'id': 0, 'name': 'road', 'color': [128, 64, 128], 'supercategory': 'flat', 'isthing': 0}
    assert cats[13] == {'id': 13, 'name': 'car', 'color': [0, 0, 142], 'supercategory': 'vehicle', 'isthing': 1}
    assert instance_categories() == [{'id': i + 1, 'name': n} for i, n in enumerate(CLASS_NAMES)]


def test_semantic_restatement():
    rgb = np.zeros((2, 3, 3), np.uint8)
    rgb[0, 0] = (5, 0, 0)
    rgb[0, 1] = (0, 1, 0)          # id 256: a crowd segment
    rgb[0, 2] = (7, 0, 1)          # id 65543: not listed
    rgb[1, 0] = (5, 0, 0)
    got = semantic_reference(rgb, [{'id': 5, 'category_id': 17, 'iscrowd': 0}, {'id': 256, 'category_id': 60, 'iscrowd': 1}])
    assert got.tolist() == [[17, 60, 255], [17, 255, 255]]


# ------------------------------------------------------------------------------------------------ command line refusals
def make_raw_cityscapes(root, scenes, split='val', label_ids=True, images=True):
    """A raw download: gtFine/<split>/<city>/<base>_gtFine_{instanceIds,labelIds}.png and leftImg8bit/<split>/<city>/
    <base>_leftImg8bit.png. Returns the base names in the order given (deliberately not sorted)."""
    from PIL import Image
    rng = np.random.default_rng(3)
    bases = []
    for k, ids in enumerate(scenes):
        city = ('munster', 'aachen', 'bonn')[k % 3]
        base = '%s_%06d_000019' % (city, 7 * k)
        bases.append(base)
        d = os.path.join(root, 'gtFine', split, city)
        os.makedirs(d, exist_ok=True)
        Image.fromarray(ids.astype(np.uint16)).save(os.path.join(d, base + '_gtFine_instanceIds.png'))
        if label_ids:
            Image.fromarray(np.where(ids < 1000, ids, ids // 1000).astype(np.uint8)).save(os.path.join(d, base + '_gtFine_labelIds.png'))
        if images:
            d = os.path.join(root, 'leftImg8bit', split, city)
            os.makedirs(d, exist_ok=True)
            Image.fromarray(rng.integers(0, 256, ids.shape + (3,)).astype(np.uint8)).save(os.path.join(d, base + '_leftImg8bit.png'))
    return bases


def _no_launch(monkeypatch):
    import upsnet_amd.dataset.prepare as prepare

    def refuse(*a, **k):
        raise AssertionError('the device was touched before the file checks')
    monkeypatch.setattr(prepare, 'CityscapesPreparer', refuse)


def test_cli_refuses_existing_output(tmp_path, monkeypatch):
    from upsnet_amd.prepare import main
    _no_launch(monkeypatch)
    root = str(tmp_path)
    bases = make_raw_cityscapes(root, [LITERAL, LITERAL])
    os.makedirs(os.path.join(root, 'labels'))
    existing = os.path.join(root, 'labels', sorted(bases)[1] + '_gtFine_labelTrainIds.png')
    open(existing, 'w').close()
    with pytest.raises(FileExistsError) as e:
        main(['--dataset', 'cityscapes', '--root', root])
    assert existing in str(e.value)
    os.remove(existing)
    os.makedirs(os.path.join(root, 'annotations'))
    existing = os.path.join(root, 'annotations', 'instancesonly_gtFine_val.json')
    open(existing, 'w').close()
    with pytest.raises(FileExistsError) as e:
        main(['--dataset', 'cityscapes', '--root', root, '--images', 'none'])
    assert existing in str(e.value)
    with pytest.raises(AssertionError):            # --force passes the checks and reaches the device part
        main(['--dataset', 'cityscapes', '--root', root, '--force'])
    assert os.path.getsize(existing) == 0          # ... which, refused here, had written nothing yet


def test_cli_names_a_missing_image(tmp_path, monkeypatch):
    from upsnet_amd.prepare import main
    _no_launch(monkeypatch)
    root = str(tmp_path)
    bases = make_raw_cityscapes(root, [LITERAL, LITERAL])
    gone = os.path.join(root, 'leftImg8bit', 'val', bases[1].split('_')[0], bases[1] + '_leftImg8bit.png')
    os.remove(gone)
    with pytest.raises(FileNotFoundError) as e:
        main(['--dataset', 'cityscapes', '--root', root])
    assert gone in str(e.value)
    with pytest.raises(AssertionError):            # without images/ the file is not needed
        main(['--dataset', 'cityscapes', '--root', root, '--images', 'none'])
    with pytest.raises(FileNotFoundError):         # a split that is in neither folder
        main(['--dataset', 'cityscapes', '--root', root, '--splits', 'train'])


def test_cli_unknown_dataset(tmp_path, capsys):
    from upsnet_amd.prepare import main
    with pytest.raises(SystemExit) as e:
        main(['--dataset', 'ade20k', '--root', str(tmp_path)])
    assert e.value.code != 0 and 'ade20k' in capsys.readouterr().err
    from upsnet_amd.dataset.prepare import prepare_cityscapes
    with pytest.raises(ValueError):
        prepare_cityscapes(str(tmp_path), images='move')


def test_image_info_for_a_split_without_gtfine(tmp_path):
    """test: the image list alone, from leftImg8bit; no device work."""
    from PIL import Image
    from upsnet_amd.prepare import main
    root = str(tmp_path)
    for city, base, size in (('berlin', 'berlin_000002_000019', (12, 8)), ('bielefeld', 'bielefeld_000000_000321', (10, 6))):
        d = os.path.join(root, 'leftImg8bit', 'test', city)
        os.makedirs(d)
        Image.new('RGB', size).save(os.path.join(d, base + '_leftImg8bit.png'))
    assert main(['--dataset', 'cityscapes', '--root', root, '--splits', 'test', '--images', 'copy']) == {'test': 2}
    with open(os.path.join(root, 'annotations', 'image_info_test.json')) as f:
        js = json.load(f)
    assert js['images'] == [{'id': 1, 'file_name': 'berlin_000002_000019_leftImg8bit.png', 'height': 8, 'width': 12},
                            {'id': 2, 'file_name': 'bielefeld_000000_000321_leftImg8bit.png', 'height': 6, 'width': 10}]
    assert sorted(os.listdir(os.path.join(root, 'images'))) == [im['file_name'] for im in js['images']]
    assert not os.path.islink(os.path.join(root, 'images', js['images'][0]['file_name']))
    with pytest.raises(FileExistsError):
        main(['--dataset', 'cityscapes', '--root', root, '--splits', 'test'])


# ------------------------------------------------------------------------------------------------ COCO remap, pinned to the reference
def _golden():
    with open(os.path.join(ROOT, 'tests', 'golden', 'coco_stff.json')) as f:
        return json.load(f)


@pytest.mark.parametrize('split', ['train', 'val'])
def test_coco_remap_matches_the_reference(split):
    from upsnet_amd.dataset.prepare import coco_stff_remap
    g = _golden()
    src, want = g['inputs'][split], g['expected'][split]
    before = copy.deepcopy(src)
    cats, out = coco_stff_remap(src, sort_images=split == 'val')
    assert src == before
    assert cats == g['expected']['categories'] and out['categories'] == cats and want['categories_equal_table']
    assert [c['id'] for c in cats] == list(range(133)) and [c['isthing'] for c in cats] == [0] * 53 + [1] * 80
    assert [im['id'] for im in out['images']] == want['image_ids']
    assert [im['file_name'] for im in out['images']] == want['file_names']
    assert [a['image_id'] for a in out['annotations']] == want['annotation_image_ids']
    assert [[[s['id'], s['category_id']] for s in a['segments_info']] for a in out['annotations']] == want['segment_categories']
    assert out['info'] == src['info']


def test_coco_remap_refuses_another_table():
    from upsnet_amd.dataset.prepare import coco_stff_remap
    src = _golden()['inputs']['val']
    bad = copy.deepcopy(src)
    bad['categories'] = bad['categories'][:-1]
    with pytest.raises(ValueError):
        coco_stff_remap(bad, True)
    bad = copy.deepcopy(src)
    bad['categories'][3]['isthing'] = 0
    with pytest.raises(ValueError):
        coco_stff_remap(bad, True)
