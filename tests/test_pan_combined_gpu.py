"""GPU: the combined panoptic merge on the device (csrc/pan_combine.hip through BaseDataset.get_combined_pan_result) bit for bit against
the reference's fixture, the hand-derived cases and the numpy restatement (tests/test_pan_combined_cpu.py), at 1024 x 2048 and over
chunked calls; its input checks before any launch; and `python -m upsnet_amd.evaluate --eval_only --pan_combined` end to end."""
import copy
import json
import os

import numpy as np
import pytest
import torch

from test_pan_combined_cpu import ID_LAST_STUFF, NUM_CLASSES, encode_mask, hand_cases, load_golden, restate_combined

pytestmark = pytest.mark.gpu


@pytest.fixture()
def cityscapes_config():
    from upsnet_amd.config.config import config
    saved = copy.deepcopy(dict(config))
    config.dataset.num_classes, config.dataset.num_seg_classes = NUM_CLASSES, ID_LAST_STUFF + NUM_CLASSES
    yield config
    config.clear()
    config.update(saved)


def combined(*a, **k):
    from upsnet_amd.dataset.base_dataset import BaseDataset
    return [t.cpu().numpy() for t in BaseDataset().get_combined_pan_result(*a, **k)]


def scene(rng, h, w, n, nc=NUM_CLASSES, full_width=True):
    """A random scene: blocky semantic map with stuff and thing labels; n detections with realistic box sizes, heavy overlap
    (jittered copies) and a few full-width masks; scores spread across the threshold (ties included)."""
    sem = rng.integers(0, ID_LAST_STUFF + nc, (h // 16 + 1, w // 16 + 1)).repeat(16, 0).repeat(16, 1)[:h, :w].astype(np.uint8)
    boxes = [[]] + [[np.zeros((0, 5), np.float32)] for _ in range(1, nc)]
    masks = [[]] + [[[]] for _ in range(1, nc)]
    scores = np.round(rng.uniform(0.3, 1.0, n), 2).astype(np.float32)
    prev = []
    for d in range(n):
        m = np.zeros((h, w), bool)
        if full_width and d % 25 == 7:
            y0 = int(rng.integers(0, h - 8))
            m[y0:y0 + int(rng.integers(1, h - y0)), :] = True
        elif prev and d % 3 == 1:
            py0, py1, px0, px1 = prev[int(rng.integers(0, len(prev)))]
            dy, dx = int(rng.integers(-4, 5)), int(rng.integers(-4, 5))
            m[max(py0 + dy, 0):max(py1 + dy, 1), max(px0 + dx, 0):max(px1 + dx, 1)] = True
        else:
            bh, bw = (int(v) for v in np.exp(rng.uniform(np.log(8), np.log(max(h, w, 24) / 3), 2)))
            y0, x0 = int(rng.integers(0, max(h - bh, 1))), int(rng.integers(0, max(w - bw, 1)))
            prev.append((y0, y0 + bh, x0, x0 + bw))
            m[y0:y0 + bh, x0:x0 + bw] = True
            if d % 2:   # an ellipse inside the box
                yy, xx = np.ogrid[0:h, 0:w]
                m &= ((yy - y0 - bh / 2) / (bh / 2 + 1e-3)) ** 2 + ((xx - x0 - bw / 2) / (bw / 2 + 1e-3)) ** 2 <= 1
        c = int(rng.integers(1, nc))
        boxes[c][0] = np.vstack([boxes[c][0], np.array([[0, 0, w - 1, h - 1, scores[d]]], np.float32)])
        masks[c][0].append(encode_mask(m))
    return sem, boxes, masks


def join(scenes):
    """Per-image (seg, boxes, masks) -> segs, boxes[c][i], masks[c][i]."""
    nc = len(scenes[0][1])
    return ([s[0] for s in scenes], [[]] + [[s[1][c][0] for s in scenes] for c in range(1, nc)],
            [[]] + [[s[2][c][0] for s in scenes] for c in range(1, nc)])


def test_golden(cityscapes_config):
    for segs, boxes, masks, limit, want in load_golden():
        got = combined(segs, boxes, masks, stuff_area_limit=limit)
        assert len(got) == 1 and got[0].dtype == np.uint8 and np.array_equal(got[0], want)


def test_hand_derived_cases(cityscapes_config):
    for name, (segs, boxes, masks, kw, want) in sorted(hand_cases().items()):
        got = combined(segs, boxes, masks, **kw)
        for g, e in zip(got, want):
            assert np.array_equal(g, e), name


def test_full_resolution_scenes(cityscapes_config):
    rng = np.random.default_rng(41)
    scenes = [scene(rng, 1024, 2048, 100) for _ in range(2)]
    segs, boxes, masks = join(scenes)
    before = copy.deepcopy((segs, boxes, masks))
    got = combined(segs, boxes, masks)
    want = restate_combined(segs, boxes, masks)
    for g, e in zip(got, want):
        assert g.shape == (1024, 2048, 3) and np.array_equal(g, e)
        assert len(np.unique(g[:, :, 1])) > 3
    # inputs unchanged
    for a, b in zip(segs, before[0]):
        assert np.array_equal(a, b)
    for c in range(1, NUM_CLASSES):
        for a, b in zip(boxes[c], before[1][c]):
            assert np.array_equal(a, b)
        assert masks[c] == before[2][c]


def test_ragged_empty_and_input_kinds(cityscapes_config):
    rng = np.random.default_rng(42)
    parts = [scene(rng, 37, 53, 20), scene(rng, 128, 300, 40), scene(rng, 64, 64, 0), scene(rng, 90, 31, 15), scene(rng, 200, 100, 30)]
    # all below the threshold in image 3
    for c in range(1, NUM_CLASSES):
        b = parts[3][1][c][0]
        b[:, 4] = np.minimum(b[:, 4], np.float32(0.59))
    segs, boxes, masks = join(parts)
    want = restate_combined(segs, boxes, masks, stuff_area_limit=50)
    assert not want[2][:, :, 1].any() and not want[3][:, :, 1].any()
    kinds = [lambda s: s, lambda s: s.astype(np.int64), lambda s: torch.from_numpy(s).cuda(),
             lambda s: torch.from_numpy(s.astype(np.int64)).cuda()]
    for kind in kinds:
        in_segs = [kind(s) for s in segs]
        snap = [s.clone() if isinstance(s, torch.Tensor) else s.copy() for s in in_segs]
        got = combined(in_segs, boxes, masks, stuff_area_limit=50)
        for g, e in zip(got, want):
            assert np.array_equal(g, e)
        for s, t in zip(in_segs, snap):
            assert (torch.equal(s, t) if isinstance(s, torch.Tensor) else np.array_equal(s, t))
    # mixed kinds in one call
    got = combined([kinds[k % 4](s) for k, s in enumerate(segs)], boxes, masks, stuff_area_limit=50)
    assert all(np.array_equal(g, e) for g, e in zip(got, want))
    assert combined([], [[]] + [[] for _ in range(1, NUM_CLASSES)], [[]] + [[] for _ in range(1, NUM_CLASSES)]) == []


def test_many_images_cross_the_chunk_bound(cityscapes_config):
    from upsnet_amd import ops
    rng = np.random.default_rng(43)
    n = 300
    assert n > ops.COMBINED_PAN_CHUNK_IMAGES
    parts = [scene(rng, int(rng.integers(16, 48)), int(rng.integers(16, 64)), int(rng.integers(0, 12)), full_width=False) for _ in range(n)]
    segs, boxes, masks = join(parts)
    got = combined(segs, boxes, masks, stuff_area_limit=40)
    want = restate_combined(segs, boxes, masks, stuff_area_limit=40)
    assert len(got) == n
    for g, e in zip(got, want):
        assert np.array_equal(g, e)


def test_value_errors_before_any_launch(cityscapes_config, monkeypatch):
    from upsnet_amd import ops

    def no_launch(*a, **k):
        raise AssertionError('launched')
    monkeypatch.setattr(ops, 'lib', no_launch)
    rng = np.random.default_rng(44)
    seg, boxes, masks = scene(rng, 32, 48, 6)
    segs, boxes, masks = join([(seg, boxes, masks)])
    cases = []
    # mask size differs from the seg map
    m2 = copy.deepcopy(masks)
    c = next(c for c in range(1, NUM_CLASSES) if m2[c][0])
    m2[c][0][0] = dict(m2[c][0][0], size=[32, 47])
    cases.append((segs, boxes, m2))
    # boxes / masks lengths differ
    m3 = copy.deepcopy(masks)
    m3[c][0] = m3[c][0][1:]
    cases.append((segs, boxes, m3))
    cases.append((segs, boxes, masks[:-1]))
    # counts do not sum to H * W
    m4 = copy.deepcopy(masks)
    m4[c][0][0] = encode_mask(np.ones((32, 47), bool))
    m4[c][0][0]['size'] = [32, 48]
    b4 = copy.deepcopy(boxes)
    b4[c][0][0, 4] = 0.99
    cases.append((segs, b4, m4))
    # more than 255 candidates of one class at or above the threshold
    b5 = copy.deepcopy(boxes)
    m5 = copy.deepcopy(masks)
    b5[1][0] = np.tile(np.array([[0, 0, 1, 1, 0.9]], np.float32), (256, 1))
    m5[1][0] = [encode_mask(np.zeros((32, 48), bool))] * 256
    cases.append((segs, b5, m5))
    # more than 2^24 pixels
    big = [np.zeros((4097, 4096), np.uint8)]
    cases.append((big, [[]] + [[np.zeros((0, 5), np.float32)] for _ in range(1, NUM_CLASSES)], [[]] + [[[]] for _ in range(1, NUM_CLASSES)]))
    # labels outside 0..255
    cases.append(([seg.astype(np.int64) + 250], boxes, masks))
    for k, (s, b, m) in enumerate(cases):
        with pytest.raises(ValueError):
            combined(s, b, m)
    # 255 candidates of a class are fine up to the launch
    b5[1][0], m5[1][0] = b5[1][0][:255], m5[1][0][:255]
    with pytest.raises(AssertionError, match='launched'):
        combined(segs, b5, m5)


# ------------------------------------------------------------------------------------------------ end to end
def test_evaluate_pan_combined_end_to_end(tmp_path, cityscapes_config):
    from PIL import Image
    from test_dataset_run_cpu import make_dataset, write_cfg
    from upsnet_amd.config.config import update_config
    from upsnet_amd.dataset import Cityscapes
    from upsnet_amd.evaluate import main
    root = str(tmp_path / 'cs')
    sizes = [(256, 512), (256, 512), (128, 256)]
    make_dataset(root, 'Cityscapes', sizes, seed=5)
    cfg = write_cfg(tmp_path, 'Cityscapes', root, 'val', extra='  panoptic_stuff_area_limit: 64\n')
    update_config(cfg)
    ds = Cityscapes(image_sets=['val'], phase='test')
    # GT: random label maps / panoptic segments (PQ only has to be computed the same way twice)
    rng = np.random.default_rng(9)
    os.makedirs(ds.panoptic_gt_folder, exist_ok=True)
    imgs, anns = [], []
    for e in ds.roidb:
        h, w = e['height'], e['width']
        sem = rng.integers(0, 19, (h // 32 + 1, w // 32 + 1)).repeat(32, 0).repeat(32, 1)[:h, :w].astype(np.uint8)
        os.makedirs(os.path.dirname(ds.seg_gt_path(e)), exist_ok=True)
        Image.fromarray(sem).save(ds.seg_gt_path(e))
        ids = sem.astype(np.int64) * 256 + 1
        rgb = np.stack([ids % 256, ids // 256 % 256, ids // 65536], 2).astype(np.uint8)
        name = 'pan_%d.png' % e['id']
        Image.fromarray(rgb).save(os.path.join(ds.panoptic_gt_folder, name))
        u, cnt = np.unique(ids, return_counts=True)
        segs = [{'id': int(i), 'category_id': int(i // 256), 'iscrowd': 0, 'area': int(c)} for i, c in zip(u, cnt)]
        imgs.append({'id': 'img_%d' % e['id'], 'file_name': name})
        anns.append({'image_id': 'img_%d' % e['id'], 'file_name': name, 'segments_info': segs})
    with open(ds.panoptic_json_file, 'w') as f:
        json.dump({'images': imgs, 'annotations': anns, 'categories': [{'id': c, 'name': 'c%d' % c, 'isthing': int(c > ID_LAST_STUFF)}
                                                                        for c in range(19)]}, f)

    first = main(['--cfg', cfg, '--synthetic_weights', '--pan_combined'])
    plain = main(['--cfg', cfg, '--eval_only'])
    again = main(['--cfg', cfg, '--eval_only', '--pan_combined'])
    assert set(plain['metrics']) == {'box_ap', 'mask_ap', 'panoptic', 'sseg'}
    assert set(again['metrics']) == set(plain['metrics']) | {'panoptic_combined'}
    assert again['metrics']['panoptic'] == plain['metrics']['panoptic']
    import pickle
    with open(again['results_file'], 'rb') as f:
        res = pickle.load(f)
    order = ds.panoptic_order()
    pans = restate_combined([res['all_ssegs'][k] for k in order],
                            [[b[k] for k in order] if c else b for c, b in enumerate(res['all_boxes'])],
                            [[m[k] for k in order] if c else m for c, m in enumerate(res['all_masks'])], stuff_area_limit=64)
    want = ds.evaluate_panoptic(pans, str(tmp_path))
    assert again['metrics']['panoptic_combined'] == want
    assert first['metrics']['panoptic_combined'] == want
