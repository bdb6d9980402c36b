"""GPU: the polygon rasteriser (csrc/poly_raster.hip via dataset/polygon.py) against the literal CPU restatement of pycocotools'
rleFrPoly + merge in tests/polygon_ref.py. Every comparison is exact equality of change positions, offsets or counts: there is no
tolerance anywhere in this feature."""
import json
import os
import time

import numpy as np
import pytest
import torch

import memguard
import polygon_cases as C
import polygon_ref as R

pytestmark = pytest.mark.gpu


def device_lists(objects, h, w):
    from upsnet_amd.dataset.polygon import rasterize_polygons
    r = rasterize_polygons(objects, h, w)
    return [t.tolist() for t in r.transitions()]


def check_handle(r, total_points):
    """trans_off starts at 0, is monotone and ends inside the buffer; every position is in [0, h * w) and each list ascends strictly."""
    off = r.trans_off.cpu().numpy()
    assert off[0] == 0 and np.all(np.diff(off) >= 0) and off[-1] <= max(total_points, 1)
    for t in r.transitions():
        assert np.all(t >= 0) and np.all(t < r.height * r.width) and np.all(np.diff(t) > 0)


# ------------------------------------------------------------------------------------------------------------------ hand-derived
def test_hand_derived_cases():
    from upsnet_amd.dataset.polygon import polygons_to_rle
    h, w = C.H0, C.W0
    assert polygons_to_rle([C.RECT], h, w) == {'size': [h, w], 'counts': C.RECT_COUNTS}
    got = polygons_to_rle([C.TRIANGLE], h, w)
    assert np.array_equal(R.counts_to_mask(got['counts'], h, w), C.TRIANGLE_MASK)
    for rect in C.BORDER_RECTS:
        want = C.rect_mask(*rect, h, w)
        base = C.rect_poly(*rect)
        for poly in C.rotations_and_reversal(base) + [C.repeat_vertex(base, j) for j in range(4)]:
            got = polygons_to_rle([poly], h, w)
            assert sum(got['counts']) == h * w
            assert np.array_equal(R.counts_to_mask(got['counts'], h, w), want), (rect, poly)
    for poly in C.rotations_and_reversal(C.TRIANGLE) + [C.repeat_vertex(C.TRIANGLE, 1)]:
        assert np.array_equal(R.counts_to_mask(polygons_to_rle([poly], h, w)['counts'], h, w), C.TRIANGLE_MASK)
    # union: two rectangles that overlap, and an object without polygons
    got = polygons_to_rle([C.rect_poly(1, 1, 4, 4), C.rect_poly(3, 2, 7, 5)], h, w)
    assert np.array_equal(R.counts_to_mask(got['counts'], h, w), C.rect_mask(1, 1, 4, 4, h, w) | C.rect_mask(3, 2, 7, 5, h, w))
    assert polygons_to_rle([], h, w) == {'size': [h, w], 'counts': [h * w]}


# ------------------------------------------------------------------------------------------------------------------ random populations
@pytest.mark.parametrize('seed', [0, 1, 2])
def test_random_populations_equal_restatement(seed):
    n_obj = n_multi = n_empty = 0
    for h, w, objects in C.population(seed, 360):
        got = device_lists(objects, h, w)
        assert len(got) == len(objects)
        for o, polys in enumerate(objects):
            want = R.object_transitions(polys, h, w)
            assert got[o] == want, (seed, h, w, o, polys)
            n_obj += 1
            n_multi += len(polys) > 1
            n_empty += len(want) == 0
    assert n_obj >= 300 and n_multi >= 60 and n_empty >= 10 and n_empty < n_obj // 2


def test_grouping_independence():
    """The same objects in one call, split into two calls, and permuted: identical per-object lists."""
    from upsnet_amd.dataset.polygon import rasterize_polygons
    rng = np.random.RandomState(7)
    h, w = 97, 131
    objects = [C.random_object(rng, h, w) for _ in range(150)]
    whole = device_lists(objects, h, w)
    assert sum(len(t) for t in whole) > 1000
    assert device_lists(objects[:61], h, w) + device_lists(objects[61:], h, w) == whole
    perm = rng.permutation(len(objects))
    got = device_lists([objects[i] for i in perm], h, w)
    assert all(got[j] == whole[i] for j, i in enumerate(perm))
    assert [device_lists([ob], h, w)[0] for ob in objects[:20]] == whole[:20]
    check_handle(rasterize_polygons(objects, h, w), 1 << 30)


# ------------------------------------------------------------------------------------------------------------------ real size
def real_size_objects(seed=3, n=60, h=1024, w=2048):
    rng = np.random.RandomState(seed)
    objects = []
    for i in range(n):
        k = int(rng.randint(500, 5001))
        polys = [C.blob_contour(rng, k, rng.uniform(0, w), rng.uniform(0, h), rng.uniform(15, 110))]
        if i % 10 == 0:   # an object of two parts (occlusion)
            polys.append(C.blob_contour(rng, 500, rng.uniform(0, w), rng.uniform(0, h), rng.uniform(10, 40)))
        objects.append(polys)
    return objects


def test_real_size_image_and_sawtooth_border():
    """A 1024 x 2048 image with 60 contours of 500 to 5000 vertices and one saw-tooth polygon along the whole border whose position list
    (> 10^4 entries) cannot fit an LDS run. The CPU restatement of this case took about 1 s where this was written (its sorts and
    mask decodes are numpy's); the time of the run at hand is printed."""
    from upsnet_amd.dataset.polygon import pack_polygons, rasterize_polygons
    h, w = 1024, 2048
    objects = real_size_objects() + [[C.sawtooth_border(h, w, step=8, depth=24)]]
    assert len(R.poly_positions(objects[-1][0], h, w)) > 16000   # emitted by the saw-tooth alone; an LDS run of the sort holds 4096
    total = pack_polygons(objects)[3]
    r = rasterize_polygons(objects, h, w)
    got = r.transitions()
    check_handle(r, total)
    assert len(got[-1]) > 13000
    t0 = time.time()
    for o, polys in enumerate(objects):
        want = R.object_transitions(polys, h, w)
        assert np.array_equal(got[o], np.asarray(want, np.int32)), o
    print("CPU restatement of %d objects (%d edge-walk points): %.1f s" % (len(objects), total, time.time() - t0))


# ------------------------------------------------------------------------------------------------------------------ memory, sync
@pytest.mark.parametrize('pattern', ['A', 'B'])
def test_on_poisoned_guard_banded_memory(pattern):
    """Outputs and workspace poisoned and fenced (tests/memguard.py): bands intact (poisoned() raises otherwise), offsets monotone, no
    position outside [0, h * w), lists equal to the restatement; the tail of trans beyond trans_off[-1] may hold anything."""
    from upsnet_amd.dataset.polygon import pack_polygons, rasterize_polygons
    rng = np.random.RandomState(11)
    for h, w, n in ((1, 1, 5), (13, 17, 40), (97, 131, 60), (300, 500, 12)):
        objects = [C.random_object(rng, h, w) for _ in range(n)] + [[], [[]]]
        if h == 300:
            objects.append([C.sawtooth_border(h, w)])
        with memguard.poisoned(pattern, modules=('upsnet_amd.dataset.polygon',)) as g:
            r = rasterize_polygons(objects, h, w)
            torch.cuda.synchronize()
            assert g.count == 3   # workspace, trans, trans_off
        check_handle(r, pack_polygons(objects)[3])
        got = [t.tolist() for t in r.transitions()]
        for o, polys in enumerate(objects):
            assert got[o] == R.object_transitions(polys, h, w), (pattern, h, w, o)
    with memguard.poisoned(pattern, modules=('upsnet_amd.dataset.polygon',)):
        r = rasterize_polygons([], 5, 5)
        assert r.trans_off.tolist() == [0]
        r = rasterize_polygons([[], [[]]], 5, 5)
        assert r.trans_off.tolist() == [0, 0, 0]


def test_no_host_synchronisation():
    """rasterize_polygons under torch.cuda.set_sync_debug_mode('error'). That this torch build honours the mode is shown first: a
    device-to-host read raises under it."""
    from upsnet_amd.dataset.polygon import rasterize_polygons
    rng = np.random.RandomState(5)
    objects = [C.random_object(rng, 97, 131) for _ in range(40)]
    want = device_lists(objects, 97, 131)   # also: the library is loaded and the allocator is warm
    probe = torch.ones(4, device='cuda')
    torch.cuda.synchronize()
    old = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode('error')
    try:
        with pytest.raises(RuntimeError):
            probe.sum().item()
        r = rasterize_polygons(objects, 97, 131)
    finally:
        torch.cuda.set_sync_debug_mode(old)
    assert [t.tolist() for t in r.transitions()] == want


# ------------------------------------------------------------------------------------------------------------------ evaluator
def polygon_scene(seed, n_img, H, W):
    """test_coco_eval_gpu's scene with the GT masks replaced by polygons: a slightly shrunken box, for some a noisy blob instead or
    as a second part; two detections in three get a mask that fills their box, so that matches exist at several IoU thresholds."""
    from test_coco_eval_gpu import make_scene
    scene = make_scene(seed, n_img=n_img, H=H, W=W, segm=True)
    rng = np.random.RandomState(seed)
    out = []
    for image_id, gts, boxes, scores, cls, masks in scene:
        new = []
        for el in gts:
            el = {k: v for k, v in el.items() if k not in ('_mask', 'segmentation')}
            x, y, bw, bh = el['bbox']
            s = rng.uniform(0, 0.12, 4)
            polys = [C.rect_poly(x + s[0] * bw, y + s[1] * bh, x + (1 - s[2]) * bw, y + (1 - s[3]) * bh)]
            blob = C.blob_contour(rng, int(rng.randint(8, 60)), x + bw / 2, y + bh / 2, 0.45 * min(bw, bh) + 1)
            kind = rng.randint(4)
            if kind == 0:
                polys = [blob]
            elif kind == 1:
                polys.append(blob)
            el['_polys'] = polys
            new.append(el)
        masks = masks.copy()
        masks[::3] = 0.55 + 0.45 * masks[::3]
        masks[1::3] = 0.55 + 0.45 * masks[1::3]
        out.append((image_id, new, boxes, scores, cls, masks))
    return out


def run_segm(scene, H, W, use_views, subset_cats=None):
    from test_coco_eval_gpu import CATS
    from upsnet_amd.dataset.coco_eval import DetectionEvaluator
    from upsnet_amd.dataset.polygon import rasterize_polygons
    ev = DetectionEvaluator(subset_cats or CATS, 'segm', device='cuda')
    for image_id, gts, boxes, scores, cls, masks in scene:
        poly = [k for k, el in enumerate(gts) if not el['iscrowd']]
        rasters = rasterize_polygons([gts[k]['_polys'] for k in poly], H, W) if use_views and poly else None
        gt = []
        for k, el in enumerate(gts):
            el = dict(el)
            if use_views and not el['iscrowd']:
                el['segmentation'] = rasters[poly.index(k)]
            else:
                el['segmentation'] = R.object_rle(el['_polys'], H, W)
            gt.append(el)
        ev.add(image_id, gt, torch.from_numpy(boxes).cuda(), torch.from_numpy(scores).cuda(), torch.from_numpy(cls).cuda(),
               torch.from_numpy(masks).cuda(), image_size=(H, W))
    return ev.accumulate()


def test_evaluator_views_equal_restated_rle():
    """DetectionEvaluator('segm') fed device views of rasterize_polygons (plus RLE crowds) against the same evaluator fed RLE dicts
    made by tests/polygon_ref.py: precision, recall, scores and stats bit-identical. Once with all categories, once with a category
    subset, where GTs of other categories are dropped and the remaining views are a gathered subset of their handle."""
    from test_coco_eval_gpu import CATS
    H, W = 240, 320
    scene = polygon_scene(4, 14, H, W)
    assert any(el['iscrowd'] for s in scene for el in s[1]) and sum(not el['iscrowd'] for s in scene for el in s[1]) > 50
    for cats in (None, CATS[:5]):
        a, b = run_segm(scene, H, W, True, cats), run_segm(scene, H, W, False, cats)
        for k in ('precision', 'recall', 'scores', 'stats'):
            assert a[k].shape == b[k].shape and np.array_equal(a[k].view(np.int64), b[k].view(np.int64)), k
        assert np.any(a['precision'] > 0) and a['stats'][0] > 0


def test_evaluator_refuses_bare_lists_and_mixed_handles():
    from test_coco_eval_gpu import CATS
    from upsnet_amd.dataset.coco_eval import DetectionEvaluator
    from upsnet_amd.dataset.polygon import rasterize_polygons
    ev = DetectionEvaluator(CATS, 'segm', device='cuda')
    z = dict(det_boxes=torch.zeros((0, 4)), det_scores=torch.zeros(0), det_cls=torch.zeros(0, dtype=torch.int64),
             det_masks=torch.zeros((0, 1, 28, 28)), image_size=(6, 8))
    gt = {'id': 1, 'category_id': CATS[0], 'iscrowd': 0, 'area': 12.0, 'bbox': [2, 1, 4, 3]}
    with pytest.raises(ValueError, match='dataset.polygon'):
        ev.add(1, [dict(gt, segmentation=[C.RECT])], **z)
    r1, r2 = rasterize_polygons([[C.RECT]], 6, 8), rasterize_polygons([[C.RECT]], 6, 8)
    with pytest.raises(ValueError, match='one rasterize_polygons call'):
        ev.add(1, [dict(gt, segmentation=r1[0]), dict(gt, id=2, segmentation=r2[0])], **z)
    with pytest.raises(ValueError, match='two GTs'):
        ev.add(1, [dict(gt, segmentation=r1[0]), dict(gt, id=2, segmentation=r1[0])], **z)
    with pytest.raises(ValueError, match='differs from the image'):
        ev.add(1, [dict(gt, segmentation=rasterize_polygons([[C.RECT]], 7, 8)[0])], **z)
    assert ev.num_images == 0


# ------------------------------------------------------------------------------------------------------------------ end to end
def test_evaluate_end_to_end_polygon_gt(tmp_path):
    """python -m upsnet_amd.evaluate on a COCO-layout fixture whose instances JSON stores polygons (and a few RLE crowds): the full run
    and --eval_only give the mask AP of the twin fixture whose GT was converted to RLE by tests/polygon_ref.py, and go on to the
    panoptic and semantic metrics."""
    import copy
    from test_dataset_run_cpu import make_dataset, write_cfg
    from test_dataset_run_gpu import CASES, _direct_chain, _write_gt
    from upsnet_amd.config.config import config, update_config
    from upsnet_amd.dataset import coco
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
        # the instances GT rewritten: each annotation's mask becomes polygons inside its box; every fifth one an RLE crowd
        with open(ds.instances_json_file) as f:
            inst = json.load(f)
        size_of = {im['id']: (im['height'], im['width']) for im in inst['images']}
        assert len(inst['annotations']) >= 4
        rng = np.random.RandomState(2)
        poly_json, rle_json = copy.deepcopy(inst), copy.deepcopy(inst)
        for k, (ap, ar) in enumerate(zip(poly_json['annotations'], rle_json['annotations'])):
            h, w = size_of[ap['image_id']]
            x, y, bw, bh = ap['bbox']
            polys = [C.rect_poly(x + 0.1 * bw, y + 0.1 * bh, x + 0.9 * bw + 1, y + 0.9 * bh + 1)]
            if k % 3 == 0:
                polys.append(C.blob_contour(rng, 24, x + bw / 2, y + bh / 2, 0.5 * min(bw, bh) + 1))
            rle = R.object_rle(polys, h, w)
            ar['segmentation'] = rle
            ap['segmentation'] = rle if k % 5 == 4 else polys
            ap['iscrowd'] = ar['iscrowd'] = int(k % 5 == 4)
        assert any(isinstance(a['segmentation'], list) for a in poly_json['annotations'])

        def write(d):
            with open(ds.instances_json_file, 'w') as f:
                json.dump(d, f)
        write(poly_json)
        full = main(['--cfg', cfg, '--synthetic_weights', '--in-flight', '2'])['metrics']
        again = main(['--cfg', cfg, '--eval_only'])['metrics']
        write(rle_json)
        twin = main(['--cfg', cfg, '--eval_only'])['metrics']
        for m in (full, again):
            assert np.array_equal(np.asarray(m['mask_ap']).view(np.int64), np.asarray(twin['mask_ap']).view(np.int64))
            assert np.array_equal(m['box_ap'], twin['box_ap'])
            assert m['panoptic'] == twin['panoptic'] and m['panoptic']['All']['n'] > 0
            assert m['sseg']['meanIU'] == twin['sseg']['meanIU']
        assert 0 < twin['mask_ap'][0] <= 1
    finally:
        config.clear()
        config.update(saved)
