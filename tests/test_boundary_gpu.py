"""GPU: Boundary IoU / Boundary AP on the device (bnd_erode_kernel and the boundary mode of csrc/det_eval.hip via dataset/boundary.py
and dataset/coco_eval.py) against the numpy restatement of tests/boundary_ref.py: boundary masks, precision, recall, scores and
stats bit for bit."""
import json
import os
import pickle

import numpy as np
import pytest
import torch

import boundary_ref
import memguard
from test_coco_eval_gpu import CATS, assert_bitwise, assert_truncated, make_scene, masks_from_rle, restated_segm, rle_of
from test_dataset_run_cpu import CITYSCAPES_THINGS, make_dataset, saved_config, write_cfg  # noqa: F401  (saved_config is a fixture)

pytestmark = pytest.mark.gpu

GUARDED = memguard.MODULES + ('upsnet_amd.dataset.boundary',)     # the modules that allocate here


# ------------------------------------------------------------------------------------------------------------------ the kernel alone
def check_kernel(H, W, ratio):
    from upsnet_amd.dataset.boundary import boundary_dilation, mask_to_boundary
    d = boundary_dilation(H, W, ratio)
    cases = boundary_ref.mask_cases(H, W, d, seed=H * 10007 + W)
    masks = np.stack([m for _, m in cases])
    want = np.stack([boundary_ref.mask_to_boundary(m, ratio) for m in masks]).astype(np.uint8)
    assert want.any() and ((want != masks).any() or 2 * d + 1 > min(H, W))       # (a window larger than the image erodes nothing)
    rles = [rle_of(m) for m in masks]
    dev = torch.from_numpy(masks.astype(np.uint8)).cuda()
    for pattern in ('A', 'B'):
        with memguard.poisoned(pattern, modules=GUARDED):
            got_u8 = mask_to_boundary(memguard.banded_copy(dev, pattern), ratio)
            got_bool = mask_to_boundary(dev.bool(), ratio, size=(H, W))
            got_rle = mask_to_boundary(rles, ratio)
        for form, got in (('uint8', got_u8), ('bool', got_bool), ('rle', got_rle)):
            assert got.dtype == torch.uint8 and tuple(got.shape) == masks.shape
            bad = np.nonzero((got.cpu().numpy() != want).reshape(len(cases), -1).any(1))[0]
            assert len(bad) == 0, (form, pattern, H, W, d, [cases[k][0] for k in bad])


@pytest.mark.parametrize('H,W,ratio', boundary_ref.SIZES)
def test_mask_to_boundary_bitwise(H, W, ratio):
    check_kernel(H, W, ratio)


def test_mask_to_boundary_full_size():
    check_kernel(*boundary_ref.FULL_SIZE)


def test_mask_to_boundary_empty_list_and_refusals():
    from upsnet_amd.dataset.boundary import mask_to_boundary
    assert tuple(mask_to_boundary([], size=(5, 7)).shape) == (0, 5, 7)
    assert tuple(mask_to_boundary(torch.zeros((0, 5, 7), dtype=torch.uint8, device='cuda')).shape) == (0, 5, 7)
    with pytest.raises(ValueError, match='differs'):
        mask_to_boundary(torch.zeros((1, 5, 7), dtype=torch.uint8, device='cuda'), size=(7, 5))
    with pytest.raises(ValueError, match='exceeds'):      # d = 3536 on a 10000 x 10000 image: wider than the window tile
        mask_to_boundary([{'size': [10000, 10000], 'counts': [10000 * 10000]}], 0.25)


# ------------------------------------------------------------------------------------------------------------------ evaluator
def restated_boundary(scene, H, W, ratio=0.02):
    """restated_segm (the oracle-pasted full masks into the restated COCOeval) under the boundary rule."""
    with boundary_ref.boundary_rule(ratio):
        return restated_segm(scene, H, W)


def run(scene, H, W, iou_type='boundary', order=None, **kw):
    from upsnet_amd.dataset.coco_eval import DetectionEvaluator
    ev = DetectionEvaluator(CATS, iou_type, device='cuda', **kw)
    for k in (order if order is not None else range(len(scene))):
        image_id, gts, boxes, scores, cls, masks = scene[k]
        ev.add(image_id, gts, torch.from_numpy(boxes).cuda(), torch.from_numpy(scores).cuda(), torch.from_numpy(cls).cuda(),
               torch.from_numpy(masks).cuda(), image_size=(H, W))
    return ev


def differs(a, b):
    return any(not np.array_equal(x, y) for x, y in zip(a[:3], b[:3]))


def solid_gt(el, H, W):
    """The GT with its mask replaced by its whole box (same segmentation form): a mask with an interior, whose boundary is a ring."""
    x0, y0, x1, y1 = int(el['bbox'][0]), int(el['bbox'][1]), int(el['bbox'][0] + el['bbox'][2]), int(el['bbox'][1] + el['bbox'][3])
    m = np.zeros((H, W), bool)
    m[y0:y1, x0:x1] = True
    seg = el['segmentation']
    if isinstance(seg, torch.Tensor):
        new = torch.from_numpy(m.astype(np.uint8)).cuda()
    elif isinstance(seg['counts'], list):
        from upsnet_amd.dataset.coco_eval import rle_counts
        new = {'size': [H, W], 'counts': rle_counts(rle_of(m))[0].tolist()}
    else:
        new = rle_of(m)
    return dict(el, _mask=m, segmentation=new)


def with_interiors(scene, H, W):
    """make_scene's masks are speckle (every pixel lies within d of a hole, so a boundary is its whole mask and Boundary AP would equal
    mask AP): every other GT becomes its solid box and every other det mask a solid paste, which have interiors to erode."""
    out = []
    for image_id, gts, boxes, scores, cls, masks in scene:
        gts = [solid_gt(el, H, W) if g % 2 == 0 else el for g, el in enumerate(gts)]
        masks = masks.copy()
        masks[1::2] = 0.9
        out.append((image_id, gts, boxes, scores, cls, masks))
    return out


def rect_scene(H, W):
    """One image whose det boxes hang over each image edge, are one pixel wide or high, or paste nothing, next to plain ones; GTs in
    all three segmentation forms, one of them a crowd."""
    rng = np.random.default_rng(11)
    boxes = np.array([[-20, 10, 30, 50], [W - 30, 20, W + 25, 70], [40, -15, 90, 20], [50, H - 25, 110, H + 30],      # over each edge
                      [-10, -10, W + 10, H + 10],                                                                      # over all four
                      [70, 30, 70, 80], [20, 60, 90, 60], [33, 44, 33, 44],                                            # 1 pixel wide / high / both
                      [60, 20, 120, 70], [62, 22, 118, 72], [10, 30, 40, 80], [100, 40, 150, 90],                      # plain
                      [W + 5, 10, W + 40, 40], [30, H + 3, 60, H + 20]], np.float32)                                   # outside: empty paste
    n = len(boxes)
    masks = np.full((n, 1, 28, 28), 0.9, np.float32)
    masks[8] = rng.random((1, 28, 28)).astype(np.float32)        # a speckled one
    masks[9, :, 10:18, 10:18] = 0.1                              # a hole
    masks[10] = 0.0                                              # a box that pastes nothing
    cls = np.array([1, 1, 2, 2, 1, 3, 3, 3, 1, 1, 2, 2, 1, 2], np.int64)
    scores = np.linspace(0.95, 0.3, n).astype(np.float32)
    gts = []
    for g, (bb, c, crowd) in enumerate([([0, 10, 31, 41], 1, 0), ([W - 30, 20, 30, 51], 1, 0), ([40, 0, 51, 21], 2, 0),
                                        ([50, H - 25, 61, 25], 2, 0), ([60, 20, 61, 51], 1, 0), ([0, 0, W, H], 1, 1),
                                        ([68, 30, 5, 51], 3, 0), ([10, 30, 31, 51], 2, 0), ([100, 40, 51, 51], 2, 0)]):
        el = {'id': g + 1, 'category_id': CATS[c - 1], 'iscrowd': crowd, 'area': float(bb[2] * bb[3]), 'bbox': [float(v) for v in bb],
              'segmentation': {'size': [H, W], 'counts': [H * W]}}
        el = solid_gt(el, H, W)
        if g % 3 == 1:
            el['segmentation'] = torch.from_numpy(el['_mask'].astype(np.uint8)).cuda()
        gts.append(el)
    return [(7, gts, boxes, scores, cls, masks)]


def test_rect_limited_det_planes():
    H, W = 96, 160
    scene = rect_scene(H, W)
    want, _ = restated_boundary(scene, H, W)
    assert differs(want, restated_segm(scene, H, W)[0])
    assert np.any(want[0] > 0)
    for pattern in ('A', 'B'):
        with memguard.poisoned(pattern, modules=GUARDED):
            res = run(scene, H, W).accumulate()
        assert_bitwise(res, want, 'rect-limited det planes, pattern ' + pattern)
    # the same boxes on an image of two words per column, and d = 3
    H2, W2 = 130, 160
    scene2 = rect_scene(H2, W2)
    assert_bitwise(run(scene2, H2, W2).accumulate(), restated_boundary(scene2, H2, W2)[0], 'rect-limited det planes, 130 rows')


@pytest.mark.parametrize('seed', [4, 5])
def test_random_scenes_bitwise(seed):
    H, W = 96, 160
    scene = with_interiors(make_scene(seed, n_img=20, H=H, W=W, segm=True), H, W)
    assert_truncated(scene)
    assert any(len(s[2]) == 0 for s in scene) and any(len(s[1]) == 0 for s in scene)
    assert any(g['iscrowd'] for s in scene for g in s[1])
    want, _ = restated_boundary(scene, H, W)
    segm, _ = restated_segm(scene, H, W)
    assert differs(want, segm), "the boundary restatement equals the segm one on this scene: the test could pass by scoring segm"
    assert np.any(want[0] > 0)
    assert_bitwise(run(scene, H, W).accumulate(), want, 'seed %d' % seed)
    assert_bitwise(run(scene, H, W, 'segm').accumulate(), segm, 'segm beside it, seed %d' % seed)


def test_full_size_scene_bitwise():
    H, W = 1024, 2048
    scene = with_interiors(make_scene(12, n_img=3, H=H, W=W, segm=True), H, W)      # dets only, GT only, 150+ dets on GT with a crowd
    assert len(scene[2][2]) > 150 and any(g['iscrowd'] for g in scene[2][1])
    want, _ = restated_boundary(scene, H, W)
    res = run(scene, H, W).accumulate()
    assert_bitwise(res, want, 'boundary 1024x2048')
    segm = run(scene, H, W, 'segm').accumulate()                                     # (its own restatement: test_coco_eval_gpu.py)
    assert differs(want, (segm['precision'], segm['recall'], segm['scores']))


def test_other_dilation_ratio():
    H, W = 96, 160
    scene = with_interiors(make_scene(9, n_img=6, H=H, W=W, segm=True), H, W)
    a, _ = restated_boundary(scene, H, W, 0.02)
    b, _ = restated_boundary(scene, H, W, 0.05)
    assert differs(a, b)
    assert_bitwise(run(scene, H, W, dilation_ratio=0.05).accumulate(), b, 'ratio 0.05')


# ------------------------------------------------------------------------------------------------------------------ forms and merge
def test_forms_and_merge_give_the_same_arrays():
    from upsnet_amd.dataset.coco_eval import DetectionEvaluator, rle_counts
    from upsnet_amd.dataset.polygon import polygons_to_rle, rasterize_polygons
    H, W = 96, 160
    scene = with_interiors(make_scene(12, n_img=8, H=H, W=W, segm=True), H, W)
    # every GT mask is a polygon's raster, so that all five GT forms hold the same pixels
    polys = {}
    for s, (image_id, gts, boxes, scores, cls, masks) in enumerate(scene):
        for g, el in enumerate(gts):
            x, y, w, h = el['bbox']
            poly = [[x, y, x + w, y, x + w, y + h, x + w / 3, y + h, x, y + h / 2]]
            m = masks_from_rle(polygons_to_rle(poly, H, W))
            gts[g] = dict(el, _mask=m, segmentation=rle_of(m))
            polys[image_id, g] = poly
    want, rle_form = restated_boundary(scene, H, W)
    assert differs(want, restated_segm(scene, H, W)[0])
    single = run(scene, H, W).accumulate()
    assert_bitwise(single, want, 'add, RLE strings')

    def gt_in(form, image_id, gts):
        if form == 'polygon':
            views = rasterize_polygons([polys[image_id, g] for g in range(len(gts))], H, W) if gts else []
            return [dict(el, segmentation=views[g]) for g, el in enumerate(gts)]
        if form == 'counts':
            return [dict(el, segmentation={'size': [H, W], 'counts': rle_counts(el['segmentation'])[0].tolist()}) for el in gts]
        if form == 'uint8':
            return [dict(el, segmentation=torch.from_numpy(el['_mask'].astype(np.uint8)).cuda()) for el in gts]
        return gts
    for form in ('strings', 'counts', 'uint8', 'polygon'):
        ev = DetectionEvaluator(CATS, 'boundary')
        for image_id, gts, dets, rles in rle_form:
            ev.add_rle(image_id, gt_in(form, image_id, gts), dets, rles, image_size=(H, W))
        assert_bitwise(ev.accumulate(), want, 'add_rle, GT as ' + form)
    a, b = run(scene[:3], H, W), run(scene[3:], H, W)
    a += b
    perm = run(scene, H, W, order=np.random.default_rng(5).permutation(len(scene)))
    for name, ev in (('merged', a), ('permuted', perm)):
        res = ev.accumulate()
        for k in ('precision', 'recall', 'scores', 'stats'):
            assert np.array_equal(res[k].view(np.int64), single[k].view(np.int64)), (name, k)


# ------------------------------------------------------------------------------------------------------------------ public path
def test_evaluate_eval_only_eval_boundary(tmp_path, saved_config):     # noqa: F811
    """A hand-written instances JSON and results pickle (RLE dets equal to the GT plus one shifted det) through
    python -m upsnet_amd.evaluate --eval_only --eval_boundary [--boundary_dilation_ratio R]."""
    from upsnet_amd.evaluate import main
    H, W = 40, 60
    root = str(tmp_path / 'cs')
    anno_path, _ = make_dataset(root, 'Cityscapes', [(H, W), (H, W)], ids=[2, 1], seed=1)
    with open(anno_path) as f:
        js = json.load(f)
    cats = CITYSCAPES_THINGS

    def rect(y0, y1, x0, x1):
        m = np.zeros((H, W), bool)
        m[y0:y1, x0:x1] = True
        return m
    gt_masks = {1: [(1, rect(10, 30, 10, 40)), (3, rect(2, 12, 45, 58))], 2: [(1, rect(5, 35, 5, 25)), (2, rect(0, 10, 0, 10))]}
    anns, images = [], []
    n_cls = len(cats) + 1
    all_boxes = [[[] for _ in range(2)] for _ in range(n_cls)]
    all_masks = [[[] for _ in range(2)] for _ in range(n_cls)]
    for slot, image_id in enumerate([1, 2]):
        gts, dts = [], []
        per_cls = {}
        for c, m in gt_masks[image_id]:
            ys, xs = np.nonzero(m)
            bb = [float(xs.min()), float(ys.min()), float(xs.max() - xs.min() + 1), float(ys.max() - ys.min() + 1)]
            el = {'id': len(anns) + 1, 'image_id': image_id, 'category_id': cats[c - 1], 'iscrowd': 0, 'area': float(m.sum()), 'bbox': bb,
                  'segmentation': rle_of(m)}
            anns.append(el)
            gts.append(dict(el, mask=m))
            per_cls.setdefault(c, []).append((0.9, m, bb))
        c, m = gt_masks[image_id][0]
        shifted = np.roll(m, 2, axis=1)                                       # the issue's pair: mask IoU 0.875, boundary IoU 7/17
        per_cls[c].append((0.95, shifted, [0.0, 0.0, 1.0, 1.0]))
        for c, dets in per_cls.items():
            all_boxes[c][slot] = np.array([[bb[0], bb[1], bb[0] + bb[2] - 1, bb[1] + bb[3] - 1, s] for s, _, bb in dets], np.float32)
            all_masks[c][slot] = [rle_of(m) for _, m, _ in dets]
            dts += [{'category_id': cats[c - 1], 'score': float(np.float32(s)), 'mask': m} for s, m, _ in dets]
        images.append((image_id, gts, dts))
    js['annotations'] = anns
    with open(anno_path, 'w') as f:
        json.dump(js, f)
    head = write_cfg(tmp_path, 'Cityscapes', root, 'val')
    cfg = tmp_path / 'masks_only.yaml'
    cfg.write_text(open(head).read().replace('network:\n', 'network:\n  has_fcn_head: false\n  has_panoptic_head: false\n'))
    cfg = str(cfg)
    from upsnet_amd.config.config import update_config
    from upsnet_amd.evaluate import final_output_path
    update_config(cfg)
    results_dir = os.path.join(final_output_path(cfg), 'results')
    os.makedirs(results_dir)
    with open(os.path.join(results_dir, 'results_list.pkl'), 'wb') as f:
        pickle.dump({'all_boxes': all_boxes, 'all_masks': all_masks, 'all_ssegs': None, 'all_panos': None, 'all_pano_cls_inds': None}, f)

    plain = main(['--cfg', cfg, '--eval_only'])
    assert 'boundary_ap' not in plain['metrics'] and not os.path.exists(os.path.join(results_dir, 'boundary_results.txt'))
    with open(os.path.join(results_dir, 'detection_results.txt'), 'rb') as f:
        det_txt = f.read()
    jsons = {n: open(os.path.join(results_dir, n), 'rb').read() for n in os.listdir(results_dir) if n.endswith('_results.json')}
    assert len(jsons) == 2

    res = main(['--cfg', cfg, '--eval_only', '--eval_boundary'])
    assert list(res['metrics']) == ['box_ap', 'mask_ap', 'boundary_ap']
    want = boundary_ref.boundary_cocoeval(images, cats)
    import test_coco_eval_cpu
    segm = test_coco_eval_cpu.cocoeval_restated(images, cats, 'segm')
    assert not np.array_equal(want[3], segm[3])
    np.testing.assert_array_equal(res['metrics']['boundary_ap'], want[3])
    np.testing.assert_array_equal(res['metrics']['mask_ap'], segm[3])
    np.testing.assert_array_equal(res['metrics']['mask_ap'], plain['metrics']['mask_ap'])
    with open(os.path.join(results_dir, 'boundary_results.txt')) as f:
        lines = f.read().splitlines()
    assert len(lines) == 12 and lines[0].endswith('= %0.3f' % want[3][0])
    with open(os.path.join(results_dir, 'detection_results.txt'), 'rb') as f:
        assert f.read() == det_txt
    assert {n: open(os.path.join(results_dir, n), 'rb').read() for n in os.listdir(results_dir) if n.endswith('_results.json')} == jsons

    wide = main(['--cfg', cfg, '--eval_only', '--eval_boundary', '--boundary_dilation_ratio', '0.05'])
    want5 = boundary_ref.boundary_cocoeval(images, cats, 0.05)
    assert not np.array_equal(want5[3], want[3])
    np.testing.assert_array_equal(wide['metrics']['boundary_ap'], want5[3])
