"""GPU: COCO box / mask AP on the device (csrc/det_eval.hip via dataset/coco_eval.py) against the numpy restatement of pycocotools
in tests/test_coco_eval_cpu.py: precision, recall and scores bitwise equal on seeded scenes."""
import json

import numpy as np
import pytest
import torch

from test_coco_eval_cpu import cocoeval_restated

pytestmark = pytest.mark.gpu

CATS = [24, 26, 25, 27, 28, 31, 33, 32]   # class c -> CATS[c - 1]; deliberately not sorted (rows are the sorted ids)
NO_GT_CLASS = 8                            # its category (32) never has GT
TRUNC_EXTRA = 125                          # dets of one category added to images 3, 13, ... (truncation at maxDets 100)


def assert_truncated(scene):
    """Some (image, category) holds more than 100 dets, and its scores at ranks 99 and 100 tie (the cut falls inside a tie)."""
    hit = False
    for _, _, _, scores, cls, _ in scene:
        for c in np.unique(cls):
            s = np.sort(scores[cls == c])[::-1]
            if len(s) > 100 and s[99] == s[100]:
                hit = True
    assert hit, "no (image, category) with > 100 dets tied across the cut-off"


def assert_bitwise(res, want, msg=''):
    p, r, s, _ = want
    for name, got, exp in (('precision', res['precision'], p), ('recall', res['recall'], r), ('scores', res['scores'], s)):
        assert got.shape == exp.shape, (name, got.shape, exp.shape)
        bad = got.view(np.int64) != exp.view(np.int64)
        assert not bad.any(), (msg, name, int(bad.sum()), got[bad][:5], exp[bad][:5])
    np.testing.assert_array_equal(res['stats'], want[3])


def masks_from_rle(rle):
    from upsnet_amd.dataset.coco_eval import rle_counts
    counts, (h, w) = rle_counts(rle)
    flat = np.repeat(np.arange(len(counts)) % 2, counts).astype(bool)
    return flat.reshape(w, h).T


def rle_of(mask):
    from upsnet_amd.dataset.rle import rle_to_string
    flat = mask.T.reshape(-1).astype(np.int8)
    change = np.nonzero(np.diff(np.concatenate([[0], flat])))[0]
    counts = np.diff(np.concatenate([[0], change, [flat.size]])).tolist()
    return {'size': list(mask.shape), 'counts': rle_to_string(counts)}


def make_scene(seed, n_img=20, H=1024, W=2048, segm=False):
    """Per image: (image_id, gts, boxes f32 [n,4], scores f32 [n], cls int64 [n], masks f32 [n,1,28,28] or None)."""
    rng = np.random.default_rng(seed)
    ids = rng.choice(np.arange(1, 100000), n_img, replace=False)
    out = []
    for i, image_id in enumerate(ids):
        kind = i % 6   # 0: dets only, 1: GT only, else both
        G = 0 if kind == 0 else int(rng.integers(1, 30))
        gts, gboxes = [], []
        for g in range(G):
            w, h = np.exp(rng.uniform(np.log(4), np.log(min(300, W / 2, H / 2)), 2))
            x, y = rng.uniform(0, W - w - 1), rng.uniform(0, H - h - 1)
            bb = [float(np.floor(x)), float(np.floor(y)), float(np.ceil(w)), float(np.ceil(h))]
            cls = int(rng.integers(1, NO_GT_CLASS))
            area = bb[2] * bb[3]
            if g % 7 == 3:
                area = float(rng.choice([1024.0, 9216.0, 1023.5, 9216.5, 32 ** 2 + 1e-9]))
            el = {'id': int(rng.integers(1, 1 << 30)), 'category_id': CATS[cls - 1], 'iscrowd': int(rng.random() < 0.12),
                  'area': area, 'bbox': bb}
            if segm:
                m = np.zeros((H, W), np.uint8)
                x0, y0, x1, y1 = int(bb[0]), int(bb[1]), int(bb[0] + bb[2]), int(bb[1] + bb[3])
                m[y0:y1, x0:x1] = rng.random((y1 - y0, x1 - x0)) < 0.85
                if g % 5 == 0:
                    m[y0:(y0 + y1) // 2, x0:x1] = 0
                el['_mask'] = m.astype(bool)
                el['segmentation'] = torch.from_numpy(m).cuda() if g % 4 == 1 else rle_of(m)
                if g % 4 == 2:
                    from upsnet_amd.dataset.coco_eval import rle_counts
                    el['segmentation'] = {'size': [H, W], 'counts': rle_counts(el['segmentation'])[0].tolist()}
            gts.append(el)
            gboxes.append((bb, cls))
        n = 0 if kind == 1 else (int(rng.integers(150, 190)) if i % 5 == 2 else int(rng.integers(1, 60)))
        boxes, cls = np.zeros((n, 4), np.float32), np.zeros(n, np.int64)
        for d in range(n):
            if gboxes and rng.random() < 0.6:
                bb, c = gboxes[int(rng.integers(len(gboxes)))]
                j = rng.normal(0, 0.08, 4) * np.array([bb[2], bb[3], bb[2], bb[3]])
                boxes[d] = [bb[0] + j[0], bb[1] + j[1], bb[0] + bb[2] - 1 + j[2], bb[1] + bb[3] - 1 + j[3]]
                cls[d] = c if rng.random() < 0.9 else int(rng.integers(1, NO_GT_CLASS + 1))
            else:
                w, h = np.exp(rng.uniform(np.log(3), np.log(min(250, W / 2, H / 2)), 2))
                x, y = rng.uniform(0, W - w - 1), rng.uniform(0, H - h - 1)
                boxes[d] = [x, y, x + w, y + h]
                cls[d] = int(rng.integers(1, NO_GT_CLASS + 1))
        if i % 10 == 3 and gboxes:
            # more than 100 dets of ONE category in this image: COCOeval keeps the first 100 of each (image, category) by score
            c0 = gboxes[0][1]
            own = [bb for bb, c in gboxes if c == c0]
            extra = np.zeros((TRUNC_EXTRA, 4), np.float32)
            for d in range(TRUNC_EXTRA):
                bb = own[d % len(own)]
                j = rng.normal(0, 0.1, 4) * np.array([bb[2], bb[3], bb[2], bb[3]])
                extra[d] = [bb[0] + j[0], bb[1] + j[1], bb[0] + bb[2] - 1 + j[2], bb[1] + bb[3] - 1 + j[3]]
            boxes = np.concatenate([boxes, extra])
            cls = np.concatenate([cls, np.full(TRUNC_EXTRA, c0, np.int64)])
            n += TRUNC_EXTRA
        boxes[:, 0::2] = np.clip(boxes[:, 0::2], 0, W - 1)
        boxes[:, 1::2] = np.clip(boxes[:, 1::2], 0, H - 1)
        scores = (np.round(rng.random(n) * 20) / 20).astype(np.float32)   # many ties (21 values: some tie across rank 100)
        masks = None
        if segm:
            masks = rng.random((n, 1, 28, 28)).astype(np.float32)
            masks[::9] = 0   # empty det masks
        out.append((int(image_id), gts, boxes, scores, cls, masks))
    return out


def restated_bbox(scene):
    imgs = []
    for image_id, gts, boxes, scores, cls, _ in scene:
        b = boxes.astype(np.float64)
        dts = [{'category_id': CATS[int(c) - 1], 'score': float(s),
                'bbox': [b[d, 0], b[d, 1], b[d, 2] - b[d, 0] + 1, b[d, 3] - b[d, 1] + 1]} for d, (s, c) in enumerate(zip(scores, cls))]
        imgs.append((image_id, gts, dts))
    return cocoeval_restated(imgs, CATS, 'bbox')


def run(scene, iou_type='bbox', order=None, H=1024, W=2048):
    from upsnet_amd.dataset.coco_eval import DetectionEvaluator
    ev = DetectionEvaluator(CATS, iou_type, device='cuda')
    for k in (order if order is not None else range(len(scene))):
        image_id, gts, boxes, scores, cls, masks = scene[k]
        ev.add(image_id, gts, torch.from_numpy(boxes).cuda(), torch.from_numpy(scores).cuda(), torch.from_numpy(cls).cuda(),
               torch.from_numpy(masks).cuda() if iou_type == 'segm' else None, image_size=(H, W))
    return ev


# ------------------------------------------------------------------------------------------------------------------ bbox
@pytest.mark.parametrize('seed', [0, 1])
def test_bbox_random_scenes_bitwise(seed):
    scene = make_scene(seed)
    assert_truncated(scene)
    assert any(len(s[2]) > 150 for s in scene) and any(len(s[2]) == 0 for s in scene) and any(len(s[1]) == 0 for s in scene)
    ev = run(scene)
    res = ev.accumulate()
    want = restated_bbox(scene)
    assert_bitwise(res, want, 'seed %d' % seed)
    k_no_gt = sorted(CATS).index(CATS[NO_GT_CLASS - 1])
    assert np.all(res['precision'][:, :, k_no_gt] == -1)
    assert np.any(res['precision'] > 0) and np.any(res['precision'] == 0)
    assert ev.summary().count('\n') == 2 * (len(CATS) + 2) + 12


def test_merge_and_permuted_order():
    scene = make_scene(2, n_img=12)
    single = run(scene).accumulate()
    a, b = run(scene[:5]), run(scene[5:])
    a += b
    merged = a.accumulate()
    perm = run(scene, order=np.random.default_rng(5).permutation(len(scene))).accumulate()
    for r in (merged, perm):
        for k in ('precision', 'recall', 'scores', 'stats'):
            assert np.array_equal(r[k].view(np.int64), single[k].view(np.int64)), k


def test_add_rle_form_equals_add():
    scene = make_scene(3, n_img=8)
    from upsnet_amd.dataset.coco_eval import DetectionEvaluator
    ev = DetectionEvaluator(CATS, 'bbox')
    for image_id, gts, boxes, scores, cls, _ in scene:
        per = [[]] + [np.hstack([boxes[cls == c], scores[cls == c, None]]) for c in range(1, len(CATS) + 1)]
        ev.add_rle(image_id, gts, per)
    got = ev.accumulate()
    # the per-class regrouping keeps each (image, category)'s order, so nothing changes
    assert_bitwise(got, restated_bbox(scene))


# ------------------------------------------------------------------------------------------------------------------ segm
def restated_segm(scene, H, W):
    from upsnet_amd.dataset.rle import im_post
    imgs, rle_form = [], []
    for image_id, gts, boxes, scores, cls, masks in scene:
        boxes_all, masks_all = [[] for _ in range(len(CATS) + 1)], [[] for _ in range(len(CATS) + 1)]
        im_post(boxes_all, masks_all, torch.from_numpy(scores).cuda(), torch.from_numpy(boxes).cuda(), torch.from_numpy(masks).cuda(),
                torch.from_numpy(cls).cuda(), len(CATS) + 1, (H, W))
        dts = []
        for c in range(1, len(CATS) + 1):
            for row, rle in zip(boxes_all[c][0], masks_all[c][0]):
                dts.append({'category_id': CATS[c - 1], 'score': float(np.float32(row[4])), 'mask': masks_from_rle(rle)})
        g = [dict(el, mask=el['_mask']) for el in gts]
        imgs.append((image_id, g, dts))
        rle_form.append((image_id, gts, [[]] + [boxes_all[c][0] for c in range(1, len(CATS) + 1)],
                         [[]] + [masks_all[c][0] for c in range(1, len(CATS) + 1)]))
    return cocoeval_restated(imgs, CATS, 'segm'), rle_form


def test_segm_model_tensors_and_rle_strings_bitwise():
    H, W = 320, 480
    scene = make_scene(4, n_img=20, H=H, W=W, segm=True)
    assert_truncated(scene)
    # the RLE form groups dets by class; the restatement follows the same per-(image, category) order as the model form
    want, rle_form = restated_segm(scene, H, W)
    got = run(scene, 'segm', H=H, W=W).accumulate()
    assert_bitwise(got, want, 'segm from model tensors')
    from upsnet_amd.dataset.coco_eval import DetectionEvaluator
    ev = DetectionEvaluator(CATS, 'segm')
    for image_id, gts, dets, rles in rle_form:
        ev.add_rle(image_id, gts, dets, rles, image_size=(H, W))
    assert_bitwise(ev.accumulate(), want, 'segm from im_post RLE strings')


def test_segm_full_size_image():
    H, W = 1024, 2048
    scene = make_scene(6, n_img=4, H=H, W=W, segm=True)
    assert_truncated(scene)
    want, _ = restated_segm(scene, H, W)
    assert_bitwise(run(scene, 'segm', H=H, W=W).accumulate(), want, 'segm 1024x2048')


# ------------------------------------------------------------------------------------------------------------------ network
def test_end_to_end_on_the_network(tmp_path):
    from upsnet_amd.config.config import update_config_dict, CITYSCAPES_R50, config
    update_config_dict(CITYSCAPES_R50)
    from upsnet_amd.synthetic import build_model, make_image
    from upsnet_amd.dataset.coco_eval import DetectionEvaluator, rle_counts
    from upsnet_amd.dataset.rle import im_post
    H, W = 1024, 2048
    model = build_model(device='cuda:0')
    with torch.no_grad():
        out = model(make_image(H, W, seed=5, device='cuda:0'))
    # the reference's test loop: pred_boxes[:, 1:] / im_scale (1 here)
    boxes, scores, cls, masks = out['pred_boxes'][:, 1:].contiguous(), out['cls_probs'], out['cls_inds'], out['mask_probs']
    n_cls = config.dataset.num_classes
    cats = list(range(101, 101 + n_cls - 1))
    boxes_all, masks_all = [[] for _ in range(n_cls)], [[] for _ in range(n_cls)]
    im_post(boxes_all, masks_all, scores, boxes, masks, cls, n_cls, (H, W))
    # GT = the network's own detections (boxes in xywh; for segm the pasted masks, empty ones left out): AP 1 for every category
    # present in the GT
    for iou_type in ('bbox', 'segm'):
        gts, gid, spoiled = [], 1, set()
        for c in range(1, n_cls):
            for row, rle in zip(boxes_all[c][0], masks_all[c][0]):
                x1, y1, x2, y2 = (float(v) for v in row[:4])
                area = int(rle_counts(rle)[0][1::2].sum())
                if iou_type == 'segm' and area == 0:
                    spoiled.add(cats[c - 1])   # an empty det mask is a false positive of its category
                    continue
                gts.append({'id': gid, 'category_id': cats[c - 1], 'iscrowd': 0, 'bbox': [x1, y1, x2 - x1 + 1, y2 - y1 + 1],
                            'area': float(area) if iou_type == 'segm' else (x2 - x1 + 1) * (y2 - y1 + 1), 'segmentation': rle})
                gid += 1
        assert len(gts) >= 3
        ev = DetectionEvaluator(cats, iou_type)
        ev.add(7, gts, boxes, scores, cls, masks if iou_type == 'segm' else None, image_size=(H, W))
        res = ev.accumulate()
        present = sorted({g['category_id'] for g in gts} - spoiled)
        assert present
        for c in present:
            k = cats.index(c)
            assert np.all(np.abs(res['precision'][:, :, k, 0, 2] - 1) <= 2.5e-16), (iou_type, c)
            assert np.all(res['recall'][:, k, 0, 2] == 1), (iou_type, c)
    # a perturbed GT: shifted boxes / masks, one crowd, one dropped; bitwise against the restatement
    rng = np.random.default_rng(1)
    pert = []
    for g in gts[1:]:
        m = np.roll(masks_from_rle(g['segmentation']), (int(rng.integers(-3, 4)), int(rng.integers(-3, 4))), (0, 1))
        bb = [v + float(rng.integers(-4, 5)) for v in g['bbox'][:2]] + g['bbox'][2:]
        pert.append(dict(g, bbox=bb, segmentation=rle_of(m), _mask=m, iscrowd=int(len(pert) == 2), area=float(m.sum())))
    dts_b, dts_s = [], []
    b64, s_np, c_np = boxes.double().cpu().numpy(), scores.cpu().numpy(), cls.cpu().numpy()
    trans = {}
    for c in range(1, n_cls):
        sel = np.nonzero(c_np == c)[0]
        for d, rle in zip(sel, masks_all[c][0]):
            trans[int(d)] = masks_from_rle(rle)
    for d in range(len(s_np)):
        c = int(c_np[d])
        if not 1 <= c < n_cls:
            continue
        dts_b.append({'category_id': cats[c - 1], 'score': float(s_np[d]),
                      'bbox': [b64[d, 0], b64[d, 1], b64[d, 2] - b64[d, 0] + 1, b64[d, 3] - b64[d, 1] + 1]})
        dts_s.append({'category_id': cats[c - 1], 'score': float(s_np[d]), 'mask': trans[d]})
    want_b = cocoeval_restated([(7, pert, dts_b)], cats, 'bbox')
    want_s = cocoeval_restated([(7, [dict(g, mask=g['_mask']) for g in pert], dts_s)], cats, 'segm')
    for iou_type, want in (('bbox', want_b), ('segm', want_s)):
        ev = DetectionEvaluator(cats, iou_type)
        ev.add(7, pert, boxes, scores, cls, masks if iou_type == 'segm' else None, image_size=(H, W))
        assert_bitwise(ev.accumulate(), want, 'perturbed ' + iou_type)


def test_base_dataset_evaluate_boxes_and_masks(tmp_path):
    from upsnet_amd.dataset.base_dataset import BaseDataset
    H, W = 200, 300
    scene = make_scene(8, n_img=6, H=H, W=W, segm=True)
    want_s, rle_form = restated_segm(scene, H, W)
    images = [{'id': s[0], 'height': H, 'width': W, 'file_name': '%d.png' % s[0]} for s in scene]
    anns = []
    for image_id, gts, _, _, _, _ in scene:
        for g in gts:
            seg = g['segmentation']
            if isinstance(seg, torch.Tensor):
                seg = rle_of(seg.cpu().numpy())
            anns.append({k: v for k, v in dict(g, image_id=image_id, segmentation=seg).items() if k != '_mask'})
    js = {'images': images, 'annotations': anns, 'categories': [{'id': c, 'name': str(c)} for c in CATS]}
    path = tmp_path / 'instances.json'
    path.write_text(json.dumps(js))
    ds = BaseDataset()
    ds.instances_json_file, ds.name = str(path), 'synthetic'
    order = sorted(range(len(scene)), key=lambda i: scene[i][0])
    cls_of = {c: i + 1 for i, c in enumerate(CATS)}   # the dataset's classes: the JSON's category order (unsorted here)
    all_boxes = [[[] for _ in order] for _ in range(len(CATS) + 1)]
    all_segms = [[[] for _ in order] for _ in range(len(CATS) + 1)]
    for slot, i in enumerate(order):
        _, _, dets, rles = rle_form[i]
        for c in range(1, len(CATS) + 1):
            all_boxes[cls_of[CATS[c - 1]]][slot] = dets[c]
            all_segms[cls_of[CATS[c - 1]]][slot] = rles[c]
    stats = ds.evaluate_boxes(all_boxes, str(tmp_path))
    assert (tmp_path / 'bbox_synthetic_results.json').exists() and (tmp_path / 'detection_results.txt').exists()
    assert len(stats) == 12
    res = ds.evaluate_masks(all_boxes, all_segms, str(tmp_path))
    assert (tmp_path / 'segmentations_synthetic_results.json').exists()
    assert_bitwise({'precision': res.eval['precision'], 'recall': res.eval['recall'], 'scores': res.eval['scores'], 'stats': res.stats},
                   want_s, 'evaluate_masks')


# ------------------------------------------------------------------------------------------------------------------ errors
def test_error_paths():
    from upsnet_amd.dataset.coco_eval import DetectionEvaluator
    ev = DetectionEvaluator(CATS, 'segm')
    b, s, c, m = torch.zeros((2, 4), device='cuda'), torch.ones(2, device='cuda'), torch.ones(2, dtype=torch.int64, device='cuda'), \
        torch.zeros((2, 1, 28, 28), device='cuda')
    ev.add(1, [], b, s, c, m, image_size=(64, 64))
    with pytest.raises(ValueError, match='twice'):
        ev.add(1, [], b, s, c, m, image_size=(64, 64))
    with pytest.raises(ValueError):
        ev.add(2, [{'id': 1, 'category_id': 24, 'iscrowd': 0, 'area': 1.0, 'bbox': [0, 0, 1, 1],
                    'segmentation': torch.zeros((64, 65), dtype=torch.uint8, device='cuda')}], b, s, c, m, image_size=(64, 64))
    with pytest.raises(ValueError, match='polygon'):
        ev.add(2, [{'id': 1, 'category_id': 24, 'iscrowd': 0, 'area': 1.0, 'bbox': [0, 0, 1, 1], 'segmentation': [[0, 0, 1, 0, 1, 1]]}],
               b, s, c, m, image_size=(64, 64))
    with pytest.raises(ValueError):
        ev.add(2, [], b, s, c.float(), m, image_size=(64, 64))
    with pytest.raises(ValueError):
        ev.add(2, [], b, s, c, m[:, :, :20], image_size=(64, 64))
    other = DetectionEvaluator(CATS, 'bbox')
    with pytest.raises(ValueError):
        ev += other
    res = ev.accumulate()   # the image that went in: two dets of category 24, no GT anywhere -> -1 everywhere
    assert np.all(res['precision'] == -1) and np.all(res['stats'] == -1)
