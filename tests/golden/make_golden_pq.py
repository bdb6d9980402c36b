#!/usr/bin/env python
"""Golden vectors for panoptic quality and the semantic confusion matrix, made by the REFERENCE's own Python:
BaseDataset._converter_2ch_single_core (the 2-channel prediction -> pred PNG + JSON), BaseDataset._pq_compute_single_core on one
worker, PQStat.pq_average for All / Things / Stuff (upsnet/dataset/base_dataset.py:44-96, 466-610), and
BaseDataset.get_confusion_matrix (:806-824), imported from the reference checkout with the in-process shims of make_golden_blob.py plus a
`panopticapi.utils` stand-in (rgb2id restated; a deterministic IdGenerator handing out unique non-zero colours -- the colours only
relabel pred segments, PQ does not depend on them).

Run in the build container:  python tests/golden/make_golden_pq.py   (writes tests/golden/pq.npz)
"""
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_blob as mgb  # noqa: E402  (shims, the reference checkout on sys.path, the reference's BaseDataset)

BaseDataset, config = mgb.BaseDataset, mgb.config
PQStat = sys.modules[BaseDataset.__module__].PQStat


def rgb2id(color):
    if isinstance(color, np.ndarray) and len(color.shape) == 3:
        color = color.astype(np.int32)
        return color[:, :, 0] + 256 * color[:, :, 1] + 256 * 256 * color[:, :, 2]
    return int(color[0] + 256 * color[1] + 256 * 256 * color[2])


class IdGenerator(object):
    """Unique non-zero colours in the order asked for (deterministic)."""

    def __init__(self, categories):
        self.categories = categories
        self.next = 1

    def get_color(self, cat_id):
        i = self.next
        self.next += 1
        return [i & 255, (i >> 8) & 255, (i >> 16) & 255]


pu = types.ModuleType('panopticapi.utils')
pu.rgb2id, pu.IdGenerator = rgb2id, IdGenerator
sys.modules.setdefault('panopticapi', types.ModuleType('panopticapi'))
sys.modules['panopticapi.utils'] = pu

# Cityscapes-like table: 0..10 stuff, 11..18 things, plus 40 (stuff) and 41 (thing) that no case ever touches
CATEGORIES = {c: {'id': c, 'isthing': int(c >= 11 and c != 40), 'name': 'c%d' % c} for c in list(range(19)) + [40, 41]}


def id_rgb(ids):
    ids = np.asarray(ids, np.int64)
    return np.stack([ids & 255, (ids >> 8) & 255, (ids >> 16) & 255], -1).astype(np.uint8)


def pred2ch(cat, inst):
    return np.stack([cat, inst, np.zeros_like(cat)], -1).astype(np.uint8)


def segs_of(gt_ids, cats, crowd=(), missing=(), area_delta=None):
    """segments_info of a GT id map for the (id, category) pairs in `cats`, in that (JSON) order, except `missing`; area = pixel count
    (+ area_delta[id])."""
    info = []
    for gid, cat in cats:
        if gid in missing:
            continue
        area = int((gt_ids == gid).sum()) + (area_delta or {}).get(gid, 0)
        info.append({'id': int(gid), 'category_id': int(cat), 'iscrowd': int(gid in crowd), 'area': area})
    return info


def ref_score(images):
    """images: [(pred_2ch, gt_rgb, segments_info)] -> (PQStat, results) of a single-worker reference run."""
    annotations, pan_all = BaseDataset._converter_2ch_single_core(0, [p for p, _, _ in images], IdGenerator(CATEGORIES))
    gt_jsons = [{'image_id': i, 'segments_info': s} for i, (_, _, s) in enumerate(images)]
    stat = BaseDataset._pq_compute_single_core(0, gt_jsons, annotations, [g for _, g, _ in images], pan_all,
                                               [{'id': i} for i in range(len(images))], CATEGORIES)
    results = {}
    for name, isthing in [("All", None), ("Things", True), ("Stuff", False)]:
        try:
            results[name], per_class = stat.pq_average(CATEGORIES, isthing=isthing)
        except ZeroDivisionError:
            results[name], per_class = 'ZeroDivisionError', None
        if name == 'All':
            results['per_class'] = per_class
    return stat, results


def hand_cases():
    H, W = 20, 20
    cases = {}

    def base():
        cat = np.zeros((H, W), np.int64)        # stuff 0 everywhere
        inst = np.zeros((H, W), np.int64)
        gt = np.full((H, W), 1, np.int64)        # GT stuff id 1 (cat 0) everywhere
        return cat, inst, gt

    # exact match of a thing and of the stuff
    cat, inst, gt = base()
    cat[2:8, 2:7], inst[2:8, 2:7], gt[2:8, 2:7] = 11, 1, 7
    cases['exact'] = [(pred2ch(cat, inst), id_rgb(gt), segs_of(gt, [(1, 0), (7, 11)]))]
    # IoU exactly 0.5 (areas 15 / 15, intersection 10, union 20): no match -> FN + FP
    cat, inst, gt = base()
    cat[0, 0:15], inst[0, 0:15] = 12, 1
    gt[0, 5:20] = 9
    cases['iou_half'] = [(pred2ch(cat, inst), id_rgb(gt), segs_of(gt, [(1, 0), (9, 12)]))]
    # IoU just above 0.5 (areas 100 / 100, intersection 67, union 133)
    cat, inst, gt = base()
    cat.reshape(-1)[0:100], inst.reshape(-1)[0:100] = 12, 2
    gt.reshape(-1)[33:133] = 9
    cases['iou_above'] = [(pred2ch(cat, inst), id_rgb(gt), segs_of(gt, [(1, 0), (9, 12)]))]
    # category mismatch on the same region
    cat, inst, gt = base()
    cat[5:10, 5:10], inst[5:10, 5:10], gt[5:10, 5:10] = 13, 1, 4
    cases['cat_mismatch'] = [(pred2ch(cat, inst), id_rgb(gt), segs_of(gt, [(1, 0), (4, 14)]))]
    # VOID absorbing an unmatched pred: 6 / 10 pixels on VOID (absorbed), 5 / 10 (exactly 0.5: FP)
    cat, inst, gt = base()
    cat[0, 0:10], inst[0, 0:10] = 15, 1
    gt[0, 0:6] = 0
    cat[3, 0:10], inst[3, 0:10] = 15, 2
    gt[3, 0:5] = 0
    cases['void_absorb'] = [(pred2ch(cat, inst), id_rgb(gt), segs_of(gt, [(1, 0)]))]
    # crowd absorbing an unmatched pred (6 of 10 pixels on a crowd region of its category); crowd never counts FN
    cat, inst, gt = base()
    cat[0, 0:10], inst[0, 0:10] = 16, 1
    gt[0, 0:6] = 30
    cases['crowd_absorb'] = [(pred2ch(cat, inst), id_rgb(gt), segs_of(gt, [(1, 0), (30, 16)], crowd=(30,)))]
    # two crowd segments of one category: the LAST in JSON order is the crowd region (dict overwritten)
    cat, inst, gt = base()
    cat[0, 0:10], inst[0, 0:10] = 16, 1
    gt[0, 0:8] = 40
    cat[5, 0:10], inst[5, 0:10] = 16, 2
    gt[5, 0:8] = 21
    cases['crowd_last'] = [(pred2ch(cat, inst), id_rgb(gt), segs_of(gt, [(1, 0), (40, 16), (21, 16)], crowd=(40, 21)))]
    # a GT id in the PNG that the JSON lacks: its pixels take part in nothing
    cat, inst, gt = base()
    cat[2:6, 2:6], inst[2:6, 2:6], gt[2:6, 2:6] = 17, 1, 99
    cat[10:14, 2:6], inst[10:14, 2:6], gt[10:14, 2:6] = 17, 2, 98
    cases['gt_missing'] = [(pred2ch(cat, inst), id_rgb(gt), segs_of(gt, [(1, 0), (98, 17), (99, 17)], missing=(99,)))]
    # pred VOID with a non-zero instance: not a segment, whatever the instance
    cat, inst, gt = base()
    cat[0:4, 0:4], inst[0:4, 0:4] = 255, 3
    cat[8:12, 8:12], inst[8:12, 8:12], gt[8:12, 8:12] = 11, 1, 5
    cases['pred_void_inst'] = [(pred2ch(cat, inst), id_rgb(gt), segs_of(gt, [(1, 0), (5, 11)]))]
    # JSON areas that differ from the pixel counts (one larger: no match; one smaller: a match that pixels would not give)
    cat, inst, gt = base()
    cat[0:4, 0:10], inst[0:4, 0:10], gt[0:4, 0:10] = 11, 1, 6
    cat[6:10, 0:10], inst[6:10, 0:10] = 12, 1
    gt[6:10, 0:4] = 8
    cases['area_json'] = [(pred2ch(cat, inst), id_rgb(gt), segs_of(gt, [(1, 0), (6, 11), (8, 12)], area_delta={6: 200, 8: -10}))]
    # things and stuff mixed, several instances of one category, stuff 2 split in two GT segments
    cat, inst, gt = base()
    cat[:, 10:], gt[:, 10:15], gt[:, 15:] = 2, 50, 51
    for j, (y, x) in enumerate([(1, 1), (1, 5), (6, 1), (12, 12)]):
        cat[y:y + 4, x:x + 3], inst[y:y + 4, x:x + 3] = 18, j + 1
        gt[y:y + 4, x:x + 3] = 60 + j
    gt[12:16, 12] = 0
    cases['mixed'] = [(pred2ch(cat, inst), id_rgb(gt), segs_of(gt, [(1, 0), (50, 2), (51, 2), (60, 18), (61, 18), (62, 18), (63, 18)]))]
    # empty segments_info: GT ids all unknown, so every pred segment is an FP
    cat, inst, gt = base()
    cat[2:6, 2:6], inst[2:6, 2:6] = 11, 1
    cases['empty_json'] = [(pred2ch(cat, inst), id_rgb(gt), [])]
    # a sequence of images (IoU sums across images in order)
    seq = []
    for i in range(4):
        cat, inst, gt = base()
        cat[i:i + 7, 3:9], inst[i:i + 7, 3:9] = 11, 1
        gt[2:9, 3:9 + i % 2] = 7
        cat[12:18, 12:18], inst[12:18, 12:18], gt[11:18, 12:18] = 12, 4, 3
        seq.append((pred2ch(cat, inst), id_rgb(gt), segs_of(gt, [(1, 0), (3, 12), (7, 11)])))
    cases['sequence'] = seq
    return cases


def scene_cases():
    """Seeded 256 x 512 scenes: tests/conftest.py::gen_panoptic_maps -> the reference's get_unified_pan_result -> pred; the GT is the
    prediction shifted by a few pixels, with random GT ids, VOID noise, one crowd segment and one segment missing from the JSON."""
    sys.path.insert(0, os.path.dirname(HERE))
    from conftest import gen_panoptic_maps
    config.dataset = mgb.mg.EasyDict(num_classes=9, num_seg_classes=19)
    cases = {}
    for s in range(3):
        rng = np.random.default_rng(100 + s)
        seg, pan, cls_ind = gen_panoptic_maps(rng, 256, 512, 30)
        pred = BaseDataset.get_unified_pan_result(None, [seg], [pan], [cls_ind], stuff_area_limit=300)[0]
        key = np.roll(pred[:, :, 0].astype(np.int64) * 256 + pred[:, :, 1], (int(rng.integers(-3, 4)), int(rng.integers(-6, 7))), (0, 1))
        keys = [k for k in np.unique(key) if k >> 8 != 255]
        ids = rng.choice(np.arange(1, 1 << 24), size=len(keys), replace=False)
        gt = np.zeros(key.shape, np.int64)
        for k, i in zip(keys, ids):
            gt[key == k] = i
        gt[rng.random(gt.shape) < 0.02] = 0
        pairs = [(int(i), int(k >> 8)) for k, i in zip(keys, ids)]
        rng.shuffle(pairs)
        things = [i for i, c in pairs if c >= 11]
        info = segs_of(gt, pairs, crowd=things[:1], missing=things[1:2])
        cases['scene%d' % s] = [(pred, id_rgb(gt), info)]
    return cases


def confusion_cases():
    """GT labels go in as float32, as evaluate_ssegs reads them (cityscapes.py:451): a uint8 array would make the reference's
    gt * class_num wrap in uint8 instead of the int32 index it intends."""
    rng = np.random.default_rng(5)
    out = {}
    C = 19
    gt = rng.integers(0, C, 5000).astype(np.uint8)
    gt[rng.random(5000) < 0.1] = 255
    pred = rng.integers(0, C, 5000).astype(np.uint8)
    keep = gt != 255                                 # cityscapes.py:460-462
    out['cm_ignore'] = (gt, pred, C, 255, BaseDataset.get_confusion_matrix(None, gt[keep].astype(np.float32), pred[keep], C))
    pred2 = pred.copy()
    pred2[rng.random(5000) < 0.1] = rng.integers(C, 40, 1)[0]   # pred >= C: aliases into another cell
    out['cm_alias'] = (gt, pred2, C, -1, BaseDataset.get_confusion_matrix(None, gt.astype(np.float32), pred2, C))
    gt3 = rng.integers(0, 7, (37, 53)).astype(np.uint8)
    pred3 = rng.integers(0, 9, (37, 53)).astype(np.uint8)
    out['cm_small'] = (gt3, pred3, 7, -1, BaseDataset.get_confusion_matrix(None, gt3.reshape(-1).astype(np.float32), pred3.reshape(-1), 7))
    return out


def main():
    out = {'categories': np.array(json.dumps(list(CATEGORIES.values())))}
    cases = dict(hand_cases())
    cases.update(scene_cases())
    for name, images in cases.items():
        stat, results = ref_score(images)
        out[name + '_n'] = np.array(len(images))
        for i, (pred, gt, info) in enumerate(images):
            out['%s_%d_pred' % (name, i)] = pred
            out['%s_%d_gt' % (name, i)] = gt
            out['%s_%d_segs' % (name, i)] = np.array(json.dumps(info))
        cnt = np.zeros((3, 256), np.int64)
        iou = np.zeros(256, np.float64)
        for c, s in stat.pq_per_cat.items():
            cnt[:, c] = (s.tp, s.fp, s.fn)
            iou[c] = s.iou
        out[name + '_counts'] = cnt
        out[name + '_iou'] = iou
        out[name + '_results'] = np.array(json.dumps(results, default=float))
    for name, (gt, pred, C, ignore, cm) in confusion_cases().items():
        out.update({name + '_gt': gt, name + '_pred': pred, name + '_C': np.array(C), name + '_ignore': np.array(ignore), name + '_cm': cm})
    out['cases'] = np.array(sorted(cases))
    path = os.path.join(HERE, 'pq.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, '%d cases' % len(cases), '%d bytes' % os.path.getsize(path))


if __name__ == '__main__':
    main()
