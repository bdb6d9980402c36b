"""CPU: a numpy restatement of pycocotools' COCOeval (evaluate -> accumulate -> summarize, default Params, iouType 'bbox' / 'segm'),
written from its published algorithm and pinned here by hand-derived cases (pycocotools itself is not a dependency). The device
evaluator (dataset/coco_eval.py) is checked bit for bit against it in test_coco_eval_gpu.py. Also: the RLE string decoder and the
host-side refusals of DetectionEvaluator."""
import numpy as np
import pytest
import torch

from upsnet_amd.dataset import coco_eval
from upsnet_amd.dataset.coco_eval import AREA_RNG, IOU_THRS, MAX_DETS, REC_THRS, DetectionEvaluator, summarize_stats


# ------------------------------------------------------------------------------------------------------------------ restatement
def bb_iou(d, g, iscrowd):
    """maskApi.c bbIou: d [D,4], g [G,4] xywh -> [D,G]."""
    o = np.zeros((len(d), len(g)))
    for gi, G in enumerate(g):
        ga = G[2] * G[3]
        for di, D in enumerate(d):
            da = D[2] * D[3]
            w = min(D[2] + D[0], G[2] + G[0]) - max(D[0], G[0])
            if w <= 0:
                continue
            h = min(D[3] + D[1], G[3] + G[1]) - max(D[1], G[1])
            if h <= 0:
                continue
            i = w * h
            u = da if iscrowd[gi] else da + ga - i
            o[di, gi] = i / u
    return o


def mask_iou(d, g, iscrowd):
    """maskApi.c rleIou on decoded masks: integer intersection / union (det area for a crowd GT), 0 when they do not intersect."""
    o = np.zeros((len(d), len(g)))
    for gi, G in enumerate(g):
        for di, D in enumerate(d):
            i = int(np.count_nonzero(D & G))
            if i == 0:
                continue
            u = int(np.count_nonzero(D)) if iscrowd[gi] else int(np.count_nonzero(D | G))
            o[di, gi] = float(i) / float(u)
    return o


def cocoeval_restated(images, cat_ids, iou_type='bbox'):
    """images: list of (image_id, gts, dts). gts: dicts with id, category_id, iscrowd, area, bbox (xywh) and for 'segm' mask (bool
    [H,W]); dts: dicts with category_id, score, bbox (xywh) or mask. Returns (precision, recall, scores, stats) as pycocotools'."""
    img_ids = sorted(set(int(i) for i, _, _ in images))
    cat_ids = sorted(set(cat_ids))
    gts, dts = {}, {}
    for image_id, g, d in images:
        for el in g:
            if el['category_id'] in cat_ids:
                gts.setdefault((image_id, el['category_id']), []).append(dict(el, ignore=int(bool(el.get('iscrowd', 0)))))
        for n, el in enumerate(d):
            if el['category_id'] in cat_ids:
                area = el['bbox'][2] * el['bbox'][3] if iou_type == 'bbox' else float(np.count_nonzero(el['mask']))
                dts.setdefault((image_id, el['category_id']), []).append(dict(el, area=area, id=len(dts) * 1000 + n + 1))
    maxd = MAX_DETS[-1]

    def compute_iou(i, c):
        gt, dt = gts.get((i, c), []), dts.get((i, c), [])
        if len(gt) == 0 and len(dt) == 0:
            return []
        inds = np.argsort([-d['score'] for d in dt], kind='mergesort')
        dt = [dt[j] for j in inds][:maxd]
        if len(gt) == 0 or len(dt) == 0:
            return []
        crowd = [int(o['iscrowd']) for o in gt]
        if iou_type == 'bbox':
            return bb_iou([d['bbox'] for d in dt], [g['bbox'] for g in gt], crowd)
        return mask_iou([d['mask'] for d in dt], [g['mask'] for g in gt], crowd)

    ious = {(i, c): compute_iou(i, c) for i in img_ids for c in cat_ids}

    def evaluate_img(i, c, a_rng):
        gt, dt = gts.get((i, c), []), dts.get((i, c), [])
        if len(gt) == 0 and len(dt) == 0:
            return None
        g_ig = [1 if (g['ignore'] or g['area'] < a_rng[0] or g['area'] > a_rng[1]) else 0 for g in gt]
        gtind = np.argsort(g_ig, kind='mergesort')
        gt = [gt[j] for j in gtind]
        dtind = np.argsort([-d['score'] for d in dt], kind='mergesort')
        dt = [dt[j] for j in dtind[0:maxd]]
        crowd = [int(o['iscrowd']) for o in gt]
        io = ious[i, c][:, gtind] if len(ious[i, c]) > 0 else ious[i, c]
        nT, G, D = len(IOU_THRS), len(gt), len(dt)
        gtm, dtm = np.zeros((nT, G)), np.zeros((nT, D))
        gt_ig = np.array([g_ig[j] for j in gtind])
        dt_ig = np.zeros((nT, D))
        if not len(io) == 0:
            for tind, t in enumerate(IOU_THRS):
                for dind, d in enumerate(dt):
                    iou = min([t, 1 - 1e-10])
                    m = -1
                    for gind, g in enumerate(gt):
                        if gtm[tind, gind] > 0 and not crowd[gind]:
                            continue
                        if m > -1 and gt_ig[m] == 0 and gt_ig[gind] == 1:
                            break
                        if io[dind, gind] < iou:
                            continue
                        iou = io[dind, gind]
                        m = gind
                    if m == -1:
                        continue
                    dt_ig[tind, dind] = gt_ig[m]
                    dtm[tind, dind] = gt[m]['id']
                    gtm[tind, m] = d['id']
        a = np.array([d['area'] < a_rng[0] or d['area'] > a_rng[1] for d in dt]).reshape((1, len(dt)))
        dt_ig = np.logical_or(dt_ig, np.logical_and(dtm == 0, np.repeat(a, nT, 0)))
        return {'dtMatches': dtm, 'dtScores': [d['score'] for d in dt], 'gtIgnore': gt_ig, 'dtIgnore': dt_ig}

    nT, nR, nK, nA, nM = len(IOU_THRS), len(REC_THRS), len(cat_ids), len(AREA_RNG), len(MAX_DETS)
    precision, recall, scores = -np.ones((nT, nR, nK, nA, nM)), -np.ones((nT, nK, nA, nM)), -np.ones((nT, nR, nK, nA, nM))
    for k, c in enumerate(cat_ids):
        for a, a_rng in enumerate(AREA_RNG):
            E0 = [evaluate_img(i, c, a_rng) for i in img_ids]
            for m, max_det in enumerate(MAX_DETS):
                E = [e for e in E0 if e is not None]
                if len(E) == 0:
                    continue
                dt_scores = np.concatenate([e['dtScores'][0:max_det] for e in E])
                inds = np.argsort(-dt_scores, kind='mergesort')
                dt_scores_sorted = dt_scores[inds]
                dtm = np.concatenate([e['dtMatches'][:, 0:max_det] for e in E], axis=1)[:, inds]
                dt_ig = np.concatenate([e['dtIgnore'][:, 0:max_det] for e in E], axis=1)[:, inds]
                gt_ig = np.concatenate([e['gtIgnore'] for e in E])
                npig = np.count_nonzero(gt_ig == 0)
                if npig == 0:
                    continue
                tps = np.logical_and(dtm, np.logical_not(dt_ig))
                fps = np.logical_and(np.logical_not(dtm), np.logical_not(dt_ig))
                tp_sum = np.cumsum(tps, axis=1).astype(dtype=np.float64)
                fp_sum = np.cumsum(fps, axis=1).astype(dtype=np.float64)
                for t, (tp, fp) in enumerate(zip(tp_sum, fp_sum)):
                    tp, fp = np.array(tp), np.array(fp)
                    nd = len(tp)
                    rc = tp / npig
                    pr = tp / (fp + tp + np.spacing(1))
                    q, ss = np.zeros((nR,)), np.zeros((nR,))
                    recall[t, k, a, m] = rc[-1] if nd else 0
                    pr, q = pr.tolist(), q.tolist()
                    for i in range(nd - 1, 0, -1):
                        if pr[i] > pr[i - 1]:
                            pr[i - 1] = pr[i]
                    inds = np.searchsorted(rc, REC_THRS, side='left')
                    try:
                        for ri, pi in enumerate(inds):
                            q[ri] = pr[pi]
                            ss[ri] = dt_scores_sorted[pi]
                    except IndexError:
                        pass
                    precision[t, :, k, a, m] = np.array(q)
                    scores[t, :, k, a, m] = np.array(ss)
    stats, _ = summarize_stats(precision, recall)
    return precision, recall, scores, stats


# ------------------------------------------------------------------------------------------------------------------ hand cases
def one(x):
    """Precision 1 up to pycocotools' eps: tp / (fp + tp + 2^-52) is 1 - 2^-52 for tp = 1 and exactly 1 from tp = 2 on."""
    return np.all(np.abs(np.asarray(x) - 1) <= 2.5e-16)
def gt(i, c, bbox, crowd=0, area=None):
    return {'id': i, 'category_id': c, 'iscrowd': crowd, 'bbox': [float(v) for v in bbox],
            'area': float(bbox[2] * bbox[3]) if area is None else float(area)}


def det(c, bbox, score):
    return {'category_id': c, 'bbox': [float(v) for v in bbox], 'score': float(score)}


def test_identical_detection_is_perfect():
    p, r, s, st = cocoeval_restated([(1, [gt(1, 1, [10, 10, 50, 40])], [det(1, [10, 10, 50, 40], 0.9)])], [1])
    assert one(p[:, :, 0, 0, :]) and np.all(r[:, 0, 0, :] == 1) and np.all(s[:, :, 0, 0, :] == 0.9)
    assert one(st[[0, 1, 2, 8]])


def test_box_iou_072():
    # GT 100x100; det shifted so that the overlap is 100 x h with h / (2*10000/100 - h) = 0.72 -> h = 83.720..., IoU 0.72
    h = 2 * 100 * 0.72 / 1.72
    p, r, s, st = cocoeval_restated([(1, [gt(1, 1, [0, 0, 100, 100])], [det(1, [0, 100 - h, 100, 100], 0.8)])], [1])
    assert bb_iou([[0, 100 - h, 100, 100]], [[0, 0, 100, 100]], [0])[0, 0] == pytest.approx(0.72, abs=1e-12)
    keep = IOU_THRS <= 0.70 + 1e-12
    assert one(p[keep, :, 0, 0, 2]) and np.all(p[~keep, :, 0, 0, 2] == 0)
    assert st[0] == pytest.approx(0.5, abs=1e-15) and one(st[1]) and st[2] == 0


def test_false_positive_before_true_positive():
    p, r, s, st = cocoeval_restated([(1, [gt(1, 1, [0, 0, 50, 50])], [det(1, [200, 200, 50, 50], 0.9), det(1, [0, 0, 50, 50], 0.5)])],
                                    [1])
    # tp [0,1], fp [1,1]: pr [0, 0.5] -> envelope [0.5, 0.5]; rc [0, 1]: every recall threshold lands on index 0 or 1 -> 0.5
    assert np.all(p[:, :, 0, 0, 2] == 0.5) and st[0] == 0.5
    assert np.all(s[:, 0, 0, 0, 2] == 0.9) and np.all(s[:, 1:, 0, 0, 2] == 0.5)


def test_crowd_gt_absorbs_detections():
    imgs = [(1, [gt(1, 1, [0, 0, 100, 100]), gt(2, 1, [300, 300, 100, 100], crowd=1)],
             [det(1, [0, 0, 100, 100], 0.9), det(1, [300, 300, 40, 40], 0.8), det(1, [350, 350, 40, 40], 0.7)]),
            (2, [gt(3, 2, [0, 0, 60, 60], crowd=1)], [det(2, [0, 0, 30, 30], 0.6)])]
    p, r, s, st = cocoeval_restated(imgs, [1, 2])
    # both dets inside the crowd region are matched to it and ignored: neither TP nor FP -> precision 1 up to recall 1
    assert one(p[:, :, 0, 0, 2]) and np.all(r[:, 0, 0, 2] == 1)
    # category 2 has only a crowd GT: npig == 0 -> -1
    assert np.all(p[:, :, 1, :, :] == -1) and np.all(r[:, 1, :, :] == -1)


def test_max_dets_one():
    imgs = [(1, [gt(1, 1, [0, 0, 50, 50]), gt(2, 1, [100, 100, 50, 50])], [det(1, [0, 0, 50, 50], 0.9), det(1, [100, 100, 50, 50], 0.8)])]
    p, r, s, st = cocoeval_restated(imgs, [1])
    assert st[6] == 0.5 and st[7] == 1 and st[8] == 1


def test_area_ranges_split():
    # areas 1023 / 1024 (small, the edge is inclusive on both sides) / 1025 (medium) / 9216 (medium and large) / 9217 (large)
    areas = [1023, 1024, 1025, 9216, 9217]
    gts = [gt(i + 1, 1, [200 * i, 0, 10, 10], area=a) for i, a in enumerate(areas)]
    dts = [det(1, [200 * i, 0, 10, 10], 0.9 - 0.1 * i) for i in range(5)]
    p, r, s, st = cocoeval_restated([(1, gts, dts)], [1])
    # det areas are 100 (small): unmatched ones in medium / large are ignored, so every area range has precision 1
    assert one(p[:, :, 0, :, 2]) and np.all(r[:, 0, :, 2] == 1)
    p2, r2, _, _ = cocoeval_restated([(1, gts, [])], [1])
    assert np.all(r2[:, 0, :, 2] == 0) and np.all(p2[:, :, 0, :, 2] == 0)
    # npig per range: small {1023, 1024} = 2, medium {1024, 1025, 9216} = 3, large {9216, 9217} = 2
    _, r3, _, _ = cocoeval_restated([(1, gts, [dts[1]])], [1])
    assert r3[0, 0, 1, 2] == 1 / 2 and r3[0, 0, 2, 2] == 1 / 3 and r3[0, 0, 3, 2] == 0 and r3[0, 0, 0, 2] == 1 / 5


def test_category_without_gt_is_minus_one():
    p, r, s, st = cocoeval_restated([(1, [], [det(1, [0, 0, 10, 10], 0.5)])], [1])
    assert np.all(p == -1) and np.all(r == -1) and np.all(st == -1)


def test_segm_restatement_matches_box_case_on_rectangles():
    H, W = 64, 96
    mg = np.zeros((H, W), bool)
    mg[10:30, 20:60] = True
    md = np.zeros((H, W), bool)
    md[12:30, 20:60] = True
    g = dict(gt(1, 1, [20, 10, 40, 20]), mask=mg)
    d = {'category_id': 1, 'score': 0.7, 'mask': md}
    p, r, s, st = cocoeval_restated([(1, [g], [d])], [1], 'segm')
    iou = 18 * 40 / (20 * 40)
    assert one(p[IOU_THRS <= iou, :, 0, 0, 2]) and np.all(p[IOU_THRS > iou, :, 0, 0, 2] == 0)


# ------------------------------------------------------------------------------------------------------------------ host side
def test_rle_string_round_trip():
    from upsnet_amd.dataset.rle import rle_to_string
    rng = np.random.default_rng(0)
    for trial in range(30):
        H, W = rng.integers(1, 40, 2)
        m = rng.random((H, W)) < rng.uniform(0.05, 0.95)
        if trial % 5 == 0:
            m[:] = trial % 10 == 0
        flat = m.T.reshape(-1).astype(np.int8)   # column-major
        change = np.nonzero(np.diff(np.concatenate([[0], flat])))[0]
        counts = np.diff(np.concatenate([[0], change, [H * W]])).tolist()
        s = rle_to_string(counts)
        assert coco_eval.rle_from_string(s) == counts
        got, hw = coco_eval.rle_counts({'size': [int(H), int(W)], 'counts': s})
        assert hw == (H, W) and got.tolist() == counts
    # large counts (multi-character values, negative differences)
    counts = [0, 2000000, 5, 70000, 1, 3]
    assert coco_eval.rle_from_string(rle_to_string(counts)) == counts


def test_refusals_before_any_launch():
    ev = DetectionEvaluator([24, 25, 26], 'segm')
    seg = {'size': [4, 4], 'counts': [3, 5, 8]}
    boxes, scores, cls, masks = np.zeros((0, 4), np.float32), np.zeros(0, np.float32), np.zeros(0, np.int64), np.zeros((0, 1, 28, 28), np.float32)
    with pytest.raises(ValueError, match='polygon'):
        ev.add(1, [{'id': 1, 'category_id': 24, 'iscrowd': 0, 'area': 4.0, 'bbox': [0, 0, 2, 2], 'segmentation': [[0, 0, 2, 0, 2, 2]]}],
               boxes, scores, cls, masks, image_size=(4, 4))
    with pytest.raises(ValueError, match='id'):
        ev.add(1, [{'id': 0, 'category_id': 24, 'iscrowd': 0, 'area': 4.0, 'bbox': [0, 0, 2, 2], 'segmentation': seg}],
               boxes, scores, cls, masks, image_size=(4, 4))
    with pytest.raises(ValueError, match='differs'):
        ev.add(1, [{'id': 1, 'category_id': 24, 'iscrowd': 0, 'area': 4.0, 'bbox': [0, 0, 2, 2], 'segmentation': seg}],
               boxes, scores, cls, masks, image_size=(4, 5))
    with pytest.raises(ValueError, match='sum'):
        ev.add(1, [{'id': 1, 'category_id': 24, 'iscrowd': 0, 'area': 4.0, 'bbox': [0, 0, 2, 2], 'segmentation': {'size': [4, 4], 'counts': [3, 5]}}],
               boxes, scores, cls, masks, image_size=(4, 4))
    with pytest.raises(ValueError, match='image_size'):
        ev.add(1, [], boxes, scores, cls, masks)
    with pytest.raises(ValueError, match='det_masks'):
        ev.add(1, [], boxes, scores, cls, None, image_size=(4, 4))
    with pytest.raises(ValueError):
        ev.add(1, [], np.zeros((3, 5), np.float32), np.zeros(3, np.float32), np.zeros(3, np.int64), np.zeros((3, 1, 28, 28), np.float32), image_size=(4, 4))
    with pytest.raises(ValueError):
        ev.add(1, [], np.zeros((3, 4), np.float32), np.zeros(2, np.float32), np.zeros(3, np.int64), np.zeros((3, 1, 28, 28), np.float32), image_size=(4, 4))
    with pytest.raises(ValueError):
        ev.add(1, [], np.zeros((3, 4), np.float32), np.zeros(3, np.float32), np.zeros(3, np.float32), np.zeros((3, 1, 28, 28), np.float32), image_size=(4, 4))
    with pytest.raises(ValueError):
        ev.add(1, [], np.zeros((3, 4), np.float32), np.zeros(3, np.float32), np.zeros(3, np.int64), np.zeros((3, 2, 28, 28), np.float32), image_size=(4, 4))
    bev = DetectionEvaluator([1, 2], 'bbox')
    with pytest.raises(ValueError, match='id'):
        bev.add_rle(7, [{'id': -3, 'category_id': 1, 'iscrowd': 0, 'area': 4.0, 'bbox': [0, 0, 2, 2]}], [[], np.zeros((1, 5))])
    bev.image_ids.append(7)   # as after a successful add
    bev._ids.add(7)
    with pytest.raises(ValueError, match='twice'):
        bev.add_rle(7, [], [[], np.zeros((1, 5))])
    with pytest.raises(ValueError):
        DetectionEvaluator([1, 1])
    with pytest.raises(ValueError):
        DetectionEvaluator([1], 'keypoints')


def test_summary_text_of_restated_arrays():
    p, r, s, st = cocoeval_restated([(1, [gt(1, 1, [10, 10, 50, 40])], [det(1, [10, 10, 50, 40], 0.9)])], [1, 2])
    res = dict(precision=p, recall=r, scores=s, category_ids=[1, 2])
    res['stats'], res['summary_lines'] = summarize_stats(p, r)
    lines = coco_eval.detection_metrics_lines(res)
    assert lines[0] == '~~~~ Mean and per-category AP @ IoU=[0.50,0.95] ~~~~'
    assert lines[1:4] == ['1.000', 'nan', '1.000']
    assert lines[-12] == ' Average Precision  (AP) @[ IoU=0.50:0.95 | area=   all | maxDets=100 ] = 1.000'
    assert lines[-1] == ' Average Recall     (AR) @[ IoU=0.50:0.95 | area= large | maxDets=100 ] = -1.000'
