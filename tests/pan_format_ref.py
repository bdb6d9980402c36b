"""numpy restatements for the COCO panoptic format tests (plain helper module, no fixtures), written from the behaviour of the
reference's BaseDataset._converter_2ch_single_core (without vis_panoptic) and of the general _pq_compute_single_core on
(PNG, JSON) pairs, sanity checks included."""
import numpy as np


def rgb_to_id(rgb):
    rgb = np.asarray(rgb).astype(np.int64)
    return rgb[..., 0] + 256 * rgb[..., 1] + 65536 * rgb[..., 2]


def convert_2ch(pan_2ch, color_fn):
    """One 2-channel map (uint8 [H,W,3]: category, instance) -> (rgb uint8 [H,W,3], segments_info). Segments are the distinct
    (category, instance) pairs with category != 255, visited in ascending category * 256 + instance (the order np.unique gives the
    reference's 1000 * category + instance); color_fn(category) is called once per segment in that order and returns [R, G, B].
    area = pixel count; bbox = [x_min, y_min, x_max - x_min, y_max - y_min], the reference's arithmetic. All-pixel reductions are done
    with one sort instead of one mask per segment, so that maps of tens of thousands of segments stay affordable."""
    pan_2ch = np.asarray(pan_2ch)
    H, W = pan_2ch.shape[:2]
    key = pan_2ch[..., 0].astype(np.int64) * 256 + pan_2ch[..., 1]
    keys, inv, counts = np.unique(key.reshape(-1), return_inverse=True, return_counts=True)
    inv = inv.reshape(-1)
    order = np.argsort(inv, kind='stable')
    starts = np.cumsum(counts) - counts
    ys, xs = np.divmod(order, W)
    x_min, x_max = np.minimum.reduceat(xs, starts), np.maximum.reduceat(xs, starts)
    y_min, y_max = np.minimum.reduceat(ys, starts), np.maximum.reduceat(ys, starts)
    lut = np.zeros((len(keys), 3), np.uint8)
    info = []
    for j, k in enumerate(keys.tolist()):
        sem = k >> 8
        if sem == 255:
            continue
        color = [int(v) for v in color_fn(sem)]
        lut[j] = color
        info.append({'id': color[0] + 256 * color[1] + 65536 * color[2], 'category_id': sem, 'iscrowd': 0,
                     'bbox': [int(x_min[j]), int(y_min[j]), int(x_max[j] - x_min[j]), int(y_max[j] - y_min[j])], 'area': int(counts[j])})
    return lut[inv].reshape(H, W, 3), info


def pq_general(images, categories):
    """PQ of (pred_rgb, pred_segments_info, gt_rgb, gt_segments_info) tuples, one image after another -> tp, fp, fn (int64 [256]),
    iou (float64 [256]). Ids are R + 256 G + 65536 B, 0 = VOID on both sides. Checks first, each a KeyError naming the image index
    and the id: a non-zero id of the pred PNG that is not in its JSON; a pred segment whose category is not in `categories`; a pred
    segment of the JSON without a pixel. The pred area is the pixel count, whatever the JSON says; the GT area is the JSON's.
    Match: same category, non-crowd GT, inter / (area_p + area_g - inter - inter(VOID, p)) > 0.5 in float64, added per category in
    ascending (GT id, pred id). FN: unmatched non-crowd GT. FP: unmatched pred unless (inter(VOID, p) + inter(last crowd GT of its
    category, p)) / area_p > 0.5."""
    tp, fp, fn = (np.zeros(256, np.int64) for _ in range(3))
    iou = np.zeros(256, np.float64)
    for idx, (pred_rgb, pred_info, gt_rgb, gt_info) in enumerate(images):
        pid, gid = rgb_to_id(pred_rgb).reshape(-1), rgb_to_id(gt_rgb).reshape(-1)
        preds = {el['id']: el['category_id'] for el in pred_info}
        gts = {el['id']: el for el in gt_info}
        labels, label_counts = np.unique(pid, return_counts=True)
        area_p = {}
        for label, count in zip(labels.tolist(), label_counts.tolist()):
            if label not in preds:
                if label == 0:
                    continue
                raise KeyError('image %d: segment %d is in the PNG and not in the JSON' % (idx, label))
            area_p[label] = count
            if preds[label] not in categories:
                raise KeyError('image %d: segment %d has unknown category_id %d' % (idx, label, preds[label]))
        absent = sorted(set(preds) - set(area_p))
        if absent:
            raise KeyError('image %d: segments %s are in the JSON and not in the PNG' % (idx, absent))
        pairs, counts = np.unique(gid * (1 << 24) + pid, return_counts=True)
        inter = dict(zip(pairs.tolist(), counts.tolist()))
        matched_g, matched_p = set(), set()
        for pair, x in zip(pairs.tolist(), counts.tolist()):
            g, p = pair >> 24, pair & 0xffffff
            s = gts.get(g)
            if s is None or p not in preds or s['iscrowd'] == 1 or s['category_id'] != preds[p]:
                continue
            union = area_p[p] + s['area'] - x - inter.get(p, 0)
            with np.errstate(divide='ignore'):
                v = np.float64(x) / np.float64(union)
            if v > 0.5:
                c = s['category_id']
                tp[c] += 1
                iou[c] += v
                matched_g.add(g)
                matched_p.add(p)
        crowd = {}
        for g, s in gts.items():
            if g in matched_g:
                continue
            if s['iscrowd'] == 1:
                crowd[s['category_id']] = g
                continue
            fn[s['category_id']] += 1
        for p, a in area_p.items():
            if p in matched_p:
                continue
            x = inter.get(p, 0)
            if preds[p] in crowd:
                x += inter.get(crowd[preds[p]] * (1 << 24) + p, 0)
            if x / a > 0.5:
                continue
            fp[preds[p]] += 1
    return tp, fp, fn, iou
