"""Numpy restatement of Boundary PQ: the boundary bits of a label map by two saturated run-length sweeps, and
test_pq_cpu.pq_restated's structure with every pair scored by min(mask IoU, boundary IoU). The random scenes that the CPU and the GPU
tests share are listed here and restated once per process."""
import functools

import numpy as np

import boundary_ref
from test_pq_cpu import rgb_to_id
from test_pq_gpu import id_rgb, scene

PRED_VOID = 255 * 256            # the one label of every pred pixel with cat == 255


def pred_labels(pred_2ch):
    pred = np.asarray(pred_2ch)
    cat, inst = pred[..., 0].astype(np.int64), pred[..., 1].astype(np.int64)
    return np.where(cat == 255, PRED_VOID, cat * 256 + inst)


def _runs(eq, ok, d, axis):
    """Saturated run length (<= d + 1) ending at each position along `axis`: ok ? (eq-with-previous and previous ok ? previous + 1 : 1)
    : 0, eq[i] comparing position i with i - 1."""
    ok, eq = np.moveaxis(ok, axis, 0), np.moveaxis(eq, axis, 0)
    run = np.zeros(ok.shape, np.int64)
    run[0] = ok[0]
    for i in range(1, ok.shape[0]):
        run[i] = np.where(ok[i], np.where(eq[i] & ok[i - 1], np.minimum(run[i - 1] + 1, d + 1), 1), 0)
    return np.moveaxis(run, 0, axis)


def _both_ways(labels, ok, d, axis):
    eq = np.zeros(labels.shape, bool)
    sl = [slice(None)] * 2
    a, b = list(sl), list(sl)
    a[axis], b[axis] = slice(1, None), slice(None, -1)
    eq[tuple(a)] = labels[tuple(a)] == labels[tuple(b)]
    fwd = _runs(eq, ok, d, axis)
    flip = lambda v: np.flip(v, axis)
    eq_back = np.zeros(labels.shape, bool)
    eq_back[tuple(a)] = flip(labels)[tuple(a)] == flip(labels)[tuple(b)]
    back = flip(_runs(eq_back, flip(ok), d, axis))
    return (fwd > d) & (back > d)


def label_boundary(labels, d):
    """bool [H,W]: not interior, interior = the (2d+1)^2 window centred on the pixel lies in the image and holds the pixel's label.
    Along a row the run lengths of equal labels ending at / starting from each pixel, saturated at d + 1: rowok = both > d; down a
    column the same over "equal label and rowok": interior iff both > d."""
    labels = np.asarray(labels)
    rowok = _both_ways(labels, np.ones(labels.shape, bool), d, 1)
    return ~_both_ways(labels, rowok, d, 0)


def boundary_bits(pred_2ch=None, gt_rgb=None, ratio=0.02, d=None):
    """uint8 [H,W]: bit 0 = GT boundary, bit 1 = pred boundary (0 for a map not given)."""
    shape = np.asarray(pred_2ch if pred_2ch is not None else gt_rgb).shape[:2]
    d = boundary_ref.dilation(shape[0], shape[1], ratio) if d is None else d
    out = np.zeros(shape, np.uint8)
    if gt_rgb is not None:
        out |= label_boundary(rgb_to_id(gt_rgb), d).astype(np.uint8)
    if pred_2ch is not None:
        out |= label_boundary(pred_labels(pred_2ch), d).astype(np.uint8) << 1
    return out


def _count(keys):
    u, c = np.unique(keys, return_counts=True)
    return dict(zip(u.tolist(), c.tolist()))


def boundary_counts(pred, gt, d):
    """The integer counts of one image over the pixels whose pred is valid: area_p / area_bp [key], inter / inter_b [gid * 65536 + key]
    (gid 0 = VOID: inter[key] and void_b[key]), area_bg [gid]."""
    pred = np.asarray(pred)
    valid = pred[..., 0] != 255
    lab_p, gid_full = pred_labels(pred), rgb_to_id(gt)
    bp, bg = label_boundary(lab_p, d)[valid], label_boundary(gid_full, d)[valid]
    pkey, gid = lab_p[valid], gid_full[valid]
    pair = gid * 65536 + pkey
    return dict(area_p=_count(pkey), inter=_count(pair), area_bp=_count(pkey[bp]), area_bg=_count(gid[bg]), inter_b=_count(pair[bp & bg]),
                void_b=_count(pkey[bp & (gid == 0)]))


def boundary_pq_restated(images, categories, ratio=0.02):
    """pq_restated with the boundary rule: -> tp, fp, fn (int64 [256]), iou (float64 [256]). A pair with inter > 0, equal category
    and non-crowd GT has iou = min(iou_m, iou_b), iou_m = inter / (area_p + json_area_g - inter - inter(VOID, p)) as in pq_restated,
    iou_b = inter_b / (area_bp + area_bg - inter_b - void_b) over pixel counts (0 when that union is empty); TP iff iou > 0.5, and
    iou is what is added. FN, FP (mask counts decide the absorption) and the summation order are pq_restated's."""
    tp, fp, fn = (np.zeros(256, np.int64) for _ in range(3))
    iou = np.zeros(256, np.float64)
    for idx, (pred, gt, info) in enumerate(images):
        H, W = np.asarray(pred).shape[:2]
        c = boundary_counts(pred, gt, boundary_ref.dilation(H, W, ratio))
        area_p, inter = c['area_p'], c['inter']
        for k in area_p:
            if k >> 8 not in categories:
                raise KeyError('image %d: unknown category_id %d' % (idx, k >> 8))
        segs = {el['id']: el for el in info}
        matched_g, matched_p = set(), set()
        for pair, x in sorted(inter.items()):                       # ascending GT id, then key (= instance within a category)
            g, k = pair >> 16, pair & 65535
            s = segs.get(g)
            if s is None or s['iscrowd'] == 1 or s['category_id'] != k >> 8:
                continue
            union = area_p[k] + s['area'] - x - inter.get(k, 0)
            with np.errstate(divide='ignore', invalid='ignore'):
                iou_m = np.float64(x) / np.float64(union)
            xb = c['inter_b'].get(pair, 0)
            union_b = c['area_bp'].get(k, 0) + c['area_bg'].get(g, 0) - xb - c['void_b'].get(k, 0)
            iou_b = np.float64(xb) / np.float64(union_b) if union_b > 0 else np.float64(0.0)
            v = iou_b if iou_b < iou_m else iou_m
            if v > 0.5:
                cat = s['category_id']
                tp[cat] += 1
                iou[cat] += v
                matched_g.add(g)
                matched_p.add(k)
        crowd = {}
        for g, s in segs.items():
            if g in matched_g:
                continue
            if s['iscrowd'] == 1:
                crowd[s['category_id']] = g
                continue
            fn[s['category_id']] += 1
        for k, a in area_p.items():
            if k in matched_p:
                continue
            x = inter.get(k, 0)
            if k >> 8 in crowd:
                x += inter.get(crowd[k >> 8] * 65536 + k, 0)
            if x / a > 0.5:
                continue
            fp[k >> 8] += 1
    return tp, fp, fn, iou


# ------------------------------------------------------------------------------------------------------------------ shared inputs
CATS = {c: {'id': c, 'isthing': int(c >= 11)} for c in range(19)}
HAND_CATS = {1: {'id': 1, 'isthing': 1}, 2: {'id': 2, 'isthing': 0}}


def hand_case():
    """The issue's 40 x 60 case (d = 1): GT id 1 = cat 1 on rows 10..29 x columns 10..39, id 2 = cat 2 on the rest; pred the same
    rectangle two columns to the right."""
    H, W = 40, 60
    gid = np.full((H, W), 2, np.int64)
    gid[10:30, 10:40] = 1
    pred = np.zeros((H, W, 3), np.uint8)
    pred[..., 0] = 2
    pred[10:30, 12:42, 0] = 1
    info = [{'id': 1, 'category_id': 1, 'iscrowd': 0, 'area': 600}, {'id': 2, 'category_id': 2, 'iscrowd': 0, 'area': 1800}]
    return pred, id_rgb(gid), info


# name -> (H, W, gh, gw, seed, scene keywords): crowds, VOID specks sparse enough to leave interiors at the image's d, ids missing
# from the JSON
SCENES = {
    'small0': (96, 160, 3, 4, 100, dict(void=0.004, shift=(1, -1), crowd=0.2)),
    'small1': (96, 160, 2, 3, 101, dict(void=0.004, shift=(0, 1), crowd=0.3)),
    'small_jitter': (96, 160, 3, 3, 282, dict(void=0.004, shift=(0, 1), area_jitter=True, crowd=0.2)),
    'odd': (37, 53, 2, 2, 103, dict(void=0.01, shift=(1, 0), missing=0)),
    'full': (1024, 2048, 8, 12, 104, dict(void=1e-5, shift=(14, -20))),
    'mid_jitter': (512, 768, 5, 6, 115, dict(void=1e-4, area_jitter=True, shift=(5, 6))),
}
SMALL_SCENES = ['small0', 'small1', 'small_jitter', 'odd']


@functools.lru_cache(maxsize=None)
def scene_images(name):
    H, W, gh, gw, seed, kw = SCENES[name]
    return [scene(np.random.default_rng(seed), H, W, gh, gw, **kw)]


@functools.lru_cache(maxsize=None)
def scene_restated(name, ratio=0.02):
    return boundary_pq_restated(scene_images(name), CATS, ratio)
