"""Seeded random scenes for the Cityscapes instance-level AP tests: uint16 instance-id maps with stuff and void bands, instances, small
instances (< 100 pixels) and group regions of the eight classes, and predictions around them (jittered copies, duplicates, copies of
another class, boxes at random). Class roles, so that every AP case occurs: bus (5) only ever has group or small regions (no valid GT:
NaN, with predictions), train (6) has GT and never a prediction (0.0), motorcycle (7) has neither (NaN)."""
import numpy as np

LABEL_IDS = (24, 25, 26, 27, 28, 31, 32, 33)
# bands of the background: stuff labels, void labels (0 1 3 4 29 30), a caravan instance (29003: not void) and a licence plate region
BAND_VALUES = (7, 8, 11, 21, 23, 0, 1, 4, 29, 30, 29003, 3, 17, 20)
SIZES = [(1024, 2048), (67, 131), (129, 65), (64, 64), (1, 300), (300, 1), (37, 1000)]

# name: (seed, image sizes, regions per image) of the scene lists the GPU tests run; tests/test_cityscapes_inst_cpu.py asserts that
# each reaches every branch of the rules
GPU_SCENES = {'full': (1, [(1024, 2048)] * 2, 30), 'odd': (1, SIZES[1:], 14)}


def _shape_mask(H, W, box, ellipse):
    y0, x0, y1, x1 = box
    m = np.zeros((H, W), bool)
    if y1 <= y0 or x1 <= x0:
        return m
    if not ellipse:
        m[y0:y1, x0:x1] = True
        return m
    yy = (np.arange(y0, y1) + 0.5 - (y0 + y1) / 2.0) / ((y1 - y0) / 2.0)
    xx = (np.arange(x0, x1) + 0.5 - (x0 + x1) / 2.0) / ((x1 - x0) / 2.0)
    m[y0:y1, x0:x1] = (yy[:, None] ** 2 + xx[None, :] ** 2) <= 1.0
    return m


def _rand_box(rng, H, W, lo, hi):
    h = int(min(H, max(1, rng.integers(lo, hi + 1))))
    w = int(min(W, max(1, rng.integers(lo, hi + 1))))
    if H == 1 or W == 1:       # one-pixel-wide maps: long thin regions
        h, w = (1, int(min(W, max(1, rng.integers(lo * lo, hi * 4 + 1))))) if H == 1 else (int(min(H, max(1, rng.integers(lo * lo, hi * 4 + 1)))), 1)
    y0 = int(rng.integers(0, H - h + 1))
    x0 = int(rng.integers(0, W - w + 1))
    return (y0, x0, y0 + h, x0 + w)


def _jitter(rng, H, W, box, amount):
    y0, x0, y1, x1 = box
    h, w = y1 - y0, x1 - x0
    d = [int(round(rng.normal(0, amount) * s)) for s in (h, w, h, w)]
    y0, x0, y1, x1 = y0 + d[0], x0 + d[1], y1 + d[2], x1 + d[3]
    y0, y1 = max(0, min(y0, H - 1)), max(1, min(y1, H))
    x0, x1 = max(0, min(x0, W - 1)), max(1, min(x1, W))
    return (y0, x0, max(y1, y0 + 1), max(x1, x0 + 1))


def make_image(rng, H, W, n_regions=14, extent=None):
    """(gt uint16 [H, W], predictions [{'cls', 'conf' (np.float32), 'mask' bool [H, W]}])."""
    ext = extent or max(6, int(min(max(H, W) / 5, 260)))
    gt = np.zeros((H, W), np.uint16)
    # background bands along the longer side
    long_side = W if W >= H else H
    n_bands = int(rng.integers(4, 9))
    cuts = np.sort(rng.choice(np.arange(1, long_side), size=min(n_bands, long_side - 1), replace=False)) if long_side > 1 else np.array([], int)
    edges = np.concatenate([[0], cuts, [long_side]])
    for a, b in zip(edges[:-1], edges[1:]):
        v = BAND_VALUES[int(rng.integers(0, len(BAND_VALUES)))]
        if W >= H:
            gt[:, a:b] = v
        else:
            gt[a:b, :] = v
    regions = []
    for k in range(n_regions):
        cls = int(rng.choice([1, 1, 2, 3, 3, 3, 4, 5, 6, 8]))
        kind = rng.choice(['inst', 'inst', 'inst', 'small', 'group'])
        if cls == 5 and kind == 'inst':
            kind = 'group'
        if cls == 6 and kind != 'inst':
            kind = 'inst'
        if kind == 'small':
            box = _rand_box(rng, H, W, 2, 9)       # at most 81 pixels
            if H == 1 or W == 1:
                box = (box[0], box[1], min(box[2], box[0] + 60), min(box[3], box[1] + 60))
        else:
            box = _rand_box(rng, H, W, 12, ext)
        ellipse = bool(rng.integers(0, 2)) and H > 1 and W > 1
        m = _shape_mask(H, W, box, ellipse)
        value = LABEL_IDS[cls - 1] if kind == 'group' else LABEL_IDS[cls - 1] * 1000 + k
        gt[m] = value
        regions.append((cls, kind, box, ellipse))
    preds = []

    def add(cls, box, ellipse):
        conf = np.float32(rng.integers(1, 17) / 16.0)        # few distinct scores: ties within and across images
        preds.append({'cls': int(cls), 'conf': conf, 'mask': _shape_mask(H, W, box, ellipse)})

    for cls, kind, box, ellipse in regions:
        if cls == 6:
            continue                                             # train: never predicted
        r = rng.random()
        if r < 0.15:
            continue
        copies = 1 if r < 0.7 else 2
        for _ in range(copies):
            amount = float(rng.choice([0.0, 0.02, 0.05, 0.1, 0.2]))
            add(cls, _jitter(rng, H, W, box, amount), ellipse)
        if rng.random() < 0.15:
            add(int(rng.choice([1, 2, 3, 4, 8])), box, ellipse)  # the same pixels as another class
    for _ in range(max(2, n_regions // 3)):                     # boxes at random: void bands, stuff, several regions at once
        add(int(rng.choice([1, 2, 3, 4, 5, 8])), _rand_box(rng, H, W, 4, ext), bool(rng.integers(0, 2)) and H > 1 and W > 1)
    if rng.random() < 0.5:
        preds.append({'cls': 3, 'conf': np.float32(0.5), 'mask': np.zeros((H, W), bool)})     # a mask of no pixels
    order = rng.permutation(len(preds))
    return gt, [preds[i] for i in order]


def make_scene(seed, sizes, n_regions=14):
    rng = np.random.default_rng(seed)
    return [make_image(rng, H, W, n_regions) for H, W in sizes]


def rle_of(mask):
    """A bool [H, W] mask as a COCO RLE dict with the counts as a plain list (column-major run lengths, zeros first)."""
    flat = mask.T.reshape(-1).astype(np.int8)
    change = np.nonzero(np.diff(np.concatenate([[0], flat])))[0]
    counts = np.diff(np.concatenate([[0], change, [flat.size]])).tolist()
    return {'size': [int(mask.shape[0]), int(mask.shape[1])], 'counts': counts}


def per_class_results(preds, string_counts=None):
    """The predictions of one image as results_list.pkl holds them: (dets_per_class, rles_per_class, order) with index 0 the
    background; order = the indices of `preds` in the order add_rle sees them (classes ascending). string_counts: a function that
    turns a counts list into the compressed string (the tests pass the product's rle_to_string); None keeps the lists."""
    dets, rles, order = [[]], [[]], []
    for c in range(1, 9):
        idx = [i for i, p in enumerate(preds) if p['cls'] == c]
        order += idx
        d = np.zeros((len(idx), 5), np.float32)
        d[:, 4] = [preds[i]['conf'] for i in idx]
        r = [rle_of(preds[i]['mask']) for i in idx]
        if string_counts is not None:
            r = [{'size': x['size'], 'counts': string_counts(x['counts'])} for x in r]
        dets.append(d)
        rles.append(r)
    return dets, rles, order
