"""Seeded random scenes for the Cityscapes pixel-level IoU / iIoU tests: an instance-id map of background bands (stuff, void and
ignore-in-eval labels, group regions, caravan / trailer instances, a stuff label with an instance-like value), instances of the eight
classes on top (instance number 0 included), the label-id map that belongs to it, and a prediction derived from the ground truth
(shifted, with blobs of other labels) either as train ids (the network's output) or as label ids (a submission: ignored labels
occur as predictions too). Class roles, so that every score case occurs: train (31) has instances and is never predicted on its own
pixels, motorcycle (32) occurs neither in the ground truth nor in a prediction (NaN, leaves the mean)."""
import numpy as np

TRAIN2LABEL = np.array([7, 8, 11, 12, 13, 17, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 31, 32, 33])
INSTANCE_LABELS = (24, 25, 26, 27, 28, 31, 33)          # (32 never occurs)
# bands: stuff, void, ignore-in-eval, group regions (bare label ids of instance classes), a caravan and a trailer instance, a
# licence-plate-like stuff value with an instance number
BAND_VALUES = (7, 8, 11, 12, 13, 17, 19, 20, 21, 22, 23, 0, 1, 4, 6, 9, 10, 14, 18, 26, 24, 29, 30, 29003, 30001, 7005)
SPECIAL_VALUES = (29003, 30001, 7005, 26, 0, 9)
SIZES = [(1024, 2048), (67, 131), (129, 65), (64, 64), (1, 300), (300, 1), (37, 1000), (5, 3)]

# name: (seed, image sizes, instances per image) of the scene lists the GPU tests run; tests/test_cityscapes_pixel_cpu.py asserts
# that each reaches every branch of the rules
GPU_SCENES = {'full': (3, [(1024, 2048)] * 2, 40), 'odd': (5, SIZES[1:], 12)}


def labels_of(ids):
    """The label-id map that belongs to an instance-id map: v // 1000 for v >= 1000, else v."""
    return np.where(ids >= 1000, ids // 1000, ids).astype(np.uint8)


def _blob(rng, H, W, lo, hi):
    h = int(min(H, max(1, rng.integers(lo, hi + 1))))
    w = int(min(W, max(1, rng.integers(lo, hi + 1))))
    if H == 1:
        w = int(min(W, max(1, rng.integers(lo * lo, hi * 3 + 1))))
    if W == 1:
        h = int(min(H, max(1, rng.integers(lo * lo, hi * 3 + 1))))
    y0, x0 = int(rng.integers(0, H - h + 1)), int(rng.integers(0, W - w + 1))
    m = np.zeros((H, W), bool)
    if h > 2 and w > 2 and rng.integers(0, 2):
        yy = (np.arange(h) + 0.5 - h / 2.0) / (h / 2.0)
        xx = (np.arange(w) + 0.5 - w / 2.0) / (w / 2.0)
        m[y0:y0 + h, x0:x0 + w] = (yy[:, None] ** 2 + xx[None, :] ** 2) <= 1.0
    else:
        m[y0:y0 + h, x0:x0 + w] = True
    return m


def make_image(rng, H, W, n_inst=12, train_ids=True, noise=True):
    """(gt_labels uint8, gt_ids uint16, pred uint8 -- train ids or label ids). noise: where the shifted ground truth holds an
    ignored label the prediction is a random label per pixel (the hard case for the counting kernel); without it, road."""
    ext = max(4, int(min(max(H, W) / 5, 220)))
    ids = np.zeros((H, W), np.uint16)
    long_side = max(H, W)
    n_bands = int(rng.integers(4, 10))
    cuts = np.sort(rng.choice(np.arange(1, long_side), size=min(n_bands, long_side - 1), replace=False)) if long_side > 1 else np.array([], int)
    edges = np.concatenate([[0], cuts, [long_side]])
    for a, b in zip(edges[:-1], edges[1:]):
        v = BAND_VALUES[int(rng.integers(0, len(BAND_VALUES)))]
        if W >= H:
            ids[:, a:b] = v
        else:
            ids[a:b, :] = v
    step = long_side // (2 * len(SPECIAL_VALUES))
    for j, v in enumerate(SPECIAL_VALUES if step else ()):  # thin strips of the values whose rule every image should meet
        if W >= H:
            ids[: max(1, H // 3), j * step:j * step + max(1, step // 2)] = v
        else:
            ids[j * step:j * step + max(1, step // 2), : max(1, W // 3)] = v
    for k in range(n_inst):
        label = int(rng.choice(INSTANCE_LABELS))
        m = _blob(rng, H, W, 2, ext) if rng.random() < 0.8 else _blob(rng, H, W, 1, 4)
        ids[m] = label * 1000 + k                           # (k = 0: raw value exactly 1000 * label)
    labels = labels_of(ids)
    # the prediction: the ground truth shifted by a few pixels, ignored labels replaced, train never right on its own pixels
    dy, dx = int(rng.integers(-3, 4)), int(rng.integers(-3, 4))
    pred = np.roll(np.roll(labels, dy, 0), dx, 1).copy()
    evaluated = np.isin(pred, TRAIN2LABEL)
    pred[~evaluated] = TRAIN2LABEL[rng.integers(0, 19, int((~evaluated).sum()))] if noise else 7
    for _ in range(max(3, n_inst // 2)):                    # blobs of other labels: person <-> rider, car <-> truck, stuff on things
        m = _blob(rng, H, W, 2, ext)
        pred[m] = int(rng.choice([24, 25, 26, 27, 28, 33, 7, 8, 11, 21, 23, 20]))
    pred[pred == 32] = 33
    pred[(pred == 31) & (labels == 31)] = 28
    if not train_ids:                                       # a submission of label ids: ignored labels are predicted too
        for v in (0, 9, 29, 18):
            pred[_blob(rng, H, W, 2, ext)] = v
        return labels, ids, pred.astype(np.uint8)
    to_train = np.full(34, 255, np.uint8)
    to_train[TRAIN2LABEL] = np.arange(19)
    return labels, ids, to_train[pred]


def make_scene(seed, sizes, n_inst=12):
    """[(gt_labels, gt_ids, pred, train_ids)]: train-id and label-id predictions alternate."""
    rng = np.random.default_rng(seed)
    return [make_image(rng, H, W, n_inst, train_ids=k % 2 == 0) + (k % 2 == 0,) for k, (H, W) in enumerate(sizes)]


def as_label_ids(pred, train_ids):
    """The prediction as the restatement takes it (label ids)."""
    return TRAIN2LABEL[pred].astype(np.uint8) if train_ids else pred


def no_instance_image(seed=11, H=96, W=160):
    """Stuff and group regions only: no raw value above 1000."""
    rng = np.random.default_rng(seed)
    labels, ids, pred = make_image(rng, H, W, 0, train_ids=True)
    ids[ids > 1000] = 26
    return labels_of(ids), ids, pred, True


def many_instances_image(n=999, label=24, H=64, W=512, seed=13):
    """n instances of one class, cells of 4 rows x 8 columns numbered from 1 in row-major order (256 distinct instances in every 16
    rows: more in one stretch of pixels than a small on-chip table holds), plus instance number 0 in the last row; the prediction
    misses every fourth column and a twentieth of the rest."""
    rng = np.random.default_rng(seed)
    ids = np.full((H, W), 7, np.uint16)
    per_row = W // 8
    for k in range(1, n + 1):
        r, c = divmod(k - 1, per_row)
        ids[4 * r:4 * r + 4, 8 * c:8 * c + 8] = label * 1000 + k
    ids[H - 1, :16] = label * 1000
    labels = labels_of(ids)
    pred = labels.copy()
    pred[:, ::4] = 25 if label == 24 else 24
    pred[rng.random((H, W)) < 0.05] = 7
    return labels, ids, pred, False


def all_labels_image(H=68, W=70):
    """Every label id 0..33 in the ground truth (two rows each) and every one in the prediction (two columns each, plus a rest)."""
    labels = np.repeat(np.arange(34, dtype=np.uint8), 2)[:, None].repeat(W, 1)
    ids = labels.astype(np.uint16)
    for l in (24, 25, 26, 27, 28, 29, 30, 31, 32, 33):
        ids[2 * l, : W // 2] = l * 1000 + 7
    pred = np.repeat(np.arange(34, dtype=np.uint8), 2)[None, :].repeat(H, 0)
    pred = np.concatenate([pred, np.full((H, W - 68), 7, np.uint8)], 1)
    return labels, ids, pred, False
