"""Numpy restatement of the Boundary IoU API's mask_to_boundary and of its COCOeval's computeIoU for iouType 'boundary', written from
the published sources (the API and cv2 are not dependencies). The restated COCOeval of test_coco_eval_cpu.py is reused, not copied:
`boundary_cocoeval` swaps its mask_iou for `boundary_iou` while it runs."""
import contextlib

import numpy as np

import test_coco_eval_cpu

_MASK_IOU = test_coco_eval_cpu.mask_iou    # the rleIou restatement, taken before anything patches the module


def dilation(h, w, ratio=0.02):
    """int(round(ratio * sqrt(h^2 + w^2))) with Python's round (halves to even), at least 1."""
    d = int(round(ratio * np.sqrt(h ** 2 + w ** 2)))
    return 1 if d < 1 else d


def erode_closed_form(mask, d):
    """eroded[y, x] = 1 iff the (2d+1) x (2d+1) window centred there lies inside the image and is all ones (summed-area table)."""
    m = np.asarray(mask).astype(bool)
    H, W = m.shape
    out = np.zeros((H, W), bool)
    L = 2 * d + 1
    if L > H or L > W:
        return out
    sat = np.zeros((H + 1, W + 1), np.int64)
    sat[1:, 1:] = np.cumsum(np.cumsum(m, 0, dtype=np.int64), 1)
    win = sat[L:, L:] - sat[:-L, L:] - sat[L:, :-L] + sat[:-L, :-L]     # window with top-left (y, x), y <= H - L, x <= W - L
    out[d:H - d, d:W - d] = win == L * L
    return out


def mask_to_boundary(mask, ratio=0.02):
    """mask & ~eroded, the erosion taken on the mask's bounding box grown by d and clipped to the image: a window centred inside the
    bounding box stays inside that crop unless it leaves the image, and nothing outside the bounding box survives anyway."""
    m = np.asarray(mask).astype(bool)
    H, W = m.shape
    d = dilation(H, W, ratio)
    ys, xs = np.nonzero(m.any(1))[0], np.nonzero(m.any(0))[0]
    if len(ys) == 0:
        return m.copy()
    y0, y1, x0, x1 = max(0, ys[0] - d), min(H, ys[-1] + 1 + d), max(0, xs[0] - d), min(W, xs[-1] + 1 + d)
    out = m.copy()
    out[y0:y1, x0:x1] &= ~erode_closed_form(m[y0:y1, x0:x1], d)
    return out


def erode_iterated(mask, d):
    """Step 2 of the rule as the API states it: one ring of zeros, d rounds of a 3x3 erosion whose border outside the padded image does
    not erode, the ring cropped off again."""
    from scipy.ndimage import binary_erosion
    m = np.pad(np.asarray(mask).astype(bool), 1)
    return binary_erosion(m, np.ones((3, 3), bool), iterations=d, border_value=1)[1:-1, 1:-1]


class BoundaryIou(object):
    """computeIoU of iouType 'boundary': min(rleIou of the masks, rleIou of the boundaries). Boundaries are cached by mask identity
    (the masks of a scene are kept alive by the caller)."""

    def __init__(self, ratio=0.02):
        self.ratio = ratio
        self._cache = {}

    def boundary(self, m):
        key = id(m)
        if key not in self._cache:
            self._cache[key] = (m, mask_to_boundary(m, self.ratio))
        return self._cache[key][1]

    def __call__(self, d, g, iscrowd):
        return np.minimum(_MASK_IOU(d, g, iscrowd), _MASK_IOU([self.boundary(m) for m in d], [self.boundary(m) for m in g], iscrowd))


def boundary_iou(d, g, iscrowd, ratio=0.02):
    return BoundaryIou(ratio)(d, g, iscrowd)


@contextlib.contextmanager
def boundary_rule(ratio=0.02):
    """While active, the restated COCOeval's mask_iou is the boundary rule: cocoeval_restated(..., 'segm') then scores 'boundary'."""
    saved = test_coco_eval_cpu.mask_iou
    test_coco_eval_cpu.mask_iou = BoundaryIou(ratio)
    try:
        yield
    finally:
        test_coco_eval_cpu.mask_iou = saved


def boundary_cocoeval(images, cat_ids, ratio=0.02):
    with boundary_rule(ratio):
        return test_coco_eval_cpu.cocoeval_restated(images, cat_ids, 'segm')


# (H, W, ratio) of the kernel tests: one word and two, the first size at which a column takes a second word (65), 127 / 128 / 129
# around the word, d = 74 >= 64 with W < 2d+1 (nothing survives), d = 72 >= 64 with the window inside the image (shifts spanning more
# than one word), and the evaluation size once
SIZES = [(1, 1, .02), (5, 7, .02), (40, 60, .02), (64, 33, .02), (65, 130, .02), (127, 129, .02), (128, 64, .02), (130, 70, .5),
         (96, 160, .02), (300, 200, .2)]
FULL_SIZE = (1024, 2048, .02)


def mask_cases(H, W, d, seed):
    """[(name, bool [H,W])]: empty, all ones, one pixel, a rectangle flush with each of the four edges, a bar thinner than 2d+1 in
    each direction, a rectangle with single-pixel holes, seeded random blobs."""
    rng = np.random.default_rng(seed)
    z = lambda: np.zeros((H, W), bool)
    out = [('empty', z()), ('ones', np.ones((H, W), bool))]
    m = z(); m[H // 2, W // 3] = True
    out.append(('pixel', m))
    hh, ww = max(1, (2 * H) // 3), max(1, (2 * W) // 3)
    for name, (ys, xs) in (('top', (slice(0, hh), slice(W // 5, W // 5 + ww))), ('bottom', (slice(H - hh, H), slice(W // 5, W // 5 + ww))),
                           ('left', (slice(H // 5, H // 5 + hh), slice(0, ww))), ('right', (slice(H // 5, H // 5 + hh), slice(W - ww, W)))):
        m = z(); m[ys, xs] = True
        out.append((name, m))
    t = min(2 * d, max(1, min(H, W) // 3))     # thinner than 2d+1
    m = z(); m[H // 4:H // 4 + t, :] = True
    out.append(('hbar', m))
    m = z(); m[:, W // 4:W // 4 + t] = True
    out.append(('vbar', m))
    m = z(); m[H // 8:H - H // 8, W // 8:W - W // 8] = True
    holes = max(1, (H * W) // 4000)
    m[rng.integers(0, H, holes), rng.integers(0, W, holes)] = False
    out.append(('holes', m))
    for k in range(2):
        m = z()
        for _ in range(6):
            h, w = int(rng.integers(1, H + 1)), int(rng.integers(1, W + 1))
            y, x = int(rng.integers(0, H - h + 1)), int(rng.integers(0, W - w + 1))
            m[y:y + h, x:x + w] ^= rng.random((h, w)) < (0.999 if k else 0.9)
        out.append(('blobs%d' % k, m))
    return out
