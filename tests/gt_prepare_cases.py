"""Instance-id maps for the ground-truth preparation tests, shared by the CPU and GPU files. Cityscapes label ids: 7 road, 8 sidewalk,
11 building, 21 vegetation, 23 sky (stuff); 0, 3 (ignored); 24 person, 25 rider, 26 car, 33 bicycle (things); 29 caravan, 30 trailer
(instances of ignored labels); a value below 1000 of a thing label is a group."""
import functools

import numpy as np

# the literal map of tests/test_gt_prepare_cpu.py: road, unlabeled, a car group (26), two cars (26001 with a hole), a caravan
LITERAL = np.array([[7, 7, 26001, 26001, 26001, 0],
                    [7, 26000, 26001, 7, 26001, 0],
                    [26, 26000, 26001, 26001, 26001, 29000],
                    [26, 7, 7, 7, 7, 29000]], np.int32)

THING_LABELS = (24, 25, 26, 27, 28, 31, 32, 33)


def _stripes(H, W):
    ids = np.empty((H, W), np.int32)
    bands = (23, 11, 21, 8, 7)
    for k, lab in enumerate(bands):
        ids[k * H // len(bands):(k + 1) * H // len(bands)] = lab
    return ids


def border_frame():
    """One instance that touches all four borders (first and last pixel included) around another."""
    ids = np.full((20, 30), 26000, np.int32)
    ids[1:-1, 1:-1] = 7
    ids[5:9, 4:11] = 24003
    return ids


def hole_two_components():
    ids = _stripes(24, 40)
    ids[3:12, 5:16] = 26002
    ids[6:9, 8:12] = 11          # the hole
    ids[15:20, 30:38] = 26002    # second component
    ids[14:22, 2:9] = 33000
    return ids


def checkerboard():
    y, x = np.mgrid[0:32, 0:32]
    return np.where((x + y) % 2 == 0, 26000, 26001).astype(np.int32)


def many_instances():
    """64 x 96, 8 thing labels x 160 instance numbers = 1280 segments (more than the 1024 slots of the kernel's LDS table and more
    than a segment capacity of 1024) plus caravans and trailers; every value is present."""
    rng = np.random.default_rng(42)
    values = np.array([lab * 1000 + k for lab in THING_LABELS + (29, 30) for k in range(160)], np.int32)
    flat = values[np.arange(64 * 96) % len(values)]
    rng.shuffle(flat)
    return np.ascontiguousarray(flat.reshape(64, 96))


def ignored_only():
    ids = np.zeros((19, 23), np.int32)
    ids[4:9] = 3
    ids[10:, 5:] = 29000
    ids[0, 0] = 30001
    ids[2:4, 2:9] = 6
    return ids


def groups_and_caravans():
    ids = _stripes(30, 44)
    ids[2:8, 2:12] = 24          # person group
    ids[10:16, 20:30] = 26       # car group
    ids[18:25, 3:14] = 29001     # caravan
    ids[18:25, 30:40] = 30002    # trailer
    ids[12:20, 34:42] = 25000    # the one instance
    return ids


def random_small(H=37, W=53, seed=5):
    rng = np.random.default_rng(seed)
    ids = _stripes(H, W)
    ids[rng.random((H, W)) < 0.05] = 0
    for k in range(9):
        h, w = rng.integers(3, 14, 2)
        y, x = rng.integers(0, H - 2), rng.integers(0, W - 2)
        lab = (24, 26, 33, 29, 26)[k % 5]
        ids[y:y + h, x:x + w] = lab * 1000 + k if k % 4 else lab
    ids[H - 1, W - 3:] = 26007       # ends on the last pixel
    ids[0, 0:2] = 24008              # starts on the first
    return ids


def scene(H=1024, W=2048, seed=7, n_inst=40):
    """Seeded structured scene: stuff bands, void blobs, ellipse-shaped instances of every thing class, groups, caravans."""
    rng = np.random.default_rng(seed)
    ids = _stripes(H, W)
    for k in range(n_inst + 8):
        cy, cx = int(rng.integers(0, H)), int(rng.integers(0, W))
        ry, rx = int(rng.integers(max(2, H // 64), max(4, H // 6))), int(rng.integers(max(2, W // 64), max(4, W // 8)))
        y0, y1, x0, x1 = max(0, cy - ry), min(H, cy + ry + 1), max(0, cx - rx), min(W, cx + rx + 1)
        yy, xx = np.mgrid[y0:y1, x0:x1]
        inside = ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0
        window = ids[y0:y1, x0:x1]
        if k < n_inst:
            window[inside] = (THING_LABELS + (29, 30))[k % 10] * 1000 + k
        elif k < n_inst + 4:
            window[inside] = (24, 26, 0, 3)[k - n_inst]
        else:
            window[inside & ((yy + xx) % 3 == 0)] = 33000 + k       # a sieve: many transitions
    return np.ascontiguousarray(ids.astype(np.int32))


CASES = {
    'literal': lambda: LITERAL.copy(),
    '1x1_instance': lambda: np.array([[26000]], np.int32),
    '1x1_ignored': lambda: np.array([[0]], np.int32),
    '1xW': lambda: np.array([[7] * 5 + [26000] * 9 + [24] * 3 + [26001] * 40 + [0] * 4 + [33005] * 9], np.int32),
    'Hx1': lambda: np.array([[26001] * 30 + [7] * 5 + [26000] * 9 + [29000] * 3 + [0] * 4 + [33005] * 19], np.int32).T.copy(),
    '37x53': random_small,
    'border_frame': border_frame,
    'hole_two_components': hole_two_components,
    'checkerboard': checkerboard,
    'many_instances': many_instances,
    'ignored_only': ignored_only,
    'groups_and_caravans': groups_and_caravans,
    'scene_1024x2048': scene,
}


@functools.lru_cache(maxsize=None)
def case(name):
    """(ids, reference outputs) of a case, computed once per process; do not modify them."""
    from gt_prepare_ref import reference
    from upsnet_amd.dataset.prepare import label_tables
    ids = CASES[name]()
    return ids, reference(ids, label_tables())


def e2e_scene(k, H=64, W=128):
    """Image k of the end-to-end tree: stuff, void, a person group, a car with a hole, further instances of >= 150 pixels, a caravan."""
    ids = _stripes(H, W)
    ids[0:6, 0:20] = 0
    ids[50:64, 100:128] = 3
    ids[8:20, 90 + k:110 + k] = 24
    ids[20:40, 10 + 3 * k:50 + 3 * k] = 26000
    ids[26:32, 20 + 3 * k:30 + 3 * k] = 7
    ids[30:52, 60:80] = 26001
    ids[40:60, 5 + k:20 + k] = 24000 + k
    ids[5:18, 40:70] = 33000
    ids[44:58, 84:98] = 29000
    if k == 1:
        ids[22:36, 100:120] = 28004
    return np.ascontiguousarray(ids)
