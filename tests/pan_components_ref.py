"""The connected-component rule of include/upsnet_hip.h (upsnet_pan_components), restated twice for the tests, and the table of cases
the CPU and GPU tests share.

The rule, from the header and not from the kernel:
  - a pixel's key is c << 8 | i (bytes 0 and 1 of the 2-channel map); byte 2 is never read and always preserved;
  - a pixel with c == 255 (VOID) belongs to no component and is never changed;
  - a component is a maximal set of pixels of equal key that is connected under 4- or 8-connectivity;
  - its label is the smallest linear index y * W + x among its pixels (VOID: -1); its area is its pixel count;
  - the main component of a key is the one of largest area, ties to the smaller label;
  - a component is removed iff area < min_area and, with keep_largest, it is not the main component of its key;
  - a removed pixel becomes (255, 0, byte 2); every other pixel keeps its bytes; min_area == 0 removes nothing;
  - labels are those of the input map; stats = [distinct keys, components, components removed, pixels removed].

clean_flood: a flood fill over the horizontal runs of the map (a run = maximal stretch of one key in one row; two runs of one key in
neighbouring rows touch when their column ranges overlap, widened by one column for 8-connectivity), in plain numpy and Python.
clean_scipy: scipy.ndimage.label once per key, labels canonicalised with ndimage.minimum of the linear index.
Both return (out uint8 [H,W,3], labels int32 [H,W], stats int32 [4]).
"""
import numpy as np

VOID = 255
TH, TW = 32, 128          # the tile of csrc/pan_components.hip (PC_TH, PC_TW): the shapes below straddle it


def keys_of(pan):
    return pan[..., 0].astype(np.int64) << 8 | pan[..., 1].astype(np.int64)


def _label_flood(pan, connectivity):
    H, W = pan.shape[:2]
    key = keys_of(pan)
    valid = pan[..., 0] != VOID
    start = np.ones((H, W), bool)
    start[:, 1:] = key[:, 1:] != key[:, :-1]
    run = np.cumsum(start.reshape(-1)).reshape(H, W) - 1            # run number of every pixel, row-major
    first = np.flatnonzero(start.reshape(-1))                        # linear index of every run's first pixel
    edges = []
    for dx in ((0,) if connectivity == 4 else (-1, 0, 1)):           # pixel (y, x) against (y - 1, x + dx)
        lo, hi = max(0, -dx), W - max(0, dx)
        a, b = slice(lo, hi), slice(lo + dx, hi + dx)
        same = (key[1:, a] == key[:-1, b]) & valid[1:, a]
        edges.append(np.stack([run[1:, a][same], run[:-1, b][same]], 1))
    edges = np.unique(np.concatenate(edges), axis=0) if H > 1 else np.zeros((0, 2), np.int64)
    neighbours = [[] for _ in range(len(first))]
    for u, v in edges.tolist():
        neighbours[u].append(v)
        neighbours[v].append(u)
    run_valid = valid.reshape(-1)[first]
    label_of_run = np.full(len(first), -1, np.int64)
    for r in range(len(first)):                                      # runs ascend with their first pixel: a fill starts at its minimum
        if not run_valid[r] or label_of_run[r] >= 0:
            continue
        label_of_run[r] = first[r]
        stack = [r]
        while stack:
            for v in neighbours[stack.pop()]:
                if label_of_run[v] < 0:
                    label_of_run[v] = first[r]
                    stack.append(v)
    return label_of_run[run].astype(np.int32)


def clean_flood(pan, min_area=0, connectivity=8, keep_largest=True):
    assert connectivity in (4, 8) and min_area >= 0
    H, W = pan.shape[:2]
    labels = _label_flood(pan, connectivity)
    key = keys_of(pan).reshape(-1)
    flat = labels.reshape(-1)
    roots, areas = np.unique(flat[flat >= 0], return_counts=True)
    removed = areas < min_area
    if keep_largest:
        main = {}
        for k, (r, a) in enumerate(zip(roots.tolist(), areas.tolist())):     # ascending label: a later one must be strictly larger
            if key[r] not in main or a > areas[main[key[r]]]:
                main[key[r]] = k
        removed[np.array(list(main.values()), np.int64)] = False
    gone = np.zeros(H * W, bool)
    gone[flat >= 0] = removed[np.searchsorted(roots, flat[flat >= 0])]
    out = pan.copy().reshape(-1, 3)
    out[gone, 0] = VOID
    out[gone, 1] = 0
    stats = np.array([len(set(key[roots].tolist())), len(roots), int(removed.sum()), int(gone.sum())], np.int32)
    return out.reshape(H, W, 3), labels, stats


def clean_scipy(pan, min_area=0, connectivity=8, keep_largest=True):
    from scipy import ndimage
    assert connectivity in (4, 8) and min_area >= 0
    H, W = pan.shape[:2]
    structure = np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]]) if connectivity == 4 else np.ones((3, 3), int)
    key = keys_of(pan)
    lin = np.arange(H * W, dtype=np.int64).reshape(H, W)
    labels = np.full((H, W), -1, np.int32)
    out = pan.copy()
    stats = np.zeros(4, np.int32)
    for k in np.unique(key[pan[..., 0] != VOID]).tolist():
        lab, n = ndimage.label(key == k, structure=structure)
        index = np.arange(1, n + 1)
        mins = np.asarray(ndimage.minimum(lin, lab, index)).astype(np.int64).reshape(-1)
        areas = np.bincount(lab.reshape(-1), minlength=n + 1)[1:]
        inside = lab > 0
        labels[inside] = mins[lab[inside] - 1]
        removed = areas < min_area
        if keep_largest:
            removed[np.lexsort((mins, -areas))[0]] = False
        gone = np.zeros((H, W), bool)
        gone[inside] = removed[lab[inside] - 1]
        out[gone, 0] = VOID
        out[gone, 1] = 0
        stats += np.array([1, n, int(removed.sum()), int(gone.sum())], np.int32)
    return out, labels, stats


# ---------------------------------------------------------------------------------------------------------------- the case table
def _blank(H, W, c=VOID, i=0):
    pan = np.zeros((H, W, 3), np.uint8)
    pan[..., 0], pan[..., 1] = c, i
    return pan


def _random(rng, H, W, keys, byte2=True):
    pick = rng.integers(0, len(keys), (H, W))
    pan = np.zeros((H, W, 3), np.uint8)
    pan[..., 0] = np.array([k[0] for k in keys], np.uint8)[pick]
    pan[..., 1] = np.array([k[1] for k in keys], np.uint8)[pick]
    if byte2:
        pan[..., 2] = rng.integers(0, 256, (H, W))
    return pan


def blobs(rng, H, W, cell, keys, speck=0.002):
    """Blocks of cell x cell pixels of random keys, shifted so that they straddle the tiles, with single pixels of random keys
    sprinkled over them."""
    gh, gw = H // cell + 2, W // cell + 2
    grid = rng.integers(0, len(keys), (gh, gw))
    pick = np.repeat(np.repeat(grid, cell, 0), cell, 1)[cell // 3:cell // 3 + H, cell // 2:cell // 2 + W]
    noise = rng.random((H, W)) < speck
    pick = np.where(noise, rng.integers(0, len(keys), (H, W)), pick)
    pan = np.zeros((H, W, 3), np.uint8)
    pan[..., 0] = np.array([k[0] for k in keys], np.uint8)[pick]
    pan[..., 1] = np.array([k[1] for k in keys], np.uint8)[pick]
    return pan


KEYS = [(0, 0), (3, 0), (11, 1), (11, 2), (13, 1), (VOID, 0), (VOID, 7)]


def serpentine(H, W):
    """One pixel wide: every even row in full, joined to the next even row at alternating ends; stuff (3, 0) between."""
    pan = _blank(H, W, 3, 0)
    pan[0::2] = (11, 1, 0)
    for k, y in enumerate(range(1, H - 1, 2)):
        pan[y, W - 1 if k % 2 == 0 else 0] = (11, 1, 0)
    return pan


def u_shape():
    """Two arms in the first tile that meet only in the tile to its right."""
    pan = _blank(40, 200)
    pan[5, 100:TW + 4] = pan[9, 100:TW + 4] = (11, 1, 0)
    pan[5:10, TW + 3] = (11, 1, 0)
    return pan


def comb(seam=TH, width=150):
    """A spine 8 rows below the seam at row `seam`, teeth in every other column over rows seam - 7 .. seam + 7: every tooth crosses
    the seam and the teeth meet only in the spine. comb(TW, 70) transposed puts the teeth across the vertical seam at column TW."""
    pan = _blank(seam + 16, width, 3, 0)
    pan[seam + 8] = (11, 1, 0)
    pan[seam - 7:seam + 8, 0::2] = (11, 1, 0)
    return pan


def corner():
    """Two pixels of one key that touch only diagonally where four tiles meet, and two of another key on the other diagonal."""
    pan = _blank(2 * TH, 2 * TW)
    pan[TH - 1, TW - 1] = pan[TH, TW] = (11, 1, 0)
    pan[TH - 1, TW] = pan[TH, TW - 1] = (12, 1, 0)
    return pan


def thresholds(min_area):
    """A body and fragments of min_area - 1, min_area and min_area + 1 pixels of the same key, one of them across a seam."""
    pan = _blank(40, 140, 3, 0)
    pan[2:12, 2:20] = (11, 1, 0)
    for k, a in enumerate((min_area - 1, min_area, min_area + 1)):
        pan[20 + 6 * k, 124:124 + a] = (11, 1, 0)
    return pan


def tie():
    """Two components of one key and equal area, one of them spread over two tiles; a third, smaller one."""
    pan = _blank(36, 20)
    pan[30:34, 10:13] = (11, 1, 0)          # 12 pixels, rows 30..33 (across the seam at row 32)
    pan[3:5, 2:8] = (11, 1, 0)              # 12 pixels, the smaller label
    pan[10, 10:15] = (11, 1, 0)             # 5 pixels
    return pan


def many_instances(rng):
    """255 instances of one category in 4 x 4 cells, stuff with instance 0 around them, a few stray pixels."""
    pan = _blank(66, 70, 2, 0)
    cell = np.arange(256).reshape(16, 16)
    inst = np.repeat(np.repeat(cell, 4, 0), 4, 1) + 1
    body = pan[1:65, 3:67]
    body[..., 0] = np.where(inst <= 255, 11, 5)
    body[..., 1] = np.where(inst <= 255, inst, 0)
    ys, xs = rng.integers(0, 66, 40), rng.integers(0, 70, 40)
    pan[ys, xs, 0] = 11
    pan[ys, xs, 1] = rng.integers(1, 256, 40)
    return pan


def checkerboard(H, W):
    pan = _blank(H, W, 3, 0)
    y, x = np.mgrid[:H, :W]
    pan[(y + x) % 2 == 1] = (11, 1, 0)
    return pan


def cases(full_size=True):
    """[(name, map, min_area, keep_largest)]; every test runs each of them under both connectivities."""
    rng = np.random.default_rng(2601)
    void = _blank(37, 53)
    void[..., 1] = rng.integers(0, 256, (37, 53))
    void[..., 2] = rng.integers(0, 256, (37, 53))
    out = [
        ('1x1', _blank(1, 1, 3, 0), 2, True),
        ('1x1_void', _blank(1, 1), 2, False),
        ('1x1_gone', _blank(1, 1, 3, 0), 2, False),
        ('1xW', _random(rng, 1, 300, KEYS), 2, True),
        ('Hx1', _random(rng, 100, 1, KEYS), 2, True),
        ('one_tile', blobs(rng, TH, TW, 9, KEYS, 0.02), 4, True),
        ('one_tile_plus_one', blobs(rng, TH + 1, TW + 1, 9, KEYS, 0.02), 4, True),
        ('odd_37x53', blobs(rng, 37, 53, 7, KEYS, 0.02), 3, True),
        ('tiles_2x3_plus', blobs(rng, 2 * TH + 1, 3 * TW + 5, 21, KEYS, 0.01), 6, True),
        ('all_void', void, 5, True),
        ('one_key', _blank(2 * TH + 1, 3 * TW + 5, 11, 4), 10, True),
        ('one_key_labels_only', _blank(2 * TH + 1, 3 * TW + 5, 11, 4), 0, True),
        ('checkerboard', checkerboard(2 * TH + 1, 3 * TW + 5), 2, True),
        ('checkerboard_all_go', checkerboard(2 * TH + 1, 2 * TW + 5), 2, False),
        ('serpentine', serpentine(3 * TH + 1, 3 * TW + 5), 50, True),
        ('u_shape', u_shape(), 40, False),
        ('comb', comb(), 30, True),
        ('comb_transposed', np.ascontiguousarray(comb(TW, 70).transpose(1, 0, 2)), 30, True),
        ('corner', corner(), 2, False),
        ('thresholds', thresholds(5), 5, True),
        ('thresholds_all', thresholds(5), 5, False),
        ('tie', tie(), 13, True),
        ('tie_all', tie(), 13, False),
        ('tie_labels_only', tie(), 0, True),
        ('many_instances', many_instances(rng), 3, True),
        ('random_37x53', _random(rng, 37, 53, KEYS), 3, True),
        ('random_131x257', _random(rng, 131, 257, KEYS), 3, True),
        ('random_131x257_all', _random(rng, 131, 257, KEYS[:4], byte2=False), 2, False),
    ]
    if full_size:
        out.append(('full_1024x2048', blobs(rng, 1024, 2048, 96, KEYS + [(11, k) for k in range(3, 30)], 0.002), 40, True))
    return out
