"""Structured inputs for the panoptic head tests (plain numpy, seeded): the regimes the random draws of tests/test_ops_gpu.py never
reach -- crowds (more kept same-class predecessors under one box than the removal kernel's candidate list holds), dependency chains
(one removal round per box), overlap ratios of exactly 3/10, up to 1024 instances, score ties, mask sides other than 28, boxes on
the 64-pixel word edges of the removal bitmaps, widths that are no multiple of 4, 256 kept instances, exact argmax ties.

Every builder returns ((fcn, rois5, prob, logit, cls, S, C, H, W), tag):
  fcn [1,S,H,W] f32, rois5 [m,5] f32 (column 0 is the batch index), prob [m] f32, logit [m,1,ms,ms] f32, cls [m] int64 (1-based thing
  class), S semantic channels, C = thing classes + 1. `up_tiny` returns the low-resolution score [1,S,Hs,Ws] in the place of fcn.
tests/test_panoptic_cases_cpu.py asserts, with the oracle, that each case is in the regime it is named for.
"""
import numpy as np

F32 = np.float32
MS = 28
DEVICE_COUNT = 37      # valid rows of the `device_count` case (capacity 64)


def _fcn(rng, S, H, W):
    return rng.normal(0, 3, size=(1, S, H, W)).astype(F32)


def _rand_rois(rng, n, H, W, smin=8, smax=None):
    """Log-uniform sizes and aspect ratios, uniform centres, clipped to the image: the population of conftest.gen_rois."""
    smax = min(H, W) if smax is None else smax
    smin = min(smin, smax / 2)
    size = np.exp(rng.uniform(np.log(smin), np.log(smax), n))
    ar = np.exp(rng.uniform(np.log(0.5), np.log(2.0), n))
    w, h = size * np.sqrt(ar), size / np.sqrt(ar)
    cx, cy = rng.uniform(0, W, n), rng.uniform(0, H, n)
    b = np.stack([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2], 1)
    b[:, 0::2] = np.clip(b[:, 0::2], 0, W - 1)
    b[:, 1::2] = np.clip(b[:, 1::2], 0, H - 1)
    return b.astype(F32)


def _random(rng, m, C, H, W, ms=MS):
    """(rois4, prob, logit, cls) in the style of test_ops_gpu._pan_inputs."""
    rois = _rand_rois(rng, m, H, W)
    rois += rng.uniform(-0.9, 0.9, size=(m, 4)).astype(F32)
    rois = np.maximum(rois, 0).astype(F32)
    prob = rng.uniform(0.6, 1.0, size=m).astype(F32)
    logit = rng.normal(0.3, 2, size=(m, 1, ms, ms)).astype(F32)
    cls = rng.integers(1, C, size=m).astype(np.int64)
    return rois, prob, logit, cls


def _pack(rng, rois4, prob, logit, cls, C, H, W, S=None, fcn=None):
    rois4 = np.asarray(rois4, F32).reshape(-1, 4)
    m = rois4.shape[0]
    S = C + 3 if S is None else S
    rois5 = np.hstack([np.zeros((m, 1), F32), rois4]).astype(F32)
    fcn = _fcn(rng, S, H, W) if fcn is None else fcn
    return (fcn, rois5, np.asarray(prob, F32).reshape(m), np.asarray(logit, F32), np.asarray(cls, np.int64).reshape(m), S, C, H, W)


def _const_logit(m, value=2.0, ms=MS):
    return np.full((m, 1, ms, ms), value, F32)


def _scores_desc(m, hi=0.99, lo=0.5):
    """Strictly decreasing, distinct fp32 scores: score order == index order."""
    return np.linspace(hi, lo, m).astype(F32)


# ------------------------------------------------------------------------------------------------------------------ mask removal
CROWD_GRID = (10, 9)         # rows x columns of small boxes, pitch 12 x 28 on 128 x 256


def crowd(kind, seed=11):
    """90 small disjoint all-positive boxes of class 1 on a grid, all kept, and one box over the whole image (index `crowd_wide(kind)`).
    dropped: 10 x 20 small boxes cover 55 % of the wide mask, which comes last in score order.
    kept:    6 x 8 small boxes cover 13 % of it.
    middle:  6 x 8 small boxes; the wide box is 73rd in score order, its mask is positive in the lower part of the image only and
             is kept, so the 18 small boxes after it have it as a predecessor (those under its positive part are dropped).
    Five random instances of class 2 share the image."""
    assert kind in ('dropped', 'kept', 'middle')
    rng = np.random.default_rng(seed)
    H, W, C = 128, 256, 3
    bh, bw = (10, 20) if kind == 'dropped' else (6, 8)
    small = []
    for r in range(CROWD_GRID[0]):
        for c in range(CROWD_GRID[1]):
            y0, x0 = 2 + 12 * r, 3 + 28 * c
            small.append([x0, y0, x0 + bw - 1, y0 + bh - 1])
    small = np.asarray(small, F32)
    small = small[rng.permutation(len(small))]          # score order is not raster order
    wide = np.asarray([[0, 0, W - 1, H - 1]], F32)
    n_before = 72 if kind == 'middle' else len(small)
    rois = np.concatenate([small[:n_before], wide, small[n_before:]], 0)
    n1 = len(rois)
    logit = _const_logit(n1)
    if kind == 'middle':
        logit[n_before, 0, :12, :] = -2.0
    r2, p2, l2, _ = _random(rng, 5, 2, H, W)
    prob = np.concatenate([_scores_desc(n1), p2])
    cls = np.concatenate([np.ones(n1, np.int64), np.full(5, 2, np.int64)])
    return _pack(rng, np.concatenate([rois, r2], 0), prob, np.concatenate([logit, l2], 0), cls, C, H, W), 'crowd_' + kind


def crowd_wide(kind):
    """Index of the image-wide box in crowd(kind)."""
    return 72 if kind == 'middle' else CROWD_GRID[0] * CROWD_GRID[1]


THRESHOLD_N = 5
THRESHOLD_PAIRS = {'exact': (5, 3), 'plus': (4, 4), 'minus': (7, 2)}   # (columns, rows) of the second box that the first one covers


def threshold_exact(variant):
    """Two all-positive instances of class 1. The second box is 10 x 5 pixels (sum = 10 n, n = 5); the first, higher-scored one covers
    a corner of it: 5 x 3 = 3 n pixels (ratio exactly 3/10: kept, the rule is '>'), 4 x 4 = 3 n + 1 (dropped), 7 x 2 = 3 n - 1 (kept)."""
    cw, ch = THRESHOLD_PAIRS[variant]
    rng = np.random.default_rng(5)
    H, W, C = 32, 48, 2
    x0, y0 = 20, 10
    second = [x0, y0, x0 + 9, y0 + 4]
    first = [x0 - 12, y0 - 6, x0 + cw - 1, y0 + ch - 1]
    rois = np.asarray([first, second], F32) + F32(0.25)            # (fractional parts are truncated)
    return _pack(rng, rois, [0.9, 0.8], _const_logit(2), [1, 1], C, H, W), 'threshold_' + variant


def chain(kind, reverse=False):
    """A row of same-class all-positive boxes, each meeting only its left neighbour, in score order left to right: one removal round
    per box. alternating: 10 wide, step 6 -- 40 % of a box lies under a kept left neighbour, so every second one is dropped.
    all_kept: 6 wide, step 5 -- 1/6 of a box lies under its neighbour. reverse: the index order runs right to left."""
    assert kind in ('alternating', 'all_kept')
    rng = np.random.default_rng(3)
    H, W, C = 24, 256, 3
    bw, step, n = (10, 6, 41) if kind == 'alternating' else (6, 5, 48)
    rois = np.asarray([[2 + step * i, 5 + (i % 3), 2 + step * i + bw - 1, 16 + (i % 3)] for i in range(n)], F32)
    prob = _scores_desc(n)
    if reverse:
        rois, prob = rois[::-1].copy(), prob[::-1].copy()
    r2, p2, l2, _ = _random(rng, 4, 2, H, W)
    cls = np.concatenate([np.ones(n, np.int64), np.full(4, 2, np.int64)])
    tag = 'chain_%s%s' % (kind, '_reversed' if reverse else '')
    return _pack(rng, np.concatenate([rois, r2], 0), np.concatenate([prob, p2]), np.concatenate([_const_logit(n), l2], 0), cls, C, H, W), tag


def many(m, one_class=False, seed=None):
    """Random boxes and logits, 8 thing classes (or all of class 1), 64 x 96."""
    rng = np.random.default_rng(m + int(one_class) if seed is None else seed)
    H, W, C = 64, 96, 9
    rois, prob, logit, cls = _random(rng, m, C, H, W)
    if one_class:
        cls[:] = 1
    return _pack(rng, rois, prob, logit, cls, C, H, W, S=19), 'many_%d%s' % (m, '_one_class' if one_class else '')


def ties_all_equal(m):
    rng = np.random.default_rng(100 + m)
    H, W, C = 64, 96, 9
    rois, prob, logit, cls = _random(rng, m, C, H, W)
    prob[:] = F32(0.75)
    return _pack(rng, rois, prob, logit, cls, C, H, W, S=19), 'ties_all_equal_%d' % m


def ties_blocks(m):
    rng = np.random.default_rng(200 + m)
    H, W, C = 64, 96, 9
    rois, prob, logit, cls = _random(rng, m, C, H, W)
    prob = np.asarray([0.95, 0.9, 0.75, 0.7, 0.6], F32)[np.arange(m) % 5][rng.permutation(m)]
    return _pack(rng, rois, prob, logit, cls, C, H, W, S=19), 'ties_blocks_%d' % m


def mask_side(ms):
    rng = np.random.default_rng(300 + ms)
    H, W, C = 64, 96, 9
    rois, prob, logit, cls = _random(rng, 30, C, H, W, ms=ms)
    return _pack(rng, rois, prob, logit, cls, C, H, W, S=19), 'mask_side_%d' % ms


def word_edges(W):
    """Boxes on the 64-column word edges of the removal bitmaps and on every image border, H = 37 (W in 65, 127, 130). Two classes by
    turns, random mixed-sign logits, score order == index order except one tie."""
    assert W >= 65
    rng = np.random.default_rng(W)
    H, C = 37, 3
    e = W - 1
    boxes = [
        (63, 4, 63, 20), (64, 6, 64, 22), (0, 3, 63, 12), (63, 8, 128, 30),           # columns [63,64) [64,65) [0,64) [63,129)
        (60, 2, 66, 9), (0, 0, e, 5), (e - 9, 10, e, 30), (e, 0, e, H - 1),             # ... across the edge, ending at W - 1
        (-5.7, 4.5, 10.2, 15.5), (e - 6.5, 20.25, W + 12.75, 33.5),                     # partly outside: left, right
        (20.5, -7.9, 40.5, 6.1), (30.25, 30.5, 50.75, H + 8.5),                         # ... top, bottom
        (-0.9, -0.9, 7.9, 7.9), (-0.5, 12.0, 63.9, 12.9),                               # (-0.9 truncates to 0, not to -1)
        (-20.5, 5.0, -3.2, 15.0), (W + 3.0, 5.0, W + 20.0, 15.0),                       # wholly outside: left, right
        (5.0, -30.5, 25.0, -2.5), (5.0, H + 1.0, 25.0, H + 9.0),                        # ... above, below
        (-40.0, -40.0, W + 40.0, H + 40.0),                                             # the image lies inside the box
        (40.0, 10.0, 30.0, 20.0), (50.0, 25.0, 60.0, 15.0), (33.0, 14.0, 32.0, 13.0),   # x2 < x1, y2 < y1, both by one
        (10.2, 10.3, 10.7, 10.9), (63.1, 0.2, 63.9, 0.8), (e + 0.1, H - 0.9, e + 0.9, H - 0.1),   # sub-pixel
        (58, 14, 70, 28), (56, 12, 72, 30), (54, 10, 74, 32),                           # live / mask_sum == 0 / live, overlapping
        (0, H - 1, e, H - 1), (62, 0, 65, H - 1),
    ]
    m = len(boxes)
    rois = np.asarray(boxes, F32)
    logit = rng.normal(0.3, 2, size=(m, 1, MS, MS)).astype(F32)
    dead = m - 4
    logit[dead - 1] = np.abs(logit[dead - 1]) + F32(0.5)
    logit[dead] = -np.abs(logit[dead]) - F32(0.5)
    logit[dead + 1] = np.abs(logit[dead + 1]) + F32(0.5)
    cls = (1 + np.arange(m) % 2).astype(np.int64)
    cls[dead - 1:dead + 2] = 1
    prob = _scores_desc(m)
    prob[7] = prob[3]
    return _pack(rng, rois, prob, logit, cls, C, H, W), 'word_edges_%d' % W


def word_edges_dead(W):
    """Index of the all-negative instance of word_edges(W); its neighbours in the score order are the two live ones around it."""
    return word_edges(W)[0][1].shape[0] - 4


def device_count():
    """Capacity 64, DEVICE_COUNT valid rows; the rows after the count hold arbitrary finite values (huge boxes and scores, class
    numbers that are no class)."""
    rng = np.random.default_rng(64)
    H, W, C = 64, 96, 9
    rois, prob, logit, cls = _random(rng, 64, C, H, W)
    n = DEVICE_COUNT
    rois[n:] = rng.uniform(-1e6, 1e6, size=(64 - n, 4)).astype(F32)
    prob[n:] = rng.uniform(1.0, 1e6, size=64 - n).astype(F32)
    logit[n:] = F32(1e6)
    cls[n:] = 999
    return _pack(rng, rois, prob, logit, cls, C, H, W, S=19), 'device_count'


# ------------------------------------------------------------------------------------------------------------------ fuse / argmax
ODD_WIDTHS = {65: 33, 67: 17, 101: 31, 130: 20, 258: 128}   # W -> H; W % 4 = 1, 3, 1, 2, 2; 258 leaves a ragged second 256-pixel tile


def odd_width(W):
    rng = np.random.default_rng(1000 + W)
    H, C = ODD_WIDTHS[W], 9
    rois, prob, logit, cls = _random(rng, 24, C, H, W)
    rois[0] = [W - 3.5, 0, W - 1, H - 1]               # (a box on the last columns)
    return _pack(rng, rois, prob, logit, cls, C, H, W, S=19), 'odd_width_%d' % W


def misaligned():
    rng = np.random.default_rng(77)
    H, W, C = 40, 96, 9
    return _pack(rng, *_random(rng, 20, C, H, W), C, H, W, S=19), 'misaligned'


def kept_256():
    """256 disjoint 4 x 3 all-positive boxes on a 16 x 16 grid, classes by turns: every one is kept."""
    rng = np.random.default_rng(256)
    H, W, C = 64, 96, 9
    rois = np.asarray([[6 * c + 1, 4 * r, 6 * c + 4, 4 * r + 2] for r in range(16) for c in range(16)], F32)
    rois = rois[rng.permutation(256)]
    cls = (1 + np.arange(256) % (C - 1)).astype(np.int64)
    prob = rng.uniform(0.5, 1.0, 256).astype(F32)
    return _pack(rng, rois, prob, _const_logit(256), cls, C, H, W, S=19), 'kept_256'


def exact_ties():
    """Argmax ties (48 x 80, 3 stuff + 2 thing channels, 4 kept instances, all-positive constant masks):
      rows 0..7              stuff channels 0, 1 and 2 hold the same value, above everything else (first maximum: channel 0);
                             in columns 40.. only channels 1 and 2 tie;
      rows 40..47            every logit negative and no instance box: all four instance planes are exactly 0 (first one wins);
      box of instance 2      28 x 28 with a 28 x 28 mask of 2.0 (resampled exactly) over thing logit 1.0 and best stuff logit 3.0."""
    rng = np.random.default_rng(9)
    H, W, C, S = 48, 80, 3, 5
    fcn = rng.normal(0, 1, size=(1, S, H, W)).astype(F32)
    fcn[0, :3, 0:8, :] = F32(6.5)
    fcn[0, 0, 0:8, 40:] = F32(6.0)
    fcn[0, :, 40:48, :] = -np.abs(fcn[0, :, 40:48, :]) - F32(0.25)
    rois = np.asarray([[2, 10, 20, 30], [50, 2, 75, 20], [22, 10, 49, 37], [60, 24, 78, 38]], F32)
    cls = np.asarray([1, 2, 1, 2], np.int64)
    y0, y1, x0, x1 = 10, 38, 22, 50
    fcn[0, :3, y0:y1, x0:x1] = rng.uniform(-2, 2, size=(3, y1 - y0, x1 - x0)).astype(F32)
    fcn[0, 1, y0:y1, x0:x1] = F32(3.0)
    fcn[0, 3, y0:y1, x0:x1] = F32(1.0)                 # (the channel of thing class 1)
    fcn[0, 4, y0:y1, x0:x1] = F32(-1.0)
    prob = np.asarray([0.9, 0.8, 0.7, 0.6], F32)
    return _pack(rng, rois, prob, _const_logit(4), cls, C, H, W, S=S, fcn=fcn), 'exact_ties'


UP_TINY = [(1, 1, 19), (2, 3, 160), (3, 70, 19)]       # (Hs, Ws, S)


def up_tiny(Hs, Ws, S):
    """Inputs of panoptic_fuse_up on a tiny score map; the first element is the low-resolution score [1,S,Hs,Ws]."""
    rng = np.random.default_rng(Hs * 100 + Ws)
    H, W, C = Hs * 4, Ws * 4, 9
    rois, prob, logit, cls = _random(rng, 6, C, H, W)
    score = rng.normal(0, 3, size=(1, S, Hs, Ws)).astype(F32)
    return _pack(rng, rois, prob, logit, cls, C, H, W, S=S, fcn=score), 'up_tiny_%dx%d_S%d' % (Hs, Ws, S)


def _cases(*specs):
    return [(fn, args) for fn, *args in specs]


# (builder, arguments): every mask-removal case, and the subset (m <= 256) that also goes through the fuse / argmax paths
REMOVAL_CASES = _cases(
    (crowd, 'dropped'), (crowd, 'kept'), (crowd, 'middle'),
    (threshold_exact, 'exact'), (threshold_exact, 'plus'), (threshold_exact, 'minus'),
    (chain, 'alternating'), (chain, 'all_kept'), (chain, 'alternating', True), (chain, 'all_kept', True),
    (many, 300), (many, 1024), (many, 1024, True),
    (ties_all_equal, 70), (ties_all_equal, 300), (ties_blocks, 150), (ties_blocks, 400),
    (mask_side, 2), (mask_side, 14), (mask_side, 32),
    (word_edges, 65), (word_edges, 127), (word_edges, 130),
    (odd_width, 65), (odd_width, 67), (odd_width, 101), (odd_width, 130), (odd_width, 258), (misaligned,), (kept_256,), (exact_ties,))
FUSE_CASES = _cases(
    (odd_width, 65), (odd_width, 67), (odd_width, 101), (odd_width, 130), (odd_width, 258), (misaligned,), (kept_256,), (exact_ties,),
    (crowd, 'dropped'), (crowd, 'middle'), (chain, 'alternating'), (chain, 'all_kept', True), (ties_all_equal, 70),
    (mask_side, 2), (mask_side, 14), (mask_side, 32), (word_edges, 65), (word_edges, 127), (word_edges, 130))


def case_id(spec):
    fn, args = spec
    return '-'.join([fn.__name__] + [str(a) for a in args])
