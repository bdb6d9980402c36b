"""Structured inputs for the selection path -- proposals (csrc/proposal.hip), NMS (csrc/nms.hip), detection selection
(csrc/detect.hip) -- plain numpy, deterministic: the regimes the random draws of tests/test_ops_gpu.py reach by luck or never.

NMS builders return ((dets [n,5] f32, thresh), tag); `batched_mix` returns ((boxes [P,nmax,4], scores [P,nmax], counts [P] int32,
pre_removed [P,nmax] uint8, thresh), tag).
Proposal builders return ((cls [L] of [1,A,h,w] f32 probabilities, box [L] of [1,4A,h,w] f32, im_info [3] f32, pre, post, nms_thresh,
min_size), tag); strides 4 .. 64, three anchors per cell.
MaskROI builders return ((rois [N,5], deltas [N,4C], prob [N,C], im_info [1,3], C, score_thresh, nms_thresh, max_det), tag).
tests/test_selection_cases_cpu.py asserts, with the oracle and a restatement of the key layout, that each case is in the regime it is
named for.

Key layout of the proposal select (csrc/sort.h, csrc/common.h): key = float_key(score) << 32 | ~anchor_index; the select walks
the digits [64,53) [53,42) [42,31) grid-wide ('digit1' .. 'digit3': the 32 score bits and the top index bit) and [31,20) [20,9) [9,0)
in one workgroup ('tail1' .. 'tail3': the low index bits, reached only when the cut falls inside a run of equal scores). A level is
decided in the first pass whose picked bin holds exactly the keys still needed. With anchor indices below 2^20 the bits [31,20) of
~index are all ones: tail1 never separates two keys, so there is no 'tail1' case.
"""
import numpy as np

F32 = np.float32
STRIDES = (4, 8, 16, 32, 64)
A = 3
PASSES = ('digit1', 'digit2', 'digit3', 'tail1', 'tail2', 'tail3')
PASS_BITS = ((53, 64), (42, 53), (31, 42), (20, 31), (9, 20), (0, 9))      # (shift, hi) of every pass


def _f32_exact(t):
    """The fp32 value of a threshold as a Python float (what the float argument of the entry points becomes)."""
    return float(np.float32(t))


def below(t):
    """The next fp32 value below the fp32 value of t."""
    return float(np.nextafter(np.float32(t), np.float32(0)))


def _scores_desc(n, hi=0.99, lo=0.01):
    s = np.linspace(hi, lo, n).astype(F32)
    assert n < 2 or (np.diff(s) < 0).all()
    return s


def _dets(boxes, scores):
    return np.hstack([np.asarray(boxes, F32).reshape(-1, 4), np.asarray(scores, F32).reshape(-1, 1)]).astype(F32)


# ------------------------------------------------------------------------------------------------------------------------------ NMS
CHAIN_STEP = {0.5: 3, 0.7: 1}     # 10 x 10 boxes: step 3 -> IoU 70/130 with the neighbour, 40/160 with the next; step 1 -> 90/110, 80/120


def chain(n, thresh, reverse=False):
    """n boxes of 10 x 10 pixels in a row, box i overlapping only i-1 and i+1 above the threshold, strictly descending scores: box i
    is suppressed by i-1 iff i-1 is kept, so every second box of the visiting order is kept and the decision on box i depends on
    all i before it. reverse: scores ascending with the index, the visiting order runs against the index order."""
    step = CHAIN_STEP[thresh]
    b = np.asarray([[step * i, 2, step * i + 9, 11] for i in range(n)], F32)
    s = _scores_desc(n)
    if reverse:
        s = s[::-1].copy()
    return (_dets(b, s), _f32_exact(thresh)), 'chain_%d_%g%s' % (n, thresh, '_reversed' if reverse else '')


def chain_by_blocks(n):
    """Disjoint boxes in score order, except that box 64 k overlaps box 64 k - 1 (IoU 70/130 > 0.5): every suppression comes from
    a word of an off-diagonal tile, none from the diagonal tile of a 64-block."""
    b = np.asarray([[20 * i, 2, 20 * i + 9, 11] for i in range(n)], F32)
    for i in range(64, n, 64):
        b[i] = b[i - 1] + F32([3, 0, 3, 0])
    return (_dets(b, _scores_desc(n)), 0.5), 'chain_by_blocks_%d' % n


def all_same(n, equal_scores=False):
    """n identical boxes. Distinct scores (the highest at index n // 3): one box kept. Equal scores: the visiting order is the
    index order reversed (tie rule (i)), the box kept is n - 1."""
    b = np.tile(F32([5, 7, 24, 30]), (n, 1))
    if equal_scores:
        s = np.full(n, 0.75, F32)
    else:
        s = np.roll(_scores_desc(n), n // 3)
    return (_dets(b, s), 0.5), 'all_same_%d%s' % (n, '_equal_scores' if equal_scores else '')


def none_overlap(n):
    """n disjoint 10 x 10 boxes on a grid of pitch 12, 128 per row, scores a fixed permutation of distinct values: all kept."""
    i = np.arange(n)
    x, y = 12 * (i % 128), 12 * (i // 128)
    b = np.stack([x, y, x + 9, y + 9], 1).astype(F32)
    s = _scores_desc(n)[np.random.default_rng(n).permutation(n)]
    return (_dets(b, s), 0.5), 'none_overlap_%d' % n


EXACT_PAIRS = {0.5: ([0, 0, 9, 29], [0, 10, 9, 39]),       # 300 + 300 pixels, 200 shared: 200 / 400
               0.7: ([0, 0, 9, 16], [0, 3, 9, 19])}        # 170 + 170 pixels, 140 shared: 140 / 200
# positions (in score order == index order) of the two boxes of every pair: neighbours inside block 0, the pair on the block edge
# 63 | 64, pairs far apart inside a block and across two blocks, neighbours in block 1; the other positions hold single boxes
EXACT_POSITIONS = [(0, 1), (2, 3), (10, 11), (30, 31), (63, 64), (5, 40), (20, 100), (62, 127), (70, 71), (90, 91), (128, 129)]
EXACT_N = 130


def exact_threshold(thresh, at='exact'):
    """Pairs of integer boxes whose IoU is 1/2 (0.7: 7/10) exactly -- mirrored about the diagonal by turns, translated by multiples
    of 64 pixels so that no two pairs meet. at='exact': the NMS threshold is fp32(thresh): `>` keeps both boxes of every pair (`>=`,
    cpu_nms, drops the second); at='below': the threshold is the next float below: `>` drops the second."""
    pa, pb = EXACT_PAIRS[thresh]
    b = np.zeros((EXACT_N, 4), F32)
    member = {}
    for k, (i, j) in enumerate(EXACT_POSITIONS):
        member[i], member[j] = (k, pa), (k, pb)
    for i in range(EXACT_N):
        if i in member:
            k, box = member[i]
            x1, y1, x2, y2 = box
            if k % 2:
                x1, y1, x2, y2 = y1, x1, y2, x2
            off = F32([64 * (k + 1), 64 * (k % 3)] * 2)
        else:
            x1, y1, x2, y2 = 0, 0, 7, 7
            off = F32([64 * i, 320] * 2)
        b[i] = F32([x1, y1, x2, y2]) + off
    t = _f32_exact(thresh) if at == 'exact' else below(thresh)
    assert at in ('exact', 'below')
    return (_dets(b, _scores_desc(EXACT_N)), t), 'exact_threshold_%g_%s' % (thresh, at)


def degenerate():
    """Zero-width boxes (x2 = x1 - 1), boxes with x2 < x1 - 1 (negative width) and y2 < y1, boxes of one pixel (two of them
    identical, two adjacent), coordinates at +-1e4 (areas of 4e8 pixels are no fp32 integers: the products round). The oracle's IoU
    expression is finite on every pair here. Excluded: two zero-area boxes whose intersection is empty -- the union is 0 and the
    quotient 0/0 (the reference's kernel and the oracle then compare a NaN, which is not a regime of the selection path)."""
    b = F32([
        [50, 50, 49, 70],                  # zero width, inside the big boxes
        [30, 30, 25, 40],                  # negative width
        [80, 90, 70, 85],                  # negative width and height: a positive product
        [10, 10, 10, 10], [10, 10, 10, 10], [11, 10, 11, 10], [10, 11, 10, 11],      # one pixel: twice the same, two neighbours
        [-1e4, -1e4, 1e4, 1e4], [-1e4, -1e4, 9999, 9999], [-9999, -1e4, 1e4, 9998],  # IoU just below 1
        [-1e4, 0, 1e4, 0], [0, -1e4, 0, 1e4],                                         # one pixel high / wide, 20001 long
        [9990, 9990, 1e4, 1e4], [9991, 9991, 1e4, 1e4], [-1e4, -1e4, -9990, -9990],
        [0, 0, 99, 99], [0, 0, 99, 98], [1, 0, 99, 99],
    ])
    s = _scores_desc(len(b))[np.random.default_rng(4).permutation(len(b))]
    return (_dets(b, s), 0.5), 'degenerate'


MIX_NMAX = 1024


def batched_mix():
    """One nms_batched launch of five problems with capacity 1024: a chain of 1000 whose odd boxes are pre-removed (so nothing is
    suppressed and the 500 even ones are kept), 64 identical boxes, an empty problem, a single box, and 1024 disjoint boxes (the
    full capacity); a few pre-removed boxes in the last one too."""
    parts = [chain(1000, 0.5)[0][0], all_same(64)[0][0], np.zeros((0, 5), F32), F32([[3, 4, 20, 30, 0.5]]), none_overlap(MIX_NMAX)[0][0]]
    P = len(parts)
    boxes = np.zeros((P, MIX_NMAX, 4), F32)
    scores = np.zeros((P, MIX_NMAX), F32)
    pre = np.zeros((P, MIX_NMAX), np.uint8)
    counts = np.asarray([len(d) for d in parts], np.int32)
    for p, d in enumerate(parts):
        boxes[p, :len(d)], scores[p, :len(d)] = d[:, :4], d[:, 4]
    pre[0, 1:1000:2] = 1
    pre[4, [0, 63, 64, 500, 1023]] = 1
    # rows past a problem's count: boxes that would suppress everything, scores above every valid one, flags set and unset
    boxes[:3, 1000:] = F32([-1e5, -1e5, 1e5, 1e5])
    scores[:3, 1000:] = F32(2.0)
    boxes[1, 64:], scores[1, 64:], pre[1, 64::2] = F32([5, 7, 24, 30]), F32(3.0), 1
    return (boxes, scores, counts, pre, 0.5), 'batched_mix'


# ------------------------------------------------------------------------------------------------------------------------ proposals
def level_shapes(H, W):
    return [(max(H // s, 1), max(W // s, 1)) for s in STRIDES]


def _maps(flat_scores, flat_deltas, H, W):
    """Per level: scores [n] and deltas [n,4] in the reference's (h, w, a) enumeration -> cls [1,A,h,w], box [1,4A,h,w]."""
    cls, box = [], []
    for (h, w), s, d in zip(level_shapes(H, W), flat_scores, flat_deltas):
        cls.append(np.ascontiguousarray(np.asarray(s, F32).reshape(h, w, A).transpose(2, 0, 1)[None]))
        box.append(np.ascontiguousarray(np.asarray(d, F32).reshape(h, w, A * 4).transpose(2, 0, 1)[None]))
    return cls, box


def _rand_deltas(rng, n):
    return rng.normal(0, 0.5, size=(n, 4)).astype(F32)


def _rand_scores(rng, n):
    """Distinct probabilities below 0.7."""
    return (0.05 + 0.6 * rng.permutation(n) / F32(n)).astype(F32)


def _bits(u):
    return np.asarray(u, np.uint32).view(F32)


# fields of a positive fp32's bits as the select sees them: digit1 = sign + exponent + 2 mantissa bits, digit2 = mantissa bits 20..10,
# digit3 = mantissa bits 9..0 (and the top bit of ~index, which is constant)
D1 = int(np.float32(0.75).view(np.uint32)) >> 21       # [0.75, 0.875)
D2, D3 = 1200, 16


def _decided_scores(rng, n, pre, where, run):
    """n scores whose pre-th largest key is decided in pass `where` by a bin of exactly `run` wanted keys. The pre - run keys above
    the cut share the bins of the cut in every earlier pass, and so do some of the keys below it: no earlier pass is exact."""
    up, lo = pre - run, n - pre
    assert up > 0 and lo >= 8 and n < (1 << 20)

    def word(d1, d2, d3):
        return (np.asarray(d1, np.int64) << 21) | (np.asarray(d2, np.int64) << 10) | np.asarray(d3, np.int64)
    r11, r10 = lambda k: rng.integers(0, 2048, k), lambda k: rng.integers(0, 1024, k)
    far = word(D1 - 1 - rng.integers(0, 6, lo), r11(lo), r10(lo))        # below the cut in digit1
    idx = rng.permutation(n)
    if where == 'digit1':
        upper, cut, lower = word(D1 + 1, r11(up), r10(up)), word(D1, r11(run), r10(run)), far
    elif where == 'digit2':
        upper, cut = word(D1, D2 + 1 + rng.integers(0, 800, up), r10(up)), word(D1, D2, r10(run))
        lower = np.where(np.arange(lo) % 2 == 0, word(D1, D2 - 1 - rng.integers(0, 1000, lo), r10(lo)), far)
    elif where == 'digit3':
        assert up <= 1000
        upper, cut = word(D1, D2, D3 + 1 + rng.permutation(1000)[:up]), word(D1, D2, np.full(run, D3))     # consecutive floats above the cut
        lower = np.where(np.arange(lo) % 3 == 0, word(D1, D2, rng.integers(0, D3, lo)),
                         np.where(np.arange(lo) % 3 == 1, word(D1, D2 - 1 - rng.integers(0, 1000, lo), r10(lo)), far))
    else:
        # a run of equal scores across the cut: `tied` anchors hold the score of the cut, the `need` lowest indices among them are
        # wanted. tail2: 512-blocks 0 and 1 of the index are wanted whole (the bin of block 1 is exact), block 3 is not wanted.
        # tail3: the cut falls inside block 1.
        assert n >= 2048 and run < 200 and up > 0
        blk0 = rng.permutation(512)[:40]
        blk1 = 512 + rng.permutation(512)[:run if where == 'tail2' else run + 30]
        blk3 = 1536 + rng.permutation(512)[:50]
        tied = np.concatenate([blk0, blk1, blk3])
        up = pre - (len(blk0) + run)
        rest = np.setdiff1d(np.arange(n), tied)
        rest = rest[rng.permutation(len(rest))]
        lo = n - len(tied) - up
        upper, cut = word(D1, D2, D3 + 1 + rng.integers(0, 1000, up)), word(D1, D2, np.full(len(tied), D3))
        far = word(D1 - 1 - rng.integers(0, 6, lo), r11(lo), r10(lo))
        lower = np.where(np.arange(lo) % 3 == 0, word(D1, D2, rng.integers(0, D3, lo)), far)
        idx = np.concatenate([rest[:up], tied, rest[up:]])
    s = np.empty(n, F32)
    s[idx] = _bits(np.concatenate([upper, cut, lower]).astype(np.uint32))
    assert np.isfinite(s).all() and (s > 0).all() and (s < 1).all()
    return s


def decided_in(where, run=1, pre=300, post=300, H=128, W=128):
    """The pre-th key of every level with more than pre + 8 anchors (32 x 32 x 3 and 16 x 16 x 3; only the first for the tail passes,
    whose ties must lie more than 512 indices apart) is decided in pass `where`, by a bin of exactly `run` keys that are all wanted
    (run = 1: the bin holds the cut alone; tail3, whose bins hold one key each: `run` of the run + 30 ties of index block 1 are
    wanted). The smaller levels hold random scores and take every anchor."""
    assert where in PASSES and where != 'tail1'
    rng = np.random.default_rng(PASSES.index(where) * 100 + run)
    scores, deltas = [], []
    for l, (h, w) in enumerate(level_shapes(H, W)):
        n = h * w * A
        structured = n > pre + 8 and (where.startswith('digit') or n >= 2048)
        scores.append(_decided_scores(rng, n, pre, where, run) if structured else _rand_scores(rng, n))
        deltas.append(_rand_deltas(rng, n))
    cls, box = _maps(scores, deltas, H, W)
    return (cls, box, F32([H - 3, W - 5, 1.0]), pre, post, 0.7, 0), 'decided_in_%s_run%d' % (where, run)


def level_smaller_than_k(pre=50):
    """64 x 64: levels of 768, 192, 48, 12 and 3 anchors. pre = 50: three levels smaller than pre (the 'fewer keys than needed' exit
    of the select); pre = 48: one level with exactly pre anchors."""
    H = W = 64
    rng = np.random.default_rng(pre)
    ns = [h * w * A for h, w in level_shapes(H, W)]
    cls, box = _maps([_rand_scores(rng, n) for n in ns], [_rand_deltas(rng, n) for n in ns], H, W)
    return (cls, box, F32([H - 3, W - 5, 1.0]), pre, 40, 0.7, 0), 'level_smaller_than_k_pre%d' % pre


def all_equal_scores(pre=300):
    """Every anchor of every level scores 0.5: the top-k is the first pre anchors of a level (rule (ii)), the NMS visits them last
    first (rule (i)), the merge ranks equal scores by concatenation index (rule (iii))."""
    H = W = 128
    rng = np.random.default_rng(7)
    ns = [h * w * A for h, w in level_shapes(H, W)]
    cls, box = _maps([np.full(n, 0.5, F32) for n in ns], [_rand_deltas(rng, n) for n in ns], H, W)
    return (cls, box, F32([H - 3, W - 5, 1.0]), pre, 200, 0.7, 0), 'all_equal_scores_pre%d' % pre


KILL = F32([0, 0, -10, -10])      # exp(-10) of an anchor's side: a box far below one pixel


def size_filter_kills_level(kind):
    """min_size 4. 'one': every box of level 2 (8 x 8 x 3) decodes to a side below one pixel and fails the filter. 'all_but_one': every
    level but level 3 (4 x 4 x 3 = 48 anchors) fails: the joint path then has fewer survivors than pre and than post."""
    assert kind in ('one', 'all_but_one')
    H = W = 128
    rng = np.random.default_rng(len(kind))
    ns = [h * w * A for h, w in level_shapes(H, W)]
    deltas = [_rand_deltas(rng, n) for n in ns]
    for l in ([2] if kind == 'one' else [0, 1, 2, 4]):
        deltas[l][:] = KILL
    cls, box = _maps([_rand_scores(rng, n) for n in ns], deltas, H, W)
    return (cls, box, F32([H - 3, W - 5, 1.0]), 300, 100, 0.7, 4), 'size_filter_kills_level_' + kind


# (dx, dy, dw, dh) that move an anchor of any level wholly outside the image: right, left, below, above, two corners
CLIP_OUT = [F32([50, 0, 0, 0]), F32([-50, 0, 0, 0]), F32([0, 50, 0, 0]), F32([0, -50, 0, 0]), F32([40, 40, -1, -1]), F32([-40, -40, 1, 2])]


def clip_saturated():
    """dw / dh at, one float above and far beyond BBOX_XFORM_CLIP = log(1000 / 16); dx / dy that move a box wholly outside the image
    on each side (clipped to a sliver one pixel wide on the border); im_info 3 rows and 5 columns smaller than the padded map."""
    H = W = 128
    rng = np.random.default_rng(12)
    clip = F32(np.log(1000.0 / 16.0))
    sat = [clip, np.nextafter(clip, F32(10)), np.nextafter(clip, F32(0)), F32(10), F32(88)]
    out = CLIP_OUT
    ns = [h * w * A for h, w in level_shapes(H, W)]
    deltas = []
    for n in ns:
        d = _rand_deltas(rng, n)
        k = np.arange(n)
        for j, v in enumerate(sat):
            d[k % 11 == j, 2] = v
            d[k % 13 == j, 3] = v
        for j, v in enumerate(out):
            d[k % 17 == j] = v
        deltas.append(d)
    cls, box = _maps([_rand_scores(rng, n) for n in ns], deltas, H, W)
    return (cls, box, F32([H - 3, W - 5, 1.0]), 300, 300, 0.7, 0), 'clip_saturated'


def _anchor_sides(stride):
    """(width, height) of the three anchors of a level: generate_anchors(stride, sizes = 8 stride, ratios 0.5, 1, 2)."""
    out = []
    for r in (0.5, 1.0, 2.0):
        ws = np.round(np.sqrt(stride * stride / r))
        hs = np.round(ws * r)
        out.append((ws * 8, hs * 8))
    return out


def nms_all_kept_hits_post():
    """Every anchor is shrunk to a quarter of its cell and the three anchors of a cell are moved apart: the boxes of a level are
    disjoint, the per-level NMS keeps all min(pre, n) of them, a level hands on its first post = 200 and the merge cuts the 652 at post. The scores are
    four values by turns: ties inside a level (visited in reversed runs) and across levels (the merge's binary searches)."""
    H = W = 128
    scores, deltas = [], []
    for (h, w), s in zip(level_shapes(H, W), STRIDES):
        n = h * w * A
        d = np.zeros((n, 4), F32)
        for a, (aw, ah) in enumerate(_anchor_sides(s)):
            d[a::A] = F32([(a - 1) * 0.3 * s / aw, (a - 1) * 0.3 * s / ah, np.log(0.25 * s / aw), np.log(0.25 * s / ah)])
        deltas.append(d)
        scores.append(F32([0.9, 0.6, 0.8, 0.7])[(np.arange(n) * 7 // 3 + len(scores)) % 4])
    cls, box = _maps(scores, deltas, H, W)
    return (cls, box, F32([H, W, 1.0]), 300, 200, 0.7, 0), 'nms_all_kept_hits_post'


# -------------------------------------------------------------------------------------------------------------------------- MaskROI
MAX_DET = 100
MROI_FILL = 256       # rows of the output buffers that csrc/detect.hip always defines


def _grid_rois(n, rng, cols=64):
    """n disjoint 10 x 10 ROIs on a grid of pitch 16 that starts at (-3, -3): the first row and column are clipped on."""
    i = np.arange(n)
    x, y = 16 * (i % cols) - 3, 16 * (i // cols) - 3
    rois = np.zeros((n, 5), F32)
    rois[:, 1:] = np.stack([x, y, x + 9, y + 9], 1)
    H, W = 16 * ((n + cols - 1) // cols) + 16, 16 * cols + 16
    return rois[rng.permutation(n)], F32([[H, W, 1.0]])


def _small_deltas(rng, n, C):
    """At most +-1 pixel of shift and a factor of e^+-0.2 of scale under the weights (10, 10, 5, 5): grid boxes stay disjoint."""
    return np.clip(rng.normal(0, 0.5, size=(n, 4 * C)), -1, 1).astype(F32)


def _one_hot(n, C, cls, scores):
    prob = np.zeros((n, C), F32)
    prob[np.arange(n), cls] = scores
    return prob


def _distinct(rng, n, lo=0.3, hi=0.99):
    return _scores_desc(n, hi, lo)[rng.permutation(n)]


def _mroi(rng, n, C, cls, scores, max_det=MAX_DET, tag=''):
    rois, im_info = _grid_rois(n, rng)
    return (rois, _small_deltas(rng, n, C), _one_hot(n, C, cls, scores), im_info, C, 0.05, 0.5, max_det), tag


def cut(T, max_det=MAX_DET, C=9):
    """T disjoint ROIs, one class each above the threshold (classes by turns), distinct scores: exactly T detections after the NMS,
    class-wise and class-agnostic."""
    rng = np.random.default_rng(T)
    return _mroi(rng, T, C, 1 + np.arange(T) % (C - 1), _distinct(rng, T), max_det, 'cut_%d' % T)


CUT_IN_TIE_T = MAX_DET + 20


def cut_in_tie(C=9):
    """120 detections; those at ranks max_det - 2 .. max_det + 3 of the descending scores hold one score: the `>=` of the reference
    returns max_det + 3 rows."""
    rng = np.random.default_rng(21)
    T = CUT_IN_TIE_T
    s = _scores_desc(T, 0.99, 0.3)
    s[MAX_DET - 3:MAX_DET + 3] = s[MAX_DET]
    return _mroi(rng, T, C, 1 + np.arange(T) % (C - 1), s[rng.permutation(T)], MAX_DET, 'cut_in_tie')


def last_byte_scores(C=9):
    """150 detections whose scores differ in the low 8 bits only: the first three passes of the radix select see one bin."""
    rng = np.random.default_rng(22)
    T = 150
    s = _bits((int(np.float32(0.75).view(np.uint32)) + rng.permutation(256)[:T]).astype(np.uint32))
    return _mroi(rng, T, C, 1 + np.arange(T) % (C - 1), s, MAX_DET, 'last_byte_scores')


def nothing_above_threshold(C=9):
    """Every probability at or below the score threshold (some exactly on it: the rule is `>`): the dummy ROI."""
    rng = np.random.default_rng(23)
    n = 40
    rois, im_info = _grid_rois(n, rng)
    prob = rng.uniform(0, 0.05, size=(n, C)).astype(F32)
    prob[::3, 1:] = F32(0.05)
    return (rois, _small_deltas(rng, n, C), prob, im_info, C, _f32_exact(0.05), 0.5, MAX_DET), 'nothing_above_threshold'


def one_class_only(C):
    """150 detections, all of class C // 2: empty classes before and after it in the prefix table."""
    rng = np.random.default_rng(C)
    T = 150
    return _mroi(rng, T, C, np.full(T, C // 2), _distinct(rng, T), MAX_DET, 'one_class_only_C%d' % C)


def sparse_classes(C):
    """150 detections of classes 2 and C - 2 only: empty classes at the start, in the middle and at the end."""
    rng = np.random.default_rng(100 + C)
    T = 150
    return _mroi(rng, T, C, np.where(np.arange(T) % 3 == 0, 2, C - 2), _distinct(rng, T), MAX_DET, 'sparse_classes_C%d' % C)


def every_class_one_box(C):
    """C - 1 detections, one of every class; max_det = (C - 1) // 2 + 1, so that the select cuts through them."""
    rng = np.random.default_rng(200 + C)
    T = C - 1
    return _mroi(rng, T, C, 1 + rng.permutation(T), _distinct(rng, T), T // 2 + 1, 'every_class_one_box_C%d' % C)


DEVICE_COUNT = (150, 220)     # valid rows, capacity


def device_count(C=9):
    """220 rows of which a device-side count declares the first 150 valid; the others hold probabilities of 0.999 and above for
    every class and huge boxes: they would fill the whole result if read."""
    rng = np.random.default_rng(24)
    n, cap = DEVICE_COUNT
    (rois, deltas, prob, im_info, C, st, nt, md), _ = _mroi(rng, cap, C, 1 + np.arange(cap) % (C - 1), _distinct(rng, cap))
    prob[n:] = rng.uniform(0.999, 1.0, size=(cap - n, C)).astype(F32)
    rois[n:, 1:] = F32([-1e5, -1e5, 1e5, 1e5])
    return (rois, deltas, prob, im_info, C, st, nt, md), 'device_count'


def agnostic_overflow(C=9):
    """1030 ROIs x 8 classes = 8240 probabilities above the threshold: more than the 8192 slots of the class-agnostic list. The host
    must raise; nothing is compared (class-wise the case is an ordinary one of 1030 candidates per class)."""
    rng = np.random.default_rng(25)
    n = 1030
    rois, im_info = _grid_rois(n, rng)
    prob = rng.uniform(0.2, 0.9, size=(n, C)).astype(F32)
    return (rois, _small_deltas(rng, n, C), prob, im_info, C, 0.05, 0.5, MAX_DET), 'agnostic_overflow'


def _cases(*specs):
    return [(fn, args) for fn, *args in specs]


NMS_CASES = _cases(
    *[(chain, n, t) for n in (64, 65, 128, 1024, 1025, 2000) for t in (0.5, 0.7)],
    *[(chain, n, 0.5, True) for n in (64, 65, 128, 1024, 1025, 2000)],
    (chain_by_blocks, 200), (chain_by_blocks, 1100),
    *[(all_same, n, eq) for n in (2, 64, 1000) for eq in (False, True)],
    *[(none_overlap, n) for n in (63, 64, 1024, 8192)],
    *[(exact_threshold, t, at) for t in (0.5, 0.7) for at in ('exact', 'below')],
    (degenerate,))
EXACT_CASES = _cases(*[(exact_threshold, t, at) for t in (0.5, 0.7) for at in ('exact', 'below')])
# the cases pinned to the reference's own `_nms` (tests/golden/ref_selection.npz)
REF_NMS_CASES = _cases((chain, 64, 0.5), (chain, 1025, 0.5), (chain, 64, 0.7), (chain, 1025, 0.7), (chain, 1025, 0.5, True),
                       (all_same, 64, False), (all_same, 1000, True), *[(exact_threshold, t, at) for t in (0.5, 0.7) for at in ('exact', 'below')])
DECIDED = [('digit1', 1), ('digit1', 7), ('digit2', 1), ('digit2', 7), ('digit3', 1), ('digit3', 7), ('tail2', 1), ('tail2', 60), ('tail3', 25)]
PROPOSAL_CASES = _cases(
    *[(decided_in, w, r) for w, r in DECIDED], (decided_in, 'digit2', 5, 1000, 300), (decided_in, 'tail3', 100, 1000, 1000),
    (level_smaller_than_k, 50), (level_smaller_than_k, 48), (all_equal_scores, 300), (all_equal_scores, 1000),
    (size_filter_kills_level, 'one'), (size_filter_kills_level, 'all_but_one'), (clip_saturated,), (nms_all_kept_hits_post,))
MASK_ROI_CASES = _cases(
    *[(cut, T) for T in (MAX_DET - 1, MAX_DET, MAX_DET + 1, 1025, 2049)], (cut_in_tie,), (last_byte_scores,), (nothing_above_threshold,),
    (one_class_only, 9), (one_class_only, 81), (sparse_classes, 9), (sparse_classes, 81), (every_class_one_box, 9), (every_class_one_box, 81))


def case_id(spec):
    fn, args = spec
    return '-'.join([fn.__name__] + [str(a) for a in args])
