"""CPU: every structured case of tests/selection_cases.py is in the regime it is named for, shown with the oracle and a restatement
of the key layout of the selects only (csrc/sort.h, csrc/common.h: which bits a pass looks at), never of the kernels. These are
conditions on the inputs: a later edit to a builder cannot move a case back into what the random draws of tests/test_ops_gpu.py cover
already without one of these failing."""
import os
import sys
import time

import numpy as np
import pytest

import oracle
from oracle import ops as oops

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import selection_cases as sc  # noqa: E402

F32 = np.float32
IDS = sc.case_id


# ------------------------------------------------------------------------------------------------------------------------------ NMS
def iou_matrix(b):
    """nms_kernel.cu:30-38 in fp32, every product and sum rounded on its own."""
    b = np.asarray(b, F32)
    x1, y1, x2, y2 = b[:, 0], b[:, 1], b[:, 2], b[:, 3]
    one, zero = F32(1), F32(0)
    w = np.maximum(np.minimum(x2[:, None], x2[None]) - np.maximum(x1[:, None], x1[None]) + one, zero)
    h = np.maximum(np.minimum(y2[:, None], y2[None]) - np.maximum(y1[:, None], y1[None]) + one, zero)
    inter = w * h
    area = (x2 - x1 + one) * (y2 - y1 + one)
    with np.errstate(invalid='ignore', divide='ignore'):
        return inter / (area[:, None] + area[None] - inter)


def analyse_nms(dets, thresh):
    """In the visiting order: (order, kept flags, depth) with depth = 0 for a box that no earlier box overlaps above the threshold,
    else 1 + the largest depth among those that do (the number of decisions that must be known before this one: the removal
    rounds of test_panoptic_cases_cpu.analyse)."""
    order = oops.argsort_desc(dets[:, 4])
    hit = iou_matrix(dets[order, :4]) > F32(thresh)
    n = len(order)
    kept, depth = np.zeros(n, bool), np.zeros(n, np.int64)
    for i in range(n):
        prev = np.where(hit[:i, i])[0]
        depth[i] = 1 + depth[prev].max() if len(prev) else 0
        kept[i] = not kept[prev].any()
    keep = oops.gpu_nms(dets, thresh)
    assert np.array_equal(order[kept], keep), "the analysis and the oracle disagree"
    return order, kept, depth, hit


CHAINS = [s for s in sc.NMS_CASES if s[0] is sc.chain]


@pytest.mark.parametrize('spec', CHAINS, ids=[IDS(s) for s in CHAINS])
def test_chain_keeps_every_second_box_at_depth_n_minus_1(spec):
    (dets, thresh), _ = spec[0](*spec[1])
    n = len(dets)
    order, kept, depth, hit = analyse_nms(dets, thresh)
    reverse = len(spec[1]) > 2 and spec[1][2]
    assert np.array_equal(order, np.arange(n)[::-1] if reverse else np.arange(n))
    assert np.array_equal(np.where(kept)[0], np.arange(0, n, 2))          # the even positions of the visiting order
    assert depth.max() == n - 1
    # box i meets i - 1 and i + 1 only
    assert np.array_equal(hit, np.abs(np.arange(n)[:, None] - np.arange(n)[None]) <= 1)
    assert len(np.unique(dets[:, 4])) == n


def test_chain_sizes_cover_the_block_and_kernel_edges():
    ns = sorted({s[1][0] for s in CHAINS})
    assert ns == [64, 65, 128, 1024, 1025, 2000]
    assert {s[1][1] for s in CHAINS} == {0.5, 0.7} and any(len(s[1]) > 2 and s[1][2] for s in CHAINS)


@pytest.mark.parametrize('n', [200, 1100])
def test_chain_by_blocks_suppresses_through_off_diagonal_words_only(n):
    (dets, thresh), _ = sc.chain_by_blocks(n)
    order, kept, depth, hit = analyse_nms(dets, thresh)
    assert np.array_equal(order, np.arange(n))
    i, j = np.where(np.triu(hit, 1))
    assert len(i) == (n - 1) // 64 and np.array_equal(j, np.arange(64, n, 64)) and np.array_equal(i, j - 1)
    assert (i // 64 != j // 64).all()                                     # no suppression inside a diagonal tile
    assert np.array_equal(np.where(~kept)[0], np.arange(64, n, 64))
    assert (n > 1024) == (n == 1100)


@pytest.mark.parametrize('n', [2, 64, 1000])
def test_all_same_keeps_one_box(n):
    (dets, thresh), _ = sc.all_same(n)
    assert len(np.unique(dets[:, :4], axis=0)) == 1 and len(np.unique(dets[:, 4])) == n
    assert oops.gpu_nms(dets, thresh).tolist() == [n // 3] and int(np.argmax(dets[:, 4])) == n // 3
    (dets, thresh), _ = sc.all_same(n, True)
    assert len(np.unique(dets[:, :4], axis=0)) == 1 and len(np.unique(dets[:, 4])) == 1
    assert oops.gpu_nms(dets, thresh).tolist() == [n - 1]                 # tie rule (i): the highest index is visited first


@pytest.mark.parametrize('n', [63, 64, 1024, 8192])
def test_none_overlap_keeps_all(n):
    (dets, thresh), _ = sc.none_overlap(n)
    assert len(dets) == n and len(np.unique(dets[:, 4])) == n
    b = dets[:, :4]
    m = min(n, 1500)                       # (the grid is regular: its first rows show every kind of neighbour)
    iou = iou_matrix(b[:m])
    assert (iou[~np.eye(m, dtype=bool)] == 0).all()
    keep = oops.gpu_nms(dets, thresh)
    order = oops.argsort_desc(dets[:, 4])
    assert np.array_equal(keep, order) and not np.array_equal(order, np.arange(n)) and not np.array_equal(order, np.arange(n)[::-1])


@pytest.mark.parametrize('thresh', [0.5, 0.7])
def test_exact_threshold_pairs_sit_on_the_threshold(thresh):
    (dets, t_exact), _ = sc.exact_threshold(thresh, 'exact')
    (dets_b, t_below), _ = sc.exact_threshold(thresh, 'below')
    assert np.array_equal(dets, dets_b)
    assert t_exact == float(F32(thresh)) and F32(t_below) == np.nextafter(F32(thresh), F32(0)) and float(F32(t_below)) == t_below
    n = len(dets)
    assert np.array_equal(oops.argsort_desc(dets[:, 4]), np.arange(n))
    iou = iou_matrix(dets[:, :4])
    pairs = sc.EXACT_POSITIONS
    for i, j in pairs:
        assert iou[i, j] == F32(thresh) and iou[i, j].dtype == F32, (i, j)              # the fp32 quotient IS the fp32 threshold
    off = np.triu(iou, 1)
    assert (off > 0).sum() == len(pairs)                                                  # nothing else overlaps
    assert sum(1 for i, j in pairs if i // 64 == j // 64 == 0 and j == i + 1) >= 3      # several per 64-block
    assert (63, 64) in pairs and any(i // 64 != j // 64 and (i, j) != (63, 64) for i, j in pairs)
    assert any(i // 64 == j // 64 and j - i > 8 for i, j in pairs)
    # `>` (gpu_nms): both kept on the threshold, the second dropped at the next float below
    seconds = sorted(j for _, j in pairs)
    assert np.array_equal(oops.gpu_nms(dets, t_exact), np.arange(n))
    assert np.array_equal(oops.gpu_nms(dets, t_below), np.setdiff1d(np.arange(n), seconds))
    # `>=` (cpu_nms, double threshold): the opposite decision on the threshold; both kept one float above it
    order = np.arange(n)
    assert oracle.cpu_nms(dets, t_exact, order) == np.setdiff1d(np.arange(n), seconds).tolist()
    assert oracle.cpu_nms(dets, float(np.nextafter(F32(thresh), F32(1))), order) == list(range(n))
    if thresh == 0.7:      # the double 0.7 lies above fp32(0.7): `>=` against it keeps both
        assert oracle.cpu_nms(dets, 0.7, order) == list(range(n))


def test_degenerate_boxes_have_finite_overlaps():
    (dets, thresh), _ = sc.degenerate()
    b = dets[:, :4]
    iou = iou_matrix(b)
    assert np.isfinite(iou[~np.eye(len(b), dtype=bool)]).all()            # (no box is ever compared with itself)
    w, h = b[:, 2] - b[:, 0] + 1, b[:, 3] - b[:, 1] + 1
    assert (w == 0).any() and (w < 0).any() and ((w < 0) & (h < 0)).any() and ((w == 1) & (h == 1)).sum() >= 4
    assert (np.abs(b) == 1e4).any(1).sum() >= 6
    area = w.astype(np.float64) * h.astype(np.float64)
    assert (area != (w * h).astype(np.float64)).any()                     # a product that fp32 rounds
    assert (iou_matrix(b)[np.isfinite(iou)] <= 0).any() and np.signbit(iou[np.isfinite(iou)]).any()      # a negative union: -0
    keep = oops.gpu_nms(dets, thresh)
    assert 4 <= len(keep) < len(dets)


def test_batched_mix_holds_the_named_problems():
    (boxes, scores, counts, pre, thresh), _ = sc.batched_mix()
    assert boxes.shape == (5, sc.MIX_NMAX, 4) and counts.tolist() == [1000, 64, 0, 1, sc.MIX_NMAX]
    want = batched_reference(boxes, scores, counts, pre, thresh)
    assert np.array_equal(want[0], np.arange(0, 1000, 2))                 # nothing suppressed once the odd boxes are gone
    assert pre[0, 1:1000:2].all() and not pre[0, 0:1000:2].any()
    alive = iou_matrix(boxes[0, 0:1000:2])
    assert (alive[~np.eye(500, dtype=bool)] <= np.float32(thresh)).all()
    assert pre[4].sum() == 5 and pre[4, [0, 63, 64, 1023]].all() and not pre[2].any() and not pre[3].any()
    full = oops.gpu_nms(np.hstack([boxes[0, :1000], scores[0, :1000, None]]), thresh)
    assert np.array_equal(full, np.arange(0, 1000, 2))                    # (the same list, but by suppression)
    assert len(want[1]) == 1 and len(want[2]) == 0 and want[3].tolist() == [0] and len(want[4]) == sc.MIX_NMAX - 5
    # the rows past the counts would change every result if they were read
    assert (scores[0, 1000:] > scores[0, :1000].max()).all() and (scores[1, 64:] > scores[1, :64].max()).all()


def batched_reference(boxes, scores, counts, pre, thresh):
    out = []
    for p, c in enumerate(counts):
        alive = np.where(pre[p, :c] == 0)[0]
        d = np.hstack([boxes[p, :c], scores[p, :c, None]])[alive]
        out.append(alive[oops.gpu_nms(d, thresh)] if len(alive) else np.zeros((0,), np.int64))
    return out


@pytest.mark.parametrize('spec', sc.NMS_CASES, ids=[IDS(s) for s in sc.NMS_CASES])
def test_oracle_runs_every_nms_case_in_under_a_second(spec):
    (dets, thresh), tag = spec[0](*spec[1])
    assert dets.dtype == F32 and dets.shape[1] == 5 and len(dets) <= 8192 and np.isfinite(dets).all()
    t0 = time.perf_counter()
    keep = oops.gpu_nms(dets, thresh)
    dt = time.perf_counter() - t0
    assert dt < 1.0, "%s: %.2f s" % (tag, dt)
    assert len(keep) >= 1
    assert np.array_equal(spec[0](*spec[1])[0][0], dets)
    assert all(s in sc.NMS_CASES for s in sc.REF_NMS_CASES + sc.EXACT_CASES)


# ------------------------------------------------------------------------------------------------------------------------ proposals
def float_key(s):
    u = np.asarray(s, F32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def level_keys(cls_l):
    """The 64-bit keys of one level: float_key(score) << 32 | ~index, index in the (h, w, a) enumeration."""
    s = np.asarray(cls_l, F32)[0].transpose(1, 2, 0).reshape(-1)
    idx = np.arange(len(s), dtype=np.uint64)
    return (float_key(s).astype(np.uint64) << np.uint64(32)) | (~idx & np.uint64(0xffffffff)), s


def select_trace(keys, need):
    """Walk the digits of sc.PASS_BITS from the top: in every pass the bin of the need-th largest key among the keys that match the
    decided prefix. Returns (how, [(pass, keys in the picked bin, keys still needed from it)], threshold key): how = the pass
    whose picked bin holds exactly the keys still needed, 'fewer' when fewer keys than needed exist, 'last' when no pass is exact."""
    keys = np.asarray(keys, np.uint64)
    if len(keys) < need:
        return 'fewer', [], np.uint64(0)
    prefix, trace = np.uint64(0), []
    for name, (shift, hi) in zip(sc.PASSES, sc.PASS_BITS):
        m = keys if hi == 64 else keys[((keys ^ prefix) >> np.uint64(hi)) == 0]
        digit = ((m >> np.uint64(shift)) & np.uint64((1 << (hi - shift)) - 1)).astype(np.int64)
        cnt = np.bincount(digit, minlength=1 << (hi - shift))
        above = np.cumsum(cnt[::-1])[::-1] - cnt                     # keys in the bins above each bin
        b = int(np.where((above < need) & (need <= above + cnt))[0][-1])
        prefix |= np.uint64(b) << np.uint64(shift)
        need -= int(above[b])
        trace.append((name, int(cnt[b]), need))
        if cnt[b] == need:
            return name, trace, prefix
    return 'last', trace, prefix


def check_select(cls_l, pre):
    """The trace of one level, checked against the oracle's top-k (rule (ii): score descending, index ascending)."""
    keys, s = level_keys(cls_l)
    how, trace, thr = select_trace(keys, pre)
    want = np.argsort(-s, kind='stable')[:pre]
    got = np.arange(len(s)) if how == 'fewer' else np.where(keys >= thr)[0]
    assert np.array_equal(np.sort(got), np.sort(want)), "the restated select and the oracle's top-k disagree"
    return how, trace


DECIDED = [s for s in sc.PROPOSAL_CASES if s[0] is sc.decided_in]


@pytest.mark.parametrize('spec', DECIDED, ids=[IDS(s) for s in DECIDED])
def test_decided_in_the_named_pass(spec):
    where, run = spec[1][0], spec[1][1]
    (cls, box, im_info, pre, post, thr, ms), _ = sc.decided_in(*spec[1])
    hows = [check_select(c, pre) for c in cls]
    how, trace = hows[0]
    assert how == where, trace
    if where == 'tail3':       # (a bin of the last pass holds one key) `run` of the run + 30 ties of index block 1 are wanted
        assert trace[-1] == (where, 1, 1) and trace[-2] == ('tail2', run + 30, run)
    else:
        assert trace[-1] == (where, run, run)                              # the picked bin: `run` keys, all of them wanted
    assert all(v > need for _, v, need in trace[:-1])                      # no earlier pass is exact
    assert len(trace) == sc.PASSES.index(where) + 1
    for (h, _), c in zip(hows[1:], cls[1:]):
        n = c.size
        assert h == ('fewer' if n < pre else where if (n > pre + 8 and where.startswith('digit')) else h)
    assert hows[-1][0] == 'fewer'
    if where.startswith('tail'):
        keys, s = level_keys(cls[0])
        cut = np.sort(s)[::-1][pre - 1]
        tied = np.where(s == cut)[0]
        assert len(tied) > trace[2][2] and np.ptp(tied) > 512             # more ties than needed, more than 512 indices apart
        assert trace[3][1] == len(tied)                                    # tail1 separates nothing
        assert len(s) < (1 << 20)
    if where == 'digit3':
        s = level_keys(cls[0])[1]
        top = np.sort(s)[::-1][:pre]
        assert len(np.unique(top.view(np.uint32) >> 10)) == 1            # the kept scores differ in their low 10 bits only


def test_decided_in_covers_every_pass_that_can_occur():
    named = {s[1][0] for s in DECIDED}
    assert named == set(sc.PASSES) - {'tail1'}
    runs = {(s[1][0], s[1][1] == 1) for s in DECIDED}
    assert all((w, one) in runs for w in ('digit1', 'digit2', 'digit3', 'tail2') for one in (True, False))
    assert {s[1][2] for s in DECIDED if len(s[1]) > 2} == {1000}
    # tail1 = bits [31,20) of ~index: all ones below 2^20 anchors, so all matching keys share one bin and the pass cannot be exact
    assert all(c.size < (1 << 20) for s in sc.PROPOSAL_CASES for c in s[0](*s[1])[0][0])


@pytest.mark.parametrize('pre', [50, 48])
def test_levels_smaller_than_k_take_the_fewer_keys_exit(pre):
    (cls, box, im_info, pre_, post, thr, ms), _ = sc.level_smaller_than_k(pre)
    assert pre_ == pre and [c.size for c in cls] == [768, 192, 48, 12, 3]
    hows = [check_select(c, pre)[0] for c in cls]
    if pre == 50:
        assert hows[2:] == ['fewer'] * 3 and 'fewer' not in hows[:2]
    else:
        assert hows[3:] == ['fewer'] * 2 and hows[2] != 'fewer'           # exactly pre anchors: the select runs and takes them all
    _, _, levels = _proposals(sc.level_smaller_than_k(pre)[0], return_levels=True)
    assert all(k >= 1 for k in levels)


@pytest.mark.parametrize('pre', [300, 1000])
def test_all_equal_scores_select_by_index_alone(pre):
    (cls, box, im_info, pre_, post, thr, ms), _ = sc.all_equal_scores(pre)
    assert len(np.unique(np.concatenate([c.reshape(-1) for c in cls]))) == 1
    how, trace = check_select(cls[0], pre)
    assert how == 'tail3' and trace[2][1] == cls[0].size                   # the digit passes see one bin
    rois, scores = _proposals(sc.all_equal_scores(pre)[0])
    assert len(scores) == post and len(np.unique(scores)) == 1


def _proposals(inputs, individual=True, **kw):
    cls, box, im_info, pre, post, thr, ms = inputs
    return oops.pyramid_proposal(cls, box, im_info, pre_nms_top_n=pre, post_nms_top_n=post, nms_thresh=thr, min_size=ms,
                                 individual_proposals=individual, **kw)


def _decode(inputs, l):
    """Clipped boxes of every anchor of level l and the size-filter flags."""
    cls, box, im_info, pre, post, thr, ms = inputs
    s = sc.STRIDES[l]
    h, w = cls[l].shape[2:]
    sx, sy = np.meshgrid(np.arange(w) * s, np.arange(h) * s)
    shifts = np.vstack((sx.ravel(), sy.ravel(), sx.ravel(), sy.ravel())).transpose()
    anchors = (oops.generate_anchors(stride=s, sizes=np.array((8,)) * s, aspect_ratios=(0.5, 1, 2)).reshape((1, sc.A, 4)) +
               shifts.reshape((1, -1, 4)).transpose((1, 0, 2))).reshape((-1, 4))
    deltas = box[l].transpose((0, 2, 3, 1)).reshape((-1, 4))
    raw = oops.bbox_transform(anchors, deltas)
    p = oops.clip_boxes(raw, im_info[:2])
    ok = (p[:, 2] - p[:, 0] + F32(1) >= F32(ms) * im_info[2]) & (p[:, 3] - p[:, 1] + F32(1) >= F32(ms) * im_info[2])
    return raw, p, ok, deltas


@pytest.mark.parametrize('kind', ['one', 'all_but_one'])
def test_size_filter_empties_whole_levels(kind):
    inputs, _ = sc.size_filter_kills_level(kind)
    cls, box, im_info, pre, post, thr, ms = inputs
    ok = [_decode(inputs, l)[2] for l in range(5)]
    dead = [2] if kind == 'one' else [0, 1, 2, 4]
    for l in range(5):
        assert (not ok[l].any()) if l in dead else ok[l].sum() >= min(100, ok[l].size // 4)
    rois, scores, levels = _proposals(inputs, return_levels=True)
    assert [k == 0 for k in levels] == [l in dead for l in range(5)] and len(scores) >= 1
    jr, js = _proposals(inputs, individual=False, pad=False)
    assert len(js) >= 1
    if kind == 'all_but_one':
        survivors = sum(int(o.sum()) for o in ok)
        assert survivors == ok[3].sum() and 12 <= survivors < post < pre and len(js) <= survivors
        # joint keys: an anchor that fails the filter has key 0; with fewer survivors than pre the cut falls among the equal zero
        # keys, no pass is exact and the select ends on its last pass with threshold 0
        keys = np.concatenate([np.where(o, level_keys(c)[0], np.uint64(0)) for o, c in zip(ok, cls)])
        how, trace, thr_key = select_trace(keys, pre)
        assert how == 'last' and thr_key == 0 and len(trace) == 6


def test_clip_saturated_reaches_the_clip_value_and_the_borders():
    inputs, _ = sc.clip_saturated()
    cls, box, im_info, pre, post, thr, ms = inputs
    clip = oops.BBOX_XFORM_CLIP
    assert im_info[0] == cls[0].shape[2] * 4 - 3 and im_info[1] == cls[0].shape[3] * 4 - 5
    for l in range(4):                     # (the 12 anchors of the last level cannot hold every value)
        raw, p, ok, d = _decode(inputs, l)
        top = np.argsort(-level_keys(cls[l])[1], kind='stable')[:pre]     # what the kernel decodes
        for col in (2, 3):
            assert (d[top, col] == clip).any() and (d[top, col] > clip).any()
        if True:
            assert (d[top, 2] == np.nextafter(clip, F32(10))).any() and (d[top, 2] == np.nextafter(clip, F32(0))).any()
            outside = (raw[top, 0] > im_info[1]) | (raw[top, 2] < 0) | (raw[top, 1] > im_info[0]) | (raw[top, 3] < 0)
            sliver = (p[top, 2] == p[top, 0]) | (p[top, 3] == p[top, 1])
            assert outside.sum() >= 4 and (outside & sliver).sum() >= 4
            for v in sc.CLIP_OUT:          # each of the built displacements is among the decoded boxes, and ends as a sliver
                rows = (d[top] == v).all(1)
                assert rows.any() and (outside & sliver)[rows].all(), (l, v)
    rois, scores = _proposals(inputs)
    assert len(scores) >= 50


def test_nms_all_kept_hits_post_with_ties_across_levels():
    inputs, _ = sc.nms_all_kept_hits_post()
    cls, box, im_info, pre, post, thr, ms = inputs
    rois, scores, levels = _proposals(inputs, return_levels=True)
    assert levels == [min(post, c.size) for c in cls] and sum(levels) == 652 > post == len(scores)
    # (a level hands on its first post kept boxes) without that cut: every box of the top-k survives the NMS
    assert _proposals((cls, box, im_info, pre, pre, thr, ms), return_levels=True)[2] == [min(pre, c.size) for c in cls]
    assert len(np.unique(np.concatenate([c.reshape(-1) for c in cls]))) == 4
    # the score at the cut is shared by kept boxes of several levels, some before and some after the cut
    per_level = []
    for l in range(5):
        top = np.argsort(-level_keys(cls[l])[1], kind='stable')[:pre]
        per_level.append(level_keys(cls[l])[1][top])
    cut = scores[-1]
    assert sum(1 for s in per_level if (s == cut).any()) >= 3
    assert sum(int((s == cut).sum()) for s in per_level) > int((scores == cut).sum()) >= 2


@pytest.mark.parametrize('spec', sc.PROPOSAL_CASES, ids=[IDS(s) for s in sc.PROPOSAL_CASES])
def test_oracle_runs_every_proposal_case_in_under_a_second(spec):
    inputs, tag = spec[0](*spec[1])
    cls, box, im_info, pre, post, thr, ms = inputs
    assert len(cls) == 5 and cls[0].shape[2] <= 32 and cls[0].shape[3] <= 32 and post <= pre <= 1000
    assert all(c.dtype == F32 and b.dtype == F32 and c.shape[1] == sc.A and b.shape[1] == 4 * sc.A for c, b in zip(cls, box))
    assert all(((c > 0) & (c < 1)).all() for c in cls)
    for individual in (True, False):
        t0 = time.perf_counter()
        rois, scores = _proposals(inputs, individual=individual, pad=False)
        dt = time.perf_counter() - t0
        assert dt < 1.0, "%s: %.2f s" % (tag, dt)
        assert len(scores) >= 1 and rois.shape == (len(scores), 5)         # no case is satisfied by an empty result
    again, _ = spec[0](*spec[1])
    assert all(np.array_equal(a, b) for a, b in zip(again[0] + again[1], cls + box))


# -------------------------------------------------------------------------------------------------------------------------- MaskROI
def _mask_roi(inputs, agn, clip, rows=None):
    rois, deltas, prob, im_info, C, st, nt, md = inputs
    r = slice(None) if rows is None else slice(0, rows)
    return oops.mask_roi(rois[r], deltas[r], prob[r], im_info, C, nt, st, md, agn, clip=clip)


VARIANTS = [(agn, clip) for agn in (False, True) for clip in (True, False)]


@pytest.mark.parametrize('T', [sc.MAX_DET - 1, sc.MAX_DET, sc.MAX_DET + 1, 1025, 2049])
def test_cut_keeps_exactly_T_before_the_select(T):
    inputs, _ = sc.cut(T)
    rois, deltas, prob, im_info, C, st, nt, md = inputs
    assert md == sc.MAX_DET and len(rois) == T
    assert ((prob > st).sum(1) == 1).all() and len(np.unique(prob[prob > st])) == T
    assert len(np.unique(np.argmax(prob, 1))) == C - 1
    for agn, clip in VARIANTS:
        # without a cut every box survives the NMS: T detections
        s, b, c = oops.mask_roi(rois, deltas, prob, im_info, C, nt, st, 0, agn, clip=clip)
        assert len(s) == T, (agn, clip)
        s, b, c = _mask_roi(inputs, agn, clip)
        assert len(s) == min(T, md)
        assert np.array_equal(np.sort(s), np.sort(prob[prob > st])[-len(s):])
    on, off = _mask_roi(inputs, False, True)[1], _mask_roi(inputs, False, False)[1]
    assert T < md or not np.array_equal(on, off) or (off >= 0).all()
    full_on = oops.mask_roi(rois, deltas, prob, im_info, C, nt, st, 0, False, clip=True)[1]
    full_off = oops.mask_roi(rois, deltas, prob, im_info, C, nt, st, 0, False, clip=False)[1]
    assert (full_off < 0).any() and not (full_on < 0).any()                # clipping changes some boxes


def test_cut_in_tie_returns_more_than_max_det_rows():
    inputs, _ = sc.cut_in_tie()
    md = inputs[7]
    for agn, clip in VARIANTS:
        s, b, c = _mask_roi(inputs, agn, clip)
        assert len(s) == md + 3
        rs = np.sort(s)[::-1]
        assert rs[md - 1] == rs[md] and rs[md - 3] == rs[md + 2] and rs[md - 4] > rs[md - 3]
    allscores = np.sort(inputs[2][inputs[2] > inputs[5]])[::-1]
    assert len(allscores) == sc.CUT_IN_TIE_T and allscores[md + 2] > allscores[md + 3]


def test_last_byte_scores_agree_in_their_top_24_key_bits():
    inputs, _ = sc.last_byte_scores()
    prob, st, md = inputs[2], inputs[5], inputs[7]
    s = prob[prob > st]
    k = float_key(s)
    assert len(s) == 150 > md and len(np.unique(k >> 8)) == 1 and len(np.unique(k & 0xff)) == 150
    for agn, clip in VARIANTS:
        assert len(_mask_roi(inputs, agn, clip)[0]) == md


def test_nothing_above_threshold_gives_the_dummy_roi():
    inputs, _ = sc.nothing_above_threshold()
    prob, st = inputs[2], inputs[5]
    assert (prob[:, 1:] == F32(st)).any() and not (prob[:, 1:] > F32(st)).any()
    for agn, clip in VARIANTS:
        s, b, c = _mask_roi(inputs, agn, clip)
        assert s.tolist() == [1.0] and not b.any() and c.tolist() == [0]


@pytest.mark.parametrize('C', [9, 81])
def test_class_tables_have_empty_classes_where_named(C):
    for fn, classes in [(sc.one_class_only, [C // 2]), (sc.sparse_classes, [2, C - 2])]:
        inputs, _ = fn(C)
        prob, st, md = inputs[2], inputs[5], inputs[7]
        used = np.unique(np.where(prob > st)[1])
        assert used.tolist() == classes and 1 not in used and C - 1 not in used
        for agn, clip in VARIANTS:
            s, b, c = _mask_roi(inputs, agn, clip)
            assert len(s) == md < (prob > st).sum() and set(c.tolist()) == set(classes)
    inputs, _ = sc.every_class_one_box(C)
    prob, st, md = inputs[2], inputs[5], inputs[7]
    assert np.array_equal(np.sort(np.where(prob > st)[1]), np.arange(1, C)) and 1 < md < C - 1
    for agn, clip in VARIANTS:
        s, b, c = _mask_roi(inputs, agn, clip)
        assert len(s) == md and len(set(c.tolist())) == md


def test_device_count_rows_past_the_count_would_win():
    inputs, _ = sc.device_count()
    n, cap = sc.DEVICE_COUNT
    rois, deltas, prob, im_info, C, st, nt, md = inputs
    assert len(rois) == cap and np.isfinite(rois).all() and (prob[n:] > prob[:n].max()).all()
    for agn, clip in VARIANTS:
        s, b, c = _mask_roi(inputs, agn, clip, rows=n)
        assert len(s) == md and s.max() < 0.999
        s2, _, _ = _mask_roi(inputs, agn, clip)
        assert s2.max() >= 0.999                                           # read in full, the garbage comes first


def test_agnostic_overflow_exceeds_the_candidate_slots():
    inputs, _ = sc.agnostic_overflow()
    prob, C, st = inputs[2], inputs[4], inputs[5]
    assert len(prob) * (C - 1) > 8192 and (prob[:, 1:] > st).sum() > 8192 and len(prob) <= 8192


@pytest.mark.parametrize('spec', sc.MASK_ROI_CASES, ids=[IDS(s) for s in sc.MASK_ROI_CASES])
def test_oracle_runs_every_mask_roi_case_in_under_a_second(spec):
    inputs, tag = spec[0](*spec[1])
    rois, deltas, prob, im_info, C, st, nt, md = inputs
    assert rois.shape == (len(prob), 5) and deltas.shape == (len(prob), 4 * C) and prob.shape[1] == C and im_info.shape == (1, 3)
    assert all(a.dtype == F32 for a in (rois, deltas, prob, im_info))
    for agn, clip in VARIANTS:
        t0 = time.perf_counter()
        s, b, c = _mask_roi(inputs, agn, clip)
        dt = time.perf_counter() - t0
        assert dt < 1.0, "%s: %.2f s" % (tag, dt)
        assert len(s) >= 1 and (spec[0] is sc.nothing_above_threshold or c.min() >= 1)
    again, _ = spec[0](*spec[1])
    assert all(np.array_equal(a, b) for a, b in zip(again[:4], inputs[:4]))
