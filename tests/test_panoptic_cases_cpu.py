"""CPU: every structured panoptic case of tests/panoptic_cases.py is in the regime it is named for (oracle only). These are conditions
on the inputs, not measurements of the kernels: a later edit to a builder cannot move a case back into the regime the random draws
of tests/test_ops_gpu.py cover already without one of these failing."""
import os
import sys
import time

import numpy as np
import pytest

import oracle
from oracle import ops as oops

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import panoptic_cases as pc  # noqa: E402

MR_MAXCAND = 64      # candidate list of mask_removal_kernel (upsnet_amd/csrc/panoptic.hip)


def _geometry(r4, H, W):
    """MaskRemoval's box of one instance (mask_removal.py:60-77): (bx, by, w, h, x_0, x_1, y_0, y_1), clipped, stops clamped."""
    x1, y1, x2, y2 = [int(v) for v in np.asarray(r4, np.float32).astype(np.int32)]
    w, h = max(x2 - x1 + 1, 1), max(y2 - y1 + 1, 1)
    x_0, x_1 = max(x1, 0), min(x2 + 1, W, x1 + w)
    y_0, y_1 = max(y1, 0), min(y2 + 1, H, y1 + h)
    return x1, y1, w, h, x_0, x_1, y_0, y_1


def analyse(inputs, m=None):
    """Per instance, from the boxes, the resampled masks and the oracle's keep list: clipped box, mask_sum, overlap with the kept
    same-class predecessors, the number of those whose box meets its box, its decision, and the removal round that decides it
    (1 + the latest round among the live same-class predecessors whose box meets its box)."""
    fcn, rois5, prob, logit, cls, S, C, H, W = inputs
    m = len(prob) if m is None else m
    rois, prob, logit, cls = rois5[:m, 1:], prob[:m], logit[:m], cls[:m]
    keep, _ = oops.mask_removal(rois, prob, logit, cls, (H, W), want_energy=False)
    order = oops.argsort_desc(prob)
    box, mask = {}, {}
    for i in range(m):
        bx, by, w, h, x_0, x_1, y_0, y_1 = _geometry(rois[i], H, W)
        full = np.zeros((H, W), bool)
        if x_1 > x_0 and y_1 > y_0:
            full[y_0:y_1, x_0:x_1] = oracle.resize_bilinear(logit[i, 0], w, h)[y_0 - by:y_1 - by, x_0 - bx:x_1 - bx] > 0
        box[i], mask[i] = (x_0, x_1, y_0, y_1), full
    out, seen = {}, []
    occ = np.zeros((C, H, W), bool)
    for i in order:
        a = box[i]
        s = int(mask[i].sum())
        live = a[1] > a[0] and a[3] > a[2] and s > 0
        meets = [j for j in seen if cls[j] == cls[i] and a[0] < box[j][1] and box[j][0] < a[1] and a[2] < box[j][3] and box[j][2] < a[3]]
        ov = int((mask[i] & occ[cls[i]]).sum())
        kept = live and not (ov / s > 0.3)
        rnd = 0 if not live else 1 + max([out[j]['round'] for j in meets], default=0)
        out[i] = dict(box=a, sum=s, ov=ov, kept=kept, round=rnd, kept_meeting=sum(1 for j in meets if out[j]['kept']))
        if kept:
            occ[cls[i]] |= mask[i]
        seen.append(i)
    mine = [i for i in order if out[i]['kept']]
    assert mine == list(keep) or (not mine and list(keep) == [0]), "the analysis and the oracle disagree"
    return out, order


@pytest.mark.parametrize('kind,decision', [('dropped', False), ('kept', True), ('middle', True)])
def test_crowd_overflows_the_candidate_list(kind, decision):
    inputs, tag = pc.crowd(kind)
    info, order = analyse(inputs)
    wide = info[pc.crowd_wide(kind)]
    H, W = inputs[7], inputs[8]
    assert wide['box'] == (0, W, 0, H)
    assert wide['kept_meeting'] >= 65 > MR_MAXCAND
    assert wide['kept'] == decision
    ratio = wide['ov'] / wide['sum']
    assert ratio > 0.4 if kind == 'dropped' else ratio < 0.2, ratio           # clearly on its side of 0.3
    cls = inputs[4]
    assert sum(1 for i in info if cls[i] == 1 and info[i]['kept'] and i != pc.crowd_wide(kind)) >= 70
    assert (cls == 2).sum() >= 4
    if kind == 'middle':
        pos = list(order).index(pc.crowd_wide(kind))
        later = [i for i in order[pos + 1:] if cls[i] == 1]
        assert 20 < pos and len(later) >= 10
        assert any(info[i]['kept'] for i in later) and any(not info[i]['kept'] for i in later)    # the wide mask decides them


def test_threshold_pairs_sit_on_and_beside_three_tenths():
    n = pc.THRESHOLD_N
    for variant, ov, kept in [('exact', 3 * n, True), ('plus', 3 * n + 1, False), ('minus', 3 * n - 1, True)]:
        inputs, _ = pc.threshold_exact(variant)
        info, _ = analyse(inputs)
        assert info[0]['kept'] and info[0]['ov'] == 0
        assert (info[1]['ov'], info[1]['sum']) == (ov, 10 * n), variant
        assert info[1]['kept'] == kept, variant
    # the pair on the threshold separates '>' from '>=' and an fp64 compare from an fp32 one
    assert not (3 * n) / (10 * n) > 0.3 and float(np.float32(0.3)) > 0.3


@pytest.mark.parametrize('kind', ['alternating', 'all_kept'])
@pytest.mark.parametrize('reverse', [False, True])
def test_chain_needs_a_round_per_box(kind, reverse):
    inputs, _ = pc.chain(kind, reverse)
    info, order = analyse(inputs)
    cls = inputs[4]
    row = [i for i in order if cls[i] == 1]
    assert len(row) >= 40
    assert max(info[i]['round'] for i in row) >= 32
    if reverse:
        assert row == sorted(row, reverse=True)
    else:
        assert row == sorted(row)
    kept, dropped = sum(info[i]['kept'] for i in row), sum(not info[i]['kept'] for i in row)
    if kind == 'alternating':
        assert kept >= 15 and dropped >= 15
        assert all(info[a]['kept'] != info[b]['kept'] for a, b in zip(row, row[1:]))
        assert all(info[i]['ov'] / info[i]['sum'] > 0.3 for i in row if not info[i]['kept'])
    else:
        assert dropped == 0
        assert all(0 < info[i]['ov'] / info[i]['sum'] < 0.3 for i in row[1:])


def test_many_and_tie_cases_have_the_stated_sizes():
    for m, one in [(300, False), (1024, False), (1024, True)]:
        (fcn, rois5, prob, logit, cls, S, C, H, W), _ = pc.many(m, one)
        assert len(prob) == m and H * W <= 64 * 96 and C - 1 == 8
        assert (len(np.unique(cls)) == 1 and cls[0] == 1) if one else len(np.unique(cls)) == 8
    for m in (70, 300):
        prob = pc.ties_all_equal(m)[0][2]
        assert len(prob) == m and len(np.unique(prob)) == 1
    assert 70 <= 256 < 300                    # one size for each sort path of mask_removal_kernel
    for m in (150, 400):
        prob = pc.ties_blocks(m)[0][2]
        assert len(prob) == m and len(np.unique(prob)) == 5
    for ms in (2, 14, 32):
        assert pc.mask_side(ms)[0][3].shape[1:] == (1, ms, ms)


@pytest.mark.parametrize('W', [65, 127, 130])
def test_word_edges_boxes_sit_where_they_are_named(W):
    inputs, _ = pc.word_edges(W)
    info, order = analyse(inputs)
    H = inputs[7]
    assert H % 2 == 1
    cols = {info[i]['box'][:2] for i in info if info[i]['box'][1] > info[i]['box'][0] and info[i]['box'][3] > info[i]['box'][2]}
    assert {(63, 64), (64, 65), (0, 64), (63, min(129, W))} <= cols
    assert sum(1 for c in cols if c[1] == W) >= 3 and (W - 1, W) in cols
    empty = [i for i in info if not (info[i]['box'][1] > info[i]['box'][0] and info[i]['box'][3] > info[i]['box'][2])]
    assert len(empty) >= 7                    # four wholly outside, three with x2 < x1 or y2 < y1
    assert any(info[i]['box'] == (10, 11, 10, 11) for i in info)          # sub-pixel -> one pixel
    rois = inputs[1][:, 1:]
    assert ((rois < 0) & (rois != np.trunc(rois))).any()
    d = pc.word_edges_dead(W)
    pos = list(order).index(d)
    before, after = order[pos - 1], order[pos + 1]
    assert info[d]['sum'] == 0 and info[d]['box'][1] > info[d]['box'][0]
    assert inputs[4][before] == inputs[4][d] == inputs[4][after]
    assert info[before]['sum'] > 0 and info[after]['sum'] > 0 and int((_mask_and(inputs, before, after))) > 0


def _mask_and(inputs, a, b):
    """Pixels that the masks of instances a and b share."""
    H, W = inputs[7], inputs[8]
    ms = []
    for i in (a, b):
        bx, by, w, h, x_0, x_1, y_0, y_1 = _geometry(inputs[1][i, 1:], H, W)
        full = np.zeros((H, W), bool)
        full[y_0:y_1, x_0:x_1] = oracle.resize_bilinear(inputs[3][i, 0], w, h)[y_0 - by:y_1 - by, x_0 - bx:x_1 - bx] > 0
        ms.append(full)
    return (ms[0] & ms[1]).sum()


def test_device_count_rows_after_the_count_are_arbitrary():
    (fcn, rois5, prob, logit, cls, S, C, H, W), _ = pc.device_count()
    n = pc.DEVICE_COUNT
    assert len(prob) == 64 and n == 37
    assert np.isfinite(rois5).all() and np.isfinite(prob).all() and np.isfinite(logit).all()
    assert (prob[n:] > prob[:n].max()).all() and (cls[n:] > C).all()        # they would come first and index past every table
    keep, _ = oops.mask_removal(rois5[:n, 1:], prob[:n], logit[:n], cls[:n], (H, W), want_energy=False)
    assert 1 < len(keep) < n


def test_fuse_cases_have_the_widths_and_counts_they_are_named_for():
    rem = [w % 4 for w in pc.ODD_WIDTHS]
    assert {65, 101, 130, 258} <= set(pc.ODD_WIDTHS) and 0 not in rem and {1, 2, 3} <= set(rem)
    for w in pc.ODD_WIDTHS:
        inputs, _ = pc.odd_width(w)
        assert inputs[8] == w and inputs[0].shape[3] == w and inputs[7] <= 128
    assert max(pc.ODD_WIDTHS) > 256 and max(pc.ODD_WIDTHS) % 256 != 0         # two tiles of the scalar form, the second ragged
    inputs, _ = pc.misaligned()
    assert inputs[8] % 4 == 0
    (fcn, rois5, prob, logit, cls, S, C, H, W), _ = pc.kept_256()
    keep, _ = oops.mask_removal(rois5[:, 1:], prob, logit, cls, (H, W), want_energy=False)
    assert len(prob) == 256 and len(keep) == 256 and len(np.unique(cls)) > 1
    assert [s for _, _, s in pc.UP_TINY].count(160) == 1 and {(h, w) for h, w, _ in pc.UP_TINY} == {(1, 1), (2, 3), (3, 70)}


def test_exact_ties_holds_every_kind_of_tie():
    (fcn, rois5, prob, logit, cls, S, C, H, W), _ = pc.exact_ties()
    s_stuff = S - (C - 1)
    keep, energy = oops.mask_removal(rois5[:, 1:], prob, logit, cls, (H, W), want_energy=True)
    assert len(keep) >= 2
    _, seg_inst = oops.seg_term(cls[keep], fcn, rois5[keep] * np.float32(4.0), S, C)
    inst = seg_inst[0] + energy[0]
    stuff = fcn[0, :s_stuff]
    best = stuff.max(0)
    stuff_ties = ((stuff == best).sum(0) >= 2) & (best > inst.max(0))
    assert stuff_ties.sum() >= 50
    assert (stuff_ties & (stuff[0] == best)).sum() >= 50 and (stuff_ties & (stuff[0] != best)).sum() >= 50
    zero_planes = (best < 0) & (((inst == 0) & (seg_inst[0] == 0)).sum(0) >= 2) & (inst.max(0) == 0)
    no_void = zero_planes & (fcn[0, s_stuff:].max(0) < 0)          # (elsewhere a positive thing logit makes the pixel void)
    assert zero_planes.sum() >= 50 and no_void.sum() >= 50
    inst_equals_stuff = (inst == best).any(0) & (inst.max(0) == best)
    assert inst_equals_stuff.sum() >= 50
    for void in (True, False):
        pan = oops.panoptic_head(fcn, rois5, prob, logit, cls, S, C, enable_void=void)['panoptic']
        assert (pan[stuff_ties & (stuff[0] == best)] == 0).all()              # first maximum
        assert (pan[no_void] == s_stuff).all()                                # the first of the all-zero planes
        assert np.isin(pan[zero_planes], [s_stuff, 255] if void else [s_stuff]).all()
        assert (pan[inst_equals_stuff] < s_stuff).all()                       # stuff comes first


@pytest.mark.parametrize('spec', pc.REMOVAL_CASES, ids=[pc.case_id(s) for s in pc.REMOVAL_CASES])
def test_oracle_evaluates_every_case_in_a_few_seconds(spec):
    fn, args = spec
    (fcn, rois5, prob, logit, cls, S, C, H, W), tag = fn(*args)
    m = len(prob)
    assert H <= 128 and W <= 260 and m * H * ((W + 63) // 64) * 8 <= 1024 * 64 * 2 * 8
    assert fcn.shape == (1, S, H, W) and rois5.shape == (m, 5) and logit.shape[0] == m and cls.shape == (m,)
    assert all(a.dtype == np.float32 for a in (fcn, rois5, prob, logit)) and cls.dtype == np.int64
    t0 = time.perf_counter()
    keep, _ = oops.mask_removal(rois5[:, 1:], prob, logit, cls, (H, W), want_energy=False)
    if spec in pc.FUSE_CASES:
        ref = oops.panoptic_head(fcn, rois5, prob, logit, cls, S, C, enable_void=True)
        assert np.array_equal(ref['keep_inds'], keep)
    dt = time.perf_counter() - t0
    assert dt < 5.0, "%s: %.1f s" % (tag, dt)
    # the same builder gives the same arrays again
    again, _ = fn(*args)
    assert all(np.array_equal(a, b) for a, b in zip(again[:5], (fcn, rois5, prob, logit, cls)))


def test_fuse_cases_fit_the_fused_kernels():
    assert all(s in pc.REMOVAL_CASES for s in pc.FUSE_CASES)
    for fn, args in pc.FUSE_CASES:
        assert len(fn(*args)[0][2]) <= 256
    for hs, ws, s in pc.UP_TINY:
        (score, rois5, prob, logit, cls, S, C, H, W), _ = pc.up_tiny(hs, ws, s)
        assert score.shape == (1, s, hs, ws) and (H, W) == (4 * hs, 4 * ws) and S == s <= 160
