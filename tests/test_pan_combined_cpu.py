"""CPU: the combined panoptic merge (BaseDataset.get_combined_pan_result, reference upsnet/dataset/base_dataset.py:373-449) -- a
numpy restatement with the pinned rules of DESIGN 4.7, held to the reference's own output (tests/golden/pan_combined.npz) and to
hand-derived cases; the vectorised RLE decode against dataset.coco_eval.rle_from_string; the --pan_combined option."""
import os

import numpy as np
import pytest

from conftest import ROOT

ID_LAST_STUFF, NUM_CLASSES = 10, 9     # Cityscapes: 19 semantic classes, 9 detection classes (background included)


# ------------------------------------------------------------------------------------------------ restatement
def decode_mask(rle):
    from upsnet_amd.dataset.coco_eval import rle_from_string
    h, w = rle['size']
    counts = rle_from_string(rle['counts'])
    return np.repeat(np.arange(len(counts)) % 2, counts).astype(bool).reshape(w, h).T


def encode_mask(mask):
    from upsnet_amd.dataset.rle import rle_to_string
    mask = np.asarray(mask, bool)
    flat = mask.T.reshape(-1).astype(np.int8)
    pos = np.concatenate([[0], np.flatnonzero(np.diff(flat)) + 1, [flat.size]])
    counts = np.diff(pos).tolist()
    if flat.size and flat[0]:
        counts = [0] + counts
    return {'size': [int(mask.shape[0]), int(mask.shape[1])], 'counts': rle_to_string(counts)}


def restate_combined(segs, boxes, masks, id_last_stuff=ID_LAST_STUFF, score_threshold=0.6, fraction_threshold=0.7,
                     stuff_area_limit=4 * 64 * 64):
    """get_combined_pan_result with the pinned rules: stable-reversed order, float(score) < thr skips, zero area skips without an
    instance number, fl32(remain / area) < fraction_threshold compared in double rejects."""
    out = []
    for i, seg in enumerate(segs):
        sem = np.array(seg, dtype=np.int64)
        h, w = sem.shape
        sc, cl, rl = [], [], []
        for c in range(1, len(boxes)):
            b = np.asarray(boxes[c][i])
            if b.size:
                sc.append(b[:, 4].astype(np.float64))
                cl += [c] * b.shape[0]
                rl += list(masks[c][i])
        s = np.concatenate(sc) if sc else np.zeros(0)
        ins_mask = np.zeros((h, w), np.uint8)
        ins_sem = np.zeros((h, w), np.uint8)
        idx = np.zeros(len(boxes), np.int64)
        for k in np.argsort(s, kind='stable')[::-1]:
            if float(s[k]) < score_threshold:
                continue
            m = decode_mask(rl[k])
            area = int(m.sum())
            if area == 0:
                continue
            remain = m & (ins_mask == 0)
            if float(np.float32(remain.sum()) / np.float32(area)) < fraction_threshold:
                continue
            idx[cl[k]] += 1
            ins_mask[remain] = idx[cl[k]]
            ins_sem[remain] = cl[k]
        for v in np.unique(sem):
            if v <= id_last_stuff and (sem == v).sum() < stuff_area_limit:
                sem[sem == v] = 255
        c0 = sem.copy()
        c0[(sem > id_last_stuff) & (ins_mask == 0)] = 255
        c0[ins_mask != 0] = ins_sem[ins_mask != 0].astype(np.int64) + id_last_stuff
        pan = np.zeros((h, w, 3), np.uint8)
        pan[:, :, 0] = c0
        pan[:, :, 1] = ins_mask
        out.append(pan)
    return out


def load_golden():
    """[(segs, boxes, masks, stuff_area_limit, expected)] per scene of the fixture, in the reference's boxes[c][i] layout."""
    g = np.load(os.path.join(ROOT, 'tests', 'golden', 'pan_combined.npz'))
    scenes = []
    for i in range(int(g['num_scenes'])):
        seg, b, cls, rle = g['seg_%d' % i], g['boxes_%d' % i], g['cls_%d' % i], g['rle_%d' % i]
        h, w = seg.shape
        nc = int(g['num_classes'])
        boxes = [[]] + [[b[cls == c]] for c in range(1, nc)]
        masks = [[]] + [[[{'size': [h, w], 'counts': str(r)} for r in rle[cls == c]]] for c in range(1, nc)]
        scenes.append(([seg], boxes, masks, int(g['stuff_area_limit'][i]), g['pan_%d' % i]))
    return scenes


def per_class(h, w, dets, nc=NUM_CLASSES, dtype=np.float32):
    """dets: [(class, score, mask bool [h,w])] -> boxes[c][0], masks[c][0] of one image (classes in list order)."""
    boxes = [[]] + [[np.zeros((0, 5), dtype)] for _ in range(1, nc)]
    masks = [[]] + [[[]] for _ in range(1, nc)]
    for c, s, m in dets:
        boxes[c][0] = np.vstack([boxes[c][0], np.array([[0, 0, w - 1, h - 1, s]], dtype)])
        masks[c][0].append(encode_mask(m))
    return boxes, masks


def rect(h, w, y0, y1, x0, x1):
    m = np.zeros((h, w), bool)
    m[y0:y1, x0:x1] = True
    return m


def hand_cases():
    """name -> (segs, boxes, masks, kwargs, expected list of uint8 [H,W,3]); every expected map is written out by hand."""
    cases = {}
    f32_06 = np.float32(0.6)

    # remain / area = 7 / 10: fl32(0.7) == fl32(7/10) < 0.7 in double -> rejected; 71 / 100 -> accepted
    h, w = 10, 20
    seg = np.full((h, w), 3, np.uint8)
    a = rect(h, w, 0, 3, 0, 1)                       # 3 pixels of column 0
    b = rect(h, w, 0, 10, 0, 1)                      # column 0: 10 pixels, 7 unclaimed -> 7 / 10 rejected
    blk = rect(h, w, 0, 3, 5, 15) & ~rect(h, w, 2, 3, 14, 15)   # 29 pixels
    e = rect(h, w, 0, 10, 5, 15)                     # 100 pixels, 29 claimed -> 71 / 100 accepted
    boxes, masks = per_class(h, w, [(1, 0.95, a), (2, 0.9, b), (3, 0.85, blk), (4, 0.8, e)])
    exp = np.zeros((h, w, 3), np.uint8)
    exp[:, :, 0] = 3
    exp[a, 0], exp[a, 1] = ID_LAST_STUFF + 1, 1
    exp[blk, 0], exp[blk, 1] = ID_LAST_STUFF + 3, 1
    exp[e & ~blk, 0], exp[e & ~blk, 1] = ID_LAST_STUFF + 4, 1
    cases['fraction_7_10_rejected_71_100_accepted'] = ([seg], boxes, masks, dict(stuff_area_limit=1), [exp])

    # the same 7 / 10 quotient at fraction_threshold = fl32(0.7) itself is accepted (in double, fl32(0.7) >= fl32(0.7))
    boxes, masks = per_class(h, w, [(1, 0.95, a), (2, 0.9, b)])
    exp = np.zeros((h, w, 3), np.uint8)
    exp[:, :, 0] = 3
    exp[0:3, 0, 0], exp[0:3, 0, 1] = ID_LAST_STUFF + 1, 1
    exp[3:10, 0, 0], exp[3:10, 0, 1] = ID_LAST_STUFF + 2, 1
    cases['fraction_at_fl32_threshold_accepted'] = ([seg], boxes, masks, dict(stuff_area_limit=1, fraction_threshold=float(np.float32(0.7))),
                                                    [exp])

    # score exactly fl32(0.6) kept; the float32 just below it skipped (float64 boxes: the same values)
    h, w = 8, 8
    seg = np.zeros((h, w), np.uint8)
    below = np.nextafter(f32_06, np.float32(0))
    for dt in (np.float32, np.float64):
        boxes, masks = per_class(h, w, [(1, f32_06, rect(h, w, 0, 4, 0, 4)), (2, below, rect(h, w, 4, 8, 4, 8))], dtype=dt)
        exp = np.zeros((h, w, 3), np.uint8)
        exp[0:4, 0:4, 0], exp[0:4, 0:4, 1] = ID_LAST_STUFF + 1, 1
        cases['score_at_fl32_threshold_%s' % np.dtype(dt).name] = ([seg], boxes, masks, dict(stuff_area_limit=1), [exp])

    # a zero-area mask uses no instance number
    boxes, masks = per_class(h, w, [(5, 0.99, np.zeros((h, w), bool)), (5, 0.9, rect(h, w, 1, 3, 1, 3)), (5, 0.8, rect(h, w, 5, 7, 5, 7))])
    exp = np.zeros((h, w, 3), np.uint8)
    exp[1:3, 1:3, 0], exp[1:3, 1:3, 1] = ID_LAST_STUFF + 5, 1
    exp[5:7, 5:7, 0], exp[5:7, 5:7, 1] = ID_LAST_STUFF + 5, 2
    cases['zero_area_uses_no_number'] = ([seg], boxes, masks, dict(stuff_area_limit=1), [exp])

    # stuff area equal to the limit kept, one pixel less -> 255; thing pixels without an instance -> 255; an instance over stuff
    # overrides it
    h, w = 6, 10
    seg = np.zeros((h, w), np.uint8)
    seg[:, 0:2] = 4                                   # 12 pixels: kept at limit 12
    seg[:, 2:4] = 6
    seg[0, 2] = 7                                     # class 6: 11 pixels -> 255; class 7: 1 pixel -> 255
    seg[:, 4:7] = 13                                  # thing label, 18 pixels
    seg[:, 7:10] = 2                                  # stuff, 18 pixels
    inst = rect(h, w, 0, 3, 5, 9)                     # over thing (cols 5, 6) and stuff (cols 7, 8)
    boxes, masks = per_class(h, w, [(2, 0.7, inst)])
    exp = np.zeros((h, w, 3), np.uint8)
    exp[:, 0:2, 0] = 4
    exp[:, 2:4, 0] = 255
    exp[:, 4:7, 0] = 255
    exp[:, 7:10, 0] = 2
    exp[inst, 0], exp[inst, 1] = ID_LAST_STUFF + 2, 1
    cases['stuff_limit_void_things_override'] = ([seg], boxes, masks, dict(stuff_area_limit=12), [exp])

    # tied scores: the later one in the class concatenation goes first (np.argsort(kind='stable')[::-1])
    h, w = 4, 4
    seg = np.zeros((h, w), np.uint8)
    m = rect(h, w, 0, 2, 0, 4)
    boxes, masks = per_class(h, w, [(1, 0.8, m), (1, 0.8, rect(h, w, 0, 4, 0, 2)), (3, 0.8, m)])
    exp = np.zeros((h, w, 3), np.uint8)
    exp[m, 0], exp[m, 1] = ID_LAST_STUFF + 3, 1       # class 3 first; then class 1's second (4 of 8 left: rejected), first (0 left)
    cases['ties_stable_reversed'] = ([seg], boxes, masks, dict(stuff_area_limit=1), [exp])
    return cases


# ------------------------------------------------------------------------------------------------ tests
def test_golden_replays_against_restatement():
    for segs, boxes, masks, limit, want in load_golden():
        got = restate_combined(segs, boxes, masks, stuff_area_limit=limit)[0]
        assert got.dtype == np.uint8 and np.array_equal(got, want)


@pytest.mark.parametrize('name', sorted(hand_cases()))
def test_hand_derived_cases(name):
    segs, boxes, masks, kw, want = hand_cases()[name]
    got = restate_combined(segs, boxes, masks, **kw)
    for g, e in zip(got, want):
        assert np.array_equal(g, e), (name, g[:, :, 0], e[:, :, 0], g[:, :, 1], e[:, :, 1])


def test_fraction_pins():
    """The two numpy promotions of the reference's quotient test: 1.x compares fl32(7 / 10) with 0.7 in double (reject)."""
    q = np.float32(7) / np.float32(10)
    assert q == np.float32(0.7) and float(q) < 0.7
    q = np.float32(71) / np.float32(100)
    assert not float(q) < 0.7


def test_vectorised_decode_matches_rle_from_string():
    from upsnet_amd.dataset.coco_eval import rle_from_string
    from upsnet_amd.dataset.rle import decode_rle_strings, rle_to_string
    rng = np.random.default_rng(3)
    strings = ['', rle_to_string([5]), rle_to_string([0, 7]), rle_to_string([1, 2, 3])]
    for t in range(200):
        strings.append(rle_to_string(list(rng.integers(0, [3, 100, 100000, 2 ** 30][t % 4], int(rng.integers(0, 40))))))
    _, _, masks, _, _ = load_golden()[0]
    strings += [r['counts'] for c in masks[1:] for r in c[0]]
    counts, off = decode_rle_strings(strings)
    for j, s in enumerate(strings):
        assert counts[off[j]:off[j + 1]].tolist() == rle_from_string(s)
    counts, off = decode_rle_strings([s.encode() for s in strings[:5]])
    assert counts[off[3]:off[4]].tolist() == [1, 2, 3]
    with pytest.raises(ValueError):
        decode_rle_strings(['1' + chr(48 + 0x20)])


def test_cli_option_and_method_exist():
    from upsnet_amd.config.parse_args import parse_args
    from upsnet_amd.dataset.base_dataset import BaseDataset
    assert parse_args('', ['--pan_combined']).pan_combined is True
    assert parse_args('', []).pan_combined is False
    assert callable(getattr(BaseDataset, 'get_combined_pan_result', None))


@pytest.mark.parametrize('head', ['has_rcnn', 'has_mask_head', 'has_fcn_head'])
def test_pan_combined_needs_the_heads(head, tmp_path):
    """Refused with a message before the dataset, the model or any launch."""
    import copy
    from upsnet_amd.config.config import config
    from upsnet_amd.evaluate import main
    saved = copy.deepcopy(dict(config))
    try:
        cfg = tmp_path / 'exp.yaml'
        cfg.write_text('output_path: "%s"\ndataset:\n  dataset: NoSuchDataset\nnetwork:\n  %s: false\n' % (tmp_path, head))
        with pytest.raises(SystemExit, match='--pan_combined .*%s' % head):
            main(['--cfg', str(cfg), '--eval_only', '--pan_combined'])
    finally:
        config.clear()
        config.update(saved)
