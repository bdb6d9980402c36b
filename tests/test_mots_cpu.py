"""CPU: the MOTS measures. The plain numpy restatement of the rule (tests/mots_ref.py) against hand-worked cases whose
counts are written out here; the evaluator's refusals, raised before the device is touched; the commands' options; the text format."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mots_ref as ref   # noqa: E402


def run(case, categories=ref.CATEGORIES):
    ev = ref.RefMOTSEvaluator(categories)
    ev.add_sequence(*case)
    return ev


def counts(ev, c):
    return {name: getattr(ev, name).get(c, 0) for name in ref.COUNTS}


def expect(ev, c, **want):
    got = counts(ev, c)
    full = dict.fromkeys(ref.COUNTS, 0)
    full.update(want)
    assert got == full, (c, got, full)


# ------------------------------------------------------------------------------------------------ hand-worked cases
def test_perfect_sequence():
    """Two objects (categories 1 and 2) predicted exactly in 3 frames: 3 matches of IoU 1 each, every figure 1, both mostly tracked."""
    case = ref.strip_case([[(1, 1, 0, 3), (2, 4, 6, 8)]] * 3, [[(7, 0, 3), (8, 6, 8)]] * 3, [ref.seg(7, 1), ref.seg(8, 2)])
    ev = run(case)
    for c in (1, 2):
        expect(ev, c, tp=3, gt_masks=3, mt=1)
        assert ev.soft[c] == 3.0
        assert ev.figures(c) == {'motsa': 1.0, 'smotsa': 1.0, 'motsp': 1.0, 'recall': 1.0, 'precision': 1.0}
    expect(ev, 11)
    assert ev.mean() == {'motsa': 1.0, 'smotsa': 1.0, 'motsp': 1.0, 'recall': 1.0, 'precision': 1.0, 'n': 2}


def test_one_identity_switch():
    """The object is matched in all 4 frames, by key (1, 1) in two and (1, 2) in two: IDS = 1, MOTSA = (4 - 0 - 1) / 4."""
    case = ref.strip_case([[(1, 1, 0, 3)], [(1, 1, 0, 3)], [(1, 2, 0, 3)], [(1, 2, 0, 3)]], [[(7, 0, 3)]] * 4, [ref.seg(7, 1)])
    ev = run(case)
    expect(ev, 1, tp=4, gt_masks=4, ids=1, mt=1)
    assert ev.figures(1)['motsa'] == 0.75 and ev.figures(1)['smotsa'] == 0.75 and ev.figures(1)['motsp'] == 1.0


def test_switch_across_an_absence():
    """Frame 1 holds neither the object nor a hypothesis; in frame 2 it comes back under another key: `last` survives the absence, so
    IDS = 1; the object was never present and unmatched, so Frag = 0; present = tracked = 2."""
    case = ref.strip_case([[(1, 1, 0, 3)], [], [(1, 2, 0, 3)]], [[(7, 0, 3)], [], [(7, 0, 3)]], [[ref.seg(7, 1)], [], [ref.seg(7, 1)]])
    expect(run(case), 1, tp=2, gt_masks=2, ids=1, mt=1)


def test_gap_then_resumption():
    """Matched, present but missed, matched again by the same key: FN = 1, Frag = 1, IDS = 0; tracked 2 of 3 frames is PT."""
    case = ref.strip_case([[(1, 1, 0, 3)], [], [(1, 1, 0, 3)]], [[(7, 0, 3)]] * 3, [ref.seg(7, 1)])
    ev = run(case)
    expect(ev, 1, tp=2, fn=1, gt_masks=3, frag=1, pt=1)
    assert ev.figures(1)['motsa'] == 2.0 / 3 and ev.figures(1)['recall'] == 2.0 / 3


def test_a_miss_before_the_first_match_is_no_fragmentation():
    case = ref.strip_case([[], [(1, 1, 0, 3)]], [[(7, 0, 3)]] * 2, [ref.seg(7, 1)])
    expect(run(case), 1, tp=1, fn=1, gt_masks=2, pt=1)


def test_iou_of_exactly_one_half_is_no_match():
    """GT 4 pixels, prediction 2 of them: I = 2, A_g = 4, A_p = 2, 3 I = 6 = A_g + A_p -> no match: FN and FP. GT 0..2 and prediction
    1..3: I = 2, union 4, again 6 = 6. One more common pixel (prediction 0..2 of GT 0..3): 9 > 7, a match of IoU 3 / 4."""
    expect(run(ref.strip_case([[(1, 1, 0, 1)]], [[(7, 0, 3)]], [ref.seg(7, 1)])), 1, fn=1, fp=1, gt_masks=1, ml=1)
    expect(run(ref.strip_case([[(1, 1, 1, 3)]], [[(7, 0, 2)]], [ref.seg(7, 1)])), 1, fn=1, fp=1, gt_masks=1, ml=1)
    ev = run(ref.strip_case([[(1, 1, 0, 2)]], [[(7, 0, 3)]], [ref.seg(7, 1)]))
    expect(ev, 1, tp=1, gt_masks=1, mt=1)
    assert ev.soft[1] == 0.75 and ev.figures(1)['motsa'] == 1.0 and ev.figures(1)['smotsa'] == 0.75


def test_false_positive_on_void():
    """A hypothesis of 4 pixels, 2 of them on GT VOID: 2 * 2 = 4 is not > 4 -> counted. 3 of them: 6 > 4 -> exempt."""
    expect(run(ref.strip_case([[(1, 1, 0, 3)]], [[(0, 0, 1)]], [])), 1, fp=1)
    expect(run(ref.strip_case([[(1, 1, 0, 3)]], [[(0, 0, 2)]], [])), 1, fp_ignored=1)
    # an id that is in no segments_info is ignored like 0
    expect(run(ref.strip_case([[(1, 1, 0, 3)]], [[(4242, 0, 2)]], [])), 1, fp_ignored=1)


def test_false_positive_on_a_crowd_row_of_its_own_category_only():
    """Two hypotheses of category 1: (1, 1) lies on a crowd row of category 1 -> exempt; (1, 5) lies on a crowd row of category 2 ->
    counted. Crowd rows are no objects: gt_masks = 0 everywhere."""
    case = ref.strip_case([[(1, 1, 0, 3), (1, 5, 6, 9)]], [[(3, 0, 3), (4, 6, 9)]], [ref.seg(3, 1, crowd=1), ref.seg(4, 2, crowd=1)])
    ev = run(case)
    expect(ev, 1, fp=1, fp_ignored=1)
    expect(ev, 2)


def test_cross_category_overlap_is_no_match():
    ev = run(ref.strip_case([[(2, 1, 0, 3)]], [[(6, 0, 3)]], [ref.seg(6, 1)]))
    expect(ev, 1, fn=1, gt_masks=1, ml=1)
    expect(ev, 2, fp=1)


def test_stuff_keys_and_stuff_rows_are_not_scored():
    ev = run(ref.strip_case([[(200, 0, 0, 3), (254, 0, 4, 7)]], [[(6, 4, 7)]], [ref.seg(6, 254)]))
    for c in ref.CATEGORIES:
        expect(ev, c)


def test_coverage_boundaries():
    """Five frames, four objects of category 1, tracked in 5, 4, 1 and 0 of them: 5 * 5 > 4 * 5 MT; 5 * 4 = 4 * 5 is not above 0.8 -> PT;
    5 * 1 = 5 is not below 0.2 -> PT; 0 -> ML. Six frames, tracked 5: 25 > 24 -> MT; tracked 1: 5 < 6 -> ML."""
    gt = [(1, 0, 1), (2, 3, 4), (3, 6, 7), (4, 9, 10)]
    segs = [ref.seg(g, 1) for g in (1, 2, 3, 4)]
    pred = [[(1, 1, 0, 1)] + ([(1, 2, 3, 4)] if t < 4 else []) + ([(1, 3, 6, 7)] if t == 2 else []) for t in range(5)]
    ev = run(ref.strip_case(pred, [gt] * 5, segs))
    expect(ev, 1, tp=10, fn=10, gt_masks=20, mt=1, pt=2, ml=1)
    pred = [([(1, 1, 0, 1)] if t != 3 else []) + ([(1, 2, 3, 4)] if t == 5 else []) for t in range(6)]
    ev = run(ref.strip_case(pred, [gt[:2]] * 6, segs[:2]))
    expect(ev, 1, tp=6, fn=6, gt_masks=12, frag=1, mt=1, ml=1)


def test_unknown_category_raises():
    with pytest.raises(KeyError):
        run(ref.strip_case([[(37, 1, 0, 3)]], [[]], []))


def test_blob_sequences_of_the_gpu_tests_hold_every_event():
    """The seeded sequences that tests/test_mots_gpu.py compares must make every count move in the restatement alone."""
    ev = ref.RefMOTSEvaluator(ref.CATEGORIES)
    for seed, H, W, frames, switch_at in ref.GPU_BLOBS:
        ev.add_sequence(*ref.blob_sequence(seed, H, W, frames, switch_at=switch_at))
    total = {name: sum(getattr(ev, name).values()) for name in ref.COUNTS}
    for name in ('ids', 'frag', 'fp_ignored', 'fp', 'fn', 'tp', 'mt', 'pt', 'ml'):
        assert total[name] >= 1, (name, total)
    assert any(0.0 < v != round(v) for v in ev.soft.values())


# ------------------------------------------------------------------------------------------------ the evaluator's refusals
def test_refusals_before_the_device_is_touched():
    from upsnet_amd.dataset.mots import MOTSEvaluator
    with pytest.raises(ValueError, match='category ids'):
        MOTSEvaluator({300: {'id': 300, 'isthing': 1}})
    with pytest.raises(ValueError, match='max_gt_segments'):
        MOTSEvaluator(ref.CATEGORIES, max_gt_segments=5000)
    ev = MOTSEvaluator(list(ref.CATEGORIES.values()))
    frame = np.zeros((4, 6, 3), np.uint8)
    with pytest.raises(ValueError, match='outside a sequence'):
        ev.add_frame(frame, frame)
    with pytest.raises(ValueError, match='outside a sequence'):
        ev.end_sequence()
    for bad in ([[ref.seg(0, 1)]], [[ref.seg(1 << 24, 1)]], [[ref.seg(3, 1), ref.seg(3, 1)]], [[ref.seg(3, 1)], [ref.seg(3, 2)]],
                [[ref.seg(3, 255)]], [[ref.seg(3, 1, crowd=2)]]):
        with pytest.raises(ValueError):
            ev.begin_sequence(bad)
    with pytest.raises(ValueError, match='more than max_gt_segments'):
        MOTSEvaluator(ref.CATEGORIES, max_gt_segments=1).begin_sequence([[ref.seg(3, 1), ref.seg(4, 1)]])
    ev.begin_sequence([[ref.seg(3, 1)]], name='s')
    with pytest.raises(ValueError, match='inside a sequence'):
        ev.begin_sequence([[ref.seg(3, 1)]])
    for p, g in ((frame[:, :, :2], frame), (frame.astype(np.int16), frame), (frame, frame[:, :5]), (frame[:0], frame[:0])):
        with pytest.raises(ValueError):
            ev.add_frame(p, g)
    ev.end_sequence()                      # a sequence without a scored frame: nothing is launched
    assert ev.num_sequences == 1 and ev.num_frames == 0 and ev.workspace() is None
    raw = ev.raw()
    assert not any(v.any() for v in raw.values()) and raw['soft'].dtype == np.float64
    assert ev.summary()['mean'] == {'smotsa': 0.0, 'motsa': 0.0, 'motsp': 0.0, 'recall': 0.0, 'precision': 0.0, 'n': 0}


# ------------------------------------------------------------------------------------------------ the commands' options
def test_command_line_options(capsys):
    from upsnet_amd import sequence, video_eval
    a = sequence.parse_args(['--cfg', 'x.yaml'])
    assert (a.eval_mots, a.mots_gt, a.write_mots) == (False, '', False)
    a = sequence.parse_args(['--cfg', 'x.yaml', '--video_gt', 'g', '--eval_mots', '--write_mots'])
    assert a.eval_mots and a.write_mots and a.video_gt == 'g'
    b = video_eval.parse_args(['--pred', 'p', '--mots_gt', 'm', '--eval_mots'])
    assert b.mots_gt == 'm' and b.eval_mots and b.video_gt == ''
    for parse in (sequence.parse_args, video_eval.parse_args):
        with pytest.raises(SystemExit):
            parse(['--eval_mots'])
        assert '--eval_mots' in capsys.readouterr().err
        assert parse(['--write_mots']).write_mots


def test_rescoring_command_refusals(tmp_path):
    import json
    from upsnet_amd import video_eval
    cats = str(tmp_path / 'cats.json')
    with open(cats, 'w') as f:
        json.dump({'categories': list(ref.CATEGORIES.values())}, f)
    with pytest.raises(SystemExit, match='--video_gt'):
        video_eval.main(['--pred', str(tmp_path), '--panoptic_categories', cats])
    with pytest.raises(SystemExit, match='no sequence folder'):        # --write_mots alone needs no ground truth and no categories
        video_eval.main(['--pred', str(tmp_path), '--write_mots'])
    with pytest.raises(SystemExit, match='--panoptic_categories'):
        video_eval.main(['--pred', str(tmp_path), '--mots_gt', str(tmp_path)])
    with pytest.raises(SystemExit, match='--mots_gt: no folder'):
        video_eval.main(['--pred', str(tmp_path), '--panoptic_categories', cats, '--mots_gt', str(tmp_path / 'none')])
    assert video_eval.background_category(ref.CATEGORIES) == 0
    assert video_eval.background_category({0: {'isthing': 1}, 1: {'isthing': 1}, 2: {'isthing': 0}}) == 2


# ------------------------------------------------------------------------------------------------ the text format
def test_text_round_trip(tmp_path):
    """The lines write_mots_txt writes, restated from the masks on the host, read back: every thing pixel carries category * 1000 +
    instance, the rest one background segment; a frame index beyond the last line is an empty frame."""
    from upsnet_amd.dataset.mots import read_mots_txt, segment_lines
    from upsnet_amd.dataset.rle import rle_to_string
    maps = [ref.blob_sequence(seed, 13, 17, 3, switch_at=1)[0] for seed in (1, 2)]
    maps = maps[0] + maps[1][:1]
    maps[0][0, 0] = (1, 7, 0)
    maps[0][12, 16] = (1, 7, 0)          # one segment holds the first and the last pixel
    lines = ref.mots_lines(maps, rle_to_string)
    assert len(lines) > 12 and lines[0].split()[0] == '0' and lines[0].split()[3:5] == ['13', '17']
    assert any(line.split()[:3] == ['0', '1007', '1'] for line in lines)
    # the package's own line builder, fed the restated transitions
    for t, m in enumerate(maps):
        words = sorted(k << 24 | p for k, mask in ref.thing_segments(m).items() for p in ref.transitions(mask))
        assert segment_lines(t, words, 13, 17) == [line for line in lines if line.split()[0] == str(t)]
    path = str(tmp_path / 's.txt')
    with open(path, 'w') as f:
        f.write('\n'.join(lines) + '\n')
    gts, infos = read_mots_txt(path, num_frames=len(maps) + 1, background_category=200)
    assert len(gts) == len(infos) == len(maps) + 1
    background = (1 << 24) - 1
    for m, g, info in zip(maps, gts, infos):
        want = np.full(m.shape[:2], background, np.int64)
        for k, mask in ref.thing_segments(m).items():
            want[mask] = (k >> 8) * 1000 + (k & 255)
        assert g.dtype == np.uint8 and g.shape == m.shape and np.array_equal(ref.gt_ids(g), want)
        ids, area = np.unique(want, return_counts=True)
        assert [(s['id'], s['area']) for s in info] == list(zip(ids.tolist(), area.tolist()))
        assert all(s['category_id'] == (s['id'] // 1000 if s['id'] != background else 200) and s['iscrowd'] == 0 for s in info)
    assert np.all(ref.gt_ids(gts[-1]) == background) and [s['id'] for s in infos[-1]] == [background]
    assert len(read_mots_txt(path)[0]) == len(maps)
    # frame by frame: the same maps, one at a time
    from upsnet_amd.dataset.mots import MOTSText
    text = MOTSText(path, num_frames=len(maps) + 1, background_category=200)
    assert (text.height, text.width, text.num_frames, text.background) == (13, 17, len(maps) + 1, background) and text.segments_info == infos
    assert all(np.array_equal(text.frame(t), gts[t]) for t in range(text.num_frames))


def test_reader_paints_class_10_as_void_and_refuses(tmp_path):
    from upsnet_amd.dataset.mots import read_mots_txt
    from upsnet_amd.dataset.rle import rle_to_string

    def line(t, oid, cls, mask):
        return '%d %d %d %d %d %s' % (t, oid, cls, mask.shape[0], mask.shape[1], rle_to_string(ref.rle_counts(mask)))

    def write(lines):
        path = str(tmp_path / 'g.txt')
        with open(path, 'w') as f:
            f.write('\n'.join(lines) + '\n')
        return path
    a, b = np.zeros((3, 5), bool), np.zeros((3, 5), bool)
    a[0:2, 0:2] = True
    b[1:3, 3:5] = True
    top = (1 << 24) - 1
    gts, infos = read_mots_txt(write([line(0, top, 2, a), line(0, 10000, 10, b)]))
    ids = ref.gt_ids(gts[0])
    assert np.all(ids[a] == top) and np.all(ids[b] == 0) and np.all(ids[~a & ~b] == top - 1)      # the background id steps aside
    assert [(s['id'], s['category_id'], s['area']) for s in infos[0]] == [(top - 1, 0, 7), (top, 2, 4)] or \
        [(s['id'], s['category_id'], s['area']) for s in infos[0]] == [(top, 2, 4), (top - 1, 0, 7)]
    c = np.zeros((3, 5), bool)
    c[1, 1:4] = True
    with pytest.raises(ValueError, match='overlaps'):
        read_mots_txt(write([line(0, 1, 1, a), line(0, 2, 1, c)]))
    read_mots_txt(write([line(0, 1, 1, a), line(1, 2, 1, c)]))         # (in different frames they do not)
    with pytest.raises(ValueError, match='size'):
        read_mots_txt(write([line(0, 1, 1, a), line(1, 1, 1, np.zeros((3, 6), bool))]))
    for oid in (0, 1 << 24, -4):
        with pytest.raises(ValueError, match='outside 1..2\\^24-1'):
            read_mots_txt(write([line(0, oid, 1, a)]))
    with pytest.raises(ValueError, match='background_category'):         # the default background category 0 must not be an object's class
        read_mots_txt(write([line(0, 1, 0, a)]))
    with pytest.raises(ValueError, match='background_category'):
        read_mots_txt(write([line(0, 1, 2, a)]), background_category=2)
    with pytest.raises(ValueError, match='frame index'):
        read_mots_txt(write([line(2, 1, 1, a)]), num_frames=2)
    with pytest.raises(ValueError, match='6 fields'):
        read_mots_txt(write(['0 1 1 3 5']))
    with pytest.raises(ValueError, match='add up'):
        read_mots_txt(write(['0 1 1 4 5 ' + rle_to_string(ref.rle_counts(a))]))
    with pytest.raises(ValueError, match='no mask'):
        read_mots_txt(write(['']))
