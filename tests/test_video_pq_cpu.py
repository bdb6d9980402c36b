"""CPU: the video metrics' rule and host logic. The plain numpy restatement (tests/video_pq_ref.py) on hand-derived
cases, each with its arithmetic; the evaluator's refusals that need no device; the arguments of both commands; the folder pairing of
the re-scoring command."""
import json
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import video_pq_ref as ref   # noqa: E402


def run(case):
    preds, gts, infos, windows = case
    ev = ref.RefVideoEvaluator(ref.CATEGORIES, windows)
    ev.add_sequence(preds, gts, infos)
    return ev


def counts(ev, n, cat):
    return ev.tp[n].get(cat, 0), ev.fp[n].get(cat, 0), ev.fn[n].get(cat, 0), ev.iou[n].get(cat, 0.0)


# ------------------------------------------------------------------------------------------------ hand-derived cases
def test_perfect_prediction():
    """GT = prediction in 4 frames (stuff 200, things (1,1) and (2,5)): in every window every row meets its own key with inter = area_p
    = area_g, iou = 1; 5 - n windows of length n, so tp = 5 - n per category, PQ_n = 1. Every GT track has G = P = I: (1 / G) * I * (I / G)
    = 1 each, AQ = 2 / 2; the confusion matrix is diagonal, iou = 1; STQ = sqrt(1 * 1)."""
    ev = run(ref.case_perfect())
    for n in (1, 2, 3, 4):
        for cat in (200, 1, 2):
            assert counts(ev, n, cat) == (5 - n, 0, 0, float(5 - n))
        assert ev.pq(n) == (1.0, 1.0, 1.0, 3)
    assert ev.vpq() == 1.0 and ev.vpq(True) == 1.0 and ev.vpq(False) == 1.0
    assert ev.stq() == {'stq': 1.0, 'aq': 1.0, 'iou': 1.0, 'num_tracks': 2}


@pytest.mark.parametrize('S', [6, 7])
def test_identity_switch(S):
    """One GT thing of S pixels in each of 4 frames; the prediction covers it exactly with key (1,1) in frames 0-1 and (1,2) in 2-3.
    n = 1: 4 windows, iou = S / (S + S - S) = 1 each: tp 4, PQ 1.
    n = 2: [0,1] and [2,3]: one key of 2S on a row of 2S, iou 1 -> tp 2, iou_sum 2; [1,2]: row 2S, each key S with inter S: iou = S /
           (S + 2S - S) = 1/2, not > 0.5 -> fn 1, fp 2. PQ = 2 / (2 + 2/2 + 1/2) = 4/7.
    n = 3: [0,1,2]: row 3S; key (1,1) 2S: iou = 2S / (2S + 3S - 2S) = 2/3 -> tp; key (1,2) S: fp. [1,2,3] mirrored. tp 2, fp 2, fn 0,
           iou_sum 4/3, PQ = (4/3) / (2 + 1) = 4/9.
    n = 4: row 4S, each key 2S: iou = 2S / (2S + 4S - 2S) = 1/2 -> tp 0, fn 1, fp 2, PQ 0.
    STQ: G = 4S, each key P = I = 2S: I * I / (G + P - I) = 2S * (2S / 4S) = S; AQ = (1 / 4S) * 2S = 1/2; iou = 1; STQ = sqrt(1/2)."""
    ev = run(ref.case_identity_switch(S))
    assert counts(ev, 1, 1) == (4, 0, 0, 4.0)
    assert counts(ev, 2, 1) == (2, 2, 1, 2.0)
    tp, fp, fn, iou = counts(ev, 3, 1)
    assert (tp, fp, fn) == (2, 2, 0) and iou == 2.0 * S / (3.0 * S) + 2.0 * S / (3.0 * S)
    assert counts(ev, 4, 1) == (0, 2, 1, 0.0)
    assert ev.pq(1)[0] == 1.0 and ev.pq(2)[0] == 2.0 / 3.5 and ev.pq(4)[0] == 0.0
    assert abs(ev.pq(3)[0] - 4.0 / 9.0) < 1e-15
    assert abs(ev.vpq() - (1.0 + 4.0 / 7.0 + 4.0 / 9.0) / 4.0) < 1e-15
    s = ev.stq()
    assert s['aq'] == 0.5 and s['iou'] == 1.0 and s['num_tracks'] == 1 and s['stq'] == math.sqrt(0.5)


def test_iou_exactly_half_is_not_matched():
    """GT 4 pixels, pred 2 of them: iou = 2 / (2 + 4 - 2) = 0.5, and the rule is `>`: fn 1, and the key (no ignored pixel) is an fp."""
    ev = run(ref.case_iou_half())
    assert counts(ev, 1, 1) == (0, 1, 1, 0.0)


def test_fp_skip_threshold():
    """A pred tube of 4 pixels on stuff GT of another category: with 2 of them on VOID ign / area = 2/4 is not > 0.5 -> fp; with 3,
    3/4 > 0.5 -> skipped. The stuff row is unmatched either way: fn[200] = 1."""
    ev = run(ref.case_fp_skip(2))
    assert counts(ev, 1, 1) == (0, 1, 0, 0.0) and counts(ev, 1, 200) == (0, 0, 1, 0.0)
    ev = run(ref.case_fp_skip(3))
    assert counts(ev, 1, 1) == (0, 0, 0, 0.0) and counts(ev, 1, 200) == (0, 0, 1, 0.0)


def test_crowd_exemption():
    """Crowd thing id 3 (4 pixels), GT track id 4 (2 pixels), pred tube (1,1) over all 6. VPQ: row 4: iou = 2 / (6 + 2 - 2) = 1/3 -> fn 1;
    the crowd row is no fn; the key: ign = 0 + 4 (crowd), 4/6 > 0.5 -> no fp. STQ: one GT track; P = 6 - 4 = 2 (the crowd pixels leave
    it), G = I = 2: (1/2) * 2 * (2 / (2 + 2 - 2)) = 1 (it would be 1/3 with P = 6). conf[1][1] = 6: iou 1."""
    ev = run(ref.case_crowd())
    assert counts(ev, 1, 1) == (0, 0, 1, 0.0)
    assert ev.stq() == {'stq': 1.0, 'aq': 1.0, 'iou': 1.0, 'num_tracks': 1}
    assert ev.conf[1, 1] == 6 and ev.conf.sum() == 6


def test_cross_category_overlap():
    """GT track of category 1 covered exactly by a pred track of category 2. VPQ counts no inter: fn[1] = 1, fp[2] = 1. AQ: G = P = I = 4
    -> 1. Semantic: conf[1][2] = 4, IoU_1 = 0 / 4 and IoU_2 = 0 / 4 -> iou 0, STQ 0."""
    ev = run(ref.case_cross_category())
    assert counts(ev, 1, 1) == (0, 0, 1, 0.0) and counts(ev, 1, 2) == (0, 1, 0, 0.0)
    assert ev.stq() == {'stq': 0.0, 'aq': 1.0, 'iou': 0.0, 'num_tracks': 1}
    assert ev.conf[1, 2] == 4 and ev.conf.sum() == 4


def test_short_sequence_adds_nothing_to_a_longer_window():
    ev = run(ref.case_short())
    assert counts(ev, 1, 1) == (2, 0, 0, 2.0)
    assert ev.tp[3] == {} and ev.fp[3] == {} and ev.fn[3] == {} and ev.pq(3) == (0.0, 0.0, 0.0, 0)


def test_blob_sequence_has_what_it_promises():
    preds, gts, infos = ref.blob_sequence(3, 37, 53, 6, switch_at=3)
    ev = ref.RefVideoEvaluator(ref.CATEGORIES)
    ev.add_sequence(preds, gts, infos)
    cells = ev.seq_cells[0]
    assert any(r < 0 and k >= 0 for r, k in cells) and any(k < 0 and r >= 0 for r, k in cells)      # GT VOID and pred VOID
    assert any(s['iscrowd'] for segs in infos for s in segs)
    table = ref.sequence_table(infos)
    assert any(r >= 0 and k >= 0 and table[r][1] != k >> 8 for r, k in cells)                      # cross-category overlap
    assert 0 < ev.vpq() < 1 and 0 < ev.stq()['stq'] < 1
    assert sum(ev.tp[1].values()) > 0 and sum(ev.fp[4].values()) > 0 and sum(ev.fn[4].values()) > 0


# ------------------------------------------------------------------------------------------------ refusals that need no device
def test_sequence_table_refusals():
    from upsnet_amd.dataset.video_pq import sequence_rows
    s = ref.seg
    rows = sequence_rows([[s(9, 1), s(3, 200)], [s(3, 200), s(5, 2, 1)]], 4096)
    assert rows.tolist() == [[3, 200, 0], [5, 2, 1], [9, 1, 0]]
    for frames, text in (([[s(3, 1)], [s(3, 2)]], 'one object'), ([[s(3, 1)], [s(3, 1, 1)]], 'one object'), ([[s(0, 1)]], 'id 0'),
                         ([[s(3, 1), s(3, 1)]], 'duplicate'), ([[s(3, 255)]], 'category'), ([[s(3, -1)]], 'category'),
                         ([[s(1 << 24, 1)]], 'outside'), ([[s(1, 1), s(2, 1)], [s(3, 1)]], 'max_gt_segments')):
        with pytest.raises(ValueError, match=text):
            sequence_rows(frames, 2)


def test_evaluator_refusals_without_a_device():
    from upsnet_amd.dataset.video_pq import VideoPanopticEvaluator
    for windows in ((), (0,), (9,), (2, 1), (1, 1), (1.5,), 3):
        with pytest.raises(ValueError, match='windows'):
            VideoPanopticEvaluator(ref.CATEGORIES, windows=windows)
    with pytest.raises(ValueError, match='category ids'):
        VideoPanopticEvaluator({255: {'isthing': 1}})
    with pytest.raises(ValueError, match='max_gt_segments'):
        VideoPanopticEvaluator(ref.CATEGORIES, max_gt_segments=4097)
    ev = VideoPanopticEvaluator(ref.CATEGORIES)
    frame = np.zeros((4, 4, 3), np.uint8)
    with pytest.raises(ValueError, match='outside a sequence'):
        ev.add_frame(frame, frame)
    with pytest.raises(ValueError, match='outside a sequence'):
        ev.end_sequence()
    with pytest.raises(ValueError, match='duplicate'):
        ev.begin_sequence([[ref.seg(3, 1), ref.seg(3, 1)]])
    with pytest.raises(ValueError, match='outside a sequence'):     # the refused sequence did not begin
        ev.add_frame(frame, frame)
    ev.begin_sequence([[ref.seg(3, 1)]])
    with pytest.raises(ValueError, match='inside a sequence'):
        ev.begin_sequence([[ref.seg(3, 1)]])
    for bad in (frame.astype(np.int32), frame[:, :, :2], frame[0]):
        with pytest.raises(ValueError, match='uint8'):
            ev.add_frame(bad, frame)
        with pytest.raises(ValueError):
            ev.add_frame(frame, bad)
    with pytest.raises(ValueError, match='differ in shape'):
        ev.add_frame(frame, np.zeros((4, 5, 3), np.uint8))
    big = np.broadcast_to(np.zeros((1, 1, 3), np.uint8), (4097, 4096, 3))
    with pytest.raises(ValueError, match='2\\^24'):
        ev.add_frame(big, big)
    assert ev._state is None and ev._ws is None and ev._seq.frames == 0 and ev.num_frames == 0      # nothing reached the device


# ------------------------------------------------------------------------------------------------ the commands' arguments and pairing
def test_parse_args_of_both_commands(capsys):
    from upsnet_amd import sequence, video_eval
    a = sequence.parse_args(['--cfg', 'x.yaml', '--track_only', 'p', '--out', 'o', '--video_gt', 'g'])
    assert a.video_gt == 'g' and a.vpq_windows == (1, 2, 3, 4)
    a = sequence.parse_args(['--cfg', 'x.yaml', '--video_gt', 'g', '--vpq_windows', '1', '3'])
    assert a.vpq_windows == (1, 3)
    a = sequence.parse_args(['--cfg', 'x.yaml'])
    assert a.video_gt == '' and a.track_iou == 0.3 and a.track_max_age == 0
    b = video_eval.parse_args(['--pred', 'p', '--video_gt', 'g', '--panoptic_categories', 'c.json', '--vpq_windows', '2'])
    assert (b.pred, b.video_gt, b.panoptic_categories, b.vpq_windows, b.out) == ('p', 'g', 'c.json', (2,), '')
    for parse in (sequence.parse_args, video_eval.parse_args):
        with pytest.raises(SystemExit):
            parse(['--vpq_windows', '1', '2'])
        assert 'needs --video_gt' in capsys.readouterr().err
        for bad in (['3', '1'], ['0'], ['9'], ['2', '2']):
            with pytest.raises(SystemExit):
                parse(['--video_gt', 'g', '--vpq_windows'] + bad)
            assert 'ascending' in capsys.readouterr().err


def test_rescoring_command_refusals(tmp_path):
    from upsnet_amd import video_eval
    cats = str(tmp_path / 'cats.json')
    with open(cats, 'w') as f:
        json.dump({'categories': list(ref.CATEGORIES.values())}, f)
    with pytest.raises(SystemExit, match='--pred'):
        video_eval.main(['--video_gt', str(tmp_path), '--panoptic_categories', cats])
    with pytest.raises(SystemExit, match='--video_gt'):
        video_eval.main(['--pred', str(tmp_path), '--panoptic_categories', cats])
    with pytest.raises(SystemExit, match='--panoptic_categories'):
        video_eval.main(['--pred', str(tmp_path), '--video_gt', str(tmp_path)])
    with pytest.raises(SystemExit, match='no sequence folder'):
        video_eval.main(['--pred', str(tmp_path), '--video_gt', str(tmp_path), '--panoptic_categories', cats])


def test_folder_pairing(tmp_path):
    from PIL import Image
    from upsnet_amd import video_eval
    pred_names = ['f_%06d.png' % k for k in range(0, 30, 5)]
    anns = [{'file_name': 'f_%06d_leftImg8bit.png' % k, 'segments_info': []} for k in (20, 0, 10)]
    pairs = video_eval.pair_frames('s', pred_names, anns)
    assert [(k, a['file_name']) for k, a in pairs] == [(0, 'f_000000_leftImg8bit.png'), (2, 'f_000010_leftImg8bit.png'),
                                                       (4, 'f_000020_leftImg8bit.png')]     # a subset, in the prediction's order
    with pytest.raises(SystemExit, match='f_000030.png, which was not predicted'):
        video_eval.pair_frames('s', pred_names, anns + [{'file_name': 'f_000030.png', 'segments_info': []}])
    with pytest.raises(SystemExit, match='twice'):
        video_eval.pair_frames('s', pred_names, anns + [{'file_name': 'f_000010.png', 'segments_info': []}])
    # the folders: pan_2ch/ marks a sequence of the prediction; gt.json goes before pred.json; what is missing is named
    root, gt = tmp_path / 'pred', tmp_path / 'gt'
    for name in ('b', 'a'):
        os.makedirs(str(root / name / 'pan_2ch'))
        for f in pred_names[:2]:
            Image.fromarray(np.zeros((2, 2, 3), np.uint8)).save(str(root / name / 'pan_2ch' / f))
    os.makedirs(str(root / 'not_a_sequence'))
    (root / 'video_scores.json').write_text('{}')
    found = video_eval.discover_predictions(str(root))
    assert [(n, [os.path.basename(p) for p in ps]) for n, ps in found] == [('a', pred_names[:2]), ('b', pred_names[:2])]
    with pytest.raises(SystemExit, match='no ground truth of sequence a'):
        video_eval.load_video_gt(str(gt), 'a')
    os.makedirs(str(gt / 'a'))
    with pytest.raises(SystemExit, match='neither gt.json nor pred.json'):
        video_eval.load_video_gt(str(gt), 'a')
    (gt / 'a' / 'pred.json').write_text(json.dumps({'annotations': [{'file_name': 'p.png', 'segments_info': []}]}))
    with pytest.raises(SystemExit, match='no folder of panoptic PNGs'):
        video_eval.load_video_gt(str(gt), 'a')
    os.makedirs(str(gt / 'a' / 'pan'))
    assert video_eval.load_video_gt(str(gt), 'a')[0][0]['file_name'] == 'p.png'
    (gt / 'a' / 'gt.json').write_text(json.dumps({'annotations': [{'file_name': 'g.png', 'segments_info': []}]}))
    anns, pan = video_eval.load_video_gt(str(gt), 'a')
    assert anns[0]['file_name'] == 'g.png' and pan == str(gt / 'a' / 'pan')
    with pytest.raises(SystemExit, match='no PNG at'):
        video_eval.load_png(os.path.join(pan, 'g.png'))
