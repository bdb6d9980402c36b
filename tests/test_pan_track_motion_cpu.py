"""CPU: the tracking rule with constant-velocity motion prediction as tests/pan_track_motion_ref.py restates it, held to
hand-derived literals; its two equalities with the plain restatement (tests/pan_track_ref.py); the refusals of the option. The device
is held to the restatement by tests/test_pan_track_motion_gpu.py."""
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pan_track_motion_ref as mref   # noqa: E402
import pan_track_ref as ref   # noqa: E402


def run(case):
    """[(map, rows, segments, key, frame index, predicted, motion state)] per frame."""
    frames, kw = case
    trk = mref.RefMotionTracker(**kw)
    res = []
    for f in frames:
        out, rows, segs = trk.update(f)
        res.append((out, rows.tolist(), segs) + trk.state() + (trk.predicted(), trk.motion_state()))
    return res


def keys_at(pred, k):
    return sorted(zip(*[a.tolist() for a in np.nonzero(pred == k)]))


def test_accelerating_object_keeps_one_identity():
    """3 x 40, a 4-pixel-wide object at x = 0, 1, 4, 7, 10, thr 0.3, age 0. Frame 1: in place, I 9, U 15, cx 1 -> 2: v = 1. Frame 2:
    predicted at 2..5 against 4..7: I 2 x 3 = 6, U 18 (in place: I 3, U 21 < 0.3); cx 5: v = 3. From then on the prediction is exact."""
    r = run(mref.case_accelerating())
    assert [x[1] for x in r] == [[[1, 1, 1, 0, 0, 12, 12, 0]], [[1, 1, 1, 1, 9, 15, 12, 0]], [[1, 1, 1, 1, 6, 18, 12, 0]],
                                 [[1, 1, 1, 1, 12, 12, 12, 0]], [[1, 1, 1, 1, 12, 12, 12, 0]]]
    assert [[s['track_id'] for s in x[2]] for x in r] == [[1]] * 5
    assert [x[6][(1, 1)] for x in r] == [(1, 1, 0, 0), (2, 1, 1, 0), (5, 1, 3, 0), (8, 1, 3, 0), (11, 1, 3, 0)]
    assert np.array_equal(r[2][5], np.where(np.isin(np.arange(40), [2, 3, 4, 5])[None, :].repeat(3, 0), 257, -1))
    # the memory stays the last seen mask, in place
    assert np.array_equal(r[2][3], np.where(np.isin(np.arange(40), [4, 5, 6, 7])[None, :].repeat(3, 0), 257, -1))
    plain = ref.track_sequence(mref.case_accelerating()[0], **mref.case_accelerating()[1])
    assert [[s['track_id'] for s in x[2]] for x in plain] == [[1], [1], [2], [3], [4]]


def test_hidden_moving_object_is_reacquired():
    """x = 0, 2, 4, hidden, hidden, 10, 12 with max_age 2: at frame 5 the track (last seen at frame 2, columns 4..7, v = 2) is predicted
    at 4 + 2 * 3 = 10..13: I = U = 12, and v = (11 - 5) / 3 = 2."""
    r = run(mref.case_hidden_moving())
    assert r[5][1] == [[1, 1, 1, 1, 12, 12, 12, 0]] and r[5][6] == {(1, 1): (11, 1, 2, 0)}
    assert r[3][1] == r[4][1] == [] and r[4][6] == {(1, 1): (5, 1, 2, 0)}          # unassigned: centroid and velocity are kept
    assert [[s['track_id'] for s in x[2]] for x in r] == [[1], [1], [1], [], [], [1], [1]]
    assert keys_at(r[4][5], 257) == [(y, x) for y in range(3) for x in (8, 9, 10, 11)]
    plain = ref.track_sequence(*[mref.case_hidden_moving()[0]], **mref.case_hidden_moving()[1])
    assert [s['track_id'] for s in plain[5][2]] == [2]


def test_crossing_objects_keep_their_identities():
    r = run(mref.case_crossing())
    serial_at = [{(s['category'], s['instance_in']): s['track_id'] for s in x[2]} for x in r]
    # the object moving left is instance 1 while it is the right one of the two (frames 0..5), then instance 2
    assert [d[(1, 1 if t < 6 else 2)] for t, d in enumerate(serial_at)] == [1] * 8
    assert [d[(1, 2 if t < 6 else 1)] for t, d in enumerate(serial_at)] == [2] * 8
    assert max(max(d.values()) for d in serial_at) == 2
    plain = ref.track_sequence(mref.case_crossing()[0], **mref.case_crossing()[1])
    assert max(s['track_id'] for x in plain for s in x[2]) > 2


def test_vote_conflicts():
    # equal ages: the smaller key takes every contested pixel; the loser is predicted nowhere, yet remembered
    r = run(mref.case_conflict_equal_age())
    assert r[1][6] == {(1, 1): (3, 0, 2, 0), (1, 2): (11, 0, -2, 0)}
    want = np.full((1, 24), -1, np.int32)
    want[0, 6:10] = 257
    assert np.array_equal(r[3][5], want)
    assert r[3][1] == [[1, 1, 1, 1, 4, 4, 4, 0]]
    assert keys_at(r[3][3], 258) == [(0, 10), (0, 11), (0, 12), (0, 13)] and r[3][6][(1, 2)] == (11, 0, -2, 0)
    # the younger track wins, though its key is the larger
    r = run(mref.case_conflict_younger())
    want = np.full((1, 24), -1, np.int32)
    want[0, 8:12] = 258
    assert np.array_equal(r[4][5], want)
    assert r[4][1] == [[1, 1, 2, 1, 4, 4, 4, 0]] and r[4][6] == {(1, 2): (9, 0, -2, 0)}


def test_a_track_predicted_off_the_image_stays_live():
    r = run(mref.case_off_image_wrap())
    bar = 2 << 8 | 1
    assert r[0][1][0] == [2, 1, 1, 0, 0, 4, 4, 0] and [x[2] for x in r[0][1]] == list(range(1, 255))
    assert r[1][1] == [[2, 1, 1, 1, 2, 6, 4, 0]] and r[1][6][(2, 1)] == (1, 0, -2, 0)
    assert keys_at(r[2][5], bar) == [(0, 0), (0, 1)] and r[2][1] == [[2, 1, 255, 0, 0, 1, 1, 0]]       # columns -2..1; the cursor wraps
    # frame 3: predicted nowhere, remembered at columns 0..3 (last written by frame 1); id 1 is skipped
    assert keys_at(r[3][5], bar) == [] and keys_at(r[2][3], bar) == [(0, 0), (0, 1), (0, 2), (0, 3)]
    assert int(r[2][4][0, 0]) == 1 and (2, 1) in r[2][6]
    assert r[3][1] == [[2, 1, 2, 0, 0, 1, 1, 0]]
    assert keys_at(r[3][3], bar) == [] and (2, 1) not in r[3][6]                                        # max_age 1 has run out
    assert [s['track_id'] for s in r[3][2]] == [256]


def test_velocity_truncates_toward_zero():
    r = run(mref.case_truncation())
    assert r[1][6] == {(1, 1): (19, 0, -3, 0)}
    assert keys_at(r[3][5], 257) == [(0, x) for x in range(11, 17)]
    assert r[3][1] == [[1, 1, 1, 1, 5, 7, 6, 0]] and r[3][6] == {(1, 1): (14, 0, -2, 0)}


def same_as_plain(frames, kw):
    a, b = mref.RefMotionTracker(**kw), ref.RefTracker(**kw)
    for t, f in enumerate(frames):
        (ao, ar, asg), (bo, br, bsg) = a.update(f), b.update(f)
        assert np.array_equal(ao, bo) and np.array_equal(ar, br) and asg == bsg, t
        assert all(np.array_equal(x, y) for x, y in zip(a.state(), b.state())), t
    return a


def test_static_scene_equals_the_plain_rule():
    """Nothing moves (objects appear, hide and come back in place): every velocity stays zero, the predicted memory is the real one."""
    rng = np.random.default_rng(5)
    boxes = [(int(rng.choice([1, 2])), 12 * (k // 4) + int(rng.integers(0, 4)), 13 * (k % 4) + int(rng.integers(0, 4)),
              int(rng.integers(2, 9)), int(rng.integers(2, 9))) for k in range(12)]      # one per 12 x 13 cell: none hides another
    frames = []
    for t in range(8):
        f = ref.blank(37, 53)
        count = {}
        for b in rng.permutation(12):
            c, y, x, h, w = boxes[b]
            if rng.random() < 0.25:
                continue
            count[c] = count.get(c, 0) + 1
            ref.put(f, c, count[c], y, min(y + h, 37) - 1, x, min(x + w, 53) - 1)
        frames.append(f)
    trk = same_as_plain(frames, dict(iou_thresh=0.3, max_age=2))
    assert all(v[2:] == (0, 0) for v in trk.motion_state().values())


@pytest.mark.parametrize('seed', [1, 2, 3])
def test_first_two_frames_equal_the_plain_rule(seed):
    frames = ref.blob_sequence(seed, 37, 53, 20, 2, [1, 2, 11])
    same_as_plain(frames, dict(iou_thresh=0.3, max_age=1))


def test_generator_moves_at_constant_velocity():
    frames = mref.velocity_sequence(3, 96, 160, 10, 16, [11, 12], blink=0.15)
    assert len(frames) == 16 and all(f.shape == (96, 160, 3) and f.dtype == np.uint8 for f in frames)
    a = mref.track_sequence(frames, iou_thresh=0.3, max_age=2)
    b = ref.track_sequence(frames, iou_thresh=0.3, max_age=2)
    serials = [max([s['track_id'] for x in r for s in x[2]]) for r in (a, b)]
    assert serials[0] < serials[1]          # fewer identities for the same objects


# ------------------------------------------------------------------------------------------------ the option's refusals
def test_tracker_refuses_an_unknown_motion():
    from upsnet_amd.dataset.pan_track import PanopticTracker, check_params
    for bad in ('kalman', None, '', 'Constant_Velocity', 1):
        with pytest.raises(ValueError):
            PanopticTracker(motion=bad)
        with pytest.raises(ValueError):
            check_params(0.3, 0, bad)
    check_params(0.3, 0)
    for good in ('none', 'constant_velocity'):
        assert PanopticTracker(motion=good).motion == good
    assert PanopticTracker().motion == 'none'
    with pytest.raises(RuntimeError):
        PanopticTracker().predicted()
    with pytest.raises(RuntimeError):
        PanopticTracker(motion='constant_velocity').motion_state()       # no frame yet


@pytest.fixture()
def saved_config():
    import copy
    from upsnet_amd.config.config import config
    saved = copy.deepcopy(dict(config))
    yield config
    config.clear()
    config.update(saved)


def test_command_refuses_a_bad_track_motion(tmp_path, saved_config, capsys):
    from PIL import Image
    from test_dataset_run_cpu import write_cfg
    from upsnet_amd import sequence
    cfg = write_cfg(tmp_path, 'Cityscapes', str(tmp_path / 'data'), 'val')
    cats = tmp_path / 'cats.json'
    cats.write_text(json.dumps({'categories': [{'id': 0, 'name': 'road', 'isthing': 0}]}))
    os.makedirs(tmp_path / 'frames')
    Image.fromarray(np.zeros((2, 3, 3), np.uint8)).save(str(tmp_path / 'frames' / 'f0.png'))
    base = ['--cfg', cfg, '--out', str(tmp_path / 'out'), '--panoptic_categories', str(cats)]
    for mode in (['--track_only', str(tmp_path / 'frames')], ['--frames', str(tmp_path / 'frames'), '--synthetic_weights']):
        with pytest.raises(SystemExit):
            sequence.main(base + mode + ['--track_motion', 'kalman'])
        assert '--track_motion' in capsys.readouterr().err
        assert not os.path.exists(tmp_path / 'out')            # refused before anything ran
    args = sequence.parse_args(base + ['--track_only', str(tmp_path / 'frames')])
    assert args.track_motion == 'none'
    args = sequence.parse_args(base + ['--track_only', str(tmp_path / 'frames'), '--track_motion', 'constant_velocity'])
    assert args.track_motion == 'constant_velocity'
