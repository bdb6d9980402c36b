"""CPU: the tracking rule as tests/pan_track_ref.py restates it, held to hand-derived cases; the host statements of
the frame-stable colours; the frame discovery and the refusals of the sequence command. The device is held to the restatement by
tests/test_pan_track_gpu.py."""
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pan_track_ref as ref   # noqa: E402


def run(case):
    frames, kw = case
    trk = ref.RefTracker(**kw)
    res = []
    for f in frames:
        out, rows, segs = trk.update(f)
        res.append((out, rows.tolist(), segs) + trk.state())
    return res


def key_map(H, W, *boxes):
    """int32 [H,W] of -1 with (c, j, y0, y1, x0, x1) boxes of c << 8 | j."""
    k = np.full((H, W), -1, np.int32)
    for c, j, y0, y1, x0, x1 in boxes:
        k[y0:y1 + 1, x0:x1 + 1] = c << 8 | j
    return k


def test_three_frame_example():
    r = run(ref.case_three_frames())
    frames, _ = ref.case_three_frames()
    # frame 0: nothing remembered, ids from the cursors: (3,1) -> 1, (3,2) -> 2; the map is unchanged
    assert np.array_equal(r[0][0], frames[0])
    assert r[0][1] == [[3, 1, 1, 0, 0, 8, 8, 0], [3, 2, 2, 0, 0, 12, 12, 0]]
    assert np.array_equal(r[0][3], key_map(6, 8, (3, 1, 0, 1, 0, 3), (3, 2, 3, 5, 4, 7)))
    assert np.array_equal(r[0][4], np.where(r[0][3] >= 0, 0, -1))
    # frame 1: detection 1 is the lower object (I 9, U 12 + 12 - 9 = 15), detection 2 the upper one (I 6, U 8 + 8 - 6 = 10): the
    # numbers swap back; category 5 starts its own cursor
    want = ref.blank(6, 8)
    ref.put(want, 7, 0, 2, 2, 0, 7)
    ref.put(want, 3, 2, 3, 5, 3, 6)
    ref.put(want, 3, 1, 0, 1, 1, 4)
    ref.put(want, 5, 1, 5, 5, 0, 1)
    assert np.array_equal(r[1][0], want)
    assert r[1][1] == [[3, 1, 2, 1, 9, 15, 12, 0], [3, 2, 1, 1, 6, 10, 8, 0], [5, 1, 1, 0, 0, 2, 2, 0]]
    assert np.array_equal(r[1][3], key_map(6, 8, (3, 2, 3, 5, 3, 6), (3, 1, 0, 1, 1, 4), (5, 1, 5, 5, 0, 1)))
    assert np.array_equal(r[1][4], np.where(r[1][3] >= 0, 1, -1))
    # frame 2: the lower object again (I 9, U 15); a new object far from track 1 gets id 3 (cursor 2; 1 and 2 are live); with
    # max_age 0 the memory is exactly frame 2's tracked things: tracks (3,1) and (5,1) are gone
    want = ref.blank(6, 8)
    ref.put(want, 7, 0, 2, 2, 0, 7)
    ref.put(want, 3, 2, 3, 5, 2, 5)
    ref.put(want, 3, 3, 0, 0, 6, 7)
    assert np.array_equal(r[2][0], want)
    assert r[2][1] == [[3, 1, 2, 1, 9, 15, 12, 0], [3, 2, 3, 0, 0, 2, 2, 0]]
    assert np.array_equal(r[2][3], key_map(6, 8, (3, 2, 3, 5, 2, 5), (3, 3, 0, 0, 6, 7)))
    assert np.array_equal(r[2][4], np.where(r[2][3] >= 0, 2, -1))
    # serials: inherited on a match, fresh for a new track
    assert [[s['track_id'] for s in x[2]] for x in r] == [[1, 2], [2, 1, 3], [2, 4]]
    assert [s['iou'] for s in r[1][2]] == [9 / 15, 6 / 10, 0.0]
    assert r[1][2][0] == {'category': 3, 'instance_in': 1, 'instance': 2, 'track_id': 2, 'matched': True, 'iou': 0.6, 'area': 12}


def test_contested_greedy():
    """Tracks 1 (cols 0-5), 2 (6-11), 3 (12-25). Segment a = cols 3-21 overlaps all three: I / U = 3/22, 6/19, 10/23; segment b = cols
    22-27 overlaps track 3: 4/16. At 1/8 all four are candidates; order 10/23 > 6/19 > 4/16 > 3/22: a takes 3, (a,2) and (a,1) fall to
    a being taken, (b,3) to track 3 being taken, b is new: id 4 (cursor 3). At 0.6 nothing is a candidate: a -> 4, b -> 5."""
    assert 10 / 23 > 6 / 19 > 4 / 16 > 3 / 22 >= 1 / 8
    r = run(ref.case_contested(0.125))
    assert r[1][1] == [[1, 1, 3, 1, 10, 23, 19, 0], [1, 2, 4, 0, 0, 6, 6, 0]]
    assert np.array_equal(r[1][3], key_map(1, 40, (1, 3, 0, 0, 3, 21), (1, 4, 0, 0, 22, 27)))
    r = run(ref.case_contested(0.6))
    assert r[1][1] == [[1, 1, 4, 0, 0, 19, 19, 0], [1, 2, 5, 0, 0, 6, 6, 0]]


def test_exact_tie_goes_by_i_then_j():
    """Segment 1 meets tracks 1 and 2 with I / U = 2/10 each, segment 2 meets track 2 with 1/5: three exactly equal ratios with
    different terms. (1,1) < (1,2) < (2,2): 1 -> 1, then (1,2) falls, then 2 -> 2. Any other order of the ties leaves a segment new."""
    r = run(ref.case_tie())
    assert r[1][1] == [[1, 1, 1, 1, 2, 10, 8, 0], [1, 2, 2, 1, 1, 5, 2, 0]]


@pytest.mark.parametrize('thr,rows_eq,rows_short', [(0.5, [1, 1, 1, 1, 2, 4, 2, 0], [1, 1, 2, 0, 0, 2, 2, 0]),
                                                     (0.25, [1, 1, 1, 1, 2, 8, 4, 0], [1, 1, 2, 0, 0, 4, 4, 0])])
def test_threshold_equality(thr, rows_eq, rows_short):
    """I = thr * U exactly is accepted (>=); with one pixel of intersection less (I, U = 1, 5 and 1, 9) it is refused."""
    assert run(ref.case_equality(thr, False))[1][1] == [rows_eq]
    assert run(ref.case_equality(thr, True))[1][1] == [rows_short]


def test_max_age():
    r = run(ref.case_hidden(1))
    # frame 1: stuff over the object; the entries of frame 0 are one frame old and stay
    assert r[1][1] == [] and np.array_equal(r[1][0], ref.case_hidden(1)[0][1])
    assert np.array_equal(r[1][3], key_map(1, 12, (1, 1, 0, 0, 0, 3))) and r[1][4][0, :5].tolist() == [0, 0, 0, 0, -1]
    # frame 2: re-acquired from its last mask (I 3, U 5); its stale pixel (column 0) is cleared because the track lives elsewhere now
    assert r[2][1] == [[1, 1, 1, 1, 3, 5, 4, 0]] and r[2][2][0]['track_id'] == 1
    assert np.array_equal(r[2][3], key_map(1, 12, (1, 1, 0, 0, 1, 4))) and r[2][4][0, :6].tolist() == [-1, 2, 2, 2, 2, -1]
    r = run(ref.case_hidden(0))
    assert (r[1][3] == -1).all() and (r[1][4] == -1).all()
    assert r[2][1] == [[1, 1, 2, 0, 0, 4, 4, 0]] and r[2][2][0]['track_id'] == 2      # re-issued as new
    # not matched and too old: cleared after max_age frames without the track being seen
    frames, _ = ref.case_hidden(1)
    trk = ref.RefTracker(0.3, 1)
    for f in (frames[0], frames[1], frames[1]):
        trk.update(f)
    assert (trk.state()[0] == -1).all()


def test_cursor_wraps_and_skips_live_ids():
    r = run(ref.case_wrap())
    assert [row[2] for row in r[0][1]] == list(range(1, 255))
    assert [row[2:4] for row in r[1][1]] == [[1, 1], [3, 1]]
    # cursor 254: id 255, then 1 is live, 2 is free, 3 is live, 4 and 5 are free
    assert [row[2:4] for row in r[2][1]] == [[1, 1], [3, 1], [255, 0], [2, 0], [4, 0], [5, 0]]
    assert [row[7] for row in r[2][1]] == [0] * 6


def test_take_over():
    r = run(ref.case_takeover())
    rows = r[1][1]
    assert len(rows) == 255
    assert [row[2:4] for row in rows[:254]] == [[j, 1] for j in range(2, 256)]      # instance i sits on track i + 1's old pixel
    assert rows[254] == [4, 255, 1, 0, 0, 1, 1, 1]                                   # the one new segment takes over id 1
    key, frame = r[1][3], r[1][4]
    assert key[0, 0] == -1 and frame[0, 0] == -1                                     # the taken-over track's old pixel is cleared
    assert key.reshape(-1)[255] == (4 << 8 | 1) and (frame.reshape(-1)[1:] == 1).all()
    assert [s['track_id'] for s in r[1][2]] == list(range(2, 256)) + [256]           # a taken-over id is a new track
    r = run(ref.case_takeover_all())
    assert [row[2:4] + row[7:] for row in r[1][1]] == [[j, 0, 1] for j in range(1, 256)]
    assert (r[1][3].reshape(-1)[:256] == -1).all()
    # frame 2: tracks 1 and 45 are matched; the new segment finds all 255 ids live and takes the smallest unmatched one, 2
    assert r[2][1] == [[4, 1, 2, 0, 0, 1, 1, 1], [4, 2, 1, 1, 1, 1, 1, 0], [4, 3, 45, 1, 1, 1, 1, 0]]


def test_serials():
    frames, kw = ref.case_hidden(0)
    trk = ref.RefTracker(**kw)
    seen = []
    for f in frames + frames:
        seen.append([s['track_id'] for s in trk.update(f)[2]])
    assert seen == [[1], [], [2], [2], [], [3]]      # frame 3 matches frame 2's mask (I 3, U 5); every re-issue is a fresh serial
    r = run(ref.case_wrap())
    assert [s['track_id'] for s in r[2][2]] == [1, 3, 255, 256, 257, 258]     # id 2 is recycled, its serial is not


def test_parameter_ranges():
    for thr in (0.0624, 1.0001, float('nan'), 0.0):
        with pytest.raises(ValueError):
            ref.RefTracker(iou_thresh=thr)
    with pytest.raises(ValueError):
        ref.RefTracker(max_age=-1)
    ref.RefTracker(iou_thresh=1.0 / 16.0)
    ref.RefTracker(iou_thresh=1.0, max_age=7)
    from upsnet_amd.dataset.pan_track import check_params
    for thr in (0.0624, 1.0001, float('nan')):
        with pytest.raises(ValueError):
            check_params(thr, 0)
    with pytest.raises(ValueError):
        check_params(0.3, -1)
    trk = ref.RefTracker()
    trk.update(ref.blank(2, 3))
    with pytest.raises(ValueError):
        trk.update(ref.blank(3, 2))


CATEGORIES = [{'id': 0, 'name': 'road', 'isthing': 0, 'color': [128, 64, 128]}, {'id': 2, 'name': 'person', 'isthing': 1, 'color': [220, 20, 60]},
              {'id': 4, 'name': 'dark', 'isthing': 1, 'color': [0, 0, 0]}, {'id': 5, 'name': 'white', 'isthing': 1, 'color': [255, 255, 255]},
              {'id': 254, 'name': 'last', 'isthing': 1}]


def test_stable_colours_are_a_pure_nonzero_function():
    from upsnet_amd.dataset import pan_format as pf
    cats = pf.category_dict(CATEGORIES)
    seen = {}
    for c in (2, 4, 5, 254):
        base = pf.category_color(c, cats[c])
        for i in range(0, 256):
            col = pf.stable_color(c, i, cats[c])
            assert col == list(ref.stable_picture_colour(c, i, base, 1))       # the product's host statement = the restatement
            assert tuple(col) != (0, 0, 0) and all(abs(a - b) <= 30 for a, b in zip(col, base))
            seen[(c, i)] = col
    assert all(pf.stable_color(c, i, cats[c]) == col for (c, i), col in seen.items())     # no state between calls
    assert pf.stable_color(0, 0, cats[0]) == [128, 64, 128] and pf.stable_color(0, 7, cats[0]) == [128, 64, 128]   # stuff
    # attempt 0 of (4, i) around black is black whenever all three offsets are <= 0: a later attempt is taken then
    assert any(pf.color_attempt((0, 0, 0), 4, i, 0) == (0, 0, 0) for i in range(256))
    assert len(set(map(tuple, (seen[(2, i)] for i in range(1, 256))))) > 200            # instances of a class mostly differ


def test_png_ids_are_unique_within_an_image():
    from upsnet_amd.dataset import pan_format as pf
    ids = {}
    for c in range(255):
        for i in range(256):
            r, g, b = pf.stable_id_color(c, i)
            assert [r, g, b] == list(ref.stable_png_colour(c, i)) and b == 1
            ids[r + 256 * g + 65536 * b] = (c, i)
    assert len(ids) == 255 * 256 and 0 not in ids
    assert pf.stable_id_color(255, 3) == [0, 0, 0]
    f = ref.case_three_frames()[0][1]
    png = ref.stable_png(f)
    assert np.array_equal(png[0, 1], [3, 2, 1]) and np.array_equal(png[2, 0], [7, 0, 1]) and np.array_equal(png[5, 7], [0, 0, 0])


# ------------------------------------------------------------------------------------------------ the sequence command
def _touch(path):
    from PIL import Image
    os.makedirs(os.path.dirname(path), exist_ok=True)
    Image.fromarray(np.zeros((2, 3, 3), np.uint8)).save(path)


def test_frame_discovery(tmp_path):
    from upsnet_amd.sequence import discover_sequences
    root = tmp_path / 'demo'
    for name in ('b_000002.png', 'b_000010.png', 'a_000001.jpg', 'notes.txt'):
        if name.endswith('.txt'):
            os.makedirs(root, exist_ok=True)
            (root / name).write_text('x')
        else:
            _touch(str(root / name))
    for sub, names in (('seq_b', ('f2.png', 'f1.png')), ('seq_a', ('x.PNG',))):
        for name in names:
            _touch(str(root / sub / name))
    got = discover_sequences(str(root))
    assert [n for n, _ in got] == ['demo', 'seq_a', 'seq_b']                      # the folder's own frames first, then subfolders by name
    assert [os.path.basename(p) for p in got[0][1]] == ['a_000001.jpg', 'b_000002.png', 'b_000010.png']     # by name; no text file
    assert [os.path.basename(p) for p in got[2][1]] == ['f1.png', 'f2.png']
    with pytest.raises(SystemExit) as e:
        discover_sequences(str(tmp_path / 'nowhere'))
    assert 'nowhere' in str(e.value)
    os.makedirs(root / 'seq_empty')
    with pytest.raises(SystemExit) as e:
        discover_sequences(str(root))
    assert 'seq_empty' in str(e.value)
    os.makedirs(tmp_path / 'hollow')
    with pytest.raises(SystemExit) as e:
        discover_sequences(str(tmp_path / 'hollow'), '--track_only')
    assert 'hollow' in str(e.value) and '--track_only' in str(e.value)


@pytest.fixture()
def saved_config():
    import copy
    from upsnet_amd.config.config import config
    saved = copy.deepcopy(dict(config))
    yield config
    config.clear()
    config.update(saved)


def test_command_refusals(tmp_path, saved_config, monkeypatch):
    from test_dataset_run_cpu import write_cfg
    from upsnet_amd import sequence
    cfg = write_cfg(tmp_path, 'Cityscapes', str(tmp_path / 'data'), 'val')
    cats = tmp_path / 'cats.json'
    cats.write_text(json.dumps({'categories': [{'id': 0, 'name': 'road', 'isthing': 0}]}))
    frames = tmp_path / 'frames'
    _touch(str(frames / 'f0.png'))
    base = ['--cfg', cfg, '--out', str(tmp_path / 'out'), '--panoptic_categories', str(cats)]

    def refused(argv, *words):
        with pytest.raises(SystemExit) as e:
            sequence.main(argv)
        for w in words:
            assert w in str(e.value), (w, str(e.value))
    refused(['--frames', str(frames), '--synthetic_weights'], '--cfg')
    refused(base, '--frames', '--track_only')
    refused(base + ['--frames', str(frames), '--track_only', str(frames)], '--frames', '--track_only')
    refused(base[:4] + ['--frames', str(frames), '--synthetic_weights'], '--panoptic_categories')
    refused(base + ['--frames', str(frames)], '--weight_path', '--synthetic_weights')
    refused(base + ['--frames', str(frames), '--synthetic_weights', '--track_iou', '0.05'], '--track_iou', '1/16')
    refused(base + ['--frames', str(frames), '--synthetic_weights', '--track_max_age', '-1'], '--track_max_age')
    refused(base + ['--frames', str(tmp_path / 'missing'), '--synthetic_weights'], 'missing')
    refused(base + ['--track_only', str(frames), '--vis_panoptic', 'overlay'], 'flat')
    refused(base + ['--track_only', str(frames), '--combined'], '--track_only')
    no_pan = write_cfg(tmp_path, 'Cityscapes', str(tmp_path / 'data'), 'val', name='no_pan.yaml')
    with open(no_pan, 'a') as f:
        f.write('\n')
    saved_config.network.has_panoptic_head = True
    text = open(no_pan).read().replace('  has_rpn: true', '  has_rpn: true\n  has_panoptic_head: false\n  has_mask_head: false')
    open(no_pan, 'w').write(text)
    refused(['--cfg', no_pan] + base[2:] + ['--frames', str(frames), '--synthetic_weights'], 'has_panoptic_head')
    refused(['--cfg', no_pan] + base[2:] + ['--frames', str(frames), '--synthetic_weights', '--combined'], 'has_mask_head')
    monkeypatch.setenv('WORLD_SIZE', '2')
    refused(base + ['--frames', str(frames), '--synthetic_weights'], 'one rank')
