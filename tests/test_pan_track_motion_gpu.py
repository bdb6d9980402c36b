"""GPU: panoptic tracking with constant-velocity motion prediction (csrc/pan_track.hip, dataset/pan_track.py).
PanopticTracker(motion='constant_velocity') against the plain numpy restatement of the rule (tests/pan_track_motion_ref.py), bit for
bit and frame by frame: output map, row table, memory key and frame index, predicted memory and motion state; on poisoned and
guard-banded memory (tests/memguard.py, patterns A and B). Then motion='none' against the plain restatement, the workspace contract,
the refusals, reset() and the sequence command."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import memguard       # noqa: E402
import pan_track_motion_ref as mref   # noqa: E402
import pan_track_ref as ref   # noqa: E402

pytestmark = pytest.mark.gpu

GUARDED = memguard.MODULES + ('upsnet_amd.dataset.pan_track', 'upsnet_amd.dataset.pan_format', 'upsnet_amd.dataset.pan_vis')
MOTION = 'constant_velocity'


def device_run(frames, kw, pattern=None, unaligned=False, motion=MOTION):
    """[(map, rows, segments, key, frame index, predicted, motion state)] per frame from a fresh PanopticTracker; with a pattern, on
    poisoned allocations and banded inputs. unaligned: the input starts one byte into its buffer."""
    from upsnet_amd.dataset.pan_track import PanopticTracker

    def run():
        trk = PanopticTracker(motion=motion, **kw)
        res = []
        for f in frames:
            t = torch.from_numpy(f).cuda()
            if pattern is not None:
                t = memguard.banded_copy(t, pattern)
            if unaligned:
                flat = torch.empty((t.numel() + 1,), dtype=torch.uint8, device='cuda')
                if pattern is not None:
                    flat = memguard.banded_copy(flat.fill_(memguard.poison_byte(torch.uint8, pattern)), pattern)
                flat[1:].copy_(t.reshape(-1))
                t = flat[1:].view(t.shape)
            out, segs = trk.update(t)
            extra = (trk.predicted(), trk.motion_state()) if motion != 'none' else (None, None)
            res.append((out.cpu().numpy(), segs.rows.copy(), list(segs)) + trk.state() + extra)
        torch.cuda.synchronize()
        return res
    if pattern is None:
        return run()
    with memguard.poisoned(pattern, modules=GUARDED):
        return run()


def reference_run(frames, kw):
    trk = mref.RefMotionTracker(**kw)
    want = []
    for f in frames:
        want.append(trk.update(f) + trk.state() + (trk.predicted(), trk.motion_state()))
    return want


def compare(got, want):
    assert len(got) == len(want)
    for t, (g, w) in enumerate(zip(got, want)):
        assert g[0].dtype == np.uint8 and np.array_equal(g[0], w[0]), 'frame %d: output map' % t
        assert g[1].dtype == np.int32 and np.array_equal(g[1], w[1]), 'frame %d: rows\n%s\n%s' % (t, g[1][:8], w[1][:8])
        assert g[2] == w[2], 'frame %d: segments' % t
        assert g[3].dtype == np.int32 and np.array_equal(g[3], w[3]), 'frame %d: memory key' % t
        assert g[4].dtype == np.int32 and np.array_equal(g[4], w[4]), 'frame %d: memory frame index' % t
        assert g[5].dtype == np.int32 and g[5].shape == w[5].shape and np.array_equal(g[5], w[5]), 'frame %d: predicted memory' % t
        assert g[6] == w[6], 'frame %d: motion state' % t


def check_against_ref(frames, kw, patterns='AB', unaligned=False):
    want = reference_run(frames, kw)
    runs = [device_run(frames, kw, p, unaligned=unaligned) for p in patterns]
    for got in runs:
        compare(got, want)
    return runs[0]


# ------------------------------------------------------------------------------------------------ the hand-derived cases
def test_accelerating_object_keeps_one_identity():
    got = check_against_ref(*mref.case_accelerating())
    assert [[s['track_id'] for s in g[2]] for g in got] == [[1]] * 5
    assert got[2][1].tolist() == [[1, 1, 1, 1, 6, 18, 12, 0]]
    assert [g[6][(1, 1)] for g in got] == [(1, 1, 0, 0), (2, 1, 1, 0), (5, 1, 3, 0), (8, 1, 3, 0), (11, 1, 3, 0)]


def test_hidden_moving_object_is_reacquired():
    got = check_against_ref(*mref.case_hidden_moving())
    assert got[5][1].tolist() == [[1, 1, 1, 1, 12, 12, 12, 0]] and got[5][6] == {(1, 1): (11, 1, 2, 0)}
    assert [[s['track_id'] for s in g[2]] for g in got] == [[1], [1], [1], [], [], [1], [1]]


def test_crossing_objects_keep_their_identities():
    got = check_against_ref(*mref.case_crossing())
    assert max(s['track_id'] for g in got for s in g[2]) == 2


@pytest.mark.parametrize('name', ['conflict_equal_age', 'conflict_younger', 'off_image_wrap', 'truncation'])
def test_hand_cases_equal_the_restatement(name):
    got = check_against_ref(*getattr(mref, 'case_' + name)())
    if name == 'conflict_younger':
        assert got[4][1].tolist() == [[1, 1, 2, 1, 4, 4, 4, 0]]
    if name == 'off_image_wrap':
        assert got[2][1].tolist() == [[2, 1, 255, 0, 0, 1, 1, 0]] and got[3][1].tolist() == [[2, 1, 2, 0, 0, 1, 1, 0]]
        assert (2, 1) in got[2][6] and not (got[3][5] == (2 << 8 | 1)).any()
    if name == 'truncation':
        assert got[3][6] == {(1, 1): (14, 0, -2, 0)}


# ------------------------------------------------------------------------------------------------ shapes, counts, thresholds, ages
@pytest.mark.parametrize('H,W', [(1, 1), (1, 67), (37, 53), (64, 64), (128, 256)])
def test_velocity_sequences_equal_the_restatement(H, W):
    """20 rectangles of three categories at fixed velocities of up to 3 pixels per frame with blink-outs over 10 frames; every
    threshold with every age."""
    for thr in (1.0 / 16.0, 0.3, 1.0):
        for age in (0, 1, 3):
            frames = mref.velocity_sequence(100 * H + W + age, H, W, 20, 10, [1, 2, 11], side=max(2, min(H, W) // 3))
            check_against_ref(frames, dict(iou_thresh=thr, max_age=age), patterns='AB' if thr == 0.3 else ('A' if age else 'B'))


def sliding_dominoes(H, W, n, frames, seed, speed=1):
    """n instances of category 6 as 1 x 3 bars on a grid, the whole pattern sliding `speed` pixels per frame to the left (so the
    leftmost columns are predicted off the image), numbered in a fresh random order per frame; one in eight blinks out for a frame."""
    rng = np.random.default_rng(seed)
    cols = W // 4
    assert n <= cols * (H // 2)
    out = []
    for t in range(frames):
        f = ref.blank(H, W)
        num = 0
        for k in rng.permutation(n):
            y, x = 2 * (k // cols), 4 * (k % cols) + 3 - speed * t
            if rng.random() < 0.125 or x + 2 < 0:
                continue
            num += 1
            ref.put(f, 6, num, y, y, max(x, 0), x + 2)
        out.append(f)
    return out


@pytest.mark.parametrize('age', [0, 3])
def test_255_of_one_category(age):
    """255 tracks of one category sliding: after two frames every id has been issued, the blink-outs and the bars that leave on the
    left make the cursor wrap while tracks are remembered that are predicted (partly or wholly) off the image."""
    frames = sliding_dominoes(40, 52, 255, 7, 3)
    assert len(np.unique(frames[0][:, :, 1])) > 200
    got = check_against_ref(frames, dict(iou_thresh=1.0 / 16.0, max_age=age))
    assert got[1][1][:, 3].sum() > 100 and got[4][1][:, 3].sum() > 100
    if age:       # some remembered track is predicted nowhere: live by the real memory alone
        assert any(len(set(np.unique(g[3]).tolist()) - set(np.unique(g[5]).tolist())) > 0 for g in got[2:])


def test_81_categories_at_once():
    frames = mref.velocity_sequence(5, 64, 64, 162, 4, list(range(81)), side=6, stuff=(200, 254))
    assert len(np.unique(frames[0][:, :, 0][frames[0][:, :, 1] > 0])) > 60
    check_against_ref(frames, dict(iou_thresh=0.3, max_age=1))


def test_unaligned_input_takes_the_byte_paths():
    frames = mref.velocity_sequence(41, 37, 53, 20, 5, [1, 2, 11])
    check_against_ref(frames, dict(iou_thresh=0.3, max_age=1), unaligned=True)


def test_full_size_sequence():
    """1024 x 2048, four frames, 30 rectangles of up to 400 pixels a side at up to 6 pixels per frame: the vector paths of every pass
    and more than one workgroup. (No sum of x over a segment of a 1024 x 2048 map can reach 2^32: the whole map sums to 1024 x 2048 x
    2047 / 2 < 2^31. test_sums_beyond_32_bits has the shapes where they do.)"""
    frames = mref.velocity_sequence(11, 1024, 2048, 30, 4, [11, 12, 13, 14], vmax=6, side=400, blink=0.1)
    check_against_ref(frames, dict(iou_thresh=0.3, max_age=1), patterns='A')


@pytest.mark.parametrize('tall', [False, True])
def test_sums_beyond_32_bits(tall):
    """One row (or one column) of 2^17 pixels with a segment over all but its first 1000 + 3 t: sum x (or sum y) is about 8.6 x 10^9
    > 2^32, the centroid about 66 000; it moves by 1.5 per frame (the start by 3, the end stays), so its floor by 2, then by 1."""
    n = 1 << 17
    frames = []
    for t in range(3):
        f = ref.blank(n, 1) if tall else ref.blank(1, n)
        f.reshape(-1, 3)[1000 + 3 * t:] = (3, 1, 0)
        frames.append(f)
    assert sum(range(1000, n)) > 1 << 32
    got = check_against_ref(frames, dict(iou_thresh=0.3, max_age=0), patterns='A')
    c = [(1000 + 3 * t + n - 1) // 2 for t in range(3)]          # floor of the mean of first and last
    v = [0, c[1] - c[0], c[2] - c[1]]
    assert c == [66035, 66037, 66038]
    assert [g[6][(3, 1)] for g in got] == [(0, c[t], 0, v[t]) if tall else (c[t], 0, v[t], 0) for t in range(3)]


# ------------------------------------------------------------------------------------------------ the default, workspace, reset
def test_motion_none_is_the_plain_tracker():
    frames = ref.blob_sequence(37 * 100 + 53, 37, 53, 20, 8, [1, 2, 11])
    kw = dict(iou_thresh=0.3, max_age=1)
    trk = ref.RefTracker(**kw)
    want = [trk.update(f) + trk.state() for f in frames]
    for p in 'AB':
        got = device_run(frames, kw, p, motion='none')
        for t, (g, w) in enumerate(zip(got, want)):
            assert np.array_equal(g[0], w[0]) and np.array_equal(g[1], w[1]) and g[2] == w[2], t
            assert np.array_equal(g[3], w[3]) and np.array_equal(g[4], w[4]), t
    from upsnet_amd.dataset.pan_track import PanopticTracker
    plain = PanopticTracker(**kw)
    plain.update(frames[0])
    assert plain.motion == 'none' and plain._mws is None        # no motion buffers unless asked for
    with pytest.raises(RuntimeError):
        plain.predicted()
    with pytest.raises(RuntimeError):
        plain.motion_state()


def test_zero_velocities_equal_the_plain_step():
    """The first two frames of a random walk: every velocity is zero while they are matched, and the device's motion step gives what
    its plain step gives."""
    frames = ref.blob_sequence(9, 64, 64, 20, 2, [1, 2, 11])
    kw = dict(iou_thresh=0.3, max_age=1)
    a, b = device_run(frames, kw), device_run(frames, kw, motion='none')
    for g, w in zip(a, b):
        assert np.array_equal(g[0], w[0]) and np.array_equal(g[1], w[1]) and g[2] == w[2]
        assert np.array_equal(g[3], w[3]) and np.array_equal(g[4], w[4])


def test_workspaces_are_zero_again_after_a_step():
    from upsnet_amd._lib import lib
    from upsnet_amd.dataset.pan_track import PanopticTracker
    frames = mref.velocity_sequence(21, 64, 64, 20, 6, [1, 2])
    trk = PanopticTracker(iou_thresh=0.3, max_age=1, motion=MOTION)
    off = int(lib().upsnet_pan_track_stamp_offset())
    lo, hi = int(lib().upsnet_pan_track_motion_count_offset()), int(lib().upsnet_pan_track_motion_pred_offset())
    assert 0 < lo < hi and hi + 4 * 64 * 64 == int(lib().upsnet_pan_track_motion_workspace_bytes(64, 64))
    for f in frames:
        trk.update(torch.from_numpy(f).cuda())
        assert int(torch.count_nonzero(trk._ws[:off])) == 0, 'count cells / segment counters left non-zero'
        assert int(torch.count_nonzero(trk._mws[lo:hi])) == 0, 'motion count cells left non-zero'
    assert int(torch.count_nonzero(trk._mws[:lo])) > 0              # (the motion state itself is kept)
    assert int(lib().upsnet_pan_track_motion_workspace_bytes(0, 5)) == 0
    assert int(lib().upsnet_pan_track_motion_workspace_bytes(4097, 4096)) == 0


def test_refusals_of_the_step():
    from upsnet_amd import ops
    H, W = 6, 8
    frames, kw = ref.case_three_frames()
    pan = torch.from_numpy(frames[0]).cuda()
    ws = torch.zeros((int(ops.lib().upsnet_pan_track_workspace_bytes(H, W)),), dtype=torch.uint8, device='cuda')
    mws = torch.zeros((int(ops.lib().upsnet_pan_track_motion_workspace_bytes(H, W)) + 16,), dtype=torch.uint8, device='cuda')
    mem = torch.zeros((H, W), dtype=torch.int16, device='cuda')
    out = torch.zeros((H, W, 3), dtype=torch.uint8, device='cuda')
    with pytest.raises(ValueError):
        ops.pan_track_step_motion(pan, 0.3, 0, 0, ws, mem, out, mws[1:])              # misaligned
    with pytest.raises(ValueError):
        ops.pan_track_step_motion(pan, 0.3, 0, 0, ws, mem, out, mws[:64])             # too small
    with pytest.raises(ValueError):
        ops.pan_track_step_motion(pan, 0.3, 0, 0, ws, mem, out, mws.view(torch.int16))
    with pytest.raises(RuntimeError):
        ops.pan_track_step_motion(pan, 0.01, 0, 0, ws, mem, out, mws)                # the plain step's refusals stand
    args = (None, pan.data_ptr(), H, W, 0.3, 0, 0, ws.data_ptr(), mem.data_ptr(), out.data_ptr(), None, 0)
    assert ops.lib().upsnet_pan_track_step_motion(*(args + (None,))) != 0           # the library itself: null, misaligned
    assert ops.lib().upsnet_pan_track_step_motion(*(args + (mws.data_ptr() + 4,))) != 0
    torch.cuda.synchronize()
    assert int(torch.count_nonzero(mem)) == 0 and int(torch.count_nonzero(mws)) == 0 and int(torch.count_nonzero(ws)) == 0
    assert ops.pan_track_step_motion(pan, 0.3, 0, 0, ws, mem, out, mws[:-16]) is out
    assert np.array_equal(out.cpu().numpy(), frames[0])


def test_reset_gives_a_fresh_tracker():
    from upsnet_amd.dataset.pan_track import PanopticTracker, track_sequence
    a = mref.velocity_sequence(31, 37, 53, 12, 4, [1, 2])
    b = mref.velocity_sequence(32, 37, 53, 12, 5, [1, 2])
    kw = dict(iou_thresh=0.3, max_age=3)
    trk = PanopticTracker(motion=MOTION, **kw)
    for f in a:
        trk.update(f)
    trk.reset(serials=True)
    with pytest.raises(RuntimeError):
        trk.predicted()
    got = []
    for f in b:
        out, segs = trk.update(f)
        got.append((out.cpu().numpy(), segs.rows.copy(), list(segs)) + trk.state() + (trk.predicted(), trk.motion_state()))
    compare(got, reference_run(b, kw))
    res = track_sequence(b, motion=MOTION, **kw)                 # the option passes through
    assert all(np.array_equal(o.cpu().numpy(), g[0]) and list(s) == g[2] for (o, s), g in zip(res, got))


# ------------------------------------------------------------------------------------------------ the command
@pytest.fixture()
def saved_config():
    import copy
    from upsnet_amd.config.config import config
    saved = copy.deepcopy(dict(config))
    yield config
    config.clear()
    config.update(saved)


def test_sequence_command_with_track_motion(tmp_path, saved_config):
    from PIL import Image
    from test_dataset_run_cpu import write_cfg
    from upsnet_amd import sequence
    frames, kw = mref.case_hidden_moving()
    raw = tmp_path / 'raw' / 'seq'
    os.makedirs(raw)
    names = ['f_%06d.png' % (5 * k) for k in range(len(frames))]
    for n, f in zip(names, frames):
        Image.fromarray(f).save(str(raw / n))
    cfg = write_cfg(tmp_path, 'Cityscapes', str(tmp_path / 'data'), 'val')
    cats = str(tmp_path / 'cats.json')
    with open(cats, 'w') as f:
        json.dump({'categories': [{'id': c, 'name': 'c%d' % c, 'isthing': int(c > 0)} for c in range(19)]}, f)
    base = ['--cfg', cfg, '--track_only', str(tmp_path / 'raw'), '--panoptic_categories', cats, '--track_max_age', '2']
    res = sequence.main(base + ['--out', str(tmp_path / 'out'), '--track_motion', 'constant_velocity'])
    want = mref.track_sequence(frames, **kw)
    for n, (w_map, _, _) in zip(names, want):
        assert np.array_equal(np.array(Image.open(str(tmp_path / 'out' / 'seq' / 'pan_2ch' / n))), w_map), n
    tracks = json.load(open(str(tmp_path / 'out' / 'seq' / 'tracks.json')))['tracks']
    assert [t['track_id'] for t in tracks] == [1] and tracks[0]['frames'] == [names[k] for k in (0, 1, 2, 5, 6)]
    assert len(res['sequences'][0][3]) == 1
    plain = sequence.main(base + ['--out', str(tmp_path / 'out_plain')])            # the default: the object comes back as another track
    assert [t['track_id'] for t in plain['sequences'][0][3]] == [1, 2]
