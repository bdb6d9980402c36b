"""GPU: panoptic tracking across frames (csrc/pan_track.hip, dataset/pan_track.py). PanopticTracker against the plain
numpy restatement of the rule (tests/pan_track_ref.py), bit for bit and frame by frame: output map, row table, memory key and frame
index; on poisoned and guard-banded memory (tests/memguard.py, patterns A and B; the results must not depend on the pattern). Then the
workspace contract, the refusals, reset(), the frame-stable colours of the formatter, and the sequence command."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import memguard       # noqa: E402
import pan_track_ref as ref   # noqa: E402

pytestmark = pytest.mark.gpu

GUARDED = memguard.MODULES + ('upsnet_amd.dataset.pan_track', 'upsnet_amd.dataset.pan_format', 'upsnet_amd.dataset.pan_vis')


def device_run(frames, kw, pattern=None, look=True, unaligned=False):
    """[(map, rows, key, frame index, segments)] per frame from a fresh PanopticTracker; with a pattern, on poisoned allocations and
    banded inputs. look=False reads the tables only after the last update. unaligned: the input starts one byte into its buffer."""
    from upsnet_amd.dataset.pan_track import PanopticTracker

    def run():
        trk = PanopticTracker(**kw)
        res, held = [], []
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
            key, fr = trk.state()
            held.append(segs)
            res.append([out.cpu().numpy(), None, key, fr, None])
            if look:
                res[-1][1], res[-1][4] = segs.rows.copy(), list(segs)
        if not look:
            for r, segs in zip(res, held):
                r[1], r[4] = segs.rows.copy(), list(segs)
        torch.cuda.synchronize()
        return res
    if pattern is None:
        return run()
    with memguard.poisoned(pattern, modules=GUARDED):
        return run()


def check_against_ref(frames, kw, patterns='AB', unaligned=False):
    trk = ref.RefTracker(**kw)
    want = []
    for f in frames:
        want.append(trk.update(f) + trk.state())
    runs = [device_run(frames, kw, p, unaligned=unaligned) for p in patterns]
    for got in runs:
        assert len(got) == len(want)
        for t, ((g_out, g_rows, g_key, g_fr, g_segs), (w_out, w_rows, w_segs, w_key, w_fr)) in enumerate(zip(got, want)):
            assert g_out.dtype == np.uint8 and np.array_equal(g_out, w_out), 'frame %d: output map' % t
            assert g_rows.dtype == np.int32 and np.array_equal(g_rows, w_rows), 'frame %d: rows\n%s\n%s' % (t, g_rows[:8], w_rows[:8])
            assert g_segs == w_segs, 'frame %d: segments' % t
            assert g_key.dtype == np.int32 and np.array_equal(g_key, w_key), 'frame %d: memory key' % t
            assert g_fr.dtype == np.int32 and np.array_equal(g_fr, w_fr), 'frame %d: memory frame index' % t
    return runs[0]


# ------------------------------------------------------------------------------------------------ the hand-derived cases
@pytest.mark.parametrize('name', ['three_frames', 'contested_8', 'contested_6', 'tie', 'eq_50', 'eq_50_short', 'eq_25', 'eq_25_short',
                                  'hidden_1', 'hidden_0', 'wrap', 'takeover', 'takeover_all'])
def test_hand_cases_equal_the_restatement(name):
    cases = {'three_frames': ref.case_three_frames, 'contested_8': lambda: ref.case_contested(0.125),
             'contested_6': lambda: ref.case_contested(0.6), 'tie': ref.case_tie, 'eq_50': lambda: ref.case_equality(0.5, False),
             'eq_50_short': lambda: ref.case_equality(0.5, True), 'eq_25': lambda: ref.case_equality(0.25, False),
             'eq_25_short': lambda: ref.case_equality(0.25, True), 'hidden_1': lambda: ref.case_hidden(1),
             'hidden_0': lambda: ref.case_hidden(0), 'wrap': ref.case_wrap, 'takeover': ref.case_takeover,
             'takeover_all': ref.case_takeover_all}
    frames, kw = cases[name]()
    got = check_against_ref(frames, kw)
    if name == 'takeover':
        assert got[1][1][-1].tolist() == [4, 255, 1, 0, 0, 1, 1, 1]      # the segment on the free pixel took over id 1
    if name == 'wrap':
        assert got[2][1][2:, 2].tolist() == [255, 2, 4, 5]


# ------------------------------------------------------------------------------------------------ shapes, counts, thresholds, ages
def many_of_one_category(H, W, n, frames, seed):
    """n instances of category 6 as 1 x 2 dominoes on a grid, the whole pattern sliding one pixel per frame, numbered in a fresh random
    order per frame; one domino in eight blinks out for a frame."""
    rng = np.random.default_rng(seed)
    cols = W // 3
    assert n <= cols * (H // 2)
    out = []
    for t in range(frames):
        f = ref.blank(H, W)
        order = rng.permutation(n)
        for num, k in enumerate(order):
            if rng.random() < 0.125:
                continue
            y, x = 2 * (k // cols), 3 * (k % cols) + t
            if x + 1 < W:
                ref.put(f, 6, num + 1, y, y, x, x + 1)
        out.append(f)
    return out


def many_categories(H, W, ncat, frames, seed):
    """Things of ncat categories at once (1..3 instances each) on a stuff background."""
    return ref.blob_sequence(seed, H, W, 2 * ncat, frames, list(range(ncat)), stuff=(200, 254), step=2)


@pytest.mark.parametrize('H,W', [(1, 1), (1, 67), (37, 53), (64, 64), (128, 256)])
def test_blobs_equal_the_restatement(H, W):
    """20 blobs of three categories moving by up to 3 pixels per frame with births and deaths over 12 frames; every threshold with
    every age."""
    for thr in (1.0 / 16.0, 0.3, 1.0):
        for age in (0, 1, 3):
            frames = ref.blob_sequence(100 * H + W + age, H, W, 20, 12, [1, 2, 11])
            check_against_ref(frames, dict(iou_thresh=thr, max_age=age), patterns='AB' if thr == 0.3 else ('A' if age else 'B'))


@pytest.mark.parametrize('things', [0, 1])
def test_few_things(things):
    for H, W in ((1, 1), (37, 53)):
        frames = ref.blob_sequence(7 + things, H, W, things, 4, [3], churn=0.0)
        if things:
            assert any((f[:, :, 1] > 0).any() for f in frames)
        check_against_ref(frames, dict(iou_thresh=0.3, max_age=1))


@pytest.mark.parametrize('age', [0, 3])
def test_255_of_one_category(age):
    frames = many_of_one_category(37, 53, 255, 5, 3)
    assert len(np.unique(frames[0][:, :, 1])) > 200
    got = check_against_ref(frames, dict(iou_thresh=1.0 / 16.0, max_age=age))
    assert got[1][1][:, 3].sum() > 100        # most dominoes are matched after sliding one pixel (IoU 1/3)


def test_81_categories_at_once():
    frames = many_categories(64, 64, 81, 4, 5)
    assert len(np.unique(frames[0][:, :, 0][frames[0][:, :, 1] > 0])) > 60
    check_against_ref(frames, dict(iou_thresh=0.3, max_age=1))


def test_more_segments_than_travel_with_the_step():
    """More thing segments than the tracker's one copy per step carries (FAST_ROWS): the rest of the table is fetched from the
    device when the segments are looked at, at once or only after the next step has run."""
    from upsnet_amd.dataset import pan_track
    frames = []
    for t in range(3):
        f = ref.blank(64, 64)
        flat = f.reshape(-1, 3)
        for k in range(81 * 20):
            flat[(2 * k + t) % 4096] = (k % 81, k // 81 + 1, 0)
        frames.append(f)
    kw = dict(iou_thresh=0.3, max_age=1)
    got = check_against_ref(frames, kw, patterns='A')
    assert len(got[0][1]) == 1620 > pan_track.FAST_ROWS
    lazy = device_run(frames, kw, look=False)
    for a, b in zip(got, lazy):
        assert np.array_equal(a[1], b[1]) and a[4] == b[4]


def test_more_cells_than_the_count_pass_holds_in_lds():
    """64 x 64 = one workgroup of the count pass. Every thing key of 16 categories x instances 1..255 on one pixel each, the other 16
    pixels VOID; the second frame is a permutation of the first. 4080 distinct A_cur cells (and in the second frame as many A_mem
    cells, plus the joint ones) meet an LDS table of 2048 slots, so whatever the hash does with them, more than half of the cells take
    the global fallback."""
    rng = np.random.default_rng(2048)
    flat = np.full((4096, 3), (255, 0, 0), np.uint8)
    flat[:4080] = [(c, i, 0) for c in range(16) for i in range(1, 256)]
    first = flat[rng.permutation(4096)]
    second = first[rng.permutation(4096)]
    frames = [np.ascontiguousarray(f.reshape(64, 64, 3)) for f in (first, second)]
    assert len(np.unique(frames[1].reshape(-1, 3)[:, :2], axis=0)) == 4081 > 2048
    got = check_against_ref(frames, dict(iou_thresh=0.3, max_age=1))
    assert len(got[0][1]) == len(got[1][1]) == 4080
    assert got[1][1][:, 3].sum() > 0 and got[1][1][:, 7].sum() > 0      # matches and take-overs both occur


def test_unaligned_input_takes_the_byte_paths():
    frames = ref.blob_sequence(41, 37, 53, 20, 5, [1, 2, 11])
    check_against_ref(frames, dict(iou_thresh=0.3, max_age=1), unaligned=True)


def test_full_size_sequence():
    """1024 x 2048, three frames, 30 blobs: the vector paths of every pass, more than one workgroup, counts beyond 2^16."""
    frames = ref.blob_sequence(11, 1024, 2048, 30, 3, [11, 12, 13, 14], step=6, churn=0.1)
    check_against_ref(frames, dict(iou_thresh=0.3, max_age=1), patterns='A')


# ------------------------------------------------------------------------------------------------ workspace, laziness, refusals, reset
def test_workspace_is_zero_again_and_tables_need_no_reader():
    from upsnet_amd._lib import lib
    from upsnet_amd.dataset.pan_track import PanopticTracker
    frames = ref.blob_sequence(21, 64, 64, 20, 6, [1, 2])
    kw = dict(iou_thresh=0.3, max_age=1)
    trk = PanopticTracker(**kw)
    off = int(lib().upsnet_pan_track_stamp_offset())
    for f in frames:
        trk.update(torch.from_numpy(f).cuda())
        counts = trk._ws[:off - 4 * 256]
        assert int(torch.count_nonzero(counts)) == 0, 'count cells left non-zero'
        assert int(torch.count_nonzero(trk._ws[off - 4 * 256:off])) == 0, 'segment counters left non-zero'
    eager, lazy = device_run(frames, kw, look=True), device_run(frames, kw, look=False)
    for a, b in zip(eager, lazy):
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[4] == b[4]
        assert np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])


def test_refusals_leave_the_state_untouched():
    from upsnet_amd.dataset.pan_track import PanopticTracker
    for thr in (0.0624, 1.0001, float('nan'), -1.0):
        with pytest.raises(ValueError):
            PanopticTracker(iou_thresh=thr)
    for age in (-1, 0.5):
        with pytest.raises(ValueError):
            PanopticTracker(max_age=age)
    frames, kw = ref.case_three_frames()
    trk = PanopticTracker(**kw)
    trk.update(frames[0])
    key, fr = trk.state()
    with pytest.raises(ValueError):
        trk.update(torch.zeros((6, 9, 3), dtype=torch.uint8, device='cuda'))
    with pytest.raises(ValueError):
        trk.update(np.zeros((6, 8), np.uint8))
    with pytest.raises(ValueError):
        trk.update(np.zeros((6, 8, 3), np.int32))
    assert trk.frame_index == 1
    k2, f2 = trk.state()
    assert np.array_equal(key, k2) and np.array_equal(fr, f2)
    out, segs = trk.update(frames[1])
    want = ref.track_sequence(frames[:2], **kw)
    assert np.array_equal(out.cpu().numpy(), want[1][0]) and list(segs) == want[1][2]
    big = PanopticTracker()
    huge = torch.empty((4097, 4096, 3), dtype=torch.uint8, device='meta')      # H * W > 2^24: refused before anything is allocated
    with pytest.raises(ValueError):
        big.update(huge)
    assert big.shape is None and big.frame_index == 0


def test_reset_gives_a_fresh_tracker():
    from upsnet_amd.dataset.pan_track import PanopticTracker
    a = ref.blob_sequence(31, 37, 53, 12, 4, [1, 2])
    b = ref.blob_sequence(32, 37, 53, 12, 4, [1, 2])
    kw = dict(iou_thresh=0.3, max_age=3)
    trk = PanopticTracker(**kw)
    for f in a:
        trk.update(f)
    trk.reset(serials=True)
    fresh = device_run(b, kw)
    for f, want in zip(b, fresh):
        out, segs = trk.update(f)
        key, fr = trk.state()
        assert np.array_equal(out.cpu().numpy(), want[0]) and list(segs) == want[4]
        assert np.array_equal(key, want[2]) and np.array_equal(fr, want[3])
    # reset() alone: ids and memory start again, the serials go on
    n = trk.next_serial
    trk.reset()
    out, segs = trk.update(b[0])
    assert np.array_equal(out.cpu().numpy(), fresh[0][0])
    assert [s['track_id'] for s in segs] == [s['track_id'] + n - 1 for s in fresh[0][4]]
    # a frame of another size is taken after reset()
    trk.reset()
    other, kw2 = ref.case_three_frames()
    assert np.array_equal(trk.update(other[0])[0].cpu().numpy(), other[0])


# ------------------------------------------------------------------------------------------------ frame-stable colours
CATEGORIES = [{'id': 0, 'name': 'road', 'isthing': 0, 'color': [128, 64, 128]}, {'id': 1, 'name': 'sky', 'isthing': 0, 'color': [70, 130, 180]},
              {'id': 2, 'name': 'person', 'isthing': 1, 'color': [220, 20, 60]}, {'id': 3, 'name': 'car', 'isthing': 1, 'color': [0, 0, 142]},
              {'id': 4, 'name': 'dark', 'isthing': 1, 'color': [0, 0, 0]}, {'id': 254, 'name': 'last', 'isthing': 1}]


def stable_map(H, W, seed):
    rng = np.random.default_rng(seed)
    f = ref.blank(H, W)
    f[:H // 2] = (0, 0, 0)
    f[H // 2:, :W // 2] = (1, 0, 0)
    for k in range(40):
        c = int(rng.choice([2, 3, 4, 254]))
        y, x = int(rng.integers(0, H)), int(rng.integers(0, W))
        ref.put(f, c, int(rng.integers(1, 256)), y, min(y + 3, H - 1), x, min(x + 5, W - 1))
    return f


@pytest.mark.parametrize('H,W', [(1, 1), (37, 53), (64, 80)])
def test_stable_colours_equal_the_host_statement(H, W):
    from upsnet_amd import ops
    from upsnet_amd.dataset import pan_format as pf
    cats = pf.category_dict(CATEGORIES)
    f = stable_map(H, W, H + W)
    want_png = ref.stable_png(f)
    want_pic = np.zeros_like(f)
    for c, i in set(map(tuple, f[:, :, :2].reshape(-1, 2).tolist())):
        if c != 255:
            want_pic[(f[:, :, 0] == c) & (f[:, :, 1] == i)] = ref.stable_picture_colour(c, i, pf.category_color(c, cats[c]), cats[c]['isthing'])
    res = []
    for p in 'AB':
        with memguard.poisoned(p, modules=GUARDED):
            d = memguard.banded_copy(torch.from_numpy(f).cuda(), p)
            table = memguard.banded_copy(torch.from_numpy(pf.category_table(CATEGORIES)).cuda(), p)
            png = ops.pan_stable_colors(d, None, 0, pf.torch.empty(f.shape, dtype=torch.uint8, device='cuda'))
            pic = ops.pan_stable_colors(d, table, 1, pf.torch.empty(f.shape, dtype=torch.uint8, device='cuda'))
            fmt = pf.PanopticFormatter(CATEGORIES, stable_ids=True)
            rgb, rgb_host, info = fmt.finish(fmt.submit(d))
            res.append((png.cpu().numpy(), pic.cpu().numpy(), rgb.cpu().numpy(), rgb_host.copy(), info))
    for png, pic, rgb, rgb_host, info in res:
        assert np.array_equal(png, want_png) and np.array_equal(pic, want_pic)
        assert np.array_equal(rgb, want_png) and np.array_equal(rgb_host, want_png)
        keys = sorted(set(c << 8 | i for c, i in f[:, :, :2].reshape(-1, 2).tolist() if c != 255))
        assert [s['id'] for s in info] == [(k >> 8) + 256 * (k & 255) + 65536 for k in keys]
        assert [s['category_id'] for s in info] == [k >> 8 for k in keys]
        r64 = rgb.astype(np.int64)
        ids = r64[:, :, 0] + 256 * r64[:, :, 1] + 65536 * r64[:, :, 2]
        for s in info:
            assert int((ids == s['id']).sum()) == s['area']
    assert res[0][4] == res[1][4]


def test_default_mode_is_unchanged_by_the_new_argument():
    from upsnet_amd.dataset import pan_format as pf
    from upsnet_amd.dataset.pan_vis import PanopticRenderer
    f = stable_map(37, 53, 9)
    d = torch.from_numpy(f).cuda()
    photo = torch.from_numpy(np.random.default_rng(0).integers(0, 256, (37, 53, 3), dtype=np.uint8)).cuda()
    a = pf.PanopticFormatter(CATEGORIES)
    b = pf.PanopticFormatter(CATEGORIES, None, False)
    ra, rb = a.finish(a.submit(d)), b.finish(b.submit(d))
    assert np.array_equal(ra[0].cpu().numpy(), rb[0].cpu().numpy()) and ra[2] == rb[2]
    want_rgb, want_info = pf.panoptic_format(d, CATEGORIES)
    assert np.array_equal(ra[0].cpu().numpy(), want_rgb.cpu().numpy()) and ra[2] == want_info
    gen = pf.ColorGenerator(CATEGORIES)
    assert [s['id'] for s in ra[2]] == [c[0] + 256 * c[1] + 65536 * c[2] for c in (gen.get_color(s['category_id']) for s in ra[2])]
    for mode in ('flat', 'overlay'):
        pa = PanopticRenderer(CATEGORIES).submit(d, photo, mode)[0].cpu().numpy()
        pb = PanopticRenderer(CATEGORIES, None, False).submit(d, photo, mode)[0].cpu().numpy()
        assert np.array_equal(pa, pb)
    # the stable overlay differs from the default one only through the blended colours: same shape, and it is drawn at all
    ps = PanopticRenderer(CATEGORIES, stable_ids=True).submit(d, photo, 'overlay')[0].cpu().numpy()
    assert ps.shape == pa.shape and ps.dtype == np.uint8


# ------------------------------------------------------------------------------------------------ the command
@pytest.fixture()
def saved_config():
    import copy
    from upsnet_amd.config.config import config
    saved = copy.deepcopy(dict(config))
    yield config
    config.clear()
    config.update(saved)


def _write_frames(root, name, n, H, W, seed):
    """n frames of 4 x 4 colour blocks, the picture moving two pixels to the right per frame."""
    from test_dataset_run_cpu import save_image
    rng = np.random.default_rng(seed)
    rgb = rng.integers(0, 256, (H // 4 + 1, W // 4 + 1, 3)).astype(np.uint8)
    rgb = np.repeat(np.repeat(rgb, 4, 0), 4, 1)[:H, :W]
    paths = []
    for k in range(n):
        paths.append(os.path.join(root, name, 'f_%06d_leftImg8bit.png' % (k * 5)))
        save_image(paths[-1], np.ascontiguousarray(np.roll(rgb, 2 * k, 1)))
    return paths


def test_sequence_command(tmp_path, saved_config):
    from PIL import Image
    from test_dataset_run_cpu import write_cfg
    from upsnet_amd import sequence
    from upsnet_amd.config.config import update_config
    from upsnet_amd.dataset.pan_format import png_name
    from upsnet_amd.dataset.pan_track import PanopticTracker
    from upsnet_amd.evaluate import panoptic_predictions, run_inference
    from upsnet_amd.synthetic import build_model
    frames_root = str(tmp_path / 'frames')
    seqs = {'seq_a': _write_frames(frames_root, 'seq_a', 3, 96, 160, 1), 'seq_b': _write_frames(frames_root, 'seq_b', 2, 64, 128, 2)}
    cfg = write_cfg(tmp_path, 'Cityscapes', str(tmp_path / 'data'), 'val')
    cats = str(tmp_path / 'cats.json')
    with open(cats, 'w') as f:
        json.dump({'categories': [{'id': c, 'name': 'c%d' % c, 'isthing': int(c > 10)} for c in range(19)]}, f)
    # the untracked maps, from the same pieces the command uses
    update_config(cfg)
    model = build_model(device='cuda')
    untracked = {}
    for name, paths in seqs.items():
        seq = sequence.FrameSequence(name, paths)
        results, _ = run_inference(model, seq, in_flight=1, device=torch.device('cuda'))
        untracked[name] = [p.cpu().numpy() for p in panoptic_predictions(seq, results, False)]
    del model
    torch.cuda.empty_cache()

    out = str(tmp_path / 'out')
    res = sequence.main(['--cfg', cfg, '--synthetic_weights', '--frames', frames_root, '--out', out, '--panoptic_categories', cats,
                         '--track_max_age', '1', '--vis_panoptic', 'both', '--in-flight', '2'])
    assert [s[0] for s in res['sequences']] == ['seq_a', 'seq_b']
    trk = PanopticTracker(iou_thresh=0.3, max_age=1)
    serials = set()
    for name, paths in seqs.items():
        names = [png_name(os.path.basename(p)) for p in paths]
        assert names[0] == 'f_000000.png'
        for sub in ('pan_2ch', 'pan', 'vis', 'vis_flat'):
            assert sorted(os.listdir(os.path.join(out, name, sub))) == names, sub
        assert sorted(os.listdir(os.path.join(out, name))) == ['pan', 'pan_2ch', 'pred.json', 'tracks.json', 'vis', 'vis_flat']
        trk.reset()           # ids start again, serials go on: what the command documents between sequences
        want = [trk.update(p) for p in untracked[name]]
        pred = json.load(open(os.path.join(out, name, 'pred.json')))['annotations']
        tracks = json.load(open(os.path.join(out, name, 'tracks.json')))
        assert tracks['sequence'] == name and tracks['max_age'] == 1 and tracks['iou_thresh'] == 0.3
        seen = {}
        for k, (fname, (w_map, w_segs), ann) in enumerate(zip(names, want, pred)):
            got = np.array(Image.open(os.path.join(out, name, 'pan_2ch', fname)))
            assert np.array_equal(got, w_map.cpu().numpy()), (name, fname)
            png = np.array(Image.open(os.path.join(out, name, 'pan', fname)))
            assert np.array_equal(png, ref.stable_png(got))
            assert ann['file_name'] == fname and ann['image_id'] == k
            serial = {(s['category'], s['instance']): s['track_id'] for s in w_segs}
            for seg in ann['segments_info']:
                c, i = seg['category_id'], seg['id'] >> 8 & 255
                assert seg['id'] == c + 256 * i + 65536 and seg['track_id'] == serial.get((c, i), 0)
                assert seg['area'] == int(((got[:, :, 0] == c) & (got[:, :, 1] == i)).sum())
                if seg['track_id']:
                    seen.setdefault(seg['track_id'], []).append((fname, c, i))
            assert sorted(serial.values()) == sorted(s['track_id'] for s in ann['segments_info'] if s['track_id'])
        assert [t['track_id'] for t in tracks['tracks']] == sorted(seen)
        for t in tracks['tracks']:
            hits = seen[t['track_id']]
            assert t['frames'] == [h[0] for h in hits] and t['first_frame'] == hits[0][0] and t['last_frame'] == hits[-1][0]
            assert all((c, i) == (t['category_id'], t['instance']) for _, c, i in hits)
        assert not (serials & set(seen))         # the second sequence's serials continue after the first's
        if serials and seen:
            assert min(seen) > max(serials)
        serials |= set(seen)
    # --track_only on the untracked maps reproduces the tracked files byte for byte
    raw = str(tmp_path / 'raw')
    for name, paths in seqs.items():
        os.makedirs(os.path.join(raw, name))
        for p, m in zip(paths, untracked[name]):
            Image.fromarray(m).save(os.path.join(raw, name, png_name(os.path.basename(p))))
    out2 = str(tmp_path / 'out2')
    sequence.main(['--cfg', cfg, '--track_only', raw, '--out', out2, '--panoptic_categories', cats, '--track_max_age', '1',
                   '--vis_panoptic', 'flat'])
    for name, paths in seqs.items():
        rel = ['pred.json', 'tracks.json'] + [os.path.join(sub, png_name(os.path.basename(p))) for p in paths
                                              for sub in ('pan_2ch', 'pan', 'vis_flat')]
        for r in rel:
            with open(os.path.join(out, name, r), 'rb') as a, open(os.path.join(out2, name, r), 'rb') as b:
                assert a.read() == b.read(), (name, r)
