"""GPU: VPQ and STQ of tracked sequences on the device (csrc/video_eval.hip, dataset/video_pq.py).
VideoPanopticEvaluator against the plain numpy restatement of the rule (tests/video_pq_ref.py), bit for bit: the integer counts and the
raw float64 iou_sum / aq_sum words; on poisoned and guard-banded memory (tests/memguard.py, patterns A and B). Then the cross-checks
against the per-image scorers that are pinned to the reference, the limits, the workspace contract and the commands."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import memguard       # noqa: E402
import video_pq_ref as ref   # noqa: E402

pytestmark = pytest.mark.gpu

GUARDED = memguard.MODULES + ('upsnet_amd.dataset.video_pq',)


def on_device(a, pattern=None, unaligned=False):
    t = torch.from_numpy(a).cuda()
    if pattern is not None:
        t = memguard.banded_copy(t, pattern)
    if unaligned:       # the map starts one byte into its buffer: the byte loads
        flat = torch.empty((t.numel() + 1,), dtype=torch.uint8, device='cuda')
        if pattern is not None:
            flat = memguard.banded_copy(flat.fill_(memguard.poison_byte(torch.uint8, pattern)), pattern)
        flat[1:].copy_(t.reshape(-1))
        t = flat[1:].view(t.shape)
    return t


def feed(ev, sequences, pattern=None, unaligned=False):
    for preds, gts, infos in sequences:
        ev.begin_sequence(infos)
        for p, g in zip(preds, gts):
            ev.add_frame(on_device(p, pattern, unaligned), on_device(g, pattern, unaligned))
        ev.end_sequence()


def device_run(sequences, categories, windows, pattern=None, unaligned=False, **kw):
    """(raw(), summary(), evaluator) of a fresh evaluator; with a pattern, on poisoned allocations and banded inputs."""
    from upsnet_amd.dataset.video_pq import VideoPanopticEvaluator

    def run():
        ev = VideoPanopticEvaluator(categories, windows=windows, **kw)
        feed(ev, sequences, pattern, unaligned)
        raw = ev.raw()
        return raw, ev.summary(), ev
    if pattern is None:
        return run()
    with memguard.poisoned(pattern, modules=GUARDED):
        return run()


def ref_run(sequences, categories, windows):
    ev = ref.RefVideoEvaluator(categories, windows)
    for preds, gts, infos in sequences:
        ev.add_sequence(preds, gts, infos)
    return ev


def words(x):
    return np.asarray(x, np.float64).view(np.int64)


def assert_equal_to_ref(raw, summary, want):
    for w, n in enumerate(want.windows):
        for name, got in (('tp', raw['tp']), ('fp', raw['fp']), ('fn', raw['fn'])):
            exp = np.zeros(256, np.int64)
            for c, v in getattr(want, name)[n].items():
                exp[c] = v
            assert got.dtype == np.int64 and np.array_equal(got[w], exp), 'window %d: %s\n%s\n%s' % (n, name, np.nonzero(got[w] - exp), exp[exp > 0])
        exp = np.zeros(256, np.float64)
        for c, v in want.iou[n].items():
            exp[c] = v
        assert raw['iou'].dtype == np.float64 and np.array_equal(words(raw['iou'][w]), words(exp)), 'window %d: iou_sum words' % n
    assert np.array_equal(raw['conf'], want.conf), 'confusion matrix'
    assert raw['num_tracks'] == want.num_tracks
    assert np.array_equal(words(raw['aq_sums']), words(want.aq_sums)), 'aq_sum words'
    stq = want.stq()
    for k in ('stq', 'aq', 'iou', 'num_tracks'):
        assert summary['stq'][k] == stq[k], k
    for n in want.windows:
        for name, isthing in (('All', None), ('Things', True), ('Stuff', False)):
            pq, sq, rq, k = want.pq(n, isthing)
            got = summary['vpq']['per_window'][n][name]
            assert (got['pq'], got['sq'], got['rq'], got['n']) == (pq, sq, rq, k), (n, name)
    assert summary['vpq']['All']['pq'] == want.vpq() and summary['vpq']['Things']['pq'] == want.vpq(True)
    assert summary['sequences'] == want.sequences and summary['frames'] == want.frames


def check(sequences, categories=ref.CATEGORIES, windows=(1, 2, 3, 4), patterns='AB', unaligned=False, **kw):
    want = ref_run(sequences, categories, windows)
    out = None
    for p in patterns:
        raw, summary, ev = device_run(sequences, categories, windows, p, unaligned, **kw)
        assert_equal_to_ref(raw, summary, want)
        out = (raw, summary, ev)
    return want, out


# ------------------------------------------------------------------------------------------------ the hand-derived cases
@pytest.mark.parametrize('name', ['perfect', 'switch_6', 'switch_7', 'iou_half', 'fp_keep', 'fp_skip', 'crowd', 'cross', 'short'])
def test_hand_cases_equal_the_restatement(name):
    case = {'perfect': ref.case_perfect, 'switch_6': lambda: ref.case_identity_switch(6), 'switch_7': lambda: ref.case_identity_switch(7),
            'iou_half': ref.case_iou_half, 'fp_keep': lambda: ref.case_fp_skip(2), 'fp_skip': lambda: ref.case_fp_skip(3),
            'crowd': ref.case_crowd, 'cross': ref.case_cross_category, 'short': ref.case_short}[name]()
    preds, gts, infos, windows = case
    want, (raw, summary, _) = check([(preds, gts, infos)], windows=windows)
    if name == 'perfect':
        assert summary['vpq']['All']['pq'] == 1.0 and summary['stq']['stq'] == 1.0
    if name.startswith('switch'):
        assert summary['stq']['aq'] == 0.5 and raw['tp'][:, 1].tolist() == [4, 2, 2, 0] and raw['fp'][:, 1].tolist() == [0, 2, 2, 2]
    if name == 'iou_half':
        assert (raw['tp'][0, 1], raw['fp'][0, 1], raw['fn'][0, 1]) == (0, 1, 1)
    if name == 'fp_keep':
        assert raw['fp'][0, 1] == 1
    if name == 'fp_skip':
        assert raw['fp'][0, 1] == 0
    if name == 'crowd':
        assert (raw['tp'][0, 1], raw['fp'][0, 1], raw['fn'][0, 1]) == (0, 0, 1) and summary['stq']['aq'] == 1.0
    if name == 'cross':
        assert summary['stq']['aq'] == 1.0 and summary['stq']['iou'] == 0.0 and raw['fp'][0, 2] == 1 and raw['fn'][0, 1] == 1
    if name == 'short':
        assert not raw['tp'][1].any() and not raw['fp'][1].any() and not raw['fn'][1].any()


# ------------------------------------------------------------------------------------------------ random blobs
@pytest.mark.parametrize('H,W', [(1, 1), (1, 67), (37, 53), (64, 64), (128, 256)])
def test_blobs_equal_the_restatement(H, W):
    """Two sequences of 5 and 6 frames (drifting rectangles of 3 thing and 2 stuff categories, a crowd segment, a GT VOID band, an id
    outside the table, pred VOID holes, a wrong-category prediction, an identity switch) into one evaluator."""
    sequences = [ref.blob_sequence(100 * H + W, H, W, 5, switch_at=2), ref.blob_sequence(100 * H + W + 1, H, W, 6, switch_at=3)]
    check(sequences)
    if (H, W) == (37, 53):
        check(sequences, patterns='A', unaligned=True)


# ------------------------------------------------------------------------------------------------ cross-checks against pinned scorers
def blob_frames_for_cross_checks():
    preds, gts, infos = ref.blob_sequence(11, 64, 96, 6, switch_at=3, unknown_id=False)
    for gt, segs in zip(gts, infos):       # JSON areas = pixel counts
        gid = gt[:, :, 0].astype(np.int64) + 256 * gt[:, :, 1].astype(np.int64) + 65536 * gt[:, :, 2].astype(np.int64)
        for s in segs:
            s['area'] = int((gid == s['id']).sum())
            assert s['area'] > 0
    return preds, gts, infos


def test_window_1_equals_the_per_image_scorer():
    """windows=(1,): every frame is its own window, so VPQ_1's counts are PanopticEvaluator's over the same frames (JSON areas = pixel
    counts, one crowd segment per category at most, no id outside segments_info): tp / fp / fn equal, the iou words bit-equal."""
    from upsnet_amd.dataset.pq import PanopticEvaluator
    preds, gts, infos = blob_frames_for_cross_checks()
    _, _, ev = device_run([(preds, gts, infos)], ref.CATEGORIES, (1,))
    pe = PanopticEvaluator(ref.CATEGORIES)
    for p, g, s in zip(preds, gts, infos):
        pe.add(p, g, s)
    a, b = ev.vpq_stat()[1], pe.pq_stat()
    cats = sorted(set(a.pq_per_cat) | set(b.pq_per_cat))
    assert len(cats) >= 4 and sum(b[c].tp for c in cats) > 0 and sum(b[c].fp for c in cats) > 0 and sum(b[c].fn for c in cats) > 0
    for c in cats:
        assert (a[c].tp, a[c].fp, a[c].fn) == (b[c].tp, b[c].fp, b[c].fn), c
        assert words(a[c].iou) == words(b[c].iou), c


def test_confusion_matrix_equals_confusion_accumulate():
    from upsnet_amd import ops
    preds, gts, infos = blob_frames_for_cross_checks()
    raw, _, _ = device_run([(preds, gts, infos)], ref.CATEGORIES, (1,))
    table = {r[0]: r[1] for r in ref.sequence_table(infos)}
    conf = torch.zeros((256, 256), dtype=torch.int64, device='cuda')
    for p, g in zip(preds, gts):
        gid = g[:, :, 0].astype(np.int64) + 256 * g[:, :, 1].astype(np.int64) + 65536 * g[:, :, 2].astype(np.int64)
        gcat = np.full(gid.shape, 255, np.uint8)
        for i, c in table.items():
            gcat[gid == i] = c
        ops.confusion_accumulate(torch.from_numpy(gcat).cuda(), torch.from_numpy(np.ascontiguousarray(p[:, :, 0])).cuda(), 256, 255, conf)
    assert np.array_equal(raw['conf'], conf.cpu().numpy()) and raw['conf'][:, 255].sum() > 0


# ------------------------------------------------------------------------------------------------ limits
def dominoes(H, W, n, frames, cat=6):
    """n instances of one category as 1 x 2 dominoes; the prediction slides one pixel to the right per frame."""
    cols = W // 3
    assert n <= cols * (H // 2) and n <= 255
    preds, gts, infos = [], [], []
    for t in range(frames):
        p, g = ref.blank_pred(H, W), ref.blank_gt(H, W)
        for k in range(n):
            y, x = 2 * (k // cols), 3 * (k % cols)
            ref.put_gt(g, 1000 + k, y, y, x, x + 1)
            ref.put_pred(p, cat, k + 1, y, y, min(x + (t & 1), W - 1), min(x + 1 + (t & 1), W - 1))
        preds.append(p)
        gts.append(g)
        infos.append([ref.seg(1000 + k, cat) for k in range(n)])
    return preds, gts, infos


def test_255_instances_of_one_category():
    want, _ = check([dominoes(37, 53, 255, 5)], categories={6: {'id': 6, 'isthing': 1}})
    assert want.num_tracks == 255 and want.tp[1][6] > 255 and want.fn[1][6] > 0 and want.tp[2][6] > 0


def test_81_categories_at_once():
    H, W, frames = 37, 53, 4
    cats = {c: {'id': c, 'isthing': int(c % 3 != 0)} for c in range(81)}
    preds, gts, infos = [], [], []
    for t in range(frames):
        p, g = ref.blank_pred(H, W), ref.blank_gt(H, W)
        for c in range(81):
            y, x = 2 * (c // 13), 4 * (c % 13)
            ref.put_gt(g, 100 + c, y, y + 1, x, x + 2)
            ref.put_pred(p, c, 0 if c % 3 == 0 else 1 + (t > 1 and c == 7), y, y + 1, x + (c & 1) * (t & 1), x + 2)
        preds.append(p)
        gts.append(g)
        infos.append([ref.seg(100 + c, c) for c in range(81)])
    want, _ = check([(preds, gts, infos)], categories=cats)
    assert len(want.tp[1]) == 81


def noise_frames(block, frames=2):
    """64 x 64, every block x block tile its own (GT segment, pred key) pair."""
    per = 64 // block
    n = per * per
    idx = (np.arange(64)[:, None] // block) * per + np.arange(64)[None, :] // block
    preds, gts, infos = [], [], []
    for t in range(frames):
        p, g = ref.blank_pred(64, 64), ref.blank_gt(64, 64)
        k = (idx + t) % n
        p[:, :, 0], p[:, :, 1] = k // 256, k % 256
        gid = idx + 1
        g[:, :, 0], g[:, :, 1] = gid & 255, gid >> 8
        preds.append(p)
        gts.append(g)
        infos.append([ref.seg(i + 1, i // 256) for i in range(n)])
    return preds, gts, infos, {c: {'id': c, 'isthing': 1} for c in range(max(n // 256, 1))}


def test_noise_like_frames_are_exact_or_refused():
    """1024 pairs per frame load the frame table (4096 slots for 64 x 64) to three quarters: exact. 4096 pairs per frame (every pixel
    its own) are more cells than the table has slots: the documented RuntimeError, never a wrong result."""
    preds, gts, infos, cats = noise_frames(2)
    check([(preds, gts, infos)], categories=cats, windows=(1, 2))
    preds, gts, infos, cats = noise_frames(1)
    try:
        raw, summary, _ = device_run([(preds, gts, infos)], cats, (1, 2), 'A')
    except RuntimeError as e:
        assert 'was full' in str(e) and 'counts were dropped' in str(e)
    else:
        assert_equal_to_ref(raw, summary, ref_run([(preds, gts, infos)], cats, (1, 2)))


def test_unknown_category_is_a_key_error_naming_the_place():
    from upsnet_amd.dataset.video_pq import VideoPanopticEvaluator
    preds, gts, infos = ref.blob_sequence(5, 37, 53, 4)
    bad = [p.copy() for p in preds]
    bad[2][0, 0, 0], bad[2][0, 0, 1] = 37, 1
    bad[3][0, 0, 0], bad[3][0, 0, 1] = 36, 1
    ev = VideoPanopticEvaluator(ref.CATEGORIES)
    feed(ev, [(preds, gts, infos)])
    ev.begin_sequence(infos, name='street')
    for p, g in zip(bad, gts):
        ev.add_frame(p, g)
    with pytest.raises(KeyError, match='sequence street .index 1 in the order added. frame 2 a segment has unknown category_id 37'):
        ev.summary()


# ------------------------------------------------------------------------------------------------ the workspace contract
def test_workspace_is_zero_again_and_a_second_sequence_scores_as_on_a_fresh_evaluator():
    from upsnet_amd.dataset.video_pq import VideoPanopticEvaluator
    a, b = ref.blob_sequence(21, 37, 53, 6, switch_at=2), ref.blob_sequence(22, 37, 53, 5, switch_at=1)
    with memguard.poisoned('A', modules=GUARDED):
        ev = VideoPanopticEvaluator(ref.CATEGORIES)
        feed(ev, [a], 'A')
        ws = ev.workspace()
        assert ws is not None and ws.numel() > 0 and not bool(ws.any()), 'the workspace is not zero after end_sequence'
        first = ev.raw()
        feed(ev, [b], 'A')
        assert ev.workspace() is ws and not bool(ws.any())
        both = ev.raw()
        fresh = VideoPanopticEvaluator(ref.CATEGORIES)
        feed(fresh, [b], 'A')
        alone = fresh.raw()
    for k in ('tp', 'fp', 'fn'):
        assert np.array_equal(both[k] - first[k], alone[k]), k
    assert np.array_equal(both['conf'] - first['conf'], alone['conf'])
    assert words(both['aq_sums'][1:]).tolist() == words(alone['aq_sums']).tolist()
    assert_equal_to_ref(both, ev.summary(), ref_run([a, b], ref.CATEGORIES, (1, 2, 3, 4)))


def test_a_used_evaluator_takes_sequences_of_other_sizes_like_a_fresh_one():
    """One evaluator over 65 x 129, 37 x 53 and 65 x 129 again (other content; the workspace is replaced at each change of size, the
    accumulators, seq_out and the pinned buffers are kept): after every sequence the integer counts and the confusion cells it added
    and its aq_sum are those of a fresh evaluator on that sequence alone, bit for bit, and the totals -- the float64 iou sums included --
    are the restatement's over all three."""
    from upsnet_amd.dataset.video_pq import VideoPanopticEvaluator
    seqs = [ref.blob_sequence(41, 65, 129, 4, switch_at=2), ref.blob_sequence(42, 37, 53, 5, switch_at=1), ref.blob_sequence(43, 65, 129, 3, switch_at=1)]
    ev = VideoPanopticEvaluator(ref.CATEGORIES)
    before = ev.raw()
    for k, seq in enumerate(seqs):
        feed(ev, [seq])
        assert not bool(ev.workspace().any()) and tuple(ev._ws_shape) == seq[0][0].shape[:2]
        after = ev.raw()
        fresh = VideoPanopticEvaluator(ref.CATEGORIES)
        feed(fresh, [seq])
        alone = fresh.raw()
        for name in ('tp', 'fp', 'fn', 'conf'):
            assert np.array_equal(after[name] - before[name], alone[name]), (k, name)
        assert after['num_tracks'] - before['num_tracks'] == alone['num_tracks']
        assert words(after['aq_sums'][-1:]).tolist() == words(alone['aq_sums']).tolist(), k
        if k == 0:
            assert np.array_equal(words(after['iou']), words(alone['iou']))
        before = {n: (v.copy() if isinstance(v, np.ndarray) else v) for n, v in after.items()}
    assert_equal_to_ref(ev.raw(), ev.summary(), ref_run(seqs, ref.CATEGORIES, (1, 2, 3, 4)))


def test_refusals_leave_the_state_untouched():
    from upsnet_amd.dataset.video_pq import VideoPanopticEvaluator
    preds, gts, infos = ref.blob_sequence(31, 37, 53, 5, switch_at=2)
    ev = VideoPanopticEvaluator(ref.CATEGORIES)
    ev.begin_sequence(infos)
    for t, (p, g) in enumerate(zip(preds, gts)):
        if t == 2:
            for bad_p, bad_g in ((np.zeros((37, 54, 3), np.uint8), np.zeros((37, 54, 3), np.uint8)), (p, g[:, :52]), (p.astype(np.int16), g),
                                 (torch.from_numpy(p).cuda()[:, :, :2], g)):
                with pytest.raises(ValueError):
                    ev.add_frame(bad_p, bad_g)
            with pytest.raises(ValueError, match='inside a sequence'):
                ev.begin_sequence(infos)
        ev.add_frame(p, g)
    ev.end_sequence()
    with pytest.raises(ValueError, match='one object'):
        ev.begin_sequence([[ref.seg(3, 1)], [ref.seg(3, 2)]])
    with pytest.raises(ValueError, match='outside a sequence'):
        ev.add_frame(preds[0], gts[0])
    assert not bool(ev.workspace().any())
    assert_equal_to_ref(ev.raw(), ev.summary(), ref_run([(preds, gts, infos)], ref.CATEGORIES, (1, 2, 3, 4)))


# ------------------------------------------------------------------------------------------------ full size
def test_full_size_sequence():
    """1024 x 2048, 6 frames, 30 moving things of 3 categories on two stuff halves, one identity switch, against the restatement."""
    H, W, frames = 1024, 2048, 6
    rng = np.random.default_rng(7)
    things = [(int(rng.integers(0, H - 200)), int(rng.integers(0, W - 300)), int(rng.integers(20, 200)), int(rng.integers(20, 300)),
               (1, 2, 11)[k % 3], int(rng.integers(-9, 10)), int(rng.integers(-9, 10))) for k in range(30)]
    preds, gts, infos = [], [], []
    for t in range(frames):
        p, g = ref.blank_pred(H, W), ref.blank_gt(H, W)
        ref.put_gt(g, 1000, 0, H - 1, 0, W // 2)
        ref.put_gt(g, 1001, 0, H - 1, W // 2 + 1, W - 1)
        ref.put_pred(p, 200, 0, 0, H - 1, 0, W // 2 - 7)
        ref.put_pred(p, 254, 0, 0, H - 1, W // 2 - 6, W - 1)
        segs = [ref.seg(1000, 200), ref.seg(1001, 254)]
        for k, (y, x, h, w, cat, dy, dx) in enumerate(things):
            y, x = max(0, min(y + t * dy, H - h)), max(0, min(x + t * dx, W - w))
            ref.put_gt(g, 2000 + k, y, y + h - 1, x, x + w - 1)
            ref.put_pred(p, cat, k + 1 if not (k == 0 and t >= 3) else 77, y + 2, min(y + h + 1, H - 1), x + 3, min(x + w + 2, W - 1))
            segs.append(ref.seg(2000 + k, cat, crowd=int(k == 5)))
        ref.put_gt(g, 0, 500, 503, 0, W - 1)
        ref.put_pred(p, ref.VOID, 0, 0, 3, 0, W - 1)
        preds.append(p)
        gts.append(g)
        infos.append(segs)
    want, _ = check([(preds, gts, infos)], patterns='A')
    assert want.num_tracks >= 20 and sum(want.tp[4].values()) >= 5


# ------------------------------------------------------------------------------------------------ the commands
@pytest.fixture
def saved_config():
    from upsnet_amd.config.config import config
    import copy
    saved = copy.deepcopy(dict(config))
    yield
    config.clear()
    config.update(saved)


def test_commands(tmp_path, saved_config):
    from PIL import Image
    from test_dataset_run_cpu import write_cfg
    from upsnet_amd import sequence, video_eval
    from upsnet_amd.dataset.video_pq import VideoPanopticEvaluator
    cfg = write_cfg(tmp_path, 'Cityscapes', str(tmp_path / 'data'), 'val')
    cats = str(tmp_path / 'cats.json')
    with open(cats, 'w') as f:
        json.dump({'categories': list(ref.CATEGORIES.values())}, f)
    raw = tmp_path / 'raw'
    names = ['f_%06d.png' % (5 * k) for k in range(5)]
    for seq, seed in (('seq_a', 41), ('seq_b', 42)):
        os.makedirs(str(raw / seq))
        preds, _, _ = ref.blob_sequence(seed, 48, 64, 5)
        for n, p in zip(names, preds):
            Image.fromarray(p).save(str(raw / seq / n))
    base = ['--cfg', cfg, '--panoptic_categories', cats, '--track_max_age', '1']
    # without --video_gt: the folders are what they were
    out = str(tmp_path / 'out')
    sequence.main(base + ['--track_only', str(raw), '--out', out])
    assert sorted(os.listdir(out)) == ['seq_a', 'seq_b']
    assert sorted(os.listdir(os.path.join(out, 'seq_a'))) == ['pan', 'pan_2ch', 'pred.json', 'tracks.json']
    # scored against its own output as ground truth: VPQ = 1, STQ = 1
    out2 = str(tmp_path / 'out2')
    res = sequence.main(base + ['--track_only', str(raw), '--out', out2, '--video_gt', out, '--vpq_windows', '1', '2', '3'])
    scores = res['video_scores']
    # (STQ to rounding: every track contributes (1.0 / G) * G, which is 1 to within an ulp)
    assert scores['vpq']['All']['pq'] == 1.0 and scores['vpq']['Things']['sq'] == 1.0 and abs(scores['stq']['stq'] - 1.0) < 1e-12
    assert scores['stq']['iou'] == 1.0
    assert scores['sequences'] == 2 and scores['frames'] == 10 and sorted(scores['vpq']['per_window']) == [1, 2, 3]
    assert sorted(os.listdir(out2)) == ['seq_a', 'seq_b', 'video_scores.json']
    assert sorted(os.listdir(os.path.join(out2, 'seq_a'))) == ['pan', 'pan_2ch', 'pred.json', 'tracks.json']
    written = json.load(open(os.path.join(out2, 'video_scores.json')))
    assert written['windows'] == [1, 2, 3] and written['summary']['stq']['stq'] == scores['stq']['stq']
    assert written['sequences'] == [{'name': 'seq_a', 'frames': 5}, {'name': 'seq_b', 'frames': 5}]
    for seq in ('seq_a', 'seq_b'):
        for n in names:
            with open(os.path.join(out, seq, 'pan_2ch', n), 'rb') as a, open(os.path.join(out2, seq, 'pan_2ch', n), 'rb') as b:
                assert a.read() == b.read()
    # the re-scoring command against a shifted copy that covers a subset of the frames: the evaluator called directly
    gt = tmp_path / 'gt'
    ev = VideoPanopticEvaluator(ref.CATEGORIES, windows=(1, 2))
    for seq in ('seq_a', 'seq_b'):
        os.makedirs(str(gt / seq / 'pan'))
        anns = json.load(open(os.path.join(out, seq, 'pred.json')))['annotations']
        keep = [a for a in anns if a['file_name'] != names[1]]
        maps, gts = [], []
        for a in keep:
            png = np.roll(np.array(Image.open(os.path.join(out, seq, 'pan', a['file_name']))), 3, 1)
            Image.fromarray(png).save(str(gt / seq / 'pan' / a['file_name']))
            gts.append(png)
            maps.append(np.array(Image.open(os.path.join(out, seq, 'pan_2ch', a['file_name']))))
        with open(str(gt / seq / 'gt.json'), 'w') as f:
            json.dump({'annotations': [{'file_name': a['file_name'], 'segments_info': a['segments_info']} for a in reversed(keep)]}, f)
        ev.begin_sequence([a['segments_info'] for a in keep])
        for m, g in zip(maps, gts):
            ev.add_frame(m, g)
        ev.end_sequence()
    want = ev.summary()
    got = video_eval.main(['--pred', out, '--video_gt', str(gt), '--panoptic_categories', cats, '--vpq_windows', '1', '2',
                           '--out', str(tmp_path / 'scores.json')])
    assert got == want and 0 < got['vpq']['All']['pq'] < 1 and 0 < got['stq']['stq'] < 1 and got['frames'] == 8
    assert json.load(open(str(tmp_path / 'scores.json')))['summary']['stq'] == json.loads(json.dumps(want['stq']))
    # a ground-truth frame that was not predicted ends the run, naming it
    os.remove(os.path.join(out, 'seq_b', 'pan_2ch', names[4]))
    with pytest.raises(SystemExit, match='seq_b has ground truth for frame f_000020.png, which was not predicted'):
        video_eval.main(['--pred', out, '--video_gt', str(gt), '--panoptic_categories', cats])
