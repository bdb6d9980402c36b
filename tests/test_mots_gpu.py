"""GPU: the MOTS measures of tracked sequences on the device (csrc/mots_eval.hip, dataset/mots.py). MOTSEvaluator against
the plain numpy restatement of the rule (tests/mots_ref.py): every integer equal and the float64 soft words bit-equal, on poisoned and
guard-banded memory (tests/memguard.py, patterns A and B, and an unaligned base pointer). Then the limits, the workspace contract, the
run-length kernel behind the text format, and the commands."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import memguard       # noqa: E402
import mots_ref as ref   # noqa: E402
import video_pq_ref as vref   # noqa: E402

pytestmark = pytest.mark.gpu

GUARDED = memguard.MODULES + ('upsnet_amd.dataset.mots',)


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


def device_run(sequences, categories, pattern=None, unaligned=False, **kw):
    """(raw(), summary(), evaluator) of a fresh evaluator; with a pattern, on poisoned allocations and banded inputs."""
    from upsnet_amd.dataset.mots import MOTSEvaluator

    def run():
        ev = MOTSEvaluator(categories, **kw)
        feed(ev, sequences, pattern, unaligned)
        raw = ev.raw()
        return raw, ev.summary(), ev
    if pattern is None:
        return run()
    with memguard.poisoned(pattern, modules=GUARDED) as guard:
        out = run()
        assert_fenced(guard, out[2])
    return out


OUTPUTS = 5     # what the kernels write: the workspace, counts, soft, mtl, status


def assert_fenced(guard, *evaluators):
    """Every buffer the MOTS kernels write came from the guard: poisoned before it was zeroed, between bands that the guard's exit
    checks. (An evaluator that never saw a frame allocates nothing.)"""
    live = [ev for ev in evaluators if ev.workspace() is not None]
    assert guard.count >= OUTPUTS * len(live), (guard.count, len(live))
    sites = ' '.join(site for _, _, _, site in guard.records)
    assert 'mots.py' in sites
    for ev in live:
        fenced = {buf.data_ptr() + memguard.GUARD for buf, _, _, _ in guard.records}
        for t in (ev.workspace(), ev._state['counts'], ev._state['soft'], ev._state['mtl'], ev._state['status']):
            assert t.data_ptr() in fenced, 'a kernel output was not allocated through the guard'


def ref_run(sequences, categories):
    ev = ref.RefMOTSEvaluator(categories)
    for preds, gts, infos in sequences:
        ev.add_sequence(preds, gts, infos)
    return ev


def words(x):
    return np.asarray(x, np.float64).view(np.int64)


def assert_equal_to_ref(raw, summary, want):
    for name in ref.COUNTS:
        exp = want.vector(name)
        assert raw[name].dtype == np.int64 and np.array_equal(raw[name], exp), '%s: categories %s\n%s\n%s' % (
            name, np.nonzero(raw[name] - exp)[0], raw[name][np.nonzero(raw[name] - exp)[0]], exp[np.nonzero(raw[name] - exp)[0]])
    assert raw['soft'].dtype == np.float64 and np.array_equal(words(raw['soft']), words(want.vector('soft'))), 'soft words'
    assert sorted(summary['per_class']) == want.things
    for c in want.things:
        fig = want.figures(c)
        for k, v in fig.items():
            assert summary['per_class'][c][k] == v, (c, k)
    assert summary['mean'] == want.mean()
    assert summary['sequences'] == want.sequences and summary['frames'] == want.frames


def check(sequences, categories=ref.CATEGORIES, patterns='AB', unaligned=False, **kw):
    want = ref_run(sequences, categories)
    out = None
    for p in patterns:
        raw, summary, ev = device_run(sequences, categories, p, unaligned, **kw)
        assert_equal_to_ref(raw, summary, want)
        out = (raw, summary, ev)
    return want, out


# ------------------------------------------------------------------------------------------------ hand-worked cases (tests/test_mots_cpu.py)
def test_hand_cases_equal_the_restatement():
    seg = ref.seg
    cases = [ref.strip_case([[(1, 1, 0, 3), (2, 4, 6, 8)]] * 3, [[(7, 0, 3), (8, 6, 8)]] * 3, [seg(7, 1), seg(8, 2)]),
             ref.strip_case([[(1, 1, 0, 3)], [(1, 1, 0, 3)], [(1, 2, 0, 3)], [(1, 2, 0, 3)]], [[(7, 0, 3)]] * 4, [seg(7, 1)]),
             ref.strip_case([[(1, 1, 0, 3)], [], [(1, 2, 0, 3)]], [[(7, 0, 3)], [], [(7, 0, 3)]], [[seg(7, 1)], [], [seg(7, 1)]]),
             ref.strip_case([[(1, 1, 0, 3)], [], [(1, 1, 0, 3)]], [[(7, 0, 3)]] * 3, [seg(7, 1)]),
             ref.strip_case([[(1, 1, 0, 1)]], [[(7, 0, 3)]], [seg(7, 1)]),
             ref.strip_case([[(1, 1, 0, 2)]], [[(7, 0, 3)]], [seg(7, 1)]),
             ref.strip_case([[(1, 1, 0, 3)]], [[(0, 0, 1)]], []),
             ref.strip_case([[(1, 1, 0, 3)]], [[(0, 0, 2)]], []),
             ref.strip_case([[(1, 1, 0, 3), (1, 5, 6, 9)]], [[(3, 0, 3), (4, 6, 9)]], [seg(3, 1, crowd=1), seg(4, 2, crowd=1)]),
             ref.strip_case([[(2, 1, 0, 3)]], [[(6, 0, 3)]], [seg(6, 1)])]
    # the coverage boundaries: objects tracked in 5, 4, 1, 0 of 5 frames (MT, PT at exactly 0.8, PT at exactly 0.2, ML), then in 5 and 1
    # of 6 frames (MT just above 0.8, ML just below 0.2): the strict inequalities of the end-of-sequence kernel
    gt = [(1, 0, 1), (2, 3, 4), (3, 6, 7), (4, 9, 10)]
    segs = [seg(g, 1) for g in (1, 2, 3, 4)]
    cases.append(ref.strip_case([[(1, 1, 0, 1)] + ([(1, 2, 3, 4)] if t < 4 else []) + ([(1, 3, 6, 7)] if t == 2 else []) for t in range(5)],
                                [gt] * 5, segs))
    cases.append(ref.strip_case([([(1, 1, 0, 1)] if t != 3 else []) + ([(1, 2, 3, 4)] if t == 5 else []) for t in range(6)], [gt[:2]] * 6, segs[:2]))
    for case, mtl in zip(cases[-2:], ((1, 2, 1), (1, 0, 1))):
        one = device_run([case], ref.CATEGORIES)[0]
        assert (one['mt'][1], one['pt'][1], one['ml'][1]) == mtl
    want, (raw, summary, _) = check(cases)
    # the sums of the counts written out case by case in tests/test_mots_cpu.py
    assert (raw['tp'][1], raw['fp'][1], raw['fn'][1], raw['gt_masks'][1], raw['ids'][1], raw['frag'][1], raw['fp_ignored'][1]) == (28, 3, 19, 47, 2, 2, 2)
    assert (raw['tp'][2], raw['fp'][2], raw['mt'][1], raw['pt'][1], raw['ml'][1], raw['mt'][2]) == (3, 1, 6, 3, 4, 1)
    assert raw['soft'][1] == 27.75 and raw['soft'][2] == 3.0
    single = device_run(cases[:1], ref.CATEGORIES)[1]
    assert single['mean'] == {'smotsa': 1.0, 'motsa': 1.0, 'motsp': 1.0, 'recall': 1.0, 'precision': 1.0, 'n': 2}


# ------------------------------------------------------------------------------------------------ random blobs
@pytest.mark.parametrize('H,W', [(1, 1), (1, 67), (67, 1), (37, 53), (48, 64)])
def test_blobs_equal_the_restatement(H, W):
    """Two sequences of 6 frames (drifting rectangles of 3 thing and 2 stuff categories, a crowd segment, a GT VOID band, an id outside
    the table, pred VOID holes, a wrong-category prediction, an identity switch, a gap and a lost object) into one evaluator."""
    if (H, W) == (48, 64):
        sequences = [ref.blob_sequence(*b[:4], switch_at=b[4]) for b in ref.GPU_BLOBS]
    else:
        sequences = [ref.blob_sequence(100 * H + W, H, W, 6, switch_at=2), ref.blob_sequence(100 * H + W + 1, H, W, 6, switch_at=3)]
    want, _ = check(sequences)
    if (H, W) == (48, 64):
        for name in ('ids', 'frag', 'fp_ignored', 'fp', 'fn', 'mt', 'pt', 'ml'):
            assert sum(getattr(want, name).values()) >= 1, name
    if (H, W) == (37, 53):
        check(sequences, patterns='A', unaligned=True)


# ------------------------------------------------------------------------------------------------ limits
def dominoes(H, W, n, frames, cat=6):
    """n instances of one category as 1 x 2 dominoes; the prediction slides one pixel to the right in the odd frames, and the first
    object is predicted under instance number 0 from frame 3 on (all of 1..255 are taken; a hypothesis is a key whatever its j)."""
    cols = W // 3
    assert n <= cols * (H // 2) and n <= 255
    preds, gts, infos = [], [], []
    for t in range(frames):
        p, g = vref.blank_pred(H, W), vref.blank_gt(H, W)
        for k in range(n):
            y, x = 2 * (k // cols), 3 * (k % cols)
            vref.put_gt(g, 1000 + k, y, y, x, x + 1)
            vref.put_pred(p, cat, 0 if (k == 0 and t >= 3) else k + 1, y, y, x + (t & 1), x + 1 + (t & 1))
        preds.append(p)
        gts.append(g)
        infos.append([ref.seg(1000 + k, cat) for k in range(n)])
    return preds, gts, infos


def test_255_instances_of_one_category():
    """In the even frames all 255 match; in the odd ones the prediction covers half of each object: no match, 255 FN and 255 FP."""
    want, _ = check([dominoes(37, 53, 255, 5)], categories={6: {'id': 6, 'isthing': 1}})
    assert want.tp[6] == 3 * 255 and want.fn[6] == 2 * 255 and want.fp[6] == 2 * 255 and want.frag[6] == 2 * 255 and want.pt[6] == 255
    assert want.ids[6] == 1


def test_81_categories_at_once():
    H, W, frames = 37, 53, 4
    cats = {c: {'id': c, 'isthing': int(c % 3 != 0)} for c in range(81)}
    preds, gts, infos = [], [], []
    for t in range(frames):
        p, g = vref.blank_pred(H, W), vref.blank_gt(H, W)
        for c in range(81):
            y, x = 2 * (c // 13), 4 * (c % 13)
            vref.put_gt(g, 100 + c, y, y + 1, x, x + 2)
            vref.put_pred(p, c, 0 if c % 3 == 0 else 1 + (t > 1 and c == 7), y, y + 1, x + (c & 1) * (t & 1), x + 2)
        preds.append(p)
        gts.append(g)
        infos.append([ref.seg(100 + c, c) for c in range(81)])
    want, _ = check([(preds, gts, infos)], categories=cats)
    assert len(want.tp) == 54 and want.ids == {7: 1}


def test_gt_id_of_2_to_the_24_minus_1():
    top = (1 << 24) - 1
    case = ref.strip_case([[(1, 1, 0, 3), (1, 2, 5, 9)]] * 2, [[(top, 0, 3), (top - 1, 5, 8)]] * 2, [ref.seg(top, 1), ref.seg(top - 1, 1)])
    want, _ = check([case])
    assert want.tp[1] == 4 and abs(want.soft[1] - 3.6) < 1e-12        # IoU 1 and 4 / 5, twice


def test_sequence_with_zero_scored_frames():
    from upsnet_amd.dataset.mots import MOTSEvaluator
    a = ref.blob_sequence(5, 37, 53, 3, switch_at=1)
    ev = MOTSEvaluator(ref.CATEGORIES)
    ev.begin_sequence([])
    ev.end_sequence()
    feed(ev, [a])
    ev.begin_sequence(a[2][:1])
    ev.end_sequence()
    want = ref_run([a], ref.CATEGORIES)
    want.sequences = 3
    assert_equal_to_ref(ev.raw(), ev.summary(), want)
    assert not bool(ev.workspace().any())


def noise_frames(bh, bw, frames=2):
    """64 x 64, every bh x bw tile its own (GT segment, pred key) pair of a thing category (256 pairs per category)."""
    per = 64 // bw
    n = per * (64 // bh)
    idx = (np.arange(64)[:, None] // bh) * per + np.arange(64)[None, :] // bw
    preds, gts, infos = [], [], []
    for t in range(frames):
        p, g = vref.blank_pred(64, 64), vref.blank_gt(64, 64)
        k = idx if t == 0 else np.roll(idx, bw, 1)
        p[:, :, 0], p[:, :, 1] = k // 256, k % 256
        gid = idx + 1
        g[:, :, 0], g[:, :, 1] = gid & 255, gid >> 8
        preds.append(p)
        gts.append(g)
        infos.append([ref.seg(i + 1, i // 256) for i in range(n)])
    return preds, gts, infos, {c: {'id': c, 'isthing': 1} for c in range(max(n // 256, 1))}


def test_noise_like_frames_are_exact_or_refused():
    """512 objects under 512 keys are 1536 cells (area of the row, area of the key, their joint cell) in a frame table of 4096 slots
    (64 x 64), a load of 3 / 8: required exact -- at that load a linear-probing table is far from a cluster of the 256 slots a probe
    walks, whatever the hash. 1024 of each are 3072 cells, a load of 3 / 4, and 4096 of each (every pixel its own) are more cells than
    the table has slots: there a cluster may or must exceed the probe length, so either the result is exact or the documented
    RuntimeError is raised, never a wrong count."""
    preds, gts, infos, cats = noise_frames(2, 4)
    want, _ = check([(preds, gts, infos)], categories=cats)
    assert sum(want.tp.values()) == 1024 and sum(want.ids.values()) == 512
    for block in (2, 1):
        preds, gts, infos, cats = noise_frames(block, block)
        try:
            raw, summary, _ = device_run([(preds, gts, infos)], cats, 'A')
        except RuntimeError as e:
            assert 'was full' in str(e) and 'counts were dropped' in str(e)
        else:
            assert_equal_to_ref(raw, summary, ref_run([(preds, gts, infos)], cats))


def test_unknown_category_is_a_key_error_naming_the_place():
    from upsnet_amd.dataset.mots import MOTSEvaluator
    preds, gts, infos = ref.blob_sequence(5, 37, 53, 4)
    bad = [p.copy() for p in preds]
    bad[2][0, 0, 0], bad[2][0, 0, 1] = 37, 1
    bad[3][0, 0, 0], bad[3][0, 0, 1] = 36, 1
    ev = MOTSEvaluator(ref.CATEGORIES)
    feed(ev, [(preds, gts, infos)])
    ev.begin_sequence(infos, name='street')
    for p, g in zip(bad, gts):
        ev.add_frame(p, g)
    with pytest.raises(KeyError, match='sequence street .index 1 in the order added. frame 2 a segment has unknown category_id 37'):
        ev.summary()


# ------------------------------------------------------------------------------------------------ the workspace contract
def test_workspace_is_zero_again_and_a_second_sequence_scores_as_on_a_fresh_evaluator():
    from upsnet_amd.dataset.mots import MOTSEvaluator
    a, b = ref.blob_sequence(21, 37, 53, 6, switch_at=2), ref.blob_sequence(22, 37, 53, 5, switch_at=1)
    with memguard.poisoned('A', modules=GUARDED) as guard:
        ev = MOTSEvaluator(ref.CATEGORIES)
        feed(ev, [a], 'A')
        ws = ev.workspace()
        assert ws is not None and ws.numel() > 0 and not bool(ws.any()), 'the workspace is not zero after end_sequence'
        first = ev.raw()
        feed(ev, [b], 'A')
        assert ev.workspace() is ws and not bool(ws.any())
        both = ev.raw()
        fresh = MOTSEvaluator(ref.CATEGORIES)
        feed(fresh, [b], 'A')
        alone = fresh.raw()
        assert_fenced(guard, ev, fresh)
    for k in ref.COUNTS:
        assert np.array_equal(both[k] - first[k], alone[k]), k
    assert_equal_to_ref(both, ev.summary(), ref_run([a, b], ref.CATEGORIES))


def test_a_used_evaluator_takes_sequences_of_other_sizes_like_a_fresh_one():
    """One evaluator over 65 x 129, 37 x 53 and 65 x 129 again (other content; the workspace is replaced at each change of size, the
    accumulators and the status are kept): after every sequence the integer counts it added are those of a fresh evaluator on that
    sequence alone, bit for bit, and the totals -- the float64 soft sum included -- are the restatement's over all three."""
    from upsnet_amd.dataset.mots import MOTSEvaluator
    seqs = [ref.blob_sequence(41, 65, 129, 4, switch_at=2), ref.blob_sequence(42, 37, 53, 5, switch_at=1), ref.blob_sequence(43, 65, 129, 3, switch_at=1)]
    ev = MOTSEvaluator(ref.CATEGORIES)
    before = ev.raw()
    for k, seq in enumerate(seqs):
        feed(ev, [seq])
        assert not bool(ev.workspace().any()) and tuple(ev._ws_shape) == seq[0][0].shape[:2]
        after = ev.raw()
        fresh = MOTSEvaluator(ref.CATEGORIES)
        feed(fresh, [seq])
        alone = fresh.raw()
        for name in ref.COUNTS + ('mt', 'pt', 'ml'):
            assert np.array_equal(after[name] - before[name], alone[name]), (k, name)
        if k == 0:
            assert np.array_equal(words(after['soft']), words(alone['soft']))
        before = after
    assert_equal_to_ref(ev.raw(), ev.summary(), ref_run(seqs, ref.CATEGORIES))


def test_refusals_leave_the_state_untouched():
    from upsnet_amd.dataset.mots import MOTSEvaluator
    preds, gts, infos = ref.blob_sequence(31, 37, 53, 5, switch_at=2)
    ev = MOTSEvaluator(ref.CATEGORIES)
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
    assert not bool(ev.workspace().any())
    assert_equal_to_ref(ev.raw(), ev.summary(), ref_run([(preds, gts, infos)], ref.CATEGORIES))


# ------------------------------------------------------------------------------------------------ the run-length kernel
def rle_maps():
    blobs = ref.blob_sequence(9, 37, 53, 2, switch_at=1)[0]
    edge = vref.blank_pred(5, 7)
    vref.put_pred(edge, 3, 9, 0, 4, 0, 0)         # the whole first column, pixel 0 included
    edge[4, 6] = (3, 9, 0)                        # ... and the last pixel: a run that ends at H * W
    edge[2, 3] = (4, 1, 0)                        # a single-pixel segment
    edge[4, 2] = (5, 2, 0)                        # a run across the wrap from one column's last pixel
    edge[0, 3] = (5, 2, 0)                        # to the next column's first
    edge[1, 5] = (200, 0, 0)                      # instance 0: no thing segment
    stuff = vref.blank_pred(4, 9)
    vref.put_pred(stuff, 200, 0, 0, 3, 0, 4)
    one = vref.blank_pred(1, 1)
    one[0, 0] = (7, 255, 0)
    thing = (blobs[0][:, :, 0] != 255) & (blobs[0][:, :, 1] != 0)
    r, c = int(thing.sum(1).argmax()), int(thing.sum(0).argmax())     # the row and the column with the most thing pixels
    return {'blob0': blobs[0], 'blob1': blobs[1], 'edge': edge, 'no_thing': stuff, 'one_pixel': one, 'row': blobs[0][r:r + 1].copy(),
            'column': blobs[0][:, c:c + 1].copy()}


@pytest.mark.parametrize('name', sorted(rle_maps()))
def test_rle_transitions_equal_numpy(name):
    from upsnet_amd.dataset.mots import segment_transitions
    pan = rle_maps()[name]
    want = sorted(k << 24 | p for k, mask in ref.thing_segments(pan).items() for p in ref.transitions(mask))
    assert len(want) == {'no_thing': 0, 'one_pixel': 1, 'edge': 7}.get(name, len(want)) and (len(want) > 2 or name in ('no_thing', 'one_pixel'))
    for pattern in 'AB':
        with memguard.poisoned(pattern, modules=GUARDED) as guard:
            got = segment_transitions(on_device(pan, pattern, unaligned=(pattern == 'B')))
            assert got.dtype == torch.int64 and got.cpu().tolist() == want, name
            assert guard.count == 2            # the pair buffer and the count came poisoned and fenced
            if len(want) > 1:      # a buffer that is too small: the count comes back whole and the call is repeated
                assert segment_transitions(on_device(pan, pattern), cap=1).cpu().tolist() == want
                assert segment_transitions(on_device(pan, pattern), cap=0).cpu().tolist() == want
                assert guard.count == 10
    if name == 'edge':
        segs = ref.thing_segments(pan)
        assert ref.rle_counts(segs[3 << 8 | 9]) == [0, 5, 29, 1] and ref.rle_counts(segs[5 << 8 | 2]) == [14, 2, 19]


def test_write_mots_txt_equals_the_restated_lines(tmp_path):
    from upsnet_amd.dataset.mots import read_mots_txt, write_mots_txt
    from upsnet_amd.dataset.rle import rle_to_string
    maps = ref.blob_sequence(9, 37, 53, 3, switch_at=1)[0]
    path = str(tmp_path / 'mots.txt')
    n = write_mots_txt(path, [maps[0], torch.from_numpy(maps[1]).cuda(), maps[2]])
    with open(path) as f:
        lines = f.read().splitlines()
    assert lines == ref.mots_lines(maps, rle_to_string) and n == len(lines) > 10
    gts, _ = read_mots_txt(path)
    for m, g in zip(maps, gts):
        for k, mask in ref.thing_segments(m).items():
            assert np.all(ref.gt_ids(g)[mask] == (k >> 8) * 1000 + (k & 255))


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
    cfg = write_cfg(tmp_path, 'Cityscapes', str(tmp_path / 'data'), 'val')
    cats = str(tmp_path / 'cats.json')
    with open(cats, 'w') as f:
        json.dump({'categories': list(ref.CATEGORIES.values())}, f)
    raw = tmp_path / 'raw'
    names = ['f_%06d.png' % (5 * k) for k in range(5)]
    for seq, seed in (('seq_a', 41), ('seq_b', 42)):
        os.makedirs(str(raw / seq))
        preds, _, _ = vref.blob_sequence(seed, 48, 64, 5)
        for n, p in zip(names, preds):
            Image.fromarray(p).save(str(raw / seq / n))
    base = ['--cfg', cfg, '--panoptic_categories', cats, '--track_max_age', '1']
    # --write_mots adds mots.txt to every sequence folder and nothing else
    out = str(tmp_path / 'out')
    res = sequence.main(base + ['--track_only', str(raw), '--out', out, '--write_mots'])
    assert sorted(res) == ['sequences'] and sorted(os.listdir(out)) == ['seq_a', 'seq_b']
    assert sorted(os.listdir(os.path.join(out, 'seq_a'))) == ['mots.txt', 'pan', 'pan_2ch', 'pred.json', 'tracks.json']
    # the re-scoring command writes the same files from the written maps, with no ground truth and no category table
    written = {seq: open(os.path.join(out, seq, 'mots.txt')).read() for seq in ('seq_a', 'seq_b')}
    for seq in written:
        os.remove(os.path.join(out, seq, 'mots.txt'))
    assert video_eval.main(['--pred', out, '--write_mots']) is None and sorted(os.listdir(out)) == ['seq_a', 'seq_b']
    assert {seq: open(os.path.join(out, seq, 'mots.txt')).read() for seq in written} == written and len(written['seq_a']) > 100
    # re-scored against its own text files: every hypothesis is an object's mask
    txt = tmp_path / 'txt'
    os.makedirs(str(txt))
    for seq in ('seq_a', 'seq_b'):
        with open(os.path.join(out, seq, 'mots.txt')) as f, open(str(txt / (seq + '.txt')), 'w') as g:
            g.write(f.read())
    scores = video_eval.main(['--pred', out, '--mots_gt', str(txt), '--panoptic_categories', cats])
    assert scores['sequences'] == 2 and scores['frames'] == 10 and scores['mean']['n'] >= 2 and scores['mean']['motsa'] == 1.0
    present = [c for c, r in scores['per_class'].items() if r['gt_masks'] > 0]
    assert len(present) >= 2
    for c in present:
        r = scores['per_class'][c]
        assert r['motsa'] == 1.0 and r['ids'] == 0 and r['fp'] == 0 and r['fn'] == 0 and r['smotsa'] == 1.0 and r['tp'] == r['gt_masks']
    assert sorted(os.listdir(out)) == ['mots_scores.json', 'seq_a', 'seq_b']
    written = json.load(open(os.path.join(out, 'mots_scores.json')))
    assert written['sequences'] == [{'name': 'seq_a', 'frames': 5}, {'name': 'seq_b', 'frames': 5}]
    assert written['summary']['mean'] == scores['mean'] and written['mots_gt'] == str(txt)
    os.remove(os.path.join(out, 'mots_scores.json'))
    # the same through the sequence command
    out2 = str(tmp_path / 'out2')
    res = sequence.main(base + ['--track_only', str(raw), '--out', out2, '--mots_gt', str(txt)])
    assert res['mots_scores']['per_class'] == scores['per_class'] and 'video_scores' not in res
    assert sorted(os.listdir(out2)) == ['mots_scores.json', 'seq_a', 'seq_b']
    assert sorted(os.listdir(os.path.join(out2, 'seq_a'))) == ['pan', 'pan_2ch', 'pred.json', 'tracks.json']
    # --video_gt with and without --eval_mots: 'mots' is added and nothing else changes
    plain = video_eval.main(['--pred', out, '--video_gt', out, '--panoptic_categories', cats, '--out', str(tmp_path / 'plain.json')])
    both = video_eval.main(['--pred', out, '--video_gt', out, '--panoptic_categories', cats, '--out', str(tmp_path / 'both.json'), '--eval_mots'])
    assert 'mots' not in plain and sorted(set(both) - set(plain)) == ['mots']
    a, b = json.load(open(str(tmp_path / 'plain.json'))), json.load(open(str(tmp_path / 'both.json')))
    mots = b['summary'].pop('mots')
    assert a == b and sorted(mots) == ['frames', 'mean', 'per_class', 'sequences', 'total']
    assert mots['mean']['motsa'] == 1.0 and mots['total']['ids'] == 0 and mots['total']['fp'] == 0 and mots['total']['tp'] > 10
    assert not os.path.exists(os.path.join(out, 'mots_scores.json')) and not os.path.exists(os.path.join(out, 'video_scores.json'))
    out3 = str(tmp_path / 'out3')
    res = sequence.main(base + ['--track_only', str(raw), '--out', out3, '--video_gt', out, '--eval_mots'])
    assert res['video_scores']['mots']['per_class'] == both['mots']['per_class']
    assert sorted(os.listdir(out3)) == ['seq_a', 'seq_b', 'video_scores.json']
    assert sorted(json.load(open(os.path.join(out3, 'video_scores.json')))['summary']) == sorted(list(plain) + ['mots'])
