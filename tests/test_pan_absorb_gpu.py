"""GPU: small panoptic fragments absorbed into the segment they border most (csrc/pan_components.hip via ops.pan_absorb,
dataset.clean_panoptic(mode='absorb') and --pan_component_mode absorb) against the restatements of tests/pan_absorb_ref.py. Every
comparison is a byte or integer equality. Every table case runs twice, with workspace, output and label map taken from poisoned,
guard-banded memory of pattern A and then B: the kernels must initialise what they read and write nothing outside their buffers. The
vote table is sized from the bound on the pairs, so no case can fill it: stats[7] is 0 everywhere."""
import copy
import json
import os

import numpy as np
import pytest
import torch

import memguard
import pan_absorb_ref as aref
import pan_components_ref as ref

pytestmark = pytest.mark.gpu

CASES = ref.cases() + aref.cases()
_WANT = {}


def want(name, pan, min_area, conn, keep):
    """The restatement's answer, computed once per (case, connectivity) and never changed: the vectorised path (tests/
    test_pan_absorb_cpu.py holds the two paths together)."""
    if (name, conn) not in _WANT:
        _WANT[name, conn] = aref.absorb_vec(pan, min_area, conn, keep)
    return _WANT[name, conn]


def case(name):
    return CASES[[c[0] for c in CASES].index(name)]


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture()
def saved_config():
    from upsnet_amd.config.config import config
    saved = copy.deepcopy(dict(config))
    yield config
    config.clear()
    config.update(saved)


def run_poisoned(pan, min_area, conn, keep, pattern):
    from upsnet_amd import ops
    from upsnet_amd._lib import lib
    H, W = pan.shape[:2]
    with memguard.poisoned(pattern, modules=()) as g:
        ws = g.empty((int(lib().upsnet_pan_absorb_workspace_bytes(H, W)),), dtype=torch.uint8, device='cuda')
        out = g.empty((H, W, 3), dtype=torch.uint8, device='cuda')
        labels = g.empty((H, W), dtype=torch.int32, device='cuda')
        src = memguard.banded_copy(cuda(pan), pattern)
        got = ops.pan_absorb(src, min_area, conn, keep, workspace=ws, out=out, labels=labels)
        assert got[0] is out and got[2] is labels and got[1].dtype == torch.int32 and got[1].is_cuda and tuple(got[1].shape) == (8,)
        res = out.cpu().numpy(), labels.cpu().numpy(), got[1].cpu().numpy()
        assert np.array_equal(src.cpu().numpy(), pan)                   # the input is not written
    assert g.count == 3
    return res


@pytest.mark.parametrize('conn', [4, 8])
@pytest.mark.parametrize('case', CASES, ids=[c[0] for c in CASES])
def test_table_case_bit_for_bit_under_both_poisons(case, conn):
    name, pan, min_area, keep = case
    exp = want(name, pan, min_area, conn, keep)
    a = run_poisoned(pan, min_area, conn, keep, 'A')
    b = run_poisoned(pan, min_area, conn, keep, 'B')
    assert a[2][7] == 0, "%s: the vote table overflowed" % name
    for what, x, y, e in zip(('out', 'labels', 'stats'), a, b, exp):
        assert x.dtype == e.dtype and x.shape == e.shape, (name, what)
        assert np.array_equal(x, y), "%s: %s differs between the poison patterns" % (name, what)
        assert np.array_equal(x, e), "%s: %s differs from the restatement (%d elements)" % (name, what, int((x != e).sum()))


def test_defaults_allocate_and_only_label():
    from upsnet_amd import ops
    _, pan, _, _ = case('tiles_2x3_plus')
    src = cuda(pan)
    out, stats, labels = ops.pan_absorb(src)
    assert labels is None and out.data_ptr() != src.data_ptr() and torch.equal(out, src)             # min_area 0: the identity
    exp = aref.absorb_vec(pan, 0, 8, True)
    assert stats.cpu().numpy().tolist() == exp[2].tolist() and exp[2][2:].tolist() == [0] * 6
    out, stats, labels = ops.pan_absorb(src, 6, 4, False, want_labels=True)
    exp = aref.absorb_vec(pan, 6, 4, False)
    assert np.array_equal(out.cpu().numpy(), exp[0]) and np.array_equal(labels.cpu().numpy(), exp[1])
    assert np.array_equal(stats.cpu().numpy(), exp[2]) and exp[2][4] > 0
    for bad in (dict(workspace=ops.pan_components_workspace(pan.shape[0], pan.shape[1], 'cuda')),    # the void mode's is too small
                dict(out=torch.zeros((3, 3, 3), dtype=torch.uint8, device='cuda')),
                dict(labels=torch.zeros(pan.shape[:2], dtype=torch.int64, device='cuda')), dict(connectivity=5), dict(min_area=-2)):
        with pytest.raises(ValueError, match='pan_absorb'):
            ops.pan_absorb(src, **bad)


def test_differs_from_the_void_mode_on_the_absorbed_pixels_and_is_a_fixed_point():
    from upsnet_amd import ops
    for name in ('absorb_70x300', 'absorb_70x300_all', 'seam_cross', 'stripes'):
        _, pan, min_area, keep = case(name)
        for conn in (4, 8):
            src = cuda(pan)
            out, stats, _ = ops.pan_absorb(src, min_area, conn, keep)
            void, vstats, _ = ops.pan_components(src, min_area, conn, keep)
            assert torch.equal(stats[:4], vstats) and int(stats[5]) > 0
            differs = (out != void).any(-1)
            assert int(differs.sum()) == int(stats[5]) and bool((void[differs][:, 0] == 255).all()) and bool((out[differs][:, 0] != 255).all())
            again, s2, _ = ops.pan_absorb(out, min_area, conn, keep)
            assert torch.equal(again, out) and s2[2:].tolist() == [0] * 6


def test_in_place():
    from upsnet_amd import ops
    for name in ('tiles_2x3_plus', 'random_131x257', 'odd_37x53', 'seam_cross', 'long_fragment'):
        _, pan, min_area, keep = case(name)
        for conn in (4, 8):
            exp = want(name, pan, min_area, conn, keep)
            buf = cuda(pan)
            out, stats, labels = ops.pan_absorb(buf, min_area, conn, keep, out=buf, want_labels=True)
            assert out is buf and np.array_equal(buf.cpu().numpy(), exp[0]) and not np.array_equal(exp[0], pan)
            assert np.array_equal(labels.cpu().numpy(), exp[1]) and np.array_equal(stats.cpu().numpy(), exp[2])


def test_unaligned_base_pointer_and_width():
    """Maps that start 3 bytes into their allocation: one with H * W and W multiples of 16, one with W % 16 != 0, where a thread's 16
    pixels run over the end of a row. The input is read-only and is handed on as an aligned copy; an output that starts there is
    refused before any launch, so the kernels' byte path for such bases is no longer reached from Python."""
    from upsnet_amd import ops
    rng = np.random.default_rng(91)
    for H, W in ((40, 160), (40, 157)):
        pan = ref.blobs(rng, H, W, 11, ref.KEYS, 0.03)
        exp = aref.absorb_vec(pan, 4, 8, True)
        assert exp[2][4] > 0
        src = cuda(np.concatenate([pan.reshape(-1, 3)[:1], pan.reshape(-1, 3)]))[1:].view(H, W, 3)
        dst = torch.zeros((H * W + 1, 3), dtype=torch.uint8, device='cuda')[1:].view(H, W, 3)
        assert src.data_ptr() % 16 and dst.data_ptr() % 16 and src.is_contiguous()
        with pytest.raises(ValueError, match='aligned'):
            ops.pan_absorb(src, 4, 8, True, out=dst)
        assert not dst.any()
        out, stats, _ = ops.pan_absorb(src, 4, 8, True)
        assert np.array_equal(out.cpu().numpy(), exp[0]) and np.array_equal(stats.cpu().numpy(), exp[2])
        assert np.array_equal(src.cpu().numpy(), pan)
        out, stats, _ = ops.pan_absorb(cuda(pan), 4, 8, True)           # and aligned: the 16-byte path of the same map
        assert np.array_equal(out.cpu().numpy(), exp[0]) and np.array_equal(stats.cpu().numpy(), exp[2])


def test_reused_workspace():
    """One workspace across different maps of one size and then a smaller size: as with a fresh workspace each time."""
    from upsnet_amd import ops
    rng = np.random.default_rng(92)
    a = ref.blobs(rng, 70, 300, 13, ref.KEYS, 0.03)
    b = ref._random(rng, 70, 300, ref.KEYS)
    c = ref.blobs(rng, 37, 53, 5, ref.KEYS, 0.05)
    d = aref.stripes(70, 300)                                            # fills most of the table; the next map must not see it
    ws = ops.pan_absorb_workspace(70, 300, 'cuda')
    for pan in (a, d, b, a, c, d, b):
        got = ops.pan_absorb(cuda(pan), 3, 8, True, want_labels=True, workspace=ws)
        fresh = ops.pan_absorb(cuda(pan), 3, 8, True, want_labels=True)
        exp = aref.absorb_vec(pan, 3, 8, True)
        for x, y, e in zip((got[0], got[2], got[1]), (fresh[0], fresh[2], fresh[1]), exp):
            assert torch.equal(x, y) and np.array_equal(x.cpu().numpy(), e)


def test_byte_2_is_preserved_and_never_read():
    from upsnet_amd import ops
    rng = np.random.default_rng(93)
    pan = ref.blobs(rng, 45, 133, 6, ref.KEYS, 0.05)
    pan[..., 2] = rng.integers(0, 256, pan.shape[:2])
    other = pan.copy()
    other[..., 2] = rng.integers(0, 256, pan.shape[:2])
    for conn in (4, 8):
        out, stats, _ = ops.pan_absorb(cuda(pan), 5, conn, True)
        out2, stats2, _ = ops.pan_absorb(cuda(other), 5, conn, True)
        out, out2 = out.cpu().numpy(), out2.cpu().numpy()
        assert np.array_equal(out[..., 2], pan[..., 2]) and np.array_equal(out2[..., 2], other[..., 2])
        assert np.array_equal(out[..., :2], out2[..., :2]) and torch.equal(stats, stats2)
        assert np.array_equal(out, aref.absorb_vec(pan, 5, conn, True)[0]) and int(stats[5]) > 0


def test_clean_panoptic_and_the_dataset_method(saved_config, caplog):
    import logging
    from upsnet_amd.dataset import clean_panoptic
    from upsnet_amd.dataset.base_dataset import BaseDataset
    rng = np.random.default_rng(94)
    pans = [ref.blobs(rng, 60, 90, 7, ref.KEYS, 0.04), ref.blobs(rng, 60, 90, 7, ref.KEYS, 0.04), ref.blobs(rng, 41, 50, 5, ref.KEYS, 0.04)]
    given = [pans[0], cuda(pans[1]), pans[2]]                          # numpy arrays are uploaded
    got = clean_panoptic(given, 4, connectivity=4, keep_largest=False, mode='absorb')
    exp = [aref.absorb_vec(p, 4, 4, False) for p in pans]
    assert all(g.is_cuda and np.array_equal(g.cpu().numpy(), e[0]) for g, e in zip(got, exp))
    assert np.array_equal(given[1].cpu().numpy(), pans[1])              # the inputs are untouched
    _, total = clean_panoptic(given, 4, connectivity=4, keep_largest=False, return_stats=True, mode='absorb')
    assert tuple(total.shape) == (8,) and total.cpu().numpy().tolist() == sum(e[2].astype(np.int64) for e in exp).tolist()
    void = clean_panoptic(given, 4, connectivity=4, keep_largest=False)                              # the default mode is the void one
    assert all(np.array_equal(v.cpu().numpy(), ref.clean_flood(p, 4, 4, False)[0]) for v, p in zip(void, pans))
    saved_config.test.pan_min_component, saved_config.test.pan_component_connectivity = 5, 8
    saved_config.test.pan_component_mode = 'absorb'
    with caplog.at_level(logging.INFO):
        got = BaseDataset().clean_pan_result(given)
    exp = [aref.absorb_vec(p, 5, 8, True) for p in pans]
    assert all(np.array_equal(g.cpu().numpy(), e[0]) for g, e in zip(got, exp))
    removed, absorbed = sum(int(e[2][2]) for e in exp), sum(int(e[2][4]) for e in exp)
    assert absorbed > 0 and ('%d of %d connected components' % (removed, sum(int(e[2][1]) for e in exp))) in caplog.text
    assert ('%d of them (%d pixels) absorbed' % (absorbed, sum(int(e[2][5]) for e in exp))) in caplog.text
    caplog.clear()
    with caplog.at_level(logging.INFO):
        got = BaseDataset().clean_pan_result(given, mode='void')
    assert all(np.array_equal(g.cpu().numpy(), ref.clean_flood(p, 5, 8, True)[0]) for g, p in zip(got, pans))
    assert 'connected components' in caplog.text and 'absorbed' not in caplog.text


def test_clean_pan_result_raises_on_a_reported_overflow(saved_config, monkeypatch):
    """The table cannot fill, so the report is made up: clean_pan_result must refuse to hand on maps whose stats[7] is set."""
    from upsnet_amd.dataset import pan_components
    from upsnet_amd.dataset.base_dataset import BaseDataset
    real = pan_components.clean_panoptic

    def overflowed(*a, **kw):
        cleaned, total = real(*a, **kw)
        total[7] = 1
        return cleaned, total
    monkeypatch.setattr(pan_components, 'clean_panoptic', overflowed)
    saved_config.test.pan_min_component, saved_config.test.pan_component_mode = 5, 'absorb'
    with pytest.raises(RuntimeError, match='overflowed'):
        BaseDataset().clean_pan_result([case('odd_37x53')[1]])


def test_sequence_track_only_absorbs_before_it_tracks(tmp_path, saved_config):
    """upsnet_amd.sequence --track_only --pan_min_component N --pan_component_mode absorb writes what the tracker makes of
    clean_panoptic(mode='absorb') of the maps."""
    from PIL import Image
    from test_dataset_run_cpu import write_cfg
    from upsnet_amd import sequence
    from upsnet_amd.dataset import clean_panoptic, track_sequence
    rng = np.random.default_rng(95)
    keys = [(0, 0), (3, 0), (11, 1), (11, 2), (13, 1)]
    maps = [ref.blobs(rng, 60, 90, 15, keys, 0.03) for _ in range(3)]
    raw = tmp_path / 'raw'
    raw.mkdir()
    for k, m in enumerate(maps):
        Image.fromarray(m).save(str(raw / ('f%02d.png' % k)))
    cfg = write_cfg(tmp_path, 'Cityscapes', str(tmp_path / 'data'), 'val')
    cats = str(tmp_path / 'cats.json')
    with open(cats, 'w') as f:
        json.dump({'categories': [{'id': c, 'name': 'c%d' % c, 'isthing': int(c > 10)} for c in range(19)]}, f)
    absorbed = clean_panoptic(maps, 6, connectivity=4, mode='absorb')
    voided = clean_panoptic(maps, 6, connectivity=4)
    assert any(not torch.equal(a, v) for a, v in zip(absorbed, voided))
    out = str(tmp_path / 'out')
    sequence.main(['--cfg', cfg, '--track_only', str(raw), '--out', out, '--panoptic_categories', cats, '--pan_min_component', '6',
                   '--pan_component_connectivity', '4', '--pan_component_mode', 'absorb'])
    assert saved_config.test.pan_component_mode == 'absorb'
    for k, (w_map, _) in enumerate(track_sequence(absorbed)):
        got = np.array(Image.open(os.path.join(out, 'raw', 'pan_2ch', 'f%02d.png' % k)))
        assert np.array_equal(got, w_map.cpu().numpy()), k
    saved_config.test.pan_min_component, saved_config.test.pan_component_mode = 0, 'void'
    with pytest.raises(SystemExit, match='pan_component_mode'):
        sequence.main(['--cfg', cfg, '--track_only', str(raw), '--out', str(tmp_path / 'o'), '--panoptic_categories', cats,
                       '--pan_component_mode', 'absorb'])


def test_evaluate_end_to_end_scores_writes_and_draws_the_absorbed_maps(tmp_path, saved_config):
    """evaluate.main on a generated COCO-layout dataset, without and with --pan_min_component N --pan_component_mode absorb: what the
    second run scores, writes and draws is clean_panoptic(mode='absorb') of the first run's maps. The first run's maps serve as the
    panoptic ground truth, so that the plain maps score 1 and any pixel changed shows in the metrics."""
    from PIL import Image
    from test_dataset_run_cpu import make_dataset, write_cfg
    from test_pan_components_gpu import write_ground_truth, write_panoptic_gt
    from upsnet_amd.config.config import update_config
    from upsnet_amd.dataset import clean_panoptic, coco
    from upsnet_amd.evaluate import main
    N = 200
    root = str(tmp_path / 'coco')
    make_dataset(root, 'coco', [(200, 300), (256, 384)], seed=11)
    cfg = write_cfg(tmp_path, 'coco', root, 'val2017')
    update_config(cfg)
    ds = coco(image_sets=['val2017'], phase='test')
    write_ground_truth(ds, np.random.default_rng(82))

    def read(folder, sub, names):
        return [np.array(Image.open(os.path.join(folder, sub, n))) for n in names]

    plain = main(['--cfg', cfg, '--synthetic_weights', '--write_panoptic'])
    assert saved_config.test.pan_min_component == 0 and saved_config.test.pan_component_mode == 'void'
    out = os.path.join(os.path.dirname(plain['results_file']), 'pans_unified')
    with open(os.path.join(out, 'pred.json')) as f:
        names, ids = zip(*[(a['file_name'], a['image_id']) for a in json.load(f)['annotations']])
    before = read(out, 'pan_2ch', names)
    write_panoptic_gt(ds, before, ids)
    cleaned = clean_panoptic(before, N, mode='absorb')
    voided = clean_panoptic(before, N)
    assert any(not torch.equal(c, v) for c, v in zip(cleaned, voided)), "nothing absorbed: the run shows nothing"
    want_metrics = ds.evaluate_panoptic(cleaned, out)
    assert want_metrics != ds.evaluate_panoptic(voided, out)
    want_pictures = [open(p, 'rb').read() for p in ds.vis_panoptic(cleaned, str(tmp_path / 'want'), mode='flat')]
    res = main(['--cfg', cfg, '--synthetic_weights', '--write_panoptic', '--vis_panoptic', 'flat', '--pan_min_component', str(N),
                '--pan_component_mode', 'absorb'])
    assert saved_config.test.pan_min_component == N and saved_config.test.pan_component_mode == 'absorb'
    assert res['metrics']['panoptic'] == want_metrics                                                                    # scored
    for got, c in zip(read(out, 'pan_2ch', names), cleaned):                                                             # written
        assert np.array_equal(got, c.cpu().numpy())
    pictures = [p for p in res['vis_panoptic_files'] if os.sep + 'vis_flat' + os.sep in p]                               # drawn
    assert len(pictures) == len(want_pictures) == 2
    assert [open(p, 'rb').read() for p in pictures] == want_pictures
