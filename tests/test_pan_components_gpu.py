"""GPU: connected components of 2-channel maps on the device (csrc/pan_components.hip via ops.pan_components, dataset/pan_components.py
and the evaluation's --pan_min_component) against the restatement of tests/pan_components_ref.py. Every comparison is a byte or integer
equality. Every table case runs twice, with workspace, output and label map taken from poisoned, guard-banded memory of pattern A and
then B: the kernels must initialise what they read and write nothing outside their buffers."""
import copy
import json
import os

import numpy as np
import pytest
import torch

import memguard
import pan_components_ref as ref

pytestmark = pytest.mark.gpu

CASES = ref.cases()
_WANT = {}


def want(name, pan, min_area, conn, keep):
    """The restatement's answer, computed once per (case, connectivity) and never changed. The full-size frame takes the scipy path
    (tests/test_pan_components_cpu.py holds the two paths together on every case, that one included)."""
    if (name, conn) not in _WANT:
        fn = ref.clean_scipy if pan.shape[0] * pan.shape[1] > (1 << 18) else ref.clean_flood
        _WANT[name, conn] = fn(pan, min_area, conn, keep)
    return _WANT[name, conn]


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run_poisoned(pan, min_area, conn, keep, pattern):
    from upsnet_amd import ops
    from upsnet_amd._lib import lib
    H, W = pan.shape[:2]
    with memguard.poisoned(pattern, modules=()) as g:
        ws = g.empty((int(lib().upsnet_pan_components_workspace_bytes(H, W)),), dtype=torch.uint8, device='cuda')
        out = g.empty((H, W, 3), dtype=torch.uint8, device='cuda')
        labels = g.empty((H, W), dtype=torch.int32, device='cuda')
        src = memguard.banded_copy(cuda(pan), pattern)
        got = ops.pan_components(src, min_area, conn, keep, workspace=ws, out=out, labels=labels)
        assert got[0] is out and got[2] is labels and got[1].dtype == torch.int32 and got[1].is_cuda
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
    for what, x, y, e in zip(('out', 'labels', 'stats'), a, b, exp):
        assert x.dtype == e.dtype and x.shape == e.shape, (name, what)
        assert np.array_equal(x, y), "%s: %s differs between the poison patterns" % (name, what)
        assert np.array_equal(x, e), "%s: %s differs from the restatement (%d elements)" % (name, what, int((x != e).sum()))


def test_defaults_allocate_and_only_label():
    from upsnet_amd import ops
    _, pan, _, _ = CASES[[c[0] for c in CASES].index('tiles_2x3_plus')]
    src = cuda(pan)
    out, stats, labels = ops.pan_components(src)
    assert labels is None and out.data_ptr() != src.data_ptr() and torch.equal(out, src)
    exp = want('labels_only', pan, 0, 8, True)
    assert stats.cpu().numpy().tolist() == exp[2].tolist() and exp[2][2:].tolist() == [0, 0]
    out, stats, labels = ops.pan_components(src, 6, 4, False, want_labels=True)
    exp = ref.clean_flood(pan, 6, 4, False)
    assert np.array_equal(out.cpu().numpy(), exp[0]) and np.array_equal(labels.cpu().numpy(), exp[1])
    assert np.array_equal(stats.cpu().numpy(), exp[2]) and exp[2][2] > 0
    for bad in (dict(workspace=torch.zeros(100, dtype=torch.uint8, device='cuda')), dict(out=torch.zeros((3, 3, 3), dtype=torch.uint8, device='cuda')),
                dict(labels=torch.zeros(pan.shape[:2], dtype=torch.int64, device='cuda')), dict(connectivity=5), dict(min_area=-2)):
        with pytest.raises(ValueError, match='pan_components'):
            ops.pan_components(src, **bad)


def test_in_place():
    from upsnet_amd import ops
    for name in ('tiles_2x3_plus', 'random_131x257', 'odd_37x53'):
        _, pan, min_area, keep = CASES[[c[0] for c in CASES].index(name)]
        for conn in (4, 8):
            exp = want(name, pan, min_area, conn, keep)
            buf = cuda(pan)
            out, stats, labels = ops.pan_components(buf, min_area, conn, keep, out=buf, want_labels=True)
            assert out is buf and np.array_equal(buf.cpu().numpy(), exp[0]) and not np.array_equal(exp[0], pan)
            assert np.array_equal(labels.cpu().numpy(), exp[1]) and np.array_equal(stats.cpu().numpy(), exp[2])


def test_unaligned_input_and_output():
    """Maps that start 3 bytes into their allocation, with H * W a multiple of 16 and W too. The input is read-only and is handed on as
    an aligned copy; an output that starts there is refused before any launch, so the kernels' byte path for such bases
    is no longer reached from Python."""
    from upsnet_amd import ops
    rng = np.random.default_rng(77)
    pan = ref.blobs(rng, 40, 160, 11, ref.KEYS, 0.02)
    exp = ref.clean_flood(pan, 4, 8, True)
    src = cuda(np.concatenate([pan.reshape(-1, 3)[:1], pan.reshape(-1, 3)]))[1:].view(40, 160, 3)
    dst = torch.zeros((40 * 160 + 1, 3), dtype=torch.uint8, device='cuda')[1:].view(40, 160, 3)
    assert src.data_ptr() % 16 and dst.data_ptr() % 16 and src.is_contiguous()
    with pytest.raises(ValueError, match='aligned'):
        ops.pan_components(src, 4, 8, True, out=dst)
    assert not dst.any()
    out, stats, _ = ops.pan_components(src, 4, 8, True)
    assert np.array_equal(out.cpu().numpy(), exp[0]) and np.array_equal(stats.cpu().numpy(), exp[2])
    assert np.array_equal(src.cpu().numpy(), pan)
    out, stats, _ = ops.pan_components(cuda(pan), 4, 8, True)          # and aligned: the 16-byte path of the same map
    assert np.array_equal(out.cpu().numpy(), exp[0]) and np.array_equal(stats.cpu().numpy(), exp[2])


def test_reused_workspace():
    """One workspace across two maps of one size and then a smaller size: as with a fresh workspace each time."""
    from upsnet_amd import ops
    rng = np.random.default_rng(78)
    a = ref.blobs(rng, 70, 300, 13, ref.KEYS, 0.03)
    b = ref._random(rng, 70, 300, ref.KEYS)
    c = ref.blobs(rng, 37, 53, 5, ref.KEYS, 0.05)
    ws = ops.pan_components_workspace(70, 300, 'cuda')
    for pan in (a, b, a, c, b):
        got = ops.pan_components(cuda(pan), 3, 8, True, want_labels=True, workspace=ws)
        fresh = ops.pan_components(cuda(pan), 3, 8, True, want_labels=True)
        exp = ref.clean_flood(pan, 3, 8, True)
        for x, y, e in zip((got[0], got[2], got[1]), (fresh[0], fresh[2], fresh[1]), exp):
            assert torch.equal(x, y) and np.array_equal(x.cpu().numpy(), e)


def test_byte_2_is_preserved():
    from upsnet_amd import ops
    rng = np.random.default_rng(79)
    pan = ref.blobs(rng, 45, 133, 6, ref.KEYS, 0.05)
    pan[..., 2] = rng.integers(0, 256, pan.shape[:2])
    other = pan.copy()
    other[..., 2] = rng.integers(0, 256, pan.shape[:2])
    for conn in (4, 8):
        out, stats, _ = ops.pan_components(cuda(pan), 5, conn, True)
        out2, stats2, _ = ops.pan_components(cuda(other), 5, conn, True)
        out, out2 = out.cpu().numpy(), out2.cpu().numpy()
        assert np.array_equal(out[..., 2], pan[..., 2]) and np.array_equal(out2[..., 2], other[..., 2])
        assert np.array_equal(out[..., :2], out2[..., :2]) and torch.equal(stats, stats2)      # byte 2 is never read
        assert np.array_equal(out, ref.clean_flood(pan, 5, conn, True)[0]) and int(stats[3]) > 0


def test_clean_panoptic_and_the_dataset_method(saved_config, caplog):
    import logging
    from upsnet_amd.dataset import clean_panoptic
    from upsnet_amd.dataset.base_dataset import BaseDataset
    rng = np.random.default_rng(80)
    pans = [ref.blobs(rng, 60, 90, 7, ref.KEYS, 0.04), ref.blobs(rng, 60, 90, 7, ref.KEYS, 0.04), ref.blobs(rng, 41, 50, 5, ref.KEYS, 0.04)]
    given = [pans[0], cuda(pans[1]), pans[2]]                          # numpy arrays are uploaded
    got = clean_panoptic(given, 4, connectivity=4, keep_largest=False)
    exp = [ref.clean_flood(p, 4, 4, False) for p in pans]
    assert all(g.is_cuda and np.array_equal(g.cpu().numpy(), e[0]) for g, e in zip(got, exp))
    assert np.array_equal(given[1].cpu().numpy(), pans[1])              # the inputs are untouched
    _, total = clean_panoptic(given, 4, connectivity=4, keep_largest=False, return_stats=True)
    assert total.cpu().numpy().tolist() == sum(e[2].astype(np.int64) for e in exp).tolist()
    saved_config.test.pan_min_component, saved_config.test.pan_component_connectivity = 5, 8
    with caplog.at_level(logging.INFO):
        got = BaseDataset().clean_pan_result(given)
    exp = [ref.clean_flood(p, 5, 8, True) for p in pans]
    assert all(np.array_equal(g.cpu().numpy(), e[0]) for g, e in zip(got, exp))
    removed = sum(int(e[2][2]) for e in exp)
    assert removed > 0 and ('%d of %d connected components' % (removed, sum(int(e[2][1]) for e in exp))) in caplog.text


def test_sequence_track_only_cleans_before_it_tracks(tmp_path, saved_config):
    """upsnet_amd.sequence --track_only --pan_min_component N writes what the tracker makes of clean_panoptic of the maps."""
    from PIL import Image
    from test_dataset_run_cpu import write_cfg
    from upsnet_amd import sequence
    from upsnet_amd.dataset import clean_panoptic, track_sequence
    rng = np.random.default_rng(81)
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
    cleaned = clean_panoptic(maps, 6, connectivity=4)
    assert any(not np.array_equal(c.cpu().numpy(), m) for c, m in zip(cleaned, maps))
    for extra, source in (([], maps), (['--pan_min_component', '6', '--pan_component_connectivity', '4'], cleaned)):
        out = str(tmp_path / ('out%d' % len(extra)))
        sequence.main(['--cfg', cfg, '--track_only', str(raw), '--out', out, '--panoptic_categories', cats] + extra)
        want = track_sequence(source)
        for k, (w_map, _) in enumerate(want):
            got = np.array(Image.open(os.path.join(out, 'raw', 'pan_2ch', 'f%02d.png' % k)))
            assert np.array_equal(got, w_map.cpu().numpy()), (extra, k)
        saved_config.test.pan_min_component = 0
    with pytest.raises(SystemExit, match='pan_component_connectivity'):
        sequence.main(['--cfg', cfg, '--track_only', str(raw), '--out', str(tmp_path / 'o'), '--panoptic_categories', cats,
                       '--pan_component_connectivity', '4'])


# ------------------------------------------------------------------------------------------------ end to end on the network
@pytest.fixture()
def saved_config():
    from upsnet_amd.config.config import config
    saved = copy.deepcopy(dict(config))
    yield config
    config.clear()
    config.update(saved)


def write_panoptic_gt(ds, maps, image_ids):
    """2-channel maps as the dataset's panoptic ground truth: one PNG (id = category * 256 + instance + 1) and one annotation per map,
    in the order given."""
    from PIL import Image
    os.makedirs(ds.panoptic_gt_folder, exist_ok=True)
    images, anns = [], []
    for m, image_id in zip(maps, image_ids):
        ids = np.where(m[..., 0] == 255, 0, m[..., 0].astype(np.int64) * 256 + m[..., 1] + 1)
        name = 'pan_%s.png' % image_id
        Image.fromarray(np.stack([ids % 256, ids // 256 % 256, ids // 65536], 2).astype(np.uint8)).save(os.path.join(ds.panoptic_gt_folder, name))
        u, cnt = np.unique(ids[ids > 0], return_counts=True)
        segs = [{'id': int(i), 'category_id': int((i - 1) // 256), 'iscrowd': 0, 'area': int(c)} for i, c in zip(u, cnt)]
        images.append({'id': image_id, 'file_name': name})
        anns.append({'image_id': image_id, 'file_name': name, 'segments_info': segs})
    categories = [{'id': c, 'name': 'c%d' % c, 'isthing': int(c > 10)} for c in range(19)]
    with open(ds.panoptic_json_file, 'w') as f:
        json.dump({'images': images, 'annotations': anns, 'categories': categories}, f)


def write_ground_truth(ds, rng):
    """Ground truth for every head of a generated dataset, without the network: semantic label PNGs and panoptic maps from seeded
    blob maps (annotations in another order than the image list), one rectangle per image in the instances JSON."""
    from PIL import Image
    keys = [(0, 0), (3, 0), (7, 0), (11, 1), (11, 2), (13, 1)]
    maps = {}
    with open(ds.instances_json_file) as f:
        inst = json.load(f)
    inst['annotations'] = []
    for entry in ds.roidb:
        w, h = Image.open(entry['image']).size
        maps[entry['id']] = m = ref.blobs(rng, h, w, 40, keys, 0.0)
        os.makedirs(os.path.dirname(ds.seg_gt_path(entry)), exist_ok=True)
        Image.fromarray(np.ascontiguousarray(m[..., 0])).save(ds.seg_gt_path(entry))
        x, y, bw, bh = w // 4, h // 4, w // 3, h // 3
        inst['annotations'].append({'id': len(inst['annotations']) + 1, 'image_id': entry['id'], 'category_id': inst['categories'][0]['id'],
                                    'iscrowd': 0, 'area': float(bw * bh), 'bbox': [float(x), float(y), float(bw), float(bh)],
                                    'segmentation': [[float(v) for v in (x, y, x + bw, y, x + bw, y + bh, x, y + bh)]]})
    with open(ds.instances_json_file, 'w') as f:
        json.dump(inst, f)
    order = [e['id'] for e in ds.roidb][::-1]
    write_panoptic_gt(ds, [maps[i] for i in order], order)


def test_evaluate_end_to_end_scores_writes_and_draws_the_cleaned_maps(tmp_path, saved_config):
    """evaluate.main on a generated COCO-layout dataset, without and with --pan_min_component: what the second run scores, writes and
    draws is clean_panoptic of the first run's maps. The first run's maps then serve as the panoptic ground truth, so that the plain
    maps score 1 and any pixel removed shows in the metrics."""
    from PIL import Image
    from test_dataset_run_cpu import make_dataset, write_cfg
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
    assert saved_config.test.pan_min_component == 0
    out = os.path.join(os.path.dirname(plain['results_file']), 'pans_unified')
    with open(os.path.join(out, 'pred.json')) as f:
        names, ids = zip(*[(a['file_name'], a['image_id']) for a in json.load(f)['annotations']])
    assert list(ids) == [e['id'] for e in ds.roidb][::-1]                       # the annotations' order, not the image list's
    before = read(out, 'pan_2ch', names)
    write_panoptic_gt(ds, before, ids)
    plain_metrics = ds.evaluate_panoptic(before, out)
    assert all(r['pq'] == 1.0 for r in plain_metrics['per_class'].values() if 'tp' in r)
    cleaned = clean_panoptic(before, N)
    assert any(not np.array_equal(c.cpu().numpy(), b) for c, b in zip(cleaned, before)), "nothing to remove: the run shows nothing"
    want_metrics = ds.evaluate_panoptic(cleaned, out)
    want_pictures = [open(p, 'rb').read() for p in ds.vis_panoptic(cleaned, str(tmp_path / 'want'), mode='flat')]
    res = main(['--cfg', cfg, '--synthetic_weights', '--write_panoptic', '--vis_panoptic', 'flat', '--pan_min_component', str(N)])
    assert saved_config.test.pan_min_component == N
    assert res['metrics']['panoptic'] == want_metrics and want_metrics != plain_metrics      # scored
    for got, c in zip(read(out, 'pan_2ch', names), cleaned):                                                             # written
        assert np.array_equal(got, c.cpu().numpy())
    pictures = [p for p in res['vis_panoptic_files'] if os.sep + 'vis_flat' + os.sep in p]                               # drawn
    assert len(pictures) == len(want_pictures) == 2
    assert [open(p, 'rb').read() for p in pictures] == want_pictures
