"""GPU: the Cityscapes instance prediction files (upsnet_amd/dataset/cityscapes_inst_format.py, csrc/cs_inst_format.hip). The expand
kernel in both forms byte for byte against the numpy restatement (tests/cityscapes_inst_format_ref.py) on the seeded run lists that
tests/test_cityscapes_inst_format_cpu.py shows to reach every special case, chunked and on poisoned guard-banded memory; written
folders scored by evaluate_instances_files against evaluate_instances on the in-memory lists, bit for bit; and end to end through
`python -m upsnet_amd.evaluate --write_instances / --score_instances`. Every comparison is equality."""
import functools
import os

import numpy as np
import pytest
import torch
from PIL import Image

from conftest import ROOT  # noqa: F401  (puts the repo root on sys.path)

import cityscapes_inst_cases as cases
import cityscapes_inst_format_ref as ref
import memguard

pytestmark = pytest.mark.gpu

MODULE = ('upsnet_amd.dataset.cityscapes_inst_format',)


@functools.lru_cache(maxsize=None)
def scene(H, W):
    """(trans, off, expected 8-bit planes, expected 1-bit planes) of one size, computed once and never written to."""
    _, counts = ref.real_scene() if (H, W) == ref.REAL_SIZE else ref.make_scene(H, W)
    trans, off = ref.runs_of_counts(counts)
    p8, p1 = ref.expected_planes(counts, H, W)
    for a in (p8, p1):
        a.setflags(write=False)
    return trans, off, p8, p1


def same_bytes(got, want):
    assert got.dtype == torch.uint8 and tuple(got.shape) == want.shape, (got.dtype, tuple(got.shape), want.shape)
    return np.array_equal(got.cpu().numpy(), want)


@pytest.mark.parametrize('one_bit', [False, True])
@pytest.mark.parametrize('size', ref.SIZES + [ref.REAL_SIZE], ids=lambda s: '%dx%d' % s)
def test_expand_equals_the_restatement(size, one_bit):
    from upsnet_amd.dataset.cityscapes_inst_format import expand_masks
    H, W = size
    trans, off, p8, p1 = scene(H, W)
    want = p1 if one_bit else p8
    got = expand_masks(trans, off, H, W, one_bit=one_bit)
    assert same_bytes(got, want)
    # device run lists and a caller's buffer (filled with what must not survive)
    out = torch.full(want.shape, 0x5A, dtype=torch.uint8, device='cuda')
    back = expand_masks(torch.from_numpy(trans.copy()).cuda(), torch.from_numpy(off.copy()).cuda(), H, W, one_bit=one_bit, out=out)
    assert back is out and same_bytes(out, want)


def test_no_masks_launch_nothing(monkeypatch):
    from upsnet_amd.dataset import cityscapes_inst_format as cif

    def no_launch(*a, **k):
        raise AssertionError('a launch was reached')
    monkeypatch.setattr(cif, '_expand_into', no_launch)
    for one_bit, shape in ((False, (0, 37, 53)), (True, (0, 37, 7))):
        got = cif.expand_masks(np.zeros(0, np.int32), np.zeros(1, np.int32), 37, 53, one_bit=one_bit)
        assert got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == shape


@pytest.mark.parametrize('one_bit', [False, True])
def test_chunked_equals_unchunked(one_bit, monkeypatch):
    from upsnet_amd.dataset import cityscapes_inst_format as cif
    H, W = 65, 129
    trans, off, p8, p1 = scene(H, W)
    want = p1 if one_bit else p8
    n, per = want.shape[0], cif.plane_bytes(H, W, one_bit)
    assert n >= 6
    calls = []
    real = cif.lib().upsnet_cs_inst_expand

    class Lib(object):
        def __getattr__(self, name):
            return getattr(real_lib, name)

        def upsnet_cs_inst_expand(self, *a):
            calls.append(a[3])
            return real(*a)
    real_lib = cif.lib()
    monkeypatch.setattr(cif, 'lib', lambda: Lib())
    for max_bytes, masks_per_launch in ((3 * per + per // 2, 3), (per, 1), (1, 1), (n * per, n)):
        del calls[:]
        assert same_bytes(cif.expand_masks(trans, off, H, W, one_bit=one_bit, max_bytes=max_bytes), want)
        assert calls == [masks_per_launch] * (n // masks_per_launch) + ([n % masks_per_launch] if n % masks_per_launch else [])


@pytest.mark.parametrize('one_bit', [False, True])
@pytest.mark.parametrize('size', [(37, 53), (65, 129), (128, 200)], ids=lambda s: '%dx%d' % s)
def test_poisoned_guard_banded_memory(size, one_bit):
    """The output in poisoned, fenced memory and the run lists inside bands of poison: the restatement's bytes under both patterns
    (so every output byte is written, and nothing read beyond the lists reaches it), every band intact."""
    from upsnet_amd.dataset.cityscapes_inst_format import expand_masks
    H, W = size
    trans, off, p8, p1 = scene(H, W)
    want = p1 if one_bit else p8
    d_trans, d_off = torch.from_numpy(trans.copy()).cuda(), torch.from_numpy(off.copy()).cuda()
    for pattern in ('A', 'B'):
        with memguard.poisoned(pattern, modules=MODULE) as g:
            got = expand_masks(memguard.banded_copy(d_trans, pattern), memguard.banded_copy(d_off, pattern), H, W, one_bit=one_bit)
            chunked = expand_masks(memguard.banded_copy(d_trans, pattern), memguard.banded_copy(d_off, pattern), H, W, one_bit=one_bit,
                                   max_bytes=2 * want[0].size)
        assert g.count == 2
        assert same_bytes(got, want) and same_bytes(chunked, want), pattern


# ------------------------------------------------------------------------------------------------ round trip
@pytest.fixture()
def saved_config():
    import copy
    from upsnet_amd.config.config import config
    saved = copy.deepcopy(dict(config))
    yield config
    config.clear()
    config.update(saved)


def same_bits(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a.view(np.uint64)[~np.isnan(a)],
                                                                                            b.view(np.uint64)[~np.isnan(b)])


def same_summary(got, want):
    assert got['aps'].dtype == np.float64 and got['aps'].shape == (8, 10)
    assert same_bits(got['aps'], want['aps']) and same_bits(got['AP'], want['AP']) and same_bits(got['AP50'], want['AP50'])
    for name, r in want['per_class'].items():
        assert same_bits(got['per_class'][name]['ap'], r['ap']) and same_bits(got['per_class'][name]['ap50'], r['ap50']), name
    return True


def check_folder(ds, all_boxes, all_segms, masks, folder, one_bit):
    """The written files against the restatement: the txt bytes, and every PNG read with PIL."""
    for i, entry in enumerate(ds.roidb):
        base = os.path.splitext(os.path.basename(entry['image']))[0]
        with open(os.path.join(folder, base + 'pred.txt'), 'rb') as f:
            text = f.read().decode()
        assert text == ref.pred_txt(entry['image'], [[]] + [all_boxes[c][i] for c in range(1, 9)])
        lines = text.splitlines()
        assert len(lines) == sum(len(all_segms[c][i]) for c in range(1, 9))
        row = 0
        for c in range(1, 9):
            for k in range(len(all_segms[c][i])):
                with Image.open(os.path.join(folder, *lines[row].split(' ')[0].split('/'))) as im:
                    assert im.mode == ('1' if one_bit else 'L')
                    got = np.asarray(im.convert('L'))
                assert np.array_equal(got, ref.plane_8bit(masks[i][c][k].astype(np.uint8))), (i, c, k)
                row += 1


def test_written_folders_score_like_the_lists_in_memory(tmp_path, saved_config):
    from test_dataset_run_cpu import make_dataset, write_cfg
    from upsnet_amd.config.config import update_config
    from upsnet_amd.dataset import Cityscapes
    from upsnet_amd.dataset.cityscapes_eval import InstanceEvaluator
    from upsnet_amd.dataset.cityscapes_inst_format import score_instance_files
    from upsnet_amd.dataset.rle import rle_to_string
    root = str(tmp_path / 'Cityscapes')
    make_dataset(root, 'Cityscapes', [(96, 160), (37, 53)], seed=3)
    update_config(write_cfg(tmp_path, 'Cityscapes', root, 'val'))
    ds = Cityscapes(image_sets=['val'], phase='test')
    rng = np.random.default_rng(7)
    all_boxes, all_segms = [[] for _ in range(9)], [[] for _ in range(9)]
    masks, gts, orders = [], [], []
    for i, entry in enumerate(ds.roidb):
        gt, preds = cases.make_image(rng, entry['height'], entry['width'], n_regions=10, extent=16)
        dets, rles, order = cases.per_class_results(preds, rle_to_string if i % 2 == 0 else None)
        for c in range(1, 9):
            all_boxes[c].append(dets[c])
            all_segms[c].append(rles[c])
        masks.append({c: [p['mask'] for p in preds if p['cls'] == c] for c in range(1, 9)})
        os.makedirs(os.path.dirname(ds.instance_gt_path(entry)), exist_ok=True)
        Image.fromarray(gt).save(ds.instance_gt_path(entry))
        gts.append(gt)
        orders.append(order)
    assert sorted((e['height'], e['width']) for e in ds.roidb) == [(37, 53), (96, 160)] and all(len(o) > 3 for o in orders)

    want = ds.evaluate_instances(all_boxes, all_segms, str(tmp_path / 'memory'))
    assert np.nanmax(want['aps']) > 0
    counts = []
    for i in range(len(ds.roidb)):       # the integer counts of every image from the lists in memory
        ev = InstanceEvaluator()
        ev.add_rle(gts[i], [[]] + [all_boxes[c][i] for c in range(1, 9)], [[]] + [all_segms[c][i] for c in range(1, 9)])
        counts.append({k: v.cpu().numpy() for k, v in ev.last_counts().items()})

    for one_bit in (False, True):
        out = str(tmp_path / ('bits1' if one_bit else 'bits8'))
        written = ds.write_instance_result(all_boxes, all_segms, out, one_bit=one_bit)
        folder = os.path.join(out, 'inst_seg')
        assert written == [os.path.join(folder, os.path.splitext(os.path.basename(e['image']))[0] + 'pred.txt') for e in ds.roidb]
        check_folder(ds, all_boxes, all_segms, masks, folder, one_bit)
        got = ds.evaluate_instances_files(folder, str(tmp_path / 'files'))
        assert same_summary(got, want)
        with open(str(tmp_path / 'files' / 'instance_results.txt')) as f, open(str(tmp_path / 'memory' / 'instance_results.txt')) as g:
            assert f.read() == g.read()
        seen = []

        def after_image(i, ev, pred):
            seen.append(i)
            c = {k: v.cpu().numpy() for k, v in ev.last_counts().items()}
            assert sorted(c) == sorted(counts[i])
            for k in c:
                assert np.array_equal(c[k], counts[i][k]), (i, k)
            assert pred['scores'].tolist() == [p for cc in range(1, 9) for p in np.asarray(all_boxes[cc][i], np.float32).reshape(-1, 5)[:, 4].tolist()]
        ev = score_instance_files(ds, folder, after_image=after_image)
        assert seen == list(range(len(ds.roidb))) and ev.num_images == len(ds.roidb)
    # without ground truth: the writer works, the scorer refuses
    ds.has_gt = False
    assert len(ds.write_instance_result(all_boxes, all_segms, str(tmp_path / 'no_gt'))) == len(ds.roidb)
    with pytest.raises(ValueError, match='no ground truth'):
        ds.evaluate_instances_files(os.path.join(str(tmp_path / 'no_gt'), 'inst_seg'))


# ------------------------------------------------------------------------------------------------ end to end
def test_evaluate_end_to_end_write_and_score_instances(tmp_path, saved_config):
    """The generated Cityscapes tree of tests/test_cityscapes_inst_gpu.py's end-to-end test (instance-id maps painted from the
    network's own masks): a run with --eval_instances --write_instances, then --score_instances on the written folder gives the same
    bits; --eval_only --write_instances --instances_1bit rewrites the folder with 1-bit masks, which score the same; the refusals."""
    import cityscapes_inst_ref as inst_ref
    from test_cityscapes_inst_gpu import _decode
    from test_dataset_run_cpu import make_dataset, write_cfg
    from test_dataset_run_gpu import _direct_chain, _write_gt
    from upsnet_amd.config.config import update_config
    from upsnet_amd.dataset import Cityscapes
    from upsnet_amd.evaluate import main
    from upsnet_amd.synthetic import build_model
    root = str(tmp_path / 'Cityscapes')
    make_dataset(root, 'Cityscapes', [(256, 512), (128, 256)], seed=11)
    cfg = write_cfg(tmp_path, 'Cityscapes', root, 'val')
    update_config(cfg)
    ds = Cityscapes(image_sets=['val'], phase='test')
    model = build_model(device='cuda')
    model.use_graph = False
    chains = [_direct_chain(model, e['image'], ds.num_classes) for e in ds.roidb]
    n = len(ds.roidb)
    _write_gt(ds, chains, list(range(n)), ['img_%d' % e['id'] for e in ds.roidb])
    del model
    torch.cuda.empty_cache()
    for k, entry in enumerate(ds.roidb):
        H, W = entry['height'], entry['width']
        ids = np.full((H, W), 7, np.uint16)
        for c in range(1, 9):
            for j, rle in enumerate(chains[k]['masks'][c - 1]):
                ids[_decode(rle)] = inst_ref.CLASSES[c - 1][1] * 1000 + j
        ids[:, :W // 8] = 0                                   # a void band
        os.makedirs(os.path.dirname(ds.instance_gt_path(entry)), exist_ok=True)
        Image.fromarray(ids).save(ds.instance_gt_path(entry))

    res = main(['--cfg', cfg, '--synthetic_weights', '--eval_instances', '--write_instances'])
    want = res['metrics']['instance_ap']
    folder = os.path.join(os.path.dirname(res['results_file']), 'inst_seg')
    txts = sorted(f for f in os.listdir(folder) if f.endswith('pred.txt'))
    assert txts == sorted(os.path.splitext(os.path.basename(e['image']))[0] + 'pred.txt' for e in ds.roidb)
    pngs = [os.path.join(d, f) for d, _, files in os.walk(os.path.join(folder, 'seg_results')) for f in files]
    assert len(pngs) > 0
    for p in pngs:
        with Image.open(p) as im:
            assert im.mode == 'L'
    scored = main(['--cfg', cfg, '--score_instances', folder])
    assert scored['results_file'] is None and scored['times'] is None and set(scored['metrics']) == {'instance_ap'}
    assert same_summary(scored['metrics']['instance_ap'], want)

    again = main(['--cfg', cfg, '--eval_only', '--write_instances', '--instances_1bit'])
    assert 'instance_ap' not in again['metrics']
    for p in pngs:
        with Image.open(p) as im:
            assert im.mode == '1'
    assert same_summary(main(['--cfg', cfg, '--score_instances', folder])['metrics']['instance_ap'], want)

    with pytest.raises(SystemExit, match='--instances_1bit'):
        main(['--cfg', cfg, '--eval_only', '--instances_1bit'])
    with pytest.raises(SystemExit, match='--score_instances: no folder'):
        main(['--cfg', cfg, '--score_instances', os.path.join(folder, 'nowhere')])
    os.remove(ds.instance_gt_path(ds.roidb[1]))
    with pytest.raises(FileNotFoundError, match='gtFine_instanceIds.png'):
        main(['--cfg', cfg, '--score_instances', folder])
