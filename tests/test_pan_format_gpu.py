"""GPU: the COCO panoptic format on the device (csrc/pan_format.hip via dataset/pan_format.py, PanopticEvaluator.add_png and the
BaseDataset / evaluate.py entry points) against the numpy restatements of tests/pan_format_ref.py. Every comparison is an integer or
byte equality. The one floating-point quantity is the IoU sum of the PQ round trip: add_png is bit-identical to the restated general
PQ over the same files always, and to add() over the 2-channel maps on all cases whose JSON areas equal the pixel counts; on the
others (a GT segment may then match several predictions, which are added in pred-id order, and the written ids do not ascend with the
instance number) it is compared to one ulp of the sum. Measured on an MI355X: the difference was 0.0 on every golden case, `area_json`
included, and on every random scene."""
import json
import os

import numpy as np
import pytest
import torch

import memguard
import size_population
from pan_format_ref import convert_2ch, pq_general, rgb_to_id
from test_pan_format_cpu import areas_consistent
from test_pq_cpu import golden, golden_categories, golden_images
from test_pq_gpu import CATS, evaluate, id_rgb, raw, scene

pytestmark = pytest.mark.gpu

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ALL_CATS = {c: {'id': c, 'isthing': c % 2} for c in range(255)}
COLOURED = {c: {'id': c, 'isthing': int(c >= 11), 'color': [(c * 40) % 256, 128, 250 - c]} for c in range(19)}


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def expected(pred, cats):
    from upsnet_amd.dataset.pan_format import ColorGenerator
    return convert_2ch(pred, ColorGenerator(cats).get_color)


def check_format(pred, cats, tensor=None):
    """panoptic_format on the device == the restatement: table and RGB map, and the id of every pixel."""
    from upsnet_amd.dataset.pan_format import panoptic_format
    rgb, info = panoptic_format(cuda(pred) if tensor is None else tensor, cats)
    assert rgb.is_cuda and rgb.dtype == torch.uint8 and tuple(rgb.shape) == pred.shape
    want_rgb, want_info = expected(pred, cats)
    assert info == want_info
    assert all(type(v) is int for el in info for v in [el['id'], el['area'], el['category_id'], el['iscrowd']] + el['bbox'])
    got = rgb.cpu().numpy()
    assert np.array_equal(got, want_rgb)
    key = pred[..., 0].astype(np.int64) * 256 + pred[..., 1]
    id_of = np.zeros(65536, np.int64)
    keys = [k for k in np.unique(key).tolist() if k >> 8 != 255]
    assert len(keys) == len(info)
    for k, el in zip(keys, info):                      # segments_info is in ascending key
        assert el['category_id'] == k >> 8
        id_of[k] = el['id']
    assert np.array_equal(rgb_to_id(got), np.where(pred[..., 0] == 255, 0, id_of[key]))
    return got, info


# ------------------------------------------------------------------------------------------------ table and map vs the restatement
def test_golden_maps():
    g = np.load(os.path.join(G, "unified_pan.npz"))
    for name in 'abc':
        check_format(g[name + '_out'], ALL_CATS)
        check_format(g[name + '_out'], {c: dict(e, color=[c, 255 - c, 7]) for c, e in ALL_CATS.items()})
    g = golden()
    cats = golden_categories(g)
    for name in g['cases'].tolist():
        for pred, _, _ in golden_images(g, name):
            check_format(np.ascontiguousarray(pred), cats)


def population_sizes():
    sizes = [r for r, _ in size_population.cityscapes_sizes()]
    coco = [r for r, _ in size_population.one_per_padded(size_population.coco_padded_sizes())]
    return sizes + coco[::max(1, len(coco) // 5)]


def test_random_scenes_at_the_population_sizes():
    sizes = population_sizes()
    assert (1024, 2048) in sizes and any(h > w for h, w in sizes) and len(sizes) >= 6
    for seed, (H, W) in enumerate(sizes):
        rng = np.random.default_rng(100 + seed)
        pred, _, _ = scene(rng, H, W, int(rng.integers(3, 14)), int(rng.integers(3, 14)))
        check_format(pred, COLOURED if seed % 2 else CATS)


def test_unaligned_and_odd_sizes():
    rng = np.random.default_rng(14)
    pred, _, _ = scene(rng, 101, 77, 4, 5)
    assert (101 * 77) % 16 != 0
    t = cuda(np.concatenate([pred[:1], pred]))[1:]
    assert t.data_ptr() % 16 != 0
    check_format(pred, CATS, tensor=t)
    pred, _, _ = scene(rng, 3, 1, 1, 1)              # one column: every pixel starts a row
    check_format(pred, CATS)


def test_one_pixel_and_all_void():
    one = np.array([[[12, 3, 0]]], np.uint8)
    _, info = check_format(one, CATS)
    assert info[0]['bbox'] == [0, 0, 0, 0] and info[0]['area'] == 1
    void = np.full((37, 53, 3), 255, np.uint8)
    void[..., 1] = 9
    got, info = check_format(void, CATS)
    assert info == [] and not got.any()
    check_format(np.array([[[255, 0, 0]]], np.uint8), CATS)


def test_pixel_noise_with_every_key():
    """All 65280 keys in one map: the LDS tables overflow into the global atomics, the table needs its second copy."""
    rng = np.random.default_rng(7)
    H, W = 512, 1024
    key = rng.integers(0, 65280, H * W)
    key[rng.random(H * W) < 0.05] = 255 * 256 + 3
    key[rng.permutation(H * W)[:65280]] = np.arange(65280)
    pred = np.stack([key >> 8, key & 255, np.zeros_like(key)], -1).astype(np.uint8).reshape(H, W, 3)
    _, info = check_format(pred, ALL_CATS)
    assert len(info) == 65280 and len({el['id'] for el in info}) == 65280


def test_two_runs_are_byte_identical_and_the_workspace_is_left_zeroed():
    from upsnet_amd.dataset.pan_format import PanopticFormatter
    rng = np.random.default_rng(3)
    a, _, _ = scene(rng, 512, 1024, 9, 11)
    b, _, _ = scene(rng, 300, 517, 5, 4)
    fmt = PanopticFormatter(COLOURED, device='cuda')
    outs = []
    for pred in (a, b, a, b):                         # one formatter, one workspace: an image never sees the previous one
        rgb, host, info = fmt.finish(fmt.submit(cuda(pred)))
        assert np.array_equal(rgb.cpu().numpy(), host)
        outs.append((host.copy(), info))
    for i in (0, 1):
        assert np.array_equal(outs[i][0], outs[i + 2][0]) and outs[i][1] == outs[i + 2][1]
        want_rgb, want_info = expected((a, b)[i], COLOURED)
        assert np.array_equal(outs[i][0], want_rgb) and outs[i][1] == want_info
    ws = fmt._state['ws'].view(torch.int32)
    assert not bool(ws[:5 * 65536].any()) and not bool(ws[6 * 65536:].any())   # all but the key -> colour table


# ------------------------------------------------------------------------------------------------ files
def _images(n, kind='coco'):
    if kind == 'coco':
        return [{'id': 100 + i, 'file_name': '%012d.jpg' % (100 + i)} for i in range(n)]
    return [{'id': 'img_%d' % i, 'file_name': 'city_%06d_000019_leftImg8bit.png' % i} for i in range(n)]


def test_file_round_trip(tmp_path):
    from PIL import Image
    from upsnet_amd.dataset.pan_format import read_panoptic, write_panoptic
    rng = np.random.default_rng(5)
    preds = [scene(rng, 120 + 7 * i, 200 + 3 * i, 3 + i, 4)[0] for i in range(5)]
    for kind in ('coco', 'Cityscapes'):
        out = str(tmp_path / kind)
        os.makedirs(out)
        images = _images(len(preds), kind)
        anns = write_panoptic([cuda(p) if i % 2 else p for i, p in enumerate(preds)], images, COLOURED, out)
        with open(os.path.join(out, 'pred.json')) as f:
            js = json.load(f)
        assert js == {'annotations': anns} and sorted(os.listdir(out)) == ['pan', 'pan_2ch', 'pred.json']
        assert len(os.listdir(os.path.join(out, 'pan'))) == len(preds)
        for i, (pred, ann) in enumerate(zip(preds, anns)):
            name = ('%012d.png' % (100 + i)) if kind == 'coco' else 'city_%06d_000019.png' % i
            assert ann['file_name'] == name and ann['image_id'] == images[i]['id']
            want_rgb, want_info = expected(pred, COLOURED)
            assert ann['segments_info'] == want_info
            assert np.array_equal(np.array(Image.open(os.path.join(out, 'pan', name))), want_rgb)
            assert np.array_equal(np.array(Image.open(os.path.join(out, 'pan_2ch', name))), pred)
            assert sum(el['area'] for el in ann['segments_info']) == int((pred[..., 0] != 255).sum())
        back = list(read_panoptic(os.path.join(out, 'pred.json'), os.path.join(out, 'pan')))
        assert [info for _, info in back] == [a['segments_info'] for a in anns]
        assert all(np.array_equal(rgb, expected(p, COLOURED)[0]) for (rgb, _), p in zip(back, preds))
    ids = write_panoptic(preds[:2], _images(2), COLOURED, str(tmp_path / 'coco'), image_ids=[7, 9])
    assert [a['image_id'] for a in ids] == [7, 9]


def test_dataset_write_panoptic_without_ground_truth(tmp_path):
    """A test-dev style set: names and ids from the image list, categories from the caller or a panoptic JSON, no gt.json."""
    from upsnet_amd.dataset.base_dataset import BaseDataset
    rng = np.random.default_rng(6)
    preds = [scene(rng, 64, 96, 3, 3)[0] for _ in range(2)]

    class DS(BaseDataset):
        has_gt = False
        name = 'coco_test-dev2017'
        roidb = [{'id': 5, 'file_name': '000000000005.jpg'}, {'id': 9, 'file_name': '000000000009.jpg'}]
    (tmp_path / 'cats.json').write_text(json.dumps({'categories': list(COLOURED.values())}))
    for k, kw in enumerate((dict(categories=COLOURED), dict(categories_json=str(tmp_path / 'cats.json')))):
        out = str(tmp_path / ('out%d' % k))
        anns = DS().write_panoptic([cuda(p) for p in preds], out, **kw)
        assert sorted(os.listdir(out)) == ['pan', 'pan_2ch', 'pred.json']
        assert [(a['image_id'], a['file_name']) for a in anns] == [(5, '000000000005.png'), (9, '000000000009.png')]
        assert [a['segments_info'] for a in anns] == [expected(p, COLOURED)[1] for p in preds]


def _round_trip(images, cats, out, name):
    """write_panoptic, then add_png over the files == add over the maps == the restated general PQ over the files."""
    from upsnet_amd.dataset.pan_format import read_panoptic, write_panoptic
    from upsnet_amd.dataset.pq import PanopticEvaluator
    os.makedirs(out)
    write_panoptic([cuda(p) for p, _, _ in images], _images(len(images)), cats, out)
    files = list(read_panoptic(os.path.join(out, 'pred.json'), os.path.join(out, 'pan')))
    ev = PanopticEvaluator(cats, device='cuda')
    for k, ((rgb, info), (_, gt, segs)) in enumerate(zip(files, images)):
        info = [dict(el, area=-5) for el in info]                          # the JSON's pred area is ignored
        if k % 2:
            ev.add_png(rgb, info[::-1], np.ascontiguousarray(gt), segs)    # numpy inputs, JSON order reversed
        else:
            ev.add_png(cuda(rgb), info, cuda(gt), segs)
    cnt, iou = raw(ev)
    ref_cnt, ref_iou = raw(evaluate(images, cats))
    gen = pq_general([(rgb, info, gt, segs) for (rgb, info), (_, gt, segs) in zip(files, images)], cats)
    np.testing.assert_array_equal(cnt, np.stack(gen[:3]), err_msg=name)
    assert np.array_equal(iou.view(np.int64), gen[3].view(np.int64)), name
    np.testing.assert_array_equal(cnt, ref_cnt, err_msg=name)
    print(name, 'max |add_png - add| of the IoU sums:', float(np.abs(iou - ref_iou).max()))
    if areas_consistent(images):
        assert np.array_equal(iou.view(np.int64), ref_iou.view(np.int64)), name
    else:
        assert np.all(np.abs(iou - ref_iou) <= np.spacing(np.maximum(iou, ref_iou))), name
    assert ev.pq_stat() is not None                                        # no sanity check trips
    return areas_consistent(images)


def test_pq_round_trip_golden(tmp_path):
    g = golden()
    cats = golden_categories(g)
    exact = [_round_trip(golden_images(g, name), cats, str(tmp_path / name), name) for name in g['cases'].tolist()]
    assert sum(exact) >= 10


@pytest.mark.parametrize("H,W,gh,gw,seed", [(1024, 2048, 8, 12, 0), (800, 1333, 7, 19, 3), (37, 53, 3, 4, 4), (1, 1, 1, 1, 5)])
def test_pq_round_trip_random_scenes(tmp_path, H, W, gh, gw, seed):
    rng = np.random.default_rng(seed)
    assert _round_trip([scene(rng, H, W, gh, gw) for _ in range(2)], CATS, str(tmp_path / 'scene'), 'scene%d' % seed)


# ------------------------------------------------------------------------------------------------ the relabel kernel
def _grid(H, W, gh, gw, values):
    cell = np.arange(gh * gw).reshape(gh, gw)
    return values[np.repeat(np.repeat(cell, H // gh, 0), W // gw, 1)]


def test_relabel_adversarial_ids():
    """Ids up to 2^24 - 1, the JSON in descending id order, 4096 GT segments next to 256 pred segments of one category."""
    from upsnet_amd.dataset.pan_format import relabel, segments_table
    from upsnet_amd.dataset.pq import PanopticEvaluator
    rng = np.random.default_rng(9)
    H = W = 512
    pred_ids = np.concatenate([[(1 << 24) - 1, 1], rng.choice(np.arange(2, (1 << 24) - 1), 254, replace=False)])
    gt_ids = rng.choice(np.arange(1, 1 << 24), 4096, replace=False)
    pid = np.roll(_grid(H, W, 16, 16, pred_ids), (3, 5), (0, 1))
    pid[rng.random((H, W)) < 0.03] = 0
    gid = _grid(H, W, 64, 64, gt_ids)
    pred_info = [{'id': int(i), 'category_id': 4, 'area': 0} for i in sorted(pred_ids.tolist(), reverse=True)]
    uniq, areas = np.unique(gid, return_counts=True)
    gt_info = [{'id': int(i), 'category_id': int(c), 'iscrowd': 0, 'area': int(a)} for i, c, a in zip(uniq, rng.integers(3, 6, 4096), areas)]
    assert len(gt_info) == 4096
    table = segments_table(pred_info)
    assert table[:, 2].tolist() == list(range(256)) and table[-1, 0] == (1 << 24) - 1
    status = torch.zeros(2, dtype=torch.int64, device='cuda')
    out, counts = relabel(cuda(id_rgb(pid)), table, 0, status)
    slot = np.searchsorted(table[:, 0], pid)
    want = np.stack([np.where(pid == 0, 255, 4), np.where(pid == 0, 0, slot % 256), np.zeros_like(pid)], -1).astype(np.uint8)
    assert np.array_equal(out.cpu().numpy(), want)
    assert counts.cpu().numpy().tolist() == [int((pid == i).sum()) for i in table[:, 0]]
    assert status.cpu().tolist() == [0, 0]
    ev = PanopticEvaluator(CATS, device='cuda')
    ev.add_png(id_rgb(pid), pred_info, id_rgb(gid), gt_info)
    cnt, iou = raw(ev)
    gen = pq_general([(id_rgb(pid), pred_info, id_rgb(gid), gt_info)], CATS)
    np.testing.assert_array_equal(cnt, np.stack(gen[:3]))
    assert np.array_equal(iou.view(np.int64), gen[3].view(np.int64)) and cnt.sum() > 256


def test_relabel_more_segments_than_the_lds_table():
    from upsnet_amd.dataset.pan_format import relabel, segments_table
    rng = np.random.default_rng(10)
    H, W, n = 300, 411, 5000
    ids = rng.choice(np.arange(1, 1 << 24), n, replace=False)
    pid = ids[rng.integers(0, n, (H, W))]
    pid[rng.random((H, W)) < 0.1] = 0
    info = [{'id': int(i), 'category_id': k % 20} for k, i in enumerate(ids)]
    table = segments_table(info)
    status = torch.zeros(2, dtype=torch.int64, device='cuda')
    t = cuda(np.concatenate([id_rgb(pid)[:1], id_rgb(pid)]))[1:]            # not 16-byte aligned, H * W odd
    out, counts = relabel(t, table, 0, status)
    row = np.searchsorted(table[:, 0], pid) % n
    want = np.stack([np.where(pid == 0, 255, table[row, 1]), np.where(pid == 0, 0, table[row, 2]), np.zeros_like(pid)], -1).astype(np.uint8)
    assert np.array_equal(out.cpu().numpy(), want)
    assert counts.cpu().numpy().tolist() == np.bincount(row[pid != 0], minlength=n).tolist()


# ------------------------------------------------------------------------------------------------ errors at the synchronisation
def _good_files(rng, n=3):
    out = []
    for _ in range(n):
        pred, gt, segs = scene(rng, 64, 96, 3, 3)
        rgb, info = expected(pred, CATS)
        out.append((rgb, info, gt, segs))
    return out


def test_png_and_json_sanity_checks_name_the_image_and_the_id():
    from upsnet_amd.dataset.pq import PanopticEvaluator
    rng = np.random.default_rng(41)
    files = _good_files(rng, 4)
    rgb, info, gt, segs = files[3]
    stray = rgb.copy()
    stray[5:9, 5:9] = (77, 0, 0)                                           # id 77: in the PNG, not in the JSON
    ev = PanopticEvaluator(CATS, device='cuda')
    for f in files[:3] + [(stray, info, gt, segs), files[0]]:
        ev.add_png(*f)                                                     # no exception while queueing
    with pytest.raises(KeyError, match=r"index 3 .*ID 77 is presented in PNG and not presented in JSON"):
        ev.pq_stat()
    with pytest.raises(KeyError):
        pq_general(files[:3] + [(stray, info, gt, segs)], CATS)
    ghost = info + [{'id': 123456, 'category_id': 3}]                      # in the JSON, no pixel in the PNG
    ev = PanopticEvaluator(CATS, device='cuda')
    for f in files[:2] + [(rgb, ghost, gt, segs), files[0]]:
        ev.add_png(*f)
    with pytest.raises(KeyError, match=r"index 2 .*ID 123456 is presented in JSON and not presented in PNG"):
        ev.summary()
    # merged: the error keeps its image index relative to the merged sequence
    a = PanopticEvaluator(CATS, device='cuda')
    a.add_png(*files[1])
    a += ev
    with pytest.raises(KeyError, match=r"index 3 .*ID 123456"):
        a.pq_stat()
    # a pred category that is not in the table, through add_png
    ev = PanopticEvaluator(CATS, device='cuda')
    ev.add_png(*files[0])
    ev.add_png(rgb, [dict(el, category_id=77) if k == 0 else el for k, el in enumerate(info)], gt, segs)
    with pytest.raises(KeyError, match=r"index 1 .*category_id 77"):
        ev.pq_stat()


def test_unknown_category_when_writing(tmp_path):
    from upsnet_amd.dataset.pan_format import PanopticFormatter, panoptic_format, write_panoptic
    rng = np.random.default_rng(42)
    preds = [scene(rng, 64, 96, 3, 3)[0] for _ in range(4)]
    bad = preds[3].copy()
    bad[5:9, 5:9, 0] = 77
    bad[20:24, 5:9, 0] = 99
    fmt = PanopticFormatter(CATS, device='cuda')
    handles = [fmt.submit(cuda(p)) for p in preds[:3] + [bad]]             # no exception while queueing
    for h in handles[:3]:
        fmt.finish(h)
    with pytest.raises(KeyError, match=r"index 3 .*category_id 77"):
        fmt.finish(handles[3])
    rgb, _, info = fmt.finish(fmt.submit(cuda(preds[0])))                  # the formatter goes on, its workspace is clean
    assert info == expected(preds[0], CATS)[1]
    with pytest.raises(KeyError, match=r"category_id 77"):
        panoptic_format(cuda(bad), CATS)
    with pytest.raises(KeyError, match=r"index 3 .*category_id 77"):
        write_panoptic(preds[:3] + [bad], _images(4), CATS, str(tmp_path))


# ------------------------------------------------------------------------------------------------ poisoned memory
MODS = ('upsnet_amd.dataset.pan_format', 'upsnet_amd.dataset.pq')


def test_poisoned_memory_panoptic_format():
    from upsnet_amd.dataset.pan_format import PanopticFormatter
    rng = np.random.default_rng(51)
    pred, _, _ = scene(rng, 101, 77, 4, 5)
    want_rgb, want_info = expected(pred, COLOURED)
    for pattern in 'AB':
        with memguard.poisoned(pattern, modules=MODS) as g:
            fmt = PanopticFormatter(COLOURED, device='cuda')
            rgb, host, info = fmt.finish(fmt.submit(memguard.banded_copy(cuda(pred), pattern)))
            rgb = rgb.clone()
        assert g.count >= 1
        assert np.array_equal(rgb.cpu().numpy(), want_rgb) and np.array_equal(host, want_rgb) and info == want_info, pattern
        ws = fmt._state['ws'].view(torch.int32)
        assert not bool(ws[:5 * 65536].any()) and not bool(ws[6 * 65536:].any())


def test_poisoned_memory_relabel_and_add_png():
    from upsnet_amd.dataset.pan_format import relabel, segments_table
    from upsnet_amd.dataset.pq import PanopticEvaluator
    rng = np.random.default_rng(52)
    files = _good_files(rng, 2)
    want = pq_general(files, CATS)
    outs = []
    for pattern in 'AB':
        with memguard.poisoned(pattern, modules=MODS) as g:
            ev = PanopticEvaluator(CATS, device='cuda')
            for rgb, info, gt, segs in files:
                ev.add_png(memguard.banded_copy(cuda(rgb), pattern), info, memguard.banded_copy(cuda(gt), pattern), segs)
            status = torch.zeros(2, dtype=torch.int64, device='cuda')
            out, counts = relabel(memguard.banded_copy(cuda(files[0][0]), pattern), segments_table(files[0][1]), 0, status)
            out, counts = out.clone(), counts.clone()
        assert g.count >= 3
        cnt, iou = raw(ev)
        np.testing.assert_array_equal(cnt, np.stack(want[:3]))
        assert np.array_equal(iou.view(np.int64), want[3].view(np.int64))
        # the evaluator's workspace is zero afterwards where pq_accumulate keeps it zero between images: every count cell and the
        # length of the key list (its segment table, IoU rows and key list are scratch that each image overwrites before reading)
        ws, cells = ev._state['ws'], (2 * 65536 + ev.max_gt_segments * 256) * 4
        nkeys = cells + ev.max_gt_segments * (24 + 8) + 256 * 4
        assert not bool(ws[:cells].any()) and not bool(ws[nkeys:nkeys + 8].any())
        assert ev._state['png_status'].cpu().tolist() == [0, 0] and status.cpu().tolist() == [0, 0]
        outs.append((out, counts))
    assert memguard.bit_equal(outs[0][0], outs[1][0]) and memguard.bit_equal(outs[0][1], outs[1][1])
    assert int(outs[0][1].sum()) == int((rgb_to_id(files[0][0]) != 0).sum())


# ------------------------------------------------------------------------------------------------ end to end on the network
def test_write_then_score_end_to_end(tmp_path, saved_config):
    """evaluate.main --write_panoptic on the generated COCO-layout dataset (annotations in another order than the image list), then
    --score_panoptic on the written pred.json: the same PQ dict as the run itself, from the files alone."""
    from PIL import Image
    from test_dataset_run_cpu import make_dataset, write_cfg
    from test_dataset_run_gpu import CASES, _direct_chain, _write_gt
    from upsnet_amd.config.config import update_config
    from upsnet_amd.dataset import coco
    from upsnet_amd.evaluate import main
    from upsnet_amd.synthetic import build_model
    image_set, sizes = CASES['coco']
    root = str(tmp_path / 'coco')
    make_dataset(root, 'coco', sizes, seed=11)
    cfg = write_cfg(tmp_path, 'coco', root, image_set)
    update_config(cfg)
    ds = coco(image_sets=[image_set], phase='test')
    model = build_model(device='cuda')
    model.use_graph = False
    chains = [_direct_chain(model, e['image'], ds.num_classes) for e in ds.roidb]
    ann_order = [2, 0, 3, 1]
    _write_gt(ds, chains, ann_order, [e['id'] for e in ds.roidb])
    del model
    torch.cuda.empty_cache()
    res = main(['--cfg', cfg, '--synthetic_weights', '--write_panoptic'])
    out = os.path.join(os.path.dirname(res['results_file']), 'pans_unified')
    assert sorted(os.listdir(out)) == ['gt.json', 'pan', 'pan_2ch', 'pred.json']
    with open(os.path.join(out, 'pred.json')) as f:
        anns = json.load(f)['annotations']
    assert [a['image_id'] for a in anns] == [ds.roidb[k]['id'] for k in ann_order]
    from upsnet_amd.config.config import config
    for a, k in zip(anns, ann_order):
        ch = chains[k]                                # the maps the run scores: the configured stuff area limit, not the chain's default
        want = ds.get_unified_pan_result([ch['sseg']], [ch['pano']], [ch['cls']],
                                         stuff_area_limit=config.test.panoptic_stuff_area_limit)[0].cpu().numpy()
        assert np.array_equal(np.array(Image.open(os.path.join(out, 'pan_2ch', a['file_name']))), want)
        assert a['segments_info'] == expected(want, {c: {'id': c, 'isthing': int(c > 10)} for c in range(19)})[1]
        assert np.array_equal(np.array(Image.open(os.path.join(out, 'pan', a['file_name']))), expected(want, CATS)[0])
    assert any(len(a['segments_info']) >= 3 for a in anns)
    scored = main(['--cfg', cfg, '--score_panoptic', os.path.join(out, 'pred.json'), '--score_panoptic_folder', os.path.join(out, 'pan')])
    assert scored['times'] is None and scored['metrics']['panoptic'] == res['metrics']['panoptic']
    assert all(r['pq'] == 1.0 for r in res['metrics']['panoptic']['per_class'].values() if 'tp' in r)
    again = main(['--cfg', cfg, '--eval_only', '--write_panoptic'])        # re-scoring writes the same bytes again
    assert again['metrics']['panoptic'] == res['metrics']['panoptic']
    with open(os.path.join(out, 'pred.json')) as f:
        assert json.load(f)['annotations'] == anns


@pytest.fixture()
def saved_config():
    import copy
    from upsnet_amd.config.config import config
    saved = copy.deepcopy(dict(config))
    yield config
    config.clear()
    config.update(saved)
