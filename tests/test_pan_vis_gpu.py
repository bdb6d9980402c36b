"""GPU: the panoptic pictures (csrc/pan_vis.hip, dataset/pan_vis.py) against the numpy restatement of the drawing rule
(tests/pan_vis_ref.py), byte for byte, in both modes: the hand-derived pictures, seeded scenes at sizes around the tile, a pixel-noise
map (LDS-table overflow, label cap), a map whose coordinate sums pass 2^32, poisoned and guard-banded outputs and workspaces, the
zeroed-again workspace, misaligned bases, and `python -m upsnet_amd.evaluate --vis_panoptic both` on generated datasets."""
import copy
import json
import os

import numpy as np
import pytest
import torch

import memguard
import pan_vis_ref
from test_dataset_run_cpu import make_dataset, write_cfg
from test_pan_vis_cpu import NO_LABELS, flat_cases, font, label_case_picture, label_cases, many_segments, overlay_hand_case

pytestmark = pytest.mark.gpu

MODS = ('upsnet_amd.dataset.pan_vis', 'upsnet_amd.dataset.pan_format')
NAMES = ['road', 'sidewalk', 'building', 'wall', 'fence', 'pole', 'traffic light', 'traffic sign', 'vegetation', 'terrain', 'sky',
         'person', 'rider', 'car', 'truck', 'bus', 'train', 'motorcycle', 'bicycle']
CATS19 = {c: {'id': c, 'isthing': int(c >= 11), 'color': [(c * 40 + 7) % 256, (128 + 9 * c) % 256, 250 - c], 'name': NAMES[c]} for c in range(19)}
PLAIN19 = {c: {'id': c, 'isthing': int(c >= 11)} for c in range(19)}          # default colours, str(id) as the name


@pytest.fixture()
def saved_config():
    from upsnet_amd.config.config import config
    saved = copy.deepcopy(dict(config))
    yield config
    config.clear()
    config.update(saved)


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def scene(seed, H, W, n, void=True):
    """(pred_2ch, image): n segments as the nearest-seed cells of n random points (so that segments touch every edge), categories
    0..18 with instance numbers counted per category from 1 for things and from 0 for stuff, one cell in eight VOID."""
    rng = np.random.default_rng(seed)
    image = rng.integers(0, 256, (H, W, 3)).astype(np.uint8)
    if n == 0:
        pred = np.zeros((H, W, 3), np.uint8)
        pred[..., 0] = 255
        pred[..., 1] = rng.integers(0, 256, (H, W))
        return pred, image
    n = min(n, H * W)
    pts = rng.permutation(H * W)[:n]
    py, px = pts // W, pts % W
    yy, xx = np.mgrid[0:H, 0:W]
    cell = np.argmin((yy[..., None] - py) ** 2 + (xx[..., None] - px) ** 2, -1)
    cat = rng.integers(0, 19, n)
    inst = np.zeros(n, np.int64)
    for c in range(19):
        sel = np.nonzero(cat == c)[0]
        inst[sel] = np.arange(len(sel)) + (1 if c >= 11 else 0)
    if void and n >= 8:
        cat[rng.permutation(n)[:n // 8]] = 255
    pred = np.stack([cat[cell], inst[cell], np.zeros_like(cell)], -1).astype(np.uint8)
    return np.ascontiguousarray(pred), image


def device(pred, cats, image, mode, min_area=1024):
    from upsnet_amd.dataset import pan_vis
    out = pan_vis.render_panoptic(cuda(pred), cats, None if image is None else cuda(image), mode, min_area)
    torch.cuda.synchronize()
    assert out.is_cuda and out.dtype == torch.uint8 and tuple(out.shape) == pred.shape
    return out.cpu().numpy()


def same(got, want, what=''):
    bad = np.argwhere((got != want).any(2))
    assert bad.size == 0, '%s: %d pixels differ, first (y, x) %s' % (what, len(bad), bad[:6].tolist())


def check_both(pred, cats, image, min_area, what=''):
    same(device(pred, cats, None, 'flat'), pan_vis_ref.render_flat(pred, cats), what + ' flat')
    want, _, _ = pan_vis_ref.render_overlay(pred, cats, image, font(), min_area)
    same(device(pred, cats, image, 'overlay', min_area), want, what + ' overlay')


def raw_flat(pred, cats):
    """The entry point in flat mode with everything it ignores NULL, also for maps whose categories the formatter refuses."""
    from upsnet_amd._lib import check, lib, ptr, stream
    from upsnet_amd.dataset.pan_format import category_table
    H, W = pred.shape[:2]
    d_pred, table = cuda(pred), cuda(category_table(cats))
    ws = torch.zeros((int(lib().upsnet_pan_vis_workspace_bytes()),), dtype=torch.uint8, device='cuda')
    out = torch.empty((H, W, 3), dtype=torch.uint8, device='cuda')
    info = torch.full((2,), -1, dtype=torch.int32, device='cuda')
    check(lib().upsnet_pan_vis(stream(), 0, ptr(d_pred), None, None, None, H, W, ptr(table), None, None, 0, ptr(ws), ptr(out), ptr(info)),
          'pan_vis')
    torch.cuda.synchronize()
    assert info.tolist() == [0, 0]
    return out.cpu().numpy()


# ------------------------------------------------------------------------------------------------ hand cases
@pytest.mark.parametrize('case', flat_cases(), ids=lambda c: c[0])
def test_device_draws_the_flat_hand_pictures(case):
    from upsnet_amd.dataset import pan_vis
    name, pred, cats, want = case
    same(raw_flat(pred, cats), want, name)
    if name == 'no_contour_void_and_unknown_category':
        with pytest.raises(KeyError):
            pan_vis.render_panoptic(cuda(pred), cats, mode='flat')
    else:
        same(device(pred, cats, None, 'flat'), want, name)


def test_device_draws_the_overlay_hand_picture():
    pred, cats, image, want = overlay_hand_case()
    same(device(pred, cats, image, 'overlay', NO_LABELS), want)


@pytest.mark.parametrize('case', label_cases(), ids=lambda c: c[0])
def test_device_draws_the_hand_derived_labels(case):
    name, pred, cats, image, min_area, boxes = case
    same(device(pred, cats, image, 'overlay', min_area), label_case_picture(pred, cats, image, boxes), name)


# ------------------------------------------------------------------------------------------------ seeded scenes
@pytest.mark.parametrize('H,W', [(1, 1), (1, 40), (40, 1), (33, 65), (32, 64), (64, 32), (65, 33), (257, 513)])
def test_scenes_match_restatement(H, W):
    for k, n in enumerate((0, 1, 120)):
        pred, image = scene(1000 * H + 10 * W + k, H, W, n)
        keys = pan_vis_ref.segments(pred)[0]
        if n and H * W > 1:
            assert len(keys) >= 1
        min_area = 1 if H * W < 4096 else H * W // 480
        check_both(pred, CATS19 if k % 2 else PLAIN19, image, min_area, '%d x %d, %d segments' % (H, W, n))
    if (H, W) == (257, 513):          # segments on every edge, things with contours, labels drawn
        top = set(map(tuple, pred[0, :, :2].tolist())) | set(map(tuple, pred[-1, :, :2].tolist()))
        assert len(top) > 4 and len(pan_vis_ref.label_boxes(pred, CATS19, min_area)[0]) > 20
        assert (pan_vis_ref.render_flat(pred, CATS19) == 255).all(2).sum() > 1000


def test_pixel_noise_overflows_the_lds_table_and_hits_the_label_cap():
    from upsnet_amd.dataset import pan_vis
    rng = np.random.default_rng(8)
    H, W = 64, 96
    key = rng.integers(0, 19 * 256, (H, W))
    key[rng.random((H, W)) < 0.05] = 255 << 8 | 3
    pred = np.stack([key >> 8, key & 255, np.zeros_like(key)], -1).astype(np.uint8)
    n = len(pan_vis_ref.segments(pred)[0])
    assert n > 3000                                    # far more keys than the 1024 slots of a workgroup's table
    image = rng.integers(0, 256, (H, W, 3)).astype(np.uint8)
    check_both(pred, PLAIN19, image, 1, 'noise')
    want, qualified, drawn = pan_vis_ref.render_overlay(pred, PLAIN19, image, font(), 1)
    assert (qualified, drawn) == (n, 256)
    r = pan_vis.PanopticRenderer(PLAIN19, 'cuda')
    out, info, handle = r.submit(cuda(pred), cuda(image), 'overlay', 1)
    assert info.tolist() == [n, 256]
    same(out.cpu().numpy(), want)
    pred, cats = many_segments()                       # 300 one-pixel segments: the first 256 keys
    image = rng.integers(0, 256, pred.shape).astype(np.uint8)
    out, info, handle = pan_vis.PanopticRenderer(cats, 'cuda').submit(cuda(pred), cuda(image), 'overlay', 1)
    assert info.tolist() == [300, 256]
    same(out.cpu().numpy(), pan_vis_ref.render_overlay(pred, cats, image, font(), 1)[0])


def test_coordinate_sums_beyond_32_bits():
    """2048 x 4096, one segment: sum x = 2048 * 4096 * 4095 / 2 > 2^32; a 32-bit moment would move the label."""
    H, W = 2048, 4096
    pred = np.zeros((H, W, 3), np.uint8)
    pred[..., 0], pred[..., 1] = 13, 1
    image = np.random.default_rng(4).integers(0, 256, (H, W, 3)).astype(np.uint8)
    keys, area, sx, sy = pan_vis_ref.segments(pred)
    assert sx[0] > 1 << 32 and sy[0] > 1 << 32
    assert pan_vis_ref.label_boxes(pred, CATS19, 1024)[0] == [(13 << 8 | 1, 2047 - 6 * 3, 1023 - 8, b'car')]
    want, _, _ = pan_vis_ref.render_overlay(pred, CATS19, image, font(), 1024)
    same(device(pred, CATS19, image, 'overlay'), want)
    same(device(pred, CATS19, None, 'flat'), pan_vis_ref.render_flat(pred, CATS19))


# ------------------------------------------------------------------------------------------------ memory
SIZES = [(150, 210, 30), (67, 95, 9), (190, 260, 60)]


def test_poisoned_output_and_workspace_over_images_of_different_size():
    from upsnet_amd._lib import lib
    from upsnet_amd.dataset import pan_vis
    scenes = [scene(60 + k, h, w, n) for k, (h, w, n) in enumerate(SIZES)]
    wants = [(pan_vis_ref.render_flat(p, CATS19), pan_vis_ref.render_overlay(p, CATS19, im, font(), 200)[0]) for p, im in scenes]
    zeroed = int(lib().upsnet_pan_vis_workspace_zeroed_bytes())
    runs = []
    for pattern in ('A', 'B'):
        with memguard.poisoned(pattern, modules=MODS) as guard:
            r = pan_vis.PanopticRenderer(CATS19, 'cuda')            # one renderer: one workspace over all images
            outs = []
            for pred, image in scenes:
                d_pred, d_image = memguard.banded_copy(cuda(pred), pattern), memguard.banded_copy(cuda(image), pattern)
                flat = r.submit(d_pred, None, 'flat')[0]
                over = r.submit(d_pred, d_image, 'overlay', 200)[0]
                outs.append((flat, over))
            torch.cuda.synchronize()
            assert guard.count >= 1 + 4 * len(scenes)               # the workspace; per picture its output and its counts
            assert not bool(r._state['ws'][:zeroed].any())
        runs.append([(a.cpu().numpy(), b.cpu().numpy()) for a, b in outs])
    for outs in runs:
        for (flat, over), (want_flat, want_over) in zip(outs, wants):
            same(flat, want_flat, 'flat')
            same(over, want_over, 'overlay')


def test_used_workspace_gives_the_bytes_of_a_fresh_one():
    from upsnet_amd._lib import lib
    from upsnet_amd.dataset import pan_vis
    a, b = scene(71, 130, 200, 40), scene(72, 96, 64, 3000)
    zeroed = int(lib().upsnet_pan_vis_workspace_zeroed_bytes())
    used = pan_vis.PanopticRenderer(CATS19, 'cuda')
    first = used.submit(cuda(a[0]), cuda(a[1]), 'overlay', 50)[0].cpu().numpy()
    for pred, image in (b, a, b):
        got = used.submit(cuda(pred), cuda(image), 'overlay', 50)[0].cpu().numpy()
        assert not bool(used._state['ws'][:zeroed].any())
        fresh = pan_vis.PanopticRenderer(CATS19, 'cuda').submit(cuda(pred), cuda(image), 'overlay', 50)[0].cpu().numpy()
        assert np.array_equal(got, fresh)
        same(got, pan_vis_ref.render_overlay(pred, CATS19, image, font(), 50)[0])
    assert np.array_equal(first, used.submit(cuda(a[0]), cuda(a[1]), 'overlay', 50)[0].cpu().numpy())     # two runs, the same bytes


@pytest.mark.parametrize('shift', [1, 2, 3])
def test_misaligned_bases_take_the_byte_path(shift):
    """The map and the image start `shift` bytes into their buffers: read-only inputs, handed on as aligned copies; an output that
    starts there is refused before any launch, so the kernel's byte path for such bases is no longer reached from Python."""
    from upsnet_amd.dataset import pan_vis
    H, W = 70, 37                                      # 111 bytes per row: the rows' alignment changes from row to row as well
    pred, image = scene(80 + shift, H, W, 25)

    def off(a):
        flat = torch.zeros((a.size + 16,), dtype=torch.uint8, device='cuda')
        t = flat[shift:shift + a.size].view(a.shape)
        t.copy_(cuda(a))
        assert t.data_ptr() % 4 == shift and t.is_contiguous()
        return t

    r = pan_vis.PanopticRenderer(CATS19, 'cuda')
    out = off(np.zeros((H, W, 3), np.uint8))
    with pytest.raises(ValueError, match='aligned'):
        r.submit(off(pred), off(image), 'overlay', 30, out=out)
    assert not out.any()
    out = torch.zeros((H, W, 3), dtype=torch.uint8, device='cuda')
    r.submit(off(pred), off(image), 'overlay', 30, out=out)
    same(out.cpu().numpy(), pan_vis_ref.render_overlay(pred, CATS19, image, font(), 30)[0], 'overlay')
    out = torch.zeros((H, W, 3), dtype=torch.uint8, device='cuda')
    r.submit(off(pred), None, 'flat', out=out)
    same(out.cpu().numpy(), pan_vis_ref.render_flat(pred, CATS19), 'flat')


# ------------------------------------------------------------------------------------------------ the dataset classes and the CLI
@pytest.mark.parametrize('kind', ['Cityscapes', 'coco'])
def test_evaluate_vis_panoptic_end_to_end(kind, tmp_path, saved_config):
    from PIL import Image
    from upsnet_amd.config.config import update_config
    from upsnet_amd.dataset import Cityscapes, coco, pan_vis, vis
    from upsnet_amd.evaluate import main
    from upsnet_amd.synthetic import build_model
    from test_dataset_run_gpu import CASES, _direct_chain, _write_gt
    image_set, sizes = CASES[kind]
    sizes = sizes[-3:]
    root = str(tmp_path / kind)
    make_dataset(root, kind, sizes, seed=11)
    cfg = write_cfg(tmp_path, kind, root, image_set)
    update_config(cfg)
    ds = (Cityscapes if kind == 'Cityscapes' else coco)(image_sets=[image_set], phase='test')
    model = build_model(device='cuda')
    model.use_graph = False
    chains = [_direct_chain(model, e['image'], ds.num_classes) for e in ds.roidb]
    n = len(ds.roidb)
    if kind == 'Cityscapes':
        ann_order, pan_ids = list(range(n)), ['img_%d' % e['id'] for e in ds.roidb]
    else:
        ann_order, pan_ids = [2, 0, 1], [e['id'] for e in ds.roidb]
    _write_gt(ds, chains, ann_order, pan_ids)
    del model
    torch.cuda.empty_cache()
    with open(ds.panoptic_json_file) as f:
        gt = json.load(f)
    combined = kind == 'coco'

    res = main(['--cfg', cfg, '--synthetic_weights', '--write_panoptic', '--vis_panoptic', 'both', '--vis_panoptic_min_area', '64']
               + (['--pan_combined'] if combined else []))
    assert 'panoptic' in res['metrics']                      # drawn beside the evaluation, not instead of it
    results_dir = os.path.dirname(res['results_file'])
    folders = ['pans_unified'] + (['pans_combined'] if combined else [])
    names = [im['file_name'] for im in gt['images']]
    assert res['vis_panoptic_files'] == [os.path.join(results_dir, f, sub, name) for f in folders for sub in ('vis_flat', 'vis')
                                         for name in names]
    labelled = 0
    for f in folders:
        out = os.path.join(results_dir, f)
        assert sorted(os.listdir(out)) == ['gt.json', 'pan', 'pan_2ch', 'pred.json', 'vis', 'vis_flat']
        for name, k in zip(names, ann_order):
            pred = np.array(Image.open(os.path.join(out, 'pan_2ch', name)))
            image = vis.load_image(ds.roidb[k]['image'])
            assert image.shape == pred.shape
            for mode, sub in (('flat', 'vis_flat'), ('overlay', 'vis')):
                png = np.asarray(Image.open(os.path.join(out, sub, name)))
                want = pan_vis.render_panoptic(cuda(pred), gt['categories'], cuda(image), mode, 64).cpu().numpy()
                assert png.dtype == np.uint8 and np.array_equal(png, want), (f, sub, name)
            same(want, pan_vis_ref.render_overlay(pred, gt['categories'], image, font(), 64)[0], name)
            labelled += len(pan_vis_ref.label_boxes(pred, gt['categories'], 64)[0])
    assert labelled > 0

    saved = {}
    for path in res['vis_panoptic_files']:
        with open(path, 'rb') as f:
            saved[path] = f.read()
        os.remove(path)
    again = main(['--cfg', cfg, '--eval_only', '--vis_panoptic', 'both', '--vis_panoptic_min_area', '64']
                 + (['--pan_combined'] if combined else []))                                      # the same files again
    assert again['vis_panoptic_files'] == res['vis_panoptic_files'] and again['times'] is None
    for path in res['vis_panoptic_files']:
        with open(path, 'rb') as f:
            assert f.read() == saved[path], path
        os.remove(path)
    again = main(['--cfg', cfg, '--eval_only', '--vis_panoptic', 'overlay'] + (['--pan_combined'] if combined else []))
    assert again['vis_panoptic_files'] == [p for p in res['vis_panoptic_files'] if os.sep + 'vis' + os.sep in p]
    assert all(os.path.isfile(p) for p in again['vis_panoptic_files']) and again['metrics']['panoptic'] == res['metrics']['panoptic']
    assert not os.listdir(os.path.join(results_dir, 'pans_unified', 'vis_flat'))


def test_dataset_vis_panoptic_without_ground_truth(tmp_path):
    """A test-dev style set: names from the image list, categories from the caller or a panoptic JSON."""
    from PIL import Image
    from upsnet_amd.dataset import pan_vis
    from upsnet_amd.dataset.base_dataset import BaseDataset
    scenes = [scene(90 + i, 64, 96, 12) for i in range(2)]
    paths = [str(tmp_path / ('%012d.png' % i)) for i in (5, 9)]
    for (_, image), p in zip(scenes, paths):
        Image.fromarray(image).save(p)

    class DS(BaseDataset):
        has_gt = False
        name = 'coco_test-dev2017'
        roidb = [{'id': 5, 'file_name': '000000000005.jpg', 'image': paths[0]}, {'id': 9, 'file_name': '000000000009.jpg', 'image': paths[1]}]
    (tmp_path / 'cats.json').write_text(json.dumps({'categories': list(CATS19.values())}))
    with pytest.raises(ValueError):
        DS().vis_panoptic([cuda(p) for p, _ in scenes], str(tmp_path / 'none'), mode='flat')
    for k, kw in enumerate((dict(categories=CATS19), dict(categories_json=str(tmp_path / 'cats.json')))):
        out = str(tmp_path / ('out%d' % k))
        for mode, sub in (('flat', 'vis_flat'), ('overlay', 'vis')):
            got = DS().vis_panoptic([cuda(p) for p, _ in scenes], out, mode=mode, label_min_area=100, **kw)
            assert got == [os.path.join(out, sub, '%012d.png' % i) for i in (5, 9)]
            for path, (pred, image) in zip(got, scenes):
                want = pan_vis_ref.render_flat(pred, CATS19) if mode == 'flat' else pan_vis_ref.render_overlay(pred, CATS19, image, font(), 100)[0]
                same(np.asarray(Image.open(path)), want, path)
