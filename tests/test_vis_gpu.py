"""GPU: the detection visualisations (csrc/vis_render.hip, dataset/vis.py) against the numpy restatement of the drawing rule
(tests/vis_ref.py), byte for byte: hand-derived pictures, seeded random scenes over the image sizes of an evaluation set, poisoned and
guard-banded outputs and workspaces, and `python -m upsnet_amd.evaluate --vis_mask` in both modes on generated datasets."""
import copy
import os
import pickle

import numpy as np
import pytest
import torch

from conftest import gen_dets
import memguard
import size_population
import vis_cases
import vis_ref
from test_dataset_run_cpu import make_dataset, write_cfg

pytestmark = pytest.mark.gpu

VIS_MODULE = ('upsnet_amd.dataset.vis',)


@pytest.fixture()
def saved_config():
    from upsnet_amd.config.config import config
    saved = copy.deepcopy(dict(config))
    yield config
    config.clear()
    config.update(saved)


def _device_render(image, boxes, labels, colours, masks):
    from upsnet_amd.dataset import vis
    H, W = image.shape[:2]
    trans, off = vis_cases.scene_transitions(masks, H, W)
    out = vis.render_detections(torch.from_numpy(image).cuda(), boxes, labels, colours, trans, off)
    torch.cuda.synchronize()
    assert out.dtype == torch.uint8 and tuple(out.shape) == (H, W, 3) and out.is_cuda
    return out.cpu().numpy()


def _check_scene(seed, H, W, n, **kw):
    from upsnet_amd.dataset import vis
    image, boxes, labels, colours, masks = vis_cases.random_scene(seed, H, W, n, gen_dets, **kw)
    got = _device_render(image, boxes, labels, colours, masks)
    want = vis_ref.render(image, boxes, labels, colours, masks, vis.font_table())
    bad = np.argwhere((got != want).any(2))
    assert bad.size == 0, ('%d x %d, %d detections: %d pixels differ, first (y, x) %s' % (H, W, n, len(bad), bad[:5].tolist()))


# ------------------------------------------------------------------------------------------------ hand cases
@pytest.mark.parametrize('case', vis_cases.hand_cases(), ids=lambda c: c[0])
def test_device_draws_the_hand_derived_pictures(case):
    name, boxes, labels, colours, masks, want = case
    got = _device_render(vis_cases.hand_image(), np.asarray(boxes, np.float32), labels, colours, masks)
    assert np.array_equal(got, want), (name, np.argwhere((got != want).any(2))[:8].tolist())


# ------------------------------------------------------------------------------------------------ random scenes
def _population():
    sizes = [r for r, _ in size_population.one_per_padded(size_population.coco_padded_sizes())]
    return sizes + [r for r, _ in size_population.cityscapes_sizes()]


def test_image_size_population_matches_restatement():
    sizes = _population()
    assert len(sizes) > 20 and any(h % 32 or w % 64 for h, w in sizes)
    for k, (h, w) in enumerate(sizes):
        _check_scene(100 + k, h, w, 3 + k % 4)


@pytest.mark.parametrize('H,W,n', [(37, 1, 5), (1, 50, 5), (1, 1, 2), (31, 63, 9), (33, 65, 9), (64, 64, 9), (97, 130, 1), (97, 130, 0),
                                   (200, 333, 256), (512, 1024, 100), (375, 500, 100)])
def test_odd_sizes_and_detection_counts_match_restatement(H, W, n):
    _check_scene(7 * H + W + n, H, W, n)


def test_zero_pixel_and_full_image_masks():
    from upsnet_amd.dataset import vis
    H, W = 70, 90
    image = np.random.default_rng(5).integers(0, 256, (H, W, 3)).astype(np.uint8)
    masks = [np.zeros((H, W), bool), np.ones((H, W), bool), np.zeros((H, W), bool), np.ones((H, W), bool)]
    masks[2][H - 1, W - 1] = True
    masks[3][0, 0] = False
    boxes = np.array([[0, 0, W - 1, H - 1], [-0.5, -0.5, W, H], [W - 1, H - 1, W + 30, H + 30], [10.5, 30.2, 11.0, 30.9]], np.float32)
    labels, colours = ['car.87', 'person1.00', 'bus.50', '~{|}'], [(1, 2, 3), (250, 0, 9), (0, 255, 0), (255, 255, 255)]
    got = _device_render(image, boxes, labels, colours, masks)
    assert np.array_equal(got, vis_ref.render(image, boxes, labels, colours, masks, vis.font_table()))


def test_limits_are_refused_not_clamped():
    from upsnet_amd.dataset import vis
    image = torch.zeros((8, 8, 3), dtype=torch.uint8, device='cuda')
    n = vis.MAX_DETECTIONS + 1
    with pytest.raises(ValueError):
        vis.render_detections(image, np.zeros((n, 4), np.float32), ['a'] * n, np.zeros((n, 3), np.uint8), np.zeros(0, np.int32),
                              np.zeros(n + 1, np.int32))
    with pytest.raises(ValueError):
        vis.render_detections(image, np.zeros((1, 4), np.float32), ['a' * (vis.MAX_LABEL + 1)], np.zeros((1, 3), np.uint8),
                              np.zeros(0, np.int32), np.zeros(2, np.int32))
    with pytest.raises(ValueError):
        vis.render_detections(image, np.zeros((1, 4), np.float32), ['a'], np.zeros((1, 3), np.uint8), np.array([65], np.int32),
                              np.array([0, 1], np.int32))
    with pytest.raises(RuntimeError):
        vis.render_detections(image.cpu(), np.zeros((0, 4), np.float32), [], np.zeros((0, 3), np.uint8), np.zeros(0, np.int32),
                              np.zeros(1, np.int32))


# ------------------------------------------------------------------------------------------------ poisoned memory
def test_poisoned_output_and_workspace_two_images_of_different_size():
    """The header asks no zeroing of the workspace and promises every output byte: both patterns of poison, guard bands around the
    output and the workspace, two consecutive images of different size (the second smaller, then larger), twice."""
    from upsnet_amd.dataset import vis
    font = vis.font_table()
    scenes = [vis_cases.random_scene(40 + k, h, w, n, gen_dets) for k, (h, w, n) in enumerate([(150, 210, 12), (67, 95, 5), (190, 260, 20)])]
    wants = [vis_ref.render(s[0], s[1], s[2], s[3], s[4], font) for s in scenes]
    runs = []
    for pattern in ('A', 'B', 'A'):
        with memguard.poisoned(pattern, modules=VIS_MODULE) as guard:
            outs = []
            for image, boxes, labels, colours, masks in scenes:
                trans, off = vis_cases.scene_transitions(masks, image.shape[0], image.shape[1])
                outs.append(vis.render_detections(memguard.banded_copy(torch.from_numpy(image).cuda(), pattern), boxes, labels, colours,
                                                  trans, off))
            torch.cuda.synchronize()
            assert guard.count == 2 * len(scenes)            # the output and the workspace of every image
        runs.append([o.cpu().numpy() for o in outs])
    for outs in runs:
        for got, want in zip(outs, wants):
            assert np.array_equal(got, want)
    assert all(np.array_equal(a, b) for a, b in zip(runs[0], runs[2]))


# ------------------------------------------------------------------------------------------------ the real path and the CLI
def _boosted(all_boxes):
    """The results' boxes with every second detection's score lifted to 0.5 or above, so that the untrained model draws something."""
    out = []
    for per_image in all_boxes:
        rows = []
        for b in per_image:
            b = np.array(b, np.float32, copy=True)
            if b.ndim == 2 and b.shape[0]:
                b[::2, 4] = np.float32(0.5) + np.float32(0.49) * b[::2, 4]
            rows.append(b)
        out.append(rows)
    return out


def _expected(ds, all_boxes, all_masks, class_names, colour_of):
    from PIL import Image
    from upsnet_amd.dataset import vis
    font, counter, pictures, drawn = vis.font_table(), 0, [], 0
    for i, entry in enumerate(ds.roidb):
        image = np.asarray(Image.open(entry['image']).convert('RGB'))
        kept = vis.kept_detections(all_boxes, all_masks, i, class_names)
        trans, off = vis.rle_transitions([e[5] for e in kept], image.shape[0], image.shape[1])
        masks = vis_ref.dense_masks(trans, off, image.shape[0], image.shape[1])
        colours = [colour_of(e[0], counter + m) for m, e in enumerate(kept)]
        counter += len(kept)
        drawn += sum(int(m.any()) for m in masks)
        pictures.append(vis_ref.render(image, [e[2] for e in kept], [e[4] for e in kept], colours, masks, font))
    return pictures, counter, drawn


@pytest.mark.parametrize('kind', ['Cityscapes', 'coco'])
def test_evaluate_vis_mask_end_to_end(kind, tmp_path, saved_config):
    from PIL import Image
    from upsnet_amd.config.config import update_config
    from upsnet_amd.dataset import Cityscapes, coco, vis
    from upsnet_amd.dataset.cityscapes_pixel_eval import TRAIN_ID_COLOURS
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
    _write_gt(ds, chains, list(range(n)), ['img_%d' % e['id'] for e in ds.roidb] if kind == 'Cityscapes' else [e['id'] for e in ds.roidb])
    del model
    torch.cuda.empty_cache()

    # a run: the pickle is written, the pictures are drawn, nothing is scored
    res = main(['--cfg', cfg, '--synthetic_weights', '--vis_mask'])
    assert res['metrics'] == {} and res['times'] is not None
    results_dir = os.path.dirname(res['results_file'])
    with open(res['results_file'], 'rb') as f:
        got = pickle.load(f)
    if kind == 'Cityscapes':
        names = [os.path.basename(e['image'])[:-len('_leftImg8bit.png')] + '.png' for e in ds.roidb]
        class_names = ('__background__', 'person', 'rider', 'car', 'truck', 'bus', 'train', 'motorcycle', 'bicycle')
        colour_of = lambda j, k: TRAIN_ID_COLOURS[10 + j]          # noqa: E731
    else:
        names = [os.path.basename(e['image']) + '.png' for e in ds.roidb]
        class_names = ds.dataset.classes
        colour_of = lambda j, k: vis.coco_colour(k)                 # noqa: E731
    assert res['vis_files'] == [os.path.join(results_dir, 'vis', name) for name in names]
    assert sorted(os.listdir(os.path.join(results_dir, 'vis'))) == sorted(names)
    want, _, _ = _expected(ds, got['all_boxes'], got['all_masks'], class_names, colour_of)
    arrays = ds.vis_all_mask(got['all_boxes'], got['all_masks'])
    for path, w, a in zip(res['vis_files'], want, arrays):
        png = np.asarray(Image.open(path))
        assert png.dtype == np.uint8 and np.array_equal(png, w) and np.array_equal(a, w), path
        os.remove(path)

    # --eval_only: drawn first, then scored
    again = main(['--cfg', cfg, '--eval_only', '--vis_mask'])
    assert again['vis_files'] == res['vis_files'] and again['times'] is None
    assert {'box_ap', 'mask_ap', 'panoptic', 'sseg'} <= set(again['metrics'])
    for path, w in zip(again['vis_files'], want):
        assert np.array_equal(np.asarray(Image.open(path)), w), path

    # the real path with detections above the threshold: im_post's strings of the untrained model, every second score lifted
    boosted = _boosted(got['all_boxes'])
    want, kept, drawn = _expected(ds, boosted, got['all_masks'], class_names, colour_of)
    assert kept > 0 and drawn > 0
    arrays = ds.vis_all_mask(boosted, got['all_masks'], None)
    assert len(arrays) == n
    for i, (a, w) in enumerate(zip(arrays, want)):
        assert a.dtype == np.uint8 and np.array_equal(a, w), (i, np.argwhere((a != w).any(2))[:5].tolist())
