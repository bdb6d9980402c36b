"""CPU: the detection visualisations (config.test.vis_mask, dataset/vis.py) -- the drawing rule's numpy
restatement against hand-derived pictures, the reference's iteration over the results, labels, colours, file names, the config key,
the command line and its refusals, and the font table of the library."""
import copy
import os

import numpy as np
import pytest

from conftest import ROOT  # noqa: F401  (puts the repo root on sys.path)
import vis_cases
import vis_ref
from test_dataset_run_cpu import make_dataset, write_cfg


@pytest.fixture()
def saved_config():
    from upsnet_amd.config.config import config
    saved = copy.deepcopy(dict(config))
    yield config
    config.clear()
    config.update(saved)


def _font():
    from upsnet_amd.dataset import vis
    return vis.font_table()


# ------------------------------------------------------------------------------------------------ the rule
@pytest.mark.parametrize('case', vis_cases.hand_cases(), ids=lambda c: c[0])
def test_restatement_draws_the_hand_derived_pictures(case):
    name, boxes, labels, colours, masks, want = case
    got = vis_ref.render(vis_cases.hand_image(), boxes, labels, colours, masks, _font())
    assert got.dtype == np.uint8 and got.shape == want.shape
    assert np.array_equal(got, want), (name, np.argwhere((got != want).any(2))[:8])


def test_order_of_overlapping_detections_matters():
    cases = {c[0]: c for c in vis_cases.hand_cases()}
    a, b = cases['orange_then_blue'][5], cases['blue_then_orange'][5]
    differ = np.argwhere((a != b).any(2))
    assert sorted(map(tuple, differ.tolist())) == [(4, 4), (4, 5), (5, 4), (5, 5)]      # (y, x): the four shared pixels


def test_blend_is_the_stated_integer_formula():
    from upsnet_amd.dataset import vis
    assert vis.blend(40, 200, 1, 2) == 120 and vis.blend(120, 255, 1, 2) == 188 and vis.blend(80, 128, 2, 5) == 99
    assert vis.blend(255, 255, 1, 2) == 255 and vis.blend(0, 0, 2, 5) == 0 and vis.blend(1, 0, 1, 2) == 1
    v = np.arange(256)
    assert np.array_equal(vis.blend(v, 255, 2, 5), vis_ref.blend(v, 255, 2, 5))


def test_mask_transitions_round_trip():
    rng = np.random.default_rng(3)
    for H, W in ((5, 7), (1, 9), (9, 1), (16, 24)):
        masks = [rng.random((H, W)) < p for p in (0.0, 0.3, 0.7, 1.0)]
        trans = [vis_ref.mask_transitions(m) for m in masks]
        off = np.concatenate([[0], np.cumsum([len(t) for t in trans])])
        back = vis_ref.dense_masks(np.concatenate(trans), off, H, W)
        assert all(np.array_equal(a, b) for a, b in zip(masks, back))
        got_t, got_off = vis_cases.scene_transitions(masks, H, W)          # through the RLE strings and the product's decoder
        assert np.array_equal(got_t, np.concatenate(trans)) and np.array_equal(got_off, off)


# ------------------------------------------------------------------------------------------------ labels, iteration, colours, names
def test_label_strings():
    from upsnet_amd.dataset.vis import format_label
    assert format_label('car', np.float32(0.87)) == 'car.87'
    assert format_label('car', np.float32(0.5)) == 'car.50'
    assert format_label('person', np.float32(1.0)) == 'person1.00'
    as_float32 = ('%.2f' % float(np.float32(0.995))).lstrip('0')
    assert as_float32 in ('.99', '1.00') and format_label('bus', 0.995) == 'bus' + as_float32
    assert format_label('bus', np.float32(0.004)) == 'bus.00'


def _reference_iteration(all_boxes, all_masks, i, classes):
    """upsnet/dataset/base_dataset.py:858-871, the loops alone."""
    out = []
    for j, name in enumerate(classes):
        if name == '__background__':
            continue
        boxes = all_boxes[j][i]
        segms = all_masks[j][i]
        if segms == []:
            continue
        for k in range(boxes.shape[0]):
            score = boxes[k, -1]
            if score < 0.5:
                continue
            out.append((j, k))
    return out


def test_kept_detections_follow_the_reference_iteration():
    from upsnet_amd.dataset.vis import kept_detections
    classes = ['__background__', 'person', 'rider', 'car', 'truck']
    rle = lambda t: {'size': [4, 4], 'counts': t}          # noqa: E731  (never decoded here)
    scores = {1: [0.9, 0.499999, 0.5, 1.0, 0.995], 2: [], 3: [0.3, 0.49], 4: [0.51]}
    all_boxes, all_masks = [[]], [[]]
    for j in range(1, 5):
        s = np.asarray(scores[j], np.float32)
        b = np.hstack([np.arange(4 * len(s), dtype=np.float32).reshape(-1, 4) + j, s[:, None]]).astype(np.float32)
        all_boxes.append([None, b if len(s) else np.zeros((0, 5), np.float32)])
        all_masks.append([None, [rle('m%d_%d' % (j, k)) for k in range(len(s))]])
    kept = kept_detections(all_boxes, all_masks, 1, classes)
    assert [(e[0], e[1]) for e in kept] == _reference_iteration(all_boxes, all_masks, 1, classes) == [(1, 0), (1, 2), (1, 3), (1, 4), (4, 0)]
    assert [e[4] for e in kept] == ['person.90', 'person.50', 'person1.00', 'person' + ('%.2f' % float(np.float32(0.995))).lstrip('0'),
                                    'truck.51']
    assert all(e[2].dtype == np.float32 and e[2].shape == (4,) for e in kept)
    assert np.array_equal(kept[1][2], all_boxes[1][1][2, :4]) and kept[1][5] == rle('m1_2')
    assert kept[4][5] == rle('m4_0')


def test_coco_colour_sequence():
    from upsnet_amd.dataset.vis import blend, coco_colour
    assert coco_colour(0) == (blend(31, 255, 2, 5), blend(113, 255, 2, 5), blend(197, 255, 2, 5)) == (121, 170, 220)
    assert coco_colour(3) == tuple((c * 3 + 512) // 5 for c in ((97 * 3 + 31) % 256, (57 * 3 + 113) % 256, (181 * 3 + 197) % 256))
    cols = [coco_colour(k) for k in range(256)]
    assert len(set(cols)) == 256 and all(102 <= v <= 255 for c in cols for v in c)
    assert coco_colour(256) == coco_colour(0)


def test_dataset_classes_draw_with_the_reference_signature(tmp_path, saved_config, monkeypatch):
    import inspect
    from upsnet_amd.config.config import update_config
    from upsnet_amd.dataset import Cityscapes, coco, vis
    from upsnet_amd.dataset.base_dataset import BaseDataset
    for cls in (BaseDataset, Cityscapes):
        assert list(inspect.signature(cls.vis_all_mask).parameters) == ['self', 'all_boxes', 'all_masks', 'save_path']
        assert inspect.signature(cls.vis_all_mask).parameters['save_path'].default is None
    assert Cityscapes.vis_all_mask is not BaseDataset.vis_all_mask and coco.vis_all_mask is BaseDataset.vis_all_mask
    seen = {}

    def fake(dataset, all_boxes, all_masks, class_names, colour_of, name_of, save_path=None):
        seen[type(dataset).__name__] = (list(class_names), [colour_of(j, 7) for j in range(1, len(class_names))],
                                        [name_of(e) for e in dataset.roidb], save_path)
        return []
    monkeypatch.setattr(vis, 'vis_all_mask', fake)
    for kind, image_set in (('Cityscapes', 'val'), ('coco', 'val2017')):
        root = str(tmp_path / kind)
        make_dataset(root, kind, [(8, 12), (8, 12)], seed=1)
        update_config(write_cfg(tmp_path, kind, root, image_set, name='%s.yaml' % kind))
        ds = (Cityscapes if kind == 'Cityscapes' else coco)(image_sets=[image_set], phase='test')
        ds.vis_all_mask([[]] * 9, [[]] * 9, str(tmp_path / 'vis'))
    names, colours, files, save_path = seen['Cityscapes']
    assert names == ['__background__', 'person', 'rider', 'car', 'truck', 'bus', 'train', 'motorcycle', 'bicycle']
    assert colours == [(220, 20, 60), (255, 0, 0), (0, 0, 142), (0, 0, 70), (0, 60, 100), (0, 80, 100), (0, 0, 230), (119, 11, 32)]
    assert files == ['city1_000001_000019.png', 'city2_000002_000019.png'] and save_path == str(tmp_path / 'vis')
    names, colours, files, _ = seen['coco']
    assert names == ['__background__'] + ['cat%d' % c for c in range(1, 9)]
    assert colours == [vis.coco_colour(7)] * 8
    assert files == ['000000000001.jpg.png', '000000000002.jpg.png']


# ------------------------------------------------------------------------------------------------ config and command line
def test_config_default_and_flag(tmp_path, saved_config):
    from upsnet_amd.config.config import config
    from upsnet_amd.config.parse_args import parse_args
    assert config.test.vis_mask is False
    root = str(tmp_path / 'cs')
    make_dataset(root, 'Cityscapes', [(8, 12)], seed=1)
    cfg = write_cfg(tmp_path, 'Cityscapes', root, 'val')
    args = parse_args('', ['--cfg', cfg])
    assert args.vis_mask is False and config.test.vis_mask is False
    args = parse_args('', ['--cfg', cfg, '--vis_mask'])
    assert args.vis_mask is True and config.test.vis_mask is True
    cfg_on = write_cfg(tmp_path, 'Cityscapes', root, 'val', name='on.yaml', extra='  vis_mask: true\n')
    config.test.vis_mask = False
    parse_args('', ['--cfg', cfg_on])
    assert config.test.vis_mask is True


@pytest.mark.parametrize('extra,flag', [('network:\n  has_mask_head: false\n', True), ('network:\n  has_rcnn: false\n', True),
                                        ('network:\n  has_mask_head: false\ntest:\n  vis_mask: true\n', False)])
def test_vis_mask_needs_a_mask_head(extra, flag, tmp_path, saved_config):
    from upsnet_amd.evaluate import main
    root = str(tmp_path / 'cs')
    make_dataset(root, 'Cityscapes', [(8, 12)], seed=1)
    head = write_cfg(tmp_path, 'Cityscapes', root, 'val')
    text = open(head).read()
    if 'test:\n' in extra:       # one `test:` and one `network:` mapping per yaml
        net, tst = extra.split('test:\n')
        text = text.replace('network:\n', net).replace('test:\n', 'test:\n' + tst)
    else:
        text = text.replace('network:\n', extra)
    cfg = tmp_path / 'refuse.yaml'
    cfg.write_text(text)
    with pytest.raises(SystemExit) as e:
        main(['--cfg', str(cfg), '--synthetic_weights'] + (['--vis_mask'] if flag else []))
    assert 'vis_mask' in str(e.value) and 'has_mask_head' in str(e.value) and 'has_rcnn' in str(e.value)


def test_vis_mask_eval_only_checks_the_images_first(tmp_path, saved_config):
    """With --eval_only the images are read again: a missing one is reported before anything is drawn or scored."""
    import pickle
    from upsnet_amd.evaluate import final_output_path, main
    from upsnet_amd.config.config import update_config
    root = str(tmp_path / 'cs')
    _, paths = make_dataset(root, 'Cityscapes', [(8, 12), (8, 12)], seed=1,
                            anno_name='image_info_test.json')       # a set without ground truth: no GT file is asked for
    cfg = write_cfg(tmp_path, 'Cityscapes', root, 'test')
    update_config(cfg)
    results_dir = os.path.join(final_output_path(cfg), 'results')
    os.makedirs(results_dir)
    with open(os.path.join(results_dir, 'results_list.pkl'), 'wb') as f:
        pickle.dump({'all_boxes': [[]] * 9, 'all_masks': [[]] * 9, 'all_ssegs': [], 'all_panos': [], 'all_pano_cls_inds': []}, f)
    os.remove(paths[2])
    with pytest.raises(FileNotFoundError) as e:
        main(['--cfg', cfg, '--eval_only', '--vis_mask'])
    assert os.path.basename(paths[2]) in str(e.value)
    assert not os.path.exists(os.path.join(results_dir, 'vis'))


# ------------------------------------------------------------------------------------------------ the font
def test_font_table_and_the_glyphs_of_car87():
    font = _font()
    assert font.shape == (95, 8) and font.dtype == np.uint8
    assert not font[:, 7].any() and int(font.max()) < 32 and not font[0].any()        # eighth row, sixth column, the space
    assert len({bytes(font[c]) for c in range(95)}) == 95                              # no two characters look alike
    for ch, rows in vis_cases.CAR87.items():
        art = [''.join('#' if int(font[ord(ch) - 32][r]) >> (4 - c) & 1 else '.' for c in range(5)) for r in range(7)]
        assert art == rows, (ch, art)


def test_limits_are_those_of_the_library():
    from upsnet_amd._lib import lib
    from upsnet_amd.dataset import vis
    assert lib().upsnet_vis_max_detections() == vis.MAX_DETECTIONS == 256
    assert lib().upsnet_vis_max_label() == vis.MAX_LABEL == 32
    recs = lib().upsnet_vis_workspace_bytes(0, 1, 1)
    assert recs > 0 and lib().upsnet_vis_workspace_bytes(3, 33, 5) == recs + 3 * 5 * 2 * 4       # a column of 33 rows is two words
    for n, h, w in ((257, 8, 8), (-1, 8, 8), (1, 0, 8), (1, 8, 32769), (1, 32768, 16384)):
        assert lib().upsnet_vis_workspace_bytes(n, h, w) == 0
    assert lib().upsnet_vis_workspace_bytes(1, 16384, 16384) > 0
    seen = []

    def refused():      # (the error text is per thread: a thread of its own leaves the test session's untouched)
        rc = lib().upsnet_vis_render(None, None, 8, 8, 0, None, None, None, None, None, None, 0, None, None)
        seen.append((rc, lib().upsnet_last_error()))
    import threading
    th = threading.Thread(target=refused)
    th.start()
    th.join()
    assert seen[0][0] != 0 and b'null pointer' in seen[0][1]
