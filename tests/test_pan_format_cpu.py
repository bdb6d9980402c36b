"""CPU: the COCO panoptic format, host side -- the numpy restatement of the reference's converter (tests/pan_format_ref.py) against
hand-derived cases, the colour rule of dataset/pan_format.py, the restated general PQ against the PQ restatement of
tests/test_pq_cpu.py on every golden case, every host-side refusal (raised before any launch), the command line, file naming."""
import json
import os

import numpy as np
import pytest

from pan_format_ref import convert_2ch, pq_general, rgb_to_id
from test_dataset_run_cpu import make_dataset, saved_config, write_cfg  # noqa: F401  (saved_config is a fixture)
from test_pq_cpu import golden, golden_categories, golden_images, pq_restated

CATS = {c: {'id': c, 'isthing': int(c >= 11)} for c in range(19)}


def fixed(color):
    return lambda sem: color


def areas_consistent(images):
    """True iff every GT segment's JSON area equals its pixel count (then a GT segment matches at most one prediction and the IoU sum
    does not depend on the order of the pred ids)."""
    for _, gt, info in images:
        ids, counts = np.unique(rgb_to_id(gt), return_counts=True)
        count = dict(zip(ids.tolist(), counts.tolist()))
        if any(el['area'] != count.get(el['id'], 0) for el in info):
            return False
    return True


# ------------------------------------------------------------------------------------------------ the restated converter
def test_converter_hand_derived_cases():
    pan = np.full((5, 7, 3), 255, np.uint8)
    pan[..., 2] = 0
    pan[:, :, 1] = 9                      # VOID with a non-zero instance: no segment
    pan[3, 4, :2] = (12, 1)               # one pixel
    rgb, info = convert_2ch(pan, fixed([10, 20, 30]))
    assert info == [{'id': 10 + 256 * 20 + 65536 * 30, 'category_id': 12, 'iscrowd': 0, 'bbox': [4, 3, 0, 0], 'area': 1}]
    assert rgb[3, 4].tolist() == [10, 20, 30] and rgb.sum() == 60 and rgb.dtype == np.uint8
    # a segment touching all four borders (a frame), one inside it, in ascending (category, instance)
    pan = np.zeros((6, 9, 3), np.uint8)
    pan[..., 0] = 3
    pan[1:5, 1:8, 0] = 11
    pan[1:5, 1:8, 1] = 2
    pan[2:4, 3:5, 1] = 1
    colors = iter([[1, 0, 0], [2, 0, 0], [3, 0, 0]])
    rgb, info = convert_2ch(pan, lambda sem: next(colors))
    assert [(el['category_id'], el['id'], el['bbox'], el['area']) for el in info] == \
        [(3, 1, [0, 0, 8, 5], 54 - 28), (11, 2, [3, 2, 1, 1], 4), (11, 3, [1, 1, 6, 3], 24)]
    assert rgb[0, 0, 0] == 1 and rgb[2, 3, 0] == 2 and rgb[1, 1, 0] == 3
    # all VOID
    rgb, info = convert_2ch(np.full((4, 4, 3), 255, np.uint8), fixed([9, 9, 9]))
    assert info == [] and not rgb.any()
    # every value is a plain int
    assert all(type(v) is int for el in convert_2ch(pan, fixed([5, 5, 5]))[1] for v in [el['id'], el['area']] + el['bbox'])


# ------------------------------------------------------------------------------------------------ colours
def test_default_colour():
    from upsnet_amd.dataset.pan_format import ColorGenerator, category_table, default_color
    cols = [tuple(default_color(c)) for c in range(255)]
    assert len(set(cols)) == 255 and (0, 0, 0) not in cols and all(0 <= v <= 255 for c in cols for v in c)
    assert default_color(0) == [41, 83, 127] and default_color(7) == [(67 * 7 + 41) % 256, (137 * 7 + 83) % 256, (29 * 7 + 127) % 256]
    g = ColorGenerator(CATS)
    assert g.get_color(3) == default_color(3) and g.get_color(12) == default_color(12)
    t = category_table(CATS)
    assert t.dtype == np.int32 and t.shape == (256,) and t[19] == -1 and t[255] == -1
    r, gg, b = default_color(12)
    assert t[12] == (r | gg << 8 | b << 16 | 1 << 24) and t[3] >> 24 == 0
    assert category_table({5: {'isthing': 1, 'color': [1, 2, 3]}})[5] == (1 | 2 << 8 | 3 << 16 | 1 << 24)
    with pytest.raises(ValueError):
        category_table({5: {'isthing': 1, 'color': [1, 2, 300]}})
    with pytest.raises(ValueError):
        category_table({255: {'isthing': 1}})


def test_colour_rule():
    from upsnet_amd.dataset.pan_format import ColorGenerator, color_attempt
    cats = {1: {'isthing': 0, 'color': [100, 100, 100]}, 2: {'isthing': 0, 'color': [110, 100, 100]},
            5: {'isthing': 1, 'color': [105, 100, 100]},      # both stuff colours lie within +-30 of it
            6: {'isthing': 1, 'color': [100, 100, 100]},      # its base is a stuff colour: never handed out
            7: {'isthing': 1, 'color': [2, 1, 0]},            # near the clamp
            8: {'isthing': 1, 'color': [0, 0, 0]}}            # black: not even the first instance may take it
    stuff = {(100, 100, 100), (110, 100, 100)}

    def draw():
        g = ColorGenerator(cats)
        out = {c: [tuple(g.get_color(c)) for _ in range(256)] for c in (5, 6, 7, 8)}
        out[1] = [tuple(g.get_color(1))]
        out[2] = [tuple(g.get_color(2))]
        return out
    a, b = draw(), draw()
    assert a == b                                             # deterministic
    assert a[1] == [(100, 100, 100)] and a[2] == [(110, 100, 100)]
    assert a[5][0] == (105, 100, 100) and a[7][0] == (2, 1, 0)
    assert a[6][0] != (100, 100, 100) and a[8][0] != (0, 0, 0)
    things = [c for k in (5, 6, 7, 8) for c in a[k]]
    assert len(set(things)) == 4 * 256                        # unique within the image, 256 instances of a category included
    assert (0, 0, 0) not in things and not stuff & set(things)
    for k in (5, 6, 7, 8):
        base = cats[k]['color']
        assert all(abs(v - w) <= 30 and 0 <= v <= 255 for c in a[k] for v, w in zip(c, base)), k
    assert max(max(c) for c in a[8]) <= 30                    # the clamp: only [0, 30]^3 is reachable from black
    # the sequence is a function of (category, ordinal, attempt) and visits every cell of the cube once
    assert color_attempt((100, 100, 100), 5, 3, 0) == color_attempt((100, 100, 100), 5, 3, 0)
    seen = {color_attempt((100, 100, 100), 5, 3, k) for k in range(61 ** 3)}
    assert len(seen) == 61 ** 3
    # a further segment of a stuff category gets a colour of its own, so ids stay unique
    g = ColorGenerator(cats)
    first, second = tuple(g.get_color(1)), tuple(g.get_color(1))
    assert first == (100, 100, 100) and second not in stuff and second != first
    with pytest.raises(KeyError):
        g.get_color(40)


# ------------------------------------------------------------------------------------------------ general PQ restatement
def test_general_pq_restatement_matches_the_2ch_restatement_on_the_golden():
    from upsnet_amd.dataset.pan_format import ColorGenerator
    g = golden()
    cats = golden_categories(g)
    exact = 0
    for name in sorted(g['cases'].tolist()):
        images = golden_images(g, name)
        want = pq_restated(images, cats)
        conv = [convert_2ch(pred, ColorGenerator(cats).get_color) for pred, _, _ in images]
        for (rgb, info), (pred, _, _) in zip(conv, images):
            ids = [el['id'] for el in info]
            assert len(set(ids)) == len(ids) and 0 not in ids, name
            assert sum(el['area'] for el in info) == int((np.asarray(pred)[..., 0] != 255).sum()), name
        got = pq_general([(rgb, info, gt, segs) for (rgb, info), (_, gt, segs) in zip(conv, images)], cats)
        np.testing.assert_array_equal(np.stack(got[:3]), np.stack(want[:3]), err_msg=name)
        if areas_consistent(images):
            exact += 1
            assert np.array_equal(got[3].view(np.int64), want[3].view(np.int64)), name
        else:   # several preds can match one GT segment and are then added in pred-id order: one ulp of the sum
            assert np.all(np.abs(got[3] - want[3]) <= np.spacing(np.maximum(got[3], want[3]))), name
    assert exact >= 10


def test_general_pq_restatement_sanity_checks():
    rgb = np.zeros((4, 4, 3), np.uint8)
    rgb[:2, :, 0] = 7
    info = [{'id': 7, 'category_id': 3}]
    gt = np.zeros((4, 4, 3), np.uint8)
    tp, fp, fn, iou = pq_general([(rgb, info, gt, [])], CATS)
    assert fp.sum() == 0 and tp.sum() == 0        # wholly on VOID: absorbed
    with pytest.raises(KeyError, match="image 1: segment 7 is in the PNG"):
        pq_general([(rgb, info, gt, []), (rgb, [], gt, [])], CATS)
    with pytest.raises(KeyError, match=r"image 0: segments \[9\] are in the JSON"):
        pq_general([(rgb, info + [{'id': 9, 'category_id': 3}], gt, [])], CATS)
    with pytest.raises(KeyError, match="unknown category_id 77"):
        pq_general([(rgb, [{'id': 7, 'category_id': 77}], gt, [])], CATS)


# ------------------------------------------------------------------------------------------------ host refusals, before any launch
def _img(H=8, W=8):
    return np.zeros((H, W, 3), np.uint8)


@pytest.mark.parametrize("segs,what", [
    ([{'id': 3, 'category_id': 1}, {'id': 3, 'category_id': 2}], "duplicate"),
    ([{'id': 0, 'category_id': 1}], "id 0"),
    ([{'id': 1 << 24, 'category_id': 1}], "2\\^24"),
    ([{'id': 4, 'category_id': 255}], "0..254"),
    ([{'id': 4, 'category_id': -1}], "0..254"),
    ([{'id': i + 1, 'category_id': 1} for i in range(257)], "more than 256"),
])
def test_add_png_refuses_on_the_host(segs, what):
    from upsnet_amd.dataset.pq import PanopticEvaluator
    ev = PanopticEvaluator({1: {'isthing': 0}, 2: {'isthing': 1}}, device='cuda:0')
    with pytest.raises(ValueError, match=what):
        ev.add_png(_img(), segs, _img(), [])
    assert ev._state is None and ev.num_images == 0   # nothing allocated, nothing queued


def test_add_png_refuses_shapes_and_gt():
    from upsnet_amd.dataset.pq import PanopticEvaluator
    ev = PanopticEvaluator({1: {'isthing': 0}}, device='cuda:0')
    with pytest.raises(ValueError, match="differ in shape"):
        ev.add_png(_img(8, 8), [], _img(8, 9), [])
    with pytest.raises(ValueError, match=r"uint8 \[H,W,3\]"):
        ev.add_png(_img().astype(np.int32), [], _img(), [])
    with pytest.raises(ValueError, match="duplicate GT"):
        ev.add_png(_img(), [], _img(), [{'id': 3, 'category_id': 1, 'iscrowd': 0, 'area': 1}] * 2)
    assert ev._state is None


def test_segments_table_slots_ascend_with_the_id():
    from upsnet_amd.dataset.pan_format import segments_table
    t = segments_table([{'id': 900, 'category_id': 4}, {'id': 5, 'category_id': 7}, {'id': 17, 'category_id': 4}, {'id': 16777215, 'category_id': 4}])
    assert t.dtype == np.int32 and t.tolist() == [[5, 7, 0], [17, 4, 0], [900, 4, 1], [16777215, 4, 2]]
    assert segments_table([]).shape == (0, 3)


def test_write_panoptic_refuses_on_the_host(tmp_path):
    from upsnet_amd.dataset.pan_format import write_panoptic
    ims = [{'id': 1, 'file_name': 'a.jpg'}, {'id': 2, 'file_name': 'b.jpg'}]
    with pytest.raises(ValueError, match="1 predictions for 2 images"):
        write_panoptic([_img()], ims, CATS, str(tmp_path))
    with pytest.raises(ValueError, match="image ids"):
        write_panoptic([_img(), _img()], ims, CATS, str(tmp_path), image_ids=[1])
    with pytest.raises(ValueError, match="file_name"):
        write_panoptic([_img()], [{'id': 1}], CATS, str(tmp_path))
    with pytest.raises(ValueError, match="share one output name"):
        write_panoptic([_img(), _img()], [{'id': 1, 'file_name': 'a.jpg'}, {'id': 2, 'file_name': 'a.png'}], CATS, str(tmp_path))
    with pytest.raises(ValueError, match=r"uint8 \[H,W,3\]"):
        write_panoptic([_img()[:, :, 0]], ims[:1], CATS, str(tmp_path))
    with pytest.raises(ValueError, match="0..254"):
        write_panoptic([_img()], ims[:1], {300: {'isthing': 0}}, str(tmp_path))
    assert not os.listdir(str(tmp_path))


def _panoptic_dataset(tmp_path, pred_anns, gt_ids=(1, 2)):
    from PIL import Image
    from upsnet_amd.dataset.base_dataset import BaseDataset
    folder = tmp_path / "gt"
    folder.mkdir()
    for i in gt_ids:
        Image.fromarray(_img()).save(folder / ("%s.png" % i))
    js = {'images': [{'id': i, 'file_name': '%s.png' % i} for i in gt_ids],
          'annotations': [{'image_id': i, 'file_name': '%s.png' % i, 'segments_info': []} for i in gt_ids],
          'categories': [{'id': 3, 'isthing': 1}]}
    (tmp_path / "gt.json").write_text(json.dumps(js))
    (tmp_path / "pred.json").write_text(json.dumps({'annotations': pred_anns}))

    class DS(BaseDataset):
        panoptic_json_file = str(tmp_path / "gt.json")
        panoptic_gt_folder = str(folder)
    return DS()


@pytest.mark.parametrize("ids,what", [((1,), "1 GT images without a prediction"), ((1, 2, 3), "1 predictions without a GT image"),
                                      ((1, 2, 2), "occurs twice")])
def test_evaluate_panoptic_files_refuses_missing_and_surplus_images(tmp_path, ids, what):
    ds = _panoptic_dataset(tmp_path, [{'image_id': i, 'file_name': '%d.png' % i, 'segments_info': []} for i in ids])
    with pytest.raises(ValueError, match=what):
        ds.evaluate_panoptic_files(str(tmp_path / "pred.json"), str(tmp_path / "gt"))


def test_dataset_write_panoptic_needs_categories_without_gt(tmp_path):
    from upsnet_amd.dataset.base_dataset import BaseDataset

    class DS(BaseDataset):
        has_gt = False
        name = 'coco_test-dev2017'
        roidb = [{'id': 5, 'file_name': '000000000005.jpg'}]
    with pytest.raises(ValueError, match="no ground truth and so no category table"):
        DS().write_panoptic([_img()], str(tmp_path / "out"))
    assert not (tmp_path / "out").exists()


# ------------------------------------------------------------------------------------------------ command line, naming
def test_parse_args_accepts_the_new_flags():
    from upsnet_amd.config.parse_args import parse_args
    a = parse_args('', [])
    assert a.write_panoptic is False and a.score_panoptic == '' and a.score_panoptic_folder == '' and a.panoptic_categories == ''
    a = parse_args('', ['--write_panoptic', '--score_panoptic', 'p/pred.json', '--score_panoptic_folder', 'p/pan', '--panoptic_categories', 'c.json'])
    assert a.write_panoptic and a.score_panoptic == 'p/pred.json' and a.score_panoptic_folder == 'p/pan' and a.panoptic_categories == 'c.json'


def test_evaluate_option_checks(tmp_path, saved_config):
    from upsnet_amd.evaluate import main
    root = str(tmp_path / 'Cityscapes')
    make_dataset(root, 'Cityscapes', [(64, 128)])
    no_pan = write_cfg(tmp_path, 'Cityscapes', root, 'val', name='no_pan.yaml')
    with open(no_pan) as f:
        text = f.read()
    assert "network:\n" in text
    with open(no_pan, 'w') as f:
        f.write(text.replace("network:\n", "network:\n  has_panoptic_head: false\n"))
    with pytest.raises(SystemExit, match="--write_panoptic writes the panoptic predictions"):
        main(['--cfg', no_pan, '--synthetic_weights', '--write_panoptic'])
    cfg = write_cfg(tmp_path, 'Cityscapes', root, 'val')
    with pytest.raises(SystemExit, match="--score_panoptic_folder names the PNG folder"):
        main(['--cfg', cfg, '--score_panoptic_folder', str(tmp_path)])
    with pytest.raises(SystemExit, match="no prediction JSON"):
        main(['--cfg', cfg, '--score_panoptic', str(tmp_path / 'nope.json')])
    (tmp_path / 'pred.json').write_text('{"annotations": []}')
    with pytest.raises(SystemExit, match="no PNG folder"):
        main(['--cfg', cfg, '--score_panoptic', str(tmp_path / 'pred.json')])


def test_png_names():
    from upsnet_amd.dataset.pan_format import png_name
    assert png_name('frankfurt_000000_000294_leftImg8bit.png') == 'frankfurt_000000_000294.png'
    assert png_name('000000000139.jpg') == '000000000139.png'
    assert png_name('a/b_leftImg8bit.jpeg') == 'a/b.png'
    assert png_name('plain.png') == 'plain.png'
