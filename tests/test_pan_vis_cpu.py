"""CPU: the panoptic drawing rule of DESIGN.md section 4.20 (tests/pan_vis_ref.py) against hand-derived pictures, the label rules, the
host-side checks of dataset/pan_vis.py, the command line and the entry point's argument refusals. The device is held to the same
pictures and to the restatement in tests/test_pan_vis_gpu.py."""
import copy
import ctypes

import numpy as np
import pytest

import pan_vis_ref
from test_dataset_run_cpu import make_dataset, write_cfg

S, T = (10, 20, 30), (200, 100, 50)          # the colours of the stuff category 1 and the thing category 12
W_, K = (255, 255, 255), (0, 0, 0)
CATS = {1: {'id': 1, 'isthing': 0, 'color': list(S), 'name': 'T'}, 12: {'id': 12, 'isthing': 1, 'color': list(T), 'name': 'T'}}
NO_LABELS = 1 << 30

# the glyph of 'T' in the label font: 5 x 7 dots (the sixth column and the eighth row of a cell are empty)
GLYPH_T = ['#####', '..#..', '..#..', '..#..', '..#..', '..#..', '..#..']
GLYPH_Q = ['.###.', '#...#', '....#', '...#.', '..#..', '.....', '..#..']      # '?'


@pytest.fixture()
def saved_config():
    from upsnet_amd.config.config import config
    saved = copy.deepcopy(dict(config))
    yield config
    config.clear()
    config.update(saved)


def font():
    from upsnet_amd.dataset import vis
    return vis.font_table()


def pred_of(cat, inst):
    cat, inst = np.asarray(cat, np.uint8), np.asarray(inst, np.uint8)
    return np.ascontiguousarray(np.stack([cat, inst, np.zeros_like(cat)], -1))


def picture(rows, legend):
    return np.array([[legend[ch] for ch in row.split()] for row in rows], np.uint8)


def paint_label(pic, left, top, glyphs):
    """The stated label step, written out independently of the restatement: black at 2/5 over the box of 12 x 16 pixels per glyph at
    (left, top), then every dot as a white 2 x 2 block; clipped to the picture."""
    H, W = pic.shape[:2]
    out = pic.astype(np.int64)
    for y in range(top, min(top + 16, H)):
        for x in range(left, min(left + 12 * len(glyphs), W)):
            u, v = x - left, y - top
            g, col, row = glyphs[u // 12], (u % 12) // 2, v // 2
            dot = row < 7 and col < 5 and g[row][col] == '#'
            out[y, x] = 255 if dot else (out[y, x] * 3 + 2) // 5
    return out.astype(np.uint8)


# ------------------------------------------------------------------------------------------------ hand-derived pictures
def flat_cases():
    """[(name, pred, categories, picture)] with every pixel written out."""
    L = {'S': S, 'T': T, 'W': W_, 'K': K}
    cases = []
    # a 3 x 3 instance (12, 1) at rows 2..4, columns 3..5 of a 6 x 6 stuff map, touching the right edge. Its edge pixels are the ring of
    # 8 (the centre (3, 4) has four neighbours of its own key). Widened by one pixel to the right and down the ring covers its own
    # centre ((3, 3) is to its left) and row 5; column 6 would leave the image.
    cat = np.full((6, 6), 1)
    inst = np.zeros((6, 6), int)
    cat[2:5, 3:6], inst[2:5, 3:6] = 12, 1
    cases.append(('ring_3x3_at_the_right_edge', pred_of(cat, inst), CATS, picture([
        'S S S S S S',
        'S S S S S S',
        'S S S W W W',
        'S S S W W W',
        'S S S W W W',
        'S S S W W W'], L)))
    # a 4 x 4 instance at rows 1..4, columns 1..4 of 7 x 7: the ring is 12 pixels, the widened ring is rows 1..5 x columns 1..5 without
    # (3, 3), whose left, upper and upper-left neighbours are all interior pixels
    cat = np.full((7, 7), 1)
    inst = np.zeros((7, 7), int)
    cat[1:5, 1:5], inst[1:5, 1:5] = 12, 1
    cases.append(('ring_4x4_keeps_one_interior_pixel', pred_of(cat, inst), CATS, picture([
        'S S S S S S S',
        'S W W W W W S',
        'S W W W W W S',
        'S W W T W W S',
        'S W W W W W S',
        'S W W W W W S',
        'S S S S S S S'], L)))
    # no contour around stuff, nor around a thing with instance number 0; VOID (whatever its instance) and a category that is not in
    # the table (40, instance 1) are black
    cat = np.array([[1] * 4, [12] * 4, [255] * 4, [40] * 4])
    inst = np.array([[0] * 4, [0] * 4, [7] * 4, [1] * 4])
    cases.append(('no_contour_void_and_unknown_category', pred_of(cat, inst), CATS, picture([
        'S S S S',
        'T T T T',
        'K K K K',
        'K K K K'], L)))
    # two instances side by side and a border towards VOID: every thing pixel is an edge pixel (rows 0..1 x columns 0..2); widened, the
    # contour also covers the VOID column 3 and row 2 up to column 3
    cat = np.array([[12, 12, 12, 255, 1], [12, 12, 12, 255, 1], [1, 1, 1, 1, 1]])
    inst = np.array([[1, 2, 2, 0, 0], [1, 2, 2, 0, 0], [0, 0, 0, 0, 0]])
    cases.append(('two_instances_and_void', pred_of(cat, inst), CATS, picture([
        'W W W W S',
        'W W W W S',
        'W W W W S'], L)))
    return cases


def overlay_hand_case():
    """4 x 4, image (100, 51, 200) everywhere: stuff (1, 0) on rows 0..2 x columns 0..2 (colour S, its centre is its only pixel that is
    no edge), the thing (12, 1) on column 3 of rows 0..2 (colour T, all edge), row 3 VOID.
      stuff: blend(100, 10) = 55, blend(51, 20) = 36, blend(200, 30) = 115; edge on top: 155, 146, 185
      thing: blend(100, 200) = 150, blend(51, 100) = 76, blend(200, 50) = 125; edge on top: 203, 166, 190"""
    cat = np.array([[1, 1, 1, 12]] * 3 + [[255] * 4])
    inst = np.array([[0, 0, 0, 1]] * 3 + [[0, 3, 0, 3]])
    image = np.empty((4, 4, 3), np.uint8)
    image[...] = (100, 51, 200)
    L = {'a': (55, 36, 115), 'A': (155, 146, 185), 'B': (203, 166, 190), 'I': (100, 51, 200)}
    want = picture(['A A A B', 'A a A B', 'A A A B', 'I I I I'], L)
    return pred_of(cat, inst), CATS, image, want


def one_blob(H, W, cy, cx, key=(12, 1)):
    """VOID everywhere but a 3 x 3 segment centred on (cy, cx)."""
    cat, inst = np.full((H, W), 255), np.zeros((H, W), int)
    cat[cy - 1:cy + 2, cx - 1:cx + 2], inst[cy - 1:cy + 2, cx - 1:cx + 2] = key
    return cat, inst


def label_cases():
    """[(name, pred, categories, image, label_min_area, [(left, top, glyphs)] in drawing order)]: the boxes are derived by hand from
    left = max(min(cx - 6 L, W - 12 L), 0), top = max(min(cy - 8, H - 16), 0)."""
    rng = np.random.default_rng(2)
    cases = []
    for name, cy, cx, box in (('pushed_in_from_the_left', 20, 1, (0, 12)), ('pushed_in_from_the_right', 20, 38, (28, 12)),
                              ('pushed_in_from_the_top', 1, 20, (14, 0)), ('pushed_in_from_the_bottom', 38, 20, (14, 24)),
                              ('centred', 20, 20, (14, 12))):
        cases.append((name, pred_of(*one_blob(40, 40, cy, cx)), CATS, rng.integers(0, 256, (40, 40, 3)).astype(np.uint8), 9,
                      [(box[0], box[1], [GLYPH_T])]))
    two = dict(CATS)
    two[12] = dict(CATS[12], name='TT')
    # an image narrower and lower than its label of 24 x 16: the box starts at (0, 0) and is clipped
    cases.append(('image_smaller_than_the_label', pred_of(*one_blob(12, 10, 5, 5)), two, rng.integers(0, 256, (12, 10, 3)).astype(np.uint8),
                  9, [(0, 0, [GLYPH_T, GLYPH_T])]))
    # two overlapping labels: (12, 1) centred on (11, 11) -> box (5, 3), (12, 2) centred on (11, 17) -> box (11, 3), drawn second
    cat, inst = one_blob(30, 30, 11, 11)
    cat[10:13, 16:19], inst[10:13, 16:19] = 12, 2
    cases.append(('two_overlapping_labels', pred_of(cat, inst), CATS, rng.integers(0, 256, (30, 30, 3)).astype(np.uint8), 9,
                  [(5, 3, [GLYPH_T]), (11, 3, [GLYPH_T])]))
    return cases


def label_case_picture(pred, cats, image, boxes):
    pic, _, _ = pan_vis_ref.render_overlay(pred, cats, image, font(), NO_LABELS)        # steps 1-3, checked by the 4 x 4 case
    for left, top, glyphs in boxes:
        pic = paint_label(pic, left, top, glyphs)
    return pic


@pytest.mark.parametrize('case', flat_cases(), ids=lambda c: c[0])
def test_flat_hand_derived_pictures(case):
    _, pred, cats, want = case
    got = pan_vis_ref.render_flat(pred, cats)
    assert got.dtype == np.uint8 and np.array_equal(got, want), np.argwhere((got != want).any(2)).tolist()


def test_overlay_hand_derived_picture():
    pred, cats, image, want = overlay_hand_case()
    got, qualified, drawn = pan_vis_ref.render_overlay(pred, cats, image, font(), NO_LABELS)
    assert np.array_equal(got, want) and (qualified, drawn) == (0, 0)
    assert pan_vis_ref.blend(100, 10, 1, 2) == 55 and pan_vis_ref.blend(55, 255, 1, 2) == 155 and pan_vis_ref.blend(155, 0, 2, 5) == 93


def test_glyphs_are_those_of_the_font():
    f = font()
    for ch, glyph in (('T', GLYPH_T), ('?', GLYPH_Q)):
        rows = [''.join('#' if f[ord(ch) - 32][r] >> (4 - c) & 1 else '.' for c in range(5)) for r in range(7)]
        assert rows == glyph and f[ord(ch) - 32][7] == 0


@pytest.mark.parametrize('case', label_cases(), ids=lambda c: c[0])
def test_label_hand_derived_boxes(case):
    name, pred, cats, image, min_area, boxes = case
    got, qualified, drawn = pan_vis_ref.render_overlay(pred, cats, image, font(), min_area)
    want = label_case_picture(pred, cats, image, boxes)
    assert np.array_equal(got, want), (name, np.argwhere((got != want).any(2))[:8].tolist())
    assert qualified == drawn == len(boxes)
    assert [(b[1], b[2]) for b in pan_vis_ref.label_boxes(pred, cats, min_area)[0]] == [(b[0], b[1]) for b in boxes]
    if name == 'two_overlapping_labels':         # the later key is on top: the other order is another picture
        assert not np.array_equal(want, label_case_picture(pred, cats, image, boxes[::-1]))
    if name == 'image_smaller_than_the_label':   # the whole image lies in the box
        assert (got != pan_vis_ref.render_overlay(pred, cats, image, font(), NO_LABELS)[0]).any(2).sum() >= 100


def test_centroid_is_floored_on_an_l_shaped_segment():
    cat, inst = np.full((60, 60), 255), np.zeros((60, 60), int)
    for y, x in ((20, 20), (21, 20), (22, 20), (22, 21), (22, 22)):      # sum x = 103, sum y = 107, area 5: centroid (21, 20)
        cat[y, x], inst[y, x] = 12, 1
    pred = pred_of(cat, inst)
    keys, area, sx, sy = pan_vis_ref.segments(pred)
    assert (keys.tolist(), area.tolist(), sx.tolist(), sy.tolist()) == ([12 << 8 | 1], [5], [103], [107])
    assert sx.dtype == np.int64 and sy.dtype == np.int64
    assert pan_vis_ref.label_boxes(pred, CATS, 5) == ([(12 << 8 | 1, 14, 13, b'T')], 1)


def test_label_min_area_is_inclusive():
    pred = pred_of(*one_blob(40, 40, 20, 20))
    for min_area, n in ((8, 1), (9, 1), (10, 0)):
        boxes, qualified = pan_vis_ref.label_boxes(pred, CATS, min_area)
        assert (len(boxes), qualified) == (n, n)


def many_segments():
    """10 x 30: 300 one-pixel segments, categories 11 and 12 with instances 0..149, in scrambled positions."""
    keys = np.array([c << 8 | i for c in (11, 12) for i in range(150)])
    keys = keys[np.random.default_rng(9).permutation(300)].reshape(10, 30)
    cats = {11: {'id': 11, 'isthing': 1, 'name': 'a'}, 12: {'id': 12, 'isthing': 1, 'name': 'b'}}
    return pred_of(keys >> 8, keys & 255), cats


def test_label_cap_keeps_the_first_256_keys():
    pred, cats = many_segments()
    boxes, qualified = pan_vis_ref.label_boxes(pred, cats, 1)
    assert qualified == 300 and len(boxes) == 256
    assert [b[0] for b in boxes] == sorted(c << 8 | i for c in (11, 12) for i in range(150))[:256]
    image = np.zeros((10, 30, 3), np.uint8)
    assert pan_vis_ref.render_overlay(pred, cats, image, font(), 1)[1:] == (300, 256)


def test_name_rules():
    from upsnet_amd.dataset import pan_vis
    cats = {3: {'id': 3, 'isthing': 1}, 4: {'id': 4, 'isthing': 0, 'name': 'café'}, 5: {'id': 5, 'isthing': 0, 'name': 'x' * 32}}
    names, lens = pan_vis.name_table(cats)
    assert names.shape == (256, 32) and names.dtype == np.uint8 and lens.dtype == np.int32
    assert bytes(names[3, :lens[3]]) == b'3' == pan_vis_ref.label_bytes(3, cats[3])            # no name: str(id)
    assert bytes(names[4, :lens[4]]) == b'caf\xc3\xa9' == pan_vis_ref.label_bytes(4, cats[4])   # UTF-8: two bytes, two '?'
    assert lens[5] == 32 and lens[6] == 0
    f = font()
    assert np.array_equal(pan_vis_ref.text_dots(b'caf\xc3\xa9', f), pan_vis_ref.text_dots(b'caf??', f))
    assert np.array_equal(pan_vis_ref.text_dots(b'\x1f\x7f', f), pan_vis_ref.text_dots(b'??', f))
    with pytest.raises(ValueError):
        pan_vis.name_table({5: {'id': 5, 'isthing': 0, 'name': 'x' * 33}})
    with pytest.raises(ValueError):
        pan_vis.PanopticRenderer({5: {'id': 5, 'isthing': 0, 'name': 'é' * 17}})                 # 34 bytes


def test_host_checks_come_before_any_launch(tmp_path):
    """Every one of these is refused without touching the device (this test runs without one)."""
    from upsnet_amd.dataset import pan_vis
    pred = np.zeros((4, 5, 3), np.uint8)
    with pytest.raises(ValueError):
        pan_vis.render_panoptic(pred, CATS, mode='overlay')                                     # no image
    with pytest.raises(ValueError):
        pan_vis.render_panoptic(pred, CATS, image=np.zeros((5, 4, 3), np.uint8))                # another size
    with pytest.raises(ValueError):
        pan_vis.render_panoptic(pred, CATS, mode='contours')
    with pytest.raises(ValueError):
        pan_vis.render_panoptic(pred, CATS, image=np.zeros((4, 5, 3), np.uint8), label_min_area=-1)
    with pytest.raises(ValueError):
        pan_vis.render_panoptic(pred[..., :2], CATS, mode='flat')
    images = [{'id': 1, 'file_name': 'a_leftImg8bit.png'}, {'id': 2, 'file_name': 'b.jpg'}]
    with pytest.raises(ValueError):
        pan_vis.vis_panoptic([pred], images, CATS, str(tmp_path), 'flat')                       # counts
    with pytest.raises(ValueError):
        pan_vis.vis_panoptic([pred, pred], images, CATS, str(tmp_path), 'overlay')              # overlay without photographs
    with pytest.raises(ValueError):
        pan_vis.vis_panoptic([pred, pred], [images[0], {'id': 3, 'file_name': 'a.png'}], CATS, str(tmp_path), 'flat')   # one name twice
    with pytest.raises(ValueError):
        pan_vis.vis_panoptic([pred, pred], [images[0], {'id': 3}], CATS, str(tmp_path), 'flat')
    assert not list(tmp_path.iterdir())


def test_file_names_and_folders():
    from upsnet_amd.dataset import pan_vis
    from upsnet_amd.dataset.pan_format import png_name
    assert pan_vis.FOLDERS == {'overlay': 'vis', 'flat': 'vis_flat'} and pan_vis.MODES == {'flat': 0, 'overlay': 1}
    assert png_name('frankfurt/f_000000_000294_leftImg8bit.png') == 'frankfurt/f_000000_000294.png'
    assert png_name('000000000139.jpg') == '000000000139.png'
    from upsnet_amd._lib import lib
    assert lib().upsnet_pan_vis_max_labels() == pan_vis.MAX_LABELS == pan_vis_ref.MAX_LABELS == 256
    assert lib().upsnet_pan_vis_workspace_zeroed_bytes() == 2 * 65536 * 8 < lib().upsnet_pan_vis_workspace_bytes()


# ------------------------------------------------------------------------------------------------ the command line
def test_flags_parse(tmp_path, saved_config):
    from upsnet_amd.config.parse_args import parse_args
    root = str(tmp_path / 'cs')
    make_dataset(root, 'Cityscapes', [(8, 12)], seed=1)
    cfg = write_cfg(tmp_path, 'Cityscapes', root, 'val')
    args = parse_args('', ['--cfg', cfg])
    assert args.vis_panoptic is None and args.vis_panoptic_min_area is None
    args = parse_args('', ['--cfg', cfg, '--vis_panoptic', 'both', '--vis_panoptic_min_area', '64'])
    assert args.vis_panoptic == 'both' and args.vis_panoptic_min_area == 64
    with pytest.raises(SystemExit):
        parse_args('', ['--cfg', cfg, '--vis_panoptic', 'contours'])


def test_vis_panoptic_refusals(tmp_path, saved_config):
    from upsnet_amd.evaluate import main
    root = str(tmp_path / 'cs')
    make_dataset(root, 'Cityscapes', [(8, 12)], seed=1)
    head = write_cfg(tmp_path, 'Cityscapes', root, 'val')
    cfg = tmp_path / 'refuse.yaml'
    cfg.write_text(open(head).read().replace('network:\n', 'network:\n  has_panoptic_head: false\n'))
    with pytest.raises(SystemExit) as e:
        main(['--cfg', head, '--synthetic_weights', '--vis_panoptic_min_area', '5'])
    assert 'vis_panoptic_min_area' in str(e.value) and 'missing' in str(e.value)
    with pytest.raises(SystemExit) as e:
        main(['--cfg', head, '--synthetic_weights', '--vis_panoptic', 'flat', '--vis_panoptic_min_area', '5'])
    assert 'vis_panoptic_min_area' in str(e.value)
    with pytest.raises(SystemExit) as e:
        main(['--cfg', head, '--synthetic_weights', '--vis_panoptic', 'overlay', '--vis_panoptic_min_area', '-1'])
    assert 'negative' in str(e.value)
    with pytest.raises(SystemExit) as e:        # (last: the yaml's switch stays in the shared config)
        main(['--cfg', str(cfg), '--synthetic_weights', '--vis_panoptic', 'flat'])
    assert 'vis_panoptic' in str(e.value) and 'has_panoptic_head' in str(e.value) and 'pan_combined' in str(e.value)


def test_eval_only_overlay_checks_the_images_first(tmp_path, saved_config):
    """--eval_only reads the photographs again for the overlay: a missing one is reported before anything is drawn."""
    import os
    import pickle
    from upsnet_amd.config.config import update_config
    from upsnet_amd.evaluate import final_output_path, main
    root = str(tmp_path / 'cs')
    _, paths = make_dataset(root, 'Cityscapes', [(8, 12), (8, 12)], seed=1, anno_name='image_info_test.json')
    cfg = write_cfg(tmp_path, 'Cityscapes', root, 'test')
    update_config(cfg)
    results_dir = os.path.join(final_output_path(cfg), 'results')
    os.makedirs(results_dir)
    with open(os.path.join(results_dir, 'results_list.pkl'), 'wb') as f:
        pickle.dump({'all_boxes': [[]] * 9, 'all_masks': [[]] * 9, 'all_ssegs': [], 'all_panos': [], 'all_pano_cls_inds': []}, f)
    os.remove(paths[2])
    with pytest.raises(FileNotFoundError) as e:
        main(['--cfg', cfg, '--eval_only', '--vis_panoptic', 'both'])
    assert os.path.basename(paths[2]) in str(e.value)
    assert not os.path.exists(os.path.join(results_dir, 'pans_unified'))


# ------------------------------------------------------------------------------------------------ the entry point
def test_entry_point_refuses_bad_arguments_without_a_gpu():
    from upsnet_amd._lib import lib
    l = lib()
    one = ctypes.c_void_p(1 << 20)          # never dereferenced: every call below is refused before anything is launched

    def call(mode=1, pred=one, id_rgb=one, table=one, image=one, H=8, W=8, cat=one, names=one, lens=one, min_area=0, ws=one, out=one, info=one):
        return l.upsnet_pan_vis(None, mode, pred, id_rgb, table, image, H, W, cat, names, lens, min_area, ws, out, info)

    for kw, word in ((dict(mode=2), b'mode'), (dict(mode=-1), b'mode'), (dict(pred=None), b'null'), (dict(cat=None), b'null'),
                     (dict(ws=None), b'null'), (dict(out=None), b'null'), (dict(info=None), b'null'), (dict(id_rgb=None), b'null'),
                     (dict(table=None), b'null'), (dict(image=None), b'null'), (dict(names=None), b'null'), (dict(lens=None), b'null'),
                     (dict(mode=0, pred=None), b'null'), (dict(H=0), b'sides'), (dict(W=0), b'sides'), (dict(H=32769, W=1), b'sides'),
                     (dict(W=32769, H=1), b'sides'), (dict(H=32768, W=8193), b'2^28'), (dict(min_area=-1), b'negative'),
                     (dict(mode=0, min_area=-1), b'negative')):
        assert call(**kw) != 0, kw
        assert word in l.upsnet_last_error(), (kw, l.upsnet_last_error())
