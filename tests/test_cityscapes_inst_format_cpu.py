"""CPU: the host half of the Cityscapes instance prediction files (upsnet_amd/dataset/cityscapes_inst_format.py): the pred.txt text
and the file names against bytes written out by hand, the reader's rules on folders built here with PIL, expand_masks' argument
checks (every one raised before the library is touched), the writer's upfront checks, the command line's refusals, and that the
seeded scenes of the GPU test reach every special case."""
import os

import numpy as np
import pytest
import torch
from PIL import Image

from conftest import ROOT  # noqa: F401  (puts the repo root on sys.path)

import cityscapes_inst_format_ref as ref

IMAGES = ['/data/images/frankfurt_000000_000294_leftImg8bit.png', '/data/images/munster_000001_000019_leftImg8bit.png']


def entry(path, H=6, W=5):
    return {'image': path, 'height': H, 'width': W, 'id': 0}


# ------------------------------------------------------------------------------------------------------------------ text
def test_pred_txt_bytes_and_names_by_hand():
    from upsnet_amd.dataset import cityscapes_inst_format as cif
    boxes0 = [[]] + [np.zeros((0, 5), np.float32) for _ in range(8)]
    boxes0[1] = np.array([[0, 0, 1, 1, 0.1]], np.float32)                        # one person
    boxes0[3] = np.array([[0, 0, 1, 1, 1e-5], [0, 0, 1, 1, 1.0]], np.float32)    # two cars
    boxes1 = [[]] + [np.zeros((0, 5), np.float32) for _ in range(8)]             # an image without detections
    e0, e1 = entry(IMAGES[0]), entry(IMAGES[1])
    assert cif.pred_txt_name(e0) == 'frankfurt_000000_000294_leftImg8bitpred.txt'
    assert cif.pred_txt_name(e1) == 'munster_000001_000019_leftImg8bitpred.txt'
    want = ('seg_results/frankfurt_000000_000294_leftImg8bit/frankfurt_000000_000294_leftImg8bit_person_0.png 24 0.1\n'
            'seg_results/frankfurt_000000_000294_leftImg8bit/frankfurt_000000_000294_leftImg8bit_car_0.png 26 1e-05\n'
            'seg_results/frankfurt_000000_000294_leftImg8bit/frankfurt_000000_000294_leftImg8bit_car_1.png 26 1.0\n')
    assert ''.join(cif.pred_txt_lines(e0, boxes0)) == want == ref.pred_txt(IMAGES[0], boxes0)
    assert ''.join(cif.pred_txt_lines(e1, boxes1)) == '' == ref.pred_txt(IMAGES[1], boxes1)
    assert cif.png_name(e0, 8, 12) == 'seg_results/frankfurt_000000_000294_leftImg8bit/frankfurt_000000_000294_leftImg8bit_bicycle_12.png'
    # the score text reads back to the same float32
    rng = np.random.default_rng(0)
    for s in rng.random(200).astype(np.float32).tolist() + [np.float32(1) / np.float32(3), np.float32(1e-30)]:
        b = [[]] + [np.array([[0, 0, 1, 1, s]], np.float32)] + [[] for _ in range(7)]
        text = cif.pred_txt_lines(e0, b)[0][:-1].split(' ')[2]
        assert np.float32(float(text)) == np.float32(s) and text == str(np.float32(s))
    assert cif.image_key(e0) == 'frankfurt_000000_000294'


# ------------------------------------------------------------------------------------------------------------------ reader
def make_folder(tmp_path, lines, pngs, txt='frankfurt_000000_000294_anything.txt', sub=''):
    """A prediction folder: `pngs` {relative path: PIL image} next to the txt (in `sub`), `lines` the txt's lines."""
    folder = tmp_path / 'pred'
    base = folder / sub if sub else folder
    os.makedirs(str(base), exist_ok=True)
    for rel, im in pngs.items():
        os.makedirs(os.path.dirname(str(base / rel)), exist_ok=True)
        im.save(str(base / rel))
    with open(str(base / txt), 'w') as f:
        f.write(''.join(lines))
    return str(folder)


def test_reader_modes_label_filter_and_sub_directory(tmp_path):
    from upsnet_amd.dataset import cityscapes_inst_format as cif
    H, W = 6, 5
    m = np.zeros((H, W), np.uint8)
    m[1:4, 2:5] = 1
    pal = Image.fromarray(m * 3)                     # palette index 3 inside, 0 outside
    pal.putpalette([0, 0, 0] + [9, 9, 9] * 2 + [200, 10, 10] + [0, 0, 0] * 252)
    rgb = np.zeros((H, W, 3), np.uint8)
    rgb[5, 0] = (0, 0, 1)                            # luma (299 R + 587 G + 114 B) / 1000 rounds to 0: outside, as in the devkit
    rgb[0, 0] = (0, 0, 9)                            # luma 1: inside
    pngs = {'masks/l.png': Image.fromarray(m * 255), 'masks/one.png': Image.fromarray(m.astype(bool)), 'masks/p.png': pal,
            'masks/rgb.png': Image.fromarray(rgb), 'masks/road.png': Image.fromarray(np.full((H, W), 255, np.uint8))}
    lines = ['masks/l.png 26 0.5\n', '\n', 'masks/road.png 7 0.9\n', 'masks/one.png 24 0.25\n', 'masks/p.png 33 1e-05\n',
             'masks/rgb.png 31 0.30000001192092896\n', 'masks/road.png -1 0.9\n']
    folder = make_folder(tmp_path, lines, pngs, sub='some/where')
    got = cif.read_instance_predictions(folder, entry(IMAGES[0], H, W))
    assert got['file'].endswith(os.path.join('some', 'where', 'frankfurt_000000_000294_anything.txt'))
    assert got['classes'].tolist() == [3, 1, 8, 6] and got['classes'].dtype == np.int64
    assert got['scores'].dtype == np.float32
    assert got['scores'].tolist() == [np.float32(0.5), np.float32(0.25), np.float32(1e-5), np.float32(0.3)]
    masks = got['masks'].numpy()
    assert masks.dtype == np.uint8 and masks.shape == (4, H, W)
    want_rgb = (np.asarray(Image.fromarray(rgb).convert('L')) != 0).astype(np.uint8)
    assert want_rgb[0, 0] == 1 and want_rgb[5, 0] == 0 and want_rgb.sum() == 1
    for k, want in enumerate([m, m, m, want_rgb]):
        assert np.array_equal(masks[k], want), k
    # an image whose file holds no instance line at all
    folder2 = make_folder(tmp_path / 'b', ['masks/road.png 7 0.9\n'], {'masks/road.png': pngs['masks/road.png']})
    got = cif.read_instance_predictions(folder2, entry(IMAGES[0], H, W))
    assert tuple(got['masks'].shape) == (0, H, W) and got['scores'].shape == (0,) and got['classes'].shape == (0,)
    # our own file name is found by the same rule
    folder3 = make_folder(tmp_path / 'c', [], {}, txt='frankfurt_000000_000294_leftImg8bitpred.txt')
    assert cif.read_instance_predictions(folder3, entry(IMAGES[0], H, W))['file'].endswith('leftImg8bitpred.txt')


def test_reader_errors(tmp_path):
    from upsnet_amd.dataset import cityscapes_inst_format as cif
    H, W = 6, 5
    ok = Image.fromarray(np.full((H, W), 255, np.uint8))
    e = entry(IMAGES[0], H, W)
    outside = tmp_path / 'outside.png'
    ok.save(str(outside))

    def folder_of(name, lines, pngs=None, **kw):
        return make_folder(tmp_path / name, lines, {'m.png': ok} if pngs is None else pngs, **kw)

    bad = {
        'two fields': (['m.png 26\n'], ValueError, 'line 1'),
        'four fields': (['m.png 26 0.5 7\n'], ValueError, 'line 1'),
        'double space': (['m.png  26 0.5\n'], ValueError, 'line 1'),
        'tab': (['m.png\t26\t0.5\n'], ValueError, 'line 1'),
        'label text': (['m.png 26 0.5\n', 'm.png car 0.5\n'], ValueError, 'line 2'),
        'label float': (['m.png 26.0 0.5\n'], ValueError, 'line 1'),
        'score text': (['m.png 26 high\n'], ValueError, 'line 1'),
        'score nan': (['m.png 26 nan\n'], ValueError, 'NaN'),
        'label 34': (['m.png 34 0.5\n'], ValueError, 'no Cityscapes label'),
        'label -2': (['m.png -2 0.5\n'], ValueError, 'no Cityscapes label'),
        'absolute': (['%s 26 0.5\n' % outside], ValueError, 'absolute'),
        'escaping': (['../../outside.png 26 0.5\n'], ValueError, 'leaves'),
        'missing png': (['n.png 26 0.5\n'], FileNotFoundError, 'n.png'),
        'missing png of a skipped line': (['n.png 7 0.5\n'], FileNotFoundError, 'n.png'),
    }
    for what, (lines, exc, match) in bad.items():
        folder = folder_of(what.replace(' ', '_'), lines)
        with pytest.raises(exc, match=match):
            cif.read_instance_predictions(folder, e)
            pytest.fail('%s: no error' % what)
    with pytest.raises(ValueError, match='frankfurt_000000_000294_anything.txt'):       # the file is named
        cif.read_instance_predictions(folder_of('named', ['m.png 26\n']), e)
    # the wrong size
    small = folder_of('size', ['m.png 26 0.5\n'], {'m.png': Image.fromarray(np.zeros((H, W + 1), np.uint8))})
    with pytest.raises(ValueError, match='a mask of 6 x 6 for an image of 6 x 5'):
        cif.read_instance_predictions(small, e)
    # no file, several files: the image is named
    none = folder_of('none', [], {}, txt='munster_000001_000019_x.txt')
    with pytest.raises(ValueError, match='frankfurt_000000_000294_leftImg8bit.png: no prediction file'):
        cif.read_instance_predictions(none, e)
    two = folder_of('two', [], {})
    with open(os.path.join(two, 'frankfurt_000000_000294_b.txt'), 'w'):
        pass
    with pytest.raises(ValueError, match='frankfurt_000000_000294_leftImg8bit.png: more than one prediction file'):
        cif.read_instance_predictions(two, e)


# ------------------------------------------------------------------------------------------------------------------ checks
def test_expand_masks_value_errors_come_before_the_library(monkeypatch):
    from upsnet_amd.dataset import cityscapes_inst_format as cif

    def no_lib(*a, **k):
        raise AssertionError('the library was reached')
    monkeypatch.setattr(cif, 'lib', no_lib)
    monkeypatch.setattr(cif, 'stream', no_lib)
    H, W = 6, 5
    t = np.array([3, 7, 10, 12], np.int32)
    o = np.array([0, 2, 4], np.int32)
    good_out = torch.empty((2, H, W), dtype=torch.uint8)
    bad = {
        'trans dtype': lambda: cif.expand_masks(t.astype(np.int64), o, H, W),
        'off dtype': lambda: cif.expand_masks(t, o.astype(np.int64), H, W),
        'trans list': lambda: cif.expand_masks(t.tolist(), o, H, W),
        'trans dims': lambda: cif.expand_masks(t.reshape(2, 2), o, H, W),
        'trans tensor dtype': lambda: cif.expand_masks(torch.from_numpy(t).long(), o, H, W),
        'off empty': lambda: cif.expand_masks(t[:0], o[:0], H, W),
        'off start': lambda: cif.expand_masks(t, np.array([1, 2, 4], np.int32), H, W),
        'off end': lambda: cif.expand_masks(t, np.array([0, 2, 3], np.int32), H, W),
        'off beyond': lambda: cif.expand_masks(t, np.array([0, 2, 5], np.int32), H, W),
        'off falls': lambda: cif.expand_masks(t, np.array([0, 3, 2, 4], np.int32), H, W),
        'H zero': lambda: cif.expand_masks(t, o, 0, W),
        'W negative': lambda: cif.expand_masks(t, o, H, -1),
        'H float': lambda: cif.expand_masks(t, o, 6.0, W),
        'too many pixels': lambda: cif.expand_masks(t, o, 1 << 15, (1 << 15) + 1),
        'negative position': lambda: cif.expand_masks(np.array([-1, 7, 10, 12], np.int32), o, H, W),
        'position H * W': lambda: cif.expand_masks(np.array([3, 7, 10, 30], np.int32), o, H, W),
        'falls within a mask': lambda: cif.expand_masks(np.array([7, 3, 10, 12], np.int32), o, H, W),
        'falls within the last mask': lambda: cif.expand_masks(np.array([3, 7, 12, 10], np.int32), o, H, W),
        'out shape': lambda: cif.expand_masks(t, o, H, W, out=torch.empty((2, W, H), dtype=torch.uint8)),
        'out shape 1 bit': lambda: cif.expand_masks(t, o, H, W, one_bit=True, out=good_out),
        'out dtype': lambda: cif.expand_masks(t, o, H, W, out=good_out.to(torch.int8)),
        'out strides': lambda: cif.expand_masks(t, o, H, W, out=torch.empty((2, W, H), dtype=torch.uint8).transpose(1, 2)),
        'out numpy': lambda: cif.expand_masks(t, o, H, W, out=np.zeros((2, H, W), np.uint8)),
        'out on the host': lambda: cif.expand_masks(t, o, H, W, out=good_out),
        'trans on the host': lambda: cif.expand_masks(torch.from_numpy(t), o, H, W),
        'max_bytes': lambda: cif.expand_masks(t, o, H, W, max_bytes=0),
    }
    for what, call in bad.items():
        with pytest.raises(ValueError):
            call()
            pytest.fail('%s: no ValueError' % what)
    # what is valid: a mask may start lower than the one before ended, equal positions, an empty list
    assert cif.check_runs(np.array([12, 20, 3, 3, 29], np.int32), np.array([0, 2, 2, 5], np.int32), H, W) == 3
    assert cif.check_runs(np.zeros(0, np.int32), np.array([0], np.int32), H, W) == 0
    assert cif.check_runs(np.zeros(0, np.int32), np.array([0, 0], np.int32), 1 << 15, 1 << 15) == 1
    assert cif.MAX_LAUNCH_BYTES == 256 << 20
    assert cif.plane_bytes(37, 53, False) == 37 * 53 and cif.plane_bytes(37, 53, True) == 37 * 7


def test_writer_checks_come_before_any_file(tmp_path, monkeypatch):
    from upsnet_amd.dataset import cityscapes_inst_format as cif

    class Dataset(object):
        roidb = [entry(IMAGES[0]), entry(IMAGES[1])]

    def reached(*a, **k):
        raise AssertionError('the device half was reached')
    monkeypatch.setattr(cif, 'InstanceMaskFormatter', reached)
    rle = {'size': [6, 5], 'counts': [3, 4, 23]}
    det = np.array([[0, 0, 1, 1, 0.5]], np.float32)

    def results(n_cls=9, n_img=2):
        return [[[] for _ in range(n_img)] for _ in range(n_cls)], [[[] for _ in range(n_img)] for _ in range(n_cls)]

    cases = {}
    cases['ten classes'] = results(n_cls=10)
    cases['eight classes'] = results(n_cls=8)
    cases['three images'] = results(n_img=3)
    b, s = results()
    s[3] = s[3][:1]
    cases['one class short of an image'] = (b, s)
    b, s = results()
    b[3][1], s[3][1] = det, [{'size': [6, 6], 'counts': [3, 4, 29]}]
    cases['rle size'] = (b, s)
    b, s = results()
    b[3][1], s[3][1] = det, [rle, rle]
    cases['detections / masks'] = (b, s)
    b, s = results()
    b[3][0], s[3][0] = det, [[0.0, 0.0, 1.0, 1.0, 2.0, 0.0]]
    cases['polygon'] = (b, s)
    out = tmp_path / 'out'
    for what, (b, s) in cases.items():
        with pytest.raises(ValueError):
            cif.write_instance_predictions(Dataset(), b, s, str(out))
            pytest.fail('%s: no ValueError' % what)
    assert not out.exists()
    b, s = results()
    b[3][1], s[3][1] = det, [rle]
    with pytest.raises(AssertionError, match='the device half was reached'):       # and valid results do get there
        cif.write_instance_predictions(Dataset(), b, s, str(out))


def test_command_line_refusals(tmp_path):
    """The refusals that need neither a dataset nor a device."""
    import copy
    from test_dataset_run_cpu import make_dataset, write_cfg
    from upsnet_amd.config.config import config
    from upsnet_amd.evaluate import main
    saved = copy.deepcopy(dict(config))
    try:
        cs = write_cfg(tmp_path, 'Cityscapes', str(tmp_path / 'nowhere'), 'val')
        with pytest.raises(SystemExit, match='--instances_1bit'):
            main(['--cfg', cs, '--eval_only', '--instances_1bit'])
        with pytest.raises(SystemExit, match='--score_instances: no folder'):
            main(['--cfg', cs, '--score_instances', str(tmp_path / 'missing')])
        config.clear()
        config.update(copy.deepcopy(saved))
        root = str(tmp_path / 'cs_test')
        make_dataset(root, 'Cityscapes', [(8, 12)], anno_name='image_info_test.json')      # an image set without ground truth
        (tmp_path / 't').mkdir()
        test_split = write_cfg(tmp_path / 't', 'Cityscapes', root, 'test')
        with pytest.raises(SystemExit, match='--score_instances: cityscapes_test has no ground truth'):
            main(['--cfg', test_split, '--score_instances', str(tmp_path)])
        config.clear()
        config.update(copy.deepcopy(saved))
        (tmp_path / 'm').mkdir()
        no_masks = write_cfg(tmp_path / 'm', 'Cityscapes', root, 'test', extra='network:\n  has_mask_head: false\n')
        with pytest.raises(SystemExit, match='--write_instances'):
            main(['--cfg', no_masks, '--eval_only', '--write_instances'])
        config.clear()
        config.update(copy.deepcopy(saved))
        (tmp_path / 'c').mkdir()
        coco = write_cfg(tmp_path / 'c', 'coco', str(tmp_path / 'nowhere'), 'val2017')
        with pytest.raises(SystemExit, match='--write_instances'):
            main(['--cfg', coco, '--eval_only', '--write_instances'])
        with pytest.raises(SystemExit, match='--score_instances'):
            main(['--cfg', coco, '--score_instances', str(tmp_path)])
    finally:
        config.clear()
        config.update(saved)


def test_c_entry_point_validates_before_launching():
    """Error code and message for every argument outside the contract; none of these calls reaches a launch (no device here)."""
    import ctypes
    from upsnet_amd import _lib
    l = _lib.lib()
    one = ctypes.c_void_p(256)

    def call(trans=one, off=one, n=1, H=4, W=4, bits=8, out=one):
        return l.upsnet_cs_inst_expand(None, trans, off, n, H, W, bits, out)
    for kw, text in [(dict(H=0), b'H * W'), (dict(W=-1), b'H * W'), (dict(H=1 << 15, W=(1 << 15) + 1), b'H * W'), (dict(bits=4), b'bits'),
                     (dict(n=-1), b'masks'), (dict(trans=None), b'null pointer'), (dict(off=None), b'null pointer'),
                     (dict(out=None), b'null pointer'), (dict(trans=ctypes.c_void_p(258)), b'misaligned')]:
        assert call(**kw) != 0, kw
        assert text in l.upsnet_last_error(), (kw, l.upsnet_last_error())
    assert call(n=0, trans=None, off=None, out=None) == 0          # nothing to do: nothing launched


# ------------------------------------------------------------------------------------------------------------------ scenes
def test_seeded_scenes_reach_every_special_case():
    """The restatement on the scenes the GPU test expands: every special mask is what its name says, and the run lists are valid input
    (zero-length runs included: equal neighbouring positions)."""
    from upsnet_amd.dataset import cityscapes_inst_format as cif
    seen = set()
    for H, W in ref.SIZES + [ref.REAL_SIZE]:
        names, counts = ref.make_scene(H, W) if (H, W) != ref.REAL_SIZE else ref.real_scene()
        assert 1 <= len(counts) <= 20
        trans, off = ref.runs_of_counts(counts)
        assert cif.check_runs(trans, off, H, W) == len(counts)
        p8, p1 = ref.expected_planes(counts, H, W)
        assert p8.shape == (len(counts), H, W) and p1.shape == (len(counts), H, (W + 7) // 8)
        assert set(np.unique(p8).tolist()) <= {0, 255}
        assert np.array_equal(np.unpackbits(p1, axis=2)[:, :, :W] * 255, p8) and not np.unpackbits(p1, axis=2)[:, :, W:].any()
        for k, name in enumerate(names):
            m, t = p8[k] != 0, trans[off[k]:off[k + 1]]
            col = m.T.reshape(-1)
            if name == 'all_zero':
                assert not m.any() and t.size == 0
            elif name == 'all_one':
                assert m.all() and t.tolist() == [0]
            elif name == 'starts_inside':
                assert col[0] and t[0] == 0 and not m.all()
            elif name == 'last_pixel':
                assert col[-1] and col.sum() == 1 and t.tolist() == [H * W - 1]
            elif name == 'duplicates':
                assert np.any(np.diff(t) == 0) and m.any() and not m.all()
            elif name == 'crosses_column':
                inside = np.flatnonzero(col)
                assert inside.size == 2 and inside[0] // H != inside[1] // H and inside[1] == inside[0] + 1
            else:
                continue
            seen.add(name)
    assert seen == {'all_zero', 'all_one', 'starts_inside', 'last_pixel', 'duplicates', 'crosses_column'}
    # the sizes reach both store paths of both kernels, a ragged last byte and a ragged last wave
    assert any(W % 4 == 0 for _, W in ref.SIZES) and any(W % 4 for _, W in ref.SIZES)
    assert any(((W + 7) // 8) % 4 == 0 for _, W in ref.SIZES) and any(((W + 7) // 8) % 4 for _, W in ref.SIZES)
    assert any(W % 8 for _, W in ref.SIZES) and any(W % 64 and W > 64 for _, W in ref.SIZES)
    assert any(H > 64 for H, _ in ref.SIZES) and any(H > 128 for H, _ in [ref.REAL_SIZE])
