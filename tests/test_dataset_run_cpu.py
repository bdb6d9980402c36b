"""CPU: the evaluation run over a dataset (python -m upsnet_amd.evaluate) -- the index tables of the label-map restore (cv2
INTER_NEAREST, hand-derived; PIL NEAREST, against PIL itself), the test-phase dataset classes on generated datasets (image order,
the reference's path layouts, decoding as cv2.imread does, upfront file checks, panoptic pairing) and the run's option checks."""
import copy
import json
import os

import numpy as np
import pytest

from conftest import ROOT  # noqa: F401  (puts the repo root on sys.path)

YAML = """
output_path: "%(out)s"
model_prefix: "upsnet_test_"
symbol: resnet_50_upsnet
gpus: '0'
dataset:
  num_classes: 9
  num_seg_classes: 19
  dataset: %(dataset)s
  dataset_path: "%(root)s"
  image_set: train
  test_image_set: %(image_set)s
network:
  has_rpn: true
  fcn_num_layers: 2
test:
  scales:
  - 256
  max_size: 512
  test_iteration: 1
"""

CITYSCAPES_THINGS = [24, 25, 26, 27, 28, 31, 32, 33]    # the 8 thing categories of the Cityscapes instances JSON, in its order


@pytest.fixture()
def saved_config():
    from upsnet_amd.config.config import config
    saved = copy.deepcopy(dict(config))
    yield config
    config.clear()
    config.update(saved)


def write_cfg(tmp_path, dataset, root, image_set, name='exp_eval.yaml', extra=''):
    p = tmp_path / name
    p.write_text(YAML % dict(out=tmp_path / 'output', dataset=dataset, root=root, image_set=image_set) + extra)
    return str(p)


def save_image(path, rgb, exif_orientation=None):
    from PIL import Image
    os.makedirs(os.path.dirname(path), exist_ok=True)
    im = Image.fromarray(rgb)
    if exif_orientation is None:
        im.save(path, quality=95) if path.endswith('.jpg') else im.save(path)
    else:
        exif = Image.Exif()
        exif[0x0112] = exif_orientation
        im.save(path, quality=95, exif=exif)


def make_dataset(root, kind, sizes, ids=None, seed=0, categories=None, anno_name=None):
    """A generated dataset in the reference's layout: RGB images of the given (H, W) sizes (Cityscapes: PNG, COCO: JPEG) and an
    instances JSON listing them in the order of `ids` (default: descending, so that the loader must sort), without annotations.
    Returns (instances JSON path, {image id: image path})."""
    rng = np.random.default_rng(seed)
    ids = list(ids) if ids is not None else list(range(len(sizes), 0, -1))
    if kind == 'Cityscapes':
        img_dir, anno = os.path.join(root, 'images'), anno_name or 'instancesonly_gtFine_val.json'
        names = ['city%d_%06d_000019_leftImg8bit.png' % (i, i) for i in ids]
        cats = categories or [{'id': c, 'name': 'thing%d' % c} for c in CITYSCAPES_THINGS]
    else:
        img_dir, anno = os.path.join(root, 'images', 'val2017'), anno_name or 'instances_val2017.json'
        names = ['%012d.jpg' % i for i in ids]
        cats = categories or [{'id': c, 'name': 'cat%d' % c} for c in range(1, 9)]
    images, paths = [], {}
    for i, name, (h, w) in zip(ids, names, sizes):
        rgb = rng.integers(0, 256, (h, w, 3)).astype(np.uint8)
        rgb = np.repeat(np.repeat(rgb[::4, ::4], 4, 0), 4, 1)[:h, :w]   # 4x4 blocks: JPEG keeps them close to the drawn colours
        paths[i] = os.path.join(img_dir, name)
        save_image(paths[i], np.ascontiguousarray(rgb))
        images.append({'id': i, 'file_name': name, 'height': h, 'width': w})
    os.makedirs(os.path.join(root, 'annotations'), exist_ok=True)
    anno_path = os.path.join(root, 'annotations', anno)
    with open(anno_path, 'w') as f:
        json.dump({'images': images, 'annotations': [], 'categories': cats}, f)
    return anno_path, paths


# ------------------------------------------------------------------------------------------------ index tables
def test_cv2_nearest_tables_hand_derived():
    from upsnet_amd.dataset.restore import cv2_nearest_tables
    # im_scale 2 (fx 0.5): width 5 -> cvRound(2.5) = 2 (half to even), height 7 -> cvRound(3.5) = 4; sources floor(x * 2)
    y, x = cv2_nearest_tables((7, 5, 2.0))
    assert x.tolist() == [0, 2] and y.tolist() == [0, 2, 4, 6]
    y, x = cv2_nearest_tables((3, 3, 2.0))           # cvRound(1.5) = 2
    assert x.tolist() == [0, 2]
    # upscaling: im_scale 0.5 (fx 2): 3 -> 6, sources floor(x / 2)
    y, x = cv2_nearest_tables((2, 3, 0.5))
    assert x.tolist() == [0, 0, 1, 1, 2, 2] and y.tolist() == [0, 0, 1, 1]
    # im_scale 1: the identity over the crop
    y, x = cv2_nearest_tables((4, 6, 1.0))
    assert x.tolist() == list(range(6)) and y.tolist() == list(range(4))
    # float32 fx = 1 / 3 = 0.3333333432674408: 1 / fx = 2.9999999105930328 in double, just under 3 -- x * (1 / fx) floors to
    # 2 and 5, not 3 and 6; the size is cvRound(9 * fx) = cvRound(3.0000000894) = 3
    y, x = cv2_nearest_tables((9, 9, 3.0))
    assert x.tolist() == [0, 2, 5] and y.tolist() == [0, 2, 5]
    # im_scale 0.75: fx = float32(1 / 0.75) = 1.3333333730697632, 1 / fx = 0.74999997764825821 -- x = 4 gives 2.9999999,
    # source column 2, not 3; sizes cvRound(4 * fx) = 5, cvRound(3 * fx) = 4; the crop is int(im_info[:2])
    y, x = cv2_nearest_tables((3.9, 4.2, 0.75))
    assert x.tolist() == [0, 0, 1, 2, 2] and y.tolist() == [0, 0, 1, 2]
    assert x.dtype == np.int32 and y.dtype == np.int32


def test_pil_nearest_tables_match_pil():
    from PIL import Image
    from upsnet_amd.dataset.restore import pil_nearest_tables
    rng = np.random.default_rng(3)
    pairs = [tuple(int(v) for v in rng.integers(1, 200, 4)) for _ in range(400)]
    pairs += [(1024, 2048, 1025, 2049), (1024, 2048, 1023, 2047), (800, 1333, 480, 640), (3, 3, 9, 9), (9, 9, 3, 3), (1, 1, 5, 7)]
    for hs, ws, hd, wd in pairs:
        lab = rng.integers(0, 256, (hs, ws)).astype(np.uint8)
        want = np.array(Image.fromarray(lab).resize((wd, hd), Image.NEAREST))
        y, x = pil_nearest_tables((hs, ws), (hd, wd))
        assert np.array_equal(lab[y][:, x], want), (hs, ws, hd, wd)


# ------------------------------------------------------------------------------------------------ dataset classes
def test_roidb_order_and_cityscapes_layout(tmp_path, saved_config):
    from upsnet_amd.config.config import update_config
    from upsnet_amd.dataset import Cityscapes
    root = str(tmp_path / 'cityscapes')
    make_dataset(root, 'Cityscapes', [(8, 12), (10, 6), (5, 5)], ids=[30, 4, 17])
    update_config(write_cfg(tmp_path, 'Cityscapes', root, 'val'))
    ds = Cityscapes(image_sets=['val'], flip=False, result_path='', phase='test')
    assert [e['id'] for e in ds.roidb] == [4, 17, 30] and len(ds) == 3
    e = ds.roidb[0]
    assert e['image'] == os.path.join(root, 'images', 'city4_000004_000019_leftImg8bit.png')
    assert ds.seg_gt_path(e) == os.path.join(root, 'labels', 'city4_000004_000019_gtFine_labelTrainIds.png')
    assert ds.instances_json_file == os.path.join(root, 'annotations', 'instancesonly_gtFine_val.json')
    assert ds.panoptic_json_file == os.path.join(root, 'annotations', 'cityscapes_fine_val.json')
    assert ds.panoptic_gt_folder == os.path.join(root, 'panoptic')
    assert ds.name == 'cityscapes_val' and ds.num_classes == 9 and ds.has_gt


def test_coco_layout(tmp_path, saved_config):
    from upsnet_amd.config.config import update_config
    from upsnet_amd.dataset import coco
    root = str(tmp_path / 'coco')
    make_dataset(root, 'coco', [(8, 12), (10, 6)], ids=[139, 5])
    update_config(write_cfg(tmp_path, 'coco', root, 'val2017'))
    ds = coco(image_sets=['val2017'], flip=False, result_path='', phase='test')
    assert [e['id'] for e in ds.roidb] == [5, 139]
    e = ds.roidb[1]
    assert e['image'] == os.path.join(root, 'images', 'val2017', '000000000139.jpg')
    assert ds.seg_gt_path(e) == os.path.join(root, 'annotations', 'panoptic_val2017_semantic_trainid_stff', '000000000139.png')
    assert ds.panoptic_json_file == os.path.join(root, 'annotations', 'panoptic_val2017_stff.json')
    assert ds.panoptic_gt_folder == os.path.join(root, 'annotations', 'panoptic_val2017')
    assert ds.name == 'coco_val2017' and ds.num_classes == 9
    # test-dev: no GT -- only the images are required
    make_dataset(root, 'coco', [(8, 12)], ids=[7], anno_name='image_info_test-dev2017.json')
    os.makedirs(os.path.join(root, 'images', 'test2017'))
    os.rename(os.path.join(root, 'images', 'val2017', '000000000007.jpg'), os.path.join(root, 'images', 'test2017', '000000000007.jpg'))
    td = coco(image_sets=['test-dev2017'], phase='test')
    assert not td.has_gt and td.panoptic_json_file.endswith('image_info_test-dev2017.json')
    assert td.required_files() == [os.path.join(root, 'images', 'test2017', '000000000007.jpg')]
    td.check_files()


def test_image_decoding_like_cv2_imread(tmp_path):
    from PIL import Image
    from upsnet_amd.dataset.json_dataset import imread_bgr
    rgb = np.zeros((4, 6, 3), np.uint8)
    rgb[..., 0], rgb[..., 1], rgb[..., 2] = 10, 20, 30
    rgb[1, 2] = (200, 100, 50)
    p = str(tmp_path / 'c.png')
    save_image(p, rgb)
    bgr = imread_bgr(p)
    assert bgr.dtype == np.uint8 and bgr.shape == (4, 6, 3) and bgr.flags['C_CONTIGUOUS']
    assert bgr[0, 0].tolist() == [30, 20, 10] and bgr[1, 2].tolist() == [50, 100, 200]
    # grayscale: three equal channels (PNG exact, JPEG as decoded)
    g = (np.arange(48).reshape(6, 8) * 5).astype(np.uint8)
    Image.fromarray(g).save(str(tmp_path / 'g.png'))
    assert np.array_equal(imread_bgr(str(tmp_path / 'g.png')), np.repeat(g[:, :, None], 3, 2))
    Image.fromarray(g).save(str(tmp_path / 'g.jpg'), quality=95)
    gj = imread_bgr(str(tmp_path / 'g.jpg'))
    assert gj.shape == (6, 8, 3) and np.array_equal(gj[..., 0], gj[..., 2])
    assert np.array_equal(gj[..., 0], np.asarray(Image.open(str(tmp_path / 'g.jpg'))))
    # palette
    pal = Image.fromarray(np.array([[0, 1], [1, 0]], np.uint8), mode='P')
    pal.putpalette([0, 0, 0, 255, 128, 7] + [0] * 762)
    pal.save(str(tmp_path / 'p.png'))
    assert imread_bgr(str(tmp_path / 'p.png'))[0, 1].tolist() == [7, 128, 255]
    # EXIF orientation 6 (rotate 90 degrees clockwise to display): the decoded image is rotated, as cv2.imread does
    src = np.zeros((16, 24, 3), np.uint8)
    src[:8, :8] = (250, 0, 0)
    p = str(tmp_path / 'rot.jpg')
    save_image(p, src, exif_orientation=6)
    raw = np.asarray(Image.open(p).convert('RGB'))
    got = imread_bgr(p)
    assert raw.shape == (16, 24, 3) and got.shape == (24, 16, 3)
    assert np.array_equal(got, np.ascontiguousarray(np.rot90(raw, -1)[..., ::-1]))
    assert got[2, 13, 2] > 200 and got[2, 2, 2] < 50      # the red top-left block is now top-right


def test_unsupported_phases_raise(tmp_path, saved_config):
    from upsnet_amd.config.config import update_config
    from upsnet_amd.dataset import Cityscapes, coco
    root = str(tmp_path / 'cityscapes')
    make_dataset(root, 'Cityscapes', [(8, 12)])
    update_config(write_cfg(tmp_path, 'Cityscapes', root, 'val'))
    with pytest.raises(NotImplementedError):
        Cityscapes(image_sets=['val'], phase='train')
    with pytest.raises(NotImplementedError):
        Cityscapes(image_sets=['val'], flip=True, phase='test')
    with pytest.raises(NotImplementedError):
        Cityscapes(image_sets=['val'], proposal_files=['p.pkl'], phase='test')
    with pytest.raises(NotImplementedError):
        coco(image_sets=['val2017'], phase='train')


def test_missing_files_raise_before_any_launch(tmp_path, saved_config, monkeypatch):
    """A missing image (or GT file of a configured head) is named by FileNotFoundError before the model is built."""
    import upsnet_amd.synthetic as synthetic
    import upsnet_amd.upsnet_end2end_test as e2e
    from upsnet_amd.config.config import update_config
    from upsnet_amd.dataset import Cityscapes
    from upsnet_amd.evaluate import main

    def no_launch(*a, **k):
        raise AssertionError('the GPU was touched before the file checks')
    monkeypatch.setattr(synthetic, 'build_model', no_launch)
    monkeypatch.setattr(e2e, 'init_distributed', no_launch)
    root = str(tmp_path / 'cityscapes')
    _, paths = make_dataset(root, 'Cityscapes', [(8, 12), (6, 6)])
    cfg = write_cfg(tmp_path, 'Cityscapes', root, 'val')
    os.remove(paths[1])
    with pytest.raises(FileNotFoundError) as e:
        main(['--cfg', cfg, '--synthetic_weights'])
    assert paths[1] in str(e.value)
    # images present, GT label PNGs missing (the semantic head is configured)
    save_image(paths[1], np.zeros((6, 6, 3), np.uint8))
    update_config(cfg)
    ds = Cityscapes(image_sets=['val'], phase='test')
    with pytest.raises(FileNotFoundError) as e:
        main(['--cfg', cfg, '--synthetic_weights'])
    assert ds.seg_gt_path(ds.roidb[0]) in str(e.value)
    # label PNGs present: the panoptic JSON is next
    from PIL import Image
    for en in ds.roidb:
        os.makedirs(os.path.dirname(ds.seg_gt_path(en)), exist_ok=True)
        Image.fromarray(np.zeros((en['height'], en['width']), np.uint8)).save(ds.seg_gt_path(en))
    with pytest.raises(FileNotFoundError) as e:
        main(['--cfg', cfg, '--synthetic_weights'])
    assert ds.panoptic_json_file in str(e.value)
    # the panoptic JSON names its PNGs
    with open(ds.panoptic_json_file, 'w') as f:
        json.dump({'images': [{'id': 'a', 'file_name': 'a_gtFine_panoptic.png'}], 'annotations': [], 'categories': []}, f)
    with pytest.raises(FileNotFoundError) as e:
        main(['--cfg', cfg, '--synthetic_weights'])
    assert os.path.join(root, 'panoptic', 'a_gtFine_panoptic.png') in str(e.value)


def test_panoptic_pairing(tmp_path, saved_config, caplog):
    from upsnet_amd.config.config import update_config
    from upsnet_amd.dataset import Cityscapes
    from upsnet_amd.dataset.json_dataset import panoptic_pairing
    # by id: annotation order [30, 4, 17] over roidb order [4, 17, 30]; a subset pairs too
    assert panoptic_pairing([4, 17, 30], [30, 4, 17]) == [2, 0, 1]
    assert panoptic_pairing([4, 17, 30], [17]) == [1]
    # ids outside the image list (Cityscapes' panoptic JSON names images by string): positional, logged
    with caplog.at_level('INFO'):
        assert panoptic_pairing([4, 17, 30], ['c_a', 'c_b', 'c_c']) == [0, 1, 2]
    assert 'by position' in caplog.text
    with pytest.raises(ValueError):
        panoptic_pairing([4, 17, 30], ['c_a', 'c_b'])
    with pytest.raises(ValueError):
        panoptic_pairing([4, 17], [4, 17, 99])
    # through the dataset: the panoptic JSON's annotation order
    root = str(tmp_path / 'cityscapes')
    make_dataset(root, 'Cityscapes', [(8, 12), (6, 6), (5, 7)], ids=[30, 4, 17])
    update_config(write_cfg(tmp_path, 'Cityscapes', root, 'val'))
    ds = Cityscapes(image_sets=['val'], phase='test')
    with open(ds.panoptic_json_file, 'w') as f:
        json.dump({'images': [], 'annotations': [{'image_id': i, 'segments_info': []} for i in (17, 30, 4)], 'categories': []}, f)
    assert ds.panoptic_order() == [1, 2, 0]


# ------------------------------------------------------------------------------------------------ options
def test_more_than_one_rank_is_refused(tmp_path, saved_config, monkeypatch):
    from upsnet_amd.evaluate import main
    root = str(tmp_path / 'cityscapes')
    make_dataset(root, 'Cityscapes', [(8, 12)])
    monkeypatch.setenv('WORLD_SIZE', '2')
    with pytest.raises(SystemExit) as e:
        main(['--cfg', write_cfg(tmp_path, 'Cityscapes', root, 'val'), '--synthetic_weights'])
    assert 'WORLD_SIZE=2' in str(e.value)


def test_eval_only_without_results_fails_cleanly(tmp_path, saved_config):
    from upsnet_amd.evaluate import main
    root = str(tmp_path / 'cityscapes')
    make_dataset(root, 'Cityscapes', [(8, 12)])
    cfg = write_cfg(tmp_path, 'Cityscapes', root, 'val')
    with pytest.raises(SystemExit) as e:
        main(['--cfg', cfg, '--eval_only'])
    want = os.path.join(str(tmp_path / 'output'), 'exp_eval', 'val', 'results', 'results_list.pkl')
    assert want in str(e.value)
    with pytest.raises(SystemExit):
        main(['--cfg', cfg, '--weight_path', 'x.pth', '--synthetic_weights'])
    with pytest.raises(SystemExit):
        main(['--synthetic_weights'])


def test_unknown_dataset_name(tmp_path, saved_config):
    from upsnet_amd.evaluate import main
    root = str(tmp_path / 'ade')
    make_dataset(root, 'Cityscapes', [(8, 12)])
    with pytest.raises(ValueError):
        main(['--cfg', write_cfg(tmp_path, 'ade20k', root, 'val'), '--synthetic_weights'])


def test_default_checkpoint_path_must_exist(tmp_path, saved_config):
    """Without --weight_path the reference's default checkpoint (output_path / <cfg> / <image_set> / <prefix><iteration>.pth) is
    loaded, and a missing one raises FileNotFoundError naming it -- never replaced by synthetic weights."""
    from upsnet_amd.evaluate import main
    root = str(tmp_path / 'cityscapes')
    make_dataset(root, 'Cityscapes', [(8, 12)], anno_name='image_info_test.json')
    with pytest.raises(FileNotFoundError) as e:
        main(['--cfg', write_cfg(tmp_path, 'Cityscapes', root, 'test')])
    assert os.path.join(str(tmp_path / 'output'), 'exp_eval', 'train', 'upsnet_test_1.pth') in str(e.value)
