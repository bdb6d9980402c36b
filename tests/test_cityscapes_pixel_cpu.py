"""CPU: the Cityscapes pixel-level IoU / iIoU rules. Hand-derived cases pin the numpy restatement
(tests/cityscapes_pixel_ref.py) that the GPU tests compare the device evaluator with, and the product's own host-side scoring
(cityscapes_pixel_eval.scores, pure numpy) on the restatement's sums; the seeded scenes of the GPU tests are shown to reach every
branch of the rules; the writer's file names and palette, the dataset's paths, the command-line flags and the refusals that need no
device."""
import copy
import math
import os

import numpy as np
import pytest

from conftest import ROOT  # noqa: F401  (puts the repo root on sys.path)

import cityscapes_pixel_cases as cases
import cityscapes_pixel_ref as ref

ROAD, SIDEWALK, PARKING, BUILDING, PERSON, RIDER, CAR, TRUCK, CARAVAN = 7, 8, 9, 11, 24, 25, 26, 27, 29
AVG1 = {n: 100.0 for n in ref.INSTANCE_CLASSES}          # every class's average size 100: weights are 100 / size


def maps(H=10, W=10, label=ROAD):
    return np.full((H, W), label, np.uint8), np.full((H, W), label, np.uint16), np.full((H, W), label, np.uint8)


def wsum_of(res):
    """The restatement's instance statistics as the product's wsum array [10, 4]."""
    rows = [res['inst_stats']['classes'][n] for n in ref.INSTANCE_CLASSES] + [res['inst_stats']['categories'][c] for c in ('human', 'vehicle')]
    return np.array([[r['tp'], r['tpWeighted'], r['fn'], r['fnWeighted']] for r in rows], np.float64)


def same(a, b):
    return (math.isnan(a) and math.isnan(b)) or a == b


def check_product_scoring(res):
    """The product's host-side scoring of the same sums gives the same bits as the restatement."""
    from upsnet_amd.dataset import cityscapes_pixel_eval as pe
    got = pe.scores(res['conf'], wsum_of(res), with_instances=all(t is not None for t in res['inst']))
    for key, want in (('IoU_class', 'averageScoreClasses'), ('iIoU_class', 'averageScoreInstClasses'),
                      ('IoU_category', 'averageScoreCategories'), ('iIoU_category', 'averageScoreInstCategories')):
        assert same(got[key], res[want]), (key, got[key], res[want])
    for name, r in got['per_class'].items():
        assert same(r['iou'], res['classScores'][name]) and same(r['iiou'], res['classInstScores'][name]), name
    for name, r in got['per_category'].items():
        assert same(r['iou'], res['categoryScores'][name]) and same(r['iiou'], res['categoryInstScores'][name]), name
    return got


def test_false_positive_on_ignored_ground_truth_is_not_counted():
    """100 pixels: 60 road GT predicted road, 20 sidewalk GT predicted road, 20 'unlabeled' (0, ignored) GT predicted road.
    road: tp 60, fn 0, fp = the 20 on sidewalk only (the 20 on label 0 are left out) -> 60 / 80 = 0.75 (0.6 if they counted).
    sidewalk: tp 0, fn 20, fp 0 -> 0.0. Mean over the two classes present: 0.375."""
    gl, gi, pr = maps()
    gl[6:8] = SIDEWALK
    gl[8:] = 0
    res = ref.evaluate([(gl, gl.astype(np.uint16), pr)])
    assert res['classScores']['road'] == 0.75 and res['classScores']['sidewalk'] == 0.0
    assert res['averageScoreClasses'] == 0.375
    assert math.isnan(res['classScores']['unlabeled'])
    check_product_scoring(res)


def test_prediction_of_an_ignored_label_is_a_false_negative():
    """100 road pixels, 30 of them predicted 'parking' (9, ignored): road tp 70, fn 30, fp 0 -> 0.7; parking itself has no score."""
    gl, gi, pr = maps()
    pr[:3] = PARKING
    res = ref.evaluate([(gl, gi, pr)])
    assert res['classScores']['road'] == 0.7 and math.isnan(res['classScores']['parking'])
    assert res['averageScoreClasses'] == 0.7 and res['categoryScores']['flat'] == 0.7
    check_product_scoring(res)


def test_absent_class_is_nan_and_leaves_the_mean():
    """Only road, all right: road 1.0, the other 18 evaluated classes have tp + fp + fn = 0 -> NaN; the mean is over road alone.
    No instance anywhere: the weighted sums are 0 and fp is 0, so every iIoU is NaN too, and so are their means."""
    gl, gi, pr = maps()
    res = ref.evaluate([(gl, gi, pr)])
    assert res['classScores']['road'] == 1.0 and res['averageScoreClasses'] == 1.0
    assert sum(math.isnan(v) for v in res['classScores'].values()) == 33
    assert math.isnan(res['averageScoreInstClasses']) and math.isnan(res['averageScoreInstCategories'])
    got = check_product_scoring(res)
    assert len(got['per_class']) == 19 and math.isnan(got['per_class']['car']['iou'])


def test_two_instances_of_unequal_size_give_iiou_other_than_iou():
    """Two persons: a of 40 pixels, 30 predicted person; b of 10 pixels, 1 predicted person; the misses predicted road, the road
    GT all right. IoU person = 31 / (31 + 0 + 19) = 0.62. With average size 100: weights 2.5 and 10; tpWeighted = 30 * 2.5 + 1 * 10 =
    85, fnWeighted = 10 * 2.5 + 9 * 10 = 115, fp 0 -> iIoU = 85 / 200 = 0.425 (the small instance weighs as much as the large)."""
    gl, gi, pr = maps()
    gi[0:4, :] = 24001
    gi[5, :] = 24002
    gl = cases.labels_of(gi)
    pr[0:3, :] = PERSON
    pr[5, 0] = PERSON
    res = ref.evaluate([(gl, gi, pr)], AVG1)
    assert res['inst'] == [{24001: (40, 30, 30), 24002: (10, 1, 1)}]
    assert res['classScores']['person'] == 0.62
    s = res['inst_stats']['classes']['person']
    assert (s['tp'], s['fn'], s['tpWeighted'], s['fnWeighted']) == (31, 19, 85.0, 115.0)
    assert res['classInstScores']['person'] == 0.425
    assert res['averageScoreInstClasses'] == 0.425 and res['categoryInstScores']['human'] == 0.425
    check_product_scoring(res)


def test_group_region_and_caravan_contribute_no_instance_and_number_zero_does():
    """Raw value 26 (a car group region: not above 1000), 29003 (a caravan instance: ignore-in-eval) and 7005 (a stuff label) give
    no instance; 26000 = 1000 * 26 + 0 is above 1000 and is car instance number 0 (10 pixels, 5 hit: weight 10, tpWeighted 50)."""
    gl, gi, pr = maps()
    gi[0] = 26
    gi[1] = 29003
    gi[2] = 7005
    gi[3] = 26000
    gl = cases.labels_of(gi)
    pr[0] = CAR
    pr[1] = CAR
    pr[3, :5] = CAR
    stats = {}
    res = ref.evaluate([(gl, gi, pr)], AVG1, stats)
    assert res['inst'] == [{26000: (10, 5, 5)}]
    assert stats == dict(stats, instance_of_ignored_label=1, instance_value_of_stuff_label=1, instance_number_zero=1, instances=1)
    s = res['inst_stats']['classes']['car']
    assert (s['tp'], s['fn'], s['tpWeighted'], s['fnWeighted']) == (5, 5, 50.0, 50.0)
    # car: tp 15 (group row + 5), fn 5, fp 0 (the 10 on the caravan row are on ignored ground truth) -> 0.75; iIoU 50 / 100
    assert res['classScores']['car'] == 0.75 and res['classInstScores']['car'] == 0.5
    check_product_scoring(res)


def test_category_false_positives_ignore_confusion_inside_the_category():
    """20 person GT pixels: 10 predicted person, 10 rider; 10 rider GT pixels predicted person; 70 road right.
    Classes: person tp 10, fn 10, fp 10 -> 1/3; rider tp 0, fn 10, fp 10 -> 0. Category human: L = {person, rider}: tp = all 30
    (person <-> rider stays inside), fn 0, fp 0 -> 1.0; flat 1.0. One person instance of the 20 pixels: class tp 10, category tp 20."""
    gl, gi, pr = maps()
    gi[0:2] = 24001
    gi[2] = 25
    gl = cases.labels_of(gi)
    pr[0] = PERSON
    pr[1] = RIDER
    pr[2] = PERSON
    stats = {}
    res = ref.evaluate([(gl, gi, pr)], AVG1, stats)
    assert res['classScores']['person'] == 10.0 / 30.0 and res['classScores']['rider'] == 0.0
    assert res['categoryScores']['human'] == 1.0 and res['categoryScores']['flat'] == 1.0
    assert res['inst'] == [{24001: (20, 10, 20)}] and stats['confusion_inside_category'] == 1 and stats['category_hit_of_another_class'] == 1
    # weight 5: class 50 / (50 + fp 10 + 50); category 100 / (100 + 0 + 0)
    assert res['classInstScores']['person'] == 50.0 / 110.0 and res['categoryInstScores']['human'] == 1.0
    check_product_scoring(res)


def test_an_image_without_its_instance_map_leaves_iou_only():
    gl, gi, pr = maps()
    gi[0] = 24001
    gl = cases.labels_of(gi)
    res = ref.evaluate([(gl, gi, pr), (gl, None, pr)], AVG1)
    assert res['classScores']['person'] == 0.0 and math.isnan(res['classInstScores']['person'])
    assert math.isnan(res['averageScoreInstClasses'])
    check_product_scoring(res)


# ------------------------------------------------------------------------------------------------ the GPU tests' scenes
BRANCHES = ('instances', 'instance_number_zero', 'instance_of_ignored_label', 'instance_value_of_stuff_label',
            'category_hit_of_another_class', 'partly_hit_instance', 'class_absent', 'prediction_on_ignored_gt', 'iiou_differs_from_iou',
            'confusion_inside_category')


@pytest.mark.parametrize('name', sorted(cases.GPU_SCENES))
def test_random_scenes_reach_every_branch(name):
    """A condition on the inputs of tests/test_cityscapes_pixel_gpu.py: each scene list, through the restatement alone, takes every
    branch of the rules; both kinds of prediction occur; group regions occur."""
    seed, sizes, n_inst = cases.GPU_SCENES[name]
    scene = cases.make_scene(seed, sizes, n_inst)
    stats = {}
    res = ref.evaluate([(g, i, cases.as_label_ids(p, t)) for g, i, p, t in scene], None, stats)
    for key in BRANCHES + ('ignored_label_predicted_on_evaluated_gt',):
        assert stats.get(key, 0) > 0, (key, stats)
    assert {t for _, _, _, t in scene} == {True, False}
    assert any(((i < 1000) & (i >= 24)).any() for _, i, _, _ in scene), "no group region"
    assert math.isnan(res['classScores']['motorcycle']) and res['classScores']['train'] < 0.2
    for key in ('averageScoreClasses', 'averageScoreInstClasses', 'averageScoreCategories', 'averageScoreInstCategories'):
        assert 0.0 < res[key] < 1.0, (key, res[key])
    check_product_scoring(res)


def test_special_images():
    labels, ids, pred, train = cases.no_instance_image()
    assert train and not (ids > 1000).any() and ((ids >= 24) & (ids < 34)).any()
    labels, ids, pred, train = cases.many_instances_image()
    v = np.unique(ids[ids > 1000])
    assert v.size == 1000 and v[0] == 24000 and v[-1] == 24999 and not train
    assert max(np.unique(ids.reshape(-1)[k:k + 8192]).size for k in range(0, ids.size, 8192)) > 129      # more than a 128-entry table
    labels, ids, pred, train = cases.all_labels_image()
    assert np.unique(labels).tolist() == list(range(34)) and np.unique(pred).tolist() == list(range(34))


# ------------------------------------------------------------------------------------------------ module tables, writer, paths, flags
@pytest.fixture()
def saved_config():
    from upsnet_amd.config.config import config
    saved = copy.deepcopy(dict(config))
    yield config
    config.clear()
    config.update(saved)


def test_module_tables():
    from upsnet_amd.dataset import cityscapes_pixel_eval as pe
    assert [(n, c) for n, c in pe.LABELS] == [(ref.LABELS[i][0], ref.LABELS[i][1]) for i in range(34)]
    assert list(pe.EVAL_LABEL_IDS) == [i for i in range(34) if not ref.LABELS[i][3]] == ref.TRAIN2LABEL == list(pe.TRAIN_TO_LABEL_ID)
    assert [i for i in range(34) if ref.LABELS[i][2]] == list(range(24, 34))
    assert list(pe.WSUM_ROWS[:8]) == ref.INSTANCE_CLASSES and len(pe.AVG_CLASS_SIZE) == 8 and all(v > 0 for v in pe.AVG_CLASS_SIZE)
    lut = pe.lookup_table(True)
    assert lut[:19].tolist() == ref.TRAIN2LABEL and set(lut[19:].tolist()) == {255}
    lut = pe.lookup_table(False)
    assert lut[:34].tolist() == list(range(34)) and set(lut[34:].tolist()) == {255}
    with pytest.raises(ValueError):
        pe.PixelEvaluator(avg_class_size=[1.0] * 7)
    with pytest.raises(ValueError):
        pe.PixelEvaluator(avg_class_size=dict(ref.AVG, car=0.0))
    assert pe.PixelEvaluator(avg_class_size=ref.OTHER_AVG).avg_class_size == tuple(ref.OTHER_AVG[n] for n in ref.INSTANCE_CLASSES)


def test_parse_args_knows_the_flags():
    from upsnet_amd.config.parse_args import parse_args
    a = parse_args('', ['--eval_pixels', '--write_ssegs', '--ssegs_label_ids', '--score_ssegs', 'x'])
    assert a.eval_pixels and a.write_ssegs and a.ssegs_label_ids and a.score_ssegs == 'x'
    a = parse_args('', [])
    assert not (a.eval_pixels or a.write_ssegs or a.ssegs_label_ids) and a.score_ssegs == ''


def _dataset(tmp_path, sizes):
    from test_dataset_run_cpu import make_dataset, write_cfg
    from upsnet_amd.config.config import update_config
    from upsnet_amd.dataset import Cityscapes
    root = str(tmp_path / 'cs')
    make_dataset(root, 'Cityscapes', sizes)
    update_config(write_cfg(tmp_path, 'Cityscapes', root, 'val'))
    return Cityscapes(image_sets=['val'], phase='test'), root


def test_paths_and_label_map_loading(tmp_path, saved_config):
    from PIL import Image
    ds, root = _dataset(tmp_path, [(8, 12), (8, 12)])
    e = ds.roidb[0]
    assert ds.label_gt_path(e) == os.path.join(root, 'gtFine', 'val', 'city1', 'city1_000001_000019_gtFine_labelIds.png')
    assert os.path.dirname(ds.label_gt_path(e)) == os.path.dirname(ds.instance_gt_path(e))
    with pytest.raises(FileNotFoundError, match='city1_000001_000019_gtFine_labelIds.png'):
        ds.check_pixel_files()
    os.makedirs(os.path.dirname(ds.label_gt_path(e)))
    lab = (np.arange(96, dtype=np.uint8).reshape(8, 12) % 34)
    Image.fromarray(lab).save(ds.label_gt_path(e))
    with pytest.raises(FileNotFoundError, match='city1_000001_000019_gtFine_instanceIds.png'):
        ds.check_pixel_files()
    got = ds.load_label_gt(e)
    assert got.dtype == np.uint8 and np.array_equal(got, lab)
    Image.fromarray(lab[:, :5].copy()).save(ds.label_gt_path(e))
    with pytest.raises(ValueError, match='city1_000001_000019_gtFine_labelIds.png is 8 x 5'):
        ds.load_label_gt(e)
    with open(ds.label_gt_path(e), 'wb') as f:
        f.write(b'not a png')
    with pytest.raises(ValueError, match='cannot read .*city1_000001_000019_gtFine_labelIds.png'):
        ds.load_label_gt(e)


def test_writer_file_names_palette_and_label_ids(tmp_path, saved_config):
    """The reference's file names (<base>.png) and palette: entry t < 19 = the Cityscapes colour of train id t's label, the rest
    zero (tests/golden/cityscapes_pallete.npy: the 768 bytes recorded from the reference's get_pallete); the pixel values are the
    train ids. label_ids=True: grey PNGs of the label ids."""
    from PIL import Image
    ds, root = _dataset(tmp_path, [(8, 12), (6, 10)])
    rng = np.random.default_rng(0)
    segs = [rng.integers(0, 19, (1, e['height'], e['width'])).astype(np.int64) for e in ds.roidb]
    golden = np.load(os.path.join(ROOT, 'tests', 'golden', 'cityscapes_pallete.npy'))
    assert golden.dtype == np.uint8 and golden.shape == (768,)
    assert golden[:9].tolist() == [128, 64, 128, 244, 35, 232, 70, 70, 70] and golden[54:57].tolist() == [119, 11, 32] and not golden[57:].any()
    assert np.array_equal(ds.get_pallete(), golden)
    out = str(tmp_path / 'ssegs')
    ds.write_segmentation_result(segs, out)
    assert sorted(os.listdir(out)) == ['city1_000001_000019.png', 'city2_000002_000019.png']
    for e, seg in zip(ds.roidb, segs):
        with Image.open(ds.segmentation_result_path(e, out)) as im:
            assert im.mode == 'P'
            assert np.array_equal(np.asarray(im), seg[0].astype(np.uint8))
            pal = np.array(im.getpalette(), np.uint8)
            assert np.array_equal(pal, golden[:pal.size]) and pal.size >= 57
    out = str(tmp_path / 'ssegs_label_ids')
    ds.write_segmentation_result(segs, out, label_ids=True)
    for e, seg in zip(ds.roidb, segs):
        with Image.open(ds.segmentation_result_path(e, out)) as im:
            assert im.mode == 'L' and np.array_equal(np.asarray(im), np.array(ref.TRAIN2LABEL, np.uint8)[seg[0]])
    segs[1][0, 0, 0] = 19
    with pytest.raises(ValueError, match='no train id'):
        ds.write_segmentation_result(segs, out, label_ids=True)
    segs[1][0, 0, 0] = 256 + 3          # (a uint8 cast would make it train id 3)
    with pytest.raises(ValueError, match='outside 0..255'):
        ds.write_segmentation_result(segs, out)
    with pytest.raises(ValueError, match='1 semantic predictions for 2 images'):
        ds.write_segmentation_result(segs[:1], out)


@pytest.mark.parametrize('yaml', ['dataset:\n  dataset: coco\n  test_image_set: val\n  dataset_path: "/nonexistent"\n',
                                  'dataset:\n  dataset: Cityscapes\n  test_image_set: val\n  dataset_path: "/nonexistent"\nnetwork:\n  has_fcn_head: false\n'])
def test_flags_need_cityscapes_and_a_semantic_head(yaml, tmp_path, saved_config):
    """Refused with a message naming the flag before the dataset is read (its path does not exist). --score_ssegs builds no model
    and scores any tool's files: it needs Cityscapes only, whatever heads the configuration has."""
    from upsnet_amd.evaluate import main
    cfg = tmp_path / 'exp.yaml'
    cfg.write_text('output_path: "%s"\n' % tmp_path + yaml)
    if 'coco' not in yaml:
        with pytest.raises(FileNotFoundError, match='annotation file not found'):      # past the flag checks, at the dataset
            main(['--cfg', str(cfg), '--score_ssegs', str(tmp_path)])
    for flags in (['--eval_pixels'], ['--write_ssegs']) + ((['--score_ssegs', str(tmp_path)],) if 'coco' in yaml else ()):
        for extra in ([], ['--eval_only']):
            with pytest.raises(SystemExit, match=flags[0]):
                main(['--cfg', str(cfg), '--synthetic_weights'] + flags + extra)


def test_test_split_writes_and_refuses_scoring(tmp_path, saved_config):
    """An image set without ground truth (image_info_test.json): --eval_pixels and --score_ssegs are refused, --ssegs_label_ids
    needs --write_ssegs; --eval_only --write_ssegs writes both kinds from a results pickle (no device is touched)."""
    import pickle
    from PIL import Image
    from test_dataset_run_cpu import make_dataset, write_cfg
    from upsnet_amd.evaluate import main
    root = str(tmp_path / 'cs')
    make_dataset(root, 'Cityscapes', [(8, 12), (6, 10)], anno_name='image_info_test.json')
    cfg = write_cfg(tmp_path, 'Cityscapes', root, 'test')
    with pytest.raises(SystemExit, match='--ssegs_label_ids'):
        main(['--cfg', cfg, '--eval_only', '--ssegs_label_ids'])
    results_dir = os.path.join(str(tmp_path / 'output'), 'exp_eval', 'test', 'results')
    os.makedirs(results_dir)
    rng = np.random.default_rng(1)
    ssegs = [rng.integers(0, 19, (8, 12)).astype(np.uint8), rng.integers(0, 19, (6, 10)).astype(np.uint8)]
    with open(os.path.join(results_dir, 'results_list.pkl'), 'wb') as f:
        pickle.dump({'all_boxes': [[] for _ in range(9)], 'all_masks': [[] for _ in range(9)], 'all_ssegs': ssegs, 'all_panos': [],
                     'all_pano_cls_inds': []}, f)
    with pytest.raises(SystemExit, match='--eval_pixels: cityscapes_test has no ground truth'):
        main(['--cfg', cfg, '--eval_only', '--eval_pixels'])
    with pytest.raises(SystemExit, match='--score_ssegs: cityscapes_test has no ground truth'):
        main(['--cfg', cfg, '--score_ssegs', results_dir])
    with pytest.raises(SystemExit, match='--score_ssegs: no folder'):
        main(['--cfg', cfg, '--score_ssegs', os.path.join(results_dir, 'nowhere')])
    assert main(['--cfg', cfg, '--eval_only', '--write_ssegs'])['metrics'] == {}
    assert main(['--cfg', cfg, '--eval_only', '--write_ssegs', '--ssegs_label_ids'])['metrics'] == {}
    for k, base in enumerate(('city1_000001_000019.png', 'city2_000002_000019.png')):
        with Image.open(os.path.join(results_dir, 'ssegs', base)) as im:
            assert im.mode == 'P' and np.array_equal(np.asarray(im), ssegs[k])
        with Image.open(os.path.join(results_dir, 'ssegs_label_ids', base)) as im:
            assert im.mode == 'L' and np.array_equal(np.asarray(im), np.array(ref.TRAIN2LABEL, np.uint8)[ssegs[k]])


def test_c_entry_point_validates_before_launching():
    """Error code and message for every argument outside the contract; none of these calls reaches a launch (no device here)."""
    import ctypes
    from upsnet_amd import _lib
    l = _lib.lib()
    one = ctypes.c_void_p(256)
    avg = (ctypes.c_double * 8)(*([10.0] * 8))
    assert l.upsnet_cs_pixel_inst_ints() == 8 * 1000 * 3

    def call(gl=one, gi=one, pr=one, lut=one, H=4, W=4, a=avg, conf=one, inst=one, wsum=one, bad=one):
        return l.upsnet_cs_pixel_image(None, gl, gi, pr, lut, H, W, a, conf, inst, wsum, bad)
    zero_avg = (ctypes.c_double * 8)(*([10.0] * 7 + [0.0]))
    for kw, msg in (({'gl': None}, b'null pointer'), ({'pr': None}, b'null pointer'), ({'lut': None}, b'null pointer'),
                    ({'conf': None}, b'null pointer'), ({'bad': None}, b'null pointer'), ({'inst': None}, b'needs inst'),
                    ({'wsum': None}, b'needs inst'), ({'a': None}, b'needs inst'), ({'H': 0}, b'H * W'),
                    ({'H': 1 << 16, 'W': 1 << 15}, b'H * W'), ({'a': zero_avg}, b'average size'),
                    ({'conf': ctypes.c_void_p(260)}, b'misaligned'), ({'gi': ctypes.c_void_p(257)}, b'misaligned')):
        assert call(**kw) != 0, kw
        assert msg in l.upsnet_last_error(), (kw, l.upsnet_last_error())
