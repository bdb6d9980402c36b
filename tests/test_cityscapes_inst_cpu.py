"""CPU: the Cityscapes instance-level AP rules. Hand-derived cases pin the numpy restatement
(tests/cityscapes_inst_ref.py) that the GPU tests compare the device evaluator with; the seeded scenes of the GPU tests are shown to
reach every branch of the rules; the command-line flag, the dataset's paths and the refusals that need no device.

Notation of the hand-derived cases: the AP of one (class, threshold) is sum_i precision[i] * w[i] with w = convolve([r0, r0, r1, ...,
0, 0], [-.5, 0, .5], 'valid'), i.e. w[i] = (r[i - 1] - r[i + 1]) / 2 over the recall list padded with its first value in front and 0
behind, precision / recall listed for ascending unique scores and ending with the artificial point (1, 0)."""
import copy
import os

import numpy as np
import pytest

from conftest import ROOT  # noqa: F401  (puts the repo root on sys.path)

import cityscapes_inst_cases as cases
import cityscapes_inst_ref as ref

T = ref.OVERLAPS
PERSON, RIDER, CAR, TRUCK, BUS, TRAIN, MOTORCYCLE, BICYCLE = range(8)


def road(H=60, W=80):
    return np.full((H, W), 7, np.uint16)


def rect(H, W, y0, x0, h, w):
    m = np.zeros((H, W), bool)
    m[y0:y0 + h, x0:x0 + w] = True
    return m


def pred(cls, conf, mask):
    return {'cls': cls, 'conf': np.float32(conf), 'mask': mask}


def car_with_tp(gt, conf=0.5, value=26001):
    """A valid car region of 20 x 20 at (2, 2) and its exact prediction."""
    m = rect(gt.shape[0], gt.shape[1], 2, 2, 20, 20)
    gt[m] = value
    return pred(3, conf, m)


def only_class(aps, c):
    others = [k for k in range(8) if k != c]
    assert np.all(np.isnan(aps[others])), aps
    return aps[c]


def test_thresholds_are_numpys_doubles():
    assert T.tolist() == [0.5, 0.55, 0.6000000000000001, 0.6500000000000001, 0.7000000000000002, 0.7500000000000002,
                          0.8000000000000003, 0.8500000000000003, 0.9000000000000004, 0.9500000000000004]


def test_perfect_prediction():
    """One entry (1, .9), no hard FN: precision [1, 1], recall [1, 0], w = [(1 - 0) / 2, (1 - 0) / 2] -> AP 1 at every threshold."""
    gt = road()
    p = car_with_tp(gt, 0.9)
    aps, avg, counts = ref.evaluate([(gt, [p])])
    assert np.all(only_class(aps, CAR) == 1.0)
    assert avg['AP'] == 1.0 and avg['AP50'] == 1.0 and avg['per_class']['car'] == {'ap': 1.0, 'ap50': 1.0}
    assert np.isnan(avg['per_class']['person']['ap'])
    assert counts[0] == [{'area': 400, 'void': 0, 'inter': {26001: 400}}]


def test_overlap_exactly_300_of_500_matches_at_the_first_two_thresholds_only():
    """GT 20 x 20, the prediction the same box 5 columns to the right: intersection 20 x 15 = 300, union 500, overlap = 0.6 (the
    double nearest 0.6). 0.6 > 0.5 and 0.6 > 0.55 match; the third threshold is 0.6000000000000001 > 0.6, and the match is strict: no
    match from there on. Unmatched, the prediction is a false positive (ignore share 0) and the GT a hard FN: precision [0, 1],
    recall [0, 0] -> AP 0. Average over the ten thresholds 0.2."""
    gt = road()
    car_with_tp(gt)
    aps, avg, _ = ref.evaluate([(gt, [pred(3, 0.9, rect(60, 80, 2, 7, 20, 20))])])
    assert only_class(aps, CAR).tolist() == [1.0, 1.0] + [0.0] * 8
    assert avg['AP'] == pytest.approx(0.2, abs=1e-15) and avg['AP50'] == 1.0


def test_second_prediction_on_one_gt_is_a_false_positive_with_its_own_score():
    """GT a with exact predictions of .9 and .6, GT b with one of .3. Entries (1, .9), (0, .6), (1, .3). Ascending scores .3 .6 .9, true
    1 0 1: at .3 tp 2 fp 1 fn 0 -> (2/3, 1); at .6 tp 1 fp 1 fn 1 -> (1/2, 1/2); at .9 tp 1 fp 0 fn 1 -> (1, 1/2); then (1, 0).
    Recall list 1 .5 .5 0 -> w = [.25, .25, .25, .25]; AP = (2/3 + 1/2 + 1 + 1) / 4 = 19/24. (Were the .9 the false positive and the .6
    the true one, the AP would be 5/12.)"""
    gt = road()
    a = rect(60, 80, 2, 2, 20, 20)
    b = rect(60, 80, 30, 40, 20, 20)
    gt[a] = 26001
    gt[b] = 26002
    aps, _, _ = ref.evaluate([(gt, [pred(3, 0.6, a), pred(3, 0.3, b), pred(3, 0.9, a)])])
    assert np.allclose(only_class(aps, CAR), 19.0 / 24.0, rtol=0, atol=1e-15)


def test_prediction_lying_80_percent_on_void():
    """A car prediction of 100 pixels, 80 of them on raw value 0 (void) and 20 on road, score .9; elsewhere a car GT with its exact
    prediction of .5. Ignore share = 80 / 100 = 0.8 (the double 0.8000000000000000444). It is ignored while 0.8 > t: t[0..5] (up to
    0.7500000000000002); t[6] = 0.8000000000000003 >= 0.8, so from index 6 on it is a false positive above the true one: entries
    (1, .5), (0, .9): at .5 tp 1 fp 1 -> (1/2, 1); at .9 tp 0 fp 1 fn 1 -> (0, 0); then (1, 0). Recall list 1 0 0 -> w = [.5, .5, 0]:
    AP = 1/4. Before that the single true positive gives 1."""
    gt = road()
    tp = car_with_tp(gt)
    gt[40:50, 30:38] = 0
    aps, _, counts = ref.evaluate([(gt, [tp, pred(3, 0.9, rect(60, 80, 40, 30, 10, 10))])])
    assert counts[0][1] == {'area': 100, 'void': 80, 'inter': {}}
    assert only_class(aps, CAR).tolist() == [1.0] * 6 + [0.25] * 4


def test_prediction_on_a_group_region():
    """A group region (raw value 26) of 20 x 20. Its exact prediction (.9) overlaps it with 1.0 > t: found, but a group is no valid GT,
    so it is neither true nor false positive: the AP stays 1. A second scene: a prediction of 100 pixels with 60 on the group and 40 on
    road: overlap 60 / (400 + 100 - 60) < 0.5, ignore share 60 / 100 = 0.6: ignored at 0.5 and 0.55, and 0.6 <= 0.6000000000000001
    makes it a false positive from index 2 on (1/4, as in the void case)."""
    gt = road()
    tp = car_with_tp(gt)
    g = rect(60, 80, 30, 40, 20, 20)
    gt[g] = 26
    aps, _, _ = ref.evaluate([(gt, [tp, pred(3, 0.9, g)])])
    assert np.all(only_class(aps, CAR) == 1.0)
    aps, _, counts = ref.evaluate([(gt, [tp, pred(3, 0.9, rect(60, 80, 35, 36, 10, 10))])])
    assert counts[0][1] == {'area': 100, 'void': 0, 'inter': {26: 60}}
    assert only_class(aps, CAR).tolist() == [1.0, 1.0] + [0.25] * 8


def test_gt_of_99_pixels_is_not_valid():
    """A car instance of 9 x 11 = 99 pixels alone: no valid GT, the class is NaN whatever is predicted. Next to a valid GT with its
    true positive (.5), the exact prediction of the small one (.9) is found (overlap 1) and so neither counted nor a false positive: 1.
    A prediction of 198 pixels holding the 99: overlap 0.5, not > 0.5; ignore share 99 / 198 = 0.5 <= t everywhere: a false positive
    at every threshold (1/4)."""
    gt = road()
    small = rect(60, 80, 40, 40, 9, 11)
    gt[small] = 26005
    aps, _, _ = ref.evaluate([(gt, [pred(3, 0.9, small)])])
    assert np.all(np.isnan(aps))
    tp = car_with_tp(gt)
    aps, _, _ = ref.evaluate([(gt, [tp, pred(3, 0.9, small)])])
    assert np.all(only_class(aps, CAR) == 1.0)
    aps, _, counts = ref.evaluate([(gt, [tp, pred(3, 0.9, rect(60, 80, 40, 40, 18, 11))])])
    assert counts[0][1] == {'area': 198, 'void': 0, 'inter': {26005: 99}}
    assert np.all(only_class(aps, CAR) == 0.25)


def test_raw_value_29003_is_not_void_but_29_is():
    """The void test is on the raw value: a caravan instance 29003 is not void (the prediction on it is a false positive: 1/4), the
    bare label 29 is (the prediction on it is ignored at every threshold: 1)."""
    for value, want, void in ((29003, 0.25, 0), (29, 1.0, 100)):
        gt = road()
        tp = car_with_tp(gt)
        gt[40:50, 30:40] = value
        aps, _, counts = ref.evaluate([(gt, [tp, pred(3, 0.9, rect(60, 80, 40, 30, 10, 10))])])
        assert counts[0][1]['void'] == void
        assert np.all(only_class(aps, CAR) == want), value


def test_class_with_gt_and_no_prediction_is_zero_and_class_with_neither_is_left_out():
    """person: a valid GT, no prediction -> 0.0; car: perfect -> 1.0; rider: a prediction and no GT -> NaN; the other five NaN. The
    means run over person and car only: AP = AP50 = 0.5."""
    gt = road()
    tp = car_with_tp(gt)
    gt[rect(60, 80, 30, 40, 20, 20)] = 24001
    aps, avg, _ = ref.evaluate([(gt, [tp, pred(2, 0.7, rect(60, 80, 30, 10, 10, 10))])])
    assert np.all(aps[PERSON] == 0.0) and np.all(aps[CAR] == 1.0)
    assert np.all(np.isnan(aps[[RIDER, TRUCK, BUS, TRAIN, MOTORCYCLE, BICYCLE]]))
    assert avg['AP'] == 0.5 and avg['AP50'] == 0.5
    assert avg['per_class']['person'] == {'ap': 0.0, 'ap50': 0.0} and np.isnan(avg['per_class']['rider']['ap50'])


def test_equal_scores_in_two_images():
    """Image 1: a true positive of .5; image 2: a car prediction on road of .5. One unique score: tp 1 fp 1 -> (1/2, 1), then (1, 0);
    recall list 1 0 -> w = [.5, .5]; AP = 1/4 + 1/2 = 3/4 (1 or 1/4 if the tie were broken either way)."""
    gt1 = road()
    tp = car_with_tp(gt1)
    gt2 = road()
    fp = pred(3, 0.5, rect(60, 80, 30, 30, 10, 10))
    for images in ([(gt1, [tp]), (gt2, [fp])], [(gt2, [fp]), (gt1, [tp])]):
        aps, _, _ = ref.evaluate(images)
        assert np.all(only_class(aps, CAR) == 0.75)


def test_zero_area_prediction_is_dropped():
    gt = road()
    tp = car_with_tp(gt)
    aps, _, counts = ref.evaluate([(gt, [pred(3, 0.9, np.zeros((60, 80), bool)), tp])])
    assert counts[0][0] is None and np.all(only_class(aps, CAR) == 1.0)
    # alone it does not even make the class "predicted": GT without predictions -> 0.0
    aps, _, _ = ref.evaluate([(gt, [pred(3, 0.9, np.zeros((60, 80), bool))])])
    assert np.all(only_class(aps, CAR) == 0.0)


# ------------------------------------------------------------------------------------------------ the GPU tests' scenes
@pytest.mark.parametrize('name', sorted(cases.GPU_SCENES))
def test_random_scenes_reach_every_branch(name):
    """A condition on the inputs of tests/test_cityscapes_inst_gpu.py: each scene list, through the restatement alone, takes every
    branch of the rules and has a class of each of the three AP cases."""
    seed, sizes, n_regions = cases.GPU_SCENES[name]
    stats = {}
    aps, _, counts = ref.evaluate(cases.make_scene(seed, sizes, n_regions), stats)
    for key in ('duplicate_matchers', 'ignored_predictions', 'group_intersections', 'small_gt_intersections', 'void_intersections',
                'matched_only_non_valid', 'tied_scores_across_images', 'hard_false_negatives', 'false_positives', 'ap_curve', 'ap_zero',
                'ap_nan', 'ap_nan_with_pred'):
        assert stats.get(key, 0) > 0, (key, stats)
    assert any(c is None for img in counts for c in img), "no prediction of zero area"
    assert np.all(aps[TRAIN] == 0.0) and np.all(np.isnan(aps[[BUS, MOTORCYCLE]]))
    curve = aps[[PERSON, CAR]]
    assert np.all((curve > 0.0) & (curve < 1.0)), curve      # neither trivial case
    assert len(np.unique(aps[CAR])) > 3                       # the thresholds separate the matches


def test_rle_of_round_trips():
    rng = np.random.default_rng(5)
    for H, W in ((7, 5), (1, 9), (9, 1)):
        m = rng.random((H, W)) < 0.5
        m[0, 0] = True
        r = cases.rle_of(m)
        flat = np.repeat(np.arange(len(r['counts'])) % 2, r['counts']).astype(bool)
        assert r['counts'][0] == 0 and np.array_equal(flat.reshape(W, H).T, m)


# ------------------------------------------------------------------------------------------------ command line, paths, refusals
@pytest.fixture()
def saved_config():
    from upsnet_amd.config.config import config
    saved = copy.deepcopy(dict(config))
    yield config
    config.clear()
    config.update(saved)


def test_parse_args_knows_the_flag():
    from upsnet_amd.config.parse_args import parse_args
    assert parse_args('', ['--eval_instances']).eval_instances is True
    assert parse_args('', []).eval_instances is False


def test_module_tables():
    from upsnet_amd.dataset import cityscapes_eval as ce
    assert list(zip(ce.CLASS_NAMES, ce.CLASS_LABEL_IDS)) == ref.CLASSES
    assert list(ce.VOID_VALUES) == ref.VOID_IDS and ce.MIN_REGION_SIZE == 100
    assert ce.OVERLAPS.dtype == np.float64 and np.array_equal(ce.OVERLAPS, np.arange(0.5, 1.0, 0.05))


def test_instance_gt_path(tmp_path, saved_config):
    from test_dataset_run_cpu import make_dataset, write_cfg
    from upsnet_amd.config.config import update_config
    from upsnet_amd.dataset import Cityscapes
    root = str(tmp_path / 'cs')
    make_dataset(root, 'Cityscapes', [(8, 8)] * 2)
    update_config(write_cfg(tmp_path, 'Cityscapes', root, 'val'))
    ds = Cityscapes(image_sets=['val'], phase='test')
    assert ds.instance_gt_path(ds.roidb[0]) == os.path.join(root, 'gtFine', 'val', 'city1', 'city1_000001_000019_gtFine_instanceIds.png')
    e = {'image': os.path.join(root, 'images', 'frankfurt_000001_000294_leftImg8bit.png')}
    assert ds.instance_gt_path(e) == os.path.join(root, 'gtFine', 'val', 'frankfurt', 'frankfurt_000001_000294_gtFine_instanceIds.png')
    with pytest.raises(ValueError, match='leftImg8bit'):
        ds.instance_gt_path({'image': os.path.join(root, 'images', 'x.jpg')})
    with pytest.raises(FileNotFoundError, match='city1_000001_000019_gtFine_instanceIds.png'):
        ds.check_instance_files()
    assert callable(getattr(Cityscapes, 'evaluate_instances', None))


def test_unreadable_or_wrongly_sized_map_is_named(tmp_path, saved_config):
    from PIL import Image
    from test_dataset_run_cpu import make_dataset, write_cfg
    from upsnet_amd.config.config import update_config
    from upsnet_amd.dataset import Cityscapes
    root = str(tmp_path / 'cs')
    make_dataset(root, 'Cityscapes', [(8, 12)])
    update_config(write_cfg(tmp_path, 'Cityscapes', root, 'val'))
    ds = Cityscapes(image_sets=['val'], phase='test')
    path = ds.instance_gt_path(ds.roidb[0])
    os.makedirs(os.path.dirname(path))
    ids = (np.arange(96, dtype=np.uint16).reshape(8, 12) * 600)
    Image.fromarray(ids).save(path)
    got = ds.load_instance_gt(ds.roidb[0])
    assert got.dtype == np.uint16 and np.array_equal(got, ids)
    Image.fromarray(ids[:, :5].copy()).save(path)
    with pytest.raises(ValueError, match='city1_000001_000019_gtFine_instanceIds.png is 8 x 5'):
        ds.load_instance_gt(ds.roidb[0])
    with open(path, 'wb') as f:
        f.write(b'not a png')
    with pytest.raises(ValueError, match='cannot read .*city1_000001_000019_gtFine_instanceIds.png'):
        ds.load_instance_gt(ds.roidb[0])


@pytest.mark.parametrize('yaml', ['dataset:\n  dataset: coco\n  dataset_path: "/nonexistent"\n',
                                  'dataset:\n  dataset: Cityscapes\n  dataset_path: "/nonexistent"\nnetwork:\n  has_mask_head: false\n'])
def test_eval_instances_needs_cityscapes_and_a_mask_head(yaml, tmp_path, saved_config):
    """Refused with a message naming the flag before the dataset is read (its path does not exist)."""
    from upsnet_amd.evaluate import main
    cfg = tmp_path / 'exp.yaml'
    cfg.write_text('output_path: "%s"\n' % tmp_path + yaml)
    for extra in ([], ['--eval_only']):
        with pytest.raises(SystemExit, match='--eval_instances'):
            main(['--cfg', str(cfg), '--synthetic_weights', '--eval_instances'] + extra)


def test_c_entry_point_validates_before_launching():
    """Error code and message for every argument outside the contract; none of these calls reaches a launch (no device here)."""
    import ctypes
    from upsnet_amd import _lib
    l = _lib.lib()
    thr = (ctypes.c_double * 2)(0.5, 0.75)
    one = ctypes.c_void_p(256)
    assert l.upsnet_cs_inst_counts_ints(2) == 2 * 1003 + 8 * 1001 and l.upsnet_cs_inst_counts_ints(-1) == 0
    assert l.upsnet_cs_inst_counts_ints(65536) == 0 and l.upsnet_cs_inst_workspace_bytes(65536) == 0
    assert l.upsnet_cs_inst_workspace_bytes(0) >= 24 and l.upsnet_cs_inst_state_words() == 8 * 16 + 16

    def call(gt=one, H=4, W=4, n=0, cls=None, sc=None, tr=None, off=None, masks=None, thresholds=thr, nt=2, counts=one, ws=one, state=one):
        return l.upsnet_cs_inst_image(None, gt, H, W, n, cls, sc, tr, off, masks, 0, None, thresholds, nt, counts, ws, None, None, None, state)
    for kw, msg in (({'gt': None}, b'null pointer'), ({'counts': None}, b'null pointer'), ({'state': None}, b'null pointer'),
                    ({'H': 0}, b'H * W'), ({'H': 1 << 16, 'W': 1 << 15}, b'H * W'), ({'n': -1}, b'predictions'), ({'n': 65536}, b'predictions'),
                    ({'nt': 0}, b'thresholds'), ({'nt': 17}, b'thresholds'), ({'thresholds': (ctypes.c_double * 2)(0.4, 0.5)}, b'outside'),
                    ({'n': 1}, b'null pointer'), ({'counts': ctypes.c_void_p(258)}, b'misaligned')):
        assert call(**kw) != 0, kw
        assert msg in l.upsnet_last_error(), (kw, l.upsnet_last_error())
    rec = (one, one, one)

    def call_n(tr, off, masks):
        return l.upsnet_cs_inst_image(None, one, 4, 4, 1, one, one, tr, off, masks, 0, None, thr, 2, one, one, *rec, one)
    assert call_n(one, one, one) != 0 and b'not both or neither' in l.upsnet_last_error()
    assert call_n(None, None, None) != 0 and b'not both or neither' in l.upsnet_last_error()
    assert call_n(None, one, None) != 0 and b'null pointer' in l.upsnet_last_error()
    assert call_n(one, one, None) != 0 and b'gt_t' in l.upsnet_last_error()
