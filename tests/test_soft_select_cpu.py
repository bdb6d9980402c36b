"""CPU: the soft detection selection. The numpy restatement (tests/soft_select_ref.py) on a hand-derived case, its
method-0 form against the hard selection of the oracle, the empty and tied cases; the configuration keys and the command line; the C
entry point's argument refusals (no launch without a GPU)."""
import copy
import ctypes

import numpy as np
import pytest

from conftest import ROOT  # noqa: F401  (puts the repo root on sys.path)

import box_vote_ref as bref
import soft_select_ref as ref
from oracle import ops as oops
from test_dataset_run_cpu import write_cfg

F = np.float32
W1 = (1.0, 1.0, 1.0, 1.0)
IM = np.array([600.0, 900.0, 1.0], F)
FLOOR = 1e-4


@pytest.fixture()
def saved_config():
    from upsnet_amd.config.config import config
    saved = copy.deepcopy(dict(config))
    yield config
    config.clear()
    config.update(saved)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def hand_case():
    """Three rows, two classes, zero deltas (an integer roi decodes to itself exactly):
        A = [0,0,9,9] 0.9 (area 100)     B = [0,0,9,4] 0.8 (area 50, inside A: IoU 50 / 100 = 0.5)     C = [100,100,109,109] 0.7"""
    rois = np.array([[0, 0, 0, 9, 9], [0, 0, 0, 9, 4], [0, 100, 100, 109, 109]], F)
    prob = np.array([[0.1, 0.9], [0.2, 0.8], [0.3, 0.7]], F)
    return rois, np.zeros((3, 8), F), prob


def select(rois, delta, prob, n=None, clip=True, score_thresh=0.05, nms_thresh=0.3, max_det=100, method=1, sigma=0.5, floor=FLOOR,
           weights=W1):
    return ref.soft_select(rois, delta, prob, len(prob) if n is None else n, IM, weights, clip, score_thresh, nms_thresh, max_det,
                           method, sigma, floor)


# ------------------------------------------------------------------------------------------------ the rule
def test_hand_case_linear():
    rois, delta, prob = hand_case()
    r = select(rois, delta, prob, method=1)
    assert r['num'] == 3 and r['T'] == 3 and r['per_class'] == [3]
    assert r['src'][:3].tolist() == [0, 2, 1]                     # A, then C (0.7 beats B's decayed 0.4), then B
    assert same_bits(r['scores'][:3], np.array([F(0.9), F(0.7), F(0.8) * F(0.5)], F))
    assert same_bits(r['boxes'][:3], np.concatenate([np.zeros((3, 1), F), rois[[0, 2, 1], 1:]], 1))
    assert r['cls'][:3].tolist() == [1, 1, 1]
    # the rows up to max(max_det, 256), clamped to the capacity (C - 1) * N = 3, are zero rows: here there is none left
    assert len(r['scores']) == 3
    r2 = select(rois, delta, prob, method=1, max_det=2)           # the 2nd largest decayed score is 0.7: A and C stay
    assert r2['num'] == 2 and r2['T'] == 3 and r2['src'][:2].tolist() == [0, 2]
    assert same_bits(r2['scores'][:2], np.array([0.9, 0.7], F))
    assert r2['scores'][2] == 0 and r2['src'][2] == -1 and r2['cls'][2] == 0 and not r2['boxes'][2].any()


def test_hand_case_gaussian():
    rois, delta, prob = hand_case()
    r = select(rois, delta, prob, method=2, sigma=0.5)
    ov = F(50) / F(100)
    weight = F(np.exp(np.float64(-(ov * ov) / F(0.5))))           # the rule: the exponent in float32, exp in double, rounded once
    assert weight == F(np.exp(-0.5))
    assert r['src'][:3].tolist() == [0, 2, 1]
    assert same_bits(r['scores'][:3], np.array([F(0.9), F(0.7), weight * F(0.8)], F))
    assert ref.decayed(r, prob).tolist() == [False, False, True]


def test_hand_case_hard_rule_and_score_threshold():
    rois, delta, prob = hand_case()
    r = select(rois, delta, prob, method=0)                       # B: weight 0, score 0 < floor, removed
    assert r['num'] == 2 and r['src'][:2].tolist() == [0, 2]
    r = select(rois, delta, prob, method=1, score_thresh=0.7)     # strict: C (0.7) is no candidate
    assert r['per_class'] == [2] and r['src'][:2].tolist() == [0, 1]
    r = select(rois, delta, prob, method=1, nms_thresh=0.5)       # linear decays only above Nt (strict): IoU 0.5 is not above 0.5
    assert r['src'][:3].tolist() == [0, 1, 2] and not ref.decayed(r, prob).any()


CLUSTER_CASES = [(63, 2, 100), (64, 9, 100), (200, 9, 100), (1000, 9, 100), (300, 81, 100), (1000, 81, 0), (300, 81, 1000)]


@pytest.mark.parametrize('N,C,max_det', CLUSTER_CASES)
def test_method_zero_is_the_hard_selection(N, C, max_det):
    """Method 0 drops what the hard NMS drops whenever no pair sits near the threshold (the two compute the IoU differently: fp32
    here, double areas in cpu_soft_nms) and the scores are distinct (the hard NMS visits ties by index descending, soft-NMS takes the
    first): asserted here in float64 before the comparison."""
    rng = np.random.default_rng(5)
    rois, delta, prob = ref.cluster_inputs(rng, N, C)
    case = dict(rois=rois, delta=delta, prob=prob)
    n, clip, st, nt = N - 7, True, 0.05, 0.5
    cands = ref.candidates(case['rois'], case['delta'], case['prob'], n, bref.IM_INFO, bref.REG_WEIGHTS, clip, st)
    margin = 1.0
    for c, (dets, rows) in cands.items():
        assert len(np.unique(dets[:, 4])) == len(dets)
        b = dets[:, :4].astype(np.float64)
        iw = np.minimum(b[:, None, 2], b[None, :, 2]) - np.maximum(b[:, None, 0], b[None, :, 0]) + 1
        ih = np.minimum(b[:, None, 3], b[None, :, 3]) - np.maximum(b[:, None, 1], b[None, :, 1]) + 1
        inter = np.clip(iw, 0, None) * np.clip(ih, 0, None)
        area = (b[:, 2] - b[:, 0] + 1) * (b[:, 3] - b[:, 1] + 1)
        iou = inter / (area[:, None] + area[None, :] - inter)
        if len(dets):
            margin = min(margin, float(np.abs(iou - nt).min()))
    assert margin >= 1e-3, margin
    got = ref.soft_select(case['rois'], case['delta'], case['prob'], n, bref.IM_INFO, bref.REG_WEIGHTS, clip, st, nt, max_det, 0, 0.5,
                          FLOOR, cands=cands)
    scores, boxes, cls = oops.mask_roi(case['rois'][:n], case['delta'][:n], case['prob'][:n], bref.IM_INFO, C, nms_thresh=nt,
                                       score_thresh=st, max_det=max_det, bbox_reg_weights=bref.REG_WEIGHTS, clip=clip)
    k = got['num']
    assert k == len(scores) > 0
    assert same_bits(got['scores'][:k], scores) and same_bits(got['boxes'][:k], boxes) and same_bits(got['cls'][:k], cls)
    assert not ref.decayed(got, case['prob']).any()


@pytest.mark.parametrize('method', [1, 2])
def test_soft_methods_keep_decayed_rows_on_cluster_inputs(method):
    """The soft methods keep what the hard rule drops, with a changed score: at C = 9 the hard selection keeps 40 rows (5 clusters x 8
    classes), the soft ones fill max_det = 100 and most of those rows are decayed."""
    rng = np.random.default_rng(5)
    case = bref.cluster_case(rng, 200, 9, 0)
    args = (case['rois'], case['delta'], case['prob'], 193, bref.IM_INFO, bref.REG_WEIGHTS, True, 0.05, 0.5, 100)
    hard = ref.soft_select(*args, 0, 0.5, FLOOR)
    soft = ref.soft_select(*args, method, 0.5, FLOOR)
    assert hard['num'] == 40 and soft['num'] == 100 and soft['T'] > 100
    assert ref.decayed(soft, case['prob']).sum() == 60
    # every undecayed row of the soft result is a row of the hard result
    und = ~ref.decayed(soft, case['prob'])
    assert set(zip(soft['src'][:100][und].tolist(), soft['cls'][:100][und].tolist())) == set(zip(hard['src'][:40].tolist(), hard['cls'][:40].tolist()))


def test_empty_selection_gives_the_dummy_row():
    rois, delta, prob = hand_case()
    for kw in (dict(score_thresh=0.95), dict(n=0), dict(n=-3)):
        r = select(rois, delta, prob, **kw)
        assert r['num'] == 1 and r['T'] == 0
        assert r['scores'][0] == 1 and r['cls'][0] == 0 and r['src'][0] == 0 and not r['boxes'][0].any()
        assert not r['scores'][1:].any() and (r['src'][1:] == -1).all()


def test_exact_score_ties_pass_the_max_det_rule_together():
    """Four boxes that do not overlap, scores 0.9, 0.5, 0.5, 0.5, max_det = 2: the 2nd largest score is 0.5 and `>=` keeps all FOUR
    rows (the reference's rule, mask_roi.py:109-119); ties are visited in row order (first position of the maximum)."""
    rois = np.array([[0, 0, 0, 9, 9], [0, 50, 0, 59, 9], [0, 100, 0, 109, 9], [0, 150, 0, 159, 9]], F)
    prob = np.array([[0.1, 0.5], [0.1, 0.9], [0.1, 0.5], [0.1, 0.5]], F)
    r = select(rois, np.zeros((4, 8), F), prob, max_det=2)
    assert r['num'] == 4 and r['T'] == 4 and r['src'][:4].tolist() == [1, 0, 2, 3]


def test_a_class_beyond_the_limit_is_reported_not_clamped_silently():
    N = ref.CLASS_LIMIT + 1
    rng = np.random.default_rng(3)
    case = bref.cluster_case(rng, N, 2, 0)
    case['prob'][:, 1] = rng.uniform(0.06, 1.0, N).astype(F)
    args = (case['rois'], case['delta'], case['prob'])
    rest = (bref.IM_INFO, bref.REG_WEIGHTS, True, 0.05, 0.5, 100, 1, 0.5, FLOOR)
    over = ref.soft_select(*args, N, *rest)
    fits = ref.soft_select(*args, N - 1, *rest)
    assert over['per_class'] == [N] and fits['per_class'] == [N - 1]
    assert over['num'] == -fits['num'] < 0                         # the first 4096 candidates, and the negative count
    for k in ('boxes', 'scores', 'cls', 'src'):
        assert same_bits(over[k], fits[k])


# ------------------------------------------------------------------------------------------------ configuration and command line
def test_config_defaults_and_validation(saved_config):
    from upsnet_amd.tta import augmentation_enabled, eager_path_enabled, soft_nms_params
    t = saved_config.test
    assert t.soft_nms is False and t.soft_nms_method == 'linear' and t.soft_nms_sigma == 0.5 and t.soft_nms_score_thresh == 0.0001
    assert soft_nms_params() is None and not eager_path_enabled()
    t.soft_nms = True
    assert soft_nms_params() == (1, 0.5, 0.0001)
    assert eager_path_enabled() and not augmentation_enabled()     # soft-NMS alone: the eager path, no augmentation
    t.soft_nms_method, t.soft_nms_sigma, t.soft_nms_score_thresh = 'gaussian', 0.3, 0.0
    assert soft_nms_params() == (2, 0.3, 0.0)
    t.soft_nms_method = 'hard'
    with pytest.raises(ValueError, match='soft_nms_method'):
        soft_nms_params()
    t.soft_nms_method = 'linear'
    for bad in (0.0, -1.0, float('nan')):
        t.soft_nms_sigma = bad
        with pytest.raises(ValueError, match='soft_nms_sigma'):
            soft_nms_params()
    t.soft_nms_sigma = 0.5
    for bad in (-1e-4, float('nan')):
        t.soft_nms_score_thresh = bad
        with pytest.raises(ValueError, match='soft_nms_score_thresh'):
            soft_nms_params()


def test_cli_options_set_the_config(saved_config):
    from upsnet_amd.config.parse_args import parse_args
    t = saved_config.test
    args = parse_args('t', [])
    assert not args.soft_nms and args.soft_nms_method is None and args.soft_nms_sigma is None and t.soft_nms is False
    parse_args('t', ['--soft_nms'])
    assert t.soft_nms is True and t.soft_nms_method == 'linear' and t.soft_nms_sigma == 0.5
    t.soft_nms = False
    parse_args('t', ['--soft_nms', '--soft_nms_method', 'gaussian', '--soft_nms_sigma', '0.3'])
    assert t.soft_nms is True and t.soft_nms_method == 'gaussian' and t.soft_nms_sigma == 0.3
    t.soft_nms = False
    for extra in (['--soft_nms_method', 'gaussian'], ['--soft_nms_sigma', '0.3'], ['--soft_nms', '--soft_nms_method', 'hard']):
        with pytest.raises(SystemExit):
            parse_args('t', extra)                                  # a parameter of a soft-NMS that is off; an unknown method
        t.soft_nms = False


def test_yaml_keys_set_the_config(tmp_path, saved_config):
    from upsnet_amd.config.parse_args import parse_args
    from upsnet_amd.tta import soft_nms_params
    cfg = write_cfg(tmp_path, 'Cityscapes', str(tmp_path / 'data'), 'val',
                    extra='  soft_nms: true\n  soft_nms_method: gaussian\n  soft_nms_sigma: 0.4\n  soft_nms_score_thresh: 0.001\n')
    parse_args('t', ['--cfg', cfg])
    assert soft_nms_params() == (2, 0.4, 0.001)
    parse_args('t', ['--cfg', cfg, '--soft_nms_method', 'linear'])  # the yaml switched it on
    assert soft_nms_params() == (1, 0.4, 0.001)


def test_eval_proposals_and_bad_parameters_are_refused_up_front(tmp_path, saved_config):
    from upsnet_amd.evaluate import main
    cfg = write_cfg(tmp_path, 'Cityscapes', str(tmp_path / 'data'), 'val')
    with pytest.raises(SystemExit) as e:
        main(['--cfg', cfg, '--synthetic_weights', '--soft_nms', '--eval_proposals'])
    assert '--eval_proposals' in str(e.value) and '--soft_nms' in str(e.value)
    saved_config.test.soft_nms = False
    with pytest.raises(SystemExit) as e:
        main(['--cfg', cfg, '--synthetic_weights', '--soft_nms', '--soft_nms_sigma', '0'])
    assert 'soft_nms_sigma' in str(e.value)


def test_forward_tta_refuses_keep_proposals_with_soft_nms_alone(saved_config):
    from upsnet_amd.tta import forward_tta

    class Model:
        keep_proposals = True
    saved_config.test.soft_nms = True
    with pytest.raises(ValueError, match='proposal'):
        forward_tta(Model(), np.zeros((8, 8, 3), np.uint8))


def test_mask_roi_module_refuses_soft_nms_with_the_class_agnostic_selection():
    from upsnet_amd.operators.modules.mask_roi import MaskROI, check_count_soft
    with pytest.raises(ValueError, match='class'):
        MaskROI(True, False, 100, 9, class_agnostic=True, soft_nms=(1, 0.5, 1e-4))
    m = MaskROI(True, False, 100, 9, soft_nms=[2, 0.5, 1e-4])
    assert m.soft_nms == (2, 0.5, 1e-4) and MaskROI(True, False, 100, 9).soft_nms is None
    assert check_count_soft(7) == 7
    with pytest.raises(RuntimeError, match='4096'):
        check_count_soft(-7)


def test_bbox_transform_soft_nms_on_an_empty_input():
    from upsnet_amd.bbox.bbox_transform import soft_nms
    dets = np.zeros((0, 5), F)
    out, keep = soft_nms(dets)
    assert out is dets and keep == []
    with pytest.raises(ValueError, match='method'):
        soft_nms(np.zeros((1, 5), F), method='cubic')


# ------------------------------------------------------------------------------------------------ C entry point
def test_entry_point_refuses_bad_arguments_without_a_gpu():
    from upsnet_amd import _lib
    lib = _lib.lib()
    one = ctypes.c_void_p(64)
    w = (ctypes.c_float * 4)(10.0, 10.0, 5.0, 5.0)
    err = lambda: lib.upsnet_last_error()

    def call(rois=one, delta=one, prob=one, N=100, ndev=one, C=9, im=one, clip=1, st=0.05, nt=0.5, max_det=100, weights=w, method=1,
             sigma=0.5, floor=1e-4, boxes=one, scores=one, cls=one, src=one, num=one, ws=one):
        return lib.upsnet_mask_roi_soft(None, rois, delta, prob, N, ndev, C, im, clip, st, nt, max_det, weights, method, sigma, floor,
                                        boxes, scores, cls, src, num, ws)
    for name in ('rois', 'delta', 'prob', 'im', 'weights', 'boxes', 'scores', 'cls', 'src', 'num', 'ws'):
        assert call(**{name: None}) != 0 and b"null pointer" in err(), name
    for N in (0, -1):
        assert call(N=N) != 0 and b"roi" in err()
    assert call(N=8193) != 0 and b"8192" in err()
    for C in (1, 0, -3):
        assert call(C=C) != 0 and b"classes" in err()
    for method in (-1, 3):
        assert call(method=method) != 0 and b"method" in err()
    for sigma in (0.0, -0.5, float('nan')):
        assert call(method=2, sigma=sigma) != 0 and b"sigma" in err()
    assert call(nt=float('nan')) != 0 and b"NaN" in err()
    assert call(floor=float('nan')) != 0 and b"NaN" in err()
    # the workspace: the candidate tables of every class (16 + 4 * 5 bytes per row) and nothing for an NMS mask
    small, hard = lib.upsnet_mask_roi_soft_workspace_bytes(1000, 81), lib.upsnet_mask_roi_workspace_bytes(1000, 81, 0)
    assert 80 * 1000 * 36 <= small < hard
