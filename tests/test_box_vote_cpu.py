"""CPU: the box voting rule. The numpy float32 restatement (tests/box_vote_ref.py) on a hand-derived case, its stated
consequences, and against the same formula in float64; the configuration keys and the command line; the C entry point's argument
refusals (no launch without a GPU)."""
import copy
import ctypes

import numpy as np
import pytest

from conftest import ROOT  # noqa: F401  (puts the repo root on sys.path)

import box_vote_ref as ref
from test_dataset_run_cpu import write_cfg

F = np.float32
W1 = (1.0, 1.0, 1.0, 1.0)
IM = np.array([600.0, 900.0, 1.0], F)


@pytest.fixture()
def saved_config():
    from upsnet_amd.config.config import config
    saved = copy.deepcopy(dict(config))
    yield config
    config.clear()
    config.update(saved)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def hand_case():
    """70 rows, 2 classes, zero deltas (the class-1 candidate of a row is its roi, exactly). Kept box [10,10,50,50]; voters in the
    stripes 0, 3 and 5 with the weights 1/2, 1/4, 1/4:
        row 0   [10,10,50,50]  0.5      row 3   [12,10,50,52]  0.25      row 69  [8,10,54,48]  0.25
    S_w = 1, S = (5 + 3 + 2, 5 + 2.5 + 2.5, 25 + 12.5 + 13.5, 25 + 13 + 12) = (10, 10, 51, 50): every term and sum is exact.
    Not voters: row 1 overlaps but has probability 0.05 (not > 0.05), row 2 has probability 0.9 but lies elsewhere, row 64 (stripe 0)
    overlaps with IoU 0.15 < 0.5."""
    N, C = 70, 2
    rois = np.zeros((N, 5), F)
    rois[:, 1:] = [700, 400, 760, 470]
    prob = np.full((N, C), 0.01, F)
    rois[0, 1:], prob[0, 1] = [10, 10, 50, 50], 0.5
    rois[3, 1:], prob[3, 1] = [12, 10, 50, 52], 0.25
    rois[69, 1:], prob[69, 1] = [8, 10, 54, 48], 0.25
    rois[1, 1:], prob[1, 1] = [10, 10, 50, 50], 0.05
    prob[2, 1] = 0.9
    rois[64, 1:], prob[64, 1] = [30, 30, 70, 70], 0.9
    delta = np.zeros((N, 4 * C), F)
    boxes = np.zeros((3, 5), F)
    boxes[0] = [0, 10, 10, 50, 50]
    boxes[1] = [7, 300, 100, 350, 160]           # no candidate near it
    boxes[2] = [3, 1, 2, 3, 4]                   # past the count
    cls = np.array([1, 1, 1], np.int64)
    return rois, delta, prob, boxes, cls


def test_hand_derived_case_is_exact():
    rois, delta, prob, boxes, cls = hand_case()
    voted, counts = ref.box_vote(rois, delta, prob, 70, IM, W1, True, boxes, cls, 2, 0.05, 0.5, want_counts=True)
    assert counts == [3, 0]
    assert same_bits(voted[0], np.array([0, 10, 10, 51, 50], F))
    assert same_bits(voted[1:], boxes[1:])                     # no voter: unchanged; past the count: a copy
    # a device row count of 69 takes row 69 out: S_w = 0.75, S = (8, 7.5, 37.5, 38) -> 32/3, 10, 50, 152/3 rounded once
    voted = ref.box_vote(rois, delta, prob, 69, IM, W1, True, boxes, cls, 2, 0.05, 0.5)
    assert same_bits(voted[0], np.array([0, F(8) / F(0.75), 10, 50, F(38) / F(0.75)], F))


def test_iou_threshold_above_one_returns_the_input():
    rng = np.random.default_rng(1)
    case = ref.cluster_case(rng, 200, 9, 20, big=150)
    voted = ref.box_vote(case['rois'], case['delta'], case['prob'], 200, ref.IM_INFO, ref.REG_WEIGHTS, True, case['boxes'], case['cls'],
                         case['num'], 0.05, 1.5)
    assert same_bits(voted, case['boxes'])


def test_class_without_candidate_above_the_threshold_is_unchanged():
    rng = np.random.default_rng(2)
    case = ref.cluster_case(rng, 200, 9, 20, big=150)
    case['prob'][:, 3] = rng.uniform(0, 0.05, 200).astype(F)       # class 3: nothing above 0.05 (0.05 itself is not above)
    case['prob'][0, 3] = F(0.05)
    voted, counts = ref.box_vote(case['rois'], case['delta'], case['prob'], 200, ref.IM_INFO, ref.REG_WEIGHTS, True, case['boxes'],
                                 case['cls'], case['num'], 0.05, 0.5, want_counts=True)
    rows = np.nonzero(case['cls'][:20] == 3)[0]
    assert len(rows) > 0 and all(counts[k] == 0 for k in rows)
    assert same_bits(voted[rows], case['boxes'][rows])
    assert any(counts[k] >= 2 for k in range(20)) and not same_bits(voted[:20], case['boxes'][:20])


@pytest.mark.parametrize('num', [0, 7, 20, 57, 100, -1, -20])
def test_rows_at_or_past_the_count_are_copies(num):
    rng = np.random.default_rng(3)
    case = ref.cluster_case(rng, 100, 5, 20)                       # cap = 57
    voted = ref.box_vote(case['rois'], case['delta'], case['prob'], 100, ref.IM_INFO, ref.REG_WEIGHTS, True, case['boxes'], case['cls'],
                         num, 0.05, 0.5)
    kn = min(max(num, 0), 57)
    assert same_bits(voted[kn:], case['boxes'][kn:])
    assert same_bits(voted[:, 0], case['boxes'][:, 0])
    if 0 < kn <= 20:
        assert not same_bits(voted[:kn], case['boxes'][:kn])


def test_single_voter_comes_back_within_an_ulp():
    """A row whose only voter is itself: (w * x) / w may round, so it is within 1 ulp and not special-cased."""
    rng = np.random.default_rng(4)
    for _ in range(50):
        case = ref.cluster_case(rng, 5, 3, 1, clip=False)
        case['rois'][:, 1:] += (np.arange(5) * 1000)[:, None].astype(F)      # no two rows overlap
        case['boxes'][0, 1:] = ref.decode(case['rois'], case['delta'], int(case['cls'][0]), 5, ref.IM_INFO, ref.REG_WEIGHTS, False)[case['src'][0]]
        case['prob'][case['src'][0], case['cls'][0]] = F(rng.uniform(0.1, 1.0))
        voted, counts = ref.box_vote(case['rois'], case['delta'], case['prob'], 5, ref.IM_INFO, ref.REG_WEIGHTS, False, case['boxes'],
                                     case['cls'], 1, 0.05, 0.8, want_counts=True)
        assert counts == [1]
        b = case['boxes'][0, 1:]
        assert np.all(np.abs(voted[0, 1:] - b) <= np.spacing(np.abs(b)))


def test_same_source_and_class_gives_the_same_box_in_any_kept_list():
    rng = np.random.default_rng(5)
    case = ref.cluster_case(rng, 300, 9, 30, big=150)
    args = (case['rois'], case['delta'], case['prob'], 300, ref.IM_INFO, ref.REG_WEIGHTS, True)
    a = ref.box_vote(*args, case['boxes'], case['cls'], 30, 0.05, 0.8)
    order = rng.permutation(30)[:11]
    b = ref.box_vote(*args, case['boxes'][order], case['cls'][order], 11, 0.05, 0.8)
    assert same_bits(b, a[order])


def test_float32_rule_against_float64_on_seeded_cases():
    """300 seeded cases; per row the bound max|coord| * (2 * ceil(V / 64) + 16) * 2^-24 of DESIGN 4.21 (ref.bound)."""
    rng = np.random.default_rng(6)
    worst, most = 0.0, 0
    for i in range(300):
        N = int(rng.choice([1, 5, 63, 64, 65, 130, 200, 400]))
        C = int(rng.choice([2, 5, 9]))
        kept = int(rng.integers(1, 7))
        clip = bool(i % 2)
        thr = (0.5, 0.8)[(i // 2) % 2]
        case = ref.cluster_case(rng, N, C, kept, clip=clip, big=(150 if N >= 200 else 0), pad=2)
        n = N - (N // 9)
        args = (case['rois'], case['delta'], case['prob'], n, ref.IM_INFO, ref.REG_WEIGHTS, clip, case['boxes'], case['cls'], kept, 0.05, thr)
        got, counts = ref.box_vote(*args, want_counts=True)
        want, counts64, mags = ref.box_vote_f64(*args)
        assert counts == counts64
        for k in range(kept):
            err = float(np.abs(got[k, 1:].astype(np.float64) - want[k]).max())
            lim = ref.bound(mags[k], counts[k])
            assert err <= lim, (i, k, counts[k], err, lim)
            if lim:
                worst = max(worst, err / lim)
            most = max(most, counts[k])
    print('largest error / bound %.3f, most voters %d' % (worst, most))
    assert most > 128


# ------------------------------------------------------------------------------------------------ configuration and command line
def test_config_defaults(saved_config):
    from upsnet_amd.tta import augmentation_enabled, bbox_vote_params, eager_path_enabled
    assert saved_config.test.bbox_vote is False and saved_config.test.bbox_vote_thresh == 0.8
    assert bbox_vote_params() is None and not eager_path_enabled() and not augmentation_enabled()
    saved_config.test.bbox_vote = True
    assert bbox_vote_params() == (float(saved_config.test.score_thresh), 0.8)
    assert eager_path_enabled() and not augmentation_enabled()          # voting alone: the eager path, no augmentation
    saved_config.test.score_thresh, saved_config.test.panoptic_score_thresh, saved_config.test.bbox_vote_thresh = 0.1, 0.6, 0.65
    assert bbox_vote_params() == (0.1, 0.65)                             # always test.score_thresh
    for bad in (0.0, -0.5, float('nan')):
        saved_config.test.bbox_vote_thresh = bad
        with pytest.raises(ValueError, match='bbox_vote_thresh'):
            bbox_vote_params()


def test_cli_options_set_the_config(saved_config):
    from upsnet_amd.config.parse_args import parse_args
    args = parse_args('t', [])
    assert not args.bbox_vote and args.bbox_vote_thresh is None
    assert saved_config.test.bbox_vote is False and saved_config.test.bbox_vote_thresh == 0.8
    args = parse_args('t', ['--bbox_vote'])
    assert args.bbox_vote and saved_config.test.bbox_vote is True and saved_config.test.bbox_vote_thresh == 0.8
    saved_config.test.bbox_vote = False
    parse_args('t', ['--bbox_vote', '--bbox_vote_thresh', '0.65'])
    assert saved_config.test.bbox_vote is True and saved_config.test.bbox_vote_thresh == 0.65
    saved_config.test.bbox_vote = False
    with pytest.raises(SystemExit):
        parse_args('t', ['--bbox_vote_thresh', '0.65'])                  # the threshold of a vote that is off


def test_yaml_keys_set_the_config(tmp_path, saved_config):
    from upsnet_amd.config.parse_args import parse_args
    cfg = write_cfg(tmp_path, 'Cityscapes', str(tmp_path / 'data'), 'val', extra='  bbox_vote: true\n  bbox_vote_thresh: 0.7\n')
    parse_args('t', ['--cfg', cfg])
    assert saved_config.test.bbox_vote is True and saved_config.test.bbox_vote_thresh == 0.7
    parse_args('t', ['--cfg', cfg, '--bbox_vote_thresh', '0.6'])        # the yaml switched voting on
    assert saved_config.test.bbox_vote_thresh == 0.6


def test_eval_proposals_is_refused_with_box_voting(tmp_path, saved_config):
    from upsnet_amd.evaluate import main
    cfg = write_cfg(tmp_path, 'Cityscapes', str(tmp_path / 'data'), 'val')
    with pytest.raises(SystemExit) as e:
        main(['--cfg', cfg, '--synthetic_weights', '--bbox_vote', '--eval_proposals'])
    assert '--eval_proposals' in str(e.value) and '--bbox_vote' in str(e.value)
    saved_config.test.bbox_vote = False
    with pytest.raises(SystemExit) as e:
        main(['--cfg', cfg, '--synthetic_weights', '--bbox_vote', '--bbox_vote_thresh', '0'])
    assert 'bbox_vote_thresh' in str(e.value)


def test_forward_tta_refuses_keep_proposals_with_voting_alone(saved_config):
    from upsnet_amd.tta import forward_tta

    class Model:
        keep_proposals = True
    saved_config.test.bbox_vote = True
    with pytest.raises(ValueError, match='proposal'):
        forward_tta(Model(), np.zeros((8, 8, 3), np.uint8))


# ------------------------------------------------------------------------------------------------ C entry point
def test_entry_point_refuses_bad_arguments_without_a_gpu():
    from upsnet_amd import _lib
    lib = _lib.lib()
    one = ctypes.c_void_p(64)
    w = (ctypes.c_float * 4)(10.0, 10.0, 5.0, 5.0)
    err = lambda: lib.upsnet_last_error()

    def call(rois=one, delta=one, prob=one, N=100, ndev=one, C=9, im=one, clip=1, weights=w, st=0.05, it=0.8, boxes=one, cls=one,
             num=one, cap=16, voted=one):
        return lib.upsnet_box_vote(None, rois, delta, prob, N, ndev, C, im, clip, weights, st, it, boxes, cls, num, cap, voted)
    for name in ('rois', 'delta', 'prob', 'im', 'weights', 'boxes', 'cls', 'num', 'voted'):
        assert call(**{name: None}) != 0 and b"null pointer" in err(), name
    for N in (0, -1):
        assert call(N=N) != 0 and b"rois" in err()
    for C in (1, 0, -3):
        assert call(C=C) != 0 and b"classes" in err()
    assert call(cap=-1) != 0 and b"capacity" in err()
    for it in (0.0, -0.5, float('nan')):
        assert call(it=it) != 0 and b"IoU threshold" in err()
    # nothing to do: no launch, success (the row pointers may be NULL, the device row count is optional)
    assert call(cap=0, boxes=None, cls=None, voted=None, ndev=None) == 0
    assert call(cap=0, rois=None) != 0 and b"null pointer" in err()
