"""CPU: the merge rule of test-time augmentation. The numpy float32 restatement (tests/tta_ref.py) against its
hand-derived properties and against the same formula in float64; the box mapping's identities; augmentation_list; the command line;
the C entry points' argument refusals (no launch without a GPU)."""
import copy
import ctypes

import numpy as np
import pytest

from conftest import ROOT  # noqa: F401  (puts the repo root on sys.path)

import tta_ref
from test_dataset_run_cpu import write_cfg

F = np.float32


@pytest.fixture()
def saved_config():
    from upsnet_amd.config.config import config
    saved = copy.deepcopy(dict(config))
    yield config
    config.clear()
    config.update(saved)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ------------------------------------------------------------------------------------------------ semantic merge
@pytest.mark.parametrize('cell', [4, 1])
@pytest.mark.parametrize('shape', [(1, 1, 1), (5, 7, 3), (8, 16, 19), (6, 10, 20)])
def test_one_augmentation_is_the_identity(shape, cell):
    rng = np.random.default_rng(shape[0] * 100 + shape[2])
    m = rng.normal(0, 4, shape).astype(F)
    out = tta_ref.seg_merge([m], [F(1)], [F(cell * shape[1])], [False], cell)
    assert same_bits(out, m)


@pytest.mark.parametrize('cell', [4, 1])
@pytest.mark.parametrize('shape', [(1, 1, 1), (5, 7, 3), (8, 16, 19), (6, 10, 20)])
def test_map_and_its_mirror_average_to_the_map(shape, cell):
    """The map and its left-right mirror as the flipped augmentation of the same scale, Wr = cell * Ws: (m + m) / 2 == m exactly."""
    rng = np.random.default_rng(shape[1] * 100 + shape[2])
    m = rng.normal(0, 4, shape).astype(F)
    wr = F(cell * shape[1])
    out = tta_ref.seg_merge([m, np.ascontiguousarray(m[:, ::-1])], [F(1), F(1)], [wr, wr], [False, True], cell)
    assert same_bits(out, m)


def test_flip_with_a_width_that_is_no_multiple_of_the_cell_hand_derived():
    """One row, cell 4, Wr = 10 (2.5 cells): base column x reads the flipped map at u = (2.5 - (x + 0.5)) - 0.5 = 1.5 - x, clamped to
    [0, Ws - 1]: x = 0 -> 1.5 (half way between columns 1 and 2), x = 1 -> 0.5, x = 2 -> 0 (clamped from -0.5)."""
    m = np.array([[[0.0], [8.0], [32.0]]], F)           # [1, 3, 1]
    s = tta_ref.seg_sample(m, 1, 3, F(1), F(10), True, 4)
    assert s[0, :, 0].tolist() == [20.0, 4.0, 0.0]


def test_scaled_sample_hand_derived():
    """q = 0.5 (an augmentation at half the base scale), 1 x 2 map [10, 30], base grid 1 x 4: u = (x + 0.5) / 2 - 0.5 =
    -0.25 (clamped to 0), 0.25, 0.75, 1.25 (clamped to 1)."""
    m = np.array([[[10.0], [30.0]]], F)
    s = tta_ref.seg_sample(m, 1, 4, F(0.5), F(8), False, 4)
    assert s[0, :, 0].tolist() == [10.0, 15.0, 25.0, 30.0]


def test_restatement_against_float64():
    """float32 against the same formula in float64 (the same float32 q and Wr). Bound: max|v| * (2^-19 * max(Hs, Ws) + 8 A 2^-24):
    a sampling coordinate of magnitude <= max(Hs, Ws) carries a few float32 round-offs (product, two differences: < 4 * 2^-24 * max),
    a coordinate error e moves a bilinear sample by at most 2 e max|v| per axis (so 2 axes: 2^-19 max(Hs, Ws) max|v| in all), the
    blend adds 6 round-offs of values <= max|v| and the A-term sum and the division A + 1 more per term."""
    rng = np.random.default_rng(418)
    worst = 0.0
    for case in range(300):
        A = int(rng.integers(1, 9))
        cell = int(rng.choice([1, 4]))
        S = int(rng.choice([1, 3, 19]))
        Hb, Wb = int(rng.integers(1, 40)), int(rng.integers(1, 60))
        scales = [1.0] + list(rng.uniform(0.5, 2.0, A - 1))
        q, _ = tta_ref.ratios(scales)
        maps, wr, flip = [], [], []
        for a in range(A):
            hs, ws = (Hb, Wb) if a == 0 else (max(1, int(round(Hb * float(q[a])))), max(1, int(round(Wb * float(q[a])))))
            maps.append(rng.normal(0, 10, (hs, ws, S)).astype(F))
            wr.append(F(cell * ws - int(rng.integers(0, cell))))
            flip.append(bool(rng.integers(0, 2)) and a > 0)
        got = tta_ref.seg_merge(maps, q, wr, flip, cell)
        want = tta_ref.seg_merge(maps, q, wr, flip, cell, dtype=np.float64)
        assert got.dtype == F and want.dtype == np.float64
        vmax = max(float(np.abs(m).max()) for m in maps)
        bound = vmax * (2.0 ** -19 * max(max(m.shape[:2]) for m in maps) + 8 * A * 2.0 ** -24)
        err = float(np.abs(got.astype(np.float64) - want).max())
        worst = max(worst, err / bound)
        assert err <= bound, (case, err, bound)
    print('restatement vs float64: worst error / bound = %.4f' % worst)


# ------------------------------------------------------------------------------------------------ boxes
def _boxes(rng, n, limit):
    x = np.sort(rng.uniform(0, limit, (n, 2)), 1)
    y = np.sort(rng.uniform(0, limit, (n, 2)), 1)
    return np.stack([np.zeros(n), x[:, 0], y[:, 0], x[:, 1], y[:, 1]], 1).astype(F)


def test_unit_ratio_without_flip_is_the_identity():
    rng = np.random.default_rng(1)
    rois = _boxes(rng, 1000, 2048)
    assert same_bits(tta_ref.roi_to_base(rois, F(1), F(2048), False), rois)
    assert same_bits(tta_ref.boxes_to_aug(rois, [F(1)], [F(2048)], [False])[0], rois)
    delta, prob = rng.normal(0, 1, (1000, 36)).astype(F), rng.uniform(0, 1, (1000, 9)).astype(F)
    r, d, p, n = tta_ref.roi_union([rois], [delta], [prob], [1000], [F(1)], [F(2048)], [False])
    assert n == 1000 and same_bits(r, rois) and same_bits(d, delta) and same_bits(p, prob)


@pytest.mark.parametrize('flip', [False, True])
def test_round_trip_base_to_augmentation_and_back(flip):
    """10 000 seeded boxes up to 2048 px, scales from 0.5 to 2: base -> augmentation -> base stays within 1e-3 px (each mapping is a
    product and a sum of float32 values below 4096: a few units of 2^-13 px)."""
    rng = np.random.default_rng(7 + flip)
    boxes = _boxes(rng, 10000, 2048)
    worst = 0.0
    for s in (0.5, 0.75, 192.0 / 256.0, 1.0, 1.25, 320.0 / 256.0, 2.0):
        q, r = tta_ref.ratios([1.0, s])
        wr = F(np.rint(2048 * s))
        there = tta_ref.boxes_to_aug(boxes, [q[1]], [wr], [flip])[0]
        back = tta_ref.roi_to_base(there, r[1], wr, flip)
        worst = max(worst, float(np.abs(back[:, 1:].astype(np.float64) - boxes[:, 1:]).max()))
    print('round trip: at most %.2e px' % worst)
    assert worst <= 1e-3


@pytest.mark.parametrize('flip', [False, True])
def test_decoding_commutes_with_the_mapping(flip):
    """bbox_transform on the mapped ROI row (dx negated when flipped) equals the mapped decoded box: the extent [x1, x2 + 1) is what is
    scaled, so the +1 width convention commutes. The ROI is mapped in float32 (the restatement), both decodes and the comparison's own
    mapping run in float64, so what remains is the float32 rounding of the mapped ROI: <= 2 round-offs of values below 4096 per
    corner (2.4e-4 px), which the decode with |dw|, |dh| <= 0.5 carries to at most 6.1e-4 px (centre 3.0e-4 + half extent 0.5 e^0.5
    3.7e-4); the flip adds one round-off of a value below 2048 (6e-5) to each x corner."""
    from upsnet_amd.bbox.bbox_transform import bbox_transform
    rng = np.random.default_rng(11 + flip)
    n = 10000
    wr_a = 2048.0
    rois = _boxes(rng, n, wr_a - 1)
    delta = rng.uniform(-0.5, 0.5, (n, 4))
    worst = 0.0
    for s in (0.5, 192.0 / 256.0, 1.0, 320.0 / 256.0, 2.0):
        _, r = tta_ref.ratios([1.0, s])
        r64 = float(r[1])
        mapped = tta_ref.roi_to_base(rois, r[1], F(wr_a), flip).astype(np.float64)
        d = delta.copy()
        if flip:
            d[:, 0] = -d[:, 0]
        got = bbox_transform(mapped[:, 1:], d)
        dec = bbox_transform(rois[:, 1:].astype(np.float64), delta)
        x1, y1, x2, y2 = dec.T
        if flip:
            x1, x2 = (wr_a - 1) - x2, (wr_a - 1) - x1
        want = np.stack([r64 * x1, r64 * y1, r64 * x2 + (r64 - 1), r64 * y2 + (r64 - 1)], 1)
        worst = max(worst, float(np.abs(got - want).max()))
    print('decode of the mapped ROI vs mapped decode: at most %.2e px' % worst)
    assert worst <= 1e-3


def test_union_packs_valid_rows_in_order_and_zeroes_the_rest():
    rng = np.random.default_rng(3)
    R, C = 8, 9
    rois = [_boxes(rng, R, 300) for _ in range(3)]
    delta = [rng.normal(0, 1, (R, 4 * C)).astype(F) for _ in range(3)]
    prob = [rng.uniform(0, 1, (R, C)).astype(F) for _ in range(3)]
    q, r = tta_ref.ratios([1.0, 1.0, 0.75])
    o_r, o_d, o_p, n = tta_ref.roi_union(rois, delta, prob, [2, 0, 3], r, [F(301), F(301), F(226)], [False, True, True])
    assert n == 5 and o_r.shape == (24, 5) and o_d.shape == (24, 36) and o_p.shape == (24, 9)
    assert same_bits(o_r[:2], rois[0][:2]) and same_bits(o_d[:2], delta[0][:2]) and same_bits(o_p[2:5], prob[2][:3])
    assert not o_r[5:].any() and not o_d[5:].any() and not o_p[5:].any()
    assert same_bits(o_d[2:5, 0::4], -delta[2][:3, 0::4]) and same_bits(o_d[2:5, 1::4], delta[2][:3, 1::4])
    # hand-derived: flipped at width 226 then scaled by r = 4/3: x1' = r * (225 - x2)
    x1 = r[2] * ((F(226) - F(1)) - rois[2][0, 3])
    assert o_r[2, 1] == x1 and o_r[2, 0] == 0


def test_mask_merge_mirrors_a_flipped_augmentation():
    rng = np.random.default_rng(5)
    L = rng.normal(0, 3, (4, 9, 28, 28)).astype(F)
    assert same_bits(tta_ref.mask_merge([L], [False]), L)
    assert same_bits(tta_ref.mask_merge([L, np.ascontiguousarray(L[..., ::-1])], [False, True]), L)
    three = tta_ref.mask_merge([L, L, L], [False, False, False])
    assert same_bits(three, ((L + L) + L) / F(3))


# ------------------------------------------------------------------------------------------------ augmentation list
def test_augmentation_list_order_and_max_sizes(saved_config):
    from upsnet_amd.tta import augmentation_enabled, augmentation_list
    cfg = saved_config
    cfg.test.scales, cfg.test.max_size, cfg.test.rpn_post_nms_top_n = [256], 512, 1000
    cfg.test.aug_scales, cfg.test.aug_flip = [], False
    assert not augmentation_enabled() and augmentation_list() == [(256, 512, False)]
    cfg.test.aug_flip = True
    assert augmentation_enabled() and augmentation_list() == [(256, 512, False), (256, 512, True)]
    cfg.test.aug_scales = [192, 320]
    assert augmentation_list() == [(256, 512, False), (256, 512, True), (192, 384, False), (192, 384, True), (320, 640, False),
                                   (320, 640, True)]
    cfg.test.aug_flip = False
    assert augmentation_enabled() and augmentation_list() == [(256, 512, False), (192, 384, False), (320, 640, False)]
    cfg.test.scales, cfg.test.max_size, cfg.test.aug_scales = [800], 1333, [600, 1000]
    assert augmentation_list() == [(800, 1333, False), (600, int(round(1333 * 600 / 800)), False), (1000, int(round(1333 * 1000 / 800)), False)]
    assert augmentation_list()[1][1] == 1000 and augmentation_list()[2][1] == 1666


def test_augmentation_list_refuses_too_many(saved_config):
    from upsnet_amd.tta import augmentation_list
    cfg = saved_config
    cfg.test.scales, cfg.test.max_size, cfg.test.rpn_post_nms_top_n = [256], 512, 100
    cfg.test.aug_scales, cfg.test.aug_flip = [192, 224, 288, 320], True       # 10 augmentations
    with pytest.raises(ValueError, match='at most 8'):
        augmentation_list()
    cfg.test.aug_scales = [192, 224, 288]                                       # 8: allowed
    assert len(augmentation_list()) == 8
    cfg.test.rpn_post_nms_top_n = 1025                                          # 8 x 1025 > 8192
    with pytest.raises(ValueError, match='8192'):
        augmentation_list()
    cfg.test.rpn_post_nms_top_n = 1024
    assert len(augmentation_list()) == 8


def test_forward_tta_refuses_keep_proposals(saved_config):
    from upsnet_amd.tta import forward_tta

    class Model:
        keep_proposals = True
    saved_config.test.aug_flip = True
    with pytest.raises(ValueError, match='proposal'):
        forward_tta(Model(), np.zeros((8, 8, 3), np.uint8))


# ------------------------------------------------------------------------------------------------ command line
def test_cli_options_set_the_config(saved_config):
    from upsnet_amd.config.parse_args import parse_args
    assert saved_config.test.aug_scales == [] and saved_config.test.aug_flip is False
    args = parse_args('t', ['--aug_scales', '192', '320', '--aug_flip'])
    assert args.aug_scales == [192, 320] and args.aug_flip
    assert saved_config.test.aug_scales == [192, 320] and saved_config.test.aug_flip is True
    saved_config.test.aug_scales, saved_config.test.aug_flip = [], False
    parse_args('t', [])
    assert saved_config.test.aug_scales == [] and saved_config.test.aug_flip is False


def test_yaml_keys_set_the_config(tmp_path, saved_config):
    from upsnet_amd.config.parse_args import parse_args
    cfg = write_cfg(tmp_path, 'Cityscapes', str(tmp_path / 'data'), 'val', extra='  aug_scales:\n  - 192\n  aug_flip: true\n')
    parse_args('t', ['--cfg', cfg])
    assert saved_config.test.aug_scales == [192] and saved_config.test.aug_flip is True


def test_eval_proposals_is_refused_with_augmentation(tmp_path, saved_config):
    from upsnet_amd.evaluate import main
    cfg = write_cfg(tmp_path, 'Cityscapes', str(tmp_path / 'data'), 'val')
    with pytest.raises(SystemExit) as e:
        main(['--cfg', cfg, '--synthetic_weights', '--aug_scales', '192', '--eval_proposals'])
    assert '--eval_proposals' in str(e.value) and 'no single proposal list' in str(e.value)
    saved_config.test.aug_scales = []
    with pytest.raises(SystemExit) as e:
        main(['--cfg', cfg, '--synthetic_weights', '--aug_flip', '--aug_scales', '192', '200', '208', '216'])   # 10 augmentations
    assert 'at most 8' in str(e.value)


# ------------------------------------------------------------------------------------------------ C entry points
def test_entry_points_refuse_bad_arguments_without_a_gpu():
    from upsnet_amd import _lib
    lib = _lib.lib()
    one = ctypes.c_void_p(64)
    ptrs = (ctypes.c_void_p * 9)(*([64] * 9))
    ints = (ctypes.c_int * 9)(*([4] * 9))
    flts = (ctypes.c_float * 9)(*([1.0] * 9))
    err = lambda: lib.upsnet_last_error()
    for A in (0, 9, -1):
        assert lib.upsnet_tta_seg_merge(None, A, ptrs, ints, ints, flts, flts, ints, 4, 19, 4, 4, one) != 0
        assert b"1..8 augmentations" in err()
        assert lib.upsnet_tta_roi_union(None, A, ptrs, ptrs, ptrs, ptrs, flts, flts, ints, 8, 36, 9, one, one, one, one) != 0
        assert b"1..8 augmentations" in err()
        assert lib.upsnet_tta_boxes_to_aug(None, A, flts, flts, ints, one, 4, one) != 0
        assert b"1..8 augmentations" in err()
        assert lib.upsnet_tta_mask_merge(None, A, ptrs, ints, 4, 9, 28, 0, one) != 0
        assert b"1..8 augmentations" in err()
    # null pointers
    assert lib.upsnet_tta_seg_merge(None, 2, ptrs, ints, ints, flts, flts, ints, 4, 19, 4, 4, None) != 0 and b"null pointer" in err()
    assert lib.upsnet_tta_seg_merge(None, 2, None, ints, ints, flts, flts, ints, 4, 19, 4, 4, one) != 0 and b"null pointer" in err()
    holed = (ctypes.c_void_p * 9)(64, None, 64, 64, 64, 64, 64, 64, 64)
    assert lib.upsnet_tta_seg_merge(None, 2, holed, ints, ints, flts, flts, ints, 4, 19, 4, 4, one) != 0 and b"null pointer" in err()
    assert lib.upsnet_tta_roi_union(None, 2, ptrs, holed, ptrs, ptrs, flts, flts, ints, 8, 36, 9, one, one, one, one) != 0
    assert b"null pointer" in err()
    assert lib.upsnet_tta_roi_union(None, 2, ptrs, ptrs, ptrs, ptrs, flts, flts, ints, 8, 36, 9, one, one, one, None) != 0
    assert b"null pointer" in err()
    assert lib.upsnet_tta_boxes_to_aug(None, 2, flts, flts, ints, None, 4, one) != 0 and b"null pointer" in err()
    assert lib.upsnet_tta_boxes_to_aug(None, 2, None, flts, ints, one, 4, one) != 0 and b"null pointer" in err()
    assert lib.upsnet_tta_mask_merge(None, 2, holed, ints, 4, 9, 28, 0, one) != 0 and b"null pointer" in err()
    assert lib.upsnet_tta_mask_merge(None, 2, ptrs, ints, 4, 9, 28, 0, None) != 0 and b"null pointer" in err()
    # sizes
    for S, H, W in ((0, 4, 4), (19, 0, 4), (19, 4, -1)):
        assert lib.upsnet_tta_seg_merge(None, 2, ptrs, ints, ints, flts, flts, ints, 4, S, H, W, one) != 0 and b"non-positive" in err()
    zeros = (ctypes.c_int * 9)(4, 0, 4, 4, 4, 4, 4, 4, 4)
    assert lib.upsnet_tta_seg_merge(None, 2, ptrs, ints, zeros, flts, flts, ints, 4, 19, 4, 4, one) != 0 and b"non-positive" in err()
    assert lib.upsnet_tta_seg_merge(None, 2, ptrs, ints, ints, flts, flts, ints, 2, 19, 4, 4, one) != 0 and b"cell" in err()
    for R, D, C in ((0, 36, 9), (8, 0, 9), (8, 36, 0)):
        assert lib.upsnet_tta_roi_union(None, 2, ptrs, ptrs, ptrs, ptrs, flts, flts, ints, R, D, C, one, one, one, one) != 0
        assert b"non-positive" in err()
    assert lib.upsnet_tta_roi_union(None, 2, ptrs, ptrs, ptrs, ptrs, flts, flts, ints, 8, 34, 9, one, one, one, one) != 0
    assert b"multiple of 4" in err()
    assert lib.upsnet_tta_roi_union(None, 8, ptrs, ptrs, ptrs, ptrs, flts, flts, ints, 1025, 36, 9, one, one, one, one) != 0
    assert b"8192" in err()
    assert lib.upsnet_tta_boxes_to_aug(None, 2, flts, flts, ints, one, -1, one) != 0 and b"box count" in err()
    assert lib.upsnet_tta_mask_merge(None, 2, ptrs, ints, 4, 0, 28, 0, one) != 0 and b"non-positive" in err()
    assert lib.upsnet_tta_mask_merge(None, 2, ptrs, ints, 4, 9, 0, 0, one) != 0 and b"non-positive" in err()
    assert lib.upsnet_tta_mask_merge(None, 2, ptrs, ints, -1, 9, 28, 0, one) != 0 and b"row count" in err()
    # nothing to do: no launch, success
    assert lib.upsnet_tta_boxes_to_aug(None, 2, flts, flts, ints, None, 0, None) == 0
    assert lib.upsnet_tta_mask_merge(None, 2, ptrs, ints, 0, 9, 28, 0, None) == 0
