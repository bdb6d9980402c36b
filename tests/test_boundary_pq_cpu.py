"""CPU: the Boundary PQ rule (tests/boundary_pq_ref.py) pinned by the per-segment mask_to_boundary of tests/boundary_ref.py, by the
hand-derived case and by its relations to mask PQ (test_pq_cpu.pq_restated); the host-side refusals of the device path
(PanopticEvaluator(boundary=True), dataset.boundary.panoptic_boundary, the evaluate command line, the C entry points)."""
import ctypes
import math
from fractions import Fraction

import numpy as np
import pytest

from conftest import ROOT  # noqa: F401  (puts the repo root on sys.path)
import boundary_ref
import boundary_pq_ref as ref
from test_dataset_run_cpu import make_dataset, saved_config, write_cfg  # noqa: F401  (saved_config is a fixture)
from test_pq_cpu import pq_restated, rgb_to_id
from test_pq_gpu import id_rgb, scene


def grid_labels(rng, H, W, gh, gw):
    """A gh x gw grid of segments, some of them merged into one label, plus a few single-pixel specks."""
    ids = rng.integers(1, max(2, gh * gw - 1), (gh, gw))
    lab = np.repeat(np.repeat(ids, -(-H // gh), 0), -(-W // gw), 1)[:H, :W].copy()
    for _ in range(3):
        lab[rng.integers(0, H), rng.integers(0, W)] = 0
    return lab


def assert_per_segment(lab, d, ratio):
    H, W = lab.shape
    assert boundary_ref.dilation(H, W, ratio) == d
    got = ref.label_boundary(lab, d)
    for s in np.unique(lab):
        assert np.array_equal(got & (lab == s), boundary_ref.mask_to_boundary(lab == s, ratio)), (H, W, d, int(s))
    return got


# ------------------------------------------------------------------------------------------------------------------ the rule
@pytest.mark.parametrize('H,W', [(1, 1), (7, 9), (40, 60), (33, 65), (64, 48), (20, 20)])
def test_label_boundary_is_mask_to_boundary_of_every_segment(H, W):
    rng = np.random.default_rng(H * 100 + W)
    for d in range(1, 9):
        ratio = d / math.sqrt(H ** 2 + W ** 2)
        for gh, gw in ((1, 1), (2, 3), (3, 2)):
            assert_per_segment(grid_labels(rng, H, W, min(gh, H), min(gw, W)), d, ratio)


def test_label_boundary_wide_windows():
    rng = np.random.default_rng(7)
    lab = grid_labels(rng, 96, 160, 1, 2)
    assert boundary_ref.dilation(96, 160, 0.4) == 75                    # d >= 64; 2d+1 = 151 exceeds the height only
    assert assert_per_segment(lab, 75, 0.4).all()
    d = 64
    assert not assert_per_segment(np.zeros((200, 200), np.int64), d, d / math.sqrt(2 * 200 ** 2)).all()   # d >= 64 with an interior
    lab = grid_labels(rng, 40, 9, 1, 1)                                  # 2d+1 = 11 exceeds only the width
    assert assert_per_segment(lab, 5, 5 / math.sqrt(40 ** 2 + 9 ** 2)).all()
    lab = grid_labels(rng, 9, 40, 1, 1)                                  # ... and only the height
    assert assert_per_segment(lab, 5, 5 / math.sqrt(40 ** 2 + 9 ** 2)).all()


def test_pred_void_is_one_label_and_gt_ids_use_24_bits():
    pred = np.zeros((9, 9, 3), np.uint8)
    pred[..., 0] = 255
    pred[..., 1] = np.arange(81).reshape(9, 9)                           # VOID pixels with differing instance bytes
    pred[..., 2] = 7
    assert not ref.boundary_bits(pred_2ch=pred, d=1)[1:-1, 1:-1].any()
    for byte in (1, 2):                                                  # ids that differ only in the G / only in the B byte
        gt = np.zeros((9, 9, 3), np.uint8)
        gt[..., 0] = 5
        gt[:, 4:, byte] = 1
        bits = ref.boundary_bits(gt_rgb=gt, d=1)
        assert bits[1:-1, 3:5].all() and not bits[1:-1, 1:3].any() and not bits[1:-1, 5:8].any()


def test_hand_derived_case():
    """40 x 60, d = 1: mask PQ has both TP (7/8 and 22/23); the boundary rule turns cat 1 into FN + FP (iou_b = 7/17) and scores cat 2
    with 32/43."""
    from upsnet_amd.dataset.base_dataset import PQStat
    pred, gt, info = ref.hand_case()
    assert boundary_ref.dilation(40, 60) == 1
    tp, fp, fn, iou = pq_restated([(pred, gt, info)], ref.HAND_CATS)
    assert (tp[1], fp[1], fn[1], tp[2], fp[2], fn[2]) == (1, 0, 0, 1, 0, 0)
    assert iou[1] == 7 / 8 and iou[2] == 1760 / 1840 and Fraction(1760, 1840) == Fraction(22, 23)
    c = ref.boundary_counts(pred, gt, 1)
    k1, k2 = 1 * 256, 2 * 256
    assert (c['area_bp'][k1], c['area_bg'][1], c['inter_b'][1 * 65536 + k1]) == (96, 96, 56)
    assert Fraction(56, 96 + 96 - 56) == Fraction(7, 17) < Fraction(1, 2)
    assert (c['area_bp'][k2], c['area_bg'][2], c['inter_b'][2 * 65536 + k2]) == (300, 300, 256)
    assert Fraction(256, 300 + 300 - 256) == Fraction(32, 43) < Fraction(22, 23)
    assert not c['void_b']
    tp, fp, fn, iou = ref.boundary_pq_restated([(pred, gt, info)], ref.HAND_CATS)
    assert (tp[1], fp[1], fn[1], tp[2], fp[2], fn[2]) == (0, 1, 1, 1, 0, 0) and tp.sum() + fp.sum() + fn.sum() == 3
    assert iou[1] == 0.0 and iou[2] == 256 / 344 == 32 / 43
    stat = PQStat()
    for cat in (1, 2):
        s = stat[cat]
        s.tp, s.fp, s.fn, s.iou = int(tp[cat]), int(fp[cat]), int(fn[cat]), float(iou[cat])
    res = {name: stat.pq_average(ref.HAND_CATS, isthing=t)[0]['pq'] for name, t in (('All', None), ('Things', True), ('Stuff', False))}
    assert res == {'All': 16 / 43, 'Things': 0.0, 'Stuff': 32 / 43}


def test_perfect_prediction_scores_one():
    from upsnet_amd.dataset.base_dataset import PQStat
    rng = np.random.default_rng(3)
    pred, _, _ = scene(rng, 96, 160, 3, 4, void=0.0)
    key = ref.pred_labels(pred)
    gid = key + 1
    info = [{'id': int(g), 'category_id': int((g - 1) >> 8), 'iscrowd': 0, 'area': int((gid == g).sum())} for g in np.unique(gid)]
    tp, fp, fn, iou = ref.boundary_pq_restated([(pred, id_rgb(gid), info)], ref.CATS)
    assert fp.sum() == 0 and fn.sum() == 0 and tp.sum() == len(info) and np.array_equal(iou, tp.astype(np.float64))
    stat = PQStat()
    for c in np.nonzero(tp)[0]:
        s = stat[int(c)]
        s.tp, s.iou = int(tp[c]), float(iou[c])
    res, per_class = stat.pq_average(ref.CATS, isthing=None)
    assert (res['pq'], res['sq'], res['rq']) == (1.0, 1.0, 1.0)
    assert all((r['pq'], r['sq'], r['rq']) == (1.0, 1.0, 1.0) for r in per_class.values() if r.get('tp'))


# ------------------------------------------------------------------------------------------------------------------ relations to mask PQ
@pytest.mark.parametrize('name', ['small0', 'small1', 'odd'])
def test_window_larger_than_the_image_is_mask_pq(name):
    """Consistent JSON areas and 2d+1 > min(H, W): every pixel is boundary, the boundary union is never larger than the mask union
    (area_bg counts only the pixels whose pred is valid, the JSON area all of them), so min() keeps iou_m bit for bit."""
    images = ref.scene_images(name)
    H, W = images[0][0].shape[:2]
    assert 2 * boundary_ref.dilation(H, W, 0.5) + 1 > min(H, W)
    got, want = ref.boundary_pq_restated(images, ref.CATS, 0.5), pq_restated(images, ref.CATS)
    for g, w in zip(got[:3], want[:3]):
        assert np.array_equal(g, w)
    assert np.array_equal(got[3].view(np.int64), want[3].view(np.int64)) and want[0].sum() > 0


@pytest.mark.parametrize('name', sorted(ref.SCENES))
def test_boundary_pq_never_matches_more_and_differs(name):
    images = ref.scene_images(name)
    tp_b, fp_b, fn_b, iou_b = ref.scene_restated(name)
    tp, fp, fn, iou = pq_restated(images, ref.CATS)
    assert (tp_b <= tp).all() and np.array_equal(tp_b + fn_b, tp + fn) and (tp_b + fp_b >= tp + fp).all()
    assert tp.sum() > 0
    # conditions on the inputs: the boundary rule shows on this scene, which has VOID in both maps
    assert not np.array_equal(iou_b.view(np.int64), iou.view(np.int64))
    assert (rgb_to_id(images[0][1]) == 0).any() and (images[0][0][..., 0] == 255).any()
    if name in ('small0', 'small_jitter', 'mid_jitter', 'full'):         # ... keeps some matches and loses others, next to a crowd GT
        assert 0 < tp_b.sum() < tp.sum() and fp.sum() > 0 and any(el['iscrowd'] for el in images[0][2])
        assert len({el['id'] for el in images[0][2]}) < len(np.unique(rgb_to_id(images[0][1]))) - 1     # ids missing from the JSON


# ------------------------------------------------------------------------------------------------------------------ refusals
def test_evaluator_refusals_before_any_launch():
    from upsnet_amd.dataset.pq import PanopticEvaluator
    for bad in (0, -1.0, float('nan'), float('inf')):
        with pytest.raises(ValueError, match='dilation_ratio'):
            PanopticEvaluator(ref.CATS, boundary=True, dilation_ratio=bad)
    a, b = PanopticEvaluator(ref.CATS, boundary=True), PanopticEvaluator(ref.CATS, boundary=True, dilation_ratio=0.05)
    assert a.boundary and a.dilation_ratio == 0.02 and b.dilation_ratio == 0.05
    with pytest.raises(ValueError, match='dilation_ratio'):
        a += b
    plain = PanopticEvaluator(ref.CATS)
    assert not plain.boundary and plain.dilation_ratio is None
    with pytest.raises(ValueError, match='boundary'):
        a += plain
    with pytest.raises(ValueError, match='boundary'):
        plain += a
    a += PanopticEvaluator(ref.CATS, boundary=True, dilation_ratio=0.02)    # equal rules merge (nothing was added: no device)
    assert a._state is None and a.num_images == 0
    pred, gt, info = ref.hand_case()
    with pytest.raises(ValueError, match='differ in shape'):
        a.add(pred, gt[:, :-1], info)
    assert a._state is None


def test_panoptic_boundary_refusals_before_any_launch():
    import torch
    from upsnet_amd.dataset.boundary import panoptic_boundary
    z = torch.zeros((4, 4, 3), dtype=torch.uint8)
    with pytest.raises(ValueError, match='device tensors'):
        panoptic_boundary(z, z)
    with pytest.raises(ValueError, match='neither'):
        panoptic_boundary()
    with pytest.raises(ValueError, match=r'uint8 \[H,W,3\]'):
        panoptic_boundary(gt_rgb=torch.zeros((4, 4), dtype=torch.uint8))
    with pytest.raises(ValueError, match=r'uint8 \[H,W,3\]'):
        panoptic_boundary(pred_2ch=np.zeros((4, 4, 3), np.uint8))
    for bad in (0, -1.0, float('nan'), float('inf')):
        with pytest.raises(ValueError, match='dilation_ratio'):
            panoptic_boundary(z, z, ratio=bad)


def test_command_line_refusals(tmp_path, saved_config):     # noqa: F811
    from upsnet_amd.evaluate import main
    root = str(tmp_path / 'cs')
    make_dataset(root, 'Cityscapes', [(8, 12)], seed=1)
    cfg = write_cfg(tmp_path, 'Cityscapes', root, 'val')
    with pytest.raises(SystemExit, match='--boundary_pq_dilation_ratio sets the boundary width of --eval_boundary_pq'):
        main(['--cfg', cfg, '--eval_only', '--boundary_pq_dilation_ratio', '0.05'])
    with pytest.raises(SystemExit, match='--boundary_pq_dilation_ratio sets the boundary width of --eval_boundary_pq'):
        main(['--cfg', cfg, '--eval_only', '--eval_boundary', '--boundary_pq_dilation_ratio', '0.05'])
    for bad in ('0', '-0.1', 'nan', 'inf'):
        with pytest.raises(SystemExit, match='boundary_pq_dilation_ratio.*dilation_ratio'):
            main(['--cfg', cfg, '--eval_only', '--eval_boundary_pq', '--boundary_pq_dilation_ratio', bad])
    p = tmp_path / 'no_head.yaml'
    p.write_text(open(cfg).read().replace('network:\n', 'network:\n  has_panoptic_head: false\n'))
    with pytest.raises(SystemExit) as e:
        main(['--cfg', str(p), '--eval_only', '--eval_boundary_pq'])
    assert '--eval_boundary_pq' in str(e.value) and 'has_panoptic_head' in str(e.value) and '--pan_combined' in str(e.value)
    with pytest.raises(SystemExit, match='no results to evaluate'):      # accepted with --pan_combined: the run gets to the missing pickle
        main(['--cfg', str(p), '--eval_only', '--eval_boundary_pq', '--pan_combined'])


def test_entry_points_validate_on_the_host():
    from upsnet_amd import _lib
    lib = _lib.lib()
    one = ctypes.c_void_p(16)
    assert lib.upsnet_pq_boundary_workspace_bytes(4097, 8, 8) == 0 and lib.upsnet_pq_boundary_workspace_bytes(-1, 8, 8) == 0
    assert lib.upsnet_pq_boundary_workspace_bytes(16, 0, 8) == 0 and lib.upsnet_pq_boundary_workspace_bytes(16, 8, -1) == 0
    assert lib.upsnet_pq_boundary_workspace_bytes(16, 1 << 16, 1 << 15) == 0
    small, large = lib.upsnet_pq_boundary_workspace_bytes(100, 8, 8), lib.upsnet_pq_boundary_workspace_bytes(100, 1024, 2048)
    assert small > lib.upsnet_pq_workspace_bytes(100) + (2 * 65536 + 100 * 256 + 100) * 4 + 2 * 64
    assert large - small >= 2 * (1024 * 2048 - 64)
    assert lib.upsnet_pan_boundary_workspace_bytes(0, 4) == 0 and lib.upsnet_pan_boundary_workspace_bytes(37, 53) >= 37 * 53

    def acc(dilation=1, pred=one, gt=one, H=4, W=4, segs=None, n=0, known=one, index=0, max_gt=16, ws=one, tp=one, status=one):
        return lib.upsnet_pq_boundary_accumulate(None, dilation, pred, gt, H, W, segs, n, known, index, max_gt, ws, tp, one, one, one, status)
    for kw in (dict(pred=None), dict(gt=None), dict(known=None), dict(ws=None), dict(tp=None), dict(status=None), dict(n=1)):
        assert acc(**kw) != 0 and b"null pointer" in lib.upsnet_last_error(), kw
    for kw in (dict(H=0), dict(W=-3), dict(H=1 << 16, W=1 << 15)):
        assert acc(**kw) != 0 and b"bad image size" in lib.upsnet_last_error(), kw
    for d in (0, -1):
        assert acc(dilation=d) != 0 and b"dilation" in lib.upsnet_last_error()
    assert acc(segs=one, n=17) != 0 and b"17 GT segments" in lib.upsnet_last_error()
    assert acc(max_gt=4097) != 0 and b"max_gt" in lib.upsnet_last_error()
    assert acc(ws=ctypes.c_void_p(8)) != 0 and b"aligned" in lib.upsnet_last_error()

    def bmap(dilation=1, pred=one, gt=one, H=4, W=4, ws=one, out=one):
        return lib.upsnet_pan_boundary_map(None, dilation, pred, gt, H, W, ws, out)
    for kw in (dict(ws=None), dict(out=None)):
        assert bmap(**kw) != 0 and b"null pointer" in lib.upsnet_last_error(), kw
    assert bmap(pred=None, gt=None) != 0 and b"null pointer" in lib.upsnet_last_error()
    assert bmap(H=0) != 0 and b"bad image size" in lib.upsnet_last_error()
    assert bmap(dilation=0) != 0 and b"dilation" in lib.upsnet_last_error()


def test_ops_refuse_before_any_launch():
    import torch
    from upsnet_amd import ops
    z8 = torch.zeros((4, 4, 3), dtype=torch.uint8)
    with pytest.raises(Exception, match="not implemented"):   # require_cuda, as the reference's Functions
        ops.pq_boundary_accumulate(1, z8, z8, torch.zeros((0, 4), dtype=torch.int64), torch.zeros(256, dtype=torch.uint8), 0, 16,
                                   torch.zeros(16, dtype=torch.uint8), *(torch.zeros(256, dtype=torch.int64) for _ in range(3)),
                                   torch.zeros(256, dtype=torch.float64), torch.zeros(1, dtype=torch.int64))
    buf = torch.zeros(16, dtype=torch.uint8)
    with pytest.raises(Exception, match="not implemented"):
        ops.pan_boundary_map(1, z8, z8, buf, torch.zeros((4, 4), dtype=torch.uint8))
    with pytest.raises(ValueError, match="neither"):
        ops.pan_boundary_map(1, None, None, buf, buf)
    with pytest.raises(ValueError, match="out of range"):
        ops.pan_boundary_workspace_bytes(0, 4)
    assert ops.pan_boundary_workspace_bytes(37, 53) >= 37 * 53
    with pytest.raises(ValueError, match="outside 0..4096"):
        ops.pq_boundary_workspace(5000, 8, 8, 'cpu')
