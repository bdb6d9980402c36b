"""CPU: the Boundary IoU rule (tests/boundary_ref.py: mask_to_boundary in closed form, min(mask IoU, boundary IoU) inside the restated
COCOeval) pinned by the iterated 3x3 erosion it abbreviates and by hand-derived cases; the host-side pieces of the device path
(boundary_dilation, the refusals of DetectionEvaluator and of the evaluate command line)."""
import math

import numpy as np
import pytest

from conftest import ROOT  # noqa: F401  (puts the repo root on sys.path)
import boundary_ref
import test_coco_eval_cpu
from test_dataset_run_cpu import make_dataset, saved_config, write_cfg  # noqa: F401  (saved_config is a fixture)

DILATIONS = [((1024, 2048), 46), ((800, 1333), 31), ((480, 640), 16), ((130, 70), 3), ((96, 160), 4), ((64, 64), 2), ((40, 60), 1),
             ((1, 1), 1)]


def rect(H, W, y0, y1, x0, x1):
    m = np.zeros((H, W), bool)
    m[y0:y1, x0:x1] = True
    return m


# ------------------------------------------------------------------------------------------------------------------ the rule
def test_boundary_dilation_table():
    from upsnet_amd.dataset.boundary import boundary_dilation
    for (h, w), d in DILATIONS:
        assert boundary_dilation(h, w) == d == boundary_ref.dilation(h, w), (h, w)
    assert boundary_dilation(130, 70, 0.5) == 74
    assert boundary_dilation(300, 200, 0.2) == 72
    assert boundary_dilation(40, 60, 1e-6) == 1 and boundary_dilation(1, 1, 0.02) == 1      # the floor
    assert boundary_dilation(3, 4, 0.5) == 2 and boundary_dilation(3, 4, 1.5) == 8          # 2.5 and 7.5: halves go to even
    for bad in (0, -0.02, float('nan'), float('inf')):
        with pytest.raises(ValueError, match='dilation_ratio'):
            boundary_dilation(40, 60, bad)


@pytest.mark.parametrize('H,W,ratio', boundary_ref.SIZES + [boundary_ref.FULL_SIZE])
def test_closed_form_is_the_iterated_erosion(H, W, ratio):
    d = boundary_ref.dilation(H, W, ratio)
    cases = boundary_ref.mask_cases(H, W, d, seed=H * 10007 + W)
    if H * W > 1 << 20:
        cases = [c for c in cases if c[0] in ('ones', 'holes', 'blobs1')]
    for name, m in cases:
        it = boundary_ref.erode_iterated(m, d)
        assert np.array_equal(boundary_ref.erode_closed_form(m, d), it), (name, H, W, d)
        assert np.array_equal(boundary_ref.mask_to_boundary(m, ratio), m & ~it), (name, H, W, d)      # the bounding-box shortcut


def test_hand_derived_boundaries():
    b = boundary_ref.mask_to_boundary
    g = rect(40, 60, 10, 30, 10, 40)
    assert boundary_ref.dilation(40, 60) == 1 and int(b(g).sum()) == 96 == 20 * 30 - 18 * 28        # a ring one pixel wide
    assert int(b(rect(40, 60, 0, 10, 0, 10)).sum()) == 36 == 100 - 8 * 8         # the image corner: boundary along the image edges too
    assert boundary_ref.dilation(64, 64) == 2 and int(b(np.ones((64, 64), bool)).sum()) == 496 == 64 * 64 - 60 * 60
    thin = rect(64, 64, 20, 24, 5, 50)                                           # 4 rows at d = 2: no row is 2 away from both sides
    assert np.array_equal(b(thin), thin)
    assert np.array_equal(b(np.ones((1, 1), bool)), np.ones((1, 1), bool))


def test_hand_derived_boundary_iou():
    g, d = rect(40, 60, 10, 30, 10, 40), rect(40, 60, 10, 30, 12, 42)
    assert test_coco_eval_cpu.mask_iou([d], [g], [0])[0, 0] == 0.875 == 560 / 640
    bg, bd = boundary_ref.mask_to_boundary(g), boundary_ref.mask_to_boundary(d)
    assert int((bg & bd).sum()) == 56 and int((bg | bd).sum()) == 136
    assert boundary_ref.boundary_iou([d], [g], [0])[0, 0] == 56 / 136 == 7 / 17
    assert boundary_ref.boundary_iou([d], [g], [1])[0, 0] == 56 / 96            # a crowd GT: the det boundary's own area as the union
    far = rect(40, 60, 32, 38, 45, 55)
    assert boundary_ref.boundary_iou([far], [g], [0])[0, 0] == 0.0


def _pair():
    g, d = rect(40, 60, 10, 30, 10, 40), rect(40, 60, 10, 30, 12, 42)
    gts = [{'id': 1, 'category_id': 1, 'iscrowd': 0, 'area': 600.0, 'bbox': [10.0, 10.0, 30.0, 20.0], 'mask': g}]
    dts = [{'category_id': 1, 'score': 0.9, 'mask': d}]
    return [(1, gts, dts)]


def test_shifted_det_scores_08_on_masks_and_0_on_boundaries(monkeypatch):
    images = _pair()
    segm = test_coco_eval_cpu.cocoeval_restated(images, [1], 'segm')
    assert abs(segm[3][0] - 0.8) < 1e-12                                         # matched at 0.50 .. 0.85, 8 of 10 thresholds
    assert np.all(segm[1][:8, 0, 0, 2] == 1) and np.all(segm[1][8:, 0, 0, 2] == 0)
    monkeypatch.setattr(test_coco_eval_cpu, 'mask_iou', boundary_ref.boundary_iou)
    bnd = test_coco_eval_cpu.cocoeval_restated(images, [1], 'segm')
    assert bnd[3][0] == 0.0 and np.all(bnd[1][:, 0, 0, 2] == 0)                  # 7/17 < 0.5: unmatched at every threshold
    monkeypatch.undo()
    again = boundary_ref.boundary_cocoeval(images, [1])
    for a, b in zip(bnd, again):
        assert np.array_equal(a, b)
    assert test_coco_eval_cpu.mask_iou is boundary_ref._MASK_IOU


# ------------------------------------------------------------------------------------------------------------------ refusals
def test_evaluator_refusals_before_any_launch():
    from upsnet_amd.dataset.coco_eval import DetectionEvaluator
    for bad in (0, -1.0, float('nan'), float('inf')):
        with pytest.raises(ValueError, match='dilation_ratio'):
            DetectionEvaluator([1], 'boundary', dilation_ratio=bad)
    for other in ('keypoints', 'Boundary', ''):
        with pytest.raises(ValueError, match='iou_type'):
            DetectionEvaluator([1], other)
    a, b = DetectionEvaluator([1], 'boundary'), DetectionEvaluator([1], 'boundary', dilation_ratio=0.05)
    assert a.iou_type == 'boundary' and a.segm and a.dilation_ratio == 0.02
    with pytest.raises(ValueError, match='dilation_ratio'):
        a += b
    with pytest.raises(ValueError, match='iou_type'):
        a += DetectionEvaluator([1], 'segm')
    a += DetectionEvaluator([1], 'boundary', dilation_ratio=0.02)                # equal ratios merge (nothing was added: no device)
    with pytest.raises(ValueError, match='det_masks'):
        a.add(1, [], np.zeros((0, 4), np.float32), np.zeros(0, np.float32), np.zeros(0, np.int64), image_size=(8, 8))
    with pytest.raises(ValueError, match='image_size'):
        a.add(1, [], np.zeros((0, 4), np.float32), np.zeros(0, np.float32), np.zeros(0, np.int64), np.zeros((0, 1, 28, 28), np.float32))
    assert DetectionEvaluator([1], 'segm').dilation_ratio is None                # the ratio belongs to 'boundary' alone


def test_mask_to_boundary_refusals_before_any_launch():
    import torch
    from upsnet_amd.dataset.boundary import mask_to_boundary
    with pytest.raises(ValueError, match='device tensor'):
        mask_to_boundary(torch.zeros((1, 4, 4), dtype=torch.uint8))
    with pytest.raises(ValueError, match='uint8 / bool'):
        mask_to_boundary(torch.zeros((1, 4, 4)))
    with pytest.raises(ValueError, match='dilation_ratio'):
        mask_to_boundary(torch.zeros((1, 4, 4), dtype=torch.uint8), dilation_ratio=math.nan)
    with pytest.raises(ValueError, match='size'):
        mask_to_boundary([])
    with pytest.raises(ValueError, match='differs'):
        mask_to_boundary([{'size': [2, 2], 'counts': [4]}, {'size': [2, 3], 'counts': [6]}])


def test_command_line_refusals(tmp_path, saved_config):     # noqa: F811
    from upsnet_amd.evaluate import main
    root = str(tmp_path / 'cs')
    make_dataset(root, 'Cityscapes', [(8, 12)], seed=1)
    cfg = write_cfg(tmp_path, 'Cityscapes', root, 'val')
    with pytest.raises(SystemExit, match='--boundary_dilation_ratio sets the boundary width of --eval_boundary'):
        main(['--cfg', cfg, '--eval_only', '--boundary_dilation_ratio', '0.05'])
    for bad in ('0', '-0.1', 'nan', 'inf'):
        with pytest.raises(SystemExit, match='dilation_ratio'):
            main(['--cfg', cfg, '--eval_only', '--eval_boundary', '--boundary_dilation_ratio', bad])
    text = open(cfg).read()
    for k, extra in enumerate(('network:\n  has_mask_head: false\n', 'network:\n  has_rcnn: false\n')):
        p = tmp_path / ('no_head%d.yaml' % k)
        p.write_text(text.replace('network:\n', extra))
        with pytest.raises(SystemExit) as e:
            main(['--cfg', str(p), '--eval_only', '--eval_boundary'])
        assert '--eval_boundary' in str(e.value) and 'has_mask_head' in str(e.value) and 'has_rcnn' in str(e.value)
