"""GPU: Boundary PQ on the device (csrc/pq_boundary.hip via dataset/boundary.panoptic_boundary and PanopticEvaluator(boundary=True))
against the numpy restatement of tests/boundary_pq_ref.py (pinned on the CPU by tests/test_boundary_pq_cpu.py): the boundary bit maps
byte for byte under both poison patterns, counts exact and IoU sums bit-identical."""
import json
import math
import os
import pickle

import numpy as np
import pytest
import torch

import boundary_ref
import boundary_pq_ref as ref
import memguard
from test_dataset_run_cpu import make_dataset, saved_config, write_cfg  # noqa: F401  (saved_config is a fixture)
from test_pq_cpu import pq_restated, rgb_to_id
from test_pq_gpu import assert_same, id_rgb, raw, scene

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------------------------ the bit map
GUARDED = memguard.MODULES + ('upsnet_amd.dataset.boundary',)     # panoptic_boundary allocates its workspace and its output itself


def gt_from(lab, byte=0):
    """Labels as GT ids that differ only in one byte of the PNG colour (the other two bytes constant and non-zero)."""
    lab = np.asarray(lab, np.int64) & 255
    return id_rgb({0: lab + (3 << 8) + (2 << 16), 1: 5 + (lab << 8) + (2 << 16), 2: 5 + (3 << 8) + (lab << 16)}[byte])


def pred_from(lab, by='cat', void=None, rng=None):
    """Labels as pred keys that differ only in the category or only in the instance byte; `void` pixels get cat 255 and random other
    bytes (one VOID label whatever they hold)."""
    lab = np.asarray(lab, np.int64)
    pred = np.zeros(lab.shape + (3,), np.uint8)
    if by == 'cat':
        pred[..., 0], pred[..., 1] = lab % 250, 9
    else:
        pred[..., 0], pred[..., 1] = 4, lab & 255
    if void is not None:
        pred[void, 0] = 255
        pred[void, 1:] = rng.integers(0, 256, (int(void.sum()), 2))
    return pred


def label_maps(H, W, d, rng):
    """[(name, label map)]: uniform, a checkerboard of 1-pixel segments, bars of width 2d, 2d+1 and 2d+2 in both directions, a segment
    flush with each image edge, seeded blocks."""
    yy, xx = np.mgrid[0:H, 0:W]
    out = [('uniform', np.full((H, W), 7)), ('checker', (yy + xx) & 1)]
    for name, c in (('vbars', xx), ('hbars', yy)):
        widths = np.array([2 * d, 2 * d + 1, 2 * d + 2, 2 * d + 1, 2 * d])
        edges = np.cumsum(np.tile(widths, 1 + max(H, W) // int(widths.sum())))
        out.append((name, np.searchsorted(edges, c, side='right')))
    hh, ww = max(1, (2 * H) // 3), max(1, (2 * W) // 3)
    flush = np.zeros((H, W), np.int64)
    flush[:hh, :ww] = 1                      # top and left
    flush[H - max(1, H // 4):, W - ww:] = 2  # bottom and right
    out.append(('flush', flush))
    bh, bw = max(1, H // 3), max(1, W // 4)
    blocks = rng.integers(0, 5, (-(-H // bh), -(-W // bw)))
    lab = np.repeat(np.repeat(blocks, bh, 0), bw, 1)[:H, :W].copy()
    lab[rng.random((H, W)) < 0.002] = 6
    out.append(('blocks', lab))
    return out


def device_bits(pred, gt, ratio, pattern):
    from upsnet_amd.dataset.boundary import panoptic_boundary
    with memguard.poisoned(pattern, modules=GUARDED) as guard:
        p = memguard.banded_copy(torch.from_numpy(pred).cuda(), pattern) if pred is not None else None
        g = memguard.banded_copy(torch.from_numpy(gt).cuda(), pattern) if gt is not None else None
        out = panoptic_boundary(p, g, ratio)
        assert out.dtype == torch.uint8 and tuple(out.shape) == (pred if pred is not None else gt).shape[:2]
        out = out.cpu().numpy()
        assert guard.count == 2            # the workspace and the bit map came poisoned
    return out


# d >= 64 with the window inside the image (several 64-pixel seam steps, slab = d): (200, 600, 72), (300, 700, 72), (300, 700, 130)
# 2d+1 > H only: (5, 7, 3), (96, 160, 72); > W only: (37, 1, 2); both: (1, 1, 1), (1, 37, 1), (16, 16, 46), (17, 33, 46), (64, 65, 46)
BIT_CASES = [(1, 1, 1), (1, 37, 1), (37, 1, 2), (5, 7, 1), (5, 7, 2), (5, 7, 3), (16, 16, 1), (16, 16, 7), (16, 16, 46), (17, 33, 1),
             (17, 33, 2), (17, 33, 7), (17, 33, 46), (64, 65, 1), (64, 65, 2), (64, 65, 7), (64, 65, 46), (96, 160, 1), (96, 160, 2),
             (96, 160, 7), (96, 160, 46), (96, 160, 72), (200, 600, 72), (300, 700, 72), (300, 700, 130)]


@pytest.mark.parametrize('H,W,d', BIT_CASES)
def test_panoptic_boundary_bits(H, W, d):
    ratio = d / math.sqrt(H ** 2 + W ** 2)
    assert boundary_ref.dilation(H, W, ratio) == d
    rng = np.random.default_rng(H * 1000 + W * 10 + d)
    maps = label_maps(H, W, d, rng)
    for i, (name, lab) in enumerate(maps):
        other = maps[(i + 1) % len(maps)][1]
        void = None
        if name in ('uniform', 'blocks'):                 # a VOID rectangle whose instance bytes differ from pixel to pixel
            void = np.zeros((H, W), bool)
            void[H // 4:H // 2 + 1, W // 4:W // 2 + 1] = True
        gt = gt_from(lab, byte=i % 3)
        pred = pred_from(other, by='cat' if i % 2 else 'inst', void=void, rng=rng)
        want = ref.boundary_bits(pred, gt, d=d)
        for pattern in ('A', 'B'):
            assert np.array_equal(device_bits(pred, gt, ratio, pattern), want), (name, pattern)
        if i == 0:
            assert np.array_equal(device_bits(pred, None, ratio, 'A'), want & 2), name           # pred only
            assert np.array_equal(device_bits(None, gt, ratio, 'B'), want & 1), name             # GT only
            assert (want == 3).all() == (2 * d + 1 > H or 2 * d + 1 > W), name                  # ... else uniform has an interior


def test_panoptic_boundary_label_bytes():
    """Ids that differ only in the G or only in the B byte are different segments; pred keys that differ only in the category or only
    in the instance too; VOID pixels are one label whatever their instance byte."""
    from upsnet_amd.dataset.boundary import panoptic_boundary
    H, W, d = 24, 40, 2
    ratio = d / math.sqrt(H ** 2 + W ** 2)
    lab = (np.mgrid[0:H, 0:W][1] >= 20).astype(np.int64)
    rng = np.random.default_rng(5)
    for byte in (1, 2):
        for by in ('cat', 'inst'):
            gt, pred = gt_from(lab, byte), pred_from(lab, by)
            got = panoptic_boundary(torch.from_numpy(pred).cuda(), torch.from_numpy(gt).cuda(), ratio).cpu().numpy()
            assert np.array_equal(got, ref.boundary_bits(pred, gt, d=d))
            assert (got[d:-d, 18:22] == 3).all() and (got[d:-d, d:18] == 0).all() and (got[d:-d, 22:W - d] == 0).all()
    void = np.ones((H, W), bool)
    pred = pred_from(lab, 'cat', void=void, rng=rng)
    got = panoptic_boundary(pred_2ch=torch.from_numpy(pred).cuda(), ratio=ratio).cpu().numpy()
    assert (got[d:-d, d:-d] == 0).all() and (got[:d] == 2).all() and (got[:, -d:] == 2).all()


def test_panoptic_boundary_full_size_and_views():
    """1024 x 2048 at the default ratio (d = 46), once: a scene with bars of the critical widths pasted in; and a non-contiguous input
    view, which is copied (ops.pan_boundary_map)."""
    from upsnet_amd.dataset.boundary import panoptic_boundary
    H, W, d = 1024, 2048, 46
    assert boundary_ref.dilation(H, W) == d
    pred, gt, _ = ref.scene_images('full')[0]
    pred, gt = pred.copy(), gt.copy()
    rng = np.random.default_rng(9)
    bars = dict(label_maps(300, 900, d, rng))
    gt[100:400, 200:1100] = gt_from(bars['vbars'], 1)
    pred[600:900, 1000:1900] = pred_from(bars['hbars'], 'inst')
    want = ref.boundary_bits(pred, gt)
    assert 0.01 < (want == 0).mean() < 0.95
    for pattern in ('A', 'B'):
        assert np.array_equal(device_bits(pred, gt, 0.02, pattern), want), pattern
    wide = torch.from_numpy(np.concatenate([pred[:, :5], pred, pred[:, :3]], 1)).cuda()
    view = wide[:, 5:5 + W]
    assert not view.is_contiguous()
    got = panoptic_boundary(pred_2ch=view, ratio=0.02).cpu().numpy()
    assert np.array_equal(got, want & 2)


# ------------------------------------------------------------------------------------------------------------------ the evaluator
def evaluate(images, cats=ref.CATS, ratio=0.02, max_gt=4096, to_device=True):
    from upsnet_amd.dataset.pq import PanopticEvaluator
    ev = PanopticEvaluator(cats, device='cuda', max_gt_segments=max_gt, boundary=True, dilation_ratio=ratio)
    for pred, gt, info in images:
        if to_device:
            pred, gt = torch.from_numpy(np.ascontiguousarray(pred)).cuda(), torch.from_numpy(np.ascontiguousarray(gt)).cuda()
        ev.add(pred, gt, info)
    return ev


def test_hand_case():
    images = [ref.hand_case()]
    ev = evaluate(images, ref.HAND_CATS)
    assert_same(ev, ref.boundary_pq_restated(images, ref.HAND_CATS))
    res = ev.summary()
    assert (res['All']['pq'], res['Things']['pq'], res['Stuff']['pq']) == (16 / 43, 0.0, 32 / 43)
    assert set(res) == {'All', 'Things', 'Stuff', 'per_class'}


@pytest.mark.parametrize('name', sorted(ref.SCENES))
def test_random_scenes(name):
    images = ref.scene_images(name)
    assert_same(evaluate(images), ref.scene_restated(name), msg=name)


def test_scenes_from_host_arrays_in_sequence():
    """Images of different sizes through one evaluator (the workspace grows once), host arrays uploaded by the evaluator."""
    names = ['odd', 'small0', 'small1', 'mid_jitter', 'small_jitter']
    images = [ref.scene_images(n)[0] for n in names]
    ev = evaluate(images, to_device=False)
    assert ev.num_images == 5
    assert_same(ev, ref.boundary_pq_restated(images, ref.CATS))


def test_pixel_noise_map():
    rng = np.random.default_rng(11)
    images = [scene(rng, 128, 256, 6, 6, noise=True, void=0.1)]
    assert_same(evaluate(images), ref.boundary_pq_restated(images, ref.CATS))


def test_many_gt_segments():
    """More than 1000 GT segments and pred keys; d = 2 so that the 16 x 19 pixel cells keep an interior."""
    rng = np.random.default_rng(12)
    images = [scene(rng, 512, 768, 32, 40, missing=0, void=0.0005, shift=(1, 0))]
    assert len(images[0][2]) > 1000 and boundary_ref.dilation(512, 768, 0.002) == 2
    want = ref.boundary_pq_restated(images, ref.CATS, 0.002)
    assert 0 < want[0].sum() < pq_restated(images, ref.CATS)[0].sum()
    assert_same(evaluate(images, ratio=0.002), want)
    assert_same(evaluate(images * 2, ratio=0.002, max_gt=1280), ref.boundary_pq_restated(images * 2, ref.CATS, 0.002))


def test_all_void_pred():
    H, W = 60, 77
    gt = id_rgb(np.full((H, W), 5))
    info = [{'id': 5, 'category_id': 3, 'iscrowd': 0, 'area': H * W}]
    void = np.full((H, W, 3), 255, np.uint8)
    void[..., 1] = np.arange(W) & 255
    images = [(void, gt, info), (void, id_rgb(np.zeros((H, W))), [])]
    ev = evaluate(images)
    assert raw(ev)[0][:, 3].tolist() == [0, 0, 1] and raw(ev)[0].sum() == 1
    assert_same(ev, ref.boundary_pq_restated(images, ref.CATS))


def test_add_png_on_a_relabelled_prediction():
    """The prediction as a COCO panoptic PNG of arbitrary ids: relabelled on the device, then scored like add()."""
    from upsnet_amd.dataset.pq import PanopticEvaluator
    for name in ('small0', 'mid_jitter'):
        pred, gt, info = ref.scene_images(name)[0]
        key = ref.pred_labels(pred)
        ids = np.where(key == ref.PRED_VOID, 0, key * 7 + 11)
        pinfo = [{'id': int(i), 'category_id': int((i - 11) // 7 >> 8)} for i in np.unique(ids) if i]
        ev = PanopticEvaluator(ref.CATS, device='cuda', boundary=True)
        ev.add_png(id_rgb(ids), pinfo, gt, info)
        assert_same(ev, ref.scene_restated(name), msg=name)


def test_merge_determinism_and_zeroed_workspace():
    names = ['small0', 'small1', 'odd']
    images = [ref.scene_images(n)[0] for n in names]
    max_gt = 64
    ev = evaluate(images, max_gt=max_gt)
    want = ref.boundary_pq_restated(images, ref.CATS)
    assert_same(ev, want)
    cnt1, iou1 = raw(ev)
    cnt2, iou2 = raw(evaluate(images, max_gt=max_gt))
    assert np.array_equal(cnt1, cnt2) and np.array_equal(iou1.view(np.int64), iou2.view(np.int64))
    # every count cell of both areas and the key counter are zero again after the last call
    ws = ev._state['ws'].cpu().numpy()
    cells = 2 * (2 * 65536 + max_gt * 256) + max_gt
    assert not ws[:cells * 4].any()
    nkeys = cells * 4 + max_gt * (24 + 8) + 256 * 4
    assert not ws[nkeys:nkeys + 8].any()
    # two evaluators merged: PQStat semantics, a's sums plus b's
    from upsnet_amd.dataset.base_dataset import PQStat
    a, b = evaluate(images[:1]), evaluate(images[1:])
    a += b
    assert a.num_images == 3
    merged = PQStat()
    for chunk in (images[:1], images[1:]):
        part = PQStat()
        tp, fp, fn, iou = ref.boundary_pq_restated(chunk, ref.CATS)
        for c in np.nonzero(tp + fp + fn)[0]:
            s = part[int(c)]
            s.tp, s.fp, s.fn, s.iou = int(tp[c]), int(fp[c]), int(fn[c]), float(iou[c])
        merged += part
    got = a.pq_stat()
    assert {c: (s.tp, s.fp, s.fn, s.iou) for c, s in got.pq_per_cat.items()} == \
        {c: (s.tp, s.fp, s.fn, s.iou) for c, s in merged.pq_per_cat.items()}
    one = evaluate(images).pq_stat()
    assert {c: (s.tp, s.fp, s.fn) for c, s in got.pq_per_cat.items()} == {c: (s.tp, s.fp, s.fn) for c, s in one.pq_per_cat.items()}
    with pytest.raises(ValueError, match='dilation_ratio'):
        a += evaluate(images[:1], ratio=0.05)


def test_poisoned_memory_evaluator():
    images = [ref.scene_images('small0')[0], ref.scene_images('odd')[0]]
    want = ref.boundary_pq_restated(images, ref.CATS)
    for pattern in ('A', 'B'):
        with memguard.poisoned(pattern):
            ev = evaluate([(memguard.banded_copy(torch.from_numpy(p).cuda(), pattern), memguard.banded_copy(torch.from_numpy(g).cuda(), pattern),
                            info) for p, g, info in images], to_device=False)
            assert_same(ev, want, msg=pattern)


@pytest.mark.parametrize('name', ['small0', 'small1', 'odd'])
def test_window_larger_than_the_image_equals_the_plain_evaluator(name):
    """The link to the pinned path: with 2d+1 > min(H, W) and consistent JSON areas the boundary evaluator equals the plain
    PanopticEvaluator on the same images bit for bit."""
    from upsnet_amd.dataset.pq import PanopticEvaluator
    images = ref.scene_images(name) + [ref.hand_case()]
    cats = dict(ref.CATS)
    plain = PanopticEvaluator(cats, device='cuda')
    for pred, gt, info in images:
        plain.add(pred, gt, info)
    b = evaluate(images, cats, ratio=0.5)
    cnt, iou = raw(plain)
    cnt_b, iou_b = raw(b)
    assert np.array_equal(cnt, cnt_b) and np.array_equal(iou.view(np.int64), iou_b.view(np.int64)) and cnt[0].sum() > 0
    assert plain.summary() == b.summary()


# ------------------------------------------------------------------------------------------------------------------ command line
def test_evaluate_eval_only_eval_boundary_pq(tmp_path, saved_config):     # noqa: F811
    """A generated Cityscapes-layout dataset with a hand-written panoptic GT and results pickle through
    python -m upsnet_amd.evaluate --eval_only --eval_boundary_pq, then --score_panoptic --eval_boundary_pq on the written files."""
    from PIL import Image
    from upsnet_amd.config.config import config, update_config
    from upsnet_amd.dataset import Cityscapes
    from upsnet_amd.dataset.base_dataset import PQStat
    from upsnet_amd.dataset.pq import pq_summary
    from upsnet_amd.evaluate import final_output_path, main
    H, W = 64, 96
    root = str(tmp_path / 'cs')
    make_dataset(root, 'Cityscapes', [(H, W), (H, W)], ids=[2, 1], seed=1)
    head = write_cfg(tmp_path, 'Cityscapes', root, 'val')
    cfg = tmp_path / 'panoptic_only.yaml'
    cfg.write_text(open(head).read().replace('network:\n', 'network:\n  has_rcnn: false\n  has_mask_head: false\n  has_fcn_head: false\n')
                   .replace('test:\n', 'test:\n  panoptic_stuff_area_limit: 16\n'))
    cfg = str(cfg)
    update_config(cfg)
    ds = Cityscapes(image_sets=['val'], phase='test')
    rng = np.random.default_rng(2)
    ssegs, panos, clss = [], [], []
    for _ in ds.roidb:
        # a 2 x 3 grid: stuff classes in the top row, three instances (thing classes 1..8, 1-based) in the bottom row
        stuff, cls = rng.choice(11, 3, replace=False), rng.integers(1, 9, 3)
        grid = np.array([stuff, 11 + np.arange(3)])
        pano = np.repeat(np.repeat(grid, H // 2, 0), W // 3, 1)
        sseg = np.where(pano <= 10, pano, 10 + cls[np.clip(pano - 11, 0, 2)])
        ssegs.append(sseg.astype(np.uint8)), panos.append(pano.astype(np.uint8)), clss.append(cls.astype(np.int64))
    preds = [p.cpu().numpy() for p in ds.get_unified_pan_result(ssegs, panos, clss, stuff_area_limit=16)]
    assert all((p[..., 0] != 255).all() and len(np.unique(ref.pred_labels(p))) == 6 for p in preds)
    os.makedirs(ds.panoptic_gt_folder)
    images, pan_images, pan_anns = [], [], []
    for entry, pred in zip(ds.roidb, preds):
        key = ref.pred_labels(pred)
        gid = np.roll(key + 1, (0, 1), (0, 1))                                 # the GT: the prediction shifted, with some VOID
        gid[rng.random((H, W)) < 0.002] = 0
        info = [{'id': int(g), 'category_id': int((g - 1) >> 8), 'iscrowd': 0, 'area': int((gid == g).sum())} for g in np.unique(gid) if g]
        name = 'pan_%d.png' % entry['id']
        Image.fromarray(id_rgb(gid)).save(os.path.join(ds.panoptic_gt_folder, name))
        pan_images.append({'id': entry['id'], 'file_name': name})
        pan_anns.append({'image_id': entry['id'], 'file_name': name, 'segments_info': info})
        images.append((pred, id_rgb(gid), info))
    categories = [{'id': c, 'name': 'c%d' % c, 'isthing': int(c > 10)} for c in range(19)]
    with open(ds.panoptic_json_file, 'w') as f:
        json.dump({'images': pan_images, 'annotations': pan_anns, 'categories': categories}, f)
    results_dir = os.path.join(final_output_path(cfg), 'results')
    os.makedirs(results_dir)
    with open(os.path.join(results_dir, 'results_list.pkl'), 'wb') as f:
        pickle.dump({'all_boxes': None, 'all_masks': None, 'all_ssegs': ssegs, 'all_panos': panos, 'all_pano_cls_inds': clss}, f)

    cats = {c['id']: c for c in categories}

    def summary(counts):
        stat = PQStat()
        tp, fp, fn, iou = counts
        for c in np.nonzero(tp + fp + fn)[0]:
            s = stat[int(c)]
            s.tp, s.fp, s.fn, s.iou = int(tp[c]), int(fp[c]), int(fn[c]), float(iou[c])
        return pq_summary(stat, cats)
    want, want_mask = summary(ref.boundary_pq_restated(images, cats)), summary(pq_restated(images, cats))
    want5 = summary(ref.boundary_pq_restated(images, cats, 0.05))
    assert want != want_mask and want5 != want and want['All']['pq'] > 0

    plain = main(['--cfg', cfg, '--eval_only'])
    assert list(plain['metrics']) == ['panoptic'] and plain['metrics']['panoptic'] == want_mask
    res = main(['--cfg', cfg, '--eval_only', '--eval_boundary_pq', '--write_panoptic'])
    assert list(res['metrics']) == ['panoptic', 'panoptic_boundary']
    assert res['metrics']['panoptic'] == plain['metrics']['panoptic'] and res['metrics']['panoptic_boundary'] == want
    wide = main(['--cfg', cfg, '--eval_only', '--eval_boundary_pq', '--boundary_pq_dilation_ratio', '0.05'])
    assert wide['metrics']['panoptic_boundary'] == want5 and wide['metrics']['panoptic'] == want_mask
    out = os.path.join(results_dir, 'pans_unified')
    scored = main(['--cfg', cfg, '--score_panoptic', os.path.join(out, 'pred.json'), '--score_panoptic_folder', os.path.join(out, 'pan'),
                   '--eval_boundary_pq'])
    assert list(scored['metrics']) == ['panoptic', 'panoptic_boundary'] and scored['times'] is None
    assert scored['metrics']['panoptic'] == want_mask and scored['metrics']['panoptic_boundary'] == want
    assert config.network.has_panoptic_head

    # --pan_combined with --eval_boundary_pq: the combined merge of the same scenes' detections and semantic maps, scored by both rules
    # (evaluate_results' branch; through main it also needs the box, mask and semantic ground truth of the other heads)
    from test_pan_combined_cpu import per_class, restate_combined
    from upsnet_amd.evaluate import evaluate_results
    per_image = [per_class(H, W, [(int(c), 0.9 - 0.1 * i, pano == 11 + i) for i, c in enumerate(cls)]) for pano, cls in zip(panos, clss)]
    all_boxes = [[]] + [[b[c][0] for b, _ in per_image] for c in range(1, 9)]
    all_masks = [[]] + [[m[c][0] for _, m in per_image] for c in range(1, 9)]
    results = {'all_boxes': all_boxes, 'all_masks': all_masks, 'all_ssegs': ssegs, 'all_panos': panos, 'all_pano_cls_inds': clss}
    metrics = evaluate_results(ds, results, results_dir, pan_combined=True, boundary_pq_ratio=0.02)
    assert list(metrics) == ['panoptic', 'panoptic_boundary', 'panoptic_combined', 'panoptic_combined_boundary']
    combined = [(p, gt, info) for p, (_, gt, info) in zip(restate_combined(ssegs, all_boxes, all_masks, stuff_area_limit=16), images)]
    assert all(len(np.unique(ref.pred_labels(p))) == 6 for p, _, _ in combined)
    want_c, want_c_mask = summary(ref.boundary_pq_restated(combined, cats)), summary(pq_restated(combined, cats))
    assert want_c != want_c_mask and want_c['All']['pq'] > 0
    assert metrics['panoptic_combined_boundary'] == want_c and metrics['panoptic_combined'] == want_c_mask
    assert metrics['panoptic_boundary'] == want and metrics['panoptic'] == want_mask
    assert 'panoptic_combined_boundary' not in evaluate_results(ds, results, results_dir, pan_combined=True)
