"""GPU: panoptic quality and the confusion matrix on the device (csrc/pq_eval.hip via dataset/pq.py and dataset/base_dataset.py)
against the reference-Python golden (tests/golden/pq.npz) and against the numpy restatement of tests/test_pq_cpu.py (itself pinned
to the golden): counts exact, IoU sums bit-identical wherever the JSON areas equal the pixel counts."""
import numpy as np
import pytest
import torch

from test_pq_cpu import golden, golden_categories, golden_images, golden_results, pq_restated

pytestmark = pytest.mark.gpu

CATS = {c: {'id': c, 'isthing': int(c >= 11)} for c in range(19)}


def evaluate(images, cats, max_gt=4096, to_device=True):
    from upsnet_amd.dataset.pq import PanopticEvaluator
    ev = PanopticEvaluator(cats, device='cuda', max_gt_segments=max_gt)
    for pred, gt, info in images:
        if to_device:
            pred, gt = torch.from_numpy(np.ascontiguousarray(pred)).cuda(), torch.from_numpy(np.ascontiguousarray(gt)).cuda()
        ev.add(pred, gt, info)
    return ev


def raw(ev):
    st = ev._state
    return (torch.stack([st['tp'], st['fp'], st['fn']]).cpu().numpy(), st['iou'].cpu().numpy())


def assert_same(ev, want, bit=True, msg=''):
    cnt, iou = raw(ev)
    tp, fp, fn, wiou = want
    np.testing.assert_array_equal(cnt, np.stack([tp, fp, fn]), err_msg=msg)
    if bit:
        assert np.array_equal(iou.view(np.int64), wiou.view(np.int64)), (msg, iou[iou != wiou], wiou[iou != wiou])
    else:
        np.testing.assert_allclose(iou, wiou, rtol=1e-12, atol=0, err_msg=msg)


def id_rgb(ids):
    ids = np.asarray(ids, np.int64)
    return np.stack([ids & 255, (ids >> 8) & 255, (ids >> 16) & 255], -1).astype(np.uint8)


def scene(rng, H, W, gh, gw, n_cat=19, void=0.02, shift=(3, -5), relabel=0.1, crowd=0.05, missing=2, noise=False, area_jitter=False):
    """GT: a gh x gw grid of segments (random unique ids / categories, VOID noise, some crowd, some missing from the JSON, random JSON
    order); pred: the same grid shifted, some segments relabelled, VOID noise. noise=True: every pixel picks its segment at random."""
    K = gh * gw
    if noise:
        cell = rng.integers(0, K, (H, W))
        pcell = rng.integers(0, K, (H, W))
    else:
        grid = rng.permutation(K).reshape(gh, gw)
        cell = np.repeat(np.repeat(grid, -(-H // gh), 0), -(-W // gw), 1)[:H, :W]
        pcell = np.roll(cell, shift, (0, 1))
    seg_cat = rng.integers(0, n_cat, K)
    seg_id = rng.choice(np.arange(1, 1 << 24), K, replace=False)
    gt = seg_id[cell]
    gt[rng.random((H, W)) < void] = 0
    pcat = seg_cat.copy()
    flip = rng.random(K) < relabel
    pcat[flip] = rng.integers(0, n_cat, int(flip.sum()))
    pinst = np.zeros(K, np.int64)
    for c in range(n_cat):
        sel = np.nonzero(pcat == c)[0]
        pinst[sel] = np.arange(len(sel)) % 256
    cat, inst = pcat[pcell], pinst[pcell]
    cat[rng.random((H, W)) < void] = 255
    pred = np.stack([cat, inst, np.zeros_like(cat)], -1).astype(np.uint8)
    present, counts = np.unique(cell[gt != 0], return_counts=True)
    area = np.zeros(K, np.int64)
    area[present] = counts
    order = rng.permutation(K)[missing:]
    info = [{'id': int(seg_id[s]), 'category_id': int(seg_cat[s]), 'iscrowd': int(rng.random() < crowd),
             'area': int(area[s]) + (int(rng.integers(-3, 4)) if area_jitter else 0)} for s in order]
    return pred, id_rgb(gt), info


# ------------------------------------------------------------------------------------------------ golden (reference Python)
def test_golden_cases_bit_identical():
    from upsnet_amd.dataset.pq import pq_summary
    g = golden()
    cats = golden_categories(g)
    for name in g['cases'].tolist():
        ev = evaluate(golden_images(g, name), cats)
        cnt, iou = raw(ev)
        np.testing.assert_array_equal(cnt, g[name + '_counts'], err_msg=name)
        assert np.array_equal(iou.view(np.int64), g[name + '_iou'].view(np.int64)), name
        want = golden_results(g, name)
        if 'ZeroDivisionError' in (want['All'], want['Things'], want['Stuff']):
            with pytest.raises(ZeroDivisionError):
                ev.summary()
        else:
            assert ev.summary() == want == pq_summary(ev.pq_stat(), cats), name


def test_golden_sequence_from_host_arrays():
    """numpy inputs are uploaded by the evaluator; same result as device tensors."""
    g = golden()
    ev = evaluate(golden_images(g, 'sequence'), golden_categories(g), to_device=False)
    cnt, iou = raw(ev)
    np.testing.assert_array_equal(cnt, g['sequence_counts'])
    assert np.array_equal(iou, g['sequence_iou'])


# ------------------------------------------------------------------------------------------------ random scenes vs the restatement
@pytest.mark.parametrize("H,W,gh,gw,seed", [(1024, 2048, 8, 12, 0), (1024, 2048, 16, 24, 1), (800, 1333, 10, 10, 2),
                                            (800, 1333, 7, 19, 3), (37, 53, 3, 4, 4), (1, 1, 1, 1, 5)])
def test_random_scenes(H, W, gh, gw, seed):
    rng = np.random.default_rng(seed)
    images = [scene(rng, H, W, gh, gw)]
    assert_same(evaluate(images, CATS), pq_restated(images, CATS), msg=(H, W, seed))


def test_pixel_noise_maps():
    rng = np.random.default_rng(11)
    images = [scene(rng, 1024, 2048, 20, 20, noise=True, void=0.1)]
    assert_same(evaluate(images, CATS), pq_restated(images, CATS))


def test_many_gt_segments_and_pred_keys():
    rng = np.random.default_rng(12)
    pred, gt, info = scene(rng, 1024, 2048, 50, 64, missing=0)   # 3200 GT segments
    keys = np.unique(pred[..., 0].astype(np.int64) * 256 + pred[..., 1])
    assert len(info) >= 3000 and (keys >> 8 != 255).sum() > 2000
    images = [(pred, gt, info)]
    assert_same(evaluate(images, CATS), pq_restated(images, CATS))
    assert_same(evaluate(images[:1] * 2, CATS, max_gt=3200), pq_restated(images * 2, CATS))


def test_single_segment_and_all_void():
    H, W = 300, 517
    pred = np.zeros((H, W, 3), np.uint8)
    pred[..., 0] = 3
    gt = id_rgb(np.full((H, W), 5))
    info = [{'id': 5, 'category_id': 3, 'iscrowd': 0, 'area': H * W}]
    ev = evaluate([(pred, gt, info)], CATS)
    cnt, iou = raw(ev)
    assert cnt[:, 3].tolist() == [1, 0, 0] and iou[3] == 1.0 and cnt.sum() == 1
    void = np.full((H, W, 3), 255, np.uint8)
    void[..., 1] = 7
    images = [(void, gt, info), (void, id_rgb(np.zeros((H, W))), [])]
    ev = evaluate(images, CATS)
    assert raw(ev)[0][:, 3].tolist() == [0, 0, 1]
    assert_same(ev, pq_restated(images, CATS))


def test_inconsistent_json_areas():
    rng = np.random.default_rng(13)
    images = [scene(rng, 512, 768, 9, 11, area_jitter=True) for _ in range(2)]
    assert_same(evaluate(images, CATS), pq_restated(images, CATS), bit=False)


def test_unaligned_and_odd_sizes():
    """Views whose data do not start on a 16-byte boundary, and sizes that are no multiple of 16 pixels."""
    rng = np.random.default_rng(14)
    pred, gt, info = scene(rng, 101, 77, 4, 5)
    tp = torch.from_numpy(np.concatenate([pred[:1], pred])).cuda()[1:]
    tg = torch.from_numpy(np.concatenate([gt[:1], gt])).cuda()[1:]
    assert tp.data_ptr() % 16 != 0
    from upsnet_amd.dataset.pq import PanopticEvaluator
    ev = PanopticEvaluator(CATS, device='cuda')
    ev.add(tp, tg, info)
    assert_same(ev, pq_restated([(pred, gt, info)], CATS))


# ------------------------------------------------------------------------------------------------ streaming, merging, determinism
def test_streaming_merge_and_determinism():
    from upsnet_amd.dataset.base_dataset import PQStat
    rng = np.random.default_rng(21)
    images = [scene(rng, 512, 1024, int(rng.integers(3, 12)), int(rng.integers(3, 12))) for _ in range(8)]
    ev = evaluate(images, CATS)
    assert_same(ev, pq_restated(images, CATS))
    cnt1, iou1 = raw(ev)
    cnt2, iou2 = raw(evaluate(images, CATS))
    assert np.array_equal(cnt1, cnt2) and np.array_equal(iou1.view(np.int64), iou2.view(np.int64))
    # two ranks: reference semantics are PQStat() += chunk0; += chunk1
    a, b = evaluate(images[:3], CATS), evaluate(images[3:], CATS)
    a += b
    want = PQStat()
    for chunk in (images[:3], images[3:]):
        part = PQStat()
        tp, fp, fn, iou = pq_restated(chunk, CATS)
        for c in np.nonzero(tp + fp + fn)[0]:
            s = part[int(c)]
            s.tp, s.fp, s.fn, s.iou = int(tp[c]), int(fp[c]), int(fn[c]), float(iou[c])
        want += part
    got = a.pq_stat()
    assert a.num_images == 8
    assert {c: (s.tp, s.fp, s.fn, s.iou) for c, s in got.pq_per_cat.items()} == \
        {c: (s.tp, s.fp, s.fn, s.iou) for c, s in want.pq_per_cat.items()}


# ------------------------------------------------------------------------------------------------ end to end on the network
def test_end_to_end_on_the_network():
    from upsnet_amd.config.config import update_config_dict, CITYSCAPES_R50
    update_config_dict(CITYSCAPES_R50)
    from upsnet_amd.synthetic import build_model, make_image
    from upsnet_amd.dataset.base_dataset import BaseDataset
    model = build_model(device='cuda:0')
    with torch.no_grad():
        out = model(make_image(256, 512, seed=3, device='cuda:0'))
    pan_2ch = BaseDataset().get_unified_pan_result([out['fcn_outputs']], [out['panoptic_outputs']], [out['panoptic_cls_inds']])[0]
    pred = pan_2ch.cpu().numpy()
    key = pred[..., 0].astype(np.int64) * 256 + pred[..., 1]
    keys = [int(k) for k in np.unique(key) if k >> 8 != 255]
    assert len(keys) >= 3
    rng = np.random.default_rng(3)
    ids = rng.choice(np.arange(1, 1 << 24), len(keys), replace=False)
    gid = np.zeros(key.shape, np.int64)
    for k, i in zip(keys, ids):
        gid[key == k] = i
    info = [{'id': int(i), 'category_id': k >> 8, 'iscrowd': 0, 'area': int((gid == i).sum())} for k, i in zip(keys, ids)]
    ev = evaluate([(pan_2ch, torch.from_numpy(id_rgb(gid)).cuda(), info)], CATS, to_device=False)
    res = ev.summary()
    present = {k >> 8 for k in keys}
    assert all(res['per_class'][c]['pq'] == 1.0 for c in present) and res['All']['pq'] == 1.0 and res['All']['n'] == len(present)
    # a perturbed GT: shifted, VOID noise, one id dropped from the JSON, one segment crowd
    gid2 = np.roll(gid, (2, -3), (0, 1))
    gid2[rng.random(gid2.shape) < 0.05] = 0
    info2 = [dict(el, area=int((gid2 == el['id']).sum())) for el in info[1:]]
    info2[0]['iscrowd'] = 1
    images = [(pred, id_rgb(gid2), info2)]
    assert_same(evaluate([(pan_2ch, torch.from_numpy(id_rgb(gid2)).cuda(), info2)], CATS, to_device=False), pq_restated(images, CATS))


# ------------------------------------------------------------------------------------------------ confusion matrix / mIoU
def test_confusion_matrix_golden_and_miou():
    from upsnet_amd.dataset.base_dataset import BaseDataset
    g = golden()
    ds = BaseDataset()
    for name in ('cm_ignore', 'cm_alias', 'cm_small'):
        gt, pred, C, ignore = g[name + '_gt'], g[name + '_pred'], int(g[name + '_C']), int(g[name + '_ignore'])
        if ignore == 255:
            keep = gt != 255
            got = ds.get_confusion_matrix(gt[keep].astype(np.float32), pred[keep], C)
            res = ds.evaluate_ssegs_arrays([gt], [pred], C)
            assert np.array_equal(res['confusion_matrix'], g[name + '_cm'])
            cm = g[name + '_cm']
            tp = np.diag(cm)
            iu = tp / np.maximum(1.0, cm.sum(1) + cm.sum(0) - tp)
            assert np.array_equal(res['IU_array'], iu) and res['meanIU'] == iu.mean()
        else:
            got = ds.get_confusion_matrix(gt.astype(np.float32), pred, C)
        assert got.dtype == np.float64 and np.array_equal(got, g[name + '_cm']), name


def test_confusion_large_classes_and_sequence():
    """class_num beyond the LDS table (global atomics), several maps summed, 255 ignored, pred >= C aliasing."""
    from upsnet_amd.dataset.base_dataset import BaseDataset
    rng = np.random.default_rng(31)
    C = 133
    gts = [rng.integers(0, C, (300, 411)).astype(np.uint8) for _ in range(3)]
    preds = [np.where(rng.random(x.shape) < 0.7, x, rng.integers(0, 160, x.shape)).astype(np.uint8) for x in gts]
    gts[1][:50] = 255
    want = np.zeros((C, C))
    for gt, pred in zip(gts, preds):
        idx = (gt[gt != 255].astype(np.int64) * C + pred[gt != 255]).astype(np.int32)
        bc = np.bincount(idx, minlength=C * C)[:C * C]
        want += bc.reshape(C, C)
    res = BaseDataset().evaluate_ssegs_arrays([torch.from_numpy(x).cuda() for x in gts], preds, C)
    assert np.array_equal(res['confusion_matrix'], want)


# ------------------------------------------------------------------------------------------------ errors
def test_unknown_pred_category_raises_at_first_sync():
    rng = np.random.default_rng(41)
    images = [scene(rng, 64, 96, 3, 3) for _ in range(3)]
    bad = images[1][0].copy()
    bad[5:9, 5:9, 0] = 77
    images[1] = (bad, images[1][1], images[1][2])
    ev = evaluate(images, CATS)            # no exception while queueing
    with pytest.raises(KeyError, match=r"index 1 .*category_id 77"):
        ev.pq_stat()
    # merged: the first error keeps its image index relative to the merged sequence
    a = evaluate(images[:1], CATS)
    a += ev
    with pytest.raises(KeyError, match=r"index 2 .*category_id 77"):
        a.summary()


def test_cpu_tensors_raise():
    from upsnet_amd.dataset.pq import PanopticEvaluator
    ev = PanopticEvaluator(CATS, device='cuda')
    z = torch.zeros((4, 4, 3), dtype=torch.uint8)
    with pytest.raises(Exception, match="not implemented"):
        ev.add(z, z, [])
    from upsnet_amd import ops
    with pytest.raises(Exception, match="not implemented"):   # require_cuda, as the reference's Functions
        ops.confusion_accumulate(torch.zeros(5, dtype=torch.uint8), torch.zeros(5, dtype=torch.uint8), 3, -1,
                                 torch.zeros((3, 3), dtype=torch.int64))
