"""CPU: panoptic quality (PQ) host side -- the PQStat mirror against the reference-Python golden results (tests/golden/pq.npz,
made by tests/golden/make_golden_pq.py), a numpy restatement of the PQ rules pinned to the same golden (tests/test_pq_gpu.py holds
the device to it), host validation before any launch, and the PIL / JSON loading of evaluate_panoptic."""
import json
import os

import numpy as np
import pytest
import torch

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def golden():
    return np.load(os.path.join(G, "pq.npz"))


def golden_categories(g):
    return {el['id']: el for el in json.loads(str(g['categories']))}


def golden_images(g, name):
    return [(g['%s_%d_pred' % (name, i)], g['%s_%d_gt' % (name, i)], json.loads(str(g['%s_%d_segs' % (name, i)])))
            for i in range(int(g[name + '_n']))]


def golden_results(g, name):
    r = json.loads(str(g[name + '_results']))
    if r['per_class'] is not None:
        r['per_class'] = {int(k): v for k, v in r['per_class'].items()}
    return r


def rgb_to_id(rgb):
    rgb = np.asarray(rgb).astype(np.int64)
    return rgb[..., 0] + 256 * rgb[..., 1] + 65536 * rgb[..., 2]


def pq_restated(images, categories):
    """The PQ rules restated with numpy, one image after another: -> tp, fp, fn (int64 [256]), iou (float64 [256]).
    Pred segments: distinct (cat, inst) with cat != 255, area = pixel count. GT: segments_info (JSON area), id 0 = VOID, ids
    missing from the JSON ignored. Match: same category, non-crowd GT, iou = inter / (area_p + area_g - inter - inter(VOID, p)) > 0.5
    in float64, added per category in ascending (GT id, instance). FN: unmatched non-crowd GT. FP: unmatched pred unless
    (inter(VOID, p) + inter(last crowd GT of its category, p)) / area_p > 0.5."""
    tp, fp, fn = (np.zeros(256, np.int64) for _ in range(3))
    iou = np.zeros(256, np.float64)
    for idx, (pred, gt, info) in enumerate(images):
        pred = np.asarray(pred)
        cat, inst = pred[..., 0].astype(np.int64), pred[..., 1].astype(np.int64)
        valid = cat != 255
        pkey = (cat * 256 + inst)[valid]
        gid = rgb_to_id(gt)[valid]
        keys, areas = np.unique(pkey, return_counts=True)
        area_p = dict(zip(keys.tolist(), areas.tolist()))
        for k in area_p:
            if k >> 8 not in categories:
                raise KeyError('image %d: unknown category_id %d' % (idx, k >> 8))
        pairs, counts = np.unique(gid * 65536 + pkey, return_counts=True)
        inter = dict(zip(pairs.tolist(), counts.tolist()))
        segs = {el['id']: el for el in info}
        matched_g, matched_p = set(), set()
        for pair, x in zip(pairs.tolist(), counts.tolist()):        # ascending GT id, then key (= instance within a category)
            g, k = pair >> 16, pair & 65535
            s = segs.get(g)
            if s is None or s['iscrowd'] == 1 or s['category_id'] != k >> 8:
                continue
            union = area_p[k] + s['area'] - x - inter.get(k, 0)
            with np.errstate(divide='ignore'):
                v = np.float64(x) / np.float64(union)
            if v > 0.5:
                c = s['category_id']
                tp[c] += 1
                iou[c] += v
                matched_g.add(g)
                matched_p.add(k)
        crowd = {}
        for g, s in segs.items():
            if g in matched_g:
                continue
            if s['iscrowd'] == 1:
                crowd[s['category_id']] = g
                continue
            fn[s['category_id']] += 1
        for k, a in area_p.items():
            if k in matched_p:
                continue
            x = inter.get(k, 0)
            if k >> 8 in crowd:
                x += inter.get(crowd[k >> 8] * 65536 + k, 0)
            if x / a > 0.5:
                continue
            fp[k >> 8] += 1
    return tp, fp, fn, iou


def test_pq_average_mirror_matches_reference_golden():
    from upsnet_amd.dataset.base_dataset import PQStat
    from upsnet_amd.dataset.pq import pq_summary
    g = golden()
    cats = golden_categories(g)
    for name in g['cases'].tolist():
        stat = PQStat()
        cnt, iou = g[name + '_counts'], g[name + '_iou']
        for c in np.nonzero(cnt.sum(0))[0]:
            s = stat[int(c)]
            s.tp, s.fp, s.fn, s.iou = int(cnt[0, c]), int(cnt[1, c]), int(cnt[2, c]), float(iou[c])
        want = golden_results(g, name)
        if want['All'] == 'ZeroDivisionError':
            with pytest.raises(ZeroDivisionError):
                pq_summary(stat, cats)
            continue
        got = {}
        for metric, isthing in [("All", None), ("Things", True), ("Stuff", False)]:
            try:
                got[metric], per_class = stat.pq_average(cats, isthing=isthing)
            except ZeroDivisionError:
                got[metric], per_class = 'ZeroDivisionError', None
            if metric == 'All':
                got['per_class'] = per_class
        assert got == want, name
        if 'ZeroDivisionError' not in (want['Things'], want['Stuff']):
            assert pq_summary(stat, cats) == want


def test_pqstat_iadd_merges_per_category():
    from upsnet_amd.dataset.base_dataset import PQStat
    a, b = PQStat(), PQStat()
    a[3].tp, a[3].iou, b[3].tp, b[3].iou, b[5].fn = 1, 0.75, 2, 1.5, 4
    a += b
    assert (a[3].tp, a[3].iou, a[5].fn, a[5].tp) == (3, 2.25, 4, 0)


def test_restatement_matches_reference_golden():
    """The restatement reproduces the reference's counts and IoU sums on every golden case, and through the host PQStat mirror its
    result dicts; the fixture covers what its case names say."""
    from upsnet_amd.dataset.base_dataset import PQStat
    g = golden()
    cats = golden_categories(g)
    names = set(g['cases'].tolist())
    assert {'exact', 'iou_half', 'iou_above', 'cat_mismatch', 'void_absorb', 'crowd_absorb', 'crowd_last', 'gt_missing',
            'pred_void_inst', 'area_json', 'mixed', 'empty_json', 'sequence', 'scene0', 'scene1', 'scene2'} <= names
    assert g['iou_half_counts'][:, 12].tolist() == [0, 1, 1]
    assert g['iou_above_counts'][:, 12].tolist() == [1, 0, 0]
    assert g['void_absorb_counts'][:, 15].tolist() == [0, 1, 0]
    assert g['crowd_last_counts'][:, 16].tolist() == [0, 1, 0]
    assert all(g[n + '_counts'][:, 40].sum() == 0 for n in names)
    assert os.path.getsize(os.path.join(G, "pq.npz")) < 1 << 20
    for name in sorted(names):
        tp, fp, fn, iou = pq_restated(golden_images(g, name), cats)
        np.testing.assert_array_equal(np.stack([tp, fp, fn]), g[name + '_counts'], err_msg=name)
        assert np.array_equal(iou.view(np.int64), g[name + '_iou'].view(np.int64)), name   # bit-identical
        stat = PQStat()
        for c in np.nonzero(tp + fp + fn)[0]:
            s = stat[int(c)]
            s.tp, s.fp, s.fn, s.iou = int(tp[c]), int(fp[c]), int(fn[c]), float(iou[c])
        want = golden_results(g, name)
        if want['All'] != 'ZeroDivisionError':
            assert stat.pq_average(cats, None) == (want['All'], want['per_class']), name


def test_alias_tree_exposes_host_classes():
    from upsnet.dataset.base_dataset import PQStat, PQStatCat, BaseDataset
    from upsnet_amd.dataset import base_dataset
    assert PQStat is base_dataset.PQStat and PQStatCat is base_dataset.PQStatCat
    assert hasattr(BaseDataset, 'evaluate_panoptic') and hasattr(BaseDataset, 'get_confusion_matrix')


def _img(H=8, W=8):
    return np.zeros((H, W, 3), np.uint8)


@pytest.mark.parametrize("segs,kw,what", [
    ([{'id': 3, 'category_id': 1, 'iscrowd': 0, 'area': 1}, {'id': 3, 'category_id': 2, 'iscrowd': 0, 'area': 1}], {}, "duplicate"),
    ([{'id': 0, 'category_id': 1, 'iscrowd': 0, 'area': 1}], {}, "id 0"),
    ([{'id': 4, 'category_id': 255, 'iscrowd': 0, 'area': 1}], {}, "0..254"),
    ([{'id': 4, 'category_id': -1, 'iscrowd': 0, 'area': 1}], {}, "0..254"),
    ([{'id': i + 1, 'category_id': 1, 'iscrowd': 0, 'area': 1} for i in range(3)], {'max_gt_segments': 2}, "max_gt_segments"),
])
def test_host_validation_raises_before_any_launch(segs, kw, what):
    from upsnet_amd.dataset.pq import PanopticEvaluator
    ev = PanopticEvaluator({1: {'isthing': 0}, 2: {'isthing': 1}}, device='cuda:0', **kw)
    with pytest.raises(ValueError, match=what):
        ev.add(_img(), _img(), segs)
    assert ev._state is None and ev.num_images == 0   # nothing allocated, nothing queued


def test_host_validation_shapes():
    from upsnet_amd.dataset.pq import PanopticEvaluator
    ev = PanopticEvaluator([{'id': 1, 'isthing': 0}], device='cuda:0')
    with pytest.raises(ValueError, match="differ in shape"):
        ev.add(_img(8, 8), _img(8, 9), [])
    with pytest.raises(ValueError, match=r"uint8 \[H,W,3\]"):
        ev.add(_img()[:, :, :2], _img()[:, :, :2], [])
    with pytest.raises(ValueError, match=r"uint8 \[H,W,3\]"):
        ev.add(_img().astype(np.int32), _img(), [])
    with pytest.raises(ValueError):
        PanopticEvaluator({255: {'isthing': 0}})
    assert ev._state is None


def test_ops_refuse_cpu_tensors():
    from upsnet_amd import ops
    z8 = torch.zeros((4, 4, 3), dtype=torch.uint8)
    with pytest.raises(Exception, match="not implemented"):   # require_cuda, as the reference's Functions
        ops.pq_accumulate(z8, z8, torch.zeros((0, 4), dtype=torch.int64), torch.zeros(256, dtype=torch.uint8), 0, 16,
                          torch.zeros(16, dtype=torch.uint8), *(torch.zeros(256, dtype=torch.int64) for _ in range(3)),
                          torch.zeros(256, dtype=torch.float64), torch.zeros(1, dtype=torch.int64))
    with pytest.raises(Exception, match="not implemented"):   # require_cuda, as the reference's Functions
        ops.confusion_accumulate(torch.zeros(5, dtype=torch.uint8), torch.zeros(5, dtype=torch.uint8), 3, -1,
                                 torch.zeros((3, 3), dtype=torch.int64))


def test_pq_entry_points_validate_on_the_host():
    from upsnet_amd import _lib
    lib = _lib.lib()
    assert lib.upsnet_pq_workspace_bytes(4097) == 0 and lib.upsnet_pq_workspace_bytes(-1) == 0
    assert lib.upsnet_pq_workspace_bytes(100) > 2 * 65536 * 4 + 100 * 256 * 4
    one = ctypes_p(1)
    assert lib.upsnet_pq_accumulate(None, None, one, 4, 4, None, 0, one, 0, 16, one, one, one, one, one, one) != 0
    assert b"null pointer" in lib.upsnet_last_error()
    assert lib.upsnet_pq_accumulate(None, one, one, 4, 4, one, 17, one, 0, 16, one, one, one, one, one, one) != 0
    assert b"17 GT segments" in lib.upsnet_last_error()
    assert lib.upsnet_confusion_accumulate(None, one, one, 10, 300, -1, one) != 0
    assert b"class_num" in lib.upsnet_last_error()


def ctypes_p(v):
    import ctypes
    return ctypes.c_void_p(v)


def test_evaluate_panoptic_loading(tmp_path):
    """The PIL / JSON side of evaluate_panoptic: a panoptic PNG (RGB or RGBA) becomes the expected id map, in the JSON's image order."""
    from PIL import Image
    from upsnet_amd.dataset.base_dataset import BaseDataset, load_panoptic_png
    rng = np.random.default_rng(0)
    ids = [rng.integers(0, 1 << 24, (6, 9)), rng.integers(0, 300, (5, 4))]
    folder = tmp_path / "gt"
    folder.mkdir()
    rgb = [np.stack([i & 255, (i >> 8) & 255, (i >> 16) & 255], -1).astype(np.uint8) for i in ids]
    Image.fromarray(rgb[0]).save(folder / "b.png")
    Image.fromarray(np.concatenate([rgb[1], np.full(rgb[1].shape[:2] + (1,), 255, np.uint8)], -1), mode='RGBA').save(folder / "a.png")
    js = {'images': [{'id': 1, 'file_name': 'b.png'}, {'id': 2, 'file_name': 'a.png'}],
          'annotations': [{'image_id': 1, 'segments_info': []}, {'image_id': 2, 'segments_info': [{'id': 7, 'category_id': 3}]}],
          'categories': [{'id': 3, 'isthing': 1}, {'id': 0, 'isthing': 0}]}
    (tmp_path / "pan.json").write_text(json.dumps(js))

    class DS(BaseDataset):
        panoptic_json_file = str(tmp_path / "pan.json")
        panoptic_gt_folder = str(folder)

    images, annotations, categories = DS().load_panoptic_gt()
    images = list(images)
    assert [rgb_to_id(im).tolist() for im in images] == [i.tolist() for i in ids]
    assert all(im.dtype == np.uint8 and im.shape[2] == 3 for im in images)
    assert annotations == js['annotations'] and sorted(categories) == [0, 3] and categories[3]['isthing'] == 1
    (folder / "bad.png").write_bytes(b"not a png")
    with pytest.raises(Exception):
        load_panoptic_png(str(folder / "bad.png"))
    Image.fromarray(ids[1].astype(np.uint8)).save(folder / "gray.png")
    with pytest.raises(ValueError):
        load_panoptic_png(str(folder / "gray.png"))
