"""GPU: the label-map restore kernel (csrc/restore.hip) against its numpy restatement, and the evaluation run
(python -m upsnet_amd.evaluate) end to end on generated Cityscapes- and COCO-layout datasets whose ground truth is the direct chain's
own output: every pickled field equals the direct chain bit for bit, and every metric of a present category is exactly 1."""
import copy
import json
import os
import pickle

import numpy as np
import pytest
import torch

from test_dataset_run_cpu import make_dataset, write_cfg

pytestmark = pytest.mark.gpu


@pytest.fixture()
def saved_config():
    from upsnet_amd.config.config import config
    saved = copy.deepcopy(dict(config))
    yield config
    config.clear()
    config.update(saved)


# ------------------------------------------------------------------------------------------------ restore kernel
def _maps(rng, H, W, pad=0):
    """Two random int64 maps with values beyond uint8 (negative and > 255: the low byte is kept), as [1,H,W] views of wider buffers
    when pad > 0 (row stride W + pad)."""
    out = []
    for _ in range(2):
        big = torch.from_numpy(rng.integers(-700, 70000, (1, H, W + pad))).cuda()
        out.append(big[:, :, :W])
    return out


@pytest.mark.parametrize('im_info,pad', [((37, 53, 2.0), 0), ((37, 53, 0.5), 3), ((64, 96, 1.0), 0), ((61, 123, 1.6666666), 5),
                                         ((100, 141, 0.8533333), 0), ((1, 1, 3.0), 0)])
def test_restore_cv2_rule_matches_numpy(im_info, pad):
    from upsnet_amd import ops
    from upsnet_amd.dataset.restore import cv2_nearest_tables, restore_to_image
    rng = np.random.default_rng(int(im_info[0] * 1000 + im_info[1]))
    H, W = int(np.ceil(im_info[0] / 32.0) * 32), int(np.ceil(im_info[1] / 32.0) * 32)   # network resolution: padded
    sseg, pano = _maps(rng, H, W, pad)
    y, x = cv2_nearest_tables(im_info)
    hc, wc = int(im_info[0]), int(im_info[1])
    for s_map, p_map in ((sseg, pano), (sseg, None)):
        got_s, got_p = restore_to_image(s_map, p_map, im_info)
        torch.cuda.synchronize()
        want_s = s_map[0].cpu().numpy().astype('uint8')[:hc, :wc][y][:, x]
        assert got_s.dtype == torch.uint8 and tuple(got_s.shape) == (len(y), len(x))
        assert np.array_equal(got_s.cpu().numpy(), want_s)
        if p_map is None:
            assert got_p is None
        else:
            assert np.array_equal(got_p.cpu().numpy(), p_map[0].cpu().numpy().astype('uint8')[:hc, :wc][y][:, x])
    # a contiguous [H, W] map and host tables give the same bytes
    got, _ = ops.restore_label_maps(sseg[0].contiguous(), None, y, x)
    assert np.array_equal(got.cpu().numpy(), sseg[0].cpu().numpy().astype('uint8')[y][:, x])


@pytest.mark.parametrize('src,dst', [((37, 53), (40, 61)), ((256, 512), (1024, 2048)), ((1024, 2048), (1023, 2047)), ((7, 9), (3, 5)),
                                     ((33, 17), (33, 17)), ((5, 5), (1, 1))])
def test_restore_pil_rule_matches_pil(src, dst):
    from PIL import Image
    from upsnet_amd import ops
    from upsnet_amd.dataset.restore import pil_nearest_tables
    rng = np.random.default_rng(src[0] * 7 + dst[1])
    lab = rng.integers(0, 256, src).astype(np.uint8)
    y, x = pil_nearest_tables(src, dst)
    got, _ = ops.restore_label_maps(torch.from_numpy(lab.astype(np.int64)).cuda(), None, y, x)
    want = np.array(Image.fromarray(lab).resize((dst[1], dst[0]), Image.NEAREST))
    assert np.array_equal(got.cpu().numpy(), want)


def test_restore_rejects_tables_outside_the_source():
    from upsnet_amd import ops
    m = torch.zeros((1, 8, 8), dtype=torch.int64, device='cuda')
    with pytest.raises(ValueError):
        ops.restore_label_maps(m, None, np.array([0, 8], np.int32), np.array([0], np.int32))
    with pytest.raises(ValueError):
        ops.restore_label_maps(m.int(), None, np.array([0], np.int32), np.array([0], np.int32))


# ------------------------------------------------------------------------------------------------ end to end
NUM_SEG, ID_LAST_STUFF = 19, 10


def _direct_chain(model, path, num_classes):
    """PIL decode -> get_image_blob -> eager model -> float32 box scaling -> im_post -> numpy restore -> get_unified_pan_result."""
    from PIL import Image
    from upsnet_amd.dataset.base_dataset import BaseDataset
    from upsnet_amd.dataset.blob import get_image_blob
    from upsnet_amd.dataset.restore import cv2_nearest_tables
    from upsnet_amd.dataset.rle import im_post
    bgr = np.ascontiguousarray(np.asarray(Image.open(path).convert('RGB'))[:, :, ::-1])
    data = get_image_blob(bgr)
    im_info = data['im_info'][0]
    with torch.no_grad():
        out = model({'data': data['data'], 'im_info': data['im_info']})
    boxes = out['pred_boxes'][:, 1:].cpu().numpy() / im_info[2]          # float32 / float32, as im_detect
    assert boxes.dtype == np.float32
    b_all, m_all = [[] for _ in range(num_classes)], [[] for _ in range(num_classes)]
    im_post(b_all, m_all, out['cls_probs'], torch.from_numpy(boxes).cuda(), out['mask_probs'], out['cls_inds'], num_classes,
            np.round(im_info[:2] / im_info[2]).astype(np.int32))
    y, x = cv2_nearest_tables(im_info)
    hc, wc = int(im_info[0]), int(im_info[1])
    sseg = out['fcn_outputs'].cpu().numpy().squeeze(0).astype('uint8')[:hc, :wc][y][:, x]
    pano = out['panoptic_outputs'].cpu().numpy().squeeze(0).astype('uint8')[:hc, :wc][y][:, x]
    cls = out['panoptic_cls_inds'].cpu().numpy()
    pan_2ch = BaseDataset().get_unified_pan_result([sseg], [pano], [cls])[0].cpu().numpy()
    return dict(boxes=[b[0] for b in b_all[1:]], masks=[m[0] for m in m_all[1:]], sseg=sseg, pano=pano, cls=cls, pan_2ch=pan_2ch,
                im_scale=float(im_info[2]))


def _write_gt(ds, chains, ann_order, pan_ids):
    """The direct chain's outputs as the dataset's GT: label PNGs, panoptic PNGs + JSON (annotations in ann_order, image ids
    pan_ids), instances JSON annotations (one per detection with a non-empty mask). Returns the set of classes with an empty mask."""
    from PIL import Image
    from upsnet_amd.bbox.bbox_transform import xyxy_to_xywh
    os.makedirs(ds.panoptic_gt_folder, exist_ok=True)
    pan_images, pan_anns = [], []
    for k in ann_order:
        entry, ch = ds.roidb[k], chains[k]
        os.makedirs(os.path.dirname(ds.seg_gt_path(entry)), exist_ok=True)
        Image.fromarray(ch['sseg']).save(ds.seg_gt_path(entry))
        cat, inst = ch['pan_2ch'][:, :, 0].astype(np.int64), ch['pan_2ch'][:, :, 1].astype(np.int64)
        ids = np.where(cat == 255, 0, cat * 256 + inst + 1)
        rgb = np.stack([ids % 256, ids // 256 % 256, ids // 65536], 2).astype(np.uint8)
        name = 'pan_%d.png' % entry['id']
        Image.fromarray(rgb).save(os.path.join(ds.panoptic_gt_folder, name))
        u, cnt = np.unique(ids[ids > 0], return_counts=True)
        segs = [{'id': int(i), 'category_id': int((i - 1) // 256), 'iscrowd': 0, 'area': int(c)} for i, c in zip(u, cnt)]
        pan_images.append({'id': pan_ids[k], 'file_name': name})
        pan_anns.append({'image_id': pan_ids[k], 'file_name': name, 'segments_info': segs})
    categories = [{'id': c, 'name': 'c%d' % c, 'isthing': int(c > ID_LAST_STUFF)} for c in range(NUM_SEG)]
    with open(ds.panoptic_json_file, 'w') as f:
        json.dump({'images': pan_images, 'annotations': pan_anns, 'categories': categories}, f)
    with open(ds.instances_json_file) as f:
        inst = json.load(f)
    cat_ids = [c['id'] for c in inst['categories']]
    anns, empty = [], set()
    for k, entry in enumerate(ds.roidb):
        for c in range(1, len(cat_ids) + 1):
            dets, rles = chains[k]['boxes'][c - 1], chains[k]['masks'][c - 1]
            for d, rle in zip(dets, rles):
                area = _rle_area(rle)
                if area == 0:
                    empty.add(c)
                    continue
                anns.append({'id': len(anns) + 1, 'image_id': entry['id'], 'category_id': cat_ids[c - 1], 'iscrowd': 0, 'area': area,
                             'bbox': [float(v) for v in xyxy_to_xywh(d[None, :4].astype(np.float64))[0]], 'segmentation': rle})
    inst['annotations'] = anns
    with open(ds.instances_json_file, 'w') as f:
        json.dump(inst, f)
    return empty


def _rle_area(rle):
    """Pixel count of a compressed COCO RLE string (pycocotools' rleFrString, restated)."""
    s, counts, p = rle['counts'], [], 0
    while p < len(s):
        x, k, more = 0, 0, True
        while more:
            c = ord(s[p]) - 48
            x |= (c & 0x1f) << (5 * k)
            more = bool(c & 0x20)
            p += 1
            k += 1
            if not more and (c & 0x10):
                x |= -1 << (5 * k)
        if len(counts) > 2:
            x += counts[-2]
        counts.append(x)
    return int(sum(counts[1::2]))


CASES = {
    # dataset class: image sizes -> im_scale under scales 256 / max_size 512
    # Cityscapes (PNG): 1.0 (x5, one shape: graph replay with 2 images in flight), 2.0, 0.8533
    'Cityscapes': ('val', [(256, 512)] * 5 + [(128, 256), (300, 600)]),
    # COCO (JPEG): 1.28, 1.0, 0.64, 1.4222
    'coco': ('val2017', [(200, 300), (256, 384), (400, 500), (180, 250)]),
}


@pytest.mark.parametrize('kind', ['Cityscapes', 'coco'])
def test_evaluate_end_to_end_self_consistent(kind, tmp_path, saved_config):
    from upsnet_amd.config.config import update_config
    from upsnet_amd.dataset import Cityscapes, coco
    from upsnet_amd.evaluate import main
    from upsnet_amd.synthetic import build_model
    image_set, sizes = CASES[kind]
    root = str(tmp_path / kind)
    make_dataset(root, kind, sizes, seed=11)
    cfg = write_cfg(tmp_path, kind, root, image_set)
    update_config(cfg)
    ds = (Cityscapes if kind == 'Cityscapes' else coco)(image_sets=[image_set], phase='test')
    model = build_model(device='cuda')
    model.use_graph = False
    chains = [_direct_chain(model, e['image'], ds.num_classes) for e in ds.roidb]
    scales = sorted(set(round(c['im_scale'], 4) for c in chains))
    assert scales[0] < 1.0 < scales[-1] and 1.0 in scales, scales
    n = len(ds.roidb)
    if kind == 'Cityscapes':   # panoptic ids are strings, as in Cityscapes' panoptic JSON: positional pairing
        ann_order, pan_ids = list(range(n)), ['img_%d' % e['id'] for e in ds.roidb]
    else:                      # COCO: the same image ids, annotations in another order: pairing by id
        ann_order, pan_ids = [2, 0, 3, 1], [e['id'] for e in ds.roidb]
    empty = _write_gt(ds, chains, ann_order, pan_ids)
    del model
    torch.cuda.empty_cache()

    res = main(['--cfg', cfg, '--synthetic_weights', '--in-flight', '2'])
    with open(res['results_file'], 'rb') as f:
        got = pickle.load(f)
    assert res['results_file'] == os.path.join(str(tmp_path / 'output'), 'exp_eval', image_set, 'results', 'results_list.pkl')
    assert set(got) == {'all_boxes', 'all_masks', 'all_ssegs', 'all_panos', 'all_pano_cls_inds'}
    assert got['all_boxes'][0] == [] and got['all_masks'][0] == [] and len(got['all_boxes']) == ds.num_classes
    for k, ch in enumerate(chains):
        for c in range(1, ds.num_classes):
            b = got['all_boxes'][c][k]
            assert isinstance(b, np.ndarray) and b.dtype == ch['boxes'][c - 1].dtype
            assert np.array_equal(b, ch['boxes'][c - 1]), (k, c)
            assert got['all_masks'][c][k] == ch['masks'][c - 1], (k, c)
        for key, want in (('all_ssegs', ch['sseg']), ('all_panos', ch['pano']), ('all_pano_cls_inds', ch['cls'])):
            assert isinstance(got[key][k], np.ndarray) and got[key][k].dtype == want.dtype and np.array_equal(got[key][k], want), (key, k)
    n_det = sum(len(b) for ch in chains for b in ch['boxes'])
    assert n_det > 0 and sum(len(ch['cls']) for ch in chains) > 0

    m = res['metrics']
    for name, r in m['panoptic']['per_class'].items():
        if 'tp' in r:
            assert r['pq'] == 1.0 and r['sq'] == 1.0 and r['rq'] == 1.0, (name, r)
    present = [c for c in range(NUM_SEG) if any((ch['sseg'] == c).any() for ch in chains)]
    assert present and all(m['sseg']['IU_array'][c] == 1.0 for c in present)
    # box / mask AP: 1 for every category with detections (those with an empty mask have a detection without GT: left out)
    scored = [c for c in range(1, ds.num_classes) if any(len(ch['boxes'][c - 1]) for ch in chains) and c not in empty]
    assert scored
    results_dir = os.path.dirname(res['results_file'])
    for iou_type, segms in (('bbox', None), ('segm', got['all_masks'])):
        ev = ds._evaluate_detections(got['all_boxes'], segms, results_dir, iou_type)
        prec = ev.eval['precision']
        for c in scored:
            assert np.all(prec[:, :, c - 1, 0, -1] == 1.0), (iou_type, c)
    if not empty:
        assert m['box_ap'][0] == 1.0 and m['mask_ap'][0] == 1.0

    again = main(['--cfg', cfg, '--eval_only'])
    assert again['times'] is None
    e = again['metrics']
    assert np.array_equal(e['box_ap'], m['box_ap']) and np.array_equal(e['mask_ap'], m['mask_ap'])
    assert e['panoptic'] == m['panoptic']
    assert e['sseg']['meanIU'] == m['sseg']['meanIU'] and np.array_equal(e['sseg']['IU_array'], m['sseg']['IU_array'])
    assert np.array_equal(e['sseg']['confusion_matrix'], m['sseg']['confusion_matrix'])
