"""GPU: the merge kernels of test-time augmentation (csrc/tta.hip) against the numpy restatement of DESIGN.md 4.18 (tests/tta_ref.py),
bit for bit, on poisoned and guard-banded memory (tests/memguard.py, patterns A and B); the augmented forward against the plain
forward (base augmentation alone) and against the restatement applied to its own parts; the evaluation run with augmentation."""
import copy
import os
import pickle
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import memguard  # noqa: E402
import tta_ref   # noqa: E402

pytestmark = pytest.mark.gpu

F = np.float32
GUARDED = memguard.MODULES + ('upsnet_amd.tta',)


def dev(x):
    return torch.from_numpy(np.array(x, order='C', copy=True)).cuda()     # (a copy: a mirrored view of a size-1 axis keeps a negative stride)


def host(t):
    return t.detach().cpu().numpy()


def same_bits(got, want):
    """device tensor (any layout) against a numpy array, logical order, bitwise."""
    g = np.ascontiguousarray(host(got))
    return g.shape == want.shape and g.dtype == want.dtype and np.array_equal(g.view(np.uint8), np.ascontiguousarray(want).view(np.uint8))


def both_patterns(run):
    """run(pattern) under poisoned allocations and checked guard bands, once per pattern; the results must agree bitwise."""
    res = []
    for pattern in 'AB':
        with memguard.poisoned(pattern, modules=GUARDED):
            out = run(pattern)
            torch.cuda.synchronize()
        res.append([np.ascontiguousarray(host(t)) for t in (out if isinstance(out, (list, tuple)) else [out])])
    for a, b in zip(*res):
        assert a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8)), 'result depends on the poison pattern'
    return res[0]


def seg_input(m, pattern):
    """numpy [H,W,S] -> logical [1,S,H,W] device tensor with channels-last memory, inside poison bands."""
    return memguard.banded_copy(dev(m)[None].permute(0, 3, 1, 2), pattern)


# ------------------------------------------------------------------------------------------------ semantic merge
AUG_SCALES = [1.0, 0.75, 1.25, 0.5, 2.0, 1.0, 0.6, 1.7]      # q below and above 1


def seg_case(rng, S, Hb, Wb, A, cell):
    q, _ = tta_ref.ratios(AUG_SCALES[:A])
    maps, wr, flip = [], [], []
    for a in range(A):
        hs = Hb if a == 0 else max(1, int(round(Hb * float(q[a]))))
        ws = Wb if a == 0 else max(1, int(round(Wb * float(q[a]))))
        if A == 8 and a == 7:
            hs = ws = 1                                       # a 1 x 1 augmentation map
        maps.append(rng.normal(0, 5, (hs, ws, S)).astype(F))
        wr.append(F(cell * ws - (a % cell)))                  # cell 4: resized widths that are no multiple of the cell
        flip.append(a % 2 == 1)
    return maps, q, wr, flip


@pytest.mark.parametrize('cell', [4, 1])
@pytest.mark.parametrize('S', [1, 3, 19, 20])
def test_seg_merge_equals_the_restatement(S, cell):
    from upsnet_amd import ops
    rng = np.random.default_rng(S * 10 + cell)
    for Hb, Wb in ((1, 1), (5, 7), (8, 16)):
        for A in (1, 2, 8):
            maps, q, wr, flip = seg_case(rng, S, Hb, Wb, A, cell)
            want = tta_ref.seg_merge(maps, q, wr, flip, cell).transpose(2, 0, 1)[None]
            got, = both_patterns(lambda p: ops.tta_seg_merge([seg_input(m, p) for m in maps], q, wr, flip, cell))
            assert got.shape == want.shape and np.array_equal(got.view(np.uint8), np.ascontiguousarray(want).view(np.uint8)), (Hb, Wb, A)


def test_seg_merge_output_layout_and_more_than_one_block():
    """A grid of several workgroups in both forms (S = 20: 16-byte accesses; S = 19: scalar) and the result's layout."""
    from upsnet_amd import ops
    rng = np.random.default_rng(2)
    for S in (20, 19):
        maps, q, wr, flip = seg_case(rng, S, 24, 40, 4, 4)
        want = tta_ref.seg_merge(maps, q, wr, flip, 4).transpose(2, 0, 1)[None]
        out = ops.tta_seg_merge([dev(m)[None].permute(0, 3, 1, 2) for m in maps], q, wr, flip, 4)
        assert tuple(out.shape) == (1, S, 24, 40) and out.dtype == torch.float32
        assert out.permute(0, 2, 3, 1).is_contiguous()
        assert same_bits(out, want)


def test_seg_merge_unaligned_bases_take_the_scalar_form():
    """S % 4 == 0 but a map that starts 4 bytes off a 16-byte boundary: same bits through the scalar form."""
    from upsnet_amd import ops
    rng = np.random.default_rng(3)
    maps, q, wr, flip = seg_case(rng, 20, 5, 7, 2, 4)
    want = tta_ref.seg_merge(maps, q, wr, flip, 4).transpose(2, 0, 1)[None]
    ins = []
    for m in maps:
        buf = torch.zeros(m.size + 1, dtype=torch.float32, device='cuda')
        buf[1:].copy_(dev(m).reshape(-1))
        t = buf[1:].view(1, *m.shape).permute(0, 3, 1, 2)
        assert t.data_ptr() % 16 == 4
        ins.append(t)
    assert same_bits(ops.tta_seg_merge(ins, q, wr, flip, 4), want)


@pytest.mark.parametrize('cell', [4, 1])
def test_seg_merge_hand_properties_as_byte_equality(cell):
    from upsnet_amd import ops
    rng = np.random.default_rng(4 + cell)
    for shape in ((1, 1, 1), (5, 7, 3), (8, 16, 19), (8, 16, 20)):
        m = rng.normal(0, 4, shape).astype(F)
        want = m.transpose(2, 0, 1)[None]
        wr = F(cell * shape[1])
        one, = both_patterns(lambda p: ops.tta_seg_merge([seg_input(m, p)], [F(1)], [wr], [False], cell))
        assert np.array_equal(one.view(np.uint8), np.ascontiguousarray(want).view(np.uint8))
        mirror = np.ascontiguousarray(m[:, ::-1])
        two, = both_patterns(lambda p: ops.tta_seg_merge([seg_input(m, p), seg_input(mirror, p)], [F(1), F(1)], [wr, wr],
                                                         [False, True], cell))
        assert np.array_equal(two.view(np.uint8), np.ascontiguousarray(want).view(np.uint8))


def test_wrappers_refuse_bad_arguments():
    from upsnet_amd import ops
    m = torch.zeros((1, 3, 4, 4), device='cuda')
    with pytest.raises(ValueError):
        ops.tta_seg_merge([m] * 9, [1.0] * 9, [16.0] * 9, [False] * 9, 4)
    with pytest.raises(ValueError):
        ops.tta_seg_merge([], [], [], [], 4)
    with pytest.raises(ValueError):
        ops.tta_seg_merge([m, torch.zeros((1, 4, 4, 4), device='cuda')], [1.0] * 2, [16.0] * 2, [False] * 2, 4)
    with pytest.raises(RuntimeError, match='cell'):
        ops.tta_seg_merge([m], [1.0], [16.0], [False], 2)
    with pytest.raises(Exception):
        ops.tta_seg_merge([m.cpu()], [1.0], [16.0], [False], 4)
    n = torch.zeros((1,), dtype=torch.int32, device='cuda')
    r, d, p = torch.zeros((1100, 5), device='cuda'), torch.zeros((1100, 36), device='cuda'), torch.zeros((1100, 9), device='cuda')
    with pytest.raises(ValueError, match='8192'):
        ops.tta_roi_union([r] * 8, [d] * 8, [p] * 8, [n] * 8, [1.0] * 8, [100.0] * 8, [False] * 8)


# ------------------------------------------------------------------------------------------------ proposal union
def union_case(rng, R, C, counts, scales, flips):
    A = len(counts)
    _, r = tta_ref.ratios(scales)
    rois, delta, prob, wr = [], [], [], []
    for a in range(A):
        w = F(np.rint(640 * scales[a]))
        x = np.sort(rng.uniform(0, float(w) - 1, (R, 2)), 1)
        y = np.sort(rng.uniform(0, 300, (R, 2)), 1)
        # (rows past the count hold values too: they must not reach the output)
        rois.append(np.stack([np.zeros(R), x[:, 0], y[:, 0], x[:, 1], y[:, 1]], 1).astype(F))
        delta.append(rng.normal(0, 1, (R, 4 * C)).astype(F))
        prob.append(rng.uniform(0, 1, (R, C)).astype(F))
        wr.append(w)
    return rois, delta, prob, r, wr


@pytest.mark.parametrize('R,C', [(8, 9), (8, 81), (1000, 9), (1000, 81)])
def test_roi_union_equals_the_restatement(R, C):
    from upsnet_amd import ops
    rng = np.random.default_rng(R + C)
    cases = [
        ([0, 1, R], [1.0, 0.75, 1.25], [False, True, False]),
        ([R, 0, 1], [1.0, 1.0, 0.75], [False, True, True]),
        ([1, R, 0, R // 2], [1.0, 1.25, 0.5, 2.0], [False, False, True, True]),
        ([0, 0, 0], [1.0, 0.75, 1.25], [False, True, False]),
        ([R], [1.0], [False]),
        ([R, R - 1, 0, 1, R, 3 % (R + 1), R, R], [1.0, 1.0, 0.75, 0.75, 1.25, 1.25, 0.5, 2.0], [False, True] * 4),
    ]
    for counts, scales, flips in cases:
        rois, delta, prob, r, wr = union_case(rng, R, C, counts, scales, flips)
        want = tta_ref.roi_union(rois, delta, prob, counts, r, wr, flips)

        def run(p):
            b = lambda xs: [memguard.banded_copy(dev(x), p) for x in xs]
            nd = [memguard.banded_copy(torch.tensor([c], dtype=torch.int32, device='cuda'), p) for c in counts]
            return ops.tta_roi_union(b(rois), b(delta), b(prob), nd, r, wr, flips)
        g_r, g_d, g_p, g_n = both_patterns(run)
        A = len(counts)
        assert g_r.shape == (A * R, 5) and g_d.shape == (A * R, 4 * C) and g_p.shape == (A * R, C)
        assert g_n.dtype == np.int32 and int(g_n[0]) == want[3] == sum(counts)
        for g, w in zip((g_r, g_d, g_p), want[:3]):
            assert g.dtype == np.float32 and np.array_equal(g.view(np.uint8), w.view(np.uint8)), (counts,)
        assert not g_r[want[3]:].any() and not g_d[want[3]:].any() and not g_p[want[3]:].any()


def test_roi_union_clamps_counts_to_the_capacity():
    """A device count outside 0..R (never produced by the proposal op) is clamped, so no row is read past an input."""
    from upsnet_amd import ops
    rng = np.random.default_rng(9)
    R, C = 8, 9
    rois, delta, prob, r, wr = union_case(rng, R, C, [R, R], [1.0, 0.75], [False, True])
    want = tta_ref.roi_union(rois, delta, prob, [R, 0], r, wr, [False, True])

    def run(p):
        b = lambda xs: [memguard.banded_copy(dev(x), p) for x in xs]
        nd = [torch.tensor([c], dtype=torch.int32, device='cuda') for c in (R + 5, -3)]
        return ops.tta_roi_union(b(rois), b(delta), b(prob), nd, r, wr, [False, True])
    g_r, g_d, g_p, g_n = both_patterns(run)
    assert int(g_n[0]) == R
    assert np.array_equal(g_r.view(np.uint8), want[0].view(np.uint8)) and np.array_equal(g_d.view(np.uint8), want[1].view(np.uint8))


# ------------------------------------------------------------------------------------------------ final boxes and mask logits
@pytest.mark.parametrize('n', [0, 1, 100])
def test_boxes_to_aug_equals_the_restatement(n):
    from upsnet_amd import ops
    rng = np.random.default_rng(20 + n)
    x = np.sort(rng.uniform(0, 480, (n, 2)), 1)
    y = np.sort(rng.uniform(0, 255, (n, 2)), 1)
    boxes = np.stack([np.zeros(n), x[:, 0], y[:, 0], x[:, 1], y[:, 1]], 1).astype(F)
    scales = [1.024, 1.024, 0.768, 1.28, 0.5]
    q, _ = tta_ref.ratios(scales)
    wr, flip = [F(481), F(481), F(361), F(602), F(235)], [False, True, False, True, True]
    want = tta_ref.boxes_to_aug(boxes, q, wr, flip)
    got, = both_patterns(lambda p: ops.tta_boxes_to_aug(memguard.banded_copy(dev(boxes), p) if n else dev(boxes), q, wr, flip))
    assert got.shape == (5, n, 5) and got.dtype == np.float32 and np.array_equal(got.view(np.uint8), want.view(np.uint8))
    if n:
        assert np.array_equal(got[0].view(np.uint8), boxes.view(np.uint8))     # q = 1, no flip: the identity


@pytest.mark.parametrize('channels_last', [False, True])
@pytest.mark.parametrize('n', [0, 1, 100])
def test_mask_merge_equals_the_restatement(n, channels_last):
    from upsnet_amd import ops
    rng = np.random.default_rng(30 + n)
    C, ms = 9, 28
    for flip in ([False], [False, True], [False, False, True, True, False], [True] * 8, [False] * 3):
        logits = [rng.normal(0, 3, (n, C, ms, ms)).astype(F) for _ in flip]
        want = tta_ref.mask_merge(logits, flip)

        def run(p):
            ins = [dev(L) for L in logits]
            if channels_last:
                ins = [t.contiguous(memory_format=torch.channels_last) for t in ins]
            if n:
                ins = [memguard.banded_copy(t, p) for t in ins]
            return ops.tta_mask_merge(ins, flip)
        got, = both_patterns(run)
        assert got.shape == (n, C, ms, ms) and got.dtype == np.float32
        assert np.array_equal(got.view(np.uint8), np.ascontiguousarray(want).view(np.uint8)), (flip,)
    if n:
        L = logits[0]
        out = ops.tta_mask_merge([dev(L), dev(np.ascontiguousarray(L[..., ::-1]))], [False, True])
        assert same_bits(out, L)                      # a plane and its mirror as the flipped augmentation: the plane itself


# ------------------------------------------------------------------------------------------------ the model
IMAGE_HW = (250, 470)       # under scales 256 / max size 512: resized 256 x 481 (padded to 512), im_scale 1.024


@pytest.fixture(scope='module')
def tta_model():
    from upsnet_amd.config.config import config, update_config_dict, CITYSCAPES_R50
    from upsnet_amd.synthetic import build_model
    saved = copy.deepcopy(dict(config))
    update_config_dict(CITYSCAPES_R50)
    update_config_dict(dict(test=dict(scales=[256], max_size=512, aug_scales=[], aug_flip=False)))
    model = build_model(device='cuda')
    yield model
    del model
    config.clear()
    config.update(saved)
    torch.cuda.empty_cache()


def test_base_augmentation_alone_equals_the_plain_forward(tta_model):
    from upsnet_amd.dataset.blob import get_image_blob
    from upsnet_amd.synthetic import make_image_u8
    from upsnet_amd.tta import augmentation_list
    assert augmentation_list() == [(256, 512, False)]
    img = make_image_u8(*IMAGE_HW, seed=5, device='cuda')
    data = get_image_blob(img)
    assert tuple(data['im_info'][0][:2]) == (256.0, 481.0)
    with torch.no_grad():
        want = tta_model({'data': data['data'], 'im_info': data['im_info']})
    got = tta_model.forward_tta(img)
    assert set(got) == set(want)
    assert want['cls_inds'].numel() > 0 and want['panoptic_cls_inds'].numel() > 0
    for k in want:
        assert memguard.bit_equal(got[k].contiguous(), want[k].contiguous()), k


def _hwc(t):
    return np.ascontiguousarray(host(t)[0].transpose(1, 2, 0))


def test_augmented_forward_equals_the_restatement_on_its_parts(tta_model, monkeypatch):
    from upsnet_amd import tta
    from upsnet_amd.dataset.blob import get_image_blob
    from upsnet_amd.synthetic import make_image_u8
    augs = [(256, 512, False), (256, 512, True), (192, 384, False), (320, 640, False)]
    monkeypatch.setattr(tta, 'augmentation_list', lambda cfg=None: list(augs))
    img = make_image_u8(*IMAGE_HW, seed=5, device='cuda')
    with memguard.poisoned('A', modules=GUARDED):
        out, parts = tta_model.forward_tta(img, return_parts=True)
        torch.cuda.synchronize()
    A = len(augs)
    assert parts['augs'] == augs and [tuple(i[:2]) for i in parts['im_info']] == [(256, 481), (256, 481), (192, 361), (320, 602)]
    q, r = tta_ref.ratios([i[2] for i in parts['im_info']])
    wr, flip, cell = [F(i[1]) for i in parts['im_info']], [a[2] for a in augs], parts['cell']
    assert [float(v) for v in parts['q']] == [float(v) for v in q] and [float(v) for v in parts['r']] == [float(v) for v in r]

    # 1. semantic scores
    want = tta_ref.seg_merge([_hwc(s) for s in parts['score']], q, wr, flip, cell)
    assert same_bits(parts['merged_score'], want.transpose(2, 0, 1)[None])
    # 2. proposal union
    counts = [int(n.item()) for n in parts['n_rois']]
    assert all(c > 0 for c in counts)
    w_r, w_d, w_p, w_n = tta_ref.roi_union([host(t) for t in parts['rois']], [host(t) for t in parts['delta']],
                                           [host(t) for t in parts['prob']], counts, r, wr, flip)
    assert int(parts['merged_n_rois'].item()) == w_n == sum(counts) > counts[0]
    assert same_bits(parts['merged_rois'], w_r) and same_bits(parts['merged_delta'], w_d) and same_bits(parts['merged_prob'], w_p)
    # 3. final boxes and mask logits
    n_det, n_pan, n_extra = parts['n_det'], parts['n_pan'], parts['n_extra']
    assert n_det > 0 and n_pan > 0
    boxes = host(parts['boxes'])
    assert boxes.shape == (n_det + n_extra, 5)
    assert np.array_equal(boxes[:n_det], host(parts['det_boxes'])) and np.array_equal(boxes[n_det:], host(parts['extra_boxes'][:n_extra]))
    assert same_bits(parts['boxes_aug'], tta_ref.boxes_to_aug(boxes, q, wr, flip))
    assert len(parts['mask_logits']) == A
    assert same_bits(parts['merged_mask_logits'], tta_ref.mask_merge([host(t) for t in parts['mask_logits']], flip))

    # 4. the existing tail (the eager continuation of _forward_fused) on the merged tensors
    merged = parts['merged_mask_logits']
    if n_extra:   # the continuation would run the mask head on the extra boxes: hand it the merged rows instead
        monkeypatch.setattr(type(tta_model.mask_branch), 'forward', lambda self, feats, b: merged[n_det:n_det + b.shape[0]])
    st = dict(feats=parts['feats'][0], fuse_up=cell == 4, fcn=parts['merged_score'], tail=None,
              nums=torch.tensor([n_det, n_pan, n_extra], dtype=torch.int32), det_boxes=parts['det_boxes'], det_scores=parts['det_scores'],
              det_cls=parts['det_cls'], pan_boxes=parts['pan_boxes'], pan_scores=parts['pan_scores'], pan_cls=parts['pan_cls'],
              pan_row=parts['pan_row'], extra_boxes=parts['extra_boxes'], mask_det=merged, max_det=merged.shape[0],
              rois=parts['merged_rois'], n_rois=parts['merged_n_rois'])
    data = get_image_blob(img)
    with torch.no_grad():
        want_out = tta_model._forward_fused({'data': data['data'], 'im_info': data['im_info']}, st=st, try_graph=False)
        plain = tta_model({'data': data['data'], 'im_info': data['im_info']})
    assert set(out) == set(want_out) == set(plain)
    for k in out:
        assert memguard.bit_equal(out[k].contiguous(), want_out[k].contiguous()), k
        assert out[k].dtype == plain[k].dtype and out[k].dim() == plain[k].dim() and out[k].shape[1:] == plain[k].shape[1:], k
    assert out['fcn_outputs'].shape == plain['fcn_outputs'].shape and out['panoptic_outputs'].shape == plain['panoptic_outputs'].shape
    assert out['mask_probs'].shape[0] == out['pred_boxes'].shape[0] == out['cls_inds'].shape[0] == n_det


def test_forward_tta_refuses_keep_proposals(tta_model):
    from upsnet_amd.synthetic import make_image_u8
    tta_model.keep_proposals = True
    try:
        with pytest.raises(ValueError, match='proposal'):
            tta_model.forward_tta(make_image_u8(64, 64, seed=1, device='cuda'))
    finally:
        tta_model.keep_proposals = False


# ------------------------------------------------------------------------------------------------ the evaluation run
def test_evaluate_main_with_augmentation(tta_model, tmp_path):
    from test_dataset_run_cpu import make_dataset, write_cfg
    from test_dataset_run_gpu import _direct_chain, _write_gt
    from upsnet_amd.config.config import config, update_config
    from upsnet_amd.dataset import Cityscapes
    from upsnet_amd.evaluate import main
    saved = copy.deepcopy(dict(config))
    try:
        sizes = [(256, 512), (128, 256)]
        root = str(tmp_path / 'Cityscapes')
        make_dataset(root, 'Cityscapes', sizes, seed=11)
        cfg = write_cfg(tmp_path, 'Cityscapes', root, 'val')
        update_config(cfg)
        ds = Cityscapes(image_sets=['val'], phase='test')
        # ground truth = the plain single-scale chain's own output (as tests/test_dataset_run_gpu.py builds it)
        chains = [_direct_chain(tta_model, e['image'], ds.num_classes) for e in ds.roidb]
        _write_gt(ds, chains, list(range(len(sizes))), ['img_%d' % e['id'] for e in ds.roidb])

        res = main(['--cfg', cfg, '--synthetic_weights', '--aug_scales', '192', '--aug_flip'])
        with open(res['results_file'], 'rb') as f:
            got = pickle.load(f)
        assert got['test_aug'] == [[256, 512, False], [256, 512, True], [192, 384, False], [192, 384, True]]
        assert set(got) == {'all_boxes', 'all_masks', 'all_ssegs', 'all_panos', 'all_pano_cls_inds', 'test_aug'}
        n = len(sizes)
        assert len(got['all_ssegs']) == len(got['all_panos']) == len(got['all_pano_cls_inds']) == n
        # base frame, restored to the original image size; the results follow the roidb (ascending image id, make_dataset numbers the
        # images in descending order)
        assert sorted((e['height'], e['width']) for e in ds.roidb) == sorted(sizes)
        for k, e in enumerate(ds.roidb):
            assert got['all_ssegs'][k].shape == (e['height'], e['width']) and got['all_panos'][k].shape == (e['height'], e['width'])
        assert all(len(got['all_boxes'][c]) == n for c in range(1, ds.num_classes))
        m = res['metrics']
        assert {'box_ap', 'mask_ap', 'panoptic', 'sseg'} <= set(m)
        assert 0.0 <= m['sseg']['meanIU'] <= 1.0 and np.isfinite(m['sseg']['meanIU'])
        assert len(res['times']['net_time']) == n
    finally:
        config.clear()
        config.update(saved)
