"""GPU: the soft detection selection (csrc/detect.hip mroi_soft_kernel). ops.mask_roi_soft against the numpy
restatement of the rule (tests/soft_select_ref.py), bit for bit over every defined row, on poisoned and guard-banded memory
(tests/memguard.py, patterns A and B); the soft augmented forward against the restatement applied to its own parts; the evaluation run
with --soft_nms."""
import copy
import os
import pickle
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import memguard       # noqa: E402
import box_vote_ref as bref   # noqa: E402
import soft_select_ref as ref   # noqa: E402

pytestmark = pytest.mark.gpu

F = np.float32
GUARDED = memguard.MODULES + ('upsnet_amd.tta',)
ST, NT, SIGMA, FLOOR = 0.05, 0.5, 0.5, 1e-4
KEYS = ('boxes', 'scores', 'cls', 'src')


def dev(x):
    return torch.from_numpy(np.array(x, order='C', copy=True)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def bits_equal(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def device_select(rois, delta, prob, n, clip, max_det, method, sigma=SIGMA, floor=FLOOR, st=ST, nt=NT, defined=None):
    """ops.mask_roi_soft on banded copies of the inputs under both poison patterns: dict(boxes, scores, cls, src) cut to the `defined`
    rows (rows past them are the allocator's, here poison), num."""
    from upsnet_amd import ops
    res = []
    for p in 'AB':
        with memguard.poisoned(p, modules=GUARDED):
            b = lambda x: memguard.banded_copy(dev(x), p)
            out = ops.mask_roi_soft(b(rois), b(delta), b(prob), b(bref.IM_INFO), st, nt, max_det, bref.REG_WEIGHTS, method, sigma, floor,
                                    num_rois_dev=b(np.array([n], np.int32)), clip_boxes=clip)
            torch.cuda.synchronize()
        res.append([np.ascontiguousarray(host(t)) for t in out])
    N, C = prob.shape
    assert res[0][0].shape == ((C - 1) * N, 5) and all(r.shape == ((C - 1) * N,) for r in res[0][1:4])
    assert [r.dtype for r in res[0]] == [np.float32, np.float32, np.int64, np.int32, np.int32]
    num = int(res[0][4][0])
    d = defined if defined is not None else max(abs(num), min((C - 1) * N, max(max_det, ref.FILL)))
    for a, b_, k in zip(res[0][:4], res[1][:4], KEYS):
        assert bits_equal(a[:d], b_[:d]), 'the defined rows of %s depend on the poison pattern' % k
    assert num == int(res[1][4][0])
    return dict(zip(KEYS, (r[:d] for r in res[0][:4])), num=num)


def assert_equal(got, want, what):
    assert got['num'] == want['num'], (what, got['num'], want['num'])
    for k in KEYS:
        assert bits_equal(got[k], want[k]), (what, k)


# ------------------------------------------------------------------------------------------------ the kernel against the rule
@pytest.mark.parametrize('C', [2, 9, 81])
@pytest.mark.parametrize('N', [1, 63, 64, 65, 200, 1000, 1024, 1025])
def test_soft_selection_equals_the_restatement(N, C):
    """Methods 0, 1, 2 x max_det 100, 0, 1000 with the device row count n = N - 7 (the rows past it are good candidates that must not
    enter; at N = 1 also n = 1), clip on and off alternating. 1024 is the last size on one wavefront, 1025 the first on four.
    So that the comparison cannot pass on undecayed rows alone: for the soft methods, from N = 64 on and whenever C <= 9 or max_det is
    0 or 1000, at least a quarter of the returned rows carry a score that is no longer prob[src, cls]. With C = 81 and max_det = 100
    no returned row is decayed -- the 400 cluster winners (5 clusters x 80 classes) fill the 100 rows -- which is expected."""
    rng = np.random.default_rng(5)
    rois, delta, prob = ref.cluster_inputs(rng, N, C)
    i = 0
    for n in ((N - 7, 1) if N == 1 else (N - 7,)):
        cands = {clip: ref.candidates(rois, delta, prob, n, bref.IM_INFO, bref.REG_WEIGHTS, clip, ST) for clip in (True, False)}
        for method in (0, 1, 2):
            for max_det in (100, 0, 1000):
                clip = bool((i + 1) % 2)
                i += 1
                want = ref.soft_select(rois, delta, prob, n, bref.IM_INFO, bref.REG_WEIGHTS, clip, ST, NT, max_det, method, SIGMA, FLOOR,
                                       cands=cands[clip])
                got = device_select(rois, delta, prob, n, clip, max_det, method, defined=len(want['scores']))
                assert_equal(got, want, (n, method, max_det, clip))
                k = want['num']
                assert k > 0 and (n > 0 or (k == 1 and want['cls'][0] == 0))
                dec = int(ref.decayed(want, prob).sum())
                if method == 0 or (C == 81 and max_det == 100 and N >= 64):
                    assert dec == 0
                elif N >= 64:
                    assert 4 * dec >= k, (method, max_det, dec, k)


@pytest.mark.parametrize('method', [1, 2])
def test_duplicated_rows_exact_score_ties(method):
    """Every row twice (the same box and probabilities at rows r and r + 100): the arg-max meets exact ties (the first position wins),
    and a duplicate has IoU 1 with its original (linear: weight 0, dropped below the floor; gaussian: x exp(-2), kept)."""
    rng = np.random.default_rng(21)
    rois, delta, prob = ref.cluster_inputs(rng, 100, 9)
    rois, delta, prob = np.concatenate([rois, rois]), np.concatenate([delta, delta]), np.concatenate([prob, prob])
    for max_det in (100, 0):
        want = ref.soft_select(rois, delta, prob, 200, bref.IM_INFO, bref.REG_WEIGHTS, True, ST, NT, max_det, method, SIGMA, FLOOR)
        got = device_select(rois, delta, prob, 200, True, max_det, method, defined=len(want['scores']))
        assert_equal(got, want, (method, max_det))
        src = want['src'][:want['num']] + 1000 * want['cls'][:want['num']]      # (class, row)
        both = np.intersect1d(src[src % 1000 < 100] + 100, src[src % 1000 >= 100])     # rows that came back together with their duplicate
        assert (len(both) > 0) == (method == 2)


def test_nothing_above_the_threshold_and_no_rows_give_the_dummy_row():
    rng = np.random.default_rng(22)
    rois, delta, prob = ref.cluster_inputs(rng, 200, 9)
    low = (prob * F(0.04)).astype(F)
    for p, n in ((low, 200), (prob, 0), (prob, -5)):
        want = ref.soft_select(rois, delta, p, n, bref.IM_INFO, bref.REG_WEIGHTS, True, ST, NT, 100, 1, SIGMA, FLOOR)
        assert want['num'] == 1 and want['scores'][0] == 1 and want['cls'][0] == 0 and len(want['scores']) == 256
        assert_equal(device_select(rois, delta, p, n, True, 100, 1, defined=256), want, n)


def _limit_case(k):
    """N = 4200 rows, two classes, exactly k rows of class 1 above the score threshold (in random places)."""
    rng = np.random.default_rng(23)
    N = 4200
    rois, delta, prob = ref.cluster_inputs(rng, N, 2, distinct=False)
    prob[:, 1] = F(0.01)
    rows = rng.permutation(N)[:k]
    prob[rows, 1] = rng.uniform(0.06, 1.0, k).astype(F)
    return rois, delta, prob


def test_a_class_of_exactly_4096_candidates():
    rois, delta, prob = _limit_case(4096)
    want = ref.soft_select(rois, delta, prob, 4200, bref.IM_INFO, bref.REG_WEIGHTS, True, ST, NT, 100, 1, SIGMA, FLOOR)
    assert want['per_class'] == [4096] and want['num'] > 0
    assert_equal(device_select(rois, delta, prob, 4200, True, 100, 1, defined=len(want['scores'])), want, 4096)


def test_a_class_of_4097_candidates_is_a_handled_overflow():
    from upsnet_amd.operators.modules.mask_roi import MaskROI
    rois, delta, prob = _limit_case(4097)
    want = ref.soft_select(rois, delta, prob, 4200, bref.IM_INFO, bref.REG_WEIGHTS, True, ST, NT, 100, 1, SIGMA, FLOOR)
    assert want['per_class'] == [4097] and want['num'] < 0
    got = device_select(rois, delta, prob, 4200, True, 100, 1, defined=len(want['scores']))
    assert_equal(got, want, 4097)                               # negative count, the first 4096 candidates selected: all rows defined
    module = MaskROI(True, False, 100, 2, nms_thresh=NT, score_thresh=ST, soft_nms=(1, SIGMA, FLOOR))
    with pytest.raises(RuntimeError, match='4096'):
        module(dev(rois), dev(delta), dev(prob), bref.IM_INFO)
    # ... and with one candidate fewer the module returns the selection
    rois, delta, prob = _limit_case(4096)
    scores, boxes, cls = module(dev(rois), dev(delta), dev(prob), bref.IM_INFO)
    assert scores.shape[0] == boxes.shape[0] == cls.shape[0] > 0


def test_method_zero_equals_the_hard_selection_on_the_device():
    """On inputs whose pair IoUs keep a margin to the threshold and whose scores are distinct (asserted in
    test_soft_select_cpu.test_method_zero_is_the_hard_selection for these very inputs)."""
    from upsnet_amd import ops
    for N, C, max_det in ((200, 9, 100), (300, 81, 100), (300, 81, 1000)):
        rng = np.random.default_rng(5)
        rois, delta, prob = ref.cluster_inputs(rng, N, C)
        nd = dev(np.array([N - 7], np.int32))
        hard = ops.mask_roi(dev(rois), dev(delta), dev(prob), dev(bref.IM_INFO), False, ST, NT, max_det, bref.REG_WEIGHTS, nd)
        soft = ops.mask_roi_soft(dev(rois), dev(delta), dev(prob), dev(bref.IM_INFO), ST, NT, max_det, bref.REG_WEIGHTS, 0, SIGMA, FLOOR, nd)
        k = int(hard[4].item())
        assert k == int(soft[4].item()) > 0
        d = max(k, max(max_det, 256))
        for a, b in zip(hard[:3], soft[:3]):                     # boxes, scores, classes (and the zero rows after them)
            assert memguard.bit_equal(a[:d], b[:d])
        assert memguard.bit_equal(hard[3][:k], soft[3][:k])


def test_soft_nms_batched_still_equals_the_oracle():
    """The trips moved into a header shared with the selection: the stand-alone entry point on one wavefront and on four."""
    import oracle
    from upsnet_amd import ops
    rng = np.random.default_rng(24)
    for n, method in ((300, 1), (1500, 2)):
        rois, delta, prob = ref.cluster_inputs(rng, n, 2)
        dets, _ = ref.candidates(rois, delta, prob, n, bref.IM_INFO, bref.REG_WEIGHTS, True, ST)[1]
        want, inds = oracle.soft_nms(dets, sigma=SIGMA, Nt=NT, threshold=FLOOR, method=method)
        b, i, cnt = ops.soft_nms_batched(dev(dets)[None], None, SIGMA, NT, FLOOR, method)
        k = int(cnt[0].item())
        assert k == len(inds) > 5
        assert bits_equal(host(b[0, :k]), want[:k]) and np.array_equal(host(i[0, :k]), inds)


def test_wrappers_refuse_bad_arguments():
    from upsnet_amd import ops
    from upsnet_amd.bbox.bbox_transform import soft_nms
    rng = np.random.default_rng(25)
    rois, delta, prob = (dev(x) for x in ref.cluster_inputs(rng, 20, 3))
    im = dev(bref.IM_INFO)
    tail = (ST, NT, 100, bref.REG_WEIGHTS)
    with pytest.raises(RuntimeError, match='method'):
        ops.mask_roi_soft(rois, delta, prob, im, *tail, 3, SIGMA, FLOOR)
    with pytest.raises(RuntimeError, match='sigma'):
        ops.mask_roi_soft(rois, delta, prob, im, *tail, 2, 0.0, FLOOR)
    with pytest.raises(ValueError):
        ops.mask_roi_soft(rois, delta[:, :4], prob, im, *tail, 1, SIGMA, FLOOR)
    with pytest.raises(ValueError):
        ops.mask_roi_soft(rois, delta, prob, im, *tail, 1, SIGMA, FLOOR, num_rois_dev=torch.tensor([20], device='cuda'))
    with pytest.raises(Exception):
        ops.mask_roi_soft(rois.cpu(), delta, prob, im, *tail, 1, SIGMA, FLOOR)
    # the reference-shaped wrapper: Detectron's soft_nms on the hand case of the CPU tests (A, C, then B at 0.8 * 0.5)
    dets = np.array([[0, 0, 9, 9, 0.9], [0, 0, 9, 4, 0.8], [100, 100, 109, 109, 0.7]], F)
    out, keep = soft_nms(dets, overlap_thresh=0.3, method='linear')
    assert keep.tolist() == [0, 2, 1] and bits_equal(out[:, 4], np.array([F(0.9), F(0.7), F(0.8) * F(0.5)], F))


# ------------------------------------------------------------------------------------------------ the model
IMAGE_HW = (250, 470)       # under scales 256 / max size 512: resized 256 x 481 (padded to 512), im_scale 1.024


def _sixtieth_score(off_parts):
    """The 60th largest score of the hard class-wise selection (100 rows, distinct scores): a threshold that leaves 59 winners."""
    scores = np.sort(host(off_parts['det_scores']))[::-1]
    assert len(scores) == 100 and scores[58] > scores[59] > 0.05
    return float(scores[59])


AUG_LISTS = {'base': [(256, 512, False)], 'three': [(256, 512, False), (256, 512, True), (192, 384, False)]}


@pytest.fixture(scope='module')
def soft_model():
    from upsnet_amd.config.config import config, update_config_dict, CITYSCAPES_R50
    from upsnet_amd.synthetic import build_model
    saved = copy.deepcopy(dict(config))
    update_config_dict(CITYSCAPES_R50)
    update_config_dict(dict(test=dict(scales=[256], max_size=512, aug_scales=[], aug_flip=False, bbox_vote=False, bbox_vote_thresh=0.5,
                                      soft_nms=False, soft_nms_method='linear', soft_nms_sigma=0.5, soft_nms_score_thresh=0.0001)))
    model = build_model(device='cuda')
    yield model
    del model
    config.clear()
    config.update(saved)
    torch.cuda.empty_cache()


def _selected_by_the_rule(model, parts):
    from upsnet_amd.config.config import config
    method, sigma, floor = parts['soft_nms']
    return ref.soft_select(host(parts['merged_rois']), host(parts['merged_delta']), host(parts['merged_prob']),
                           int(parts['merged_n_rois'].item()), parts['im_info'][0], config.network.bbox_reg_weights,
                           bool(model.mask_roi.clip_boxes), model.mask_roi.score_thresh, model.mask_roi.nms_thresh, config.test.max_det,
                           method, sigma, floor)


@pytest.mark.parametrize('method', ['linear', 'gaussian'])
@pytest.mark.parametrize('augs', ['base', 'three'])
def test_soft_forward_equals_the_restatement_on_its_parts(soft_model, monkeypatch, augs, method):
    from upsnet_amd import ops, tta
    from upsnet_amd.config.config import config
    from upsnet_amd.synthetic import make_image_u8
    monkeypatch.setattr(tta, 'augmentation_list', lambda cfg=None: list(AUG_LISTS[augs]))
    monkeypatch.setitem(config.test, 'soft_nms_method', method)
    img = make_image_u8(*IMAGE_HW, seed=5, device='cuda')

    # soft-NMS off: not one soft call, and (base augmentation alone) the plain forward
    monkeypatch.setitem(config.test, 'soft_nms', False)
    calls = []
    real = ops.mask_roi_soft
    monkeypatch.setattr(ops, 'mask_roi_soft', lambda *a, **kw: calls.append(1) or real(*a, **kw))
    off, off_parts = soft_model.forward_tta(img, return_parts=True)
    assert not calls and off_parts['soft_nms'] is None
    if augs == 'base' and method == 'linear':
        from upsnet_amd.dataset.blob import get_image_blob
        data = get_image_blob(img)
        with torch.no_grad():
            plain = soft_model({'data': data['data'], 'im_info': data['im_info']})
        assert set(off) == set(plain)
        for k in plain:
            assert memguard.bit_equal(off[k].contiguous(), plain[k].contiguous()), k

    # The synthetic model puts several hundred hard winners above 0.4 on this image, and a linearly decayed score is below half its
    # probability: at test.score_thresh the first max_det = 100 rows would all be undecayed winners. With the class-wise selection's
    # own threshold at the 60th hard score, 59 winners remain and decayed rows are returned beside them (asserted below); the
    # panoptic selection keeps its threshold.
    monkeypatch.setattr(soft_model.mask_roi, 'score_thresh', _sixtieth_score(off_parts))
    off, off_parts = soft_model.forward_tta(img, return_parts=True)
    assert not calls and off_parts['n_det'] == 59

    # soft-NMS on
    monkeypatch.setitem(config.test, 'soft_nms', True)
    with memguard.poisoned('A', modules=GUARDED):
        out, parts = soft_model.forward_tta(img, return_parts=True)
        torch.cuda.synchronize()
    assert len(calls) == 1
    assert parts['soft_nms'] == (tta.SOFT_NMS_METHODS[method], 0.5, 0.0001)
    n_det, n_pan, n_extra = parts['n_det'], parts['n_pan'], parts['n_extra']
    assert n_det > 0 and n_pan > 0
    # 1. the class-wise selection is the rule applied to the merged union
    want = _selected_by_the_rule(soft_model, parts)
    assert want['num'] == n_det
    assert bits_equal(host(parts['det_boxes']), want['boxes'][:n_det]) and bits_equal(host(parts['det_scores']), want['scores'][:n_det])
    assert bits_equal(host(parts['det_cls']), want['cls'][:n_det])
    dec = ref.decayed(want, host(parts['merged_prob']))
    print('hard rows %d, soft rows %d of T = %d, decayed %d' % (off_parts['n_det'], n_det, want['T'], int(dec.sum())))
    assert n_det > off_parts['n_det']
    assert dec.any(), 'no returned detection carries a decayed score: the soft rule was not exercised'
    # 2. the panoptic selection is the hard one, untouched
    for k in ('pan_boxes', 'pan_scores', 'pan_cls'):
        assert memguard.bit_equal(parts[k], off_parts[k]), k
    assert n_pan == off_parts['n_pan']
    # 3. the mask head's rows: the soft detections, then the panoptic rows the dedup did not pair; paired rows carry equal boxes
    boxes, pan_row = host(parts['boxes']), host(parts['pan_row'])[:n_pan]
    assert boxes.shape == (n_det + n_extra, 5)
    assert bits_equal(boxes[:n_det], want['boxes'][:n_det]) and bits_equal(boxes[pan_row], host(parts['pan_boxes']))
    paired = pan_row < n_det
    assert np.array_equal(want['cls'][:n_det][pan_row[paired]], host(parts['pan_cls'])[paired])
    # 4. the outputs are the tail on the merged tensors and these selections
    with torch.no_grad():
        want_out = tta._tail(soft_model, parts['merged_score'], parts['cell'] == 4, parts['merged_mask_logits'], n_det, n_pan,
                             parts['det_boxes'], parts['det_scores'], parts['det_cls'], parts['pan_boxes'], parts['pan_scores'],
                             parts['pan_cls'], parts['pan_row'])
    assert set(out) == set(want_out) == set(off)
    for k in out:
        assert memguard.bit_equal(out[k].contiguous(), want_out[k].contiguous()), k
    assert bits_equal(host(out['cls_probs']), want['scores'][:n_det])         # the decayed scores
    assert out['mask_probs'].shape[0] == n_det
    # 5. the panoptic list is the one of the run without soft-NMS
    for k in ('panoptic_cls_inds', 'panoptic_cls_probs', 'panoptic_outputs', 'fcn_outputs'):
        assert memguard.bit_equal(out[k].contiguous(), off[k].contiguous()), k


def test_soft_nms_with_box_voting_moves_boxes_not_scores(soft_model, monkeypatch):
    from upsnet_amd import tta
    from upsnet_amd.config.config import config
    from upsnet_amd.synthetic import make_image_u8
    monkeypatch.setattr(tta, 'augmentation_list', lambda cfg=None: list(AUG_LISTS['three']))
    monkeypatch.setitem(config.test, 'soft_nms', True)
    img = make_image_u8(*IMAGE_HW, seed=5, device='cuda')
    monkeypatch.setitem(config.test, 'soft_nms', False)
    monkeypatch.setattr(soft_model.mask_roi, 'score_thresh', _sixtieth_score(soft_model.forward_tta(img, return_parts=True)[1]))
    monkeypatch.setitem(config.test, 'soft_nms', True)      # (59 winners: decayed rows among the 100, see above)
    soft, soft_parts = soft_model.forward_tta(img, return_parts=True)
    monkeypatch.setitem(config.test, 'bbox_vote', True)
    both, parts = soft_model.forward_tta(img, return_parts=True)
    assert parts['bbox_vote'] == (float(config.test.score_thresh), 0.5) and parts['soft_nms'] == (1, 0.5, 0.0001)
    assert parts['n_det'] == soft_parts['n_det']
    assert memguard.bit_equal(parts['det_boxes_prevote'], soft_parts['det_boxes'])        # voting starts from the soft selection
    assert memguard.bit_equal(both['cls_probs'], soft['cls_probs']) and memguard.bit_equal(both['cls_inds'], soft['cls_inds'])
    assert (host(both['pred_boxes']) != host(soft['pred_boxes'])).any()
    voted = bref.box_vote(host(parts['merged_rois']), host(parts['merged_delta']), host(parts['merged_prob']),
                          int(parts['merged_n_rois'].item()), parts['im_info'][0], config.network.bbox_reg_weights,
                          bool(soft_model.mask_roi.clip_boxes), host(soft_parts['det_boxes']), host(parts['det_cls']), parts['n_det'],
                          float(config.test.score_thresh), 0.5)
    assert bits_equal(host(both['pred_boxes']), voted)


# ------------------------------------------------------------------------------------------------ the evaluation run
def test_evaluate_main_with_soft_nms(soft_model, tmp_path):
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
        chains = [_direct_chain(soft_model, e['image'], ds.num_classes) for e in ds.roidb]
        _write_gt(ds, chains, list(range(len(sizes))), ['img_%d' % e['id'] for e in ds.roidb])

        # soft-NMS alone: the eager path with the base augmentation
        res = main(['--cfg', cfg, '--synthetic_weights', '--soft_nms', '--soft_nms_method', 'gaussian'])
        with open(res['results_file'], 'rb') as f:
            got = pickle.load(f)
        assert got['soft_nms'] == [2, 0.5, 0.0001]
        assert got['test_aug'] == [[config.test.scales[0], config.test.max_size, False]]
        assert set(got) == {'all_boxes', 'all_masks', 'all_ssegs', 'all_panos', 'all_pano_cls_inds', 'test_aug', 'soft_nms'}
        n = len(sizes)
        assert len(got['all_ssegs']) == len(got['all_panos']) == len(got['all_pano_cls_inds']) == n
        assert all(len(got['all_boxes'][c]) == n for c in range(1, ds.num_classes))
        m = res['metrics']
        assert {'box_ap', 'mask_ap', 'panoptic', 'sseg'} <= set(m)
        assert 0.0 <= m['sseg']['meanIU'] <= 1.0 and np.isfinite(m['sseg']['meanIU'])
        assert len(res['times']['net_time']) == n
    finally:
        config.clear()
        config.update(saved)
