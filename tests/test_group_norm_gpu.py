"""GPU: GroupNorm(32, C) on the kernels of csrc/group_norm.hip -- the op against torch.nn.functional.group_norm in float64 on the CPU
(the reference project uses nn.GroupNorm itself), cancellation at mean 64 / std 1, the fused epilogues, independence of a sample from its
launch, determinism, multi-map == single-map bits, poisoned memory, the five head modules with with_norm = 'group_norm' layer by layer,
and the whole model (eager, HIP graph, ROI independence of the mask head).

Tolerance everywhere: |err| <= 1e-4 + 1e-4 |ref| (tests/test_trunk_gpu.py)."""
import copy
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import memguard  # noqa: E402
from conftest import gen_rois  # noqa: E402

pytestmark = pytest.mark.gpu

TOL = 1e-4
EPS = 1e-5
SHAPES = [(1, 256, 14, 14), (3, 256, 14, 14), (2, 128, 37, 53), (1, 256, 1, 1), (1, 256, 3, 5), (5, 1024, 1, 1), (67, 1024, 1, 1), (1, 128, 1, 2)]
SHAPES += [(2, 384, 5, 7), (1, 640, 3, 3)]   # groups of 3 and 5 lanes: they straddle waves and are combined through the LDS
CHUNKS = ['P', '2P-1', '2P', '2P+1', '3P+7']
PYRAMID = [(16, 24), (8, 12), (4, 6), (2, 3), (1, 2)]   # P2..P6 of a 64 x 96 image


def _chunk_shapes():
    """Maps of P (the largest sample of the small form), 2P - 1, 2P, 2P + 1 and 3P + 7 pixels for the stats kernel's chunk size P: a
    ragged last chunk, more than two partials."""
    from upsnet_amd import group_norm
    P = group_norm.chunk_pixels()
    return [(2, 256, 2, P // 2), (1, 256, 1, 2 * P - 1), (1, 256, 2, P), (1, 256, 1, 2 * P + 1), (1, 256, 1, 3 * P + 7)]


def _ref64(x, gamma, beta, eps=EPS, relu=False, residual=None, residual_up=False):
    y = F.group_norm(x.detach().double().cpu(), 32, gamma.detach().double().cpu(), beta.detach().double().cpu(), eps)
    if residual is not None:
        r = residual.detach().double().cpu()
        y = y + (F.interpolate(r, scale_factor=2, mode='nearest') if residual_up else r)
    return F.relu(y) if relu else y


def _worst(got, ref):
    got = got.detach().double().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert bool(torch.isfinite(got).all())
    return float(((got - ref).abs() / (TOL + TOL * ref.abs())).max()) if ref.numel() else 0.0


def _inputs(shape, seed, mean=0.0):
    g = torch.Generator().manual_seed(seed)
    n, c, h, w = shape
    x = (torch.randn(shape, generator=g) + mean).cuda().contiguous(memory_format=torch.channels_last)
    gamma = (1.0 + (torch.rand(c, generator=g) - 0.5)).cuda()
    beta = (torch.rand(c, generator=g) - 0.5).cuda()
    return x, gamma, beta


def _forms(x, gamma, beta, relu=False):
    """Every form that takes this input: {name: output as [N,C,H,W]}."""
    from upsnet_amd import group_norm
    outs = {'two-phase': group_norm.group_norm(x, gamma, beta, EPS, relu=relu)}
    n, c, h, w = x.shape
    if h * w <= group_norm.chunk_pixels():
        outs['small'] = group_norm.group_norm_small(x, gamma, beta, EPS, relu=relu)
    if h * w == 1:
        outs['rows'] = group_norm.group_norm_small(x.reshape(n, c), gamma, beta, EPS, relu=relu).view(n, c, 1, 1)
    return outs


def _check_op(shape, seed, mean):
    x, gamma, beta = _inputs(shape, seed, mean)
    ref = _ref64(x, gamma, beta)
    outs = _forms(x, gamma, beta)
    for name, y in outs.items():
        w = _worst(y, ref)
        print('group_norm %s %s mean %g: worst error %.3f of the bound' % (name, shape, mean, w))
        assert w <= 1.0, (name, shape, w)
    if 'small' in outs and shape[2] * shape[3] > 1:   # same walk, same order: same bits
        assert memguard.bit_equal(outs['small'], outs['two-phase'])


@pytest.mark.parametrize("shape", SHAPES + CHUNKS, ids=str)
def test_op_matches_float64(shape):
    if isinstance(shape, str):
        shape = _chunk_shapes()[CHUNKS.index(shape)]
    _check_op(shape, seed=1, mean=0.0)


@pytest.mark.parametrize("shape", SHAPES + CHUNKS, ids=str)
def test_no_cancellation_at_mean_64_std_1(shape):
    """x = 64 + N(0, 1): E[x^2] - mean^2 in fp32 misses the bound 4-490 times over; torch's own fp32 GroupNorm sits at 0.14-0.23 of it."""
    if isinstance(shape, str):
        shape = _chunk_shapes()[CHUNKS.index(shape)]
    _check_op(shape, seed=2, mean=64.0)


@pytest.mark.parametrize("shape", [(3, 256, 14, 14), (2, 128, 37, 53), (5, 1024, 1, 1)], ids=str)
def test_all_zero_sample_returns_beta_exactly(shape):
    x, gamma, beta = _inputs(shape, seed=3)
    x[1].zero_()
    for name, y in _forms(x, gamma, beta).items():
        assert memguard.bit_equal(y[1], beta.view(-1, 1, 1).expand_as(y[1])), name


EPILOGUES = [dict(relu=True), dict(res='same'), dict(res='up'), dict(relu=True, res='same'), dict(relu=True, res='up')]


def _epilogue_case(case, seed=4, wrap=lambda t: t):
    from upsnet_amd import group_norm
    x, gamma, beta = _inputs((2, 256, 8, 12), seed)
    g = torch.Generator().manual_seed(seed + 100)
    res = {None: None, 'same': torch.randn(2, 256, 8, 12, generator=g), 'up': torch.randn(2, 256, 4, 6, generator=g)}[case.get('res')]
    if res is not None:
        res = res.cuda().contiguous(memory_format=torch.channels_last)
    kw = dict(relu=case.get('relu', False), residual=None if res is None else wrap(res), residual_up=case.get('res') == 'up')
    y = group_norm.group_norm(wrap(x), wrap(gamma), wrap(beta), EPS, **kw)
    return y, _ref64(x, gamma, beta, EPS, kw['relu'], res, kw['residual_up'])


@pytest.mark.parametrize("case", EPILOGUES, ids=str)
def test_epilogues(case):
    y, ref = _epilogue_case(case)
    assert _worst(y, ref) <= 1.0
    if case.get('relu'):
        assert float(y.min()) >= 0.0 and float((y == 0).float().mean()) > 0.05


def test_a_sample_does_not_depend_on_its_launch():
    from upsnet_amd import group_norm
    x, gamma, beta = _inputs((100, 256, 14, 14), seed=5)
    whole = group_norm.group_norm_small(x, gamma, beta, EPS, relu=True)
    assert memguard.bit_equal(whole, group_norm.group_norm_small(x, gamma, beta, EPS, relu=True))       # two runs of one launch
    three = group_norm.group_norm_small(x[:3], gamma, beta, EPS, relu=True)
    two_phase = group_norm.group_norm(x, gamma, beta, EPS, relu=True)
    assert memguard.bit_equal(two_phase, group_norm.group_norm(x, gamma, beta, EPS, relu=True))
    assert memguard.bit_equal(two_phase, whole)
    for i in (0, 1, 2, 57, 99):
        alone = group_norm.group_norm_small(x[i:i + 1], gamma, beta, EPS, relu=True)
        assert memguard.bit_equal(whole[i:i + 1], alone), i
        assert memguard.bit_equal(group_norm.group_norm(x[i:i + 1], gamma, beta, EPS, relu=True), alone), i
        if i < 3:
            assert memguard.bit_equal(three[i:i + 1], alone), i
    # rows: the box head's fc6
    r, gamma, beta = _inputs((67, 1024, 1, 1), seed=6)
    r = r.reshape(67, 1024)
    rows = group_norm.group_norm_small(r, gamma, beta, EPS, relu=True)
    assert memguard.bit_equal(rows, group_norm.group_norm_small(r, gamma, beta, EPS, relu=True))
    for i in (0, 7, 8, 31, 66):
        assert memguard.bit_equal(rows[i:i + 1], group_norm.group_norm_small(r[i:i + 1], gamma, beta, EPS, relu=True)), i
    assert memguard.bit_equal(rows[:3], group_norm.group_norm_small(r[:3].contiguous(), gamma, beta, EPS, relu=True))


def _pyramid_maps(seed, channels=256, batch=1):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(batch, channels, h, w, generator=g).cuda().contiguous(memory_format=torch.channels_last) for h, w in PYRAMID]


def test_multi_map_launch_equals_single_launches():
    from upsnet_amd import group_norm
    xs = _pyramid_maps(7, batch=2)
    _, gamma, beta = _inputs((1, 256, 1, 1), seed=7)
    for relu in (False, True):
        multi = group_norm.group_norm_multi(xs, gamma, beta, EPS, relu=relu)
        again = group_norm.group_norm_multi(xs, gamma, beta, EPS, relu=relu)
        for x, y, y2 in zip(xs, multi, again):
            assert memguard.bit_equal(y, group_norm.group_norm(x, gamma, beta, EPS, relu=relu)), tuple(x.shape)
            assert memguard.bit_equal(y, y2)
            assert _worst(y, _ref64(x, gamma, beta, EPS, relu)) <= 1.0
    # a map of several chunks among small ones, in both positions
    big = _inputs(_chunk_shapes()[4], seed=8)[0]
    for order in ([big, xs[1], xs[4]], [xs[4], big, xs[1]]):
        for x, y in zip(order, group_norm.group_norm_multi(order, gamma, beta, EPS)):
            assert memguard.bit_equal(y, group_norm.group_norm(x, gamma, beta, EPS)), tuple(x.shape)


def _poisoned_run(fn):
    """fn(wrap) under both poison patterns, inputs inside bands of poison: the results must agree bit for bit and every band be intact
    (checked when the guard exits)."""
    outs = {}
    for pattern in 'AB':
        with memguard.poisoned(pattern, modules=('upsnet_amd.group_norm',)) as g:
            outs[pattern] = fn(lambda t: memguard.banded_copy(t, pattern))
            torch.cuda.synchronize()
        assert g.count > 0
    return outs


@pytest.mark.parametrize("shape", SHAPES + CHUNKS, ids=str)
def test_poisoned_memory_op(shape):
    if isinstance(shape, str):
        shape = _chunk_shapes()[CHUNKS.index(shape)]
    x, gamma, beta = _inputs(shape, seed=9)
    ref = _ref64(x, gamma, beta)
    outs = _poisoned_run(lambda wrap: _forms(wrap(x), wrap(gamma), wrap(beta)))
    for name in outs['A']:
        assert memguard.bit_equal(outs['A'][name], outs['B'][name]), name
        assert _worst(outs['A'][name], ref) <= 1.0, name


@pytest.mark.parametrize("case", EPILOGUES, ids=str)
def test_poisoned_memory_epilogues(case):
    outs = _poisoned_run(lambda wrap: _epilogue_case(case, wrap=wrap))
    assert memguard.bit_equal(outs['A'][0], outs['B'][0])
    assert _worst(outs['A'][0], outs['A'][1]) <= 1.0


# ------------------------------------------------------------------------------------------------ modules
def _randomise_norms(module, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in module.modules():
            if isinstance(m, nn.GroupNorm):
                m.weight.copy_(1.0 + (torch.rand(m.weight.shape, generator=g) - 0.5))
                m.bias.copy_(torch.rand(m.bias.shape, generator=g) - 0.5)
            elif isinstance(m, nn.Conv2d) and float(m.weight.abs().max()) == 0.0:   # the zero-initialised offset predictors
                m.weight.copy_(torch.randn(m.weight.shape, generator=g) * 0.01)


def _traced(fn):
    from upsnet_amd.models import hipconv
    del hipconv.FALLBACKS[:]
    hipconv.TRACE = []
    try:
        with torch.no_grad():
            out = fn()
        torch.cuda.synchronize()
        trace = hipconv.TRACE
    finally:
        hipconv.TRACE = None
    assert hipconv.FALLBACKS == []
    return out, [r for r in trace if r['kind'] == 'gn']


def _check_gn_records(recs, label):
    worst = 0.0
    for r in recs:
        gn = r['module']
        assert r['form'] != 'library', r['form']
        ref = _ref64(r['x'], gn.weight, gn.bias, gn.eps, r['relu'], r['residual'], r['residual_up'])
        got = r['out']
        w = _worst(got.view(ref.shape), ref)
        worst = max(worst, w)
        assert w <= 1.0, (label, r['form'], tuple(r['x'].shape), w)
    print('%s: %d gn launches, worst error %.3f of the bound' % (label, len(recs), worst))


@pytest.fixture
def cityscapes():
    from upsnet_amd.config.config import update_config_dict, CITYSCAPES_R50, config
    update_config_dict(CITYSCAPES_R50)
    saved = {k: config.network[k] for k in ('fpn_with_norm', 'rcnn_with_norm', 'fcn_with_norm')}
    yield config
    for k, v in saved.items():
        setattr(config.network, k, v)


def _prepared(m, seed):
    _randomise_norms(m, seed)
    return m.cuda().eval().to(memory_format=torch.channels_last)


def _rois(n, seed):
    return torch.from_numpy(gen_rois(np.random.default_rng(seed), n, 64, 96, smin=8, smax=60)).cuda()


def test_fpn_module(cityscapes):
    from upsnet_amd.models.fpn import FPN
    torch.manual_seed(11)
    fpn = _prepared(FPN(feature_dim=256, with_norm='group_norm'), 11)
    g = torch.Generator().manual_seed(12)
    res = [torch.randn(1, c, h, w, generator=g).cuda().contiguous(memory_format=torch.channels_last)
           for c, (h, w) in zip((256, 512, 1024, 2048), PYRAMID[:4])]
    outs, recs = _traced(lambda: fpn(*res))
    assert len(recs) == 8 and sum(1 for r in recs if r['residual_up']) == 3
    _check_gn_records(recs, 'FPN')
    # the reference's forward (fpn.py:78-104) in float64
    m = copy.deepcopy(fpn).cpu().double()
    r2, r3, r4, r5 = [t.detach().double().cpu() for t in res]
    up = lambda t: F.interpolate(t, scale_factor=2, mode='nearest')
    with torch.no_grad():
        p5_1 = m.fpn_p5_1x1(r5)
        p4_plus = up(p5_1) + m.fpn_p4_1x1(r4)
        p3_plus = up(p4_plus) + m.fpn_p3_1x1(r3)
        p2_plus = up(p3_plus) + m.fpn_p2_1x1(r2)
        p5 = m.fpn_p5(p5_1)
        want = [m.fpn_p2(p2_plus), m.fpn_p3(p3_plus), m.fpn_p4(p4_plus), p5, p5[:, :, ::2, ::2]]
    assert len(outs) == 5
    for name, got, ref in zip(('p2', 'p3', 'p4', 'p5', 'p6'), outs, want):
        w = _worst(got, ref)
        print('FPN %s: %.3f of the bound' % (name, w))
        assert w <= 1.0, name


def test_rpn_module(cityscapes):
    from upsnet_amd.models.rpn import RPN, rpn_forward_levels
    torch.manual_seed(13)
    rpn = _prepared(RPN(num_anchors=3, input_dim=256, with_norm='group_norm'), 13)
    feats = _pyramid_maps(14)
    (scores, boxes, probs), recs = _traced(lambda: rpn_forward_levels(rpn, feats))
    assert len(recs) == 5 and all(r['relu'] and r['form'] == 'gn multi' for r in recs)
    _check_gn_records(recs, 'RPN')
    assert len(scores) == 5 and all(bool(torch.isfinite(s).all()) for s in scores)
    # the per-level forward: the same layers on one map
    (s1, b1, p1), recs1 = _traced(lambda: rpn(feats[1]))
    assert len(recs1) == 1 and recs1[0]['relu'] and recs1[0]['form'] != 'library'
    _check_gn_records(recs1, 'RPN.forward')
    assert _worst(s1, scores[1].detach().double().cpu()) <= 1.0


def test_mask_branch_module(cityscapes):
    from upsnet_amd.models.rcnn import MaskBranch
    torch.manual_seed(15)
    mb = _prepared(MaskBranch(9, dim_in=256, with_norm='group_norm'), 15)
    feats, rois = _pyramid_maps(16)[:4], _rois(5, 16)
    out, recs = _traced(lambda: mb(feats, rois))
    assert len(recs) == 4 and all(r['relu'] and r['form'] == 'gn small' and tuple(r['x'].shape) == (5, 256, 14, 14) for r in recs)
    _check_gn_records(recs, 'MaskBranch')
    # the reference's forward (rcnn.py:79-87) in float64, from the pooled features of the product run
    m = copy.deepcopy(mb).cpu().double()
    with torch.no_grad():
        x = mb.roi_pooling(feats, rois).detach().double().cpu()
        for blk in (m.mask_conv1, m.mask_conv2, m.mask_conv3, m.mask_conv4, m.mask_deconv1):
            x = blk(x)
        ref = m.mask_score(x)
    w = _worst(out, ref)
    print('MaskBranch logits: %.3f of the bound' % w)
    assert w <= 1.0


def test_rcnn_module(cityscapes):
    from upsnet_amd.models.rcnn import RCNN
    torch.manual_seed(17)
    rcnn = _prepared(RCNN(9, 9, dim_in=256, with_norm='group_norm'), 17)
    feats, rois = _pyramid_maps(18)[:4], _rois(7, 18)
    out, recs = _traced(lambda: rcnn(feats, rois))
    assert len(recs) == 1 and recs[0]['form'] == 'gn rows' and tuple(recs[0]['x'].shape) == (7, 1024) and recs[0]['relu']
    _check_gn_records(recs, 'RCNN')
    assert tuple(out['cls_score'].shape) == (7, 9) and bool(torch.isfinite(out['cls_score']).all())
    assert float(out['fc_feat'].min()) >= 0.0


def test_fcn_head_module(cityscapes):
    from upsnet_amd.models.fcn import FCNHead
    torch.manual_seed(19)
    head = _prepared(FCNHead(256, 19, num_layers=3, with_norm='group_norm', upsample_rate=4), 19)
    feats = _pyramid_maps(20)[:4]
    out, recs = _traced(lambda: head(*feats))
    assert len(recs) == 12 and all(r['relu'] and r['form'] == 'gn multi' for r in recs)
    assert [r['x'].shape[1] for r in recs] == [256] * 4 + [128] * 8
    _check_gn_records(recs, 'FCNHead')
    assert bool(torch.isfinite(out['fcn_output']).all())
    # one level through the per-module forward: the same layers, per level
    y, recs1 = _traced(lambda: head.fcn_subnet(feats[2]))
    assert len(recs1) == 3 and all(r['form'] != 'library' for r in recs1)
    _check_gn_records(recs1, 'FCNSubNet.forward')


# ------------------------------------------------------------------------------------------------ whole model
@pytest.fixture
def gn_model(cityscapes):
    from upsnet_amd.synthetic import build_model
    for k in ('fpn_with_norm', 'rcnn_with_norm', 'fcn_with_norm'):
        setattr(cityscapes.network, k, 'group_norm')
    model = build_model(device='cuda')
    _randomise_norms(model, 21)
    model.invalidate_graphs()
    return model


def test_whole_model_with_group_norm_heads(gn_model):
    from upsnet_amd.config.config import config
    from upsnet_amd.synthetic import make_image
    model = gn_model
    imgs = [make_image(128, 256, seed=30 + j, device='cuda') for j in range(3)]
    keys = ('panoptic_outputs', 'pred_boxes', 'cls_probs', 'cls_inds', 'mask_probs', 'panoptic_cls_inds', 'fcn_outputs')
    out, recs = _traced(lambda: model(imgs[0]))
    for k in keys:
        assert out[k].dtype not in (torch.float32,) or bool(torch.isfinite(out[k]).all()), k
    n_layers = config.network.fcn_num_layers
    assert len(recs) >= 8 + 1 + 4 + 4 * n_layers
    assert sum(1 for r in recs if r['form'] == 'gn rows') == 1 and sum(1 for r in recs if r['form'] == 'gn multi') == 4 * n_layers
    _check_gn_records(recs, 'UPSNet-50 128x256')
    # HIP-graph replay == eager, bit for bit (tests/test_model_gpu.py::test_hip_graph_replay_equals_eager, one shape)
    was = model.use_graph, model.graph_slots
    try:
        with torch.no_grad():
            model.use_graph = False
            eager = [{k: v.clone() for k, v in model(im).items()} for im in imgs]
            model.use_graph = True
            model._graphs.clear()
            model.graph_slots = 2
            for step, j in enumerate([0, 1, 2, 0, 1, 2, 0, 1, 2, 2]):
                got = model(imgs[j])
                for k in keys:
                    assert torch.equal(got[k], eager[j][k]), (step, j, k)
            assert sum(1 for e in model._graphs.values() for sl in e['slots'] if 'graph' in sl) == 2
    finally:
        model.use_graph, model.graph_slots = was
        model._graphs.clear()
    # the mask logits of a ROI do not depend on how many ROIs share the launch: alone == among the padded max_det rows
    with torch.no_grad():
        feats = list(model._pyramid(imgs[0])[:4])
        max_det = int(config.test.max_det)
        rois = torch.zeros(max_det, 5, device='cuda')
        picked = torch.cat([eager[0]['pred_boxes'][:4].float(), torch.from_numpy(gen_rois(np.random.default_rng(5), 3, 128, 256, smin=8, smax=100)).cuda()])
        rois[:picked.shape[0]] = picked
        padded = model.mask_branch(feats, rois)
        for i in range(picked.shape[0]):
            assert memguard.bit_equal(padded[i:i + 1], model.mask_branch(feats, rois[i:i + 1])), i
        assert bool(torch.isfinite(padded).all())
