"""End-to-end GPU tests on seeded synthetic weights + image.

Library convolutions / GEMMs (MIOpen, hipBLASLt) are not bit-repeatable run to run on this stack, so the
end-to-end parity claim is made stage-wise on the tensors recorded during ONE forward (model.taps): every
custom-op stage must reproduce the oracle bit-for-bit from that stage's recorded inputs
(oracle.forward.check_taps). Both execution styles (fused MI355X pipeline / reference-shaped modules) are
checked this way, which also proves them equivalent.
"""
import numpy as np
import pytest
import torch

from oracle.draws import DRAWS, fit_cls_gain

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def setup():
    from upsnet_amd.config.config import update_config_dict, CITYSCAPES_R50
    update_config_dict(CITYSCAPES_R50)
    from upsnet_amd.synthetic import build_model, make_image
    model = build_model()
    data = make_image(256, 512, seed=0, device='cuda')
    return model, data


@pytest.mark.parametrize("pipeline", ["fused", "modules"])
def test_stagewise_parity(setup, pipeline):
    from oracle.forward import check_taps
    model, data = setup
    model.pipeline = pipeline
    model.taps = {}
    with torch.no_grad():
        out = model(data)
    taps, model.taps, model.pipeline = model.taps, None, 'fused'
    res = check_taps(taps, enable_void=model.enable_void)
    counts = res.pop('counts')
    assert all(res.values()), (res, counts)
    assert counts['n_rois'] > 100 and counts['n_det'] >= 1 and counts['n_inst'] >= 2, counts
    # result dict is consistent with the recorded stages
    assert torch.equal(out['pred_boxes'], taps['det_boxes']) and torch.equal(out['panoptic_outputs'], taps['panoptic'])
    assert torch.equal(out['panoptic_cls_inds'], taps['pan_cls'][taps['keep']])
    assert out['mask_probs'].shape == (counts['n_det'], 9, 28, 28)
    assert out['panoptic_outputs'].dtype == torch.int64 and out['panoptic_outputs'].shape == (1, 256, 512)


def test_full_size_stagewise_parity():
    """The benchmark configuration itself: 1024x2048, label map bit-identical to the oracle."""
    from oracle.forward import check_taps
    from upsnet_amd.config.config import update_config_dict, CITYSCAPES_R50
    update_config_dict(CITYSCAPES_R50)
    from upsnet_amd.synthetic import build_model, make_image
    model = build_model()
    data = make_image(1024, 2048, seed=1, device='cuda')
    model.taps = {}
    with torch.no_grad():
        model(data)
    res = check_taps(model.taps, enable_void=True)
    counts = res.pop('counts')
    assert all(res.values()), (res, counts)
    assert counts['label_mismatch'] == 0 and counts['n_inst'] >= 5, counts


def test_custom_ops_bit_repeatable(setup):
    """Forward kernels have one writer per output and no atomics on data: same inputs -> same bits."""
    from upsnet_amd import ops
    model, data = setup
    model.taps = {}
    with torch.no_grad():
        model(data)
        t, model.taps = model.taps, None
        for _ in range(3):
            r, s, n = model.pyramid_proposal.forward_padded(t['rpn_cls_prob'], t['rpn_bbox_pred'], t['im_info'])
            assert torch.equal(r, t['rois']) and int(n.item()) == int(t['n_rois'].item())
            b, sc, c, _, num = model.mask_roi_panoptic.forward_padded(t['rois'], t['bbox_pred'], t['cls_prob'], t['im_info'], t['n_rois'])
            k = int(num.item())
            assert torch.equal(b[:k], t['pan_boxes']) and torch.equal(c[:k], t['pan_cls'])
            H, W = t['fcn_score'].shape[2] * 4, t['fcn_score'].shape[3] * 4
            keep, nk, real = model.mask_removal.select(t['pan_boxes'][:, 1:], t['pan_scores'], t['pan_logit'], t['pan_cls'], (H, W))
            pan, sem = ops.panoptic_fuse_up(t['fcn_score'], 4, 11, t['pan_boxes'], t['pan_logit'], t['pan_cls'], keep, nk, real,
                                            model.seg_term.class_map)
            assert torch.equal(pan, t['panoptic']) and torch.equal(sem, t['sem'])


def test_coco_r101_dcn_config_stagewise_parity():
    """BASELINE.json configs[3] shape family: UPSNet-101-DCN (DCN v1 in every res3-5 block, GAP in FPN, 3 FCN layers,
    81 / 133 classes, 300 proposals) on a small COCO-shaped image; every custom-op stage vs the oracle."""
    from oracle.forward import check_taps
    from upsnet_amd.config.config import update_config_dict, COCO_R101_DCN, CITYSCAPES_R50
    update_config_dict(COCO_R101_DCN)
    try:
        from upsnet_amd.synthetic import build_model, make_image
        model = build_model()
        assert sum(1 for n, _ in model.named_modules() if n.endswith('conv2_offset')) == 4 + 23 + 3
        data = make_image(200, 333, seed=2, device='cuda')   # padded to 224 x 352
        model.taps = {}
        with torch.no_grad():
            out = model(data)
        res = check_taps(model.taps, enable_void=True)
        counts = res.pop('counts')
        assert all(res.values()), (res, counts)
        assert counts['n_rois'] <= 300 and out['panoptic_outputs'].shape == (1, 224, 352)
    finally:
        update_config_dict(CITYSCAPES_R50)


def test_coco_r101_dcn_full_size_stagewise_parity():
    """BASELINE.json configs[3] at its real size: UPSNet-101-DCN, COCO-shaped 800x1333 (padded to 800x1344), 300 proposals,
    81 / 133 classes -- every custom-op stage recomputed by the oracle from the recorded inputs, label map bit-identical."""
    from oracle.forward import check_taps
    from upsnet_amd.config.config import update_config_dict, COCO_R101_DCN, CITYSCAPES_R50
    update_config_dict(COCO_R101_DCN)
    try:
        from upsnet_amd.synthetic import build_model, make_image
        model = build_model()
        data = make_image(800, 1333, seed=5, device='cuda')
        model.taps = {}
        with torch.no_grad():
            out = model(data)
        res = check_taps(model.taps, enable_void=True)
        counts = res.pop('counts')
        assert all(res.values()), (res, counts)
        assert counts['label_mismatch'] == 0 and counts['n_rois'] <= 300 and counts['n_det'] >= 1, counts
        assert out['panoptic_outputs'].shape == (1, 800, 1344)
    finally:
        update_config_dict(CITYSCAPES_R50)


def test_mask_head_dedup_is_bit_identical_to_two_passes(setup):
    """The fused pipeline runs the mask head once over [per-class detections ; panoptic detections not among them] and reuses
    rows for the duplicates; the reference-shaped pipeline runs it twice (resnet_upsnet.py:190,215). Same bits."""
    model, data = setup
    outs = {}
    with torch.no_grad():
        for pipeline in ("fused", "modules"):
            model.pipeline = pipeline
            model.taps = {}
            o = model(data)
            outs[pipeline] = (model.taps, o)
    model.taps, model.pipeline = None, 'fused'
    tf, of = outs["fused"]
    tm, om = outs["modules"]
    assert tf['pan_boxes'].shape[0] >= 2 and torch.equal(tf['pan_boxes'], tm['pan_boxes'])
    assert torch.equal(tf['pan_logit'], tm['pan_logit'])
    assert torch.equal(of['mask_probs'], om['mask_probs'])
    assert torch.equal(of['panoptic_outputs'], om['panoptic_outputs'])
    # the dedup actually removed work: panoptic detections are (mostly) a subset of the per-class detections
    from upsnet_amd import ops
    r, s, n = model.pyramid_proposal.forward_padded(tf['rpn_cls_prob'], tf['rpn_bbox_pred'], tf['im_info'])
    d = model.mask_roi.forward_padded(r, tf['bbox_pred'], tf['cls_prob'], tf['im_info'], n)
    p = model.mask_roi_panoptic.forward_padded(r, tf['bbox_pred'], tf['cls_prob'], tf['im_info'], n)
    row, extra, n_extra = ops.mask_roi_dedup(d[3], d[2], d[4], p[3], p[2], p[0], p[4])
    n_det, n_pan, n_extra = int(d[4].item()), int(p[4].item()), int(n_extra.item())
    assert n_extra < n_pan
    rows = row[:n_pan].cpu().numpy()
    allb = torch.cat([d[0][:n_det], extra[:n_extra]], 0)
    assert torch.equal(allb[torch.from_numpy(rows).long().cuda()], p[0][:n_pan])
    assert sorted(rows[rows >= n_det].tolist()) == list(range(n_det, n_det + n_extra))


def test_mixed_resolution_stream_r101_dcn():
    """BASELINE.json configs[4] shape family: ONE UPSNet-101-DCN model object fed an alternating stream of Cityscapes-shaped and
    COCO-shaped images (different padded sizes, different proposal counts): every step stage-wise identical to the oracle, and
    identical to the same image run in isolation (no state leaks between resolutions: workspaces, packed weights, streams)."""
    from oracle.forward import check_taps
    from upsnet_amd.config.config import update_config_dict, COCO_R101_DCN, CITYSCAPES_R50
    update_config_dict(COCO_R101_DCN)
    try:
        from upsnet_amd.synthetic import build_model, make_image
        model = build_model()
        imgs = [make_image(128, 256, seed=3, device='cuda'), make_image(100, 167, seed=4, device='cuda')]   # second pads to 128 x 192
        first = {}
        with torch.no_grad():
            for step in range(4):
                j = step % 2
                model.taps = {}
                out = model(imgs[j])
                res = check_taps(model.taps, enable_void=True)
                counts = res.pop('counts')
                assert all(res.values()), (step, res, counts)
                if j in first:
                    assert torch.equal(out['panoptic_outputs'], first[j]['panoptic_outputs'])
                    assert torch.equal(out['pred_boxes'], first[j]['pred_boxes'])
                else:
                    first[j] = out
        model.taps = None
        assert first[0]['panoptic_outputs'].shape == (1, 128, 256) and first[1]['panoptic_outputs'].shape == (1, 128, 192)
    finally:
        update_config_dict(CITYSCAPES_R50)


def test_coco_r101_dcn_at_1024x2048_stagewise_parity():
    """BASELINE.json configs[4], its Cityscapes-shaped half at the real size: UPSNet-101-DCN on a 1024x2048 image -- every custom-op
    stage recomputed by the oracle from the recorded inputs, label map bit-identical (VERDICT r03 next #1b)."""
    from oracle.forward import check_taps
    from upsnet_amd.config.config import update_config_dict, COCO_R101_DCN, CITYSCAPES_R50
    update_config_dict(COCO_R101_DCN)
    try:
        from upsnet_amd.synthetic import build_model, make_image
        model = build_model()
        data = make_image(1024, 2048, seed=6, device='cuda')
        model.taps = {}
        with torch.no_grad():
            out = model(data)
        res = check_taps(model.taps, enable_void=True)
        counts = res.pop('counts')
        assert all(res.values()), (res, counts)
        assert counts['label_mismatch'] == 0 and counts['n_rois'] <= 300 and counts['n_det'] >= 1, counts
        assert out['panoptic_outputs'].shape == (1, 1024, 2048)
    finally:
        update_config_dict(CITYSCAPES_R50)


@pytest.mark.parametrize("weight_seed,image_seed", DRAWS)
@pytest.mark.parametrize("preset,h,w", [('CITYSCAPES_R50', 1024, 2048), ('COCO_R101_DCN', 800, 1333)])
def test_stagewise_parity_on_other_draws(preset, h, w, weight_seed, image_seed):
    """Both benchmark configurations on the draws of oracle.draws.DRAWS (classifier gain oracle.draws.fit_cls_gain): other proposals, NMS
    ties, MaskROI outputs, mask-removal keeps and panoptic counts than the seed-235 network of the tests above -- every custom-op
    stage bit-identical to the oracle, label map included, with at least 5 instances in the panoptic output."""
    from oracle.forward import check_taps
    from upsnet_amd.config import config as cfgmod
    from upsnet_amd.config.config import update_config_dict, CITYSCAPES_R50
    update_config_dict(getattr(cfgmod, preset))
    try:
        from upsnet_amd.synthetic import build_model, make_image
        model = build_model(seed=weight_seed, cls_gain=fit_cls_gain)
        data = make_image(h, w, seed=image_seed, device='cuda')
        model.taps = {}
        with torch.no_grad():
            model(data)
        res = check_taps(model.taps, enable_void=True)
        counts = res.pop('counts')
        assert all(res.values()), (res, counts)
        assert counts['label_mismatch'] == 0 and counts['n_inst'] >= 5, counts
        print('%s %dx%d draw (%d, %d), cls_gain %.2f: %s' % (preset, h, w, weight_seed, image_seed, model.cls_gain, counts))
    finally:
        update_config_dict(CITYSCAPES_R50)


def test_mixed_stream_at_real_sizes_graph_replay_equals_eager():
    """BASELINE.json configs[4] as benchmarked (`--workload upsnet101dcn_mixed_1024x2048_800x1333`): ONE UPSNet-101-DCN fed the
    alternating 1024x2048 / 800x1333 stream through the HIP-graph path with two images in flight (forward_async, two graph instances per
    shape, each on its own stream). Every output of every step == the eager single-stream forward of that image; the eager forward
    itself is stage-wise identical to the oracle (check_taps) at both sizes."""
    from oracle.forward import check_taps
    from upsnet_amd.config.config import update_config_dict, COCO_R101_DCN, CITYSCAPES_R50
    update_config_dict(COCO_R101_DCN)
    try:
        from upsnet_amd.synthetic import build_model, make_image
        model = build_model()
        imgs = [make_image(1024, 2048, seed=7, device='cuda'), make_image(800, 1333, seed=8, device='cuda'),
                make_image(1024, 2048, seed=9, device='cuda'), make_image(800, 1333, seed=10, device='cuda')]
        keys = ('panoptic_outputs', 'pred_boxes', 'cls_probs', 'cls_inds', 'mask_probs', 'panoptic_cls_inds', 'fcn_outputs')
        with torch.no_grad():
            g, model.use_graph = model.use_graph, False
            eager = []
            for j, im in enumerate(imgs):
                model.taps = {} if j < 2 else None
                out = model(im)
                if j < 2:
                    res = check_taps(model.taps, enable_void=True)
                    counts = res.pop('counts')
                    assert all(res.values()) and counts['label_mismatch'] == 0, (j, res, counts)
                    model.taps = None
                eager.append({k: out[k].clone() for k in keys})
            assert eager[0]['panoptic_outputs'].shape == (1, 1024, 2048) and eager[1]['panoptic_outputs'].shape == (1, 800, 1344)
            model.use_graph = True
            assert model.graph_slots >= 2
            for _ in range(3 * model.graph_slots):       # eager, eager, capture -- per instance and shape
                for im in imgs[:2]:
                    model(im)
            pending, seen = [], 0
            for step in range(12):
                j = step % 4
                pending.append((j, model.forward_async(imgs[j])))
                if len(pending) >= 2:
                    jj, h = pending.pop(0)
                    out = h.result()
                    for k in keys:
                        assert torch.equal(out[k], eager[jj][k]), (step, jj, k)
                    seen += 1
            for jj, h in pending:
                out = h.result()
                for k in keys:
                    assert torch.equal(out[k], eager[jj][k]), (jj, k)
            graphs = sum(1 for slots in model._graphs.values() for ent in slots['slots'] if 'graph' in ent)
            assert graphs == 2 * model.graph_slots, graphs      # both shapes really ran as graph replays
            model.use_graph = g
    finally:
        update_config_dict(CITYSCAPES_R50)


# Agreement of the bf16 mode with the fp32 run ON THE SAME IMAGE, measured on MI355X (r10) and asserted with a small margin (0.03) below the
# measured value (a random synthetic network has no decision margin: a bf16 rounding moves near-tied logits; trained weights agree
# far better). name: (semantic arg-max agreement, panoptic label-map agreement)
_BF16_AGREE = {(256, 512): (0.885, 0.80), (1024, 2048): (0.875, 0.86)}   # measured 0.9152 / 0.8330 and 0.9036 / 0.8899 (one box; the assertion held on every box of r10); margin 0.03


def test_bf16_mode_at_1024x2048_stagewise_parity_and_agreement():
    """BASELINE.json configs[2] at the size it is benchmarked (VERDICT r03 next #1a): the bf16-mode forward of the 1024x2048 image --
    every custom-op stage recomputed by the oracle from the recorded inputs, bit for bit (the selection / sampling / fusion kernels do
    not change with the convolution precision) -- and the agreement of its semantic arg-max and of its panoptic label map with the
    fp32 run of the same image."""
    from oracle.forward import check_taps
    from upsnet_amd.config.config import update_config_dict, CITYSCAPES_R50
    from upsnet_amd.models import hipconv
    update_config_dict(CITYSCAPES_R50)
    from upsnet_amd.synthetic import build_model, make_image
    model = build_model()
    data = make_image(1024, 2048, seed=1, device='cuda')
    with torch.no_grad():
        ref = {k: v.clone() for k, v in model(data).items()}
        hipconv.PRECISION = 'bf16'
        try:
            model.taps = {}
            out = model(data)
            taps, model.taps = model.taps, None
        finally:
            hipconv.PRECISION = 'fp32'
    res = check_taps(taps, enable_void=True)
    counts = res.pop('counts')
    assert all(res.values()), (res, counts)
    assert counts['label_mismatch'] == 0 and counts['n_det'] >= 1 and counts['n_inst'] >= 5, counts
    sem = float((out['fcn_outputs'] == ref['fcn_outputs']).float().mean())
    pan = float((out['panoptic_outputs'] == ref['panoptic_outputs']).float().mean())
    print('bf16 vs fp32 at 1024x2048: semantic arg-max agreement %.4f, panoptic label-map agreement %.4f, n_det %d / %d, n_inst %d / %d' %
          (sem, pan, out['cls_inds'].numel(), ref['cls_inds'].numel(), out['panoptic_cls_inds'].numel(), ref['panoptic_cls_inds'].numel()))
    want_sem, want_pan = _BF16_AGREE[(1024, 2048)]
    assert sem >= want_sem and pan >= want_pan, (sem, pan)


# (preset name, h, w, precision) -> floors (semantic, panoptic) = measured on MI355X in round 5 minus 0.03 (bf16) / fixed (bf16x3).
# Measured: UPSNet-101-DCN 800x1333 bf16 vs fp32: semantic arg-max 0.4939, panoptic map 0.7348 -- HALF of the semantic labels differ.
# Every launch of that forward meets its per-launch bound on its own recorded inputs (test_layerwise_gpu.py, 171 launches), so this is
# not a kernel defect: 30 deformable bottlenecks in sequence amplify ANY rounding difference on the spatially white feature maps of a
# random-weight network (torch fp32 vs float64 free-running differ by 1.5 absolute at res4). The bf16 mode on
# UPSNet-101-DCN is a throughput experiment WITHOUT an end-to-end parity claim; the assertion below only pins what was measured.
# UPSNet-50 1024x2048 bf16x3: 0.9998 / 0.9993.
_MODE_AGREE = {('COCO_R101_DCN', 800, 1333, 'bf16'): (0.46, 0.70), ('CITYSCAPES_R50', 1024, 2048, 'bf16x3'): (0.999, 0.99)}


@pytest.mark.parametrize("preset,h,w,precision", [('COCO_R101_DCN', 800, 1333, 'bf16'), ('CITYSCAPES_R50', 1024, 2048, 'bf16x3')])
def test_reduced_precision_modes_at_their_quoted_sizes_stagewise_parity_and_agreement(preset, h, w, precision):
    """VERDICT r04 missing #3 / weak #1b: the two reduced-precision numbers the documents quote without a parity test at their own size --
    UPSNet-101-DCN 800x1333 in the bf16 mode (30 bf16 deformable bottlenecks in sequence) and UPSNet-50 1024x2048 in the bf16x3 mode.
    Every custom-op stage of the mode's forward recomputed by the oracle from its recorded inputs bit for bit (check_taps), label map
    == oracle, and the agreement of the semantic arg-max / panoptic map with the fp32 run of the same image."""
    from oracle.forward import check_taps
    from upsnet_amd.config import config as cfgmod
    from upsnet_amd.config.config import update_config_dict, CITYSCAPES_R50
    from upsnet_amd.models import hipconv
    update_config_dict(getattr(cfgmod, preset))
    try:
        from upsnet_amd.synthetic import build_model, make_image
        model = build_model()
        data = make_image(h, w, seed=1, device='cuda')
        with torch.no_grad():
            ref = {k: v.clone() for k, v in model(data).items()}
            hipconv.PRECISION = precision
            try:
                model.taps = {}
                out = model(data)
                taps, model.taps = model.taps, None
            finally:
                hipconv.PRECISION = 'fp32'
        res = check_taps(taps, enable_void=model.enable_void)
        counts = res.pop('counts')
        assert all(res.values()), (res, counts)
        assert counts['label_mismatch'] == 0 and counts['n_det'] >= 1, counts
        sem = float((out['fcn_outputs'] == ref['fcn_outputs']).float().mean())
        pan = float((out['panoptic_outputs'] == ref['panoptic_outputs']).float().mean())
        print('%s %s vs fp32 at %dx%d: semantic arg-max agreement %.4f, panoptic label-map agreement %.4f, n_det %d / %d, n_inst %d / %d' %
              (preset, precision, h, w, sem, pan, out['cls_inds'].numel(), ref['cls_inds'].numel(), out['panoptic_cls_inds'].numel(),
               ref['panoptic_cls_inds'].numel()))
        want_sem, want_pan = _MODE_AGREE[(preset, h, w, precision)]
        assert sem >= want_sem and pan >= want_pan, (sem, pan)
    finally:
        update_config_dict(CITYSCAPES_R50)


@pytest.mark.parametrize("precision,min_agree", [("bf16x3", 0.999), ("bf16", _BF16_AGREE[(256, 512)][0])])
def test_bf16_matrix_core_convs_end_to_end(setup, precision, min_agree):
    """BASELINE.json configs[2] (and its fp32-equivalent 3-term split): dense convolutions on the bf16 matrix cores. Every custom-op
    stage still reproduces the oracle bit-for-bit from its recorded inputs; the label map agrees with the fp32 run to the extent
    the precision allows (bf16x3: essentially everywhere; bf16: most pixels -- random synthetic weights have no margin)."""
    from oracle.forward import check_taps
    from upsnet_amd.models import hipconv
    model, data = setup
    with torch.no_grad():
        ref = model(data)
        hipconv.PRECISION = precision
        try:
            model.taps = {}
            out = model(data)
            taps, model.taps = model.taps, None
        finally:
            hipconv.PRECISION = 'fp32'
    res = check_taps(taps, enable_void=model.enable_void)
    counts = res.pop('counts')
    assert all(res.values()), (res, counts)
    agree = float((out['fcn_outputs'] == ref['fcn_outputs']).float().mean())
    pan = float((out['panoptic_outputs'] == ref['panoptic_outputs']).float().mean())
    print('%s vs fp32 at 256x512: semantic arg-max agreement %.4f, panoptic label-map agreement %.4f' % (precision, agree, pan))
    assert agree >= min_agree, agree
    assert pan >= (0.99 if precision == 'bf16x3' else _BF16_AGREE[(256, 512)][1]), pan


@pytest.mark.parametrize("overlap", [True, False])
def test_hip_graph_replay_equals_eager(setup, overlap):
    """The static-shape part of the forward (trunk, semantic head on the side stream, proposal / detection chain) is captured as a
    HIP graph on the third image of a shape; replays must equal the eager forward on every output, for changing images of that
    shape and when another shape is interleaved. overlap=False: the purely LINEAR capture (UPSNET_OVERLAP=0) with one and with
    two instances -- the configuration that faulted on the GPU at replay in r01-r05 (root cause: hipMemsetAsync nodes captured
    into a linear graph; the forward now zero-fills with kernels, csrc/fill.hip)."""
    from upsnet_amd.synthetic import make_image
    model, _ = setup
    was_overlap, model.overlap_streams = model.overlap_streams, overlap
    imgs = [make_image(256, 512, seed=11 + j, device='cuda') for j in range(3)] + [make_image(192, 320, seed=20, device='cuda')]
    keys = ('panoptic_outputs', 'pred_boxes', 'cls_probs', 'cls_inds', 'mask_probs', 'panoptic_cls_inds', 'fcn_outputs')
    with torch.no_grad():
        model.use_graph = False
        eager = [{k: v.clone() for k, v in model(im).items()} for im in imgs]
        model.use_graph = True
        for slots in (1, 2):
            model._graphs.clear()
            model.graph_slots = slots
            # every graph instance of a shape is captured at ITS 3rd visit: shape A, then shape B (index 3) interleaved
            order = [0, 1, 2, 0, 1, 2, 3, 0, 3, 1, 3, 2, 3, 0, 3, 3, 3, 1]
            for step, j in enumerate(order):
                out = model(imgs[j])
                for k in keys:
                    assert torch.equal(out[k], eager[j][k]), (slots, step, j, k)
            assert sum(1 for e in model._graphs.values() for sl in e['slots'] if 'graph' in sl) == 2 * slots
        # two images in flight: launch i+1 before reading i; the outputs of i stay valid while i+1 runs
        order = [0, 1, 2, 0, 3, 3, 1, 2, 3, 0]
        pending = None
        for step, j in enumerate(order + [None]):
            nxt = (j, model.forward_async(imgs[j])) if j is not None else None
            if pending is not None:
                out = pending[1].result()
                for k in keys:
                    assert torch.equal(out[k], eager[pending[0]][k]), ('async', step, pending[0], k)
            pending = nxt
        # a longer run of overlapping replays of both instances of one shape
        pending = None
        for step in range(25):
            j = step % 3
            nxt = (j, model.forward_async(imgs[j]))
            if pending is not None:
                out = pending[1].result()
                assert torch.equal(out['panoptic_outputs'], eager[pending[0]]['panoptic_outputs']), ('stress', step)
                assert torch.equal(out['mask_probs'], eager[pending[0]]['mask_probs']), ('stress', step)
            pending = nxt
        pending[1].result()
    model._graphs.clear()
    model.graph_slots = 2
    model.overlap_streams = was_overlap


def test_hip_graph_fallback_when_assumptions_fail(setup):
    """The in-graph tail assumes every panoptic detection is also a per-class detection (and <= max_det / <= 256 rows). With a
    very low panoptic score threshold that is false: the forward must notice after its single host read and redo the tail
    eagerly -- same outputs as the eager forward."""
    from upsnet_amd.synthetic import make_image
    model, _ = setup
    img = make_image(256, 512, seed=31, device='cuda')
    keys = ('panoptic_outputs', 'pred_boxes', 'cls_probs', 'cls_inds', 'mask_probs', 'panoptic_cls_inds', 'fcn_outputs')
    old, old_det = model.mask_roi_panoptic.score_thresh, model.mask_roi.score_thresh
    model.mask_roi_panoptic.score_thresh = 0.02
    model.mask_roi.score_thresh = 0.97   # few per-class detections, many panoptic ones: most of them are "extra" rows
    try:
        with torch.no_grad():
            model.use_graph = False
            ref = {k: v.clone() for k, v in model(img).items()}
            model.use_graph = True
            model._graphs.clear()
            for step in range(5):
                out = model(img)
                for k in keys:
                    assert torch.equal(out[k], ref[k]), (step, k)
            for step in range(3):
                out = model.forward_async(img).result()
                for k in keys:
                    assert torch.equal(out[k], ref[k]), ('async', step, k)
            ent = next(iter(model._graphs.values()))['slots'][0]
            n_det, n_pan, n_extra, _ = ent['out']['tail']['counters'].tolist()
            assert n_extra > 0 or n_pan > 256 or n_det > ent['out']['max_det'], (n_det, n_pan, n_extra)   # the fallback was exercised
    finally:
        model.mask_roi_panoptic.score_thresh, model.mask_roi.score_thresh = old, old_det
        model._graphs.clear()
