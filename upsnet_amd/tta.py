"""Multi-scale and flip test-time augmentation, merged on the device.

The reference reads config.test.scales[0] only and its test script has no augmentation path, so the rule is this project's own: the
image runs through the network once per augmentation (target size, max size, flip); the semantic scores are resampled into the base
frame and averaged, the proposals of every augmentation are mapped to the base frame and go through the detection selection together,
the mask logits of the final boxes are computed in every augmentation and averaged, and the panoptic tail runs once on the merged
tensors. The three merges are the kernels of csrc/tta.hip (ops.tta_*); everything else is the staged model as forward() runs it.

    config.test.aug_scales = [S, ...]     further target sizes beside config.test.scales[0]
    config.test.aug_flip = True           every scale also mirrored left to right

    config.test.bbox_vote = True          box voting (csrc/box_vote.hip): every kept detection box becomes the
                                          score-weighted mean of the candidates of its class above test.score_thresh whose IoU with
                                          it is >= test.bbox_vote_thresh; on its own it runs this path with the base augmentation alone

    config.test.soft_nms = True           soft-NMS in the class-wise selection (csrc/detect.hip): overlapping candidates
                                          stay with a decayed score (test.soft_nms_method / _sigma / _score_thresh); on its own it
                                          runs this path with the base augmentation alone

The run is eager: no HIP graph, one image in flight. All outputs are in the base frame (the first augmentation, the plain forward's
input), so evaluate.post_image takes them with the base im_info. Whether the augmentations raise PQ has not been measured: no trained
checkpoint exists here."""
import numpy as np
import torch
import torch.nn.functional as F

from . import ops
from ._lib import aligned, check, dense, f32c, float_array, int_array, lib, nhwc, ptr, ptr_array, require_cuda, stream
from .config.config import config
from .operators.modules.mask_roi import check_count, check_count_soft

MAX_AUG = ops.TTA_MAX_AUG
MAX_UNION_ROWS = 8192     # candidate rows the device detection selection takes (csrc/detect.hip)


# ------------------------------------------------------------------------- the four merge launches (csrc/tta.hip), the vote (csrc/box_vote.hip)
def _tta_count(num_aug, what):
    if not 1 <= num_aug <= MAX_AUG:
        raise ValueError("%s: 1..%d augmentations (got %d)" % (what, MAX_AUG, num_aug))


def seg_merge(maps, q, resized_w, flip, cell):
    """the semantic score maps of the augmentations (logical [1,S,Hs_a,Ws_a]; consumed channels-last) resampled
    into the frame of maps[0] and averaged in the given order. q[a] = s_a / s_0 (float32), resized_w[a] = Wr_a, flip[a]; cell = 4
    for the quarter-resolution score map, 1 for the full-resolution one. Returns a channels-last [1,S,Hb,Wb] tensor; one launch."""
    _tta_count(len(maps), "tta_seg_merge")
    require_cuda(*maps)
    maps = [nhwc(t.float()) for t in maps]
    _, S, Hb, Wb = maps[0].shape
    for t in maps:
        if t.dim() != 4 or t.shape[0] != 1 or t.shape[1] != S:
            raise ValueError("tta_seg_merge: every map must be [1,%d,H,W], got %s" % (S, tuple(t.shape)))
    out = ops._nhwc_out(1, S, Hb, Wb, maps[0].device)
    check(lib().upsnet_tta_seg_merge(stream(), len(maps), ptr_array(maps), int_array([t.shape[2] for t in maps]),
                                     int_array([t.shape[3] for t in maps]), float_array(q), float_array(resized_w),
                                     int_array([bool(f) for f in flip]), int(cell), S, Hb, Wb, ptr(out)), "tta_seg_merge")
    return out


def roi_union(rois, delta, prob, num_rois_dev, r, resized_w, flip):
    """the valid proposal rows of every augmentation (rois[a] [R,5], delta[a] [R,D], prob[a] [R,C], device
    count num_rois_dev[a] int32 [1]) mapped to the base frame (r[a] = s_0 / s_a, float32) and packed behind each other. Returns
    (rois [A*R,5], delta [A*R,D], prob [A*R,C], num int32 [1]); rows past num are zero. One launch, no host read."""
    A = len(rois)
    _tta_count(A, "tta_roi_union")
    require_cuda(*rois, *delta, *prob, *num_rois_dev)
    rois, delta, prob = [f32c(t) for t in rois], [f32c(t) for t in delta], [f32c(t) for t in prob]
    R, D, C = rois[0].shape[0], delta[0].shape[1], prob[0].shape[1]
    for a in range(A):
        if tuple(rois[a].shape) != (R, 5) or tuple(delta[a].shape) != (R, D) or tuple(prob[a].shape) != (R, C):
            raise ValueError("tta_roi_union: augmentation %d has shapes %s %s %s, expected %s %s %s"
                             % (a, tuple(rois[a].shape), tuple(delta[a].shape), tuple(prob[a].shape), (R, 5), (R, D), (R, C)))
        if num_rois_dev[a].dtype != torch.int32 or num_rois_dev[a].numel() != 1:
            raise ValueError("tta_roi_union: the count of augmentation %d must be one int32" % a)
    num_rois_dev = [dense(t) for t in num_rois_dev]
    if A * R > 8192:
        raise ValueError("tta_roi_union: %d x %d rows exceed the 8192 the detection selection takes" % (A, R))
    dev = rois[0].device
    rois_out = torch.empty((A * R, 5), dtype=torch.float32, device=dev)
    delta_out = torch.empty((A * R, D), dtype=torch.float32, device=dev)
    prob_out = torch.empty((A * R, C), dtype=torch.float32, device=dev)
    num = torch.empty((1,), dtype=torch.int32, device=dev)
    check(lib().upsnet_tta_roi_union(stream(), A, ptr_array(rois), ptr_array(delta), ptr_array(prob), ptr_array(num_rois_dev),
                                     float_array(r), float_array(resized_w), int_array([bool(f) for f in flip]), R, D, C,
                                     ptr(rois_out), ptr(delta_out), ptr(prob_out), ptr(num)), "tta_roi_union")
    return rois_out, delta_out, prob_out, num


def boxes_to_aug(boxes, q, resized_w, flip):
    """boxes [n,5] of the base frame mapped into every augmentation's frame, [A,n,5]; one launch."""
    A = len(q)
    _tta_count(A, "tta_boxes_to_aug")
    require_cuda(boxes)
    boxes = f32c(boxes)
    if boxes.dim() != 2 or boxes.shape[1] != 5:
        raise ValueError("tta_boxes_to_aug: boxes must be [n,5], got %s" % (tuple(boxes.shape),))
    n = boxes.shape[0]
    out = torch.empty((A, n, 5), dtype=torch.float32, device=boxes.device)
    check(lib().upsnet_tta_boxes_to_aug(stream(), A, float_array(q), float_array(resized_w), int_array([bool(f) for f in flip]),
                                        ptr(boxes) if n else None, n, ptr(out) if n else None), "tta_boxes_to_aug")
    return out


def mask_merge(logits, flip):
    """the mask logits of the augmentations ([n,C,ms,ms] each, rows = the same final boxes) averaged in the given
    order, a flipped augmentation read mirrored left to right. The result has the memory layout of logits[0] (NCHW or channels-last)."""
    A = len(logits)
    _tta_count(A, "tta_mask_merge")
    require_cuda(*logits)
    first = logits[0].float()
    n, C, ms, ms2 = first.shape
    if ms != ms2:
        raise ValueError("tta_mask_merge: square masks expected, got %s" % (tuple(first.shape),))
    is_nhwc = (not first.is_contiguous()) and first.is_contiguous(memory_format=torch.channels_last)
    fmt = torch.channels_last if is_nhwc else torch.contiguous_format
    logits = [aligned(t.float().contiguous(memory_format=fmt)) for t in logits]
    for t in logits:
        if tuple(t.shape) != (n, C, ms, ms):
            raise ValueError("tta_mask_merge: shapes differ: %s and %s" % (tuple(t.shape), (n, C, ms, ms)))
    out = ops._nhwc_out(n, C, ms, ms, first.device) if is_nhwc else torch.empty((n, C, ms, ms), dtype=torch.float32, device=first.device)
    check(lib().upsnet_tta_mask_merge(stream(), A, ptr_array(logits) if n else ptr_array([None] * A), int_array([bool(f) for f in flip]),
                                      n, C, ms, int(is_nhwc), ptr(out) if n else None), "tta_mask_merge")
    return out


def box_vote(rois, bbox_delta, cls_prob, im_info, boxes, cls, num, vote_score_thresh, vote_iou_thresh, reg_weights,
             num_rois_dev=None, clip_boxes=True):
    """Score-weighted box voting (csrc/box_vote.hip) on the output of mask_roi: boxes [cap,5], cls [cap] int64, num device
    int32, with the rois / bbox_delta / cls_prob / im_info / reg_weights / num_rois_dev / clip_boxes the selection was given. Returns
    voted [cap,5]: row k < num is the mean of the class-cls[k] candidates with cls_prob > vote_score_thresh and IoU >= vote_iou_thresh
    with boxes[k], weighted by cls_prob; rows from num on are copies. One launch, no host read."""
    require_cuda(rois, bbox_delta, cls_prob, im_info, boxes, cls, num)
    rois, bbox_delta, cls_prob, boxes, cls = f32c(rois), f32c(bbox_delta), f32c(cls_prob), f32c(boxes), dense(cls)
    N, C = cls_prob.shape
    cap = boxes.shape[0]
    if tuple(rois.shape) != (N, 5) or bbox_delta.dim() != 2 or tuple(bbox_delta.shape) != (N, 4 * C):
        raise ValueError("box_vote: rois %s / bbox_delta %s do not go with cls_prob %s (class-wise deltas: [N,5], [N,4C], [N,C])"
                         % (tuple(rois.shape), tuple(bbox_delta.shape), (N, C)))
    if boxes.dim() != 2 or boxes.shape[1] != 5 or tuple(cls.shape) != (cap,) or cls.dtype != torch.int64:
        raise ValueError("box_vote: boxes must be [cap,5] and cls int64 [cap], got %s and %s %s" % (tuple(boxes.shape), cls.dtype, tuple(cls.shape)))
    if num.dtype != torch.int32 or num.numel() != 1 or (num_rois_dev is not None and (num_rois_dev.dtype != torch.int32 or num_rois_dev.numel() != 1)):
        raise ValueError("box_vote: the counts must be one int32 each")
    num, num_rois_dev = dense(num), dense(num_rois_dev)
    voted = torch.empty((cap, 5), dtype=torch.float32, device=boxes.device)
    im_info = f32c(im_info.reshape(-1))
    check(lib().upsnet_box_vote(stream(), ptr(rois), ptr(bbox_delta), ptr(cls_prob), N, ptr(num_rois_dev), C,
                                ptr(im_info), int(bool(clip_boxes)), float_array(reg_weights), float(vote_score_thresh),
                                float(vote_iou_thresh), ptr(boxes) if cap else None, ptr(cls) if cap else None, ptr(num), cap,
                                ptr(voted) if cap else None), "box_vote")
    return voted


SOFT_NMS_METHODS = {'linear': 1, 'gaussian': 2}      # cpu_soft_nms's numbering (0 is the hard rule)


def mask_roi_soft(rois, bbox_delta, cls_prob, im_info, score_thresh, nms_thresh, max_det, reg_weights, method, sigma, floor,
                  num_rois_dev=None, clip_boxes=True):
    """The class-wise detection selection with soft-NMS (csrc/detect.hip mroi_soft_kernel): per class cpu_soft_nms(sigma,
    Nt = nms_thresh, threshold = floor, method 0 hard / 1 linear / 2 gaussian) on the candidates above score_thresh, then the
    top-max_det rule on the decayed scores. Returns fixed-capacity (boxes [cap,5], scores [cap], cls [cap] int64, src [cap] int32, num
    device int32) as ops.mask_roi; a negative num reports a class of more than 4096 candidates. Two launches, no host read."""
    require_cuda(rois, bbox_delta, cls_prob, im_info)
    rois, bbox_delta, cls_prob = f32c(rois), f32c(bbox_delta), f32c(cls_prob)
    if cls_prob.dim() != 2:
        raise ValueError("mask_roi_soft: cls_prob must be [N,C], got %s" % (tuple(cls_prob.shape),))
    N, C = cls_prob.shape
    if tuple(rois.shape) != (N, 5) or tuple(bbox_delta.shape) != (N, 4 * C):
        raise ValueError("mask_roi_soft: rois %s / bbox_delta %s do not go with cls_prob %s (class-wise deltas: [N,5], [N,4C], [N,C])"
                         % (tuple(rois.shape), tuple(bbox_delta.shape), (N, C)))
    if num_rois_dev is not None and (num_rois_dev.dtype != torch.int32 or num_rois_dev.numel() != 1):
        raise ValueError("mask_roi_soft: the row count must be one int32")
    num_rois_dev = dense(num_rois_dev)
    dev = rois.device
    cap = lib().upsnet_mask_roi_capacity(max(N, 1), max(C, 2), 0)
    boxes = torch.empty((cap, 5), dtype=torch.float32, device=dev)
    scores = torch.empty((cap,), dtype=torch.float32, device=dev)
    cls = torch.empty((cap,), dtype=torch.int64, device=dev)
    src = torch.empty((cap,), dtype=torch.int32, device=dev)
    num = torch.empty((1,), dtype=torch.int32, device=dev)
    ws = torch.empty((int(lib().upsnet_mask_roi_soft_workspace_bytes(N, C)),), dtype=torch.uint8, device=dev)
    im_info = f32c(im_info.reshape(-1))
    check(lib().upsnet_mask_roi_soft(stream(), ptr(rois), ptr(bbox_delta), ptr(cls_prob), N, ptr(num_rois_dev), C,
                                     ptr(im_info), int(bool(clip_boxes)), float(score_thresh), float(nms_thresh),
                                     int(max_det), float_array(reg_weights), int(method), float(sigma), float(floor), ptr(boxes),
                                     ptr(scores), ptr(cls), ptr(src), ptr(num), ptr(ws)), "mask_roi_soft")
    return boxes, scores, cls, src, num


# ------------------------------------------------------------------------------------------------ the augmented forward
def augmentation_enabled(cfg=None):
    t = (config if cfg is None else cfg).test
    return bool(list(t.get('aug_scales', []) or [])) or bool(t.get('aug_flip', False))


def bbox_vote_params(cfg=None):
    """(vote_score_thresh, vote_iou_thresh) when config.test.bbox_vote is on, else None. The score threshold is always
    test.score_thresh, for the class-wise and the panoptic selection alike."""
    t = (config if cfg is None else cfg).test
    if not t.get('bbox_vote', False):
        return None
    iou = float(t.get('bbox_vote_thresh', 0.8))
    if not iou > 0.0:
        raise ValueError("test.bbox_vote_thresh must be a positive IoU (got %r)" % (t.get('bbox_vote_thresh'),))
    return float(t.score_thresh), iou


def soft_nms_params(cfg=None):
    """(method, sigma, floor) when config.test.soft_nms is on, else None: method in cpu_soft_nms's numbering (1 linear,
    2 gaussian), floor = test.soft_nms_score_thresh, the score below which a decayed candidate is dropped."""
    t = (config if cfg is None else cfg).test
    if not t.get('soft_nms', False):
        return None
    name = t.get('soft_nms_method', 'linear')
    if name not in SOFT_NMS_METHODS:
        raise ValueError("test.soft_nms_method must be one of %s (got %r)" % (sorted(SOFT_NMS_METHODS), name))
    sigma, floor = float(t.get('soft_nms_sigma', 0.5)), float(t.get('soft_nms_score_thresh', 0.0001))
    if not sigma > 0.0:
        raise ValueError("test.soft_nms_sigma must be positive (got %r)" % (t.get('soft_nms_sigma'),))
    if not floor >= 0.0:
        raise ValueError("test.soft_nms_score_thresh must not be negative (got %r)" % (t.get('soft_nms_score_thresh'),))
    return SOFT_NMS_METHODS[name], sigma, floor


def eager_path_enabled(cfg=None):
    """Whether the evaluation run goes through forward_tta: test-time augmentation, or box voting or soft-NMS (which live on that path
    only; on their own they run the base augmentation alone)."""
    t = (config if cfg is None else cfg).test
    return augmentation_enabled(cfg) or bool(t.get('bbox_vote', False)) or bool(t.get('soft_nms', False))


def augmentation_list(cfg=None):
    """[(target_size, max_size, flip)]: the base (scales[0], max_size, False) first; for each scale S of [scales[0]] + aug_scales, in
    order, (S, M_S, False) and with aug_flip (S, M_S, True) directly after, M_S = int(round(max_size * S / scales[0])).
    ValueError when the list has more than 8 entries or len(list) * rpn_post_nms_top_n exceeds 8192; nothing is clamped."""
    t = (config if cfg is None else cfg).test
    s0 = t.scales[0]
    flip = bool(t.get('aug_flip', False))
    augs = []
    for S in [s0] + list(t.get('aug_scales', []) or []):
        m = int(round(t.max_size * S / s0))
        augs.append((S, m, False))
        if flip:
            augs.append((S, m, True))
    if not 1 <= len(augs) <= MAX_AUG:
        raise ValueError("test-time augmentation: %d augmentations (scales %s%s), at most %d are supported"
                         % (len(augs), [a[0] for a in augs if not a[2]], ', each flipped' if flip else '', MAX_AUG))
    if len(augs) * int(t.rpn_post_nms_top_n) > MAX_UNION_ROWS:
        raise ValueError("test-time augmentation: %d augmentations x rpn_post_nms_top_n %d = %d proposal rows, the detection selection "
                         "takes at most %d; lower test.rpn_post_nms_top_n or use fewer augmentations"
                         % (len(augs), int(t.rpn_post_nms_top_n), len(augs) * int(t.rpn_post_nms_top_n), MAX_UNION_ROWS))
    return augs


def _stage(model, data, fuse_up):
    """One augmentation up to the box head, eagerly: (feats, score, rois, n_rois, delta, prob)."""
    from .models.rpn import rpn_forward_levels
    pyramid = model._pyramid({'data': data['data']})
    feats = list(pyramid[:4])
    score = model.fcn_head.forward_score(*feats) if fuse_up else model.fcn_head(*feats)['fcn_output']
    _, rpn_bbox_pred, rpn_cls_prob = rpn_forward_levels(model.rpn, list(pyramid))
    rois, _, n_rois = model.pyramid_proposal.forward_padded(rpn_cls_prob, rpn_bbox_pred, data['im_info'])
    rcnn_output = model.rcnn(feats, rois, n_rois)
    return feats, score, rois, n_rois, rcnn_output['bbox_pred'], F.softmax(rcnn_output['cls_score'], dim=1)


def forward_tta(model, image_u8_bgr, device=None, return_parts=False):
    """image_u8_bgr: the decoded uint8 [H,W,3] BGR image (numpy array or tensor). Returns the output dict of model.forward() for the
    base blob, computed from all augmentations of augmentation_list(config); with return_parts also a dict of the per-augmentation
    tensors, the merged tensors, the selections and the final boxes (what the tests check each merge from)."""
    from .dataset.blob import get_image_blob
    augs = augmentation_list()
    vote = bbox_vote_params()
    soft = soft_nms_params()
    if getattr(model, 'keep_proposals', False):
        raise ValueError("keep_proposals (--eval_proposals) with test-time augmentation: there is no single proposal list to keep")
    if isinstance(image_u8_bgr, np.ndarray):
        image_u8_bgr = torch.from_numpy(np.ascontiguousarray(image_u8_bgr))
    if device is None:
        device = image_u8_bgr.device if image_u8_bgr.is_cuda else torch.device('cuda', torch.cuda.current_device())
    image_u8_bgr = image_u8_bgr.to(device, non_blocking=True)      # one upload for all augmentations
    fuse_up = model.enable_void and model.fcn_head.upsample_rate == 4
    cell = 4 if fuse_up else 1
    A = len(augs)
    with torch.no_grad():
        im_infos, stages = [], []
        for target, max_size, flip in augs:
            img = torch.flip(image_u8_bgr, [1]).contiguous() if flip else image_u8_bgr
            data = get_image_blob(img, target, max_size, device=device)
            im_infos.append(np.asarray(data['im_info'], dtype=np.float32).reshape(-1)[:3])
            stages.append(_stage(model, data, fuse_up))
        s0 = im_infos[0][2]
        q = [np.float32(im[2]) / np.float32(s0) for im in im_infos]     # float32 divisions, made once on the host
        r = [np.float32(s0) / np.float32(im[2]) for im in im_infos]
        wr = [np.float32(im[1]) for im in im_infos]
        flips = [a[2] for a in augs]
        im_info0 = im_infos[0].reshape(1, 3)

        score = ops.tta_seg_merge([s[1] for s in stages], q, wr, flips, cell)
        rois, delta, prob, n_rois = ops.tta_roi_union([s[2] for s in stages], [s[4] for s in stages], [s[5] for s in stages],
                                                      [s[3] for s in stages], r, wr, flips)
        # with soft-NMS the class-wise selection keeps the union's overlapping candidates with decayed scores; the
        # panoptic selection stays hard (the panoptic head wants a non-overlapping instance set)
        det_boxes, det_scores, det_cls, det_src, det_num = model.mask_roi.forward_padded(rois, delta, prob, im_info0, n_rois, soft_nms=soft)
        pan_boxes, pan_scores, pan_cls, pan_src, pan_num = model.mask_roi_panoptic.forward_padded(rois, delta, prob, im_info0, n_rois)
        det_boxes_prevote, pan_boxes_prevote = det_boxes, pan_boxes
        if vote is not None:
            # both kept lists voted on the union, before the dedup: it pairs rows by (source ROI, class), and such rows get
            # the same voted box from either list, so extra_boxes come out voted and "same ROI, same class, same mask logits" holds
            w = config.network.bbox_reg_weights
            im0 = torch.from_numpy(im_infos[0].copy()).to(rois.device, non_blocking=True)
            det_boxes = ops.box_vote(rois, delta, prob, im0, det_boxes, det_cls, det_num, vote[0], vote[1], w, n_rois,
                                     clip_boxes=bool(model.mask_roi.clip_boxes))
            pan_boxes = ops.box_vote(rois, delta, prob, im0, pan_boxes, pan_cls, pan_num, vote[0], vote[1], w, n_rois,
                                     clip_boxes=bool(model.mask_roi_panoptic.clip_boxes))
        pan_row, extra_boxes, extra_num = ops.mask_roi_dedup(det_src, det_cls, det_num, pan_src, pan_cls, pan_boxes, pan_num)
        n_det, n_pan, n_extra = torch.cat([det_num, pan_num, extra_num]).tolist()
        (check_count if soft is None else check_count_soft)(n_det), check_count(n_pan)
        det_boxes, det_scores, det_cls = det_boxes[:n_det], det_scores[:n_det], det_cls[:n_det]
        pan_boxes, pan_scores, pan_cls = pan_boxes[:n_pan], pan_scores[:n_pan], pan_cls[:n_pan]
        det_boxes_prevote, pan_boxes_prevote = det_boxes_prevote[:n_det], pan_boxes_prevote[:n_pan]

        boxes = torch.cat([det_boxes, extra_boxes[:n_extra]], 0) if n_extra else det_boxes
        n = boxes.shape[0]
        boxes_aug = ops.tta_boxes_to_aug(boxes, q, wr, flips)
        ms = config.network.mask_size
        if n:
            logits = [model.mask_branch(stages[a][0], boxes_aug[a]) for a in range(A)]
        else:
            logits = [torch.zeros((0, model.num_classes, ms, ms), dtype=torch.float32, device=boxes.device) for _ in range(A)]
        mask_score = ops.tta_mask_merge(logits, flips)
        out = _tail(model, score, fuse_up, mask_score, n_det, n_pan, det_boxes, det_scores, det_cls, pan_boxes, pan_scores, pan_cls, pan_row)
    if not return_parts:
        return out
    parts = dict(augs=augs, im_info=im_infos, q=q, r=r, resized_w=wr, flip=flips, cell=cell,
                 score=[s[1] for s in stages], rois=[s[2] for s in stages], n_rois=[s[3] for s in stages],
                 delta=[s[4] for s in stages], prob=[s[5] for s in stages], mask_logits=logits, boxes_aug=boxes_aug,
                 feats=[s[0] for s in stages],
                 merged_score=score, merged_rois=rois, merged_delta=delta, merged_prob=prob, merged_n_rois=n_rois,
                 merged_mask_logits=mask_score, boxes=boxes, n_det=n_det, n_pan=n_pan, n_extra=n_extra,
                 det_boxes=det_boxes, det_scores=det_scores, det_cls=det_cls, pan_boxes=pan_boxes, pan_scores=pan_scores,
                 pan_cls=pan_cls, pan_row=pan_row, extra_boxes=extra_boxes, det_boxes_prevote=det_boxes_prevote,
                 pan_boxes_prevote=pan_boxes_prevote, bbox_vote=vote, soft_nms=soft)
    return out, parts


def _tail(model, score, fuse_up, mask_score, n_det, n_pan, det_boxes, det_scores, det_cls, pan_boxes, pan_scores, pan_cls, pan_row):
    """The eager continuation of resnet_upsnet._forward_fused on the merged tensors: mask probabilities, the panoptic logits' row and
    class gather, mask removal, the panoptic fusion and the output dictionary."""
    ms = config.network.mask_size
    fcn_score, fcn_output = (score, None) if fuse_up else (None, score)
    H, W = (fcn_score.shape[2] * 4, fcn_score.shape[3] * 4) if fuse_up else fcn_output.shape[2:]
    mask_prob = torch.sigmoid(mask_score[:n_det])
    pan_logit = mask_score.index_select(0, pan_row[:n_pan].long()).gather(1, pan_cls.view(-1, 1, 1, 1).expand(-1, -1, ms, ms))
    keep, num_keep, real_keep = model.mask_removal.select(pan_boxes[:, 1:], pan_scores, pan_logit, pan_cls, (H, W))
    panoptic, sem, conf = model._panoptic_fusion(fcn_score, fcn_output, n_pan, pan_boxes, pan_logit, pan_cls, keep, num_keep, real_keep)
    keep = keep[:int(num_keep.item())]
    out = {
        'cls_probs': det_scores, 'pred_boxes': det_boxes, 'mask_probs': mask_prob, 'fcn_outputs': sem,
        'cls_inds': det_cls, 'panoptic_cls_inds': pan_cls[keep], 'panoptic_cls_probs': pan_scores[keep],
        'panoptic_outputs': panoptic,
    }
    if conf is not None:
        out['panoptic_conf'] = conf
    return out
