"""Global configuration of the inference path.

Mirrors upsnet/config/config.py:20-198 of the reference (same field names and defaults, same
``update_config(yaml)`` entry point) without the easydict dependency. Only the fields that
parameterise the inference hot path are kept (SURVEY.md section 5 "Config / flags").
"""
import numpy as np
import yaml


class AttrDict(dict):
    """Minimal easydict stand-in: attribute access, nested dicts converted on assignment."""

    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError:
            raise AttributeError(k)

    def __setattr__(self, k, v):
        self[k] = AttrDict(v) if isinstance(v, dict) and not isinstance(v, AttrDict) else v


config = AttrDict()
config.symbol = 'resnet_50_upsnet'
config.gpus = '0'

config.network = AttrDict()
config.network.backbone_fix_bn = True
config.network.backbone_with_dilation = False
config.network.backbone_with_dpyramid = False
config.network.backbone_with_dconv = 100
config.network.backbone_freeze_at = 2
config.network.use_caffe_model = True
config.network.use_syncbn = False
config.network.has_rcnn = True
config.network.has_mask_head = True
config.network.has_fcn_head = True
config.network.has_panoptic_head = True
config.network.pixel_means = np.array((102.9801, 115.9465, 122.7717,))
config.network.cls_agnostic_bbox_reg = False
config.network.rcnn_feat_stride = 32
config.network.bbox_reg_weights = (10., 10., 5., 5.,)
config.network.rpn_feat_stride = (4, 8, 16, 32, 64,)
config.network.anchor_ratios = (0.5, 1, 2)
config.network.anchor_scales = (8,)
config.network.num_anchors = 3
config.network.rpn_with_norm = 'none'
config.network.has_fpn = True
config.network.fpn_feature_dim = 256
config.network.fpn_with_gap = False
config.network.fpn_upsample_method = 'nearest'
config.network.fpn_with_norm = 'none'
config.network.rcnn_with_norm = 'none'
config.network.mask_size = 28
config.network.binary_thresh = 0.5
config.network.has_mask_rcnn = True
config.network.fcn_with_norm = 'none'
config.network.fcn_num_layers = 3
config.network.fcn_head = 'FCNHead'

config.dataset = AttrDict()
config.dataset.num_classes = 9        # Cityscapes defaults (upsnet_resnet50_cityscapes_16gpu.yaml)
config.dataset.num_seg_classes = 19

config.train = AttrDict()
config.train.use_horovod = False
config.train.rpn_individual_proposals = True
config.train.panoptic_box_keep_fraction = 0.7
config.train.fcn_with_roi_loss = False
config.train.gt_min_area = -1             # JsonDataset._add_gt_annotations: GTs of a smaller JSON area are dropped

config.test = AttrDict()
config.test.rpn_nms_thresh = 0.7
config.test.rpn_pre_nms_top_n = 1000
config.test.rpn_post_nms_top_n = 1000
config.test.rpn_min_size = 0
config.test.nms_thresh = 0.5
config.test.max_det = 100
config.test.score_thresh = 0.05
config.test.panoptic_score_thresh = 0.6
config.test.panoptic_stuff_area_limit = 4096
config.test.batch_size = 1
config.test.scales = [1024]
config.test.max_size = 2048
config.test.vis_mask = False          # upsnet_end2end_test.py:172-173, 300-301: draw the detections instead of scoring them
# multi-scale / flip test-time augmentation (upsnet_amd/tta.py; the reference reads scales[0] only): further target sizes
# beside scales[0], and whether every scale is also run mirrored left to right. Both off: the plain single-scale forward.
config.test.aug_scales = []
config.test.aug_flip = False
# box voting on the augmented (eager) path (csrc/box_vote.hip; the reference has none): every kept detection box becomes
# the score-weighted mean of the candidates of its class above test.score_thresh whose IoU with it is >= bbox_vote_thresh. On its own
# (no aug_scales / aug_flip) the evaluation run takes the eager path with the base augmentation alone.
config.test.bbox_vote = False
config.test.bbox_vote_thresh = 0.8
# soft-NMS in the class-wise detection selection of the augmented (eager) path (csrc/detect.hip mroi_soft_kernel; Detectron's
# TEST.SOFT_NMS): a candidate that overlaps a kept one stays with a decayed score ('linear': x (1 - IoU) above test.nms_thresh;
# 'gaussian': x exp(-IoU^2 / sigma)) and is dropped only below soft_nms_score_thresh. The panoptic selection stays hard NMS. On its
# own (no aug_scales / aug_flip) the evaluation run takes the eager path with the base augmentation alone.
config.test.soft_nms = False
config.test.soft_nms_method = 'linear'
config.test.soft_nms_sigma = 0.5
config.test.soft_nms_score_thresh = 0.0001
# disconnected fragments of the panoptic predictions (csrc/pan_components.hip; the reference has none): with
# pan_min_component > 0 every connected component (4- or 8-connectivity) of a (category, instance) pair with fewer pixels than that
# becomes VOID before the maps are scored, written, drawn or tracked; with keep_largest the largest component of a pair always stays.
config.test.pan_min_component = 0
config.test.pan_component_connectivity = 8
config.test.pan_component_keep_largest = True
# 'void': such a component becomes VOID; 'absorb' (DESIGN 4.27): it takes the (category, instance) of the kept segment it shares the
# longest border with, and becomes VOID only where it borders none
config.test.pan_component_mode = 'void'
# panoptic confidence (csrc/panoptic.hip: panoptic_fuse_up_conf_kernel, csrc/pan_confidence.hip; the reference keeps the
# arg-max only): with pan_confidence the model also returns 'panoptic_conf', one byte per pixel = 255 x the softmax over the panoptic
# logits at the winning label; the evaluation then writes a "score" per segment. pan_min_score > 0 (implies pan_confidence) turns every
# unified segment whose mean confidence is below it into VOID before the maps are cleaned, scored, written or drawn.
config.test.pan_confidence = False
config.test.pan_min_score = 0.0


def pan_confidence_wanted():
    """config.test.pan_confidence, or a pan_min_score that needs it"""
    return bool(config.test.get('pan_confidence', False)) or config.test.get('pan_min_score', 0.0) > 0


def _merge(dst, src):
    for k, v in src.items():
        if isinstance(v, dict):
            if k not in dst or not isinstance(dst[k], dict):
                dst[k] = AttrDict()
            _merge(dst[k], v)
        else:
            if k in ('bbox_reg_weights', 'anchor_ratios', 'anchor_scales', 'rpn_feat_stride') and isinstance(v, list):
                v = tuple(v)
            dst[k] = v


def update_config(config_file):
    """config.py:177-198: merge a reference experiment yaml into the global config."""
    with open(config_file) as f:
        exp = yaml.safe_load(f)
    _merge(config, exp)
    return config


def update_config_dict(d):
    _merge(config, d)
    return config


# experiment presets equivalent to the reference yamls that matter for the benchmark configs
CITYSCAPES_R50 = dict(symbol='resnet_50_upsnet', dataset=dict(num_classes=9, num_seg_classes=19),
                      network=dict(fcn_num_layers=2, fpn_with_gap=False, backbone_with_dconv=100),
                      test=dict(rpn_post_nms_top_n=1000, rpn_pre_nms_top_n=1000, scales=[1024], max_size=2048),
                      train=dict(panoptic_box_keep_fraction=0.7))
COCO_R101_DCN = dict(symbol='resnet_101_upsnet', dataset=dict(num_classes=81, num_seg_classes=133),
                     network=dict(fcn_num_layers=3, fpn_with_gap=True, backbone_with_dconv=3),
                     test=dict(rpn_post_nms_top_n=300, rpn_pre_nms_top_n=1000, scales=[800], max_size=1333),
                     train=dict(panoptic_box_keep_fraction=0.7))
