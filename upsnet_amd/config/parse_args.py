"""Command line of the reference's entry points (upsnet/config/parse_args.py:17-31): `--cfg <experiment yaml>` is merged into the
global config before anything else is parsed; `--eval_only`, `--weight_path` as in the reference. Extra options of this
implementation (synthetic workload, steps) are accepted too, so that one parser serves both spellings of the entry point."""
import argparse

from .config import config, update_config


def add_pan_component_arguments(parser, before):
    """--pan_min_component / --pan_component_connectivity of the evaluation and the sequence command lines."""
    parser.add_argument('--pan_min_component', type=int, default=None, metavar='N',
                        help='sets config.test.pan_min_component: every connected component of a (category, instance) pair with fewer '
                        'than N pixels becomes VOID in the panoptic predictions before they are %s (on the device); the largest '
                        'component of a pair always stays (test.pan_component_keep_largest); 0 = off' % before)
    parser.add_argument('--pan_component_connectivity', type=int, default=None, metavar='{4,8}',
                        help='with --pan_min_component: sets config.test.pan_component_connectivity, 4 or 8 (default 8)')
    parser.add_argument('--pan_component_mode', default=None, metavar='{void,absorb}',
                        help='with --pan_min_component: sets config.test.pan_component_mode. void (default): such a component becomes '
                        'VOID; absorb: it takes the (category, instance) of the segment it shares the longest border with, and becomes '
                        'VOID only where it borders none')


def apply_pan_component_arguments(args, fail):
    """The three options into config.test, once the yaml is merged; then the resulting values are checked, whichever of the two set them.
    fail(message) ends the run (parser.error, or a SystemExit): every message names the option or the yaml key."""
    if args.pan_min_component is not None:
        if args.pan_min_component < 0:
            fail('--pan_min_component must be an integer >= 0, got %d' % args.pan_min_component)
        config.test.pan_min_component = int(args.pan_min_component)
    if args.pan_component_connectivity is not None:
        if not config.test.get('pan_min_component', 0):
            fail('--pan_component_connectivity is a parameter of --pan_min_component, which is missing')
        if args.pan_component_connectivity not in (4, 8):
            fail('--pan_component_connectivity must be 4 or 8, got %d' % args.pan_component_connectivity)
        config.test.pan_component_connectivity = int(args.pan_component_connectivity)
    if args.pan_component_mode is not None:
        if not config.test.get('pan_min_component', 0):
            fail('--pan_component_mode is a parameter of --pan_min_component, which is missing')
        if args.pan_component_mode not in ('void', 'absorb'):
            fail("--pan_component_mode must be void or absorb, got %r" % (args.pan_component_mode,))
        config.test.pan_component_mode = args.pan_component_mode
    n, c = config.test.get('pan_min_component', 0), config.test.get('pan_component_connectivity', 8)
    if isinstance(n, bool) or not isinstance(n, int) or n < 0:
        fail('test.pan_min_component must be an integer >= 0, got %r' % (n,))
    if isinstance(c, bool) or c not in (4, 8):
        fail('test.pan_component_connectivity must be 4 or 8, got %r' % (c,))
    if not isinstance(config.test.get('pan_component_keep_largest', True), bool):
        fail('test.pan_component_keep_largest must be true or false, got %r' % (config.test.pan_component_keep_largest,))
    if config.test.get('pan_component_mode', 'void') not in ('void', 'absorb'):
        fail("test.pan_component_mode must be void or absorb, got %r" % (config.test.pan_component_mode,))


def parse_args(description='', argv=None):
    parser = argparse.ArgumentParser(description=description)
    parser.add_argument('--cfg', help='experiment configure file name', required=False, type=str, default='')
    parser.add_argument('--eval_only', help='if only eval existing results', action='store_true')
    parser.add_argument('--weight_path', help='manually specify model weights', type=str, default='')
    parser.add_argument('--workload', help='synthetic workload (upsnet_amd.upsnet_end2end_test.WORKLOADS): the config preset when --cfg is '
                        'absent (default upsnet50_cityscapes_1024x2048); with --cfg only its image sizes', type=str, default='')
    parser.add_argument('--synthetic_weights', action='store_true',
                        help='with --cfg and no --weight_path: seeded synthetic weights instead of the default checkpoint path')
    parser.add_argument('--steps', type=int, default=20)
    parser.add_argument('--warmup', type=int, default=10)
    parser.add_argument('--in-flight', type=int, default=1, help='images in flight per rank (1 = the reference loop)')
    parser.add_argument('--pan_combined', action='store_true',
                        help='also score the combined (heuristic merge) panoptic result of the detections and the semantic map')
    parser.add_argument('--eval_proposals', action='store_true',
                        help='also keep the RPN proposals of every image and score their recall (AR@100/300/1000, all/small/medium/large)')
    parser.add_argument('--eval_boundary', action='store_true',
                        help='also score the instance masks with Boundary AP (COCOeval with IoU = min(mask IoU, boundary IoU)); needs '
                        'a mask head')
    parser.add_argument('--boundary_dilation_ratio', type=float, default=None, metavar='R',
                        help='with --eval_boundary: the boundary width as a fraction of the image diagonal (default 0.02)')
    parser.add_argument('--eval_boundary_pq', action='store_true',
                        help='also score every panoptic result with Boundary PQ (PQ with IoU = min(mask IoU, boundary IoU)); needs a '
                        'panoptic head or --pan_combined; with --score_panoptic the prediction files are scored with both')
    parser.add_argument('--boundary_pq_dilation_ratio', type=float, default=None, metavar='R',
                        help='with --eval_boundary_pq: the boundary width as a fraction of the image diagonal (default 0.02)')
    parser.add_argument('--eval_instances', action='store_true',
                        help='Cityscapes only: also score the instance masks with the Cityscapes instance-level AP / AP50% '
                        '(the gtFine instanceIds maps are read)')
    parser.add_argument('--eval_pixels', action='store_true',
                        help='Cityscapes only: also score the semantic predictions with the Cityscapes pixel-level IoU / iIoU per class '
                        'and category (the gtFine labelIds and instanceIds maps are read)')
    parser.add_argument('--write_ssegs', action='store_true',
                        help='Cityscapes only: write the semantic predictions as PNGs to results/ssegs (palette PNGs of train ids, as the '
                        'reference does); also for image sets without ground truth')
    parser.add_argument('--ssegs_label_ids', action='store_true',
                        help='with --write_ssegs: grey 8-bit PNGs of label ids in results/ssegs_label_ids instead (the format the '
                        'benchmark server takes)')
    parser.add_argument('--score_ssegs', type=str, default='', metavar='FOLDER',
                        help='Cityscapes only: score a folder of semantic prediction PNGs (<base>.png; palette = train ids, grey = label '
                        'ids) with the pixel-level IoU / iIoU against the ground truth of --cfg; no model is built')
    parser.add_argument('--write_instances', action='store_true',
                        help='Cityscapes only: write the instance predictions in the benchmark format, results/inst_seg/<image>pred.txt '
                        'and one mask PNG per detection under results/inst_seg/seg_results (as the reference does); also for image sets '
                        'without ground truth')
    parser.add_argument('--instances_1bit', action='store_true',
                        help='with --write_instances: mask PNGs of bit depth 1 instead of 8-bit grey 0 / 255')
    parser.add_argument('--score_instances', type=str, default='', metavar='FOLDER',
                        help='Cityscapes only: score a folder of instance predictions in the benchmark format (one <image key>*.txt per '
                        'image naming its mask PNGs) with the instance-level AP against the ground truth of --cfg; no model is built')
    parser.add_argument('--write_panoptic', action='store_true',
                        help='write the panoptic predictions in COCO panoptic format: results/pans_unified/{pan_2ch,pan,pred.json,gt.json} '
                        '(and results/pans_combined/... with --pan_combined); also for image sets without ground truth')
    parser.add_argument('--panoptic_categories', type=str, default='',
                        help='with --write_panoptic on an image set without ground truth: a panoptic JSON whose categories (ids, isthing, '
                        'color) to use')
    parser.add_argument('--score_panoptic', type=str, default='', metavar='PRED_JSON',
                        help='score an existing COCO-panoptic prediction (pred.json and its PNG folder) against the panoptic ground '
                        'truth of --cfg; no model is built')
    parser.add_argument('--score_panoptic_folder', type=str, default='',
                        help='the PNG folder of --score_panoptic (default: the directory beside the JSON named like it without .json)')
    parser.add_argument('--vis_mask', action='store_true',
                        help='sets config.test.vis_mask: draw the detections of score >= 0.5 over every image into results/vis (one PNG '
                        'per image); in a run instead of the evaluation, with --eval_only before it, as the reference does')
    parser.add_argument('--vis_panoptic', choices=('flat', 'overlay', 'both'), default=None,
                        help='draw every panoptic result that is scored: flat = category colours with white contours around the thing '
                        'instances into results/pans_unified/vis_flat, overlay = segments, borders and category names over the '
                        'photograph into results/pans_unified/vis (results/pans_combined/... with --pan_combined); the evaluation '
                        'still runs; on an image set without ground truth the categories come from --panoptic_categories')
    parser.add_argument('--vis_panoptic_min_area', type=int, default=None, metavar='N',
                        help='with --vis_panoptic overlay / both: segments of fewer than N pixels get no label (default 1024)')
    parser.add_argument('--aug_scales', type=int, nargs='+', default=None, metavar='S',
                        help='sets config.test.aug_scales: test-time augmentation, further target sizes beside test.scales[0] (the '
                        'max size scales along); merged on the device')
    parser.add_argument('--aug_flip', action='store_true',
                        help='sets config.test.aug_flip: test-time augmentation, every scale also mirrored left to right')
    parser.add_argument('--bbox_vote', action='store_true',
                        help='sets config.test.bbox_vote: every kept detection box becomes the score-weighted mean of the candidates of '
                        'its class that overlap it (box voting, on the device); the run is the eager one of the test-time augmentation')
    parser.add_argument('--bbox_vote_thresh', type=float, default=None, metavar='T',
                        help='with --bbox_vote: sets config.test.bbox_vote_thresh, the IoU from which a candidate votes (default 0.8)')
    parser.add_argument('--soft_nms', action='store_true',
                        help='sets config.test.soft_nms: the class-wise detection selection keeps overlapping candidates with a decayed '
                        'score instead of dropping them (soft-NMS, on the device); the run is the eager one of the test-time augmentation')
    parser.add_argument('--soft_nms_method', choices=('linear', 'gaussian'), default=None, metavar='M',
                        help='with --soft_nms: sets config.test.soft_nms_method, linear (default) or gaussian')
    parser.add_argument('--soft_nms_sigma', type=float, default=None, metavar='S',
                        help='with --soft_nms: sets config.test.soft_nms_sigma, the width of the gaussian decay (default 0.5)')
    add_pan_component_arguments(parser, 'scored, written or drawn')
    parser.add_argument('--pan_confidence', action='store_true',
                        help='sets config.test.pan_confidence: the panoptic head also returns its confidence, one byte per pixel (255 x '
                        'the softmax over the panoptic logits at the winning label); --write_panoptic then writes a "score" per segment '
                        'of the unified result, its mean confidence')
    parser.add_argument('--pan_min_score', type=float, default=None, metavar='T',
                        help='sets config.test.pan_min_score (implies --pan_confidence): every segment of the unified panoptic result whose '
                        'mean confidence is below T (0..1) becomes VOID before the maps are cleaned, scored, written or drawn; 0 = off')
    parser.add_argument('--write_pan_confidence', action='store_true',
                        help='with --write_panoptic and --pan_confidence (or --pan_min_score): also write the confidence planes as 8-bit '
                        'grey PNGs to results/pans_unified/conf')
    args, rest = parser.parse_known_args(argv)
    if args.cfg:
        update_config(args.cfg)
    if args.vis_mask:
        config.test.vis_mask = True
    if args.aug_scales is not None:
        config.test.aug_scales = list(args.aug_scales)
    if args.aug_flip:
        config.test.aug_flip = True
    if args.bbox_vote:
        config.test.bbox_vote = True
    if args.bbox_vote_thresh is not None:
        if not config.test.get('bbox_vote', False):
            parser.error('--bbox_vote_thresh sets the IoU threshold of --bbox_vote, which is missing')
        config.test.bbox_vote_thresh = float(args.bbox_vote_thresh)
    if args.soft_nms:
        config.test.soft_nms = True
    for name in ('soft_nms_method', 'soft_nms_sigma'):
        if getattr(args, name) is not None:
            if not config.test.get('soft_nms', False):
                parser.error('--%s is a parameter of --soft_nms, which is missing' % name)
            config.test[name] = getattr(args, name)
    apply_pan_component_arguments(args, parser.error)
    if args.pan_confidence:
        config.test.pan_confidence = True
    if args.pan_min_score is not None:
        config.test.pan_min_score = float(args.pan_min_score)
    t = config.test.get('pan_min_score', 0.0)
    if isinstance(t, bool) or not isinstance(t, (int, float)) or not (0.0 <= t <= 1.0):
        parser.error('--pan_min_score (test.pan_min_score) must be a number in 0..1, got %r' % (t,))
    if not isinstance(config.test.get('pan_confidence', False), bool):
        parser.error('test.pan_confidence must be true or false, got %r' % (config.test.pan_confidence,))
    if rest:    # (the reference re-parses strictly, parse_args.py:32; an option neither parser knows is reported, not swallowed)
        parser.error('unrecognized arguments: %s' % ' '.join(rest))
    return args
