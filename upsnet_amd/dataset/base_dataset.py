"""Post-processing and evaluation of the network outputs -- host mirror of the reference's BaseDataset methods after the inference
path: get_unified_pan_result (upsnet/dataset/base_dataset.py:332-371, csrc/postprocess.hip), get_combined_pan_result (:373-449,
csrc/pan_combine.hip), evaluate_panoptic (:209-330, PQ through
dataset/pq.py and csrc/pq_eval.hip) with its PQStat / PQStatCat host classes (:44-96), and get_confusion_matrix (:806-824) plus the
mIoU of evaluate_ssegs (cityscapes.py:445-492), all counting on the device."""
import json
import logging
import os
from collections import defaultdict

import numpy as np
import torch

from .. import ops
from ..config.config import config

logger = logging.getLogger(__name__)


class PQStatCat(object):
    """Per-category PQ counts: matched IoU sum, true positives, false positives, false negatives."""

    def __init__(self):
        self.iou = 0.0
        self.tp = 0
        self.fp = 0
        self.fn = 0

    def __iadd__(self, other):
        self.iou += other.iou
        self.tp += other.tp
        self.fp += other.fp
        self.fn += other.fn
        return self


class PQStat(object):
    """PQStatCat per category id (created on first access); `+=` merges per category."""

    def __init__(self):
        self.pq_per_cat = defaultdict(PQStatCat)

    def __getitem__(self, i):
        return self.pq_per_cat[i]

    def __iadd__(self, other):
        for label, stat in other.pq_per_cat.items():
            self.pq_per_cat[label] += stat
        return self

    def pq_average(self, categories, isthing):
        """Mean PQ / SQ / RQ over the categories (isthing None: all; True / False: things / stuff) that have any tp, fp or fn, and
        the per-category results; the reference's float arithmetic and summation order (categories in the table's order)."""
        pq, sq, rq, n = 0, 0, 0, 0
        per_class = {}
        for label, info in categories.items():
            if isthing is not None and isthing != (info['isthing'] == 1):
                continue
            s = self.pq_per_cat[label]
            iou, tp, fp, fn = s.iou, s.tp, s.fp, s.fn
            if tp + fp + fn == 0:
                per_class[label] = {'pq': 0.0, 'sq': 0.0, 'rq': 0.0}
                continue
            n += 1
            denom = tp + 0.5 * fp + 0.5 * fn
            pq_c = iou / denom
            sq_c = iou / tp if tp != 0 else 0
            rq_c = tp / denom
            per_class[label] = {'pq': pq_c, 'sq': sq_c, 'rq': rq_c, 'iou': iou, 'tp': tp, 'fp': fp, 'fn': fn}
            pq += pq_c
            sq += sq_c
            rq += rq_c
        return {'pq': pq / n, 'sq': sq / n, 'rq': rq / n, 'n': n}, per_class


def _as_device_u8(a, dev):
    """uint8 device tensor of integer labels 0..255 (the reference passes float32 GT / uint8 pred arrays); ValueError otherwise."""
    t = torch.as_tensor(a)
    if t.dtype != torch.uint8:
        t = t.to(dev)
        if t.numel() and (bool((t != t.round()).any()) or int(t.min()) < 0 or int(t.max()) > 255):
            raise ValueError("labels must be integers in 0..255")
        t = t.to(torch.uint8)
    return t.to(dev).contiguous()


def load_panoptic_png(path):
    """GT panoptic PNG -> uint8 [H,W,3] RGB (id = R + 256 G + 65536 B). Raises where the reference's loader skips an unreadable
    file silently (base_dataset.py:455-464), which would misalign every later image with its annotation."""
    from PIL import Image
    im = np.array(Image.open(path))
    if im.dtype != np.uint8 or im.ndim != 3 or im.shape[2] < 3:
        raise ValueError("%s: not an RGB panoptic PNG (%s %s)" % (path, im.shape, im.dtype))
    return np.ascontiguousarray(im[:, :, :3])


class BaseDataset(object):
    """Only the result-shaping and scoring methods of the reference class that follow the inference path."""

    def get_unified_pan_result(self, segs, pans, cls_inds, stuff_area_limit=4 * 64 * 64):
        """segs / pans: per-image int64 label maps ([H,W] or [1,H,W], device tensors; numpy arrays are uploaded);
        cls_inds: per-image 1-based thing classes of the panoptic instances. Returns a list of uint8 [H,W,3] device tensors
        (channel 0 category, channel 1 instance id), like the reference's list of numpy arrays."""
        id_last_stuff = config.dataset.num_seg_classes - config.dataset.num_classes
        out = []
        for seg, pan, cls_ind in zip(segs, pans, cls_inds):
            dev = pan.device if isinstance(pan, torch.Tensor) and pan.is_cuda else torch.device('cuda', torch.cuda.current_device())
            seg, pan, cls_ind = (torch.as_tensor(t).to(dev) for t in (seg, pan, cls_ind))
            out.append(ops.unified_pan_result(pan, seg, cls_ind, id_last_stuff, config.dataset.num_seg_classes, stuff_area_limit))
        return out

    def get_combined_pan_result(self, segs, boxes, masks, score_threshold=0.6, fraction_threshold=0.7, stuff_area_limit=4 * 64 * 64):
        """The heuristic panoptic merge (reference :373-449) on the device, all images in one call (ops.combined_pan_result,
        csrc/pan_combine.hip). segs: per-image semantic maps [H,W] (numpy or tensor, uint8 or int64 in 0..255); boxes[c][i]: [n,5]
        arrays and masks[c][i]: lists of RLE dicts for c = 1..num_classes-1. Returns a list of uint8 [H,W,3] device tensors
        (channel 0 category, channel 1 instance id), like get_unified_pan_result. Pinned where the reference is ambiguous:
          - merge order: classes 1..C-1 concatenated, np.argsort(score, kind='stable')[::-1] (ties: the later candidate first);
          - a candidate is skipped iff float(score) < score_threshold (double: numpy 1.x promotion);
          - zero-area masks are skipped and use no instance number; otherwise a mask is rejected iff the float32 quotient
            remain / area is < fraction_threshold compared in double (numpy 1.x; numpy 2 compares in float32 and accepts
            remain / area == fl32(fraction_threshold), e.g. 7 / 10 against 0.7);
          - instances are numbered per class from 1 in acceptance order.
        ValueError before any launch: more than 255 candidates of one class at or above the score threshold, an image of more
        than 2^24 pixels, a mask size or RLE counts sum that does not match its semantic map, boxes / masks of different lengths.
        Images may differ in size; the inputs are never modified."""
        id_last_stuff = config.dataset.num_seg_classes - config.dataset.num_classes
        return ops.combined_pan_result(segs, boxes, masks, id_last_stuff, score_threshold=score_threshold,
                                       fraction_threshold=fraction_threshold, stuff_area_limit=stuff_area_limit)

    def clean_pan_result(self, pans, min_area=None, connectivity=None, keep_largest=None, what='panoptic', mode=None):
        """get_unified_pan_result's / get_combined_pan_result's maps with the disconnected fragments of fewer than min_area pixels
        turned into VOID (dataset/pan_components.clean_panoptic) or, with mode 'absorb', into the segment they border most
        (DESIGN 4.27); the parameters default to config.test.pan_min_component, pan_component_connectivity,
        pan_component_keep_largest and pan_component_mode. Logs the components and pixels removed (and absorbed) over all maps, once.
        RuntimeError if the absorb mode's vote table overflowed on any map (it is sized so that it cannot)."""
        from .pan_components import clean_panoptic
        min_area = config.test.pan_min_component if min_area is None else min_area
        connectivity = config.test.pan_component_connectivity if connectivity is None else connectivity
        keep_largest = config.test.pan_component_keep_largest if keep_largest is None else keep_largest
        mode = config.test.get('pan_component_mode', 'void') if mode is None else mode
        cleaned, total = clean_panoptic(pans, min_area, connectivity, keep_largest, return_stats=True, mode=mode)
        if total is not None:
            total = total.cpu().tolist()
            _, comps, gone, pixels = total[:4]
            kept = ', the largest of every segment kept' if keep_largest else ''
            if mode == 'void':
                logger.info('%s: %d of %d connected components (%d pixels) of fewer than %d pixels removed from %d maps (%d-connectivity%s)',
                            what, gone, comps, pixels, min_area, len(cleaned), connectivity, kept)
            else:
                absorbed, absorbed_pixels, _, overflow = total[4:]
                if overflow:
                    raise RuntimeError("%s: the vote table of pan_absorb overflowed on %d of %d maps: those maps were not cleaned"
                                       % (what, overflow, len(cleaned)))
                logger.info('%s: %d of %d connected components (%d pixels) of fewer than %d pixels removed from %d maps (%d-connectivity%s), '
                            '%d of them (%d pixels) absorbed into the segment they border most', what, gone, comps, pixels, min_area,
                            len(cleaned), connectivity, kept, absorbed, absorbed_pixels)
        return cleaned

    def score_pan_segments(self, pans, confs):
        """One dictionary per map, {(category, instance): (area, sum_q, score)}: the mean panoptic confidence of every segment of
        get_unified_pan_result's maps (dataset/pan_confidence.segment_scores); confs: the confidence planes of the same
        images at the maps' size (results['all_pano_confs'])."""
        from .pan_confidence import segment_scores
        pans, confs = list(pans), list(confs)
        if len(pans) != len(confs):
            raise ValueError("%d maps and %d confidence planes" % (len(pans), len(confs)))
        return [segment_scores(p, c) for p, c in zip(pans, confs)]

    def filter_pan_result(self, pans, confs, min_score=None, what='unified pano result'):
        """get_unified_pan_result's maps with every segment whose mean confidence is below min_score (default:
        config.test.pan_min_score) turned into VOID (dataset/pan_confidence.filter_by_score). Logs the segments removed
        over all maps, once."""
        from .pan_confidence import filter_by_score
        min_score = config.test.pan_min_score if min_score is None else min_score
        kept, (before, after) = filter_by_score(pans, confs, min_score, return_stats=True)
        logger.info('%s: %d of %d segments of mean confidence below %g removed from %d maps', what, before - after, before, min_score, len(kept))
        return kept

    def load_panoptic_gt(self):
        """(images, annotations, categories) of self.panoptic_json_file; images yields the uint8 [H,W,3] GT PNGs of
        self.panoptic_gt_folder in the JSON's 'images' order (as the reference loads them), lazily."""
        with open(self.panoptic_json_file, 'r') as f:
            gt_json = json.load(f)
        categories = {el['id']: el for el in gt_json['categories']}
        images = (load_panoptic_png(os.path.join(self.panoptic_gt_folder, item['file_name'])) for item in gt_json['images'])
        return images, gt_json['annotations'], categories

    def evaluate_panoptic(self, pred_pans_2ch, output_dir, max_gt_segments=4096):
        """PQ / SQ / RQ of the 2-channel predictions (get_unified_pan_result's list, at GT resolution) against the panoptic GT,
        computed on the device (dataset/pq.py: semantics, summation order and deviations). Returns the reference's dict
        {'All', 'Things', 'Stuff', 'per_class'} and logs its tables. Scoring writes nothing to output_dir (the reference's pred PNG /
        JSON dumps only recolour the segments; PQ does not depend on them): write_panoptic(pred_pans_2ch, output_dir) writes them."""
        from .pq import PanopticEvaluator
        images, annotations, categories = self.load_panoptic_gt()
        if len(pred_pans_2ch) != len(annotations):
            raise ValueError("%d predictions for %d GT annotations" % (len(pred_pans_2ch), len(annotations)))
        ev = PanopticEvaluator(categories, max_gt_segments=max_gt_segments)
        for pred, gt, ann in zip(pred_pans_2ch, images, annotations):
            ev.add(pred, gt, ann['segments_info'])
        return ev.summary()

    def evaluate_panoptic_boundary(self, pred_pans_2ch, output_dir, dilation_ratio=0.02, max_gt_segments=4096):
        """evaluate_panoptic with Boundary PQ (PanopticEvaluator(boundary=True): every pair scored by min(mask IoU, boundary IoU),
        boundaries of width dilation_ratio x the image diagonal). Same dict shape; writes nothing to output_dir."""
        from .pq import PanopticEvaluator
        images, annotations, categories = self.load_panoptic_gt()
        if len(pred_pans_2ch) != len(annotations):
            raise ValueError("%d predictions for %d GT annotations" % (len(pred_pans_2ch), len(annotations)))
        ev = PanopticEvaluator(categories, max_gt_segments=max_gt_segments, boundary=True, dilation_ratio=dilation_ratio)
        for pred, gt, ann in zip(pred_pans_2ch, images, annotations):
            ev.add(pred, gt, ann['segments_info'])
        return ev.summary()

    def write_panoptic(self, pred_pans_2ch, output_dir, categories=None, categories_json=None, confs=None, write_conf=False):
        """The files of the reference's evaluate_panoptic (:321-327): output_dir/pan_2ch/*.png, pan/*.png, pred.json and -- with ground
        truth -- gt.json (dataset/pan_format.write_panoptic: colours, naming, deviations). With ground truth the predictions are
        those of evaluate_panoptic (one per annotation of self.panoptic_json_file, in its order); names come from the JSON's
        'images', image ids from its annotations, categories from its 'categories'. A set without ground truth (has_gt false) takes
        names and ids from the image list, and its categories from `categories` (a table as PanopticEvaluator takes it) or from the
        'categories' of the panoptic JSON `categories_json`; ValueError if neither is given. Returns the annotations written.
        confs (the confidence planes of the same images): every segments_info entry gains "score", the mean confidence of
        the segment on the map as written; write_conf: the planes also go to output_dir/conf/*.png as 8-bit grey. Without confs the
        files are what they always were."""
        from .pan_format import write_panoptic
        if getattr(self, 'has_gt', True):
            with open(self.panoptic_json_file, 'r') as f:
                gt_json = json.load(f)
            images, annotations = gt_json['images'], gt_json['annotations']
            if len(images) != len(annotations):
                raise ValueError("%s lists %d images and %d annotations" % (self.panoptic_json_file, len(images), len(annotations)))
            if categories is None and categories_json is None:
                categories = gt_json['categories']
            image_ids = [a['image_id'] for a in annotations]
        else:
            gt_json = None
            images = [{'id': e['id'], 'file_name': e['file_name']} for e in self.roidb]
            image_ids = None
        if categories is None:
            if categories_json is None:
                raise ValueError("%s has no ground truth and so no category table: pass categories= or the path of a panoptic JSON "
                                 "whose 'categories' to use (categories_json=)" % getattr(self, 'name', type(self).__name__))
            with open(categories_json, 'r') as f:
                categories = json.load(f)['categories']
        os.makedirs(output_dir, exist_ok=True)
        annotations = write_panoptic(pred_pans_2ch, images, categories, output_dir, image_ids=image_ids, confs=confs, write_conf=write_conf)
        if gt_json is not None:
            with open(os.path.join(output_dir, 'gt.json'), 'w') as f:
                json.dump(gt_json, f)
        logger.info('%d panoptic predictions written to %s', len(annotations), os.path.abspath(output_dir))
        return annotations

    def vis_panoptic(self, pred_pans_2ch, output_dir, mode='overlay', categories=None, categories_json=None, label_min_area=1024):
        """The predictions write_panoptic would write, as pictures (dataset/pan_vis.vis_panoptic): mode 'flat' -- the
        reference's vis_panoptic picture, category colours with white contours around the thing instances -- to output_dir/vis_flat,
        mode 'overlay' -- the photograph with the segments, their borders and their names -- to output_dir/vis; file names as
        write_panoptic's. Predictions, names and categories are resolved exactly as write_panoptic resolves them (with ground truth:
        one prediction per annotation of self.panoptic_json_file, in its order; without: the image list's order and categories= or
        categories_json=). Returns the written paths."""
        from .pan_vis import vis_panoptic
        if getattr(self, 'has_gt', True):
            with open(self.panoptic_json_file, 'r') as f:
                gt_json = json.load(f)
            images = gt_json['images']
            if len(images) != len(gt_json['annotations']):
                raise ValueError("%s lists %d images and %d annotations" % (self.panoptic_json_file, len(images), len(gt_json['annotations'])))
            if categories is None and categories_json is None:
                categories = gt_json['categories']
            order = self.panoptic_order() if mode == 'overlay' else None
        else:
            images = [{'id': e['id'], 'file_name': e['file_name']} for e in self.roidb]
            order = list(range(len(self.roidb)))
        if categories is None:
            if categories_json is None:
                raise ValueError("%s has no ground truth and so no category table: pass categories= or the path of a panoptic JSON "
                                 "whose 'categories' to use (categories_json=)" % getattr(self, 'name', type(self).__name__))
            with open(categories_json, 'r') as f:
                categories = json.load(f)['categories']
        image_paths = [self.roidb[k]['image'] for k in order] if mode == 'overlay' else None
        os.makedirs(output_dir, exist_ok=True)
        return vis_panoptic(pred_pans_2ch, images, categories, output_dir, mode, image_paths=image_paths, label_min_area=label_min_area)

    def evaluate_panoptic_files(self, pred_json, pred_folder, max_gt_segments=4096, boundary=False, dilation_ratio=0.02):
        """PQ / SQ / RQ of a prediction in COCO panoptic format (pred_json with its PNG folder: write_panoptic's output, or any other
        tool's) against the panoptic GT, through PanopticEvaluator.add_png. Annotations are paired with the GT by image_id;
        ValueError if an image of the GT has no prediction, or a prediction no GT image, or an image id occurs twice.
        boundary=True scores Boundary PQ at dilation_ratio instead (evaluate_panoptic_boundary)."""
        from .pq import PanopticEvaluator
        with open(pred_json, 'r') as f:
            pred_anns = json.load(f)['annotations']
        images, annotations, categories = self.load_panoptic_gt()
        preds = {}
        for a in pred_anns:
            if a['image_id'] in preds:
                raise ValueError("%s: image_id %s occurs twice" % (pred_json, a['image_id']))
            preds[a['image_id']] = a
        gt_ids = [a['image_id'] for a in annotations]
        missing = [i for i in gt_ids if i not in preds]
        surplus = sorted(set(preds) - set(gt_ids), key=str)
        if missing or surplus:
            raise ValueError("%s does not cover the ground truth: %d GT images without a prediction (first: %s), %d predictions without "
                             "a GT image (first: %s)" % (pred_json, len(missing), missing[:3], len(surplus), surplus[:3]))
        if boundary:
            ev = PanopticEvaluator(categories, max_gt_segments=max_gt_segments, boundary=True, dilation_ratio=dilation_ratio)
        else:
            ev = PanopticEvaluator(categories, max_gt_segments=max_gt_segments)
        for gt, ann in zip(images, annotations):
            pred = preds[ann['image_id']]
            ev.add_png(load_panoptic_png(os.path.join(pred_folder, pred['file_name'])), pred['segments_info'], gt, ann['segments_info'])
        return ev.summary()

    # ---------------------------------------------------------------------------------------------- COCO box / mask AP
    def load_instances_gt(self):
        """(image_ids ascending, {image_id: (height, width)}, {image_id: [annotations in JSON order]}, category ids in JSON order) of
        the COCO instances JSON self.instances_json_file. Class c >= 1 of all_boxes / all_segms is the c-th category of the JSON's
        'categories' list, as the reference's classes follow COCO.getCatIds()."""
        with open(self.instances_json_file, 'r') as f:
            gt_json = json.load(f)
        image_ids = sorted(int(im['id']) for im in gt_json['images'])
        sizes = {int(im['id']): (int(im['height']), int(im['width'])) for im in gt_json['images']}
        anns = defaultdict(list)
        for a in gt_json['annotations']:
            anns[int(a['image_id'])].append(a)
        return image_ids, sizes, anns, [int(c['id']) for c in gt_json['categories']]

    def _evaluate_detections(self, all_boxes, all_segms, output_dir, iou_type, dilation_ratio=0.02):
        """The reference's evaluate_boxes / evaluate_masks: results JSON written as the reference writes it, COCOeval on the device
        (dataset/coco_eval.py), the metrics logged and the summary lines written to detection_results.txt. iou_type 'boundary'
        (evaluate_boundary): no results JSON (evaluate_masks writes the segmentations), the summary goes to boundary_results.txt."""
        from .coco_eval import DetectionEvaluator, EvalResult, detection_metrics_lines
        from ..bbox.bbox_transform import xyxy_to_xywh
        image_ids, sizes, anns, cat_ids = self.load_instances_gt()
        name = getattr(self, 'name', 'instances')
        results = []
        n_cls = min(len(all_boxes), len(cat_ids) + 1)
        for c in range(1, n_cls):
            if len(all_boxes[c]) != len(image_ids) or (all_segms is not None and len(all_segms[c]) != len(image_ids)):
                raise ValueError("class %d: results for %d images, the GT has %d" % (c, len(all_boxes[c]), len(image_ids)))
            for i, image_id in enumerate(image_ids):
                dets = all_boxes[c][i]
                if isinstance(dets, list) and len(dets) == 0:
                    continue
                dets = np.asarray(dets).astype(np.float64)
                xywh = xyxy_to_xywh(dets[:, 0:4])
                for k in range(dets.shape[0]):
                    r = {'image_id': image_id, 'category_id': cat_ids[c - 1], 'score': float(dets[k, -1])}
                    if all_segms is None:
                        r['bbox'] = [float(v) for v in xywh[k]]
                    else:
                        r['segmentation'] = all_segms[c][i][k]
                    results.append(r)
        if iou_type != 'boundary':
            res_file = os.path.join(output_dir, ('bbox_' if all_segms is None else 'segmentations_') + name + '_results.json')
            logger.info('Writing %s results json to: %s', iou_type, os.path.abspath(res_file))
            with open(res_file, 'w') as fid:
                json.dump(results, fid)
        ev = DetectionEvaluator(cat_ids, iou_type, dilation_ratio=dilation_ratio)
        for i, image_id in enumerate(image_ids):
            dets = [[]] + [all_boxes[c][i] for c in range(1, n_cls)]
            rles = None if all_segms is None else [[]] + [all_segms[c][i] for c in range(1, n_cls)]
            gt = anns.get(image_id, [])
            if all_segms is not None:
                gt = self._rasterize_polygon_gt(gt, sizes[image_id])
            ev.add_rle(image_id, gt, dets, rles, image_size=sizes[image_id])
        res = ev.accumulate()
        for line in detection_metrics_lines(res)[:-12]:
            logger.info(line)
        with open(os.path.join(output_dir, 'boundary_results.txt' if iou_type == 'boundary' else 'detection_results.txt'), 'w') as f:
            for line in res['summary_lines']:
                print(line)
                f.write(line + '\n')
        return EvalResult(res)

    @staticmethod
    def _rasterize_polygon_gt(gt, size):
        """The image's annotations with every polygon segmentation (a list: all non-crowd objects of the COCO and Cityscapes instance
        files) replaced by a view of one rasterize_polygons call (dataset/polygon.py: on the device, nothing synchronised); RLE
        segmentations (crowds) pass as they are. The annotations themselves are not modified."""
        from .polygon import rasterize_polygons
        poly = [k for k, a in enumerate(gt) if isinstance(a.get('segmentation'), (list, tuple))]
        if not poly:
            return gt
        rasters = rasterize_polygons([gt[k]['segmentation'] for k in poly], size[0], size[1])
        gt = list(gt)
        for j, k in enumerate(poly):
            gt[k] = dict(gt[k], segmentation=rasters[j])
        return gt

    def evaluate_boxes(self, all_boxes, output_dir):
        """COCO box AP of all_boxes[class][image] ([n,5] x1 y1 x2 y2 score, images in ascending id) against
        self.instances_json_file; returns the 12 summary stats. Writes bbox_<name>_results.json and detection_results.txt."""
        return self._evaluate_detections(all_boxes, None, output_dir, 'bbox').stats

    def evaluate_masks(self, all_boxes, all_segms, output_dir):
        """COCO mask AP of all_segms[class][image] (im_post's RLE dicts) scored by all_boxes; returns an object with .stats and
        .eval (precision / recall / scores). Writes segmentations_<name>_results.json and detection_results.txt. Polygon GT
        segmentations are rasterised on the device, one call per image (dataset/polygon.py)."""
        return self._evaluate_detections(all_boxes, all_segms, output_dir, 'segm')

    def evaluate_boundary(self, all_boxes, all_segms, output_dir, dilation_ratio=0.02):
        """Boundary AP (the Boundary IoU API's COCOeval, iouType 'boundary') of the same inputs as evaluate_masks: IoU = min(mask IoU,
        boundary IoU), boundaries eroded by dilation_ratio x the image diagonal on the device (dataset/boundary.py). Returns an
        object with .stats and .eval; writes boundary_results.txt only (detection_results.txt and the results JSONs stay as
        evaluate_masks left them)."""
        return self._evaluate_detections(all_boxes, all_segms, output_dir, 'boundary', dilation_ratio)

    # ---------------------------------------------------------------------------------------------- RPN proposal recall (AR)
    def evaluate_box_proposals(self, roidb, thresholds=None, area='all', limit=None):
        """The reference's evaluate_box_proposals (upsnet/dataset/base_dataset.py:723-805): roidb = dicts with 'boxes' (GT rows and
        proposal rows), 'gt_classes' (0 = proposal), 'is_crowd' and 'seg_areas'. Returns {'ar', 'recalls', 'thresholds',
        'gt_overlaps', 'num_pos'}, bit-identical to the reference; the greedy matching runs on the device
        (dataset/proposal_eval.py, csrc/prop_eval.hip)."""
        from .proposal_eval import ProposalRecallEvaluator
        ev = ProposalRecallEvaluator(areas=(area,), limits=(limit,))
        for entry in roidb:
            ev.add_entry(entry)
        return ev.summary(thresholds)[(area, ev.limits[0])]

    def load_proposal_gt(self):
        """(image_ids ascending, {image_id: dict(boxes float32 [G,4], gt_classes int32 [G], is_crowd bool [G], seg_areas float32 [G])})
        built from the instances JSON by the rules of the reference's JsonDataset._add_gt_annotations (json_dataset.py:164-230):
        area < config.train.gt_min_area and ignore == 1 dropped; x2 = x1 + max(0, w - 1) clipped to the image; a box is kept iff
        area > 0, x2 > x1 and y2 > y1. Classes are 1-based in the order of the JSON's categories."""
        from .proposal_eval import gt_entry
        with open(self.instances_json_file, 'r') as f:
            gt_json = json.load(f)
        image_ids = sorted(int(im['id']) for im in gt_json['images'])
        sizes = {int(im['id']): (int(im['height']), int(im['width'])) for im in gt_json['images']}
        cls_of = {int(c['id']): i + 1 for i, c in enumerate(gt_json['categories'])}
        anns = defaultdict(list)
        for a in gt_json['annotations']:
            anns[int(a['image_id'])].append(a)
        min_area = config.train.get('gt_min_area', -1)
        return image_ids, {i: gt_entry(anns.get(i, []), sizes[i], cls_of, min_area) for i in image_ids}

    def evaluate_proposals(self, all_proposals, output_dir):
        """Proposal recall of all_proposals (per image in ascending image id, float32 [n, 4] x1 y1 x2 y2 in rank order, original image
        scale) against self.instances_json_file: limits (100, 300, 1000) x areas (all, small, medium, large) in one device pass.
        Returns {'AR@100', 'ARs@100', 'ARm@100', 'ARl@100', ..., 'ARl@1000'}, logged and written to proposal_recall.txt."""
        from .proposal_eval import AR_AREAS, AR_LIMITS, ProposalRecallEvaluator, ar_metrics
        image_ids, gts = self.load_proposal_gt()
        if len(all_proposals) != len(image_ids):
            raise ValueError("proposals for %d images, the GT has %d" % (len(all_proposals), len(image_ids)))
        ev = ProposalRecallEvaluator(areas=[a for a, _ in AR_AREAS], limits=AR_LIMITS)
        for i, image_id in enumerate(image_ids):
            g = gts[image_id]
            ev.add(all_proposals[i], g['boxes'], g['gt_classes'], g['is_crowd'], g['seg_areas'])
        metrics = ar_metrics(ev.summary())
        lines = ['%s: %.4f' % (k, v) for k, v in metrics.items()]
        for line in lines:
            logger.info(line)
        os.makedirs(output_dir, exist_ok=True)
        with open(os.path.join(output_dir, 'proposal_recall.txt'), 'w') as f:
            for line in lines:
                f.write(line + '\n')
        return metrics

    # ---------------------------------------------------------------------------------------------- detection visualisations
    def vis_all_mask(self, all_boxes, all_masks, save_path=None):
        """The reference's vis_all_mask (:826-896): every image of the list with its detections of score >= 0.5 drawn over it (box
        outline, name.score label, half-transparent mask with a white contour), one PNG per image named <image basename>.png (so
        x.jpg.png) under save_path; save_path None returns the rendered uint8 [H, W, 3] arrays instead. Drawn on the device by the
        integer rule of dataset/vis.py. The k-th kept detection of the run has the colour vis.coco_colour(k), this
        project's own sequence (the reference cycles Detectron's list). Returns the written paths."""
        from . import vis
        return vis.vis_all_mask(self, all_boxes, all_masks, self.dataset.classes, lambda j, k: vis.coco_colour(k),
                                lambda entry: '{}.png'.format(entry['image'].split('/')[-1]), save_path)

    def evaluate_all(self, all_boxes, all_segms, output_dir):
        all_results = self.evaluate_boxes(all_boxes, output_dir)
        self.evaluate_masks(all_boxes, all_segms, output_dir)
        return all_results

    def get_confusion_matrix(self, gt_label, pred_label, class_num):
        """Confusion matrix [class_num, class_num] float64 (numpy) of two label arrays of one shape, counted on the device: cell
        (gt, pred) for index gt * class_num + pred < class_num^2; a pred value >= class_num aliases into another cell, as the
        reference's np.bincount does. Labels must be integers in 0..255."""
        dev = torch.device('cuda', torch.cuda.current_device())
        cm = torch.zeros((class_num, class_num), dtype=torch.int64, device=dev)
        ops.confusion_accumulate(_as_device_u8(gt_label, dev), _as_device_u8(pred_label, dev), class_num, -1, cm)
        return cm.cpu().numpy().astype(np.float64)

    def evaluate_ssegs_arrays(self, gts, preds, num_seg_classes):
        """evaluate_ssegs (cityscapes.py:445-492) over in-memory label maps instead of PNG files: pixels with gt == 255 dropped,
        confusion matrices summed on the device, then the reference's IoU formula. Returns {'meanIU', 'IU_array', 'confusion_matrix'}."""
        dev = torch.device('cuda', torch.cuda.current_device())
        cm = torch.zeros((num_seg_classes, num_seg_classes), dtype=torch.int64, device=dev)
        for gt, pred in zip(gts, preds):
            ops.confusion_accumulate(_as_device_u8(gt, dev), _as_device_u8(pred, dev), num_seg_classes, 255, cm)
        confusion_matrix = cm.cpu().numpy().astype(np.float64)
        pos = confusion_matrix.sum(1)
        res = confusion_matrix.sum(0)
        tp = np.diag(confusion_matrix)
        IU_array = tp / np.maximum(1.0, pos + res - tp)
        return {'meanIU': IU_array.mean(), 'IU_array': IU_array, 'confusion_matrix': confusion_matrix}
