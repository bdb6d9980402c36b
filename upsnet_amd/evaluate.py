"""Run and score a checkpoint over a Cityscapes or COCO evaluation set: the reference's test command over a real image list
(upsnet/upsnet_end2end_test.py:155-314).

    python -m upsnet_amd.evaluate --cfg <yaml> (--weight_path <pth> | --synthetic_weights) [--eval_only] [--in-flight N] [--pan_combined]
                                  [--eval_proposals] [--eval_instances] [--write_panoptic [--panoptic_categories <json>]]
                                  [--eval_pixels] [--write_ssegs [--ssegs_label_ids]] [--vis_mask]
                                  [--vis_panoptic {flat,overlay,both} [--vis_panoptic_min_area N]]
                                  [--write_instances [--instances_1bit]] [--eval_boundary [--boundary_dilation_ratio R]]
                                  [--eval_boundary_pq [--boundary_pq_dilation_ratio R]] [--aug_scales S [S ...]] [--aug_flip]
                                  [--bbox_vote [--bbox_vote_thresh T]] [--soft_nms [--soft_nms_method M] [--soft_nms_sigma S]]
                                  [--pan_min_component N [--pan_component_connectivity {4,8}]]
                                  [--pan_confidence] [--pan_min_score T] [--write_pan_confidence]
    python -m upsnet_amd.evaluate --cfg <yaml> --score_panoptic <pred.json> [--score_panoptic_folder <dir>] [--eval_boundary_pq ...]
    python -m upsnet_amd.evaluate --cfg <yaml> --score_ssegs <folder>
    python -m upsnet_amd.evaluate --cfg <yaml> --score_instances <folder>

The dataset is `config.dataset.dataset` (Cityscapes or coco) on `config.dataset.test_image_set`. Every image and every GT file the
configured heads need is checked before the first launch. Images are decoded by a bounded host thread pool ahead of the device;
the network runs through forward_async with up to N images in flight (its own graph policy: one fixed input shape replays HIP
graphs, a new shape / im_info runs eagerly). Per image, as the reference's im_detect / im_post / loop (:55-152, 222-274): boxes
scaled by 1 / im_scale in float32, masks run-length encoded by dataset/rle.im_post, the semantic and panoptic maps restored to the
original resolution by one gather launch (csrc/restore.hip, cv2 INTER_NEAREST tables). The results pickle has the reference's
path, keys and nesting (numpy objects only); evaluation follows the reference's order: boxes, masks, panoptic, semantic.
`--eval_only` re-scores the pickle without building the model. `--pan_combined` also scores get_combined_pan_result (the
heuristic merge of the detections and the semantic map) next to the unified result. `--eval_proposals` keeps the RPN proposals
of every image (results['all_proposals'], original image scale) and scores their recall (metrics['proposal_ar']).
`--eval_boundary` (a mask head) also scores the instance masks with Boundary AP (metrics['boundary_ap'], 12 stats; boundaries of width
`--boundary_dilation_ratio` x the image diagonal, default 0.02; dataset/boundary.py), written to results/boundary_results.txt.
`--eval_boundary_pq` (a panoptic head, or --pan_combined) also scores every panoptic result with Boundary PQ (metrics['panoptic_boundary']
after metrics['panoptic'], metrics['panoptic_combined_boundary'] with --pan_combined; PQ with every pair scored by min(mask IoU,
boundary IoU), boundaries of width `--boundary_pq_dilation_ratio` x the image diagonal, default 0.02; dataset/pq.py); with
`--score_panoptic` the prediction files are scored with both.
`--eval_instances` (Cityscapes with a mask head) also scores the instance masks with the Cityscapes instance-level AP against the
gtFine instanceIds maps (metrics['instance_ap'], dataset/cityscapes_eval.py). `--write_panoptic` writes the panoptic predictions in
COCO panoptic format under the reference's paths, results/pans_unified/{pan_2ch,pan,pred.json,gt.json} (and results/pans_combined/...
with --pan_combined), also for an image set without ground truth (categories then from --panoptic_categories). `--score_panoptic`
scores such a prediction, or any other tool's, against the panoptic ground truth without building the model
(metrics['panoptic']). `--eval_pixels` (Cityscapes with a semantic head) also scores the semantic predictions with the Cityscapes
pixel-level IoU / iIoU per class and category against the gtFine labelIds and instanceIds maps (metrics['pixel_iou'],
dataset/cityscapes_pixel_eval.py). `--write_ssegs` writes the semantic predictions as the reference does, palette PNGs of train ids
under results/ssegs, or with `--ssegs_label_ids` grey PNGs of label ids under results/ssegs_label_ids (what the benchmark server
takes), also for an image set without ground truth; `--score_ssegs <folder>` scores such a folder, or another tool's, without
building the model (metrics['pixel_iou']). `--write_instances` (Cityscapes with a mask head) writes the instance predictions in the
benchmark's format, results/inst_seg/<image>pred.txt and one mask PNG per detection under results/inst_seg/seg_results (8-bit grey, or
bit depth 1 with `--instances_1bit`; dataset/cityscapes_inst_format.py), also for an image set without ground truth;
`--score_instances <folder>` scores such a folder, or another tool's, without building the model (metrics['instance_ap']). `--vis_mask` (or `test.vis_mask: true` in the yaml; needs a mask head) draws the detections
of score >= 0.5 over every image into results/vis, one PNG per image (BaseDataset.vis_all_mask, dataset/vis.py), with the reference's
control flow: a run writes the pickle, draws and skips the evaluation (upsnet_end2end_test.py:300-301); with `--eval_only` the drawing
comes first and the evaluation follows (:172-173), and the images must be on disk. `--vis_panoptic {flat,overlay,both}` (a panoptic
head, or --pan_combined) draws every panoptic result that is scored into the folder --write_panoptic uses: <folder>/vis_flat (category
colours, white contours around the thing instances: the reference's vis_panoptic picture) and / or <folder>/vis (segments, borders and
category names over the photograph; labels from `--vis_panoptic_min_area` pixels, default 1024), beside the evaluation and also for an
image set without ground truth (dataset/pan_vis.py; the paths come back as 'vis_panoptic_files'). `--aug_scales S [S ...]` and `--aug_flip` (or
`test.aug_scales` / `test.aug_flip` in the yaml) turn on multi-scale / flip test-time augmentation (upsnet_amd/tta.py): every
image runs once per augmentation, eagerly and with one image in flight, the results are merged on the device in the base frame, and the
results pickle also carries 'test_aug', the augmentation list; `--eval_proposals` is refused with it (there is no single proposal list).
`--bbox_vote [--bbox_vote_thresh T]` (or `test.bbox_vote` / `test.bbox_vote_thresh` in the yaml) turns on box voting (csrc/box_vote.hip,
DESIGN 4.21): every kept detection box, class-wise and panoptic, becomes the score-weighted mean of the candidates of its class above
`test.score_thresh` whose IoU with it is >= T (default 0.8); scores, classes and order stay. Voting lives on the eager path of the
augmentation: on its own it runs that path with the base augmentation alone; the results pickle also carries 'bbox_vote',
[score_thresh, T]; `--eval_proposals` is refused with it as well.
`--soft_nms [--soft_nms_method linear|gaussian] [--soft_nms_sigma S]` (or `test.soft_nms` / `test.soft_nms_method` / `test.soft_nms_sigma` /
`test.soft_nms_score_thresh` in the yaml) turns on soft-NMS in the class-wise detection selection (csrc/detect.hip): a
candidate that overlaps a kept one stays with a decayed score and is dropped only below `test.soft_nms_score_thresh` (0.0001); the
detection scores written are the decayed ones; the panoptic selection stays hard NMS. It lives on the same eager path (on its own: the
base augmentation alone), comes before the voting, and the results pickle also carries 'soft_nms', [method, sigma, floor];
`--eval_proposals` is refused with it too.
`--pan_min_component N [--pan_component_connectivity {4,8}]` (or `test.pan_min_component` / `test.pan_component_connectivity` /
`test.pan_component_keep_largest` in the yaml) removes disconnected fragments from every panoptic result before it is scored, written
or drawn (csrc/pan_components.hip): a connected component of a (category, instance) pair with fewer than N pixels becomes
VOID, the largest component of the pair excepted; the results pickle is not changed, so `--eval_only` may try another N. With
`--pan_component_mode absorb` (or `test.pan_component_mode`) such a component takes the pair of the segment it shares the
longest border with, and becomes VOID only where it borders none.
`--pan_confidence` (or `test.pan_confidence`) makes the panoptic head also return its confidence, one byte per pixel: 255 x
the softmax over the panoptic logits at the winning label (csrc/panoptic.hip). The planes are restored beside the label maps and
pickled as 'all_pano_confs', so `--eval_only` can score again; `--write_panoptic` then writes a "score" per segment of the unified
result, its mean confidence on the map as written, and `--write_pan_confidence` the planes as grey PNGs to results/pans_unified/conf.
`--pan_min_score T` (or `test.pan_min_score`; implies the above) turns every unified segment of a mean confidence below T into VOID
(csrc/pan_confidence.hip) after get_unified_pan_result and before the fragment cleaning; a results pickle written without the option
holds no planes, and using it with the option raises a ValueError that says so. The combined merge has no panoptic logits: with
`--pan_combined` only the unified result is scored or filtered (logged once).
One rank only (WORLD_SIZE > 1 is refused)."""
import logging
import os
import pickle
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from .config.config import config, pan_confidence_wanted

logger = logging.getLogger(__name__)

MAX_DECODE_THREADS = 8


def final_output_path(cfg):
    """lib/utils/logging.py:20-40: <output_path>/<cfg name>/<test_image_set, '+' -> '_'>."""
    return os.path.join(config.output_path, os.path.basename(cfg).split('.')[0],
                        '_'.join(str(config.dataset.test_image_set).split('+')))


def default_weight_path(cfg):
    """The checkpoint the reference loads without --weight_path (upsnet_end2end_test.py:190-193): output_path / <cfg name> /
    <image_set> / <model_prefix><test_iteration>.pth."""
    return os.path.join(config.get('output_path', ''), os.path.basename(cfg).split('.')[0],
                        '_'.join(str(config.dataset.get('image_set', '')).split('+')),
                        '%s%s.pth' % (config.get('model_prefix', ''), config.test.get('test_iteration', '')))


def build_dataset(result_path):
    from . import dataset as datasets
    name = config.dataset.dataset
    cls = getattr(datasets, name, None)
    if cls is None:
        raise ValueError('config.dataset.dataset %r names no dataset class (Cityscapes, coco)' % (name,))
    return cls(image_sets=str(config.dataset.test_image_set).split('+'), flip=False, result_path=result_path, phase='test')


def scale_boxes(pred_boxes, im_info):
    """im_detect's pred_boxes[:, 1:] / im_info[2] (float32 numpy divided by a float32 scalar)."""
    return pred_boxes[:, 1:].float().cpu().numpy() / np.float32(im_info[2])


def post_image(out, im_info, num_classes, all_boxes, all_masks, all_ssegs, all_panos, all_pano_cls_inds, all_proposals=None,
               all_pano_confs=None):
    """One image's share of the reference's loop after the network (upsnet_end2end_test.py:254-272): appends to the result lists;
    with all_proposals (a list), also the box head's proposals at the original image scale (scale_boxes' rule), float32 [n, 4]; with
    all_pano_confs (a list), also the panoptic confidence plane restored beside the label maps (config.test.pan_confidence)."""
    if all_proposals is not None:
        all_proposals.append(scale_boxes(out['proposals'], im_info))
    from .dataset.restore import restore_plane_to_image, restore_to_image
    from .dataset.rle import im_post
    net = config.network
    if net.has_rcnn:
        boxes = scale_boxes(out['pred_boxes'], im_info)
        cls_inds = out['cls_inds']
        if net.has_mask_head:
            im_size = np.round(im_info[:2] / im_info[2]).astype(np.int32)
            im_post(all_boxes, all_masks, out['cls_probs'], torch.from_numpy(boxes).to(out['mask_probs'].device), out['mask_probs'],
                    cls_inds, num_classes, im_size)
        else:
            cls_np, scores = cls_inds.cpu().numpy(), out['cls_probs'].cpu().numpy().reshape(-1, 1)
            for idx in range(1, num_classes):
                sel = cls_np == idx
                all_boxes[idx].append(np.hstack([boxes[sel], scores[sel]]))
    if net.has_fcn_head or net.has_panoptic_head:
        sseg, pano = restore_to_image(out['fcn_outputs'], out['panoptic_outputs'] if net.has_panoptic_head else None, im_info)
        if net.has_fcn_head:
            all_ssegs.append(sseg.cpu().numpy())
        if net.has_panoptic_head:
            all_panos.append(pano.cpu().numpy())
            all_pano_cls_inds.append(out['panoptic_cls_inds'].cpu().numpy())
            if all_pano_confs is not None:
                all_pano_confs.append(restore_plane_to_image(out['panoptic_conf'], im_info).cpu().numpy())


def run_inference(model, dataset, in_flight=1, device=None, keep_proposals=False):
    """The test loop over the whole image list. Returns (results dict as pickled, per-image timings). keep_proposals: also
    results['all_proposals'] (model.keep_proposals is set for the run)."""
    from .dataset.blob import blob_geometry, get_image_blob
    net = config.network
    n, num_classes = len(dataset), dataset.num_classes
    all_boxes = [[] for _ in range(num_classes)]
    all_masks = [[] for _ in range(num_classes)] if net.has_mask_head else None
    all_ssegs = [] if net.has_fcn_head else None
    all_panos, all_pano_cls_inds = ([], []) if net.has_panoptic_head else (None, None)
    all_proposals = [] if keep_proposals else None
    all_pano_confs = [] if net.has_panoptic_head and pan_confidence_wanted() else None
    from .tta import augmentation_list, bbox_vote_params, eager_path_enabled, soft_nms_params
    test_aug = augmentation_list() if eager_path_enabled() else None     # (box voting / soft-NMS alone: the base augmentation, eagerly)
    bbox_vote = bbox_vote_params()
    soft_nms = soft_nms_params()
    if test_aug is not None and keep_proposals:
        raise ValueError('keep_proposals with test-time augmentation, box voting or soft-NMS: there is no single proposal list to keep')
    if keep_proposals:
        model.keep_proposals = True
    depth = max(1, min(int(in_flight), getattr(model, 'graph_slots', 1))) if hasattr(model, 'forward_async') else 1
    launch = model.forward_async if depth > 1 else model
    if test_aug is not None:     # one forward per augmentation of the decoded image, eagerly, one image in flight
        depth = 1
    workers = max(1, min(MAX_DECODE_THREADS, n))     # (never sized from the host's CPU count)
    ahead = 2 * workers                               # images decoded ahead of the device
    times = {'data_time': [], 'net_time': [], 'post_time': []}
    pending = []

    def finish(i, handle, im_info, data_time, t_launch):
        t0 = time.perf_counter()
        out = handle.result() if hasattr(handle, 'result') else handle
        if device is not None and device.type == 'cuda':
            torch.cuda.synchronize(device)
        t1 = time.perf_counter()
        # (with keep_proposals, out['proposals'] may be a view of a graph slot's buffer: it is read here, after the synchronise
        # above and before that slot's next replay -- the next image of the slot is launched only after this finish())
        post_image(out, im_info, num_classes, all_boxes, all_masks, all_ssegs, all_panos, all_pano_cls_inds, all_proposals, all_pano_confs)
        post_time = time.perf_counter() - t1
        # net_time: host time blocked on the network for this image (launch + wait); with one image in flight that is the
        # reference's forward + synchronize
        times['data_time'].append(data_time)
        times['net_time'].append(t_launch + t1 - t0)
        times['post_time'].append(post_time)
        logger.info('Batch %d/%d, data_time:%.3f, net_time:%.3f, post_time:%.3f', i + 1, n, data_time, times['net_time'][-1], post_time)

    with ThreadPoolExecutor(max_workers=workers) as pool, torch.no_grad():
        decoded = {j: pool.submit(dataset.load_image, j) for j in range(min(ahead, n))}
        for i in range(n):
            if i + ahead < n:
                decoded[i + ahead] = pool.submit(dataset.load_image, i + ahead)
            t0 = time.perf_counter()
            image = decoded.pop(i).result()
            if test_aug is not None:     # (forward_tta builds every augmentation's blob itself; the outputs are in the base frame)
                im_scale, resized, _ = blob_geometry(image.shape[0], image.shape[1], config.test.scales[0], config.test.max_size)
                im_info = np.array([[resized[0], resized[1], im_scale]], dtype=np.float32)
                t1 = time.perf_counter()
                handle = model.forward_tta(image, device=device)
            else:
                data = get_image_blob(image, device=device)
                im_info = data['im_info']
                t1 = time.perf_counter()
                handle = launch({'data': data['data'], 'im_info': data['im_info']})
            pending.append((i, handle, im_info[0], t1 - t0, time.perf_counter() - t1))
            if len(pending) >= depth:
                finish(*pending.pop(0))
        while pending:
            finish(*pending.pop(0))
    results = {'all_boxes': all_boxes, 'all_masks': all_masks, 'all_ssegs': all_ssegs, 'all_panos': all_panos,
               'all_pano_cls_inds': all_pano_cls_inds}
    if keep_proposals:
        results['all_proposals'] = all_proposals
    if all_pano_confs is not None:
        results['all_pano_confs'] = all_pano_confs
    if test_aug is not None:
        results['test_aug'] = [list(a) for a in test_aug]
    if bbox_vote is not None:
        results['bbox_vote'] = list(bbox_vote)
    if soft_nms is not None:
        results['soft_nms'] = list(soft_nms)
    return results, times


_COMBINED_NOTE = []     # (the note about the combined merge is logged once per process)


def panoptic_confs(results, combined, order):
    """The confidence planes that go with panoptic_predictions' maps, or None: the option is off, or the maps are the combined merge's,
    which has no panoptic logits (logged once). ValueError: the option needs planes that an older result file does not hold."""
    if not pan_confidence_wanted():
        return None
    if combined:
        if not _COMBINED_NOTE:
            _COMBINED_NOTE.append(True)
            logger.info('panoptic confidence: the combined merge has no panoptic logits; only the unified result is scored or filtered')
        return None
    if results.get('all_pano_confs') is None:
        raise ValueError("test.pan_confidence / test.pan_min_score need the confidence planes, and these results hold none "
                         "('all_pano_confs' is missing: the result file was written without the option; run the inference again)")
    return [results['all_pano_confs'][k] for k in order]


def panoptic_predictions(dataset, results, combined, order=None):
    """The 2-channel maps of the results, unified (the panoptic head's) or combined (the heuristic merge), one per entry of `order`
    (positions in the image list; default: the image list's own order). With config.test.pan_min_score > 0 the unified maps first lose
    the segments of a lower mean confidence (dataset.filter_pan_result). With config.test.pan_min_component > 0 the maps
    then pass through dataset.clean_pan_result (disconnected fragments become VOID): scoring, writing and drawing see the
    same maps."""
    order = list(range(len(dataset))) if order is None else order
    if not combined:
        pans = dataset.get_unified_pan_result([results['all_ssegs'][k] for k in order], [results['all_panos'][k] for k in order],
                                              [results['all_pano_cls_inds'][k] for k in order],
                                              stuff_area_limit=config.test.panoptic_stuff_area_limit)
        if config.test.get('pan_min_score', 0.0) > 0:
            pans = dataset.filter_pan_result(pans, panoptic_confs(results, False, order))
    else:
        def ordered(per_class):
            return [[v[k] for k in order] if c else v for c, v in enumerate(per_class)]
        pans = dataset.get_combined_pan_result([results['all_ssegs'][k] for k in order], ordered(results['all_boxes']),
                                               ordered(results['all_masks']), stuff_area_limit=config.test.panoptic_stuff_area_limit)
    if config.test.get('pan_min_component', 0) > 0:
        pans = dataset.clean_pan_result(pans, what='combined pano result' if combined else 'unified pano result')
    return pans


def ssegs_folder(results_dir, label_ids):
    return os.path.join(results_dir, 'ssegs_label_ids' if label_ids else 'ssegs')


def evaluate_results(dataset, results, results_dir, pan_combined=False, eval_proposals=False, eval_instances=False, write_panoptic=False,
                     panoptic_categories=None, eval_pixels=False, write_ssegs=False, ssegs_label_ids=False, write_instances=False,
                     instances_1bit=False, eval_boundary=False, boundary_dilation_ratio=0.02, boundary_pq_ratio=None, vis_panoptic=None,
                     vis_panoptic_min_area=1024, vis_panoptic_files=None, write_pan_confidence=False):
    """The reference's evaluation calls (upsnet_end2end_test.py:300-314), each only when its head is configured. Returns
    {'box_ap': stats, 'mask_ap': stats, 'panoptic': PQ dict, 'sseg': mIoU dict} (the keys of the heads that ran), plus
    'panoptic_combined' (PQ dict of get_combined_pan_result) with pan_combined and 'proposal_ar' (AR@100 ... ARl@1000 of
    results['all_proposals']) with eval_proposals and 'instance_ap' (Cityscapes instance-level AP summary) with eval_instances.
    write_panoptic: every panoptic result that is scored (or, without ground truth, would be) is also written in COCO panoptic format
    to results_dir/pans_unified or pans_combined (BaseDataset.write_panoptic). eval_pixels adds 'pixel_iou' (Cityscapes pixel-level
    IoU / iIoU); write_ssegs writes the semantic predictions to results_dir/ssegs (palette PNGs of train ids) or, with
    ssegs_label_ids, to results_dir/ssegs_label_ids (grey PNGs of label ids), with or without ground truth. write_instances writes
    the instance predictions in the Cityscapes benchmark format to results_dir/inst_seg (Cityscapes.write_instance_result; mask PNGs
    of bit depth 1 with instances_1bit), with or without ground truth. eval_boundary adds 'boundary_ap' (the 12 stats of Boundary AP
    at boundary_dilation_ratio, BaseDataset.evaluate_boundary) after the mask AP. boundary_pq_ratio (not None) adds 'panoptic_boundary'
    after 'panoptic' and 'panoptic_combined_boundary' after 'panoptic_combined': Boundary PQ of the same predictions at that ratio
    (BaseDataset.evaluate_panoptic_boundary). vis_panoptic ('flat', 'overlay' or 'both'): every panoptic result that is scored (or,
    without ground truth, would be) is also drawn into the folder write_panoptic uses, <folder>/vis_flat and / or <folder>/vis
    (BaseDataset.vis_panoptic, labels from vis_panoptic_min_area pixels); the written paths are appended to vis_panoptic_files.
    With config.test.pan_confidence (or pan_min_score > 0) and results['all_pano_confs'], write_panoptic's pred.json of the unified
    result carries a "score" per segment; write_pan_confidence also writes the planes to pans_unified/conf/*.png."""
    net = config.network
    metrics = {}
    if write_ssegs:
        dataset.write_segmentation_result(results['all_ssegs'], ssegs_folder(results_dir, ssegs_label_ids), label_ids=ssegs_label_ids)
    if write_instances:
        dataset.write_instance_result(results['all_boxes'], results['all_masks'], results_dir, one_bit=instances_1bit)
    if not dataset.has_gt:
        logger.info('%s has no annotations (%s): evaluation skipped', dataset.name, os.path.basename(dataset.instances_json_file))
        if write_panoptic or vis_panoptic:
            for combined in ([False] if net.has_panoptic_head else []) + ([True] if pan_combined else []):
                pans = panoptic_predictions(dataset, results, combined)
                folder = os.path.join(results_dir, 'pans_combined' if combined else 'pans_unified')
                if write_panoptic:
                    dataset.write_panoptic(pans, folder, categories_json=panoptic_categories,
                                           confs=panoptic_confs(results, combined, list(range(len(dataset)))),
                                           write_conf=write_pan_confidence and not combined)
                draw_panoptic(dataset, pans, folder, vis_panoptic, vis_panoptic_min_area, panoptic_categories, vis_panoptic_files)
        return metrics
    os.makedirs(results_dir, exist_ok=True)
    if net.has_rcnn:
        metrics['box_ap'] = dataset.evaluate_boxes(results['all_boxes'], results_dir)
    if net.has_rcnn and net.has_mask_head:
        metrics['mask_ap'] = dataset.evaluate_masks(results['all_boxes'], results['all_masks'], results_dir).stats
    if eval_boundary:
        logger.info('boundary result:')
        metrics['boundary_ap'] = dataset.evaluate_boundary(results['all_boxes'], results['all_masks'], results_dir,
                                                           dilation_ratio=boundary_dilation_ratio).stats
    if net.has_panoptic_head:
        logger.info('unified pano result:')
        pans = panoptic_predictions(dataset, results, False, dataset.panoptic_order())
        metrics['panoptic'] = dataset.evaluate_panoptic(pans, os.path.join(results_dir, 'pans_unified'))
        if boundary_pq_ratio is not None:
            logger.info('unified pano boundary result:')
            metrics['panoptic_boundary'] = dataset.evaluate_panoptic_boundary(pans, os.path.join(results_dir, 'pans_unified'),
                                                                              dilation_ratio=boundary_pq_ratio)
        if write_panoptic:
            dataset.write_panoptic(pans, os.path.join(results_dir, 'pans_unified'), confs=panoptic_confs(results, False, dataset.panoptic_order()),
                                   write_conf=write_pan_confidence)
        draw_panoptic(dataset, pans, os.path.join(results_dir, 'pans_unified'), vis_panoptic, vis_panoptic_min_area, None, vis_panoptic_files)
    if pan_combined:
        logger.info('combined pano result:')
        pans = panoptic_predictions(dataset, results, True, dataset.panoptic_order())
        metrics['panoptic_combined'] = dataset.evaluate_panoptic(pans, os.path.join(results_dir, 'pans_combined'))
        if boundary_pq_ratio is not None:
            logger.info('combined pano boundary result:')
            metrics['panoptic_combined_boundary'] = dataset.evaluate_panoptic_boundary(pans, os.path.join(results_dir, 'pans_combined'),
                                                                                       dilation_ratio=boundary_pq_ratio)
        if write_panoptic:
            dataset.write_panoptic(pans, os.path.join(results_dir, 'pans_combined'), confs=panoptic_confs(results, True, None))
        draw_panoptic(dataset, pans, os.path.join(results_dir, 'pans_combined'), vis_panoptic, vis_panoptic_min_area, None, vis_panoptic_files)
    if net.has_fcn_head:
        metrics['sseg'] = dataset.evaluate_ssegs(results['all_ssegs'], os.path.join(results_dir, 'ssegs'))
    if eval_proposals:
        logger.info('proposal recall:')
        # (the roidb, and so the results lists, are in ascending image id, the order evaluate_proposals takes)
        metrics['proposal_ar'] = dataset.evaluate_proposals(results['all_proposals'], results_dir)
    if eval_instances:
        logger.info('instance-level result:')
        metrics['instance_ap'] = dataset.evaluate_instances(results['all_boxes'], results['all_masks'], results_dir)
    if eval_pixels:
        logger.info('pixel-level result:')
        metrics['pixel_iou'] = dataset.evaluate_pixels(results['all_ssegs'], results_dir)
    return metrics


def draw_panoptic(dataset, pans, folder, which, min_area, categories_json, files):
    """--vis_panoptic: the pictures of one panoptic result into folder/vis_flat and / or folder/vis; `files` collects the paths."""
    for mode in {'flat': ('flat',), 'overlay': ('overlay',), 'both': ('flat', 'overlay')}.get(which, ()):
        paths = dataset.vis_panoptic(pans, folder, mode=mode, categories_json=categories_json, label_min_area=min_area)
        if files is not None:
            files.extend(paths)


def check_pixel_run(dataset, args):
    """--eval_pixels before anything runs: refused on an image set without ground truth (writing still works there), and the
    label-id and instance-id maps join the upfront file check."""
    if not args.eval_pixels:
        return
    if not dataset.has_gt:
        raise SystemExit('--eval_pixels: %s has no ground truth to score against (--write_ssegs [--ssegs_label_ids] writes its '
                         'predictions)' % dataset.name)
    dataset.check_pixel_files()


def draw_results(dataset, results, results_dir):
    """config.test.vis_mask: test_dataset.vis_all_mask(all_boxes, all_masks, <results>/vis); returns the written paths."""
    return dataset.vis_all_mask(results['all_boxes'], results['all_masks'], os.path.join(results_dir, 'vis'))


def main(argv=None):
    """Returns {'metrics': ..., 'results_file': path, 'times': per-image timings (None with --eval_only)}, and with config.test.vis_mask
    also 'vis_files': the PNGs written under results/vis, and with --vis_panoptic 'vis_panoptic_files': the pictures written under
    results/pans_unified (and pans_combined)."""
    from .config.parse_args import parse_args
    args = parse_args('UPSNet: run and score a checkpoint over an evaluation set', argv)
    logging.basicConfig(level=logging.INFO, format='%(asctime)-15s | %(message)s')
    world = int(os.environ.get('WORLD_SIZE', '1'))
    if world > 1:
        raise SystemExit('upsnet_amd.evaluate runs on one rank; WORLD_SIZE=%d is refused (sharding the image list across ranks is '
                         'not implemented)' % world)
    if not args.cfg:
        raise SystemExit('--cfg <experiment yaml> is required: it names the dataset, the image set and the output path')
    if args.weight_path and args.synthetic_weights:
        raise SystemExit('--weight_path and --synthetic_weights exclude each other')
    net = config.network
    if args.pan_combined and not (net.has_rcnn and net.has_mask_head and net.has_fcn_head):
        raise SystemExit('--pan_combined merges detections, instance masks and the semantic map: it needs network.has_rcnn, '
                         'has_mask_head and has_fcn_head (has_rcnn=%s, has_mask_head=%s, has_fcn_head=%s)'
                         % (net.has_rcnn, net.has_mask_head, net.has_fcn_head))
    if args.eval_instances and not (config.dataset.dataset == 'Cityscapes' and net.has_rcnn and net.has_mask_head):
        raise SystemExit('--eval_instances scores instance masks against the Cityscapes gtFine instanceIds maps: it needs '
                         'dataset.dataset = Cityscapes and network.has_rcnn and has_mask_head (dataset=%s, has_rcnn=%s, has_mask_head=%s)'
                         % (config.dataset.dataset, net.has_rcnn, net.has_mask_head))
    if args.eval_boundary and not (net.has_rcnn and net.has_mask_head):
        raise SystemExit('--eval_boundary scores the instance masks with Boundary AP: it needs network.has_rcnn and has_mask_head '
                         '(has_rcnn=%s, has_mask_head=%s)' % (net.has_rcnn, net.has_mask_head))
    if args.boundary_dilation_ratio is not None and not args.eval_boundary:
        raise SystemExit('--boundary_dilation_ratio sets the boundary width of --eval_boundary, which is missing')
    if args.eval_boundary:
        from .dataset.boundary import check_dilation_ratio
        try:
            check_dilation_ratio(0.02 if args.boundary_dilation_ratio is None else args.boundary_dilation_ratio)
        except ValueError as e:
            raise SystemExit('--boundary_dilation_ratio: %s' % e)
    if args.eval_boundary_pq and not (net.has_panoptic_head or args.pan_combined or args.score_panoptic):
        raise SystemExit('--eval_boundary_pq scores the panoptic predictions with Boundary PQ: it needs network.has_panoptic_head, or '
                         '--pan_combined (has_panoptic_head=%s)' % net.has_panoptic_head)
    if args.boundary_pq_dilation_ratio is not None and not args.eval_boundary_pq:
        raise SystemExit('--boundary_pq_dilation_ratio sets the boundary width of --eval_boundary_pq, which is missing')
    boundary_pq_ratio = None
    if args.eval_boundary_pq:
        from .dataset.boundary import check_dilation_ratio
        try:
            boundary_pq_ratio = check_dilation_ratio(0.02 if args.boundary_pq_dilation_ratio is None else args.boundary_pq_dilation_ratio)
        except ValueError as e:
            raise SystemExit('--boundary_pq_dilation_ratio: %s' % e)
    if args.write_instances and not (config.dataset.dataset == 'Cityscapes' and net.has_rcnn and net.has_mask_head):
        raise SystemExit('--write_instances writes the instance masks in the Cityscapes benchmark format: it needs dataset.dataset = '
                         'Cityscapes and network.has_rcnn and has_mask_head (dataset=%s, has_rcnn=%s, has_mask_head=%s)'
                         % (config.dataset.dataset, net.has_rcnn, net.has_mask_head))
    if args.instances_1bit and not args.write_instances:
        raise SystemExit('--instances_1bit chooses the mask format of --write_instances, which is missing')
    if args.score_instances and config.dataset.dataset != 'Cityscapes':     # (no model is built: the heads do not matter)
        raise SystemExit('--score_instances scores instance prediction files against the Cityscapes gtFine instanceIds maps: it needs '
                         'dataset.dataset = Cityscapes (dataset=%s)' % config.dataset.dataset)
    from .tta import augmentation_enabled, augmentation_list, bbox_vote_params, eager_path_enabled, soft_nms_params
    if eager_path_enabled() and not (args.eval_only or args.score_panoptic or args.score_ssegs or args.score_instances):
        if args.eval_proposals and augmentation_enabled():
            raise SystemExit('--eval_proposals with test-time augmentation (--aug_scales / --aug_flip) is refused: the detections come from '
                             'the union of every augmentation\'s proposals, so there is no single proposal list to score')
        if args.eval_proposals and config.test.get('soft_nms', False):
            raise SystemExit('--eval_proposals with soft-NMS (--soft_nms) is refused: the soft selection runs on the eager path of the '
                             'test-time augmentation, which keeps no single proposal list to score')
        if args.eval_proposals:
            raise SystemExit('--eval_proposals with box voting (--bbox_vote) is refused: voting runs on the eager path of the test-time '
                             'augmentation, which keeps no single proposal list to score')
        try:
            augmentation_list()
        except ValueError as e:
            raise SystemExit('--aug_scales / --aug_flip: %s' % e)
        try:
            bbox_vote_params()
        except ValueError as e:
            raise SystemExit('--bbox_vote_thresh: %s' % e)
        try:
            soft_nms_params()
        except ValueError as e:
            raise SystemExit('--soft_nms: %s' % e)
    vis_mask = bool(config.test.get('vis_mask', False))
    if vis_mask and not (net.has_rcnn and net.has_mask_head):
        raise SystemExit('--vis_mask (config.test.vis_mask) draws the detections and their instance masks: it needs network.has_rcnn and '
                         'has_mask_head (has_rcnn=%s, has_mask_head=%s)' % (net.has_rcnn, net.has_mask_head))
    if args.score_ssegs and config.dataset.dataset != 'Cityscapes':     # (no model is built: the heads do not matter)
        raise SystemExit('--score_ssegs scores semantic PNGs against the Cityscapes gtFine maps: it needs dataset.dataset = Cityscapes '
                         '(dataset=%s)' % config.dataset.dataset)
    for flag in ('eval_pixels', 'write_ssegs'):
        if getattr(args, flag) and not (config.dataset.dataset == 'Cityscapes' and net.has_fcn_head):
            raise SystemExit('--%s works on the semantic predictions of a Cityscapes run (label ids, gtFine maps): it needs dataset.dataset '
                             '= Cityscapes and network.has_fcn_head (dataset=%s, has_fcn_head=%s)' % (flag, config.dataset.dataset, net.has_fcn_head))
    if args.ssegs_label_ids and not args.write_ssegs:
        raise SystemExit('--ssegs_label_ids chooses the format of --write_ssegs, which is missing')
    if args.write_panoptic and not (net.has_panoptic_head or args.pan_combined):
        raise SystemExit('--write_panoptic writes the panoptic predictions: it needs network.has_panoptic_head, or --pan_combined '
                         '(has_panoptic_head=%s)' % net.has_panoptic_head)
    if args.vis_panoptic and not (net.has_panoptic_head or args.pan_combined):
        raise SystemExit('--vis_panoptic draws the panoptic predictions: it needs network.has_panoptic_head, or --pan_combined '
                         '(has_panoptic_head=%s)' % net.has_panoptic_head)
    if args.vis_panoptic_min_area is not None and args.vis_panoptic not in ('overlay', 'both'):
        raise SystemExit('--vis_panoptic_min_area sets the smallest labelled segment of --vis_panoptic overlay / both, which is missing')
    if args.vis_panoptic_min_area is not None and args.vis_panoptic_min_area < 0:
        raise SystemExit('--vis_panoptic_min_area: %d is negative' % args.vis_panoptic_min_area)
    if pan_confidence_wanted() and not net.has_panoptic_head:
        raise SystemExit('--pan_confidence / --pan_min_score read the panoptic head\'s logits: they need network.has_panoptic_head '
                         '(has_panoptic_head=%s)' % net.has_panoptic_head)
    if args.write_pan_confidence and not (args.write_panoptic and pan_confidence_wanted()):
        raise SystemExit('--write_pan_confidence writes the confidence planes beside the files of --write_panoptic: it needs '
                         '--write_panoptic and --pan_confidence (or --pan_min_score)')
    pv_files = []
    pv_kw = dict(vis_panoptic=args.vis_panoptic, vis_panoptic_files=pv_files, write_pan_confidence=args.write_pan_confidence,
                 vis_panoptic_min_area=1024 if args.vis_panoptic_min_area is None else args.vis_panoptic_min_area)
    pv_out = {'vis_panoptic_files': pv_files} if args.vis_panoptic else {}
    if args.score_panoptic_folder and not args.score_panoptic:
        raise SystemExit('--score_panoptic_folder names the PNG folder of --score_panoptic <pred.json>, which is missing')
    boundary_ratio = 0.02 if args.boundary_dilation_ratio is None else args.boundary_dilation_ratio
    out_dir = final_output_path(args.cfg)
    if args.score_panoptic:
        if not os.path.isfile(args.score_panoptic):
            raise SystemExit('--score_panoptic: no prediction JSON at %s' % args.score_panoptic)
        folder = args.score_panoptic_folder or os.path.splitext(args.score_panoptic)[0]
        if not os.path.isdir(folder):
            raise SystemExit('--score_panoptic: no PNG folder at %s (name it with --score_panoptic_folder)' % folder)
        dataset = build_dataset(out_dir)
        if not dataset.has_gt:
            raise SystemExit('--score_panoptic: %s has no ground truth to score against' % dataset.name)
        for p in (dataset.panoptic_json_file,):
            if not os.path.isfile(p):
                raise SystemExit('--score_panoptic: no panoptic ground truth at %s' % p)
        logger.info('panoptic result of %s:', args.score_panoptic)
        metrics = {'panoptic': dataset.evaluate_panoptic_files(args.score_panoptic, folder)}
        if boundary_pq_ratio is not None:
            logger.info('panoptic boundary result of %s:', args.score_panoptic)
            metrics['panoptic_boundary'] = dataset.evaluate_panoptic_files(args.score_panoptic, folder, boundary=True,
                                                                           dilation_ratio=boundary_pq_ratio)
        return {'metrics': metrics, 'results_file': None, 'times': None}
    if args.score_ssegs:
        if not os.path.isdir(args.score_ssegs):
            raise SystemExit('--score_ssegs: no folder at %s' % args.score_ssegs)
        dataset = build_dataset(out_dir)
        if not dataset.has_gt:
            raise SystemExit('--score_ssegs: %s has no ground truth to score against' % dataset.name)
        dataset.check_pixel_files()
        logger.info('pixel-level result of %s:', args.score_ssegs)
        return {'metrics': {'pixel_iou': dataset.evaluate_pixels_files(args.score_ssegs)}, 'results_file': None, 'times': None}
    if args.score_instances:
        if not os.path.isdir(args.score_instances):
            raise SystemExit('--score_instances: no folder at %s' % args.score_instances)
        dataset = build_dataset(out_dir)
        if not dataset.has_gt:
            raise SystemExit('--score_instances: %s has no ground truth to score against' % dataset.name)
        dataset.check_instance_files()
        logger.info('instance-level result of %s:', args.score_instances)
        return {'metrics': {'instance_ap': dataset.evaluate_instances_files(args.score_instances)}, 'results_file': None, 'times': None}
    results_dir = os.path.join(out_dir, 'results')
    results_file = os.path.join(results_dir, 'results_list.pkl')
    if args.eval_only:
        if not os.path.isfile(results_file):
            raise SystemExit('--eval_only: no results to evaluate at %s (run without --eval_only first)' % results_file)
        with open(results_file, 'rb') as f:
            results = pickle.load(f)
        if args.eval_proposals and 'all_proposals' not in results:
            raise SystemExit('--eval_only --eval_proposals: %s holds no proposals (all_proposals); run with --eval_proposals without '
                             '--eval_only first' % results_file)
        dataset = build_dataset(out_dir)
        dataset.check_files(images=vis_mask or args.vis_panoptic in ('overlay', 'both'))
        if args.eval_instances:
            dataset.check_instance_files()
        check_pixel_run(dataset, args)
        if vis_mask:        # (upsnet_end2end_test.py:172-173: drawn first, then evaluated)
            vis_files = draw_results(dataset, results, results_dir)
            return {'metrics': evaluate_results(dataset, results, results_dir, args.pan_combined, args.eval_proposals, args.eval_instances,
                                                 args.write_panoptic, args.panoptic_categories or None, args.eval_pixels, args.write_ssegs,
                                                 args.ssegs_label_ids, args.write_instances, args.instances_1bit, args.eval_boundary, boundary_ratio,
                                            boundary_pq_ratio=boundary_pq_ratio, **pv_kw),
                    'results_file': results_file, 'times': None, 'vis_files': vis_files, **pv_out}
        return {'metrics': evaluate_results(dataset, results, results_dir, args.pan_combined, args.eval_proposals, args.eval_instances,
                                             args.write_panoptic, args.panoptic_categories or None, args.eval_pixels, args.write_ssegs,
                                             args.ssegs_label_ids, args.write_instances, args.instances_1bit, args.eval_boundary, boundary_ratio,
                                            boundary_pq_ratio=boundary_pq_ratio, **pv_kw),
                'results_file': results_file, 'times': None, **pv_out}

    dataset = build_dataset(out_dir)
    dataset.check_files()       # every image and GT file, before the first launch
    if args.eval_instances:
        dataset.check_instance_files()
    check_pixel_run(dataset, args)
    from .upsnet_end2end_test import init_distributed, load_checkpoint_model
    _, _, device = init_distributed()
    if args.synthetic_weights:
        from .synthetic import build_model
        logging.warning('seeded SYNTHETIC weights (upsnet_amd.synthetic, seed 235): the metrics are not those of a trained model')
        model = build_model(device=device)
    else:
        weight_path = args.weight_path or default_weight_path(args.cfg)
        model = load_checkpoint_model(weight_path, device)
        logging.info('loaded %s into %s (resume=True)', weight_path, config.symbol)
    results, times = run_inference(model, dataset, in_flight=args.in_flight, device=device, keep_proposals=args.eval_proposals)
    os.makedirs(results_dir, exist_ok=True)
    with open(results_file, 'wb') as f:
        pickle.dump(results, f, protocol=2)
    logging.info('%d images, results written to %s', len(dataset), results_file)
    if vis_mask:            # (upsnet_end2end_test.py:300-301, an if / else: drawn instead of evaluated)
        del model
        return {'metrics': {}, 'results_file': results_file, 'times': times, 'vis_files': draw_results(dataset, results, results_dir), **pv_out}
    return {'metrics': evaluate_results(dataset, results, results_dir, args.pan_combined, args.eval_proposals, args.eval_instances,
                                             args.write_panoptic, args.panoptic_categories or None, args.eval_pixels, args.write_ssegs,
                                             args.ssegs_label_ids, args.write_instances, args.instances_1bit, args.eval_boundary, boundary_ratio,
                                            boundary_pq_ratio=boundary_pq_ratio, **pv_kw),
            'results_file': results_file, 'times': times, **pv_out}


if __name__ == '__main__':
    main()
