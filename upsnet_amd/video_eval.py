"""Score tracked sequences against video ground truth: VPQ and STQ (dataset/video_pq.py).

    python -m upsnet_amd.video_eval --pred <out folder of a sequence run> --video_gt <folder> --panoptic_categories <json>
                                    [--vpq_windows N [N ...]] [--out <json>]

Re-scores the written pan_2ch/ folders of `python -m upsnet_amd.sequence` without a model; the same scoring runs inside a sequence run
with its --video_gt option. Every subfolder of --pred that holds a pan_2ch/ folder is one sequence, in the order of the names.

The ground truth of sequence <name> is <video_gt>/<name>/gt.json, {'annotations': [{'file_name', 'segments_info'}]} with segments
(id, category_id, iscrowd), and one panoptic PNG per annotation, <video_gt>/<name>/pan/<frame>.png (id = R + 256 G + 65536 B, 0 = VOID);
an id means the same object in every frame. Where there is no gt.json, a sequence run's own pan/ + pred.json is taken the same way,
so two runs can be compared. Frames pair by the name of their PNG (pan_format.png_name of the annotation's file_name). The ground
truth may cover a subset of the predicted frames (Cityscapes-VPS labels every fifth): only those frames are scored, in the order of
the prediction. A ground-truth frame without a prediction ends the run, naming it.
Written: <pred>/video_scores.json (or --out): {'video_gt', 'windows', 'sequences': [{'name', 'frames'}], 'summary'}; the summary is logged.
"""
import argparse
import json
import logging
import os

import numpy as np

logger = logging.getLogger(__name__)

DEFAULT_WINDOWS = (1, 2, 3, 4)


def add_arguments(p):
    p.add_argument('--video_gt', type=str, default='', metavar='FOLDER',
                   help='score the tracked sequences (VPQ, STQ) against <FOLDER>/<sequence>/gt.json and <FOLDER>/<sequence>/pan/<frame>.png')
    p.add_argument('--vpq_windows', type=int, nargs='+', default=None, metavar='N',
                   help='VPQ window lengths in scored frames: ascending, unique, each in 1..8 (default 1 2 3 4)')


def check_arguments(p, args):
    """The refusals both commands share (argparse's exit): --vpq_windows without --video_gt, windows that are not ascending in 1..8."""
    from .dataset.video_pq import check_windows
    if args.vpq_windows is not None and not args.video_gt:
        p.error('--vpq_windows sets the windows of the video scores: it needs --video_gt <folder>')
    try:
        args.vpq_windows = check_windows(args.vpq_windows if args.vpq_windows is not None else DEFAULT_WINDOWS)
    except ValueError as e:
        p.error('--vpq_windows: %s' % e)
    return args


def load_video_gt(folder, name):
    """(annotations, folder of the PNGs) of sequence `name`; SystemExit naming what is missing."""
    root = os.path.join(folder, name)
    if not os.path.isdir(root):
        raise SystemExit('--video_gt: no ground truth of sequence %s at %s' % (name, root))
    for json_name in ('gt.json', 'pred.json'):
        path = os.path.join(root, json_name)
        if os.path.isfile(path):
            break
    else:
        raise SystemExit('--video_gt: %s holds neither gt.json nor pred.json' % root)
    with open(path, 'r') as f:
        annotations = json.load(f)['annotations']
    pan = os.path.join(root, 'pan')
    if not os.path.isdir(pan):
        raise SystemExit('--video_gt: no folder of panoptic PNGs at %s' % pan)
    return annotations, pan


def pair_frames(name, pred_names, annotations):
    """[(index of the predicted frame, annotation)] in the order of the prediction: the GT frames paired with the predicted frames by
    PNG name. SystemExit: a GT frame without a prediction, or named twice."""
    from .dataset.pan_format import png_name
    index = {png_name(n): k for k, n in enumerate(pred_names)}
    pairs = {}
    for ann in annotations:
        png = png_name(ann['file_name'])
        if png not in index:
            raise SystemExit('--video_gt: sequence %s has ground truth for frame %s, which was not predicted' % (name, png))
        if index[png] in pairs:
            raise SystemExit('--video_gt: sequence %s names frame %s twice' % (name, png))
        pairs[index[png]] = ann
    return [(k, pairs[k]) for k in sorted(pairs)]


def load_png(path, option='--video_gt', what='an RGB panoptic PNG'):
    from PIL import Image
    if not os.path.isfile(path):
        raise SystemExit('%s: no PNG at %s' % (option, path))
    im = np.array(Image.open(path))
    if im.dtype != np.uint8 or im.ndim != 3 or im.shape[2] < 3:
        raise SystemExit('%s: %s is not %s, but %s %s' % (option, path, what, im.shape, im.dtype))
    return np.ascontiguousarray(im[:, :, :3])


def score_sequence(evaluator, name, pred_maps, pred_names, video_gt):
    """Add one tracked sequence (its 2-channel maps, device tensors or numpy arrays, and their file names) to the evaluator; returns
    the number of frames scored."""
    from .dataset.pan_format import png_name
    annotations, pan = load_video_gt(video_gt, name)
    pairs = pair_frames(name, pred_names, annotations)
    gts = [load_png(os.path.join(pan, png_name(ann['file_name']))) for _, ann in pairs]
    try:
        evaluator.begin_sequence([ann['segments_info'] for _, ann in pairs], name=name)
        for (k, _), gt in zip(pairs, gts):
            evaluator.add_frame(pred_maps[k], gt)
    except ValueError as e:
        raise SystemExit('--video_gt: sequence %s: %s' % (name, e))
    evaluator.end_sequence()
    return len(pairs)


def write_scores(evaluator, video_gt, scored, path):
    summary = evaluator.summary()
    with open(path, 'w') as f:
        json.dump({'video_gt': os.path.abspath(video_gt), 'windows': list(evaluator.windows),
                   'sequences': [{'name': n, 'frames': k} for n, k in scored], 'summary': summary}, f)
    logger.info('video scores of %d sequences written to %s', len(scored), os.path.abspath(path))
    return summary


def discover_predictions(folder):
    """[(sequence name, [paths of its pan_2ch PNGs sorted by name])] of a sequence run's output folder."""
    from .sequence import _frames_in
    if not os.path.isdir(folder):
        raise SystemExit('--pred: no folder at %s' % folder)
    sequences = []
    for sub in sorted(d for d in os.listdir(folder) if os.path.isdir(os.path.join(folder, d, 'pan_2ch'))):
        frames = _frames_in(os.path.join(folder, sub, 'pan_2ch'))
        if not frames:
            raise SystemExit('--pred: %s holds no 2-channel map' % os.path.join(folder, sub, 'pan_2ch'))
        sequences.append((sub, frames))
    if not sequences:
        raise SystemExit('--pred: %s holds no sequence folder with a pan_2ch/ folder' % folder)
    return sequences


def parse_args(argv=None):
    p = argparse.ArgumentParser(description='UPSNet: VPQ and STQ of written, tracked sequences')
    p.add_argument('--pred', type=str, default='', metavar='FOLDER', help='the output folder of a sequence run (one subfolder per sequence)')
    p.add_argument('--panoptic_categories', type=str, default='', metavar='JSON', help="a panoptic JSON whose 'categories' to use")
    p.add_argument('--out', type=str, default='', metavar='JSON', help='where to write the scores (default <pred>/video_scores.json)')
    add_arguments(p)
    return check_arguments(p, p.parse_args(argv))


def main(argv=None):
    """Returns the summary."""
    args = parse_args(argv)
    logging.basicConfig(level=logging.INFO, format='%(asctime)-15s | %(message)s')
    if not args.pred:
        raise SystemExit('--pred <out folder of a sequence run> is required')
    if not args.video_gt:
        raise SystemExit('--video_gt <folder> is required')
    if not args.panoptic_categories or not os.path.isfile(args.panoptic_categories):
        raise SystemExit("--panoptic_categories: no panoptic JSON at %r (its 'categories' say which are things)" % args.panoptic_categories)
    if not os.path.isdir(args.video_gt):
        raise SystemExit('--video_gt: no folder at %s' % args.video_gt)
    sequences = discover_predictions(args.pred)
    with open(args.panoptic_categories, 'r') as f:
        categories = json.load(f)['categories']
    from .dataset.video_pq import VideoPanopticEvaluator
    evaluator = VideoPanopticEvaluator(categories, windows=args.vpq_windows)
    scored = []
    for name, paths in sequences:
        maps = [load_png(p, '--pred', 'a 2-channel panoptic map (an RGB PNG)') for p in paths]
        scored.append((name, score_sequence(evaluator, name, maps, [os.path.basename(p) for p in paths], args.video_gt)))
    return write_scores(evaluator, args.video_gt, scored, args.out or os.path.join(args.pred, 'video_scores.json'))


if __name__ == '__main__':
    main()
