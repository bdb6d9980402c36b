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

The MOTS measures (sMOTSA, MOTSA, MOTSP, IDS, Frag, MT / PT / ML; dataset/mots.py) are opt-in:
    --eval_mots          the same frames against the same --video_gt also go through MOTSEvaluator: 'mots' in the summary
    --mots_gt <folder>   (instead of, or beside, --video_gt) MOTS alone against <folder>/<sequence>.txt in the MOTS text format
                         (`<frame> <id> <class> <H> <W> <rle>`; class 10 is an ignore region); the frames pair by index;
                         written: <pred>/mots_scores.json {'mots_gt', 'sequences', 'summary'}
    --write_mots         writes <pred>/<sequence>/mots.txt, every tracked thing segment in that format (id = category * 1000 + instance);
                         alone it needs neither a ground truth nor --panoptic_categories
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
    p.add_argument('--eval_mots', action='store_true',
                   help="also score the MOTS measures (sMOTSA, MOTSA, MOTSP, IDS, Frag, MT/PT/ML) against --video_gt: 'mots' in the summary")
    p.add_argument('--mots_gt', type=str, default='', metavar='FOLDER',
                   help='score the MOTS measures against <FOLDER>/<sequence>.txt (MOTS text format, frames pair by index): mots_scores.json')
    p.add_argument('--write_mots', action='store_true', help='write every tracked sequence in the MOTS text format: <sequence>/mots.txt')


def check_arguments(p, args):
    """The refusals both commands share (argparse's exit): --vpq_windows without --video_gt, windows that are not ascending in 1..8,
    --eval_mots without a ground truth."""
    from .dataset.video_pq import check_windows
    if args.eval_mots and not args.video_gt and not args.mots_gt:
        p.error('--eval_mots scores against a ground truth: it needs --video_gt <folder> or --mots_gt <folder>')
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


def score_sequence(evaluator, name, pred_maps, pred_names, video_gt, mots=None):
    """Add one tracked sequence (its 2-channel maps, device tensors or numpy arrays, and their file names) to the evaluator -- and to
    `mots`, a MOTSEvaluator, if given: the same frames against the same ground truth --; returns the number of frames scored."""
    from .dataset.pan_format import png_name
    annotations, pan = load_video_gt(video_gt, name)
    pairs = pair_frames(name, pred_names, annotations)
    gts = [load_png(os.path.join(pan, png_name(ann['file_name']))) for _, ann in pairs]
    for ev in (evaluator, mots):
        if ev is None:
            continue
        try:
            ev.begin_sequence([ann['segments_info'] for _, ann in pairs], name=name)
            for (k, _), gt in zip(pairs, gts):
                ev.add_frame(pred_maps[k], gt)
        except ValueError as e:
            raise SystemExit('--video_gt: sequence %s: %s' % (name, e))
        ev.end_sequence()
    return len(pairs)


def background_category(categories):
    """The category of the pixels no mask of a MOTS text file covers: the smallest id that is not a thing category."""
    cats = categories if isinstance(categories, dict) else {el['id']: el for el in categories}
    return min(c for c in range(255) if cats.get(c, {}).get('isthing') != 1)


def score_mots_txt(evaluator, name, pred_maps, mots_gt):
    """Add one tracked sequence to a MOTSEvaluator against <mots_gt>/<name>.txt, frames paired by index; returns the frames scored."""
    from .dataset.mots import MOTSText
    path = os.path.join(mots_gt, name + '.txt')
    if not os.path.isfile(path):
        raise SystemExit('--mots_gt: no ground truth of sequence %s at %s' % (name, path))
    try:
        text = MOTSText(path, num_frames=len(pred_maps), background_category=background_category(evaluator.categories))
        evaluator.begin_sequence(text.segments_info, name=name)
        for t, m in enumerate(pred_maps):
            evaluator.add_frame(m, text.frame(t))        # (one frame of ground truth at a time, however long the sequence)
    except ValueError as e:
        raise SystemExit('--mots_gt: sequence %s: %s' % (name, e))
    evaluator.end_sequence()
    return text.num_frames


def write_mots_scores(evaluator, mots_gt, scored, path):
    summary = evaluator.summary()
    with open(path, 'w') as f:
        json.dump({'mots_gt': os.path.abspath(mots_gt), 'sequences': [{'name': n, 'frames': k} for n, k in scored], 'summary': summary}, f)
    logger.info('MOTS scores of %d sequences written to %s', len(scored), os.path.abspath(path))
    return summary


class Scoring(object):
    """What the options of a run ask for after a sequence is tracked: --video_gt (VPQ, STQ; with --eval_mots also MOTS), --mots_gt
    (MOTS against text files) and --write_mots. The constructor refuses a ground-truth folder that does not exist (SystemExit).
    add(name, tracked maps, file names, the sequence's folder) once per sequence; finish(result, folder, video_path=None) writes
    <folder>/video_scores.json (or video_path, the re-scoring command's --out) and <folder>/mots_scores.json and adds 'video_scores' /
    'mots_scores' to result."""

    def __init__(self, args, categories):
        self.args = args
        self.video = self.mots = self.mots_txt = None
        self.scored, self.scored_txt = [], []
        for option in ('video_gt', 'mots_gt'):
            folder = getattr(args, option)
            if folder and not os.path.isdir(folder):
                raise SystemExit('--%s: no folder at %s' % (option, folder))
        if args.video_gt:
            from .dataset.video_pq import VideoPanopticEvaluator
            self.video = VideoPanopticEvaluator(categories, windows=args.vpq_windows)
        if args.video_gt and args.eval_mots:
            from .dataset.mots import MOTSEvaluator
            self.mots = MOTSEvaluator(categories)
        if args.mots_gt:
            from .dataset.mots import MOTSEvaluator
            self.mots_txt = MOTSEvaluator(categories)

    def add(self, name, maps, file_names, seq_dir):
        if self.args.write_mots:
            from .dataset.mots import write_mots_txt
            os.makedirs(seq_dir, exist_ok=True)
            write_mots_txt(os.path.join(seq_dir, 'mots.txt'), maps)
        if self.video is not None:
            self.scored.append((name, score_sequence(self.video, name, maps, file_names, self.args.video_gt, mots=self.mots)))
        if self.mots_txt is not None:
            self.scored_txt.append((name, score_mots_txt(self.mots_txt, name, maps, self.args.mots_gt)))

    def finish(self, result, folder, video_path=None):
        if self.video is not None:
            result['video_scores'] = write_scores(self.video, self.args.video_gt, self.scored,
                                                  video_path or os.path.join(folder, 'video_scores.json'), mots=self.mots)
        if self.mots_txt is not None:
            result['mots_scores'] = write_mots_scores(self.mots_txt, self.args.mots_gt, self.scored_txt, os.path.join(folder, 'mots_scores.json'))
        return result


def write_scores(evaluator, video_gt, scored, path, mots=None):
    summary = evaluator.summary()
    if mots is not None:
        summary['mots'] = mots.summary()
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
    """Returns the summary (with --mots_gt alone, that of the MOTS measures; with --write_mots alone, None)."""
    args = parse_args(argv)
    logging.basicConfig(level=logging.INFO, format='%(asctime)-15s | %(message)s')
    if not args.pred:
        raise SystemExit('--pred <out folder of a sequence run> is required')
    if not args.video_gt and not args.mots_gt and not args.write_mots:
        raise SystemExit('--video_gt <folder> is required (or --mots_gt <folder>: the MOTS measures alone; or --write_mots: no scores)')
    categories = None
    if args.video_gt or args.mots_gt:          # (writing the text files needs no category table)
        if not args.panoptic_categories or not os.path.isfile(args.panoptic_categories):
            raise SystemExit("--panoptic_categories: no panoptic JSON at %r (its 'categories' say which are things)" % args.panoptic_categories)
        with open(args.panoptic_categories, 'r') as f:
            categories = json.load(f)['categories']
    scoring = Scoring(args, categories)
    sequences = discover_predictions(args.pred)
    for name, paths in sequences:
        maps = [load_png(p, '--pred', 'a 2-channel panoptic map (an RGB PNG)') for p in paths]
        scoring.add(name, maps, [os.path.basename(p) for p in paths], os.path.join(args.pred, name))
    res = scoring.finish({}, args.pred, args.out or None)
    return res.get('video_scores', res.get('mots_scores'))


if __name__ == '__main__':
    main()
