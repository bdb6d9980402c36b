"""Run a checkpoint over a folder of frames and track the panoptic instances across each sequence.

    python -m upsnet_amd.sequence --cfg <yaml> (--weight_path <pth> | --synthetic_weights) --frames <folder> --out <dir>
                                  --panoptic_categories <json> [--track_iou T] [--track_max_age N] [--combined]
                                  [--track_motion {none,constant_velocity}]
                                  [--vis_panoptic {flat,overlay,both}] [--in-flight N] [--video_gt <folder> [--vpq_windows N [N ...]]]
                                  [--pan_min_component N [--pan_component_connectivity {4,8}] [--pan_component_mode {void,absorb}]]
    python -m upsnet_amd.sequence --cfg <yaml> --track_only <folder of pan_2ch PNGs> --out <dir> --panoptic_categories <json> [...]

No annotation JSON is needed. The image files directly in --frames, sorted by name, are one sequence (named after the folder); every
subfolder is a sequence of its own (named after the subfolder), sequences in the order of their names. A missing folder, a folder
without a sequence and an empty subfolder end the run with the folder's name.

Per sequence the frames run through evaluate.run_inference (decode pool, get_image_blob, forward_async, restore_to_image) and
get_unified_pan_result -- with --combined, get_combined_pan_result -- exactly as an evaluation run; then PanopticTracker
(dataset/pan_track.py; --track_iou, default 0.3, and --track_max_age, default 0) renumbers the thing instances, and the writers run
in their frame-stable mode (dataset/pan_format.py). The tracker is reset between sequences: the 8-bit instance ids start again, the
serials (track_id) go on counting, so a track_id names one object of one sequence in the whole run. Written under <out>/<sequence>/:
  pan_2ch/<frame>.png   the tracked 2-channel maps
  pan/<frame>.png       (R, G, B) = (category, instance, 1), VOID (0,0,0)
  pred.json             COCO panoptic annotations; every segment also carries 'track_id' (0 for stuff)
  tracks.json           {'tracks': [{'track_id', 'category_id', 'instance', 'first_frame', 'last_frame', 'frames'}]}, frames by name
  vis/, vis_flat/       with --vis_panoptic: the pictures, every track in one colour throughout
--track_motion constant_velocity (default none) lets the tracker predict every track's place from its velocity
before it associates: for objects in persistent motion in sparsely sampled sequences, where it keeps identities through occlusions,
accelerations and crossings; on erratic motion it matches fewer segments than the default. It applies to --track_only too.
--track_only tracks an already written prediction (for instance results/pans_unified/pan_2ch of an evaluation run) without building
the model; the photographs are not there, so of the pictures only 'flat' can be drawn. One rank only.
--pan_min_component N (or test.pan_min_component in the yaml) turns the connected components of fewer than N pixels into VOID in every
map before the tracker sees it, the largest of every segment excepted (dataset/pan_components.py), so that a
stray fragment does not overlap another track; --track_only inputs are cleaned the same way. --pan_component_mode absorb gives such a
component to the segment it shares the longest border with instead (section 4.27), which leaves no hole in that segment's mask.
--video_gt <folder> scores every sequence, once it is tracked and written, against <folder>/<sequence>/gt.json and
<folder>/<sequence>/pan/<frame>.png (VPQ and STQ on the device; upsnet_amd/video_eval.py says how the frames
pair and re-scores written runs); --vpq_windows sets the window lengths (default 1 2 3 4). Then <out>/video_scores.json is written and
the summary logged. Without --video_gt nothing else is written than above.
The MOTS measures (sMOTSA, MOTSA, MOTSP, IDS, Frag, MT / PT / ML) are opt-in: --eval_mots adds them, against
--video_gt, as 'mots' in the summary; --mots_gt <folder> scores them alone against <folder>/<sequence>.txt in the MOTS text format
(frames pair by index) and writes <out>/mots_scores.json; --write_mots writes <out>/<sequence>/mots.txt in that format.
"""
import argparse
import json
import logging
import os

import numpy as np

from .config.config import config, update_config

logger = logging.getLogger(__name__)

IMAGE_EXTENSIONS = ('.png', '.jpg', '.jpeg', '.bmp', '.ppm')


def _frames_in(folder):
    return sorted(os.path.join(folder, f) for f in os.listdir(folder)
                  if f.lower().endswith(IMAGE_EXTENSIONS) and os.path.isfile(os.path.join(folder, f)))


def discover_sequences(folder, option='--frames'):
    """[(sequence name, [frame paths sorted by name])]: the image files directly in `folder` (one sequence, named after the folder),
    then every subfolder in the order of its name. SystemExit naming the folder: a missing folder, an empty subfolder, no sequence."""
    if not os.path.isdir(folder):
        raise SystemExit('%s: no folder at %s' % (option, folder))
    sequences = []
    direct = _frames_in(folder)
    if direct:
        sequences.append((os.path.basename(os.path.abspath(folder)), direct))
    for sub in sorted(d for d in os.listdir(folder) if os.path.isdir(os.path.join(folder, d))):
        frames = _frames_in(os.path.join(folder, sub))
        if not frames:
            raise SystemExit('%s: the sequence folder %s holds no image file' % (option, os.path.join(folder, sub)))
        sequences.append((sub, frames))
    if not sequences:
        raise SystemExit('%s: %s holds no image file and no sequence folder' % (option, folder))
    names = [n for n, _ in sequences]
    if len(set(names)) != len(names):
        raise SystemExit('%s: %s holds frames of its own and a subfolder of its own name; both would be written to one place' % (option, folder))
    return sequences


class FrameSequence(object):
    """The frames of one sequence as the image list evaluate.run_inference and evaluate.panoptic_predictions take."""

    def __init__(self, name, paths):
        from .dataset.base_dataset import BaseDataset
        self.name = name
        self.roidb = [{'id': k, 'image': p, 'file_name': os.path.basename(p)} for k, p in enumerate(paths)]
        self.num_classes = config.dataset.num_classes
        self._base = BaseDataset()

    def __len__(self):
        return len(self.roidb)

    def load_image(self, index):
        from .dataset.json_dataset import imread_bgr
        return imread_bgr(self.roidb[index]['image'])

    def get_unified_pan_result(self, *a, **kw):
        return self._base.get_unified_pan_result(*a, **kw)

    def get_combined_pan_result(self, *a, **kw):
        return self._base.get_combined_pan_result(*a, **kw)

    def clean_pan_result(self, *a, **kw):
        return self._base.clean_pan_result(*a, **kw)


def load_pan_2ch(path):
    from PIL import Image
    im = np.array(Image.open(path))
    if im.dtype != np.uint8 or im.ndim != 3 or im.shape[2] < 3:
        raise SystemExit('--track_only: %s is not a 2-channel panoptic map (an RGB PNG), but %s %s' % (path, im.shape, im.dtype))
    return np.ascontiguousarray(im[:, :, :3])


def track_and_write(tracker, name, pans, file_names, categories, out_dir, vis=None, image_paths=None, score=None):
    """Track one sequence's 2-channel maps and write its files under out_dir; returns (annotations, tracks). score(name, tracked maps,
    file names), if given, is called once everything is written."""
    from .dataset.pan_format import write_panoptic
    from .dataset.pan_vis import vis_panoptic
    tracker.reset()
    tracked, segments = [], []
    for pan in pans:
        out, segs = tracker.update(pan)
        tracked.append(out)
        segments.append(segs)
    images = [{'id': k, 'file_name': f} for k, f in enumerate(file_names)]
    os.makedirs(out_dir, exist_ok=True)
    annotations = write_panoptic(tracked, images, categories, out_dir, stable_ids=True)
    tracks = {}
    for ann, segs in zip(annotations, segments):
        serial = {(s['category'], s['instance']): s['track_id'] for s in segs}
        for seg in ann['segments_info']:
            inst = (seg['id'] >> 8) & 255
            seg['track_id'] = serial.get((seg['category_id'], inst), 0)
        for s in segs:
            t = tracks.setdefault(s['track_id'], {'track_id': s['track_id'], 'category_id': s['category'], 'instance': s['instance'],
                                                  'first_frame': ann['file_name'], 'last_frame': ann['file_name'], 'frames': []})
            t['last_frame'] = ann['file_name']
            t['frames'].append(ann['file_name'])
    with open(os.path.join(out_dir, 'pred.json'), 'w') as f:
        json.dump({'annotations': annotations}, f)
    tracks = [tracks[k] for k in sorted(tracks)]
    with open(os.path.join(out_dir, 'tracks.json'), 'w') as f:
        json.dump({'sequence': name, 'iou_thresh': tracker.iou_thresh, 'max_age': tracker.max_age, 'tracks': tracks}, f)
    for mode in {'flat': ('flat',), 'overlay': ('overlay',), 'both': ('flat', 'overlay')}.get(vis, ()):
        vis_panoptic(tracked, images, categories, out_dir, mode, image_paths=image_paths, stable_ids=True)
    logger.info('sequence %s: %d frames, %d tracks, written to %s', name, len(tracked), len(tracks), os.path.abspath(out_dir))
    if score is not None:
        score(name, tracked, file_names)
    return annotations, tracks


def _exit(message):
    raise SystemExit(message)


def parse_args(argv=None):
    p = argparse.ArgumentParser(description='UPSNet: panoptic segmentation of frame sequences with instances tracked across frames')
    p.add_argument('--cfg', type=str, default='', help='experiment yaml: the network and its test scales')
    p.add_argument('--weight_path', type=str, default='', help='checkpoint to load')
    p.add_argument('--synthetic_weights', action='store_true', help='seeded synthetic weights instead of a checkpoint')
    p.add_argument('--frames', type=str, default='', metavar='FOLDER', help='image files (one sequence) and / or one subfolder per sequence')
    p.add_argument('--track_only', type=str, default='', metavar='FOLDER',
                   help='track written 2-channel maps (pan_2ch PNGs; same folder layout as --frames) without building the model')
    p.add_argument('--out', type=str, default='', metavar='DIR', help='output folder; one subfolder per sequence')
    p.add_argument('--panoptic_categories', type=str, default='', metavar='JSON', help="a panoptic JSON whose 'categories' to use")
    p.add_argument('--track_iou', type=float, default=0.3, metavar='T', help='mask IoU from which a segment may continue a track, in [1/16, 1]')
    p.add_argument('--track_max_age', type=int, default=0, metavar='N', help='frames a track may be missing and still be re-acquired')
    p.add_argument('--track_motion', choices=('none', 'constant_velocity'), default='none',
                   help='constant_velocity: predict every track from its velocity before associating (for persistent motion)')
    p.add_argument('--combined', action='store_true', help='track get_combined_pan_result (detections + semantic map) instead of the panoptic head')
    p.add_argument('--vis_panoptic', choices=('flat', 'overlay', 'both'), default=None, help='also draw the tracked maps')
    p.add_argument('--in-flight', type=int, default=1, help='images in flight (1 = the reference loop)')
    from .config.parse_args import add_pan_component_arguments
    add_pan_component_arguments(p, 'tracked; also on --track_only inputs')
    from .video_eval import add_arguments, check_arguments
    add_arguments(p)
    return check_arguments(p, p.parse_args(argv))


def main(argv=None):
    """Returns {'sequences': [(name, output folder, annotations, tracks)]}, with --video_gt also 'video_scores': the summary, with
    --mots_gt also 'mots_scores'."""
    args = parse_args(argv)
    logging.basicConfig(level=logging.INFO, format='%(asctime)-15s | %(message)s')
    world = int(os.environ.get('WORLD_SIZE', '1'))
    if world > 1:
        raise SystemExit('upsnet_amd.sequence runs on one rank; WORLD_SIZE=%d is refused' % world)
    if not args.cfg:
        raise SystemExit('--cfg <experiment yaml> is required: it names the network and its test scales')
    if bool(args.frames) == bool(args.track_only):
        raise SystemExit('give exactly one of --frames <folder> (run the network) and --track_only <folder of pan_2ch PNGs>')
    if not args.out:
        raise SystemExit('--out <dir> is required')
    if not args.panoptic_categories or not os.path.isfile(args.panoptic_categories):
        raise SystemExit("--panoptic_categories: no panoptic JSON at %r (its 'categories' name and colour the segments)" % args.panoptic_categories)
    from .dataset.pan_track import PanopticTracker, check_params
    try:
        check_params(args.track_iou, args.track_max_age, args.track_motion)
    except ValueError as e:
        raise SystemExit('--track_iou / --track_max_age / --track_motion: %s' % e)
    update_config(args.cfg)
    from .config.parse_args import apply_pan_component_arguments
    apply_pan_component_arguments(args, _exit)
    net = config.network
    if args.track_only:
        if args.weight_path or args.synthetic_weights or args.combined:
            raise SystemExit('--track_only builds no model: --weight_path, --synthetic_weights and --combined do not go with it')
        if args.vis_panoptic in ('overlay', 'both'):
            raise SystemExit("--track_only has no photographs to draw over: of --vis_panoptic only 'flat' goes with it")
    else:
        if bool(args.weight_path) == bool(args.synthetic_weights):
            raise SystemExit('give exactly one of --weight_path <pth> and --synthetic_weights')
        if args.combined and not (net.has_rcnn and net.has_mask_head and net.has_fcn_head):
            raise SystemExit('--combined merges detections, instance masks and the semantic map: it needs network.has_rcnn, '
                             'has_mask_head and has_fcn_head (has_rcnn=%s, has_mask_head=%s, has_fcn_head=%s)'
                             % (net.has_rcnn, net.has_mask_head, net.has_fcn_head))
        if not args.combined and not net.has_panoptic_head:
            raise SystemExit('the tracked maps come from the panoptic head: it needs network.has_panoptic_head, or --combined '
                             '(has_panoptic_head=%s)' % net.has_panoptic_head)
    sequences = discover_sequences(args.frames or args.track_only, '--frames' if args.frames else '--track_only')
    with open(args.panoptic_categories, 'r') as f:
        categories = json.load(f)['categories']
    tracker = PanopticTracker(iou_thresh=args.track_iou, max_age=args.track_max_age, motion=args.track_motion)
    done = []
    score, finish = None, lambda res: res
    if args.video_gt or args.mots_gt or args.write_mots:
        from . import video_eval
        scoring = video_eval.Scoring(args, categories)

        def score(name, tracked, file_names):
            scoring.add(name, tracked, file_names, os.path.join(args.out, name))

        def finish(res):
            return scoring.finish(res, args.out)
    if args.track_only:
        for name, paths in sequences:
            pans = [load_pan_2ch(p) for p in paths]
            if config.test.get('pan_min_component', 0) > 0:
                from .dataset.base_dataset import BaseDataset
                pans = BaseDataset().clean_pan_result(pans, what='sequence %s' % name)
            out_dir = os.path.join(args.out, name)
            done.append((name, out_dir) + track_and_write(tracker, name, pans, [os.path.basename(p) for p in paths], categories, out_dir,
                                                          vis=args.vis_panoptic, score=score))
        return finish({'sequences': done})
    from .evaluate import panoptic_predictions, run_inference
    from .upsnet_end2end_test import init_distributed, load_checkpoint_model
    _, _, device = init_distributed()
    if args.synthetic_weights:
        from .synthetic import build_model
        logging.warning('seeded SYNTHETIC weights (upsnet_amd.synthetic, seed 235): the maps are not those of a trained model')
        model = build_model(device=device)
    else:
        model = load_checkpoint_model(args.weight_path, device)
    for name, paths in sequences:
        seq = FrameSequence(name, paths)
        results, _ = run_inference(model, seq, in_flight=args.in_flight, device=device)
        pans = panoptic_predictions(seq, results, args.combined)
        out_dir = os.path.join(args.out, name)
        done.append((name, out_dir) + track_and_write(tracker, name, pans, [e['file_name'] for e in seq.roidb], categories, out_dir,
                                                      vis=args.vis_panoptic, image_paths=paths, score=score))
    return finish({'sequences': done})


if __name__ == '__main__':
    main()
