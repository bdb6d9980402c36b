"""The evaluation ground truth from the raw dataset downloads: every derived file the dataset classes read,
made from a plain Cityscapes gtFine + leftImg8bit tree or a plain COCO panoptic annotation download.

    python -m upsnet_amd.prepare --dataset cityscapes --root <dir> [--splits val ...] [--images link|copy|none] [--force]
    python -m upsnet_amd.prepare --dataset coco --root <dir> [--splits val2017 ...] [--force]

Cityscapes. The reference downloads its annotation files from its author's site (init_cityscapes.sh) and takes the labelTrainIds maps
from the Cityscapes devkit; neither is available offline, so the rules of the devkit's createTrainIdLabelImgs / createPanopticImgs
and of Detectron's convert_cityscapes_to_coco are restated here (unpinned: no build of them is at hand). The per-pixel work of an
image runs on the device (csrc/gt_prepare.hip, dataset/gt_prepare.py). With v a raw value of <base>_gtFine_instanceIds.png,
label = v if v < 1000 else v // 1000:
  * labels/<base>_gtFine_labelTrainIds.png: the label's train id, 255 for the labels ignored in evaluation;
  * panoptic/<base>_gtFine_panoptic.png: (v % 256, v // 256 % 256, v // 65536), (0, 0, 0) where the label is ignored;
  * annotations/cityscapes_fine_<split>.json, COCO panoptic format: one segment per distinct v whose label is not ignored, ascending:
    id = v, category_id = train id, area, bbox [x, y, w, h], iscrowd = 1 exactly when v < 1000 and the label has instances (a group);
    the 19 categories carry name, colour, supercategory (the label's category) and isthing;
  * annotations/instancesonly_gtFine_<split>.json: one annotation per v >= 1000 of the eight classes of CLASS_NAMES (groups, caravan
    and trailer are none), ascending v per image: category_id 1..8 in CLASS_NAMES order, iscrowd 0, area = pixel count, bbox
    [x_min, y_min, x_max - x_min + 1, y_max - y_min + 1] as floats, segmentation = the mask's compressed COCO RLE;
  * images/<base>_leftImg8bit.png, linked or copied from leftImg8bit/;
  * a split without gtFine (test): annotations/image_info_<split>.json, the image list alone, from leftImg8bit.
Files are handled in sorted base-name order, which defines the integer image ids 1..N of a split.

Deliberate deviations. The panoptic JSON's image_id is that integer id (the devkit writes the base name), so that predictions are
paired with annotations by id (json_dataset.panoptic_pairing). Detectron writes contour polygons, which lose holes; here the
segmentation is the exact RLE, which DetectionEvaluator takes for non-crowd ground truth.

COCO. panoptic_coco_categories_stff.json and panoptic_<split>_stff.json by the remap of the reference's init_coco.py (stuff becomes
0..52, things 53..132 by their position in the category list, 'jpg' -> 'png' in file names, val images sorted by id; the category
table is the JSON's own 'categories'), pinned to the reference by tests/golden/coco_stff.json; and
annotations/panoptic_<split>_semantic_trainid_stff/*.png, every pixel the remapped category of its segment (crowds included), 255
for id 0 and ids without a segment (panopticapi's panoptic-to-semantic converter, restated; gt_prepare.panoptic_semantic).

Nothing in the download folders is written. Existing outputs are refused (FileExistsError naming the first) unless force is set;
all file checks come before the first launch.
"""
import argparse
import copy
import glob
import json
import logging
import os
import shutil
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from .cityscapes_eval import CLASS_LABEL_IDS, CLASS_NAMES
from .cityscapes_pixel_eval import LABELS, TRAIN_ID_COLOURS, TRAIN_TO_LABEL_ID
from .rle import counts_from_transitions, rle_to_string

logger = logging.getLogger(__name__)

MAX_ENCODE_THREADS = 8          # PNG encoder threads (never sized from the host's CPU count)
FIRST_INSTANCE_LABEL = 24       # hasInstances = label id >= 24 (dataset/cityscapes_pixel_eval.py)
ROW = 9                         # v, label, train id, iscrowd, area, x_min, y_min, x_max, y_max
NUM_STUFF, NUM_THINGS = 53, 80  # COCO panoptic


# ------------------------------------------------------------------------------------------------ tables and JSON writers (host only)
def label_tables():
    """int32 [3, 256] for the kernel: per label id the train id (255 = ignored in evaluation), hasInstances, and the row 0..7 of its
    thing class or -1."""
    t = np.zeros((3, 256), np.int32)
    t[0] = 255
    t[2] = -1
    for train_id, label in enumerate(TRAIN_TO_LABEL_ID):
        t[0, label] = train_id
    t[1, FIRST_INSTANCE_LABEL:len(LABELS)] = 1
    for row, label in enumerate(CLASS_LABEL_IDS):
        t[2, label] = row
    return t


def panoptic_categories():
    """The 19 categories of the Cityscapes panoptic JSON, ids = train ids."""
    things = set(CLASS_LABEL_IDS)
    return [{'id': t, 'name': LABELS[label][0], 'color': list(TRAIN_ID_COLOURS[t]), 'supercategory': LABELS[label][1],
             'isthing': int(label in things)} for t, label in enumerate(TRAIN_TO_LABEL_ID)]


def instance_categories():
    return [{'id': i + 1, 'name': name} for i, name in enumerate(CLASS_NAMES)]


def panoptic_segments(rows):
    """Segment rows (int [n, 9]) -> the segments_info of the panoptic JSON, in the rows' order (ascending v)."""
    return [{'id': r[0], 'category_id': r[2], 'area': r[4], 'bbox': [r[5], r[6], r[7] - r[5] + 1, r[8] - r[6] + 1], 'iscrowd': r[3]}
            for r in np.asarray(rows).reshape(-1, ROW).tolist()]


def instance_rows(rows):
    """The rows of the instances (v >= 1000 of a thing class), in order: the lists of trans_off follow them."""
    thing = label_tables()[2]
    return [r for r in np.asarray(rows).reshape(-1, ROW).tolist() if r[0] >= 1000 and thing[r[1]] >= 0]


def instance_annotations(image_id, rows, trans_off, trans, height, width, first_id):
    """The instances JSON's annotations of one image from its segment rows and run lists; ids from first_id."""
    thing = label_tables()[2]
    inst = instance_rows(rows)
    trans_off, trans = np.asarray(trans_off, np.int64), np.asarray(trans, np.int64)
    if len(trans_off) != len(inst) + 1:
        raise ValueError("%d run lists for %d instances" % (len(trans_off) - 1, len(inst)))
    anns = []
    for j, r in enumerate(inst):
        counts = counts_from_transitions(trans[trans_off[j]:trans_off[j + 1]], height * width)
        anns.append({'id': first_id + j, 'image_id': image_id, 'category_id': int(thing[r[1]]) + 1, 'iscrowd': 0, 'area': r[4],
                     'bbox': [float(r[5]), float(r[6]), float(r[7] - r[5] + 1), float(r[8] - r[6] + 1)],
                     'segmentation': {'size': [height, width], 'counts': rle_to_string(counts)}})
    return anns


def read_id_map(path):
    """A gtFine_instanceIds PNG as int32 [H, W], read as Cityscapes.load_instance_gt reads it (PIL mode I;16)."""
    from PIL import Image
    try:
        with Image.open(path) as im:
            if im.mode not in ('I;16', 'I;16L', 'I;16B', 'I', 'L'):
                raise ValueError('mode %s, not a 16-bit id map' % im.mode)
            gt = np.asarray(im)
    except (OSError, ValueError) as e:
        raise ValueError('cannot read the instance-id map %s: %s' % (path, e))
    if gt.ndim != 2 or gt.min() < 0 or gt.max() > 65535:
        raise ValueError('%s is not a 16-bit id map' % path)
    return np.ascontiguousarray(gt.astype(np.int32))


def _read_label_map(path, shape):
    from PIL import Image
    with Image.open(path) as im:
        if im.mode not in ('L', 'P'):
            raise ValueError('%s: mode %s, not an 8-bit label map' % (path, im.mode))
        gt = np.asarray(im)
    if gt.shape != shape:
        raise ValueError('%s is %s, its instance-id map %s' % (path, gt.shape, shape))
    return np.ascontiguousarray(gt.astype(np.uint8))


def _save_png(array, path):
    from PIL import Image
    Image.fromarray(array).save(path)


def _refuse_existing(paths, force):
    if force:
        return
    for p in paths:
        if os.path.lexists(p):
            raise FileExistsError('%s exists already (pass force / --force to overwrite)' % p)


def _place_image(src, dst, mode):
    if os.path.lexists(dst):
        os.remove(dst)
    if mode == 'link':
        os.symlink(os.path.abspath(src), dst)
    else:
        shutil.copyfile(src, dst)


# ------------------------------------------------------------------------------------------------ Cityscapes
class _Pending(object):
    __slots__ = ('name', 'shape', 'dev', 'host', 'event', 'args')


class CityscapesPreparer(object):
    """Id maps -> (train-id map, panoptic RGB, segment rows, trans_off, trans) on one device. submit() queues an image on the current
    stream and starts the copy of both maps and the status words into pinned memory without synchronising; finish() waits for that
    copy (the one host read of the image's counts), then fetches the rows and run lists at their counted sizes with three blocking
    copies on the same stream: by then the next image is queued there, so they wait for its launches, and what overlaps the device is
    the PNG encoding, not these copies. The transition buffer has a default size; an image that outgrows it is run again at the size
    its counting pass reported (gt_prepare.gt_prepare_regrow)."""

    def __init__(self, device=None, seg_capacity=None):
        import torch
        from . import gt_prepare as ops
        self.device = torch.device(device) if device is not None else torch.device('cuda', torch.cuda.current_device())
        self.seg_capacity = int(seg_capacity or ops.GT_PREPARE_SEGMENTS)
        self.tables = torch.from_numpy(label_tables()).to(self.device)
        self.workspace = ops.gt_prepare_workspace(self.device, self.seg_capacity)

    def submit(self, ids, label_ids=None, name='image'):
        import torch
        from . import gt_prepare as ops
        H, W = ids.shape
        args = (torch.from_numpy(ids).pin_memory().to(self.device, non_blocking=True),
                None if label_ids is None else torch.from_numpy(label_ids).pin_memory().to(self.device, non_blocking=True))
        p = _Pending()
        p.name, p.shape, p.args = name, (H, W), args
        p.dev = ops.gt_prepare_launch(args[0], self.tables, args[1], self.seg_capacity, None, self.workspace)
        train_map, rgb, _, _, _, status = p.dev
        p.host = (torch.empty((H, W), dtype=torch.uint8, pin_memory=True), torch.empty((H, W, 3), dtype=torch.uint8, pin_memory=True),
                  torch.empty((ops.GT_STATUS,), dtype=torch.int32, pin_memory=True))
        for h, d in zip(p.host, (train_map, rgb, status)):
            h.copy_(d, non_blocking=True)
        p.event = torch.cuda.Event()
        p.event.record()
        return p

    def finish(self, p):
        """-> (train_map uint8 [H,W], rgb uint8 [H,W,3], rows int32 [n,9], trans_off int32 [m+1], trans int32 [t]) as numpy arrays."""
        from . import gt_prepare as ops
        p.event.synchronize()
        out, status = ops.gt_prepare_regrow(p.dev, p.host[2].numpy(), p.args[0], self.tables, self.seg_capacity, self.workspace)
        _, _, table, trans_off, trans, _ = out
        n_seg, n_inst, n_trans = ops.gt_prepare_check(status, self.seg_capacity, int(trans.shape[0]), p.name)
        return (p.host[0].numpy(), p.host[1].numpy(), table[:n_seg].cpu().numpy(), trans_off[:n_inst + 1].cpu().numpy(),
                trans[:n_trans].cpu().numpy())


def _split_files(root, split):
    """(bases, {base: instanceIds path}) of gtFine/<split>, or (bases, None) from leftImg8bit/<split> when the split has no gtFine."""
    suffix = '_gtFine_instanceIds.png'
    found = glob.glob(os.path.join(root, 'gtFine', split, '*', '*' + suffix))
    if found:
        by_base = {os.path.basename(p)[:-len(suffix)]: p for p in found}
        if len(by_base) != len(found):
            raise ValueError('gtFine/%s holds two files of one base name' % split)
        return sorted(by_base), by_base
    suffix = '_leftImg8bit.png'
    found = glob.glob(os.path.join(root, 'leftImg8bit', split, '*', '*' + suffix))
    if not found:
        raise FileNotFoundError('no *_gtFine_instanceIds.png under %s and no *_leftImg8bit.png under %s'
                                % (os.path.join(root, 'gtFine', split), os.path.join(root, 'leftImg8bit', split)))
    return sorted(os.path.basename(p)[:-len(suffix)] for p in found), None


def _source_image(root, split, base):
    return os.path.join(root, 'leftImg8bit', split, base.split('_')[0], base + '_leftImg8bit.png')


def prepare_cityscapes(root, splits=('val',), images='link', device=None, force=False):
    """Write labels/, panoptic/, images/ and the annotation JSONs of the given splits under `root` (module docstring). Returns
    {split: number of images}. FileNotFoundError naming a missing leftImg8bit image, FileExistsError naming the first existing
    output unless `force`; both before any launch."""
    if images not in ('link', 'copy', 'none'):
        raise ValueError("images must be 'link', 'copy' or 'none', got %r" % (images,))
    if isinstance(splits, str):
        splits = [splits]
    plan = []
    for split in splits:
        bases, id_files = _split_files(root, split)
        outputs = []
        if id_files is None:
            outputs.append(os.path.join(root, 'annotations', 'image_info_%s.json' % split))
        else:
            outputs += [os.path.join(root, 'annotations', n % split) for n in ('instancesonly_gtFine_%s.json', 'cityscapes_fine_%s.json')]
            outputs += [os.path.join(root, 'labels', b + '_gtFine_labelTrainIds.png') for b in bases]
            outputs += [os.path.join(root, 'panoptic', b + '_gtFine_panoptic.png') for b in bases]
        if images != 'none':
            for b in bases:
                if not os.path.isfile(_source_image(root, split, b)):
                    raise FileNotFoundError('file not found: %s' % _source_image(root, split, b))
            outputs += [os.path.join(root, 'images', b + '_leftImg8bit.png') for b in bases]
        _refuse_existing(outputs, force)
        plan.append((split, bases, id_files))
    done = {}
    for split, bases, id_files in plan:
        for sub in ('annotations', 'images') if id_files is None else ('annotations', 'images', 'labels', 'panoptic'):
            if sub != 'images' or images != 'none':
                os.makedirs(os.path.join(root, sub), exist_ok=True)
        if id_files is None:
            _write_image_info(root, split, bases)
        else:
            _prepare_split(root, split, bases, id_files, device)
        if images != 'none':
            for b in bases:
                _place_image(_source_image(root, split, b), os.path.join(root, 'images', b + '_leftImg8bit.png'), images)
        logger.info('cityscapes %s: %d images prepared under %s', split, len(bases), os.path.abspath(root))
        done[split] = len(bases)
    return done


def _write_image_info(root, split, bases):
    from PIL import Image
    imgs = []
    for k, b in enumerate(bases):
        with Image.open(_source_image(root, split, b)) as im:
            w, h = im.size
        imgs.append({'id': k + 1, 'file_name': b + '_leftImg8bit.png', 'height': h, 'width': w})
    with open(os.path.join(root, 'annotations', 'image_info_%s.json' % split), 'w') as f:
        json.dump({'images': imgs, 'categories': instance_categories()}, f)


def _prepare_split(root, split, bases, id_files, device):
    prep = CityscapesPreparer(device)
    inst_images, inst_anns, pan_images, pan_anns = [], [], [], []
    workers = max(1, min(MAX_ENCODE_THREADS, len(bases)))
    with ThreadPoolExecutor(max_workers=workers) as pool:
        jobs = []

        def retire(p, k):
            base, image_id = bases[k], k + 1
            train_map, rgb, rows, trans_off, trans = prep.finish(p)
            H, W = p.shape
            pan_name = base + '_gtFine_panoptic.png'
            jobs.append(pool.submit(_save_png, train_map, os.path.join(root, 'labels', base + '_gtFine_labelTrainIds.png')))
            jobs.append(pool.submit(_save_png, rgb, os.path.join(root, 'panoptic', pan_name)))
            while len(jobs) > 4 * workers:          # bounds the pinned buffers waiting for an encoder
                jobs.pop(0).result()
            inst_images.append({'id': image_id, 'file_name': base + '_leftImg8bit.png', 'height': H, 'width': W,
                                'seg_file_name': os.path.basename(id_files[base])})
            inst_anns.extend(instance_annotations(image_id, rows, trans_off, trans, H, W, len(inst_anns) + 1))
            pan_images.append({'id': image_id, 'file_name': pan_name, 'height': H, 'width': W})
            pan_anns.append({'image_id': image_id, 'file_name': pan_name, 'segments_info': panoptic_segments(rows)})

        pending = None
        for k, base in enumerate(bases):
            ids = read_id_map(id_files[base])
            label_path = id_files[base][:-len('instanceIds.png')] + 'labelIds.png'
            labels = _read_label_map(label_path, ids.shape) if os.path.isfile(label_path) else None
            p = prep.submit(ids, labels, name=os.path.basename(id_files[base]))   # image k is on the device while k - 1 is encoded
            if pending is not None:
                retire(*pending)
            pending = (p, k)
        if pending is not None:
            retire(*pending)
        for job in jobs:
            job.result()
    with open(os.path.join(root, 'annotations', 'instancesonly_gtFine_%s.json' % split), 'w') as f:
        json.dump({'images': inst_images, 'annotations': inst_anns, 'categories': instance_categories()}, f)
    with open(os.path.join(root, 'annotations', 'cityscapes_fine_%s.json' % split), 'w') as f:
        json.dump({'images': pan_images, 'annotations': pan_anns, 'categories': panoptic_categories()}, f)


# ------------------------------------------------------------------------------------------------ COCO
def coco_stff_remap(pano_json, sort_images):
    """(categories_stff, panoptic JSON with them) by the remap of the reference's init_coco.py: with the 133 categories in the
    download's order (80 things, then 53 stuff), the stuff category at position 80 + k becomes id k and the thing category at position
    k becomes id 53 + k; every segment's category_id follows; 'jpg' -> 'png' in the images' file names; images sorted by id when
    sort_images (the reference sorts val only). The input is not modified."""
    cats = pano_json['categories']
    n = NUM_STUFF + NUM_THINGS
    if len(cats) != n or any(c['isthing'] != 1 for c in cats[:NUM_THINGS]) or any(c['isthing'] != 0 for c in cats[NUM_THINGS:]):
        raise ValueError("the panoptic JSON's categories must be COCO's 80 things followed by its 53 stuff classes, got %d" % len(cats))
    position = {c['id']: i for i, c in enumerate(cats)}
    if len(position) != n:
        raise ValueError("the panoptic JSON's category ids are not unique")
    new_id = lambda pos: pos + NUM_STUFF if pos < NUM_THINGS else pos - NUM_THINGS      # noqa: E731
    cats_stff = [None] * n
    for pos, c in enumerate(cats):
        cats_stff[new_id(pos)] = dict(copy.deepcopy(c), id=new_id(pos))
    out = copy.deepcopy(pano_json)
    out['categories'] = cats_stff
    for ann in out['annotations']:
        for seg in ann['segments_info']:
            seg['category_id'] = new_id(position[seg['category_id']])
    for img in out['images']:
        img['file_name'] = img['file_name'].replace('jpg', 'png')
    if sort_images:
        out['images'] = sorted(out['images'], key=lambda x: x['id'])
    return cats_stff, out


def prepare_coco(root, split='val2017', device=None, force=False):
    """Write annotations/panoptic_coco_categories_stff.json, annotations/panoptic_<split>_stff.json and
    annotations/panoptic_<split>_semantic_trainid_stff/*.png from annotations/panoptic_<split>.json and its PNG folder (module
    docstring). Returns the number of images."""
    ann_dir = os.path.join(root, 'annotations')
    src_json, src_dir = os.path.join(ann_dir, 'panoptic_%s.json' % split), os.path.join(ann_dir, 'panoptic_%s' % split)
    if not os.path.isfile(src_json):
        raise FileNotFoundError('file not found: %s' % src_json)
    with open(src_json, 'r') as f:
        pano = json.load(f)
    cats_stff, stff = coco_stff_remap(pano, sort_images=split.startswith('val'))
    sem_dir = os.path.join(ann_dir, 'panoptic_%s_semantic_trainid_stff' % split)
    cat_file, stff_file = os.path.join(ann_dir, 'panoptic_coco_categories_stff.json'), os.path.join(ann_dir, 'panoptic_%s_stff.json' % split)
    for ann in stff['annotations']:
        if not os.path.isfile(os.path.join(src_dir, ann['file_name'])):
            raise FileNotFoundError('file not found: %s' % os.path.join(src_dir, ann['file_name']))
    same_cats = False                  # (the category file is shared by the splits: one that holds the same table is not in the way)
    if os.path.isfile(cat_file):
        with open(cat_file, 'r') as f:
            same_cats = f.read() == json.dumps(cats_stff)
    _refuse_existing(([] if same_cats else [cat_file]) + [stff_file] + [os.path.join(sem_dir, a['file_name']) for a in stff['annotations']],
                     force)
    import torch
    from . import gt_prepare as ops
    from .base_dataset import load_panoptic_png
    dev = torch.device(device) if device is not None else torch.device('cuda', torch.cuda.current_device())
    os.makedirs(sem_dir, exist_ok=True)
    workers = max(1, min(MAX_ENCODE_THREADS, len(stff['annotations'])))
    with ThreadPoolExecutor(max_workers=workers) as pool:
        jobs = []
        for ann in stff['annotations']:
            rgb = torch.from_numpy(load_panoptic_png(os.path.join(src_dir, ann['file_name']))).to(dev)
            sem = ops.panoptic_semantic(rgb, ann['segments_info']).cpu().numpy()
            jobs.append(pool.submit(_save_png, sem, os.path.join(sem_dir, ann['file_name'])))
            while len(jobs) > 4 * workers:
                jobs.pop(0).result()
        for job in jobs:
            job.result()
    with open(cat_file, 'w') as f:
        json.dump(cats_stff, f)
    with open(stff_file, 'w') as f:
        json.dump(stff, f)
    logger.info('coco %s: %d images prepared under %s', split, len(stff['annotations']), os.path.abspath(root))
    return len(stff['annotations'])


# ------------------------------------------------------------------------------------------------ command line
def main(argv=None):
    ap = argparse.ArgumentParser(prog='python -m upsnet_amd.prepare', description='Build the evaluation ground truth from a raw '
                                 'Cityscapes (gtFine + leftImg8bit) or COCO panoptic download. The download folders are only read.')
    ap.add_argument('--dataset', required=True, choices=['cityscapes', 'coco'])
    ap.add_argument('--root', required=True, help='the dataset directory (config.dataset.dataset_path)')
    ap.add_argument('--splits', nargs='+', default=None, help='default: val (cityscapes), val2017 (coco)')
    ap.add_argument('--images', choices=['link', 'copy', 'none'], default='link', help='cityscapes: how images/ is filled')
    ap.add_argument('--force', action='store_true', help='overwrite existing outputs')
    args = ap.parse_args(argv)
    if args.dataset == 'cityscapes':
        return prepare_cityscapes(args.root, tuple(args.splits or ('val',)), images=args.images, force=args.force)
    return {s: prepare_coco(args.root, s, force=args.force) for s in (args.splits or ('val2017',))}
