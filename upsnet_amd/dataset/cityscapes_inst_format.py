"""Cityscapes instance-level predictions in the benchmark's file format, both directions (csrc/cs_inst_format.hip; DESIGN.md section
4.16).

Writing: the files of the reference's Cityscapes.evaluate_masks (upsnet/dataset/cityscapes.py:368-395), which are the devkit's input
and the only thing the benchmark server takes for the instance-level task. Per image <basename> = the image's file name without its
extension:
    <output_dir>/inst_seg/<basename>pred.txt                                       (no separator before 'pred', as in the reference)
    <output_dir>/inst_seg/seg_results/<basename>/<basename>_<class name>_<k>.png   one mask per detection k of a class
One line of the txt per detection, classes 1..8 in order and detections in their stored order: '<png path relative to the txt, forward
slashes> <label id> <score>\\n', the score as str(np.float32(score)) (the shortest text that reads back to the same float32: what the
reference's '{}'.format prints). An image without detections has an empty txt. The masks are 8-bit grey PNGs of 0 / 255 (the
reference's cv2.imwrite(mask * 255)) or, with one_bit, PNGs of bit depth 1. `expand_masks` turns the column-major run lists of im_post's
RLEs into the row-major planes on the device; `write_instance_predictions` encodes the PNGs of image i on host threads while image
i + 1 is on the device. No ground truth is read: the test split can be written.

Reading: the rules of the devkit's evalInstanceLevelSemanticLabeling for its prediction files, restated (the devkit is not part of
the reference tree; never compared with a devkit build):
  * the prediction file of the image <city>_<sequence>_<frame>_leftImg8bit.png is the one file anywhere under the folder whose name
    matches <city>_<sequence>_<frame>*.txt; none or several is an error;
  * every non-empty line has exactly three fields separated by single spaces: mask path, integer label id, float confidence;
  * the mask path is relative, is resolved against the txt file's directory, must stay inside the folder and must exist (checked for
    every line, also one the next rule skips);
  * a line whose label id is not one of the eight instance classes is skipped (the devkit's `if not labelName in args.instLabels:
    continue`); a label id that is no Cityscapes label (outside -1..33) is an error;
  * a mask is opened with PIL and converted with .convert('L') (the devkit's call: palette PNGs go through their palette's luma, RGB
    through ITU-R 601 luma, bit depth 1 becomes 0 / 255); a pixel is inside when the result is non-zero; a mask of another size than
    the image is an error.
Deviations: the confidence is rounded to float32 (the evaluator keeps float32 scores; a file written here round-trips exactly, a third
party's double-precision scores can only change by becoming tied); a NaN confidence is an error; those of
dataset/cityscapes_eval.py apply to the scoring.
"""
import fnmatch
import logging
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from .._lib import aligned, check, dense, i32c, lib, ptr, stream, written
from .cityscapes_eval import CLASS_LABEL_IDS, CLASS_NAMES, MAX_PREDS, NUM_CLASSES, _transitions
from .pan_format import MAX_ENCODE_THREADS

logger = logging.getLogger(__name__)

MAX_LAUNCH_BYTES = 256 << 20      # output of one expand launch, and of one staging copy (at least one mask whatever its size)
MAX_PIXELS = 1 << 30
LABEL_ID_RANGE = (-1, 33)         # the ids of the Cityscapes label table


def plane_bytes(H, W, one_bit):
    return H * ((W + 7) // 8) if one_bit else H * W


def _host_array(x, name):
    """A run-list argument as a contiguous int32 numpy array (a device tensor is copied back to be checked)."""
    if isinstance(x, torch.Tensor):
        if x.dtype != torch.int32 or x.dim() != 1:
            raise ValueError("%s must be int32 [k], got %s %s" % (name, tuple(x.shape), x.dtype))
        return x.detach().cpu().numpy()
    if not isinstance(x, np.ndarray) or x.dtype != np.int32 or x.ndim != 1:
        raise ValueError("%s must be an int32 [k] numpy array or tensor, got %r %s" % (name, type(x), getattr(x, 'dtype', None)))
    return np.ascontiguousarray(x)


def check_runs(trans, off, H, W):
    """ValueError unless (trans, off) are run lists of H x W masks as the device op takes them; returns the mask count."""
    if not all(isinstance(v, (int, np.integer)) for v in (H, W)):
        raise ValueError("H and W must be integers, got %r, %r" % (H, W))
    if H <= 0 or W <= 0 or H * W > MAX_PIXELS:
        raise ValueError("masks of %d x %d: H * W must be in 1..2^30" % (H, W))
    if off.size < 1 or int(off[0]) != 0 or int(off[-1]) != trans.size or np.any(np.diff(off) < 0):
        raise ValueError("off must rise from 0 to len(trans) = %d, got %s" % (trans.size, off[:8].tolist()))
    if trans.size:
        if int(trans.min()) < 0 or int(trans.max()) >= H * W:
            raise ValueError("transitions must lie in [0, %d x %d)" % (H, W))
        falls = np.diff(trans) < 0
        starts = off[1:-1]
        falls[starts[(starts > 0) & (starts < trans.size)] - 1] = False      # (a new mask may start lower)
        if np.any(falls):
            raise ValueError("transitions must not decrease within a mask (entry %d)" % (int(np.flatnonzero(falls)[0]) + 1))
    return int(off.size - 1)


def _expand_into(d_trans, d_off, n, H, W, one_bit, out, max_bytes):
    """The launches of n checked masks: chunks of whole masks whose output stays within max_bytes (one mask at least)."""
    per = plane_bytes(H, W, one_bit)
    step = max(1, int(max_bytes) // per)
    d_trans, d_off = i32c(d_trans), i32c(d_off)
    flat = written(out, torch.uint8, "expand_masks: out").view(-1)
    for m0 in range(0, n, step):
        nm = min(step, n - m0)
        # a chunk's offsets and planes start wherever the chunk does: the offsets are read from an aligned copy, and a chunk of planes
        # that starts off 16 bytes (H * W or the bit rows need not be a multiple of 16) is expanded into a buffer of its own and copied
        off = aligned(d_off[m0:m0 + nm + 1])
        dst = flat[m0 * per:(m0 + nm) * per]
        planes = aligned(dst)
        check(lib().upsnet_cs_inst_expand(stream(), ptr(d_trans), ptr(off), nm, H, W, 1 if one_bit else 8, ptr(planes)), "cs_inst_expand")
        if planes is not dst:
            dst.copy_(planes)


def expand_masks(trans, off, H, W, one_bit=False, out=None, max_bytes=None):
    """Run lists -> mask planes on the device. trans int32: the column-major change positions of all masks concatenated, the final
    H * W dropped (cityscapes_eval._transitions); off int32 [n + 1]: where each mask's list starts; numpy arrays (uploaded) or device
    tensors (copied back to be checked, used where they are). Returns uint8 [n, H, W] of 0 / 255, or with one_bit uint8
    [n, H, ceil(W / 8)] in the row layout of a PNG of bit depth 1 (leftmost pixel in the most significant bit, rows padded with zero
    bits); `out`: a contiguous device tensor of that shape to fill instead. max_bytes: the output bytes of one launch (default
    MAX_LAUNCH_BYTES; the tests lower it). ValueError before any launch for anything else; no host synchronisation after the checks."""
    t_np, o_np = _host_array(trans, 'trans'), _host_array(off, 'off')
    n = check_runs(t_np, o_np, H, W)
    H, W = int(H), int(W)
    shape = (n, H, (W + 7) // 8 if one_bit else W)
    max_bytes = MAX_LAUNCH_BYTES if max_bytes is None else int(max_bytes)
    if max_bytes < 1:
        raise ValueError("max_bytes must be positive, got %d" % max_bytes)
    if out is not None:
        if not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or tuple(out.shape) != shape or not out.is_contiguous():
            raise ValueError("out must be a contiguous uint8 tensor of shape %s, got %s %s" % (shape, tuple(getattr(out, 'shape', ())),
                                                                                               getattr(out, 'dtype', None)))
        if not out.is_cuda:
            raise ValueError("out must be on the device")
    devs = [x.device for x in (trans, off, out) if isinstance(x, torch.Tensor) and x.is_cuda]
    if any(isinstance(x, torch.Tensor) and not x.is_cuda for x in (trans, off)):
        raise ValueError("trans and off must be numpy arrays or device tensors")
    if any(d != devs[0] for d in devs):
        raise ValueError("trans, off and out are on different devices")
    dev = devs[0] if devs else torch.device('cuda', torch.cuda.current_device())
    with torch.cuda.device(dev):
        if out is None:
            out = torch.empty(shape, dtype=torch.uint8, device=dev)
        if n == 0:
            return out
        d_trans = dense(trans) if isinstance(trans, torch.Tensor) else torch.from_numpy(t_np).to(dev)
        d_off = dense(off) if isinstance(off, torch.Tensor) else torch.from_numpy(o_np).to(dev)
        if d_trans.numel() == 0:
            d_trans = torch.zeros((1,), dtype=torch.int32, device=dev)       # never empty (a valid address)
        _expand_into(d_trans, d_off, n, H, W, one_bit, out, max_bytes)
    return out


# ------------------------------------------------------------------------------------------------------------------ writer
def image_basename(entry):
    return os.path.splitext(os.path.basename(entry['image']))[0]


def pred_txt_name(entry):
    return image_basename(entry) + 'pred.txt'


def png_name(entry, j, k):
    """The path of detection k of class j as the txt holds it (forward slashes on every platform)."""
    b = image_basename(entry)
    return 'seg_results/%s/%s_%s_%d.png' % (b, b, CLASS_NAMES[j - 1], k)


def pred_txt_lines(entry, boxes_per_class):
    """The lines of one image's pred.txt; boxes_per_class[j]: [n_j, 5] for j = 1..8 (index 0 ignored)."""
    lines = []
    for j in range(1, len(boxes_per_class)):
        for k in range(len(boxes_per_class[j])):
            lines.append('%s %d %s\n' % (png_name(entry, j, k), CLASS_LABEL_IDS[j - 1], str(np.float32(boxes_per_class[j][k][4]))))
    return lines


def _check_results(roidb, all_boxes, all_segms):
    """The writer's upfront checks (nothing is written before they pass)."""
    if len(all_boxes) != NUM_CLASSES + 1 or len(all_segms) != NUM_CLASSES + 1:
        raise ValueError('results of %d / %d classes (boxes / masks): Cityscapes has %d and the background'
                         % (len(all_boxes), len(all_segms), NUM_CLASSES))
    for c in range(1, NUM_CLASSES + 1):
        if len(all_boxes[c]) != len(roidb) or len(all_segms[c]) != len(roidb):
            raise ValueError('class %d: results for %d images, the image list has %d' % (c, len(all_boxes[c]), len(roidb)))
    names = [image_basename(e) for e in roidb]
    if len(set(names)) != len(names):
        raise ValueError('two images share one output name: %s' % sorted(n for n in set(names) if names.count(n) > 1)[:5])
    for i, entry in enumerate(roidb):
        H, W = int(entry['height']), int(entry['width'])
        count = 0
        for c in range(1, NUM_CLASSES + 1):
            dets, rles = all_boxes[c][i], all_segms[c][i]
            if len(dets) != len(rles):
                raise ValueError('%s, class %d: %d detections with %d masks' % (entry['image'], c, len(dets), len(rles)))
            if len(dets) and (np.asarray(dets).ndim != 2 or np.asarray(dets).shape[1] != 5):
                raise ValueError('%s, class %d: detections must be [n, 5] rows, got %s' % (entry['image'], c, np.asarray(dets).shape))
            for r in rles:
                if not isinstance(r, dict) or 'counts' not in r or 'size' not in r:
                    raise ValueError("%s, class %d: a mask must be an RLE dict with 'size' and 'counts', got %r" % (entry['image'], c, type(r)))
                if tuple(int(v) for v in r['size']) != (H, W):
                    raise ValueError('%s, class %d: RLE of size %s on an image of %d x %d' % (entry['image'], c, list(r['size']), H, W))
            count += len(rles)
        if count > MAX_PREDS:
            raise ValueError('%s: %d predictions in one image: at most %d are supported' % (entry['image'], count, MAX_PREDS))


def _save_mask_png(plane, width, one_bit, path):
    from PIL import Image
    if one_bit:
        im = Image.frombytes('1', (width, plane.shape[0]), plane.tobytes())     # (raw mode '1': MSB first, rows padded to a byte)
    else:
        im = Image.fromarray(plane)
    im.save(path)


class _Pending(object):
    __slots__ = ('paths', 'chunks', 'shape')


class InstanceMaskFormatter(object):
    """The device half of the writer. submit() uploads one image's run lists in one copy (the packing of InstanceEvaluator.add_rle),
    queues the expand launches and the copy of every chunk into pinned memory on the current stream, without synchronising; finish()
    waits for those copies alone and returns the planes as numpy views of the pinned buffers."""

    def __init__(self, one_bit=False):
        self.one_bit = bool(one_bit)
        self.device = None

    def submit(self, rles_per_class, H, W):
        """rles_per_class[j]: the RLE dicts of class j = 1..8 (index 0 ignored). ValueError before any launch as _transitions raises."""
        if self.device is None:
            self.device = torch.device('cuda', torch.cuda.current_device())
        trans, lens = [], []
        for j in range(1, len(rles_per_class)):
            if len(rles_per_class[j]):
                t, ln = _transitions(list(rles_per_class[j]), H, W)
                trans.append(t)
                lens.append(ln)
        p = _Pending()
        p.shape, p.chunks = (H, W), []
        if not lens:
            return p
        trans = np.concatenate(trans)
        off = np.concatenate([[0], np.cumsum(np.concatenate(lens))])
        if int(off[-1]) > 0x7FFFFFFF:
            raise ValueError("%d run boundaries in one image: at most 2^31 - 1" % int(off[-1]))
        off = off.astype(np.int32)
        n = off.size - 1
        check_runs(trans, off, H, W)
        # one pinned host buffer, one upload: offsets | transitions (all 4-byte items; the transitions start on a 16-byte boundary)
        t0 = (off.size + 3) // 4 * 4
        host = torch.empty((t0 + trans.size + 1,), dtype=torch.int32, pin_memory=True)
        hn = host.numpy()
        hn[:off.size] = off
        hn[t0:t0 + trans.size] = trans
        per = plane_bytes(H, W, self.one_bit)
        step = max(1, MAX_LAUNCH_BYTES // per)
        with torch.cuda.device(self.device):
            d = host.to(self.device, non_blocking=True)
            d_off, d_trans = d[:off.size], d[t0:]          # (d_trans is never empty: the spare item)
            for m0 in range(0, n, step):
                nm = min(step, n - m0)
                planes = torch.empty((nm, H, per // H), dtype=torch.uint8, device=self.device)
                _expand_into(d_trans, d_off[m0:m0 + nm + 1], nm, H, W, self.one_bit, planes, MAX_LAUNCH_BYTES)
                staged = torch.empty((nm, H, per // H), dtype=torch.uint8, pin_memory=True)
                staged.copy_(planes, non_blocking=True)
                ev = torch.cuda.Event()
                ev.record()
                p.chunks.append((staged, ev, planes))
        return p

    def finish(self, p):
        """-> the planes of the image in the order submitted: a list of uint8 [H, W] (or [H, ceil(W / 8)]) numpy views."""
        planes = []
        for staged, ev, _ in p.chunks:
            ev.synchronize()
            planes.extend(staged.numpy())
        p.chunks = []
        return planes


def write_instance_predictions(dataset, all_boxes, all_segms, output_dir, one_bit=False):
    """Write <output_dir>/inst_seg/<basename>pred.txt and the mask PNGs under <output_dir>/inst_seg/seg_results/<basename>/ for every
    image of dataset.roidb (module docstring); all_boxes[class][image] [n, 5] rows scored by column 4, all_segms[class][image] im_post's
    RLE dicts. one_bit: PNGs of bit depth 1 instead of 8-bit grey 0 / 255. Returns the pred.txt paths. ValueError before any file is
    written: a class count or per-class image count that does not match the image list, detections and masks that do not pair, an RLE
    of another size than its image."""
    roidb = dataset.roidb
    _check_results(roidb, all_boxes, all_segms)
    root = os.path.join(output_dir, 'inst_seg')
    os.makedirs(root, exist_ok=True)
    fmt = InstanceMaskFormatter(one_bit)
    written = []
    workers = MAX_ENCODE_THREADS
    with ThreadPoolExecutor(max_workers=workers) as pool:
        jobs = []

        def retire(p, i):
            entry = roidb[i]
            planes = fmt.finish(p)
            if planes:
                os.makedirs(os.path.join(root, 'seg_results', image_basename(entry)), exist_ok=True)
            names = [png_name(entry, j, k) for j in range(1, NUM_CLASSES + 1) for k in range(len(all_segms[j][i]))]
            assert len(names) == len(planes)
            for name, plane in zip(names, planes):
                jobs.append(pool.submit(_save_mask_png, plane, p.shape[1], one_bit, os.path.join(root, *name.split('/'))))
                while len(jobs) > 4 * workers:     # bounds the pinned buffers waiting for an encoder
                    jobs.pop(0).result()
            txt = os.path.join(root, pred_txt_name(entry))
            with open(txt, 'w', newline='') as f:
                f.writelines(pred_txt_lines(entry, [[]] + [all_boxes[j][i] for j in range(1, NUM_CLASSES + 1)]))
            written.append(txt)

        pending = None
        for i, entry in enumerate(roidb):
            p = fmt.submit([[]] + [all_segms[j][i] for j in range(1, NUM_CLASSES + 1)], int(entry['height']), int(entry['width']))
            if pending is not None:     # image i is on the device while image i - 1 is compressed
                retire(*pending)
            pending = (p, i)
        if pending is not None:
            retire(*pending)
        for job in jobs:
            job.result()
    logger.info('%d instance prediction files (%s masks) written to %s', len(written), '1-bit' if one_bit else '8-bit', os.path.abspath(root))
    return written


# ------------------------------------------------------------------------------------------------------------------ reader
def list_txt_files(folder):
    """Every .txt file under folder (recursively), sorted: the candidates of find_prediction_file."""
    found = []
    for d, _, files in os.walk(folder):
        found += [os.path.join(d, f) for f in files if f.endswith('.txt')]
    return sorted(found)


def image_key(entry):
    """<city>_<sequence>_<frame> of the image <city>_<sequence>_<frame>_leftImg8bit.png."""
    base = image_basename(entry)
    return base[:-len('_leftImg8bit')] if base.endswith('_leftImg8bit') else base


def find_prediction_file(folder, entry, txt_files=None):
    """The one file under folder named <key>*.txt; ValueError naming the image for none or several."""
    txt_files = list_txt_files(folder) if txt_files is None else txt_files
    pattern = image_key(entry) + '*.txt'
    hits = [p for p in txt_files if fnmatch.fnmatchcase(os.path.basename(p), pattern)]
    if len(hits) != 1:
        raise ValueError('%s: %s prediction file matching %s under %s%s' % (os.path.basename(entry['image']), 'no' if not hits else 'more than one',
                                                                          pattern, folder, ''.join('\n  ' + h for h in hits[:5])))
    return hits[0]


def parse_prediction_file(path, folder):
    """[(mask path, label id, float32 score)] of every line of one prediction file, lines of other labels included."""
    root = os.path.abspath(folder)
    rows = []
    with open(path, 'r') as f:
        for no, line in enumerate(f, 1):
            line = line.rstrip('\r\n')
            if not line.strip():
                continue
            where = '%s, line %d' % (path, no)
            fields = line.split(' ')
            if len(fields) != 3 or any(not v for v in fields):
                raise ValueError('%s: expected "<mask png> <label id> <confidence>", got %r' % (where, line))
            try:
                label = int(fields[1])
            except ValueError:
                raise ValueError('%s: the label id %r is not an integer' % (where, fields[1]))
            try:
                score = float(fields[2])
            except ValueError:
                raise ValueError('%s: the confidence %r is not a number' % (where, fields[2]))
            if score != score:
                raise ValueError('%s: the confidence is NaN' % where)
            if not LABEL_ID_RANGE[0] <= label <= LABEL_ID_RANGE[1]:
                raise ValueError('%s: %d is no Cityscapes label id (%d..%d)' % ((where, label) + LABEL_ID_RANGE))
            if os.path.isabs(fields[0]) or fields[0].startswith(('/', '\\')):
                raise ValueError('%s: the mask path %s is absolute; it must be relative to the file' % (where, fields[0]))
            png = os.path.abspath(os.path.join(os.path.dirname(path), fields[0]))
            if os.path.commonpath([root, png]) != root:
                raise ValueError('%s: the mask path %s leaves %s' % (where, fields[0], folder))
            if not os.path.isfile(png):
                raise FileNotFoundError('%s: no mask at %s' % (where, png))
            rows.append((png, label, np.float32(score)))
    return rows


def _decode_mask(path, shape, out):
    from PIL import Image
    with Image.open(path) as im:
        if (im.size[1], im.size[0]) != shape:
            raise ValueError('%s: a mask of %d x %d for an image of %d x %d' % (path, im.size[1], im.size[0], shape[0], shape[1]))
        np.not_equal(np.asarray(im.convert('L')), 0, out=out.view(bool))


def read_instance_predictions(folder, entry, txt_files=None, pool=None):
    """The predictions of one image from a folder in the benchmark's format (module docstring): {'file', 'masks' uint8 [n, H, W] (0 / 1;
    a pinned host tensor), 'scores' float32 [n], 'classes' int64 [n] in 1..8}, in the file's order, lines of other labels left out.
    txt_files: list_txt_files(folder), to walk the folder once for many images; pool: the executor that decodes the PNGs (default: one
    of MAX_ENCODE_THREADS threads for this call)."""
    path = find_prediction_file(folder, entry, txt_files)
    rows = [r for r in parse_prediction_file(path, folder) if r[1] in CLASS_LABEL_IDS]
    if len(rows) > MAX_PREDS:
        raise ValueError('%s: %d predictions in one image: at most %d are supported' % (path, len(rows), MAX_PREDS))
    H, W = int(entry['height']), int(entry['width'])
    masks = torch.empty((len(rows), H, W), dtype=torch.uint8, pin_memory=torch.cuda.is_available())
    views = masks.numpy()
    own = pool is None
    if own:
        pool = ThreadPoolExecutor(max_workers=MAX_ENCODE_THREADS)
    try:
        for job in [pool.submit(_decode_mask, r[0], (H, W), views[k]) for k, r in enumerate(rows)]:
            job.result()
    finally:
        if own:
            pool.shutdown()
    return {'file': path, 'masks': masks, 'scores': np.array([r[2] for r in rows], np.float32),
            'classes': np.array([CLASS_LABEL_IDS.index(r[1]) + 1 for r in rows], np.int64)}


def score_instance_files(dataset, folder, after_image=None):
    """Score a prediction folder against dataset's gtFine instanceIds maps with InstanceEvaluator.add_masks; returns the evaluator.
    The masks of an image go up as one uint8 [n, H, W] tensor, in copies of at most MAX_LAUNCH_BYTES. after_image(index, evaluator,
    predictions): called after each image is queued (the tests read last_counts() there)."""
    from .cityscapes_eval import InstanceEvaluator
    ev = InstanceEvaluator()
    txt_files = list_txt_files(folder)
    dev = ev._dev()
    with ThreadPoolExecutor(max_workers=MAX_ENCODE_THREADS) as pool:
        for i, entry in enumerate(dataset.roidb):
            gt = dataset.load_instance_gt(entry)
            pred = read_instance_predictions(folder, entry, txt_files, pool)
            host = pred['masks']
            n, (H, W) = int(host.shape[0]), gt.shape
            masks = torch.empty((n, H, W), dtype=torch.uint8, device=dev)
            step = max(1, MAX_LAUNCH_BYTES // (H * W))
            for m0 in range(0, n, step):
                masks[m0:m0 + step].copy_(host[m0:m0 + step], non_blocking=True)
            ev.add_masks(gt, masks, pred['scores'], pred['classes'])
            if after_image is not None:
                after_image(i, ev, pred)
    return ev
