"""Panoptic predictions in COCO panoptic format, both directions (csrc/pan_format.hip).

Writing: the reference's _converter_2ch_single_core (upsnet/dataset/base_dataset.py:463-511, without vis_panoptic) and the save_image /
json.dump calls of its evaluate_panoptic (:321-327). `panoptic_format` turns one 2-channel map into the panoptic PNG content and its
segments_info on the device; `write_panoptic` writes pan_2ch/*.png, pan/*.png and pred.json, compressing image i on host threads
while image i + 1 is on the device. Reading: `read_panoptic` yields the (PNG, segments_info) pairs of a written prediction, and
`relabel` is the device half of PanopticEvaluator.add_png (dataset/pq.py).

The colour rule is the contract of panopticapi's IdGenerator with its np.random draw replaced by a fixed counter-based sequence, so
that the same map and category table give byte-identical files on every run. Segments are visited in ascending key (category << 8 |
instance); `ordinal` counts the segments of one category from 0; the taken set starts as the colours of all stuff categories.
  * The first segment of a category takes the category colour, unless that is (0,0,0) or, for a thing, already taken.
  * Every other segment (a further thing instance; also a further segment of a stuff category, which this project's own maps never
    hold, so that ids stay unique) tries attempt a = 0, 1, ...: cell = (lowbias32(category << 16 | ordinal) + a * 100003) mod 61^3,
    per-channel offset (cell mod 61, cell // 61 mod 61, cell // 3721) - 30, colour = clamp(base + offset, 0, 255), until the colour
    is neither (0,0,0) nor taken. 100003 is coprime to 61^3: the attempts visit every cell of the +-30 cube exactly once.
  * A category without 'color' gets default_color(id): ((67 id + 41) mod 256, (137 id + 83) mod 256, (29 id + 127) mod 256), non-zero
    and distinct per id (67 is odd).
ColorGenerator is the host statement of the rule; the device (pan_color_kernel) is held to it by tests/test_pan_format_gpu.py.

Frame-stable mode (`stable_ids=True`, opt-in; for maps whose instance numbers are track ids, dataset/pan_track.py): colours and ids are
pure functions of (category, instance), so a track looks the same in every frame of a sequence. The PNG colour is (R, G, B) =
(category, instance, 1), VOID (0,0,0): unique within an image and decodable without the JSON, and segments_info[].id = R + 256 G +
65536 B follows from it. The picture colour (stable_color; what pan_vis blends in) is the category colour for stuff and, for a thing,
the offset rule above with ordinal := instance and the first attempt whose colour is not (0,0,0); there is no taken set, so two
segments of an image may share a picture colour. The default mode is unchanged by this.

Deviations from the reference: `bbox` is the reference's [x_min, y_min, x_max - x_min, y_max - y_min] (one less than COCO's width and
height; PQ does not read it); one colour generator per image (ids only have to be unique within an image); every annotation of
pred.json also carries `image_id` and `file_name`; invalid input raises ValueError before any launch, a segment whose category is not
in the table raises KeyError at the image's synchronisation.
"""
import json
import logging
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from .._lib import check, dense, lib, ptr, require_cuda, stream, written
from .pq import MAX_CATEGORY, _check_image

logger = logging.getLogger(__name__)

MAX_ENCODE_THREADS = 8        # PNG encoder threads (never sized from the host's CPU count), as evaluate.MAX_DECODE_THREADS
FAST_ROWS = 1024              # table rows that travel with the RGB map in the one device-to-host copy of an image
HEAD, ROW = 8, 8              # ints before the first row / per row of the device table (include/upsnet_hip.h)
MAX_SEGMENTS = 255 * 256
CUBE, STEP = 61 ** 3, 100003
INV62 = 1 << 62


def default_color(cat_id):
    """The colour of a category whose table entry has no 'color': non-zero and distinct per id in 0..254."""
    i = int(cat_id)
    return [(67 * i + 41) % 256, (137 * i + 83) % 256, (29 * i + 127) % 256]


def category_dict(categories):
    """{id: entry} of a category table given as that dict or as the JSON's list; ValueError for ids outside 0..254."""
    if not isinstance(categories, dict):
        categories = {el['id']: el for el in categories}
    bad = [c for c in categories if not 0 <= int(c) <= MAX_CATEGORY]
    if bad:
        raise ValueError("category ids must lie in 0..%d, got %s" % (MAX_CATEGORY, bad))
    return categories


def category_color(cat_id, entry):
    color = entry.get('color')
    if color is None:
        return default_color(cat_id)
    color = [int(v) for v in color]
    if len(color) != 3 or any(not 0 <= v <= 255 for v in color):
        raise ValueError("category %s: 'color' must be three values in 0..255, got %s" % (cat_id, color))
    return color


def category_table(categories):
    """int32 [256] for the device: -1 = not in the table, else R | G << 8 | B << 16 | isthing << 24."""
    table = np.full(256, -1, np.int32)
    for c, entry in category_dict(categories).items():
        r, g, b = category_color(c, entry)
        table[int(c)] = r | g << 8 | b << 16 | int(entry['isthing'] != 0) << 24
    return table


def _lowbias32(x):
    x ^= x >> 16
    x = (x * 0x7feb352d) & 0xffffffff
    x ^= x >> 15
    x = (x * 0x846ca68b) & 0xffffffff
    x ^= x >> 16
    return x


def color_attempt(base, cat_id, ordinal, attempt):
    """Attempt `attempt` of the ordinal-th segment of a category around its base colour: the counter-based sequence of the rule."""
    cell = (_lowbias32((int(cat_id) << 16 | int(ordinal)) & 0xffffffff) % CUBE + attempt * STEP) % CUBE
    offset = (cell % 61 - 30, cell // 61 % 61 - 30, cell // 3721 - 30)
    return tuple(min(255, max(0, b + d)) for b, d in zip(base, offset))


def stable_color(cat_id, instance, entry):
    """The frame-stable picture colour of (category, instance): the host statement of pan_stable_kernel's mode 1."""
    base = tuple(category_color(cat_id, entry))
    if entry['isthing'] == 0:
        return list(base)
    for attempt in range(CUBE):
        color = color_attempt(base, cat_id, instance, attempt)
        if color != (0, 0, 0):
            return list(color)
    raise RuntimeError("unreachable: the +-30 cube holds a non-zero offset")


def stable_id_color(cat_id, instance):
    """The frame-stable PNG colour of (category, instance): (category, instance, 1); VOID (category 255) is (0,0,0)."""
    return [0, 0, 0] if int(cat_id) == 255 else [int(cat_id), int(instance), 1]


class ColorGenerator(object):
    """The colour rule on the host, one object per image; get_color(category id) in ascending key order. KeyError for a category
    that is not in the table."""

    def __init__(self, categories):
        self.categories = category_dict(categories)
        self.taken = set(tuple(category_color(c, e)) for c, e in self.categories.items() if e['isthing'] == 0)
        self.count = {}

    def get_color(self, cat_id):
        entry = self.categories[cat_id]
        ordinal = self.count.get(cat_id, 0)
        self.count[cat_id] = ordinal + 1
        base = tuple(category_color(cat_id, entry))
        if ordinal == 0 and base != (0, 0, 0) and (entry['isthing'] == 0 or base not in self.taken):
            color = base
        else:
            for attempt in range(CUBE):
                color = color_attempt(base, cat_id, ordinal, attempt)
                if color != (0, 0, 0) and color not in self.taken:
                    break
            else:
                raise RuntimeError("no free colour left within +-30 of category %s's colour %s" % (cat_id, list(base)))
        self.taken.add(color)
        return list(color)


def png_name(file_name):
    """The reference's save_image naming (base_dataset.py:263)."""
    return file_name.replace('_leftImg8bit', '').replace('jpg', 'png').replace('jpeg', 'png')


class _Pending(object):
    __slots__ = ('index', 'shape', 'offset', 'buf', 'host', 'event', 'pred_host')


class PanopticFormatter(object):
    """2-channel maps -> (RGB id map, segments_info) on one device, for one category table. submit() queues an image on the current
    stream and starts its one device-to-host copy (RGB map, table header and the first FAST_ROWS rows) into pinned memory without
    synchronising; finish() waits for that copy alone. An image of more than FAST_ROWS segments costs a second copy."""

    def __init__(self, categories, device=None, stable_ids=False):
        self.cat_table_host = category_table(categories)
        self.device = torch.device(device) if device is not None else None
        self.num_images = 0
        self._state = None
        self.stable_ids = bool(stable_ids)     # frame-stable ids and colours (the module's docstring); the default path is untouched

    def _dev_state(self):
        if self._state is None:
            dev = self.device if self.device is not None else torch.device('cuda', torch.cuda.current_device())
            self.device = dev
            self._state = dict(cat_table=torch.from_numpy(self.cat_table_host).to(dev),
                               ws=torch.zeros((int(lib().upsnet_pan_format_workspace_bytes()),), dtype=torch.uint8, device=dev))
        return self._state

    def submit(self, pred_2ch, keep_input=False):
        """pred_2ch: uint8 [H,W,3] device tensor (a numpy array is uploaded). keep_input: the handle also carries the 2-channel map
        on the host (copied in the same group)."""
        _check_image('pred_2ch', pred_2ch)
        st = self._dev_state()
        pred_host = None
        if isinstance(pred_2ch, np.ndarray):
            pred_host = np.ascontiguousarray(pred_2ch)
            pred_2ch = torch.from_numpy(pred_host).to(self.device, non_blocking=True)
        require_cuda(pred_2ch)
        pred_2ch = dense(pred_2ch)
        H, W = int(pred_2ch.shape[0]), int(pred_2ch.shape[1])
        if H * W == 0 or H * W >= 1 << 31:
            raise ValueError("pred_2ch of %d x %d pixels" % (H, W))
        p = _Pending()
        p.index, p.shape = self.num_images, (H, W)
        p.offset = (H * W * 3 + 15) // 16 * 16
        p.buf = torch.empty((p.offset + 4 * int(lib().upsnet_pan_format_table_ints()),), dtype=torch.uint8, device=self.device)
        table = p.buf[p.offset:].view(torch.int32)
        check(lib().upsnet_pan_format(stream(), ptr(pred_2ch), H, W, ptr(st['cat_table']), ptr(st['ws']), ptr(p.buf), ptr(table)),
              "pan_format")
        if self.stable_ids:     # the table (areas, boxes) stays; the id map is repainted as (category, instance, 1)
            from .. import ops
            ops.pan_stable_colors(pred_2ch, None, 0, p.buf[:H * W * 3])
        self.num_images += 1
        nfast = p.offset + 4 * (HEAD + ROW * FAST_ROWS)
        p.host = torch.empty((nfast,), dtype=torch.uint8, pin_memory=True)
        p.host.copy_(p.buf[:nfast], non_blocking=True)
        p.pred_host = None
        if keep_input:
            if pred_host is None:
                pred_host = torch.empty((H, W, 3), dtype=torch.uint8, pin_memory=True)
                pred_host.copy_(pred_2ch, non_blocking=True)
                pred_host = pred_host.numpy()
            p.pred_host = pred_host
        p.event = torch.cuda.Event()
        p.event.record()
        return p

    def finish(self, p):
        """-> (rgb uint8 [H,W,3] device tensor, the same map as a numpy view of the pinned host copy, segments_info)."""
        p.event.synchronize()
        H, W = p.shape
        host = p.host.numpy()
        n, err, cat = (int(v) for v in host[p.offset:p.offset + 12].view(np.int32))
        if err == 1:
            raise KeyError('In the image with index {} (in the order added) a segment has unknown category_id {}.'.format(p.index, cat))
        if err:
            raise RuntimeError('image %d: no free colour left within +-30 of the colour of category %d' % (p.index, cat))
        first = p.offset + 4 * HEAD
        if n <= FAST_ROWS:
            rows = host[first:first + 4 * ROW * n]
        else:   # (beyond the rows that travelled with the map: a second copy, noise-like maps only)
            rows = p.buf[first:first + 4 * ROW * n].cpu().numpy()
        rows = rows.view(np.int32).reshape(n, ROW).tolist()
        if self.stable_ids:
            for r in rows:
                r[6] = (r[0] >> 8) + 256 * (r[0] & 255) + 65536
        segments_info = [{'id': r[6], 'category_id': r[0] >> 8, 'iscrowd': 0, 'bbox': [r[2], r[3], r[4] - r[2], r[5] - r[3]], 'area': r[1]}
                         for r in rows]
        rgb = p.buf[:H * W * 3].view(H, W, 3)
        return rgb, host[:H * W * 3].reshape(H, W, 3), segments_info


def panoptic_format(pred_2ch, categories):
    """One 2-channel map (uint8 [H,W,3] device tensor as unified_pan_result / combined_pan_result return it) -> (rgb uint8 [H,W,3]
    device tensor with id = R + 256 G + 65536 B and VOID (0,0,0), segments_info: dicts of id, category_id, iscrowd 0, bbox, area in
    ascending (category, instance), plain ints). KeyError if a segment's category is not in `categories`."""
    fmt = PanopticFormatter(categories, pred_2ch.device if isinstance(pred_2ch, torch.Tensor) else None)
    rgb, _, segments_info = fmt.finish(fmt.submit(pred_2ch))
    return rgb, segments_info


def _save_png(array, path):
    from PIL import Image
    Image.fromarray(array).save(path)


def write_panoptic(pred_pans_2ch, images, categories, output_dir, image_ids=None, stable_ids=False, confs=None, write_conf=False):
    """Write output_dir/pan_2ch/<name>.png (the 2-channel maps), output_dir/pan/<name>.png (the panoptic PNGs) and
    output_dir/pred.json ({'annotations': [{'image_id', 'file_name', 'segments_info'}]}); name = png_name(images[i]['file_name']),
    image_id = image_ids[i] if given, else images[i]['id']. Returns the annotations. ValueError before any launch: counts that do
    not match, an image without file_name (or id), two images of one output name, a map that is not uint8 [H,W,3]. stable_ids: the
    frame-stable ids and colours of the module's docstring (for tracked maps). confs (one uint8 [H,W] confidence plane per map, device
    tensors or numpy arrays): every segments_info entry gains "score" = the mean confidence of the segment over 255
    (dataset/pan_confidence.segment_scores, on the map as given); write_conf: the planes are also written to
    output_dir/conf/<name>.png, 8-bit grey. Without confs every file is byte for byte what it is without the argument."""
    preds, images = list(pred_pans_2ch), list(images)
    if len(preds) != len(images):
        raise ValueError("%d predictions for %d images" % (len(preds), len(images)))
    confs = None if confs is None else list(confs)
    if confs is not None and len(confs) != len(preds):
        raise ValueError("%d confidence planes for %d predictions" % (len(confs), len(preds)))
    if write_conf and confs is None:
        raise ValueError("write_conf needs the confidence planes (confs=)")
    if image_ids is not None and len(image_ids) != len(images):
        raise ValueError("%d image ids for %d images" % (len(image_ids), len(images)))
    names = []
    for i, im in enumerate(images):
        if 'file_name' not in im or (image_ids is None and 'id' not in im):
            raise ValueError("image %d has no file_name / id: %s" % (i, im))
        names.append(png_name(im['file_name']))
    if len(set(names)) != len(names):
        raise ValueError("two images share one output name: %s" % sorted(n for n in set(names) if names.count(n) > 1)[:5])
    ids = list(image_ids) if image_ids is not None else [im['id'] for im in images]
    for pred in preds:
        _check_image('pred_2ch', pred)
    fmt = PanopticFormatter(categories, stable_ids=stable_ids)
    for sub in ('pan_2ch', 'pan') + (('conf',) if write_conf else ()):
        for name in names:
            os.makedirs(os.path.dirname(os.path.join(output_dir, sub, name)), exist_ok=True)
    annotations = [None] * len(preds)
    workers = max(1, min(MAX_ENCODE_THREADS, len(preds)))
    with ThreadPoolExecutor(max_workers=workers) as pool:
        jobs = []

        def retire(p, k):
            _, rgb_host, segments_info = fmt.finish(p)
            if confs is not None:     # (both tables list the non-VOID keys of one map in ascending key)
                from .pan_confidence import segment_scores
                scores = segment_scores(preds[k], confs[k])
                if len(scores) != len(segments_info):
                    raise RuntimeError("image %d: %d scored segments for %d written ones" % (k, len(scores), len(segments_info)))
                for seg, ((cat, _), (_, _, score)) in zip(segments_info, scores.items()):
                    if seg['category_id'] != cat:
                        raise RuntimeError("image %d: score of category %d for a segment of category %d" % (k, cat, seg['category_id']))
                    seg['score'] = score
                if write_conf:
                    plane = confs[k].cpu().numpy() if isinstance(confs[k], torch.Tensor) else np.asarray(confs[k])
                    jobs.append(pool.submit(_save_png, np.ascontiguousarray(plane), os.path.join(output_dir, 'conf', names[k])))
            annotations[k] = {'image_id': ids[k], 'file_name': names[k], 'segments_info': segments_info}
            jobs.append(pool.submit(_save_png, p.pred_host, os.path.join(output_dir, 'pan_2ch', names[k])))
            jobs.append(pool.submit(_save_png, rgb_host, os.path.join(output_dir, 'pan', names[k])))
            while len(jobs) > 4 * workers:     # bounds the pinned buffers waiting for an encoder
                jobs.pop(0).result()

        pending = None
        for k, pred in enumerate(preds):
            p = fmt.submit(pred, keep_input=True)     # image k is on the device while image k - 1 is compressed
            if pending is not None:
                retire(*pending)
            pending = (p, k)
        if pending is not None:
            retire(*pending)
        for job in jobs:
            job.result()
    with open(os.path.join(output_dir, 'pred.json'), 'w') as f:
        json.dump({'annotations': annotations}, f)
    return annotations


def read_panoptic(pred_json, pred_folder):
    """Yield (rgb uint8 [H,W,3], segments_info) per annotation of a COCO panoptic prediction, in the JSON's order."""
    from .base_dataset import load_panoptic_png
    with open(pred_json, 'r') as f:
        annotations = json.load(f)['annotations']
    for ann in annotations:
        yield load_panoptic_png(os.path.join(pred_folder, ann['file_name'])), ann['segments_info']


def segments_table(pred_segments_info):
    """A prediction's segments_info -> int32 [n,3] (id, category, instance slot) sorted by id, slots per category from 0 in ascending
    id. ValueError: an id outside 1..2^24-1 or used twice, a category outside 0..254, more than 256 segments of one category."""
    n = len(pred_segments_info)
    segs = np.array([(el['id'], el['category_id']) for el in pred_segments_info], np.int64).reshape(n, 2)
    ids, cats = segs[:, 0], segs[:, 1]
    if np.any(ids == 0):
        raise ValueError("pred segment with id 0 (the VOID id of the panoptic PNG)")
    if np.any((ids < 0) | (ids >= 1 << 24)):
        raise ValueError("pred segment ids must lie in 1..2^24-1 (the ids a PNG can hold)")
    uniq, counts = np.unique(ids, return_counts=True)
    if np.any(counts > 1):
        raise ValueError("duplicate pred segment ids %s" % uniq[counts > 1].tolist())
    if np.any((cats < 0) | (cats > MAX_CATEGORY)):
        raise ValueError("pred category ids must lie in 0..%d, got %s" % (MAX_CATEGORY, sorted(set(cats[(cats < 0) | (cats > MAX_CATEGORY)].tolist()))))
    segs = segs[np.argsort(ids, kind='stable')]
    slots = np.zeros(n, np.int64)
    seen = {}
    for i, c in enumerate(segs[:, 1].tolist()):
        slots[i] = seen.get(c, 0)
        seen[c] = slots[i] + 1
    many = sorted(c for c, k in seen.items() if k > 256)
    if many:
        raise ValueError("more than 256 pred segments of one category: %s" % many)
    return np.ascontiguousarray(np.concatenate([segs, slots[:, None]], 1).astype(np.int32))


def relabel(rgb, table, image_index, status):
    """Panoptic PNG on the device -> (2-channel map uint8 [H,W,3], pixels per table row int32 [n]); table: segments_table's array;
    status: int64 [2] device tensor kept across images (include/upsnet_hip.h). No host synchronisation."""
    require_cuda(rgb, status)
    if rgb.dtype != torch.uint8 or rgb.dim() != 3 or rgb.shape[2] != 3:
        raise ValueError("relabel: rgb must be uint8 [H,W,3], got %s %s" % (tuple(rgb.shape), rgb.dtype))
    written(status, torch.int64, "relabel: status")
    table = np.ascontiguousarray(table, np.int32).reshape(-1, 3)
    n = int(table.shape[0])
    rgb = dense(rgb)
    H, W = int(rgb.shape[0]), int(rgb.shape[1])
    out = torch.empty((H, W, 3), dtype=torch.uint8, device=rgb.device)
    counts = torch.zeros((max(n, 1),), dtype=torch.int32, device=rgb.device)
    dtable = None
    if n:
        dtable = torch.from_numpy(table)
        if torch.cuda.is_available():
            dtable = dtable.pin_memory()
        dtable = dtable.to(rgb.device, non_blocking=True)
    check(lib().upsnet_pan_relabel(stream(), ptr(rgb), H, W, ptr(dtable), n, int(image_index), ptr(out), ptr(counts), ptr(status)),
          "pan_relabel")
    return out, counts[:n]
