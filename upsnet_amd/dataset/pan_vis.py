"""Panoptic predictions as pictures, on the device (csrc/pan_vis.hip): the vis_panoptic branch of the
reference's _converter_2ch_single_core (upsnet/dataset/base_dataset.py:463-511) and the same map over the photograph.

The reference paints every segment in its category colour and draws white contours around the thing instances with cv2.findContours
and PIL's draw.line(width=2), both third-party rasterisers and no parity target. The rule here states what is drawn in integers (the
kernel file's header has it in full):
  * mode 'flat': the category colour per pixel (VOID black), and white on every pixel that is, or has to its left, above it or
    diagonally up-left, an edge pixel of a thing segment with a non-zero instance number: the contour, two pixels wide;
  * mode 'overlay': the photograph, every segment blended in at 1/2 in its own colour (pan_format's per-segment rule, so instances of
    one class differ), every segment border pixel white at 1/2 on top, then for the segments of at least label_min_area pixels (at
    most the first MAX_LABELS in ascending key) the category name centred on the segment's integer centroid and pushed into the image.

`render_panoptic` draws one map; `vis_panoptic` is the file loop (decode ahead, draw, copy back, encode, all on bounded pools).
Refused with ValueError before any launch: overlay without an image, an image of another size than the map, a category name of more
than MAX_NAME bytes. A segment whose category is not in the table raises the formatter's KeyError.
"""
import logging
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from .._lib import check, dense, lib, ptr, stream, written
from .pan_format import PanopticFormatter, category_dict, png_name
from .pq import _check_image
from .vis import MAX_DECODE_THREADS, MAX_ENCODE_THREADS, _save_png, load_image

logger = logging.getLogger(__name__)

MODES = {'flat': 0, 'overlay': 1}     # the `mode` argument of upsnet_pan_vis (include/upsnet_hip.h)
MAX_LABELS = 256                      # labels drawn per image (upsnet_pan_vis_max_labels)
MAX_NAME = 32                         # bytes per category name
FOLDERS = {'flat': 'vis_flat', 'overlay': 'vis'}


def label_text(cat_id, entry):
    """The bytes drawn for a category: its 'name', or str(id) for an entry without one."""
    name = entry.get('name')
    text = str(cat_id) if name is None else name
    return text if isinstance(text, bytes) else str(text).encode('utf-8')


def name_table(categories):
    """(uint8 [256, MAX_NAME], int32 [256]) for the device: the label bytes and their count per category id. ValueError for a label of
    more than MAX_NAME bytes."""
    names = np.zeros((256, MAX_NAME), np.uint8)
    lens = np.zeros(256, np.int32)
    for c, entry in category_dict(categories).items():
        b = label_text(c, entry)
        if len(b) > MAX_NAME:
            raise ValueError("category %s: the name %r has %d bytes, at most %d are drawn" % (c, b, len(b), MAX_NAME))
        names[int(c), :len(b)] = np.frombuffer(b, np.uint8)
        lens[int(c)] = len(b)
    return names, lens


def _check_mode(mode):
    if mode not in MODES:
        raise ValueError("mode must be one of %s, got %r" % (sorted(MODES), mode))


class PanopticRenderer(object):
    """2-channel maps -> pictures on one device, for one category table: a PanopticFormatter (segment table, per-segment colours) and
    the drawing workspace, both kept across images. submit() queues one picture on the current stream without synchronising and
    returns (picture uint8 [H,W,3] device tensor, info int32 [2] device tensor: segments that qualified for a label, labels drawn,
    the formatter's handle); the handle's finish() raises the KeyError of an unknown category."""

    def __init__(self, categories, device=None, stable_ids=False):
        self.names_host, self.lens_host = name_table(categories)
        self.formatter = PanopticFormatter(categories, device, stable_ids=stable_ids)
        self.stable_ids = bool(stable_ids)     # overlay: segments blended in pan_format.stable_color, the same in every frame
        self._state = None

    def _dev_state(self):
        if self._state is None:
            self.formatter._dev_state()
            dev = self.formatter.device
            ws = torch.empty((int(lib().upsnet_pan_vis_workspace_bytes()),), dtype=torch.uint8, device=dev)
            ws[:int(lib().upsnet_pan_vis_workspace_zeroed_bytes())].zero_()     # once; every call leaves it zeroed again
            self._state = dict(ws=ws, names=torch.from_numpy(self.names_host).to(dev), lens=torch.from_numpy(self.lens_host).to(dev))
        return self._state

    def submit(self, pred_2ch, image=None, mode='overlay', label_min_area=1024, out=None):
        """out: a contiguous uint8 [H,W,3] device tensor to draw into (default: a new one); it must overlap no input."""
        _check_mode(mode)
        _check_image('pred_2ch', pred_2ch)
        label_min_area = int(label_min_area)
        if label_min_area < 0:
            raise ValueError("label_min_area must not be negative, got %d" % label_min_area)
        H, W = int(pred_2ch.shape[0]), int(pred_2ch.shape[1])
        if mode == 'overlay':
            if image is None:
                raise ValueError("mode 'overlay' draws over the photograph: pass image= (RGB uint8 [H, W, 3])")
            _check_image('image', image)
            if tuple(image.shape) != (H, W, 3):
                raise ValueError("the image is %s, the panoptic map %s" % (tuple(image.shape), (H, W, 3)))
        if not 1 <= H <= 32768 or not 1 <= W <= 32768 or H * W > 1 << 28:
            raise ValueError("a map of %d x %d cannot be drawn: sides in 1..32768 and at most 2^28 pixels" % (H, W))
        st = self._dev_state()
        dev = self.formatter.device
        if isinstance(pred_2ch, np.ndarray):
            pred_2ch = torch.from_numpy(np.ascontiguousarray(pred_2ch)).to(dev, non_blocking=True)
        if not pred_2ch.is_cuda:
            raise RuntimeError("render_panoptic: the map must be on the device (there is no CPU fallback)")
        pred_2ch = dense(pred_2ch)
        if mode == 'overlay':
            if isinstance(image, np.ndarray):
                image = torch.from_numpy(np.ascontiguousarray(image)).to(dev, non_blocking=True)
            if not image.is_cuda:
                raise RuntimeError("render_panoptic: the image must be on the device (there is no CPU fallback)")
            image = dense(image)
        with torch.cuda.device(dev):
            handle = self.formatter.submit(pred_2ch)
            table = handle.buf[handle.offset:].view(torch.int32)
            if out is None:
                out = torch.empty((H, W, 3), dtype=torch.uint8, device=dev)
            elif not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.uint8 and tuple(out.shape) == (H, W, 3)
                      and out.is_contiguous()):
                raise ValueError("out must be a contiguous uint8 device tensor of shape %s" % ((H, W, 3),))
            written(out, torch.uint8, "render_panoptic: out")
            info = torch.empty((2,), dtype=torch.int32, device=dev)
            overlay = mode == 'overlay'
            colours = handle.buf
            if overlay and self.stable_ids:
                from .. import ops
                colours = ops.pan_stable_colors(pred_2ch, self.formatter._state['cat_table'], 1,
                                                torch.empty((H, W, 3), dtype=torch.uint8, device=dev))
            check(lib().upsnet_pan_vis(stream(), MODES[mode], ptr(pred_2ch), ptr(colours) if overlay else None,
                                       ptr(table) if overlay else None, ptr(image) if overlay else None, H, W,
                                       ptr(self.formatter._state['cat_table']), ptr(st['names']), ptr(st['lens']), label_min_area,
                                       ptr(st['ws']), ptr(out), ptr(info)), "pan_vis")
        return out, info, handle


def render_panoptic(pred_2ch, categories, image=None, mode='overlay', label_min_area=1024):
    """One 2-channel map (uint8 [H,W,3], a device tensor as unified_pan_result / combined_pan_result return it, or a numpy array that
    is uploaded) -> its picture, uint8 [H,W,3] on the device. mode 'flat' needs no image; 'overlay' takes the photograph as RGB uint8
    [H,W,3]. KeyError if a segment's category is not in `categories`; ValueError for overlay without an image, an image of another
    size, a category name of more than MAX_NAME bytes."""
    _check_mode(mode)
    r = PanopticRenderer(categories, pred_2ch.device if isinstance(pred_2ch, torch.Tensor) else None)
    out, info, handle = r.submit(pred_2ch, image, mode, label_min_area)
    r.formatter.finish(handle)
    return out


def vis_panoptic(pred_pans_2ch, images, categories, output_dir, mode, image_paths=None, label_min_area=1024, stable_ids=False):
    """Write one picture per prediction: mode 'overlay' to output_dir/vis/<name>, 'flat' to output_dir/vis_flat/<name>, name =
    png_name(images[i]['file_name']) as write_panoptic names its files. image_paths[i] is the photograph of prediction i (overlay
    only). Image i + k is decoded ahead on a bounded thread pool, picture i is copied back through pinned memory while picture i + 1
    is drawn, and its PNG is written by a bounded pool. Returns the written paths. ValueError before any launch: counts that do not
    match, an image without file_name, two images of one output name, overlay without image_paths. stable_ids: segments in their
    frame-stable colours (pan_format's docstring; for tracked maps)."""
    _check_mode(mode)
    preds, images = list(pred_pans_2ch), list(images)
    if len(preds) != len(images):
        raise ValueError("%d predictions for %d images" % (len(preds), len(images)))
    if mode == 'overlay' and (image_paths is None or len(image_paths) != len(images)):
        raise ValueError("mode 'overlay' needs one image path per prediction (%s for %d)"
                         % ('none' if image_paths is None else len(image_paths), len(images)))
    for i, im in enumerate(images):
        if 'file_name' not in im:
            raise ValueError("image %d has no file_name: %s" % (i, im))
    names = [png_name(im['file_name']) for im in images]
    if len(set(names)) != len(names):
        raise ValueError("two images share one output name: %s" % sorted(n for n in set(names) if names.count(n) > 1)[:5])
    for pred in preds:
        _check_image('pred_2ch', pred)
    renderer = PanopticRenderer(categories, stable_ids=stable_ids)
    paths = [os.path.join(output_dir, FOLDERS[mode], name) for name in names]
    for path in paths:
        os.makedirs(os.path.dirname(path), exist_ok=True)
    n = len(preds)
    overlay = mode == 'overlay'
    workers = max(1, min(MAX_DECODE_THREADS, n))
    ahead = 2 * workers
    dropped = 0
    dev = torch.device('cuda', torch.cuda.current_device())
    with ThreadPoolExecutor(max_workers=workers) as dec, ThreadPoolExecutor(max_workers=max(1, min(MAX_ENCODE_THREADS, n))) as enc:
        jobs = []

        def retire(i, host, info_host, handle, event):
            event.synchronize()
            renderer.formatter.finish(handle)          # (the KeyError of an unknown category)
            jobs.append(enc.submit(_save_png, host.numpy(), paths[i]))
            while len(jobs) > 4 * MAX_ENCODE_THREADS:      # bounds the pinned buffers waiting for an encoder
                jobs.pop(0).result()
            return max(0, int(info_host[0]) - int(info_host[1]))

        decoded = {j: dec.submit(load_image, image_paths[j]) for j in range(min(ahead, n))} if overlay else {}
        pending = None
        for i in range(n):
            image = None
            if overlay:
                if i + ahead < n:
                    decoded[i + ahead] = dec.submit(load_image, image_paths[i + ahead])
                image = torch.from_numpy(decoded.pop(i).result()).pin_memory().to(dev, non_blocking=True)
            out, info, handle = renderer.submit(preds[i], image, mode, label_min_area)
            host = torch.empty(tuple(out.shape), dtype=torch.uint8, pin_memory=True)
            host.copy_(out, non_blocking=True)
            info_host = torch.empty((2,), dtype=torch.int32, pin_memory=True)
            info_host.copy_(info, non_blocking=True)
            event = torch.cuda.Event()
            event.record()
            if pending is not None:
                dropped += retire(*pending)
            pending = (i, host, info_host, handle, event)
        if pending is not None:
            dropped += retire(*pending)
        for job in jobs:
            job.result()
    if dropped:
        logger.info('%d labels beyond the %d of an image were not drawn', dropped, MAX_LABELS)
    logger.info('%d panoptic pictures (%s) written to %s', n, mode, os.path.abspath(os.path.join(output_dir, FOLDERS[mode])))
    return paths
