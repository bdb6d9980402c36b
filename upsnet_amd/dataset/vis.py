"""Detection visualisations on the device: the reference's vis_all_mask (upsnet/dataset/base_dataset.py:826-896, overridden with the
class palette in cityscapes.py:236-345; config.test.vis_mask) by the integer drawing rule of DESIGN.md section 4.13, rendered by
csrc/vis_render.hip.

The reference draws with matplotlib, cv2.findContours and pycocotools on the host; matplotlib's anti-aliased rasteriser is no parity
target. The rule here restates what is drawn, in which order and with which opacity, in integers (the kernel file's header has it in
full): per kept detection, in the reference's order, a 3-pixel green box ring at 1/2, the mask in the detection's colour at 1/2 and
its 4-neighbour boundary pixels in white at 1/2 on top; then per detection the label `name + '.87'` in a 5 x 7 dot font at scale 2 on
a green background at 2/5, its box's bottom-left pixel at (floor(x1), floor(y1) - 2).

`kept_detections` is the reference's iteration (classes ascending, stored row order, score < 0.5 skipped in float32, classes with an
empty mask list skipped). `coco_colour` is this project's own colour sequence for datasets without a palette: the reference cycles
Detectron's colour list, which is not copied; these colours are not a parity target. Refused with ValueError before any launch: more
than MAX_DETECTIONS kept detections in an image, a label of more than MAX_LABEL bytes, an RLE whose size is not the image's.
"""
import ctypes
import logging
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from .._lib import check, dense, lib, ptr, stream

logger = logging.getLogger(__name__)

MAX_DETECTIONS = 256          # per image (include/upsnet_hip.h: upsnet_vis_max_detections)
MAX_LABEL = 32                # bytes per label (upsnet_vis_max_label)
MAX_DECODE_THREADS = 8        # image decoder threads (never sized from the host's CPU count), as evaluate.MAX_DECODE_THREADS
MAX_ENCODE_THREADS = 8        # PNG encoder threads, as pan_format.MAX_ENCODE_THREADS
SCORE_THRESHOLD = np.float32(0.5)


def blend(dst, src, a, b):
    """(dst * (b - a) + src * a + b // 2) // b: the rule's only arithmetic (ints or integer arrays)."""
    return (dst * (b - a) + src * a + b // 2) // b


def format_label(name, score):
    """The reference's name + '{:0.2f}'.format(score).lstrip('0') on the float32 score: car.87, person1.00."""
    return name + ('%.2f' % float(np.float32(score))).lstrip('0')


def coco_colour(k):
    """Colour of the k-th kept detection of a run (k counts across the whole image list): the sequence ((97 k + 31) mod 256,
    (57 k + 113) mod 256, (181 k + 197) mod 256), lightened once as blend(c, 255, 2/5)."""
    k = int(k)
    return tuple(blend(c, 255, 2, 5) for c in ((97 * k + 31) % 256, (57 * k + 113) % 256, (181 * k + 197) % 256))


def font_table():
    """uint8 [95, 8]: the cells of characters 32..126, one byte per cell row, bit 4 = the leftmost of 5 dots (the library's table)."""
    cells = np.zeros((95, 8), np.uint8)
    check(lib().upsnet_vis_font(cells.ctypes.data_as(ctypes.c_void_p)), "vis_font")
    return cells


def load_image(path):
    """The photograph at `path` as RGB uint8 [H, W, 3] (json_dataset.imread_bgr's decoding, channels reversed)."""
    from .json_dataset import imread_bgr
    return np.ascontiguousarray(imread_bgr(path)[:, :, ::-1])


def kept_detections(all_boxes, all_masks, i, class_names):
    """The detections of image i that the reference draws, in its order: [(class index j, row k, box float32 [4], score float32,
    label str, RLE dict)]. class_names[j] is the name of class j; '__background__' is skipped."""
    kept = []
    for j, name in enumerate(class_names):
        if name == '__background__':
            continue
        boxes, segms = all_boxes[j][i], all_masks[j][i]
        if isinstance(segms, (list, tuple)) and len(segms) == 0:
            continue
        boxes = np.asarray(boxes)
        if len(segms) != boxes.shape[0]:
            raise ValueError("class %d, image %d: %d detections with %d masks" % (j, i, boxes.shape[0], len(segms)))
        for k in range(boxes.shape[0]):
            score = np.float32(boxes[k, -1])
            if score < SCORE_THRESHOLD:
                continue
            kept.append((j, k, boxes[k, :4].astype(np.float32), score, format_label(name, score), segms[k]))
    return kept


def rle_transitions(rles, height, width):
    """im_post's RLE dicts -> (trans int32, trans_off int32 [n + 1]) as the render call takes them; ValueError on a size other than
    (height, width) or counts that do not sum to height * width."""
    from .cityscapes_eval import _transitions
    if not rles:
        return np.zeros(0, np.int32), np.zeros(1, np.int32)
    trans, lens = _transitions(list(rles), int(height), int(width))
    return trans, np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)


def _label_bytes(labels):
    out = np.zeros((len(labels), MAX_LABEL), np.uint8)
    lens = np.zeros(len(labels), np.int32)
    for d, s in enumerate(labels):
        b = s if isinstance(s, bytes) else s.encode('utf-8')
        if len(b) > MAX_LABEL:
            raise ValueError("label %r has %d bytes: at most %d are drawn" % (s, len(b), MAX_LABEL))
        out[d, :len(b)] = np.frombuffer(b, np.uint8)
        lens[d] = len(b)
    return out, lens


def render_detections(image_rgb, boxes, labels, colours, trans, trans_off):
    """One image: image_rgb uint8 [H, W, 3] (a device tensor, or a numpy array that is uploaded), the n detections in drawing order:
    boxes float [n, 4], labels n str / bytes, colours uint8 [n, 3], masks as ascending column-major change positions trans (all lists
    one after the other) with trans_off int [n + 1]. Returns the picture, uint8 [H, W, 3] on the device. Everything small travels in
    one pinned upload; nothing is synchronised."""
    if isinstance(image_rgb, np.ndarray):
        image_rgb = torch.from_numpy(np.ascontiguousarray(image_rgb)).to(torch.device('cuda', torch.cuda.current_device()), non_blocking=True)
    if not isinstance(image_rgb, torch.Tensor) or image_rgb.dtype != torch.uint8 or image_rgb.dim() != 3 or image_rgb.shape[2] != 3:
        raise ValueError("image_rgb must be uint8 [H, W, 3], got %r" % (getattr(image_rgb, 'shape', type(image_rgb)),))
    if not image_rgb.is_cuda:
        raise RuntimeError("render_detections: the image must be on the device (there is no CPU fallback)")
    image_rgb = dense(image_rgb)
    dev = image_rgb.device
    H, W = int(image_rgb.shape[0]), int(image_rgb.shape[1])
    boxes = np.ascontiguousarray(np.asarray(boxes, np.float32).reshape(-1, 4))
    n = int(boxes.shape[0])
    colours = np.asarray(colours)
    if colours.size and (colours.min() < 0 or colours.max() > 255):
        raise ValueError("colours must lie in 0..255")
    colours = np.ascontiguousarray(colours.astype(np.uint8).reshape(-1, 3))
    label_bytes, label_len = _label_bytes(list(labels))
    trans = np.ascontiguousarray(np.asarray(trans, np.int32).reshape(-1))
    trans_off = np.ascontiguousarray(np.asarray(trans_off, np.int64).reshape(-1))
    if n > MAX_DETECTIONS:
        raise ValueError("%d detections in one image: at most %d are drawn" % (n, MAX_DETECTIONS))
    if colours.shape[0] != n or label_len.shape[0] != n or trans_off.shape[0] != n + 1:
        raise ValueError("%d boxes with %d colours, %d labels and %d mask offsets" % (n, colours.shape[0], label_len.shape[0], trans_off.shape[0]))
    if trans_off[0] != 0 or trans_off[-1] != trans.size or np.any(np.diff(trans_off) < 0):
        raise ValueError("trans_off must rise from 0 to the number of change positions (%d)" % trans.size)
    if trans.size and (trans.min() < 0 or trans.max() > H * W):
        raise ValueError("a change position lies outside the image of %d x %d" % (H, W))
    ws_bytes = int(lib().upsnet_vis_workspace_bytes(n, H, W))
    if ws_bytes == 0:
        raise ValueError("an image of %d x %d cannot be drawn: sides up to 32768 and at most 2^28 pixels" % (H, W))
    with torch.cuda.device(dev):
        out = torch.empty((H, W, 3), dtype=torch.uint8, device=dev)
        ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=dev)
        views = [None] * 6
        if n:
            # one pinned host buffer, one upload: the 4-byte items first, then the bytes; every part starts on a 16-byte boundary
            parts = [boxes.view(np.uint8).reshape(-1), label_len.view(np.uint8), trans_off.astype(np.int32).view(np.uint8), trans.view(np.uint8),
                     label_bytes.reshape(-1), colours.reshape(-1)]
            host = torch.empty((sum((p.size + 15) // 16 * 16 for p in parts) + 16,), dtype=torch.uint8, pin_memory=True)
            hn, o, spans = host.numpy(), 0, []
            for p in parts:
                hn[o:o + p.size] = p
                spans.append((o, max(p.size, 4)))
                o += (p.size + 15) // 16 * 16
            d = host.to(dev, non_blocking=True)
            kinds = (torch.float32, torch.int32, torch.int32, torch.int32, torch.uint8, torch.uint8)
            views = [d[a:a + b].view(k) for (a, b), k in zip(spans, kinds)]
        d_boxes, d_len, d_off, d_trans, d_labels, d_colours = views
        check(lib().upsnet_vis_render(stream(), ptr(image_rgb), H, W, n, ptr(d_boxes), ptr(d_colours), ptr(d_labels), ptr(d_len),
                                      ptr(d_trans) if trans.size else None, ptr(d_off), int(trans.size), ptr(ws), ptr(out)), "vis_render")
    return out


def render_kept(image_rgb, kept, colours):
    """render_detections for kept_detections' list and one colour per entry."""
    H, W = int(image_rgb.shape[0]), int(image_rgb.shape[1])
    if len(kept) > MAX_DETECTIONS:
        raise ValueError("%d detections at or above a score of 0.5 in one image: at most %d are drawn" % (len(kept), MAX_DETECTIONS))
    trans, trans_off = rle_transitions([e[5] for e in kept], H, W)
    boxes = np.stack([e[2] for e in kept]) if kept else np.zeros((0, 4), np.float32)
    return render_detections(image_rgb, boxes, [e[4] for e in kept], np.asarray(colours, np.int64).reshape(-1, 3), trans, trans_off)


def _save_png(array, path):
    from PIL import Image
    Image.fromarray(array).save(path)


def vis_all_mask(dataset, all_boxes, all_masks, class_names, colour_of, name_of, save_path=None):
    """The loop of the reference's vis_all_mask over dataset.roidb: image i is decoded (dataset.load_image, BGR -> RGB) on a bounded
    thread pool ahead of the device, drawn, copied back through pinned memory while image i + 1 is drawn, and its PNG written by a
    bounded pool to save_path / name_of(entry). colour_of(class index, running count of kept detections) -> (r, g, b). Returns the
    list of written paths, or with save_path None (the reference's plt.show()) the list of rendered uint8 [H, W, 3] arrays."""
    n = len(dataset.roidb)
    for j in range(1, len(class_names)):
        if len(all_boxes[j]) != n or len(all_masks[j]) != n:
            raise ValueError("class %d: results for %d images, the image list has %d" % (j, len(all_boxes[j]), n))
    if save_path is not None:
        os.makedirs(save_path, exist_ok=True)
    paths = [None if save_path is None else os.path.join(save_path, name_of(e)) for e in dataset.roidb]
    if save_path is not None and len(set(paths)) != len(paths):
        raise ValueError("two images share one output name under %s" % save_path)
    results = [None] * n
    workers = max(1, min(MAX_DECODE_THREADS, n))
    ahead = 2 * workers
    counter = 0
    dev = torch.device('cuda', torch.cuda.current_device())
    with ThreadPoolExecutor(max_workers=workers) as dec, ThreadPoolExecutor(max_workers=max(1, min(MAX_ENCODE_THREADS, n))) as enc:
        jobs = []

        def retire(i, host, event):
            event.synchronize()
            if save_path is None:
                results[i] = host.numpy()
            else:
                jobs.append(enc.submit(_save_png, host.numpy(), paths[i]))
                results[i] = paths[i]
                while len(jobs) > 4 * MAX_ENCODE_THREADS:      # bounds the pinned buffers waiting for an encoder
                    jobs.pop(0).result()

        decoded = {j: dec.submit(dataset.load_image, j) for j in range(min(ahead, n))}
        pending = None
        for i in range(n):
            if i + ahead < n:
                decoded[i + ahead] = dec.submit(dataset.load_image, i + ahead)
            rgb = np.ascontiguousarray(decoded.pop(i).result()[:, :, ::-1])
            kept = kept_detections(all_boxes, all_masks, i, class_names)
            colours = [colour_of(e[0], counter + m) for m, e in enumerate(kept)]
            counter += len(kept)
            out = render_kept(torch.from_numpy(rgb).pin_memory().to(dev, non_blocking=True), kept, colours)
            host = torch.empty(tuple(out.shape), dtype=torch.uint8, pin_memory=True)
            host.copy_(out, non_blocking=True)
            event = torch.cuda.Event()
            event.record()
            if pending is not None:
                retire(*pending)
            pending = (i, host, event)
        if pending is not None:
            retire(*pending)
        for job in jobs:
            job.result()
    if save_path is not None:
        logger.info('%d detection visualisations written to %s', n, os.path.abspath(save_path))
    return results
