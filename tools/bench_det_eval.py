"""COCO box / mask / boundary AP on the device (dataset/coco_eval.py): microseconds per DetectionEvaluator.add at 1024x2048 with 100
dets and 30 GT (bbox, segm, and boundary on the segm scene at dilation ratios 0.02 and 0.005; GPU events over a warm window),
accumulate for 500 images x 8 categories, and the numpy restatements of the same rules (tests/test_coco_eval_cpu.py,
tests/boundary_ref.py) on one core for comparison. For the boundary kernel: the rectangle words of the scene's det and GT planes, the
bytes it must read and write for them and the time those take at 8 TB/s; its own time comes from a kernel trace of `--trace-run`
(boundary adds only), and `--boundary-kernel-us T` puts that figure and its share of the bound into the line. Prints one JSON line.

    python tools/bench_det_eval.py [--images 500] [--reps 50] [--boundary-kernel-us T]
    rocprofv3 --kernel-trace --stats -d <dir> -o det -- python tools/bench_det_eval.py --trace-run     (bnd_erode_kernel: 2 launches / add)
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

CATS = list(range(24, 32))


def image(rng, H, W, segm, n_det=100, n_gt=30):
    gts = []
    boxes = np.zeros((n_det, 4), np.float32)
    for g in range(n_gt):
        w, h = np.exp(rng.uniform(np.log(8), np.log(300), 2))
        x, y = rng.uniform(0, W - w - 1), rng.uniform(0, H - h - 1)
        el = {'id': g + 1, 'category_id': CATS[g % len(CATS)], 'iscrowd': int(g % 10 == 9), 'bbox': [x, y, w, h], 'area': w * h}
        if segm:
            m = np.zeros((H, W), bool)
            m[int(y):int(y + h), int(x):int(x + w)] = True
            el['_mask'] = m
        gts.append(el)
    for d in range(n_det):
        x, y, w, h = gts[d % n_gt]['bbox']
        j = rng.normal(0, 0.05, 4) * np.array([w, h, w, h])
        boxes[d] = [x + j[0], y + j[1], x + w - 1 + j[2], y + h - 1 + j[3]]
    boxes[:, 0::2] = np.clip(boxes[:, 0::2], 0, W - 1)
    boxes[:, 1::2] = np.clip(boxes[:, 1::2], 0, H - 1)
    cls = np.array([1 + (d % n_gt) % len(CATS) for d in range(n_det)], np.int64)
    return gts, boxes, rng.random(n_det).astype(np.float32), cls, rng.random((n_det, 1, 28, 28)).astype(np.float32)


def to_rle(gts):
    from test_coco_eval_gpu import rle_of
    return [dict({k: v for k, v in g.items() if k != '_mask'}, segmentation=rle_of(g['_mask'])) if '_mask' in g else g for g in gts]


def rect_words(boxes, gts, H, W, ms=28):
    """The words of the planes' rectangles the boundary kernel reads and writes: a det's is its pasted box (expand_boxes in float32,
    truncated, clipped: csrc/impaste.h) by the words its rows touch, a run-length GT's its columns by all words of a column."""
    nw = (H + 63) // 64
    scale = np.float32((ms + 2.0) / ms)
    words = 0
    for b in boxes.astype(np.float32):
        wh, hh = (b[2] - b[0]) * np.float32(.5) * scale, (b[3] - b[1]) * np.float32(.5) * scale
        xc, yc = (b[2] + b[0]) * np.float32(.5), (b[3] + b[1]) * np.float32(.5)
        x0, x1 = max(int(xc - wh), 0), min(int(xc + wh) + 1, W)
        y0, y1 = max(int(yc - hh), 0), min(int(yc + hh) + 1, H)
        if x1 > x0 and y1 > y0:
            words += (x1 - x0) * (((y1 - 1) >> 6) + 1 - (y0 >> 6))
    for g in gts:
        cols = np.nonzero(g['_mask'].any(0))[0]
        if len(cols):
            words += (cols[-1] + 1 - cols[0]) * nw
    return int(words)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--images', type=int, default=500)
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--trace-run', action='store_true', help='boundary adds only (for a kernel trace); prints nothing')
    ap.add_argument('--boundary-kernel-us', type=float, default=None,
                    help="bnd_erode_kernel's time per add from a kernel trace of --trace-run (both launches)")
    args = ap.parse_args()
    from upsnet_amd.dataset.coco_eval import DetectionEvaluator
    from test_coco_eval_cpu import cocoeval_restated
    H, W = 1024, 2048
    rng = np.random.default_rng(0)
    out = {}
    scene = {}
    for iou_type in ('bbox', 'segm', 'boundary', 'boundary_r005'):
        segm = iou_type != 'bbox'
        if iou_type.startswith('boundary'):     # the segm scene again: the two figures come from the same call
            gts, boxes, scores, cls, masks = (scene[k] for k in ('gts', 'boxes', 'scores', 'cls', 'masks'))
        else:
            gts, boxes, scores, cls, masks = image(rng, H, W, segm)
            scene = dict(gts=gts, boxes=boxes, scores=scores, cls=cls, masks=masks)
        if args.trace_run and iou_type != 'boundary':
            continue
        gt_dev = to_rle(gts) if segm else gts
        tb, ts, tc, tm = (torch.from_numpy(a).cuda() for a in (boxes, scores, cls, masks))
        if iou_type.startswith('boundary'):
            ev = DetectionEvaluator(CATS, 'boundary', dilation_ratio=0.005 if iou_type.endswith('r005') else 0.02)
        else:
            ev = DetectionEvaluator(CATS, iou_type)
        for i in range(5):
            ev.add(i, gt_dev, tb, ts, tc, tm if segm else None, image_size=(H, W))
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        for i in range(args.reps):
            ev.add(100 + i, gt_dev, tb, ts, tc, tm if segm else None, image_size=(H, W))
        e1.record()
        torch.cuda.synchronize()
        out['add_%s_us' % iou_type] = round(e0.elapsed_time(e1) * 1000 / args.reps, 1)
        out['add_%s_host_us' % iou_type] = round((time.perf_counter() - t0) * 1e6 / args.reps, 1)
        if args.trace_run:
            return
        if iou_type.startswith('boundary'):
            if iou_type == 'boundary':
                # one core, masks decoded as for segm below (gts / dts of the segm leg)
                import boundary_ref
                t0 = time.perf_counter()
                boundary_ref.boundary_cocoeval([(1, np_gts, np_dts)], CATS)
                out['numpy_boundary_ms_per_image'] = round((time.perf_counter() - t0) * 1e3, 1)
                words = rect_words(boxes, gts, H, W)
                out['boundary_rect_words'] = words
                out['boundary_min_bytes'] = 16 * words                                   # every word read once and written once
                out['boundary_bound_us_at_8TBps'] = round(16 * words / 8e12 * 1e6, 2)
                if args.boundary_kernel_us is not None:
                    out['boundary_kernel_us'] = args.boundary_kernel_us
                    out['boundary_kernel_share_of_bound'] = round(16 * words / 8e12 * 1e6 / args.boundary_kernel_us, 4)
            continue
        # numpy restatement of one image on one core (segm: masks already decoded)
        dts = [{'category_id': CATS[int(c) - 1], 'score': float(s), 'bbox': [float(b[0]), float(b[1]), float(b[2]) - float(b[0]) + 1,
                                                                               float(b[3]) - float(b[1]) + 1]}
               for b, s, c in zip(boxes, scores, cls)]
        if segm:
            from upsnet_amd.dataset.rle import im_post
            from test_coco_eval_gpu import masks_from_rle
            ba, ma = [[] for _ in range(len(CATS) + 1)], [[] for _ in range(len(CATS) + 1)]
            im_post(ba, ma, ts, tb, tm, tc, len(CATS) + 1, (H, W))
            dts = [{'category_id': CATS[c - 1], 'score': float(row[4]), 'mask': masks_from_rle(r)}
                   for c in range(1, len(CATS) + 1) for row, r in zip(ba[c][0], ma[c][0])]
            gts = [dict(g, mask=g['_mask']) for g in gts]
            np_gts, np_dts = gts, dts
        t0 = time.perf_counter()
        cocoeval_restated([(1, gts, dts)], CATS, iou_type)
        out['numpy_%s_ms_per_image' % iou_type] = round((time.perf_counter() - t0) * 1e3, 1)
    # accumulate over images x categories (bbox records)
    ev = DetectionEvaluator(CATS, 'bbox')
    for i in range(args.images):
        gts, boxes, scores, cls, _ = image(rng, H, W, False)
        ev.add(i + 1, gts, torch.from_numpy(boxes).cuda(), torch.from_numpy(scores).cuda(), torch.from_numpy(cls).cuda())
    torch.cuda.synchronize()
    ev.accumulate()
    times = []
    for _ in range(5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ev.accumulate()
        times.append(time.perf_counter() - t0)
    out['accumulate_ms'] = round(1e3 * float(np.median(times)), 2)
    out['accumulate_images'] = args.images
    print(json.dumps(out))


if __name__ == '__main__':
    main()
