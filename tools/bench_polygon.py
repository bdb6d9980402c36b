"""Polygon GT rasterisation on the device (dataset/polygon.py, csrc/poly_raster.hip) on the real-size fixture of
tests/test_polygon_gpu.py: a 1024x2048 image with 60 Cityscapes-like contours of 500 to 5000 vertices. Device microseconds per image
of rasterize_polygons (GPU events over a warm window; host microseconds per call beside them), of DetectionEvaluator.add ('segm', 100
detections) fed the views of that image, i.e. upsnet_det_eval_image's own time for the same image, and the seconds the CPU
restatement (tests/polygon_ref.py) takes for it on one core. Prints one JSON line.

    python tools/bench_polygon.py [--reps 30]
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


def window(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    host = time.perf_counter() - t0
    torch.cuda.synchronize()
    return round(e0.elapsed_time(e1) * 1000 / reps, 1), round(host * 1e6 / reps, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=30)
    args = ap.parse_args()
    import polygon_ref as R
    from test_polygon_gpu import real_size_objects
    from upsnet_amd.dataset.coco_eval import DetectionEvaluator
    from upsnet_amd.dataset.polygon import pack_polygons, rasterize_polygons
    H, W = 1024, 2048
    objects = real_size_objects()
    verts, _, _, points = pack_polygons(objects)
    out = {'objects': len(objects), 'vertices': len(verts), 'edge_walk_points': points}
    out['raster_us'], out['raster_host_us'] = window(lambda: rasterize_polygons(objects, H, W), args.reps)
    rasters = rasterize_polygons(objects, H, W)
    lists = rasters.transitions()
    out['positions'] = int(sum(len(t) for t in lists))

    # the evaluator's own work for this image: GT = the views, 100 detections around the contours' boxes
    rng = np.random.default_rng(0)
    gts, boxes = [], np.zeros((100, 4), np.float32)
    for g, polys in enumerate(objects):
        p = np.asarray(polys[0]).reshape(-1, 2)
        x0, y0 = np.clip(p.min(0), 0, [W - 1, H - 1])
        x1, y1 = np.clip(p.max(0), 0, [W - 1, H - 1])
        gts.append({'id': g + 1, 'category_id': CATS[g % len(CATS)], 'iscrowd': 0, 'bbox': [x0, y0, x1 - x0, y1 - y0],
                    'area': float((x1 - x0) * (y1 - y0)), 'segmentation': rasters[g]})
    for d in range(100):
        x, y, w, h = gts[d % len(gts)]['bbox']
        j = rng.normal(0, 0.05, 4) * np.array([w, h, w, h])
        boxes[d] = [x + j[0], y + j[1], x + w - 1 + j[2], y + h - 1 + j[3]]
    boxes[:, 0::2] = np.clip(boxes[:, 0::2], 0, W - 1)
    boxes[:, 1::2] = np.clip(boxes[:, 1::2], 0, H - 1)
    cls = np.array([1 + (d % len(gts)) % len(CATS) for d in range(100)], np.int64)
    tb, tc = torch.from_numpy(boxes).cuda(), torch.from_numpy(cls).cuda()
    ts, tm = torch.from_numpy(rng.random(100).astype(np.float32)).cuda(), torch.from_numpy(rng.random((100, 1, 28, 28)).astype(np.float32)).cuda()
    ev = DetectionEvaluator(CATS, 'segm')
    ids = iter(range(1, 1 << 30))
    out['det_eval_add_us'], out['det_eval_add_host_us'] = window(lambda: ev.add(next(ids), gts, tb, ts, tc, tm, image_size=(H, W)), args.reps)

    t0 = time.perf_counter()
    want = [R.object_transitions(polys, H, W) for polys in objects]
    out['cpu_restatement_s'] = round(time.perf_counter() - t0, 2)
    out['equal'] = all(np.array_equal(a, np.asarray(b, np.int32)) for a, b in zip(lists, want))
    print(json.dumps(out))


if __name__ == '__main__':
    main()
