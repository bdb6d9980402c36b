#!/usr/bin/env python
"""Time BaseDataset.get_combined_pan_result (csrc/pan_combine.hip) on 1024 x 2048 scenes with 100 detections of realistic box sizes
(log-uniform 16..700 px edges, rectangles and ellipses, scores uniform in 0.3..1, Cityscapes class counts).

    python tools/bench_pan_combined.py [--images 50] [--big 500] [--iters 5] [--restate 2] [--out results/bench_pan_combined.json]

Reports, per image: the host part of the call (validation, RLE decode, table upload and the launches: the call's time until it
returns, without a synchronise), the whole call (until a device synchronise), the same for one call of --big images (throughput),
and the numpy restatement of tests/test_pan_combined_cpu.py on one core. Kernel times: run under
`rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bench_pan_combined.py --iters 2 --big 0 --restate 0` in a separate run
(cpan_hist_kernel, cpan_greedy_kernel, cpan_merge_kernel).
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

H, W, NDET, NUM_CLASSES, ID_LAST_STUFF = 1024, 2048, 100, 9, 10


def rle_of_columns(y0, y1, h, w):
    """Column-major RLE string of a mask holding rows [y0[x], y1[x]) of every column x (empty where y1 <= y0)."""
    from upsnet_amd.dataset.rle import rle_to_string
    xs = np.flatnonzero(y1 > y0)
    if xs.size == 0:
        return {'size': [h, w], 'counts': rle_to_string([h * w])}
    a = xs * h + y0[xs]
    b = xs * h + y1[xs]
    # merge runs that touch across a column boundary
    keep = np.concatenate([[True], a[1:] != b[:-1]])
    starts = a[keep]
    ends = b[np.concatenate([keep[1:], [True]])]
    pos = np.stack([starts, ends], 1).reshape(-1)
    counts = np.diff(np.concatenate([[0], pos, [h * w]])).tolist()
    return {'size': [h, w], 'counts': rle_to_string(counts)}


def scene(rng):
    sem = rng.integers(0, ID_LAST_STUFF + NUM_CLASSES, (H // 32, W // 32)).repeat(32, 0).repeat(32, 1).astype(np.uint8)
    boxes = [[]] + [[np.zeros((0, 5), np.float32)] for _ in range(1, NUM_CLASSES)]
    masks = [[]] + [[[]] for _ in range(1, NUM_CLASSES)]
    xs = np.arange(W)
    for d in range(NDET):
        bh, bw = np.exp(rng.uniform(np.log(16), np.log(700), 2))
        cy, cx = rng.uniform(0, H), rng.uniform(0, W)
        if d % 2:
            t = np.clip(1 - ((xs - cx) / (bw / 2)) ** 2, 0, None)
            half = np.where(np.abs(xs - cx) <= bw / 2, np.sqrt(t) * bh / 2, -1)
            y0 = np.clip(np.ceil(cy - half), 0, H).astype(np.int64)
            y1 = np.clip(np.floor(cy + half) + 1, 0, H).astype(np.int64)
            y1 = np.where(half < 0, 0, y1)
        else:
            inside = (xs >= cx - bw / 2) & (xs < cx + bw / 2)
            y0 = np.full(W, int(np.clip(cy - bh / 2, 0, H)))
            y1 = np.where(inside, int(np.clip(cy + bh / 2, 0, H)), 0)
        c = int(rng.integers(1, NUM_CLASSES))
        box = [cx - bw / 2, cy - bh / 2, cx + bw / 2, cy + bh / 2, rng.uniform(0.3, 1.0)]
        boxes[c][0] = np.vstack([boxes[c][0], np.array([box], np.float32)])
        masks[c][0].append(rle_of_columns(y0, y1, H, W))
    return sem, boxes, masks


def batch(scenes, n):
    pick = [scenes[i % len(scenes)] for i in range(n)]
    return ([s[0] for s in pick], [[]] + [[s[1][c][0] for s in pick] for c in range(1, NUM_CLASSES)],
            [[]] + [[s[2][c][0] for s in pick] for c in range(1, NUM_CLASSES)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--images', type=int, default=50)
    ap.add_argument('--big', type=int, default=500)
    ap.add_argument('--iters', type=int, default=5)
    ap.add_argument('--restate', type=int, default=2)
    ap.add_argument('--out', default='', help='also write the result as JSON to this file')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_pan_combined: no GPU visible (there is no CPU path to time)')
    from upsnet_amd.config.config import config
    from upsnet_amd.dataset.base_dataset import BaseDataset
    config.dataset.num_classes, config.dataset.num_seg_classes = NUM_CLASSES, ID_LAST_STUFF + NUM_CLASSES
    rng = np.random.default_rng(0)
    scenes = [scene(rng) for _ in range(20)]
    ds = BaseDataset()
    res = {'height': H, 'width': W, 'detections': NDET}

    def timed(n, iters):
        segs, boxes, masks = batch(scenes, n)
        ds.get_combined_pan_result(segs, boxes, masks)       # warm-up (code objects, allocator)
        torch.cuda.synchronize()
        host, total = [], []
        for _ in range(iters):
            t0 = time.perf_counter()
            out = ds.get_combined_pan_result(segs, boxes, masks)
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            host.append(t1 - t0)
            total.append(t2 - t0)
            del out
        return 1e6 * float(np.median(host)) / n, 1e6 * float(np.median(total)) / n

    res['host_us_per_image'], res['call_us_per_image'] = timed(args.images, args.iters)
    res['images_per_call'] = args.images
    if args.big:
        res['big_host_us_per_image'], res['big_call_us_per_image'] = timed(args.big, max(1, args.iters // 2))
        res['big_images'] = args.big
        res['big_images_per_s'] = 1e6 / res['big_call_us_per_image']
    if args.restate:
        sys.path.insert(0, os.path.join(ROOT, 'tests'))
        from test_pan_combined_cpu import restate_combined
        segs, boxes, masks = batch(scenes, args.restate)
        t0 = time.perf_counter()
        want = restate_combined(segs, boxes, masks)
        res['numpy_restatement_ms_per_image'] = 1e3 * (time.perf_counter() - t0) / args.restate
        got = [t.cpu().numpy() for t in ds.get_combined_pan_result(segs, boxes, masks)]
        res['bitwise_equal_to_restatement'] = all(np.array_equal(g, e) for g, e in zip(got, want))
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
