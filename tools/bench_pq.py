#!/usr/bin/env python
"""Time panoptic-quality accumulation per 1024 x 2048 image: PanopticEvaluator.add on the device (csrc/pq_eval.hip; GPU events around
a warm window of >= 100 images, one result read-back after it) and the numpy restatement of the PQ rules (tests/test_pq_cpu.py, the
same integer work the reference does with np.unique per image) on one core, over the same seeded maps. Prints one JSON line.
--boundary times PanopticEvaluator(boundary=True) (Boundary PQ, csrc/pq_boundary.hip) against tests/boundary_pq_ref.py instead, and
the boundary pass alone (dataset.boundary.panoptic_boundary: two launches) with the least bytes it must move over its time.

    python tools/bench_pq.py [--images 200] [--segments 120] [--boundary [--ratio 0.02]] [--void 0.02] [--out results/bench_pq.json]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))


def make_maps(rng, H, W, n_seg, n_cat=19, void=0.02):
    """A Cityscapes-sized scene: n_seg rectangular GT segments over stuff bands; the prediction is the GT shifted by a few pixels
    with `void` (2 %) VOID noise, segments keyed (category, instance)."""
    cell = np.repeat(np.sort(rng.integers(0, 11, W))[None, :], H, 0)   # stuff bands 0..10
    seg_cat = list(range(11))
    for j in range(n_seg - 11):
        h, w = int(rng.integers(16, H // 4)), int(rng.integers(16, W // 6))
        y, x = int(rng.integers(0, H - h)), int(rng.integers(0, W - w))
        cell[y:y + h, x:x + w] = len(seg_cat)
        seg_cat.append(int(rng.integers(11, n_cat)))
    seg_cat = np.array(seg_cat)
    K = len(seg_cat)
    ids = rng.choice(np.arange(1, 1 << 24), K, replace=False)
    gid = ids[cell]
    gid[rng.random((H, W)) < void] = 0
    inst = np.zeros(K, np.int64)
    for c in range(n_cat):
        sel = np.nonzero(seg_cat == c)[0]
        inst[sel] = 0 if c < 11 else np.arange(1, len(sel) + 1) % 256
    pcell = np.roll(cell, (2, -3), (0, 1))
    cat = seg_cat[pcell]
    cat[rng.random((H, W)) < void] = 255
    pred = np.stack([cat, inst[pcell], np.zeros_like(cat)], -1).astype(np.uint8)
    gt = np.stack([gid & 255, (gid >> 8) & 255, (gid >> 16) & 255], -1).astype(np.uint8)
    present, cnt = np.unique(cell[gid != 0], return_counts=True)
    area = np.zeros(K, np.int64)
    area[present] = cnt
    info = [{'id': int(ids[s]), 'category_id': int(seg_cat[s]), 'iscrowd': 0, 'area': int(area[s])} for s in range(K)]
    return pred, gt, info


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=200)
    ap.add_argument("--distinct", type=int, default=8, help="distinct seeded maps cycled through")
    ap.add_argument("--segments", type=int, default=120)
    ap.add_argument("--height", type=int, default=1024)
    ap.add_argument("--width", type=int, default=2048)
    ap.add_argument("--numpy-images", type=int, default=8)
    ap.add_argument("--boundary", action="store_true", help="time Boundary PQ (PanopticEvaluator(boundary=True)) and its boundary pass")
    ap.add_argument("--ratio", type=float, default=0.02, help="with --boundary: the dilation ratio")
    ap.add_argument("--void", type=float, default=0.02, help="fraction of VOID noise pixels in both maps")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_pq.py measures the device path: it needs a GPU"
    from upsnet_amd.dataset.pq import PanopticEvaluator
    from test_pq_cpu import pq_restated
    kw = {}
    if a.boundary:
        from boundary_pq_ref import boundary_pq_restated
        kw = dict(boundary=True, dilation_ratio=a.ratio)
        restated = lambda images, cats: boundary_pq_restated(images, cats, a.ratio)
    else:
        restated = pq_restated
    rng = np.random.default_rng(0)
    cats = {c: {'id': c, 'isthing': int(c >= 11)} for c in range(19)}
    maps = [make_maps(rng, a.height, a.width, a.segments, void=a.void) for _ in range(a.distinct)]
    dev = [(torch.from_numpy(p).cuda(), torch.from_numpy(g).cuda(), info) for p, g, info in maps]

    ev = PanopticEvaluator(cats, device='cuda', **kw)
    for i in range(20):   # warm-up: code objects, pinned-memory pool
        ev.add(*dev[i % len(dev)])
    ev.pq_stat()
    reps = []
    for _ in range(3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        for i in range(a.images):
            ev.add(*dev[i % len(dev)])
        e1.record()
        t_host = time.perf_counter() - t0
        torch.cuda.synchronize()
        reps.append((e0.elapsed_time(e1) * 1e3 / a.images, t_host * 1e6 / a.images))
    stat = ev.pq_stat()

    # the same maps through the numpy restatement, one image at a time on this core
    t0 = time.perf_counter()
    for i in range(a.numpy_images):
        restated([maps[i % len(maps)]], cats)
    t_np = (time.perf_counter() - t0) * 1e6 / a.numpy_images

    # exactness on the timed maps: device accumulators of one pass == the restatement
    chk = PanopticEvaluator(cats, device='cuda', **kw)
    for d in dev:
        chk.add(*d)
    tp, fp, fn, iou = restated(maps, cats)
    s = chk.pq_stat()
    same = all((s[c].tp, s[c].fp, s[c].fn, s[c].iou) == (int(tp[c]), int(fp[c]), int(fn[c]), float(iou[c])) for c in range(19))

    dev_us = sorted(r[0] for r in reps)
    res = {'what': 'PanopticEvaluator.add per image', 'H': a.height, 'W': a.width, 'gt_segments': a.segments, 'images': a.images,
           'device_us_per_image': round(dev_us[len(dev_us) // 2], 2), 'device_us_reps': [round(r[0], 2) for r in reps],
           'host_enqueue_us_per_image': round(sorted(r[1] for r in reps)[1], 2), 'numpy_us_per_image_one_core': round(t_np, 1),
           'speedup_vs_numpy': round(t_np / dev_us[len(dev_us) // 2], 1), 'bytes_read_per_image': 6 * a.height * a.width,
           'matches_restatement': bool(same), 'pq_all': stat.pq_average(cats, None)[0]['pq']}
    if a.boundary:
        from upsnet_amd.dataset.boundary import boundary_dilation, panoptic_boundary
        for i in range(10):
            panoptic_boundary(dev[i % len(dev)][0], dev[i % len(dev)][1], a.ratio)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for i in range(a.images):
            bits = panoptic_boundary(dev[i % len(dev)][0], dev[i % len(dev)][1], a.ratio)
        e1.record()
        torch.cuda.synchronize()
        pass_us = e0.elapsed_time(e1) * 1e3 / a.images
        least = 7 * a.height * a.width                     # two 3-byte maps read, one byte map written
        res.update({'what': 'PanopticEvaluator(boundary=True).add per image', 'ratio': a.ratio, 'void': a.void,
                    'dilation': boundary_dilation(a.height, a.width, a.ratio), 'boundary_pass_us_per_image': round(pass_us, 2),
                    'boundary_pass_least_bytes': least, 'boundary_pass_gb_per_s': round(least / pass_us / 1e3, 1),
                    'boundary_pixel_fraction': [round(float(((bits & b) != 0).float().mean()), 4) for b in (1, 2)]})
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
