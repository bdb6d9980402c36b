#!/usr/bin/env python
"""Time proposal recall (ProposalRecallEvaluator, csrc/prop_eval.hip) on COCO-like images: 1000 proposals per image (boxes drawn as
tests/conftest.gen_rois draws them, half of them jittered copies of GT boxes), G heavy-tailed up to 90 GT boxes, 4 areas x 3 limits
(AR@100 / 300 / 1000 for all, small, medium and large).

    python tools/bench_proposal_eval.py [--images 500] [--restate 20] [--out results/bench_proposal_eval.json]

Reports: device time per image (events around back-to-back add()s plus a final synchronise), the summary() time, and the numpy
restatement of tests/proposal_recall_ref.py on one core, per image. Kernel times: run under
`rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bench_proposal_eval.py --images 50` in a separate run (prop_recall_kernel).
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

H, W, P, GMAX = 640, 640, 1000, 90
AREAS, LIMITS = ['all', 'small', 'medium', 'large'], [100, 300, 1000]


def boxes(rng, n, smin=8, smax=500):
    size = np.exp(rng.uniform(np.log(smin), np.log(smax), n))
    ar = np.exp(rng.uniform(np.log(0.5), np.log(2.0), n))
    w, h = size * np.sqrt(ar), size / np.sqrt(ar)
    cx, cy = rng.uniform(0, W, n), rng.uniform(0, H, n)
    b = np.stack([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2], 1)
    b[:, 0::2] = np.clip(b[:, 0::2], 0, W - 1)
    b[:, 1::2] = np.clip(b[:, 1::2], 0, H - 1)
    return b.astype(np.float32)


def image(rng):
    G = int(min(GMAX, max(1, np.floor(rng.pareto(1.2) * 4 + 1))))
    gt = boxes(rng, G)
    props = boxes(rng, P)
    src = rng.integers(0, G, P // 2)
    props[:P // 2] = gt[src] + rng.normal(0, 8, (P // 2, 4)).astype(np.float32)
    props = props[rng.permutation(P)]
    areas = ((gt[:, 2] - gt[:, 0] + 1) * (gt[:, 3] - gt[:, 1] + 1) * rng.uniform(0.4, 0.9, G)).astype(np.float32)
    return props, gt, np.ones(G, np.int32), rng.random(G) < 0.05, areas


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--images', type=int, default=500)
    ap.add_argument('--restate', type=int, default=20, help='images timed for the numpy restatement (0: skip)')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    from upsnet_amd.dataset.proposal_eval import ProposalRecallEvaluator
    rng = np.random.default_rng(0)
    imgs = [image(rng) for _ in range(args.images)]
    # warm-up (library load, allocator, pinned pool)
    ev = ProposalRecallEvaluator(AREAS, LIMITS)
    for im in imgs[:5]:
        ev.add(*im)
    ev.summary()
    torch.cuda.synchronize()
    ev = ProposalRecallEvaluator(AREAS, LIMITS)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    for im in imgs:
        ev.add(*im)
    e1.record()
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    summ = ev.summary()
    t2 = time.perf_counter()
    res = {'images': args.images, 'proposals_per_image': P, 'mean_gt': float(np.mean([len(im[1]) for im in imgs])),
           'max_gt': int(max(len(im[1]) for im in imgs)), 'device_ms_per_image': e0.elapsed_time(e1) / args.images,
           'wall_ms_per_image': 1e3 * (t1 - t0) / args.images, 'summary_ms': 1e3 * (t2 - t1),
           'AR@100': float(summ[('all', 100)]['ar']), 'AR@1000': float(summ[('all', 1000)]['ar'])}
    if args.restate:
        import proposal_recall_ref as prr
        n = min(args.restate, args.images)
        roidb = [prr.roidb_entry(*im) for im in imgs[:n]]
        t0 = time.perf_counter()
        for area in AREAS:
            for lim in LIMITS:
                prr.evaluate_box_proposals(roidb, None, area, lim)
        res['numpy_ms_per_image'] = 1e3 * (time.perf_counter() - t0) / n
        res['numpy_images'] = n
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(args.out) or '.', exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
