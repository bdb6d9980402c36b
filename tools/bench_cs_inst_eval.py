"""Cityscapes instance-level AP on the device (dataset/cityscapes_eval.py): microseconds per InstanceEvaluator.add_rle (both walks of
the id map) and add_masks at 1024x2048 with 100 predictions and about 60 GT regions (GPU events over back-to-back images after a
warm-up, and the host's wall time per call with the share of the RLE decoding), accumulate, and the numpy restatement of the same rules
on full boolean masks (tests/cityscapes_inst_ref.py) on one core for comparison. Prints one JSON line.

    python tools/bench_cs_inst_eval.py [--reps 50] [--no-numpy]
    rocprofv3 --kernel-trace --stats -d <dir> -o cs -- python tools/bench_cs_inst_eval.py --trace-run     (per-kernel times)
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

H, W, N_PRED, N_REGIONS = 1024, 2048, 100, 60


def image(seed=0):
    import cityscapes_inst_cases as cases
    rng = np.random.default_rng(seed)
    gt, preds = cases.make_image(rng, H, W, N_REGIONS)
    preds = [p for p in preds if p['mask'].any()]
    while len(preds) < N_PRED:
        p = preds[int(rng.integers(0, len(preds)))]
        preds.append(dict(p, conf=np.float32(rng.integers(1, 17) / 16.0)))
    return gt, preds[:N_PRED]


def timed(fn, reps, warmup=5):
    for _ in range(warmup):
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
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--no-numpy', action='store_true')
    ap.add_argument('--trace-run', action='store_true', help='10 images through each path and nothing else (to be run under a profiler)')
    args = ap.parse_args()
    import cityscapes_inst_cases as cases
    from upsnet_amd.dataset import cityscapes_eval as ce
    from upsnet_amd.dataset.rle import rle_to_string
    gt, preds = image()
    dets, rles, _ = cases.per_class_results(preds, rle_to_string)
    gt_dev = torch.from_numpy(gt).cuda()
    masks = torch.from_numpy(np.stack([p['mask'] for p in preds]).astype(np.uint8)).cuda()
    scores = torch.from_numpy(np.array([p['conf'] for p in preds], np.float32)).cuda()
    classes = np.array([p['cls'] for p in preds], np.int64)
    evs = {w: ce.InstanceEvaluator(walk=w) for w in ('transposed', 'strided')}
    dense = ce.InstanceEvaluator()
    if args.trace_run:
        for _ in range(10):
            evs['transposed'].add_rle(gt_dev, dets, rles)
            evs['strided'].add_rle(gt_dev, dets, rles)
            dense.add_masks(gt_dev, masks, scores, classes)
        torch.cuda.synchronize()
        return
    out = {'height': H, 'width': W, 'predictions': len(preds), 'mask_pixels': int(sum(int(p['mask'].sum()) for p in preds)),
           'gt_regions': int(np.unique(gt).size), 'runs': int(sum(len(r['counts']) for c in rles for r in c))}
    for w, ev in evs.items():
        out['add_rle_%s_us' % w], out['add_rle_%s_host_us' % w] = timed(lambda: ev.add_rle(gt_dev, dets, rles), args.reps)
    out['add_rle_numpy_map_us'], out['add_rle_numpy_map_host_us'] = timed(lambda: evs['transposed'].add_rle(gt, dets, rles), args.reps)
    out['add_masks_us'], out['add_masks_host_us'] = timed(lambda: dense.add_masks(gt_dev, masks, scores, classes), args.reps)
    t0 = time.perf_counter()
    for _ in range(args.reps):
        for c in range(1, 9):
            if len(rles[c]):
                ce._transitions(rles[c], H, W)
    out['rle_decode_host_us'] = round((time.perf_counter() - t0) * 1e6 / args.reps, 1)
    times = []
    for _ in range(5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        evs['transposed'].accumulate()
        times.append(time.perf_counter() - t0)
    out['accumulate_ms'] = round(1e3 * float(np.median(times)), 2)
    out['accumulate_images'] = evs['transposed'].num_images
    if not args.no_numpy:
        import cityscapes_inst_ref as ref
        t0 = time.perf_counter()
        aps, _, _ = ref.evaluate([(gt, preds)])
        out['numpy_ms_per_image'] = round((time.perf_counter() - t0) * 1e3, 1)
        one = ce.InstanceEvaluator()
        one.add_rle(gt_dev, dets, rles)
        got = one.accumulate()
        out['equal_to_numpy'] = bool(np.array_equal(got, aps, equal_nan=True))
    print(json.dumps(out))


if __name__ == '__main__':
    main()
