"""Cityscapes pixel-level IoU / iIoU on the device (dataset/cityscapes_pixel_eval.py): microseconds per PixelEvaluator.add at
1024x2048 with about 60 ground-truth instances (GPU events over back-to-back images after a warm-up, and the host's wall time per
call), with device-resident maps, with host maps (the upload included) and without the instance-id map; accumulate; the bytes the
tile kernel reads (4 per pixel: two uint8 maps and the uint16 map); and the numpy restatement of the same rules on full maps
(tests/cityscapes_pixel_ref.py) on one core for comparison. Prints one JSON line.

    python tools/bench_cs_pixel_eval.py [--reps 200] [--no-numpy]
    rocprofv3 --kernel-trace --stats -d <dir> -o px -- python tools/bench_cs_pixel_eval.py --trace-run     (per-kernel times)
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

H, W, N_INST = 1024, 2048, 60


def timed(fn, reps, warmup=10):
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


def distinct_keys(labels, ids, pred):
    """Mean number of distinct (label, prediction, instance) keys among 64 pixels spaced 16 apart: the merge-loop trips of one wave
    per pixel step (sampled: every 37th stretch of 1024 pixels)."""
    n = labels.size // 1024 * 1024
    key = (labels.reshape(-1)[:n].astype(np.int64) << 32) | (pred.reshape(-1)[:n].astype(np.int64) << 16) | ids.reshape(-1)[:n]
    sample = key.reshape(-1, 64, 16)[::37]
    return round(float(np.mean([np.unique(sample[i, :, j]).size for i in range(sample.shape[0]) for j in range(16)])), 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=200)
    ap.add_argument('--no-numpy', action='store_true')
    ap.add_argument('--noise', action='store_true', help="the tests' image: a random label per pixel wherever the ground truth is an "
                    'ignored label (default: a piecewise constant prediction, as a network gives)')
    ap.add_argument('--trace-run', action='store_true', help='20 images through add and nothing else (to be run under a profiler)')
    args = ap.parse_args()
    import cityscapes_pixel_cases as cases
    from upsnet_amd.dataset import cityscapes_pixel_eval as pe
    labels, ids, pred = cases.make_image(np.random.default_rng(0), H, W, N_INST, train_ids=True, noise=args.noise)
    d_labels, d_ids, d_pred = (torch.from_numpy(a).cuda() for a in (labels, ids, pred))
    ev = pe.PixelEvaluator()
    if args.trace_run:
        for _ in range(20):
            ev.add(d_labels, d_ids, d_pred)
        torch.cuda.synchronize()
        return
    out = {'height': H, 'width': W, 'noise': bool(args.noise), 'distinct_keys_per_wave_step': distinct_keys(labels, ids, pred), 'instances': int(np.unique(ids[ids > 1000]).size), 'raw_values': int(np.unique(ids).size),
           'tile_kernel_bytes': 4 * H * W}
    out['add_us'], out['add_host_us'] = timed(lambda: ev.add(d_labels, d_ids, d_pred), args.reps)
    ev_no, ev_host = pe.PixelEvaluator(), pe.PixelEvaluator()
    out['add_no_ids_us'], out['add_no_ids_host_us'] = timed(lambda: ev_no.add(d_labels, None, d_pred), args.reps)
    out['add_numpy_maps_us'], out['add_numpy_maps_host_us'] = timed(lambda: ev_host.add(labels, ids, pred), max(10, args.reps // 4))
    times = []
    for _ in range(5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ev.accumulate()
        times.append(time.perf_counter() - t0)
    out['accumulate_ms'] = round(1e3 * float(np.median(times)), 2)
    out['accumulate_images'] = ev.num_images
    if not args.no_numpy:
        import cityscapes_pixel_ref as ref
        t0 = time.perf_counter()
        want = ref.evaluate([(labels, ids, cases.as_label_ids(pred, True))])
        out['numpy_ms_per_image'] = round((time.perf_counter() - t0) * 1e3, 1)
        one = pe.PixelEvaluator(avg_class_size=ref.AVG)
        one.add(d_labels, d_ids, d_pred)
        got = one.summary()
        out['equal_to_numpy'] = bool(np.array_equal(got['conf'], want['conf']) and got['IoU_class'] == want['averageScoreClasses']
                                     and got['iIoU_class'] == want['averageScoreInstClasses']
                                     and got['iIoU_category'] == want['averageScoreInstCategories'])
    print(json.dumps(out))


if __name__ == '__main__':
    main()
