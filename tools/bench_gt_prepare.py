#!/usr/bin/env python
"""Time the ground-truth preparation per 1024 x 2048 Cityscapes-like image (csrc/gt_prepare.hip, ops.gt_prepare_launch): the device
work of one call (GPU events around a warm window, no copy back) against the numpy restatement (tests/gt_prepare_ref.py) on one core
over the same map, and the least bytes the passes move (the int32 map read once by the pixel pass, the two maps written, the boxes of
the instances read twice by the transition passes, the lists written) against that time and 8 TB/s. No threshold. Prints one JSON line.

    python tools/bench_gt_prepare.py [--calls 50] [--out results/bench_gt_prepare.json]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=50)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    from gt_prepare_cases import scene
    from gt_prepare_ref import reference
    from upsnet_amd import ops
    from upsnet_amd.dataset import gt_prepare as gtp
    from upsnet_amd.dataset.prepare import label_tables
    ids = scene()
    H, W = ids.shape
    tables = label_tables()
    t0 = time.perf_counter()
    _, _, rows, trans_off, trans = reference(ids, tables)
    numpy_ms = (time.perf_counter() - t0) * 1e3
    dev = torch.device('cuda')
    d_ids, d_tables = torch.from_numpy(ids).to(dev), torch.from_numpy(tables).to(dev)
    ws = ops.gt_prepare_workspace(dev)
    for _ in range(3):
        ops.gt_prepare_launch(d_ids, d_tables, workspace=ws)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(args.calls):
        out = ops.gt_prepare_launch(d_ids, d_tables, workspace=ws)
    e1.record()
    torch.cuda.synchronize()
    kernel_ms = e0.elapsed_time(e1) / args.calls
    gtp.gt_prepare_check(out[5].cpu().numpy(), out[2].shape[0], out[4].shape[0])
    inst = [r for r in rows.tolist() if r[0] >= 1000 and tables[2][r[1]] >= 0]
    box_pixels = sum((r[7] - r[5] + 1) * (r[8] - r[6] + 1) for r in inst)
    nbytes = H * W * (4 + 1 + 3) + 2 * 4 * box_pixels + 4 * len(trans)
    res = {'image': [H, W], 'segments': int(rows.shape[0]), 'instances': len(inst), 'transitions': int(len(trans)),
           'kernel_ms_per_image': round(kernel_ms, 4), 'numpy_ms_per_image': round(numpy_ms, 1),
           'speedup': round(numpy_ms / kernel_ms, 1), 'least_bytes': nbytes, 'box_pixels': box_pixels,
           'tb_per_s': round(nbytes / (kernel_ms * 1e-3) / 1e12, 4), 'fraction_of_8tbps': round(nbytes / (kernel_ms * 1e-3) / 8e12, 4)}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
