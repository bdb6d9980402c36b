#!/usr/bin/env python
"""Time the Cityscapes instance prediction writer's parts for one 1024 x 2048 image of 100 masks (csrc/cs_inst_format.hip,
dataset/cityscapes_inst_format.py): the expand launch of both forms (GPU events around warm windows, no copy back), the copy of the
planes into pinned host memory (GPU events), the PNG encode of one mask on one host thread (PIL, both forms), and the yardstick: the
numpy restatement (tests/cityscapes_inst_format_ref.py: np.repeat, transpose, packbits) on one core for the same run lists.

    python tools/bench_cs_inst_format.py [--masks 100] [--out profiles/cs_inst_format.txt]

GB/s = output bytes of the launch over its time (the run lists are a few hundred KB and stay in cache). Per-kernel times: run it under
a kernel trace of its own, with a smaller --windows (tracing slows the host)."""
import argparse
import io
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def gpu_window(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--masks", type=int, default=100)
    ap.add_argument("--height", type=int, default=1024)
    ap.add_argument("--width", type=int, default=2048)
    ap.add_argument("--calls", type=int, default=50, help="launches per timed window")
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--encode-masks", type=int, default=8)
    ap.add_argument("--numpy-masks", type=int, default=8)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_cs_inst_format.py measures the device path: it needs a GPU"
    from PIL import Image
    import cityscapes_inst_format_ref as ref
    from upsnet_amd import build
    from upsnet_amd.dataset import cityscapes_inst_format as cif
    H, W, n = a.height, a.width, a.masks
    rng = np.random.default_rng(0)
    counts = [ref.blob_counts(rng, H, W) for _ in range(n)]
    trans, off = ref.runs_of_counts(counts)
    cif.check_runs(trans, off, H, W)
    d_trans, d_off = torch.from_numpy(trans).cuda(), torch.from_numpy(off).cuda()
    res = {'what': 'expand / copy / PNG encode of one image\'s masks', 'H': H, 'W': W, 'masks': n, 'transitions': int(trans.size),
           'device': torch.cuda.get_device_name(0), 'srchash': build._source_hash(), 'calls_per_window': a.calls}
    planes = {}
    for one_bit in (False, True):
        key = '1bit' if one_bit else '8bit'
        nbytes = n * cif.plane_bytes(H, W, one_bit)
        out = torch.empty((n, H, nbytes // (n * H)), dtype=torch.uint8, device='cuda')
        host = torch.empty(out.shape, dtype=torch.uint8, pin_memory=True)

        def launch():
            cif._expand_into(d_trans, d_off, n, H, W, one_bit, out, cif.MAX_LAUNCH_BYTES)
        launch()
        us = sorted(gpu_window(launch, a.calls) for _ in range(a.windows))
        copy_us = sorted(gpu_window(lambda: host.copy_(out, non_blocking=True), max(1, a.calls // 5)) for _ in range(a.windows))
        torch.cuda.synchronize()
        planes[key] = host.numpy().copy()
        res['expand_%s_us' % key] = round(us[len(us) // 2], 2)
        res['expand_%s_us_reps' % key] = [round(v, 2) for v in us]
        res['expand_%s_output_bytes' % key] = nbytes
        res['expand_%s_output_GBps' % key] = round(nbytes / us[len(us) // 2] * 1e-3, 1)
        res['copy_to_pinned_%s_us' % key] = round(copy_us[len(copy_us) // 2], 1)
        t_enc, size = [], 0
        for k in range(min(a.encode_masks, n)):
            t0 = time.perf_counter()
            buf = io.BytesIO()
            if one_bit:
                Image.frombytes('1', (W, H), planes[key][k].tobytes()).save(buf, format='PNG')
            else:
                Image.fromarray(planes[key][k]).save(buf, format='PNG')
            t_enc.append((time.perf_counter() - t0) * 1e6)
            size += buf.tell()
        res['png_encode_%s_us_per_mask_one_thread' % key] = round(float(np.median(t_enc)), 1)
        res['png_%s_bytes_per_mask' % key] = size // max(1, len(t_enc))
    t_np, same = [], True
    for k in range(min(a.numpy_masks, n)):
        t0 = time.perf_counter()
        m = ref.mask_from_counts(counts[k], H, W)
        p8, p1 = ref.plane_8bit(m), ref.plane_1bit(m)
        t_np.append((time.perf_counter() - t0) * 1e6)
        same = same and np.array_equal(p8, planes['8bit'][k]) and np.array_equal(p1, planes['1bit'][k])
    res['numpy_restatement_us_per_mask_one_core'] = round(float(np.median(t_np)), 1)
    res['matches_restatement'] = bool(same)
    text = json.dumps(res, indent=1)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write("# tools/bench_cs_inst_format.py on %s; library source hash %s\n%s\n" % (res['device'], res['srchash'], text))


if __name__ == "__main__":
    main()
