#!/usr/bin/env python
"""Time the COCO panoptic format per 1024 x 2048 image of about 120 segments (csrc/pan_format.hip, dataset/pan_format.py):
panoptic_format's device work (GPU events around a warm window, no copy back), the whole call with its one copy back and the host
part that builds segments_info (wall clock, synchronised), the relabel of add_png (GPU events), and the PNG encode of one image on one
host thread (PIL, the pan and the pan_2ch file). The yardstick is the numpy restatement of the reference's converter
(tests/pan_format_ref.py) on one core over the same maps. Prints one JSON line.

    python tools/bench_pan_format.py [--images 200] [--segments 120] [--out results/bench_pan_format.json]

Per-kernel times: run it under a kernel trace of its own, with fewer images (tracing slows the host).
"""
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
sys.path.insert(0, os.path.join(ROOT, "tools"))


def gpu_window(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for i in range(n):
        fn(i)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=200)
    ap.add_argument("--distinct", type=int, default=8, help="distinct seeded maps cycled through")
    ap.add_argument("--segments", type=int, default=120)
    ap.add_argument("--height", type=int, default=1024)
    ap.add_argument("--width", type=int, default=2048)
    ap.add_argument("--numpy-images", type=int, default=4)
    ap.add_argument("--encode-images", type=int, default=4)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_pan_format.py measures the device path: it needs a GPU"
    from PIL import Image
    from bench_pq import make_maps
    from pan_format_ref import convert_2ch
    from upsnet_amd._lib import check, lib, ptr, stream
    from upsnet_amd.dataset.pan_format import ColorGenerator, PanopticFormatter, relabel, segments_table
    rng = np.random.default_rng(0)
    cats = {c: {'id': c, 'isthing': int(c >= 11)} for c in range(19)}
    maps = [make_maps(rng, a.height, a.width, a.segments)[0] for _ in range(a.distinct)]
    dev = [torch.from_numpy(p).cuda() for p in maps]
    H, W = a.height, a.width

    fmt = PanopticFormatter(cats, device='cuda')
    outs = [fmt.finish(fmt.submit(d)) for d in dev]                       # warm-up; also the outputs checked below
    st = fmt._state
    rgb = torch.empty((H, W, 3), dtype=torch.uint8, device='cuda')
    table = torch.empty((int(lib().upsnet_pan_format_table_ints()),), dtype=torch.int32, device='cuda')

    def launches(i):
        check(lib().upsnet_pan_format(stream(), ptr(dev[i % len(dev)]), H, W, ptr(st['cat_table']), ptr(st['ws']), ptr(rgb), ptr(table)),
              "pan_format")
    launches(0)
    device_us = sorted(gpu_window(launches, a.images) for _ in range(3))

    whole = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(a.images):
            fmt.finish(fmt.submit(dev[i % len(dev)]))
        whole.append((time.perf_counter() - t0) * 1e6 / a.images)
    t0 = time.perf_counter()
    handles = [fmt.submit(d) for d in dev]
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    for h in handles:
        fmt.finish(h)
    host_us = (time.perf_counter() - t1) * 1e6 / len(dev)                # segments_info from the pinned table, nothing to wait for

    tables = [segments_table(info) for _, _, info in outs]
    rgbs = [r.clone() for r, _, _ in outs]
    status = torch.zeros(2, dtype=torch.int64, device='cuda')
    dtab = [torch.from_numpy(t).cuda() for t in tables]
    out2 = torch.empty((H, W, 3), dtype=torch.uint8, device='cuda')
    counts = torch.zeros((4096,), dtype=torch.int32, device='cuda')

    def relabel_launch(i):
        k = i % len(dev)
        check(lib().upsnet_pan_relabel(stream(), ptr(rgbs[k]), H, W, ptr(dtab[k]), int(tables[k].shape[0]), 0, ptr(out2), ptr(counts),
                                       ptr(status)), "pan_relabel")
    relabel_launch(0)
    relabel_us = sorted(gpu_window(relabel_launch, a.images) for _ in range(3))
    back, _ = relabel(rgbs[0], tables[0], 0, status)
    keep = maps[0][..., 0] != 255
    relabel_ok = bool(np.array_equal(back.cpu().numpy()[..., 0][keep], maps[0][..., 0][keep])) and status.cpu().tolist() == [0, 0]

    t_np, same = [], True
    for i in range(a.numpy_images):
        k = i % len(maps)
        t0 = time.perf_counter()
        want_rgb, want_info = convert_2ch(maps[k], ColorGenerator(cats).get_color)
        t_np.append((time.perf_counter() - t0) * 1e6)
        same = same and np.array_equal(outs[k][1], want_rgb) and outs[k][2] == want_info

    t_enc, png_bytes = [], []
    for i in range(a.encode_images):
        k = i % len(maps)
        t0 = time.perf_counter()
        size = 0
        for arr in (outs[k][1], maps[k]):
            buf = io.BytesIO()
            Image.fromarray(arr).save(buf, format='PNG')
            size += buf.tell()
        t_enc.append((time.perf_counter() - t0) * 1e6)
        png_bytes.append(size)

    res = {'what': 'panoptic_format / relabel / PNG encode per image', 'H': H, 'W': W, 'segments': int(np.mean([len(o[2]) for o in outs])),
           'images': a.images, 'format_device_us': round(device_us[1], 2), 'format_device_us_reps': [round(v, 2) for v in device_us],
           'format_call_us_synchronised': round(sorted(whole)[1], 1), 'format_host_us_segments_info': round(host_us, 1),
           'relabel_device_us': round(relabel_us[1], 2), 'relabel_device_us_reps': [round(v, 2) for v in relabel_us],
           'png_encode_us_one_thread': round(float(np.median(t_enc)), 1), 'png_bytes_per_image': int(np.mean(png_bytes)),
           'numpy_converter_us_one_core': round(float(np.median(t_np)), 1),
           'bytes_per_format': 9 * H * W, 'bytes_per_relabel': 6 * H * W,
           'matches_restatement': bool(same), 'relabel_round_trip': relabel_ok}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
