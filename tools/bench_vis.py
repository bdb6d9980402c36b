"""Detection visualisations on the device (dataset/vis.py, csrc/vis_render.hip): device time per image of the render entry point
(GPU events around each upsnet_vis_render call on device-resident inputs, warm, the median of --reps calls) at 1024 x 2048 with 30 and
100 detections and at 800 x 1333 with 100; the bytes the call must move at least (the canvas read and written once, plus the mask bits
of the pixels inside masks' extents read once) over that time; render_detections with its upload (host wall time around a
synchronise); the numpy restatement of the rule (tests/vis_ref.py) on the same input on the host; and vis_all_mask end to end (decode,
draw, PNG write) per image on a generated image list. Prints one JSON line.

    python tools/bench_vis.py [--reps 30] [--no-numpy] [--forward-ms <ms_per_img_serial of bench.py at 1024 x 2048, same visit>]
    rocprofv3 --kernel-trace --stats -d <dir> -o vis -- python tools/bench_vis.py --trace-run     (per-kernel times)
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

CONFIGS = ((1024, 2048, 30), (1024, 2048, 100), (800, 1333, 100))


def scene(H, W, n, seed=0):
    """A street-like scene: n boxes of gen_dets with an ellipse mask inside each."""
    from conftest import gen_dets
    rng = np.random.default_rng(seed)
    image = rng.integers(0, 256, (H, W, 3)).astype(np.uint8)
    dets = gen_dets(rng, n, H, W)
    dets[:, 4] = np.maximum(dets[:, 4], np.float32(0.5))
    masks = []
    for d in range(n):
        x1, y1, x2, y2 = dets[d, :4]
        m = np.zeros((H, W), bool)
        ya, yb, xa, xb = int(max(0, y1)), int(min(H, y2 + 1)), int(max(0, x1)), int(min(W, x2 + 1))
        if yb > ya and xb > xa:
            yy, xx = np.mgrid[ya:yb, xa:xb]
            m[ya:yb, xa:xb] = ((xx - (x1 + x2) / 2) / max(1.0, (x2 - x1) / 2)) ** 2 + ((yy - (y1 + y2) / 2) / max(1.0, (y2 - y1) / 2)) ** 2 <= 1.0
        masks.append(m)
    labels = ['car' + ('%.2f' % float(s)).lstrip('0') for s in dets[:, 4]]
    colours = rng.integers(0, 256, (n, 3)).astype(np.uint8)
    return image, dets[:, :4].astype(np.float32), labels, colours, masks


def device_call(image, boxes, labels, colours, trans, off):
    """The entry point on device-resident inputs: returns (call, out)."""
    from upsnet_amd._lib import check, lib, ptr, stream
    from upsnet_amd.dataset import vis
    H, W, n = image.shape[0], image.shape[1], boxes.shape[0]
    lb, ln = vis._label_bytes(labels)
    dev = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (image, boxes, colours, lb, ln, trans, off.astype(np.int32))]
    out = torch.empty((H, W, 3), dtype=torch.uint8, device='cuda')
    ws = torch.empty((int(lib().upsnet_vis_workspace_bytes(n, H, W)),), dtype=torch.uint8, device='cuda')

    def call():
        check(lib().upsnet_vis_render(stream(), ptr(dev[0]), H, W, n, ptr(dev[1]), ptr(dev[2]), ptr(dev[3]), ptr(dev[4]), ptr(dev[5]), ptr(dev[6]),
                                      int(trans.size), ptr(ws), ptr(out)), 'vis_render')
    return call, out


def event_times_us(call, reps, warmup=5):
    for _ in range(warmup):
        call()
    torch.cuda.synchronize()
    pairs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for e0, e1 in pairs:
        e0.record()
        call()
        e1.record()
    torch.cuda.synchronize()
    return sorted(1e3 * e0.elapsed_time(e1) for e0, e1 in pairs)


def end_to_end(n_images, H, W, n_dets):
    """vis_all_mask on a generated Cityscapes-layout image list with n_dets detections per image: seconds per image."""
    import vis_ref
    from test_dataset_run_cpu import make_dataset, write_cfg
    from upsnet_amd.config.config import update_config
    from upsnet_amd.dataset import Cityscapes
    from upsnet_amd.dataset.rle import counts_from_transitions, rle_to_string
    import pathlib
    with tempfile.TemporaryDirectory() as tmp:
        root = os.path.join(tmp, 'cs')
        make_dataset(root, 'Cityscapes', [(H, W)] * n_images, seed=3)
        update_config(write_cfg(pathlib.Path(tmp), 'Cityscapes', root, 'val'))
        ds = Cityscapes(image_sets=['val'], phase='test')
        all_boxes, all_masks = [[] for _ in range(9)], [[] for _ in range(9)]
        _, boxes, _, _, masks = scene(H, W, n_dets, seed=9)
        rles = [{'size': [H, W], 'counts': rle_to_string(counts_from_transitions(vis_ref.mask_transitions(m), H * W))} for m in masks]
        per = np.array_split(np.arange(n_dets), 8)
        for c in range(1, 9):
            b = np.hstack([boxes[per[c - 1]], np.full((len(per[c - 1]), 1), 0.9, np.float32)]).astype(np.float32)
            all_boxes[c] = [b] * n_images
            all_masks[c] = [[rles[k] for k in per[c - 1]]] * n_images
        ds.vis_all_mask(all_boxes, all_masks, os.path.join(tmp, 'warm'))
        t0 = time.perf_counter()
        files = ds.vis_all_mask(all_boxes, all_masks, os.path.join(tmp, 'vis'))
        return (time.perf_counter() - t0) / len(files)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--no-numpy', action='store_true')
    ap.add_argument('--no-end-to-end', action='store_true')
    ap.add_argument('--forward-ms', type=float, default=None, help='ms_per_img_serial of bench.py at 1024 x 2048 from the same visit')
    ap.add_argument('--trace-run', action='store_true', help='20 renders of the 1024 x 2048, 100 detection scene and nothing else')
    args = ap.parse_args()
    import vis_cases
    import vis_ref
    from upsnet_amd.dataset import vis
    out = {'reps': max(20, args.reps), 'configs': []}
    for H, W, n in CONFIGS:
        image, boxes, labels, colours, masks = scene(H, W, n)
        trans, off = vis_cases.scene_transitions(masks, H, W)
        call, d_out = device_call(image, boxes, labels, colours, trans, off)
        if args.trace_run:
            if (H, W, n) == CONFIGS[1]:
                for _ in range(20):
                    call()
                torch.cuda.synchronize()
            continue
        us = event_times_us(call, max(20, args.reps))
        # the least traffic: canvas in + out, and one bit per pixel of every mask's bounding box
        box_bits = sum(int(np.ptp(np.flatnonzero(m.any(0))) + 1) * int(np.ptp(np.flatnonzero(m.any(1))) + 1) for m in masks if m.any())
        min_bytes = 2 * 3 * H * W + box_bits // 8
        row = {'height': H, 'width': W, 'detections': n, 'run_boundaries': int(trans.size), 'render_us_p50': round(us[len(us) // 2], 1),
               'render_us_min': round(us[0], 1), 'render_us_max': round(us[-1], 1), 'min_bytes': min_bytes,
               'min_bytes_over_p50_TBps': round(min_bytes / (us[len(us) // 2] * 1e-6) / 1e12, 3),
               'share_of_8TBps': round(min_bytes / (us[len(us) // 2] * 1e-6) / 8e12, 4)}
        d_image = torch.from_numpy(image).cuda()
        times = []
        for _ in range(8):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            vis.render_detections(d_image, boxes, labels, colours, trans, off)
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
        row['render_detections_wall_us_p50'] = round(1e6 * float(np.median(times[2:])), 1)
        if not args.no_numpy:
            t0 = time.perf_counter()
            want = vis_ref.render(image, boxes, labels, colours, masks, vis.font_table())
            row['numpy_ms'] = round(1e3 * (time.perf_counter() - t0), 1)
            row['equal_to_numpy'] = bool(np.array_equal(d_out.cpu().numpy(), want))
        if args.forward_ms is not None and (H, W) == (1024, 2048):
            row['forward_ms_per_img_serial'] = args.forward_ms
            row['render_over_forward'] = round(row['render_us_p50'] / 1e3 / args.forward_ms, 4)
        out['configs'].append(row)
    if args.trace_run:
        return
    if not args.no_end_to_end:
        out['vis_all_mask_s_per_image_1024x2048_30det'] = round(end_to_end(8, 1024, 2048, 30), 4)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
