"""Panoptic pictures on the device (dataset/pan_vis.py, csrc/pan_vis.hip): per mode (flat, overlay) and size
(1024 x 2048 and 800 x 1333, maps of about 120 segments) the device time of the entry point (GPU events around each upsnet_pan_vis
call on device-resident inputs, warm, the median of --reps calls, at least 20), the bytes the call must move at least (flat reads the
map and writes the picture: 3 + 3 bytes per pixel; overlay also reads the photograph and the id map: 9 + 3) over that time against the
6.3 TB/s an element-wise kernel reaches on this part (section 4.18), the numpy restatement of the rule (tests/pan_vis_ref.py) on the
same input on the host, and vis_panoptic end to end (decode, format, draw, copy back, PNG write) in seconds per image. Writes the
report to profiles/pan_vis.txt (--out) and prints its JSON.

    python tools/bench_pan_vis.py [--reps 30] [--no-numpy] [--forward-ms <ms_per_img_serial of bench.py at 1024 x 2048, same visit>]
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

CONFIGS = ((1024, 2048, 120), (800, 1333, 120))
ELEMENTWISE_TBPS = 6.3
NAMES = ['road', 'sidewalk', 'building', 'wall', 'fence', 'pole', 'traffic light', 'traffic sign', 'vegetation', 'terrain', 'sky',
         'person', 'rider', 'car', 'truck', 'bus', 'train', 'motorcycle', 'bicycle']
CATS = {c: {'id': c, 'isthing': int(c >= 11), 'color': [(c * 40 + 7) % 256, (128 + 9 * c) % 256, 250 - c], 'name': NAMES[c]} for c in range(19)}


def scene(H, W, n, seed=0):
    """(pred_2ch, image): n segments as nearest-seed cells (computed at 1/8 of the size and repeated), categories 0..18, things
    numbered per category from 1, one cell in sixteen VOID."""
    rng = np.random.default_rng(seed)
    h, w = -(-H // 8), -(-W // 8)
    pts = rng.permutation(h * w)[:n]
    yy, xx = np.mgrid[0:h, 0:w]
    cell = np.argmin((yy[..., None] - pts // w) ** 2 + (xx[..., None] - pts % w) ** 2, -1)
    cell = np.repeat(np.repeat(cell, 8, 0), 8, 1)[:H, :W]
    cat = rng.integers(0, 19, n)
    inst = np.zeros(n, np.int64)
    for c in range(19):
        sel = np.nonzero(cat == c)[0]
        inst[sel] = np.arange(len(sel)) + (1 if c >= 11 else 0)
    cat[rng.permutation(n)[:n // 16]] = 255
    pred = np.ascontiguousarray(np.stack([cat[cell], inst[cell], np.zeros_like(cell)], -1).astype(np.uint8))
    return pred, rng.integers(0, 256, (H, W, 3)).astype(np.uint8)


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


def device_call(pred, image, mode, min_area):
    """The entry point alone on device-resident inputs, after one upsnet_pan_format of the same map: returns (call, out, info)."""
    from upsnet_amd._lib import check, lib, ptr, stream
    from upsnet_amd.dataset import pan_vis
    H, W = pred.shape[:2]
    r = pan_vis.PanopticRenderer(CATS, 'cuda')
    d_pred, d_image = torch.from_numpy(pred).cuda(), torch.from_numpy(image).cuda()
    st = r._dev_state()
    handle = r.formatter.submit(d_pred)
    r.formatter.finish(handle)
    table = handle.buf[handle.offset:].view(torch.int32)
    out = torch.empty((H, W, 3), dtype=torch.uint8, device='cuda')
    info = torch.zeros((2,), dtype=torch.int32, device='cuda')
    overlay = mode == 'overlay'

    def call():
        check(lib().upsnet_pan_vis(stream(), pan_vis.MODES[mode], ptr(d_pred), ptr(handle.buf) if overlay else None, ptr(table) if overlay else None,
                                   ptr(d_image) if overlay else None, H, W, ptr(r.formatter._state['cat_table']), ptr(st['names']),
                                   ptr(st['lens']), min_area, ptr(st['ws']), ptr(out), ptr(info)), 'pan_vis')
    return call, out, info


def end_to_end(n_images, H, W, n, mode, min_area):
    """vis_panoptic over n_images generated photographs (PNG) and maps: seconds per image, after a warm pass."""
    from PIL import Image
    from upsnet_amd.dataset import pan_vis
    with tempfile.TemporaryDirectory() as tmp:
        preds, paths, images = [], [], []
        for i in range(n_images):
            pred, image = scene(H, W, n, seed=20 + i)
            image = np.repeat(np.repeat(image[::4, ::4], 4, 0), 4, 1)[:H, :W]       # 4 x 4 blocks: a PNG of a plausible size
            path = os.path.join(tmp, 'img_%d_leftImg8bit.png' % i)
            Image.fromarray(np.ascontiguousarray(image)).save(path)
            preds.append(torch.from_numpy(pred).cuda())
            paths.append(path)
            images.append({'id': i, 'file_name': os.path.basename(path)})
        pan_vis.vis_panoptic(preds[:2], images[:2], CATS, os.path.join(tmp, 'warm'), mode, image_paths=paths[:2], label_min_area=min_area)
        t0 = time.perf_counter()
        files = pan_vis.vis_panoptic(preds, images, CATS, os.path.join(tmp, 'out'), mode, image_paths=paths, label_min_area=min_area)
        return (time.perf_counter() - t0) / len(files)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--no-numpy', action='store_true')
    ap.add_argument('--no-end-to-end', action='store_true')
    ap.add_argument('--min-area', type=int, default=1024)
    ap.add_argument('--forward-ms', type=float, default=None, help='ms_per_img_serial of bench.py at 1024 x 2048 from the same visit')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'pan_vis.txt'))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_pan_vis.py measures the device path: it needs a GPU"
    import pan_vis_ref
    from upsnet_amd.dataset import vis
    reps = max(20, args.reps)
    res = {'what': 'upsnet_pan_vis per image', 'reps': reps, 'label_min_area': args.min_area, 'elementwise_TBps': ELEMENTWISE_TBPS, 'configs': []}
    for H, W, n in CONFIGS:
        pred, image = scene(H, W, n)
        for mode in ('flat', 'overlay'):
            call, d_out, d_info = device_call(pred, image, mode, args.min_area)
            us = event_times_us(call, reps)
            p50 = us[len(us) // 2]
            min_bytes = (6 if mode == 'flat' else 12) * H * W
            row = {'height': H, 'width': W, 'mode': mode, 'segments': int(len(pan_vis_ref.segments(pred)[0])), 'labels': d_info.tolist(),
                   'device_us_p50': round(p50, 1), 'device_us_min': round(us[0], 1), 'device_us_max': round(us[-1], 1), 'min_bytes': min_bytes,
                   'min_bytes_over_p50_TBps': round(min_bytes / (p50 * 1e-6) / 1e12, 3),
                   'share_of_elementwise': round(min_bytes / (p50 * 1e-6) / 1e12 / ELEMENTWISE_TBPS, 4)}
            if not args.no_numpy:
                t0 = time.perf_counter()
                want = pan_vis_ref.render_flat(pred, CATS) if mode == 'flat' else pan_vis_ref.render_overlay(pred, CATS, image, vis.font_table(),
                                                                                                            args.min_area)[0]
                row['numpy_ms'] = round(1e3 * (time.perf_counter() - t0), 1)
                row['equal_to_numpy'] = bool(np.array_equal(d_out.cpu().numpy(), want))
            if args.forward_ms is not None and (H, W) == (1024, 2048):
                row['forward_ms_per_img_serial'] = args.forward_ms
                row['render_over_forward'] = round(p50 / 1e3 / args.forward_ms, 4)
            if not args.no_end_to_end:
                row['vis_panoptic_s_per_image'] = round(end_to_end(8, H, W, n, mode, args.min_area), 4)
            res['configs'].append(row)
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write('Panoptic pictures on the device: csrc/pan_vis.hip through dataset/pan_vis.py (DESIGN.md section 4.20)\n'
                    '1x MI355X; tools/bench_pan_vis.py --reps %d%s\n\n' % (reps, '' if args.forward_ms is None else ' --forward-ms %s' % args.forward_ms))
            f.write(text + '\n\n'
                    '  device_us_p50             the launches of one upsnet_pan_vis call (flat: compose; overlay: moments, labels, compose), warm\n'
                    '  min_bytes                 flat 3 + 3, overlay 9 + 3 bytes per pixel; share_of_elementwise = min_bytes / p50 over %.1f TB/s\n'
                    '  numpy_ms                  the restatement of the rule (tests/pan_vis_ref.py) on the same input, one host core\n'
                    '  vis_panoptic_s_per_image  the file loop over 8 images: PNG decode, format, draw, copy back, PNG encode on its pools\n'
                    % ELEMENTWISE_TBPS)


if __name__ == '__main__':
    main()
