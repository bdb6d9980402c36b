"""Connected components on the device (ops.pan_components, csrc/pan_components.hip) on one seeded 1024 x 2048 blob
map (blocks of about 100 pixels a side of some thirty keys, single stray pixels sprinkled over them), in one process:

  - the five launches of ops.pan_components (workspace and output reused), GPU events around each call after a warm-up: the median,
    and the time per call of the whole timed loop;
  - PanopticEvaluator.add (ops.pq_accumulate) on the same map, as a scale;
  - the host route it replaces: device -> host copy, scipy.ndimage.label once per key, host -> device copy (host clock around work
    that ends in a synchronise). Its output must equal the device's byte for byte, or the tool stops.

The bytes each pass must move at least, from the shapes, stand beside the times. Writes the report to profiles/pan_components.txt
(--out) and prints its JSON.

    python tools/bench_pan_components.py [--iters 300] [--min-area 40] [--connectivity 8]

Per-kernel durations come from a run of their own under the profiler, whose statistics are then appended to the report:

    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/bench_pan_components.py --device-only --out /dev/null
    python tools/bench_pan_components.py --append-kernel-stats <dir>
"""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ELEMENTWISE_TBPS = 6.3
H, W = 1024, 2048
KEYS = [(0, 0), (3, 0), (5, 0), (8, 0), (255, 0)] + [(11 + k % 7, 1 + k // 7) for k in range(27)]


def blob_map(seed=0, cell=96, speck=0.002):
    rng = np.random.default_rng(seed)
    grid = rng.integers(0, len(KEYS), (H // cell + 2, W // cell + 2))
    pick = np.repeat(np.repeat(grid, cell, 0), cell, 1)[cell // 3:cell // 3 + H, cell // 2:cell // 2 + W]
    pick = np.where(rng.random((H, W)) < speck, rng.integers(0, len(KEYS), (H, W)), pick)
    pan = np.zeros((H, W, 3), np.uint8)
    pan[..., 0] = np.array([k[0] for k in KEYS], np.uint8)[pick]
    pan[..., 1] = np.array([k[1] for k in KEYS], np.uint8)[pick]
    return pan


def host_route(pan_dev, min_area, connectivity):
    from scipy import ndimage
    a = pan_dev.cpu().numpy()
    structure = np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]]) if connectivity == 4 else np.ones((3, 3), int)
    key = a[..., 0].astype(np.int32) << 8 | a[..., 1]
    out = a.copy()
    for k in np.unique(key[a[..., 0] != 255]).tolist():
        lab, n = ndimage.label(key == k, structure=structure)
        areas = np.bincount(lab.reshape(-1), minlength=n + 1)
        small = areas < min_area
        small[0] = False
        small[1 + int(np.argmax(areas[1:]))] = False          # (the first of the largest: scipy numbers components in raster order)
        gone = small[lab]
        out[gone, 0] = 255
        out[gone, 1] = 0
    return torch.from_numpy(out).to(pan_dev.device)


def events(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    pairs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for e0, e1 in pairs:
        e0.record()
        fn()
        e1.record()
    b.record()
    torch.cuda.synchronize()
    us = sorted(1000.0 * e0.elapsed_time(e1) for e0, e1 in pairs)
    return {'device_us_p50': round(us[len(us) // 2], 1), 'device_us_min': round(us[0], 1), 'device_us_max': round(us[-1], 1),
            'loop_us_per_call': round(1000.0 * a.elapsed_time(b) / iters, 1), 'iters': iters}


def append_kernel_stats(folder, out):
    rows = []
    for d, _, files in os.walk(folder):
        for f in files:
            if f.endswith('kernel_stats.csv'):
                with open(os.path.join(d, f)) as fh:
                    rows += [r for r in csv.DictReader(fh) if r.get('Name', '').startswith('pc_')]
    if not rows:
        raise SystemExit('no kernel_stats.csv with pc_* kernels under %s' % folder)
    lines = ['', 'Per-kernel durations, rocprofv3 --kernel-trace --stats, a run of its own (--device-only):',
             '%-20s %8s %12s %12s %12s' % ('kernel', 'calls', 'avg us', 'min us', 'max us')]
    for r in sorted(rows, key=lambda r: r['Name']):
        lines.append('%-20s %8s %12.1f %12.1f %12.1f' % (r['Name'].split('(')[0], r['Calls'], float(r['AverageNs']) / 1e3,
                                                          float(r['MinNs']) / 1e3, float(r['MaxNs']) / 1e3))
    with open(out, 'a') as f:
        f.write('\n'.join(lines) + '\n')
    print('\n'.join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=300)
    ap.add_argument('--warmup', type=int, default=30)
    ap.add_argument('--host-iters', type=int, default=5)
    ap.add_argument('--min-area', type=int, default=40)
    ap.add_argument('--connectivity', type=int, default=8, choices=(4, 8))
    ap.add_argument('--device-only', action='store_true', help='only the device loop (the target of a profiler run)')
    ap.add_argument('--append-kernel-stats', default='', metavar='DIR', help="append the pc_* rows of a rocprofv3 --stats run to --out")
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'pan_components.txt'))
    args = ap.parse_args()
    if args.append_kernel_stats:
        return append_kernel_stats(args.append_kernel_stats, args.out)
    if not torch.cuda.is_available():
        raise SystemExit('bench_pan_components measures on the GPU; none is visible')
    from upsnet_amd import ops
    pan_np = blob_map()
    pan = torch.from_numpy(pan_np).cuda()
    ws = ops.pan_components_workspace(H, W, 'cuda')
    out = pan.clone()
    labels = torch.zeros((H, W), dtype=torch.int32, device='cuda')

    def device():
        return ops.pan_components(pan, args.min_area, args.connectivity, True, workspace=ws, out=out, labels=labels)
    stats = device()[1].cpu().tolist()
    runs = {'pan_components': events(device, args.iters, args.warmup)}
    if args.device_only:
        print(json.dumps(runs))
        return
    want = host_route(pan, args.min_area, args.connectivity)
    if not torch.equal(want, out):
        raise SystemExit('the host route and the device disagree on %d pixels' % int((want != out).any(-1).sum()))

    from upsnet_amd.dataset.pq import PanopticEvaluator
    ids = np.where(pan_np[..., 0] == 255, 0, pan_np[..., 0].astype(np.int64) * 256 + pan_np[..., 1] + 1)
    gt = torch.from_numpy(np.stack([ids % 256, ids // 256 % 256, ids // 65536], 2).astype(np.uint8)).cuda()
    u, cnt = np.unique(ids[ids > 0], return_counts=True)
    segs = [{'id': int(i), 'category_id': int((i - 1) // 256), 'iscrowd': 0, 'area': int(c)} for i, c in zip(u, cnt)]
    pe = PanopticEvaluator({c: {'id': c, 'isthing': int(c >= 11)} for c in range(255)})
    runs['pq_accumulate'] = events(lambda: pe.add(pan, gt, segs), args.iters, args.warmup)
    pe.pq_stat()

    host = []
    host_route(pan, args.min_area, args.connectivity)
    for _ in range(args.host_iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host_route(pan, args.min_area, args.connectivity)
        torch.cuda.synchronize()
        host.append(1e6 * (time.perf_counter() - t0))
    host.sort()
    runs['host_route_scipy'] = {'us_p50': round(host[len(host) // 2], 1), 'us_min': round(host[0], 1), 'us_max': round(host[-1], 1),
                                'iters': args.host_iters, 'keys': stats[0]}
    npix = H * W
    ty, tx = (H + 31) // 32, (W + 127) // 128
    passes = {'pc_tile_kernel': npix * (3 + 4 + 4),                    # map read; parent and area written
              'pc_seam_kernel': ((ty - 1) * W + (tx - 1) * H) * (2 * 2 + 2 * 4),   # two keys and two parents per seam pixel, at least
              'pc_flatten_kernel': npix * (4 + 4),                     # parent read and written (+ one area atomic per run)
              'pc_main_kernel': npix * 4,                              # parent read (+ one 8-byte atomic per component)
              'pc_apply_kernel': npix * (3 + 4 + 3 + 4)}               # map and parent read; map and labels written
    total = sum(passes.values())
    dev_us = runs['pan_components']['device_us_p50']
    report = {'what': 'ops.pan_components per 1024 x 2048 map', 'height': H, 'width': W, 'min_area': args.min_area,
              'connectivity': args.connectivity, 'stats_keys_components_removed_pixels': stats, 'runs': runs,
              'min_bytes_per_pass': passes, 'min_bytes': total,
              'min_bytes_over_p50_TBps': round(total / (dev_us * 1e-6) / 1e12, 3), 'elementwise_TBps': ELEMENTWISE_TBPS,
              'share_of_elementwise': round(total / (dev_us * 1e-6) / 1e12 / ELEMENTWISE_TBPS, 4),
              'pan_components_over_pq_accumulate': round(dev_us / runs['pq_accumulate']['device_us_p50'], 3),
              'host_route_over_device': round(runs['host_route_scipy']['us_p50'] / dev_us, 1),
              'device_faster_than_host_route': bool(dev_us < runs['host_route_scipy']['us_min'])}
    text = json.dumps(report, indent=1)
    head = ('Connected components on the device: csrc/pan_components.hip through ops.pan_components (DESIGN.md section 4.26)\n'
            '1x MI355X; tools/bench_pan_components.py --iters %d --min-area %d --connectivity %d\n\n'
            % (args.iters, args.min_area, args.connectivity))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(head + text + '\n')
    print(text)


if __name__ == '__main__':
    main()
