"""Fragments absorbed on the device (ops.pan_absorb, csrc/pan_components.hip) on the seeded 1024 x 2048 blob map
of tools/bench_pan_components.py, in one process:

  - the eight launches of ops.pan_absorb (workspace, output and labels reused), GPU events around each call after a warm-up: the median;
  - ops.pan_components on the same map and build, the yardstick: this change leaves its launches as they were;
  - the host route: device -> host copy, the vectorised restatement of tests/pan_absorb_ref.py (on scipy.ndimage.label), host -> device
    copy, host clock around work that ends in a synchronise. Its output must equal the device's byte for byte, or the tool stops.

Writes the report to profiles/pan_absorb.txt (--out) and prints its JSON.

    python tools/bench_pan_absorb.py [--iters 300] [--min-area 40] [--connectivity 8]

Per-kernel durations come from a run of their own under the profiler, whose statistics are then appended to the report:

    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/bench_pan_absorb.py --device-only --out /dev/null
    python tools/bench_pan_absorb.py --append-kernel-stats <dir>
"""
import argparse
import csv
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))

from bench_pan_components import H, W, blob_map, events


def append_kernel_stats(folder, out):
    rows = []
    for d, _, files in os.walk(folder):
        for f in files:
            if f.endswith('kernel_stats.csv'):
                with open(os.path.join(d, f)) as fh:
                    rows += [r for r in csv.DictReader(fh) if r.get('Name', '').startswith(('pc_', 'pa_'))]
    if not rows:
        raise SystemExit('no kernel_stats.csv with pc_* / pa_* kernels under %s' % folder)
    lines = ['', 'Per-kernel durations, rocprofv3 --kernel-trace --stats, a run of its own (--device-only: the loop of ops.pan_absorb and',
             'then that of ops.pan_components, so the pc_* labelling kernels have twice the calls):',
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
    ap.add_argument('--host-iters', type=int, default=3)
    ap.add_argument('--min-area', type=int, default=40)
    ap.add_argument('--connectivity', type=int, default=8, choices=(4, 8))
    ap.add_argument('--device-only', action='store_true', help='only the device loops (the target of a profiler run)')
    ap.add_argument('--append-kernel-stats', default='', metavar='DIR', help="append the pc_* / pa_* rows of a rocprofv3 --stats run to --out")
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'pan_absorb.txt'))
    args = ap.parse_args()
    if args.append_kernel_stats:
        return append_kernel_stats(args.append_kernel_stats, args.out)
    if not torch.cuda.is_available():
        raise SystemExit('bench_pan_absorb measures on the GPU; none is visible')
    from upsnet_amd import ops
    pan_np = blob_map()
    pan = torch.from_numpy(pan_np).cuda()
    ws = ops.pan_absorb_workspace(H, W, 'cuda')
    ws_void = ops.pan_components_workspace(H, W, 'cuda')
    out, out_void = pan.clone(), pan.clone()
    labels = torch.zeros((H, W), dtype=torch.int32, device='cuda')

    def absorb():
        return ops.pan_absorb(pan, args.min_area, args.connectivity, True, workspace=ws, out=out, labels=labels)

    def void():
        return ops.pan_components(pan, args.min_area, args.connectivity, True, workspace=ws_void, out=out_void, labels=labels)
    stats = absorb()[1].cpu().tolist()
    runs = {'pan_absorb': events(absorb, args.iters, args.warmup), 'pan_components': events(void, args.iters, args.warmup)}
    if args.device_only:
        print(json.dumps(runs))
        return

    import pan_absorb_ref

    def host_route():
        a = pan.cpu().numpy()
        return torch.from_numpy(pan_absorb_ref.absorb_vec(a, args.min_area, args.connectivity, True)[0]).cuda()
    want = host_route()
    if not torch.equal(want, out):
        raise SystemExit('the host route and the device disagree on %d pixels' % int((want != out).any(-1).sum()))
    host = []
    for _ in range(args.host_iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host_route()
        torch.cuda.synchronize()
        host.append(1e6 * (time.perf_counter() - t0))
    host.sort()
    runs['host_route_numpy_scipy'] = {'us_p50': round(host[len(host) // 2], 1), 'us_min': round(host[0], 1), 'us_max': round(host[-1], 1),
                                      'iters': args.host_iters}
    a_us, v_us = runs['pan_absorb']['device_us_p50'], runs['pan_components']['device_us_p50']
    report = {'what': 'ops.pan_absorb per 1024 x 2048 map', 'height': H, 'width': W, 'min_area': args.min_area,
              'connectivity': args.connectivity,
              'stats_keys_components_fragments_pixels_absorbed_absorbedpixels_pairs_overflow': stats,
              'workspace_bytes': {'pan_absorb': ws.numel(), 'pan_components': ws_void.numel()}, 'runs': runs,
              'pan_absorb_over_pan_components': round(a_us / v_us, 3),
              'host_route_over_device': round(runs['host_route_numpy_scipy']['us_p50'] / a_us, 1)}
    text = json.dumps(report, indent=1)
    head = ('Fragments absorbed on the device: csrc/pan_components.hip through ops.pan_absorb (DESIGN.md section 4.27)\n'
            '1x MI355X; tools/bench_pan_absorb.py --iters %d --min-area %d --connectivity %d\n\n'
            % (args.iters, args.min_area, args.connectivity))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(head + text + '\n')
    print(text)


if __name__ == '__main__':
    main()
