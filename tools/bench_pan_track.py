"""Panoptic tracking on the device (dataset/pan_track.py, csrc/pan_track.hip): the time of PanopticTracker.update
per frame at 1024 x 2048 with about 30 moving things over a few hundred device-resident frames, for max_age 0 and 3. Two figures per
setting, after a warm-up: the device time of one step (GPU events around each update, the median over the frames), and the time per
frame of the whole loop (events around all updates, no table looked at: what a video loop pays, launches and the previous frame's
table read included). The bytes a step must move at least (count pass: map 3 + memory 2 per pixel; relabel pass: 3 + 2 read, 3 + 2
written) over the step's device time is given against the 6.3 TB/s an element-wise kernel reaches on this part. Writes the report to
profiles/pan_track.txt (--out) and prints its JSON.

    python tools/bench_pan_track.py [--frames 300] [--things 30] [--forward-ms <ms_per_img_serial of bench.py at 1024 x 2048, same visit>]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ELEMENTWISE_TBPS = 6.3
THING_CATS = (11, 12, 13, 14, 15, 17, 18)


def sequence(H, W, things, frames, seed=0):
    """Frames of stuff bands with `things` rectangles (20..240 pixels a side) that drift by up to 6 pixels per frame; one in twenty
    is replaced per frame; instance numbers follow a fresh random order per frame."""
    rng = np.random.default_rng(seed)

    def born():
        return [int(rng.choice(THING_CATS)), int(rng.integers(0, H - 20)), int(rng.integers(0, W - 20)), int(rng.integers(20, 240)),
                int(rng.integers(20, 240))]
    blobs = [born() for _ in range(things)]
    base = np.zeros((H, W, 3), np.uint8)
    for k in range(8):
        base[k * H // 8:(k + 1) * H // 8, :, 0] = k
    base[:8] = (255, 0, 0)
    out = []
    for _ in range(frames):
        f = base.copy()
        count = {}
        for b in rng.permutation(things):
            c, y, x, h, w = blobs[b]
            count[c] = count.get(c, 0) + 1
            f[y:y + h, x:x + w] = (c, count[c], 0)
        out.append(torch.from_numpy(f).cuda())
        for b in range(things):
            if rng.random() < 0.05:
                blobs[b] = born()
            else:
                blobs[b][1] = int(np.clip(blobs[b][1] + rng.integers(-6, 7), 0, H - 20))
                blobs[b][2] = int(np.clip(blobs[b][2] + rng.integers(-6, 7), 0, W - 20))
    return out


def measure(frames, max_age, warmup, motion='none'):
    from upsnet_amd.dataset.pan_track import PanopticTracker
    trk = PanopticTracker(iou_thresh=0.3, max_age=max_age, motion=motion)
    for f in frames[:warmup]:
        trk.update(f)
    torch.cuda.synchronize()
    timed = frames[warmup:]
    pairs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in timed]
    held = []
    for f, (e0, e1) in zip(timed, pairs):
        e0.record()
        held.append(trk.update(f)[1])
        e1.record()
    torch.cuda.synchronize()
    step_us = sorted(1000.0 * e0.elapsed_time(e1) for e0, e1 in pairs)
    matched = sum(s['matched'] for segs in held for s in segs)
    total = sum(len(segs) for segs in held)
    # the whole loop, from a fresh tracker on the same frames
    trk = PanopticTracker(iou_thresh=0.3, max_age=max_age, motion=motion)
    for f in frames[:warmup]:
        trk.update(f)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for f in timed:
        trk.update(f)
    b.record()
    torch.cuda.synchronize()
    return {'max_age': max_age, 'frames_timed': len(timed), 'segments_per_frame': round(total / len(timed), 1),
            'matched_share': round(matched / max(total, 1), 3), 'tracks_issued': trk.next_serial - 1,
            'step_device_us_p50': round(step_us[len(step_us) // 2], 1), 'step_device_us_min': round(step_us[0], 1),
            'step_device_us_max': round(step_us[-1], 1), 'loop_us_per_frame': round(1000.0 * a.elapsed_time(b) / len(timed), 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=300)
    ap.add_argument('--things', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--repeats', type=int, default=3, help='each setting is measured this often, alternating')
    ap.add_argument('--forward-ms', type=float, default=None)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'pan_track.txt'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_pan_track measures on the GPU; none is visible')
    H, W = 1024, 2048
    frames = sequence(H, W, args.things, args.frames)
    min_bytes = H * W * (5 + 10)
    runs = []
    for _ in range(args.repeats):
        for age in (0, 3):
            r = measure(frames, age, args.warmup)
            r['min_bytes'] = min_bytes
            r['min_bytes_over_p50_TBps'] = round(min_bytes / (r['step_device_us_p50'] * 1e-6) / 1e12, 3)
            r['share_of_elementwise'] = round(r['min_bytes_over_p50_TBps'] / ELEMENTWISE_TBPS, 4)
            if args.forward_ms:
                r['forward_ms_per_img_serial'] = args.forward_ms
                r['loop_over_forward'] = round(r['loop_us_per_frame'] / 1000.0 / args.forward_ms, 4)
            runs.append(r)
    report = {'what': 'PanopticTracker.update per frame', 'height': H, 'width': W, 'things': args.things, 'frames': args.frames,
              'warmup': args.warmup, 'elementwise_TBps': ELEMENTWISE_TBPS, 'runs': runs}
    text = json.dumps(report, indent=1)
    head = ('Panoptic tracking on the device: csrc/pan_track.hip through dataset/pan_track.py (DESIGN.md section 4.23)\n'
            '1x MI355X; tools/bench_pan_track.py --frames %d --things %d%s\n\n'
            % (args.frames, args.things, ' --forward-ms %s' % args.forward_ms if args.forward_ms else ''))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(head + text + '\n')
    print(text)


if __name__ == '__main__':
    main()
