"""Constant-velocity motion prediction of the panoptic tracker: what a motion step costs and what it does to
the identities.

Time: the protocol of tools/bench_pan_track.py (1024 x 2048, about 30 moving things, device-resident frames, a warm-up, the median of
the per-update event pairs and the time per frame of the whole loop), the motion-off and the motion-on tracker alternating, both in this
run. The motion-off step runs the plain tracker's kernels.

Quality, on synthetic sequences with ground-truth identities (there is no trained checkpoint and no real video here: nothing below is
a claim about real data): rectangles over a stuff background, numbered afresh per frame, (a) each with a fixed velocity and blink-outs,
(b) a random walk without persistent velocity. The tracked maps are scored by VideoPanopticEvaluator (VPQ, STQ; the masks are exact,
so only the identities cost anything) and the serials and matches counted, with and without motion.

    python tools/bench_pan_track_motion.py [--frames 300] [--things 30] [--out profiles/pan_track_motion.txt]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_pan_track import measure, sequence   # noqa: E402

H, W = 96, 160
STUFF, THINGS = (7, 9), (11, 12)
CATEGORIES = [{'id': c, 'name': 'c%d' % c, 'isthing': int(c in THINGS)} for c in STUFF + THINGS]


def scene(seed, things, frames, mode, vmax=3, step=2, side=10, blink=0.15):
    """[(prediction uint8 [H,W,3] with per-frame numbering, ground truth uint8 [H,W,3] with id = R + 256 G, segments_info)] per frame.
    mode 'velocity': a fixed velocity of up to vmax per axis per object; 'walk': up to `step` pixels per axis per frame, anew each
    frame, clipped to the image. An object blinks out of a frame with probability `blink` (of prediction and ground truth alike)."""
    rng = np.random.default_rng(seed)
    objs = [[int(rng.choice(THINGS)), int(rng.integers(0, H - side)), int(rng.integers(0, W - side)),
             int(rng.integers(-vmax, vmax + 1)), int(rng.integers(-vmax, vmax + 1))] for _ in range(things)]
    out = []
    for _ in range(frames):
        p, g = np.zeros((H, W, 3), np.uint8), np.zeros((H, W, 3), np.uint8)
        segs = []
        for k, c in enumerate(STUFF):
            p[k * H // 2:(k + 1) * H // 2] = (c, 0, 0)
            g[k * H // 2:(k + 1) * H // 2] = (k + 1, 0, 0)
            segs.append({'id': k + 1, 'category_id': c, 'iscrowd': 0})
        count = {}
        for b in rng.permutation(things):
            c, y, x = objs[b][:3]
            y0, y1, x0, x1 = max(y, 0), min(y + side, H), max(x, 0), min(x + side, W)
            if rng.random() < blink or y0 >= y1 or x0 >= x1:
                continue
            count[c] = count.get(c, 0) + 1
            p[y0:y1, x0:x1] = (c, count[c], 0)
            g[y0:y1, x0:x1] = ((100 + b) & 255, (100 + b) >> 8, 0)
            segs.append({'id': 100 + int(b), 'category_id': c, 'iscrowd': 0})
        ids = g[:, :, 0].astype(np.int64) + 256 * g[:, :, 1].astype(np.int64)
        area = np.bincount(ids.reshape(-1), minlength=100 + things)
        out.append((p, g, [dict(sg, area=int(area[sg['id']])) for sg in segs if area[sg['id']]]))
        for o in objs:
            if mode == 'velocity':
                o[1] += o[3]
                o[2] += o[4]
            else:
                o[1] = int(np.clip(o[1] + rng.integers(-step, step + 1), 0, H - 1))
                o[2] = int(np.clip(o[2] + rng.integers(-step, step + 1), 0, W - 1))
    return out


def quality(name, seeds, motion, max_age=2, **kw):
    from upsnet_amd.dataset.pan_track import PanopticTracker
    from upsnet_amd.dataset.video_pq import VideoPanopticEvaluator
    ev = VideoPanopticEvaluator(CATEGORIES, windows=(1, 2, 3, 4))
    trk = PanopticTracker(iou_thresh=0.3, max_age=max_age, motion=motion)
    matched = total = objects = 0
    for seed in seeds:
        frames = scene(seed, **kw)
        objects += len(set(sg['id'] for _, _, info in frames for sg in info if sg['id'] >= 100))
        trk.reset()
        ev.begin_sequence([info for _, _, info in frames])
        for p, g, _ in frames:
            out, segs = trk.update(p)
            ev.add_frame(out, torch.from_numpy(g).cuda())
            matched += sum(s['matched'] for s in segs)
            total += len(segs)
        ev.end_sequence()
    res = ev.summary()
    return {'sequences': name, 'motion': motion, 'max_age': max_age, 'objects': objects, 'serials': trk.next_serial - 1, 'segments': total,
            'matched': matched, 'vpq': round(res['vpq']['All']['pq'], 4), 'vpq_things': round(res['vpq']['Things']['pq'], 4),
            'stq': round(res['stq']['stq'], 4), 'aq': round(res['stq']['aq'], 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=300)
    ap.add_argument('--things', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--repeats', type=int, default=3, help='each setting is measured this often, alternating')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'pan_track_motion.txt'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_pan_track_motion measures on the GPU; none is visible')
    frames = sequence(1024, 2048, args.things, args.frames)
    runs = []
    for _ in range(args.repeats):
        for age in (0, 3):
            for motion in ('none', 'constant_velocity'):
                r = measure(frames, age, args.warmup, motion)
                r['motion'] = motion
                runs.append(r)
    ratio = {}
    for age in (0, 3):
        p50 = {m: sorted(r['step_device_us_p50'] for r in runs if r['max_age'] == age and r['motion'] == m) for m in ('none', 'constant_velocity')}
        loop = {m: sorted(r['loop_us_per_frame'] for r in runs if r['max_age'] == age and r['motion'] == m) for m in ('none', 'constant_velocity')}
        mid = len(p50['none']) // 2
        ratio['max_age_%d' % age] = {'step_device_us_p50': {m: p50[m][mid] for m in p50}, 'loop_us_per_frame': {m: loop[m][mid] for m in loop},
                                     'step_ratio': round(p50['constant_velocity'][mid] / p50['none'][mid], 3),
                                     'loop_ratio': round(loop['constant_velocity'][mid] / loop['none'][mid], 3)}
    seeds = list(range(8))
    qual = []
    for name, kw in (('constant velocity, up to 3 px/frame', dict(things=10, frames=16, mode='velocity', vmax=3)),
                     ('constant velocity, up to 5 px/frame', dict(things=10, frames=16, mode='velocity', vmax=5)),
                     ('random walk, step 2', dict(things=10, frames=16, mode='walk', step=2)),
                     ('random walk, step 6', dict(things=10, frames=16, mode='walk', step=6)),
                     ('random walk, step 10', dict(things=10, frames=16, mode='walk', step=10))):
        for motion in ('none', 'constant_velocity'):
            qual.append(quality(name, seeds, motion, **kw))
    report = {'what': 'PanopticTracker.update per frame, motion none against constant_velocity', 'height': 1024, 'width': 2048,
              'things': args.things, 'frames': args.frames, 'warmup': args.warmup, 'time_median_of_repeats': ratio, 'runs': runs,
              'quality_what': '8 synthetic sequences of 16 frames of %d x %d, 10 rectangles of 10 x 10, 15 %% blink-outs, iou_thresh 0.3, '
                              'max_age 2; exact masks, so VPQ / STQ move with the identities only; no real data' % (H, W),
              'quality': qual}
    text = json.dumps(report, indent=1)
    head = ('Panoptic tracking with constant-velocity motion prediction: csrc/pan_track.hip through dataset/pan_track.py (DESIGN.md section '
            '4.28)\n1x MI355X; tools/bench_pan_track_motion.py --frames %d --things %d\n\n' % (args.frames, args.things))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(head + text + '\n')
    print(text)


if __name__ == '__main__':
    main()
