"""Video scoring on the device (dataset/video_pq.py, csrc/video_eval.hip): the device time of
VideoPanopticEvaluator.add_frame per frame at 1024 x 2048 with about 30 moving things, for windows (1, 2, 3, 4) and for (1,) -- the
difference is what the longer windows cost --, beside two yardsticks from the same visit and the same device-resident frames:
ops.pq_accumulate per image (the existing single-image scorer) and PanopticTracker.update. After a warm-up, GPU events around each
call (a span that includes the host's launch gaps wherever the device is ahead of the host, for all three alike); the median over the
timed frames, and the time per frame of the whole timed loop; each setting measured `--repeats` times, alternating. The frames come in sequences of
`--length` frames; end_sequence is timed the same way. Writes the report to profiles/video_eval.txt (--out) and prints its JSON.

    python tools/bench_video_eval.py [--frames 240] [--length 30] [--things 30]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

THING_CATS = (11, 12, 13, 14, 15, 17, 18)
CATEGORIES = {c: {'id': c, 'isthing': int(c >= 11)} for c in range(19)}


def sequences(H, W, things, frames, length, seed=0):
    """[(preds, gts, frames_segments_info)]: stuff bands with `things` rectangles (20..240 pixels a side) that drift by up to 6 pixels
    per frame; the GT id of an object is fixed for its sequence; the prediction is the GT moved by (2, 3) pixels with an 8-row VOID band,
    the tube numbers those of the objects, one object in ten renumbered half-way through its sequence. Device tensors."""
    rng = np.random.default_rng(seed)
    out = []
    for s in range(frames // length):
        blobs = [[int(rng.choice(THING_CATS)), int(rng.integers(0, H - 240)), int(rng.integers(0, W - 240)), int(rng.integers(20, 240)),
                  int(rng.integers(20, 240))] for _ in range(things)]
        inst, count = [], {}
        for b in blobs:
            count[b[0]] = count.get(b[0], 0) + 1
            inst.append(count[b[0]])
        preds, gts, infos = [], [], []
        for t in range(length):
            p, g = np.zeros((H, W, 3), np.uint8), np.zeros((H, W, 3), np.uint8)
            segs = []
            for k in range(8):
                p[k * H // 8:(k + 1) * H // 8, :, 0] = k
                g[k * H // 8:(k + 1) * H // 8, :, 0] = k + 1
                segs.append({'id': k + 1, 'category_id': k, 'iscrowd': 0, 'area': 0})
            for k, (c, y, x, h, w) in enumerate(blobs):
                g[y:y + h, x:x + w] = (100 + k, 0, 0)
                switched = k % 10 == 0 and t >= length // 2
                p[y + 2:y + 2 + h, x + 3:x + 3 + w] = (c, inst[k] + (100 if switched else 0), 0)
                segs.append({'id': 100 + k, 'category_id': c, 'iscrowd': int(k == 7), 'area': 0})
            p[:8] = (255, 0, 0)
            g[H - 8:] = 0
            preds.append(torch.from_numpy(p).cuda())
            gts.append(torch.from_numpy(g).cuda())
            area = np.bincount(g[:, :, 0].reshape(-1), minlength=256)      # (ids < 256: channel 0 is the id; the JSON area = pixels)
            infos.append([dict(sg, area=int(area[sg['id']])) for sg in segs if area[sg['id']]])
            for b in blobs:
                b[1] = int(np.clip(b[1] + rng.integers(-6, 7), 0, H - 242))
                b[2] = int(np.clip(b[2] + rng.integers(-6, 7), 0, W - 243))
        out.append((preds, gts, infos))
    return out


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    return e0, e1


class Loop(object):
    """Events around the whole timed part of a loop: what the loop pays per frame, launches included."""

    def __init__(self):
        self.a, self.b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        self.started = False

    def start_once(self):
        if not self.started:
            self.a.record()
            self.started = True

    def per_frame(self, n):
        self.b.record()
        torch.cuda.synchronize()
        return round(1000.0 * self.a.elapsed_time(self.b) / max(n, 1), 1)


def p50(pairs):
    us = sorted(1000.0 * a.elapsed_time(b) for a, b in pairs)
    return round(us[len(us) // 2], 1), round(us[0], 1), round(us[-1], 1)


def measure_video(seqs, windows, warm):
    from upsnet_amd.dataset.video_pq import VideoPanopticEvaluator
    ev = VideoPanopticEvaluator(CATEGORIES, windows=windows)
    frames, ends, loop = [], [], Loop()
    for s, (preds, gts, infos) in enumerate(seqs):
        if s >= warm:
            loop.start_once()
        ev.begin_sequence(infos)
        for p, g in zip(preds, gts):
            pair = timed(lambda: ev.add_frame(p, g))
            if s >= warm:
                frames.append(pair)
        pair = timed(ev.end_sequence)
        if s >= warm:
            ends.append(pair)
    per_frame = loop.per_frame(len(frames))
    res = ev.summary()
    f, e = p50(frames), p50(ends)
    return {'what': 'add_frame', 'windows': list(windows), 'frames_timed': len(frames), 'device_us_p50': f[0], 'device_us_min': f[1],
            'device_us_max': f[2], 'loop_us_per_frame': per_frame, 'end_sequence_us_p50': e[0], 'vpq': round(res['vpq']['All']['pq'], 4), 'stq': round(res['stq']['stq'], 4)}


def measure_pq(seqs, warm):
    from upsnet_amd.dataset.pq import PanopticEvaluator
    pe = PanopticEvaluator(CATEGORIES)
    pairs, loop = [], Loop()
    for s, (preds, gts, infos) in enumerate(seqs):
        if s >= warm:
            loop.start_once()
        for p, g, segs in zip(preds, gts, infos):
            pair = timed(lambda: pe.add(p, g, segs))
            if s >= warm:
                pairs.append(pair)
    per_frame = loop.per_frame(len(pairs))
    pe.pq_stat()
    f = p50(pairs)
    return {'what': 'PanopticEvaluator.add (ops.pq_accumulate)', 'frames_timed': len(pairs), 'device_us_p50': f[0], 'device_us_min': f[1],
            'device_us_max': f[2], 'loop_us_per_frame': per_frame}


def measure_tracker(seqs, warm):
    from upsnet_amd.dataset.pan_track import PanopticTracker
    trk = PanopticTracker(iou_thresh=0.3, max_age=0)
    pairs, loop = [], Loop()
    for s, (preds, _, _) in enumerate(seqs):
        if s >= warm:
            loop.start_once()
        trk.reset()
        for p in preds:
            pair = timed(lambda: trk.update(p))
            if s >= warm:
                pairs.append(pair)
    per_frame = loop.per_frame(len(pairs))
    f = p50(pairs)
    return {'what': 'PanopticTracker.update', 'frames_timed': len(pairs), 'device_us_p50': f[0], 'device_us_min': f[1], 'device_us_max': f[2],
            'loop_us_per_frame': per_frame}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=240)
    ap.add_argument('--length', type=int, default=30, help='frames per sequence')
    ap.add_argument('--things', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=1, help='sequences that are run and not timed')
    ap.add_argument('--repeats', type=int, default=3, help='each setting is measured this often, alternating')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'video_eval.txt'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_video_eval measures on the GPU; none is visible')
    H, W = 1024, 2048
    seqs = sequences(H, W, args.things, args.frames, args.length)
    runs = []
    for _ in range(args.repeats):
        runs.append(measure_video(seqs, (1, 2, 3, 4), args.warmup))
        runs.append(measure_video(seqs, (1,), args.warmup))
        runs.append(measure_pq(seqs, args.warmup))
        runs.append(measure_tracker(seqs, args.warmup))

    def med(what, windows=None):
        v = sorted(r['device_us_p50'] for r in runs if r['what'] == what and (windows is None or r['windows'] == windows))
        return v[len(v) // 2]
    full, one, pq, trk = med('add_frame', [1, 2, 3, 4]), med('add_frame', [1]), med('PanopticEvaluator.add (ops.pq_accumulate)'), \
        med('PanopticTracker.update')
    report = {'what': 'VideoPanopticEvaluator.add_frame per frame', 'height': H, 'width': W, 'things': args.things, 'frames': args.frames,
              'sequence_length': args.length, 'warmup_sequences': args.warmup, 'repeats': args.repeats,
              'add_frame_us_windows_1234': full, 'add_frame_us_windows_1': one, 'pq_accumulate_us': pq, 'tracker_step_us': trk,
              'add_frame_over_pq_accumulate': round(full / pq, 3), 'windows_234_us': round(full - one, 1), 'runs': runs}
    text = json.dumps(report, indent=1)
    head = ('Video scoring on the device: csrc/video_eval.hip through dataset/video_pq.py (DESIGN.md section 4.24)\n'
            '1x MI355X; tools/bench_video_eval.py --frames %d --length %d --things %d\n\n' % (args.frames, args.length, args.things))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(head + text + '\n')
    print(text)


if __name__ == '__main__':
    main()
