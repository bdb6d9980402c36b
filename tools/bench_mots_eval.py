"""MOTS scoring on the device (dataset/mots.py, csrc/mots_eval.hip): the device time per 1024 x 2048 frame of
MOTSEvaluator.add_frame (the MOTS frame step: three launches) and of upsnet_pan_rle_transitions (the kernel behind write_mots_txt),
beside VideoPanopticEvaluator.add_frame with windows (1, 2, 3, 4) measured in the same run on the same device-resident frames (the
blob sequences of tools/bench_video_eval.py). After a warm-up, GPU events around each call (a span that includes the host's launch
gaps wherever the device is ahead of the host, for all alike); the median over the timed frames, and the time per frame of the whole
timed loop; each setting measured `--repeats` times, alternating. Writes the report to profiles/mots_eval.txt (--out) and prints it.

    python tools/bench_mots_eval.py [--frames 120] [--length 30] [--things 30]

Under `rocprofv3 --kernel-trace --stats -- python tools/bench_mots_eval.py --out <other file>` the per-kernel times come out as well.
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

from bench_video_eval import CATEGORIES, Loop, measure_video, p50, sequences, timed   # noqa: E402


def measure_mots(seqs, warm):
    from upsnet_amd.dataset.mots import MOTSEvaluator
    ev = MOTSEvaluator(CATEGORIES)
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
    return {'what': 'MOTSEvaluator.add_frame', 'frames_timed': len(frames), 'device_us_p50': f[0], 'device_us_min': f[1], 'device_us_max': f[2],
            'loop_us_per_frame': per_frame, 'end_sequence_us_p50': e[0], 'smotsa': round(res['mean']['smotsa'], 4),
            'motsa': round(res['mean']['motsa'], 4), 'ids': res['total']['ids'], 'tp': res['total']['tp'], 'fp': res['total']['fp']}


def measure_transitions(seqs, warm):
    """The kernel alone (its memset and launch; the pair buffer is allocated once, no count is read back inside the timed span)."""
    from upsnet_amd._lib import check, lib, ptr, stream
    cap = 1 << 20
    pairs = torch.empty((cap,), dtype=torch.int64, device='cuda')
    count = torch.empty((1,), dtype=torch.int32, device='cuda')
    spans, loop, most = [], Loop(), 0
    for s, (preds, _, _) in enumerate(seqs):
        if s >= warm:
            loop.start_once()
        for p in preds:
            H, W = int(p.shape[0]), int(p.shape[1])
            pair = timed(lambda: check(lib().upsnet_pan_rle_transitions(stream(), ptr(p), H, W, cap, ptr(pairs), ptr(count)), 'pan_rle_transitions'))
            if s >= warm:
                spans.append(pair)
    per_frame = loop.per_frame(len(spans))
    most = int(count.item())
    f = p50(spans)
    return {'what': 'upsnet_pan_rle_transitions', 'frames_timed': len(spans), 'device_us_p50': f[0], 'device_us_min': f[1], 'device_us_max': f[2],
            'loop_us_per_frame': per_frame, 'transitions_last_frame': most}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=120)
    ap.add_argument('--length', type=int, default=30, help='frames per sequence')
    ap.add_argument('--things', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=1, help='sequences that are run and not timed')
    ap.add_argument('--repeats', type=int, default=3, help='each setting is measured this often, alternating')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'mots_eval.txt'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_mots_eval measures on the GPU; none is visible')
    H, W = 1024, 2048
    seqs = sequences(H, W, args.things, args.frames, args.length)
    runs = []
    for _ in range(args.repeats):
        runs.append(measure_mots(seqs, args.warmup))
        runs.append(measure_video(seqs, (1, 2, 3, 4), args.warmup))
        runs.append(measure_transitions(seqs, args.warmup))

    def med(what):
        v = sorted(r['device_us_p50'] for r in runs if r['what'] == what)
        return v[len(v) // 2]
    mots, vpq, rle = med('MOTSEvaluator.add_frame'), med('add_frame'), med('upsnet_pan_rle_transitions')
    report = {'what': 'MOTSEvaluator.add_frame and upsnet_pan_rle_transitions per frame, beside VideoPanopticEvaluator.add_frame',
              'height': H, 'width': W, 'things': args.things, 'frames': args.frames, 'sequence_length': args.length,
              'warmup_sequences': args.warmup, 'repeats': args.repeats, 'mots_frame_step_us': mots, 'vpq_frame_step_us_windows_1234': vpq,
              'rle_transitions_us': rle, 'mots_over_vpq': round(mots / vpq, 3), 'runs': runs}
    text = json.dumps(report, indent=1)
    head = ('MOTS scoring on the device: csrc/mots_eval.hip through dataset/mots.py (DESIGN.md section 4.25)\n'
            '1x MI355X; tools/bench_mots_eval.py --frames %d --length %d --things %d\n\n' % (args.frames, args.length, args.things))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(head + text + '\n')
    print(text)


if __name__ == '__main__':
    main()
