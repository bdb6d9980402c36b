"""Panoptic confidence on the device (csrc/panoptic.hip: panoptic_fuse_up_conf_kernel, csrc/pan_confidence.hip):
what the option costs at the benchmark shape, 1024 x 2048 with about 30 instances, in one visit. Alternating repeats, the median of
GPU event pairs around single calls:
  * ops.panoptic_fuse_up (label maps only) against ops.panoptic_fuse_up_conf (label maps and the confidence plane) on the same inputs,
    and both entry points again straight through ctypes on preallocated outputs ("raw": no wrapper work between the two events); with
    --parent-lib <libupsnet_hip.so of the parent commit> also upsnet_panoptic_fuse_up of that build, raw on the same pointers, so that
    the label-only kernel is compared across the two builds;
  * ops.pan_segment_scores (three launches) and ops.pan_score_filter (one) on a unified 2-channel map of that size against
    PanopticEvaluator.add of the same map scored against itself (the pq_accumulate pixel pass and its table kernels).
Writes the report to profiles/pan_confidence.txt (--out; appended below whatever the file holds up to the marker line) and prints its JSON.

    python tools/bench_pan_confidence.py [--instances 30] [--calls 200] [--repeats 5] [--parent-lib PATH]
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

MARK = '==== measured (tools/bench_pan_confidence.py) ====\n'


def median_us(fn, calls, warmup=10):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    pairs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(calls)]
    for e0, e1 in pairs:
        e0.record()
        fn()
        e1.record()
    torch.cuda.synchronize()
    us = sorted(1000.0 * e0.elapsed_time(e1) for e0, e1 in pairs)
    return us[len(us) // 2]


def head_inputs(instances, seed=0):
    """Cityscapes-shaped inputs of the fused head: score [1,19,256,512] channels_last, `instances` boxes of 40..400 pixels a side."""
    from upsnet_amd import ops
    rng = np.random.default_rng(seed)
    H, W, S, C = 1024, 2048, 19, 9
    score = torch.from_numpy(rng.normal(0, 3, size=(1, S, H // 4, W // 4)).astype(np.float32)).cuda().contiguous(memory_format=torch.channels_last)
    wh = rng.uniform(40, 400, size=(instances, 2))
    xy = rng.uniform(0, 1, size=(instances, 2)) * (np.array([W, H]) - wh)
    rois5 = np.zeros((instances, 5), np.float32)
    rois5[:, 1:3], rois5[:, 3:5] = xy, xy + wh - 1
    prob = np.sort(rng.uniform(0.6, 1.0, instances).astype(np.float32))[::-1].copy()
    logit = rng.normal(0.3, 2, size=(instances, 1, 28, 28)).astype(np.float32)
    cls = rng.integers(1, C, size=instances).astype(np.int64)
    t = [torch.from_numpy(a).cuda() for a in (rois5, prob, logit, cls)]
    keep, num, real = ops.mask_removal(t[0][:, 1:].contiguous(), t[1], t[2], t[3], C - 1, (H, W))
    cmap = torch.zeros((C,), dtype=torch.int64)
    cmap[1:] = torch.arange(S - C + 1, S)
    return dict(score=score, rois5=t[0], logit=t[2], cls=t[3], keep=keep, num=num, real=real, cmap=cmap.cuda(), s_stuff=S - (C - 1),
                kept=int(num.item()))


def raw_call(path, inp, conf=False):
    """upsnet_panoptic_fuse_up (or, with conf, upsnet_panoptic_fuse_up_conf) of the library at `path` -- this build's or another's --
    straight through ctypes on the same device tensors and preallocated outputs: no wrapper work between the two events."""
    from upsnet_amd._lib import ptr, stream
    lib = ctypes.CDLL(path)
    P, I = ctypes.c_void_p, ctypes.c_int
    entry = lib.upsnet_panoptic_fuse_up_conf if conf else lib.upsnet_panoptic_fuse_up
    entry.restype = I
    entry.argtypes = [P, P, I, I, I, I, I, I, P, P, P, P, P, P, I, I, P, P, P] + ([P] if conf else [])
    sc = inp['score']
    _, S, Hs, Ws = sc.shape
    m = inp['rois5'].shape[0]
    logit = inp['logit'].reshape(m, -1).contiguous()
    pan = torch.empty((1, Hs * 4, Ws * 4), dtype=torch.int64, device='cuda')
    sem = torch.empty((1, Hs * 4, Ws * 4), dtype=torch.int64, device='cuda')
    extra = (ptr(torch.empty((1, Hs * 4, Ws * 4), dtype=torch.uint8, device='cuda')),) if conf else ()
    args = (stream(), ptr(sc), 1, S, Hs, Ws, 4, inp['s_stuff'], ptr(inp['rois5']), ptr(logit), ptr(inp['cls']), ptr(inp['keep']),
            ptr(inp['num']), ptr(inp['real']), m, 28, ptr(inp['cmap']), ptr(pan), ptr(sem)) + extra

    def call():
        assert entry(*args) == 0
    call.keep = (logit, extra)      # (the pointers in `args` stay valid as long as the closure lives)
    return call, pan, sem


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--instances', type=int, default=30)
    ap.add_argument('--calls', type=int, default=200)
    ap.add_argument('--repeats', type=int, default=5, help='each variant is measured this often, alternating')
    ap.add_argument('--parent-lib', default=None)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'pan_confidence.txt'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_pan_confidence measures on the GPU; none is visible')
    from upsnet_amd import ops
    from upsnet_amd._lib import lib
    from upsnet_amd.dataset.pan_format import panoptic_format
    from upsnet_amd.dataset.pq import PanopticEvaluator
    from conftest import gen_panoptic_maps
    from oracle import ops as oops

    inp = head_inputs(args.instances)
    a = (inp['score'], 4, inp['s_stuff'], inp['rois5'], inp['logit'], inp['cls'], inp['keep'], inp['num'], inp['real'], inp['cmap'])
    variants = {'fuse_up': lambda: ops.panoptic_fuse_up(*a), 'fuse_up_conf': lambda: ops.panoptic_fuse_up_conf(*a)}
    pan, sem, conf = ops.panoptic_fuse_up_conf(*a)
    pan0, sem0 = ops.panoptic_fuse_up(*a)
    assert torch.equal(pan, pan0) and torch.equal(sem, sem0)
    from upsnet_amd._lib import LIB_PATH
    for name, path, with_conf in (('fuse_up_raw', LIB_PATH, False), ('fuse_up_conf_raw', LIB_PATH, True),
                                  ('fuse_up_raw_parent_build', args.parent_lib, False)):
        if path:
            call, ppan, psem = raw_call(path, inp, with_conf)
            call()
            assert torch.equal(ppan, pan) and torch.equal(psem, sem), "%s: the label maps differ" % name
            variants[name] = call

    rng = np.random.default_rng(1)
    seg, p, cls = gen_panoptic_maps(rng, 1024, 2048, args.instances)
    map_2ch = torch.from_numpy(oops.get_unified_pan_result(seg, p, cls, 19, 9)).cuda()
    plane = conf[0].contiguous()
    ws = torch.zeros((int(lib().upsnet_pan_segment_scores_workspace_bytes()),), dtype=torch.uint8, device='cuda')
    table = torch.zeros((int(lib().upsnet_pan_segment_scores_table_ints()),), dtype=torch.int32, device='cuda')
    out = torch.zeros_like(map_2ch)
    cats = {c: {'id': c, 'isthing': int(c > 10), 'color': [c, 255 - c, 7]} for c in range(19)}
    rgb, info = panoptic_format(map_2ch, cats)
    ev = PanopticEvaluator(cats)
    variants['segment_scores'] = lambda: ops.pan_segment_scores(map_2ch, plane, workspace=ws, table=table)
    variants['score_filter'] = lambda: ops.pan_score_filter(map_2ch, table, 0.5, out=out)
    variants['pq_add'] = lambda: ev.add(map_2ch, rgb, info)

    runs = {k: [] for k in variants}
    for _ in range(args.repeats):
        for k, fn in variants.items():
            runs[k].append(round(median_us(fn, args.calls), 2))
    med = {k: sorted(v)[len(v) // 2] for k, v in runs.items()}
    report = {'what': 'median device time of one call, us', 'height': 1024, 'width': 2048, 'instances': args.instances,
              'kept_instances': inp['kept'], 'calls': args.calls, 'repeats': args.repeats, 'runs_us': runs, 'median_us': med,
              'conf_over_labels_only': round(med['fuse_up_conf'] / med['fuse_up'], 3),
              'conf_over_labels_only_raw': round(med['fuse_up_conf_raw'] / med['fuse_up_raw'], 3),
              'segment_scores_over_pq_add': round(med['segment_scores'] / med['pq_add'], 3)}
    if args.parent_lib:
        report['labels_only_raw_over_parent_build'] = round(med['fuse_up_raw'] / med['fuse_up_raw_parent_build'], 3)
    text = json.dumps(report, indent=1)
    keep = ''
    if os.path.exists(args.out):
        with open(args.out) as f:
            keep = f.read().split(MARK)[0]
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(keep + MARK + '1x MI355X; tools/bench_pan_confidence.py --instances %d --calls %d --repeats %d%s\n\n'
                % (args.instances, args.calls, args.repeats, ' --parent-lib <parent build>' if args.parent_lib else '') + text + '\n')
    print(text)


if __name__ == '__main__':
    main()
