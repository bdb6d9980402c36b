"""Test-time augmentation (upsnet_amd/tta.py, csrc/tta.hip): what the four merge launches cost beside the forwards they merge.

    python tools/bench_tta.py [--out profiles/tta.txt] [--workloads NAME ...] [--augs 2 4 8]

Per workload (UPSNet-50 at 1024x2048 with 19 semantic classes, UPSNet-101-DCN at 800x1333 with 133; seeded synthetic weights and image)
and per number of augmentations A (2: base + flip; 4: base and 0.75x, each with its flip; 8: base, 0.75x, 1.25x and 0.5x, each with
its flip):
  * each merge entry point on the tensors of a real augmented forward of that image: graph-replay time (tools/gputime.py: median of 5
    replays of 20 calls, no host cost in the number), the least bytes it must move computed from the shapes (every input element read
    once, every output element written once) over that time, and that rate against the 6.3 TB/s an element-wise kernel reaches here;
  * forward_tta in ms per image (host clock around the call and a device synchronise, median of `--steps` images after 2 warm-ups);
  * the plain forward, strictly serial (forward + synchronise per image, bench.py's ms_per_img_serial window), at every augmentation's
    blob size, and their sum; the four merge launches as a share of that sum (the yardstick: below 2 %).
No time is asserted anywhere; the numbers are what this run measured."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch

from gputime import gpu_time

HBM_ELEMENTWISE_TBS = 6.3
AUG_SETS = {2: ([], True), 4: ([0.75], True), 8: ([0.75, 1.25, 0.5], True)}


def median(xs):
    return sorted(xs)[len(xs) // 2]


def serial_ms(model, data, steps):
    ts = []
    with torch.no_grad():
        for k in range(steps + 4):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            model({'data': data['data'], 'im_info': data['im_info']})
            torch.cuda.synchronize()
            if k >= 4:
                ts.append(time.perf_counter() - t0)
    return 1000.0 * median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--workloads', nargs='+', default=['upsnet50_cityscapes_1024x2048', 'upsnet101dcn_coco_800x1333'])
    ap.add_argument('--augs', nargs='+', type=int, default=[2, 4, 8])
    ap.add_argument('--steps', type=int, default=8)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_tta needs a GPU"
    from upsnet_amd import build, ops, tta
    from upsnet_amd.config.config import config, update_config_dict
    from upsnet_amd.dataset.blob import get_image_blob
    from upsnet_amd.synthetic import build_model, make_image_u8
    from upsnet_amd.upsnet_end2end_test import WORKLOADS
    lines = ["# tools/bench_tta.py on %s; library source hash %s" % (torch.cuda.get_device_name(0), build._source_hash())]

    def say(s):
        lines.append(s)
        print(s, flush=True)

    for name in args.workloads:
        preset, H, W, gain = WORKLOADS[name]
        update_config_dict(preset)
        config.test.aug_scales, config.test.aug_flip = [], False
        model = build_model(cls_gain=gain, device='cuda')
        img = make_image_u8(H, W, seed=0, device='cuda')
        s0 = config.test.scales[0]
        S, C = config.dataset.num_seg_classes, config.dataset.num_classes
        say("# %s: %dx%d, %d semantic classes, %d classes, rpn_post_nms_top_n %d" % (name, H, W, S, C, config.test.rpn_post_nms_top_n))
        serial = {}
        for A in args.augs:
            rel, flip = AUG_SETS[A]
            config.test.aug_scales, config.test.aug_flip = [int(round(s0 * r)) for r in rel], flip
            augs = tta.augmentation_list()
            assert len(augs) == A
            for _ in range(2):
                out, parts = model.forward_tta(img, return_parts=True)
            torch.cuda.synchronize()
            ts = []
            for _ in range(args.steps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                model.forward_tta(img)
                torch.cuda.synchronize()
                ts.append(time.perf_counter() - t0)
            tta_ms = 1000.0 * median(ts)
            for target, max_size, _ in augs:          # (a flipped blob has the size of the unflipped one)
                if (target, max_size) not in serial:
                    serial[(target, max_size)] = serial_ms(model, get_image_blob(img, target, max_size), args.steps + 4)
            sum_ms = sum(serial[(t, m)] for t, m, _ in augs)

            q, r, wr, fl, cell = parts['q'], parts['r'], parts['resized_w'], parts['flip'], parts['cell']
            n = int(parts['boxes'].shape[0])
            n_valid = int(parts['merged_n_rois'].item())
            R, D = parts['rois'][0].shape[0], parts['delta'][0].shape[1]
            ms = parts['mask_logits'][0].shape[-1]
            entries = [
                ('tta_seg_merge', lambda: ops.tta_seg_merge(parts['score'], q, wr, fl, cell),
                 4.0 * (sum(t.numel() for t in parts['score']) + parts['merged_score'].numel())),
                ('tta_roi_union', lambda: ops.tta_roi_union(parts['rois'], parts['delta'], parts['prob'], parts['n_rois'], r, wr, fl),
                 4.0 * (5 + D + C) * (n_valid + A * R)),
                ('tta_boxes_to_aug', lambda: ops.tta_boxes_to_aug(parts['boxes'], q, wr, fl), 4.0 * 5 * n * (1 + A)),
                ('tta_mask_merge', lambda: ops.tta_mask_merge(parts['mask_logits'], fl), 4.0 * (A + 1) * n * C * ms * ms),
            ]
            say("  A = %d  %s" % (A, ' '.join('%dx%d%s' % (int(i[0]), int(i[1]), 'f' if f else '') for i, f in zip(parts['im_info'], fl))))
            say("    n_rois %s -> union %d of %d rows; %d final boxes (n_det %d, n_extra %d)"
                % ([int(v.item()) for v in parts['n_rois']], n_valid, A * R, n, parts['n_det'], parts['n_extra']))
            total_us = 0.0
            with torch.no_grad():
                for label, fn, nbytes in entries:
                    us = gpu_time(fn)
                    total_us += us
                    tbs = nbytes / us * 1e-6
                    say("    %-18s %9.1f us  %8.3f MB  %6.3f TB/s  %5.1f %% of %.1f TB/s"
                        % (label, us, nbytes * 1e-6, tbs, 100.0 * tbs / HBM_ELEMENTWISE_TBS, HBM_ELEMENTWISE_TBS))
            say("    forward_tta %.2f ms/img; plain forward serial: %s = %.2f ms; four merge launches %.1f us = %.2f %% of that sum"
                % (tta_ms, ' + '.join('%.2f' % serial[(t, m)] for t, m, _ in augs), sum_ms, total_us, 100.0 * total_us * 1e-3 / sum_ms))
            del out, parts
        del model
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
