"""Soft-NMS in the detection selection (upsnet_amd/tta.py, csrc/detect.hip mroi_soft_kernel): what the soft class-wise
selection costs beside the hard one and beside the augmented forward.

    python tools/bench_soft_select.py [--out profiles/soft_select.txt] [--workloads NAME ...] [--augs 1 2 8]

Per workload (UPSNet-50 at 1024x2048, UPSNet-101-DCN at 800x1333; seeded synthetic weights and image) and per number of augmentations A
(1: the base alone, what --soft_nms runs on its own; 2: base + flip; 8: base, 0.75x, 1.25x and 0.5x, each with its flip), on the union
tensors of a real forward_tta of that image:
  * ops.mask_roi (hard) and ops.mask_roi_soft (linear, gaussian) with the model's thresholds: graph-replay time (tools/gputime.py:
    median of 5 replays of 20 calls, no host cost in the number), the rows each returns and how many of them carry a decayed score;
  * the candidates per class above test.score_thresh (the trips of a class are sequential: least / median / most);
  * the soft result against the numpy restatement of the rule (tests/soft_select_ref.py), bit for bit;
  * forward_tta in ms per image with soft-NMS off (host clock around the call and a device synchronise, median of `--steps` images
    after 2 warm-ups), and the ADDED selection time (soft - hard) as a share of it (the yardstick: below 2 %).
No time is asserted anywhere; the numbers are what this run measured."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np
import torch

from gputime import gpu_time

AUG_SETS = {1: ([], False), 2: ([], True), 4: ([0.75], True), 8: ([0.75, 1.25, 0.5], True)}


def median(xs):
    return sorted(xs)[len(xs) // 2]


def tta_ms(model, img, steps):
    for _ in range(2):
        model.forward_tta(img)
    ts = []
    for _ in range(steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        model.forward_tta(img)
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return 1000.0 * median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--workloads', nargs='+', default=['upsnet50_cityscapes_1024x2048', 'upsnet101dcn_coco_800x1333'])
    ap.add_argument('--augs', nargs='+', type=int, default=[1, 2, 8])
    ap.add_argument('--steps', type=int, default=8)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_soft_select needs a GPU"
    import soft_select_ref as ref
    from upsnet_amd import build, ops, tta
    from upsnet_amd.config.config import config, update_config_dict
    from upsnet_amd.synthetic import build_model, make_image_u8
    from upsnet_amd.upsnet_end2end_test import WORKLOADS
    lines = ["# tools/bench_soft_select.py on %s; library source hash %s" % (torch.cuda.get_device_name(0), build._source_hash())]

    def say(s):
        lines.append(s)
        print(s, flush=True)

    host = lambda t: t.detach().cpu().numpy()
    for name in args.workloads:
        preset, H, W, gain = WORKLOADS[name]
        update_config_dict(preset)
        config.test.aug_scales, config.test.aug_flip, config.test.bbox_vote, config.test.soft_nms = [], False, False, False
        model = build_model(cls_gain=gain, device='cuda')
        img = make_image_u8(H, W, seed=0, device='cuda')
        s0 = config.test.scales[0]
        sel = model.mask_roi
        st, nt, max_det, clip = sel.score_thresh, sel.nms_thresh, config.test.max_det, bool(sel.clip_boxes)
        sigma, floor = float(config.test.soft_nms_sigma), float(config.test.soft_nms_score_thresh)
        say("# %s: %dx%d, %d classes, rpn_post_nms_top_n %d, score_thresh %g, nms_thresh %g, max_det %d, sigma %g, floor %g"
            % (name, H, W, config.dataset.num_classes, config.test.rpn_post_nms_top_n, st, nt, max_det, sigma, floor))
        weights = config.network.bbox_reg_weights
        for A in args.augs:
            rel, flip = AUG_SETS[A]
            config.test.aug_scales, config.test.aug_flip = [int(round(s0 * r)) for r in rel], flip
            assert len(tta.augmentation_list()) == A
            off_ms = tta_ms(model, img, args.steps)
            out, parts = model.forward_tta(img, return_parts=True)
            torch.cuda.synchronize()
            rois, delta, prob, n_rois = parts['merged_rois'], parts['merged_delta'], parts['merged_prob'], parts['merged_n_rois']
            im = torch.from_numpy(parts['im_info'][0].copy()).cuda()
            n = int(n_rois.item())
            cands = ref.candidates(host(rois), host(delta), host(prob), n, parts['im_info'][0], weights, clip, st)
            per_class = sorted(len(r) for _, r in cands.values())
            say("  A = %d  union %d of %d rows; candidates per class least %d median %d most %d"
                % (A, n, rois.shape[0], per_class[0], median(per_class), per_class[-1]))
            hard = lambda: ops.mask_roi(rois, delta, prob, im, False, st, nt, max_det, weights, n_rois, clip_boxes=clip)
            with torch.no_grad():
                hard_us = gpu_time(hard)
                hard_rows = int(hard()[4].item())
            say("    mask_roi (hard)            %8.1f us  %4d rows" % (hard_us, hard_rows))
            for mname, method in (('linear', 1), ('gaussian', 2)):
                soft = lambda: ops.mask_roi_soft(rois, delta, prob, im, st, nt, max_det, weights, method, sigma, floor, n_rois, clip_boxes=clip)
                with torch.no_grad():
                    us = gpu_time(soft)
                    got = [host(t) for t in soft()]
                want = ref.soft_select(host(rois), host(delta), host(prob), n, parts['im_info'][0], weights, clip, st, nt, max_det, method,
                                       sigma, floor, cands=cands)
                d = len(want['scores'])
                same = int(got[4][0]) == want['num'] and all(
                    np.array_equal(np.ascontiguousarray(g[:d]).view(np.uint8), np.ascontiguousarray(want[k]).view(np.uint8))
                    for g, k in zip(got[:4], ('boxes', 'scores', 'cls', 'src')))
                say("    mask_roi_soft %-9s    %8.1f us  %4d rows of T = %d, %d decayed; %s the restatement; added %.1f us = %.3f %% of "
                    "forward_tta with soft-NMS off (%.2f ms/img)"
                    % (mname, us, want['num'], want['T'], int(ref.decayed(want, host(prob)).sum()), 'bit-equal to' if same else 'DIFFERS FROM',
                       us - hard_us, 100.0 * (us - hard_us) * 1e-3 / off_ms, off_ms))
            del out, parts
        del model
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
