"""Box voting (upsnet_amd/tta.py, csrc/box_vote.hip): what the two voting launches cost beside the augmented forward.

    python tools/bench_box_vote.py [--out profiles/box_vote.txt] [--workloads NAME ...] [--augs 1 2 8] [--thresh 0.8]

Per workload (UPSNet-50 at 1024x2048, UPSNet-101-DCN at 800x1333; seeded synthetic weights and image) and per number of augmentations A
(1: the base alone, what --bbox_vote runs on its own; 2: base + flip; 8: base, 0.75x, 1.25x and 0.5x, each with its flip):
  * the two voting launches (the class-wise and the panoptic kept list) on the tensors of a real forward_tta of that image: graph-replay
    time (tools/gputime.py: median of 5 replays of 20 calls, no host cost in the number);
  * the kept rows, and how many voters they had (least / median / most, rows with two or more), counted by the numpy restatement of the
    rule (tests/box_vote_ref.py), which the device result is also compared with bit for bit;
  * forward_tta in ms per image with voting off and on (host clock around the call and a device synchronise, median of `--steps` images
    after 2 warm-ups), and the two launches as a share of the run with voting off (the yardstick: below 2 %).
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
    ap.add_argument('--thresh', type=float, default=0.8)
    ap.add_argument('--steps', type=int, default=8)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_box_vote needs a GPU"
    import box_vote_ref as ref
    from upsnet_amd import build, ops, tta
    from upsnet_amd.config.config import config, update_config_dict
    from upsnet_amd.synthetic import build_model, make_image_u8
    from upsnet_amd.upsnet_end2end_test import WORKLOADS
    lines = ["# tools/bench_box_vote.py on %s; library source hash %s" % (torch.cuda.get_device_name(0), build._source_hash())]

    def say(s):
        lines.append(s)
        print(s, flush=True)

    host = lambda t: t.detach().cpu().numpy()
    for name in args.workloads:
        preset, H, W, gain = WORKLOADS[name]
        update_config_dict(preset)
        config.test.aug_scales, config.test.aug_flip, config.test.bbox_vote = [], False, False
        config.test.bbox_vote_thresh = args.thresh
        model = build_model(cls_gain=gain, device='cuda')
        img = make_image_u8(H, W, seed=0, device='cuda')
        s0 = config.test.scales[0]
        say("# %s: %dx%d, %d classes, rpn_post_nms_top_n %d, score_thresh %g, vote IoU >= %g"
            % (name, H, W, config.dataset.num_classes, config.test.rpn_post_nms_top_n, config.test.score_thresh, args.thresh))
        weights = config.network.bbox_reg_weights
        for A in args.augs:
            rel, flip = AUG_SETS[A]
            config.test.aug_scales, config.test.aug_flip = [int(round(s0 * r)) for r in rel], flip
            assert len(tta.augmentation_list()) == A
            config.test.bbox_vote = False
            off_ms = tta_ms(model, img, args.steps)
            config.test.bbox_vote = True
            on_ms = tta_ms(model, img, args.steps)
            out, parts = model.forward_tta(img, return_parts=True)
            torch.cuda.synchronize()
            st, it = parts['bbox_vote']
            rois, delta, prob, n_rois = parts['merged_rois'], parts['merged_delta'], parts['merged_prob'], parts['merged_n_rois']
            im = torch.from_numpy(parts['im_info'][0].copy()).cuda()
            say("  A = %d  union %d of %d rows" % (A, int(n_rois.item()), rois.shape[0]))
            total_us = 0.0
            for which, sel in (('det', model.mask_roi), ('pan', model.mask_roi_panoptic)):
                pre, cls = parts[which + '_boxes_prevote'].contiguous(), parts[which + '_cls'].contiguous()
                num = torch.tensor([pre.shape[0]], dtype=torch.int32, device='cuda')
                clip = bool(sel.clip_boxes)
                fn = lambda: ops.box_vote(rois, delta, prob, im, pre, cls, num, st, it, weights, n_rois, clip_boxes=clip)
                with torch.no_grad():
                    us = gpu_time(fn)
                    got = host(fn())
                want, counts = ref.box_vote(host(rois), host(delta), host(prob), int(n_rois.item()), parts['im_info'][0], weights, clip,
                                            host(pre), host(cls), pre.shape[0], st, it, want_counts=True)
                same = got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32))
                moved = float(np.abs(got[:, 1:] - host(pre)[:, 1:]).max()) if len(counts) else 0.0
                total_us += us
                say("    box_vote %s  %8.1f us  %3d kept rows; voters least %d median %d most %d, %d rows with >= 2; largest move %.2f px; "
                    "%s the restatement" % (which, us, len(counts), min(counts), median(counts), max(counts), sum(c >= 2 for c in counts),
                                            moved, 'bit-equal to' if same else 'DIFFERS FROM'))
            say("    forward_tta %.2f ms/img with voting off, %.2f with voting on; the two voting launches %.1f us = %.3f %% of the run "
                "with voting off" % (off_ms, on_ms, total_us, 100.0 * total_us * 1e-3 / off_ms))
            del out, parts
        del model
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
