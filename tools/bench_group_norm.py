"""GroupNorm(32, C) kernels (csrc/group_norm.hip: stats + apply, the one-launch small form, the rows form) against
torch.nn.functional.group_norm + the separate ReLU / upsample-add it replaces, on the same channels-last input in the same process, at
the shapes the heads with with_norm = 'group_norm' produce: the four pyramid maps of 1024x2048 and of 800x1333 (padded to 800x1344) at
256 channels (plain + ReLU, and the FPN top-down form with the nearest x2 residual), the semantic subnet's 128-channel maps, the four
levels in one multi-map launch, the mask head's [100,256,14,14] and the box head's [1000,1024].

    python tools/bench_group_norm.py [--out profiles/group_norm.txt]

Times are graph-replay times (tools/gputime.py: no host cost in the number), the median of 5 replays of 20 calls. GB/s = the bytes the
algorithm needs (map read twice and written once, + the residual read once) over that time; maps below ~85 MB stay in the 256 MiB
Infinity Cache between calls, for both contenders alike. `diff` = max |ours - torch| (fp32 both)."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch
import torch.nn.functional as F

from upsnet_amd import build, group_norm
from gputime import gpu_time

EPS = 1e-5


def _maps(shapes, c, n=1, seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(n, c, h, w, generator=g).cuda().contiguous(memory_format=torch.channels_last) for h, w in shapes]


def _affine(c):
    g = torch.Generator().manual_seed(c)
    return (1.0 + (torch.rand(c, generator=g) - 0.5)).cuda(), (torch.rand(c, generator=g) - 0.5).cuda()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_group_norm needs a GPU"
    lines = ["# tools/bench_group_norm.py on %s; library source hash %s; chunk %d pixels" %
             (torch.cuda.get_device_name(0), build._source_hash(), group_norm.chunk_pixels()),
             "# %-34s %-12s %9s %9s %7s %8s %9s" % ("shape", "epilogue", "ours us", "torch us", "ratio", "GB/s", "diff")]

    def row(name, epi, ours, theirs, nbytes):
        with torch.no_grad():
            a, b = ours(), theirs()
            diff = max(float((x - y).abs().max()) for x, y in zip(a, b))
            t0, t1 = gpu_time(ours), gpu_time(theirs)
        lines.append("  %-34s %-12s %9.1f %9.1f %7.2f %8.0f %9.2e" % (name, epi, t0, t1, t1 / t0, nbytes / t0 * 1e-3, diff))
        print(lines[-1], flush=True)

    pyr = {'1024x2048': [(256, 512), (128, 256), (64, 128), (32, 64)], '800x1333': [(200, 336), (100, 168), (50, 84), (25, 42)]}
    for c in (256, 128):
        gamma, beta = _affine(c)
        for im, shapes in pyr.items():
            if c == 128 and im != '1024x2048':
                continue
            xs = _maps(shapes, c)
            for lvl, x in zip(('P2', 'P3', 'P4', 'P5'), xs):
                nb = 3.0 * x.numel() * 4
                row("%s %s [1,%d,%d,%d]" % (im, lvl, c, x.shape[2], x.shape[3]), "relu",
                    lambda x=x: [group_norm.group_norm(x, gamma, beta, EPS, relu=True)],
                    lambda x=x: [torch.relu_(F.group_norm(x, 32, gamma, beta, EPS))], nb)
            if c == 256:
                for lvl, x, r in zip(('P2', 'P3', 'P4'), xs[:3], xs[1:]):
                    nb = 3.0 * x.numel() * 4 + r.numel() * 4
                    row("%s %s [1,%d,%d,%d]" % (im, lvl, c, x.shape[2], x.shape[3]), "+ up(res)",
                        lambda x=x, r=r: [group_norm.group_norm(x, gamma, beta, EPS, residual=r, residual_up=True)],
                        lambda x=x, r=r: [F.group_norm(x, 32, gamma, beta, EPS) + F.interpolate(r, scale_factor=2, mode='nearest')], nb)
            nb = 3.0 * sum(x.numel() for x in xs) * 4
            row("%s P2..P5 one launch, C = %d" % (im, c), "relu",
                lambda xs=xs: group_norm.group_norm_multi(xs, gamma, beta, EPS, relu=True),
                lambda xs=xs: [torch.relu_(F.group_norm(x, 32, gamma, beta, EPS)) for x in xs], nb)
    gamma, beta = _affine(256)
    x = _maps([(14, 14)], 256, n=100)[0]
    row("mask head [100,256,14,14]", "relu", lambda: [group_norm.group_norm_small(x, gamma, beta, EPS, relu=True)],
        lambda: [torch.relu_(F.group_norm(x, 32, gamma, beta, EPS))], 3.0 * x.numel() * 4)
    gamma, beta = _affine(1024)
    r = torch.randn(1000, 1024, generator=torch.Generator().manual_seed(1)).cuda()
    row("box head fc6 [1000,1024]", "relu", lambda: [group_norm.group_norm_small(r, gamma, beta, EPS, relu=True)],
        lambda: [torch.relu_(F.group_norm(r, 32, gamma, beta, EPS))], 2.0 * r.numel() * 4)
    if args.out:
        with open(args.out, 'w') as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
