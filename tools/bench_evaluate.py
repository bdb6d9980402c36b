#!/usr/bin/env python
"""Time a full evaluation run (python -m upsnet_amd.evaluate) over a generated Cityscapes-layout set of 1024 x 2048 PNG images: the
per-image data_time (host decode + blob), net_time (host time blocked on the network) and post_time (box scaling, mask RLE, label-map
restore) of the run's own log line, reported as p50 / p90 over the images after the first 10 (the reference's net_time window).
The images are seeded (4 x 4 colour blocks plus per-pixel noise, so that PNG decoding costs about what a photograph's does) and
listed in an image_info JSON, so the run infers and writes results_list.pkl but evaluates nothing. Seeded synthetic weights.
Prints one JSON line.

    python tools/bench_evaluate.py --root /tmp/cs_bench [--images 200] [--in-flight 2] [--out results/bench_evaluate.json]
"""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

YAML = """
output_path: "%(root)s/output"
symbol: resnet_50_upsnet
dataset:
  num_classes: 9
  num_seg_classes: 19
  dataset: Cityscapes
  dataset_path: "%(root)s"
  image_set: train
  test_image_set: test
network:
  fcn_num_layers: 2
test:
  scales:
  - 1024
  max_size: 2048
"""


def make_image(path, seed, H, W):
    from PIL import Image
    rng = np.random.default_rng(seed)
    blocks = rng.integers(0, 256, (H // 4, W // 4, 3))
    im = np.repeat(np.repeat(blocks, 4, 0), 4, 1) + rng.integers(-8, 9, (H, W, 3))
    Image.fromarray(np.clip(im, 0, 255).astype(np.uint8)).save(path, compress_level=1)


def make_dataset(root, n, H, W, threads=8):
    img_dir = os.path.join(root, 'images')
    os.makedirs(img_dir, exist_ok=True)
    os.makedirs(os.path.join(root, 'annotations'), exist_ok=True)
    names = ['bench_%06d_000019_leftImg8bit.png' % i for i in range(n)]
    with ThreadPoolExecutor(max_workers=threads) as pool:
        list(pool.map(lambda i: make_image(os.path.join(img_dir, names[i]), 1000 + i, H, W), range(n)))
    images = [{'id': i, 'file_name': names[i], 'height': H, 'width': W} for i in range(n)]
    with open(os.path.join(root, 'annotations', 'image_info_test.json'), 'w') as f:
        json.dump({'images': images, 'categories': []}, f)
    cfg = os.path.join(root, 'bench_cityscapes.yaml')
    with open(cfg, 'w') as f:
        f.write(YAML % dict(root=root))
    return cfg


def pct(v, q):
    return float(np.percentile(np.asarray(v), q)) if len(v) else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", required=True, help="directory for the generated dataset and the run's output")
    ap.add_argument("--images", type=int, default=200)
    ap.add_argument("--height", type=int, default=1024)
    ap.add_argument("--width", type=int, default=2048)
    ap.add_argument("--in-flight", type=int, default=2)
    ap.add_argument("--skip", type=int, default=10, help="first images left out of the percentiles")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    t0 = time.perf_counter()
    cfg = make_dataset(a.root, a.images, a.height, a.width)
    gen_s = time.perf_counter() - t0
    from upsnet_amd.evaluate import main as run
    t0 = time.perf_counter()
    res = run(['--cfg', cfg, '--synthetic_weights', '--in-flight', str(a.in_flight)])
    wall = time.perf_counter() - t0
    times = {k: v[a.skip:] for k, v in res['times'].items()}
    out = dict(images=a.images, size=[a.height, a.width], in_flight=a.in_flight, generate_s=round(gen_s, 1), run_wall_s=round(wall, 2),
               percentiles_over=len(times['net_time']))
    for k, v in times.items():
        out[k + '_p50_ms'] = round(1e3 * pct(v, 50), 2)
        out[k + '_p90_ms'] = round(1e3 * pct(v, 90), 2)
    # restore kernel traffic at scale 1: two int64 source reads and two uint8 writes per output pixel
    out['restore_bytes_per_image'] = a.height * a.width * (2 * 8 + 2)
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == "__main__":
    main()
