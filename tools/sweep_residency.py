"""Same-process sweep of residency caps (csrc/residency.h, upsnet_residency_tuning) on the benchmark workload: one model, the graphs
re-captured for every setting, two images in flight (development aid; profiles/residency_sweep.txt was written from it). The model asks
for the measured defaults around its capture; here that call is answered with the setting under test. One line per run; the setting
without caps is interleaved to show the same-build spread.
Usage (on the GPU box): python tools/sweep_residency.py single                 # one family at a time, then everything at 1 and at 2
                        python tools/sweep_residency.py <tag> '{}' '{"pair32": 1}' '{"pair32": 1, "ksw": 2}' ...   # SWEEP_STEPS=300 for longer runs"""
import gc
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from upsnet_amd._lib import lib
from upsnet_amd.upsnet_end2end_test import upsnet_test, resolve_workload
from upsnet_amd.config.config import update_config_dict
from upsnet_amd.synthetic import build_model

NAMES = ['frag', 'pair', 'pair32', 'ksw', 'w3264', 'w3232', 'dcn']
STEPS = int(os.environ.get('SWEEP_STEPS', '150'))
which = sys.argv[1] if len(sys.argv) > 1 else 'single'

l = lib()
real = l.upsnet_residency_tuning
current = {}


def wrapper(kernel, cap):
    if kernel == -1 and cap == -1:
        real(-1, 0)
        for k, c in current.items():
            real(NAMES.index(k), c)
        return 0
    return real(kernel, cap)


l.upsnet_residency_tuning = wrapper

if which == 'single':
    CONFIGS = [{}, {'frag': 1}, {'frag': 2}, {'frag': 3}, {}, {'pair': 1}, {'pair': 2}, {'pair32': 1}, {}, {'ksw': 1}, {'ksw': 2}, {'ksw': 3},
               {}, {'w3264': 1}, {'w3232': 1}, {'dcn': 1}, {'dcn': 2}, {},
               {k: 1 for k in NAMES}, {k: 2 for k in NAMES}, {}]
else:
    CONFIGS = [json.loads(a) for a in sys.argv[2:]]

preset, sizes, gain = resolve_workload('upsnet50_cityscapes_1024x2048')
update_config_dict(preset)
model = build_model(cls_gain=gain, device=torch.device('cuda'), pipeline='fused')
for i, cfg in enumerate(CONFIGS):
    current.clear()
    current.update(cfg)
    model._graphs = {}
    gc.collect()
    torch.cuda.synchronize()
    res = upsnet_test('upsnet50_cityscapes_1024x2048', steps=STEPS, warmup=10, model=model, in_flight=2)
    net = sorted(res['net_times'])
    line = "run %2d caps %-40s value %7.2f img/s  p50 %.3f ms  p10 %.3f ms" % (
        i, json.dumps(cfg, sort_keys=True), STEPS / res['elapsed'], 1000 * net[len(net) // 2], 1000 * net[len(net) // 10])
    print(line, flush=True)
real(-1, 0)
