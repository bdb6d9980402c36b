#!/usr/bin/env python
"""Record the state-dict layout (sorted (key, shape) lists, nothing else) of the REFERENCE's head modules built with
with_norm = 'none' and 'group_norm', by importing the reference's own Python modules from /root/reference.

Run where /root/reference exists:   python tests/golden/make_golden_gn.py
The fixture tests/golden/gn_state_dict.json is committed; tests/test_group_norm_cpu.py holds this project's modules to it.

As in make_golden.py the reference cannot be imported as-is: this script supplies, in-process only, an `easydict` stand-in and an empty
stand-ins for the compiled ROIAlign / deformable extensions, and makes Tensor.cuda a no-op (the reference's DeformConv constructor calls it;
no forward is run here, only constructors).
"""
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
sys.path.insert(0, REF)

np.float = float
np.int = int
torch.Tensor.cuda = lambda self, *a, **k: self


class EasyDict(dict):
    def __init__(self, d=None, **kw):
        super().__init__()
        for k, v in dict(d or {}, **kw).items():
            setattr(self, k, v)

    def __setattr__(self, k, v):
        if isinstance(v, dict) and not isinstance(v, EasyDict):
            v = EasyDict(v)
        super().__setitem__(k, v)
        super().__setattr__(k, v)

    __setitem__ = __setattr__


def _module(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    sys.modules[name] = m
    return m


# (this repository ships a regular package called `upsnet` as well: pin the name to the REFERENCE directory)
_module("upsnet", __path__=[os.path.join(REF, "upsnet")])
# (upsnet/models/__init__.py imports the whole network and with it the compiled NMS: only the head modules' files are wanted)
_module("upsnet.models", __path__=[os.path.join(REF, "upsnet", "models")])
_module("easydict", EasyDict=EasyDict)
_module("upsnet.operators._ext", __path__=[])
_module("upsnet.operators._ext.roi_align", roi_align_cuda=None)
_module("upsnet.operators._ext.deform_conv", deform_conv_cuda=None)

from upsnet.config.config import config  # noqa: E402

config.network.fpn_with_gap = False
config.network.mask_size = 28

from upsnet.models.fcn import FCNHead  # noqa: E402
from upsnet.models.fpn import FPN  # noqa: E402
from upsnet.models.rcnn import RCNN, MaskBranch  # noqa: E402
from upsnet.models.rpn import RPN  # noqa: E402

for _cls in (FPN, RPN, RCNN, MaskBranch, FCNHead):   # really the reference's classes
    assert sys.modules[_cls.__module__].__file__.startswith(REF + os.sep), (_cls, sys.modules[_cls.__module__].__file__)

# the constructor arguments tests/test_group_norm_cpu.py repeats
BUILD = {
    'FPN': lambda wn: FPN(feature_dim=256, with_norm=wn),
    'RPN': lambda wn: RPN(num_anchors=3, input_dim=256, with_norm=wn),
    'RCNN': lambda wn: RCNN(9, 9, dim_in=256, with_norm=wn),
    'MaskBranch': lambda wn: MaskBranch(9, dim_in=256, with_norm=wn),
    'FCNHead': lambda wn: FCNHead(256, 19, num_layers=3, with_norm=wn, upsample_rate=4),
}


def main():
    rec = {}
    for name, make in BUILD.items():
        rec[name] = {wn: sorted((k, list(v.shape)) for k, v in make(wn).state_dict().items()) for wn in ('none', 'group_norm')}
    path = os.path.join(HERE, "gn_state_dict.json")
    with open(path, "w") as f:
        json.dump(rec, f, indent=0, sort_keys=True)
        f.write("\n")
    print("wrote", path, {k: {wn: len(v) for wn, v in d.items()} for k, d in rec.items()})


if __name__ == "__main__":
    main()
