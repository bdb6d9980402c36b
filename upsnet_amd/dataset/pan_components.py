"""Disconnected fragments removed from 2-channel panoptic maps by connected components, on the device (csrc/pan_components.hip;
DESIGN.md section 4.26).

A (category, instance) pair of a predicted map should be one region, but the panoptic head's per-pixel argmax and the combined merge's
pasted masks both leave specks of a segment far from its body. clean_panoptic labels the connected components of every map and turns
those of fewer than min_area pixels into VOID, except (keep_largest) the largest component of each pair, so a segment never vanishes
entirely. With mode='absorb' (config.test.pan_component_mode) such a component takes the pair of the segment it
shares the longest border with instead, so that a speck of "car 3" in the road becomes road and not a hole. The reference has no such
step; the rules are this project's own, stated in include/upsnet_hip.h and restated in plain numpy in tests/pan_components_ref.py and
tests/pan_absorb_ref.py. Off unless config.test.pan_min_component > 0.

    cleaned = clean_panoptic(pans, min_area=64)                  # uint8 [H,W,3] device tensors (numpy arrays are uploaded)
    cleaned = clean_panoptic(pans, min_area=64, mode='absorb')
"""
import numpy as np
import torch

from .. import ops
from .pq import _check_image

MAX_PIXELS = 1 << 24


def check_params(min_area, connectivity=8):
    """ValueError unless min_area is an integer >= 0 and connectivity is 4 or 8."""
    if isinstance(min_area, bool) or int(min_area) != min_area or min_area < 0:
        raise ValueError("min_area must be an integer >= 0, got %r" % (min_area,))
    if connectivity not in (4, 8):
        raise ValueError("connectivity must be 4 or 8, got %r" % (connectivity,))


MODES = ('void', 'absorb')


def clean_panoptic(pans, min_area, connectivity=8, keep_largest=True, return_stats=False, mode='void'):
    """The maps of `pans` (uint8 [H,W,3]; device tensors, or numpy arrays, which are uploaded) with every connected component of fewer
    than min_area pixels turned into VOID, unless keep_largest and it is the largest of its (category, instance) pair: a list of new
    uint8 [H,W,3] device tensors, the inputs untouched. Five launches per map, nothing waits for the host; one workspace serves
    consecutive maps of one size. return_stats (what clean_pan_result's log line reads): also the int32 [4] device tensor of the sums
    over the maps of (distinct pairs, components, components removed, pixels removed). ValueError before any launch: a map that is not uint8 [H,W,3] or of more than 2^24
    pixels, a bad min_area or connectivity.

    mode='absorb' (eight launches per map): such a component takes the (category, instance) of the kept segment it shares
    the longest border with, and becomes VOID only where it borders none (ops.pan_absorb states the rule). Its stats are int32 [8]: the
    four above, components absorbed, pixels absorbed, (component, donor) pairs voted for, vote table overflow. Any other mode:
    ValueError."""
    if mode not in MODES:
        raise ValueError("mode must be 'void' or 'absorb', got %r" % (mode,))
    workspace_of, clean = ((ops.pan_components_workspace, ops.pan_components) if mode == 'void' else
                           (ops.pan_absorb_workspace, ops.pan_absorb))
    check_params(min_area, connectivity)
    pans = list(pans)
    for pan in pans:
        _check_image('pan_2ch', pan)
        if pan.shape[0] * pan.shape[1] == 0 or pan.shape[0] * pan.shape[1] > MAX_PIXELS:
            raise ValueError("a map of %d x %d pixels cannot be cleaned: H * W must lie in 1..2^24" % (pan.shape[0], pan.shape[1]))
    out, total, ws, ws_key = [], None, None, None
    for pan in pans:
        if isinstance(pan, np.ndarray):
            dev = torch.device('cuda', torch.cuda.current_device())
            pan = torch.from_numpy(np.ascontiguousarray(pan)).to(dev, non_blocking=True)
        if not pan.is_cuda:
            raise RuntimeError("clean_panoptic: the map must be on the device (there is no CPU fallback)")
        key = (int(pan.shape[0]), int(pan.shape[1]), pan.device)
        if key != ws_key:
            ws, ws_key = workspace_of(key[0], key[1], pan.device), key
        cleaned, stats, _ = clean(pan.contiguous(), int(min_area), connectivity, keep_largest, workspace=ws)
        out.append(cleaned)
        if return_stats:
            total = stats if total is None else total + stats.to(total.device)
    if return_stats:
        return out, total
    return out
