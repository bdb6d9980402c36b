"""Device side of the ground-truth preparation (csrc/gt_prepare.hip): tensor plumbing over upsnet_gt_prepare
and the panoptic-to-semantic conversion through csrc/pan_format.hip's relabel kernel. dataset/prepare.py is the host layer; ops.py
re-exports these functions."""
import numpy as np
import torch

from .._lib import check, dense, lib, ptr, require_cuda, stream, written

GT_PREPARE_SEGMENTS = 4096      # default segment capacity of gt_prepare (a Cityscapes image holds a few hundred)
GT_ROW = 9                      # ints per segment row: v, label, train id, iscrowd, area, x_min, y_min, x_max, y_max
GT_STATUS = 8                   # segments | instances | transitions | flags | labelIds mismatches | 0 0 0
GT_FLAG_SEGMENTS, GT_FLAG_TRANSITIONS, GT_FLAG_RANGE = 1, 2, 4


def gt_prepare_workspace(device, seg_capacity=GT_PREPARE_SEGMENTS):
    """Workspace of gt_prepare_launch for `seg_capacity` segments, zeroed once here (csrc/fill.hip); every call leaves it ready for
    the next, also one that overflowed."""
    nbytes = int(lib().upsnet_gt_prepare_workspace_bytes(int(seg_capacity)))
    if nbytes == 0:
        raise ValueError("gt_prepare_workspace: segment capacity %d outside 1..65536" % seg_capacity)
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=device)
    check(lib().upsnet_zero_fill(stream(), ptr(ws), nbytes), "zero_fill")
    return ws


def gt_prepare_default_transitions(height, width):
    """Default transition capacity, which real scenes stay far below (two per position is the bound); the status words carry the true
    count, at which gt_prepare and CityscapesPreparer run an image that outgrew it once more."""
    return int(height) * int(width) // 4 + 4096


def gt_prepare_launch(ids, tables, label_ids=None, seg_capacity=GT_PREPARE_SEGMENTS, trans_capacity=None, workspace=None):
    """One Cityscapes instanceIds map on the device (include/upsnet_hip.h: upsnet_gt_prepare): ids int32 [H,W]; tables int32 [3,256]
    device tensor (train id, hasInstances, thing row per label); label_ids uint8 [H,W] or None. Returns the device tensors
    (train_map uint8 [H,W], rgb uint8 [H,W,3], table int32 [seg_capacity,9], trans_off int32 [seg_capacity+1], trans int32
    [trans_capacity], status int32 [8]) without synchronising; gt_prepare reads them."""
    require_cuda(ids, tables, label_ids, workspace)
    if ids.dtype != torch.int32 or ids.dim() != 2 or ids.numel() == 0:
        raise ValueError("gt_prepare: ids must be a non-empty int32 [H,W] map, got %s %s" % (tuple(ids.shape), ids.dtype))
    if tables.dtype != torch.int32 or tuple(tables.shape) != (3, 256):
        raise ValueError("gt_prepare: tables must be int32 [3,256], got %s %s" % (tuple(tables.shape), tables.dtype))
    H, W = int(ids.shape[0]), int(ids.shape[1])
    if label_ids is not None and (label_ids.dtype != torch.uint8 or tuple(label_ids.shape) != (H, W)):
        raise ValueError("gt_prepare: label_ids must be uint8 [%d,%d], got %s %s" % (H, W, tuple(label_ids.shape), label_ids.dtype))
    if H > 32768 or W > 32768 or H * W >= 1 << 30:
        raise ValueError("gt_prepare: image of %d x %d pixels" % (H, W))
    seg_capacity = int(seg_capacity)
    trans_capacity = gt_prepare_default_transitions(H, W) if trans_capacity is None else int(trans_capacity)
    if not 1 <= seg_capacity <= 65536 or not 0 <= trans_capacity < 1 << 31:
        raise ValueError("gt_prepare: capacities %d segments / %d transitions" % (seg_capacity, trans_capacity))
    ids, tables, label_ids = dense(ids), dense(tables), dense(label_ids)
    dev = ids.device
    if workspace is None:
        workspace = gt_prepare_workspace(dev, seg_capacity)
    elif written(workspace, None, "gt_prepare: workspace").numel() * workspace.element_size() < int(lib().upsnet_gt_prepare_workspace_bytes(seg_capacity)):
        raise ValueError("gt_prepare: workspace too small for %d segments" % seg_capacity)
    train_map = torch.empty((H, W), dtype=torch.uint8, device=dev)
    rgb = torch.empty((H, W, 3), dtype=torch.uint8, device=dev)
    table = torch.empty((seg_capacity, GT_ROW), dtype=torch.int32, device=dev)
    trans_off = torch.empty((seg_capacity + 1,), dtype=torch.int32, device=dev)
    trans = torch.empty((max(trans_capacity, 1),), dtype=torch.int32, device=dev)
    status = torch.empty((GT_STATUS,), dtype=torch.int32, device=dev)
    check(lib().upsnet_gt_prepare(stream(), ptr(ids), ptr(label_ids), H, W, ptr(tables[0]), ptr(tables[1]), ptr(tables[2]), seg_capacity,
                                  trans_capacity, ptr(workspace), ptr(train_map), ptr(rgb), ptr(table), ptr(trans_off), ptr(trans),
                                  ptr(status)), "gt_prepare")
    return train_map, rgb, table, trans_off, trans, status


def gt_prepare_check(status, seg_capacity, trans_capacity, name='image'):
    """ValueError for what the status words (host ints) of one gt_prepare call report."""
    n_seg, n_inst, n_trans, flags, mismatch = (int(v) for v in status[:5])
    if flags & GT_FLAG_RANGE:
        raise ValueError("%s: the instance-id map holds values that encode no label (outside 0..255 and 1000..65535)" % name)
    if flags & GT_FLAG_SEGMENTS:
        raise ValueError("%s: %d segments, the capacity is %d" % (name, n_seg, seg_capacity))
    if mismatch:
        raise ValueError("%s: %d pixels of the labelIds map differ from the label of the instanceIds map" % (name, mismatch))
    if flags & GT_FLAG_TRANSITIONS:
        raise ValueError("%s: %d mask transitions, the capacity is %d" % (name, n_trans, trans_capacity))
    return n_seg, n_inst, n_trans


def gt_prepare_regrow(out, host, ids, tables, seg_capacity, workspace):
    """The one retry of the default transition capacity, shared by gt_prepare and CityscapesPreparer.finish. `out` is what
    gt_prepare_launch returned for `ids` with trans_capacity None, `host` its status words on the host. When they report nothing but
    an outgrown transition buffer, the image is run once more at the size its counting pass reported, all six launches (the workspace
    may have served another image since); the maps of the first run are complete and are kept. Returns (out, host) to go on with."""
    if int(host[3]) != GT_FLAG_TRANSITIONS or int(host[4]):
        return out, host
    again = gt_prepare_launch(ids, tables, None, seg_capacity, int(host[2]), workspace)
    return out[:2] + again[2:], again[5].cpu().numpy()


def gt_prepare(ids, tables, label_ids=None, seg_capacity=GT_PREPARE_SEGMENTS, trans_capacity=None, workspace=None):
    """gt_prepare_launch, synchronised: (train_map, rgb, table int32 [segments,9], trans_off int32 [instances+1], trans int32
    [transitions]) as device tensors cut to their counts. trans_capacity None: a default size, and a map that outgrows it is run once
    more at the size its counting pass reported. ValueError: more segments than seg_capacity or more transitions than a given
    trans_capacity (the message carries the true count; the workspace stays usable), a value that encodes no label (outside 0..255 and
    1000..65535), a labelIds map that disagrees."""
    require_cuda(ids)
    if workspace is None:
        workspace = gt_prepare_workspace(ids.device, seg_capacity)
    out = gt_prepare_launch(ids, tables, label_ids, seg_capacity, trans_capacity, workspace)
    host = out[5].cpu().numpy()
    if trans_capacity is None:
        out, host = gt_prepare_regrow(out, host, ids, tables, seg_capacity, workspace)
    train_map, rgb, table, trans_off, trans, _ = out
    n_seg, n_inst, n_trans = gt_prepare_check(host, table.shape[0], trans.shape[0] if trans_capacity != 0 else 0)
    return train_map, rgb, table[:n_seg], trans_off[:n_inst + 1], trans[:n_trans]


def panoptic_semantic(rgb, segments_info):
    """COCO panoptic PNG (uint8 [H,W,3] device tensor, id = R + 256 G + 65536 B) -> semantic map uint8 [H,W]: each pixel the
    category_id of its segment in segments_info (crowd segments included), 255 for id 0 and for ids without a segment: panopticapi's
    panoptic-to-semantic conversion. Channel 0 of csrc/pan_format.hip's relabel kernel. ValueError: ids outside 1..2^24-1 or used
    twice, categories outside 0..254."""
    from .pan_format import relabel
    n = len(segments_info)
    segs = np.array([(el['id'], el['category_id']) for el in segments_info], np.int64).reshape(n, 2)
    if np.any((segs[:, 0] < 1) | (segs[:, 0] >= 1 << 24)) or len(set(segs[:, 0].tolist())) != n:
        raise ValueError("panoptic_semantic: segment ids must be unique and lie in 1..2^24-1")
    if np.any((segs[:, 1] < 0) | (segs[:, 1] > 254)):
        raise ValueError("panoptic_semantic: category ids must lie in 0..254")
    segs = segs[np.argsort(segs[:, 0], kind='stable')]
    table = np.concatenate([segs, np.zeros((n, 1), np.int64)], 1).astype(np.int32)
    status = torch.empty((2,), dtype=torch.int64, device=rgb.device)
    check(lib().upsnet_zero_fill(stream(), ptr(status), 16), "zero_fill")
    out, _ = relabel(rgb, table, 0, status)
    return out[:, :, 0].contiguous()
