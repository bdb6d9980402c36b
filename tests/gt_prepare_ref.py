"""numpy restatement of csrc/gt_prepare.hip and of the panoptic-to-semantic conversion: np.unique, one full mask per
value, np.flatnonzero(np.diff(...)) over the mask in column-major order with a leading zero. Slow and plain on purpose."""
import numpy as np

ROW = 9


def reference(ids, tables):
    """ids int [H, W] (raw instanceIds values: 0..255 are labels, 1000..65535 label * 1000 + instance number), tables int [3, 256]
    (train id / hasInstances / thing row per label) -> (train_map uint8 [H, W], rgb uint8 [H, W, 3], rows int32 [n, 9], trans_off
    int32 [m + 1], trans int32 [t]). ValueError for a value that encodes no label."""
    ids = np.asarray(ids).astype(np.int64)
    if np.any((ids < 0) | ((ids >= 256) & (ids < 1000)) | (ids > 65535)):
        raise ValueError('a value outside 0..255 and 1000..65535 encodes no label')
    tables = np.asarray(tables)
    H, W = ids.shape
    label = np.where(ids < 1000, ids, ids // 1000)
    train = tables[0][label]
    colour = np.where(train == 255, 0, ids)
    rgb = np.stack([colour % 256, colour // 256 % 256, colour // 65536], 2).astype(np.uint8)
    rows, lists = [], []
    for v in np.unique(ids).tolist():
        lab = v if v < 1000 else v // 1000
        if tables[0][lab] == 255:
            continue
        mask = ids == v
        ys, xs = np.flatnonzero(mask.any(1)), np.flatnonzero(mask.any(0))
        rows.append([v, lab, int(tables[0][lab]), int(v < 1000 and tables[1][lab] != 0), int(mask.sum()), int(xs.min()), int(ys.min()),
                     int(xs.max()), int(ys.max())])
        if v >= 1000 and tables[2][lab] >= 0:
            column_major = np.concatenate([[0], mask.ravel(order='F').astype(np.int8)])
            lists.append(np.flatnonzero(np.diff(column_major)))
    trans_off = np.concatenate([[0], np.cumsum([len(t) for t in lists])]).astype(np.int32)
    trans = (np.concatenate(lists) if lists else np.zeros(0)).astype(np.int32)
    return train.astype(np.uint8), rgb, np.array(rows, np.int32).reshape(-1, ROW), trans_off, trans


def semantic_reference(rgb, segments_info):
    """Panoptic PNG content uint8 [H, W, 3] -> uint8 [H, W]: the category_id of each pixel's segment, 255 for id 0 and unlisted ids."""
    ids = rgb[:, :, 0].astype(np.int64) + 256 * rgb[:, :, 1].astype(np.int64) + 65536 * rgb[:, :, 2].astype(np.int64)
    out = np.full(ids.shape, 255, np.uint8)
    for seg in segments_info:
        if seg['id'] != 0:
            out[ids == seg['id']] = seg['category_id']
    return out
