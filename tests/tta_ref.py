"""The merge rule of test-time augmentation restated in numpy float32, written from the rule and not from the kernels
(csrc/tta.hip): what tests/test_tta_cpu.py checks against float64 and by hand, and what tests/test_tta_gpu.py holds the device to bit
for bit. Every operation is one float32 numpy operation in the order the rule writes it (numpy never contracts a product and a sum).

An augmentation is described by q = s_a / s_0, r = s_0 / s_a (one float32 division each), its resized width Wr and its flip flag."""
import numpy as np

F = np.float32


def ratios(scales):
    """(q, r) lists of float32 for the im_scale values `scales` (element 0 is the base)."""
    s = [F(v) for v in scales]
    return [v / s[0] for v in s], [s[0] / v for v in s]


def seg_sample(m, Hb, Wb, q, wr, flip, cell, dtype=np.float32):
    """m: [Hs, Ws, S] (channels last). The bilinear sample of m at every cell of the Hb x Wb base grid, [Hb, Wb, S]."""
    T = dtype
    m = m.astype(T)
    Hs, Ws = m.shape[:2]
    q, wr = T(q), T(wr)
    ty = (np.arange(Hb).astype(T) + T(0.5)) * q
    tx = (np.arange(Wb).astype(T) + T(0.5)) * q
    v = ty - T(0.5)
    u = (wr * T(1.0 / cell) - tx) - T(0.5) if flip else tx - T(0.5)
    v = np.minimum(np.maximum(v, T(0)), T(Hs - 1))
    u = np.minimum(np.maximum(u, T(0)), T(Ws - 1))
    y0f, x0f = np.floor(v), np.floor(u)
    fy, fx = (v - y0f)[:, None, None], (u - x0f)[None, :, None]
    y0, x0 = y0f.astype(np.int64), x0f.astype(np.int64)
    y1, x1 = np.minimum(y0 + 1, Hs - 1), np.minimum(x0 + 1, Ws - 1)
    m00, m01 = m[y0][:, x0], m[y0][:, x1]
    m10, m11 = m[y1][:, x0], m[y1][:, x1]
    one = T(1)
    return (one - fy) * ((one - fx) * m00 + fx * m01) + fy * ((one - fx) * m10 + fx * m11)


def seg_merge(maps, q, wr, flip, cell, dtype=np.float32):
    """maps[a]: [Hs_a, Ws_a, S]; the output has the grid of maps[0]: (((sample_0 + sample_1) + ...) + sample_{A-1}) / A."""
    Hb, Wb = maps[0].shape[:2]
    acc = None
    for a, m in enumerate(maps):
        s = seg_sample(m, Hb, Wb, q[a], wr[a], flip[a], cell, dtype)
        acc = s if acc is None else acc + s
    return acc / dtype(len(maps))


def roi_to_base(rois, r, wr, flip):
    """rois [n,5] of an augmentation's frame -> the base frame (column 0 becomes 0)."""
    rois = rois.astype(F)
    r, wr = F(r), F(wr)
    x1, y1, x2, y2 = rois[:, 1], rois[:, 2], rois[:, 3], rois[:, 4]
    if flip:
        x1, x2 = (wr - F(1)) - x2, (wr - F(1)) - x1
    out = np.zeros_like(rois)
    out[:, 1], out[:, 2] = r * x1, r * y1
    out[:, 3], out[:, 4] = r * x2 + (r - F(1)), r * y2 + (r - F(1))
    return out


def roi_union(rois, delta, prob, counts, r, wr, flip):
    """Per augmentation rois[a] [R,5], delta[a] [R,D], prob[a] [R,C] and the count of valid rows. Returns (rois [A*R,5], delta, prob, n)."""
    A, R = len(rois), rois[0].shape[0]
    D, C = delta[0].shape[1], prob[0].shape[1]
    o_r, o_d, o_p = np.zeros((A * R, 5), F), np.zeros((A * R, D), F), np.zeros((A * R, C), F)
    off = 0
    for a in range(A):
        n = int(counts[a])
        o_r[off:off + n] = roi_to_base(rois[a][:n], r[a], wr[a], flip[a])
        d = delta[a][:n].astype(F).copy()
        if flip[a]:
            d[:, 0::4] = -d[:, 0::4]
        o_d[off:off + n] = d
        o_p[off:off + n] = prob[a][:n]
        off += n
    return o_r, o_d, o_p, off


def boxes_to_aug(boxes, q, wr, flip):
    """boxes [n,5] of the base frame -> [A,n,5]: the inverse rule, q_a in place of r_a, then the flip; column 0 is copied."""
    boxes = boxes.astype(F)
    out = np.zeros((len(q),) + boxes.shape, F)
    for a in range(len(q)):
        qa, w = F(q[a]), F(wr[a])
        x1, y1 = qa * boxes[:, 1], qa * boxes[:, 2]
        x2, y2 = qa * boxes[:, 3] + (qa - F(1)), qa * boxes[:, 4] + (qa - F(1))
        if flip[a]:
            x1, x2 = (w - F(1)) - x2, (w - F(1)) - x1
        out[a, :, 0] = boxes[:, 0]
        out[a, :, 1], out[a, :, 2], out[a, :, 3], out[a, :, 4] = x1, y1, x2, y2
    return out


def mask_merge(logits, flip):
    """logits[a]: [n,C,ms,ms]; a flipped augmentation is read at column ms - 1 - x."""
    acc = None
    for a, L in enumerate(logits):
        L = L.astype(F)
        if flip[a]:
            L = L[:, :, :, ::-1]
        acc = L if acc is None else acc + L
    return acc / F(len(logits))
