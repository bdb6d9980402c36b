"""CPU restatement of pycocotools' polygon rasteriser (maskApi.c rleFrPoly, then merge = union), written for clarity and independent
of the product code. Everything in Python floats (IEEE double) and ints; int() truncates toward zero like the C cast.

  poly_points(poly)              steps 1-2: the upsampled walk of every edge, as (u, v) lists
  poly_positions(poly, h, w)     step 3: the positions emitted, in emission order (values up to h * w)
  fold_counts(positions, h, w)   the literal tail of rleFrPoly: append h * w, sort, difference, fold zero differences pairwise
  odd_counts(positions, h, w)    the rule the kernel uses: positions < h * w emitted an odd number of times
  polygon_counts / polygon_mask / object_mask / object_counts / object_transitions: one polygon, and the union of an object's polygons
"""
import numpy as np


def poly_points(poly):
    k = len(poly) // 2
    x = [int(5 * float(poly[2 * j]) + .5) for j in range(k)]
    y = [int(5 * float(poly[2 * j + 1]) + .5) for j in range(k)]
    if k == 0:
        return [], []
    x.append(x[0])
    y.append(y[0])
    u, v = [], []
    for j in range(k):
        xs, xe, ys, ye = x[j], x[j + 1], y[j], y[j + 1]
        dx, dy = abs(xe - xs), abs(ys - ye)
        flip = (dx >= dy and xs > xe) or (dx < dy and ys > ye)
        if flip:
            xs, xe = xe, xs
            ys, ye = ye, ys
        if dx >= dy:
            s = float(ye - ys) / dx if dx else 0.0   # 0 / 0 in the original; the point's y is never read
            for d in range(dx + 1):
                t = dx - d if flip else d
                u.append(t + xs)
                v.append(int(ys + s * t + .5))
        else:
            s = float(xe - xs) / dy
            for d in range(dy + 1):
                t = dy - d if flip else d
                v.append(t + ys)
                u.append(int(xs + s * t + .5))
    return u, v


def poly_positions(poly, h, w):
    u, v = poly_points(poly)
    out = []
    for j in range(1, len(u)):
        if u[j] == u[j - 1]:
            continue
        xd = float(u[j] if u[j] < u[j - 1] else u[j] - 1)
        xd = (xd + .5) / 5 - .5
        if np.floor(xd) != xd or xd < 0 or xd > w - 1:
            continue
        yd = float(v[j] if v[j] < v[j - 1] else v[j - 1])
        yd = (yd + .5) / 5 - .5
        if yd < 0:
            yd = 0.0
        elif yd > h:
            yd = float(h)
        yd = np.ceil(yd)
        out.append(int(xd) * h + int(yd))
    return out


def fold_counts(positions, h, w):
    a = sorted(list(positions) + [h * w])
    p = 0
    for j in range(len(a)):
        t = a[j]
        a[j] -= p
        p = t
    n = len(a)
    b = [a[0]]
    j = 1
    while j < n:
        if a[j] > 0:
            b.append(a[j])
            j += 1
        else:
            j += 1
            if j < n:
                b[-1] += a[j]
                j += 1
    return b


def odd_transitions(positions, h, w):
    vals, cnt = np.unique(np.asarray(list(positions), np.int64), return_counts=True)
    return [int(p) for p, c in zip(vals, cnt) if c % 2 == 1 and p < h * w]


def transitions_to_counts(trans, h, w):
    edges = [0] + list(trans) + [h * w]
    return [edges[i + 1] - edges[i] for i in range(len(edges) - 1)]


def odd_counts(positions, h, w):
    return transitions_to_counts(odd_transitions(positions, h, w), h, w)


def counts_to_mask(counts, h, w):
    """uint8 [h, w] of uncompressed RLE counts (column-major runs, zeros first)."""
    flat = np.zeros(h * w, np.uint8)
    p, val = 0, 0
    for c in counts:
        flat[p:p + c] = val
        p += c
        val ^= 1
    assert p == h * w, (p, h * w)
    return flat.reshape(w, h).T.copy()


def mask_to_transitions(mask):
    flat = np.asarray(mask, np.uint8).T.reshape(-1)
    prev = np.concatenate([[0], flat[:-1]])
    return [int(p) for p in np.nonzero(flat != prev)[0]]


def polygon_counts(poly, h, w):
    return fold_counts(poly_positions(poly, h, w), h, w)


def polygon_mask(poly, h, w):
    return counts_to_mask(polygon_counts(poly, h, w), h, w)


def object_mask(polygons, h, w):
    m = np.zeros((h, w), np.uint8)
    for p in polygons:
        m |= polygon_mask(p, h, w)
    return m


def object_transitions(polygons, h, w):
    return mask_to_transitions(object_mask(polygons, h, w))


def object_counts(polygons, h, w):
    return transitions_to_counts(object_transitions(polygons, h, w), h, w)


def object_rle(polygons, h, w):
    return {'size': [h, w], 'counts': object_counts(polygons, h, w)}
