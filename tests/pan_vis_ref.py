"""The panoptic drawing rule of DESIGN.md section 4.20 in numpy, on dense arrays: what csrc/pan_vis.hip is held to, byte for byte.

    pred_2ch uint8 [H, W, 3]: channel 0 category (255 = VOID), channel 1 instance; key = ch0 << 8 | ch1.
    edge(p), p not VOID: one of the four neighbours has another key or lies outside the image.
    blend(dst, src, a/b) = (dst * (b - a) + src * a + b // 2) // b.

flat:    category colour per pixel (VOID and categories missing from the table black); white where one of (y, x), (y, x-1), (y-1, x),
         (y-1, x-1) is an edge pixel of a segment with isthing and ch1 != 0.
overlay: image; non-VOID: blend(., segment colour, 1/2) with the per-segment colours of pan_format.ColorGenerator in ascending key;
         edge: blend(., white, 1/2); then the labels of the segments of area >= label_min_area in ascending key, at most 256.

Only integers; the centroid sums are int64. `font` is vis.font_table() (uint8 [95, 8], bit 4 = the leftmost of 5 dots).
"""
import numpy as np

MAX_LABELS = 256
CELL_W, CELL_H = 12, 16


def blend(dst, src, a, b):
    return (dst * (b - a) + src * a + b // 2) // b


def category_dict(categories):
    return categories if isinstance(categories, dict) else {el['id']: el for el in categories}


def keys_of(pred):
    return pred[..., 0].astype(np.int64) << 8 | pred[..., 1].astype(np.int64)


def edge_map(pred):
    """bool [H, W]: the edge pixels (never a VOID pixel)."""
    key = keys_of(pred)
    H, W = key.shape
    pad = np.full((H + 2, W + 2), -1, np.int64)
    pad[1:-1, 1:-1] = key
    differs = (pad[:-2, 1:-1] != key) | (pad[2:, 1:-1] != key) | (pad[1:-1, :-2] != key) | (pad[1:-1, 2:] != key)
    return differs & (pred[..., 0] != 255)


def label_bytes(cat_id, entry):
    name = entry.get('name')
    text = str(cat_id) if name is None else name
    return text if isinstance(text, bytes) else text.encode('utf-8')


def render_flat(pred, categories):
    """-> uint8 [H, W, 3]."""
    from upsnet_amd.dataset.pan_format import category_color
    cats = category_dict(categories)
    H, W = pred.shape[:2]
    colour = np.zeros((256, 3), np.uint8)
    thing = np.zeros(256, bool)
    for c, entry in cats.items():
        colour[int(c)] = category_color(c, entry)
        thing[int(c)] = entry['isthing'] != 0
    colour[255] = 0
    thing[255] = False
    out = colour[pred[..., 0]]
    contour = edge_map(pred) & thing[pred[..., 0]] & (pred[..., 1] != 0)
    wide = contour.copy()
    wide[:, 1:] |= contour[:, :-1]          # (y, x-1)
    wide[1:, :] |= contour[:-1, :]          # (y-1, x)
    wide[1:, 1:] |= contour[:-1, :-1]       # (y-1, x-1)
    out[wide] = 255
    return out


def segments(pred):
    """(keys ascending, areas, sum of x, sum of y) of the non-VOID segments, int64."""
    H, W = pred.shape[:2]
    key = keys_of(pred).reshape(-1)
    keep = np.nonzero(pred[..., 0].reshape(-1) != 255)[0]
    if keep.size == 0:
        z = np.zeros(0, np.int64)
        return z, z, z, z
    order = keep[np.argsort(key[keep], kind='stable')]
    sk = key[order]
    first = np.concatenate([[0], np.nonzero(sk[1:] != sk[:-1])[0] + 1])
    area = np.diff(np.concatenate([first, [sk.size]])).astype(np.int64)
    sx = np.add.reduceat((order % W).astype(np.int64), first)
    sy = np.add.reduceat((order // W).astype(np.int64), first)
    return sk[first], area, sx, sy


def label_boxes(pred, categories, label_min_area=1024):
    """([(key, left, top, text bytes)] of the labels drawn, in drawing order; number of segments that qualified)."""
    cats = category_dict(categories)
    H, W = pred.shape[:2]
    keys, area, sx, sy = segments(pred)
    boxes, qualified = [], 0
    for k, a, x, y in zip(keys.tolist(), area.tolist(), sx.tolist(), sy.tolist()):
        if a < label_min_area:
            continue
        qualified += 1
        if qualified > MAX_LABELS:
            continue
        text = label_bytes(k >> 8, cats[k >> 8])
        L = len(text)
        cx, cy = x // a, y // a
        left = max(min(cx - 6 * L, W - CELL_W * L), 0)
        top = max(min(cy - 8, H - CELL_H), 0)
        boxes.append((k, left, top, text))
    return boxes, qualified


def text_dots(text, font):
    """bool [16, 12 L]: the glyph dots of the text at scale 2."""
    dots = np.zeros((CELL_H, CELL_W * len(text)), bool)
    for i, ch in enumerate(bytearray(text)):
        if ch < 32 or ch > 126:
            ch = ord('?')
        cell = font[ch - 32]
        for row in range(8):
            for col in range(5):
                if cell[row] >> (4 - col) & 1:
                    dots[2 * row:2 * row + 2, CELL_W * i + 2 * col:CELL_W * i + 2 * col + 2] = True
    return dots


def render_overlay(pred, categories, image, font, label_min_area=1024):
    """-> (uint8 [H, W, 3], segments that qualified for a label, labels drawn)."""
    from upsnet_amd.dataset.pan_format import ColorGenerator
    H, W = pred.shape[:2]
    assert image.shape == (H, W, 3) and image.dtype == np.uint8
    key = keys_of(pred)
    nonvoid = pred[..., 0] != 255
    gen = ColorGenerator(categories)
    colour = np.zeros((65536, 3), np.int64)
    for k in np.unique(key[nonvoid]).tolist():          # ascending key
        colour[k] = gen.get_color(k >> 8)
    out = image.astype(np.int64)
    out[nonvoid] = blend(out[nonvoid], colour[key[nonvoid]], 1, 2)
    edge = edge_map(pred)
    out[edge] = blend(out[edge], 255, 1, 2)
    boxes, qualified = label_boxes(pred, categories, label_min_area)
    for _, left, top, text in boxes:
        if not text:
            continue
        dots = text_dots(text, font)
        h, w = min(CELL_H, H - top), min(dots.shape[1], W - left)       # clipped to the image
        box = out[top:top + h, left:left + w]
        box[...] = blend(box, 0, 2, 5)
        box[dots[:h, :w]] = 255
    return out.astype(np.uint8), qualified, len(boxes)
