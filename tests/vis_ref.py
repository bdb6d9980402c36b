"""The drawing rule of the detection visualisations restated in numpy, written for clarity: masks are dense
arrays, and every layer of every detection is one pass over the whole image. Plain helper module: no fixtures, nothing of the product
but the font table it is handed.

    blend(dst, src, a / b) = (dst * (b - a) + src * a + b // 2) // b      per channel, integers

Layers: per detection in order the box ring (green at 1/2), the mask (its colour at 1/2) and the mask's boundary pixels (white at 1/2 on
top); then per detection in order the label (green at 2/5 over the text box, glyph dots white and opaque)."""
import numpy as np

GREEN = (0, 128, 0)
WHITE = (255, 255, 255)
COORD_LIMIT = 65536
CELL_W, CELL_H, SCALE = 6, 8, 2


def blend(dst, src, a, b):
    return (dst * (b - a) + src * a + b // 2) // b


def box_corners(box):
    """floor of the float32 coordinates, beyond +-65536 taken as +-65536 and a NaN as -65536, each pair in ascending order."""
    v = []
    for c in np.asarray(box, np.float32):
        f = np.floor(c)
        f = -COORD_LIMIT if not f >= -COORD_LIMIT else min(float(f), COORD_LIMIT)
        v.append(int(f))
    return min(v[0], v[2]), min(v[1], v[3]), max(v[0], v[2]), max(v[1], v[3])


def on_border(x, y, corners):
    """The one-pixel rectangle border through the corners, on the unbounded grid."""
    bx0, by0, bx1, by1 = corners
    inside = (x >= bx0) & (x <= bx1) & (y >= by0) & (y <= by1)
    return inside & ((x == bx0) | (x == bx1) | (y == by0) | (y == by1))


def ring_pixels(H, W, corners):
    """Pixels of the image whose Chebyshev distance to the border is <= 1: a border pixel among the pixel and its 8 neighbours."""
    y, x = np.mgrid[0:H, 0:W]
    ring = np.zeros((H, W), bool)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            ring |= on_border(x + dx, y + dy, corners)
    return ring


def contour_pixels(mask):
    """Mask pixels with at least one of the four neighbours outside the mask (outside the image = outside the mask)."""
    p = np.pad(mask, 1)
    all_four = p[:-2, 1:-1] & p[2:, 1:-1] & p[1:-1, :-2] & p[1:-1, 2:]
    return mask & ~all_four


def text_pixels(H, W, corners, label, font):
    """(text box, glyph dots) as boolean images: box columns bx0 .. bx0 + 12 L - 1, rows by0 - 17 .. by0 - 2, clipped to the image."""
    bx0, by0 = corners[0], corners[1]
    label = label if isinstance(label, bytes) else label.encode('utf-8')
    L = len(label)
    box, dots = np.zeros((H, W), bool), np.zeros((H, W), bool)
    if L == 0:
        return box, dots
    cells = np.zeros((CELL_H, CELL_W * L), bool)
    for i, ch in enumerate(label):
        if ch < 32 or ch > 126:
            ch = ord('?')
        for row in range(CELL_H):
            for col in range(5):
                cells[row, CELL_W * i + col] = bool(int(font[ch - 32][row]) >> (4 - col) & 1)
    big = np.repeat(np.repeat(cells, SCALE, 0), SCALE, 1)          # [16, 12 L]
    top, left = by0 - 2 - (CELL_H * SCALE - 1), bx0
    for v in range(big.shape[0]):
        for u in range(big.shape[1]):
            y, x = top + v, left + u
            if 0 <= y < H and 0 <= x < W:
                box[y, x] = True
                dots[y, x] = big[v, u]
    return box, dots


def paint(canvas, where, colour, a, b):
    for c in range(3):
        ch = canvas[:, :, c]
        ch[where] = blend(ch[where], colour[c], a, b)


def render(image, boxes, labels, colours, masks, font):
    """image uint8 [H, W, 3]; per detection in drawing order a box (x1 y1 x2 y2), a label (str / bytes), a colour (r, g, b) and a dense
    boolean mask [H, W]. Returns the picture, uint8 [H, W, 3]."""
    canvas = np.asarray(image).astype(np.int64).copy()
    H, W = canvas.shape[:2]
    corners = [box_corners(b) for b in boxes]
    for d in range(len(corners)):
        paint(canvas, ring_pixels(H, W, corners[d]), GREEN, 1, 2)
        mask = np.asarray(masks[d], bool)
        paint(canvas, mask, tuple(int(v) for v in colours[d]), 1, 2)
        paint(canvas, contour_pixels(mask), WHITE, 1, 2)
    for d in range(len(corners)):
        box, dots = text_pixels(H, W, corners[d], labels[d], font)
        paint(canvas, box, GREEN, 2, 5)
        for c in range(3):
            canvas[:, :, c][dots] = 255
    return canvas.astype(np.uint8)


def dense_masks(trans, trans_off, H, W):
    """Ascending column-major change positions (x * H + y) -> list of dense boolean masks [H, W]."""
    out = []
    for d in range(len(trans_off) - 1):
        flips = np.zeros(H * W + 1, np.int64)
        np.add.at(flips, np.asarray(trans[trans_off[d]:trans_off[d + 1]], np.int64), 1)
        out.append((np.cumsum(flips)[:H * W] % 2 == 1).reshape(W, H).T.copy())
    return out


def mask_transitions(mask):
    """Dense boolean mask [H, W] -> its ascending column-major change positions (the last one, H * W, dropped), int32."""
    flat = np.asarray(mask, bool).T.reshape(-1).astype(np.int8)
    return (np.flatnonzero(np.diff(np.concatenate([[0], flat]))) ).astype(np.int32)
