"""Polygon inputs for the polygon rasteriser tests: hand-derived cases (checkable by eye from the rule "an integer rectangle
[x0, x1] x [y0, y1] covers columns x0 .. x1 - 1, rows y0 .. y1 - 1, clipped to the image") and seeded random populations."""
import numpy as np

H0, W0 = 6, 8


def rect_poly(x0, y0, x1, y1):
    return [x0, y0, x1, y0, x1, y1, x0, y1]


def rect_mask(x0, y0, x1, y1, h, w):
    m = np.zeros((h, w), np.uint8)
    m[max(y0, 0):max(min(y1, h), 0), max(x0, 0):max(min(x1, w), 0)] = 1
    return m


def rows_mask(rows, h, w):
    """{y: '01111110'} -> uint8 [h, w]."""
    m = np.zeros((h, w), np.uint8)
    for y, s in rows.items():
        m[y] = [int(c) for c in s]
    return m


TRIANGLE = [1, 1, 7, 1, 4, 5]
TRIANGLE_MASK = rows_mask({1: '01111110', 2: '00111100', 3: '00011000'}, H0, W0)
RECT = rect_poly(2, 1, 6, 4)
RECT_COUNTS = [13, 3, 3, 3, 3, 3, 3, 3, 14]

# integer rectangles touching and crossing each image border of the 6 x 8 grid: (x0, y0, x1, y1)
BORDER_RECTS = [(0, 0, 3, 2), (0, 2, 2, 6), (5, 0, 8, 3), (3, 4, 8, 6), (0, 0, 8, 6),           # touching
                (-2, 1, 3, 4), (2, -3, 5, 2), (6, 2, 11, 5), (1, 4, 4, 9), (-3, -2, 12, 9),      # crossing
                (-5, -5, -1, -1), (9, 1, 12, 4), (2, 7, 5, 9)]                                    # wholly outside


def rotations_and_reversal(poly):
    pts = [(poly[2 * j], poly[2 * j + 1]) for j in range(len(poly) // 2)]
    out = []
    for r in range(len(pts)):
        rot = pts[r:] + pts[:r]
        out.append([c for p in rot for c in p])
        out.append([c for p in rot[::-1] for c in p])
    return out


def repeat_vertex(poly, j):
    pts = [(poly[2 * i], poly[2 * i + 1]) for i in range(len(poly) // 2)]
    pts = pts[:j + 1] + pts[j:]
    return [c for p in pts for c in p]


# ------------------------------------------------------------------------------------------------------------------ random populations
def _closed_curve(rng, k, cx, cy, r, kind):
    ang = np.sort(rng.uniform(0, 2 * np.pi, k))
    if kind == 'convex':
        rad = np.full(k, r)
    elif kind == 'star':
        rad = r * rng.uniform(0.2, 1.0, k)
    else:   # self-intersecting: the angles are not sorted
        ang = rng.uniform(0, 2 * np.pi, k)
        rad = r * rng.uniform(0.2, 1.0, k)
    return np.stack([cx + rad * np.cos(ang), cy + rad * np.sin(ang)], 1)


def random_polygon(rng, h, w):
    """One flat polygon; the kinds of the test population in turn by chance."""
    kind = rng.choice(['convex', 'star', 'self', 'outside', 'negative', 'half', 'dup', 'collinear', 'tiny', 'many'])
    k = int(rng.randint(3, 13))
    scale = max(h, w)
    cx, cy, r = rng.uniform(0, w), rng.uniform(0, h), rng.uniform(0.5, 0.7 * scale + 1)
    if kind in ('convex', 'star', 'self'):
        pts = _closed_curve(rng, k, cx, cy, r, kind)
    elif kind == 'outside':   # wholly outside the image
        pts = _closed_curve(rng, k, w + 2 * r + rng.uniform(1, 20), cy, r, 'star') if rng.rand() < .5 else \
            _closed_curve(rng, k, cx, -2 * r - rng.uniform(1, 20), r, 'star')
    elif kind == 'negative':
        pts = _closed_curve(rng, k, rng.uniform(-w, 0.3 * w), rng.uniform(-h, 0.3 * h), r, 'star')
    elif kind == 'half':      # half-pixel grid: positions repeat and cancel
        pts = rng.randint(-4, 2 * scale + 6, (k, 2)) / 2.0
    elif kind == 'dup':       # consecutive duplicate vertices
        pts = np.repeat(_closed_curve(rng, k, cx, cy, r, 'star'), rng.randint(1, 4, k), axis=0)
    elif kind == 'collinear':
        t = rng.uniform(-1, 2, k)
        a, b = rng.uniform(0, scale, 2), rng.uniform(0, scale, 2)
        pts = a[None] + t[:, None] * (b - a)[None]
        if rng.rand() < .3:
            pts = np.round(pts)
    elif kind == 'tiny':      # 0, 1 or 2 vertices: the real files hold a few
        pts = rng.uniform(0, scale, (int(rng.randint(0, 3)), 2))
    else:                     # up to 400 vertices
        pts = _closed_curve(rng, int(rng.randint(100, 401)), cx, cy, r, 'star')
    if rng.rand() < .25:
        pts = np.round(pts)
    return [float(v) for v in np.asarray(pts, np.float64).reshape(-1)]


def random_object(rng, h, w):
    """1 to 6 polygons (now and then none): independent ones overlap or are disjoint by chance; some nest inside the first."""
    n = int(rng.choice([0, 1, 1, 1, 1, 2, 2, 3, 4, 5, 6]))
    polys = [random_polygon(rng, h, w) for _ in range(n)]
    if n >= 2 and rng.rand() < .4 and len(polys[0]) >= 6:   # nest: a shrunken copy of the first polygon about its centroid
        p = np.asarray(polys[0]).reshape(-1, 2)
        polys[1] = [float(v) for v in (p.mean(0) + 0.5 * (p - p.mean(0))).reshape(-1)]
    return polys


SIZES = [(1, 1), (1, 9), (7, 1), (2, 3), (6, 8), (13, 17), (31, 32), (64, 65), (97, 131)]


def population(seed, n_objects):
    """[(h, w, [object, ...])]: n_objects objects spread over SIZES."""
    rng = np.random.RandomState(seed)
    out = []
    per = -(-n_objects // len(SIZES))
    for h, w in SIZES:
        out.append((h, w, [random_object(rng, h, w) for _ in range(per)]))
    return out


def blob_contour(rng, k, cx, cy, r):
    """A noisy closed curve around a blob: k vertices (Cityscapes-like instance contours)."""
    ang = np.linspace(0, 2 * np.pi, k, endpoint=False)
    rad = r * (1 + 0.25 * np.sin(3 * ang + rng.uniform(0, 6)) + 0.1 * np.sin(7 * ang + rng.uniform(0, 6))) + rng.uniform(-1.5, 1.5, k)
    pts = np.stack([cx + rad * np.cos(ang), cy + rad * np.sin(ang)], 1)
    return [float(v) for v in np.round(pts * 2).reshape(-1) / 2]   # Cityscapes polygons are integer or half-pixel


def sawtooth_border(h, w, step=2, depth=3):
    """One polygon along the whole image border with a saw-tooth inner edge: every tooth emits positions, far more than an LDS run."""
    pts = []
    for x in range(0, w, step):                 # top edge, left to right
        pts += [(x, 0), (x + step / 2.0, depth)]
    for y in range(0, h, step):                 # right edge, downwards
        pts += [(w, y), (w - depth, y + step / 2.0)]
    for x in range(w, 0, -step):                # bottom edge, right to left
        pts += [(x, h), (x - step / 2.0, h - depth)]
    for y in range(h, 0, -step):                # left edge, upwards
        pts += [(0, y), (depth, y - step / 2.0)]
    return [float(c) for p in pts for c in p]
