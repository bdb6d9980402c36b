"""Shared cases of the detection-visualisation tests (plain helper module, no fixtures): the hand-derived pictures with their expected
pixels written out, and seeded random scenes."""
import numpy as np

import vis_ref

H0, W0 = 16, 24
CANVAS = (40, 80, 120)
FAR = (-1000.0, -1000.0, -900.0, -900.0)      # a box (and with it a label) nowhere near the image
ORANGE, BLUE = (200, 100, 0), (0, 0, 250)

# blend(canvas, colour, 1/2), then blend(that, white, 1/2), by hand:
#   orange fill  ((40 + 200 + 1) // 2, (80 + 100 + 1) // 2, (120 + 0 + 1) // 2) = (120, 90, 60); contour ((120 + 256) // 2, ...) = (188, 173, 158)
#   blue fill    (20, 40, 185); contour (138, 148, 220)
#   ring         blend(canvas, (0, 128, 0), 1/2) = (20, 104, 60)
#   label ground blend(canvas, (0, 128, 0), 2/5) = ((120 + 2) // 5, (240 + 256 + 2) // 5, (360 + 2) // 5) = (24, 99, 72)
BASE_KEY = {'.': CANVAS, 'A': (120, 90, 60), 'a': (188, 173, 158), 'B': (20, 40, 185), 'b': (138, 148, 220), 'g': (20, 104, 60),
            'l': (24, 99, 72), 'W': (255, 255, 255)}


def rect_mask(x0, y0, x1, y1, holes=()):
    m = np.zeros((H0, W0), bool)
    m[y0:y1 + 1, x0:x1 + 1] = True
    for x, y in holes:
        m[y, x] = False
    return m


def picture(rows, key):
    """The expected picture of a character map (one string per row, one character per pixel)."""
    assert len(rows) == H0 and all(len(r) == W0 for r in rows), [len(r) for r in rows]
    return np.array([[key[ch] for ch in r] for r in rows], np.uint8)


def hand_cases():
    """[(name, boxes, labels, colours, dense masks, expected uint8 [16, 24, 3])] over a canvas of one colour."""
    cases = []
    # a 4 x 4 mask (x 5..8, y 3..6) with a one-pixel hole at (6, 5): only (7, 4) has its four neighbours in the mask
    cases.append(('hole', [FAR], [''], [ORANGE], [rect_mask(5, 3, 8, 6, holes=[(6, 5)])], picture([
        '........................',
        '........................',
        '........................',
        '.....aaaa...............',
        '.....aaAa...............',
        '.....a.aa...............',
        '.....aaaa...............',
        '........................',
        '........................',
        '........................',
        '........................',
        '........................',
        '........................',
        '........................',
        '........................',
        '........................'], BASE_KEY)))
    # a 4 x 4 mask in the top-left corner: the pixels on the image edges are contour, as those on the mask's open sides
    cases.append(('edges', [FAR], [''], [ORANGE], [rect_mask(0, 0, 3, 3)], picture([
        'aaaa....................',
        'aAAa....................',
        'aAAa....................',
        'aaaa....................'] + ['.' * W0] * 12, BASE_KEY)))
    # a box ring partly outside: corners floor(-3.5, 2.2, 4.9, 6.0) = (-4, 2, 4, 6): outer [-5, 5] x [1, 7] without [-2, 2] x [4, 4]
    cases.append(('ring', [(-3.5, 2.2, 4.9, 6.0)], [''], [ORANGE], [np.zeros((H0, W0), bool)], picture([
        '........................',
        'gggggg..................',
        'gggggg..................',
        'gggggg..................',
        '...ggg..................',
        'gggggg..................',
        'gggggg..................',
        'gggggg..................'] + ['.' * W0] * 8, BASE_KEY)))
    # two overlapping masks, orange x 2..5 y 2..5 and blue x 4..7 y 4..7; the four shared pixels p (4,4), q (5,4) and (4,5), r (5,5):
    #   orange first: p = orange fill, then blue fill + contour: (120, 90, 60) -> (60, 45, 155) -> (158, 150, 205)
    #                 q = orange contour, then blue fill + contour: (188, 173, 158) -> (94, 87, 204) -> (175, 171, 230)
    #                 r = orange contour, then blue fill: (94, 87, 204)
    #   blue first:   p = blue contour, then orange fill: (138, 148, 220) -> (169, 124, 110)
    #                 q = blue contour, then orange fill + contour: (169, 124, 110) -> (212, 190, 183)
    #                 r = blue fill, then orange fill + contour: (20, 40, 185) -> (110, 70, 93) -> (183, 163, 174)
    rows = ['........................',
            '........................',
            '..aaaa..................',
            '..aAAa..................',
            '..aApqbb................',
            '..aaqrBb................',
            '....bBBb................',
            '....bbbb................'] + ['.' * W0] * 8
    orange, blue = rect_mask(2, 2, 5, 5), rect_mask(4, 4, 7, 7)
    cases.append(('orange_then_blue', [FAR, FAR], ['', ''], [ORANGE, BLUE], [orange, blue],
                  picture(rows, dict(BASE_KEY, p=(158, 150, 205), q=(175, 171, 230), r=(94, 87, 204)))))
    cases.append(('blue_then_orange', [FAR, FAR], ['', ''], [BLUE, ORANGE], [blue, orange],
                  picture(rows, dict(BASE_KEY, p=(169, 124, 110), q=(212, 190, 183), r=(183, 163, 174)))))
    # a label clipped by the top edge: box (3, 9, 20, 13), text box columns 3..14, rows -8..7; of the '7' (rows 1F 01 02 04 08 08 08) the
    # cell rows 4..6 (one dot in cell column 1 -> columns 5..6, rows 0..5) and the empty row 7 are inside. Ring: outer [2, 21] x [8, 14]
    # without [5, 18] x [11, 11].
    cases.append(('label', [(3.0, 9.0, 20.0, 13.0)], ['7'], [ORANGE], [np.zeros((H0, W0), bool)], picture([
        '...llWWllllllll.........',
        '...llWWllllllll.........',
        '...llWWllllllll.........',
        '...llWWllllllll.........',
        '...llWWllllllll.........',
        '...llWWllllllll.........',
        '...llllllllllll.........',
        '...llllllllllll.........',
        '..gggggggggggggggggggg..',
        '..gggggggggggggggggggg..',
        '..gggggggggggggggggggg..',
        '..ggg..............ggg..',
        '..gggggggggggggggggggg..',
        '..gggggggggggggggggggg..',
        '..gggggggggggggggggggg..',
        '........................'], BASE_KEY)))
    return cases


def hand_image():
    return np.tile(np.array(CANVAS, np.uint8), (H0, W0, 1))


# the glyphs of 'car.87', one string per cell row (5 dots; the sixth column and the eighth row of a cell are empty)
CAR87 = {
    'c': ['.....', '.....', '.###.', '#....', '#....', '#...#', '.###.'],
    'a': ['.....', '.....', '.###.', '....#', '.####', '#...#', '.####'],
    'r': ['.....', '.....', '#.##.', '##..#', '#....', '#....', '#....'],
    '.': ['.....', '.....', '.....', '.....', '.....', '.##..', '.##..'],
    '8': ['.###.', '#...#', '#...#', '.###.', '#...#', '#...#', '.###.'],
    '7': ['#####', '....#', '...#.', '..#..', '.#...', '.#...', '.#...'],
}

NAMES = ('person', 'rider', 'car', 'truck', 'bus', 'train', 'motorcycle', 'bicycle', 'traffic light', 'hair drier')


def random_scene(seed, H, W, n, gen_dets, empty_masks=True, full_masks=True):
    """(image, boxes float32 [n, 4], labels, colours uint8 [n, 3], dense masks) of a seeded scene: a random image, gen_dets boxes of
    which some are moved onto and beyond every image edge, masks of random blobs (a few of zero pixels, a few covering the image),
    labels as the product forms them plus a few with bytes outside printable ASCII."""
    rng = np.random.default_rng(seed)
    image = rng.integers(0, 256, (H, W, 3)).astype(np.uint8)
    dets = gen_dets(rng, n, H, W) if n else np.zeros((0, 5), np.float32)
    boxes = dets[:, :4].copy()
    labels, masks = [], []
    yy, xx = np.mgrid[0:H, 0:W]
    for d in range(n):
        move = d % 6
        bw, bh = boxes[d, 2] - boxes[d, 0], boxes[d, 3] - boxes[d, 1]
        if move == 1:
            boxes[d, [0, 2]] -= boxes[d, 0] + rng.uniform(0, bw + 3)         # over the left edge
        elif move == 2:
            boxes[d, [1, 3]] -= boxes[d, 1] + rng.uniform(0, bh + 3)         # over the top edge
        elif move == 3:
            boxes[d, [0, 2]] += W - boxes[d, 2] + rng.uniform(-2, bw + 3)    # over the right edge
        elif move == 4:
            boxes[d, [1, 3]] += H - boxes[d, 3] + rng.uniform(-2, bh + 3)    # over the bottom edge
        kind = int(rng.integers(0, 12))
        if kind == 0 and empty_masks:
            m = np.zeros((H, W), bool)
        elif kind == 1 and full_masks:
            m = np.ones((H, W), bool)
        else:
            m = np.zeros((H, W), bool)
            for _ in range(int(rng.integers(1, 4))):
                cx, cy = rng.uniform(-5, W + 5), rng.uniform(-5, H + 5)
                rx, ry = rng.uniform(1, max(2.0, W / 5.0)), rng.uniform(1, max(2.0, H / 5.0))
                m |= ((xx - cx) / rx) ** 2 + ((yy - cy) / ry) ** 2 <= 1.0
            if kind == 2:                                                    # ragged: holes and specks
                m ^= rng.random((H, W)) < 0.05
        masks.append(m)
        label = NAMES[int(rng.integers(0, len(NAMES)))] + ('%.2f' % float(dets[d, 4])).lstrip('0')
        if d % 7 == 3:
            label = label.encode('ascii') + bytes([200, 10, 127])
        labels.append(label)
    colours = rng.integers(0, 256, (n, 3)).astype(np.uint8)
    return image, boxes.astype(np.float32), labels, colours, masks


def scene_transitions(masks, H, W):
    """The dense masks through the existing RLE path: pycocotools-style compressed strings (dataset/rle.py), then the product's decoder
    (vis.rle_transitions) -> (trans, trans_off)."""
    from upsnet_amd.dataset import vis
    from upsnet_amd.dataset.rle import counts_from_transitions, rle_to_string
    rles = [{'size': [H, W], 'counts': rle_to_string(counts_from_transitions(vis_ref.mask_transitions(m), H * W))} for m in masks]
    return vis.rle_transitions(rles, H, W)
