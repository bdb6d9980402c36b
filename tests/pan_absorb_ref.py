"""The absorbing rule of include/upsnet_hip.h (upsnet_pan_absorb), restated twice on top of tests/pan_components_ref.py, and the cases
the CPU and GPU tests add to that module's table.

The rule, from the header and not from the kernels:
  - keys, VOID, components, labels, areas, main components and which components are removed: upsnet_pan_components' rule on the same
    arguments (pan_components_ref). A removed component is a FRAGMENT, every other component is KEPT;
  - for every pixel p of a fragment r and each of the four EDGE neighbours q of p inside the image, whatever the connectivity: if q is
    not VOID and lies in a kept component, the key of q gets one vote from r (one vote per pixel edge); VOID pixels, pixels outside the
    image and pixels of other fragments give none;
  - the donor of r is the key with the most votes, ties to the smaller key; no votes, no donor;
  - a fragment pixel with a donor becomes (donor category, donor instance, byte 2), one without (255, 0, byte 2); every other pixel keeps
    its bytes. One round, nothing is iterated;
  - labels are those of the input map; stats = [distinct keys, components, fragments, fragment pixels, fragments absorbed, pixels
    absorbed, distinct (fragment, donor key) pairs that received a vote, 0].

absorb_loop: a loop over the fragment pixels and their neighbours, votes in a dict, on pan_components_ref.clean_flood.
absorb_vec: the four directed edge arrays between the label maps, np.unique over root << 16 | key with counts, the winner by lexsort,
on pan_components_ref.clean_scipy for the maps too large for absorb_loop and on clean_flood for the others (clean_scipy labels once
per key, and some cases here have thousands of keys); tests/test_pan_components_cpu.py holds those two together.
Both return (out uint8 [H,W,3], labels int32 [H,W], stats int32 [8]).
"""
import numpy as np

import pan_components_ref as ref

VOID = ref.VOID
TH, TW = ref.TH, ref.TW
LOOP_MAX_PIXELS = 100000          # absorb_loop is run on maps up to this size


def absorb_loop(pan, min_area=0, connectivity=8, keep_largest=True):
    void_out, labels, stats = ref.clean_flood(pan, min_area, connectivity, keep_largest)
    H, W = pan.shape[:2]
    key = ref.keys_of(pan)
    fragment = void_out[..., 0] != pan[..., 0]                       # a removed pixel was not VOID and is VOID now
    votes = {}
    for y, x in zip(*np.nonzero(fragment)):
        for qy, qx in ((y - 1, x), (y + 1, x), (y, x - 1), (y, x + 1)):
            if 0 <= qy < H and 0 <= qx < W and pan[qy, qx, 0] != VOID and not fragment[qy, qx]:
                pair = (int(labels[y, x]), int(key[qy, qx]))
                votes[pair] = votes.get(pair, 0) + 1
    donor = {}
    for (root, k), n in votes.items():
        if root not in donor or (n, -k) > (donor[root][0], -donor[root][1]):
            donor[root] = (n, k)
    out = void_out.copy()
    absorbed = 0
    for y, x in zip(*np.nonzero(fragment)):
        if int(labels[y, x]) in donor:
            k = donor[int(labels[y, x])][1]
            out[y, x, 0], out[y, x, 1] = k >> 8, k & 255
            absorbed += 1
    return out, labels, np.array(stats.tolist() + [len(donor), absorbed, len(votes), 0], np.int32)


def absorb_vec(pan, min_area=0, connectivity=8, keep_largest=True, base=None):
    """base: the (out, labels, stats) of the void rule on the same arguments, if the caller has them already."""
    if base is None:
        void_rule = ref.clean_scipy if pan.shape[0] * pan.shape[1] > LOOP_MAX_PIXELS else ref.clean_flood
        base = void_rule(pan, min_area, connectivity, keep_largest)
    void_out, labels, stats = base
    key = ref.keys_of(pan)
    fragment = void_out[..., 0] != pan[..., 0]
    kept = (pan[..., 0] != VOID) & ~fragment
    lab = labels.astype(np.int64)
    codes = []
    for p, q in ((np.s_[:, :-1], np.s_[:, 1:]), (np.s_[:, 1:], np.s_[:, :-1]),          # p votes for its right, left,
                 (np.s_[:-1, :], np.s_[1:, :]), (np.s_[1:, :], np.s_[:-1, :])):         # lower and upper neighbour q
        edge = fragment[p] & kept[q]
        codes.append(lab[p][edge] << 16 | key[q][edge])
    pairs, counts = np.unique(np.concatenate(codes), return_counts=True)
    roots, keys = pairs >> 16, pairs & 0xffff
    order = np.lexsort((keys, -counts, roots))                       # by root, then most votes, then the smaller key
    first = np.ones(len(order), bool)
    first[1:] = roots[order][1:] != roots[order][:-1]
    win_root, win_key = roots[order][first], keys[order][first]      # (ascending roots)
    out = void_out.copy()
    flat, fl, ff = out.reshape(-1, 3), lab.reshape(-1), fragment.reshape(-1)
    hit = np.zeros(len(fl), bool)
    if len(win_root):
        pos = np.searchsorted(win_root, fl[ff])
        pos[pos == len(win_root)] = 0
        has = win_root[pos] == fl[ff]
        idx = np.flatnonzero(ff)[has]
        flat[idx, 0] = win_key[pos[has]] >> 8
        flat[idx, 1] = win_key[pos[has]] & 255
        hit[idx] = True
    return out, labels, np.array(stats.tolist() + [len(win_root), int(hit.sum()), len(pairs), 0], np.int32)


# ---------------------------------------------------------------------------------------------------------------- literal maps
K, K7, K8, S, M, V = (11, 1), (11, 7), (11, 8), (3, 0), (5, 0), (VOID, 0)
I1, I2 = (13, 1), (13, 2)


def build(rows, byte2=0):
    """uint8 [H,W,3] from rows of (category, instance) pairs."""
    pan = np.zeros((len(rows), len(rows[0]), 3), np.uint8)
    for y, row in enumerate(rows):
        for x, (c, i) in enumerate(row):
            pan[y, x] = (c, i, byte2)
    return pan


def literals():
    """[(name, rows, min_area, keep_largest, expected rows, expected stats)]: every expectation is derived by hand from the rule and
    holds under both connectivities."""
    return [
        # a one-pixel speck of K7 in S; the body of K7 is elsewhere
        ('speck', [[S, S, S, S, S, S, S],
                   [S, K7, S, S, K7, K7, S],
                   [S, S, S, S, K7, K7, S],
                   [S, S, S, S, S, S, S]], 2, True,
         [[S, S, S, S, S, S, S],
          [S, S, S, S, K7, K7, S],
          [S, S, S, S, K7, K7, S],
          [S, S, S, S, S, S, S]], [2, 3, 1, 1, 1, 1, 1, 0]),
        # the two K pixels of row 1: three edges to M (up, left, down of the first), two to S (up, down of the second), one to VOID;
        # the key with more votes is the larger one
        ('three_to_two', [[M, M, S, S, S],
                          [M, K, K, V, S],
                          [M, M, S, S, S],
                          [K, K, K, V, V]], 3, True,
         [[M, M, S, S, S],
          [M, M, M, V, S],
          [M, M, S, S, S],
          [K, K, K, V, V]], [3, 4, 1, 2, 1, 2, 2, 0]),
        # one vote each: the smaller category wins (its one-pixel donors are kept as the main components of their keys)
        ('tie_by_category', [[M, K7, S, V, K7, K7]], 2, True, [[M, S, S, V, K7, K7]], [3, 4, 1, 1, 1, 1, 2, 0]),
        ('tie_by_instance', [[I2, K7, I1, V, K7, K7]], 2, True, [[I2, I1, I1, V, K7, K7]], [3, 4, 1, 1, 1, 1, 2, 0]),
        # the K7 pixel at (2, 2) touches S only across a corner: no vote, under 8-connectivity too
        ('diagonal_only', [[S, S, V, V, K7, K7],
                           [S, S, V, V, V, V],
                           [V, V, K7, V, V, V]], 2, True,
         [[S, S, V, V, K7, K7],
          [S, S, V, V, V, V],
          [V, V, V, V, V, V]], [2, 3, 1, 1, 0, 0, 0, 0]),
        ('void_and_border_only', [[K7, V, K7, K7]], 2, True, [[V, V, K7, K7]], [1, 2, 1, 1, 0, 0, 0, 0]),
        # two fragments side by side: the first borders S, the second only the first and VOID -- a single round
        ('adjacent_fragments', [[S, S, K7, K8, V, K7, K7, K8, K8]], 2, True, [[S, S, S, V, V, K7, K7, K8, K8]],
         [3, 5, 2, 2, 1, 1, 1, 0]),
        # M has one pixel, fewer than min_area, but is the main component of its key: kept, and a donor
        ('small_main_donor', [[M, K7, V, K7, K7]], 2, True, [[M, M, V, K7, K7]], [2, 3, 1, 1, 1, 1, 1, 0]),
        # without keep_largest a whole small segment goes to its surroundings
        ('whole_segment', [[S, S, S, S],
                           [S, K, S, S]], 2, False,
         [[S, S, S, S],
          [S, S, S, S]], [2, 2, 1, 1, 1, 1, 1, 0]),
    ]


# ---------------------------------------------------------------------------------------------------------------- the case table
def seam_cross():
    """A plus-shaped fragment over the point where four tiles meet, every quadrant another key; the body of its key elsewhere."""
    pan = ref._blank(2 * TH, 2 * TW, 3, 0)
    pan[:TH, TW:] = (5, 0, 0)
    pan[TH:, :TW] = (7, 0, 0)
    pan[TH:, TW:] = (13, 1, 0)
    pan[2:12, 2:12] = (11, 7, 0)                        # 100 pixels: the main component
    pan[TH - 1:TH + 1, TW - 14:TW + 6] = (11, 7, 0)
    pan[TH - 9:TH + 11, TW - 1:TW + 1] = (11, 7, 0)     # 76 pixels
    return pan


def corners():
    """One fragment in every corner of the image: one, two, three and four pixels."""
    pan = ref._blank(40, 150, 3, 0)
    pan[15:25, 60:70] = (11, 7, 0)
    pan[0, 0] = pan[0, 148:] = (11, 7, 0)
    pan[38:, 0] = pan[39, 1] = (11, 7, 0)
    pan[38:, 148:] = (11, 7, 0)
    return pan


def long_fragment():
    """A fragment one pixel high and 200 long (min_area 256): 70 kept keys of 3 columns each above it, one kept key below it and at its
    ends, which collects 202 votes from the 14 threads the fragment runs through."""
    pan = ref._blank(12, 210, 3, 0)
    for k in range(70):
        pan[:5, 3 * k:3 * k + 3] = (20 + k, 0, 0)
    pan[5, 5:205] = (11, 7, 0)
    pan[9:, :100] = (11, 7, 0)                          # 300 pixels: the main component
    return pan


def stripes(H=2 * TH, W=2 * TW):
    """As many (fragment, donor) pairs as a map allows: a checkerboard of one-pixel kept segments, each its own key (kept as main
    components), and one-pixel fragments whose key alternates with the row, so that they stay apart under 8-connectivity too: four
    pairs per inner fragment, close to the map's 2HW - H - W edges."""
    y, x = np.mgrid[:H, :W]
    n = (y * W + x) // 2
    pan = np.zeros((H, W, 3), np.uint8)
    pan[..., 0], pan[..., 1] = n // 256, n % 256
    odd = (y + x) % 2 == 1
    pan[..., 0][odd] = (200 + y % 2)[odd]
    pan[..., 1][odd] = 1
    return pan


def cases():
    """[(name, map, min_area, keep_largest)], beside pan_components_ref.cases(); every test runs each under both connectivities."""
    rng = np.random.default_rng(2701)
    out = [(name, build(rows, byte2=9), m, keep) for name, rows, m, keep, _, _ in literals()]
    one = ref._blank(1, 1, 3, 0)
    out += [
        ('absorb_1x1', one, 2, False),
        ('absorb_1x40', ref.blobs(rng, 1, 40, 5, ref.KEYS, 0.1), 3, True),
        ('absorb_40x1', ref.blobs(rng, 40, 1, 5, ref.KEYS, 0.1), 3, True),
        ('absorb_33x129', ref.blobs(rng, 33, 129, 9, ref.KEYS, 0.03), 4, True),
        ('absorb_70x300', ref.blobs(rng, 70, 300, 13, ref.KEYS, 0.03), 6, True),
        ('absorb_70x300_all', ref.blobs(rng, 70, 300, 6, ref.KEYS, 0.03), 40, False),
        ('seam_cross', seam_cross(), 90, True),
        ('corners', corners(), 5, True),
        ('long_fragment', long_fragment(), 256, True),
        ('stripes', stripes(), 2, True),
        ('many_instances_cells', ref.many_instances(rng), 17, True),
        ('noise_45x133', ref._random(rng, 45, 133, ref.KEYS), 3, True),
    ]
    return out
