"""Plain numpy restatement of the video metrics of include/upsnet_hip.h (VPQ: Kim et al., CVPR 2020; STQ: Weber et al., NeurIPS 2021):
dicts and loops over the (GT row, pred key) pairs that np.unique finds per frame. The yardstick of tests/test_video_pq_*.py, and the
builders of their hand-derived cases. Nothing here is shared with the evaluator under test."""
import math

import numpy as np

VOID = 255


# ------------------------------------------------------------------------------------------------ the rule
def sequence_table(frames_segments_info):
    """The union of the frames' segments in ascending id: [(id, category, iscrowd)]."""
    rows = {}
    for segs in frames_segments_info:
        for s in segs:
            rows[int(s['id'])] = (int(s['id']), int(s['category_id']), int(s.get('iscrowd', 0)))
    return [rows[k] for k in sorted(rows)]


def frame_counts(pred, gt, table):
    """{(row or -1 for ignored, key or -1 for pred VOID): pixels} of one frame."""
    row_of_id = {r[0]: i for i, r in enumerate(table)}
    key = (pred[:, :, 0].astype(np.int64) << 8) | pred[:, :, 1].astype(np.int64)
    key[pred[:, :, 0] == VOID] = -1
    gid = gt[:, :, 0].astype(np.int64) + 256 * gt[:, :, 1].astype(np.int64) + 65536 * gt[:, :, 2].astype(np.int64)
    uniq, inverse = np.unique(gid, return_inverse=True)
    row_of = np.array([row_of_id.get(g, -1) if g != 0 else -1 for g in uniq.tolist()], np.int64)
    row = row_of[inverse.reshape(-1)]
    pairs, counts = np.unique((row.reshape(-1) + 1) * 70000 + (key.reshape(-1) + 1), return_counts=True)
    return {(int(p) // 70000 - 1, int(p) % 70000 - 1): int(c) for p, c in zip(pairs, counts)}


def add_counts(total, cells):
    for k, v in cells.items():
        total[k] = total.get(k, 0) + v


def tables(cells):
    """area_p[key], area_g[row], void[key], joint[(row, key)] (every category pair) from summed pair counts."""
    area_p, area_g, void, joint = {}, {}, {}, {}
    for (row, key), v in cells.items():
        if key >= 0:
            area_p[key] = area_p.get(key, 0) + v
            if row < 0:
                void[key] = void.get(key, 0) + v
        if row >= 0:
            area_g[row] = area_g.get(row, 0) + v
            if key >= 0:
                joint[(row, key)] = v
    return area_p, area_g, void, joint


class RefVideoEvaluator(object):
    def __init__(self, categories, windows=(1, 2, 3, 4)):
        self.categories = categories if isinstance(categories, dict) else {el['id']: el for el in categories}
        self.windows = tuple(windows)
        self.tp = {n: {} for n in self.windows}
        self.fp = {n: {} for n in self.windows}
        self.fn = {n: {} for n in self.windows}
        self.iou = {n: {} for n in self.windows}        # float64 sums in the stated order
        self.conf = np.zeros((256, 256), np.int64)
        self.aq_sums = []                               # one float64 per sequence
        self.num_tracks = 0
        self.sequences = 0
        self.frames = 0
        self.seq_cells = []                             # per sequence: the summed pair counts (for the count comparisons)

    def _window(self, n, cells, table):
        area_p, area_g, void, joint = tables(cells)
        tp, fp, fn, iou = self.tp[n], self.fp[n], self.fn[n], self.iou[n]
        matched_rows, matched_keys = set(), set()
        keys_of = {}                                            # row -> its keys with inter > 0 (of any category)
        for (row, key) in joint:
            keys_of.setdefault(row, []).append(key)
        crowd_rows = [(row, cat) for row, (_, cat, crowd) in enumerate(table) if crowd]
        for row, (_, cat, crowd) in enumerate(table):           # ascending id
            if crowd:
                continue
            for key in sorted(keys_of.get(row, [])):
                inter = joint[(row, key)]
                if key >> 8 != cat:
                    continue
                v = float(inter) / float(area_p[key] + area_g[row] - inter - void.get(key, 0))
                if v > 0.5:
                    tp[cat] = tp.get(cat, 0) + 1
                    iou[cat] = iou.get(cat, 0.0) + v
                    matched_rows.add(row)
                    matched_keys.add(key)
        for row, (_, cat, crowd) in enumerate(table):
            if not crowd and area_g.get(row, 0) > 0 and row not in matched_rows:
                fn[cat] = fn.get(cat, 0) + 1
        for key in sorted(area_p):
            if key in matched_keys or area_p[key] == 0:
                continue
            cat = key >> 8
            if cat not in self.categories:
                raise KeyError(cat)
            ign = void.get(key, 0)
            for row, rcat in crowd_rows:                        # ALL crowd rows of the category
                if rcat == cat:
                    ign += joint.get((row, key), 0)
            if float(ign) / float(area_p[key]) > 0.5:
                continue
            fp[cat] = fp.get(cat, 0) + 1

    def add_sequence(self, preds, gts, frames_segments_info):
        table = sequence_table(frames_segments_info)
        per_frame = [frame_counts(p, g, table) for p, g in zip(preds, gts)]
        for n in self.windows:
            for s in range(0, len(per_frame) - n + 1):
                cells = {}
                for f in per_frame[s:s + n]:
                    add_counts(cells, f)
                self._window(n, cells, table)
        cells = {}
        for f in per_frame:
            add_counts(cells, f)
        self.seq_cells.append(cells)
        area_p, area_g, void, joint = tables(cells)
        thing = lambda c: self.categories[c]['isthing'] == 1    # noqa: E731
        # semantic
        left = dict(area_g)
        for (row, key), v in joint.items():
            self.conf[table[row][1], key >> 8] += v
            left[row] -= v
        for row, v in left.items():
            self.conf[table[row][1], VOID] += v                 # the row's pixels under pred VOID
        # association
        thing_crowd = [row for row, (_, rcat, crowd) in enumerate(table) if crowd and thing(rcat)]
        P = {}
        for key in area_p:
            if thing(key >> 8):
                p = area_p[key] - void.get(key, 0)
                for row in thing_crowd:
                    p -= joint.get((row, key), 0)
                P[key] = p
        keys_of = {}
        for (row, key) in joint:
            keys_of.setdefault(row, []).append(key)
        aq_sum = 0.0
        for row, (_, cat, crowd) in enumerate(table):
            if crowd or not thing(cat) or area_g.get(row, 0) == 0:
                continue
            self.num_tracks += 1
            G = area_g[row]
            inner = 0.0
            for key in sorted(keys_of.get(row, [])):            # keys with I > 0, ascending
                if key in P:
                    I = joint[(row, key)]
                    inner += I * (float(I) / float(G + P[key] - I))
            aq_sum += (1.0 / G) * inner
        self.aq_sums.append(aq_sum)
        self.sequences += 1
        self.frames += len(per_frame)

    def pq(self, n, isthing=None):
        """(pq, sq, rq, count of categories) of window length n, as PQStat.pq_average; zeros when no category has a count."""
        pq = sq = rq = 0.0
        k = 0
        for c, info in self.categories.items():
            if isthing is not None and isthing != (info['isthing'] == 1):
                continue
            tp, fp, fn = self.tp[n].get(c, 0), self.fp[n].get(c, 0), self.fn[n].get(c, 0)
            if tp + fp + fn == 0:
                continue
            k += 1
            denom = tp + 0.5 * fp + 0.5 * fn
            pq += self.iou[n].get(c, 0.0) / denom
            sq += self.iou[n].get(c, 0.0) / tp if tp else 0
            rq += tp / denom
        return (pq / k, sq / k, rq / k, k) if k else (0.0, 0.0, 0.0, 0)

    def vpq(self, isthing=None):
        return sum(self.pq(n, isthing)[0] for n in self.windows) / len(self.windows)

    def stq(self):
        ious = []
        for c in range(255):
            denom = int(self.conf[c, :].sum()) + int(self.conf[:, c].sum()) - int(self.conf[c, c])
            if denom > 0:
                ious.append(float(self.conf[c, c]) / float(denom))
        iou = sum(ious) / len(ious) if ious else 0.0
        aq = 0.0
        for s in self.aq_sums:
            aq += s
        aq = aq / max(self.num_tracks, 1)
        return {'stq': math.sqrt(aq * iou), 'aq': aq, 'iou': iou, 'num_tracks': self.num_tracks}


# ------------------------------------------------------------------------------------------------ builders
CATEGORIES = {1: {'id': 1, 'name': 'a', 'isthing': 1, 'color': [220, 20, 60]}, 2: {'id': 2, 'name': 'b', 'isthing': 1, 'color': [0, 0, 142]},
              11: {'id': 11, 'name': 'c', 'isthing': 1, 'color': [119, 11, 32]}, 200: {'id': 200, 'name': 's', 'isthing': 0, 'color': [70, 70, 70]},
              254: {'id': 254, 'name': 't', 'isthing': 0, 'color': [107, 142, 35]}}


def blank_pred(H, W):
    f = np.zeros((H, W, 3), np.uint8)
    f[:, :, 0] = VOID
    return f


def blank_gt(H, W):
    return np.zeros((H, W, 3), np.uint8)


def put_pred(f, cat, inst, y0, y1, x0, x1):
    """Rows y0..y1 and columns x0..x1 inclusive."""
    f[y0:y1 + 1, x0:x1 + 1, 0] = cat
    f[y0:y1 + 1, x0:x1 + 1, 1] = inst


def put_gt(f, gid, y0, y1, x0, x1):
    f[y0:y1 + 1, x0:x1 + 1, 0] = gid & 255
    f[y0:y1 + 1, x0:x1 + 1, 1] = (gid >> 8) & 255
    f[y0:y1 + 1, x0:x1 + 1, 2] = (gid >> 16) & 255


def seg(gid, cat, crowd=0):
    return {'id': gid, 'category_id': cat, 'iscrowd': crowd, 'area': 0}   # (the JSON area is never read)


def gt_from_pred(pred, categories=CATEGORIES):
    """A GT frame equal to a prediction: id = category * 256 + instance + 1 per key -> (gt_rgb, segments_info)."""
    gt = blank_gt(*pred.shape[:2])
    segs = []
    keys = np.unique((pred[:, :, 0].astype(np.int64) << 8) | pred[:, :, 1])
    for k in keys.tolist():
        if k >> 8 == VOID:
            continue
        m = (pred[:, :, 0] == k >> 8) & (pred[:, :, 1] == (k & 255))
        gid = k + 1
        gt[m, 0], gt[m, 1], gt[m, 2] = gid & 255, (gid >> 8) & 255, 0
        segs.append(seg(gid, k >> 8))
    return gt, segs


def blob_sequence(seed, H, W, frames, switch_at=None, unknown_id=True):
    """Drifting rectangles: 3 thing categories (1, 2, 11) and 2 stuff (200, 254), a crowd GT segment, a GT VOID band, pred VOID holes
    and, from frame `switch_at` on, another pred instance number for one object. The prediction is the GT shifted by a pixel with
    noise rectangles. -> (preds, gts, frames_segments_info)."""
    rng = np.random.default_rng(seed)
    nobj = 9
    cats = [1, 2, 11]
    objs = []
    for k in range(nobj):
        h, w = int(rng.integers(1, max(2, H // 3 + 1))), int(rng.integers(1, max(2, W // 3 + 1)))
        objs.append([int(rng.integers(0, H)), int(rng.integers(0, W)), h, w, cats[k % 3], k + 1, int(rng.integers(-2, 3)), int(rng.integers(-2, 3))])
    preds, gts, infos = [], [], []
    for t in range(frames):
        gt, pred = blank_gt(H, W), blank_pred(H, W)
        segs = {}
        # stuff halves
        put_gt(gt, 1000, 0, H - 1, 0, W // 2)
        put_gt(gt, 1001, 0, H - 1, W // 2 + 1, W - 1) if W > 1 else None
        put_pred(pred, 200, 0, 0, H - 1, 0, max(W // 2 - 1, 0))
        put_pred(pred, 254, 0, 0, H - 1, max(W // 2, 0), W - 1)
        for o in objs:
            y, x, h, w, cat, num, dy, dx = o
            y, x = (y + t * dy) % H, (x + t * dx) % W
            gid = 2000 + num
            put_gt(gt, gid, y, min(y + h - 1, H - 1), x, min(x + w - 1, W - 1))
            inst = num if not (switch_at is not None and t >= switch_at and num == 1) else 99
            pcat = cat if num != 4 else cats[(cats.index(cat) + 1) % 3]     # one object predicted with the wrong category
            py, px = min(y + (num & 1), H - 1), x
            put_pred(pred, pcat, inst, py, min(py + h - 1, H - 1), px, min(px + w - 1, W - 1))
        # pred VOID hole and GT VOID band (after the objects: they cut them)
        if H * W > 1:
            put_pred(pred, VOID, 0, H // 3, H // 3, 0, W // 3)
            put_gt(gt, 0, (2 * H) // 3, (2 * H) // 3, 0, W - 1 if H > 2 else W // 2)
            # an id that is in no segments_info: ignored like VOID
            if unknown_id:
                put_gt(gt, 77777, 0, 0, W - 1, W - 1)
        gid = gt[:, :, 0].astype(np.int64) + 256 * gt[:, :, 1].astype(np.int64) + 65536 * gt[:, :, 2].astype(np.int64)
        for g in np.unique(gid).tolist():
            if g == 1000:
                segs[g] = seg(g, 200)
            elif g == 1001:
                segs[g] = seg(g, 254)
            elif 2000 < g < 3000:
                num = g - 2000
                segs[g] = seg(g, objs[num - 1][4], crowd=1 if num == 3 else 0)     # object 3 is a crowd region
        preds.append(pred)
        gts.append(gt)
        infos.append([segs[k] for k in sorted(segs, reverse=True)])              # (JSON order is not id order)
    return preds, gts, infos


# ------------------------------------------------------------------------------------------------ hand-derived cases
# every case: (preds, gts, frames_segments_info, windows); the arithmetic is in tests/test_video_pq_cpu.py beside the expectations
def case_perfect(frames=4):
    preds, gts, infos = [], [], []
    for t in range(frames):
        p = blank_pred(4, 6)
        put_pred(p, 200, 0, 0, 3, 0, 5)
        put_pred(p, 1, 1, 0, 1, t % 3, t % 3 + 1)
        put_pred(p, 2, 5, 3, 3, 4, 5)
        g, s = gt_from_pred(p)
        preds.append(p)
        gts.append(g)
        infos.append(s)
    return preds, gts, infos, (1, 2, 3, 4)


def case_identity_switch(S=6):
    """One thing of S pixels per frame over 4 frames, prediction = GT per frame, the track id changes after frame 2."""
    preds, gts, infos = [], [], []
    for t in range(4):
        p, g = blank_pred(2, S), blank_gt(2, S)
        put_pred(p, 1, 1 if t < 2 else 2, 0, 0, 0, S - 1)
        put_gt(g, 7, 0, 0, 0, S - 1)
        preds.append(p)
        gts.append(g)
        infos.append([seg(7, 1)])
    return preds, gts, infos, (1, 2, 3, 4)


def case_iou_half():
    """GT 4 pixels, pred 2 of them: iou = 2 / 4 exactly -> not matched."""
    p, g = blank_pred(1, 8), blank_gt(1, 8)
    put_gt(g, 5, 0, 0, 0, 3)
    put_pred(p, 1, 1, 0, 0, 0, 1)
    return [p], [g], [[seg(5, 1)]], (1,)


def case_fp_skip(void_pixels):
    """A pred tube of 4 pixels with `void_pixels` of them on ignored GT and the rest on stuff GT of another category."""
    p, g = blank_pred(1, 8), blank_gt(1, 8)
    put_gt(g, 9, 0, 0, 0, 7)
    put_gt(g, 0, 0, 0, 0, void_pixels - 1)
    put_pred(p, 1, 1, 0, 0, 0, 3)
    return [p], [g], [[seg(9, 200)]], (1,)


def case_crowd():
    """A crowd thing (id 3, 4 pixels) with a pred tube (1, 1) of 6 pixels, 4 of them on the crowd; a GT track (id 4, 2 pixels) that
    the tube's other 2 pixels cover."""
    p, g = blank_pred(1, 8), blank_gt(1, 8)
    put_gt(g, 3, 0, 0, 0, 3)
    put_gt(g, 4, 0, 0, 4, 5)
    put_pred(p, 1, 1, 0, 0, 0, 5)
    return [p], [g], [[seg(3, 1, crowd=1), seg(4, 1)]], (1,)


def case_cross_category():
    """GT track of category 1 (4 pixels) covered exactly by a pred track of category 2."""
    p, g = blank_pred(1, 8), blank_gt(1, 8)
    put_gt(g, 6, 0, 0, 0, 3)
    put_pred(p, 2, 1, 0, 0, 0, 3)
    return [p], [g], [[seg(6, 1)]], (1,)


def case_short():
    """Two frames, windows (1, 3): the window of 3 gets nothing."""
    preds, gts, infos, _ = case_perfect(2)
    return preds, gts, infos, (1, 3)
