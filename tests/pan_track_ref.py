"""Plain numpy / Python restatement of the panoptic tracking rule, written from the text of the rule: dicts and
loops, one float64 product for the threshold test, Python ints for the cross-multiplied IoU order. The yardstick of
tests/test_pan_track_cpu.py (hand-derived cases) and tests/test_pan_track_gpu.py (bit-for-bit parity of the device).

A frame is uint8 [H,W,3]: channel 0 category (255 = VOID), channel 1 instance. A thing segment is (c, i) with c != 255 and i >= 1.

State, in the form PanopticTracker.state() documents: ``key`` int32 [H,W], c << 8 | j for a remembered track (c, j) and -1 for none;
``frame`` int32 [H,W], the index of the frame that last wrote the pixel and -1 for none.

Rows (one per current thing segment, ascending (c, i)): (c, i, id, matched, I, U, area, taken_over); an unmatched segment has
I = 0 and U = area.
"""
import functools

import numpy as np

MAX_PIXELS = 1 << 24
ROW_FIELDS = ('category', 'instance_in', 'instance', 'matched', 'inter', 'union', 'area', 'taken_over')


def check_params(iou_thresh, max_age):
    if not (1.0 / 16.0 <= float(iou_thresh) <= 1.0):      # (NaN fails too)
        raise ValueError("iou_thresh %r outside [1/16, 1]" % (iou_thresh,))
    if int(max_age) != max_age or max_age < 0:
        raise ValueError("max_age %r must be an integer >= 0" % (max_age,))


class RefTracker:
    def __init__(self, iou_thresh=0.3, max_age=0):
        check_params(iou_thresh, max_age)
        self.iou_thresh = float(iou_thresh)
        self.max_age = int(max_age)
        self.reset()

    def reset(self):
        self.shape = None
        self.key = None
        self.frame = None
        self.cursor = {}          # category -> n_c
        self.t = 0
        self.serial_of = {}       # (c, id) -> serial
        self.next_serial = 1

    def state(self):
        return self.key.copy(), self.frame.copy()

    def update(self, pan):
        pan = np.asarray(pan)
        if pan.dtype != np.uint8 or pan.ndim != 3 or pan.shape[2] != 3:
            raise ValueError("frame must be uint8 [H,W,3]")
        H, W = pan.shape[:2]
        if H * W > MAX_PIXELS:
            raise ValueError("frame of %d x %d pixels: H * W must not exceed 2^24" % (H, W))
        if self.shape is None:
            if H < 1 or W < 1:
                raise ValueError("empty frame")
            self.shape = (H, W)
            self.key = np.full((H, W), -1, np.int32)
            self.frame = np.full((H, W), -1, np.int32)
        elif (H, W) != self.shape:
            raise ValueError("frame size %s differs from the tracker's %s" % ((H, W), self.shape))
        t = self.t
        cat = pan[:, :, 0].astype(np.int64)
        ins = pan[:, :, 1].astype(np.int64)
        thing = (cat != 255) & (ins >= 1)

        # 1. counts (np.unique over the pixels; the cells go into dicts)
        key = self.key.astype(np.int64)
        has_mem = key >= 0
        a_cur, a_mem, inter, mem_frame = {}, {}, {}, {}
        ks, ns = np.unique(key[has_mem], return_counts=True)
        for k, n in zip(ks.tolist(), ns.tolist()):
            a_mem[(k >> 8, k & 255)] = n
            mem_frame[(k >> 8, k & 255)] = int(self.frame[self.key == k].min())
        cur_key = cat << 8 | ins
        ks, ns = np.unique(cur_key[thing], return_counts=True)
        for k, n in zip(ks.tolist(), ns.tolist()):
            a_cur[(k >> 8, k & 255)] = n
        both = thing & has_mem & ((key >> 8) == cat)
        ks, ns = np.unique(cur_key[both] << 8 | (key[both] & 255), return_counts=True)
        for k, n in zip(ks.tolist(), ns.tolist()):
            inter[(k >> 16, k >> 8 & 255, k & 255)] = n

        # 2. candidates, 3. greedy matching per category
        assign = {}               # (c, i) -> (id, matched, I, U, taken_over)
        taken_tracks = set()      # (c, j) matched or (re-)issued in this step
        cats = sorted(set(c for c, _ in a_cur))
        for c in cats:
            cand = []
            for (cc, i, j), I in inter.items():
                if cc != c:
                    continue
                U = a_cur[(c, i)] + a_mem[(c, j)] - I
                if I > 0 and float(I) >= self.iou_thresh * float(U):
                    cand.append((I, U, i, j))

            def before(a, b):     # a strictly precedes b
                l, r = a[0] * b[1], b[0] * a[1]          # I1 U2 against I2 U1 in exact integers
                if l != r:
                    return l > r
                return (a[2], a[3]) < (b[2], b[3])
            order = sorted(cand, key=functools.cmp_to_key(lambda a, b: -1 if before(a, b) else 1))   # (a strict total order)
            seg_done, trk_done = set(), set()
            for I, U, i, j in order:
                if i in seg_done or j in trk_done:
                    continue
                seg_done.add(i)
                trk_done.add(j)
                assign[(c, i)] = (j, 1, I, U, 0)
                taken_tracks.add((c, j))

        # 4. new tracks, ascending (c, i)
        for (c, i) in sorted(a_cur):
            if (c, i) in assign:
                continue
            live = set(j for (cc, j) in a_mem if cc == c) | set(j for (cc, j) in taken_tracks if cc == c)
            n = self.cursor.get(c, 0)
            got, over = None, 0
            for k in range(255):
                cid = (n + k) % 255 + 1
                if cid not in live:
                    got = cid
                    self.cursor[c] = n + k + 1
                    break
            if got is None:
                # all 255 ids live: take over the unmatched memory track with the oldest frame index, ties to the smallest id
                # (the cursor stays where it is)
                pool = [(mem_frame[(c, j)], j) for (cc, j) in a_mem if cc == c and (c, j) not in taken_tracks]
                got = min(pool)[1]
                over = 1
            assign[(c, i)] = (got, 0, 0, a_cur[(c, i)], over)
            taken_tracks.add((c, got))

        # 5. output map, 6. memory
        out = pan.copy()
        id_of = np.zeros(65536, np.int64)
        for (c, i), v in assign.items():
            id_of[c << 8 | i] = v[0]
        gone = np.zeros(65536, bool)
        for (c, j) in taken_tracks:
            gone[c << 8 | j] = True
        tid = id_of[cur_key & 65535]
        out[:, :, 1] = np.where(thing, tid, pan[:, :, 1])
        out[:, :, 2] = np.where(thing, 0, pan[:, :, 2])
        clear = ~thing & has_mem & (gone[np.where(has_mem, key, 0)] | (t - self.frame.astype(np.int64) > self.max_age))
        self.key = np.where(thing, cat << 8 | tid, np.where(clear, -1, key)).astype(np.int32)
        self.frame = np.where(thing, t, np.where(clear, -1, self.frame)).astype(np.int32)

        rows = []
        segments = []
        for (c, i) in sorted(a_cur):
            tid, matched, I, U, over = assign[(c, i)]
            rows.append((c, i, tid, matched, I, U, a_cur[(c, i)], over))
            if matched:
                serial = self.serial_of[(c, tid)]
            else:
                serial = self.next_serial
                self.next_serial += 1
                self.serial_of[(c, tid)] = serial
            segments.append({'category': c, 'instance_in': i, 'instance': tid, 'track_id': serial, 'matched': bool(matched),
                             'iou': float(I) / float(U), 'area': a_cur[(c, i)]})
        self.t = t + 1
        return out, np.array(rows, np.int32).reshape(-1, 8), segments


def track_sequence(pans, **kw):
    trk = RefTracker(**kw)
    return [trk.update(p) for p in pans]


# ---------------------------------------------------------------------------------------------
# Frame-stable colours: pure functions of (category, instance).
CUBE = 226981      # 61^3
STEP = 100003


def lowbias32(x):
    x &= 0xffffffff
    x ^= x >> 16
    x = (x * 0x7feb352d) & 0xffffffff
    x ^= x >> 15
    x = (x * 0x846ca68b) & 0xffffffff
    x ^= x >> 16
    return x


def stable_picture_colour(category, instance, base_rgb, isthing):
    """Stuff: the category colour. Thing: the formatter's offset rule with ordinal := instance, first attempt whose colour is not
    (0,0,0); no taken set."""
    base = tuple(int(v) for v in base_rgb)
    if not isthing:
        return base
    start = lowbias32(int(category) << 16 | int(instance)) % CUBE
    for a in range(CUBE):
        cell = (start + a * STEP) % CUBE
        d = (cell % 61 - 30, cell // 61 % 61 - 30, cell // 3721 - 30)
        col = tuple(min(max(b + o, 0), 255) for b, o in zip(base, d))
        if col != (0, 0, 0):
            return col
    raise AssertionError("unreachable: the cube holds a non-zero offset")


def stable_png_colour(category, instance):
    return (0, 0, 0) if category == 255 else (int(category), int(instance), 1)


def stable_png(pan):
    pan = np.asarray(pan)
    out = np.zeros_like(pan)
    live = pan[:, :, 0] != 255
    out[:, :, 0] = np.where(live, pan[:, :, 0], 0)
    out[:, :, 1] = np.where(live, pan[:, :, 1], 0)
    out[:, :, 2] = live
    return out


# ---------------------------------------------------------------------------------------------
# Cases shared by the CPU tests (which hold the restatement to hand-derived answers) and the GPU tests (which hold the device to the
# restatement). Every builder returns (frames, tracker keywords).
VOID = (255, 0, 0)


def blank(H, W, fill=VOID):
    f = np.zeros((H, W, 3), np.uint8)
    f[:, :] = fill
    return f


def put(f, c, i, y0, y1, x0, x1):
    """Paint rows y0..y1 and columns x0..x1 (inclusive) as (c, i, 0)."""
    f[y0:y1 + 1, x0:x1 + 1] = (c, i, 0)
    return f


def strip(W, *segs):
    """A 1 x W frame of VOID with segments (c, i, x0, x1)."""
    f = blank(1, W)
    for c, i, x0, x1 in segs:
        put(f, c, i, 0, 0, x0, x1)
    return f


def case_three_frames():
    f0 = blank(6, 8)
    put(f0, 7, 0, 2, 2, 0, 7)           # stuff
    put(f0, 3, 1, 0, 1, 0, 3)
    put(f0, 3, 2, 3, 5, 4, 7)
    f1 = blank(6, 8)
    put(f1, 7, 0, 2, 2, 0, 7)
    put(f1, 3, 1, 3, 5, 3, 6)           # the second object, one column to the left, now detection 1
    put(f1, 3, 2, 0, 1, 1, 4)           # the first object, one column to the right
    put(f1, 5, 1, 5, 5, 0, 1)           # a new object of another category
    f2 = blank(6, 8)
    put(f2, 7, 0, 2, 2, 0, 7)
    put(f2, 3, 1, 3, 5, 2, 5)
    put(f2, 3, 2, 0, 0, 6, 7)           # a new object where nothing was
    return [f0, f1, f2], dict(iou_thresh=0.3, max_age=0)


def case_contested(thr):
    f0 = strip(40, (1, 1, 0, 5), (1, 2, 6, 11), (1, 3, 12, 25))
    f1 = strip(40, (1, 1, 3, 21), (1, 2, 22, 27))
    return [f0, f1], dict(iou_thresh=thr, max_age=0)


def case_tie():
    f0 = strip(20, (1, 1, 0, 3), (1, 2, 8, 11))
    f1 = strip(20, (1, 1, 2, 9), (1, 2, 11, 12))
    return [f0, f1], dict(iou_thresh=0.125, max_age=0)


def case_equality(thr, short):
    """I = thr * U exactly (short = False) or one pixel of intersection less (short = True)."""
    if thr == 0.5:
        f0 = strip(12, (1, 1, 0, 3))
        f1 = strip(12, (1, 1, 3, 4)) if short else strip(12, (1, 1, 2, 3))      # I, U = 1, 5 | 2, 4
    elif thr == 0.25:
        f0 = strip(12, (1, 1, 0, 5))
        f1 = strip(12, (1, 1, 5, 8)) if short else strip(12, (1, 1, 4, 7))      # I, U = 1, 9 | 2, 8
    else:
        raise ValueError(thr)
    return [f0, f1], dict(iou_thresh=thr, max_age=0)


def case_hidden(max_age):
    f0 = strip(12, (1, 1, 0, 3))
    f1 = strip(12, (7, 0, 0, 3))        # stuff over the object
    f2 = strip(12, (1, 1, 1, 4))
    return [f0, f1, f2], dict(iou_thresh=0.3, max_age=max_age)


def dots(H, W, c, pixels):
    """One-pixel instances 1, 2, ... of category c at the given flat pixel indices."""
    f = blank(H, W)
    flat = f.reshape(-1, 3)
    for k, p in enumerate(pixels):
        flat[p] = (c, k + 1, 0)
    return f


def case_wrap():
    f0 = dots(17, 16, 2, range(254))                       # ids 1..254, cursor 254
    f1 = dots(17, 16, 2, [0, 2])                           # tracks 1 and 3 live on
    f2 = dots(17, 16, 2, [0, 2, 260, 261, 262, 263])       # four new segments: ids 255, 2, 4, 5
    return [f0, f1, f2], dict(iou_thresh=0.3, max_age=0)


def case_takeover():
    """16 x 16, 255 one-pixel instances at pixels 0..254, then every instance one pixel on. Only pixel 255 is free, so 254 shifted
    instances sit on the old pixel of their neighbour (and match it, IoU 1); none overlaps its own old pixel. The instance on the free
    pixel is frame 1's first (and only) new segment: all 255 ids are live, it takes over the oldest unmatched track, id 1."""
    f0 = dots(16, 16, 4, range(255))
    f1 = dots(16, 16, 4, range(1, 256))
    return [f0, f1], dict(iou_thresh=0.3, max_age=1)


def case_takeover_all():
    """16 x 32: 255 instances at pixels 0..254, then 255 at pixels 256..510 (no overlap at all): every id is taken over in turn."""
    f0 = dots(16, 32, 4, range(255))
    f1 = dots(16, 32, 4, range(256, 511))
    f2 = dots(16, 32, 4, [0, 256, 300])
    return [f0, f1, f2], dict(iou_thresh=0.3, max_age=1)


def blob_sequence(seed, H, W, things, frames, cats, stuff=(7, 9), step=3, churn=0.15):
    """`things` rectangular blobs of the thing categories `cats` over a stuff background, each moving by up to `step` pixels per
    frame; per frame a blob dies with probability `churn` and is replaced by a new one; the instance numbers of a frame follow a
    fresh random order per category (as detection scores would), later blobs paint over earlier ones; a strip of VOID stays."""
    rng = np.random.default_rng(seed)
    smax = max(2, min(H, W) // 3)

    def born():
        h, w = int(rng.integers(1, smax + 1)), int(rng.integers(1, smax + 1))
        return [int(rng.choice(cats)), int(rng.integers(0, H)), int(rng.integers(0, W)), h, w]
    blobs = [born() for _ in range(things)]
    out = []
    for _ in range(frames):
        f = blank(H, W)
        for k, c in enumerate(stuff):
            f[k * H // (len(stuff) + 1):(k + 1) * H // (len(stuff) + 1)] = (c, 0, 0)
        order = rng.permutation(len(blobs))
        count = {}
        for b in order:
            c, y, x, h, w = blobs[b]
            count[c] = count.get(c, 0) + 1
            if count[c] > 255:
                continue
            put(f, c, count[c], max(y, 0), min(y + h, H) - 1, max(x, 0), min(x + w, W) - 1)
        out.append(f)
        for b in range(len(blobs)):
            if rng.random() < churn:
                blobs[b] = born()
            else:
                blobs[b][1] = int(np.clip(blobs[b][1] + rng.integers(-step, step + 1), 0, H - 1))
                blobs[b][2] = int(np.clip(blobs[b][2] + rng.integers(-step, step + 1), 0, W - 1))
    return out
