"""Plain numpy / Python restatement of the tracking rule with constant-velocity motion prediction, written from the
text of the rule: dicts and loops, Python ints. The yardstick of tests/test_pan_track_motion_cpu.py (hand-derived cases) and
tests/test_pan_track_motion_gpu.py (bit-for-bit parity of the device). Frames, state and rows as in tests/pan_track_ref.py.

Beyond the plain tracker's state every track (c, j) carries (cx, cy, vx, vy): the floor centroid of the pixels it was last assigned
and its velocity in pixels per frame. A step first shifts every remembered pixel by its track's velocity times the track's age into
the *predicted memory* (``predicted()``: int32 [H,W], c << 8 | j, -1 for none), counts and matches against that, and decides what is
live and what may be taken over from the real memory.
"""
import functools

import numpy as np

from pan_track_ref import MAX_PIXELS, VOID, blank, check_params, dots, put, strip

AGE_CAP = 65535       # ages compete as min(age, AGE_CAP): the device packs (age, key) into 32 bits


class RefMotionTracker:
    def __init__(self, iou_thresh=0.3, max_age=0):
        check_params(iou_thresh, max_age)
        self.iou_thresh = float(iou_thresh)
        self.max_age = int(max_age)
        self.reset()

    def reset(self):
        self.shape = None
        self.key = None
        self.frame = None
        self.pred = None
        self.cursor = {}
        self.t = 0
        self.motion = {}          # (c, j) -> [cx, cy, vx, vy]
        self.serial_of = {}
        self.next_serial = 1

    def state(self):
        return self.key.copy(), self.frame.copy()

    def predicted(self):
        return self.pred.copy()

    def motion_state(self):
        """{(c, j): (cx, cy, vx, vy)} of the tracks the real memory holds."""
        return {(k >> 8, k & 255): tuple(self.motion[(k >> 8, k & 255)]) for k in np.unique(self.key[self.key >= 0]).tolist()}

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
        cur_key = cat << 8 | ins

        # 1. predict: every real-memory pixel votes for its place shifted by velocity x age; the youngest track wins a pixel, then
        # the smallest key. What is live and the frame a track was last assigned come from the real memory.
        real = {}                 # (c, j) -> (ys, xs, last frame)
        for k in np.unique(self.key[self.key >= 0]).tolist():
            ys, xs = np.nonzero(self.key == k)
            real[(k >> 8, k & 255)] = (ys.astype(np.int64), xs.astype(np.int64), int(self.frame[ys[0], xs[0]]))
        pred = np.full((H, W), -1, np.int64)
        for age, k in sorted((min(t - real[cj][2], AGE_CAP), cj[0] << 8 | cj[1]) for cj in real):
            cj = (k >> 8, k & 255)
            ys, xs, s = real[cj]
            _, _, vx, vy = self.motion[cj]
            ny, nx = ys + vy * (t - s), xs + vx * (t - s)
            ok = (ny >= 0) & (ny < H) & (nx >= 0) & (nx < W)
            ny, nx = ny[ok], nx[ok]
            free = pred[ny, nx] < 0
            pred[ny[free], nx[free]] = k
        self.pred = pred.astype(np.int32)

        # 2. counts on the predicted memory
        has_pred = pred >= 0
        a_cur, a_mem, inter = {}, {}, {}
        ks, ns = np.unique(pred[has_pred], return_counts=True)
        for k, n in zip(ks.tolist(), ns.tolist()):
            a_mem[(k >> 8, k & 255)] = n
        ks, ns = np.unique(cur_key[thing], return_counts=True)
        for k, n in zip(ks.tolist(), ns.tolist()):
            a_cur[(k >> 8, k & 255)] = n
        both = thing & has_pred & ((pred >> 8) == cat)
        ks, ns = np.unique(cur_key[both] << 8 | (pred[both] & 255), return_counts=True)
        for k, n in zip(ks.tolist(), ns.tolist()):
            inter[(k >> 16, k >> 8 & 255, k & 255)] = n

        # candidates and greedy matching per category, as in the plain rule
        assign = {}               # (c, i) -> (id, matched, I, U, taken_over)
        taken_tracks = set()
        for c in sorted(set(c for c, _ in a_cur)):
            cand = []
            for (cc, i, j), I in inter.items():
                if cc != c:
                    continue
                U = a_cur[(c, i)] + a_mem[(c, j)] - I
                if I > 0 and float(I) >= self.iou_thresh * float(U):
                    cand.append((I, U, i, j))

            def before(a, b):
                l, r = a[0] * b[1], b[0] * a[1]
                if l != r:
                    return l > r
                return (a[2], a[3]) < (b[2], b[3])
            seg_done, trk_done = set(), set()
            for I, U, i, j in sorted(cand, key=functools.cmp_to_key(lambda a, b: -1 if before(a, b) else 1)):
                if i in seg_done or j in trk_done:
                    continue
                seg_done.add(i)
                trk_done.add(j)
                assign[(c, i)] = (j, 1, I, U, 0)
                taken_tracks.add((c, j))

        # 3. new tracks, ascending (c, i): live and the take-over pool are those of the REAL memory
        for (c, i) in sorted(a_cur):
            if (c, i) in assign:
                continue
            live = set(j for (cc, j) in real if cc == c) | set(j for (cc, j) in taken_tracks if cc == c)
            n = self.cursor.get(c, 0)
            got, over = None, 0
            for k in range(255):
                cid = (n + k) % 255 + 1
                if cid not in live:
                    got = cid
                    self.cursor[c] = n + k + 1
                    break
            if got is None:
                pool = [(real[(c, j)][2], j) for (cc, j) in real if cc == c and (c, j) not in taken_tracks]
                got = min(pool)[1]
                over = 1
            assign[(c, i)] = (got, 0, 0, a_cur[(c, i)], over)
            taken_tracks.add((c, got))

        # 4. output map and real memory, as in the plain rule
        key = self.key.astype(np.int64)
        has_mem = key >= 0
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

        # 5. motion state of every assigned segment
        for (c, i) in sorted(a_cur):
            j, matched = assign[(c, i)][:2]
            ys, xs = np.nonzero(thing & (cur_key == (c << 8 | i)))
            cx, cy = sum(xs.tolist()) // len(xs), sum(ys.tolist()) // len(ys)
            vx = vy = 0
            if matched:
                ox, oy = self.motion[(c, j)][:2]
                gap = t - real[(c, j)][2]
                dx, dy = cx - ox, cy - oy
                vx = abs(dx) // gap * (1 if dx >= 0 else -1)       # truncated toward zero
                vy = abs(dy) // gap * (1 if dy >= 0 else -1)
            self.motion[(c, j)] = [cx, cy, vx, vy]

        rows, segments = [], []
        for (c, i) in sorted(a_cur):
            tid_, matched, I, U, over = assign[(c, i)]
            rows.append((c, i, tid_, matched, I, U, a_cur[(c, i)], over))
            if matched:
                serial = self.serial_of[(c, tid_)]
            else:
                serial = self.next_serial
                self.next_serial += 1
                self.serial_of[(c, tid_)] = serial
            segments.append({'category': c, 'instance_in': i, 'instance': tid_, 'track_id': serial, 'matched': bool(matched),
                             'iou': float(I) / float(U), 'area': a_cur[(c, i)]})
        self.t = t + 1
        return out, np.array(rows, np.int32).reshape(-1, 8), segments


def track_sequence(pans, **kw):
    trk = RefMotionTracker(**kw)
    return [trk.update(p) for p in pans]


# ---------------------------------------------------------------------------------------------
# Cases shared by the CPU and the GPU tests. Every builder returns (frames, tracker keywords).
def bar(H, W, xs, c=1, width=4):
    """One `width`-pixel-wide, H-pixel-high object of category c per frame at column x (None: hidden; columns past the image are cut)."""
    frames = []
    for x in xs:
        f = blank(H, W)
        if x is not None:
            put(f, c, 1, 0, H - 1, max(x, 0), min(x + width, W) - 1)
        frames.append(f)
    return frames


def case_accelerating():
    return bar(3, 40, [0, 1, 4, 7, 10]), dict(iou_thresh=0.3, max_age=0)


def case_hidden_moving():
    return bar(3, 40, [0, 2, 4, None, None, 10, 12]), dict(iou_thresh=0.3, max_age=2)


def case_crossing():
    """Two 6 x 4 objects of one category at +3 and -3 pixels per frame that pass each other; they share row 3, where the one moving
    left is painted over the other (so the other's centroid, 24 pixels against 18..23, moves by less than a pixel). Numbered afresh
    per frame from right to left."""
    frames = []
    for t in range(8):
        f = blank(7, 40)
        a, b = 2 + 3 * t, 32 - 3 * t
        put(f, 1, 1 if a > b else 2, 0, 3, a, a + 5)
        put(f, 1, 2 if a > b else 1, 3, 6, b, b + 5)
        frames.append(f)
    return frames, dict(iou_thresh=0.3, max_age=0)


def case_conflict_equal_age():
    """1 x 24. Track (1,1) moves right and track (1,2) left by 2 per frame, both hide for a frame, and at frame 3 both are predicted
    (age 2) at columns 6..9: the smaller key takes every pixel. Track (1,2) is predicted nowhere, but the real memory still holds it."""
    f0 = strip(24, (1, 1, 0, 3), (1, 2, 12, 15))
    f1 = strip(24, (1, 1, 2, 5), (1, 2, 10, 13))
    return [f0, f1, strip(24), strip(24, (1, 1, 6, 9))], dict(iou_thresh=0.3, max_age=2)


def case_conflict_younger():
    """1 x 24. As above from columns 0..3 and 16..19, but track (1,2) is seen once more (frame 2, columns 12..15). At frame 4 track
    (1,1) (age 3) and track (1,2) (age 2) are both predicted at columns 8..11: the younger one takes them, though its key is larger."""
    f0 = strip(24, (1, 1, 0, 3), (1, 2, 16, 19))
    f1 = strip(24, (1, 1, 2, 5), (1, 2, 14, 17))
    f2 = strip(24, (1, 1, 12, 15))
    return [f0, f1, f2, strip(24), strip(24, (1, 1, 8, 11))], dict(iou_thresh=0.3, max_age=2)


def case_off_image_wrap():
    """In the manner of pan_track_ref.case_wrap, 18 x 16, category 2, max_age 1. Frame 0: a 4-pixel bar on row 0 (columns 2..5, id 1)
    and 253 one-pixel instances from row 1 on (ids 2..254, cursor 254). Frame 1: the bar alone at columns 0..3 (I 2, U 6): v = (-2, 0).
    Frame 2: one new pixel; the dots are still remembered, so it gets id 255 and the cursor wraps. The bar is predicted at columns
    -2..1. Frame 3: one new pixel. The dots have expired; the bar (last seen at frame 1) is predicted at columns -4..-1, off the image,
    but the real memory holds it: id 1 is live, the pixel gets id 2. After frame 3 the bar has expired too."""
    f0 = dots(18, 16, 2, [0] + list(range(16, 269)))
    put(f0, 2, 1, 0, 0, 2, 5)
    f0[0, 0] = VOID
    f1 = put(blank(18, 16), 2, 1, 0, 0, 0, 3)
    return [f0, f1, dots(18, 16, 2, [280]), dots(18, 16, 2, [284])], dict(iou_thresh=0.3, max_age=1)


def case_truncation():
    """1 x 40: a 6-pixel object at columns 20..25 (cx 22), then 17..22 (cx 19, v = -3), hidden, then at 12..17 (cx 14) against the
    prediction 11..16 (I 5, U 7). The displacement -5 over a gap of 2 gives v = trunc(-2.5) = -2, not floor(-2.5) = -3."""
    frames = [strip(40, (1, 1, 20, 25)), strip(40, (1, 1, 17, 22)), strip(40), strip(40, (1, 1, 12, 17))]
    return frames, dict(iou_thresh=0.3, max_age=1)


def velocity_sequence(seed, H, W, things, frames, cats, vmax=3, side=10, blink=0.15, stuff=(7, 9)):
    """`things` rectangles of up to side x side pixels of the thing categories `cats` over a stuff background, each with a fixed
    velocity of up to vmax pixels per frame per axis (objects leave the image and do not come back); per frame an object blinks out
    with probability `blink`; the instance numbers of a frame follow a fresh random order per category, later objects paint over
    earlier ones; a strip of VOID stays."""
    rng = np.random.default_rng(seed)
    objs = []
    for _ in range(things):
        h, w = int(rng.integers(1, side + 1)), int(rng.integers(1, side + 1))
        objs.append([int(rng.choice(cats)), int(rng.integers(0, H)), int(rng.integers(0, W)), h, w,
                     int(rng.integers(-vmax, vmax + 1)), int(rng.integers(-vmax, vmax + 1))])
    out = []
    for _ in range(frames):
        f = blank(H, W)
        for k, c in enumerate(stuff):
            f[k * H // (len(stuff) + 1):(k + 1) * H // (len(stuff) + 1)] = (c, 0, 0)
        count = {}
        for b in rng.permutation(len(objs)):
            c, y, x, h, w, vy, vx = objs[b]
            y0, y1, x0, x1 = max(y, 0), min(y + h, H) - 1, max(x, 0), min(x + w, W) - 1
            if rng.random() < blink or y0 > y1 or x0 > x1:
                continue
            count[c] = count.get(c, 0) + 1
            if count[c] <= 255:
                put(f, c, count[c], y0, y1, x0, x1)
        out.append(f)
        for o in objs:
            o[1] += o[5]
            o[2] += o[6]
    return out
