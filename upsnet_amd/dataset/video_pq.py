"""Video metrics of tracked sequences on the device (csrc/video_eval.hip): Video Panoptic Quality (VPQ; Kim et
al., Video Panoptic Segmentation, CVPR 2020) and Segmentation and Tracking Quality (STQ; Weber et al., STEP, NeurIPS 2021).

The reference has no video metric. The rules are this project's restatement of the published definitions, stated in
include/upsnet_hip.h and restated in plain numpy in tests/video_pq_ref.py; they were never compared with a build of either tool.

    ev = VideoPanopticEvaluator(categories, windows=(1, 2, 3, 4))
    for frames in sequences:
        ev.begin_sequence([f['segments_info'] for f in frames])      # the sequence table: the union of the frames' GT segments
        for f in frames:
            ev.add_frame(f['pred_2ch'], f['gt_rgb'])                 # uint8 [H,W,3] device tensors (numpy arrays are uploaded)
        ev.end_sequence()
    result = ev.summary()

add_frame only queues work: one pass over the frame's pixels, a compaction and the window pass of every window that ends at the
frame; nothing waits for the host between begin_sequence and end_sequence. end_sequence queues the delivery of the sequence's integer
cells and one asynchronous copy of them; STQ's few float64 operations run on the host, from those integers, when vpq_stat / stq /
summary synchronise. The prediction is what PanopticTracker.update returns and what a sequence run writes to pan_2ch/.
"""
import logging
import math

import numpy as np
import torch

from .. import ops
from .._lib import lib
from .pq import MAX_CATEGORY, _check_image

logger = logging.getLogger(__name__)

MAX_PIXELS = 1 << 24
MAX_SEQUENCE_PIXELS = 1 << 31      # frames * H * W of one sequence: its counts are 32-bit
NO_KEY_ERROR = (1 << 63) - 1
FULL = {1: "the frame table was full (more distinct (GT segment, predicted tube) pairs in one frame than one per 16 pixels)",
        2: "the sequence table was full (more than 32768 distinct cells in one sequence)",
        4: "a window held more than 8192 list entries"}


def check_windows(windows):
    """The window lengths as a tuple; ValueError unless they are ascending, unique integers in 1..8."""
    try:
        w = tuple(windows)
        ok = len(w) >= 1 and all(int(n) == n and 1 <= n <= 8 for n in w) and all(b > a for a, b in zip(w, w[1:]))
    except TypeError:
        ok = False
    if not ok:
        raise ValueError("windows must be ascending, unique integers in 1..8, got %r" % (windows,))
    return tuple(int(n) for n in w)


def sequence_rows(frames_segments_info, max_gt_segments):
    """The sequence table: the union of the frames' GT segments in ascending id -> int64 [n,3] (id, category, iscrowd). ValueError: an
    id 0, outside 1..2^24-1 or twice in one frame, with two categories or two crowd flags in the sequence, a category outside 0..254,
    more than max_gt_segments rows."""
    rows = {}
    for t, segs in enumerate(frames_segments_info):
        seen = set()
        for el in segs:
            gid, cat, crowd = int(el['id']), int(el['category_id']), int(el.get('iscrowd', 0))
            if gid == 0:
                raise ValueError("frame %d: GT segment with id 0 (the VOID id of the panoptic PNG)" % t)
            if not 0 < gid < (1 << 24):
                raise ValueError("frame %d: GT segment id %d outside 1..2^24-1" % (t, gid))
            if gid in seen:
                raise ValueError("frame %d: duplicate GT segment id %d" % (t, gid))
            seen.add(gid)
            if not 0 <= cat <= MAX_CATEGORY:
                raise ValueError("frame %d: GT category id %d outside 0..%d" % (t, cat, MAX_CATEGORY))
            if crowd not in (0, 1):
                raise ValueError("frame %d: GT segment %d has iscrowd %r" % (t, gid, el.get('iscrowd')))
            if gid in rows and rows[gid] != (gid, cat, crowd):
                raise ValueError("GT id %d is (category %d, iscrowd %d) in frame %d and (category %d, iscrowd %d) before: an id means "
                                 "one object in every frame of a sequence" % (gid, cat, crowd, t, rows[gid][1], rows[gid][2]))
            rows[gid] = (gid, cat, crowd)
    if len(rows) > max_gt_segments:
        raise ValueError("%d GT segments in the sequence, more than max_gt_segments=%d" % (len(rows), max_gt_segments))
    return np.array([rows[k] for k in sorted(rows)], np.int64).reshape(len(rows), 3)


class _Sequence(object):
    __slots__ = ('index', 'name', 'rows', 'table', 'num_crowd', 'shape', 'frames', 'host', 'event')


class VideoPanopticEvaluator(object):
    """Running VPQ / STQ statistics of tracked sequences on one device.

    categories: the dataset's category table, {id: {'isthing': 0/1, ...}} or the JSON's list of dicts with 'id'. windows: the window
    lengths in frames, ascending, unique, each in 1..8 (Cityscapes-VPS: (1, 2, 3, 4) is k = 0, 5, 10, 15, only the labelled frames
    being scored).
    begin_sequence(frames_segments_info, name=None) builds and validates the sequence table; add_frame(pred_2ch, gt_rgb) queues one
    frame; end_sequence() queues the sequence's delivery. vpq_stat() -> {n: PQStat}; stq() -> dict; summary() -> everything, logged.
    ValueError before any launch, the state untouched: see sequence_rows and check_windows; a frame that is not uint8 [H,W,3], of
    another shape than the sequence's first, of more than 2^24 pixels (or 2^31 in the whole sequence); add_frame / end_sequence outside
    a sequence, begin_sequence inside one. KeyError at the first synchronisation: a pred category that is not in `categories`, naming
    sequence, frame and category. RuntimeError at the first synchronisation: a full table (counts were dropped, never silently)."""

    def __init__(self, categories, windows=(1, 2, 3, 4), max_gt_segments=4096, device=None):
        if not isinstance(categories, dict):
            categories = {el['id']: el for el in categories}
        bad = [c for c in categories if not 0 <= int(c) <= MAX_CATEGORY]
        if bad:
            raise ValueError("category ids must lie in 0..%d, got %s" % (MAX_CATEGORY, bad))
        if not 0 <= int(max_gt_segments) <= 4096:
            raise ValueError("max_gt_segments %d outside 0..4096" % max_gt_segments)
        self.categories = categories
        self.windows = check_windows(windows)
        self.max_gt_segments = int(max_gt_segments)
        self.device = torch.device(device) if device is not None else None
        self.num_sequences = 0
        self.num_frames = 0
        self.conf = np.zeros((256, 256), np.int64)
        self.aq_sums = []              # one float64 per resolved sequence, in the order added
        self.num_tracks = 0
        self.sequence_names = []
        self._seq = None
        self._pending = []
        self._free_host = []
        self._state = None
        self._ws = None
        self._ws_shape = None

    # ------------------------------------------------------------------------------------------------ device state
    def _dev_state(self):
        if self._state is None:
            dev = self.device if self.device is not None else torch.device('cuda', torch.cuda.current_device())
            self.device = dev
            known = np.zeros(256, np.uint8)
            known[[int(c) for c in self.categories]] = 1
            nw = len(self.windows)
            self._state = dict(known=torch.from_numpy(known).to(dev),
                               tp=torch.zeros((nw, 256), dtype=torch.int64, device=dev), fp=torch.zeros((nw, 256), dtype=torch.int64, device=dev),
                               fn=torch.zeros((nw, 256), dtype=torch.int64, device=dev), iou=torch.zeros((nw, 256), dtype=torch.float64, device=dev),
                               status=torch.tensor([0, NO_KEY_ERROR], dtype=torch.int64, device=dev),
                               seq_out=torch.empty((int(lib().upsnet_video_eval_sequence_ints()),), dtype=torch.int32, device=dev))
        return self._state

    def workspace(self):
        """The device workspace (None before the first frame): all zero outside a sequence."""
        return self._ws

    # ------------------------------------------------------------------------------------------------ a sequence
    def begin_sequence(self, frames_segments_info, name=None):
        if self._seq is not None:
            raise ValueError("begin_sequence inside a sequence: end_sequence() first")
        rows = sequence_rows(frames_segments_info, self.max_gt_segments)
        seq = _Sequence()
        seq.index, seq.name, seq.rows, seq.shape, seq.frames = self.num_sequences, name, rows, None, 0
        crowd = np.nonzero(rows[:, 2])[0]
        table = np.concatenate([np.stack([rows[:, 0], rows[:, 1] | rows[:, 2] << 8], 1).reshape(-1), crowd]).astype(np.int32)
        seq.num_crowd = int(crowd.size)
        seq.table = table              # (uploaded with the first frame: nothing touches the device before a frame is accepted)
        self._seq = seq

    def _upload(self, t):
        if isinstance(t, np.ndarray):
            return torch.from_numpy(np.ascontiguousarray(t)).to(self.device, non_blocking=True)
        return t

    def add_frame(self, pred_2ch, gt_rgb):
        """pred_2ch: uint8 [H,W,3] tracked 2-channel map; gt_rgb: uint8 [H,W,3] GT panoptic PNG (id = R + 256 G + 65536 B)."""
        seq = self._seq
        if seq is None:
            raise ValueError("add_frame outside a sequence: begin_sequence() first")
        _check_image('pred_2ch', pred_2ch)
        _check_image('gt_rgb', gt_rgb, pred_2ch.shape)
        H, W = int(pred_2ch.shape[0]), int(pred_2ch.shape[1])
        if H * W == 0 or H * W > MAX_PIXELS:
            raise ValueError("a frame of %d x %d pixels cannot be scored: H * W must lie in 1..2^24" % (H, W))
        if seq.shape is not None and (H, W) != seq.shape:
            raise ValueError("the frame is %d x %d, the sequence's first frame was %d x %d" % ((H, W) + seq.shape))
        if (seq.frames + 1) * H * W >= MAX_SEQUENCE_PIXELS:
            raise ValueError("frame %d of %d x %d pixels: a sequence holds fewer than 2^31 pixels" % (seq.frames, H, W))
        st = self._dev_state()
        if isinstance(seq.table, np.ndarray):
            t = torch.from_numpy(seq.table).pin_memory()
            seq.table = t.to(self.device, non_blocking=True)
        pred_2ch, gt_rgb = self._upload(pred_2ch), self._upload(gt_rgb)
        if not pred_2ch.is_cuda or not gt_rgb.is_cuda:
            raise RuntimeError("VideoPanopticEvaluator: the frames must be on the device (there is no CPU fallback)")
        with torch.cuda.device(self.device):
            if self._ws is None or self._ws_shape != (H, W):     # (the old workspace is all zero by contract: nothing to carry over)
                self._ws = ops.video_eval_workspace(self.max_gt_segments, H, W, self.windows[-1], self.device)
                self._ws_shape = (H, W)
            ops.video_eval_frame(pred_2ch, gt_rgb, seq.table, seq.rows.shape[0], seq.num_crowd, self.max_gt_segments, self.windows, seq.frames,
                                 seq.index, st['known'], self._ws, st['tp'], st['fp'], st['fn'], st['iou'], st['status'])
        seq.shape = (H, W)
        seq.frames += 1

    def end_sequence(self):
        seq = self._seq
        if seq is None:
            raise ValueError("end_sequence outside a sequence")
        self._seq = None
        self.num_sequences += 1
        self.num_frames += seq.frames
        self.sequence_names.append(seq.name if seq.name is not None else str(seq.index))
        if seq.frames == 0:
            return
        st = self._state
        seq.host = self._free_host.pop() if self._free_host else torch.empty((st['seq_out'].numel(),), dtype=torch.int32, pin_memory=True)
        with torch.cuda.device(self.device):
            ops.video_eval_end(seq.shape[0], seq.shape[1], self.max_gt_segments, self.windows[-1], self._ws, st['seq_out'], seq.host)
            seq.event = torch.cuda.Event()
            seq.event.record()
        seq.table = None
        self._pending.append(seq)

    # ------------------------------------------------------------------------------------------------ results
    def _isthing(self, cat):
        return self.categories.get(cat, {}).get('isthing') == 1

    def _resolve(self, seq):
        """STQ's sums of one sequence from its integer cells, on the host, in the stated order."""
        seq.event.synchronize()
        host = seq.host.numpy().view(np.uint32)
        n = int(host[0])
        pairs = host[2:2 + 2 * n].reshape(n, 2).astype(np.int64)
        self._free_host.append(seq.host)
        seq.host = None
        cell, count = pairs[:, 0] - 1, pairs[:, 1]
        kind, index = cell >> 28, cell & ((1 << 28) - 1)
        area_p = dict(zip(index[kind == 1].tolist(), count[kind == 1].tolist()))
        void = dict(zip(index[kind == 2].tolist(), count[kind == 2].tolist()))
        area_g = dict(zip(index[kind == 3].tolist(), count[kind == 3].tolist()))
        joint = {}     # row -> {key: count}
        for i, c in zip(index[kind == 0].tolist(), count[kind == 0].tolist()):
            joint.setdefault(i >> 16, {})[i & 0xffff] = c
        rows = seq.rows
        P = {}
        for key, a in area_p.items():
            if self._isthing(key >> 8):
                P[key] = a - void.get(key, 0)
        for row, per_key in joint.items():
            cat, crowd = int(rows[row, 1]), int(rows[row, 2])
            for key, c in per_key.items():
                self.conf[cat, key >> 8] += c
                if crowd and self._isthing(cat) and key in P:
                    P[key] -= c
        for row, g in area_g.items():
            self.conf[int(rows[row, 1]), 255] += g - sum(joint.get(row, {}).values())
        aq_sum = 0.0
        for row in range(rows.shape[0]):          # ascending id
            G = area_g.get(row, 0)
            if rows[row, 2] or not self._isthing(int(rows[row, 1])) or G == 0:
                continue
            self.num_tracks += 1
            inner = 0.0
            per_key = joint.get(row, {})
            for key in sorted(per_key):
                if key in P:
                    I = per_key[key]
                    inner += I * (float(I) / float(G + P[key] - I))
            aq_sum += (1.0 / G) * inner
        self.aq_sums.append(aq_sum)

    def _sync(self):
        """One copy of the accumulators; raises what the device reported; resolves the sequences that ended."""
        nw = len(self.windows)
        if self._state is None:
            z = np.zeros((nw, 256), np.int64)
            return z, z, z, np.zeros((nw, 256), np.float64)
        st = self._state
        host = torch.cat([st['tp'].view(-1), st['fp'].view(-1), st['fn'].view(-1), st['iou'].view(torch.int64).view(-1), st['status']]).cpu().numpy()
        k = nw * 256
        full, bad = int(host[4 * k]), int(host[4 * k + 1])
        if full:
            raise RuntimeError("VideoPanopticEvaluator: " + "; ".join(text for bit, text in sorted(FULL.items()) if full & bit)
                               + ": counts were dropped, the result is void")
        if bad != NO_KEY_ERROR:
            s, f, c = bad >> 32, (bad >> 8) & 0xffffff, bad & 255
            name = self.sequence_names[s] if s < len(self.sequence_names) else (self._seq.name if self._seq is not None and self._seq.name is not None else str(s))
            raise KeyError('In sequence {} (index {} in the order added) frame {} a segment has unknown category_id {}.'.format(name, s, f, c))
        pending, self._pending = self._pending, []
        for seq in pending:
            self._resolve(seq)
        return (host[0:k].reshape(nw, 256), host[k:2 * k].reshape(nw, 256), host[2 * k:3 * k].reshape(nw, 256),
                host[3 * k:4 * k].view(np.float64).reshape(nw, 256))

    def raw(self):
        """{'tp', 'fp', 'fn': int64 [len(windows), 256], 'iou': float64 [len(windows), 256], 'conf': int64 [256, 256], 'aq_sums': [float
        per sequence], 'num_tracks'}: the counts and the raw float64 sums behind every figure. Synchronises once."""
        tp, fp, fn, iou = self._sync()
        return {'tp': tp.copy(), 'fp': fp.copy(), 'fn': fn.copy(), 'iou': iou.copy(), 'conf': self.conf.copy(), 'aq_sums': list(self.aq_sums),
                'num_tracks': self.num_tracks}

    def vpq_stat(self):
        """Synchronise once; {window length: host PQStat of every window of that length added so far}."""
        from .base_dataset import PQStat
        tp, fp, fn, iou = self._sync()
        stats = {}
        for w, n in enumerate(self.windows):
            stat = PQStat()
            for c in np.nonzero(tp[w] + fp[w] + fn[w])[0]:
                cat = stat[int(c)]
                cat.tp, cat.fp, cat.fn, cat.iou = int(tp[w, c]), int(fp[w, c]), int(fn[w, c]), float(iou[w, c])
            stats[n] = stat
        return stats

    def stq(self):
        """{'stq', 'aq', 'iou', 'num_tracks', 'per_class_iou'} of the sequences that ended. Synchronises once."""
        self._sync()
        per_class = {}
        for c in range(255):
            denom = int(self.conf[c, :].sum()) + int(self.conf[:, c].sum()) - int(self.conf[c, c])
            if denom > 0:
                per_class[c] = float(self.conf[c, c]) / float(denom)
        iou = sum(per_class.values()) / len(per_class) if per_class else 0.0
        aq = 0.0
        for s in self.aq_sums:
            aq += s
        aq = aq / max(self.num_tracks, 1)
        return {'stq': math.sqrt(aq * iou), 'aq': aq, 'iou': iou, 'num_tracks': self.num_tracks, 'per_class_iou': per_class}

    def summary(self):
        """{'vpq': {'All' | 'Things' | 'Stuff': {pq, sq, rq, n}, 'per_window': {n: pq_summary dict}}, 'stq': {...}, 'sequences',
        'frames'}; VPQ (and its SQ, RQ, per split) is the mean of the per-window figures over `windows`. Logs the tables."""
        stats = self.vpq_stat()
        per_window = {n: window_summary(stats[n], self.categories) for n in self.windows}
        vpq = {}
        for name in ('All', 'Things', 'Stuff'):
            vpq[name] = {k: sum(per_window[n][name][k] for n in self.windows) / len(self.windows) for k in ('pq', 'sq', 'rq')}
            vpq[name]['n'] = max(per_window[n][name]['n'] for n in self.windows)
        vpq['per_window'] = per_window
        stq = self.stq()
        logger.info("{:10s}| {:>5s}  {:>5s}  {:>5s} {:>5s}".format("window", "PQ", "SQ", "RQ", "N"))
        logger.info("-" * (10 + 7 * 4))
        for n in self.windows:
            r = per_window[n]['All']
            logger.info("{:<10d}| {:5.1f}  {:5.1f}  {:5.1f} {:5d}".format(n, 100 * r['pq'], 100 * r['sq'], 100 * r['rq'], r['n']))
        for name in ('All', 'Things', 'Stuff'):
            r = vpq[name]
            logger.info("VPQ {:6s}| {:5.1f}  {:5.1f}  {:5.1f} {:5d}".format(name, 100 * r['pq'], 100 * r['sq'], 100 * r['rq'], r['n']))
        logger.info("STQ {:5.1f}  AQ {:5.1f}  IoU {:5.1f}  ({:d} GT tracks, {:d} sequences, {:d} frames)".format(
            100 * stq['stq'], 100 * stq['aq'], 100 * stq['iou'], stq['num_tracks'], self.num_sequences, self.num_frames))
        return {'vpq': vpq, 'stq': stq, 'sequences': self.num_sequences, 'frames': self.num_frames}


def window_summary(pq_stat, categories):
    """pq.pq_summary's dict for one window length ({'All', 'Things', 'Stuff': {pq, sq, rq, n}, 'per_class'}) without its tables; a
    split in which no category has a tp, fp or fn (a window longer than every sequence) is all zero instead of a division by zero."""
    results = {}
    for name, isthing in (("All", None), ("Things", True), ("Stuff", False)):
        try:
            results[name], per_class = pq_stat.pq_average(categories, isthing=isthing)
        except ZeroDivisionError:
            results[name], per_class = {'pq': 0.0, 'sq': 0.0, 'rq': 0.0, 'n': 0}, {}
        if name == 'All':
            results['per_class'] = per_class
    return results
