"""The MOTS measures of tracked sequences on the device (csrc/mots_eval.hip): sMOTSA, MOTSA, MOTSP, IDS, Frag and
MT / PT / ML (Voigtlaender et al., MOTS: Multi-Object Tracking and Segmentation, CVPR 2019), and the text format the MOTS tools read.

The reference has no video metric. The rules are this project's restatement of the published definitions, stated in
include/upsnet_hip.h and restated in plain numpy in tests/mots_ref.py; they were never compared with a build of mots_tools.

    ev = MOTSEvaluator(categories)
    for frames in sequences:
        ev.begin_sequence([f['segments_info'] for f in frames])      # the sequence table: the union of the frames' GT segments
        for f in frames:
            ev.add_frame(f['pred_2ch'], f['gt_rgb'])                 # uint8 [H,W,3] device tensors (numpy arrays are uploaded)
        ev.end_sequence()
    result = ev.summary()

add_frame only queues work (one pass over the frame's pixels, the match pass, the row-state pass); nothing waits for the host between
begin_sequence and end_sequence. The figures are computed on the host from the integer counts and the float64 sums when raw / summary
synchronise. Prediction and ground truth are exactly VideoPanopticEvaluator's (dataset/video_pq.py).

    write_mots_txt(path, maps_2ch)       # one line per thing segment per frame: <frame> <category * 1000 + instance> <category> <H> <W> <rle>
    gts, infos = read_mots_txt(path)     # such a file as ground truth: per frame a gt_rgb id map and its segments_info
"""
import logging

import numpy as np
import torch

from .. import ops
from .pq import MAX_CATEGORY, _check_image
from .rle import counts_from_transitions, decode_rle_strings, rle_to_string
from .video_pq import MAX_PIXELS, MAX_SEQUENCE_PIXELS, NO_KEY_ERROR, sequence_rows

logger = logging.getLogger(__name__)

COUNTS = ('tp', 'fp', 'fn', 'gt_masks', 'ids', 'frag', 'fp_ignored')     # the rows of the device's count table
IGNORE_CLASS = 10              # KITTI MOTS: a region that is ignored for every class
MAX_ID = (1 << 24) - 1
FULL = {1: "the frame table was full (more distinct (GT segment, predicted segment) pairs in one frame than one per 16 pixels)"}


class _Sequence(object):
    __slots__ = ('index', 'name', 'rows', 'table', 'shape', 'frames')


class MOTSEvaluator(object):
    """Running MOTS statistics of tracked sequences on one device.

    categories: the dataset's category table, {id: {'isthing': 0/1, ...}} or the JSON's list of dicts with 'id'; the scored
    categories are those with isthing == 1.
    begin_sequence(frames_segments_info, name=None) builds and validates the sequence table; add_frame(pred_2ch, gt_rgb) queues one
    frame; end_sequence() queues the classing of the sequence's objects (MT / PT / ML). raw() -> the counts; summary() -> the figures.
    ValueError before any launch, the state untouched: see video_pq.sequence_rows; a frame that is not uint8 [H,W,3], of another shape
    than the sequence's first, of more than 2^24 pixels (or 2^31 in the whole sequence); add_frame / end_sequence outside a sequence,
    begin_sequence inside one. KeyError at the first synchronisation: a pred category that is not in `categories`, naming sequence,
    frame and category. RuntimeError at the first synchronisation: a full table (counts were dropped, never silently)."""

    def __init__(self, categories, max_gt_segments=4096, device=None):
        if not isinstance(categories, dict):
            categories = {el['id']: el for el in categories}
        bad = [c for c in categories if not 0 <= int(c) <= MAX_CATEGORY]
        if bad:
            raise ValueError("category ids must lie in 0..%d, got %s" % (MAX_CATEGORY, bad))
        if not 0 <= int(max_gt_segments) <= 4096:
            raise ValueError("max_gt_segments %d outside 0..4096" % max_gt_segments)
        self.categories = categories
        self.max_gt_segments = int(max_gt_segments)
        self.device = torch.device(device) if device is not None else None
        self.num_sequences = 0
        self.num_frames = 0
        self.sequence_names = []
        self._seq = None
        self._state = None
        self._ws = None
        self._ws_shape = None

    def _isthing(self, cat):
        return self.categories.get(cat, {}).get('isthing') == 1

    def _dev_state(self):
        if self._state is None:
            dev = self.device if self.device is not None else torch.device('cuda', torch.cuda.current_device())
            self.device = dev
            info = np.zeros(256, np.uint8)
            for c in self.categories:
                info[int(c)] = 1 | (2 if self._isthing(c) else 0)
            # torch.empty + zero_: what the kernels write is the allocator's own block (the tests fence exactly these five)
            status = torch.empty((2,), dtype=torch.int64, device=dev)
            status.copy_(torch.tensor([0, NO_KEY_ERROR], dtype=torch.int64))
            self._state = dict(info=torch.from_numpy(info).to(dev), counts=torch.empty((len(COUNTS), 256), dtype=torch.int64, device=dev).zero_(),
                               soft=torch.empty((256,), dtype=torch.float64, device=dev).zero_(),
                               mtl=torch.empty((3, 256), dtype=torch.int64, device=dev).zero_(), status=status)
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
        thing = np.array([self._isthing(int(c)) for c in rows[:, 1]], np.int64).reshape(-1)
        seq.table = np.stack([rows[:, 0], rows[:, 1] | rows[:, 2] << 8 | thing << 9], 1).reshape(-1).astype(np.int32)
        self._seq = seq                # (the table is uploaded with the first frame: nothing touches the device before a frame is accepted)

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
            seq.table = torch.from_numpy(seq.table).pin_memory().to(self.device, non_blocking=True)
        pred_2ch, gt_rgb = self._upload(pred_2ch), self._upload(gt_rgb)
        if not pred_2ch.is_cuda or not gt_rgb.is_cuda:
            raise RuntimeError("MOTSEvaluator: the frames must be on the device (there is no CPU fallback)")
        with torch.cuda.device(self.device):
            if self._ws is None or self._ws_shape != (H, W):     # (the old workspace is all zero by contract: nothing to carry over)
                self._ws = torch.empty((ops.mots_eval_workspace_bytes(self.max_gt_segments, H, W),), dtype=torch.uint8, device=self.device).zero_()
                self._ws_shape = (H, W)
            ops.mots_eval_frame(pred_2ch, gt_rgb, seq.table, seq.rows.shape[0], self.max_gt_segments, seq.frames, seq.index, st['info'],
                                self._ws, st['counts'], st['soft'], st['status'])
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
        with torch.cuda.device(self.device):
            ops.mots_eval_end(seq.shape[0], seq.shape[1], seq.table, seq.rows.shape[0], self.max_gt_segments, self._ws, self._state['mtl'])
        seq.table = None

    # ------------------------------------------------------------------------------------------------ results
    def raw(self):
        """{'tp', 'fp', 'fn', 'gt_masks', 'ids', 'frag', 'fp_ignored', 'mt', 'pt', 'ml': int64 [256], 'soft': float64 [256]}: the counts
        and the raw float64 sum behind every figure (mt / pt / ml of the sequences that ended). Synchronises once; raises what the device
        reported."""
        k = len(COUNTS)
        if self._state is None:
            out = {name: np.zeros(256, np.int64) for name in COUNTS + ('mt', 'pt', 'ml')}
            out['soft'] = np.zeros(256, np.float64)
            return out
        st = self._state
        host = torch.cat([st['counts'].view(-1), st['mtl'].view(-1), st['soft'].view(torch.int64), st['status']]).cpu().numpy()
        full, bad = int(host[(k + 4) * 256]), int(host[(k + 4) * 256 + 1])
        if full:
            raise RuntimeError("MOTSEvaluator: " + "; ".join(text for bit, text in sorted(FULL.items()) if full & bit)
                               + ": counts were dropped, the result is void")
        if bad != NO_KEY_ERROR:
            s, f, c = bad >> 32, (bad >> 8) & 0xffffff, bad & 255
            name = self.sequence_names[s] if s < len(self.sequence_names) else (self._seq.name if self._seq is not None and self._seq.name is not None else str(s))
            raise KeyError('In sequence {} (index {} in the order added) frame {} a segment has unknown category_id {}.'.format(name, s, f, c))
        out = {name: host[i * 256:(i + 1) * 256].copy() for i, name in enumerate(COUNTS + ('mt', 'pt', 'ml'))}
        out['soft'] = host[(k + 3) * 256:(k + 4) * 256].copy().view(np.float64)
        return out

    def summary(self):
        """{'per_class': {category: figures and counts}, 'mean': the figures averaged over the categories with gt_masks > 0 (and 'n',
        their number), 'total': the counts summed over the thing categories, 'sequences', 'frames'}. Logs the table."""
        raw = self.raw()
        per_class = {}
        for c in sorted(int(c) for c in self.categories if self._isthing(c)):
            per_class[c] = figures({k: (float(v[c]) if k == 'soft' else int(v[c])) for k, v in raw.items()})
        scored = [r for r in per_class.values() if r['gt_masks'] > 0]
        mean = {k: (sum(r[k] for r in scored) / len(scored) if scored else 0.0) for k in ('smotsa', 'motsa', 'motsp', 'recall', 'precision')}
        mean['n'] = len(scored)
        total = {k: sum(r[k] for r in per_class.values()) for k in COUNTS + ('mt', 'pt', 'ml')}
        logger.info("{:10s}| {:>6s} {:>6s} {:>6s} {:>5s} {:>5s} {:>6s} {:>6s} {:>6s} {:>4s} {:>4s} {:>4s}".format(
            "category", "sMOTSA", "MOTSA", "MOTSP", "IDS", "Frag", "TP", "FP", "FN", "MT", "PT", "ML"))
        logger.info("-" * 86)
        for c, r in per_class.items():
            logger.info("{:<10d}| {:6.1f} {:6.1f} {:6.1f} {:5d} {:5d} {:6d} {:6d} {:6d} {:4d} {:4d} {:4d}".format(
                c, 100 * r['smotsa'], 100 * r['motsa'], 100 * r['motsp'], r['ids'], r['frag'], r['tp'], r['fp'], r['fn'], r['mt'], r['pt'], r['ml']))
        logger.info("{:10s}| {:6.1f} {:6.1f} {:6.1f} {:5d} {:5d}   ({:d} categories, {:d} sequences, {:d} frames)".format(
            "mean", 100 * mean['smotsa'], 100 * mean['motsa'], 100 * mean['motsp'], total['ids'], total['frag'], mean['n'], self.num_sequences,
            self.num_frames))
        return {'per_class': per_class, 'mean': mean, 'total': total, 'sequences': self.num_sequences, 'frames': self.num_frames}


def figures(r):
    """The figures of one category from its sums (a dict with COUNTS, 'soft', 'mt', 'pt', 'ml'), added to a copy of it."""
    r = dict(r)
    gt, tp = max(r['gt_masks'], 1), r['tp']
    r['motsa'] = float(tp - r['fp'] - r['ids']) / gt
    r['smotsa'] = (r['soft'] - r['fp'] - r['ids']) / gt
    r['motsp'] = r['soft'] / max(tp, 1)
    r['recall'] = float(tp) / gt
    r['precision'] = float(tp) / max(tp + r['fp'], 1)
    return r


# ------------------------------------------------------------------------------------------------ the text format
def segment_transitions(pan_2ch, cap=4096):
    """COCO RLE of every thing segment (category != 255, instance >= 1) of one 2-channel map on the device: the sorted int64 words
    key << 24 | p, p the column-major positions at which the key's membership changes (ops.pan_rle_transitions). `cap` is the first
    size of the pair buffer; the kernel reports the full count, and the call is repeated with a buffer of that size when it was larger."""
    cap = max(int(cap), 0)
    while True:
        pairs = torch.empty((cap,), dtype=torch.int64, device=pan_2ch.device)
        count = torch.empty((1,), dtype=torch.int32, device=pan_2ch.device)
        ops.pan_rle_transitions(pan_2ch, pairs, count)
        n = int(count.item())
        if n <= cap:
            break
        cap = n
    return torch.sort(pairs[:n])[0]


def segment_lines(frame, words, H, W):
    """The lines of one frame from the sorted words key << 24 | position of its thing segments (segment_transitions)."""
    words = np.asarray(words, np.int64)
    keys, pos = words >> 24, words & ((1 << 24) - 1)
    lines = []
    for k in np.unique(keys).tolist():
        cat, inst = k >> 8, k & 255
        rle = rle_to_string(counts_from_transitions(pos[keys == k], H * W))
        lines.append('%d %d %d %d %d %s' % (frame, cat * 1000 + inst, cat, H, W, rle))
    return lines


def write_mots_txt(path, maps_2ch, device=None):
    """Write a tracked sequence in the MOTS text format: one line per thing segment (category != 255, instance >= 1) per frame,
    `<frame index> <category * 1000 + instance> <category> <H> <W> <COCO RLE string>`, the frame index being the position in maps_2ch
    (uint8 [H,W,3] device tensors or numpy arrays). The run lengths come from the device (upsnet_pan_rle_transitions). Returns the
    number of lines."""
    lines = []
    for t, m in enumerate(maps_2ch):
        _check_image('maps_2ch[%d]' % t, m)
        if isinstance(m, np.ndarray):
            m = torch.from_numpy(np.ascontiguousarray(m)).to(device if device is not None else 'cuda')
        if not m.is_cuda:
            raise RuntimeError("write_mots_txt: the maps must be on the device (there is no CPU fallback)")
        m = m.contiguous()
        with torch.cuda.device(m.device):
            words = segment_transitions(m)
        lines.extend(segment_lines(t, words.cpu().numpy(), int(m.shape[0]), int(m.shape[1])))
    with open(path, 'w') as f:
        for line in lines:
            f.write(line + '\n')
    return len(lines)


class MOTSText(object):
    """A parsed MOTS text file as ground truth: height, width, num_frames, background (the id of the background segment),
    segments_info (one list per frame, as MOTSEvaluator.begin_sequence takes them) and frame(t) -> the gt_rgb id map of frame t
    (uint8 [H,W,3]), painted when asked for: only the run lengths of the file and one frame are ever held, however long the sequence
    is. The arguments, the conventions and the refusals are read_mots_txt's; masks that overlap are refused by frame(t)."""

    def __init__(self, path, num_frames=None, background_category=0):
        entries = []
        with open(path, 'r') as f:
            for n, line in enumerate(f):
                parts = line.split()
                if not parts:
                    continue
                if len(parts) != 6:
                    raise ValueError("%s line %d: 6 fields expected, got %d" % (path, n + 1, len(parts)))
                try:
                    t, oid, cls, h, w = (int(v) for v in parts[:5])
                except ValueError:
                    raise ValueError("%s line %d: the first five fields must be integers" % (path, n + 1))
                entries.append((t, oid, cls, h, w, parts[5], n + 1))
        if not entries:
            raise ValueError("%s holds no mask: the frame size is unknown" % path)
        H, W = entries[0][3], entries[0][4]
        if H <= 0 or W <= 0:
            raise ValueError("%s line %d: bad frame size %d x %d" % (path, entries[0][6], H, W))
        for t, oid, cls, h, w, _, n in entries:
            if (h, w) != (H, W):
                raise ValueError("%s line %d: size %d x %d, the file's first mask was %d x %d" % (path, n, h, w, H, W))
            if cls != IGNORE_CLASS and not 1 <= oid <= MAX_ID:
                raise ValueError("%s line %d: object id %d outside 1..2^24-1" % (path, n, oid))
            if cls != IGNORE_CLASS and cls == int(background_category):
                raise ValueError("%s line %d: an object of class %d, which is background_category: the background must be of a category "
                                 "that is not a thing" % (path, n, cls))
            if t < 0 or (num_frames is not None and t >= num_frames):
                raise ValueError("%s line %d: frame index %d outside 0..%s" % (path, n, t, 'num_frames-1' if num_frames is not None else ''))
        self.path, self.height, self.width = path, H, W
        self.num_frames = int(num_frames) if num_frames is not None else max(e[0] for e in entries) + 1
        used = set(e[1] for e in entries if e[2] != IGNORE_CLASS)
        self.background = MAX_ID
        while self.background in used:
            self.background -= 1
        counts, off = decode_rle_strings([e[5] for e in entries])
        self._masks = [[] for _ in range(self.num_frames)]          # per frame: (id to paint, run lengths, line number)
        infos = [{} for _ in range(self.num_frames)]
        covered = [0] * self.num_frames
        for j, (t, oid, cls, _, _, _, n) in enumerate(entries):
            c = counts[off[j]:off[j + 1]]
            if np.any(c < 0) or int(c.sum()) != H * W:
                raise ValueError("%s line %d: the run lengths do not add up to %d x %d" % (path, n, H, W))
            area = int(c[1::2].sum())
            covered[t] += area
            self._masks[t].append((0 if cls == IGNORE_CLASS else oid, c, n))
            if cls == IGNORE_CLASS:
                continue
            if oid in infos[t]:
                raise ValueError("%s line %d: object id %d twice in frame %d" % (path, n, oid, t))
            infos[t][oid] = {'id': oid, 'category_id': cls, 'iscrowd': 0, 'area': area}
        self.segments_info = []
        for t in range(self.num_frames):
            info = [infos[t][k] for k in sorted(infos[t])]
            if covered[t] < H * W:         # (masks that overlap make this too small: frame(t) refuses them)
                info.append({'id': self.background, 'category_id': int(background_category), 'iscrowd': 0, 'area': H * W - covered[t]})
            self.segments_info.append(info)

    def frame(self, t):
        H, W = self.height, self.width
        ids = np.full((H * W,), self.background, np.int32)           # column-major
        covered = np.zeros((H * W,), bool)
        for paint, c, n in self._masks[t]:
            start = np.cumsum(c) - c
            s, ln = start[1::2], c[1::2]
            px = np.repeat(s - (np.cumsum(ln) - ln), ln) + np.arange(int(ln.sum()))
            if np.any(covered[px]):
                raise ValueError("%s line %d: the mask overlaps another mask of frame %d" % (self.path, n, t))
            covered[px] = True
            ids[px] = paint
        m = ids.reshape(W, H).T
        return np.ascontiguousarray(np.stack([m & 255, (m >> 8) & 255, (m >> 16) & 255], 2).astype(np.uint8))


def read_mots_txt(path, num_frames=None, background_category=0):
    """A MOTS text file as ground truth -> (gt_rgb maps, frames_segments_info), one per frame 0..num_frames-1 (default: up to the
    file's last frame), as MOTSEvaluator takes them; MOTSText gives the same frame by frame. The id of an object is the file's id; a
    mask of class 10 is painted as id 0, that is ignored for every category (KITTI's convention). The pixels no mask covers belong to
    one background segment of `background_category`, whose id is the largest of 1..2^24-1 that no object of the file has, so that a
    hypothesis on empty ground is a false positive and not exempt; background_category must not be a thing category (an object of that
    class in the file is refused; video_eval.background_category picks one from a category table).
    ValueError: a malformed line, masks that overlap in a frame, sizes that differ within the file, an id outside 1..2^24-1, run
    lengths that do not add up to H * W, a frame index outside 0..num_frames-1, an object of background_category, a file without a mask."""
    text = MOTSText(path, num_frames, background_category)
    return [text.frame(t) for t in range(text.num_frames)], text.segments_info

