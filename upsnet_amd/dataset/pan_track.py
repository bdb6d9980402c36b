"""Panoptic instances tracked across the frames of a sequence, on the device (csrc/pan_track.hip).

The instance numbers of get_unified_pan_result / get_combined_pan_result are per image and follow the detection scores. The tracker
renumbers the thing segments of each frame so that an object keeps its (category, instance) pair from frame to frame: a mask-IoU
association of the frame's segments with a per-pixel memory of where every track was last seen. The reference has no tracking; the
rule is this project's own, stated in include/upsnet_hip.h and restated in plain numpy in tests/pan_track_ref.py.

    tracker = PanopticTracker(iou_thresh=0.3, max_age=0)
    for pan_2ch in frames:                      # uint8 [H,W,3] device tensors (numpy arrays are uploaded)
        tracked, segments = tracker.update(pan_2ch)

`tracked` is a device tensor at once; no step waits for the host. `segments` is a sequence of dicts, one per thing segment of the
frame in ascending (category, instance_in): category, instance_in, instance (the 8-bit id written to channel 1), track_id (the
serial), matched, iou (I / U as a float, for people only), area. It is read from the step's row table, which travels to pinned
memory by an asynchronous copy: the sequence resolves when it is first looked at, or at the end of the next update, whichever comes
first, so a loop that never looks at it never waits for more than the frame before.

Motion prediction (opt-in): PanopticTracker(..., motion='constant_velocity') keeps a centroid and a velocity per
track and associates each frame with the memory shifted by velocity x age instead of the memory in place, so that an object that
accelerates, reappears after an occlusion or passes another one keeps its identity. It is for persistent motion (sparsely sampled
video of moving objects); on erratic motion, a random walk for instance, it matches fewer segments than the default. The rule is
restated in tests/pan_track_motion_ref.py. predicted() and motion_state() show what the last step predicted and what it keeps.

The 8-bit id is what fits channel 1 and the existing writers; it is recycled after 255 issues per category. The serial counts from 1
over the tracker's life and is never reused: it is the identity consumers should use.
"""
from collections.abc import Sequence

import numpy as np
import torch

from .. import ops
from .._lib import lib
from .pq import _check_image

MAX_PIXELS = 1 << 24
HEAD, ROW = 8, 8              # ints before the first row / per row of the step's table (include/upsnet_hip.h)
FAST_ROWS = 1024              # rows that travel with the step's one device-to-host copy; a frame of more costs a second copy
MOTIONS = ('none', 'constant_velocity')


def check_params(iou_thresh, max_age, motion='none'):
    """ValueError unless 1/16 <= iou_thresh <= 1, max_age is an integer >= 0 and motion is one of MOTIONS. The lower bound: memory tracks are disjoint, so a
    segment has at most 1 / iou_thresh candidates, which bounds the kernel's LDS candidate list at 16 per segment, 4080 per category."""
    if not (1.0 / 16.0 <= float(iou_thresh) <= 1.0):      # (NaN fails too)
        raise ValueError("iou_thresh must lie in [1/16, 1], got %r" % (iou_thresh,))
    if int(max_age) != max_age or max_age < 0:
        raise ValueError("max_age must be an integer >= 0, got %r" % (max_age,))
    if motion not in MOTIONS:
        raise ValueError("motion must be one of %s, got %r" % (', '.join(MOTIONS), motion))


class TrackSegments(Sequence):
    """The segments of one tracked frame: a read-only sequence of dicts that waits for the frame's row table when first looked at."""

    def __init__(self, tracker, step):
        self._tracker, self._step, self._items = tracker, step, None

    def _resolve(self):
        if self._items is None:
            self._tracker._resolve(self._step)
        return self._items

    def __len__(self):
        return len(self._resolve())

    def __getitem__(self, i):
        return self._resolve()[i]

    def __eq__(self, other):
        return list(self) == list(other)

    def __repr__(self):
        return repr(self._resolve())

    @property
    def rows(self):
        """The frame's device rows, int32 [n, 8]: category, instance_in, instance, matched, I, U, area, taken over."""
        self._resolve()
        return self._rows


class _Step(object):
    __slots__ = ('frame', 'host', 'event', 'segments')


class PanopticTracker(object):
    """One sequence's tracker on one device. The frame size is fixed by the first update() (or after reset()).

    update(pan_2ch) -> (tracked uint8 [H,W,3] device tensor, TrackSegments); three launches and one asynchronous copy, nothing waits.
    motion='constant_velocity' (default 'none': the same launches as ever) predicts where every track is before it associates, for
    objects in persistent motion (seven launches and the copy). Then predicted() -> int32 [H,W] numpy array, the key of the track the
    last step predicted at a pixel and -1 for none, and motion_state() -> {(category, instance): (cx, cy, vx, vy)} for the tracks state()
    shows: the floor centroid of the pixels last assigned and the velocity in pixels per frame.
    reset() forgets every track, the frame size and the frame counter; the serials go on counting unless reset(serials=True).
    state() -> (key int32 [H,W], frame int32 [H,W]) numpy arrays: key = category << 8 | instance of the track a pixel remembers and -1
    for none; frame = the index of the frame that last wrote the pixel and -1 for none.
    ValueError, raised before any launch and leaving the state untouched: a frame that is not uint8 [H,W,3], of another size than the
    tracker's, or of more than 2^24 pixels."""

    def __init__(self, iou_thresh=0.3, max_age=0, device=None, motion='none'):
        check_params(iou_thresh, max_age, motion)
        self.iou_thresh = float(iou_thresh)
        self.max_age = int(max_age)
        self.motion = motion
        self._mws = None
        self.device = torch.device(device) if device is not None else None
        self.next_serial = 1
        self._ws = None
        self._ws_shape = None
        self.reset()

    def reset(self, serials=False):
        self._flush()
        self.shape = None
        self.frame_index = 0
        self._serial_of = {}          # (category, instance) -> serial of the track that holds the id now
        self._pending = None
        if serials:
            self.next_serial = 1

    def _flush(self):
        if getattr(self, '_pending', None) is not None:
            self._resolve(self._pending)

    def _start(self, H, W, dev):
        """Memory, workspace and the two pinned tables of a sequence of H x W frames (kept across reset() for the same size)."""
        if self._ws is None or self._ws_shape != (H, W) or self._ws.device != dev:
            self._ws = torch.empty((int(lib().upsnet_pan_track_workspace_bytes(H, W)),), dtype=torch.uint8, device=dev).zero_()
            self._ws_shape = (H, W)
            self._stamp_off = int(lib().upsnet_pan_track_stamp_offset())
            self._table_ints = int(lib().upsnet_pan_track_table_ints(H, W))
            self._table_off = int(lib().upsnet_pan_track_table_offset())
            n = min(self._table_ints, HEAD + ROW * FAST_ROWS)
            self._tables = [torch.empty((n,), dtype=torch.int32, pin_memory=True) for _ in range(2)]
            self._mem = torch.empty((H, W), dtype=torch.int16, device=dev).zero_()
            if self.motion != 'none':
                self._mws = torch.empty((int(lib().upsnet_pan_track_motion_workspace_bytes(H, W)),), dtype=torch.uint8, device=dev).zero_()
                self._pred_off = int(lib().upsnet_pan_track_motion_pred_offset())
        else:
            self._ws[self._stamp_off:].zero_()       # stamps, cursors, scratch (the count cells are zero after every step)
            self._mem.zero_()
            if self._mws is not None:
                self._mws.zero_()                    # centroids, velocities, the predicted memory
        self.device = dev
        self.shape = (H, W)

    def update(self, pan_2ch):
        _check_image('pan_2ch', pan_2ch)
        H, W = int(pan_2ch.shape[0]), int(pan_2ch.shape[1])
        if H * W == 0 or H * W > MAX_PIXELS:
            raise ValueError("a frame of %d x %d pixels cannot be tracked: H * W must lie in 1..2^24" % (H, W))
        if self.shape is not None and (H, W) != self.shape:
            raise ValueError("the frame is %d x %d, the tracker's frames are %d x %d (reset() starts a new sequence)" % ((H, W) + self.shape))
        if isinstance(pan_2ch, np.ndarray):
            dev = self.device if self.device is not None else torch.device('cuda', torch.cuda.current_device())
            pan_2ch = torch.from_numpy(np.ascontiguousarray(pan_2ch)).to(dev, non_blocking=True)
        if not pan_2ch.is_cuda:
            raise RuntimeError("PanopticTracker: the frame must be on the device (there is no CPU fallback)")
        if self.shape is None:
            self._start(H, W, pan_2ch.device)
        elif pan_2ch.device != self.device:
            raise ValueError("the frame is on %s, the tracker on %s" % (pan_2ch.device, self.device))
        step = _Step()
        step.frame = self.frame_index
        step.host = self._tables[step.frame & 1]
        with torch.cuda.device(self.device):
            out = torch.empty((H, W, 3), dtype=torch.uint8, device=self.device)
            if self._mws is None:
                ops.pan_track_step(pan_2ch.contiguous(), self.iou_thresh, self.max_age, step.frame, self._ws, self._mem, out, step.host)
            else:
                ops.pan_track_step_motion(pan_2ch.contiguous(), self.iou_thresh, self.max_age, step.frame, self._ws, self._mem, out,
                                          self._mws, step.host)
            step.event = torch.cuda.Event()
            step.event.record()
        step.segments = TrackSegments(self, step)
        self.frame_index += 1
        previous, self._pending = self._pending, step
        if previous is not None:
            self._resolve(previous)         # table t - 1, while step t runs; its pinned buffer is step t + 1's
        return out, step.segments

    def _resolve(self, step):
        """Read a step's table (steps resolve in order: the serials follow the frames)."""
        if step.segments._items is not None:
            return
        step.event.synchronize()
        host = step.host.numpy()
        n = int(host[0])
        if HEAD + ROW * n <= host.size:
            rows = host[HEAD:HEAD + ROW * n].reshape(n, ROW).copy()
        else:   # (beyond the rows that travelled with the step: the device table of frame t outlives step t + 1)
            first = self._table_off + 4 * ((step.frame & 1) * self._table_ints + HEAD)
            rows = self._ws[first:first + 4 * ROW * n].view(torch.int32).cpu().numpy().reshape(n, ROW)
        items = []
        for c, i, tid, matched, inter, union, area, _ in rows.tolist():
            if matched:
                serial = self._serial_of[(c, tid)]
            else:
                serial = self.next_serial
                self.next_serial += 1
                self._serial_of[(c, tid)] = serial
            items.append({'category': c, 'instance_in': i, 'instance': tid, 'track_id': serial, 'matched': bool(matched),
                          'iou': float(inter) / float(union), 'area': area})
        step.segments._rows = rows
        step.segments._items = items
        if self._pending is step:
            self._pending = None

    def state(self):
        if self.shape is None:
            raise RuntimeError("PanopticTracker.state(): no frame yet")
        key = self._mem.to(torch.int32) & 0xffff
        stamp = self._ws[self._stamp_off:self._stamp_off + 4 * 65536].view(torch.int32)
        frame = stamp[key.reshape(-1).long()].reshape(key.shape) - 1      # (all memory pixels of a track share its last frame)
        none = key == 0
        return key.masked_fill(none, -1).cpu().numpy(), frame.masked_fill(none, -1).cpu().numpy()


    def _motion_on(self, what):
        if self.motion == 'none':
            raise RuntimeError("PanopticTracker.%s(): the tracker was built with motion='none'" % what)
        if self.shape is None or self.frame_index == 0:
            raise RuntimeError("PanopticTracker.%s(): no frame yet" % what)

    def predicted(self):
        self._motion_on('predicted')
        H, W = self.shape
        prio = self._mws[self._pred_off:self._pred_off + 4 * H * W].view(torch.int32).reshape(H, W)
        return (0xffff - (prio & 0xffff)).masked_fill(prio == 0, -1).cpu().numpy()

    def motion_state(self):
        self._motion_on('motion_state')
        keys = torch.unique(self._mem.to(torch.int32) & 0xffff)
        keys = keys[keys != 0]
        rows = self._mws[:16 * 65536].view(torch.int32).reshape(65536, 4)[keys.long()].cpu().tolist()
        return {(k >> 8, k & 255): tuple(r) for k, r in zip(keys.cpu().tolist(), rows)}


def track_sequence(pans, **kw):
    """Track a whole list of 2-channel maps with a fresh PanopticTracker(**kw): -> [(tracked map, segments)] per frame."""
    tracker = PanopticTracker(**kw)
    return [tracker.update(p) for p in pans]
