"""COCO box and mask AP on the device: pycocotools' COCOeval (iouType 'bbox' / 'segm', default Params) as the reference's
evaluate_boxes / evaluate_masks run it (upsnet/dataset/base_dataset.py:181-204, coco.py:196-221), restated in csrc/det_eval.hip.

`add` queues one image: computeIoU and evaluateImg of every category on the device, one record per detection (no host
synchronisation). `accumulate` runs COCOeval.accumulate over all records on the device and synchronises once; `stats` (the 12
numbers of summarize) come from its arrays on the host. precision [T,R,K,A,M], recall [T,K,A,M] and scores [T,R,K,A,M] are
bit-identical to pycocotools' for the same inputs. Category rows K are the category ids in ascending order, as COCOeval sorts them.

Deliberate deviations, each refused with ValueError before any launch:
  * wrong shapes or dtypes, GT ids <= 0 (evaluateImg stores GT ids as match flags), a category id given twice, an image_id added
    twice, masks whose size differs from the image;
  * a bare polygon list as a GT segmentation: polygons are rasterised on the device by dataset/polygon.py (csrc/poly_raster.hip,
    frPyObjects + merge restated) and reach `add` / `add_rle` as views of its handle, `rasterize_polygons(...)[i]`; their run lists
    go to the kernels next to the RLE rows and never visit the host. Views of one call must come from one handle, each at most once.
Detections of classes with no category id are dropped, as pycocotools drops results of categories outside Params.catIds; so are
GTs of other categories. iou_type 'boundary' is the Boundary IoU API's COCOeval (Boundary AP): everything as 'segm' except computeIoU,
which takes min(mask IoU, boundary IoU) with boundary = mask_to_boundary(mask, dilation_ratio) (dataset/boundary.py) computed on the
device from the same bit planes; that API is not a dependency, its rule is restated from the published source. Scores must not be
NaN (they are device data and are not inspected). Proposal recall (evaluate_box_proposals) is dataset/proposal_eval.py, the Cityscapes
instance-level AP dataset/cityscapes_eval.py.
"""
import ctypes
import logging

import numpy as np
import torch

from .._lib import aligned, check, lib, ptr, ptr_array, stream
from .boundary import check_dilation_ratio, checked_dilation
from .polygon import PolygonView

logger = logging.getLogger(__name__)

IOU_THRS = np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True)
REC_THRS = np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True)
MAX_DETS = [1, 10, 100]
AREA_RNG = [[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]]
AREA_LBL = ['all', 'small', 'medium', 'large']
T, R, A, M = len(IOU_THRS), len(REC_THRS), len(AREA_RNG), len(MAX_DETS)


# ------------------------------------------------------------------------------------------------------------------ host helpers
def rle_from_string(s):
    """pycocotools' compressed RLE string -> counts (rleFrString of maskApi.c; the inverse of rle.rle_to_string)."""
    if isinstance(s, bytes):
        s = s.decode('ascii')
    counts = []
    p = 0
    while p < len(s):
        x, k, more = 0, 0, True
        while more:
            c = ord(s[p]) - 48
            x |= (c & 0x1f) << 5 * k
            more = bool(c & 0x20)
            p += 1
            k += 1
            if not more and (c & 0x10):
                x |= -1 << 5 * k
        if len(counts) > 2:
            x += counts[-2]
        counts.append(x)
    return counts


def rle_counts(seg):
    """An RLE dict ({'size': [h, w], 'counts': str | bytes | list}) -> (counts int64 array, (h, w)). Polygons: ValueError."""
    if isinstance(seg, (list, tuple)):
        raise ValueError("a bare polygon list is not taken as a segmentation: rasterise the image's polygon annotations with "
                         "dataset.polygon.rasterize_polygons and pass handle[i] (or convert one with dataset.polygon.polygons_to_rle)")
    if not isinstance(seg, dict) or 'counts' not in seg or 'size' not in seg:
        raise ValueError("segmentation must be an RLE dict with 'size' and 'counts', got %r" % type(seg))
    c = seg['counts']
    counts = np.asarray(rle_from_string(c) if isinstance(c, (str, bytes)) else c, np.int64).reshape(-1)
    h, w = (int(v) for v in seg['size'])
    if np.any(counts < 0) or int(counts.sum()) != h * w:
        raise ValueError("RLE counts sum to %d, not %d x %d" % (int(counts.sum()), h, w))
    return counts, (h, w)


def counts_to_transitions(counts):
    """counts (zeros, ones, zeros, ...) -> the column-major positions where the value changes (the last, = h * w, dropped)."""
    return np.cumsum(counts)[:-1].astype(np.int64)


def summarize_stats(precision, recall):
    """COCOeval.summarize (_summarizeDets): the 12 numbers and the 12 printed lines."""
    def one(ap, iou_thr=None, area='all', max_dets=100):
        a_ind = [i for i, l in enumerate(AREA_LBL) if l == area]
        m_ind = [i for i, m in enumerate(MAX_DETS) if m == max_dets]
        if ap == 1:
            s = precision
            if iou_thr is not None:
                s = s[np.where(iou_thr == IOU_THRS)[0]]
            s = s[:, :, :, a_ind, m_ind]
        else:
            s = recall
            if iou_thr is not None:
                s = s[np.where(iou_thr == IOU_THRS)[0]]
            s = s[:, :, a_ind, m_ind]
        mean_s = -1 if len(s[s > -1]) == 0 else np.mean(s[s > -1])
        i_str = ' {:<18} {} @[ IoU={:<9} | area={:>6s} | maxDets={:>3d} ] = {:0.3f}'
        iou_str = '{:0.2f}:{:0.2f}'.format(IOU_THRS[0], IOU_THRS[-1]) if iou_thr is None else '{:0.2f}'.format(iou_thr)
        line = i_str.format('Average Precision' if ap == 1 else 'Average Recall', '(AP)' if ap == 1 else '(AR)', iou_str, area,
                            max_dets, mean_s)
        return mean_s, line
    calls = [(1,), (1, .5, 'all', 100), (1, .75, 'all', 100), (1, None, 'small', 100), (1, None, 'medium', 100),
             (1, None, 'large', 100), (0, None, 'all', 1), (0, None, 'all', 10), (0, None, 'all', 100), (0, None, 'small', 100),
             (0, None, 'medium', 100), (0, None, 'large', 100)]
    stats = np.zeros((12,))
    lines = []
    for i, c in enumerate(calls):
        stats[i], line = one(*c)
        lines.append(line)
    return stats, lines


def _tensor(x, name, dims, dtypes):
    if isinstance(x, np.ndarray):
        x = torch.from_numpy(np.ascontiguousarray(x))
    if not isinstance(x, torch.Tensor):
        raise ValueError("%s must be a tensor or numpy array, got %r" % (name, type(x)))
    if x.dim() != dims or x.dtype not in dtypes:
        raise ValueError("%s must be a %d-d tensor of %s, got %s %s" % (name, dims, [str(d) for d in dtypes], tuple(x.shape), x.dtype))
    return x


class EvalResult(object):
    """What evaluate_masks returns: the reference returns the COCOeval object; `.stats` and `.eval` are what its callers read."""

    def __init__(self, res):
        self.stats = res['stats']
        self.eval = {'counts': [T, R, len(res['category_ids']), A, M], 'precision': res['precision'], 'recall': res['recall'],
                     'scores': res['scores']}
        self.category_ids = res['category_ids']


class DetectionEvaluator(object):
    """Running COCO box ('bbox'), mask ('segm') or boundary ('boundary': Boundary AP, masks as for 'segm', boundaries eroded by
    dilation_ratio x the image diagonal) evaluation of a sequence of images on one device.

    category_ids: the dataset's category id of each class in class order (class c >= 1 is category_ids[c - 1]; class 0 is the
    background). add() / add_rle() queue one image each (no synchronisation); accumulate() / summary() synchronise once.
    `a += b` merges the evaluator of another rank (same category_ids, iou_type and dilation_ratio, disjoint image ids)."""

    def __init__(self, category_ids, iou_type='bbox', device=None, dilation_ratio=0.02):
        if iou_type not in ('bbox', 'segm', 'boundary'):
            raise ValueError("iou_type must be 'bbox', 'segm' or 'boundary', got %r" % (iou_type,))
        self.boundary = iou_type == 'boundary'
        self.dilation_ratio = check_dilation_ratio(dilation_ratio) if self.boundary else None
        ids = [int(c) for c in category_ids]
        if len(ids) == 0 or len(set(ids)) != len(ids):
            raise ValueError("category_ids must be non-empty and distinct, got %s" % ids)
        self.class_category_ids = ids
        self.category_ids = sorted(ids)   # the rows (COCOeval's p.catIds = np.unique(...))
        self.row_of = {c: r for r, c in enumerate(self.category_ids)}
        self.iou_type = iou_type
        self.segm = iou_type in ('segm', 'boundary')   # what takes masks
        self.device = torch.device(device) if device is not None else None
        self.image_ids = []   # in the order added
        self._ids = set()
        self.num_images = 0
        self._n_rec = 0
        self._state = None

    # ---------------------------------------------------------------------------------------------------------- device state
    def _dev(self):
        if self.device is None or (self.device.type == 'cuda' and self.device.index is None):
            self.device = torch.device('cuda', torch.cuda.current_device())
        return self.device

    def _dev_state(self):
        if self._state is None:
            dev = self._dev()
            K = len(self.category_ids)
            lut = np.full(len(self.class_category_ids) + 1, -1, np.int32)
            for c, cat in enumerate(self.class_category_ids):
                lut[c + 1] = self.row_of[cat]
            params = np.concatenate([np.minimum(IOU_THRS, 1 - 1e-10), np.asarray(AREA_RNG, np.float64).reshape(-1)])
            self._state = dict(lut=torch.from_numpy(lut).to(dev), params=torch.from_numpy(params).to(dev),
                               rec_thrs=torch.from_numpy(REC_THRS.copy()).to(dev),
                               npig=torch.zeros(K * A, dtype=torch.int64, device=dev), rec=self._alloc_records(1024))
        return self._state

    def _alloc_records(self, cap):
        dev = self._dev()
        return dict(score=torch.empty(cap, dtype=torch.float64, device=dev), img=torch.empty(cap, dtype=torch.int32, device=dev),
                    rk=torch.empty(cap, dtype=torch.int32, device=dev), match=torch.empty(cap, dtype=torch.int64, device=dev),
                    ign=torch.empty(cap, dtype=torch.int64, device=dev))

    def _reserve(self, n):
        st = self._dev_state()
        cap = st['rec']['score'].numel()
        if self._n_rec + n > cap:
            new = self._alloc_records(max(2 * cap, self._n_rec + n))
            for k, v in st['rec'].items():
                new[k][:self._n_rec].copy_(v[:self._n_rec])
            st['rec'] = new
        return st

    def _upload(self, a, dtype):
        t = torch.from_numpy(np.ascontiguousarray(a, dtype=dtype).reshape(-1) if np.size(a) else np.zeros(1, dtype))
        if torch.cuda.is_available():
            t = t.pin_memory()
        return t.to(self._dev(), non_blocking=True)

    # ---------------------------------------------------------------------------------------------------------- validation
    def _check_image_id(self, image_id):
        image_id = int(image_id)
        if image_id in self._ids:
            raise ValueError("image_id %d added twice" % image_id)
        return image_id


    def _gt_arrays(self, gt, size):
        """GT dicts -> per-row grouped host arrays (input order inside a row); GTs of other categories dropped."""
        keep = []
        for el in gt:
            gid = int(el['id'])
            if gid <= 0:
                raise ValueError("GT id %d: ids must be > 0 (evaluateImg keeps GT ids as match flags)" % gid)
            if int(el['category_id']) in self.row_of:
                keep.append(el)
        rows = np.array([self.row_of[int(el['category_id'])] for el in keep], np.int64)
        order = np.argsort(rows, kind='stable')
        keep = [keep[i] for i in order]
        rows = rows[order]
        K = len(self.category_ids)
        row_off = np.searchsorted(rows, np.arange(K + 1), side='left').astype(np.int32)
        area = np.array([float(el['area']) for el in keep], np.float64)
        crowd = np.array([int(bool(el.get('iscrowd', 0))) for el in keep], np.int32)
        out = dict(n=len(keep), row_off=row_off, area=area, crowd=crowd, rows_with_gt=np.unique(rows).astype(np.int32))
        if not self.segm:
            box = np.array([[float(v) for v in el['bbox']] for el in keep], np.float64).reshape(-1, 4)
            out['box'] = box
            return out
        H, W = size
        trans, off, dst, u8, u8_dst, poly, poly_dst = [], [0], [], [], [], [], []
        for g, el in enumerate(keep):
            seg = el.get('segmentation')
            if isinstance(seg, PolygonView):
                if seg.size != (H, W):
                    raise ValueError("GT %d: mask size %s differs from the image %s" % (el['id'], seg.size, (H, W)))
                if poly and seg.rasters is not poly[0].rasters:
                    raise ValueError("GT %d: the polygon views of one image must come from one rasterize_polygons call" % el['id'])
                poly.append(seg)
                poly_dst.append(g)
                continue
            if isinstance(seg, (torch.Tensor, np.ndarray)):
                if seg.dtype not in (torch.uint8, np.uint8) or tuple(seg.shape) != (H, W):
                    raise ValueError("GT %d: uint8 mask of shape %s expected, got %s %s" % (el['id'], (H, W), tuple(seg.shape), seg.dtype))
                u8.append(seg)
                u8_dst.append(g)
                continue
            counts, hw = rle_counts(seg)
            if hw != (H, W):
                raise ValueError("GT %d: mask size %s differs from the image %s" % (el['id'], hw, (H, W)))
            t = counts_to_transitions(counts)
            trans.append(t)
            off.append(off[-1] + len(t))
            dst.append(g)
        out.update(trans=np.concatenate(trans) if trans else np.zeros(0, np.int64), trans_off=np.array(off, np.int64),
                   trans_dst=np.array(dst, np.int32), u8=u8, u8_dst=u8_dst, poly=poly, poly_dst=poly_dst)
        if len(set(v.index for v in poly)) != len(poly):
            raise ValueError("a polygon view is the segmentation of two GTs")
        return out

    def _poly_rows(self, views):
        """The run lists of the views (objects of one PolygonRasters) as (trans int32, trans_off int64 [len(views) + 1]) on the device.
        All objects of the handle in order: its own tensors. Otherwise the chosen lists are gathered into a buffer of the handle's
        capacity; every shape is known on the host, so nothing is synchronised."""
        h = views[0].rasters
        trans, off = h.trans.to(self.device), h.trans_off.to(self.device)
        idx = [v.index for v in views]
        if idx == list(range(len(h))):
            return trans, off
        idx = self._upload(np.asarray(idx), np.int64)
        start = off[idx]
        new_off = torch.cat([torch.zeros(1, dtype=torch.int64, device=self.device), torch.cumsum(off[idx + 1] - start, 0)])
        pos = torch.arange(trans.numel(), dtype=torch.int64, device=self.device)
        row = torch.searchsorted(new_off[1:].contiguous(), pos, right=True).clamp_(max=len(views) - 1)
        src = (start[row] + (pos - new_off[row])).clamp_(0, trans.numel() - 1)   # past the last list: any entry (never read)
        return trans[src], new_off

    # ---------------------------------------------------------------------------------------------------------- add
    def add(self, image_id, gt, det_boxes, det_scores, det_cls, det_masks=None, image_size=None):
        """One image: gt = its annotations (dicts with id > 0, category_id, iscrowd, area, bbox xywh and for 'segm' a segmentation:
        RLE dict or uint8 [H,W] mask); det_boxes [n,4] xyxy (pred_boxes[:, 1:] / im_scale), det_scores [n] (cls_probs),
        det_cls [n] 1-based classes (cls_inds); for 'segm' det_masks [n,C,M,M] mask probabilities (mask_probs, C = 1 or one channel per class) pasted by the
        im_post rule, and image_size = (H, W). Device tensors (numpy arrays are uploaded); nothing is synchronised."""
        image_id = self._check_image_id(image_id)
        boxes = _tensor(det_boxes, 'det_boxes', 2, (torch.float32, torch.float64))
        n = boxes.shape[0]
        if boxes.shape[1] != 4:
            raise ValueError("det_boxes must be [n,4], got %s" % (tuple(boxes.shape),))
        scores = _tensor(det_scores, 'det_scores', 1, (torch.float32, torch.float64))
        cls = _tensor(det_cls, 'det_cls', 1, (torch.int64, torch.int32))
        if scores.shape[0] != n or cls.shape[0] != n:
            raise ValueError("det_scores %s / det_cls %s do not match det_boxes [%d,4]" % (tuple(scores.shape), tuple(cls.shape), n))
        size, masks = self._image_size(image_size), None
        if self.segm:
            if det_masks is None:
                raise ValueError("iou_type %r needs det_masks" % self.iou_type)
            masks = _tensor(det_masks, 'det_masks', 4, (torch.float32,))
            C, M1, M2 = masks.shape[1:]
            if masks.shape[0] != n or M1 != M2 or not 2 <= M1 <= 32 or not (C == 1 or C >= len(self.class_category_ids) + 1):
                raise ValueError("det_masks must be [n,C,M,M] with n=%d, 2 <= M <= 32 and C = 1 or > %d, got %s"
                                 % (n, len(self.class_category_ids), tuple(masks.shape)))
        g = self._gt_arrays(gt, size)
        dev = self._dev()
        boxes, scores, cls = boxes.to(dev), scores.to(dev), cls.to(dev)
        self._launch(image_id, g, n, boxes.to(torch.float64).contiguous(), scores.to(torch.float64).contiguous(),
                     cls.to(torch.int64).contiguous(), size, box_f32=boxes.to(torch.float32).contiguous() if self.segm else None,
                     masks=masks.to(dev).contiguous() if masks is not None else None)

    def add_rle(self, image_id, gt, dets_xyxy_score, rles=None, image_size=None):
        """One image in the reference's all_boxes / all_segms form: dets_xyxy_score[c] = [n_c, 5] (x1, y1, x2, y2, score) of class c
        (entry 0, the background, is skipped), rles[c] = the n_c RLE dicts of im_post ('segm'). The image size comes from image_size
        or from the RLE dicts."""
        image_id = self._check_image_id(image_id)
        boxes, scores, cls, segs = [], [], [], []
        for c in range(1, len(dets_xyxy_score)):
            d = dets_xyxy_score[c]
            if isinstance(d, list) and len(d) == 0:
                continue
            d = np.asarray(d, np.float64)
            if d.ndim != 2 or d.shape[1] != 5:
                raise ValueError("dets_xyxy_score[%d] must be [n,5], got %s" % (c, d.shape))
            boxes.append(d[:, :4])
            scores.append(d[:, 4])
            cls.append(np.full(len(d), c, np.int64))
            if self.segm:
                if rles is None or c >= len(rles) or len(rles[c]) != len(d):
                    raise ValueError("rles[%d] must hold one RLE per detection" % c)
                segs.extend(rles[c])
        boxes = np.concatenate(boxes) if boxes else np.zeros((0, 4))
        scores = np.concatenate(scores) if scores else np.zeros(0)
        cls = np.concatenate(cls) if cls else np.zeros(0, np.int64)
        n = len(scores)
        if np.any(np.isnan(scores)):
            raise ValueError("NaN detection score")
        size = image_size
        if self.segm and size is None:
            sizes = [tuple(int(v) for v in s['size']) for s in segs if isinstance(s, dict) and 'size' in s]
            sizes += [tuple(int(v) for v in el['segmentation']['size']) for el in gt if isinstance(el.get('segmentation'), dict)]
            size = sizes[0] if sizes else (1, 1)
        size = self._image_size(size)
        trans = off = None
        if self.segm:
            ts, o = [], [0]
            for s in segs:
                counts, hw = rle_counts(s)
                if hw != size:
                    raise ValueError("detection mask size %s differs from the image %s" % (hw, size))
                t = counts_to_transitions(counts)
                ts.append(t)
                o.append(o[-1] + len(t))
            trans, off = (np.concatenate(ts) if ts else np.zeros(0, np.int64)), np.array(o, np.int64)
        g = self._gt_arrays(gt, size)
        self._launch(image_id, g, n, self._upload(boxes, np.float64), self._upload(scores, np.float64), self._upload(cls, np.int64),
                     size, trans=trans, trans_off=off)

    def _image_size(self, size):
        if not self.segm:
            return (1, 1) if size is None else tuple(int(v) for v in size)
        if size is None or len(size) != 2:
            raise ValueError("iou_type %r needs image_size = (H, W)" % self.iou_type)
        H, W = (int(v) for v in size)
        if H < 1 or W < 1 or H * W >= 1 << 31:
            raise ValueError("image size %dx%d out of range" % (H, W))
        return (H, W)

    def _launch(self, image_id, g, n, xyxy, score, cls, size, box_f32=None, masks=None, trans=None, trans_off=None):
        # the launches go to the current stream of the evaluator's device, whichever device is current for the caller
        with torch.cuda.device(self._dev()):
            self._launch_on_device(image_id, g, n, xyxy, score, cls, size, box_f32, masks, trans, trans_off)

    def _launch_on_device(self, image_id, g, n, xyxy, score, cls, size, box_f32, masks, trans, trans_off):
        H, W = size
        K = len(self.category_ids)
        dilation = checked_dilation(H, W, self.dilation_ratio) if self.boundary else 0
        st = self._reserve(n)
        if self.boundary:
            nbytes = int(lib().upsnet_det_eval_boundary_image_workspace_bytes(n, K, g['n'], H, W))
        else:
            nbytes = int(lib().upsnet_det_eval_image_workspace_bytes(n, K, g['n'], H, W, int(self.segm)))
        ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=self.device)
        up = self._upload
        gt_row_off, gt_area, gt_crowd = up(g['row_off'], np.int32), up(g['area'], np.float64), up(g['crowd'], np.int32)
        rows = up(g['rows_with_gt'], np.int32)
        gt_box = up(g['box'], np.float64) if not self.segm else None
        keep = [xyxy, score, cls, box_f32, masks, gt_row_off, gt_area, gt_crowd, rows, gt_box, ws]
        det_trans = det_off = gt_trans = gt_off = gt_dst = None
        u8_ptrs = u8_dst = None
        n_u8 = n_rle = 0
        C = Ms = 0
        if self.segm:
            if trans is not None:
                det_trans, det_off = up(trans, np.int32), up(trans_off, np.int64)
            else:
                C, Ms = masks.shape[1], masks.shape[3]
            gt_trans, gt_off = up(g['trans'], np.int32), up(g['trans_off'], np.int64)
            dst = g['trans_dst']
            if g['poly']:   # the device run lists of the polygon GTs follow the host RLE rows; gt_trans_dst maps each row to its GT
                p_trans, p_off = self._poly_rows(g['poly'])
                gt_trans = torch.cat([gt_trans[:len(g['trans'])], p_trans])
                gt_off = torch.cat([gt_off[:len(dst)], p_off + len(g['trans'])])
                dst = np.concatenate([dst, np.asarray(g['poly_dst'], np.int32)])
            gt_dst = up(dst, np.int32)
            n_rle = len(dst)
            u8 = [torch.as_tensor(m).to(self.device).contiguous() for m in g['u8']]
            n_u8 = len(u8)
            if n_u8:
                u8_ptrs = ptr_array(u8)
                u8_dst = (ctypes.c_int * n_u8)(*g['u8_dst'])
            keep += [det_trans, det_off, gt_trans, gt_off, gt_dst] + u8
        rec = st['rec']
        o = self._n_rec
        u8_p = u8_ptrs if n_u8 else None          # (host arrays: of the planes' device addresses, of their rows)
        u8_d = u8_dst if n_u8 else None
        # the image's records land behind those of the images before it, so their start is element-aligned only: a part that starts
        # off 16 bytes is written into an aligned buffer of its own and copied into place (rows past n are not touched by the launch)
        names = ('score', 'img', 'rk', 'match', 'ign')
        dst = [rec[k][o:o + n] if n else rec[k] for k in names]
        land = [aligned(d) for d in dst]
        keep += land
        recs = tuple(ptr(t) for t in land) + (ptr(st['npig']),)
        if self.boundary:
            check(lib().upsnet_det_eval_boundary_image(
                stream(), dilation, H, W, K, n, ptr(score), ptr(cls), ptr(st['lut']), st['lut'].numel(), ptr(box_f32), ptr(masks), C, Ms,
                ptr(det_trans), ptr(det_off), g['n'], ptr(gt_row_off), ptr(gt_area), ptr(gt_crowd), ptr(gt_trans), ptr(gt_off), ptr(gt_dst),
                n_rle, u8_p, u8_d, n_u8, ptr(rows), len(g['rows_with_gt']), ptr(st['params']), self.num_images, ptr(ws), *recs),
                "det_eval_boundary_image")
        else:
            check(lib().upsnet_det_eval_image(
                stream(), int(self.segm), H, W, K, n, ptr(xyxy) if not self.segm else None, ptr(score), ptr(cls), ptr(st['lut']),
                st['lut'].numel(), ptr(box_f32), ptr(masks), C, Ms, ptr(det_trans), ptr(det_off), g['n'], ptr(gt_row_off), ptr(gt_box),
                ptr(gt_area), ptr(gt_crowd), ptr(gt_trans), ptr(gt_off), ptr(gt_dst), n_rle, u8_p, u8_d, n_u8, ptr(rows),
                len(g['rows_with_gt']), ptr(st['params']), self.num_images, ptr(ws), *recs), "det_eval_image")
        for d, t in zip(dst, land):
            if t is not d:
                d.copy_(t)
        del keep, land   # the caching allocator orders the reuse of these blocks after the queued launches
        self._n_rec += n
        self.image_ids.append(image_id)
        self._ids.add(image_id)
        self.num_images += 1

    # ---------------------------------------------------------------------------------------------------------- merge / results
    def __iadd__(self, other):
        if other.class_category_ids != self.class_category_ids or other.iou_type != self.iou_type:
            raise ValueError("cannot merge evaluators of different category_ids / iou_type")
        if other.dilation_ratio != self.dilation_ratio:
            raise ValueError("cannot merge boundary evaluators of different dilation_ratio (%r, %r)" % (self.dilation_ratio, other.dilation_ratio))
        dup = self._ids & other._ids
        if dup:
            raise ValueError("image_ids %s added to both evaluators" % sorted(dup)[:8])
        if other._state is not None:
            st = self._reserve(other._n_rec)
            o, n = self._n_rec, other._n_rec
            for k, v in other._state['rec'].items():
                v = v[:n].to(self.device)
                st['rec'][k][o:o + n].copy_(v + self.num_images if k == 'img' else v)
            st['npig'] += other._state['npig'].to(self.device)
            self._n_rec += n
        self.image_ids += other.image_ids
        self._ids |= other._ids
        self.num_images += other.num_images
        return self

    def accumulate(self):
        """COCOeval.accumulate() + summarize(): {'precision', 'recall', 'scores', 'stats', 'category_ids'} (numpy, float64)."""
        st = self._dev_state()
        K, N = len(self.category_ids), self._n_rec
        img_ord = np.empty(self.num_images, np.int32)
        img_ord[np.argsort(np.asarray(self.image_ids, np.int64), kind='stable')] = np.arange(self.num_images, dtype=np.int32)
        img_ord = self._upload(img_ord, np.int32)
        ws = torch.empty(max(int(lib().upsnet_det_eval_accumulate_workspace_bytes(N, K)), 1), dtype=torch.uint8, device=self.device)
        precision = torch.empty((T, R, K, A, M), dtype=torch.float64, device=self.device)
        recall = torch.empty((T, K, A, M), dtype=torch.float64, device=self.device)
        scores = torch.empty((T, R, K, A, M), dtype=torch.float64, device=self.device)
        rec = st['rec']
        with torch.cuda.device(self.device):
            check(lib().upsnet_det_eval_accumulate(stream(), N, ptr(rec['score']), ptr(rec['img']), ptr(rec['rk']), ptr(rec['match']),
                                                   ptr(rec['ign']), ptr(img_ord), K, ptr(st['npig']), ptr(st['rec_thrs']), ptr(ws),
                                                   ptr(precision), ptr(recall), ptr(scores)), "det_eval_accumulate")
        host = torch.cat([precision.reshape(-1), recall.reshape(-1), scores.reshape(-1)]).cpu().numpy()
        np_ = precision.numel()
        res = dict(precision=host[:np_].reshape(T, R, K, A, M), recall=host[np_:np_ + recall.numel()].reshape(T, K, A, M),
                   scores=host[np_ + recall.numel():].reshape(T, R, K, A, M), category_ids=list(self.category_ids))
        res['stats'], res['summary_lines'] = summarize_stats(res['precision'], res['recall'])
        return res

    def summary(self, res=None):
        """The text log_detection_eval_metrics logs (per-category AP at IoU [0.50,0.95] and [0.50,0.50], then the summary lines);
        logged and returned."""
        res = res if res is not None else self.accumulate()
        lines = detection_metrics_lines(res)
        for line in lines:
            logger.info(line)
        return '\n'.join(lines)


def detection_metrics_lines(res):
    """log_detection_eval_metrics (base_dataset.py:674-720) as text lines."""
    def thr_ind(thr):   # the IoU threshold nearest to thr; it must be one of them (within 1e-5)
        i = int(np.argmin(np.abs(IOU_THRS - thr)))
        if abs(IOU_THRS[i] - thr) >= 1e-5:
            raise ValueError("IoU threshold %g is not evaluated" % thr)
        return i

    def mean(p):
        p = p[p > -1]
        return float('nan') if p.size == 0 else np.mean(p)
    lines = []
    for hi in [0.95, 0.5]:
        lo_i, hi_i = thr_ind(0.5), thr_ind(hi)
        lines.append('~~~~ Mean and per-category AP @ IoU=[{:.2f},{:.2f}] ~~~~'.format(0.5, hi))
        for k in range(len(res['category_ids'])):
            lines.append('{:.3f}'.format(mean(res['precision'][lo_i:hi_i + 1, :, k, 0, 2])))
        lines.append('{:.3f}'.format(mean(res['precision'][lo_i:hi_i + 1, :, :, 0, 2])))
    lines.append('~~~~ Summary metrics ~~~~')
    return lines + list(res['summary_lines'])
