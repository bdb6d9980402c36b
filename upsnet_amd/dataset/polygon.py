"""Polygon ground truth -> run-length masks on the device (csrc/poly_raster.hip): what pycocotools' COCO.annToRLE yields for a polygon
annotation (frPyObjects of the polygon list, then merge = union), restated from the published algorithm of maskApi.c's rleFrPoly. It
is pinned by hand-derived cases and a literal CPU restatement (tests/polygon_ref.py), never by a pycocotools build.

`rasterize_polygons` queues all polygon objects of one image in one call and returns a PolygonRasters handle holding the device run
lists in the form upsnet_det_eval_image takes for GT; `handle[i]` is the view a GT dict carries as its 'segmentation' into
DetectionEvaluator.add / add_rle (dataset/coco_eval.py). Nothing is synchronised. `polygons_to_rle` converts one object and
synchronises (for users and tests).

Deliberate deviations, each a ValueError before any launch:
  * a polygon with an odd number of coordinates (the original drops the last one silently);
  * a non-finite coordinate, or one with |5 * coordinate| >= 2^30 (the original's int cast overflows there);
  * a call whose edge walks hold more than MAX_POINTS points in all (an edge from (X0, Y0) to (X1, Y1) in the 5x upsampled integer
    grid holds max(|X1 - X0|, |Y1 - Y0|) + 1 of them; the workspace is sized from that count).
Polygons of 0, 1 or 2 vertices are accepted as the algorithm defines them (they emit nothing, or positions that cancel).
"""
import ctypes

import numpy as np
import torch

from .._lib import check, lib, ptr, stream

MAX_POINTS = 1 << 24   # PR_MAX_POINTS of csrc/poly_raster.hip


class PolygonView(object):
    """Object `index` of a PolygonRasters handle: a GT 'segmentation' for DetectionEvaluator."""

    def __init__(self, rasters, index):
        self.rasters = rasters
        self.index = index

    @property
    def size(self):
        return (self.rasters.height, self.rasters.width)


class PolygonRasters(object):
    """Device run lists of the objects of one rasterize_polygons call: trans int32 [capacity] (object i's ascending column-major
    change positions at trans[trans_off[i] : trans_off[i + 1]], the first starting a run of ones; the tail beyond trans_off[-1] is
    unspecified) and trans_off int64 [num_objects + 1]."""

    def __init__(self, trans, trans_off, height, width):
        self.trans = trans
        self.trans_off = trans_off
        self.height = height
        self.width = width

    def __len__(self):
        return self.trans_off.numel() - 1

    def __getitem__(self, index):
        index = int(index)
        if not 0 <= index < len(self):
            raise IndexError("object %d of %d" % (index, len(self)))
        return PolygonView(self, index)

    def transitions(self):
        """Host copies: per object the int array of change positions. Synchronises."""
        off = self.trans_off.cpu().numpy()
        trans = self.trans[:int(off[-1])].cpu().numpy()
        return [trans[off[i]:off[i + 1]] for i in range(len(self))]


def pack_polygons(objects):
    """objects (per annotation a list of flat [x0, y0, x1, y1, ...] polygons) -> (vertices float64 [total, 2], poly_off int32,
    obj_off int32, total edge-walk points); the refusals of the module docstring."""
    polys, obj_off = [], [0]
    for o, obj in enumerate(objects):
        if not isinstance(obj, (list, tuple)):
            raise ValueError("object %d: a list of polygons expected, got %r" % (o, type(obj)))
        for p in obj:
            if np.ndim(p) != 1:
                raise ValueError("object %d: a list of polygons (flat coordinate lists) expected" % o)
            a = np.asarray(p, np.float64)
            if a.size % 2:
                raise ValueError("object %d: a polygon with an odd number of coordinates (%d)" % (o, a.size))
            polys.append(a)
        obj_off.append(len(polys))
    poly_off = np.zeros(len(polys) + 1, np.int64)
    np.cumsum(np.asarray([a.size // 2 for a in polys], np.int64), out=poly_off[1:])
    verts = np.concatenate(polys).reshape(-1, 2) if polys else np.zeros((0, 2), np.float64)
    if not np.all(np.isfinite(verts)):
        raise ValueError("non-finite polygon coordinate")
    if verts.size and np.abs(5 * verts).max() >= 2.0 ** 30:
        raise ValueError("polygon coordinate out of range: |5 * c| must be < 2^30")
    total = 0
    if len(verts):
        grid = np.trunc(5 * verts + .5).astype(np.int64)   # the C cast: truncation toward zero
        nxt = np.arange(1, len(verts) + 1)
        last = poly_off[1:][poly_off[1:] > poly_off[:-1]] - 1
        nxt[last] = poly_off[:-1][poly_off[1:] > poly_off[:-1]]
        total = int((np.abs(grid[nxt] - grid).max(axis=1) + 1).sum())
    if total > MAX_POINTS or poly_off[-1] >= 1 << 31:
        raise ValueError("%d edge-walk points in one call (at most %d): rasterise the image's objects in several calls" % (total, MAX_POINTS))
    return verts, poly_off.astype(np.int32), np.asarray(obj_off, np.int32), total


def _upload(a, dev):
    t = torch.from_numpy(np.ascontiguousarray(a).reshape(-1) if a.size else np.zeros(1, a.dtype))
    if torch.cuda.is_available():
        t = t.pin_memory()
    return t.to(dev, non_blocking=True)


def rasterize_polygons(objects, height, width, device=None):
    """All polygon objects of one image -> PolygonRasters on `device` (default: the current device), one entry per object in order.
    objects: a list with one entry per annotation, each a list of flat [x0, y0, x1, y1, ...] polygons (the JSON's 'segmentation'
    value); an object's mask is the union of its polygons. Launches on the current stream of the device; no synchronisation."""
    height, width = int(height), int(width)
    if height < 1 or width < 1 or height * width >= 1 << 31:
        raise ValueError("image size %dx%d out of range" % (height, width))
    verts, poly_off, obj_off, total = pack_polygons(objects)
    dev = torch.device(device) if device is not None else torch.device('cuda', torch.cuda.current_device())
    if dev.type == 'cuda' and dev.index is None:
        dev = torch.device('cuda', torch.cuda.current_device())
    n_obj, n_poly = len(obj_off) - 1, len(poly_off) - 1
    with torch.cuda.device(dev):
        nbytes = int(lib().upsnet_poly_raster_workspace_bytes(len(verts), total))
        ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
        trans = torch.empty(max(total, 1), dtype=torch.int32, device=dev)
        trans_off = torch.empty(n_obj + 1, dtype=torch.int64, device=dev)
        v_dev, p_dev, o_dev = _upload(verts, dev), _upload(poly_off, dev), _upload(obj_off, dev)
        check(lib().upsnet_poly_raster(stream(), ptr(v_dev), poly_off.ctypes.data_as(ctypes.c_void_p), obj_off.ctypes.data_as(ctypes.c_void_p),
                                       ptr(p_dev), ptr(o_dev), n_poly, n_obj, total, height, width, ptr(ws), ptr(trans), ptr(trans_off)),
              "poly_raster")
        del ws, v_dev, p_dev, o_dev   # the caching allocator orders the reuse of these blocks after the queued launches
    return PolygonRasters(trans, trans_off, height, width)


def polygons_to_rle(polygons, height, width):
    """One object (a list of flat polygons) -> {'size': [h, w], 'counts': [...]}: uncompressed counts, zeros first
    (rle.rle_to_string gives the compressed string). Synchronises."""
    t = rasterize_polygons([polygons], height, width).transitions()[0]
    edges = np.concatenate([[0], t.astype(np.int64), [int(height) * int(width)]])
    return {'size': [int(height), int(width)], 'counts': [int(c) for c in np.diff(edges)]}
