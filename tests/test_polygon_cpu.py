"""CPU: the literal restatement of pycocotools' polygon rasteriser (tests/polygon_ref.py) on hand-derived cases, the odd-multiplicity
rule the kernel uses against the literal fold, the host-side refusals of dataset/polygon.py and the binding of the entry point."""
import ctypes

import numpy as np
import pytest

import polygon_cases as C
import polygon_ref as R


# ------------------------------------------------------------------------------------------------------------------ hand-derived
def test_rectangle_and_triangle_by_hand():
    h, w = C.H0, C.W0
    assert R.polygon_counts(C.RECT, h, w) == C.RECT_COUNTS                      # columns 2..5, rows 1..3
    assert np.array_equal(R.polygon_mask(C.RECT, h, w), C.rect_mask(2, 1, 6, 4, h, w))
    assert np.array_equal(R.polygon_mask(C.TRIANGLE, h, w), C.TRIANGLE_MASK)


@pytest.mark.parametrize('rect', C.BORDER_RECTS)
def test_integer_rectangles_at_the_borders(rect):
    """[x0, x1] x [y0, y1] covers columns x0 .. x1 - 1 and rows y0 .. y1 - 1, clipped; whatever the first vertex and the direction, and
    with a vertex repeated."""
    h, w = C.H0, C.W0
    want = C.rect_mask(*rect, h, w)
    base = C.rect_poly(*rect)
    for poly in C.rotations_and_reversal(base) + [C.repeat_vertex(base, j) for j in range(4)]:
        counts = R.polygon_counts(poly, h, w)
        assert sum(counts) == h * w
        assert np.array_equal(R.counts_to_mask(counts, h, w), want), poly


def test_triangle_order_and_repeats():
    for poly in C.rotations_and_reversal(C.TRIANGLE) + [C.repeat_vertex(C.TRIANGLE, j) for j in range(3)]:
        assert np.array_equal(R.polygon_mask(poly, C.H0, C.W0), C.TRIANGLE_MASK), poly


def test_degenerate_polygons_and_union():
    h, w = C.H0, C.W0
    for poly in ([], [3, 3], [1, 1, 5, 4]):
        assert R.polygon_counts(poly, h, w) == [h * w]
    assert R.object_transitions([], h, w) == [] and R.object_counts([], h, w) == [h * w]
    a, b = C.rect_poly(1, 1, 4, 4), C.rect_poly(3, 2, 7, 5)
    assert np.array_equal(R.object_mask([a, b], h, w), C.rect_mask(1, 1, 4, 4, h, w) | C.rect_mask(3, 2, 7, 5, h, w))
    assert R.object_counts([C.RECT], h, w) == C.RECT_COUNTS
    # (int) truncates toward zero: -0.7 * 5 + .5 = -3.0 -> -3, -0.65 * 5 + .5 = -2.75 -> -2 (floor would give -3)
    u, _ = R.poly_points([-0.65, 0, 2, 0, 2, 2])
    assert u[0] == -2


# ------------------------------------------------------------------------------------------------------------------ odd multiplicity
@pytest.mark.parametrize('seed', [0, 1])
def test_odd_multiplicity_rule_equals_literal_fold(seed):
    """The positions < h * w emitted an odd number of times are the change positions of the literally folded counts, on random polygons
    of every kind of the GPU population (out-of-image and half-pixel-grid ones repeat positions)."""
    rng = np.random.RandomState(seed)
    repeats = 0
    for h, w in C.SIZES:
        for _ in range(120):
            poly = C.random_polygon(rng, h, w)
            pos = R.poly_positions(poly, h, w)
            repeats += len(set(pos)) < len(pos)
            lit = R.fold_counts(pos, h, w)
            assert sum(lit) == h * w and all(c >= 0 for c in lit)
            odd = R.odd_counts(pos, h, w)
            assert np.array_equal(R.counts_to_mask(lit, h, w), R.counts_to_mask(odd, h, w)), (h, w, poly)
            assert R.mask_to_transitions(R.counts_to_mask(lit, h, w)) == R.odd_transitions(pos, h, w)
    assert repeats > 100


# ------------------------------------------------------------------------------------------------------------------ product, host side
def test_module_imports_and_binding_without_gpu():
    from upsnet_amd import _lib
    from upsnet_amd.dataset import polygon
    assert 'upsnet_poly_raster' in _lib.exported_symbols() and 'upsnet_poly_raster_workspace_bytes' in _lib.exported_symbols()
    lib = _lib.lib()
    assert lib.upsnet_poly_raster_workspace_bytes(4, 75) > 75 * 16
    assert lib.upsnet_poly_raster_workspace_bytes(4, polygon.MAX_POINTS + 1) == 0
    assert lib.upsnet_poly_raster_workspace_bytes(-1, 5) == 0 and lib.upsnet_poly_raster_workspace_bytes(9, 5) == 0
    assert callable(polygon.rasterize_polygons) and callable(polygon.polygons_to_rle)


def test_entry_point_validates_before_any_launch():
    from upsnet_amd import _lib
    lib = _lib.lib()
    one = ctypes.c_void_p(1)

    def call(poly_off, obj_off, points=75, h=6, w=8):
        p, o = (ctypes.c_int * len(poly_off))(*poly_off), (ctypes.c_int * len(obj_off))(*obj_off)
        return lib.upsnet_poly_raster(None, one, p, o, one, one, len(poly_off) - 1, len(obj_off) - 1, points, h, w, one, one, one)
    for args, text in ((([0, 4], [0, 1], 75, 65536, 32768), b'bad image size'), (([0, 4], [0, 1], 75, 0, 8), b'bad image size'),
                       (([0, 4, 3], [0, 2]), b'poly_off decreases'), (([0, 4, 8], [0, 2, 1, 2]), b'obj_off decreases'),
                       (([1, 4], [0, 1]), b'start at 0'), (([0, 4], [0, 2]), b'cover'), (([0, 4], [0, 1], 3), b'points'),
                       (([0, 4], [0, 1], (1 << 24) + 1), b'points')):
        assert call(*args) != 0
        assert text in lib.upsnet_last_error(), (args, lib.upsnet_last_error())
    p = (ctypes.c_int * 1)(0)
    assert lib.upsnet_poly_raster(None, one, p, p, one, one, -1, 0, 0, 6, 8, one, one, one) != 0
    assert b'negative counts' in lib.upsnet_last_error()


def test_pack_polygons_and_refusals():
    from upsnet_amd.dataset.polygon import MAX_POINTS, pack_polygons, rasterize_polygons
    verts, poly_off, obj_off, total = pack_polygons([[C.RECT], [], [[], [1, 1]], [[1, 1, 5, 4]]])
    assert verts.shape == (7, 2) and poly_off.tolist() == [0, 4, 4, 5, 7] and obj_off.tolist() == [0, 1, 1, 3, 4]
    assert total == (21 + 16 + 21 + 16) + 1 + 2 * 21     # max(|dX|, |dY|) + 1 per edge, the closing edge included
    # the count is exact: the restatement walks as many points
    rng = np.random.RandomState(3)
    for h, w in C.SIZES:
        objs = [C.random_object(rng, h, w) for _ in range(20)]
        assert pack_polygons(objs)[3] == sum(len(R.poly_points(p)[0]) for o in objs for p in o)
    for bad, text in (([[[1, 2, 3]]], 'odd number'), ([[[1, 2, float('nan'), 4]]], 'non-finite'), ([[[1, 2, float('inf'), 4]]], 'non-finite'),
                      ([[[0, 0, 2.0 ** 30 / 5, 0]]], 'out of range'), ([[[0, 0, -2.0 ** 30 / 5, 0]]], 'out of range'),
                      ([[[0, 0, MAX_POINTS / 5.0, 0, 0, 3]]], 'edge-walk points'), ([[1, 2, 3, 4]], 'list of polygons')):
        with pytest.raises(ValueError, match=text):
            pack_polygons(bad)
    # refused before the device is looked at
    for args in (([[[1, 2, 3]]], 6, 8), ([[C.RECT]], 0, 8), ([[C.RECT]], 65536, 32768)):
        with pytest.raises(ValueError):
            rasterize_polygons(*args)


def test_bare_polygon_list_is_still_refused_by_the_evaluator():
    from upsnet_amd.dataset.coco_eval import DetectionEvaluator, rle_counts
    with pytest.raises(ValueError, match='polygon') as e:
        rle_counts([C.RECT])
    assert 'dataset.polygon' in str(e.value)
    ev = DetectionEvaluator([1], 'segm', device='cuda')
    gt = [{'id': 1, 'category_id': 1, 'iscrowd': 0, 'area': 12.0, 'bbox': [2, 1, 4, 3], 'segmentation': [C.RECT]}]
    with pytest.raises(ValueError, match='dataset.polygon'):
        ev.add_rle(1, gt, [[], np.zeros((0, 5))], [[], []], image_size=(6, 8))
    assert ev.num_images == 0
