"""CPU: the population of image sizes the size-sweep GPU tests walk (tests/size_population.py) is what an evaluation set yields --
deterministic, wide, half portrait, and produced by the project's own blob_geometry."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import size_population as sp  # noqa: E402


def test_coco_population_is_deterministic_wide_and_half_portrait():
    pairs = sp.coco_padded_sizes()
    assert pairs == sp.coco_padded_sizes() and pairs == sorted(set(pairs))
    padded = sorted({p for _, p in pairs})
    assert len(padded) >= 40, len(padded)
    portrait = [p for p in padded if sp.is_portrait(p)]
    assert 3 * len(portrait) >= len(padded), (len(portrait), len(padded))
    assert ((800, 1333), (800, 1344)) in pairs
    for (hr, wr), (hp, wp) in pairs:
        assert hp % 32 == 0 and wp % 32 == 0 and max(hp, wp) <= 1344, (hp, wp)
        assert 0 <= hp - hr < 32 and 0 <= wp - wr < 32, ((hr, wr), (hp, wp))
        assert min(hr, wr) == 800 or max(hr, wr) == 1333, (hr, wr)
    print("%d (resized, padded) pairs, %d distinct padded sizes, %d portrait, largest side %d" %
          (len(pairs), len(padded), len(portrait), max(max(p) for p in padded)))


def test_one_image_per_padded_size_and_it_pads_as_the_synthetic_image_does():
    from upsnet_amd.synthetic import make_image
    pairs = sp.coco_padded_sizes()
    reps = sp.one_per_padded(pairs)
    assert [p for _, p in reps] == sorted({p for _, p in pairs}) and all(r in pairs for r in reps)
    assert ((800, 1333), (800, 1344)) in reps
    for resized, padded in (reps[0], reps[-1]):      # make_image pads a resized image to the same blob size as blob_geometry
        assert tuple(make_image(resized[0], resized[1], seed=0)['data'].shape[2:]) == padded


def test_cityscapes_list_has_the_portrait_frame():
    sizes = sp.cityscapes_sizes()
    assert ((1024, 2048), (1024, 2048)) in sizes and ((512, 1024), (512, 1024)) in sizes and ((2048, 1024), (2048, 1024)) in sizes
    assert all(hp % 32 == 0 and wp % 32 == 0 for _, (hp, wp) in sizes)
