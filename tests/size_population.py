"""The image sizes an evaluation set puts through one model object (plain helper module, no fixtures).

A COCO evaluation set is not one size: `upsnet_amd.dataset.blob.blob_geometry` scales every image to short side 800 / long side at most 1333 and
pads the blob to a multiple of 32, so the padded size -- and with it the workgroup counts every threshold of models/hipconv.py is written in --
moves with the aspect ratio, in both orientations. The population is produced by calling that function, never by restating its rule.
"""
TARGET, MAX_SIZE, STRIDE = 800, 1333, 32


def coco_source_sizes():
    """(height, width) of the source images: long side 640 with short sides 240..640 in steps of 8 (COCO's images are at most 640 on a side),
    landscape and portrait, plus the most common 500x375 / 375x500 and the square."""
    src = set()
    for short in range(240, 641, 8):
        src.add((short, 640))
        src.add((640, short))
    src.update([(375, 500), (500, 375), (640, 640)])
    return sorted(src)


def coco_padded_sizes():
    """Sorted list of the distinct ((resized h, w), (padded h, w)) that blob_geometry gives the source sizes."""
    from upsnet_amd.dataset.blob import blob_geometry
    out = set()
    for h, w in coco_source_sizes():
        _, resized, padded = blob_geometry(h, w, TARGET, MAX_SIZE, stride=STRIDE)
        out.add((tuple(int(v) for v in resized), tuple(int(v) for v in padded)))
    return sorted(out)


def one_per_padded(pairs):
    """One (resized, padded) per distinct padded size, sorted by padded size: the largest resized image that pads to it (the convolution
    launches depend on the padded size only; the largest image leaves the least zero padding, and makes 800x1333 stand for 800x1344)."""
    best = {}
    for resized, padded in pairs:
        if padded not in best or resized > best[padded]:
            best[padded] = resized
    return [(best[padded], padded) for padded in sorted(best)]


def cityscapes_sizes():
    """((resized h, w), (padded h, w)) of the Cityscapes list: the full frame, the half-size frame and the portrait full frame (the
    mixed-stream configuration feeds arbitrary sizes to one model object)."""
    return [((h, w), (h, w)) for h, w in [(512, 1024), (1024, 2048), (2048, 1024)]]


def is_portrait(size):
    return size[0] > size[1]
