"""Index tables of the two nearest-neighbour resizes that bring label maps to another resolution; the gather itself runs on the
device (csrc/restore.hip, ops.restore_label_maps).

cv2 INTER_NEAREST (the reference's restore to the original image, upsnet/upsnet_end2end_test.py:258-272), restated from OpenCV's
resize / resizeNN: the map is first cropped to (Hc, Wc) = (int(im_info[0]), int(im_info[1])); fx = float32(1) / float32(im_scale)
(the reference divides a float32 im_info row), widened to double; output size (cvRound(Wc * fx), cvRound(Hc * fx)) with cvRound
rounding half to even; source column min(floor(x * (1 / fx)), Wc - 1), rows alike.

PIL Image.NEAREST resize (evaluate_ssegs, cityscapes.py:445-492, coco.py:225-273), restated from Pillow's ImagingScaleAffine:
the source coordinate of output column x is (x + 0.5) * Ws / Wd, accumulated in double as Pillow does (xo = 0.5 * a, then xo += a
per column), truncated; rows alike.
"""
import numpy as np

from .. import ops


def cv_round(v):
    """cvRound of doubles: nearest integer, halves to even."""
    return np.rint(np.asarray(v, dtype=np.float64)).astype(np.int64)


def cv2_nearest_tables(im_info):
    """im_info = (Hr, Wr, im_scale) of one image (float32 values, as the reference's) -> (y_ofs, x_ofs) int32 tables of
    cv2.resize(map[:Hr, :Wr], None, fx=1/im_scale, fy=1/im_scale, interpolation=INTER_NEAREST). len(y_ofs) x len(x_ofs) is the
    output size (the original image's, up to the resize rounding)."""
    im_info = np.asarray(im_info, dtype=np.float32).reshape(-1)
    hc, wc = int(im_info[0]), int(im_info[1])
    fx = float(np.float32(1) / np.float32(im_info[2]))

    def table(n_src):
        n_dst = int(cv_round(n_src * fx))
        ifx = 1.0 / fx
        src = np.floor(np.arange(n_dst, dtype=np.float64) * ifx).astype(np.int64)
        return np.minimum(src, n_src - 1).astype(np.int32)

    return table(hc), table(wc)


def pil_nearest_table(n_src, n_dst):
    """Source index of each of n_dst outputs of PIL's NEAREST resize along one axis (ImagingScaleAffine: running double sum)."""
    a = float(n_src) / float(n_dst)
    steps = np.full((n_dst,), a, dtype=np.float64)
    steps[0] = a * 0.5
    xo = np.add.accumulate(steps)          # sequential, like Pillow's `xo += a[0]`
    return np.minimum(np.floor(xo).astype(np.int64), n_src - 1).astype(np.int32)


def pil_nearest_tables(src_hw, dst_hw):
    """(y_ofs, x_ofs) of Image.fromarray(label [src_hw]).resize((dst_w, dst_h), Image.NEAREST)."""
    return pil_nearest_table(int(src_hw[0]), int(dst_hw[0])), pil_nearest_table(int(src_hw[1]), int(dst_hw[1]))


def restore_to_image(sseg, pano, im_info):
    """The reference's per-image restore of the network's int64 semantic / panoptic maps ([1,H,W] device tensors at network
    resolution; pano may be None) -> uint8 device maps at the original image resolution, one launch for both."""
    y_ofs, x_ofs = cv2_nearest_tables(im_info)
    return ops.restore_label_maps(sseg, pano, y_ofs, x_ofs)


def restore_plane_to_image(plane, im_info):
    """restore_to_image's gather for a uint8 plane at network resolution (the panoptic confidence): the same tables, so a
    pixel of the restored plane belongs to the pixel of the restored label maps."""
    y_ofs, x_ofs = cv2_nearest_tables(im_info)
    return ops.restore_plane_u8(plane, y_ofs, x_ofs)
