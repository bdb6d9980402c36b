"""CPU: the oracle vs golden vectors produced by the reference's own Python modules
(tests/golden/make_golden.py, run where /root/reference exists; fixtures committed)."""
import os

import numpy as np
import pytest

import oracle
from oracle import ops as oops

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load(name):
    return np.load(os.path.join(G, name + ".npz"))


def test_anchors():
    g = load("anchors")
    for s in (4, 8, 16, 32, 64):
        assert np.array_equal(oops.generate_anchors(s, (8 * s,), (0.5, 1, 2)), g["s%d" % s])


def test_bbox_transform_and_clip():
    g = load("bbox_transform")
    dec = oops.bbox_transform(g["boxes"], g["deltas"], (10., 10., 5., 5.))
    # numpy>=2 promotes np.minimum(dw, np.float64) to float64 inside the reference (NEP 50); the 2018-era
    # numpy it was written for stayed in fp32 -> ulp-level differences only
    np.testing.assert_allclose(dec, g["decoded"], rtol=2e-6, atol=2e-4)
    assert np.array_equal(oops.clip_boxes(g["decoded"], (600, 900)), g["clipped"])


def test_py_nms():
    g = load("py_nms")
    assert np.array_equal(oops.gpu_nms(g["dets"], 0.5), g["keep05"])
    assert np.array_equal(oops.gpu_nms(g["dets"], 0.7), g["keep07"])
    assert np.array_equal(oops.py_nms(g["dets"], 0.5), g["keep05"])


def test_pyramid_proposal():
    g = load("pyramid_proposal")
    rois, scores = oops.pyramid_proposal([g["cls%d" % i] for i in range(5)], [g["box%d" % i] for i in range(5)], g["im_info"],
                                         pre_nms_top_n=200, post_nms_top_n=100, nms_thresh=0.7)
    assert np.array_equal(scores, g["scores"])       # selection + ranking identical
    np.testing.assert_allclose(rois, g["rois"], rtol=0, atol=2e-4)  # decode ulp (NEP 50, see above)


@pytest.mark.parametrize("tag", ["full", "pad"])
def test_pyramid_proposal_joint(tag):
    """individual_proposals=False -- the reference constructors' DEFAULT -- from the reference's own module (fixture of round 5). The
    padding of the "pad" case comes from numpy's global generator: same seed, same stream, same rows."""
    g = load("pyramid_proposal_joint_" + tag)
    pre, post, min_size = [int(v) for v in g["cfg"]]
    np.random.seed(int(g["seed"]))
    rois, scores = oops.pyramid_proposal([g["cls%d" % i] for i in range(5)], [g["box%d" % i] for i in range(5)], g["im_info"][0],
                                         pre_nms_top_n=pre, post_nms_top_n=post, nms_thresh=float(g["thr"]), min_size=min_size,
                                         individual_proposals=False)
    assert rois.shape == (post, 5) and (int(g["n_unique"]) < post) == (tag == "pad")
    assert np.array_equal(scores, g["scores"].reshape(-1))
    np.testing.assert_allclose(rois, g["rois"].reshape(-1, 5), rtol=0, atol=2e-4)
    # the un-padded list (what the device entry returns) = the distinct rows, in NMS order = score descending
    r2, s2 = oops.pyramid_proposal([g["cls%d" % i] for i in range(5)], [g["box%d" % i] for i in range(5)], g["im_info"][0],
                                   pre_nms_top_n=pre, post_nms_top_n=post, nms_thresh=float(g["thr"]), min_size=min_size,
                                   individual_proposals=False, pad=False)
    assert len(s2) == int(g["n_unique"]) and np.array_equal(s2, np.unique(scores)[::-1])


@pytest.mark.parametrize("tag", ["det", "pan"])
def test_mask_roi_noclip(tag):
    """MaskROI(clip_boxes=False) (modules/mask_roi.py:53-54 skipped), fixture of round 5."""
    g = load("mask_roi_noclip_" + tag)
    s, b, c = oops.mask_roi(g["rois"], g["delta"], g["prob"], g["im_info"], 9, 0.5, float(g["thr"]), 100, bool(g["agn"]), clip=False)
    assert np.array_equal(c, g["cls"]) and np.array_equal(s, g["scores"])
    np.testing.assert_allclose(b, g["boxes"], rtol=0, atol=2e-4)
    assert (b[:, 1:] < 0).any()


@pytest.mark.parametrize("tag", ["all", "small"])
def test_fpn_roi_align(tag):
    g = load("fpn_roi_align_" + tag)
    out = oops.fpn_roi_align([g["feat%d" % i] for i in range(4)], g["rois"], 7, 7)
    assert np.array_equal(out, g["out"])


@pytest.mark.parametrize("tag", ["det", "pan", "empty"])
def test_mask_roi(tag):
    g = load("mask_roi_" + tag)
    s, b, c = oops.mask_roi(g["rois"], g["delta"], g["prob"], g["im_info"], 9, 0.5, float(g["thr"]), 100, bool(g["agn"]))
    assert np.array_equal(c, g["cls"]) and np.array_equal(s, g["scores"])
    np.testing.assert_allclose(b, g["boxes"], rtol=0, atol=2e-4)


def test_panoptic_head():
    g = load("panoptic_head")
    keep, energy = oops.mask_removal(g["rois"], g["prob"], g["logit"], g["cls"], (72, 120))
    assert 0 < len(keep) < len(g["cls"])
    assert np.array_equal(keep, g["keep"]) and np.array_equal(energy, g["energy"])
    rois5 = np.hstack([np.zeros((len(g["rois"]), 1), np.float32), g["rois"]])[keep]
    seg, inst = oops.seg_term(g["cls"][keep], g["fcn"], rois5 * np.float32(4.0), 19, 9)
    assert np.array_equal(inst, g["seg_inst"])
    pan, _ = oracle.panoptic_fuse(g["fcn"][0], 11, inst[0], energy[0], True)
    assert np.array_equal(pan, g["pan_void"][0])
    pan2, _ = oracle.panoptic_fuse(g["fcn"][0], 11, inst[0], energy[0], False)
    # argmax(softmax(x)) through torch's own softmax: allow the (rare) rounding-tie pixels, report them
    assert (pan2 != g["pan_softmax"][0]).mean() < 1e-3
    # ... and every one of them an exact tie of torch's fp32 probabilities
    from oracle.forward import softmax_fuse_non_ties
    assert softmax_fuse_non_ties(g["fcn"], 11, inst, energy, pan2, g["pan_softmax"]) == []


def test_softmax_fuse_tie_check_rejects_a_non_tie():
    """The tie check of test_panoptic_head fails on one pixel moved to a label whose probability is not bit-identical."""
    import torch
    from oracle.forward import softmax_fuse_non_ties
    g = load("panoptic_head")
    p = torch.softmax(torch.cat([torch.from_numpy(g["fcn"][:, :11]), torch.from_numpy(g["seg_inst"] + g["energy"])], dim=1), dim=1)[0]
    top2 = p.topk(2, dim=0)
    ref = g["pan_softmax"]
    assert np.array_equal(top2.indices[0].numpy(), ref[0])
    args = (g["fcn"], 11, g["seg_inst"], g["energy"])
    assert softmax_fuse_non_ties(*args, ref.copy(), ref) == []
    y, x = 37, 59
    assert top2.values[0, y, x] != top2.values[1, y, x]
    pan = ref.copy()
    pan[0, y, x] = int(top2.indices[1, y, x])
    assert softmax_fuse_non_ties(*args, pan, ref) == [(y, x, int(pan[0, y, x]), int(ref[0, y, x]), float(top2.values[1, y, x]),
                                                       float(top2.values[0, y, x]))]
    # still under the 1e-3 share the older assertion allows: that one alone would not have seen it
    assert (pan != ref).mean() < 1e-3


def test_input_blob_golden_from_reference_python():
    """oracle.prep_image == BaseDataset.prep_im_for_blob + im_list_to_blob of the reference (im_scale 1: mean subtraction in
    double, HWC->CHW, zero pad to 32), fixtures from tests/golden/make_golden_blob.py."""
    import oracle
    g = np.load(os.path.join(G, "input_blob.npz"))
    means = np.array((102.9801, 115.9465, 122.7717,))
    for tag in ("even", "ragged"):
        target, max_size = [int(v) for v in g[tag + "_cfg"]]
        blob, scale = oracle.prep_image(g[tag + "_im"], means, target, max_size)
        assert scale == 1.0
        np.testing.assert_array_equal(blob, g[tag + "_blob"])


def test_unified_pan_result_golden_from_reference_python():
    """oracle.ops.get_unified_pan_result == BaseDataset.get_unified_pan_result of the reference (majority vote, stuff re-labelling,
    enumerate-index instance ids, void pass-through, stuff-area filter)."""
    g = np.load(os.path.join(G, "unified_pan.npz"))
    for tag in ("a", "b", "c"):
        out = oops.get_unified_pan_result(g[tag + "_seg"].astype(np.int64), g[tag + "_pan"].astype(np.int64), g[tag + "_cls"], 19, 9,
                                          int(g[tag + "_limit"]))
        np.testing.assert_array_equal(out, g[tag + "_out"])
    # the fixtures exercise every branch
    o = g["a_out"]
    assert (o[:, :, 0] == 255).any() and (o[:, :, 1] > 0).any() and len(np.unique(o[:, :, 1])) > 3
