"""Pins the oracle (and the HIP kernels) against the REFERENCE's own GPU kernels.

oracle/_ref/libupsnet_ref.so is built by oracle/Makefile straight from the reference tree (hipify-perl +
hipcc, -ffp-contract=off). Its outputs on the inputs below are replayed from tests/golden/ref_kernels.npz
(oracle/refvec.py), recorded by running this file with REFVEC_RECORD=1 on the GPU with the library built.
If a record is absent the tests fail (not skip): the pin is part of the parity claim.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

import oracle
from oracle import ops as oops
from conftest import ROOT, gen_dets, gen_rois
from oracle.refvec import RefLib, RefVectors

pytestmark = pytest.mark.gpu
P = ctypes.c_void_p
VEC = RefVectors(os.path.join(ROOT, "tests", "golden", "ref_kernels.npz"))


@pytest.fixture(scope="module")
def ref():
    yield RefLib(VEC, os.path.join(ROOT, "oracle", "_ref", "libupsnet_ref.so"))
    VEC.save()


@pytest.fixture(scope="module")
def ref_fma():
    yield RefLib(VEC, os.path.join(ROOT, "oracle", "_ref", "libupsnet_ref_fma.so"))
    VEC.save()


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def p(t):
    return P(t.data_ptr())


def _ref_roi(ref, feat, rois, ph, scale, want):
    def run(lib):
        f, r = cu(feat), cu(rois)
        out = torch.zeros((rois.shape[0], feat.shape[1], ph, ph), device='cuda')
        lib.ref_roi_align_forward(None, p(f), ctypes.c_float(scale), rois.shape[0], feat.shape[2], feat.shape[3], feat.shape[1],
                                  ph, ph, 2, p(r), p(out))
        torch.cuda.synchronize()
        return out.cpu().numpy()
    return ref("roi_align_forward", (feat, rois, ph, scale), want, run)


def test_reference_roi_align(ref, ref_fma):
    from upsnet_amd import ops as U
    rng = np.random.default_rng(0)
    feat = rng.normal(size=(1, 16, 40, 64)).astype(np.float32)
    rois = gen_rois(rng, 200, 160, 256, 4, 150)
    rois = np.vstack([rois, [[0, 0, 0, 0, 0]], [[0, -30, -30, -9, -9]], [[0, 300, 3, 340, 9]]]).astype(np.float32)
    for ph in (7, 14):
        want = oracle.roi_align_forward(feat, rois, ph, ph, 0.25)
        r = _ref_roi(ref, feat, rois, ph, 0.25, want)
        assert np.array_equal(r, want)                                                           # oracle == reference kernel
        assert np.array_equal(r, U.roi_align_nchw(cu(feat), cu(rois), ph, ph, 0.25).cpu().numpy())  # ours == reference kernel
        np.testing.assert_allclose(_ref_roi(ref_fma, feat, rois, ph, 0.25, want), r, rtol=0, atol=1e-4)  # FMA build (nvcc default): within the 1e-4 logit tolerance


def _ref_im2col(ref, im, off, k, pad, stride, dil, dg, mask, want):
    C, H, W = im.shape
    Ho = (H + 2 * pad - (dil * (k - 1) + 1)) // stride + 1
    Wo = (W + 2 * pad - (dil * (k - 1) + 1)) // stride + 1

    def run(lib):
        col = torch.zeros((C * k * k, Ho, Wo), device='cuda')
        i, o = cu(im), cu(off)
        if mask is None:
            lib.ref_deform_im2col(None, p(i), p(o), C, H, W, k, k, pad, pad, stride, stride, dil, dil, 1, dg, p(col))
        else:
            m = cu(mask)
            lib.ref_mod_deform_im2col(None, p(i), p(o), p(m), 1, C, H, W, Ho, Wo, k, k, pad, pad, stride, stride, dil, dil, dg, p(col))
        torch.cuda.synchronize()
        return col.cpu().numpy()
    return ref("deform_im2col" if mask is None else "mod_deform_im2col", (im, off, k, pad, stride, dil, dg) + (() if mask is None else (mask,)),
               want, run)


@pytest.mark.parametrize("C,H,W,pad,stride,dil,dg", [(16, 20, 33, 1, 1, 1, 1), (8, 12, 12, 2, 1, 2, 2), (4, 15, 15, 1, 2, 1, 1)])
def test_reference_deform_im2col(ref, ref_fma, C, H, W, pad, stride, dil, dg):
    from upsnet_amd import ops as U
    rng = np.random.default_rng(1)
    k = 3
    im = rng.normal(size=(C, H, W)).astype(np.float32)
    Ho, Wo = U.out_hw(H, W, (k, k), (pad, pad), (stride, stride), (dil, dil))
    off = (rng.normal(size=(dg * 18, Ho, Wo)) * 2.5).astype(np.float32)
    mask = rng.uniform(0, 2, size=(dg * 9, Ho, Wo)).astype(np.float32)
    for mk in (None, mask):
        want = oracle.deform_im2col(im, off, (k, k), (pad, pad), (stride, stride), (dil, dil), dg, mask=mk)
        r = _ref_im2col(ref, im, off, k, pad, stride, dil, dg, mk, want)
        assert np.array_equal(r, want)
        col = torch.zeros(r.shape, device='cuda')
        if mk is None:
            U.deform_im2col(cu(im), cu(off), (1, C, H, W), r.shape, (k, k), (pad, pad), (stride, stride), (dil, dil), 1, dg, col)
        else:
            U.mod_deform_im2col(cu(im), cu(off), cu(mk), (1, C, H, W), r.shape, (k, k), (pad, pad), (stride, stride), (dil, dil), dg, col)
        assert np.array_equal(col.cpu().numpy(), r)
        np.testing.assert_allclose(_ref_im2col(ref_fma, im, off, k, pad, stride, dil, dg, mk, want), r, rtol=0, atol=1e-4)


@pytest.mark.parametrize("n", [1, 64, 65, 500, 1000, 2000])
def test_reference_nms(ref, n):
    from upsnet_amd import ops as U
    rng = np.random.default_rng(n)
    d = gen_dets(rng, n)
    order = oops.argsort_desc(d[:, 4])
    sd = np.ascontiguousarray(d[order])
    want = oracle.nms_sorted(sd, 0.6)

    def run(lib):
        keep = np.zeros((n,), np.int32)
        num = ctypes.c_int(0)
        lib.ref_nms(keep.ctypes.data_as(P), ctypes.byref(num), sd.ctypes.data_as(P), n, 5, ctypes.c_float(0.6), 0)
        return keep[:num.value]
    rk = ref("nms", (sd, 0.6), want, run)
    assert np.array_equal(rk, want)                                       # oracle == the reference's _nms
    assert np.array_equal(rk, U.nms_host(sd, 0.6))                        # our `_nms` drop-in == reference
    assert np.array_equal(order[rk], U.gpu_nms(cu(d), 0.6).cpu().numpy())  # device pipeline == gpu_nms(order[keep])


@pytest.mark.parametrize("n,ph", [(1000, 7), (100, 14), (300, 7)])
def test_fpn_roi_align_at_the_benchmark_shapes(ref, n, ph):
    """VERDICT r03 next #1c: ROIAlign at the shapes the benchmark runs -- 1000 x 256 x 7 x 7 (box head) and 100 x 256 x 14 x 14 (mask
    head) on the four 256-channel maps of a 1024x2048 image, log-uniform random ROIs (SURVEY 8d's microbenchmark input) -- all three
    kernel variants == the oracle == the reference's own kernel (roi_align_kernel.cu:43-95,163-235, per level on the NCHW map)."""
    from upsnet_amd import ops as U
    from upsnet_amd._lib import lib
    rng = np.random.default_rng(11)
    H, W, C = 1024, 2048, 256
    feats = [rng.standard_normal(size=(1, C, H // s, W // s), dtype=np.float32) for s in (4, 8, 16, 32)]
    rois = gen_rois(rng, n, H, W, 16, 512)
    rois[0] = [0, -40, -30, 20, 25]                 # partly outside
    rois[1] = [0, W - 10, H - 12, W + 60, H + 40]
    rois[2] = [0, 17.3, 21.9, 17.3, 21.9]           # degenerate
    dev = [cu(f).contiguous(memory_format=torch.channels_last) for f in feats]
    want = oops.fpn_roi_align(feats, rois, ph, ph)  # the oracle (C restatement), whole pyramid
    lv = oops.fpn_level(rois)
    assert len(set(lv.tolist())) == 4               # every pyramid level is hit
    for variant in (0, 1, 2, 3, 4):
        lib().upsnet_roi_tuning(variant)
        try:
            got = U.fpn_roi_align(dev, cu(rois), ph, ph, [1 / 4., 1 / 8., 1 / 16., 1 / 32.]).cpu().numpy()
        finally:
            lib().upsnet_roi_tuning(-1)
        assert got.shape == (n, C, ph, ph) and np.array_equal(got, want), variant
    for l, s in enumerate((4, 8, 16, 32)):          # the reference kernel itself, level by level
        idx = np.where(lv == l)[0]
        r = _ref_roi(ref, feats[l], rois[idx], ph, 1.0 / s, want[idx])
        assert np.array_equal(r, want[idx]), l
